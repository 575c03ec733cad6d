// lightglue_geometry.hip — geometric verification (include/lightglue_glue.h, "geometric verification"): a
// fundamental matrix per image pair by RANSAC over the matcher's matches, what the reference's demo does on the
// host with cv::findFundamentalMat(points0, points1, cv::FM_RANSAC, 3, 0.99, inliers) after PostProcess
// (demo/demo_mono.cpp:326-366), and a homography by the same scheme (cv::findHomography(points0, points1,
// cv::RANSAC, 3) without its final Levenberg-Marquardt polish). The contract is restated in float64 in
// lightglue_amd/geometry_contract.py. The kernels are templates on the model (FundamentalModel, HomographyModel below):
// the sample size, the minimal solve, the error, the refit's rows and its last step are the model's, the rest
// is shared. The description that follows is in the fundamental matrix's numbers (the homography's: 4 indices,
// the 4-point system, one candidate, no rank step).
//
// Two launches. ransac_hypothesis_kernel: grid (hypothesis blocks, pairs), 64 hypotheses a workgroup; the
// workgroup gathers the pair's correspondences into LDS once (2048 x 16 B) and computes the Hartley
// normalisation; then a lane is a hypothesis: it hashes its 7 indices, solves the 7-point system in registers in
// fp64 (selects, no run-time register index) and counts the inliers of its up-to-3 candidates in one pass over the
// LDS copy. Four adjacent lanes share a hypothesis: they solve it alike (the wave executes the statements once
// either way) and each takes every fourth correspondence of the pass, the four integer counts added across the
// lanes. (F, count, root) of the best candidate goes to the workspace.
// ransac_finalize_kernel: one workgroup per pair reduces the hypotheses to the winner in index order, marks its
// inliers, runs the refits in fp64 (normal matrix, a round-robin Jacobi on the 9 x 9, rank 2, de-normalise) and
// writes every output. No atomics, no allocation, no host synchronisation; no workgroup reads what another
// wrote within a launch. The arithmetic is in lightglue_geometry_math.h; what the kernels share with the five-point
// RANSAC of lightglue_essential.hip (launch shapes, a pair's staging, the ordered sums, the Hartley
// normalisation, the normal matrix's eigenvectors, the argument checks) is in lightglue_geometry_device.h.
#include "lightglue_geometry_device.h"

namespace {

using namespace lg_geom;

constexpr int kHypRecord = 12;   // floats per hypothesis in the workspace: F[9], count, root, pad

// ---- the models ---------------------------------------------------------------------------------------------------
// kSample: indices a hypothesis; kCands: candidates a hypothesis at most; kMin: correspondences a model, a winner
// and a refit need. solve: normalised sample -> candidates in pixels; inlier: the error test; accumulate: one
// inlier's share of the refit's normal matrix; finish: the eigenvector to the matrix in pixels at unit norm.
struct FundamentalModel {
    static constexpr int kSample = 7, kCands = 3, kMin = kMinInliers;
    static __device__ __forceinline__ int solve(const double x0[7], const double y0[7], const double x1[7], const double y1[7],
                                                const NormT<double>& t, float cand[3][9]) {
        return solve7(x0, y0, x1, y1, t, cand);
    }
    static __device__ __forceinline__ bool inlier(const float f[9], float x0, float y0, float x1, float y1, float thr2) {
        return is_inlier(f, x0, y0, x1, y1, thr2);
    }
    static __device__ __forceinline__ void accumulate(double acc[45], double x0, double y0, double x1, double y1) {
        normal_accumulate_f(acc, x0, y0, x1, y1);
    }
    static __device__ __forceinline__ bool finish(double fn[9], const double c[4], const double s[2], double out[9]) {
        rank2(fn);
        return denormalise64(fn, c[0], c[1], s[0], c[2], c[3], s[1], out);
    }
};

struct HomographyModel {
    static constexpr int kSample = 4, kCands = 1, kMin = kMinInliersH;
    static __device__ __forceinline__ int solve(const double x0[4], const double y0[4], const double x1[4], const double y1[4],
                                                const NormT<double>& t, float cand[1][9]) {
        return solve4(x0, y0, x1, y1, t, cand[0]);
    }
    static __device__ __forceinline__ bool inlier(const float h[9], float x0, float y0, float x1, float y1, float thr2) {
        return is_inlier_h(h, x0, y0, x1, y1, thr2);
    }
    static __device__ __forceinline__ void accumulate(double acc[45], double x0, double y0, double x1, double y1) {
        normal_accumulate_h(acc, x0, y0, x1, y1);
    }
    static __device__ __forceinline__ bool finish(double hn[9], const double c[4], const double s[2], double out[9]) {
        return denormalise_h(hn, c[0], c[1], s[0], c[2], c[3], s[1], out);
    }
};

// GIVEN: the samples are an input and every candidate an output (lg_ransac_solve7, lg_ransac_solve4); else the samples are
// hashed and the best candidate's record goes to the workspace.
template <class M, bool GIVEN>
__global__ __launch_bounds__(kHypThreads) void ransac_hypothesis_kernel(PairArgs a, int hypotheses, uint32_t seed, float thr2,
                                                                         const int32_t* __restrict__ samples,
                                                                         float* __restrict__ hyp, float* __restrict__ cand_out,
                                                                         int32_t* __restrict__ nroots_out) {
    __shared__ float4 pts[kMaxPoints];
    __shared__ double buf[kHypThreads];
    const int p = blockIdx.y, tid = threadIdx.x, sub = tid % kHypSplit;
    const int h = blockIdx.x * kHypLanes + tid / kHypSplit;
    const bool live = h < hypotheses;
    const int count = pair_count(a, p);
    constexpr int NS = M::kSample, NC = M::kCands;
    float cand[NC][9];
    int nc = 0;
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) cand[i][k] = 0.f;
    if (count >= M::kMin) {  // (the same for the whole workgroup)
        stage_pair(a, p, count, pts, tid, kHypThreads);
        double c[4], s[2];
        hartley<kHypThreads>(pts, nullptr, count, (double)count, buf, tid, c, s, PixelCoord{});
        const NormT<double> t{c[0], c[1], s[0], c[2], c[3], s[1]};
        if (live) {  // (the lanes of a hypothesis solve it alike: the same statements on the same values)
            int idx[NS];
            if constexpr (GIVEN) {
#pragma unroll
                for (int j = 0; j < NS; ++j) idx[j] = min(max(samples[(size_t)h * NS + j], 0), count - 1);
            } else {
                sample<NS>(seed, h, count, idx);
            }
            double x0[NS], y0[NS], x1[NS], y1[NS];
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const float4 q = pts[idx[j]];
                x0[j] = ((double)q.x - t.cx0) * t.s0, y0[j] = ((double)q.y - t.cy0) * t.s0;
                x1[j] = ((double)q.z - t.cx1) * t.s1, y1[j] = ((double)q.w - t.cy1) * t.s1;
            }
            nc = M::solve(x0, y0, x1, y1, t, cand);
        }
    }
    if constexpr (GIVEN) {
        if (!live || sub != 0) return;
        float* out = cand_out + ((size_t)p * hypotheses + h) * (9 * NC);
#pragma unroll
        for (int i = 0; i < NC; ++i)
#pragma unroll
            for (int k = 0; k < 9; ++k) out[9 * i + k] = cand[i][k];
        nroots_out[(size_t)p * hypotheses + h] = nc;
    } else {
        // (n1, n2 and candidates 1, 2 exist for the model of three candidates only; the other's are constants)
        int n0 = 0, n1 = 0, n2 = 0;
        const float* c1 = cand[NC > 1 ? 1 : 0];
        const float* c2 = cand[NC > 2 ? 2 : 0];
        if (nc > 0) {
#pragma unroll 2
            for (int k = sub; k < count; k += kHypSplit) {
                const float4 q = pts[k];
                n0 += M::inlier(cand[0], q.x, q.y, q.z, q.w, thr2) ? 1 : 0;
                if constexpr (NC > 1) n1 += M::inlier(c1, q.x, q.y, q.z, q.w, thr2) ? 1 : 0;
                if constexpr (NC > 2) n2 += M::inlier(c2, q.x, q.y, q.z, q.w, thr2) ? 1 : 0;
            }
        }
#pragma unroll
        for (int d = 1; d < kHypSplit; d <<= 1) {  // (integers: the order of the sum does not matter)
            n0 += __shfl_xor(n0, d);
            if constexpr (NC > 1) n1 += __shfl_xor(n1, d);
            if constexpr (NC > 2) n2 += __shfl_xor(n2, d);
        }
        if (!live || sub != 0) return;
        // the highest count, the lowest root among equals (a zero candidate counts nothing)
        const int root = n2 > max(n0, n1) ? 2 : (n1 > n0 ? 1 : 0);
        const int best = max(n0, max(n1, n2));
        float* rec = hyp + ((size_t)p * hypotheses + h) * kHypRecord;
#pragma unroll
        for (int k = 0; k < 9; ++k) rec[k] = root == 2 ? c2[k] : (root == 1 ? c1[k] : cand[0][k]);
        rec[9] = __int_as_float(best), rec[10] = __int_as_float(root), rec[11] = 0.f;
    }
}

// lg_ransac_score, lg_ransac_score_homography: a lane is one given candidate.
template <class M>
__global__ __launch_bounds__(kHypLanes) void ransac_score_kernel(PairArgs a, const float* __restrict__ cands, int ncand,
                                                                  float thr2, int32_t* __restrict__ out) {
    __shared__ float4 pts[kMaxPoints];
    const int p = blockIdx.y, lane = threadIdx.x, c = blockIdx.x * kHypLanes + lane;
    const int count = pair_count(a, p);
    stage_pair(a, p, count, pts, lane, kHypLanes);
    __syncthreads();
    if (c >= ncand) return;
    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = cands[((size_t)p * ncand + c) * 9 + k];
    int n = 0;
    for (int k = 0; k < count; ++k) {
        const float4 q = pts[k];
        n += M::inlier(f, q.x, q.y, q.z, q.w, thr2) ? 1 : 0;
    }
    out[(size_t)p * ncand + c] = n;
}

// (f, f_out, fnew and "F" in the comments below: the model's 3 x 3 matrix, F or H.)
template <class M>
__global__ __launch_bounds__(kFinThreads) void ransac_finalize_kernel(PairArgs a, int hypotheses, int refits, float thr2,
                                                                       const float* __restrict__ hyp, float* __restrict__ f_out,
                                                                       uint8_t* __restrict__ inl_out,
                                                                       int32_t* __restrict__ num_out,
                                                                       int32_t* __restrict__ valid_out,
                                                                       int32_t* __restrict__ best_out) {
    __shared__ float4 pts[kMaxPoints];
    __shared__ uint8_t mask[kMaxPoints];
    __shared__ double buf[kFinThreads];
    __shared__ int best_c[kFinThreads], best_h[kFinThreads];
    __shared__ double part[kFinThreads / 64][45];
    __shared__ double am[81], vm[81];  // the normal matrix and the eigenvectors (columns), row-major 9 x 9
    __shared__ double rot[4][2];
    __shared__ double fnew[9];
    __shared__ int fnew_ok;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int count = pair_count(a, p);

    // the winner: the highest count, the lowest hypothesis among equals
    int bc = -1, bh = 0x7fffffff;
    for (int h = tid; h < hypotheses; h += kFinThreads) {
        const int c = __float_as_int(hyp[((size_t)p * hypotheses + h) * kHypRecord + 9]);
        if (c > bc) bc = c, bh = h;
    }
    best_c[tid] = bc, best_h[tid] = bh;
    __syncthreads();
#pragma unroll
    for (int s = kFinThreads / 2; s > 0; s >>= 1) {
        if (tid < s) {
            const int oc = best_c[tid + s], oh = best_h[tid + s];
            if (oc > best_c[tid] || (oc == best_c[tid] && oh < best_h[tid])) best_c[tid] = oc, best_h[tid] = oh;
        }
        __syncthreads();
    }
    bc = best_c[0], bh = best_h[0];
    const bool valid = count >= M::kMin && bc >= M::kMin;  // (the same for the whole workgroup)

    float f[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) f[k] = 0.f;
    int num = 0;
    if (valid) {
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = hyp[((size_t)p * hypotheses + bh) * kHypRecord + k];
        stage_pair(a, p, count, pts, tid, kFinThreads);
        __syncthreads();
        for (int round = 0;; ++round) {
            int mine = 0;
            for (int k = tid; k < count; k += kFinThreads) {
                const float4 q = pts[k];
                const bool in = M::inlier(f, q.x, q.y, q.z, q.w, thr2);
                mask[k] = in ? 1 : 0;
                mine += in ? 1 : 0;
            }
            num = (int)block_sum<kFinThreads>((double)mine, buf, tid);  // (exact: integers below 2^53)
            if (round >= refits || num < M::kMin) break;
            // normalised least squares over the inliers (8-point; the homography's DLT)
            double c[4], s[2];
            hartley<kFinThreads>(pts, mask, count, (double)num, buf, tid, c, s, PixelCoord{});
            {   // the upper triangle of the normal matrix: a thread sums its inliers (every 256th from tid on, in
                // ascending order) into 45 registers
                double acc[45];
#pragma unroll
                for (int e = 0; e < 45; ++e) acc[e] = 0.0;
                for (int k = tid; k < count; k += kFinThreads) {
                    if (!mask[k]) continue;
                    const float4 q = pts[k];
                    const double x0 = ((double)q.x - c[0]) * s[0], y0 = ((double)q.y - c[1]) * s[0];
                    const double x1 = ((double)q.z - c[2]) * s[1], y1 = ((double)q.w - c[3]) * s[1];
                    M::accumulate(acc, x0, y0, x1, y1);
                }
                normal_eigenvector(acc, part, am, vm, rot, tid);
            }
            if (tid == 0) {
                int lo = 0;
                for (int k = 1; k < 9; ++k) lo = am[10 * k] < am[10 * lo] ? k : lo;
                double fn[9], fd[9];
                for (int k = 0; k < 9; ++k) fn[k] = vm[9 * k + lo];
                fnew_ok = M::finish(fn, c, s, fd) ? 1 : 0;
                for (int k = 0; k < 9; ++k) fnew[k] = fd[k];
            }
            __syncthreads();
            if (!fnew_ok) break;  // a refit that is not finite keeps the previous F and mask
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = (float)fnew[k];
            __syncthreads();
        }
        fix_sign(f);
    }
    if (tid < 9) f_out[(size_t)p * 9 + tid] = f[tid];
    for (int k = tid; k < a.kmax; k += kFinThreads) inl_out[(size_t)p * a.kmax + k] = valid && k < count ? mask[k] : 0;
    if (tid == 0) num_out[p] = valid ? num : 0, valid_out[p] = valid ? 1 : 0, best_out[p] = valid ? bh : -1;
}

size_t hyp_bytes(int32_t pairs, int32_t hypotheses) { return (size_t)pairs * hypotheses * kHypRecord * sizeof(float); }

// The entry points below, one per model M.
template <class M>
int32_t ransac_call(const char* who, const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                    int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, float threshold, int32_t hypotheses, int32_t refits,
                    int32_t seed, void* workspace, size_t workspace_bytes, float* m, uint8_t* inliers, int32_t* num_inliers,
                    int32_t* valid, int32_t* best, hipStream_t stream) {
    if (!pair_args_ok(matches, counts, kpts0, kpts1, pairs, kmax, k0, k1) ||
        !ransac_args_ok(threshold, hypotheses, refits, workspace, workspace_bytes, hyp_bytes(pairs, hypotheses), m, inliers,
                        num_inliers, valid, best))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    const float thr2 = threshold * threshold;
    hipLaunchKernelGGL((ransac_hypothesis_kernel<M, false>), hyp_grid(hypotheses, pairs), dim3(kHypThreads), 0, stream, a,
                       hypotheses, (uint32_t)seed, thr2, (const int32_t*)nullptr, (float*)workspace, (float*)nullptr,
                       (int32_t*)nullptr);
    hipLaunchKernelGGL(ransac_finalize_kernel<M>, dim3(pairs), dim3(kFinThreads), 0, stream, a, hypotheses, refits, thr2,
                       (const float*)workspace, m, inliers, num_inliers, valid, best);
    return launched(who);
}

template <class M>
int32_t solve_call(const char* who, const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                   int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const int32_t* samples, int32_t hypotheses,
                   float* candidates, int32_t* num, hipStream_t stream) {
    if (!pair_args_ok(matches, counts, kpts0, kpts1, pairs, kmax, k0, k1) || !solve_args_ok(hypotheses, samples, candidates, num))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    hipLaunchKernelGGL((ransac_hypothesis_kernel<M, true>), hyp_grid(hypotheses, pairs), dim3(kHypThreads), 0, stream, a,
                       hypotheses, 0u, 1.f, samples, (float*)nullptr, candidates, num);
    return launched(who);
}

template <class M>
int32_t score_call(const char* who, const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                   int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* candidates, int32_t num_candidates,
                   float threshold, int32_t* inlier_counts, hipStream_t stream) {
    if (!pair_args_ok(matches, counts, kpts0, kpts1, pairs, kmax, k0, k1) ||
        !score_args_ok(threshold, num_candidates, candidates, inlier_counts))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    hipLaunchKernelGGL(ransac_score_kernel<M>, hyp_grid(num_candidates, pairs), dim3(kHypLanes), 0, stream, a, candidates,
                       num_candidates, threshold * threshold, inlier_counts);
    return launched(who);
}

}  // namespace

extern "C" {

size_t lg_ransac_workspace(int32_t pairs, int32_t kmax, int32_t hypotheses) {
    if (pairs <= 0 || kmax <= 0 || hypotheses <= 0) return 0;
    return hyp_bytes(pairs, hypotheses);
}

int32_t lg_ransac_fundamental(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                              int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, float threshold, int32_t hypotheses,
                              int32_t refits, int32_t seed, void* workspace, size_t workspace_bytes, float* f,
                              uint8_t* inliers, int32_t* num_inliers, int32_t* valid, int32_t* best, hipStream_t stream) {
    return ransac_call<FundamentalModel>("lg_ransac_fundamental", matches, counts, kpts0, kpts1, pairs, kmax, k0, k1, threshold,
                                         hypotheses, refits, seed, workspace, workspace_bytes, f, inliers, num_inliers, valid,
                                         best, stream);
}

int32_t lg_ransac_homography(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                             int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, float threshold, int32_t hypotheses,
                             int32_t refits, int32_t seed, void* workspace, size_t workspace_bytes, float* h,
                             uint8_t* inliers, int32_t* num_inliers, int32_t* valid, int32_t* best, hipStream_t stream) {
    return ransac_call<HomographyModel>("lg_ransac_homography", matches, counts, kpts0, kpts1, pairs, kmax, k0, k1, threshold,
                                        hypotheses, refits, seed, workspace, workspace_bytes, h, inliers, num_inliers, valid, best,
                                        stream);
}

int32_t lg_ransac_samples(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream) {
    return samples_call<7>("lg_ransac_samples", count, hypotheses, seed, samples, stream);
}

int32_t lg_ransac_samples4(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream) {
    return samples_call<4>("lg_ransac_samples4", count, hypotheses, seed, samples, stream);
}

int32_t lg_ransac_solve7(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1, int32_t pairs,
                         int32_t kmax, int32_t k0, int32_t k1, const int32_t* samples, int32_t hypotheses, float* candidates,
                         int32_t* num_roots, hipStream_t stream) {
    return solve_call<FundamentalModel>("lg_ransac_solve7", matches, counts, kpts0, kpts1, pairs, kmax, k0, k1, samples, hypotheses,
                                        candidates, num_roots, stream);
}

int32_t lg_ransac_solve4(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1, int32_t pairs,
                         int32_t kmax, int32_t k0, int32_t k1, const int32_t* samples, int32_t hypotheses, float* candidates,
                         int32_t* num, hipStream_t stream) {
    return solve_call<HomographyModel>("lg_ransac_solve4", matches, counts, kpts0, kpts1, pairs, kmax, k0, k1, samples, hypotheses,
                                       candidates, num, stream);
}

int32_t lg_ransac_score(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1, int32_t pairs,
                        int32_t kmax, int32_t k0, int32_t k1, const float* candidates, int32_t num_candidates, float threshold,
                        int32_t* inlier_counts, hipStream_t stream) {
    return score_call<FundamentalModel>("lg_ransac_score", matches, counts, kpts0, kpts1, pairs, kmax, k0, k1, candidates,
                                        num_candidates, threshold, inlier_counts, stream);
}

int32_t lg_ransac_score_homography(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                                   int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* candidates,
                                   int32_t num_candidates, float threshold, int32_t* inlier_counts, hipStream_t stream) {
    return score_call<HomographyModel>("lg_ransac_score_homography", matches, counts, kpts0, kpts1, pairs, kmax, k0, k1, candidates,
                                       num_candidates, threshold, inlier_counts, stream);
}

}  // extern "C"
