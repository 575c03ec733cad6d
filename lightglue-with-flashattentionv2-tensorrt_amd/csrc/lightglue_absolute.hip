// lightglue_absolute.hip — the absolute pose (include/lightglue_glue.h, "the absolute pose"): the pose of a camera from
// 2D-3D correspondences by P3P RANSAC, what cv::solvePnPRansac does on the host, and the link that carries the 3D points
// lg_triangulate wrote for one image pair onto the match rows of the next pair, so that a sequence's poses share one
// frame and one scale. The scheme is lightglue_geometry.hip's, whose launch shapes and helpers
// (lightglue_geometry_device.h) this file shares. The contract is restated in float64 in
// lightglue_amd/geometry_contract.py (by another route); the arithmetic, and the P3P route, are in
// lightglue_absolute_math.h.
//
// lg_ransac_absolute, two launches. absolute_hypothesis_kernel: grid (hypothesis blocks, pairs), 64 hypotheses a
// workgroup, four adjacent lanes a hypothesis. The workgroup gathers the pair's correspondences (five floats each) into
// LDS once. The four lanes hash the same 3 indices and set up the same quartic; lane s then owns piece s of the four
// the quartic is monotonic on: it bisects its piece and builds its root's pose, so the at most four candidates of a
// hypothesis are found side by side. The lanes rank their candidates by |R X_s0 + t| through lane shuffles; in that
// order each candidate's pose is passed to the four, each counts every fourth correspondence in LDS, and the best
// candidate's lane writes (R, t, count) to the workspace. absolute_finalize_kernel: one workgroup per pair reduces the
// hypotheses to the winner, marks its inliers and runs the refits: kAbsoluteLmRounds rounds of Levenberg-Marquardt in
// fp64 on (ω, δt) over the round's fixed set, one pass over the rows a round (lightglue_polish.hip's shape: sums in
// registers, a shuffle tree over each wave, the four waves added in index order, every thread solving the 6 x 6 system
// alike), then the mask again; a round that counts fewer inliers is dropped and ends the rounds.
// lg_link_landmarks: one workgroup per pair; the owner of each shared keypoint in LDS by an integer atomicMin over
// pair A's rows (the lowest row wins: the result does not depend on the order), then pair B's linked rows compacted in
// ascending order by a workgroup prefix sum. No floating-point atomics, no allocation, no host synchronisation.
#include "lightglue_geometry_device.h"
#include "lightglue_absolute_math.h"

namespace {

struct AbsArgs {
    const float* points;     // [pairs, kmax, 3]
    const float* image;      // [pairs, kmax, 2]
    const int32_t* counts;   // [pairs]
    const float* intr;       // [pairs, 4]
    int kmax;
};

__device__ __forceinline__ int abs_count(const AbsArgs& a, int p) { return min(max(a.counts[p], 0), a.kmax); }

__device__ __forceinline__ Camera load_camera(const AbsArgs& a, int p) {
    const float* k = a.intr + (size_t)p * 4;
    return Camera{k[0], k[1], k[2], k[3]};
}

// The pair's correspondences into LDS: (X, Y, Z, x) and y.
__device__ __forceinline__ void stage_abs(const AbsArgs& a, int p, int count, float4* pa, float* pb, int tid, int nthreads) {
    for (int k = tid; k < count; k += nthreads) {
        const size_t row = (size_t)p * a.kmax + k;
        pa[k] = make_float4(a.points[3 * row], a.points[3 * row + 1], a.points[3 * row + 2], a.image[2 * row]);
        pb[k] = a.image[2 * row + 1];
    }
}

// GIVEN: the samples are an input and every candidate an output (lg_ransac_solve3); else the samples are hashed, the
// candidates scored and the best one's record goes to the workspace.
template <bool GIVEN>
__global__ __launch_bounds__(kHypThreads) void absolute_hypothesis_kernel(AbsArgs a, int hypotheses, uint32_t seed, float thr2,
                                                                           const int32_t* __restrict__ samples,
                                                                           float* __restrict__ hyp, float* __restrict__ cand_out,
                                                                           int32_t* __restrict__ num_out) {
    __shared__ float4 pa[kMaxPoints];
    __shared__ float pb[kMaxPoints];
    const int p = blockIdx.y, tid = threadIdx.x, sub = tid % kHypSplit;
    const int h = blockIdx.x * kHypLanes + tid / kHypSplit;
    const int base = (tid % 64) - sub;  // the hypothesis' first lane in its wave
    const int count = abs_count(a, p);
    const Camera cam = load_camera(a, p);
    const bool pair_ok = count >= kMinInliersA && camera_ok(cam);  // (the same for the whole workgroup)
    // a hypothesis past the last solves the last again (the shuffles want all four lanes of every hypothesis of a
    // wave in step) and writes nothing
    const bool live = h < hypotheses;
    const int hh = live ? h : hypotheses - 1;
    float pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = 0.f;
    bool ok = false;
    double key = INFINITY;
    if (pair_ok) {
        stage_abs(a, p, count, pa, pb, tid, kHypThreads);
        __syncthreads();
        int idx[3];
        if constexpr (GIVEN) {
#pragma unroll
            for (int j = 0; j < 3; ++j) idx[j] = min(max(samples[(size_t)hh * 3 + j], 0), count - 1);
        } else {
            sample<3>(seed, hh, count, idx);
        }
        double x[3][3], px[3][2];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float4 q = pa[idx[j]];
            x[j][0] = (double)q.x, x[j][1] = (double)q.y, x[j][2] = (double)q.z;
            px[j][0] = (double)q.w, px[j][1] = (double)pb[idx[j]];
        }
        P3p s;
        p3p_setup(x, px, cam, s);
        double u;
        const bool has = p3p_root(s, sub, u);
        AbsPose q;
        ok = p3p_pose(s, x, u, q.r, q.t, key) && has;
        float rounded[12];
        ok = absolute_round(q, rounded) && ok;
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = ok ? rounded[k] : 0.f;
        key = ok ? key : INFINITY;
    }
    // the lane's place among the hypothesis' candidates: ascending key, the lower lane among equals
    int rank = 0, n = 0;
#pragma unroll
    for (int j = 0; j < kHypSplit; ++j) {
        const double kj = __shfl(key, base + j);
        const int oj = __shfl(ok ? 1 : 0, base + j);
        rank += oj && (kj < key || (kj == key && j < sub)) ? 1 : 0;
        n += oj;
    }
    if constexpr (GIVEN) {
        float* out = cand_out + ((size_t)p * hypotheses + hh) * (12 * kCands3);
        if (live && ok) {
#pragma unroll
            for (int k = 0; k < 12; ++k) out[12 * rank + k] = pose[k];
        }
        if (live && sub == 0) {
            for (int k = 12 * n; k < 12 * kCands3; ++k) out[k] = 0.f;
            num_out[(size_t)p * hypotheses + hh] = n;
        }
    } else {
        // the highest count; among equals the first in the candidates' order
        int bn = -1, bpos = -1;
#pragma unroll
        for (int pos = 0; pos < kCands3; ++pos) {
            int src = -1;
#pragma unroll
            for (int j = 0; j < kHypSplit; ++j) src = __shfl(ok ? rank : -1, base + j) == pos ? j : src;
            if (src < 0) continue;  // (the four lanes alike)
            float ps[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) ps[k] = __shfl(pose[k], base + src);
            int got = 0;
#pragma unroll 4
            for (int k = sub; k < count; k += kHypSplit) {
                const float4 q = pa[k];
                got += is_inlier_abs(ps, cam, q.x, q.y, q.z, q.w, pb[k], thr2) ? 1 : 0;
            }
#pragma unroll
            for (int d = 1; d < kHypSplit; d <<= 1) got += __shfl_xor(got, d);  // (integers: the order does not matter)
            const bool take = got > bn;
            bn = take ? got : bn, bpos = take ? pos : bpos;
        }
        if (!live) return;
        if (bpos < 0 ? sub != 0 : !(ok && rank == bpos)) return;
        float* rec = hyp + ((size_t)p * hypotheses + h) * kAbsRecord;
#pragma unroll
        for (int k = 0; k < 12; ++k) rec[k] = bpos < 0 ? 0.f : pose[k];
        rec[12] = __int_as_float(max(bn, 0)), rec[13] = 0.f, rec[14] = 0.f, rec[15] = 0.f;
    }
}

// Marks the inliers of the pose into m and returns their number (every thread).
__device__ __forceinline__ int mark_abs(const float pose[12], const Camera& cam, const float4* pa, const float* pb, int count,
                                        float thr2, uint8_t* m, double* buf, int tid) {
    int mine = 0;
    for (int k = tid; k < count; k += kFinThreads) {
        const float4 q = pa[k];
        const bool in = is_inlier_abs(pose, cam, q.x, q.y, q.z, q.w, pb[k], thr2);
        m[k] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    return (int)block_sum<kFinThreads>((double)mine, buf, tid);  // (exact: integers below 2^53)
}

// One pass over the pair's rows at the pose q: the kAbsSums sums over the rows k with (FIRST ? mask[k] and a finite
// residual at a positive depth, which also defines fixed[k] : fixed[k]), the same bits in every thread. A thread reads
// only the fixed[] entries it wrote. part: [kFinThreads / 64][kAbsSums] in LDS.
template <bool FIRST>
__device__ __forceinline__ void absolute_pass(const AbsPose& q, const Camera& cam, const float4* pa, const float* pb,
                                              const uint8_t* mask, uint8_t* fixed, int count, double (*part)[kAbsSums], int tid,
                                              double sums[kAbsSums]) {
    double acc[kAbsSums];
#pragma unroll
    for (int e = 0; e < kAbsSums; ++e) acc[e] = 0.0;
    for (int k = tid; k < count; k += kFinThreads) {
        if constexpr (FIRST) fixed[k] = 0;  // (a later pass reads every row's entry)
        if (!(FIRST ? mask[k] : fixed[k])) continue;
        const float4 w = pa[k];
        double res[2], j[2][6];
        const bool fin = absolute_row(q, cam, (double)w.x, (double)w.y, (double)w.z, (double)w.w, (double)pb[k], res, j);
        if constexpr (FIRST) {
            fixed[k] = fin ? 1 : 0;
            if (!fin) continue;
        }
        absolute_accumulate(acc, res, j);
    }
    __syncthreads();  // (the last pass's readers of part are done)
#pragma unroll
    for (int e = 0; e < kAbsSums; ++e) {
        double v = acc[e];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (tid % 64 == 0) part[tid / 64][e] = v;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kAbsSums; ++e) sums[e] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
}

__global__ __launch_bounds__(kFinThreads) void absolute_finalize_kernel(AbsArgs a, int hypotheses, int refits, float thr2,
                                                                         const float* __restrict__ hyp, float* __restrict__ r_out,
                                                                         float* __restrict__ t_out, uint8_t* __restrict__ inl_out,
                                                                         int32_t* __restrict__ num_out,
                                                                         int32_t* __restrict__ valid_out,
                                                                         int32_t* __restrict__ best_out) {
    __shared__ float4 pa[kMaxPoints];
    __shared__ float pb[kMaxPoints];
    __shared__ uint8_t mask[kMaxPoints], fixed[kMaxPoints], trial[kMaxPoints];
    __shared__ double buf[kFinThreads];
    __shared__ int best_c[kFinThreads], best_h[kFinThreads];
    __shared__ double part[kFinThreads / 64][kAbsSums];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int count = abs_count(a, p);
    const Camera cam = load_camera(a, p);

    // the winner: the highest count, the lowest hypothesis among equals
    int bc = -1, bh = 0x7fffffff;
    for (int h = tid; h < hypotheses; h += kFinThreads) {
        const int c = __float_as_int(hyp[((size_t)p * hypotheses + h) * kAbsRecord + 12]);
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
    const bool valid = count >= kMinInliersA && camera_ok(cam) && bc >= kMinInliersA;  // (the whole workgroup alike)

    float pose[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = 0.f;
    int num = 0;
    if (valid) {
        const float* rec = hyp + ((size_t)p * hypotheses + bh) * kAbsRecord;
#pragma unroll
        for (int k = 0; k < 12; ++k) pose[k] = rec[k];
        stage_abs(a, p, count, pa, pb, tid, kFinThreads);
        __syncthreads();
        num = mark_abs(pose, cam, pa, pb, count, thr2, mask, buf, tid);
        // (everything below that decides a branch is the same in every thread of the workgroup)
#pragma unroll 1
        for (int round = 0; round < refits && num >= kMinInliersA; ++round) {
            AbsPose st;
            if (!absolute_enter(pose, st)) break;
            double sums[kAbsSums];
            absolute_pass<true>(st, cam, pa, pb, mask, fixed, count, part, tid, sums);
            if (!((int)sums[28] >= kMinAbsRows && finite64(sums[27]))) break;
            double lambda = kLambdaStart;
#pragma unroll 1
            for (int it = 0; it < kAbsoluteLmRounds; ++it) {
                double delta[6];
                bool take = absolute_step(sums, lambda, delta);
                if (take) {  // (a rejected solve spares the pass)
                    AbsPose next;
                    double again[kAbsSums];
                    absolute_update(st, delta, next);
                    absolute_pass<false>(next, cam, pa, pb, mask, fixed, count, part, tid, again);
                    take = finite64(again[27]) && again[27] < sums[27];
                    if (take) {
                        st = next;
#pragma unroll
                        for (int e = 0; e < kAbsSums; ++e) sums[e] = again[e];
                    }
                }
                lambda = take ? fmax(lambda * 0.1, kLambdaMin) : fmin(lambda * 10.0, kLambdaMax);
            }
            float fine[12];
            if (!absolute_round(st, fine)) break;  // a refit that is not finite keeps the previous pose and mask
            const int again = mark_abs(fine, cam, pa, pb, count, thr2, trial, buf, tid);
            if (again < num) break;  // a refit that loses inliers is dropped
            num = again;
#pragma unroll
            for (int k = 0; k < 12; ++k) pose[k] = fine[k];
            for (int k = tid; k < count; k += kFinThreads) mask[k] = trial[k];
            __syncthreads();
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {  // (thread k writes entry k: no array is indexed by the thread)
        if (tid == k) r_out[(size_t)p * 9 + k] = pose[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (tid == k) t_out[(size_t)p * 3 + k] = pose[9 + k];
    }
    for (int k = tid; k < a.kmax; k += kFinThreads) inl_out[(size_t)p * a.kmax + k] = valid && k < count ? mask[k] : 0;
    if (tid == 0) num_out[p] = valid ? num : 0, valid_out[p] = valid ? 1 : 0, best_out[p] = valid ? bh : -1;
}

// lg_ransac_score_absolute: four lanes a pose, as the hypothesis kernel scores a candidate.
__global__ __launch_bounds__(kHypThreads) void absolute_score_kernel(AbsArgs a, const float* __restrict__ poses, int num,
                                                                      float thr2, int32_t* __restrict__ out) {
    __shared__ float4 pa[kMaxPoints];
    __shared__ float pb[kMaxPoints];
    const int p = blockIdx.y, tid = threadIdx.x, sub = tid % kHypSplit;
    const int c = blockIdx.x * kHypLanes + tid / kHypSplit;
    const int count = abs_count(a, p);
    const Camera cam = load_camera(a, p);
    const bool live = c < num;
    const int cc = live ? c : num - 1;
    stage_abs(a, p, count, pa, pb, tid, kHypThreads);
    __syncthreads();
    float ps[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) ps[k] = poses[((size_t)p * num + cc) * 12 + k];
    int got = 0;
#pragma unroll 4
    for (int k = sub; k < count; k += kHypSplit) {
        const float4 q = pa[k];
        got += is_inlier_abs(ps, cam, q.x, q.y, q.z, q.w, pb[k], thr2) ? 1 : 0;
    }
#pragma unroll
    for (int d = 1; d < kHypSplit; d <<= 1) got += __shfl_xor(got, d);
    if (live && sub == 0) out[(size_t)p * num + c] = camera_ok(cam) ? got : 0;
}

struct LinkArgs {
    const int32_t* matches_a;  // [pairs, kmax_a, 2]
    const int32_t* counts_a;   // [pairs]
    const float* points_a;     // [pairs, kmax_a, 3]
    const uint8_t* ok_a;       // [pairs, kmax_a]
    const int32_t* matches_b;  // [pairs, kmax_b, 2]
    const int32_t* counts_b;   // [pairs]
    const float* kpts_b1;      // [pairs, k_b1, 2]
    int side_a, kmax_a, kmax_b, k_shared, k_b1;
};

constexpr int kNoOwner = 0x7fffffff;

__global__ __launch_bounds__(kFinThreads) void link_kernel(LinkArgs a, float* __restrict__ points, float* __restrict__ image,
                                                            int32_t* __restrict__ rows, int32_t* __restrict__ n_out) {
    __shared__ int owner[kMaxPoints];
    __shared__ int scan[kFinThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    for (int s = tid; s < a.k_shared; s += kFinThreads) owner[s] = kNoOwner;
    __syncthreads();
    const int ca = min(max(a.counts_a[p], 0), a.kmax_a), cb = min(max(a.counts_b[p], 0), a.kmax_b);
    for (int r = tid; r < ca; r += kFinThreads) {
        const size_t row = (size_t)p * a.kmax_a + r;
        if (!a.ok_a[row]) continue;
        const int s = min(max(a.matches_a[2 * row + a.side_a], 0), a.k_shared - 1);
        atomicMin(&owner[s], r);  // (an integer minimum in LDS: the same whatever the order)
    }
    __syncthreads();
    // a thread's rows are adjacent, so that the threads' counts scanned in thread order give the rows' order
    const int chunk = (a.kmax_b + kFinThreads - 1) / kFinThreads;
    const int lo = tid * chunk, hi = min(lo + chunk, cb);
    int mine = 0;
    for (int k = lo; k < hi; ++k) {
        const int s = min(max(a.matches_b[((size_t)p * a.kmax_b + k) * 2], 0), a.k_shared - 1);
        mine += owner[s] != kNoOwner ? 1 : 0;
    }
    scan[tid] = mine;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < kFinThreads; d <<= 1) {
        const int v = tid >= d ? scan[tid - d] : 0;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    const int total = scan[kFinThreads - 1];
    int pos = scan[tid] - mine;
    for (int k = lo; k < hi; ++k) {
        const size_t row = (size_t)p * a.kmax_b + k;
        const int s = min(max(a.matches_b[2 * row], 0), a.k_shared - 1);
        const int o = owner[s];
        if (o == kNoOwner) continue;
        const int i1 = min(max(a.matches_b[2 * row + 1], 0), a.k_b1 - 1);
        const size_t dst = (size_t)p * a.kmax_b + pos, src = (size_t)p * a.kmax_a + o;
        points[3 * dst] = a.points_a[3 * src], points[3 * dst + 1] = a.points_a[3 * src + 1], points[3 * dst + 2] = a.points_a[3 * src + 2];
        image[2 * dst] = a.kpts_b1[((size_t)p * a.k_b1 + i1) * 2], image[2 * dst + 1] = a.kpts_b1[((size_t)p * a.k_b1 + i1) * 2 + 1];
        rows[dst] = k;
        ++pos;
    }
    for (int k = total + tid; k < a.kmax_b; k += kFinThreads) {
        const size_t dst = (size_t)p * a.kmax_b + k;
        points[3 * dst] = 0.f, points[3 * dst + 1] = 0.f, points[3 * dst + 2] = 0.f;
        image[2 * dst] = 0.f, image[2 * dst + 1] = 0.f;
        rows[dst] = -1;
    }
    if (tid == 0) n_out[p] = total;
}

size_t abs_bytes(int32_t pairs, int32_t hypotheses) { return (size_t)pairs * hypotheses * kAbsRecord * sizeof(float); }

bool abs_args_ok(const float* points, const float* image, const int32_t* counts, const float* intrinsics, int32_t pairs,
                 int32_t kmax) {
    return pairs >= 0 && pairs <= 65535 && kmax >= 1 && kmax <= kMaxPoints && (int64_t)pairs * kmax <= (1 << 28) && points && image &&
           counts && intrinsics && aligned4(points) && aligned4(image) && aligned4(counts) && aligned4(intrinsics);
}

}  // namespace

extern "C" {

int32_t lg_link_landmarks(const int32_t* matches_a, const int32_t* counts_a, const float* points_a, const uint8_t* ok_a,
                          int32_t side_a, const int32_t* matches_b, const int32_t* counts_b, const float* kpts_b1, int32_t pairs,
                          int32_t kmax_a, int32_t kmax_b, int32_t k_shared, int32_t k_b1, float* points, float* image,
                          int32_t* rows, int32_t* n, hipStream_t stream) {
    const char* who = "lg_link_landmarks";
    const int64_t lim = 1 << 28;
    if (pairs < 0 || pairs > 65535 || kmax_a < 1 || kmax_a > kMaxPoints || kmax_b < 1 || kmax_b > kMaxPoints || k_shared < 1 ||
        k_shared > kMaxPoints || k_b1 < 1 || (int64_t)pairs * k_b1 > lim || (side_a != 0 && side_a != 1) || !matches_a ||
        !counts_a || !points_a || !ok_a || !matches_b || !counts_b || !kpts_b1 || !points || !image || !rows || !n ||
        !aligned4(matches_a) || !aligned4(counts_a) || !aligned4(points_a) || !aligned4(matches_b) || !aligned4(counts_b) ||
        !aligned4(kpts_b1) || !aligned4(points) || !aligned4(image) || !aligned4(rows) || !aligned4(n))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const LinkArgs a{matches_a, counts_a, points_a, ok_a, matches_b, counts_b, kpts_b1, side_a, kmax_a, kmax_b, k_shared, k_b1};
    hipLaunchKernelGGL(link_kernel, dim3(pairs), dim3(kFinThreads), 0, stream, a, points, image, rows, n);
    return launched(who);
}

size_t lg_ransac_absolute_workspace(int32_t pairs, int32_t kmax, int32_t hypotheses) {
    if (pairs <= 0 || kmax <= 0 || hypotheses <= 0) return 0;
    return abs_bytes(pairs, hypotheses);
}

int32_t lg_ransac_absolute(const float* points, const float* image, const int32_t* counts, const float* intrinsics,
                           int32_t pairs, int32_t kmax, float threshold, int32_t hypotheses, int32_t refits, int32_t seed,
                           void* workspace, size_t workspace_bytes, float* r, float* t, uint8_t* inliers, int32_t* num_inliers,
                           int32_t* valid, int32_t* best, hipStream_t stream) {
    const char* who = "lg_ransac_absolute";
    if (!abs_args_ok(points, image, counts, intrinsics, pairs, kmax) ||
        !ransac_args_ok(threshold, hypotheses, refits, workspace, workspace_bytes, abs_bytes(pairs, hypotheses), r, inliers,
                        num_inliers, valid, best) ||
        !t || !aligned4(t))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const AbsArgs a{points, image, counts, intrinsics, kmax};
    const float thr2 = threshold * threshold;
    hipLaunchKernelGGL(absolute_hypothesis_kernel<false>, hyp_grid(hypotheses, pairs), dim3(kHypThreads), 0, stream, a, hypotheses,
                       (uint32_t)seed, thr2, (const int32_t*)nullptr, (float*)workspace, (float*)nullptr, (int32_t*)nullptr);
    hipLaunchKernelGGL(absolute_finalize_kernel, dim3(pairs), dim3(kFinThreads), 0, stream, a, hypotheses, refits, thr2,
                       (const float*)workspace, r, t, inliers, num_inliers, valid, best);
    return launched(who);
}

int32_t lg_ransac_samples3(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream) {
    return samples_call<3>("lg_ransac_samples3", count, hypotheses, seed, samples, stream);
}

int32_t lg_ransac_solve3(const float* points, const float* image, const int32_t* counts, const float* intrinsics, int32_t pairs,
                         int32_t kmax, const int32_t* samples, int32_t hypotheses, float* candidates, int32_t* num,
                         hipStream_t stream) {
    const char* who = "lg_ransac_solve3";
    if (!abs_args_ok(points, image, counts, intrinsics, pairs, kmax) || !solve_args_ok(hypotheses, samples, candidates, num))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const AbsArgs a{points, image, counts, intrinsics, kmax};
    hipLaunchKernelGGL(absolute_hypothesis_kernel<true>, hyp_grid(hypotheses, pairs), dim3(kHypThreads), 0, stream, a, hypotheses,
                       0u, 1.f, samples, (float*)nullptr, candidates, num);
    return launched(who);
}

int32_t lg_ransac_score_absolute(const float* points, const float* image, const int32_t* counts, const float* intrinsics,
                                 int32_t pairs, int32_t kmax, const float* poses, int32_t num_poses, float threshold,
                                 int32_t* inlier_counts, hipStream_t stream) {
    const char* who = "lg_ransac_score_absolute";
    if (!abs_args_ok(points, image, counts, intrinsics, pairs, kmax) || !score_args_ok(threshold, num_poses, poses, inlier_counts))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const AbsArgs a{points, image, counts, intrinsics, kmax};
    hipLaunchKernelGGL(absolute_score_kernel, hyp_grid(num_poses, pairs), dim3(kHypThreads), 0, stream, a, poses, num_poses,
                       threshold * threshold, inlier_counts);
    return launched(who);
}

}  // extern "C"
