// lightglue_essential.hip — calibrated relative pose (include/lightglue_glue.h, "geometric verification"): an
// essential matrix per image pair by five-point RANSAC over the matcher's matches, and (R, t) from it, by the scheme
// of lightglue_geometry.hip, whose launch shapes and helpers (lightglue_geometry_device.h) this file shares. The
// contract is restated in float64 in lightglue_amd/geometry_contract.py; the arithmetic is in
// lightglue_essential_math.h, and what the pose polish (lightglue_polish.hip) shares with this file in
// lightglue_essential_device.h.
//
// Two launches. essential_hypothesis_kernel: grid (hypothesis blocks, pairs), 64 hypotheses a workgroup, four
// adjacent lanes a hypothesis. The workgroup gathers the pair's correspondences into LDS once. The four lanes hash
// the same 5 indices and compute the same orthonormal null-space basis; then each holds five columns of the 10 x 20
// constraint matrix (50 doubles; the whole does not fit a lane), and the elimination passes each pivot column from
// the lane that holds it to the other three by lane shuffles. Rows 4..9 of the reduced right block go to all four,
// which find the roots of the degree-10 polynomial alike; lane s builds the candidates of roots s, s + 4, s + 8 (E in
// camera coordinates, F = K1⁻ᵀ E K0⁻¹ in pixels, fp32). For scoring each candidate's F is passed to the four lanes in
// turn and each counts every fourth correspondence in LDS. (F, E, count) of the best candidate goes to the workspace.
// essential_finalize_kernel: one workgroup per pair reduces the hypotheses to the winner, marks its inliers, runs the
// refits in fp64 (camera coordinates, Hartley, normal matrix, Jacobi on the 9 x 9, de-normalise, the nearest
// essential matrix; a round that counts fewer inliers is dropped and ends the rounds), takes the pose with the most
// inliers in front of both cameras and writes every output. No atomics, no allocation, no host synchronisation.
#include "lightglue_essential_device.h"

namespace {

constexpr int kPoseRecord = 20;  // floats per hypothesis in the workspace: F[9] (pixels), E[9] (camera), count, pad

__device__ __forceinline__ double from_lane(double v, int lane) { return __shfl(v, lane); }

// Steps C.. of the elimination: the lane that holds column C hands it to the four.
template <int C>
__device__ __forceinline__ void eliminate(double a[10][5], int base, double& low) {
    double col[10];
#pragma unroll
    for (int r = 0; r < 10; ++r) col[r] = from_lane(a[r][C % 5], base + C / 5);
    const double piv = slice_step<C>(a, col);
    low = piv < low || !(piv == piv) ? piv : low;
    if constexpr (C < 9) eliminate<C + 1>(a, base, low);
}

// GIVEN: the samples are an input and every candidate E an output (lg_ransac_solve5); else the samples are hashed,
// the candidates scored and the best one's record goes to the workspace.
template <bool GIVEN>
__global__ __launch_bounds__(kHypThreads) void essential_hypothesis_kernel(PairArgs a, const float* __restrict__ intr,
                                                                            int hypotheses, uint32_t seed, float thr2,
                                                                            const int32_t* __restrict__ samples,
                                                                            float* __restrict__ hyp, float* __restrict__ cand_out,
                                                                            int32_t* __restrict__ num_out) {
    __shared__ float4 pts[kMaxPoints];
    const int p = blockIdx.y, tid = threadIdx.x, sub = tid % kHypSplit;
    const int h = blockIdx.x * kHypLanes + tid / kHypSplit;
    const int base = (tid % 64) - sub;  // the hypothesis' first lane in its wave
    const int count = pair_count(a, p);
    const Intrinsics kk = load_intrinsics(intr, p);
    const bool pair_ok = count >= kMinInliersE && intrinsics_ok(kk);  // (the same for the whole workgroup)
    // a hypothesis past the last solves the last again (the shuffles want all four lanes of every hypothesis of a
    // wave in step) and writes nothing
    const bool live = h < hypotheses;
    const int hh = live ? h : hypotheses - 1;
    float cf[3][9], ce[3][9];  // the lane's candidates: roots sub, sub + 4, sub + 8
    bool cok[3] = {false, false, false};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 9; ++k) cf[i][k] = 0.f, ce[i][k] = 0.f;
    if (pair_ok) {
        stage_pair(a, p, count, pts, tid, kHypThreads);
        __syncthreads();
        int idx[5];
        if constexpr (GIVEN) {
#pragma unroll
            for (int j = 0; j < 5; ++j) idx[j] = min(max(samples[(size_t)hh * 5 + j], 0), count - 1);
        } else {
            sample<5>(seed, hh, count, idx);
        }
        double x0[5], y0[5], x1[5], y1[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            double c[4];
            camera(pts[idx[j]], kk, c);
            x0[j] = c[0], y0[j] = c[1], x1[j] = c[2], y1[j] = c[3];
        }
        double basis[4][9];
        bool ok = null_space5(x0, y0, x1, y1, basis);
        double rhs[6][10];
        {
            double m[10][5];
            fill_slice(basis, sub, m);
            double low = INFINITY;
            eliminate<0>(m, base, low);
            ok = ok && low >= (double)kPivotEps;  // (NaN: false)
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int j = 0; j < 5; ++j) rhs[r][j] = from_lane(m[4 + r][j], base + 2), rhs[r][5 + j] = from_lane(m[4 + r][j], base + 3);
        }
        Eq3 q[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) q[i] = equation(rhs[2 * i], rhs[2 * i + 1]);
        double c[11], root[10];
        bool has[10];
        determinant10(q, c);
        ok = real_roots10(c, root, has) && ok;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            // root sub + 4 i, by selects (roots 10 and 11 do not exist)
            const double z = sub == 0 ? root[4 * i] : (sub == 1 ? root[4 * i + 1] : (sub == 2 ? root[i < 2 ? 4 * i + 2 : 0] : root[i < 2 ? 4 * i + 3 : 0]));
            const bool hz = sub == 0 ? has[4 * i] : (sub == 1 ? has[4 * i + 1] : (sub == 2 ? (i < 2 && has[i < 2 ? 4 * i + 2 : 0]) : (i < 2 && has[i < 2 ? 4 * i + 3 : 0])));
            double e[9];
            bool good = candidate5(basis, q, z, e);
            good = fundamental_of_essential(e, kk, cf[i]) && good && hz && ok;
            cok[i] = good;
#pragma unroll
            for (int k = 0; k < 9; ++k) cf[i][k] = good ? cf[i][k] : 0.f, ce[i][k] = good ? (float)e[k] : 0.f;
        }
    }
    if constexpr (GIVEN) {
        // the candidates that exist first, in ascending root: candidate s goes after those of the roots before it
        float* out = cand_out + ((size_t)p * hypotheses + hh) * (9 * kCands5);
        int pos = 0;
#pragma unroll
        for (int s = 0; s < kCands5; ++s) {
            const int there = __shfl(cok[s / 4] ? 1 : 0, base + s % 4);
            if (live && there && sub == s % 4) {
#pragma unroll
                for (int k = 0; k < 9; ++k) out[9 * pos + k] = ce[s / 4][k];
            }
            pos += there;
        }
        if (live && sub == 0) {
            for (int k = 9 * pos; k < 9 * kCands5; ++k) out[k] = 0.f;
            num_out[(size_t)p * hypotheses + hh] = pos;
        }
    } else {
        // the highest count; among equals the candidate whose canonical E has the smallest entry [0, 0]
        int bn = -1, bs = -1;
        float b00 = 0.f;
#pragma unroll
        for (int s = 0; s < kCands5; ++s) {
            const int lane = base + s % 4;
            if (!__shfl(cok[s / 4] ? 1 : 0, lane)) continue;  // (the four lanes alike)
            float f[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = __shfl(cf[s / 4][k], lane);
            const float e00 = __shfl(ce[s / 4][0], lane);
            int n = 0;
#pragma unroll 4
            for (int k = sub; k < count; k += kHypSplit) {
                const float4 q = pts[k];
                n += is_inlier(f, q.x, q.y, q.z, q.w, thr2) ? 1 : 0;
            }
#pragma unroll
            for (int d = 1; d < kHypSplit; d <<= 1) n += __shfl_xor(n, d);  // (integers: the order does not matter)
            const bool take = n > bn || (n == bn && e00 < b00);
            bn = take ? n : bn, bs = take ? s : bs, b00 = take ? e00 : b00;
        }
        if (!live || sub != (bs < 0 ? 0 : bs % 4)) return;
        const int loc = bs < 0 ? 0 : bs / 4;
        float* rec = hyp + ((size_t)p * hypotheses + h) * kPoseRecord;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            rec[k] = loc == 2 ? cf[2][k] : (loc == 1 ? cf[1][k] : cf[0][k]);
            rec[9 + k] = loc == 2 ? ce[2][k] : (loc == 1 ? ce[1][k] : ce[0][k]);
        }
        rec[18] = __int_as_float(max(bn, 0)), rec[19] = 0.f;
    }
}

// The pose of e over the correspondences with mask != 0: of the four decompositions the one with the most in front
// of both cameras, the lowest index among equals; r, t zeros and 0 where e has no decomposition. Every thread
// returns the same. buf: NT doubles.
template <int NT>
__device__ __forceinline__ int pose_of(const double e[9], const float4* pts, const uint8_t* mask, int count, const Intrinsics& kk,
                                       double* buf, int tid, double r[9], double t[3]) {
    double u[9], v[9];
    const bool ok = svd3(e, u, v);
    int best = -1;
#pragma unroll
    for (int k = 0; k < 9; ++k) r[k] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double rr[9], tt[3];
        pose_candidate(u, v, i, rr, tt);
        int mine = 0;
        for (int k = tid; k < count; k += NT) {
            if (!mask[k]) continue;
            double c[4];
            camera(pts[k], kk, c);
            mine += in_front(rr, tt, c[0], c[1], c[2], c[3]) ? 1 : 0;
        }
        const int n = (int)block_sum<NT>((double)mine, buf, tid);  // (exact: integers below 2^53)
        const bool take = ok && n > best;
        best = take ? n : best;
#pragma unroll
        for (int k = 0; k < 9; ++k) r[k] = take ? rr[k] : r[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[k] = take ? tt[k] : t[k];
    }
    return max(best, 0);
}

__global__ __launch_bounds__(kFinThreads) void essential_finalize_kernel(PairArgs a, const float* __restrict__ intr, int hypotheses,
                                                                          int refits, float thr2, const float* __restrict__ hyp,
                                                                          float* __restrict__ e_out, float* __restrict__ r_out,
                                                                          float* __restrict__ t_out, uint8_t* __restrict__ inl_out,
                                                                          int32_t* __restrict__ num_out,
                                                                          int32_t* __restrict__ front_out,
                                                                          int32_t* __restrict__ valid_out,
                                                                          int32_t* __restrict__ best_out) {
    __shared__ float4 pts[kMaxPoints];
    __shared__ uint8_t mask[kMaxPoints], trial[kMaxPoints];
    __shared__ double buf[kFinThreads];
    __shared__ int best_c[kFinThreads], best_h[kFinThreads];
    __shared__ double part[kFinThreads / 64][45];
    __shared__ double am[81], vm[81];  // the normal matrix and the eigenvectors (columns), row-major 9 x 9
    __shared__ double rot[4][2];
    __shared__ double enew[9];
    __shared__ float fnew[9];
    __shared__ int enew_ok;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int count = pair_count(a, p);
    const Intrinsics kk = load_intrinsics(intr, p);

    // the winner: the highest count, the lowest hypothesis among equals
    int bc = -1, bh = 0x7fffffff;
    for (int h = tid; h < hypotheses; h += kFinThreads) {
        const int c = __float_as_int(hyp[((size_t)p * hypotheses + h) * kPoseRecord + 18]);
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
    const bool valid = count >= kMinInliersE && intrinsics_ok(kk) && bc >= kMinInliersE;  // (the whole workgroup alike)

    double e[9], r[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = 0.0, r[k] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    int num = 0, front = 0;
    if (valid) {
        float f[9];
        const float* rec = hyp + ((size_t)p * hypotheses + bh) * kPoseRecord;
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = rec[k], e[k] = (double)rec[9 + k];
        stage_pair(a, p, count, pts, tid, kFinThreads);
        __syncthreads();
        num = mark_inliers(f, pts, count, thr2, mask, buf, tid);
        for (int round = 0; round < refits && num >= kMinInliers; ++round) {
            // normalised least squares over the inliers in camera coordinates (8-point)
            double c[4], s[2];
            hartley<kFinThreads>(pts, mask, count, (double)num, buf, tid, c, s, CameraCoord{kk});
            {
                double acc[45];
#pragma unroll
                for (int i = 0; i < 45; ++i) acc[i] = 0.0;
                for (int k = tid; k < count; k += kFinThreads) {
                    if (!mask[k]) continue;
                    double q[4];
                    camera(pts[k], kk, q);
                    normal_accumulate_f(acc, (q[0] - c[0]) * s[0], (q[1] - c[1]) * s[0], (q[2] - c[2]) * s[1], (q[3] - c[3]) * s[1]);
                }
                normal_eigenvector(acc, part, am, vm, rot, tid);
            }
            if (tid == 0) {
                int lo = 0;
                for (int k = 1; k < 9; ++k) lo = am[10 * k] < am[10 * lo] ? k : lo;
                double fn[9], ed[9];
                for (int k = 0; k < 9; ++k) fn[k] = vm[9 * k + lo];
                bool ok = denormalise64(fn, c[0], c[1], s[0], c[2], c[3], s[1], ed);
                ok = project_essential(ed) && ok;
                float fd[9];
                ok = fundamental_of_essential(ed, kk, fd) && ok;
                enew_ok = ok ? 1 : 0;
                for (int k = 0; k < 9; ++k) enew[k] = ed[k], fnew[k] = fd[k];
            }
            __syncthreads();
            if (!enew_ok) break;  // a refit that is not finite keeps the previous E and mask
#pragma unroll
            for (int k = 0; k < 9; ++k) f[k] = fnew[k];
            const int again = mark_inliers(f, pts, count, thr2, trial, buf, tid);
            if (again < num) break;  // a refit that loses inliers (a planar scene's 8-point fit) is dropped: E and mask stay
            num = again;
#pragma unroll
            for (int k = 0; k < 9; ++k) e[k] = enew[k];
            for (int k = tid; k < count; k += kFinThreads) mask[k] = trial[k];
            __syncthreads();
        }
        front = pose_of<kFinThreads>(e, pts, mask, count, kk, buf, tid, r, t);
    }
    float eo[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) eo[k] = (float)e[k];
    fix_sign(eo);
    if (tid < 9) e_out[(size_t)p * 9 + tid] = eo[tid], r_out[(size_t)p * 9 + tid] = (float)r[tid];
    if (tid < 3) t_out[(size_t)p * 3 + tid] = (float)t[tid];
    for (int k = tid; k < a.kmax; k += kFinThreads) inl_out[(size_t)p * a.kmax + k] = valid && k < count ? mask[k] : 0;
    if (tid == 0) num_out[p] = valid ? num : 0, front_out[p] = valid ? front : 0, valid_out[p] = valid ? 1 : 0, best_out[p] = valid ? bh : -1;
}

// lg_pose_from_essential: one workgroup per pair.
__global__ __launch_bounds__(kFinThreads) void essential_pose_kernel(PairArgs a, const float* __restrict__ intr,
                                                                      const float* __restrict__ e_in,
                                                                      const uint8_t* __restrict__ inl_in, float* __restrict__ r_out,
                                                                      float* __restrict__ t_out, int32_t* __restrict__ front_out) {
    __shared__ float4 pts[kMaxPoints];
    __shared__ uint8_t mask[kMaxPoints];
    __shared__ double buf[kFinThreads];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int count = pair_count(a, p);
    const Intrinsics kk = load_intrinsics(intr, p);
    double e[9], r[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = (double)e_in[(size_t)p * 9 + k], r[k] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    int front = 0;
    if (intrinsics_ok(kk)) {  // (the whole workgroup alike)
        stage_pair(a, p, count, pts, tid, kFinThreads);
        for (int k = tid; k < count; k += kFinThreads) mask[k] = inl_in[(size_t)p * a.kmax + k];
        __syncthreads();
        front = pose_of<kFinThreads>(e, pts, mask, count, kk, buf, tid, r, t);
    }
    if (tid < 9) r_out[(size_t)p * 9 + tid] = (float)r[tid];
    if (tid < 3) t_out[(size_t)p * 3 + tid] = (float)t[tid];
    if (tid == 0) front_out[p] = front;
}

size_t pose_bytes(int32_t pairs, int32_t hypotheses) { return (size_t)pairs * hypotheses * kPoseRecord * sizeof(float); }

}  // namespace

extern "C" {

size_t lg_ransac_essential_workspace(int32_t pairs, int32_t kmax, int32_t hypotheses) {
    if (pairs <= 0 || kmax <= 0 || hypotheses <= 0) return 0;
    return pose_bytes(pairs, hypotheses);
}

int32_t lg_ransac_essential(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                            const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, float threshold,
                            int32_t hypotheses, int32_t refits, int32_t seed, void* workspace, size_t workspace_bytes, float* e,
                            float* r, float* t, uint8_t* inliers, int32_t* num_inliers, int32_t* num_front, int32_t* valid,
                            int32_t* best, hipStream_t stream) {
    const char* who = "lg_ransac_essential";
    if (!pair_args_ok(matches, counts, kpts0, kpts1, pairs, kmax, k0, k1) || !intrinsics || !aligned4(intrinsics) ||
        !ransac_args_ok(threshold, hypotheses, refits, workspace, workspace_bytes, pose_bytes(pairs, hypotheses), e, inliers,
                        num_inliers, valid, best) ||
        !r || !t || !num_front || !aligned4(r) || !aligned4(t) || !aligned4(num_front))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    const float thr2 = threshold * threshold;
    hipLaunchKernelGGL(essential_hypothesis_kernel<false>, hyp_grid(hypotheses, pairs), dim3(kHypThreads), 0, stream, a, intrinsics,
                       hypotheses, (uint32_t)seed, thr2, (const int32_t*)nullptr, (float*)workspace, (float*)nullptr,
                       (int32_t*)nullptr);
    hipLaunchKernelGGL(essential_finalize_kernel, dim3(pairs), dim3(kFinThreads), 0, stream, a, intrinsics, hypotheses, refits, thr2,
                       (const float*)workspace, e, r, t, inliers, num_inliers, num_front, valid, best);
    return launched(who);
}

int32_t lg_ransac_samples5(int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream) {
    return samples_call<5>("lg_ransac_samples5", count, hypotheses, seed, samples, stream);
}

int32_t lg_ransac_solve5(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                         const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const int32_t* samples,
                         int32_t hypotheses, float* candidates, int32_t* num, hipStream_t stream) {
    const char* who = "lg_ransac_solve5";
    if (!pair_args_ok(matches, counts, kpts0, kpts1, pairs, kmax, k0, k1) || !intrinsics || !aligned4(intrinsics) ||
        !solve_args_ok(hypotheses, samples, candidates, num))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    hipLaunchKernelGGL(essential_hypothesis_kernel<true>, hyp_grid(hypotheses, pairs), dim3(kHypThreads), 0, stream, a, intrinsics,
                       hypotheses, 0u, 1.f, samples, (float*)nullptr, candidates, num);
    return launched(who);
}

int32_t lg_pose_from_essential(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                               const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* e,
                               const uint8_t* inliers, float* r, float* t, int32_t* num_front, hipStream_t stream) {
    const char* who = "lg_pose_from_essential";
    if (!pair_args_ok(matches, counts, kpts0, kpts1, pairs, kmax, k0, k1) || !intrinsics || !aligned4(intrinsics) || !e ||
        !inliers || !r || !t || !num_front || !aligned4(e) || !aligned4(r) || !aligned4(t) || !aligned4(num_front))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    hipLaunchKernelGGL(essential_pose_kernel, dim3(pairs), dim3(kFinThreads), 0, stream, a, intrinsics, e, inliers, r, t, num_front);
    return launched(who);
}

}  // extern "C"
