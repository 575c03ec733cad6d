// lightglue_polish.hip — the pose polish and the triangulation (include/lightglue_glue.h, "the pose polish"): what a
// caller does with lg_ransac_essential's (R, t) next. lg_pose_polish minimises the squared Sampson distance in pixels
// over the pose's inliers by Levenberg-Marquardt on the 5 parameters of (R, t), recomputes the mask and keeps the
// result where it loses no inlier; lg_triangulate writes the 3D point of every inlier. The contract is restated in
// float64 in lightglue_amd/geometry_contract.py (by another route: scipy's least squares in another parameterisation); the
// arithmetic is in lightglue_polish_math.h.
//
// pose_polish_kernel: one workgroup of kFinThreads per pair, the shape of essential_finalize_kernel. The pair's
// correspondences go to LDS once. A pass over the rows is one loop: every thread walks its rows of the fixed set,
// evaluates residual and Jacobian row at the same state and adds to the 22 sums (JᵀJ's upper triangle, Jᵀs, Σ s², the
// number of rows) in registers; the sums are added over each wave's lanes by a shuffle tree and over the four waves in
// index order from LDS, so every thread reads the same bits. Every thread then solves the 5 x 5 system alike (no
// barrier, no broadcast; the solve's registers are dead before the next pass, whose row loop is what fills the register
// file), builds the same trial pose, and the pass at the trial pose gives both the trial's cost and, where it is
// accepted, the next round's sums: one pass a round. triangulate_kernel: a flat grid over (rows, pairs), a thread a correspondence.
// No atomics, no workspace, no host synchronisation.
#include "lightglue_essential_device.h"
#include "lightglue_polish_math.h"

namespace {

// One pass over the pair's rows at the pose q: the kPolishSums sums over the rows k with (FIRST ? mask[k] and a finite
// residual, which also defines fixed[k] : fixed[k]), the same bits in every thread. A thread reads only the fixed[]
// entries it wrote. part: [kFinThreads / 64][kPolishSums] in LDS.
template <bool FIRST>
__device__ __forceinline__ void polish_pass(const PolishPose& q, const PolishWeights& pw, const Intrinsics& kk, const float4* pts,
                                            const uint8_t* mask, uint8_t* fixed, int count, double (*part)[kPolishSums], int tid,
                                            double sums[kPolishSums]) {
    double acc[kPolishSums];
    PolishState st;
    polish_derive(q, st);
#pragma unroll
    for (int e = 0; e < kPolishSums; ++e) acc[e] = 0.0;
    for (int k = tid; k < count; k += kFinThreads) {
        if (!(FIRST ? mask[k] : fixed[k])) continue;
        double c[4], j[5];
        camera(pts[k], kk, c);
        const double s = sampson_row(st, pw, c[0], c[1], c[2], c[3], j);
        if constexpr (FIRST) {
            const bool fin = finite64(s);
            fixed[k] = fin ? 1 : 0;
            if (!fin) continue;
        }
        polish_accumulate(acc, s, j);
    }
    __syncthreads();  // (the last pass's readers of part are done)
#pragma unroll
    for (int e = 0; e < kPolishSums; ++e) {
        double v = acc[e];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
        if (tid % 64 == 0) part[tid / 64][e] = v;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kPolishSums; ++e) sums[e] = ((part[0][e] + part[1][e]) + part[2][e]) + part[3][e];
}

// The inliers of `mask` that triangulate in front of both cameras under (r, t) (every thread).
__device__ __forceinline__ int count_front(const double r[9], const double t[3], const float4* pts, const uint8_t* mask, int count,
                                           const Intrinsics& kk, double* buf, int tid) {
    int mine = 0;
    for (int k = tid; k < count; k += kFinThreads) {
        if (!mask[k]) continue;
        double c[4];
        camera(pts[k], kk, c);
        mine += in_front(r, t, c[0], c[1], c[2], c[3]) ? 1 : 0;
    }
    return (int)block_sum<kFinThreads>((double)mine, buf, tid);  // (exact: integers below 2^53)
}

__global__ __launch_bounds__(kFinThreads) void pose_polish_kernel(PairArgs a, const float* __restrict__ intr,
                                                                   const float* __restrict__ r_in, const float* __restrict__ t_in,
                                                                   const uint8_t* __restrict__ inl_in,
                                                                   const int32_t* __restrict__ valid_in, float thr2, int iterations,
                                                                   float* __restrict__ e_out, float* __restrict__ r_out,
                                                                   float* __restrict__ t_out, uint8_t* __restrict__ inl_out,
                                                                   int32_t* __restrict__ num_out, int32_t* __restrict__ front_out,
                                                                   float* __restrict__ cost_out, int32_t* __restrict__ kept_out) {
    __shared__ float4 pts[kMaxPoints];
    __shared__ uint8_t mask[kMaxPoints], fixed[kMaxPoints], trial[kMaxPoints];
    __shared__ double buf[kFinThreads];
    __shared__ double part[kFinThreads / 64][kPolishSums];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int count = pair_count(a, p);
    const Intrinsics kk = load_intrinsics(intr, p);
    // (everything below that decides a branch is the same in every thread of the workgroup)
    const bool valid = valid_in[p] != 0;
    const bool staged = valid && intrinsics_ok(kk);
    float rg[9], tg[3];  // the pose as given
#pragma unroll
    for (int k = 0; k < 9; ++k) rg[k] = r_in[(size_t)p * 9 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tg[k] = t_in[(size_t)p * 3 + k];
    PolishPose st;
    const bool pose_ok = polish_enter(rg, tg, st);
    const PolishWeights pw = polish_weights(kk);

    int n_in = 0, n_new = 0, front = 0;
    double cost0 = 0.0, cost1 = 0.0;
    bool kept = false;
    float eo[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) eo[k] = 0.f;
    if (valid) {
        if (staged) stage_pair(a, p, count, pts, tid, kFinThreads);
        int mine = 0;
        for (int k = tid; k < count; k += kFinThreads) {
            const uint8_t m = inl_in[(size_t)p * a.kmax + k] ? 1 : 0;
            mask[k] = m, fixed[k] = 0;
            mine += m;
        }
        n_in = (int)block_sum<kFinThreads>((double)mine, buf, tid);  // (exact; its barriers publish pts and mask)
    }
    if (staged) {
        if (pose_ok) {
            double sums[kPolishSums];
            polish_pass<true>(st, pw, kk, pts, mask, fixed, count, part, tid, sums);
            cost0 = cost1 = sums[20];
            if ((int)sums[21] >= kMinPolishRows && finite64(cost0)) {
                double lambda = kLambdaStart;
#pragma unroll 1
                for (int round = 0; round < iterations; ++round) {
                    double delta[5];
                    bool take = polish_step(sums, lambda, delta);
                    if (take) {  // (a rejected solve spares the pass)
                        PolishPose next;
                        double again[kPolishSums];
                        polish_update(st, delta, next);
                        polish_pass<false>(next, pw, kk, pts, mask, fixed, count, part, tid, again);
                        take = finite64(again[20]) && again[20] < sums[20];
                        if (take) {
                            st = next;
#pragma unroll
                            for (int e = 0; e < kPolishSums; ++e) sums[e] = again[e];
                        }
                    }
                    lambda = take ? fmax(lambda * 0.1, kLambdaMin) : fmin(lambda * 10.0, kLambdaMax);
                }
                cost1 = sums[20];
                // the mask of the polished pose over all the pair's correspondences, and the keep rule
                double e[9];
                float f[9];
                cross_mul(st.t, st.r, e);
                bool ok = canonical9(e);
                ok = fundamental_of_essential(e, kk, f) && ok;
#pragma unroll
                for (int k = 0; k < 9; ++k) f[k] = ok ? f[k] : 0.f;  // (zeros count nothing)
                n_new = mark_inliers(f, pts, count, thr2, trial, buf, tid);
                kept = ok && n_new >= n_in;
                if (kept) {
#pragma unroll
                    for (int k = 0; k < 9; ++k) eo[k] = (float)e[k];
                }
            }
        }
        if (kept) {
            front = count_front(st.r, st.t, pts, trial, count, kk, buf, tid);
        } else {
            double rd[9], td[3];
#pragma unroll
            for (int k = 0; k < 9; ++k) rd[k] = (double)rg[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) td[k] = (double)tg[k];
            front = count_front(rd, td, pts, mask, count, kk, buf, tid);
        }
    }
    if (!kept) {
        cost1 = cost0;
        if (valid) {  // E of the pose as given
            double rd[9], td[3], e[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) rd[k] = (double)rg[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) td[k] = (double)tg[k];
            cross_mul(td, rd, e);
            canonical9(e);  // (zeros where zero or not finite)
#pragma unroll
            for (int k = 0; k < 9; ++k) eo[k] = (float)e[k];
        }
    }
    fix_sign(eo);
#pragma unroll
    for (int k = 0; k < 9; ++k) {  // (thread k writes entry k: no array is indexed by the thread)
        if (tid == k) e_out[(size_t)p * 9 + k] = eo[k], r_out[(size_t)p * 9 + k] = kept ? (float)st.r[k] : rg[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (tid == k) t_out[(size_t)p * 3 + k] = kept ? (float)st.t[k] : tg[k];
    }
    for (int k = tid; k < a.kmax; k += kFinThreads) {
        uint8_t m = 0;
        if (k < count) m = kept ? trial[k] : (valid ? mask[k] : (inl_in[(size_t)p * a.kmax + k] ? 1 : 0));
        inl_out[(size_t)p * a.kmax + k] = m;
    }
    if (tid == 0) {
        num_out[p] = kept ? n_new : n_in, front_out[p] = front, kept_out[p] = kept ? 1 : 0;
        cost_out[(size_t)p * 2] = (float)cost0, cost_out[(size_t)p * 2 + 1] = (float)cost1;
    }
}

__global__ __launch_bounds__(kFinThreads) void triangulate_kernel(PairArgs a, const float* __restrict__ intr,
                                                                   const float* __restrict__ r_in, const float* __restrict__ t_in,
                                                                   const uint8_t* __restrict__ inl_in, float* __restrict__ points,
                                                                   uint8_t* __restrict__ ok_out) {
    const int p = blockIdx.y, k = blockIdx.x * kFinThreads + threadIdx.x;
    if (k >= a.kmax) return;
    const size_t row = (size_t)p * a.kmax + k;
    double x[3] = {0.0, 0.0, 0.0};
    bool ok = false;
    const Intrinsics kk = load_intrinsics(intr, p);
    if (k < pair_count(a, p) && inl_in[row] && intrinsics_ok(kk)) {
        const int i0 = min(max(a.matches[2 * row], 0), a.k0 - 1), i1 = min(max(a.matches[2 * row + 1], 0), a.k1 - 1);
        const float2 u = *reinterpret_cast<const float2*>(a.kpts0 + ((size_t)p * a.k0 + i0) * 2);
        const float2 v = *reinterpret_cast<const float2*>(a.kpts1 + ((size_t)p * a.k1 + i1) * 2);
        double c[4], r[9], t[3];
        camera(make_float4(u.x, u.y, v.x, v.y), kk, c);
#pragma unroll
        for (int i = 0; i < 9; ++i) r[i] = (double)r_in[(size_t)p * 9 + i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = (double)t_in[(size_t)p * 3 + i];
        ok = midpoint(r, t, c[0], c[1], c[2], c[3], x);
        const float fx = (float)x[0], fy = (float)x[1], fz = (float)x[2];
        ok = ok && fabsf(fx) < INFINITY && fabsf(fy) < INFINITY && fabsf(fz) < INFINITY;  // (finite in the output's fp32)
    }
    points[3 * row] = ok ? (float)x[0] : 0.f, points[3 * row + 1] = ok ? (float)x[1] : 0.f, points[3 * row + 2] = ok ? (float)x[2] : 0.f;
    ok_out[row] = ok ? 1 : 0;
}

bool calibrated_args_ok(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                        const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* r, const float* t,
                        const uint8_t* inliers) {
    return pair_args_ok(matches, counts, kpts0, kpts1, pairs, kmax, k0, k1) && intrinsics && aligned4(intrinsics) && r && t &&
           inliers && aligned4(r) && aligned4(t);
}

}  // namespace

extern "C" {

int32_t lg_pose_polish(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                       const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* r, const float* t,
                       const uint8_t* inliers, const int32_t* valid, float threshold, int32_t iterations, float* e_out, float* r_out,
                       float* t_out, uint8_t* inliers_out, int32_t* num_inliers, int32_t* num_front, float* cost, int32_t* kept,
                       hipStream_t stream) {
    const char* who = "lg_pose_polish";
    if (!calibrated_args_ok(matches, counts, kpts0, kpts1, intrinsics, pairs, kmax, k0, k1, r, t, inliers) || !valid ||
        !aligned4(valid) || !threshold_ok(threshold) || iterations < 1 || iterations > kMaxPolish || !e_out || !r_out || !t_out ||
        !inliers_out || !num_inliers || !num_front || !cost || !kept || !aligned4(e_out) || !aligned4(r_out) || !aligned4(t_out) ||
        !aligned4(num_inliers) || !aligned4(num_front) || !aligned4(cost) || !aligned4(kept))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    hipLaunchKernelGGL(pose_polish_kernel, dim3(pairs), dim3(kFinThreads), 0, stream, a, intrinsics, r, t, inliers, valid,
                       threshold * threshold, iterations, e_out, r_out, t_out, inliers_out, num_inliers, num_front, cost, kept);
    return launched(who);
}

int32_t lg_triangulate(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1,
                       const float* intrinsics, int32_t pairs, int32_t kmax, int32_t k0, int32_t k1, const float* r, const float* t,
                       const uint8_t* inliers, float* points, uint8_t* ok, hipStream_t stream) {
    const char* who = "lg_triangulate";
    if (!calibrated_args_ok(matches, counts, kpts0, kpts1, intrinsics, pairs, kmax, k0, k1, r, t, inliers) || !points || !ok ||
        !aligned4(points))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const PairArgs a{matches, counts, kpts0, kpts1, kmax, k0, k1};
    hipLaunchKernelGGL(triangulate_kernel, dim3((kmax + kFinThreads - 1) / kFinThreads, pairs), dim3(kFinThreads), 0, stream, a,
                       intrinsics, r, t, inliers, points, ok);
    return launched(who);
}

}  // extern "C"
