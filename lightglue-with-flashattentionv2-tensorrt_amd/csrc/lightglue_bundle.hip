// lightglue_bundle.hip — the bundle adjustment (include/lightglue_glue.h, "the bundle adjustment"): the poses of the views
// of a window and its landmarks refined together by Levenberg-Marquardt over Σ squared reprojection error, by the Schur
// complement on the cameras. The contract is restated in float64 in lightglue_amd/geometry_contract.py (by another
// route: scipy's sparse least squares over global rotation vectors); the arithmetic is in lightglue_bundle_math.h.
//
// bundle_adjust_kernel: one workgroup of 256 threads per window. A thread is an observation slot: thread tid is view
// tid % 8 of the landmark tid / 8 of the current tile of 32 landmarks, so a wave holds 8 landmarks and the 8 views of a
// landmark are 8 adjacent lanes. A landmark's 3 x 3 block V and its gradient are added over its 8 lanes by an xor
// butterfly (lanes_sum: every lane ends with the same bits, no LDS); each lane inverts the damped block alike, forms its own
// W_vl = J_cᵀ J_x (6 x 3) and Y_vl = W_vl V*⁻¹ and keeps its view's sums (U's upper triangle, g_c, Σ Y g_x, Σ r²) in
// registers. The poses are fp64 in LDS, the points and the trial points fp64 in the workspace; observations are read in
// place.
//
// The Schur product Σ_l Y_l W_lᵀ (48 x 48, the 41 parameters padded) by v_mfma_f64_16x16x4_f64. The lanes of wave w
// write their blocks transposed into the wave's own LDS buffers Yt, Wt [24][48] (k = 3 (landmark in the wave) + column,
// then the parameter row: the 16 lanes of an operand row read 16 consecutive doubles); an unseen view, a landmark that is
// not live and the pad rows are zeros, never branches. The k range of a tile is thus split over the four waves by
// construction: wave w multiplies its own 24 columns into the six upper-triangle 16 x 16 tiles, 36 MFMAs a tile of
// landmarks, and keeps the six accumulators in registers over the whole pass. After the pass the four waves' partial
// products go to LDS (over the operand buffers) and are added in wave order, as the views' sums are after a shuffle tree
// over the lanes of equal view: every thread reads the same bits, and the result does not depend on the schedule.
// LG_BA_FMA (make variant) replaces the MFMA by a thread per S entry over the same buffers, for the A/B.
//
// The reduced system (at most 41 rows) is factored in LDS by a column Cholesky over the threads, two barriers a column,
// and solved by substitutions a column at a time. A round is two passes over the landmarks: the build above, and the
// pass that recomputes each landmark's block, back-substitutes δx_l = -V*⁻¹ (g_l + W_lᵀ δc), writes the trial point and
// adds the trial's cost. No atomics, no allocation, no host synchronisation.
#include "lightglue_geometry_device.h"
#include "lightglue_bundle_math.h"

namespace {

constexpr int kBaThreads = 256;
constexpr int kBaTile = kBaThreads / kMaxViews;   // landmarks a tile
constexpr int kBaWaveK = 3 * kBaTile / 4;         // columns of a tile a wave owns
constexpr int kBaWaveBuf = 2 * kBaWaveK * kBaPad; // doubles a wave: Yt then Wt; as many as a 48 x 48 partial product
static_assert(kBaWaveBuf == kBaPad * kBaPad, "the partial products go over the operand buffers");

typedef double double4_t __attribute__((ext_vector_type(4)));

struct BaArgs {
    const float* obs;        // [B, V, L, 2]
    const uint8_t* seen;     // [B, V, L]
    const int32_t* counts;   // [B]
    const float* intr;       // [B, V, 4]
    const float* r;          // [B, V, 3, 3]
    const float* t;          // [B, V, 3]
    const float* points;     // [B, L, 3]
    int views, lmax, iterations;
};

struct BaShared {
    double tile[4][kBaWaveBuf];          // a wave's Yt, Wt; then its partial product
    double s[kBaPad][kBaPad];            // the reduced system, then its factor (lower)
    double part[4][kMaxViews][kBaSums];  // a wave's sums per view
    double rhs[kBaPad], y[kBaPad], delta[kBaPad], piv[kBaPad];
    double pose[2][kMaxViews][12];       // the current and the trial poses
    double cost[4];
    uint8_t fset[kMaxPoints];            // a landmark's views in the fixed set, a bit each; 0: not live
    int flag[kMaxViews];
};

__device__ __forceinline__ void load_pose(const double* p, Pose& q) {
#pragma unroll
    for (int k = 0; k < 9; ++k) q.r[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) q.t[k] = p[9 + k];
}

__device__ __forceinline__ double sum4(const double (*part)[kMaxViews][kBaSums], int v, int e) {
    return ((part[0][v][e] + part[1][v][e]) + part[2][v][e]) + part[3][v][e];
}

// What both passes derive for a thread's observation slot at the current state: the row (zeros where the slot is not in
// the fixed set), the landmark's block summed over its lanes and inverted.
struct BaSlot {
    double x[3], res[2], jc[2][6], jx[2][3], gx[3], inv[6];
    float2 px;
    bool inb, in, live, inverted;
};

template <bool FIRST>
__device__ __forceinline__ void slot_at(const BaArgs& a, int b, int count, int l, int v, const Pose& q, const Camera& cam,
                                        const double sb[2][3], double lambda, const double* pts, uint8_t* fset, BaSlot& s) {
    s.inb = l < a.lmax;
    const int lc = s.inb ? l : 0;
    const bool view = v < a.views;
    const size_t at = ((size_t)b * a.views + (view ? v : 0)) * a.lmax + lc;
    if constexpr (FIRST) {
        const float* p = a.points + ((size_t)b * a.lmax + lc) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) s.x[k] = (double)p[k];
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.x[k] = pts[3 * lc + k];
    }
    const uint8_t bits_in = FIRST ? 0 : fset[lc];
    const bool cand = s.inb && view && (FIRST ? (l < count && a.seen[at] != 0) : ((bits_in >> v) & 1) != 0);
    s.px = cand ? make_float2(a.obs[2 * at], a.obs[2 * at + 1]) : make_float2(0.f, 0.f);
    const bool ok = bundle_row(q, cam, v, sb, s.x, (double)s.px.x, (double)s.px.y, s.res, s.jc, s.jx);
    s.in = cand && ok;
    int bits = bits_in;
    if constexpr (FIRST) {
        bits = s.in ? 1 << v : 0;
#pragma unroll
        for (int d = 1; d < kMaxViews; d <<= 1) bits |= __shfl_xor(bits, d);
        bits = __popc(bits) >= 2 ? bits : 0;  // a landmark is live from two observations on
        s.in = s.in && bits != 0;
    }
    s.live = s.inb && bits != 0;
    if constexpr (FIRST) {
        if (v == 0 && s.inb) fset[l] = (uint8_t)bits;
    }
#pragma unroll
    for (int w = 0; w < 2; ++w) {  // a slot outside the set adds zeros
        s.res[w] = s.in ? s.res[w] : 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) s.jc[w][k] = s.in ? s.jc[w][k] : 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) s.jx[w][k] = s.in ? s.jx[w][k] : 0.0;
    }
    double vv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    s.gx[0] = s.gx[1] = s.gx[2] = 0.0;
    bundle_point_add(vv, s.gx, s.res, s.jx);
#pragma unroll
    for (int k = 0; k < 6; ++k) vv[k] = lanes_sum<kMaxViews>(vv[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) s.gx[k] = lanes_sum<kMaxViews>(s.gx[k]);
    s.inverted = bundle_point_inverse(vv, lambda, s.inv);
#pragma unroll
    for (int k = 0; k < 6; ++k) s.inv[k] = s.live && s.inverted ? s.inv[k] : 0.0;
}

// The build pass at pose set `cur`: the reduced system S and rhs in LDS, the views' sums in sh.part. FIRST: the fixed
// set is formed (sh.fset) and the points are copied into the workspace.
template <bool FIRST>
__device__ __forceinline__ void build_pass(const BaArgs& a, int b, int count, int cur, double scale, double lambda, double* pts,
                                           BaShared& sh, int tid) {
    const int v = tid % kMaxViews, li = tid / kMaxViews, wave = tid / 64, lane = tid % 64, lw = li % (kBaTile / 4);
    Pose q;
    load_pose(sh.pose[cur][v], q);
    const float* kp = a.intr + ((size_t)b * a.views + (v < a.views ? v : 0)) * 4;
    const Camera cam{kp[0], kp[1], kp[2], kp[3]};
    double sb[2][3];
    bundle_basis(q, scale, sb);
    double acc[kBaSums];
#pragma unroll
    for (int e = 0; e < kBaSums; ++e) acc[e] = 0.0;
    double* yt = sh.tile[wave];
    double* wt = yt + kBaWaveK * kBaPad;
    // the rows a lane writes: its view's block, view 1's five wide; view 0's lane writes the seven pad rows
    const int row0 = v == 0 ? kBaParams : bundle_row0(v), rows = v == 0 ? kBaPad - kBaParams : bundle_width(v);
#ifdef LG_BA_FMA
    double prod[kBaPad * kBaPad / kBaThreads];
#pragma unroll
    for (int m = 0; m < kBaPad * kBaPad / kBaThreads; ++m) prod[m] = 0.0;
#else
    double4_t c[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) c[m] = double4_t{0.0, 0.0, 0.0, 0.0};
#endif
    const int tiles = (a.lmax + kBaTile - 1) / kBaTile;
#pragma unroll 1
    for (int tile = 0; tile < tiles; ++tile) {
        const int l = tile * kBaTile + li;
        BaSlot s;
        slot_at<FIRST>(a, b, count, l, v, q, cam, sb, lambda, pts, sh.fset, s);
        if constexpr (FIRST) {
            if (v == 0 && s.inb) pts[3 * l] = s.x[0], pts[3 * l + 1] = s.x[1], pts[3 * l + 2] = s.x[2];
        }
        double w[6][3], y[6][3];
        bundle_w(s.jc, s.jx, s.inv, w, y);
        if (s.in) {
            bundle_view_add(acc, s.res, s.jc, y, s.gx);
            acc[kBaObs] += 1.0;
        }
        if (v == 0 && s.live && !s.inverted) acc[kBaBad] += 1.0;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            if (r >= rows) continue;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int at = (3 * lw + k) * kBaPad + row0 + r;
                yt[at] = v == 0 ? 0.0 : y[r < 6 ? r : 5][k];
                wt[at] = v == 0 ? 0.0 : w[r < 6 ? r : 5][k];
            }
        }
        __syncthreads();
#ifdef LG_BA_FMA
#pragma unroll
        for (int m = 0; m < kBaPad * kBaPad / kBaThreads; ++m) {
            const int i = (tid + m * kBaThreads) / kBaPad, j = (tid + m * kBaThreads) % kBaPad;
            if (i > j) continue;
            double p = prod[m];
            for (int ww = 0; ww < 4; ++ww)
#pragma unroll 8
                for (int k = 0; k < kBaWaveK; ++k)
                    p = fma(sh.tile[ww][k * kBaPad + i], sh.tile[ww][(kBaWaveK + k) * kBaPad + j], p);
            prod[m] = p;
        }
#else
#pragma unroll
        for (int kk = 0; kk < kBaWaveK / 4; ++kk) {
            const int at = (4 * kk + lane / 16) * kBaPad + lane % 16;
            const double a0 = yt[at], a1 = yt[at + 16], a2 = yt[at + 32];
            const double b0 = wt[at], b1 = wt[at + 16], b2 = wt[at + 32];
            c[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c[0], 0, 0, 0);
            c[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c[1], 0, 0, 0);
            c[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b2, c[2], 0, 0, 0);
            c[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c[3], 0, 0, 0);
            c[4] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b2, c[4], 0, 0, 0);
            c[5] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, c[5], 0, 0, 0);
        }
#endif
        __syncthreads();  // (the operands are read before the next tile's are written)
    }
    // the views' sums: over the lanes of equal view in a wave by a shuffle tree, then the waves in index order
#pragma unroll
    for (int e = 0; e < kBaSums; ++e) {
        double x = acc[e];
#pragma unroll
        for (int d = 32; d >= kMaxViews; d >>= 1) x += __shfl_down(x, d);
        if (lane < kMaxViews) sh.part[wave][v][e] = x;
    }
#ifdef LG_BA_FMA
#pragma unroll
    for (int m = 0; m < kBaPad * kBaPad / kBaThreads; ++m) {
        const int i = (tid + m * kBaThreads) / kBaPad, j = (tid + m * kBaThreads) % kBaPad;
        if (i <= j) sh.s[i][j] = -prod[m], sh.s[j][i] = -prod[m];
    }
    __syncthreads();
#else
    // accumulator m of tile (ti, tj): register r of lane holds row 4 r + lane / 16, column lane % 16
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        const int ti = m < 3 ? 0 : (m < 5 ? 1 : 2), tj = m < 3 ? m : (m < 5 ? m - 2 : 2);
#pragma unroll
        for (int r = 0; r < 4; ++r) yt[(16 * ti + 4 * r + lane / 16) * kBaPad + 16 * tj + lane % 16] = c[m][r];
    }
    __syncthreads();
    for (int e = tid; e < kBaPad * kBaPad; e += kBaThreads) {
        const int i = e / kBaPad, j = e % kBaPad;
        if (i > j) continue;
        const double x = -(((sh.tile[0][e] + sh.tile[1][e]) + sh.tile[2][e]) + sh.tile[3][e]);
        sh.s[i][j] = x, sh.s[j][i] = x;
    }
    __syncthreads();
#endif
    // S = U* - Σ Y Wᵀ on the views' diagonal blocks; rhs = -(g_c - Σ Y g_x)
    for (int e = tid; e < kMaxViews * 36; e += kBaThreads) {
        const int vv = e / 36, r = (e % 36) / 6, k = e % 6;
        if (vv < 1 || vv >= a.views || r >= bundle_width(vv) || k >= bundle_width(vv)) continue;
        const double u = sum4(sh.part, vv, upper6(min(r, k), max(r, k)));
        sh.s[bundle_row0(vv) + r][bundle_row0(vv) + k] += r == k ? u * (1.0 + lambda) : u;
        if (k == 0) sh.rhs[bundle_row0(vv) + r] = -(sum4(sh.part, vv, BaLm::kGrad + r) - sum4(sh.part, vv, kBaYg + r));
    }
    __syncthreads();
}

// The solve of sh.s δ = sh.rhs for the n leading rows (bundle_solve's statements over the threads): true where every
// pivot is positive and finite and δ is finite (the same in every thread).
__device__ __forceinline__ bool solve_system(BaShared& sh, int n, int tid) {
    bool ok = true;
#pragma unroll 1
    for (int c = 0; c < kBaParams; ++c) {
        if (c >= n) break;
        double x = 0.0;
        if (tid >= c && tid < n) {
            x = sh.s[tid][c];
            for (int k = 0; k < c; ++k) x = fma(-sh.s[tid][k], sh.s[c][k], x);
            if (tid == c) sh.piv[c] = x;
        }
        __syncthreads();
        const double piv = sh.piv[c];
        ok = ok && piv > 0.0 && finite64(piv);
        const double root = sqrt(piv), inv = 1.0 / root;
        if (tid >= c && tid < n) sh.s[tid][c] = tid == c ? root : x * inv;
        __syncthreads();
    }
    double x = tid < n ? sh.rhs[tid] : 0.0;
#pragma unroll 1
    for (int c = 0; c < kBaParams; ++c) {
        if (c >= n) break;
        if (tid == c) sh.y[c] = x / sh.s[c][c];
        __syncthreads();
        if (tid > c && tid < n) x = fma(-sh.s[tid][c], sh.y[c], x);
    }
    x = tid < n ? sh.y[tid] : 0.0;
#pragma unroll 1
    for (int c = kBaParams - 1; c >= 0; --c) {
        if (c >= n) continue;
        if (tid == c) sh.delta[c] = x / sh.s[c][c];
        __syncthreads();
        if (tid < c) x = fma(-sh.s[c][tid], sh.delta[c], x);
    }
    for (int c = 0; c < n; ++c) ok = ok && finite64(sh.delta[c]);
    return ok;
}

// The second pass of a round: every landmark's step from sh.delta, the trial points, and the trial's cost at the
// poses sh.pose[1 - cur] (every thread).
__device__ __forceinline__ double trial_pass(const BaArgs& a, int b, int cur, double scale, double lambda, const double* pts,
                                             double* trial, BaShared& sh, int tid) {
    const int v = tid % kMaxViews, li = tid / kMaxViews, wave = tid / 64, lane = tid % 64;
    Pose q, qn;
    load_pose(sh.pose[cur][v], q);
    load_pose(sh.pose[1 - cur][v], qn);
    const float* kp = a.intr + ((size_t)b * a.views + (v < a.views ? v : 0)) * 4;
    const Camera cam{kp[0], kp[1], kp[2], kp[3]};
    double sb[2][3], d[6];
    bundle_basis(q, scale, sb);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = v >= 1 && v < a.views && k < bundle_width(v) ? sh.delta[bundle_row0(v) + k] : 0.0;
    double cost = 0.0;
    const int tiles = (a.lmax + kBaTile - 1) / kBaTile;
#pragma unroll 1
    for (int tile = 0; tile < tiles; ++tile) {
        const int l = tile * kBaTile + li;
        BaSlot s;
        slot_at<false>(a, b, 0, l, v, q, cam, sb, lambda, pts, sh.fset, s);
        double wd[3], dx[3], xn[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // (W_vlᵀ δc_v)[k]
            double x = 0.0;
#pragma unroll
            for (int r = 0; r < 6; ++r) x = fma(s.jc[0][r] * s.jx[0][k] + s.jc[1][r] * s.jx[1][k], d[r], x);
            wd[k] = s.gx[k] + lanes_sum<kMaxViews>(x);
        }
        sym3_mul(s.inv, wd, dx);  // (zeros where the landmark is not live)
#pragma unroll
        for (int k = 0; k < 3; ++k) xn[k] = s.x[k] - dx[k];
        if (v == 0 && s.inb) trial[3 * l] = xn[0], trial[3 * l + 1] = xn[1], trial[3 * l + 2] = xn[2];
        if (s.in) {
            double res[2];
            bundle_residual(qn, cam, xn, (double)s.px.x, (double)s.px.y, res);
            cost = fma(res[0], res[0], cost);
            cost = fma(res[1], res[1], cost);
        }
    }
#pragma unroll
    for (int dd = 32; dd > 0; dd >>= 1) cost += __shfl_down(cost, dd);
    __syncthreads();  // (the last readers of sh.cost are done)
    if (lane == 0) sh.cost[wave] = cost;
    __syncthreads();
    return ((sh.cost[0] + sh.cost[1]) + sh.cost[2]) + sh.cost[3];
}

__global__ __launch_bounds__(kBaThreads) void bundle_adjust_kernel(BaArgs a, double* __restrict__ workspace,
                                                                    float* __restrict__ r_out, float* __restrict__ t_out,
                                                                    float* __restrict__ points_out, float* __restrict__ cost_out,
                                                                    int32_t* __restrict__ num_out, int32_t* __restrict__ kept_out) {
    __shared__ BaShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int count = min(max(a.counts[b], 0), a.lmax);
    double* pts = workspace + (size_t)b * a.lmax * 6;
    double* trial = pts + (size_t)a.lmax * 3;
    // (everything below that decides a branch is the same in every thread of the workgroup)
    if (tid < kMaxViews) {  // thread v enters view v: the pose, and whether the view is usable
        bool ok = true;
        float p[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
        if (tid < a.views) {
            const float* kp = a.intr + ((size_t)b * a.views + tid) * 4;
            ok = camera_ok(Camera{kp[0], kp[1], kp[2], kp[3]});
            if (tid >= 1) {
#pragma unroll
                for (int k = 0; k < 9; ++k) p[k] = a.r[((size_t)b * a.views + tid) * 9 + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) p[9 + k] = a.t[((size_t)b * a.views + tid) * 3 + k];
            }
        }
        Pose q;
        ok = absolute_enter(p, q) && ok;
        if (tid == 1) ok = ok && (p[9] != 0.f || p[10] != 0.f || p[11] != 0.f);
#pragma unroll
        for (int k = 0; k < 9; ++k) sh.pose[0][tid][k] = sh.pose[1][tid][k] = q.r[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) sh.pose[0][tid][9 + k] = sh.pose[1][tid][9 + k] = q.t[k];
        sh.flag[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    bool staged = true;
#pragma unroll
    for (int v = 0; v < kMaxViews; ++v) staged = staged && sh.flag[v] != 0;
    const double t1x = sh.pose[0][1][9], t1y = sh.pose[0][1][10], t1z = sh.pose[0][1][11];
    const double scale = sqrt(t1x * t1x + t1y * t1y + t1z * t1z);  // the gauge: |t1| as it enters
    staged = staged && finite64(scale) && scale > 0.0;

    const int n = bundle_params(a.views);
    int cur = 0, nobs = 0;
    double cost0 = 0.0, cost1 = 0.0;
    bool kept = false;
    if (staged) {
        double lambda = kLambdaStart;
        build_pass<true>(a, b, count, cur, scale, lambda, pts, sh, tid);
        double cost = 0.0, bad = 0.0;
        bool enough = true;
#pragma unroll
        for (int v = 0; v < kMaxViews; ++v) {
            const int mine = (int)sum4(sh.part, v, kBaObs);  // (exact: integers below 2^53)
            cost += sum4(sh.part, v, BaLm::kCost), nobs += mine;
            enough = enough && (v < 1 || v >= a.views || mine >= kMinViewObs);
        }
        bad = sum4(sh.part, 0, kBaBad);
        cost0 = cost1 = cost;
        if (enough && finite64(cost)) {
#pragma unroll 1
            for (int round = 0; round < a.iterations; ++round) {
                if (round > 0) {
                    build_pass<false>(a, b, count, cur, scale, lambda, pts, sh, tid);
                    bad = sum4(sh.part, 0, kBaBad);
                }
                bool take = bad == 0.0;
                if (take) take = solve_system(sh, n, tid);
                if (take) {  // (a rejected solve spares the pass)
                    if (tid >= 1 && tid < a.views) {
                        Pose q, next;
                        double d[6];
                        load_pose(sh.pose[cur][tid], q);
#pragma unroll
                        for (int k = 0; k < 6; ++k) d[k] = k < bundle_width(tid) ? sh.delta[bundle_row0(tid) + k] : 0.0;
                        bundle_update(q, tid, scale, d, next);
#pragma unroll
                        for (int k = 0; k < 9; ++k) sh.pose[1 - cur][tid][k] = next.r[k];
#pragma unroll
                        for (int k = 0; k < 3; ++k) sh.pose[1 - cur][tid][9 + k] = next.t[k];
                    }
                    __syncthreads();
                    const double again = trial_pass(a, b, cur, scale, lambda, pts, trial, sh, tid);
                    take = lm_accept(again, cost);
                    if (take) {
                        cost = again, cur = 1 - cur, kept = true;
                        double* swap = pts;
                        pts = trial, trial = swap;
                    }
                }
                lambda = lm_lambda(lambda, take);
            }
            cost1 = cost;
        }
    }
    // a refined state that is not finite in the outputs' fp32 is not kept (every thread takes the workgroup's answer)
    bool round_ok = true;
    if (kept) {
        if (tid < a.views * 12) round_ok = fabsf((float)sh.pose[cur][tid / 12][tid % 12]) < INFINITY;
        for (int e = tid; e < a.lmax * 3; e += kBaThreads) round_ok = round_ok && (sh.fset[e / 3] == 0 || fabsf((float)pts[e]) < INFINITY);
    }
    if (__syncthreads_or(round_ok ? 0 : 1)) kept = false, cost1 = cost0;
    if (tid < a.views * 12) {
        const int v = tid / 12, k = tid % 12;
        float x = k < 9 ? (k % 4 == 0 ? 1.f : 0.f) : 0.f;  // entry 0: the identity and zeros
        if (v >= 1) {
            const float given = k < 9 ? a.r[((size_t)b * a.views + v) * 9 + k] : a.t[((size_t)b * a.views + v) * 3 + (k - 9)];
            x = kept ? (float)sh.pose[cur][v][k] : given;
        }
        if (k < 9) r_out[((size_t)b * a.views + v) * 9 + k] = x;
        else t_out[((size_t)b * a.views + v) * 3 + (k - 9)] = x;
    }
    for (int e = tid; e < a.lmax * 3; e += kBaThreads) {
        const size_t at = (size_t)b * a.lmax * 3 + e;
        points_out[at] = kept && sh.fset[e / 3] != 0 ? (float)pts[e] : a.points[at];
    }
    if (tid == 0) {
        cost_out[(size_t)b * 2] = (float)cost0, cost_out[(size_t)b * 2 + 1] = (float)cost1;
        num_out[b] = nobs, kept_out[b] = kept ? 1 : 0;
    }
}

size_t ba_bytes(int32_t windows, int32_t lmax) { return (size_t)windows * lmax * 6 * sizeof(double); }

}  // namespace

extern "C" {

size_t lg_bundle_adjust_workspace(int32_t windows, int32_t views, int32_t lmax) {
    if (windows <= 0 || views < 2 || views > kMaxViews || lmax <= 0) return 0;
    return ba_bytes(windows, lmax);
}

int32_t lg_bundle_adjust(const float* obs, const uint8_t* seen, const int32_t* counts, const float* intrinsics, const float* r,
                         const float* t, const float* points, int32_t windows, int32_t views, int32_t lmax, int32_t iterations,
                         void* workspace, size_t workspace_bytes, float* r_out, float* t_out, float* points_out, float* cost,
                         int32_t* num_obs, int32_t* kept, hipStream_t stream) {
    const char* who = "lg_bundle_adjust";
    if (windows < 0 || windows > 65535 || views < 2 || views > kMaxViews || lmax < 1 || lmax > kMaxPoints || iterations < 1 ||
        iterations > kMaxBundle || !obs || !seen || !counts || !intrinsics || !r || !t || !points || !r_out || !t_out || !points_out ||
        !cost || !num_obs || !kept || !aligned4(obs) || !aligned4(counts) || !aligned4(intrinsics) ||
        !aligned4(r) || !aligned4(t) || !aligned4(points) || !aligned4(r_out) || !aligned4(t_out) || !aligned4(points_out) ||
        !aligned4(cost) || !aligned4(num_obs) || !aligned4(kept))
        return bad(who);
    if (windows == 0) return MHA_HD64_STATUS_SUCCESS;
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || workspace_bytes < ba_bytes(windows, lmax)) return bad(who);
    const BaArgs a{obs, seen, counts, intrinsics, r, t, points, views, lmax, iterations};
    hipLaunchKernelGGL(bundle_adjust_kernel, dim3(windows), dim3(kBaThreads), 0, stream, a, (double*)workspace, r_out, t_out,
                       points_out, cost, num_obs, kept);
    return launched(who);
}

}  // extern "C"
