// lightglue_bundle_math.h — the arithmetic of the bundle adjustment (csrc/lightglue_bundle.hip;
// include/lightglue_glue.h, "the bundle adjustment"): an observation's reprojection residual in pixels with its
// analytic Jacobians over the view's parameters and over the landmark, the damped 3 x 3 landmark block and its inverse,
// the parameter layout of a window, the views' updates and the Cholesky solve of the reduced camera system. All fp64.
// The style is lightglue_absolute_math.h's: plain __host__ __device__ functions on values and small fixed-size arrays,
// selection by selects, every loop with a compile-time bound. From lightglue_lm_math.h: Pose, Camera, rodrigues_update,
// LmSums<6> with lm_accumulate, chol3, lm_accept and lm_lambda (the rounds' rules), finite64; from
// lightglue_polish_math.h: tangent_basis, tangent_move (view 1's step in t's tangent plane); from
// lightglue_absolute_math.h: absolute_row (the residual and the Jacobian over (ω, δt)), absolute_enter, absolute_round,
// camera_ok.
//
// The parameters of a window of V views: view 0 has none; view 1 has 5, (ω, τ1, τ2), at columns 0..4: its t keeps the
// entering length s (the gauge), t = s u with u moving in its tangent plane, ∂t/∂τ_j = s b_j; view v >= 2 has 6,
// (ω, δt), at columns 5 + 6 (v - 2) ..; 6 V - 7 in all, 41 at V = 8. A view's block is carried 6 wide everywhere:
// view 1's sixth column is zeros and is never written into the system.
#pragma once

#include "lightglue_polish_math.h"
#include "lightglue_absolute_math.h"

namespace lg_geom {

constexpr int kMaxViews = 8;           // views a window at most
constexpr int kMaxBundle = 32;         // rounds at most
constexpr int kMinViewObs = 4;         // a view from 1 on needs as many observations of live landmarks
constexpr int kBaParams = 41;          // 6 * kMaxViews - 7
constexpr int kBaPad = 48;             // the parameters padded to three 16-row tiles
// A view's sums: U's upper triangle (21), g_c (6) and Σ r² as LmSums<6> lays them out, then Σ Y g_x (6), its observations
// in the fixed set, and (view 0's) the landmark blocks that did not invert.
using BaLm = LmSums<6>;
constexpr int kBaYg = BaLm::kCost + 1, kBaObs = kBaYg + 6, kBaBad = kBaObs + 1, kBaSums = kBaBad + 1;

LG_HD int bundle_params(int views) { return 6 * views - 7; }
LG_HD int bundle_row0(int v) { return v <= 1 ? 0 : 5 + 6 * (v - 2); }   // the first column of view v's block
LG_HD int bundle_width(int v) { return v == 0 ? 0 : (v == 1 ? 5 : 6); }

// view 1's ∂t/∂τ: sb[j] = scale b_j for the tangent basis (b1, b2) of t / scale (a pass derives it from the pose once).
LG_HD void bundle_basis(const Pose& q, double scale, double sb[2][3]) {
    double u[3], b[2][3];
    const double inv = 1.0 / scale;
#pragma unroll
    for (int i = 0; i < 3; ++i) u[i] = q.t[i] * inv;
    tangent_basis(u, b);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) sb[j][i] = scale * b[j][i];
}

// An observation's row: res [2] (px), jc [2][6] over the view's block (zeros for view 0), jx [2][3] over the landmark.
// sb: bundle_basis' (read for view 1 only). False where the depth is not positive or the residual not finite.
LG_HD bool bundle_row(const Pose& q, const Camera& k, int v, const double sb[2][3], const double x[3], double px, double py,
                      double res[2], double jc[2][6], double jx[2][3]) {
    double j[2][6];
    const bool ok = absolute_row(q, k, x[0], x[1], x[2], px, py, res, j);
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        const double* a = &j[w][3];  // ∂res_w / ∂X_c
        const double t1 = a[0] * sb[0][0] + a[1] * sb[0][1] + a[2] * sb[0][2];
        const double t2 = a[0] * sb[1][0] + a[1] * sb[1][1] + a[2] * sb[1][2];
#pragma unroll
        for (int i = 0; i < 3; ++i) jc[w][i] = v == 0 ? 0.0 : j[w][i];
        jc[w][3] = v == 0 ? 0.0 : (v == 1 ? t1 : a[0]);
        jc[w][4] = v == 0 ? 0.0 : (v == 1 ? t2 : a[1]);
        jc[w][5] = v <= 1 ? 0.0 : a[2];
#pragma unroll
        for (int c = 0; c < 3; ++c) jx[w][c] = a[0] * q.r[c] + a[1] * q.r[3 + c] + a[2] * q.r[6 + c];
    }
    return ok;
}

// The residual alone (the trial's cost). False as bundle_row.
LG_HD bool bundle_residual(const Pose& q, const Camera& k, const double x[3], double px, double py, double res[2]) {
    const double xc = q.r[0] * x[0] + q.r[1] * x[1] + q.r[2] * x[2] + q.t[0];
    const double yc = q.r[3] * x[0] + q.r[4] * x[1] + q.r[5] * x[2] + q.t[1];
    const double zc = q.r[6] * x[0] + q.r[7] * x[1] + q.r[8] * x[2] + q.t[2];
    const double iz = 1.0 / zc;
    res[0] = (double)k.fx * xc * iz + ((double)k.cx - px), res[1] = (double)k.fy * yc * iz + ((double)k.cy - py);
    return zc > 0.0 && finite64(res[0]) && finite64(res[1]);
}

// An observation's part of its landmark's block: vv += J_xᵀ J_x (upper triangle: 00 01 02 11 12 22), gx += J_xᵀ r.
LG_HD void bundle_point_add(double vv[6], double gx[3], const double res[2], const double jx[2][3]) {
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        int e = 0;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int c = a; c < 3; ++c) vv[e] = fma(jx[w][a], jx[w][c], vv[e]), ++e;
            gx[a] = fma(jx[w][a], res[w], gx[a]);
        }
    }
}

// The inverse (upper triangle) of V* = V + λ diag V by chol3. False where a pivot is not positive or not finite.
LG_HD bool bundle_point_inverse(const double vv[6], double lambda, double inv[6]) {
    const double d = 1.0 + lambda;
    const double a[6] = {vv[0] * d, vv[1], vv[2], vv[3] * d, vv[4], vv[5] * d};
    Chol3 c;
    const bool ok = chol3(a, c);
    const double i00 = c.i00, i11 = c.i11, i22 = c.i22;
    // M = L⁻¹ (lower), V*⁻¹ = Mᵀ M
    const double m10 = -c.l10 * i00 * i11, m21 = -c.l21 * i11 * i22, m20 = -(c.l20 * i00 + c.l21 * m10) * i22;
    inv[0] = i00 * i00 + m10 * m10 + m20 * m20, inv[1] = m10 * i11 + m20 * m21, inv[2] = m20 * i22;
    inv[3] = i11 * i11 + m21 * m21, inv[4] = m21 * i22, inv[5] = i22 * i22;
    return ok;
}

// out = the symmetric 3 x 3 matrix m (upper triangle) times x.
LG_HD void sym3_mul(const double m[6], const double x[3], double out[3]) {
    out[0] = m[0] * x[0] + m[1] * x[1] + m[2] * x[2];
    out[1] = m[1] * x[0] + m[3] * x[1] + m[4] * x[2];
    out[2] = m[2] * x[0] + m[4] * x[1] + m[5] * x[2];
}

// W = J_cᵀ J_x (6 x 3) of an observation and Y = W V*⁻¹.
LG_HD void bundle_w(const double jc[2][6], const double jx[2][3], const double inv[6], double w[6][3], double y[6][3]) {
#pragma unroll
    for (int a = 0; a < 6; ++a) {
#pragma unroll
        for (int c = 0; c < 3; ++c) w[a][c] = jc[0][a] * jx[0][c] + jc[1][a] * jx[1][c];
        sym3_mul(inv, w[a], y[a]);
    }
}

// acc += the observation's part of its view's sums: its two residuals in turn (U, g_c = J_cᵀ r, Σ r²), then Σ Y g_x
// (gx: the landmark's whole J_xᵀ r).
LG_HD void bundle_view_add(double acc[kBaSums], const double res[2], const double jc[2][6], const double y[6][3], const double gx[3]) {
    lm_accumulate<6>(acc, res[0], jc[0]);
    lm_accumulate<6>(acc, res[1], jc[1]);
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[kBaYg + a] += y[a][0] * gx[0] + y[a][1] * gx[1] + y[a][2] * gx[2];
}

LG_HD int upper6(int a, int c) { return a * 6 - a * (a - 1) / 2 + (c - a); }  // (a <= c) in a 6 x 6 upper triangle by rows

// The trial pose of view v >= 1 from its block d [6] of the step: R by rodrigues_update; view 1's t by tangent_move on
// t / scale, then at the entering length again; the others' t + δt.
LG_HD void bundle_update(const Pose& s, int v, double scale, const double d[6], Pose& out) {
    const double inv = 1.0 / scale;
    const double u[3] = {s.t[0] * inv, s.t[1] * inv, s.t[2] * inv};
    double un[3];
    rodrigues_update(s.r, d, out.r);
    tangent_move(u, d[3], d[4], un);
#pragma unroll
    for (int k = 0; k < 3; ++k) out.t[k] = v == 1 ? un[k] * scale : s.t[k] + d[3 + k];
}

// The solve of the reduced camera system S δ = rhs for the n <= kBaParams leading rows, serially (the host's route; the
// kernel runs the same factorisation column by column over its threads): s [kBaPad][kBaPad] is overwritten by its
// Cholesky factor (lower). False where a pivot is not positive or not finite, or δ is not finite.
LG_HD bool bundle_solve(double (*s)[kBaPad], const double* rhs, int n, double* delta) {
    bool ok = true;
    for (int c = 0; c < kBaParams; ++c) {
        if (c >= n) break;
        double piv = s[c][c];
        for (int k = 0; k < c; ++k) piv = fma(-s[c][k], s[c][k], piv);
        ok = ok && piv > 0.0 && finite64(piv);
        const double root = sqrt(piv), inv = 1.0 / root;
        s[c][c] = root;
        for (int r = c + 1; r < n; ++r) {
            double v = s[r][c];
            for (int k = 0; k < c; ++k) v = fma(-s[r][k], s[c][k], v);
            s[r][c] = v * inv;
        }
    }
    double y[kBaParams];
    for (int r = 0; r < kBaParams; ++r) {
        if (r >= n) break;
        double v = rhs[r];
        for (int k = 0; k < r; ++k) v = fma(-s[r][k], y[k], v);
        y[r] = v / s[r][r];
    }
    for (int r = kBaParams - 1; r >= 0; --r) {
        if (r >= n) continue;
        double v = y[r];
        for (int k = n - 1; k > r; --k) v = fma(-s[k][r], delta[k], v);  // (the kernel's order: a column at a time from the last)
        delta[r] = v / s[r][r];
        ok = ok && finite64(delta[r]);
    }
    return ok;
}

}  // namespace lg_geom
