// lightglue_window_math.h — the arithmetic of the sequence window (csrc/lightglue_window.hip;
// include/lightglue_glue.h, "the sequence window"): a posed view's ray through an observation and its part of the
// normal equations of the point closest to the rays, the 3 x 3 Cholesky solve with its smallest pivot, an observation's
// reprojection residual with its Jacobian over the point, the Gauss-Newton step and the rule for a track that is ok.
// All fp64. The style is lightglue_bundle_math.h's: plain __host__ __device__ functions on values and small fixed-size
// arrays, selection by selects, every loop with a compile-time bound. From lightglue_lm_math.h: Pose, Camera, chol3,
// finite64; from lightglue_bundle_math.h: bundle_point_add, bundle_point_inverse, sym3_mul, kMaxViews; from
// lightglue_absolute_math.h: absolute_row, absolute_enter, camera_ok.
#pragma once

#include "lightglue_bundle_math.h"

namespace lg_geom {

constexpr int kWindowGnRounds = 3;      // Gauss-Newton rounds a pass (profiles/geometry/INDEX.md has the table)
constexpr double kParallaxEps = 1e-5;   // the smallest pivot of Σ (I - d dᵀ) over the views kept below this: no point
constexpr int kWindowSums = 9;          // the normal equations' upper triangle (6) and right side (3)
constexpr int kNoLink = 0xffff;         // a 16-bit next / prev entry without a link

// A posed view's part of Σ (I - d dᵀ) X = Σ (I - d dᵀ) c: d the unit ray of the pixel in the frame's coordinates,
// Rᵀ ((px - cx) / fx, (py - cy) / fy, 1) normalised, c = -Rᵀ t the camera's centre. a[0..5]: the upper triangle
// (00 01 02 11 12 22), a[6..8]: the right side.
LG_HD void window_ray(const Pose& q, const Camera& k, double px, double py, double a[kWindowSums]) {
    const double n0 = (px - (double)k.cx) / (double)k.fx, n1 = (py - (double)k.cy) / (double)k.fy;
    const double inv = 1.0 / sqrt(n0 * n0 + n1 * n1 + 1.0);
    double d[3], c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        d[i] = (q.r[i] * n0 + q.r[3 + i] * n1 + q.r[6 + i]) * inv;
        c[i] = -(q.r[i] * q.t[0] + q.r[3 + i] * q.t[1] + q.r[6 + i] * q.t[2]);
    }
    const double dc = d[0] * c[0] + d[1] * c[1] + d[2] * c[2];
    a[0] = 1.0 - d[0] * d[0], a[1] = -d[0] * d[1], a[2] = -d[0] * d[2];
    a[3] = 1.0 - d[1] * d[1], a[4] = -d[1] * d[2], a[5] = 1.0 - d[2] * d[2];
#pragma unroll
    for (int i = 0; i < 3; ++i) a[6 + i] = c[i] - d[i] * dc;
}

// The solve of the summed system by chol3: x, and piv the smallest pivot. False where a pivot is not positive or not
// finite; x is then zeros.
LG_HD bool window_start(const double a[kWindowSums], double x[3], double& piv) {
    Chol3 c;
    const bool ok = chol3(a, c);
    const double y0 = a[6] * c.i00, y1 = fma(-c.l10, y0, a[7]) * c.i11, y2 = fma(-c.l21, y1, fma(-c.l20, y0, a[8])) * c.i22;
    x[2] = y2 * c.i22;
    x[1] = fma(-c.l21, x[2], y1) * c.i11;
    x[0] = fma(-c.l20, x[2], fma(-c.l10, x[1], y0)) * c.i00;
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = ok ? x[i] : 0.0;  // (the rounds then start from the frame's origin, as the contract's)
    piv = fmin(c.p0, fmin(c.p1, c.p2));
    return ok;
}

// An observation's residual (px) at the point x and its Jacobian over x. False where the depth is not positive or the
// residual not finite.
LG_HD bool window_row(const Pose& q, const Camera& k, const double x[3], double px, double py, double res[2], double jx[2][3]) {
    double j[2][6];
    const bool ok = absolute_row(q, k, x[0], x[1], x[2], px, py, res, j);
#pragma unroll
    for (int w = 0; w < 2; ++w)
#pragma unroll
        for (int c = 0; c < 3; ++c) jx[w][c] = j[w][3] * q.r[c] + j[w][4] * q.r[3 + c] + j[w][5] * q.r[6 + c];
    return ok;
}

// A row's part of a round's sums, s[0..5] += J_xᵀ J_x and s[6..8] += J_xᵀ r; zeros where the row is not in.
LG_HD void window_row_sums(bool in, const double res[2], const double jx[2][3], double s[kWindowSums]) {
#pragma unroll
    for (int e = 0; e < kWindowSums; ++e) s[e] = 0.0;
    bundle_point_add(s, s + 6, res, jx);
#pragma unroll
    for (int e = 0; e < kWindowSums; ++e) s[e] = in ? s[e] : 0.0;
}

// The Gauss-Newton step x <- x - (JᵀJ)⁻¹ Jᵀr from a round's summed s; x stays where JᵀJ has a pivot that is not positive
// or not finite, or the step is not finite.
LG_HD void window_step(const double s[kWindowSums], double x[3]) {
    double inv[6], dx[3];
    bool ok = bundle_point_inverse(s, 0.0, inv);
    sym3_mul(inv, s + 6, dx);
    ok = ok && finite64(dx[0]) && finite64(dx[1]) && finite64(dx[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) x[i] = ok ? x[i] - dx[i] : x[i];
}

// A check's answer for one observation: in the set, at a positive depth, with an error of at most the threshold.
LG_HD bool window_pass(bool in, bool row_ok, const double res[2], double thr2) {
    return in && row_ok && res[0] * res[0] + res[1] * res[1] <= thr2;
}

// A track is ok with at least 2 views kept that all pass, a point that is finite in fp32 and rays that are not all but
// parallel.
LG_HD bool window_ok(bool solved, int kept, bool all_pass, const double x[3], double piv) {
    return solved && kept >= 2 && all_pass && fabsf((float)x[0]) < INFINITY && fabsf((float)x[1]) < INFINITY &&
           fabsf((float)x[2]) < INFINITY && piv >= kParallaxEps * (double)kept;
}

}  // namespace lg_geom
