// lightglue_polish_math.h — the arithmetic of the pose polish and of the triangulation (csrc/lightglue_polish.hip;
// include/lightglue_glue.h, "the pose polish"): the signed Sampson residual of a correspondence in pixels with its
// analytic Jacobian row over the 5 parameters (ω, τ), the state (R, t) with the derivative matrices of E = [t]x R, the
// Levenberg-Marquardt step by a 5 x 5 Cholesky, the update by the exact Rodrigues formula, and the midpoint
// triangulation. All fp64. The style is lightglue_essential_math.h's: plain __host__ __device__ functions on values
// and small fixed-size arrays, every index a compile-time constant after unrolling, selection by selects, every loop
// with a compile-time bound.
#pragma once

#include "lightglue_essential_math.h"

namespace lg_geom {

constexpr int kMaxPolish = 16;         // rounds at most
constexpr int kMinPolishRows = 5;      // the fixed set needs as many rows as there are parameters
constexpr int kPolishSums = 22;        // JᵀJ's upper triangle (15), Jᵀs (5), Σ s² and the number of rows
constexpr double kLambdaStart = 1e-3, kLambdaMin = 1e-12, kLambdaMax = 1e12;

LG_HD bool finite64(double v) { return fabs(v) < INFINITY; }  // (NaN: false)

// out = [v]x m (row-major 3 x 3): column c of out is v x (column c of m).
LG_HD void cross_mul(const double v[3], const double m[9], double out[9]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[c] = v[1] * m[6 + c] - v[2] * m[3 + c];
        out[3 + c] = v[2] * m[c] - v[0] * m[6 + c];
        out[6 + c] = v[0] * m[3 + c] - v[1] * m[c];
    }
}

// The pose being polished: R, t at unit length.
struct PolishPose {
    double r[9], t[3];
};

// What a pass over the rows derives from the pose once: E = [t]x R and the five derivative matrices
// ∂E/∂ω_i = [t]x [e_i]x R, ∂E/∂τ_j = [b_j]x R for the tangent basis (b1, b2) of t. (Not kept between the passes: the
// 108 registers are the row loop's alone.)
struct PolishState {
    double e[9], de[5][9];
};

// (b1, b2): an orthonormal basis of t's tangent plane from the unit axis of t's smallest component in magnitude
// (the lowest index among equals): b1 = normalise(t x axis), b2 = t x b1.
LG_HD void tangent_basis(const double t[3], double b[2][3]) {
    const double a0 = fabs(t[0]), a1 = fabs(t[1]), a2 = fabs(t[2]);
    const int ax = a1 < a0 ? (a2 < a1 ? 2 : 1) : (a2 < a0 ? 2 : 0);
    const double ex = ax == 0 ? 1.0 : 0.0, ey = ax == 1 ? 1.0 : 0.0, ez = ax == 2 ? 1.0 : 0.0;
    const double c0 = t[1] * ez - t[2] * ey, c1 = t[2] * ex - t[0] * ez, c2 = t[0] * ey - t[1] * ex;
    const double inv = 1.0 / sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    b[0][0] = c0 * inv, b[0][1] = c1 * inv, b[0][2] = c2 * inv;
    b[1][0] = t[1] * b[0][2] - t[2] * b[0][1], b[1][1] = t[2] * b[0][0] - t[0] * b[0][2], b[1][2] = t[0] * b[0][1] - t[1] * b[0][0];
}

// E and the derivative matrices of the pose.
LG_HD void polish_derive(const PolishPose& q, PolishState& s) {
    double b[2][3];
    cross_mul(q.t, q.r, s.e);
    tangent_basis(q.t, b);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double ax[3] = {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0};
        double g[9];
        cross_mul(ax, q.r, g);
        cross_mul(q.t, g, s.de[i]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) cross_mul(b[j], q.r, s.de[3 + j]);
}

// The entering pose from one given in fp32: t at unit length, R one Newton step of the polar iteration nearer the
// rotations (R (3 I - Rᵀ R) / 2: the defect of a rotation rounded to fp32 falls from 1e-7 to 1e-14). False where R or
// t is not finite or t has zero length (the pose is then not to be used).
LG_HD bool polish_enter(const float r[9], const float t[3], PolishPose& s) {
    bool ok = true;
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = (double)r[k], ok = ok && finite64(m[k]);
    const double tx = (double)t[0], ty = (double)t[1], tz = (double)t[2];
    const double len = sqrt(tx * tx + ty * ty + tz * tz);
    ok = ok && finite64(len) && len > 0.0;
    const double inv = 1.0 / len;
    s.t[0] = tx * inv, s.t[1] = ty * inv, s.t[2] = tz * inv;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;  // (R (3 I - Rᵀ R))[i][j]
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double g = m[k] * m[j] + m[3 + k] * m[3 + j] + m[6 + k] * m[6 + j];  // (Rᵀ R)[k][j]
                v += m[3 * i + k] * ((k == j ? 3.0 : 0.0) - g);
            }
            s.r[3 * i + j] = 0.5 * v;
        }
    return ok;
}

struct PolishWeights {  // 1 / fx1², 1 / fy1², 1 / fx0², 1 / fy0²
    double w[4];
};

LG_HD PolishWeights polish_weights(const Intrinsics& k) {
    return PolishWeights{{1.0 / (k.fx1 * k.fx1), 1.0 / (k.fy1 * k.fy1), 1.0 / (k.fx0 * k.fx0), 1.0 / (k.fy0 * k.fy0)}};
}

// The signed Sampson distance in pixels of the correspondence (x0, y0, x1, y1) (camera coordinates) under the
// state's E, and its Jacobian row: with (a, b, c) = E q0, (a', b', .) = Eᵀ q1, d = q1 . (a, b, c) and
// n² = (a / fx1)² + (b / fy1)² + (a' / fx0)² + (b' / fy0)², s = d / n and ∂s = (∂d - s (∂n² / 2) / n) / n.
LG_HD double sampson_row(const PolishState& st, const PolishWeights& pw, double x0, double y0, double x1, double y1, double j[5]) {
    const double* e = st.e;
    const double a = e[0] * x0 + e[1] * y0 + e[2], b = e[3] * x0 + e[4] * y0 + e[5], c = e[6] * x0 + e[7] * y0 + e[8];
    const double ap = e[0] * x1 + e[3] * y1 + e[6], bp = e[1] * x1 + e[4] * y1 + e[7];
    const double d = x1 * a + y1 * b + c;
    const double n2 = a * a * pw.w[0] + b * b * pw.w[1] + ap * ap * pw.w[2] + bp * bp * pw.w[3];
    const double inv = 1.0 / sqrt(n2);
    const double s = d * inv;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const double* g = st.de[i];
        const double da = g[0] * x0 + g[1] * y0 + g[2], db = g[3] * x0 + g[4] * y0 + g[5], dc = g[6] * x0 + g[7] * y0 + g[8];
        const double dap = g[0] * x1 + g[3] * y1 + g[6], dbp = g[1] * x1 + g[4] * y1 + g[7];
        const double dd = x1 * da + y1 * db + dc;
        const double half = a * da * pw.w[0] + b * db * pw.w[1] + ap * dap * pw.w[2] + bp * dbp * pw.w[3];
        j[i] = (dd - s * half * inv) * inv;
    }
    return s;
}

// acc += the row's part of the kPolishSums sums: JᵀJ's upper triangle row by row, Jᵀs, s² and 1.
LG_HD void polish_accumulate(double acc[kPolishSums], double s, const double j[5]) {
    int e = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = a; b < 5; ++b) acc[e] = fma(j[a], j[b], acc[e]), ++e;
#pragma unroll
    for (int a = 0; a < 5; ++a) acc[15 + a] = fma(j[a], s, acc[15 + a]);
    acc[20] = fma(s, s, acc[20]);
    acc[21] += 1.0;
}

// The Levenberg-Marquardt step of the sums: (JᵀJ + λ diag(JᵀJ)) δ = -Jᵀs by a Cholesky factorisation. False where
// a pivot is not positive or not finite (δ is then not to be used).
LG_HD bool polish_step(const double sums[kPolishSums], double lambda, double delta[5]) {
    double l[5][5];
    int e = 0;
#pragma unroll
    for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = a; b < 5; ++b) l[b][a] = sums[e] * (a == b ? 1.0 + lambda : 1.0), ++e;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        double piv = l[c][c];
#pragma unroll
        for (int k = 0; k < c; ++k) piv = fma(-l[c][k], l[c][k], piv);
        ok = ok && piv > 0.0 && finite64(piv);  // (NaN: false)
        const double root = sqrt(piv), inv = 1.0 / root;
        l[c][c] = root;
#pragma unroll
        for (int r = c + 1; r < 5; ++r) {
            double v = l[r][c];
#pragma unroll
            for (int k = 0; k < c; ++k) v = fma(-l[r][k], l[c][k], v);
            l[r][c] = v * inv;
        }
    }
    double y[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        double v = -sums[15 + r];
#pragma unroll
        for (int k = 0; k < r; ++k) v = fma(-l[r][k], y[k], v);
        y[r] = v / l[r][r];
    }
#pragma unroll
    for (int r = 4; r >= 0; --r) {
        double v = y[r];
#pragma unroll
        for (int k = r + 1; k < 5; ++k) v = fma(-l[k][r], delta[k], v);
        delta[r] = v / l[r][r];
        ok = ok && finite64(delta[r]);
    }
    return ok;
}

LG_HD double sinc64(double x) { return x == 0.0 ? 1.0 : sin(x) / x; }

// The trial pose: R <- exp([ω]x) R by the Rodrigues formula, exp = I + (sin θ / θ) [ω]x + ((1 - cos θ) / θ²) [ω]x²
// with (1 - cos θ) / θ² = (sin(θ / 2) / (θ / 2))² / 2 (no cancellation at small θ), and t <- normalise(t + τ1 b1 + τ2 b2).
LG_HD void polish_update(const PolishPose& s, const double delta[5], PolishPose& out) {
    const double w[3] = {delta[0], delta[1], delta[2]};
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double ka = sinc64(theta), kh = sinc64(0.5 * theta), kb = 0.5 * kh * kh;
    double g[9], h[9], b[2][3];
    tangent_basis(s.t, b);
    cross_mul(w, s.r, g);
    cross_mul(w, g, h);
#pragma unroll
    for (int k = 0; k < 9; ++k) out.r[k] = s.r[k] + ka * g[k] + kb * h[k];
    double t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = s.t[k] + delta[3] * b[0][k] + delta[4] * b[1][k];
    const double inv = 1.0 / sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) out.t[k] = t[k] * inv;
}

// The midpoint triangulation of a correspondence (camera coordinates) under X1 = R X0 + t: in_front's depths
// (d0, d1), and X = (d0 a + Rᵀ (d1 b - t)) / 2 in camera 0's frame for the rays a = (q0, 1), b = (q1, 1). True where
// both depths are positive and X is finite (x is zeros otherwise).
LG_HD bool midpoint(const double r[9], const double t[3], double x0, double y0, double x1, double y1, double x[3]) {
    const double a0 = r[0] * x0 + r[1] * y0 + r[2], a1 = r[3] * x0 + r[4] * y0 + r[5], a2 = r[6] * x0 + r[7] * y0 + r[8];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = x1 * x1 + y1 * y1 + 1.0, ab = a0 * x1 + a1 * y1 + a2;
    const double at = a0 * t[0] + a1 * t[1] + a2 * t[2], bt = x1 * t[0] + y1 * t[1] + t[2];
    const double det = aa * bb - ab * ab;
    const double d0 = (ab * bt - bb * at) / det, d1 = (aa * bt - ab * at) / det;
    const double v0 = d1 * x1 - t[0], v1 = d1 * y1 - t[1], v2 = d1 - t[2];
    const double p0 = 0.5 * (d0 * x0 + (r[0] * v0 + r[3] * v1 + r[6] * v2));
    const double p1 = 0.5 * (d0 * y0 + (r[1] * v0 + r[4] * v1 + r[7] * v2));
    const double p2 = 0.5 * (d0 + (r[2] * v0 + r[5] * v1 + r[8] * v2));
    const bool ok = d0 > 0.0 && d1 > 0.0 && finite64(p0) && finite64(p1) && finite64(p2);  // (NaN: false)
    x[0] = ok ? p0 : 0.0, x[1] = ok ? p1 : 0.0, x[2] = ok ? p2 : 0.0;
    return ok;
}

}  // namespace lg_geom
