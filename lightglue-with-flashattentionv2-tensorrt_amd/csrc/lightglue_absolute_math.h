// lightglue_absolute_math.h — the per-lane arithmetic of the absolute pose (csrc/lightglue_absolute.hip;
// include/lightglue_glue.h, "the absolute pose"): the P3P solve of three 2D-3D correspondences, the reprojection
// inlier test, and the pieces of the Levenberg-Marquardt refit on the 6 parameters of (R, t). The style is
// lightglue_essential_math.h's: plain __host__ __device__ functions on values and small fixed-size arrays, every index
// a compile-time constant after unrolling, selection by selects, every loop with a compile-time bound. From
// lightglue_polish_math.h: finite64, cross_mul, sinc64 and the λ constants.
//
// The P3P route. Bearings f_i: the unit vectors of ((x - cx) / fx, (y - cy) / fy, 1); c_ij = f_i . f_j; the map
// distances over the first: E = |X1 - X3|² / |X1 - X2|², F = |X2 - X3|² / |X1 - X2|². With the camera distances
// s1, s2 = u s1, s3 = v s1 the law of cosines on the three sides, s1² eliminated, leaves two conics in (u, v):
//     (A)  v² - 2 c13 v + 1 - E q(u) = 0,        (B)  v² - 2 c23 u v + u² - F q(u) = 0,       q(u) = 1 - 2 c12 u + u².
// (A) - (B) is linear in v: v = N(u) / D(u), N = u² - 1 + (E - F) q(u), D = 2 (c23 u - c13); into (A) times D²:
//     N² - 2 c13 N D + (1 - E q) D² = 0,
// a quartic in u (Grunert's, in the ratio of two distances). Its real roots in (0, Cauchy bound]: the interval is
// cut at the real roots of the derivative (a cubic: cubic_roots), the quartic is monotonic on each of the four
// pieces, a piece whose ends differ in sign is bisected kAbsBisections times and the midpoint takes kAbsNewton Newton
// steps that may not leave the bracket. (The float64 contract finds the roots as eigenvalues, numpy.roots, and v from
// (A) as a quadratic.) Per root: s1 = |X1 - X2| / sqrt(q(u)), the camera points Y_i = s_i f_i, and the pose from the
// two triangles' orthonormal frames (e1 along side 12, e3 the normal, e2 = e3 x e1): R = G Eᵀ, t = Y1 - R X1 (the
// contract: an SVD absolute orientation). No candidate: u or v not positive, a depth (R X_i + t)_z not positive,
// anything not finite, or a sample triangle of area below kAreaEps of its longest side squared.
#pragma once

#include "lightglue_polish_math.h"

namespace lg_geom {

constexpr int kMinInliersA = 4;        // an absolute pose, and its refit, needs 4 correspondences
constexpr int kCands3 = 4;             // candidates a hypothesis at most
constexpr double kAreaEps = 1e-6;      // the sample triangle's area over its longest side squared
constexpr int kAbsBisections = 40;     // per piece: its width falls to 2^-40 of the root bound
constexpr int kAbsNewton = 4;          // then Newton steps that may not leave the bracket
constexpr int kAbsoluteLmRounds = 4;   // Levenberg-Marquardt rounds a refit (profiles/geometry/INDEX.md has the table)
constexpr int kAbsSums = 29;           // JᵀJ's upper triangle (21), Jᵀr (6), Σ |r|² and the number of rows
constexpr int kMinAbsRows = 3;         // the fixed set needs as many residuals as there are parameters
constexpr int kAbsRecord = 16;         // floats per hypothesis in the workspace: R[9], t[3], count, pad

struct Camera {  // (fx, fy, cx, cy) of the one camera
    float fx, fy, cx, cy;
};

LG_HD bool camera_ok(const Camera& k) {
    return fabsf(k.fx) < INFINITY && fabsf(k.fy) < INFINITY && fabsf(k.cx) < INFINITY && fabsf(k.cy) < INFINITY && k.fx > 0.f &&
           k.fy > 0.f;
}

// ---- the reprojection error -----------------------------------------------------------------------------------------
// Xc = R X + t (p: R row-major then t); err = (fx Xc.x / Xc.z + cx - x)² + (fy Xc.y / Xc.z + cy - y)² <= thr2 and
// Xc.z > 0, without the divisions: with dx = fx Xc.x + (cx - x) Xc.z and dy alike, dx² + dy² <= thr2 Xc.z², where the
// left side is finite (NaN fails every comparison).
LG_HD bool is_inlier_abs(const float p[12], const Camera& k, float X, float Y, float Z, float x, float y, float thr2) {
    const float xc = fmaf(p[0], X, fmaf(p[1], Y, fmaf(p[2], Z, p[9])));
    const float yc = fmaf(p[3], X, fmaf(p[4], Y, fmaf(p[5], Z, p[10])));
    const float zc = fmaf(p[6], X, fmaf(p[7], Y, fmaf(p[8], Z, p[11])));
    const float dx = fmaf(k.fx, xc, (k.cx - x) * zc), dy = fmaf(k.fy, yc, (k.cy - y) * zc);
    const float d2 = fmaf(dx, dx, dy * dy);
    return zc > 0.f && d2 <= thr2 * (zc * zc) && d2 < INFINITY;
}

// ---- the P3P solve -----------------------------------------------------------------------------------------------
LG_HD double quartic_at(const double c[5], double x) { return fma(fma(fma(fma(c[4], x, c[3]), x, c[2]), x, c[1]), x, c[0]); }
LG_HD double quartic_slope(const double c[5], double x) {
    return fma(fma(fma(4.0 * c[4], x, 3.0 * c[3]), x, 2.0 * c[2]), x, c[1]);
}

// What the roots of a sample share: the bearings, the quartic (c[i] of u^i), N, D, and the five cuts of (0, bound].
struct P3p {
    double f[3][3];
    double c[5], n[3], d[2];
    double c12, len12;
    double cut0, cut1, cut2, cut3, cut4;
    bool ok;
};

// x [3][3]: the sample's map points; px [3][2]: its pixels.
LG_HD void p3p_setup(const double x[3][3], const double px[3][2], const Camera& k, P3p& s) {
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double a = (px[i][0] - (double)k.cx) / (double)k.fx, b = (px[i][1] - (double)k.cy) / (double)k.fy;
        const double inv = 1.0 / sqrt(a * a + b * b + 1.0);
        s.f[i][0] = a * inv, s.f[i][1] = b * inv, s.f[i][2] = inv;
        ok = ok && finite64(a) && finite64(b);
    }
    double e01[3], e02[3], e12[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) e01[j] = x[1][j] - x[0][j], e02[j] = x[2][j] - x[0][j], e12[j] = x[2][j] - x[1][j];
    const double l01 = e01[0] * e01[0] + e01[1] * e01[1] + e01[2] * e01[2];
    const double l02 = e02[0] * e02[0] + e02[1] * e02[1] + e02[2] * e02[2];
    const double l12 = e12[0] * e12[0] + e12[1] * e12[1] + e12[2] * e12[2];
    const double n0 = e01[1] * e02[2] - e01[2] * e02[1], n1 = e01[2] * e02[0] - e01[0] * e02[2], n2 = e01[0] * e02[1] - e01[1] * e02[0];
    const double area = 0.5 * sqrt(n0 * n0 + n1 * n1 + n2 * n2);
    const double longest = fmax(l01, fmax(l02, l12));
    ok = ok && finite64(longest) && area >= kAreaEps * longest && longest > 0.0;  // (NaN: false)
    const double c12 = s.f[0][0] * s.f[1][0] + s.f[0][1] * s.f[1][1] + s.f[0][2] * s.f[1][2];
    const double c13 = s.f[0][0] * s.f[2][0] + s.f[0][1] * s.f[2][1] + s.f[0][2] * s.f[2][2];
    const double c23 = s.f[1][0] * s.f[2][0] + s.f[1][1] * s.f[2][1] + s.f[1][2] * s.f[2][2];
    const double ee = l02 / l01, ff = l12 / l01, g = ee - ff;
    s.c12 = c12, s.len12 = sqrt(l01);
    s.n[0] = g - 1.0, s.n[1] = -2.0 * c12 * g, s.n[2] = 1.0 + g;
    s.d[0] = -2.0 * c13, s.d[1] = 2.0 * c23;
    const double* n = s.n;
    const double* d = s.d;
    // N², N D, D² and (1 - E q)
    const double nn[5] = {n[0] * n[0], 2.0 * n[0] * n[1], 2.0 * n[0] * n[2] + n[1] * n[1], 2.0 * n[1] * n[2], n[2] * n[2]};
    const double nd[4] = {n[0] * d[0], n[0] * d[1] + n[1] * d[0], n[1] * d[1] + n[2] * d[0], n[2] * d[1]};
    const double dd[3] = {d[0] * d[0], 2.0 * d[0] * d[1], d[1] * d[1]};
    const double w[3] = {1.0 - ee, 2.0 * c12 * ee, -ee};
    s.c[0] = nn[0] - 2.0 * c13 * nd[0] + w[0] * dd[0];
    s.c[1] = nn[1] - 2.0 * c13 * nd[1] + w[0] * dd[1] + w[1] * dd[0];
    s.c[2] = nn[2] - 2.0 * c13 * nd[2] + w[0] * dd[2] + w[1] * dd[1] + w[2] * dd[0];
    s.c[3] = nn[3] - 2.0 * c13 * nd[3] + w[1] * dd[2] + w[2] * dd[1];
    s.c[4] = nn[4] + w[2] * dd[2];
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) big = fmax(big, fabs(s.c[i] / s.c[4]));
    const double bound = 1.0 + big;
    ok = ok && finite64(bound);
    double cr[3];
    const int nc = cubic_roots<double>(4.0 * s.c[4], 3.0 * s.c[3], 2.0 * s.c[2], s.c[1], cr);
    ok = ok && nc > 0;
    // one real critical point: the three cuts coincide and the pieces between them are empty
    cr[1] = nc == 3 ? cr[1] : cr[0], cr[2] = nc == 3 ? cr[2] : cr[0];
    s.cut0 = 0.0, s.cut4 = bound;
    s.cut1 = fmin(fmax(cr[0], 0.0), bound), s.cut2 = fmin(fmax(cr[1], 0.0), bound), s.cut3 = fmin(fmax(cr[2], 0.0), bound);
    s.ok = ok;
}

// The root of the quartic in piece `piece` (0..3) of the cuts: false where the piece's ends do not differ in sign.
LG_HD bool p3p_root(const P3p& s, int piece, double& u) {
    // (the cuts are read before the selects: a select between loads of members becomes a load through a selected
    // address, and the struct then lives in scratch)
    const double c0 = s.cut0, c1 = s.cut1, c2 = s.cut2, c3 = s.cut3, c4 = s.cut4;
    double lo = piece == 0 ? c0 : (piece == 1 ? c1 : (piece == 2 ? c2 : c3));
    double hi = piece == 0 ? c1 : (piece == 1 ? c2 : (piece == 2 ? c3 : c4));
    const double flo = quartic_at(s.c, lo), fhi = quartic_at(s.c, hi);
    const bool neg = flo < 0.0;
    const bool has = s.ok && finite64(flo) && finite64(fhi) && neg != (fhi < 0.0);
#pragma unroll 1
    for (int it = 0; it < kAbsBisections; ++it) {
        const double mid = 0.5 * (lo + hi);
        const bool same = (quartic_at(s.c, mid) < 0.0) == neg;
        lo = same ? mid : lo, hi = same ? hi : mid;
    }
    double x = 0.5 * (lo + hi);
#pragma unroll
    for (int it = 0; it < kAbsNewton; ++it) {
        const double nx = x - quartic_at(s.c, x) / quartic_slope(s.c, x);
        x = nx >= lo && nx <= hi ? nx : x;  // (NaN: stays)
    }
    u = x;
    return has;
}

// e1 along a, e3 along a x b, e2 = e3 x e1 (columns of m, row-major 3 x 3).
LG_HD void triangle_frame(const double a[3], const double b[3], double m[9]) {
    const double ia = 1.0 / sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double e1[3] = {a[0] * ia, a[1] * ia, a[2] * ia};
    const double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const double in = 1.0 / sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    const double e3[3] = {n[0] * in, n[1] * in, n[2] * in};
    const double e2[3] = {e3[1] * e1[2] - e3[2] * e1[1], e3[2] * e1[0] - e3[0] * e1[2], e3[0] * e1[1] - e3[1] * e1[0]};
#pragma unroll
    for (int i = 0; i < 3; ++i) m[3 * i] = e1[i], m[3 * i + 1] = e2[i], m[3 * i + 2] = e3[i];
}

// The pose of the root u: r, t and key = |R X1 + t| (the candidates' order); false where there is no candidate.
LG_HD bool p3p_pose(const P3p& s, const double x[3][3], double u, double r[9], double t[3], double& key) {
    const double q = fma(u, u - 2.0 * s.c12, 1.0);
    const double v = fma(fma(s.n[2], u, s.n[1]), u, s.n[0]) / fma(s.d[1], u, s.d[0]);
    const double s1 = s.len12 / sqrt(q), s2 = u * s1, s3 = v * s1;
    bool ok = u > 0.0 && v > 0.0 && s1 > 0.0 && finite64(s1) && finite64(s2) && finite64(s3);
    double y[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) y[0][j] = s1 * s.f[0][j], y[1][j] = s2 * s.f[1][j], y[2][j] = s3 * s.f[2][j];
    double a[3], b[3], ga[3], gb[3], em[9], gm[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[j] = x[1][j] - x[0][j], b[j] = x[2][j] - x[0][j], ga[j] = y[1][j] - y[0][j], gb[j] = y[2][j] - y[0][j];
    triangle_frame(a, b, em);
    triangle_frame(ga, gb, gm);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r[3 * i + j] = gm[3 * i] * em[3 * j] + gm[3 * i + 1] * em[3 * j + 1] + gm[3 * i + 2] * em[3 * j + 2];
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = y[0][i] - (r[3 * i] * x[0][0] + r[3 * i + 1] * x[0][1] + r[3 * i + 2] * x[0][2]);
#pragma unroll
    for (int k = 0; k < 9; ++k) ok = ok && finite64(r[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ok = ok && finite64(t[k]);
        ok = ok && r[6] * x[k][0] + r[7] * x[k][1] + r[8] * x[k][2] + t[2] > 0.0;  // (NaN: false)
    }
    double c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = r[3 * i] * x[0][0] + r[3 * i + 1] * x[0][1] + r[3 * i + 2] * x[0][2] + t[i];
    key = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    return ok;
}

// ---- the Levenberg-Marquardt refit --------------------------------------------------------------------------------
struct AbsPose {
    double r[9], t[3];
};

// The entering pose from one in fp32: R one Newton step of the polar iteration nearer the rotations (polish_enter's).
// False where R or t is not finite.
LG_HD bool absolute_enter(const float p[12], AbsPose& s) {
    bool ok = true;
    double m[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) m[k] = (double)p[k], ok = ok && finite64(m[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) s.t[k] = (double)p[9 + k], ok = ok && finite64(s.t[k]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;  // (R (3 I - Rᵀ R))[i][j]
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double g = m[k] * m[j] + m[3 + k] * m[3 + j] + m[6 + k] * m[6 + j];
                v += m[3 * i + k] * ((k == j ? 3.0 : 0.0) - g);
            }
            s.r[3 * i + j] = 0.5 * v;
        }
    return ok;
}

// The residual (px) of a row and its two Jacobian rows over (ω, δt): with Y = R X, Xc = Y + t,
// u = fx Xc.x / Xc.z + cx, ∂u/∂Xc = a = (fx / z, 0, -fx Xc.x / z²), ∂u/∂ω = Y x a, ∂u/∂t = a; v alike. False where the
// depth is not positive or the residual not finite.
LG_HD bool absolute_row(const AbsPose& q, const Camera& k, double X, double Y, double Z, double x, double y, double res[2],
                        double j[2][6]) {
    const double y0 = q.r[0] * X + q.r[1] * Y + q.r[2] * Z, y1 = q.r[3] * X + q.r[4] * Y + q.r[5] * Z;
    const double y2 = q.r[6] * X + q.r[7] * Y + q.r[8] * Z;
    const double xc = y0 + q.t[0], yc = y1 + q.t[1], zc = y2 + q.t[2];
    const double iz = 1.0 / zc, fx = (double)k.fx, fy = (double)k.fy;
    res[0] = fx * xc * iz + ((double)k.cx - x), res[1] = fy * yc * iz + ((double)k.cy - y);
    const double a0 = fx * iz, a2 = -fx * xc * iz * iz, b1 = fy * iz, b2 = -fy * yc * iz * iz;
    j[0][0] = y1 * a2, j[0][1] = y2 * a0 - y0 * a2, j[0][2] = -y1 * a0;           // Y x (a0, 0, a2)
    j[0][3] = a0, j[0][4] = 0.0, j[0][5] = a2;
    j[1][0] = y1 * b2 - y2 * b1, j[1][1] = -y0 * b2, j[1][2] = y0 * b1;            // Y x (0, b1, b2)
    j[1][3] = 0.0, j[1][4] = b1, j[1][5] = b2;
    return zc > 0.0 && finite64(res[0]) && finite64(res[1]);
}

// acc += the row's part of the kAbsSums sums: JᵀJ's upper triangle row by row, Jᵀr, |r|² and 1.
LG_HD void absolute_accumulate(double acc[kAbsSums], const double res[2], const double j[2][6]) {
#pragma unroll
    for (int w = 0; w < 2; ++w) {
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[e] = fma(j[w][a], j[w][b], acc[e]), ++e;
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] = fma(j[w][a], res[w], acc[21 + a]);
        acc[27] = fma(res[w], res[w], acc[27]);
    }
    acc[28] += 1.0;
}

// The Levenberg-Marquardt step of the sums: (JᵀJ + λ diag(JᵀJ)) δ = -Jᵀr by a 6 x 6 Cholesky factorisation
// (polish_step's statements at another size). False where a pivot is not positive or not finite.
LG_HD bool absolute_step(const double sums[kAbsSums], double lambda, double delta[6]) {
    double l[6][6];
    int e = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) l[b][a] = sums[e] * (a == b ? 1.0 + lambda : 1.0), ++e;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double piv = l[c][c];
#pragma unroll
        for (int k = 0; k < c; ++k) piv = fma(-l[c][k], l[c][k], piv);
        ok = ok && piv > 0.0 && finite64(piv);  // (NaN: false)
        const double root = sqrt(piv), inv = 1.0 / root;
        l[c][c] = root;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
            double v = l[r][c];
#pragma unroll
            for (int k = 0; k < c; ++k) v = fma(-l[r][k], l[c][k], v);
            l[r][c] = v * inv;
        }
    }
    double y[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        double v = -sums[21 + r];
#pragma unroll
        for (int k = 0; k < r; ++k) v = fma(-l[r][k], y[k], v);
        y[r] = v / l[r][r];
    }
#pragma unroll
    for (int r = 5; r >= 0; --r) {
        double v = y[r];
#pragma unroll
        for (int k = r + 1; k < 6; ++k) v = fma(-l[k][r], delta[k], v);
        delta[r] = v / l[r][r];
        ok = ok && finite64(delta[r]);
    }
    return ok;
}

// The trial pose: R <- exp([ω]x) R by the Rodrigues formula (polish_update's), t <- t + δt.
LG_HD void absolute_update(const AbsPose& s, const double delta[6], AbsPose& out) {
    const double w[3] = {delta[0], delta[1], delta[2]};
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double ka = sinc64(theta), kh = sinc64(0.5 * theta), kb = 0.5 * kh * kh;
    double g[9], h[9];
    cross_mul(w, s.r, g);
    cross_mul(w, g, h);
#pragma unroll
    for (int k = 0; k < 9; ++k) out.r[k] = s.r[k] + ka * g[k] + kb * h[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) out.t[k] = s.t[k] + delta[3 + k];
}

// The pose rounded to the output's fp32 (R row-major then t); false where an entry is not finite there.
LG_HD bool absolute_round(const AbsPose& s, float p[12]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) p[k] = (float)s.r[k], ok = ok && fabsf(p[k]) < INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) p[9 + k] = (float)s.t[k], ok = ok && fabsf(p[9 + k]) < INFINITY;
    return ok;
}

}  // namespace lg_geom
