// lightglue_geometry_math.h — the per-lane arithmetic of the fundamental-matrix and homography RANSAC
// (csrc/lightglue_geometry.hip; include/lightglue_glue.h, "geometric verification"): the sample hash, the
// 7-point and 4-point solves, the epipolar and transfer errors and the pieces of the fp64 refits. Plain
// functions on values and small fixed-size arrays, every index a compile-time constant after unrolling (a
// run-time index into a register array goes to scratch on this compiler): pivoting and compaction are
// selects. The functions are __host__ __device__, so a host program can run the same statements on the CPU.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LG_HD __host__ __device__ __forceinline__
#else
#define LG_HD inline
#endif

namespace lg_geom {

constexpr int kMaxPoints = 2048;     // the plugin's N limit
constexpr int kMaxHypotheses = 4096;
constexpr int kMaxRefits = 8;
constexpr int kMinInliers = 8;       // a fundamental matrix, and its refit, needs 8 correspondences
constexpr int kMinInliersH = 4;      // a homography, and its refit, needs 4
constexpr float kPivotEps = 1e-6f;   // a pivot of the 7 x 9 (8 x 9) elimination below this: no candidate
constexpr int kJacobiSweeps = 7;     // 9 x 9, fp64, 9 steps of 4 disjoint rotations a sweep; off-diagonal / diagonal
                                     // norm on the test scenes: 3e-4 after 4 sweeps, 4e-8 after 5, 6e-16 after 6
constexpr int kJacobi3Sweeps = 6;

// ---- the sample -------------------------------------------------------------------------------------------------
// A counter-based hash of (seed, hypothesis, draw): the three folded into one word by odd multipliers, then
// the "lowbias32" finaliser. The pair index is not in the key.
LG_HD uint32_t hash32(uint32_t seed, uint32_t h, uint32_t j) {
    uint32_t x = seed * 0x9E3779B1u + h * 0x85EBCA77u + j * 0xC2B2AE3Du + 0x27D4EB2Fu;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    x *= 0x846CA68Bu;
    x ^= x >> 16;
    return x;
}

// N distinct indices in [0, count), count >= N: draw j is hash % (count - j), moved past the earlier draws in
// ascending order (r += 1 for each earlier draw <= r, smallest first). idx is in draw order. The first draws do
// not depend on N: the 4-sample of a hypothesis is the first four of its 7-sample.
template <int N>
LG_HD void sample(uint32_t seed, int h, int count, int idx[N]) {
    int sorted[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        int r = (int)(hash32(seed, (uint32_t)h, (uint32_t)j) % (uint32_t)(count - j));
#pragma unroll
        for (int e = 0; e < j; ++e) r += r >= sorted[e] ? 1 : 0;
        idx[j] = r;
        int v = r;
#pragma unroll
        for (int e = 0; e < j; ++e) {  // insert: the first j stay ascending
            const int lo = sorted[e] < v ? sorted[e] : v, hi = sorted[e] < v ? v : sorted[e];
            sorted[e] = lo, v = hi;
        }
        sorted[j] = v;
    }
}

// ---- Hartley normalisation: x' = s (x - cx), y' = s (y - cy) per image ------------------------------------------
template <typename T>
struct NormT {
    T cx0, cy0, s0, cx1, cy1, s1;
};

// ---- the epipolar error -------------------------------------------------------------------------------------------
// l1 = F x0, l0 = Fᵀ x1, d = x1 · l1; err = max(d² / (l1x² + l1y²), d² / (l0x² + l0y²)) <= thr2, without the
// divisions: d² <= thr2 den on both sides, where both denominators are positive and d² is finite (a zero
// denominator or a non-finite d² makes err non-finite: no inlier; NaN fails every comparison).
LG_HD bool is_inlier(const float f[9], float x0, float y0, float x1, float y1, float thr2) {
    const float l1x = fmaf(f[0], x0, fmaf(f[1], y0, f[2]));
    const float l1y = fmaf(f[3], x0, fmaf(f[4], y0, f[5]));
    const float l1z = fmaf(f[6], x0, fmaf(f[7], y0, f[8]));
    const float l0x = fmaf(f[0], x1, fmaf(f[3], y1, f[6]));
    const float l0y = fmaf(f[1], x1, fmaf(f[4], y1, f[7]));
    const float d = fmaf(x1, l1x, fmaf(y1, l1y, l1z));
    const float d2 = d * d;
    const float den1 = fmaf(l1x, l1x, l1y * l1y), den0 = fmaf(l0x, l0x, l0y * l0y);
    return d2 <= thr2 * den1 && d2 <= thr2 * den0 && den1 > 0.f && den0 > 0.f && d2 < INFINITY;
}

// ---- the transfer error (homography) -------------------------------------------------------------------------------
// (X, Y, W) = H x0; err = (x1 - X/W)² + (y1 - Y/W)² <= thr2, without the division: with dx = x1 W - X and
// dy = y1 W - Y, dx² + dy² <= thr2 W², where W² is positive and the left side finite (W = 0 or anything
// non-finite makes err non-finite: no inlier; NaN fails every comparison).
LG_HD bool is_inlier_h(const float h[9], float x0, float y0, float x1, float y1, float thr2) {
    const float X = fmaf(h[0], x0, fmaf(h[1], y0, h[2]));
    const float Y = fmaf(h[3], x0, fmaf(h[4], y0, h[5]));
    const float W = fmaf(h[6], x0, fmaf(h[7], y0, h[8]));
    const float dx = fmaf(x1, W, -X), dy = fmaf(y1, W, -Y);
    const float d2 = fmaf(dx, dx, dy * dy), w2 = W * W;
    return d2 <= thr2 * w2 && w2 > 0.f && d2 < INFINITY;
}

// The sign rule of the output: the entry of the largest magnitude (the lowest index among equals) is positive.
LG_HD void fix_sign(float f[9]) {
    float best = fabsf(f[0]), val = f[0];
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const bool up = fabsf(f[i]) > best;
        best = up ? fabsf(f[i]) : best, val = up ? f[i] : val;
    }
    const float sg = val < 0.f ? -1.f : 1.f;
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] *= sg;
}

// float and double forms of the few library functions the solve uses. The solve is a template on its real type:
// the kernel runs it in double; float is the form that was measured on the CPU and dropped.
LG_HD float m_sqrt(float x) { return sqrtf(x); }
LG_HD double m_sqrt(double x) { return sqrt(x); }
LG_HD float m_abs(float x) { return fabsf(x); }
LG_HD double m_abs(double x) { return fabs(x); }
LG_HD float m_acos(float x) { return acosf(x); }
LG_HD double m_acos(double x) { return acos(x); }
LG_HD float m_cos(float x) { return cosf(x); }
LG_HD double m_cos(double x) { return cos(x); }
LG_HD float m_cbrt(float x) { return cbrtf(x); }
LG_HD double m_cbrt(double x) { return cbrt(x); }
LG_HD float m_fma(float a, float b, float c) { return fmaf(a, b, c); }
LG_HD double m_fma(double a, double b, double c) { return fma(a, b, c); }

template <typename T>
LG_HD T det3(const T* a, const T* b, const T* c) {
    return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) + a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// The real roots of c3 x³ + c2 x² + c1 x + c0 in ascending order (closed form, then two Newton steps on the
// polynomial itself); returns their number, 1 or 3 (0 where a coefficient ratio is not finite).
template <typename T>
LG_HD int cubic_roots(T c3, T c2, T c1, T c0, T r[3]) {
    const T a = c2 / c3, b = c1 / c3, c = c0 / c3;
    const T q = (a * a - T(3) * b) * T(1.0 / 9.0);
    const T rr = (a * (T(2) * a * a - T(9) * b) + T(27) * c) * T(1.0 / 54.0);
    const T q3 = q * q * q, a3 = a * T(1.0 / 3.0);
    int n;
    r[0] = r[1] = r[2] = T(0);
    if (!(m_abs(a) < T(INFINITY) && m_abs(b) < T(INFINITY) && m_abs(c) < T(INFINITY))) return 0;
    if (rr * rr < q3) {
        const T sq = m_sqrt(q);
        T ct = rr / (sq * q);
        ct = ct < T(-1) ? T(-1) : (ct > T(1) ? T(1) : ct);
        const T th = m_acos(ct) * T(1.0 / 3.0);
        const T k = T(2.0943951023931953);  // 2 pi / 3
        r[0] = T(-2) * sq * m_cos(th) - a3;
        r[1] = T(-2) * sq * m_cos(th + k) - a3;
        r[2] = T(-2) * sq * m_cos(th - k) - a3;
        n = 3;
    } else {
        const T e = m_cbrt(m_abs(rr) + m_sqrt(rr * rr - q3));
        const T aa = rr < T(0) ? e : -e;
        const T bb = aa != T(0) ? q / aa : T(0);
        r[0] = aa + bb - a3;
        n = 1;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const T x = r[i];
            const T p = m_fma(m_fma(m_fma(c3, x, c2), x, c1), x, c0);
            const T dp = m_fma(m_fma(T(3) * c3, x, T(2) * c2), x, c1);
            const T step = p / dp;
            if (m_abs(step) < T(INFINITY)) r[i] = x - step;
        }
    }
    if (n == 3) {  // ascending
        T lo = r[0] < r[1] ? r[0] : r[1], hi = r[0] < r[1] ? r[1] : r[0];
        const T t = hi < r[2] ? hi : r[2];
        const T mid = lo < t ? t : lo;
        lo = lo < r[2] ? lo : r[2], hi = hi < r[2] ? r[2] : hi;
        r[0] = lo, r[1] = mid, r[2] = hi;
    }
    return n;
}

// T1ᵀ F T0 of a matrix in normalised coordinates, scaled to unit Frobenius norm and rounded to fp32; false
// where the result is not finite or zero (out is then zeros).
template <typename T>
LG_HD bool denormalise(const T fn[9], const NormT<T>& t, float out[9]) {
    T m[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        m[3 * r] = t.s0 * fn[3 * r];
        m[3 * r + 1] = t.s0 * fn[3 * r + 1];
        m[3 * r + 2] = fn[3 * r + 2] - t.s0 * (t.cx0 * fn[3 * r] + t.cy0 * fn[3 * r + 1]);
    }
    T g[9], ss = T(0);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        g[k] = t.s1 * m[k];
        g[3 + k] = t.s1 * m[3 + k];
        g[6 + k] = m[6 + k] - t.s1 * (t.cx1 * m[k] + t.cy1 * m[3 + k]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) ss = m_fma(g[i], g[i], ss);
    const T inv = T(1) / m_sqrt(ss);
    const bool ok = ss > T(0) && ss < T(INFINITY) && inv < T(INFINITY);
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = ok ? (float)(g[i] * inv) : 0.f;
    return ok;
}

// The 7-point solve on normalised points, in T: the null space of the 7 x 9 system by Gauss-Jordan elimination
// with partial (row) pivoting, f1 = (-B[:, 0], 1, 0), f2 = (-B[:, 1], 0, 1) for the reduced system [I | B];
// the real roots of det(l f1 + (1 - l) f2) = 0 in ascending l; each candidate de-normalised to pixels at unit
// norm, fp32. Returns the number of candidates, 0..3, cand[n..] zeros. Rows: x1ᵀ F x0 = 0, F row-major.
template <typename T>
LG_HD int solve7(const T x0[7], const T y0[7], const T x1[7], const T y1[7], const NormT<T>& t, float cand[3][9]) {
    T a[7][9];
#pragma unroll
    for (int r = 0; r < 7; ++r) {
        a[r][0] = x1[r] * x0[r], a[r][1] = x1[r] * y0[r], a[r][2] = x1[r];
        a[r][3] = y1[r] * x0[r], a[r][4] = y1[r] * y0[r], a[r][5] = y1[r];
        a[r][6] = x0[r], a[r][7] = y0[r], a[r][8] = T(1);
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 7; ++c) {
        T best = m_abs(a[c][c]);
        int piv = c;
#pragma unroll
        for (int r = c + 1; r < 7; ++r) {
            const T v = m_abs(a[r][c]);
            const bool up = v > best;
            best = up ? v : best, piv = up ? r : piv;
        }
        ok = ok && best >= T(kPivotEps);  // (NaN: false)
#pragma unroll
        for (int r = c + 1; r < 7; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int k = c; k < 9; ++k) {
                const T u = a[c][k], v = a[r][k];
                a[c][k] = sw ? v : u, a[r][k] = sw ? u : v;
            }
        }
        const T inv = T(1) / a[c][c];
#pragma unroll
        for (int k = c + 1; k < 9; ++k) a[c][k] *= inv;
#pragma unroll
        for (int r = 0; r < 7; ++r) {
            if (r == c) continue;
            const T f = a[r][c];
#pragma unroll
            for (int k = c + 1; k < 9; ++k) a[r][k] = m_fma(-f, a[c][k], a[r][k]);
        }
    }
    T g[9], d[9];  // g = f2, d = f1 - f2: F(l) = g + l d
#pragma unroll
    for (int r = 0; r < 7; ++r) g[r] = -a[r][8], d[r] = a[r][8] - a[r][7];
    g[7] = T(0), g[8] = T(1), d[7] = T(1), d[8] = T(-1);
    const T c0 = det3(g, g + 3, g + 6);
    const T c1 = det3(d, g + 3, g + 6) + det3(g, d + 3, g + 6) + det3(g, g + 3, d + 6);
    const T c2 = det3(d, d + 3, g + 6) + det3(d, g + 3, d + 6) + det3(g, d + 3, d + 6);
    const T c3 = det3(d, d + 3, d + 6);
    T root[3];
    const int nr = ok ? cubic_roots(c3, c2, c1, c0, root) : 0;
    bool good[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        T fn[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) fn[k] = m_fma(root[i], d[k], g[k]);
        good[i] = denormalise(fn, t, cand[i]) && i < nr;
#pragma unroll
        for (int k = 0; k < 9; ++k) cand[i][k] = good[i] ? cand[i][k] : 0.f;
    }
    // the candidates that exist first, in their order
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const bool mv = !good[i] && good[i + 1];
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float u = cand[i][k], v = cand[i + 1][k];
                cand[i][k] = mv ? v : u, cand[i + 1][k] = mv ? u : v;
            }
            good[i] = good[i] || mv, good[i + 1] = good[i + 1] && !mv;
        }
    }
    return (good[0] ? 1 : 0) + (good[1] ? 1 : 0) + (good[2] ? 1 : 0);
}

// T1⁻¹ Hn T0 of a homography in normalised coordinates, scaled to unit Frobenius norm; false where the result is
// not finite or zero (out is then zeros).
template <typename T>
LG_HD bool denormalise_h(const T hn[9], T cx0, T cy0, T s0, T cx1, T cy1, T s1, T out[9]) {
    T m[9], ss = T(0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        m[3 * r] = s0 * hn[3 * r];
        m[3 * r + 1] = s0 * hn[3 * r + 1];
        m[3 * r + 2] = hn[3 * r + 2] - s0 * (cx0 * hn[3 * r] + cy0 * hn[3 * r + 1]);
    }
    const T r1 = T(1) / s1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = m_fma(cx1, m[6 + k], r1 * m[k]);
        out[3 + k] = m_fma(cy1, m[6 + k], r1 * m[3 + k]);
        out[6 + k] = m[6 + k];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) ss = m_fma(out[i], out[i], ss);
    const T inv = T(1) / m_sqrt(ss);
    const bool ok = ss > T(0) && ss < T(INFINITY) && inv < T(INFINITY);
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = ok ? out[i] * inv : T(0);
    return ok;
}

// The sign of the orientation of the triple (i, j, k) in image 0 times that in image 1: +1, -1 or 0 (a
// collinear triple in either image, or NaN).
template <typename T>
LG_HD int orientation_product(const T x0[4], const T y0[4], const T x1[4], const T y1[4], int i, int j, int k) {
    const T d0 = (x0[j] - x0[i]) * (y0[k] - y0[i]) - (y0[j] - y0[i]) * (x0[k] - x0[i]);
    const T d1 = (x1[j] - x1[i]) * (y1[k] - y1[i]) - (y1[j] - y1[i]) * (x1[k] - x1[i]);
    const int a = d0 > T(0) ? 1 : (d0 < T(0) ? -1 : 0), b = d1 > T(0) ? 1 : (d1 < T(0) ? -1 : 0);
    return a * b;
}

// The 4-point solve on normalised points, in T: the null vector of the 8 x 9 system (two rows a point:
// (-x0, -y0, -1, 0, 0, 0, x1 x0, x1 y0, x1) and (0, 0, 0, -x0, -y0, -1, y1 x0, y1 y0, y1)) by Gauss-Jordan
// elimination with partial (row) pivoting on columns 0..7, hn = (-B, 1) for the reduced system [I | B]; no
// candidate where a pivot is below kPivotEps or the four triples of the sample are not oriented alike in both
// images (all products of orientation_product positive, or all negative); de-normalised to pixels at unit norm
// with the sign rule, fp32. Returns the number of candidates, 0 or 1 (cand zeros for 0). H row-major, x1 ~ H x0.
template <typename T>
LG_HD int solve4(const T x0[4], const T y0[4], const T x1[4], const T y1[4], const NormT<T>& t, float cand[9]) {
    T a[8][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[2 * i][0] = -x0[i], a[2 * i][1] = -y0[i], a[2 * i][2] = T(-1);
        a[2 * i][3] = T(0), a[2 * i][4] = T(0), a[2 * i][5] = T(0);
        a[2 * i][6] = x1[i] * x0[i], a[2 * i][7] = x1[i] * y0[i], a[2 * i][8] = x1[i];
        a[2 * i + 1][0] = T(0), a[2 * i + 1][1] = T(0), a[2 * i + 1][2] = T(0);
        a[2 * i + 1][3] = -x0[i], a[2 * i + 1][4] = -y0[i], a[2 * i + 1][5] = T(-1);
        a[2 * i + 1][6] = y1[i] * x0[i], a[2 * i + 1][7] = y1[i] * y0[i], a[2 * i + 1][8] = y1[i];
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        T best = m_abs(a[c][c]);
        int piv = c;
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const T v = m_abs(a[r][c]);
            const bool up = v > best;
            best = up ? v : best, piv = up ? r : piv;
        }
        ok = ok && best >= T(kPivotEps);  // (NaN: false)
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int k = c; k < 9; ++k) {
                const T u = a[c][k], v = a[r][k];
                a[c][k] = sw ? v : u, a[r][k] = sw ? u : v;
            }
        }
        const T inv = T(1) / a[c][c];
#pragma unroll
        for (int k = c + 1; k < 9; ++k) a[c][k] *= inv;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            if (r == c) continue;
            const T f = a[r][c];
#pragma unroll
            for (int k = c + 1; k < 9; ++k) a[r][k] = m_fma(-f, a[c][k], a[r][k]);
        }
    }
    int pos = 0, neg = 0;
#pragma unroll
    for (int tr = 0; tr < 4; ++tr) {  // the triples (0 1 2), (0 1 3), (0 2 3), (1 2 3)
        const int o = orientation_product(x0, y0, x1, y1, tr == 3 ? 1 : 0, tr >= 2 ? 2 : 1, tr == 0 ? 2 : 3);
        pos += o > 0 ? 1 : 0, neg += o < 0 ? 1 : 0;
    }
    ok = ok && (pos == 4 || neg == 4);
    T hn[9], hd[9];
#pragma unroll
    for (int r = 0; r < 8; ++r) hn[r] = -a[r][8];
    hn[8] = T(1);
    ok = denormalise_h(hn, t.cx0, t.cy0, t.s0, t.cx1, t.cy1, t.s1, hd) && ok;
#pragma unroll
    for (int k = 0; k < 9; ++k) cand[k] = ok ? (float)hd[k] : 0.f;
    fix_sign(cand);
    return ok ? 1 : 0;
}

// ---- the refit, fp64 ---------------------------------------------------------------------------------------------
// Entry e of the 45 upper-triangle entries (i <= j) of a symmetric 9 x 9 matrix, row by row.
LG_HD void tri_index(int e, int& i, int& j) {
    i = 0;
    int left = e;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        const bool next = left >= 9 - r && i == r;
        left = next ? left - (9 - r) : left;
        i = next ? r + 1 : i;
    }
    j = i + left;
}

// One Jacobi rotation in the (p, q) plane of a symmetric matrix: (c, s) with
// t = apq / (d + sign(d) sqrt(d² + apq²)), d = (aqq - app) / 2, c = 1 / sqrt(1 + t²), s = t c.
LG_HD void jacobi_cs(double app, double aqq, double apq, double& c, double& s) {
    c = 1.0, s = 0.0;
    if (apq == 0.0 || !(fabs(apq) < INFINITY)) return;
    const double d = 0.5 * (aqq - app);
    const double t = apq / (d + copysign(sqrt(d * d + apq * apq), d));
    if (!(fabs(t) < INFINITY)) return;
    c = 1.0 / sqrt(1.0 + t * t);
    s = t * c;
}

// Step `step` of the round-robin ordering of the 36 pairs of 0..8 (9 steps a sweep, 4 disjoint pairs a step):
// pair i (0..3) is ((r + i + 1) % 9, (r + 8 - i) % 9) with r = step % 9.
LG_HD void jacobi_pair(int step, int i, int& p, int& q) {
    const int r = step % 9;
    p = (r + i + 1) % 9, q = (r + 8 - i) % 9;
}

// Rank 2 for a 3 x 3 matrix (row-major, in place): F <- F (I - v vᵀ) with v the eigenvector of FᵀF of the
// smallest eigenvalue (cyclic Jacobi on the 3 x 3, kJacobi3Sweeps sweeps).
LG_HD void rank2(double f[9]) {
    double g[3][3], v[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            g[i][j] = f[i] * f[j] + f[3 + i] * f[3 + j] + f[6 + i] * f[6 + j];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobi3Sweeps; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            constexpr int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
            const int p = P[pq], q = Q[pq];
            double c, s;
            jacobi_cs(g[p][p], g[q][q], g[p][q], c, s);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double gp = g[k][p], gq = g[k][q], vp = v[k][p], vq = v[k][q];
                g[k][p] = c * gp - s * gq, g[k][q] = s * gp + c * gq;
                v[k][p] = c * vp - s * vq, v[k][q] = s * vp + c * vq;
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double gp = g[p][k], gq = g[q][k];
                g[p][k] = c * gp - s * gq, g[q][k] = s * gp + c * gq;
            }
        }
    }
    const bool m1 = g[1][1] < g[0][0];
    const double e01 = m1 ? g[1][1] : g[0][0];
    const bool m2 = g[2][2] < e01;
    double w[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) w[k] = m2 ? v[k][2] : (m1 ? v[k][1] : v[k][0]);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double fw = f[3 * r] * w[0] + f[3 * r + 1] * w[1] + f[3 * r + 2] * w[2];
#pragma unroll
        for (int k = 0; k < 3; ++k) f[3 * r + k] -= fw * w[k];
    }
}

// T1ᵀ F T0 in fp64 with each image's (cx, cy, s), unit Frobenius norm; false where not finite or zero.
LG_HD bool denormalise64(const double fn[9], double cx0, double cy0, double s0, double cx1, double cy1, double s1,
                         double out[9]) {
    double m[9], ss = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        m[3 * r] = s0 * fn[3 * r];
        m[3 * r + 1] = s0 * fn[3 * r + 1];
        m[3 * r + 2] = fn[3 * r + 2] - s0 * (cx0 * fn[3 * r] + cy0 * fn[3 * r + 1]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        out[k] = s1 * m[k];
        out[3 + k] = s1 * m[3 + k];
        out[6 + k] = m[6 + k] - s1 * (cx1 * m[k] + cy1 * m[3 + k]);
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) ss += out[i] * out[i];
    const double inv = 1.0 / sqrt(ss);
    const bool ok = ss > 0.0 && ss < INFINITY && inv < INFINITY;
#pragma unroll
    for (int i = 0; i < 9; ++i) out[i] = ok ? out[i] * inv : 0.0;
    return ok;
}

// One inlier's share of the upper triangle of the normal matrix (45 entries, row by row), normalised points.
// The fundamental matrix: one row (x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1).
LG_HD void normal_accumulate_f(double acc[45], double x0, double y0, double x1, double y1) {
    const double row[9] = {x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, 1.0};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) acc[e] = fma(row[i], row[j], acc[e]), ++e;
}

// The homography: the row pair of solve4; products with a structural zero are left out (they add nothing), so
// entries (0..2) x (3..5) of the matrix stay exactly zero.
LG_HD void normal_accumulate_h(double acc[45], double x0, double y0, double x1, double y1) {
    const double ra[9] = {-x0, -y0, -1.0, 0.0, 0.0, 0.0, x1 * x0, x1 * y0, x1};
    const double rb[9] = {0.0, 0.0, 0.0, -x0, -y0, -1.0, y1 * x0, y1 * y0, y1};
    int e = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = i; j < 9; ++j) {
            if (!(i >= 3 && i < 6) && !(j >= 3 && j < 6)) acc[e] = fma(ra[i], ra[j], acc[e]);
            if (!(i < 3) && !(j < 3)) acc[e] = fma(rb[i], rb[j], acc[e]);
            ++e;
        }
}

}  // namespace lg_geom
