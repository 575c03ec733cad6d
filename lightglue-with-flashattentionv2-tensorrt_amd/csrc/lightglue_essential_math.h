// lightglue_essential_math.h — the arithmetic of the calibrated five-point RANSAC (csrc/lightglue_essential.hip;
// include/lightglue_glue.h, "geometric verification"): the null space of the 5 x 9 system, the ten cubic
// constraints as a 10 x 20 matrix held five columns a lane by the four lanes of a hypothesis, its elimination, the
// degree-10 polynomial in z and its real roots, a candidate from a root, E <-> F, the projection to the essential
// manifold and the pose with its cheirality test. All fp64 (the fp32 7-point solve was measured and dropped,
// DESIGN §3; a degree-10 polynomial is worse). The style is lightglue_geometry_math.h's: plain __host__ __device__
// functions on values and small fixed-size arrays, every index a compile-time constant after unrolling, pivoting
// and selection by selects, every loop with a compile-time bound.
//
// E = x X + y Y + z Z + W over the null-space basis. The columns of the 10 x 20 matrix are the monomials
//   x³ y³ x²y xy² x²z x² y²z y² xyz xy | xz² xz x yz² yz y z³ z² z 1
// (Nistér's order): after Gauss-Jordan on the left ten, rows 4..9 (x²z, x², y²z, y², xyz, xy) pair up into three
// equations row(2i) - z row(2i+1), each x p3(z) + y q3(z) + r4(z) = 0; the determinant of that 3 x 3 is the
// degree-10 polynomial, and (x, y, 1) its null vector at a root.
#pragma once

#include "lightglue_geometry_math.h"

namespace lg_geom {

constexpr int kMinInliersE = 5;     // an essential matrix needs 5 correspondences (its refit 8: kMinInliers)
constexpr int kCands5 = 10;         // candidates a hypothesis at most
constexpr int kRootBisections = 36; // per bracket: the bracket's width falls to 2^-35 of the root bound
constexpr int kRootNewton = 5;      // then Newton steps that may not leave the bracket
constexpr double kRootBoundMax = 1e9;
constexpr int kSvd3Sweeps = 8;      // one-sided Jacobi on a 3 x 3

struct Intrinsics {  // (fx, fy, cx, cy) of image 0 and of image 1
    double fx0, fy0, cx0, cy0, fx1, fy1, cx1, cy1;
};

LG_HD bool intrinsics_ok(const Intrinsics& k) {
    const double a[8] = {k.fx0, k.fy0, k.cx0, k.cy0, k.fx1, k.fy1, k.cx1, k.cy1};
    bool ok = k.fx0 > 0.0 && k.fy0 > 0.0 && k.fx1 > 0.0 && k.fy1 > 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) ok = ok && fabs(a[i]) < INFINITY;
    return ok;
}

// The sign rule and unit Frobenius norm in double; false where zero or not finite (e is then zeros).
LG_HD bool canonical9(double e[9]) {
    double ss = 0.0, best = fabs(e[0]), val = e[0];
#pragma unroll
    for (int i = 0; i < 9; ++i) ss = fma(e[i], e[i], ss);
#pragma unroll
    for (int i = 1; i < 9; ++i) {
        const bool up = fabs(e[i]) > best;
        best = up ? fabs(e[i]) : best, val = up ? e[i] : val;
    }
    const double inv = (val < 0.0 ? -1.0 : 1.0) / sqrt(ss);
    const bool ok = ss > 0.0 && ss < INFINITY && fabs(inv) < INFINITY;
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = ok ? e[i] * inv : 0.0;
    return ok;
}

// F = K1⁻ᵀ E K0⁻¹ at unit norm with the sign rule, rounded to fp32: what a candidate is scored with in pixels.
// False where the result is zero or not finite (f is then zeros).
LG_HD bool fundamental_of_essential(const double e[9], const Intrinsics& k, float f[9]) {
    double m[9], g[9];
    const double ix0 = 1.0 / k.fx0, iy0 = 1.0 / k.fy0, ix1 = 1.0 / k.fx1, iy1 = 1.0 / k.fy1;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        m[3 * r] = e[3 * r] * ix0;
        m[3 * r + 1] = e[3 * r + 1] * iy0;
        m[3 * r + 2] = e[3 * r + 2] - (k.cx0 * m[3 * r] + k.cy0 * m[3 * r + 1]);
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        g[c] = m[c] * ix1;
        g[3 + c] = m[3 + c] * iy1;
        g[6 + c] = m[6 + c] - (k.cx1 * g[c] + k.cy1 * g[3 + c]);
    }
    const bool ok = canonical9(g);
#pragma unroll
    for (int i = 0; i < 9; ++i) f[i] = (float)g[i];
    fix_sign(f);
    return ok;
}

// ---- the null space of the 5 x 9 system ----------------------------------------------------------------------------
// Rows (x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1) in camera coordinates; Gauss-Jordan with partial (row)
// pivoting on columns 0..4; basis[j] = (-B[:, j], e_j) for the reduced system [I | B], j = 0..3 (X, Y, Z, W). False
// where a pivot is below kPivotEps (NaN included).
LG_HD bool null_space5(const double x0[5], const double y0[5], const double x1[5], const double y1[5], double basis[4][9]) {
    double a[5][9];
#pragma unroll
    for (int r = 0; r < 5; ++r) {
        a[r][0] = x1[r] * x0[r], a[r][1] = x1[r] * y0[r], a[r][2] = x1[r];
        a[r][3] = y1[r] * x0[r], a[r][4] = y1[r] * y0[r], a[r][5] = y1[r];
        a[r][6] = x0[r], a[r][7] = y0[r], a[r][8] = 1.0;
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        double best = fabs(a[c][c]);
        int piv = c;
#pragma unroll
        for (int r = c + 1; r < 5; ++r) {
            const double v = fabs(a[r][c]);
            const bool up = v > best;
            best = up ? v : best, piv = up ? r : piv;
        }
        ok = ok && best >= (double)kPivotEps;  // (NaN: false)
#pragma unroll
        for (int r = c + 1; r < 5; ++r) {
            const bool sw = piv == r;
#pragma unroll
            for (int k = c; k < 9; ++k) {
                const double u = a[c][k], v = a[r][k];
                a[c][k] = sw ? v : u, a[r][k] = sw ? u : v;
            }
        }
        const double inv = 1.0 / a[c][c];
#pragma unroll
        for (int k = c + 1; k < 9; ++k) a[c][k] *= inv;
#pragma unroll
        for (int r = 0; r < 5; ++r) {
            if (r == c) continue;
            const double f = a[r][c];
#pragma unroll
            for (int k = c + 1; k < 9; ++k) a[r][k] = fma(-f, a[c][k], a[r][k]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int r = 0; r < 5; ++r) basis[j][r] = -a[r][5 + j];
#pragma unroll
        for (int r = 5; r < 9; ++r) basis[j][r] = r == 5 + j ? 1.0 : 0.0;
    }
    // orthonormal (modified Gram-Schmidt; the four are independent by their last entries): the degree-10 polynomial
    // of the raw basis loses real roots to rounding (two hypotheses of 748 on the test scenes, residuals of det E up
    // to 5e-3 on others), that of an orthonormal one does not
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int i = 0; i < j; ++i) {
            double d = 0.0;
#pragma unroll
            for (int r = 0; r < 9; ++r) d = fma(basis[i][r], basis[j][r], d);
#pragma unroll
            for (int r = 0; r < 9; ++r) basis[j][r] = fma(-d, basis[i][r], basis[j][r]);
        }
        double ss = 0.0;
#pragma unroll
        for (int r = 0; r < 9; ++r) ss = fma(basis[j][r], basis[j][r], ss);
        const double inv = 1.0 / sqrt(ss);
#pragma unroll
        for (int r = 0; r < 9; ++r) basis[j][r] *= inv;
    }
    return ok;
}

// ---- polynomials in (x, y, z) as arrays over the three exponents ---------------------------------------------------
struct Poly1 { double c[2][2][2]; };
struct Poly2 { double c[3][3][3]; };
struct Poly3 { double c[4][4][4]; };

// o += s a b for two polynomials of degree 1 (entries past the degree are never touched)
LG_HD void pmul11(const Poly1& a, const Poly1& b, double s, Poly2& o) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int ax = i >> 2, ay = (i >> 1) & 1, az = i & 1;
        if (ax + ay + az > 1) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int bx = j >> 2, by = (j >> 1) & 1, bz = j & 1;
            if (bx + by + bz > 1) continue;
            o.c[ax + bx][ay + by][az + bz] = fma(s * a.c[ax][ay][az], b.c[bx][by][bz], o.c[ax + bx][ay + by][az + bz]);
        }
    }
}

// o += a b for a polynomial of degree 2 and one of degree 1
LG_HD void pmul21(const Poly2& a, const Poly1& b, Poly3& o) {
#pragma unroll
    for (int i = 0; i < 27; ++i) {
        const int ax = i / 9, ay = (i / 3) % 3, az = i % 3;
        if (ax + ay + az > 2) continue;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int bx = j >> 2, by = (j >> 1) & 1, bz = j & 1;
            if (bx + by + bz > 1) continue;
            o.c[ax + bx][ay + by][az + bz] = fma(a.c[ax][ay][az], b.c[bx][by][bz], o.c[ax + bx][ay + by][az + bz]);
        }
    }
}

LG_HD void pzero(Poly2& p) {
#pragma unroll
    for (int i = 0; i < 27; ++i) p.c[i / 9][(i / 3) % 3][i % 3] = 0.0;
}
LG_HD void pzero(Poly3& p) {
#pragma unroll
    for (int i = 0; i < 64; ++i) p.c[i / 16][(i / 4) % 4][i % 4] = 0.0;
}

// Entry k of E(x, y, z) over the basis
LG_HD Poly1 entry_poly(const double basis[4][9], int k) {
    Poly1 p;
#pragma unroll
    for (int i = 0; i < 8; ++i) p.c[i >> 2][(i >> 1) & 1][i & 1] = 0.0;
    p.c[1][0][0] = basis[0][k], p.c[0][1][0] = basis[1][k], p.c[0][0][1] = basis[2][k], p.c[0][0][0] = basis[3][k];
    return p;
}

// The lane's five of the twenty monomial coefficients of a cubic: columns 5 sub .. 5 sub + 4 of the order above.
LG_HD void take_columns(const Poly3& p, int sub, double out[5]) {
    constexpr int EX[20] = {3, 0, 2, 1, 2, 2, 0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
    constexpr int EY[20] = {0, 3, 1, 2, 0, 0, 2, 2, 1, 1, 0, 0, 0, 1, 1, 1, 0, 0, 0, 0};
    constexpr int EZ[20] = {0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 2, 1, 0, 2, 1, 0, 3, 2, 1, 0};
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double c0 = p.c[EX[j]][EY[j]][EZ[j]], c1 = p.c[EX[5 + j]][EY[5 + j]][EZ[5 + j]];
        const double c2 = p.c[EX[10 + j]][EY[10 + j]][EZ[10 + j]], c3 = p.c[EX[15 + j]][EY[15 + j]][EZ[15 + j]];
        out[j] = sub == 0 ? c0 : (sub == 1 ? c1 : (sub == 2 ? c2 : c3));
    }
}

// The lane's slice a[10][5] of the constraint matrix: row 0 det E, row 1 + 3 i + j entry (i, j) of
// (2 E Eᵀ - tr(E Eᵀ) I) E, by generic polynomial products.
LG_HD void fill_slice(const double basis[4][9], int sub, double a[10][5]) {
    Poly1 e[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = entry_poly(basis, k);
    {   // det E = e0 (e4 e8 - e5 e7) - e1 (e3 e8 - e5 e6) + e2 (e3 e7 - e4 e6)
        Poly3 d;
        pzero(d);
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            constexpr int A[3] = {0, 1, 2}, B[3] = {4, 5, 3}, C[3] = {8, 6, 7}, D[3] = {5, 3, 4}, F[3] = {7, 8, 6};
            Poly2 m;
            pzero(m);
            pmul11(e[B[t]], e[C[t]], 1.0, m);
            pmul11(e[D[t]], e[F[t]], -1.0, m);
            pmul21(m, e[A[t]], d);
        }
        take_columns(d, sub, a[0]);
    }
    Poly2 tr;
    pzero(tr);
#pragma unroll
    for (int k = 0; k < 9; ++k) pmul11(e[k], e[k], 1.0, tr);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Poly2 lam[3];  // row i of 2 E Eᵀ - tr I
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            pzero(lam[k]);
#pragma unroll
            for (int m = 0; m < 3; ++m) pmul11(e[3 * i + m], e[3 * k + m], 2.0, lam[k]);
            if (k == i) {
#pragma unroll
                for (int q = 0; q < 27; ++q) {
                    if (q / 9 + (q / 3) % 3 + q % 3 <= 2) lam[k].c[q / 9][(q / 3) % 3][q % 3] -= tr.c[q / 9][(q / 3) % 3][q % 3];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            Poly3 c;
            pzero(c);
#pragma unroll
            for (int k = 0; k < 3; ++k) pmul21(lam[k], e[3 * k + j], c);
            take_columns(c, sub, a[1 + 3 * i + j]);
        }
    }
}

// Step C (0..9) of the Gauss-Jordan elimination of the 10 x 20 matrix on a lane's slice: col is column C of the
// whole matrix before the step (every lane of the hypothesis gets it from the lane that holds it); partial (row)
// pivoting by selects. Returns the pivot's magnitude (0 or NaN: the slice is then not finite).
template <int C>
LG_HD double slice_step(double a[10][5], double col[10]) {
    double best = fabs(col[C]);
    int piv = C;
#pragma unroll
    for (int r = C + 1; r < 10; ++r) {
        const double v = fabs(col[r]);
        const bool up = v > best;
        best = up ? v : best, piv = up ? r : piv;
    }
#pragma unroll
    for (int r = C + 1; r < 10; ++r) {
        const bool sw = piv == r;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const double u = a[C][k], v = a[r][k];
            a[C][k] = sw ? v : u, a[r][k] = sw ? u : v;
        }
        const double u = col[C], v = col[r];
        col[C] = sw ? v : u, col[r] = sw ? u : v;
    }
    const double inv = 1.0 / col[C];
#pragma unroll
    for (int k = 0; k < 5; ++k) a[C][k] *= inv;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r == C) continue;
#pragma unroll
        for (int k = 0; k < 5; ++k) a[r][k] = fma(-col[r], a[C][k], a[r][k]);
    }
    return best;
}

// ---- the degree-10 polynomial --------------------------------------------------------------------------------------
template <int DA, int DB>
LG_HD void mul_add(const double a[DA + 1], const double b[DB + 1], double s, double o[DA + DB + 1]) {
#pragma unroll
    for (int i = 0; i <= DA; ++i)
#pragma unroll
        for (int j = 0; j <= DB; ++j) o[i + j] = fma(s * a[i], b[j], o[i + j]);
}

// The three equations' coefficient polynomials in z (lowest power first) from rows 4..9 of the reduced right
// block rhs[6][10] (columns xz² xz x yz² yz y z³ z² z 1): eq[i] = {x: degree 3, y: degree 3, 1: degree 4}.
struct Eq3 {
    double x[4], y[4], c[5];
};

LG_HD Eq3 equation(const double hi[10], const double lo[10]) {  // hi - z lo
    Eq3 q;
    q.x[0] = hi[2], q.x[1] = hi[1] - lo[2], q.x[2] = hi[0] - lo[1], q.x[3] = -lo[0];
    q.y[0] = hi[5], q.y[1] = hi[4] - lo[5], q.y[2] = hi[3] - lo[4], q.y[3] = -lo[3];
    q.c[0] = hi[9], q.c[1] = hi[8] - lo[9], q.c[2] = hi[7] - lo[8], q.c[3] = hi[6] - lo[7], q.c[4] = -lo[6];
    return q;
}

// det of the 3 x 3 of polynomials: c[0..10], lowest power first.
LG_HD void determinant10(const Eq3 q[3], double c[11]) {
#pragma unroll
    for (int i = 0; i < 11; ++i) c[i] = 0.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {  // the constant column of row t times the minor of the other two rows' (x, y)
        constexpr int A[3] = {1, 0, 0}, B[3] = {2, 2, 1};
        double m[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) m[i] = 0.0;
        mul_add<3, 3>(q[A[t]].x, q[B[t]].y, 1.0, m);
        mul_add<3, 3>(q[A[t]].y, q[B[t]].x, -1.0, m);
        mul_add<6, 4>(m, q[t].c, t == 1 ? -1.0 : 1.0, c);
    }
}

constexpr double falling(int n, int k) {  // n (n - 1) .. (n - k + 1)
    double f = 1.0;
    for (int i = 0; i < k; ++i) f *= (double)(n - i);
    return f;
}

template <int K>
LG_HD double horner(const double q[K + 1], double x) {
    double v = q[K];
#pragma unroll
    for (int i = K - 1; i >= 0; --i) v = fma(v, x, q[i]);
    return v;
}

template <int K>
LG_HD double horner_derivative(const double q[K + 1], double x) {
    double v = (double)K * q[K];
#pragma unroll
    for (int i = K - 1; i >= 1; --i) v = fma(v, x, (double)i * q[i]);
    return v;
}

// The real roots of the (10 - K)-th derivative of c (degree K) between the breakpoints (-bound, prev[0..K-2],
// +bound), prev ascending: the roots of the next derivative, between which this one is monotone. Bracket i has a
// root where the signs at its ends differ: kRootBisections bisections, then kRootNewton Newton steps kept inside
// the bracket. out[i] is the root, or the bracket's left end where there is none (out stays ascending); has[i] says
// which. The K brackets advance together in one loop.
template <int K>
LG_HD void derivative_roots(const double c[11], double bound, const double prev[10], double out[10], bool has[10]) {
    constexpr int D = 10 - K;
    double q[K + 1];
#pragma unroll
    for (int j = 0; j <= K; ++j) q[j] = c[j + D] * falling(j + D, D);
    double lo[K], hi[K];
    bool up[K];  // the sign at the left end
#pragma unroll
    for (int i = 0; i < K; ++i) {
        lo[i] = i == 0 ? -bound : prev[i - 1];
        hi[i] = i == K - 1 ? bound : prev[i];
        out[i] = lo[i];
        up[i] = horner<K>(q, lo[i]) > 0.0;
        has[i] = up[i] != (horner<K>(q, hi[i]) > 0.0);
    }
#pragma unroll 1
    for (int it = 0; it < kRootBisections; ++it) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double mid = 0.5 * (lo[i] + hi[i]);
            const bool left = (horner<K>(q, mid) > 0.0) == up[i];
            lo[i] = left ? mid : lo[i], hi[i] = left ? hi[i] : mid;
        }
    }
    double x[K];
#pragma unroll
    for (int i = 0; i < K; ++i) x[i] = 0.5 * (lo[i] + hi[i]);
#pragma unroll 1
    for (int it = 0; it < kRootNewton; ++it) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const double nx = x[i] - horner<K>(q, x[i]) / horner_derivative<K>(q, x[i]);
            x[i] = nx >= lo[i] && nx <= hi[i] ? nx : x[i];  // (NaN: stays)
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i) out[i] = has[i] ? x[i] : out[i];
}

template <int K>
LG_HD void root_levels(const double c[11], double bound, double r[10], bool has[10]) {
    if constexpr (K > 1) root_levels<K - 1>(c, bound, r, has);
    double prev[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) prev[i] = r[i];
    derivative_roots<K>(c, bound, prev, r, has);
}

// The real roots of c[0] + c[1] z + .. + c[10] z^10 within the Cauchy bound 1 + max |c[i] / c[10]| (at most
// kRootBoundMax): root[i] where has[i], in ascending order with gaps. The brackets are the roots of the successive
// derivatives, from the ninth (linear) up. False where the bound is not finite.
LG_HD bool real_roots10(const double c[11], double root[10], bool has[10]) {
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 10; ++i) big = fmax(big, fabs(c[i] / c[10]));
    const bool ok = big < INFINITY;  // (NaN: false)
    const double bound = fmin(1.0 + big, kRootBoundMax);
#pragma unroll
    for (int i = 0; i < 10; ++i) root[i] = 0.0, has[i] = false;
    root_levels<10>(c, ok ? bound : 1.0, root, has);
#pragma unroll
    for (int i = 0; i < 10; ++i) has[i] = has[i] && ok;
    return ok;
}

// The candidate at a root z: (x, y, 1) is the null vector of the 3 x 3 at z, the cross product of the two rows
// whose cross product is the longest; E = x X + y Y + z Z + W, canonical. False where not finite (e zeros).
LG_HD bool candidate5(const double basis[4][9], const Eq3 q[3], double z, double e[9]) {
    double b[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i) b[i][0] = horner<3>(q[i].x, z), b[i][1] = horner<3>(q[i].y, z), b[i][2] = horner<4>(q[i].c, z);
    double n[3] = {0.0, 0.0, 0.0}, len = -1.0;
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        constexpr int A[3] = {0, 0, 1}, B[3] = {1, 2, 2};
        const double* u = b[A[t]];
        const double* v = b[B[t]];
        const double m0 = u[1] * v[2] - u[2] * v[1], m1 = u[2] * v[0] - u[0] * v[2], m2 = u[0] * v[1] - u[1] * v[0];
        const double l = m0 * m0 + m1 * m1 + m2 * m2;
        const bool take = l > len;
        n[0] = take ? m0 : n[0], n[1] = take ? m1 : n[1], n[2] = take ? m2 : n[2], len = take ? l : len;
    }
    const double x = n[0] / n[2], y = n[1] / n[2];
#pragma unroll
    for (int k = 0; k < 9; ++k) e[k] = fma(x, basis[0][k], fma(y, basis[1][k], fma(z, basis[2][k], basis[3][k])));
    return canonical9(e);
}

// ---- the essential manifold and the pose ---------------------------------------------------------------------------
// One-sided Jacobi SVD of a 3 x 3 (row-major): e = U diag(s) Vᵀ, s descending, then det U = det V = +1 by
// u3 = u1 x u2, v3 = v1 x v2 (the third singular value is the one dropped). u, v row-major with the vectors as
// columns. False where the second singular value is zero or anything is not finite.
LG_HD bool svd3(const double e[9], double u[9], double v[9]) {
    double a[3][3], w[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) a[i][j] = e[3 * i + j], w[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kSvd3Sweeps; ++sweep) {
#pragma unroll
        for (int pq = 0; pq < 3; ++pq) {
            constexpr int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
            const int p = P[pq], q = Q[pq];
            const double al = a[0][p] * a[0][p] + a[1][p] * a[1][p] + a[2][p] * a[2][p];
            const double be = a[0][q] * a[0][q] + a[1][q] * a[1][q] + a[2][q] * a[2][q];
            const double ga = a[0][p] * a[0][q] + a[1][p] * a[1][q] + a[2][p] * a[2][q];
            double c, s;
            jacobi_cs(al, be, ga, c, s);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double ap = a[k][p], aq = a[k][q], wp = w[k][p], wq = w[k][q];
                a[k][p] = c * ap - s * aq, a[k][q] = s * ap + c * aq;
                w[k][p] = c * wp - s * wq, w[k][q] = s * wp + c * wq;
            }
        }
    }
    double n[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) n[j] = a[0][j] * a[0][j] + a[1][j] * a[1][j] + a[2][j] * a[2][j];
#pragma unroll
    for (int pass = 0; pass < 3; ++pass) {  // descending: (0, 1), (1, 2), (0, 1)
        const int p = pass == 1 ? 1 : 0, q = p + 1;
        const bool sw = n[q] > n[p];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double ap = a[k][p], aq = a[k][q], wp = w[k][p], wq = w[k][q];
            a[k][p] = sw ? aq : ap, a[k][q] = sw ? ap : aq, w[k][p] = sw ? wq : wp, w[k][q] = sw ? wp : wq;
        }
        const double np = n[p], nq = n[q];
        n[p] = sw ? nq : np, n[q] = sw ? np : nq;
    }
    const double i0 = 1.0 / sqrt(n[0]), i1 = 1.0 / sqrt(n[1]);
    const bool ok = n[1] > 0.0 && n[0] < INFINITY && i0 < INFINITY && i1 < INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) u[3 * k] = a[k][0] * i0, u[3 * k + 1] = a[k][1] * i1, v[3 * k] = w[k][0], v[3 * k + 1] = w[k][1];
    u[2] = u[3] * u[7] - u[6] * u[4], u[5] = u[6] * u[1] - u[0] * u[7], u[8] = u[0] * u[4] - u[3] * u[1];
    v[2] = v[3] * v[7] - v[6] * v[4], v[5] = v[6] * v[1] - v[0] * v[7], v[8] = v[0] * v[4] - v[3] * v[1];
    return ok;
}

// The nearest essential matrix: the singular values become (1, 1, 0); canonical. False where svd3 is.
LG_HD bool project_essential(double e[9]) {
    double u[9], v[9];
    const bool ok = svd3(e, u, v);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) e[3 * i + j] = u[3 * i] * v[3 * j] + u[3 * i + 1] * v[3 * j + 1];
    return canonical9(e) && ok;
}

// Pose candidate i (0..3) of E = U diag(1, 1, 0) Vᵀ: R = U W Vᵀ (i < 2) or U Wᵀ Vᵀ, t = +u3 (i even) or -u3; W the
// quarter turn about z, so U W Vᵀ = u2 v1ᵀ - u1 v2ᵀ + u3 v3ᵀ.
LG_HD void pose_candidate(const double u[9], const double v[9], int i, double r[9], double t[3]) {
    const double sg = i < 2 ? 1.0 : -1.0, st = (i & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int b = 0; b < 3; ++b)
            r[3 * a + b] = sg * (u[3 * a + 1] * v[3 * b] - u[3 * a] * v[3 * b + 1]) + u[3 * a + 2] * v[3 * b + 2];
        t[a] = st * u[3 * a + 2];
    }
}

// Whether the correspondence (camera coordinates) triangulates in front of both cameras under X1 = R X0 + t: the
// least-squares depths (d0, d1) of d0 R a - d1 b = -t for the rays a = (q0, 1), b = (q1, 1), both positive.
LG_HD bool in_front(const double r[9], const double t[3], double x0, double y0, double x1, double y1) {
    const double a0 = r[0] * x0 + r[1] * y0 + r[2], a1 = r[3] * x0 + r[4] * y0 + r[5], a2 = r[6] * x0 + r[7] * y0 + r[8];
    const double aa = a0 * a0 + a1 * a1 + a2 * a2, bb = x1 * x1 + y1 * y1 + 1.0, ab = a0 * x1 + a1 * y1 + a2;
    const double at = a0 * t[0] + a1 * t[1] + a2 * t[2], bt = x1 * t[0] + y1 * t[1] + t[2];
    const double det = aa * bb - ab * ab;
    const double d0 = (ab * bt - bb * at) / det, d1 = (aa * bt - ab * at) / det;
    return d0 > 0.0 && d1 > 0.0;  // (NaN: false)
}

}  // namespace lg_geom
