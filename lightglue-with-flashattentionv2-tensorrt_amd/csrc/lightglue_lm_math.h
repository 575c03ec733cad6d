// lightglue_lm_math.h — the fp64 arithmetic the geometry refits share (csrc/lightglue_polish_math.h, the pose polish;
// csrc/lightglue_absolute_math.h, the absolute pose; csrc/lightglue_bundle_math.h, the bundle adjustment;
// csrc/lightglue_window_math.h, the sequence window): the pose and the camera, the polar step that enters a rotation
// and the Rodrigues formula that updates it, the packed sums of an N-parameter
// least-squares problem with their accumulation and their damped Cholesky step, the Levenberg-Marquardt rounds with
// their accept rule and λ schedule, and the 3 x 3 Cholesky factorisation. Each exists here once. The style is
// lightglue_geometry_math.h's: plain __host__ __device__ functions on values and small fixed-size arrays, every index a
// compile-time constant after unrolling, selection by selects, every loop with a compile-time bound.
#pragma once

#include "lightglue_geometry_math.h"

namespace lg_geom {

constexpr double kLambdaStart = 1e-3, kLambdaMin = 1e-12, kLambdaMax = 1e12;

LG_HD bool finite64(double v) { return fabs(v) < INFINITY; }  // (NaN: false)

LG_HD double sinc64(double x) { return x == 0.0 ? 1.0 : sin(x) / x; }

// out = [v]x m (row-major 3 x 3): column c of out is v x (column c of m).
LG_HD void cross_mul(const double v[3], const double m[9], double out[9]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        out[c] = v[1] * m[6 + c] - v[2] * m[3 + c];
        out[3 + c] = v[2] * m[c] - v[0] * m[6 + c];
        out[6 + c] = v[0] * m[3 + c] - v[1] * m[c];
    }
}

struct Pose {  // X_c = R X + t, R row-major
    double r[9], t[3];
};

struct Camera {  // (fx, fy, cx, cy) of the one camera
    float fx, fy, cx, cy;
};

// One Newton step of the polar iteration from m towards the rotations: out = m (3 I - mᵀ m) / 2 (the defect of a
// rotation rounded to fp32 falls from 1e-7 to 1e-14).
LG_HD void polar_step(const double m[9], double out[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double v = 0.0;  // (m (3 I - mᵀ m))[i][j]
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double g = m[k] * m[j] + m[3 + k] * m[3 + j] + m[6 + k] * m[6 + j];  // (mᵀ m)[k][j]
                v += m[3 * i + k] * ((k == j ? 3.0 : 0.0) - g);
            }
            out[3 * i + j] = 0.5 * v;
        }
}

// out = exp([ω]x) r by the Rodrigues formula, exp = I + (sin θ / θ) [ω]x + ((1 - cos θ) / θ²) [ω]x² with
// (1 - cos θ) / θ² = (sin(θ / 2) / (θ / 2))² / 2 (no cancellation at small θ); ω: the first three entries of the step.
LG_HD void rodrigues_update(const double r[9], const double* step, double out[9]) {
    const double w[3] = {step[0], step[1], step[2]};
    const double theta = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double ka = sinc64(theta), kh = sinc64(0.5 * theta), kb = 0.5 * kh * kh;
    double g[9], h[9];
    cross_mul(w, r, g);
    cross_mul(w, g, h);
#pragma unroll
    for (int k = 0; k < 9; ++k) out[k] = r[k] + ka * g[k] + kb * h[k];
}

// ---- the packed sums of a least-squares problem on N parameters -------------------------------------------------------
// JᵀJ's upper triangle row by row, Jᵀr, Σ r², the number of rows.
template <int N>
struct LmSums {
    static constexpr int kTri = 0, kGrad = N * (N + 1) / 2, kCost = kGrad + N, kRows = kCost + 1, kCount = kRows + 1;
};

// acc += one scalar residual's part, from its row j of the Jacobian: the triangle, the gradient and the cost (the
// number of rows is the caller's: a row may be several residuals).
template <int N>
LG_HD void lm_accumulate(double acc[LmSums<N>::kRows], double res, const double j[N]) {
    int e = LmSums<N>::kTri;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = a; b < N; ++b) acc[e] = fma(j[a], j[b], acc[e]), ++e;
#pragma unroll
    for (int a = 0; a < N; ++a) acc[LmSums<N>::kGrad + a] = fma(j[a], res, acc[LmSums<N>::kGrad + a]);
    acc[LmSums<N>::kCost] = fma(res, res, acc[LmSums<N>::kCost]);
}

// The Levenberg-Marquardt step of the sums: (JᵀJ + λ diag(JᵀJ)) δ = -Jᵀr by a Cholesky factorisation. False where a
// pivot is not positive or not finite (δ is then not to be used).
template <int N>
LG_HD bool lm_step(const double sums[LmSums<N>::kCount], double lambda, double delta[N]) {
    double l[N][N];
    int e = LmSums<N>::kTri;
#pragma unroll
    for (int a = 0; a < N; ++a)
#pragma unroll
        for (int b = a; b < N; ++b) l[b][a] = sums[e] * (a == b ? 1.0 + lambda : 1.0), ++e;
    bool ok = true;
#pragma unroll
    for (int c = 0; c < N; ++c) {
        double piv = l[c][c];
#pragma unroll
        for (int k = 0; k < c; ++k) piv = fma(-l[c][k], l[c][k], piv);
        ok = ok && piv > 0.0 && finite64(piv);  // (NaN: false)
        const double root = sqrt(piv), inv = 1.0 / root;
        l[c][c] = root;
#pragma unroll
        for (int r = c + 1; r < N; ++r) {
            double v = l[r][c];
#pragma unroll
            for (int k = 0; k < c; ++k) v = fma(-l[r][k], l[c][k], v);
            l[r][c] = v * inv;
        }
    }
    double y[N];
#pragma unroll
    for (int r = 0; r < N; ++r) {
        double v = -sums[LmSums<N>::kGrad + r];
#pragma unroll
        for (int k = 0; k < r; ++k) v = fma(-l[r][k], y[k], v);
        y[r] = v / l[r][r];
    }
#pragma unroll
    for (int r = N - 1; r >= 0; --r) {
        double v = y[r];
#pragma unroll
        for (int k = r + 1; k < N; ++k) v = fma(-l[k][r], delta[k], v);
        delta[r] = v / l[r][r];
        ok = ok && finite64(delta[r]);
    }
    return ok;
}

// A trial is accepted where its cost is finite and strictly lower; λ falls tenfold after an accepted round and rises
// tenfold after any other, within [kLambdaMin, kLambdaMax].
LG_HD bool lm_accept(double trial, double cost) { return finite64(trial) && trial < cost; }
LG_HD double lm_lambda(double lambda, bool taken) { return taken ? fmax(lambda * 0.1, kLambdaMin) : fmin(lambda * 10.0, kLambdaMax); }

struct LmUnobserved {
    LG_HD void operator()(int, const double*) const {}
};

// `rounds` rounds of Levenberg-Marquardt from the state st with its sums: update(st, δ, next) builds the trial state,
// pass(next, again) fills the trial's sums (one pass a round: they are the next round's where the trial is accepted),
// accepted(round, δ) sees each accepted round. st and sums leave as the last accepted.
template <int N, class State, class Pass, class Update, class Observer = LmUnobserved>
LG_HD void lm_rounds(State& st, double sums[LmSums<N>::kCount], int rounds, const Pass& pass, const Update& update,
                     const Observer& accepted = Observer()) {
    double lambda = kLambdaStart;
#pragma unroll 1
    for (int round = 0; round < rounds; ++round) {
        double delta[N];
        bool take = lm_step<N>(sums, lambda, delta);
        if (take) {  // (a rejected solve spares the pass)
            State next;
            double again[LmSums<N>::kCount];
            update(st, delta, next);
            pass(next, again);
            take = lm_accept(again[LmSums<N>::kCost], sums[LmSums<N>::kCost]);
            if (take) {
                st = next;
#pragma unroll
                for (int e = 0; e < LmSums<N>::kCount; ++e) sums[e] = again[e];
                accepted(round, delta);
            }
        }
        lambda = lm_lambda(lambda, take);
    }
}

// ---- the 3 x 3 Cholesky factorisation ---------------------------------------------------------------------------------
// a: a symmetric matrix's upper triangle (00 01 02 11 12 22) = L Lᵀ: L below the diagonal, the reciprocals of its
// diagonal and the three pivots. False where a pivot is not positive or not finite.
struct Chol3 {
    double l10, l20, l21, i00, i11, i22, p0, p1, p2;
};

LG_HD bool chol3(const double a[6], Chol3& c) {
    c.p0 = a[0];
    bool ok = c.p0 > 0.0 && finite64(c.p0);
    c.i00 = 1.0 / sqrt(c.p0);
    c.l10 = a[1] * c.i00, c.l20 = a[2] * c.i00;
    c.p1 = fma(-c.l10, c.l10, a[3]);
    ok = ok && c.p1 > 0.0 && finite64(c.p1);
    c.i11 = 1.0 / sqrt(c.p1);
    c.l21 = fma(-c.l20, c.l10, a[4]) * c.i11;
    c.p2 = fma(-c.l21, c.l21, fma(-c.l20, c.l20, a[5]));
    ok = ok && c.p2 > 0.0 && finite64(c.p2);
    c.i22 = 1.0 / sqrt(c.p2);
    return ok;
}

}  // namespace lg_geom
