// The homography's per-lane statements (csrc/lightglue_geometry_math.h is __host__ __device__) as a host library
// for tools/homography_host_check.py: the 4-sample, the 4-point solve in double or in float, the transfer-error
// test. No GPU, no HIP: c++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off.
#include <stdint.h>

#include "lightglue_geometry_math.h"

using namespace lg_geom;

namespace {

// Hartley normalisation over all points, sums in ascending order in double.
NormT<double> hartley(const float* pts, int count) {
    double c[4] = {0, 0, 0, 0}, d[2] = {0, 0};
    for (int k = 0; k < count; ++k)
        for (int i = 0; i < 4; ++i) c[i] += (double)pts[4 * k + i];
    for (int i = 0; i < 4; ++i) c[i] /= count;
    for (int k = 0; k < count; ++k) {
        const double ax = pts[4 * k] - c[0], ay = pts[4 * k + 1] - c[1], bx = pts[4 * k + 2] - c[2], by = pts[4 * k + 3] - c[3];
        d[0] += sqrt(ax * ax + ay * ay), d[1] += sqrt(bx * bx + by * by);
    }
    return NormT<double>{c[0], c[1], 1.4142135623730951 / (d[0] / count), c[2], c[3], 1.4142135623730951 / (d[1] / count)};
}

template <typename T>
int solve_one(const float* pts, const NormT<double>& n, const int32_t* idx, int count, float cand[9]) {
    const NormT<T> t{(T)n.cx0, (T)n.cy0, (T)n.s0, (T)n.cx1, (T)n.cy1, (T)n.s1};
    T x0[4], y0[4], x1[4], y1[4];
    for (int j = 0; j < 4; ++j) {
        int i = idx[j] < 0 ? 0 : (idx[j] > count - 1 ? count - 1 : idx[j]);
        x0[j] = ((T)pts[4 * i] - t.cx0) * t.s0, y0[j] = ((T)pts[4 * i + 1] - t.cy0) * t.s0;
        x1[j] = ((T)pts[4 * i + 2] - t.cx1) * t.s1, y1[j] = ((T)pts[4 * i + 3] - t.cy1) * t.s1;
    }
    return solve4(x0, y0, x1, y1, t, cand);
}

}  // namespace

extern "C" {

// pts [count, 4] = (x0, y0, x1, y1); samples [hypotheses, 4] -> cands [hypotheses, 9], num [hypotheses].
void host_solve4(int use_float, const float* pts, int count, const int32_t* samples, int hypotheses, float* cands, int32_t* num) {
    const NormT<double> n = hartley(pts, count);
    for (int h = 0; h < hypotheses; ++h)
        num[h] = use_float ? solve_one<float>(pts, n, samples + 4 * h, count, cands + 9 * h)
                           : solve_one<double>(pts, n, samples + 4 * h, count, cands + 9 * h);
}

void host_samples4(int32_t seed, int hypotheses, int count, int32_t* out) {
    for (int h = 0; h < hypotheses; ++h) sample<4>((uint32_t)seed, h, count, out + 4 * h);
}

// One refit round as ransac_finalize_kernel<HomographyModel> does it, serially: Hartley over the rows with
// mask != 0, the 45 sums of normal_accumulate_h, the round-robin Jacobi (the four rotations of a step computed
// from the matrix before the step, columns of A and V rotated, then rows of A), the eigenvector of the smallest
// diagonal entry, denormalise_h, rounded to fp32 with the sign rule. Returns 0 where the result is not finite.
int host_refit_h(const float* pts, const uint8_t* mask, int count, float out[9]) {
    double c[4] = {0, 0, 0, 0}, d[2] = {0, 0}, n = 0;
    for (int k = 0; k < count; ++k) {
        if (!mask[k]) continue;
        n += 1;
        for (int i = 0; i < 4; ++i) c[i] += (double)pts[4 * k + i];
    }
    for (int i = 0; i < 4; ++i) c[i] /= n;
    for (int k = 0; k < count; ++k) {
        if (!mask[k]) continue;
        const double ax = pts[4 * k] - c[0], ay = pts[4 * k + 1] - c[1], bx = pts[4 * k + 2] - c[2], by = pts[4 * k + 3] - c[3];
        d[0] += sqrt(ax * ax + ay * ay), d[1] += sqrt(bx * bx + by * by);
    }
    const double s[2] = {1.4142135623730951 / (d[0] / n), 1.4142135623730951 / (d[1] / n)};
    double acc[45];
    for (int e = 0; e < 45; ++e) acc[e] = 0.0;
    for (int k = 0; k < count; ++k) {
        if (!mask[k]) continue;
        normal_accumulate_h(acc, (pts[4 * k] - c[0]) * s[0], (pts[4 * k + 1] - c[1]) * s[0], (pts[4 * k + 2] - c[2]) * s[1],
                            (pts[4 * k + 3] - c[3]) * s[1]);
    }
    double am[81], vm[81];
    for (int e = 0; e < 45; ++e) {
        int i, j;
        tri_index(e, i, j);
        am[9 * i + j] = acc[e], am[9 * j + i] = acc[e];
    }
    for (int t = 0; t < 81; ++t) vm[t] = t / 9 == t % 9 ? 1.0 : 0.0;
    for (int step = 0; step < 9 * kJacobiSweeps; ++step) {
        double rot[4][2];
        int pp[4], qq[4];
        for (int g = 0; g < 4; ++g) {
            jacobi_pair(step, g, pp[g], qq[g]);
            jacobi_cs(am[9 * pp[g] + pp[g]], am[9 * qq[g] + qq[g]], am[9 * pp[g] + qq[g]], rot[g][0], rot[g][1]);
        }
        for (int g = 0; g < 4; ++g)
            for (int w = 0; w < 18; ++w) {
                double* m = w < 9 ? am : vm;
                const int k = w % 9;
                const double mp = m[9 * k + pp[g]], mq = m[9 * k + qq[g]];
                m[9 * k + pp[g]] = rot[g][0] * mp - rot[g][1] * mq, m[9 * k + qq[g]] = rot[g][1] * mp + rot[g][0] * mq;
            }
        for (int g = 0; g < 4; ++g)
            for (int k = 0; k < 9; ++k) {
                const double mp = am[9 * pp[g] + k], mq = am[9 * qq[g] + k];
                am[9 * pp[g] + k] = rot[g][0] * mp - rot[g][1] * mq, am[9 * qq[g] + k] = rot[g][1] * mp + rot[g][0] * mq;
            }
    }
    int lo = 0;
    for (int k = 1; k < 9; ++k) lo = am[10 * k] < am[10 * lo] ? k : lo;
    double hn[9], hd[9];
    for (int k = 0; k < 9; ++k) hn[k] = vm[9 * k + lo];
    const bool ok = denormalise_h(hn, c[0], c[1], s[0], c[2], c[3], s[1], hd);
    for (int k = 0; k < 9; ++k) out[k] = (float)hd[k];
    fix_sign(out);
    return ok ? 1 : 0;
}

void host_score_h(const float* pts, int count, const float* cands, int ncand, float thr2, int32_t* out) {
    for (int c = 0; c < ncand; ++c) {
        int n = 0;
        for (int k = 0; k < count; ++k)
            n += is_inlier_h(cands + 9 * c, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], thr2) ? 1 : 0;
        out[c] = n;
    }
}

}  // extern "C"
