// The pose polish's and the triangulation's statements (csrc/lightglue_polish_math.h is __host__ __device__) as a
// host library for tools/polish_host_check.py: pose_polish_kernel for one pair with the workgroup's rows run
// serially (one accumulator where the kernel has a tree: the order of the sums differs, the statements do not), and
// triangulate_kernel's row. No GPU, no HIP: c++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off.
#include <stdint.h>

#include "lightglue_polish_math.h"

using namespace lg_geom;

namespace {

Intrinsics intrinsics_of(const float* k) {
    return Intrinsics{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]};
}

void camera(const float* q, const Intrinsics& k, double c[4]) {
    c[0] = ((double)q[0] - k.cx0) / k.fx0, c[1] = ((double)q[1] - k.cy0) / k.fy0;
    c[2] = ((double)q[2] - k.cx1) / k.fx1, c[3] = ((double)q[3] - k.cy1) / k.fy1;
}

// polish_pass: first also defines fixed[].
void pass(const PolishPose& q, const PolishWeights& pw, const Intrinsics& kk, const float* pts, const uint8_t* mask, uint8_t* fixed,
          int count, bool first, double sums[kPolishSums]) {
    PolishState st;
    polish_derive(q, st);
    for (int e = 0; e < kPolishSums; ++e) sums[e] = 0.0;
    for (int k = 0; k < count; ++k) {
        if (!(first ? mask[k] : fixed[k])) continue;
        double c[4], j[5];
        camera(pts + 4 * k, kk, c);
        const double s = sampson_row(st, pw, c[0], c[1], c[2], c[3], j);
        if (first) {
            fixed[k] = finite64(s) ? 1 : 0;
            if (!fixed[k]) continue;
        }
        polish_accumulate(sums, s, j);
    }
}

int count_front(const double r[9], const double t[3], const float* pts, const uint8_t* mask, int count, const Intrinsics& kk) {
    int n = 0;
    for (int k = 0; k < count; ++k) {
        if (!mask[k]) continue;
        double c[4];
        camera(pts + 4 * k, kk, c);
        n += in_front(r, t, c[0], c[1], c[2], c[3]) ? 1 : 0;
    }
    return n;
}

}  // namespace

extern "C" {

// pose_polish_kernel for one pair: pts [count, 4] = (x0, y0, x1, y1) in pixels, intrinsics [8], r [9], t [3] fp32,
// inliers [count], valid -> e, r_out [9], t_out [3] fp32, inliers_out [count], out = (num_inliers, num_front, kept),
// cost [2] fp32, steps [iterations] (the length of each round's δ in radians, -1 where the round was rejected).
void host_polish(const float* pts, int count, const float* intrinsics, const float* r, const float* t, const uint8_t* inliers,
                 int valid_in, float threshold, int iterations, float* e_out, float* r_out, float* t_out, uint8_t* inliers_out,
                 int32_t* out, float* cost, double* steps) {
    const Intrinsics kk = intrinsics_of(intrinsics);
    const float thr2 = threshold * threshold;
    const bool valid = valid_in != 0, staged = valid && intrinsics_ok(kk);
    PolishPose st;
    const bool pose_ok = polish_enter(r, t, st);
    const PolishWeights pw = polish_weights(kk);
    uint8_t* mask = new uint8_t[3 * (count + 1)];
    uint8_t* fixed = mask + count + 1;
    uint8_t* trial = fixed + count + 1;
    int n_in = 0, n_new = 0, front = 0;
    double cost0 = 0.0, cost1 = 0.0;
    bool kept = false;
    float eo[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < count; ++k) mask[k] = inliers[k] ? 1 : 0, fixed[k] = 0, n_in += valid ? mask[k] : 0;
    for (int i = 0; i < iterations; ++i) steps[i] = -1.0;
    double rd[9], td[3];
    for (int k = 0; k < 9; ++k) rd[k] = (double)r[k];
    for (int k = 0; k < 3; ++k) td[k] = (double)t[k];
    if (staged) {
        if (pose_ok) {
            double sums[kPolishSums];
            pass(st, pw, kk, pts, mask, fixed, count, true, sums);
            cost0 = cost1 = sums[20];
            if ((int)sums[21] >= kMinPolishRows && finite64(cost0)) {
                double lambda = kLambdaStart;
                for (int round = 0; round < iterations; ++round) {
                    double delta[5];
                    bool take = polish_step(sums, lambda, delta);
                    if (take) {
                        PolishPose next;
                        double again[kPolishSums];
                        polish_update(st, delta, next);
                        pass(next, pw, kk, pts, mask, fixed, count, false, again);
                        take = finite64(again[20]) && again[20] < sums[20];
                        if (take) {
                            st = next;
                            for (int e = 0; e < kPolishSums; ++e) sums[e] = again[e];
                            double ss = 0.0;
                            for (int e = 0; e < 5; ++e) ss += delta[e] * delta[e];
                            steps[round] = sqrt(ss);
                        }
                    }
                    lambda = take ? fmax(lambda * 0.1, kLambdaMin) : fmin(lambda * 10.0, kLambdaMax);
                }
                cost1 = sums[20];
                double e[9];
                float f[9];
                cross_mul(st.t, st.r, e);
                bool ok = canonical9(e);
                ok = fundamental_of_essential(e, kk, f) && ok;
                for (int k = 0; k < 9; ++k) f[k] = ok ? f[k] : 0.f;
                for (int k = 0; k < count; ++k) {
                    trial[k] = is_inlier(f, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], thr2) ? 1 : 0;
                    n_new += trial[k];
                }
                kept = ok && n_new >= n_in;
                if (kept)
                    for (int k = 0; k < 9; ++k) eo[k] = (float)e[k];
            }
        }
        front = kept ? count_front(st.r, st.t, pts, trial, count, kk) : count_front(rd, td, pts, mask, count, kk);
    }
    if (!kept) {
        cost1 = cost0;
        if (valid) {
            double e[9];
            cross_mul(td, rd, e);
            canonical9(e);
            for (int k = 0; k < 9; ++k) eo[k] = (float)e[k];
        }
    }
    fix_sign(eo);
    for (int k = 0; k < 9; ++k) e_out[k] = eo[k], r_out[k] = kept ? (float)st.r[k] : r[k];
    for (int k = 0; k < 3; ++k) t_out[k] = kept ? (float)st.t[k] : t[k];
    for (int k = 0; k < count; ++k) inliers_out[k] = kept ? trial[k] : mask[k];
    out[0] = kept ? n_new : n_in, out[1] = front, out[2] = kept ? 1 : 0;
    cost[0] = (float)cost0, cost[1] = (float)cost1;
    delete[] mask;
}

// triangulate_kernel's rows: points [count, 3] fp32, ok [count].
void host_triangulate(const float* pts, int count, const float* intrinsics, const float* r, const float* t, const uint8_t* inliers,
                      float* points, uint8_t* ok_out) {
    const Intrinsics kk = intrinsics_of(intrinsics);
    double rd[9], td[3];
    for (int k = 0; k < 9; ++k) rd[k] = (double)r[k];
    for (int k = 0; k < 3; ++k) td[k] = (double)t[k];
    for (int k = 0; k < count; ++k) {
        double x[3] = {0.0, 0.0, 0.0}, c[4];
        bool ok = false;
        if (inliers[k] && intrinsics_ok(kk)) {
            camera(pts + 4 * k, kk, c);
            ok = midpoint(rd, td, c[0], c[1], c[2], c[3], x);
            ok = ok && fabsf((float)x[0]) < INFINITY && fabsf((float)x[1]) < INFINITY && fabsf((float)x[2]) < INFINITY;
        }
        for (int i = 0; i < 3; ++i) points[3 * k + i] = ok ? (float)x[i] : 0.f;
        ok_out[k] = ok ? 1 : 0;
    }
}

}  // extern "C"
