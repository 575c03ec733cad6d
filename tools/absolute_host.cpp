// The absolute pose's statements (csrc/lightglue_absolute_math.h is __host__ __device__) as a host library for
// tools/absolute_host_check.py: the 3-sample, the P3P solve with the four lanes of a hypothesis run in turn (each its
// piece of the quartic's interval, the candidates then ranked as the lanes rank them), the fp32 score, one
// Levenberg-Marquardt refit as the finalize kernel orders it (with the number of rounds a parameter, for the table
// kAbsoluteLmRounds is chosen from) and the whole call for one pair. No GPU, no HIP:
// c++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off.
#include <stdint.h>

#include "lightglue_absolute_math.h"

using namespace lg_geom;

namespace {

Camera camera_of(const float* k) { return Camera{k[0], k[1], k[2], k[3]}; }

// One hypothesis as the kernel does it: cand [4][12] fp32, those that exist first in ascending key; returns their number.
int solve_one(const float* pts, const Camera& cam, const int32_t* idx, int count, float cand[4][12]) {
    double x[3][3], px[3][2];
    for (int j = 0; j < 3; ++j) {
        const int i = idx[j] < 0 ? 0 : (idx[j] > count - 1 ? count - 1 : idx[j]);
        for (int c = 0; c < 3; ++c) x[j][c] = (double)pts[5 * i + c];
        px[j][0] = (double)pts[5 * i + 3], px[j][1] = (double)pts[5 * i + 4];
    }
    P3p s;
    p3p_setup(x, px, cam, s);
    float pose[4][12];
    double key[4];
    bool ok[4];
    for (int sub = 0; sub < 4; ++sub) {
        double u;
        const bool has = p3p_root(s, sub, u);
        AbsPose q;
        ok[sub] = p3p_pose(s, x, u, q.r, q.t, key[sub]) && has;
        ok[sub] = absolute_round(q, pose[sub]) && ok[sub];
    }
    int n = 0;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 12; ++k) cand[i][k] = 0.f;
    for (int sub = 0; sub < 4; ++sub) {
        if (!ok[sub]) continue;
        int rank = 0;
        for (int j = 0; j < 4; ++j) rank += ok[j] && (key[j] < key[sub] || (key[j] == key[sub] && j < sub)) ? 1 : 0;
        for (int k = 0; k < 12; ++k) cand[rank][k] = pose[sub][k];
        ++n;
    }
    return n;
}

int count_mask(const float pose[12], const Camera& cam, const float* pts, int count, float thr2, uint8_t* mask) {
    int n = 0;
    for (int k = 0; k < count; ++k) {
        mask[k] = is_inlier_abs(pose, cam, pts[5 * k], pts[5 * k + 1], pts[5 * k + 2], pts[5 * k + 3], pts[5 * k + 4], thr2) ? 1 : 0;
        n += mask[k];
    }
    return n;
}

// One pass over the rows, serially: the sums at the pose q over the rows with (first ? mask and a usable residual, which
// defines fixed : fixed).
void pass(const AbsPose& q, const Camera& cam, const float* pts, const uint8_t* mask, uint8_t* fixed, int count, bool first,
          double sums[kAbsSums]) {
    for (int e = 0; e < kAbsSums; ++e) sums[e] = 0.0;
    for (int k = 0; k < count; ++k) {
        if (first) fixed[k] = 0;
        if (!(first ? mask[k] : fixed[k])) continue;
        double res[2], j[2][6];
        const bool fin = absolute_row(q, cam, (double)pts[5 * k], (double)pts[5 * k + 1], (double)pts[5 * k + 2], (double)pts[5 * k + 3],
                                      (double)pts[5 * k + 4], res, j);
        if (first) {
            fixed[k] = fin ? 1 : 0;
            if (!fin) continue;
        }
        absolute_accumulate(sums, res, j);
    }
}

// One refit as absolute_finalize_kernel does it: from the fp32 pose over the rows with mask != 0, `rounds` rounds of
// Levenberg-Marquardt -> the pose rounded to fp32. False where there is no refit. cost: the entering and the final.
bool refit(const float pose[12], const Camera& cam, const float* pts, const uint8_t* mask, uint8_t* fixed, int count, int rounds,
           float out[12], double cost[2]) {
    AbsPose st;
    if (!absolute_enter(pose, st)) return false;
    double sums[kAbsSums];
    pass(st, cam, pts, mask, fixed, count, true, sums);
    cost[0] = cost[1] = sums[27];
    if (!((int)sums[28] >= kMinAbsRows && finite64(sums[27]))) return false;
    double lambda = kLambdaStart;
    for (int it = 0; it < rounds; ++it) {
        double delta[6];
        bool take = absolute_step(sums, lambda, delta);
        if (take) {
            AbsPose next;
            double again[kAbsSums];
            absolute_update(st, delta, next);
            pass(next, cam, pts, mask, fixed, count, false, again);
            take = finite64(again[27]) && again[27] < sums[27];
            if (take) {
                st = next;
                for (int e = 0; e < kAbsSums; ++e) sums[e] = again[e];
            }
        }
        lambda = take ? fmax(lambda * 0.1, kLambdaMin) : fmin(lambda * 10.0, kLambdaMax);
    }
    cost[1] = sums[27];
    return absolute_round(st, out);
}

}  // namespace

extern "C" {

int host_lm_rounds() { return kAbsoluteLmRounds; }

void host_samples3(int32_t seed, int hypotheses, int count, int32_t* out) {
    for (int h = 0; h < hypotheses; ++h) sample<3>((uint32_t)seed, h, count, out + 3 * h);
}

// pts [count, 5] = (X, Y, Z, x, y); intrinsics [4]; samples [hypotheses, 3] -> cands [hypotheses, 4, 12], num [hypotheses].
void host_solve3(const float* pts, int count, const float* intrinsics, const int32_t* samples, int hypotheses, float* cands,
                 int32_t* num) {
    const Camera cam = camera_of(intrinsics);
    for (int h = 0; h < hypotheses; ++h) num[h] = solve_one(pts, cam, samples + 3 * h, count, reinterpret_cast<float(*)[12]>(cands + 48 * h));
}

int host_score(const float* pts, int count, const float* intrinsics, const float* pose, float threshold, uint8_t* mask) {
    return count_mask(pose, camera_of(intrinsics), pts, count, threshold * threshold, mask);
}

// refit() with `rounds` rounds; returns 0 where there is no refit.
int host_refit(const float* pts, const uint8_t* mask, int count, const float* intrinsics, const float* pose, int rounds, float* out,
               double* cost) {
    uint8_t* fixed = new uint8_t[count > 0 ? count : 1];
    const bool ok = refit(pose, camera_of(intrinsics), pts, mask, fixed, count, rounds, out, cost);
    delete[] fixed;
    return ok ? 1 : 0;
}

// The whole of lg_ransac_absolute for one pair, serially, in the kernels' order: r [9], t [3] fp32, inliers [count],
// out = (num_inliers, valid, best).
void host_absolute(const float* pts, int count, const float* intrinsics, float threshold, int hypotheses, int refits, int32_t seed,
                   int rounds, float* r_out, float* t_out, uint8_t* inliers, int32_t* out) {
    const Camera cam = camera_of(intrinsics);
    const float thr2 = threshold * threshold;
    for (int i = 0; i < 9; ++i) r_out[i] = 0.f;
    for (int i = 0; i < 3; ++i) t_out[i] = 0.f;
    for (int k = 0; k < count; ++k) inliers[k] = 0;
    out[0] = out[1] = 0, out[2] = -1;
    if (count < kMinInliersA || !camera_ok(cam)) return;
    uint8_t* mask = new uint8_t[3 * count];
    uint8_t* trial = mask + count;
    uint8_t* fixed = mask + 2 * count;
    int bc = -1, bh = -1;
    float pose[12];
    for (int k = 0; k < 12; ++k) pose[k] = 0.f;
    for (int h = 0; h < hypotheses; ++h) {
        int32_t idx[3];
        float cand[4][12];
        sample<3>((uint32_t)seed, h, count, idx);
        const int n = solve_one(pts, cam, idx, count, cand);
        int bn = -1, bs = -1;
        for (int s = 0; s < n; ++s) {
            const int got = count_mask(cand[s], cam, pts, count, thr2, trial);
            if (got > bn) bn = got, bs = s;
        }
        const int c = bn < 0 ? 0 : bn;
        if (c > bc) {
            bc = c, bh = h;
            for (int k = 0; k < 12; ++k) pose[k] = bs < 0 ? 0.f : cand[bs][k];
        }
    }
    if (bc >= kMinInliersA) {
        int num = count_mask(pose, cam, pts, count, thr2, mask);
        for (int round = 0; round < refits && num >= kMinInliersA; ++round) {
            float fine[12];
            double cost[2];
            if (!refit(pose, cam, pts, mask, fixed, count, rounds, fine, cost)) break;
            const int again = count_mask(fine, cam, pts, count, thr2, trial);
            if (again < num) break;
            num = again;
            for (int k = 0; k < 12; ++k) pose[k] = fine[k];
            for (int k = 0; k < count; ++k) mask[k] = trial[k];
        }
        for (int k = 0; k < 9; ++k) r_out[k] = pose[k];
        for (int k = 0; k < 3; ++k) t_out[k] = pose[9 + k];
        for (int k = 0; k < count; ++k) inliers[k] = mask[k];
        out[0] = num, out[1] = 1, out[2] = bh;
    }
    delete[] mask;
}

}  // extern "C"
