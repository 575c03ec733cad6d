// The five-point RANSAC's statements (csrc/lightglue_essential_math.h is __host__ __device__) as a host library
// for tools/essential_host_check.py: the 5-sample, the five-point solve with the four lanes of a hypothesis run in
// turn (each its five columns of the 10 x 20 matrix, the pivot column handed over where the kernel shuffles), one
// refit round as the finalize kernel orders it, the pose, and the whole call for one pair. No GPU, no HIP:
// c++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off.
#include <stdint.h>

#include "lightglue_essential_math.h"

using namespace lg_geom;

namespace {

Intrinsics intrinsics_of(const float* k) {
    return Intrinsics{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]};
}

template <int C>
void steps(double a[4][10][5], double& low) {
    double col[10];
    for (int r = 0; r < 10; ++r) col[r] = a[C / 5][r][C % 5];
    for (int sub = 0; sub < 4; ++sub) {
        double mine[10];
        for (int r = 0; r < 10; ++r) mine[r] = col[r];
        const double p = slice_step<C>(a[sub], mine);
        low = p < low || !(p == p) ? p : low;
    }
    if constexpr (C < 9) steps<C + 1>(a, low);
}

// One hypothesis as the kernel does it: cand [10][9] canonical E in camera coordinates, the candidates that exist
// first, in ascending root; returns their number. low: the smallest pivot of the 10 x 20 elimination.
int solve_one(const float* pts, const Intrinsics& k, const int32_t* idx, int count, float cand[10][9], float fund[10][9],
              double& low) {
    double x0[5], y0[5], x1[5], y1[5];
    for (int j = 0; j < 5; ++j) {
        const int i = idx[j] < 0 ? 0 : (idx[j] > count - 1 ? count - 1 : idx[j]);
        x0[j] = ((double)pts[4 * i] - k.cx0) / k.fx0, y0[j] = ((double)pts[4 * i + 1] - k.cy0) / k.fy0;
        x1[j] = ((double)pts[4 * i + 2] - k.cx1) / k.fx1, y1[j] = ((double)pts[4 * i + 3] - k.cy1) / k.fy1;
    }
    double basis[4][9], a[4][10][5];
    bool ok = null_space5(x0, y0, x1, y1, basis);
    for (int sub = 0; sub < 4; ++sub) fill_slice(basis, sub, a[sub]);
    low = INFINITY;
    steps<0>(a, low);
    ok = ok && low >= (double)kPivotEps;
    double rhs[6][10];
    for (int r = 0; r < 6; ++r)
        for (int j = 0; j < 5; ++j) rhs[r][j] = a[2][4 + r][j], rhs[r][5 + j] = a[3][4 + r][j];
    Eq3 q[3];
    for (int i = 0; i < 3; ++i) q[i] = equation(rhs[2 * i], rhs[2 * i + 1]);
    double c[11], root[10];
    bool has[10];
    determinant10(q, c);
    ok = real_roots10(c, root, has) && ok;
    int n = 0;
    for (int i = 0; i < 10; ++i)
        for (int k9 = 0; k9 < 9; ++k9) cand[i][k9] = 0.f;
    for (int i = 0; i < 10; ++i) {
        double e[9];
        float f[9];
        if (!(ok && has[i] && candidate5(basis, q, root[i], e) && fundamental_of_essential(e, k, f))) continue;
        for (int k9 = 0; k9 < 9; ++k9) cand[n][k9] = (float)e[k9], fund[n][k9] = f[k9];
        ++n;
    }
    return n;
}

// One refit round as essential_finalize_kernel does it, serially: camera coordinates of the rows with mask != 0,
// Hartley over them, the 45 sums of normal_accumulate_f, the round-robin Jacobi, the eigenvector of the smallest
// diagonal entry, de-normalised, projected to the essential manifold (canonical, fp64).
bool refit_e(const float* pts, const uint8_t* mask, int count, const Intrinsics& kk, double e[9]) {
    auto cam = [&](int k, double q[4]) {
        q[0] = ((double)pts[4 * k] - kk.cx0) / kk.fx0, q[1] = ((double)pts[4 * k + 1] - kk.cy0) / kk.fy0;
        q[2] = ((double)pts[4 * k + 2] - kk.cx1) / kk.fx1, q[3] = ((double)pts[4 * k + 3] - kk.cy1) / kk.fy1;
    };
    double c[4] = {0, 0, 0, 0}, d[2] = {0, 0}, n = 0, q[4];
    for (int k = 0; k < count; ++k) {
        if (!mask[k]) continue;
        n += 1;
        cam(k, q);
        for (int i = 0; i < 4; ++i) c[i] += q[i];
    }
    for (int i = 0; i < 4; ++i) c[i] /= n;
    for (int k = 0; k < count; ++k) {
        if (!mask[k]) continue;
        cam(k, q);
        d[0] += sqrt((q[0] - c[0]) * (q[0] - c[0]) + (q[1] - c[1]) * (q[1] - c[1]));
        d[1] += sqrt((q[2] - c[2]) * (q[2] - c[2]) + (q[3] - c[3]) * (q[3] - c[3]));
    }
    const double s[2] = {1.4142135623730951 / (d[0] / n), 1.4142135623730951 / (d[1] / n)};
    double acc[45];
    for (int e = 0; e < 45; ++e) acc[e] = 0.0;
    for (int k = 0; k < count; ++k) {
        if (!mask[k]) continue;
        cam(k, q);
        normal_accumulate_f(acc, (q[0] - c[0]) * s[0], (q[1] - c[1]) * s[0], (q[2] - c[2]) * s[1], (q[3] - c[3]) * s[1]);
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
    double fn[9];
    for (int k = 0; k < 9; ++k) fn[k] = vm[9 * k + lo];
    bool ok = denormalise64(fn, c[0], c[1], s[0], c[2], c[3], s[1], e);
    return project_essential(e) && ok;
}

int count_mask(const float f[9], const float* pts, int count, float thr2, uint8_t* mask) {
    int n = 0;
    for (int k = 0; k < count; ++k) {
        mask[k] = is_inlier(f, pts[4 * k], pts[4 * k + 1], pts[4 * k + 2], pts[4 * k + 3], thr2) ? 1 : 0;
        n += mask[k];
    }
    return n;
}

// The pose of e over the rows with mask != 0, as pose_of does it: r, t zeros and 0 where e has no decomposition.
int pose_e(const double e[9], const float* pts, const uint8_t* mask, int count, const Intrinsics& kk, double r[9], double t[3],
           int32_t fronts[4]) {
    double u[9], v[9];
    const bool ok = svd3(e, u, v);
    int best = -1;
    for (int i = 0; i < 9; ++i) r[i] = 0.0;
    t[0] = t[1] = t[2] = 0.0;
    for (int i = 0; i < 4; ++i) {
        double rr[9], tt[3];
        pose_candidate(u, v, i, rr, tt);
        int n = 0;
        for (int k = 0; k < count; ++k) {
            if (!mask[k]) continue;
            n += in_front(rr, tt, ((double)pts[4 * k] - kk.cx0) / kk.fx0, ((double)pts[4 * k + 1] - kk.cy0) / kk.fy0,
                          ((double)pts[4 * k + 2] - kk.cx1) / kk.fx1, ((double)pts[4 * k + 3] - kk.cy1) / kk.fy1)
                     ? 1 : 0;
        }
        fronts[i] = n;
        if (ok && n > best) {
            best = n;
            for (int j = 0; j < 9; ++j) r[j] = rr[j];
            for (int j = 0; j < 3; ++j) t[j] = tt[j];
        }
    }
    return best < 0 ? 0 : best;
}

}  // namespace

extern "C" {

void host_samples5(int32_t seed, int hypotheses, int count, int32_t* out) {
    for (int h = 0; h < hypotheses; ++h) sample<5>((uint32_t)seed, h, count, out + 5 * h);
}

// pts [count, 4] = (x0, y0, x1, y1) in pixels; intrinsics [8]; samples [hypotheses, 5] -> cands [hypotheses, 10, 9]
// (E in camera coordinates), num [hypotheses], low [hypotheses] (the smallest pivot of the 10 x 20 elimination).
void host_solve5(const float* pts, int count, const float* intrinsics, const int32_t* samples, int hypotheses, float* cands,
                 int32_t* num, double* low) {
    const Intrinsics k = intrinsics_of(intrinsics);
    float fund[10][9];
    for (int h = 0; h < hypotheses; ++h)
        num[h] = solve_one(pts, k, samples + 5 * h, count, reinterpret_cast<float(*)[9]>(cands + 90 * h), fund, low[h]);
}

// F in pixels of an E in camera coordinates, as a candidate is scored.
int host_fundamental(const float* e, const float* intrinsics, float* f) {
    double d[9];
    for (int i = 0; i < 9; ++i) d[i] = e[i];
    return fundamental_of_essential(d, intrinsics_of(intrinsics), f) ? 1 : 0;
}

// refit_e on the rows with mask != 0, rounded to fp32. Returns 0 where not finite.
int host_refit_e(const float* pts, const uint8_t* mask, int count, const float* intrinsics, float out[9]) {
    double e[9];
    const bool ok = refit_e(pts, mask, count, intrinsics_of(intrinsics), e);
    for (int k = 0; k < 9; ++k) out[k] = (float)e[k];
    return ok ? 1 : 0;
}

// pose_e of e (fp32, camera coordinates) over the rows with mask != 0: r [9], t [3] fp32; returns num_front, and the
// four candidates' counts in fronts [4].
int host_pose(const float* e32, const float* pts, const uint8_t* mask, int count, const float* intrinsics, float* r, float* t,
              int32_t* fronts) {
    double e[9], rr[9], tt[3];
    for (int i = 0; i < 9; ++i) e[i] = e32[i];
    const int front = pose_e(e, pts, mask, count, intrinsics_of(intrinsics), rr, tt, fronts);
    for (int i = 0; i < 9; ++i) r[i] = (float)rr[i];
    for (int i = 0; i < 3; ++i) t[i] = (float)tt[i];
    return front;
}

// The whole of lg_ransac_essential for one pair, serially, in the kernels' order: pts [count, 4] -> e, r [9], t [3]
// fp32, inliers [count], out = (num_inliers, num_front, valid, best).
void host_essential(const float* pts, int count, const float* intrinsics, float threshold, int hypotheses, int refits,
                    int32_t seed, float* e_out, float* r_out, float* t_out, uint8_t* inliers, int32_t* out) {
    const Intrinsics kk = intrinsics_of(intrinsics);
    const float thr2 = threshold * threshold;
    for (int i = 0; i < 9; ++i) e_out[i] = 0.f, r_out[i] = 0.f;
    for (int i = 0; i < 3; ++i) t_out[i] = 0.f;
    for (int k = 0; k < count; ++k) inliers[k] = 0;
    out[0] = out[1] = out[2] = 0, out[3] = -1;
    if (count < kMinInliersE || !intrinsics_ok(kk)) return;
    uint8_t* mask = new uint8_t[2 * count];
    uint8_t* trial = mask + count;
    int bc = -1, bh = -1;
    float bf[9], be[9];
    for (int h = 0; h < hypotheses; ++h) {
        int32_t idx[5];
        float cand[10][9], fund[10][9];
        double low;
        sample<5>((uint32_t)seed, h, count, idx);
        const int n = solve_one(pts, kk, idx, count, cand, fund, low);
        int bn = -1, bs = -1;
        float b00 = 0.f;
        for (int s = 0; s < n; ++s) {
            const int got = count_mask(fund[s], pts, count, thr2, trial);
            const bool take = got > bn || (got == bn && cand[s][0] < b00);
            bn = take ? got : bn, bs = take ? s : bs, b00 = take ? cand[s][0] : b00;
        }
        const int c = bn < 0 ? 0 : bn;
        if (c > bc) {
            bc = c, bh = h;
            for (int k = 0; k < 9; ++k) bf[k] = bs < 0 ? 0.f : fund[bs][k], be[k] = bs < 0 ? 0.f : cand[bs][k];
        }
    }
    if (bc >= kMinInliersE) {
        double e[9], r[9], t[3];
        float f[9];
        for (int k = 0; k < 9; ++k) f[k] = bf[k], e[k] = (double)be[k];
        int num = count_mask(f, pts, count, thr2, mask);
        for (int round = 0; round < refits && num >= kMinInliers; ++round) {
            double en[9];
            float fn[9];
            if (!(refit_e(pts, mask, count, kk, en) && fundamental_of_essential(en, kk, fn))) break;
            const int again = count_mask(fn, pts, count, thr2, trial);
            if (again < num) break;
            num = again;
            for (int k = 0; k < 9; ++k) e[k] = en[k];
            for (int k = 0; k < count; ++k) mask[k] = trial[k];
        }
        int32_t fronts[4];
        out[1] = pose_e(e, pts, mask, count, kk, r, t, fronts);
        for (int k = 0; k < 9; ++k) e_out[k] = (float)e[k], r_out[k] = (float)r[k];
        fix_sign(e_out);
        for (int k = 0; k < 3; ++k) t_out[k] = (float)t[k];
        for (int k = 0; k < count; ++k) inliers[k] = mask[k];
        out[0] = num, out[2] = 1, out[3] = bh;
    }
    delete[] mask;
}

}  // extern "C"
