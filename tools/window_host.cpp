// The sequence window's point statements (csrc/lightglue_window_math.h is __host__ __device__) as a host library for
// tools/window_host_check.py: lg_window_points for one window, serially, in the kernel's order of steps. The 8 lanes of a
// track are 8 entries of small arrays, and their sums are added in the xor butterfly's order. No GPU, no HIP:
// c++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off. With -DWINDOW_HOST_MAIN it is a stand-alone program over a small
// built-in window with dirty entries, for a run under -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "lightglue_window_math.h"

using namespace lg_geom;

namespace {

// The sum of the 8 lanes' values in the order the butterfly adds them (lanes 1, 2, 4 apart).
double sum8(const double v[kMaxViews]) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }

void lanes_sums(const double lane[kMaxViews][kWindowSums], double s[kWindowSums]) {
    for (int e = 0; e < kWindowSums; ++e) {
        double col[kMaxViews];
        for (int v = 0; v < kMaxViews; ++v) col[v] = lane[v][e];
        s[e] = sum8(col);
    }
}

}  // namespace

extern "C" void host_window_points(const int32_t* track_kp, int32_t kept_in, const float* kpts, const float* intr, const float* r,
                                   const float* t, const uint8_t* posed, int32_t views, int32_t lmax, int32_t kp, float threshold,
                                   float* obs, uint8_t* seen, float* points, uint8_t* ok_out, uint8_t* seen_all) {
    Pose pose[kMaxViews];
    Camera cam[kMaxViews];
    bool usable[kMaxViews];
    for (int v = 0; v < kMaxViews; ++v) {
        float p[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
        cam[v] = Camera{1.f, 1.f, 0.f, 0.f};
        bool ok = false;
        if (v < views) {
            cam[v] = Camera{intr[4 * v], intr[4 * v + 1], intr[4 * v + 2], intr[4 * v + 3]};
            ok = posed[v] != 0 && camera_ok(cam[v]);
            if (v >= 1) {
                for (int k = 0; k < 9; ++k) p[k] = r[9 * v + k];
                for (int k = 0; k < 3; ++k) p[9 + k] = t[3 * v + k];
            }
        }
        usable[v] = absolute_enter(p, pose[v]) && ok;
    }
    const int kept = kept_in < 0 ? 0 : (kept_in > lmax ? lmax : kept_in);
    const double thr2 = (double)threshold * (double)threshold;
    for (int l = 0; l < lmax; ++l) {
        double px[kMaxViews][2] = {};
        bool has[kMaxViews] = {}, set[kMaxViews] = {};
        for (int v = 0; v < views; ++v) {
            const int at = l < kept ? track_kp[(size_t)v * lmax + l] : -1;
            has[v] = at >= 0 && at < kp;
            if (has[v]) px[v][0] = kpts[((size_t)v * kp + at) * 2], px[v][1] = kpts[((size_t)v * kp + at) * 2 + 1];
            set[v] = has[v] && usable[v];
        }
        double x[3] = {0.0, 0.0, 0.0}, piv = 0.0;
        bool solved = false, all_pass = false;
        int nset = 0;
        for (int pass = 0; pass < 2; ++pass) {
            double lane[kMaxViews][kWindowSums], s[kWindowSums], res[2], jx[2][3];
            nset = 0;
            for (int v = 0; v < kMaxViews; ++v) {
                window_ray(pose[v], cam[v], px[v][0], px[v][1], lane[v]);
                for (int e = 0; e < kWindowSums; ++e) lane[v][e] = set[v] ? lane[v][e] : 0.0;
                nset += set[v] ? 1 : 0;
            }
            lanes_sums(lane, s);
            solved = window_start(s, x, piv);
            for (int round = 0; round < kWindowGnRounds; ++round) {
                for (int v = 0; v < kMaxViews; ++v) {
                    const bool row_ok = window_row(pose[v], cam[v], x, px[v][0], px[v][1], res, jx);
                    window_row_sums(set[v] && row_ok, res, jx, lane[v]);
                }
                lanes_sums(lane, s);
                window_step(s, x);
            }
            bool pass_v[kMaxViews];
            all_pass = true;
            for (int v = 0; v < kMaxViews; ++v) {
                const bool row_ok = window_row(pose[v], cam[v], x, px[v][0], px[v][1], res, jx);
                pass_v[v] = window_pass(set[v], row_ok, res, thr2);
                all_pass = all_pass && !(set[v] && !pass_v[v]);
            }
            if (pass == 0)
                for (int v = 0; v < kMaxViews; ++v) set[v] = pass_v[v];
        }
        const bool ok = window_ok(solved, nset, all_pass, x, piv);
        for (int v = 0; v < views; ++v) {
            const size_t at = (size_t)v * lmax + l;
            obs[2 * at] = (float)px[v][0], obs[2 * at + 1] = (float)px[v][1];
            seen[at] = set[v] && ok ? 1 : 0, seen_all[at] = has[v] ? 1 : 0;
        }
        for (int k = 0; k < 3; ++k) points[3 * l + k] = ok ? (float)x[k] : 0.f;
        ok_out[l] = ok ? 1 : 0;
    }
}

#ifdef WINDOW_HOST_MAIN
// Three cameras a unit apart looking down z at 6 points of a plane at depth 8, and tracks with dirty entries: no
// keypoint, an index out of range, a view that is not posed, a focal length of 0, a pose that is not finite.
int main() {
    const int views = 4, lmax = 9, kp = 6;
    std::vector<float> kpts(views * kp * 2), intr(views * 4), r(views * 9, 0.f), t(views * 3, 0.f);
    std::vector<int32_t> track(views * lmax, -1);
    std::vector<uint8_t> posed(views, 1);
    for (int v = 0; v < views; ++v) {
        intr[4 * v] = intr[4 * v + 1] = 640.f, intr[4 * v + 2] = 320.f, intr[4 * v + 3] = 240.f;
        r[9 * v] = r[9 * v + 4] = r[9 * v + 8] = 1.f;
        t[3 * v] = -(float)v;
        for (int j = 0; j < kp; ++j) {
            const float X = -2.f + j, Y = 0.5f * j - 1.f, Z = 8.f;
            kpts[(v * kp + j) * 2] = 640.f * (X + t[3 * v]) / Z + 320.f, kpts[(v * kp + j) * 2 + 1] = 640.f * Y / Z + 240.f;
        }
    }
    for (int l = 0; l < 6; ++l)
        for (int v = 0; v < views; ++v) track[v * lmax + l] = l;
    track[0 * lmax + 1] = -1, track[1 * lmax + 2] = kp + 7, track[2 * lmax + 3] = -5;
    track[0 * lmax + 6] = 0, track[1 * lmax + 6] = 3;  // a track of two different points: not ok
    posed[2] = 0;
    intr[4 * 3] = 0.f;  // view 3's focal length
    std::vector<float> obs(views * lmax * 2), points(lmax * 3);
    std::vector<uint8_t> seen(views * lmax), ok(lmax), all(views * lmax);
    int total = 0;
    for (int variant = 0; variant < 3; ++variant) {
        if (variant == 1) intr[4 * 3] = 640.f, posed[2] = 1;
        if (variant == 2) r[9 * 1 + 2] = NAN;
        host_window_points(track.data(), variant == 2 ? lmax + 50 : 7, kpts.data(), intr.data(), r.data(), t.data(), posed.data(), views, lmax,
                           kp, 3.f, obs.data(), seen.data(), points.data(), ok.data(), all.data());
        int n = 0;
        for (int l = 0; l < lmax; ++l) n += ok[l];
        printf("variant %d: %d of %d tracks ok, point 0 (%.6f, %.6f, %.6f)\n", variant, n, lmax, points[0], points[1], points[2]);
        total += n;
    }
    return total > 0 ? 0 : 1;
}
#endif
