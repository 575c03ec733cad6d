// The bundle adjustment's statements (csrc/lightglue_bundle_math.h is __host__ __device__) as a host library for
// tools/bundle_host_check.py: the whole of lg_bundle_adjust for one window, serially, in the kernel's order of steps.
// The Schur product is plain loops and the sums are added in landmark order (the kernel's tree and MFMA order differ:
// the bounds' margin is for that and for nothing else). No GPU, no HIP:
// c++ -O2 -std=c++17 -shared -fPIC -ffp-contract=off.
#include <stdint.h>

#include <vector>

#include "lightglue_bundle_math.h"

using namespace lg_geom;

namespace {

struct Window {
    const float* obs;
    const uint8_t* seen;
    const float* intr;
    int views, lmax, count;
    double scale;
    std::vector<uint8_t> fset;
};

Camera camera_of(const Window& w, int v) { return Camera{w.intr[4 * v], w.intr[4 * v + 1], w.intr[4 * v + 2], w.intr[4 * v + 3]}; }

// A landmark at the poses q: its rows, block and inverse. first: the fixed set is formed.
struct Block {
    double res[kMaxViews][2], jc[kMaxViews][2][6], jx[kMaxViews][2][3], gx[3], inv[6];
    bool in[kMaxViews], live, inverted;
};

void block_at(Window& w, const Pose* q, const double* x, int l, double lambda, bool first, Block& k) {
    int bits = first ? 0 : w.fset[l];
    for (int v = 0; v < w.views; ++v) {
        double sb[2][3];
        bundle_basis(q[v], w.scale, sb);
        const size_t at = (size_t)v * w.lmax + l;
        const bool cand = first ? (l < w.count && w.seen[at] != 0) : ((bits >> v) & 1) != 0;
        const bool ok = bundle_row(q[v], camera_of(w, v), v, sb, x, cand ? (double)w.obs[2 * at] : 0.0, cand ? (double)w.obs[2 * at + 1] : 0.0,
                                   k.res[v], k.jc[v], k.jx[v]);
        k.in[v] = cand && ok;
        if (first && k.in[v]) bits |= 1 << v;
    }
    if (first) {
        int n = 0;
        for (int v = 0; v < w.views; ++v) n += (bits >> v) & 1;
        bits = n >= 2 ? bits : 0;
        w.fset[l] = (uint8_t)bits;
        for (int v = 0; v < w.views; ++v) k.in[v] = k.in[v] && bits != 0;
    }
    k.live = bits != 0;
    double vv[6] = {0, 0, 0, 0, 0, 0};
    k.gx[0] = k.gx[1] = k.gx[2] = 0.0;
    for (int v = 0; v < w.views; ++v)
        if (k.in[v]) bundle_point_add(vv, k.gx, k.res[v], k.jx[v]);
    k.inverted = bundle_point_inverse(vv, lambda, k.inv);
    for (int e = 0; e < 6; ++e) k.inv[e] = k.live && k.inverted ? k.inv[e] : 0.0;
}

}  // namespace

extern "C" {

int host_max_rounds() { return kMaxBundle; }

// lg_bundle_adjust for one window: r_out [V, 9], t_out [V, 3] fp32, points_out [L, 3] fp32, cost [2] fp64, out = (num_obs,
// kept).
void host_bundle(const float* obs, const uint8_t* seen, int count, const float* intr, const float* r, const float* t,
                 const float* points, int views, int lmax, int iterations, float* r_out, float* t_out, float* points_out, double* cost,
                 int32_t* out) {
    Window w{obs, seen, intr, views, lmax, count < 0 ? 0 : (count > lmax ? lmax : count), 0.0, std::vector<uint8_t>(lmax, 0)};
    for (int v = 0; v < views; ++v)
        for (int k = 0; k < 12; ++k) {
            const float given = v == 0 ? (k < 9 && k % 4 == 0 ? 1.f : 0.f) : (k < 9 ? r[9 * v + k] : t[3 * v + k - 9]);
            (k < 9 ? r_out[9 * v + k] : t_out[3 * v + k - 9]) = given;
        }
    for (int e = 0; e < 3 * lmax; ++e) points_out[e] = points[e];
    cost[0] = cost[1] = 0.0, out[0] = out[1] = 0;
    Pose cur[kMaxViews], next[kMaxViews];
    bool staged = true;
    for (int v = 0; v < views; ++v) {
        float p[12];
        for (int k = 0; k < 9; ++k) p[k] = r_out[9 * v + k];
        for (int k = 0; k < 3; ++k) p[9 + k] = t_out[3 * v + k];
        staged = absolute_enter(p, cur[v]) && camera_ok(camera_of(w, v)) && staged;
        if (v == 1) staged = staged && (p[9] != 0.f || p[10] != 0.f || p[11] != 0.f);
        next[v] = cur[v];
    }
    if (!staged) return;
    w.scale = sqrt(cur[1].t[0] * cur[1].t[0] + cur[1].t[1] * cur[1].t[1] + cur[1].t[2] * cur[1].t[2]);
    if (!(finite64(w.scale) && w.scale > 0.0)) return;
    const int n = bundle_params(views);
    std::vector<double> pts(3 * lmax), trial(3 * lmax);
    for (int e = 0; e < 3 * lmax; ++e) pts[e] = (double)points[e];
    static double s[kBaPad][kBaPad];
    double rhs[kBaPad], delta[kBaPad], lambda = kLambdaStart, now = 0.0;
    bool kept = false;
    for (int round = 0; round < iterations; ++round) {
        // the build pass
        double sums[kMaxViews][kBaSums];
        for (int v = 0; v < kMaxViews; ++v)
            for (int e = 0; e < kBaSums; ++e) sums[v][e] = 0.0;
        for (int i = 0; i < kBaPad; ++i)
            for (int j = 0; j < kBaPad; ++j) s[i][j] = 0.0;
        int bad = 0;
        for (int l = 0; l < lmax; ++l) {
            Block k;
            block_at(w, cur, &pts[3 * l], l, lambda, round == 0, k);
            bad += k.live && !k.inverted ? 1 : 0;
            double wl[kBaPad][3], yl[kBaPad][3];
            for (int i = 0; i < kBaPad; ++i)
                for (int c = 0; c < 3; ++c) wl[i][c] = yl[i][c] = 0.0;
            for (int v = 0; v < views; ++v) {
                if (!k.in[v]) continue;
                double ww[6][3], yy[6][3];
                bundle_w(k.jc[v], k.jx[v], k.inv, ww, yy);
                bundle_view_add(sums[v], k.res[v], k.jc[v], yy, k.gx);
                sums[v][kBaObs] += 1.0;
                for (int a = 0; a < bundle_width(v); ++a)
                    for (int c = 0; c < 3; ++c) wl[bundle_row0(v) + a][c] = ww[a][c], yl[bundle_row0(v) + a][c] = yy[a][c];
            }
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j)
                    for (int c = 0; c < 3; ++c) s[i][j] -= yl[i][c] * wl[j][c];
        }
        if (round == 0) {
            bool enough = true;
            for (int v = 0; v < views; ++v) {
                now += sums[v][BaLm::kCost], out[0] += (int)sums[v][kBaObs];
                enough = enough && (v < 1 || (int)sums[v][kBaObs] >= kMinViewObs);
            }
            cost[0] = cost[1] = now;
            if (!(enough && finite64(now))) return;
        }
        for (int v = 1; v < views; ++v)
            for (int a = 0; a < bundle_width(v); ++a) {
                for (int c = 0; c < bundle_width(v); ++c) {
                    const double u = sums[v][upper6(a < c ? a : c, a < c ? c : a)];
                    s[bundle_row0(v) + a][bundle_row0(v) + c] += a == c ? u * (1.0 + lambda) : u;
                }
                rhs[bundle_row0(v) + a] = -(sums[v][BaLm::kGrad + a] - sums[v][kBaYg + a]);
            }
        bool take = bad == 0;
        if (take) take = bundle_solve(s, rhs, n, delta);
        if (take) {
            for (int v = 1; v < views; ++v) {
                double d[6] = {0, 0, 0, 0, 0, 0};
                for (int a = 0; a < bundle_width(v); ++a) d[a] = delta[bundle_row0(v) + a];
                bundle_update(cur[v], v, w.scale, d, next[v]);
            }
            double again = 0.0;
            for (int l = 0; l < lmax; ++l) {
                Block k;
                block_at(w, cur, &pts[3 * l], l, lambda, false, k);
                double wd[3] = {k.gx[0], k.gx[1], k.gx[2]}, dx[3];
                for (int v = 1; v < views; ++v) {
                    if (!k.in[v]) continue;
                    for (int c = 0; c < 3; ++c)
                        for (int a = 0; a < bundle_width(v); ++a)
                            wd[c] += (k.jc[v][0][a] * k.jx[v][0][c] + k.jc[v][1][a] * k.jx[v][1][c]) * delta[bundle_row0(v) + a];
                }
                sym3_mul(k.inv, wd, dx);
                for (int c = 0; c < 3; ++c) trial[3 * l + c] = pts[3 * l + c] - dx[c];
                for (int v = 0; v < views; ++v) {
                    if (!k.in[v]) continue;
                    double res[2];
                    const size_t at = (size_t)v * lmax + l;
                    bundle_residual(next[v], camera_of(w, v), &trial[3 * l], (double)obs[2 * at], (double)obs[2 * at + 1], res);
                    again += res[0] * res[0] + res[1] * res[1];
                }
            }
            take = lm_accept(again, now);
            if (take) {
                now = again, kept = true;
                for (int v = 1; v < views; ++v) cur[v] = next[v];
                pts.swap(trial);
            }
        }
        lambda = lm_lambda(lambda, take);
    }
    for (int v = 1; v < views && kept; ++v) {
        float p[12];
        kept = absolute_round(cur[v], p);
    }
    for (int l = 0; l < lmax && kept; ++l)
        for (int c = 0; c < 3; ++c) kept = kept && (!w.fset[l] || fabsf((float)pts[3 * l + c]) < INFINITY);
    cost[1] = kept ? now : cost[0];
    out[1] = kept ? 1 : 0;
    if (!kept) return;
    for (int v = 1; v < views; ++v) {
        for (int k = 0; k < 9; ++k) r_out[9 * v + k] = (float)cur[v].r[k];
        for (int k = 0; k < 3; ++k) t_out[3 * v + k] = (float)cur[v].t[k];
    }
    for (int l = 0; l < lmax; ++l)
        if (w.fset[l])
            for (int c = 0; c < 3; ++c) points_out[3 * l + c] = (float)pts[3 * l + c];
}

}  // extern "C"
