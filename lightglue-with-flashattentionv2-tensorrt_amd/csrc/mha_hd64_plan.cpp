// mha_hd64_plan.cpp — the attention planner: which kernel, workgroup shape and KV split a launch
// takes, the route of fp32 inputs, and the workspace either uses. Host code with no HIP runtime
// call; the environment switches of these decisions and their setters live here too.
#include <algorithm>
#include <atomic>
#include <cstdlib>

#include "mha_hd64_internal.h"

namespace mha_hd64 {

namespace {
std::atomic<int> g_concurrency{1};

// Workgroups of `rows` query rows over all calls.
long blocks_of(const Call* calls, int n, int rows) {
    long blocks = 0;
    for (int i = 0; i < n; ++i) blocks += (long)calls[i].batch * calls[i].heads * ((calls[i].nq + rows - 1) / rows);
    return blocks;
}

// The plan of a kernel that never splits: the single-pass kernels (direct_tiles > 0), the streaming kernel.
GroupPlan no_split_plan(int n, int q_waves, int kv_waves, int rows_per_wave, int direct_tiles) {
    GroupPlan p{};
    p.q_waves = q_waves;
    p.kv_waves = kv_waves;
    p.rows_per_wave = rows_per_wave;
    p.direct_tiles = direct_tiles;
    p.stream = direct_tiles == 0;
    for (int i = 0; i < n; ++i) p.splits[i] = p.tiles_per_split[i] = 1;
    return p;
}

// A switch that is on unless its environment variable starts with `off`.
bool env_on(const char* name, char off = '0') {
    const char* e = std::getenv(name);
    return !(e && e[0] == off);
}
// A switch with a setter: unset (-1) until first read, then 0 / 1 (/ 2 where the variable may say 2).
int env_mode(std::atomic<int>& mode, const char* name, bool takes2 = false) {
    int v = mode.load();
    if (v < 0) {
        const char* e = std::getenv(name);
        int expect = -1;
        mode.compare_exchange_strong(expect, (e && e[0] == '0') ? 0 : (takes2 && e && e[0] == '2') ? 2 : 1);
        v = mode.load();
    }
    return v;
}
}  // namespace

int concurrency_hint() { return g_concurrency.load(std::memory_order_relaxed); }
int set_concurrency_hint(int streams) { return g_concurrency.exchange(std::max(1, streams)); }

size_t split_workspace_bytes(const Call& c, int splits) {
    if (splits <= 1) return 0;
    const size_t rows = (size_t)c.batch * c.heads * splits * c.nq;
    const size_t o_bytes = rows * kHeadDim * sizeof(float);  // fp32 bound (fp16 partials use half)
    return align256(o_bytes) + align256(rows * 2 * sizeof(float));  // + (m, l) per row
}

static bool direct_enabled() { static const bool on = env_on("MHA_HD64_DIRECT"); return on; }

// Tiles of 64 keys per wave of the single-pass kernels for this launch, or 0 if they do not apply:
// fp16 input, every call's keys within 8 waves x 2 tiles (x 2 passes for 32-row blocks), and at most max_wgs workgroups of `rows`
// query rows. 16-row blocks: at most 256 (one per CU, one round). 32-row blocks: at most 768 —
// up to three rounds of 256 still beat the LDS ring's plans there (tools/batch_sweep.py, graph
// replay, us per launch, 32-row kernel vs planner's ring plan: B=3 N=1024 10.3 vs 18.1, B=6 15.3 vs
// 19.7, B=6 N=512 6.3 vs 9.5, B=12 N=512 8.7 vs 13.5; at 1024 blocks the ring wins: B=8 N=1024
// 15.5 vs 21.0, B=16 N=512 10.4 vs 11.2). Past one round with 512 < nkv <= 1024 the 32-row kernel
// runs its two-workgroups-per-CU form (launch_direct): B=3 8.86 vs 10.28 for one per CU (ring
// 10.43), B=4 9.41 vs 10.68 (10.77), B=6 13.15 vs 15.23 (14.11); B=8 16.85 vs ring 15.33.
constexpr long kDirectMaxWgs16 = 256, kDirectMaxWgs32 = 768;
static int direct_tiles_for(const Call* calls, int n, InType in, bool forced, int rows = 32) {
    if (in != InType::F16 || (!forced && !direct_enabled())) return 0;
    const long wgs = blocks_of(calls, n, rows);
    int tiles = 1;
    // keys per call: <= 2048 (tiles 3, 4: the two-pass forms, 4 waves x 2 x 4 tiles)
    const int max_tiles = 4;
    for (int i = 0; i < n; ++i) {
        if (calls[i].nkv > 8 * max_tiles * kTileKV) return 0;
        tiles = std::max(tiles, (calls[i].nkv + 8 * kTileKV - 1) / (8 * kTileKV));
    }
    // two-pass forms (tiles 3, 4), one round: 16-row blocks up to 256, 32-row blocks from 96 on (tools/batch_sweep.py, us per launch, two-pass 16-row / 32-row
    // kernel vs ring plan: 2048^2 B=1 - / 9.87 vs 13.04, B=2 - / 17.6 vs 17.3; 1536^2 B=1 - / 8.13
    // vs 11.12; Nq x Nkv 1024x2048 7.40 / 8.57 vs 10.74, 768x2048 6.79 / 8.38 vs 10.24,
    // 512x2048 6.68 / 8.33 vs 7.95, 256x2048 6.61 / 8.31 vs 7.69, 1024x1536 6.32 / 8.05 vs 9.84)
    // Past one round the 32-row kernel's two-workgroups-per-CU form (4 passes x 2 tiles) takes
    // over up to 768 blocks (vs the ring plan: 2x4x2048^2 16.1 vs 17.8, 3x 21.7 vs 23.3; 2x4x1536^2
    // 12.0 vs 13.5, 3x 18.0 vs 17.7, 4x 18.6 vs 18.7; 4x4x1024x2048 15.0 vs 17.8).
    if (tiles > 2 && !forced && (rows == 16 ? wgs > 256 : wgs < 96)) return 0;
    const long max_wgs = rows == 16 ? kDirectMaxWgs16 : kDirectMaxWgs32;
    return (forced || wgs <= max_wgs) ? tiles : 0;
}

// The 16-row single-pass kernel first (default; MHA_HD64_DIRECT_ROWS=32 keeps 32-row blocks)
static bool direct16_enabled() { static const bool on = env_on("MHA_HD64_DIRECT_ROWS", '3'); return on; }

// The persistent streaming kernel (mha_hd64_stream.hip) for fp16 launches of more than one round
// of 128-row blocks (MHA_HD64_STREAM=1 / set_stream_mode(1), the default; 0: never). Round 4's
// branch-free step loop: 16 batched 1x4x1024^2 calls 23.6 vs 26.0 us for the ring kernel, 32
// calls 44.2 vs 49.8 (profiles/r04/stream_check.jsonl).
static std::atomic<int> g_stream_mode{-1};
static int stream_env() { return env_mode(g_stream_mode, "MHA_HD64_STREAM"); }
int set_stream_mode(int mode) {
    const int prev = stream_env();
    g_stream_mode.store(mode ? 1 : 0);
    return prev;
}
static bool stream_auto(const Call* calls, int n, InType in) {
    return in == InType::F16 && stream_env() > 0 && blocks_of(calls, n, 128) > 256;
}

GroupPlan plan_group(const Call* calls, int n, size_t ws_bytes, int force_q_waves, int force_kv_waves,
                     int force_splits, InType in) {
    if (force_q_waves == kForceStream || (force_q_waves == 0 && stream_auto(calls, n, in))) {
        if (in == InType::F16) {
            // 8 waves (256-row items, one workgroup per CU: the two waves of a SIMD stay in step, no
            // co-resident imbalance) when their last round of 256 items is at least 3/4 full; else
            // 4 (128-row items, two per CU: the older workgroup of a CU takes the extra items of a
            // partial round). tools/stream_check.py, 1024^2 calls per launch, us: 12 calls 20.0 vs
            // 21.1, 16: 22.5 vs 23.4, 24: 38.5 vs 34.0, 32: 43.3 vs 44.7, 64: 81.1 vs 84.3.
            // force_kv_waves 4 / 8 (forced plan 23) picks one.
            const long blocks256 = blocks_of(calls, n, 256);
            const long rounds8 = (blocks256 + 255) / 256;
            const int nw = (force_q_waves == kForceStream && (force_kv_waves == 4 || force_kv_waves == 8))
                               ? force_kv_waves
                               : (4 * (256 * rounds8 - blocks256) <= 256 ? 8 : 4);
            return no_split_plan(n, nw, nw, 32, 0);  // items of 32·nw rows (kv_waves: reported by the plan query)
        }
        force_q_waves = 0;  // fp32 inputs: the planner's choice
    }
    // 16-row blocks first: a launch of at most 256 of them runs every block on its own CU. Under a
    // concurrency hint >= 2 (several streams of independent calls) a call takes 32-row blocks on
    // half the CUs instead (launch_direct: two-per-CU form from hint 3), so the streams overlap.
    if (force_q_waves == kForceDirect16 ||
        (force_q_waves == 0 && direct16_enabled() && concurrency_hint() < 2)) {
        const int dt = direct_tiles_for(calls, n, in, force_q_waves == kForceDirect16, 16);
        if (dt > 0) return no_split_plan(n, 1, 4, 16, dt);
        if (force_q_waves == kForceDirect16) force_q_waves = 0;  // not applicable: the planner's choice
    }
    if (force_q_waves == kForceDirect || force_q_waves == 0) {
        const int dt = direct_tiles_for(calls, n, in, force_q_waves == kForceDirect);
        if (dt > 0) return no_split_plan(n, 1, 8, 32, dt);
        if (force_q_waves == kForceDirect) force_q_waves = 0;  // not applicable: the planner's choice
    }
    // Forced shapes (test/bench hook): q_waves >= 10 selects 64-row waves (RB = 2) of q_waves - 10.
    int rb = force_q_waves >= 10 ? 2 : 1;
    int qw = force_q_waves >= 10 ? force_q_waves - 10 : force_q_waves, kw = force_kv_waves;
    if (!valid_shape(qw, kw, rb)) {
        rb = 1;
        const long blocks128 = blocks_of(calls, n, 128);
        // (bench.py --sweep, profiles/r01/ring_plan_sweep.json; eager us per launch)
        if (blocks128 > 256) {
            // more than one round of 128-row blocks: 4 waves (48 KiB LDS, several workgroups per
            // CU) beat (4,2)'s 8 (96 KiB, one per CU): 1024^2 B=16 29.3 vs 33.1, 2048^2 B=8 51.5
            // vs 57.1, 1536^2 B=8 36.3 vs 40.8
            qw = 4;
            kw = 1;
        } else if (blocks128 > 128) {
            // one round of 128-row blocks: (4,2), no cross-WG split (1536^2 B=3 21.6 vs 29.0 for
            // the (2,2) split plans, B=4 22.6 vs 29.8; 1024^2 B=8 18.8 vs 19.6 for (4,1))
            qw = 4;
            kw = 2;
        } else {
            qw = 2;
            kw = 2;
            // A launch that does not fill the chip with 64-row blocks: one super-tile per split
            // (single-stage LDS ring, straight-line body) while the grid stays within one
            // residency round. First choice (1,8): 32 rows x 512 keys per workgroup (128 KiB
            // LDS, one workgroup per CU, <= 256 of them): half the splits of (2,4), so half the
            // partial round trip; else (2,4): 64 rows x 256 keys (72 KiB, two per CU, <= 512).
            long g64 = 0, wgs4 = 0, wgs8 = 0;
            bool fits4 = true, fits8 = true;
            for (int i = 0; i < n; ++i) {
                const long b = (long)calls[i].batch * calls[i].heads;
                const long g = b * ((calls[i].nq + 63) / 64);
                const long st4 = (calls[i].nkv + 255) / 256, st8 = (calls[i].nkv + 511) / 512;
                fits4 = fits4 && st4 <= kMaxSplits;
                fits8 = fits8 && st8 <= kMaxSplits;
                g64 += g;
                wgs4 += g * st4;
                wgs8 += b * ((calls[i].nq + 31) / 32) * st8;
            }
            if (g64 < 256 && fits8 && wgs8 <= 256) {
                qw = 1;
                kw = 8;
            } else if (g64 < 256 && fits4 && wgs4 <= 512) {
                kw = 4;
            }
        }
    }
    GroupPlan p{};
    p.q_waves = qw;
    p.kv_waves = kw;
    p.rows_per_wave = 32 * rb;
    const long groups = blocks_of(calls, n, 32 * qw * rb);
    // splits: as many as keep the grid within one round of 256 workgroups (a second partial
    // round costs more than the split saves: 1536^2 B=1 (2,2) 3-way 19.1 vs 2-way 13.9 us)
    int want = force_splits > 0 ? force_splits : (int)std::max(1L, 256 / std::max(1L, groups));
    want = std::max(1, std::min(want, kMaxSplits));
    if (kw >= 4) {
        // single-super-tile shapes: every split must be exactly one super-tile (their LDS ring
        // has one stage); otherwise (too many keys, or no workspace for the partials) use (2,2).
        size_t off = 0;
        bool ok = true;
        for (int i = 0; i < n; ++i) {
            const int super_total = std::max(1, (calls[i].nkv + 64 * kw - 1) / (64 * kw));
            ok = ok && super_total <= kMaxSplits;
            p.splits[i] = super_total;
            p.tiles_per_split[i] = 1;
            p.ws_offset[i] = off;
            off += split_workspace_bytes(calls[i], super_total);
        }
        p.ws_needed = off;
        if (ok && off <= ws_bytes) return p;
        return plan_group(calls, n, ws_bytes, 2, 2, force_splits, in);
    }
    for (;;) {
        size_t off = 0;
        for (int i = 0; i < n; ++i) {
            const int super_total = std::max(1, (calls[i].nkv + 64 * kw - 1) / (64 * kw));
            const int w = std::min(want, super_total);
            p.tiles_per_split[i] = (super_total + w - 1) / w;
            p.splits[i] = (super_total + p.tiles_per_split[i] - 1) / p.tiles_per_split[i];
            p.ws_offset[i] = off;
            off += split_workspace_bytes(calls[i], p.splits[i]);
        }
        p.ws_needed = off;
        if (want <= 1 || off <= ws_bytes) break;
        --want;
    }
    return p;
}

// ---- Float boundary onto the single-pass kernels (the convert launch: mha_hd64_ring.hip) ----
static bool f32_convert_enabled() { static const bool on = env_on("MHA_HD64_F32_CONVERT"); return on; }
// fp32 inputs rounded inside the 16-row kernel (one launch) where its one-pass forms apply
// (MHA_HD64_F32_INKERNEL=0 or set_f32_inkernel(0): the convert launch + fp16 kernel instead).
// 2 (MHA_HD64_F32_INKERNEL=2 / set_f32_inkernel(2)): the two-pass forms (1024 < nkv <= 2048) round
// fp32 in the kernel too. Diagnostic: measured slower than convert + fp16 kernel.
static std::atomic<int> g_f32_inkernel{-1};
static int f32_inkernel_mode() { return env_mode(g_f32_inkernel, "MHA_HD64_F32_INKERNEL", true); }
void set_f32_inkernel(int enable) { g_f32_inkernel.store(enable <= 0 ? 0 : enable >= 2 ? 2 : 1); }

// Whether an fp32-input launch whose fp16 plan is p16 takes the convert launch + that fp16 kernel
// (true) or the ring kernel rounding fp32 on load (false). The 32-row single-pass kernel after a
// convert loses to the ring kernel past one round of its blocks and at short key ranges, where
// the ring kernel's 128-row blocks share each K/V tile over four query waves (tools/f32_routes.py,
// profiles/r03/f32_routes.jsonl, us per launch, convert + 32-row kernel vs ring: 4x4x1024^2 16.4
// vs 13.9, 4x4x512^2 8.7 vs 7.6; kept: 2x4x1024^2 10.4 vs 12.8, 2x4x2048^2 22.4 vs 22.1).
static bool f32_convert_route(const Call* calls, int n, const GroupPlan& p16) {
    if (p16.stream) return true;
    if (p16.direct_tiles == 0) return false;
    if (p16.rows_per_wave == 16) return true;  // the 16-row kernel's two-pass forms (nkv > 1024)
    int max_nkv = 0;
    for (int i = 0; i < n; ++i) max_nkv = std::max(max_nkv, calls[i].nkv);
    return blocks_of(calls, n, 32) <= 256 && max_nkv > 512;
}

ChunkRoute route_chunk(const Call* calls, int n, InType in, size_t ws_bytes, bool has_workspace, int force_q_waves,
                       int force_kv_waves, int force_splits) {
    // fp32 inputs onto the fp16 kernels, unless a plan is forced or MHA_HD64_F32_CONVERT=0
    if (in == InType::F32 && force_q_waves == 0 && force_kv_waves == 0 && force_splits == 0 && f32_convert_enabled()) {
        const GroupPlan p16 = plan_group(calls, n, 0, 0, 0, 0, InType::F16);
        // rounded in the 16-row kernel: one-pass forms only (nkv <= 1024): the two-pass form rounding
        // fp32 in the kernel measured slower than convert + fp16 kernel (1x4x1024x2048 11.32 vs
        // 10.75 us, 512x1536 9.78 vs 9.24; profiles/r02/float_inkernel.jsonl)
        const int mode = f32_inkernel_mode();
        if (mode >= 1 && p16.direct_tiles > 0 && p16.direct_tiles <= (mode == 2 ? 4 : 2) && p16.rows_per_wave == 16)
            return {Route::F32InKernel, p16, 0};
        // convert launch + fp16 kernel, where the caller's workspace holds the fp16 copies; else
        // the planned launch below (the ring kernel rounds on load)
        if (has_workspace && f32_convert_route(calls, n, p16)) {
            size_t need = 0;
            for (int i = 0; i < n; ++i) {
                if (calls[i].nq <= 0 || calls[i].batch <= 0 || calls[i].heads <= 0) continue;
                need += f16_copy_bytes(calls[i], calls[i].nq) + 2 * f16_copy_bytes(calls[i], calls[i].nkv);
            }
            if (need <= ws_bytes) return {Route::F32Convert, p16, need};
        }
    }
    const GroupPlan p =
        plan_group(calls, n, has_workspace ? ws_bytes : 0, force_q_waves, force_kv_waves, force_splits, in);
    return {Route::Planned, p, p.ws_needed};
}

size_t group_workspace_bytes(const Call* calls, int n, InType in) {
    size_t need = 0;
    for (int i = 0; i < n; i += kGroupCalls)
        need = std::max(need, route_chunk(calls + i, std::min(kGroupCalls, n - i), in, (size_t)-1, true).ws_bytes);
    return need;
}

}  // namespace mha_hd64
