// lightglue_ffn_ln.hip — the FFN's input projection with LayerNorm + GELU in its epilogue, as a gfx950
// MFMA tile kernel (include/lightglue_glue.h: lg_linear_cat_ln_gelu). fp16 in/out, fp32 accumulation.
// LinArgs, the A-gather and the 256-row forms' DMA sources are shared with the projections
// (lightglue_linear.hip) through lightglue_device.h; the two-launch fallback calls lg_linear_cat and
// lg_layernorm_gelu through the C ABI. The whole FFN in one launch: lightglue_ffn.hip.
#ifdef LG_LN_STAMPS
#define FFN_STAMPS
#endif
#include <atomic>

#include "lightglue_ffn_device.h"

namespace {

// LightGlue's FFN (lightglue.py:101-106) is Linear(2d, 2d) -> LayerNorm(2d) -> GELU -> Linear(2d, d):
// lg_linear_cat writes h = [x | heads]·Wᵀ + b, a separate pass normalises it (17 us at P = 16, M =
// 32,768: 33.5 MB read, 33.5 MB written; profiles/r05/matcher_p16_kernel_stats_tile_forms_v1.csv).
// Here a workgroup owns whole rows: tiles of 128 rows x all 512 channels (8 waves as 2 (m) x 4 (n)
// tiles of 64 x 128; K in 32-deep steps through a 3-stage LDS-DMA ring of 40 KiB stages, the A-gather
// of lg_linear_cat), so the row statistics close inside the workgroup: h = fp16(acc + bias) as the
// unfused path rounds it, row sums per wave -> LDS -> mean; sums of (h - mean)^2 -> LDS -> variance
// (two passes over registers, as the unfused kernel: E[h^2] - mean^2 cancels in fp32), then
// GELU(LN(h)) (the erf of A&S 7.1.26, as the unfused fp16 kernel) rounded to fp16, staged and
// stored as in linear_tile_kernel. bias, gamma and beta sit in LDS for the whole launch.
// Diagnostic build (-DLG_LN_STAMPS, tools/ln_stamps.py; never shipped): per wave, the stamps of
// lightglue_ffn_device.h by chained segment (0 prologue, 1 K-step waits + barriers, 2 K-step DMA issue +
// fragment reads + MFMAs, 3 epilogue: h and row statistics, 4 epilogue: normalise, GELU, staging,
// stores; slot 6: the workgroup's tiles), read back by lg_diag_ln_stamps.
// the one-launch form's two tiles: 128 rows with 32-deep K steps through 3 stages of 40 KiB, and
// 64 rows with 64-deep K steps through 2 stages of 72 KiB (twice the W bytes per row: it pays only
// while the 128-row tiles would leave CUs idle; see lg_linear_cat_ln_gelu)
template <int KS, int MT, int BK, int NST, int NWV = 8>
__global__ __launch_bounds__(64 * NWV, NWV == 4 ? 2 : 1) void linear_ln_kernel(LinArgs p, const f16* __restrict__ gamma,
                                                                              const f16* __restrict__ beta, float eps) {
    constexpr int NT = kLnN;
    constexpr int WM = MT / 64, WN = NWV / WM, WTN = NT / WN, NB = WTN / 32, NP = WTN / 64;
    constexpr int SB = (MT + NT) * BK * 2;                             // 40 KiB
    constexpr int NWP = NT * BK * 2 / (NWV * 1024), NAP = MT * BK * 2 / (NWV * 1024);  // pieces per wave and step
    constexpr int D = NWP + NAP;
    constexpr int SPW = 2 * NP * 4;
    constexpr int kPar = NST * SB;                  // vectors: bias, gamma, beta [512] fp16
    constexpr int kRed = kPar + 3 * NT * 2;         // row partials [2][MT][WN] fp32
    static_assert((NST - 2) * D + SPW <= 63 && KS >= NST - 1, "shape");
    __shared__ __attribute__((aligned(16))) char smem[kRed + 2 * MT * WN * 4];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 31, hh = lane >> 5;
    const int T = p.total, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int q8 = T >> 3, r8 = T & 7;
    const int jb = xcd * q8 + min(xcd, r8), je = jb + q8 + (xcd < r8 ? 1 : 0);
    const int G = ((int)gridDim.x - xcd + 7) >> 3;
    const int j0 = jb + loc;
    if (j0 >= je) return;
    const int ntile_w = (je - j0 + G - 1) / G;
    const int nsteps = ntile_w * KS;
    FFN_STAMPS_BEGIN();

    auto src_of = [&](int t) { return tile_src<true, BK, NWP, NAP, NWV>(p, (j0 + G * t) * MT, 0, wave, lane); };
    // the vectors into LDS (loaded ahead of the first stages, written after them: the compiler's wait
    // counts the DMA pieces), visible after the first step's barrier
    f16x8 pv = {};
    const f16* const pvs = tid < 64 ? p.bias : tid < 128 ? gamma : beta;
    if (tid < 192) pv = *reinterpret_cast<const f16x8*>(pvs + (tid & 63) * 8);
    TileSrc<NWP, NAP> cur = src_of(0);  // (the next tile's sources are computed where used: registers)
#pragma unroll
    for (int i = 0; i < NST - 1; ++i) tile_issue<true, BK, KS, NT, NWV>(cur, i, smem + i * SB, wave);
    if (tid < 192) *(lds_f16x8*)(lds + kPar + tid * 16) = pv;

    auto swz = [](int row) { return BK == 64 ? (row >> 1) & 7 : (row >> 2) & 3; };
    unsigned wro[NB], aro[2];
    int wsw[NB], asw[2];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int wrow = wn * WTN + 32 * b + r;
        wro[b] = (unsigned)(wrow * BK * 2), wsw[b] = swz(wrow);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int arow = wm * 64 + 32 * b + r;
        aro[b] = (unsigned)(NT * BK * 2 + arow * BK * 2), asw[b] = swz(arow);
    }
    const int cr = lane >> 3, cc = lane & 7;
    float* const red = (float*)(void*)(smem + kRed);  // [pass][row][wn]
    auto red_sum = [&](int off) {  // the WN partials of a row, in a fixed order
        float v = 0.f;
#pragma unroll
        for (int q = 0; q < WN; q += 4) {
            const f32x4 w4 = *(__attribute__((address_space(3))) f32x4*)(lds + kRed + (off + q) * 4);
            v += (w4[0] + w4[1]) + (w4[2] + w4[3]);
        }
        return v;
    };
    int st = 0;
    for (int t = 0; t < ntile_w; ++t) {
        const int m0 = (j0 + G * t) * MT;
        const bool more = t + 1 < ntile_w;
        f32x16 acc[NB][2] = {};
        int st_last = 0;
#pragma unroll 2
        for (int ks = 0; ks < KS; ++ks) {
            const int gs = t * KS + ks;
            if (ks == 0 && t == 0) FFN_SEG(0);
            else FFN_SEG(2);
            if (gs + NST - 2 > nsteps - 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else if (ks < NST - 1 && t > 0) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D + SPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D) : "memory");
            __builtin_amdgcn_s_barrier();
            FFN_SEG(1);
            {
                char* const fb = smem + (st == 0 ? NST - 1 : st - 1) * SB;
                if (ks + NST - 1 < KS) tile_issue<true, BK, KS, NT, NWV>(cur, ks + NST - 1, fb, wave);
                else if (more) tile_issue<true, BK, KS, NT, NWV>(src_of(t + 1), ks + NST - 1 - KS, fb, wave);
            }
            const unsigned sb = (unsigned)(st * SB);
            st_last = st;
            st = st == NST - 1 ? 0 : st + 1;
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
                const int u = 2 * s + hh;
                f16x8 wf[NB], af[2];
#pragma unroll
                for (int b = 0; b < NB; ++b) wf[b] = *(lds_f16x8*)(lds + sb + wro[b] + ((u ^ wsw[b]) << 4));
#pragma unroll
                for (int b = 0; b < 2; ++b) af[b] = *(lds_f16x8*)(lds + sb + aro[b] + ((u ^ asw[b]) << 4));
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int mb = 0; mb < 2; ++mb)
                        acc[nb][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[nb], af[mb], acc[nb][mb], 0, 0, 0);
            }
        }

        FFN_SEG(2);
        // ---- epilogue: h = fp16(acc + bias) (lane: row wm*64 + 32 mb + r, 64 of the wave's channels) ----
        const int nw0 = wn * WTN;
        float rs[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            float s = 0.f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const u32x2 b4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + (nw0 + 32 * nb + 8 * g + 4 * hh) * 2);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const float a = acc[nb][mb][4 * g + u];
                        const float h = (u & 1) ? mixh<1>(a, b4[u >> 1]) : mixh<0>(a, b4[u >> 1]);
                        acc[nb][mb][4 * g + u] = h;
                        s += h;
                    }
                }
            rs[mb] = s + __shfl_xor(s, 32, 64);  // the wave's 128 channels of the row
        }
        // row sums across the 4 n-waves (this tile's partials: every wave is past the last K step's
        // reads once it reaches the barrier below, and past the previous tile's statistics reads)
        if (hh == 0) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) red[(wm * 64 + 32 * mb + r) * WN + wn] = rs[mb];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        float mean[2];
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            mean[mb] = red_sum((wm * 64 + 32 * mb + r) * WN) * (1.f / kLnN);
            float q = 0.f;
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float d = acc[nb][mb][e] - mean[mb];
                    acc[nb][mb][e] = d;  // (h - mean, reused by the normalisation)
                    q = __builtin_fmaf(d, d, q);
                }
            rs[mb] = q + __shfl_xor(q, 32, 64);
        }
        if (hh == 0) {
#pragma unroll
            for (int mb = 0; mb < 2; ++mb) red[MT * WN + (wm * 64 + 32 * mb + r) * WN + wn] = rs[mb];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // (also: every wave is done reading the last stage)
        FFN_SEG(3);
        lds_char* const stg = lds + st_last * SB + wave * 4096;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb) {
            const float rstd = __builtin_amdgcn_rsqf(red_sum(MT * WN + (wm * 64 + 32 * mb + r) * WN) * (1.f / kLnN) + eps);
#pragma unroll
            for (int np = 0; np < NP; ++np) {
#pragma unroll
                for (int nbl = 0; nbl < 2; ++nbl)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int n = nw0 + 64 * np + 32 * nbl + 8 * g + 4 * hh;
                        const u32x2 g4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + NT * 2 + n * 2);
                        const u32x2 b4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + 2 * NT * 2 + n * 2);
                        f16x4 o;
#pragma unroll
                        for (int u = 0; u < 4; u += 2) {
                            const f32x16& av = acc[2 * np + nbl][mb];
                            const f32x2 xr = f32x2{av[4 * g + u], av[4 * g + u + 1]} * rstd;
                            const f32x2 gl = gelu_as2(f32x2{mixf<0>(xr[0], g4[u >> 1], b4[u >> 1]), mixf<1>(xr[1], g4[u >> 1], b4[u >> 1])});
                            o[u] = (f16)gl[0];
                            o[u + 1] = (f16)gl[1];
                        }
                        *(__attribute__((address_space(3))) f16x4*)(stg + r * 128 + (((4 * nbl + g) ^ (r & 7)) << 4) + 8 * hh) = o;
                    }
                f16x8 o8[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rl = 8 * i + cr;
                    o8[i] = *(lds_f16x8*)(stg + rl * 128 + ((cc ^ (rl & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = min(m0 + wm * 64 + 32 * mb + 8 * i + cr, p.m - 1);
                    st_out(p.out[0] + (size_t)row * NT + nw0 + 64 * np + 8 * cc, o8[i]);
                }
            }
        }
        if (more) cur = src_of(t + 1);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FFN_SEG(4);
    FFN_STAMPS_WRITE(wave, (unsigned long long)ntile_w, 0);
}

// lg_linear_cat_ln_gelu's one-launch form (linear_ln_kernel), by size: its 128-row tiles from one
// full round of them on (256: M >= 32,768 rows, P >= 16 pairs of 1024 keypoints), its 64-row tiles
// from a full round of those (256: M >= 16,384), two launches below. Measured against the two launches
// (profiles/r05/ln_fused_by_size.jsonl, ln64_by_size.jsonl; op alone, us, two launches / 128-row /
// 64-row): P = 1 9.2 / 28.3 / 16.8, P = 4 19.7 / 29.4 / 18.3, P = 8 27.1-27.7 / 32.2 / 21.9, P = 16
// 42.2 / 36.3-39.4 / 38.4, P = 32 74.4-77.7 / 72.7 / 77.0 (few workgroups: each one's GELU vector work
// runs after its GEMM with no other wave's MFMAs beside it; more rows per tile: fewer W bytes per
// row); whole forwards P = 8 1.53-1.54 -> 1.45-1.47 ms (64-row), P = 16 2.541 -> 2.487 (128-row), P =
// 32 4.701 -> 4.642, but P = 4 (half a round of 64-row tiles) 1.03-1.04 -> 1.05-1.06 (profiles/r05/
// ln64_forms_forwards.txt). lg_linear_set_ln_fused: 1 by size (default), 0 always two launches, 2 always one.
std::atomic<int> g_ln_fused{1};
}  // namespace

extern "C" {

int32_t lg_linear_set_ln_fused(int32_t on) { return g_ln_fused.exchange(on == 2 ? 2 : on ? 1 : 0); }

int32_t lg_linear_cat_ln_gelu(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                              int32_t pairs, const void* w, const void* bias, const void* gamma, const void* beta,
                              float eps, void* out, hipStream_t stream) {
    const int k = 2 * heads * kD, m = pairs * (n0 + n1), n = k;
    if (heads <= 0 || n0 < 0 || n1 < 0 || pairs < 0 || !shape_ok(m, n, k) || !x || !w || !bias || !gamma || !beta ||
        !out || !aligned16(x) || (n0 && !aligned16(ctx0)) || (n1 && !aligned16(ctx1)) || !aligned16(w) ||
        !aligned8(bias) || !aligned8(out) || !(eps >= 0.f))
        return bad("lg_linear_cat_ln_gelu");
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;
    const int lnf = g_ln_fused.load();  // 1: by size; 2: at every size (A/B)
    const bool big = m >= 128 * kTileGrid;  // a full round of 128-row tiles (32,768 rows)
    const bool fused = lnf && n == kLnN && (lnf == 2 || big || m >= 64 * kTileGrid) && aligned16(bias) && aligned16(gamma) &&
                       aligned16(beta) && aligned16(out) && lightglue::wide_mode() != 0;
    if (!fused) {  // the projection, then LayerNorm+GELU in place (lightglue_glue.hip)
        const int32_t st = lg_linear_cat(x, ctx0, ctx1, heads, n0, n1, pairs, w, bias, n, out, stream);
        if (st != MHA_HD64_STATUS_SUCCESS) return st;
        return lg_layernorm_gelu(MHA_HD64_DT_HALF, out, gamma, beta, m, n, eps, out, stream);
    }
    LinArgs p = gather_args(x, ctx0, ctx1, w, bias, out, heads, n0, n1, pairs, n, k);
    p.mtiles = big ? (m + 127) / 128 : (m + 63) / 64;
    p.total = p.mtiles;
    const int grid = p.total < kTileGrid ? p.total : kTileGrid;
    if (big)
        hipLaunchKernelGGL((linear_ln_kernel<512 / 32, 128, 32, 3>), dim3(grid), dim3(512), 0, stream, p,
                           (const f16*)gamma, (const f16*)beta, eps);
    else
        hipLaunchKernelGGL((linear_ln_kernel<512 / 64, 64, 64, 2>), dim3(grid), dim3(512), 0, stream, p,
                           (const f16*)gamma, (const f16*)beta, eps);
    return launched("lg_linear_cat_ln_gelu");
}

}  // extern "C"
FFN_STAMPS_READBACK(lg_diag_ln_stamps)
