// lightglue_ffn.hip — the matcher's FFN as gfx950 MFMA kernels (include/lightglue_glue.h:
// lg_linear_cat_ln_gelu, lg_linear_cat_ffn, lg_ffn_pack, lg_linear_cat_ffn_proj). fp16 in/out, fp32
// accumulation. LinArgs, the A-gather, the output arithmetic and the 256-row forms' DMA sources are
// shared with the projections (lightglue_linear.hip) through lightglue_device.h; the two-launch
// fallbacks call lg_linear_cat, lg_layernorm_gelu and lg_linear through the C ABI.
#include <stdlib.h>

#include <atomic>
#include <cstdlib>

#include "lightglue_device.h"

namespace {

// ---- the FFN input projection with LayerNorm + GELU in its epilogue (lg_linear_cat_ln_gelu) ----
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
// Diagnostic build (-DLG_LN_STAMPS, tools/ln_stamps.py; never shipped): per wave, s_memtime cycles
// of linear_ln_kernel by chained segment (0 prologue, 1 K-step waits + barriers, 2 K-step DMA issue +
// fragment reads + MFMAs, 3 epilogue: h and row statistics, 4 epilogue: normalise, GELU, staging,
// stores), read back by lg_diag_ln_stamps.
#ifdef LG_LN_STAMPS
__device__ unsigned long long g_ln_stamps[256 * 8 * 8];
#define LN_SEG(k)                                                                                    \
    do {                                                                                             \
        unsigned long long t_;                                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        sg_[k] += t_ - last_;                                                                        \
        last_ = t_;                                                                                  \
    } while (0)
#else
#define LN_SEG(k) \
    do {          \
    } while (0)
#endif
constexpr int kLnN = 512;
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
#ifdef LG_LN_STAMPS
    unsigned long long sg_[5] = {0, 0, 0, 0, 0}, last_, t_entry_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_entry_)::"memory");
    last_ = t_entry_;
#endif

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
            if (ks == 0 && t == 0) LN_SEG(0);
            else LN_SEG(2);
            if (gs + NST - 2 > nsteps - 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else if (ks < NST - 1 && t > 0) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D + SPW) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D) : "memory");
            __builtin_amdgcn_s_barrier();
            LN_SEG(1);
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

        LN_SEG(2);
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
        LN_SEG(3);
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
    LN_SEG(4);
#ifdef LG_LN_STAMPS
    if (lane == 0) {
        unsigned long long* d = g_ln_stamps + ((size_t)blockIdx.x * 8 + wave) * 8;
        for (int k = 0; k < 5; ++k) d[k] = sg_[k];
        d[5] = last_ - t_entry_;
        d[6] = (unsigned long long)ntile_w;
    }
#endif
}


constexpr int kFfnOut = 256;  // the FFN's output channels (d)

// ---- the whole FFN in one launch, whole rows per workgroup (lg_linear_cat_ffn, round 6) ----
// out = x + fp16(W2 · GELU(LN(fp16(W1 · [x | heads] + b1))) + b2) with one workgroup per MT = 32 MB rows.
// At a single image pair (M = 1,024..4,096) the FFN was three launches of ~5 us each, every one near
// the launch floor (profiles/r05/single_pair_timelines.txt: 269 of 557 us of a forward at n = 1,024).
// Here one launch: 8 waves, wave w owns hidden channels [64w, 64w + 64) in phase 1 and output
// channels [32w, 32w + 32) in phase 2, so every weight fragment a wave multiplies is its own — W1 and
// W2 stream from L2 straight into VGPRs in the MFMA A-operand layout (lane (r, hh): row r of the
// wave's 32-channel block, k = 16 s + 8 hh .. + 8 of step s; lg_ffn_pack stores them in that order,
// so every load is one contiguous KiB), D steps ahead, as ONE stream that runs from phase 1 into
// phase 2 (W2's first fragments load under the LayerNorm); no barrier in either GEMM loop. The MT
// activation rows [x | heads] (the A-gather of lg_linear_cat) sit in LDS for the whole launch (rows of
// 1 KiB with 16-B units XOR (row & 15): conflict-free ds_read_b128 of 16 rows at one k), as does GELU's
// output h (the second GEMM's B operand, the same layout); the residual x is read back from the A tile.
// Per workgroup the weights are 768 KiB whatever MT (~12 k cycles at the ~64 B/clk a CU takes in):
// MT = 32 (MB = 1) gives the most workgroups for a few rows (latency: single pairs), MT = 64 (MB = 2)
// halves the weight bytes per row where there are rows enough for several rounds (its MFMA work,
// 12 k cycles per SIMD, then matches the stream).
// Arithmetic: the k16 blocks in the 64 x 64 form's order; h = fp16(acc + b1) in one rounding, the
// LayerNorm statistics from each wave's (sum, sum of squares about its own mean) of its 64 channels,
// merged over the 8 waves in a fixed order (ln_merge: no E[h^2] - mean^2 cancellation),
// normalisation and GELU as linear_ln_kernel, the output fp16(fp16(acc + b2) + x) as lin_val / res_add.
// phase 3 (lg_linear_cat_ffn_proj): the next attention's projection of the FFN output x'
enum { E3_NONE = 0, E3_SPLIT2 = 1, E3_QKV = 2, E3_PLAIN = 3 };
struct Proj3 {
    const f16* b3;      // [n3] bias
    const f16* cosv;    // E3_QKV: rotary tables [m, 64]
    const f16* sinv;
    f16* out[6];        // SPLIT2: a0 a1 b0 b1; QKV: q0 k0 v0 q1 k1 v1 (per-image head-major); PLAIN: [m, n_store]
    int n_store;        // E3_PLAIN: channels stored per row (the first n_store of 32 NB3 8)
};
// (Tried and dropped: a workgroup barrier every few 1-KiB pieces of the weight stream, so that no wave
// runs ahead of the others' streams; P = 1 / 4 / 16 FFN 10.0 / 14.6 / 46.0 us without, 10.1 / 15.1 / 46.4
// with one every 8: the CU's stream is bandwidth-bound either way, profiles/r06/ffn_wave_sync_ab.jsonl.)
// Diagnostic build (-DLG_FR_STAMPS, tools/fr_stamps.py; never shipped): per wave of the first 256
// workgroups, s_memtime cycles of chained segments (0 entry -> A in LDS, 1 phase 1, 2 LayerNorm + GELU,
// 3 phase 2, 4 epilogue), read back by lg_diag_fr_stamps.
#ifdef LG_FR_STAMPS
__device__ unsigned long long g_fr_stamps[256 * 8 * 8];
#define FR_SEG(k)                                                                                    \
    do {                                                                                             \
        unsigned long long t_;                                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
        fr_[k] = t_ - fr_last_;                                                                      \
        fr_last_ = t_;                                                                               \
    } while (0)
#else
#define FR_SEG(k) \
    do {          \
    } while (0)
#endif
// The squares of one packed pair about c: q += ((h.lo - c)^2, (h.hi - c)^2), the differences one fp32
// rounding each (v_fma_mix_f32 reads the halves in place), both squares in one v_pk_fma_f32
__device__ __forceinline__ void row_dev2(unsigned h2, float c, f32x2& q) {
    const f32x2 d = f32x2{mixn<0>(h2, 1.f, -c), mixn<1>(h2, 1.f, -c)};
    q = d * d + q;
}
// A row's mean and 1 / sqrt(variance + eps) over its 512 channels from the 8 waves' partials: s[w] the
// sum of wave w's 64 channels, q[w] their squares about that wave's own mean s[w] / 64. The variance is
// (sum q + 64 sum (s[w] / 64 - mean)^2) / 512 — the pairwise merge of (mean, M2), every term a square —
// so a row mean far from zero costs no bits (the one-pass E[h^2] - mean^2 lost log2((mean / sigma)^2)).
struct RowStats {
    float mean, rstd;
};
__device__ __forceinline__ RowStats ln_merge(f32x4 sa, f32x4 sc, f32x4 qa, f32x4 qc, float eps) {
    const float mean = (((sa[0] + sa[1]) + (sa[2] + sa[3])) + ((sc[0] + sc[1]) + (sc[2] + sc[3]))) * (1.f / 512);
    const f32x4 da = sa * (1.f / 64) - mean, dc = sc * (1.f / 64) - mean;
    const f32x4 ba = da * da, bc = dc * dc;
    const float within = ((qa[0] + qa[1]) + (qa[2] + qa[3])) + ((qc[0] + qc[1]) + (qc[2] + qc[3]));
    const float between = ((ba[0] + ba[1]) + (ba[2] + ba[3])) + ((bc[0] + bc[1]) + (bc[2] + bc[3]));
    return {mean, __builtin_amdgcn_rsqf(fmaf(between, 64.f, within) * (1.f / 512) + eps)};
}
template <int MB, int D, int E3, int NB3>
__global__ __launch_bounds__(512, 1) void ffn_rows_kernel(LinArgs p, const f16* __restrict__ gamma,
                                                          const f16* __restrict__ beta, float eps,
                                                          const f16* __restrict__ wp, const f16* __restrict__ b2,
                                                          Proj3 q3) {
    constexpr int MT = 32 * MB;                    // rows per workgroup
    constexpr int K = 512, NO = kFfnOut;           // FFN width (= hidden), output channels
    constexpr int kA = 0, kH = MT * K * 2;         // A and h tiles, [MT][1 KiB] each
    constexpr int kSP = 80;                        // output staging pitch (64 B of a row + 16)
    constexpr int kStg = MB == 1 ? 2 * kH : kH;    // staging: its own region (MB = 1), else over h
    constexpr int kPar = MB == 1 ? kStg + 8 * MT * kSP : 2 * kH;  // b1, gamma, beta [512], b2 [256] fp16
    constexpr int kRed = kPar + (3 * K + NO) * 2;  // row partials [2][MT][8 waves] fp32
    constexpr int NS1 = K / 16, NS = 2 * NS1;      // k16 steps per GEMM; the stream: phase 1, then 2
    constexpr int NS3 = NO / 16;                   // phase 3: k16 steps over x' (K = 256)
    constexpr int NP = 96 + NB3 * NS3;             // the wave's stream: pieces of 1 KiB
    constexpr int R = 2 * D;                       // pieces in flight (a register ring)
    static_assert(D >= 1 && D <= NS1 && (MB == 1 || MB == 2) && (E3 == E3_NONE) == (NB3 == 0), "shape");
    static_assert(MB == 1 || 8 * MT * kSP <= kH, "staging over h");
    // phase 3's vectors, loaded with A: b3 [32 NB3 8] fp16 and (E3_QKV) this tile's rows of cos / sin
    constexpr int kB3 = kRed + 2 * MT * 8 * 4;
    constexpr int kCS = kB3 + NB3 * 256 * 2;           // [2][MT] rows of 64 fp16, 144-B pitch (36 banks
    constexpr int kCSP = 144;                          // a row apart: a column read by 32 rows 2-way, where
    constexpr int kEnd = kCS + (E3 == E3_QKV ? 2 * MT * kCSP : 0);  // a 128-B pitch was 16-way)
    static_assert(kEnd <= 160 * 1024, "LDS");
    __shared__ __attribute__((aligned(16))) char smem[kEnd];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int m0 = blockIdx.x * MT;
#ifdef LG_FR_STAMPS
    unsigned long long fr_[6] = {0, 0, 0, 0, 0, 0}, fr_last_, fr_entry_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(fr_entry_)::"memory");
    fr_last_ = fr_entry_;
#endif

    // ---- A tile: row 8 i + wave, 16-B unit `lane` (x: units 0..31, head h of the attention output:
    // units 32 + 8 h .. + 7), loaded whole-row coalesced; rows past m repeat row m - 1 ----
    // The A tile in two halves (32-row tiles; the 64-row form measured 45.6 -> 47.6 us with it at P = 16): the
    // x half first, then the heads half — row 16 i + 2 w + lane / 32, unit lane % 32 of each; phase 1's first
    // half (k < 256) runs on x while the heads land
    constexpr bool AH = MB == 1;
    f16x8 av[AH ? 1 : 4 * MB], ax[2 * MB], ac[2 * MB];
    if constexpr (AH) {
#pragma unroll
        for (int i = 0; i < 2 * MB; ++i) {
            const int grow = min(m0 + 16 * i + 2 * wave + (lane >> 5), p.m - 1);
            ax[i] = *reinterpret_cast<const f16x8*>(p.a + (size_t)grow * (K / 2) + (lane & 31) * 8);
        }
#pragma unroll
        for (int i = 0; i < 2 * MB; ++i) {
            const int grow = min(m0 + 16 * i + 2 * wave + (lane >> 5), p.m - 1);
            const LinRow lr = lin_row(p, grow, (lane & 31) >> 3);
            ac[i] = *reinterpret_cast<const f16x8*>((lr.first ? p.ctx0 : p.ctx1) + lr.off + (lane & 7) * 8);
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4 * MB; ++i) {
            const int grow = min(m0 + 8 * i + wave, p.m - 1);
            const f16* src;
            if (lane < 32) {
                src = p.a + (size_t)grow * (K / 2) + lane * 8;
            } else {
                const LinRow lr = lin_row(p, grow, (lane - 32) >> 3);
                src = (lr.first ? p.ctx0 : p.ctx1) + lr.off + ((lane - 32) & 7) * 8;
            }
            av[i] = *reinterpret_cast<const f16x8*>(src);
        }
    }
    // the epilogue vectors: b1 / gamma / beta (64 units each) and b2 (32 units)
    f16x8 pv = {};
    if (tid < 224) {
        const f16* const pvs = tid < 64 ? p.bias : tid < 128 ? gamma : tid < 192 ? beta : b2;
        pv = *reinterpret_cast<const f16x8*>(pvs + (tid & 63) * 8);
    }

    constexpr int NV3 = NB3 * 256 * 2 / 16 + (E3 == E3_QKV ? 2 * MT * kD * 2 / 16 : 0);  // 16-B units
    constexpr int NV3T = (NV3 + 511) / 512;
    f16x8 v3[NV3T > 0 ? NV3T : 1];
#pragma unroll
    for (int i = 0; i < NV3T; ++i) {
        const int u = i * 512 + tid;
        if (u < NB3 * 256 * 2 / 16) {
            v3[i] = *reinterpret_cast<const f16x8*>(q3.b3 + u * 8);
        } else if (u < NV3) {  // cos / sin rows: table t, row rw (clamped), unit cu
            const int cu = u - NB3 * 256 * 2 / 16, t = cu / (MT * 8), rw = min(m0 + (cu % (MT * 8)) / 8, p.m - 1);
            v3[i] = *reinterpret_cast<const f16x8*>((t ? q3.sinv : q3.cosv) + (size_t)rw * kD + (cu % 8) * 8);
        }
    }

    // every wave's A loads are issued before any wave's weight stream: the loads of a CU pass its
    // texture unit in issue order, and A behind seven waves' weight prefetch waited ~2.6 k cycles
    asm volatile("s_barrier" ::: "memory");

    // ---- the weight stream (lg_ffn_pack's layout): wave w's 96 KiB, piece i at w * 96 KiB + i KiB,
    // lane l's 16 B at + 16 l: step j of phase 1, block b = piece 2 j + b; step j of phase 2 = 64 + j.
    // Every load is one contiguous KiB (whole 128-B lines: the row-major W's 32-B row pieces per
    // lane fetched each line four times, 26 vs 12 us per launch at 2,048 rows) ----
    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(wp), (short)0, 8 * NP * 1024, 0x00020000);
    const unsigned wo = (unsigned)(wave * NP * 1024 + lane * 16);
    auto piece = [&](int i) { return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wo, i * 1024, 0)); };
    f16x8 q[R];  // piece i in slot i % R; consuming piece i issues piece i + R
#pragma unroll
    for (int i = 0; i < R; ++i) {  // (in stream order: the loops' counted waits assume it)
        q[i] = piece(i);
        if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
    auto take = [&](int i) {  // piece i (compile-time after unrolling), and the refill behind it
        const f16x8 w = q[i % R];
        if (i + R < NP) q[i % R] = piece(i + R);
        return w;
    };
    // A and the vectors into LDS (the compiler's wait counts the weight loads issued after them)
    auto put_half = [&](const f16x8 (&hv)[2 * MB], int u0) {
#pragma unroll
        for (int i = 0; i < 2 * MB; ++i) {
            const int row = 16 * i + 2 * wave + (lane >> 5), u = u0 + (lane & 31);
            *(lds_f16x8*)(lds + kA + row * 1024 + ((u ^ (row & 15)) << 4)) = hv[i];
        }
    };
    if constexpr (AH) {
        put_half(ax, 0);
    } else {
#pragma unroll
        for (int i = 0; i < 4 * MB; ++i) {
            const int row = 8 * i + wave;
            *(lds_f16x8*)(lds + kA + row * 1024 + ((lane ^ (row & 15)) << 4)) = av[i];
        }
    }
    if (tid < 224) *(lds_f16x8*)(lds + kPar + tid * 16) = pv;
#pragma unroll
    for (int i = 0; i < NV3T; ++i)
        if (i * 512 + tid < NB3 * 256 * 2 / 16) {
            *(lds_f16x8*)(lds + kB3 + (i * 512 + tid) * 16) = v3[i];
        } else if (i * 512 + tid < NV3) {  // cos / sin unit (table t, row rw, unit cu % 8), padded rows
            const int cu = i * 512 + tid - NB3 * 256 * 2 / 16;
            *(lds_f16x8*)(lds + kCS + (cu / 8) * kCSP + (cu % 8) * 16) = v3[i];
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    FR_SEG(0);

    // B-operand fragments of step s from an [MT][1 KiB] tile: rows 32 mb + r, unit 2 s + hh
    struct BF {
        f16x8 v[MB];
    };
    auto bfrag = [&](int base, int s) {
        BF f;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int row = 32 * mb + r;
            f.v[mb] = *(lds_f16x8*)(lds + base + row * 1024 + (((2 * s + hh) ^ (row & 15)) << 4));
        }
        return f;
    };
    // ---- phase 1: hᵀ (the wave's 64 channels x MT rows) = W1 · Aᵀ; each step's B fragments are read
    // one step ahead (their LDS latency under the previous MFMAs) ----
    f32x16 acc[2][MB] = {};
    BF af = bfrag(kA, 0);
#pragma unroll
    for (int j = 0; j < NS1; ++j) {
        const f16x8 wa = take(2 * j), wb = take(2 * j + 1);
        if constexpr (AH) {
            if (j + 1 == NS1 / 2) {  // the heads half into LDS before step NS1 / 2's fragments are read
                put_half(ac, 32);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_s_barrier();
            }
        }
        const BF an = j + 1 < NS1 ? bfrag(kA, j + 1) : af;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            acc[0][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, af.v[mb], acc[0][mb], 0, 0, 0);
            acc[1][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wb, af.v[mb], acc[1][mb], 0, 0, 0);
        }
        af = an;
        __builtin_amdgcn_sched_barrier(0);
    }

    FR_SEG(1);
    // ---- LayerNorm over each row's 512 h values: the wave's 64 are in lanes r and r + 32 ----
    // lane (r, hh): acc[b][mb][4 g + t] = hidden channel 64 w + 32 b + 8 g + 4 hh + t of row 32 mb + r.
    // h = fp16(acc + b1) in one rounding (v_fma_mixlo_f16; the two calls' lin_val rounds through fp32
    // first: the same value but for a rare double rounding), then the wave's sum of the row's 64
    // values and their squares about the wave's own mean (a second pass over the packed registers),
    // merged over the waves by ln_merge: one exchange through LDS (vector issue bounds this phase:
    // ~20 VALU per value, two waves a SIMD)
    float* const red = (float*)(void*)(smem + kRed);  // [pass][row][wave]
    float sm[MB], sq[MB];  // the wave's sum of a row, its squares about sm / 64
    unsigned hp[2][MB][8];  // h as packed fp16 pairs: block b, rows mb, (g, pair u) at 2 g + u
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        float s1 = 0.f;
        f32x2 s2 = {0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const u32x2 b4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + (64 * wave + 32 * b + 8 * g + 4 * hh) * 2);
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    hp[b][mb][2 * g + u] = mixh2(acc[b][mb][4 * g + 2 * u], acc[b][mb][4 * g + 2 * u + 1], b4[u]);
                    row_sum2(hp[b][mb][2 * g + u], s1);
                }
            }
        sm[mb] = s1 + __shfl_xor(s1, 32, 64);
        const float c = sm[mb] * (1.f / 64);
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int i = 0; i < 8; ++i) row_dev2(hp[b][mb][i], c, s2);
        const float sl = s2[0] + s2[1];
        sq[mb] = sl + __shfl_xor(sl, 32, 64);
    }
    if (hh == 0) {
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            red[(32 * mb + r) * 8 + wave] = sm[mb];
            red[MT * 8 + (32 * mb + r) * 8 + wave] = sq[mb];
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    auto row_stats = [&](int row) {  // from the 8 waves' partials of a row, in a fixed order
        auto part = [&](int i) { return *(__attribute__((address_space(3))) f32x4*)(lds + kRed + (i + row * 8) * 4); };
        return ln_merge(part(0), part(4), part(MT * 8), part(MT * 8 + 4), eps);
    };
    // GELU(LN(h)) -> fp16 into the h tile (unit 8 w + 4 b + g of the row, half hh)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int row = 32 * mb + r;
        const RowStats st = row_stats(row);
        const float rstd = st.rstd, nmr = -st.mean * rstd;
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = 64 * wave + 32 * b + 8 * g + 4 * hh;
                const u32x2 g4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + K * 2 + n * 2);
                const u32x2 be4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + 2 * K * 2 + n * 2);
                f16x4 o;
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const unsigned h2 = hp[b][mb][2 * g + u];
                    const float x0 = mixn<0>(h2, rstd, nmr), x1 = mixn<1>(h2, rstd, nmr);
                    const f32x2 gl = gelu_as2(f32x2{mixf<0>(x0, g4[u], be4[u]), mixf<1>(x1, g4[u], be4[u])});
                    o[2 * u] = (f16)gl[0];
                    o[2 * u + 1] = (f16)gl[1];
                }
                *(__attribute__((address_space(3))) f16x4*)(lds + kH + row * 1024 + (((8 * wave + 4 * b + g) ^ (row & 15)) << 4) + 8 * hh) = o;
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // h complete
    FR_SEG(2);

    // ---- phase 2: outᵀ (the wave's 32 channels x MT rows) = W2 · hᵀ ----
    f32x16 o2[MB] = {};
    BF hf = bfrag(kH, 0);
#pragma unroll
    for (int j = NS1; j < NS; ++j) {
        const f16x8 wa = take(NS1 + j);
        const BF hn = j + 1 < NS ? bfrag(kH, j + 1 - NS1) : hf;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) o2[mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa, hf.v[mb], o2[mb], 0, 0, 0);
        hf = hn;
        __builtin_amdgcn_sched_barrier(0);
    }
    FR_SEG(3);
    if constexpr (MB > 1) {  // (the staging rows lie over h: every wave done reading it)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
    }

    // ---- out = fp16(fp16(acc + b2) + x): the wave's MT x 32 block staged row-major in its own LDS
    // rows (80-B pitch), then two lanes a row, 32 B each, with x from the A tile ----
    lds_char* const stg = lds + kStg + wave * (MT * kSP);
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int c = 32 * wave + 8 * g + 4 * hh;
            const f16x4 b4 = *(__attribute__((address_space(3))) f16x4*)(lds + kPar + 3 * K * 2 + c * 2);
            const f16x4 v = f16x4{lin_val(o2[mb][4 * g], b4[0]), lin_val(o2[mb][4 * g + 1], b4[1]),
                                  lin_val(o2[mb][4 * g + 2], b4[2]), lin_val(o2[mb][4 * g + 3], b4[3])};
            *(__attribute__((address_space(3))) f16x4*)(stg + (32 * mb + r) * kSP + (8 * g + 4 * hh) * 2) = v;
        }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the wave's own rows: LDS ops of a wave in order)
    f16x8 xo[MB][2];  // x' = this lane's out values (phase 3's input)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int rr = 32 * mb + (lane >> 1), half = lane & 1;
#pragma unroll
        for (int e2 = 0; e2 < 2; ++e2) {
            f16x8 v = *(lds_f16x8*)(stg + rr * kSP + half * 32 + e2 * 16);
            const f16x8 xr = *(lds_f16x8*)(lds + kA + rr * 1024 + (((4 * wave + 2 * half + e2) ^ (rr & 15)) << 4));
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = res_add(v[e], xr[e]);
            xo[mb][e2] = v;
            if (m0 + rr < p.m) *reinterpret_cast<f16x8*>(p.out[0] + (size_t)(m0 + rr) * NO + 32 * wave + 16 * half + 8 * e2) = v;
        }
    }
#ifdef LG_FR_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FR_SEG(4);
#endif
    if constexpr (E3 != E3_NONE) {
        // ---- phase 3: the next projection of x' (K = 256): x' rows into the A region ([MT][512 B],
        // units XOR (row & 15)) once every wave has read its residual there ----
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            const int rr = 32 * mb + (lane >> 1), half = lane & 1;
#pragma unroll
            for (int e2 = 0; e2 < 2; ++e2)
                *(lds_f16x8*)(lds + kA + rr * 512 + (((4 * wave + 2 * half + e2) ^ (rr & 15)) << 4)) = xo[mb][e2];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        auto xfrag = [&](int s) {
            BF f;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const int row = 32 * mb + r;
                f.v[mb] = *(lds_f16x8*)(lds + kA + row * 512 + (((2 * s + hh) ^ (row & 15)) << 4));
            }
            return f;
        };
        // the wave's NB3 blocks of 32 output channels, c = 32 (NB3 w + b) + ...
        f32x16 a3[NB3][MB] = {};
        BF xf = xfrag(0);
#pragma unroll
        for (int j = 0; j < NS3; ++j) {
            f16x8 w3[NB3];
#pragma unroll
            for (int b = 0; b < NB3; ++b) w3[b] = take(96 + NB3 * j + b);
            const BF xn = j + 1 < NS3 ? xfrag(j + 1) : xf;
#pragma unroll
            for (int b = 0; b < NB3; ++b)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) a3[b][mb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w3[b], xf.v[mb], a3[b][mb], 0, 0, 0);
            xf = xn;
            __builtin_amdgcn_sched_barrier(0);
        }
        // epilogue: fp16(acc + b3) (+ rotary for q, k) as the standalone projections compute it, the
        // wave's rows x 32 channels of a block staged (its own rows of the staging region), then two
        // lanes a row, 32 B each, to the row's head-major (or row-major) destination
#pragma unroll
        for (int b = 0; b < NB3; ++b) {
            const int cb = 32 * (NB3 * wave + b);  // the block's first channel (one head of one part)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int c = cb + 8 * g + 4 * hh;
                    const f16x4 b4 = *(__attribute__((address_space(3))) f16x4*)(lds + kB3 + c * 2);
                    f16x4 v = f16x4{lin_val(a3[b][mb][4 * g], b4[0]), lin_val(a3[b][mb][4 * g + 1], b4[1]),
                                    lin_val(a3[b][mb][4 * g + 2], b4[2]), lin_val(a3[b][mb][4 * g + 3], b4[3])};
                    if constexpr (E3 == E3_QKV) {
                        if (cb < 2 * NO) {  // q, k: rotary pairs (d, d + 1) from this row's tables
                            const int rw = 32 * mb + r;  // (tile row; rows past m hold row m - 1's tables)
                            const f16x4 cc = *(__attribute__((address_space(3))) f16x4*)(lds + kCS + rw * kCSP + (c % kD) * 2);
                            const f16x4 ss = *(__attribute__((address_space(3))) f16x4*)(lds + kCS + (MT + rw) * kCSP + (c % kD) * 2);
#pragma unroll
                            for (int t = 0; t < 4; t += 2) rot_pair(v, t, cc[t], ss[t], cc[t + 1], ss[t + 1]);
                        }
                    }
                    *(__attribute__((address_space(3))) f16x4*)(stg + (32 * mb + r) * kSP + (8 * g + 4 * hh) * 2) = v;
                }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                const int rr = 32 * mb + (lane >> 1), half = lane & 1;
                const f16x8 v0 = *(lds_f16x8*)(stg + rr * kSP + half * 32);
                const f16x8 v1 = *(lds_f16x8*)(stg + rr * kSP + half * 32 + 16);
                const int row = m0 + rr;
                if (row < p.m) {
                    f16* dst;
                    if constexpr (E3 == E3_PLAIN) {
                        dst = cb < q3.n_store ? q3.out[0] + (size_t)row * q3.n_store + cb + 16 * half : nullptr;
                    } else {
                        const int part = cb / NO, h = (cb % NO) / kD;
                        const LinRow lr = lin_row(p, row, h);
                        dst = q3.out[E3 == E3_QKV ? (lr.first ? 0 : 3) + part : (lr.first ? 0 : 1) + 2 * part] + lr.off +
                              cb % kD + 16 * half;
                    }
                    if (dst) {
                        *reinterpret_cast<f16x8*>(dst) = v0;
                        *reinterpret_cast<f16x8*>(dst + 8) = v1;
                    }
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the next block rewrites the staging rows)
        }
    }
#ifdef LG_FR_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FR_SEG(5);  // (phase 3 and its epilogue; segment 4 then ends at phase 2's stores)
    if (lane == 0 && blockIdx.x < 256) {
        unsigned long long* d = g_fr_stamps + ((size_t)blockIdx.x * 8 + wave) * 8;
        for (int k = 0; k < 5; ++k) d[k] = fr_[k];
        d[5] = fr_last_ - fr_entry_;
        d[6] = fr_entry_;
        d[7] = fr_[5];
    }
#endif
}

// ---- the 16-row form (round 6): the same FFN (+ phase 3) with v_mfma_f32_16x16x32_f16 on 16-row tiles ----
// At a few thousand rows the 32-row kernel above fills a quarter of the chip (2,048 rows: 64
// workgroups) and its time is the per-CU weight stream (each workgroup reads all of W1, W2, W3) plus
// the LayerNorm+GELU vector work of its 32 x 512 values (~8 k cycles, profiles/r06/ffn_rows_stamps*):
// 16-row tiles double the workgroups and halve the vector work per CU at the same stream. Operands
// (cdna_hip_programming.md §3): lane l holds A[i = l & 15][k = 8 (l >> 4) + e] (weights: channel i of a
// 16-channel block), B[k][j = l & 15] (activation row j), D[4 (l >> 4) + t][l & 15] — channels
// 4 q + t (q = l >> 4) of row l & 15. The weight stream is lg_ffn_pack's second layout: wave w's
// pieces are phase 1 W1[64 w + 16 b + i][32 s + 8 q ..] (piece 4 s + b), phase 2 W2[32 w + 16 b + i]
// (64 + 2 s + b), phase 3 W3[16 (2 NB3 w + b) + i][32 s + 8 q ..] (96 + 2 NB3 s + b): the same channel
// sets per wave as the 32-row layout, so the rounding and order of every sum are unchanged but for
// the k order inside an MFMA.
template <int D, int E3, int NB3, int SP = 1>
__global__ __launch_bounds__(512, 1) void ffn_rows16_kernel(LinArgs p, const f16* __restrict__ gamma,
                                                            const f16* __restrict__ beta, float eps,
                                                            const f16* __restrict__ wp, const f16* __restrict__ b2,
                                                            Proj3 q3) {
    constexpr int MT = 16, K = 512, NO = kFfnOut;
    constexpr int NP = 96 + NB3 * 16;              // the wave's stream: pieces of 1 KiB
    constexpr int R = 2 * D;                       // pieces in flight (a register ring)
    constexpr int NB = 2 * NB3;                    // phase 3: 16-channel blocks per wave
    constexpr int NBP = NB / (SP > 1 ? SP : 1);    // ... of them this workgroup's (SP parts of a tile)
    constexpr int NPS = 96 + 8 * NBP;              // the pieces this workgroup's waves consume
    constexpr int U3 = 32 * NB3;                   // phase 3: 16-B units per output row
    constexpr int kA = 0;                          // A tile [16][1 KiB]: x units 0..31, heads 32..63
    constexpr int kH = kA + MT * 1024;             // h tile [16][1 KiB]
    constexpr int kX = kH + MT * 1024;             // out / x' tile [16][512 B]
    constexpr int kS3 = kX + MT * 512;             // phase 3's staging [16][U3 units]
    constexpr int kPar = kS3 + MT * U3 * 16;       // b1, gamma, beta [512], b2 [256] fp16
    constexpr int kRed = kPar + (3 * K + NO) * 2;  // row partials [2][16][8 waves] fp32
    constexpr int kB3 = kRed + 2 * MT * 8 * 4;     // b3 [n3] fp16
    constexpr int kCS = kB3 + NB3 * 256 * 2;       // E3_QKV: cos / sin rows [2][16] fp16, 144-B pitch
    constexpr int kCSP = 144;                      // (36 banks a row apart: a column read by 16 rows is
                                                   // conflict-free, where a 128-B pitch was 8-way)
    constexpr int kEnd = kCS + (E3 == E3_QKV ? 2 * MT * kCSP : 0);
    static_assert(D >= 1 && D <= 16 && (E3 == E3_NONE) == (NB3 == 0) && kEnd <= 160 * 1024, "shape");
    static_assert(SP == 1 || (E3 != E3_NONE && NB % SP == 0), "parts");
    __shared__ __attribute__((aligned(16))) char smem[kEnd];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    // SP > 1: SP workgroups per 16-row tile, each running phases 1 and 2 whole and 1/SP of phase 3
    // (at a few hundred tiles the chip has the CUs; the projection's weight stream and epilogue halve)
    const int part = SP > 1 ? (int)blockIdx.x % SP : 0;
    const int m0 = (SP > 1 ? (int)blockIdx.x / SP : (int)blockIdx.x) * MT;
#ifdef LG_FR_STAMPS
    unsigned long long fr_[7] = {0, 0, 0, 0, 0, 0, 0}, fr_last_, fr_entry_;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(fr_entry_)::"memory");
    fr_last_ = fr_entry_;
#endif
    auto tile_unit = [](int row, int u) { return row * 1024 + ((u ^ (row & 15)) << 4); };  // A / h tiles
    auto x_unit = [](int row, int u) { return row * 512 + ((u ^ (row & 15)) << 4); };      // x' tile

    // ---- A tile (two 16-B units a thread: row f / 64, unit f % 64), the vectors; rows past m repeat
    // row m - 1 ----
    // (row tid / 32: its x unit tid % 32 first, then its heads unit; phase 1's first half runs on x)
    f16x8 ax, ac;
    {
        const int grow = min(m0 + (tid >> 5), p.m - 1);
        ax = *reinterpret_cast<const f16x8*>(p.a + (size_t)grow * (K / 2) + (tid & 31) * 8);
        const LinRow lr = lin_row(p, grow, (tid & 31) >> 3);
        ac = *reinterpret_cast<const f16x8*>((lr.first ? p.ctx0 : p.ctx1) + lr.off + (tid & 7) * 8);
    }
    f16x8 pv = {};
    if (tid < 224) {
        const f16* const pvs = tid < 64 ? p.bias : tid < 128 ? gamma : tid < 192 ? beta : b2;
        pv = *reinterpret_cast<const f16x8*>(pvs + (tid & 63) * 8);
    }
    constexpr int NVB = NB3 * 256 * 2 / 16;                         // b3 units
    constexpr int NV3 = NVB + (E3 == E3_QKV ? 2 * MT * 8 : 0);      // + cos / sin units
    static_assert(NV3 <= 512, "phase 3 vectors");
    f16x8 v3 = {};
    if (tid < NV3) {
        if (tid < NVB) {
            v3 = *reinterpret_cast<const f16x8*>(q3.b3 + tid * 8);
        } else {  // table t, row rw (clamped), unit cu % 8
            const int cu = tid - NVB, t = cu / (MT * 8), rw = min(m0 + (cu % (MT * 8)) / 8, p.m - 1);
            v3 = *reinterpret_cast<const f16x8*>((t ? q3.sinv : q3.cosv) + (size_t)rw * kD + (cu % 8) * 8);
        }
    }
    asm volatile("s_barrier" ::: "memory");  // (every wave's A loads ahead of the weight stream)

    const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(wp), (short)0, 8 * NP * 1024, 0x00020000);
    const unsigned wo = (unsigned)(wave * NP * 1024 + lane * 16);
    // stream position i -> packed piece (phase 3: this part's NBP blocks of each k32 step)
    const int p3off = __builtin_amdgcn_readfirstlane(part * NBP * 1024);
    auto piece = [&](int i) {
        const int so = i < 96 ? i * 1024 : (96 + NB * ((i - 96) / NBP) + (i - 96) % NBP) * 1024 + p3off;
        return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wo, so, 0));
    };
    f16x8 w_[R];
#pragma unroll
    for (int i = 0; i < R; ++i) {
        w_[i] = piece(i);
        if (i & 1) __builtin_amdgcn_sched_barrier(0);
    }
    auto take = [&](int i) {
        const f16x8 w = w_[i % R];
        if (i + R < NPS) w_[i % R] = piece(i + R);
        return w;
    };
    *(lds_f16x8*)(lds + kA + tile_unit(tid >> 5, tid & 31)) = ax;
    if (tid < 224) *(lds_f16x8*)(lds + kPar + tid * 16) = pv;
    if (tid < NVB) {
        *(lds_f16x8*)(lds + kB3 + tid * 16) = v3;
    } else if (tid < NV3) {  // cos / sin unit (table t, row rw, unit cu % 8) into its padded row
        const int cu = tid - NVB;
        *(lds_f16x8*)(lds + kCS + (cu / 8) * kCSP + (cu % 8) * 16) = v3;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    FR_SEG(0);

    // ---- phase 1: hᵀ (the wave's 64 channels x 16 rows) = W1 · Aᵀ, k32 steps, B read a step ahead ----
    f32x4 acc[4] = {};
    f16x8 bf = *(lds_f16x8*)(lds + kA + tile_unit(r, q));
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        f16x8 w4[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) w4[b] = take(4 * s + b);
        if (s + 1 == 8) {  // the heads half into LDS before step 8's fragments are read
            *(lds_f16x8*)(lds + kA + tile_unit(tid >> 5, 32 + (tid & 31))) = ac;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        const f16x8 bn = s + 1 < 16 ? *(lds_f16x8*)(lds + kA + tile_unit(r, 4 * (s + 1) + q)) : bf;
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w4[b], bf, acc[b], 0, 0, 0);
        bf = bn;
        __builtin_amdgcn_sched_barrier(0);
    }
    FR_SEG(1);

    // ---- LayerNorm: lane (r, q) holds channels 64 w + 16 b + 4 q + t of row r; h = fp16(acc + b1) in
    // one rounding, the row's sum over the 4 q lanes, the squares about the wave's own mean over them, then
    // the 8 waves via LDS (ln_merge) ----
    float* const red = (float*)(void*)(smem + kRed);
    float s1 = 0.f;
    f32x2 sd = {0.f, 0.f};
    unsigned hp[4][2];  // h as packed fp16 pairs: block b, channels 4 q + 2 u, + 1
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const u32x2 b4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + (64 * wave + 16 * b + 4 * q) * 2);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            hp[b][u] = mixh2(acc[b][2 * u], acc[b][2 * u + 1], b4[u]);
            row_sum2(hp[b][u], s1);
        }
    }
    // over the row's 4 lanes (l, l ^ 16, l ^ 32, l ^ 48) by lane-group swaps (VALU, no LDS trip)
    auto xsum = [](float x) {
        const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
        const float y = __uint_as_float(a[0]) + __uint_as_float(a[1]);
        const auto c = __builtin_amdgcn_permlane32_swap(__float_as_uint(y), __float_as_uint(y), false, false);
        return __uint_as_float(c[0]) + __uint_as_float(c[1]);
    };
    s1 = xsum(s1);
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int u = 0; u < 2; ++u) row_dev2(hp[b][u], s1 * (1.f / 64), sd);
    const float s2 = xsum(sd[0] + sd[1]);
    if (q == 0) {
        red[r * 8 + wave] = s1;
        red[MT * 8 + r * 8 + wave] = s2;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    auto row_stats = [&](int row) {  // from the 8 waves' partials of a row, in a fixed order
        auto part = [&](int i) { return *(__attribute__((address_space(3))) f32x4*)(lds + kRed + (i + row * 8) * 4); };
        return ln_merge(part(0), part(4), part(MT * 8), part(MT * 8 + 4), eps);
    };
    {
        const RowStats st = row_stats(r);
        const float rstd = st.rstd, nmr = -st.mean * rstd;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n = 64 * wave + 16 * b + 4 * q;
            const u32x2 g4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + K * 2 + n * 2);
            const u32x2 be4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + 2 * K * 2 + n * 2);
            f16x4 o;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float x0 = mixn<0>(hp[b][u], rstd, nmr), x1 = mixn<1>(hp[b][u], rstd, nmr);
                const f32x2 gl = gelu_as2(f32x2{mixf<0>(x0, g4[u], be4[u]), mixf<1>(x1, g4[u], be4[u])});
                o[2 * u] = (f16)gl[0];
                o[2 * u + 1] = (f16)gl[1];
            }
            *(__attribute__((address_space(3))) f16x4*)(lds + kH + tile_unit(r, n >> 3) + 8 * (q & 1)) = o;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // h complete
    FR_SEG(2);

    // ---- phase 2: outᵀ (the wave's 32 channels x 16 rows) = W2 · hᵀ ----
    f32x4 o2[2] = {};
    f16x8 hf = *(lds_f16x8*)(lds + kH + tile_unit(r, q));
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const f16x8 wa = take(64 + 2 * s), wb = take(64 + 2 * s + 1);
        const f16x8 hn = s + 1 < 16 ? *(lds_f16x8*)(lds + kH + tile_unit(r, 4 * (s + 1) + q)) : hf;
        o2[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa, hf, o2[0], 0, 0, 0);
        o2[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wb, hf, o2[1], 0, 0, 0);
        hf = hn;
        __builtin_amdgcn_sched_barrier(0);
    }
    FR_SEG(3);
    // ---- out = fp16(fp16(acc + b2) + x): fp16(acc + b2) into the x' tile, then one 16-B unit a thread
    // (row tid / 32, unit tid % 32) with x from the A tile, to memory and back into the x' tile ----
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int c = 32 * wave + 16 * b + 4 * q;
        const f16x4 b4 = *(__attribute__((address_space(3))) f16x4*)(lds + kPar + 3 * K * 2 + c * 2);
        const f16x4 v = f16x4{lin_val(o2[b][0], b4[0]), lin_val(o2[b][1], b4[1]), lin_val(o2[b][2], b4[2]),
                              lin_val(o2[b][3], b4[3])};
        *(__attribute__((address_space(3))) f16x4*)(lds + kX + x_unit(r, c >> 3) + 8 * (q & 1)) = v;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    {
        const int row = tid >> 5, u = tid & 31;
        f16x8 v = *(lds_f16x8*)(lds + kX + x_unit(row, u));
        const f16x8 xr = *(lds_f16x8*)(lds + kA + tile_unit(row, u));
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = res_add(v[e], xr[e]);
        if (part == 0 && m0 + row < p.m) *reinterpret_cast<f16x8*>(p.out[0] + (size_t)(m0 + row) * NO + 8 * u) = v;
        if constexpr (E3 != E3_NONE) *(lds_f16x8*)(lds + kX + x_unit(row, u)) = v;
    }
#ifdef LG_FR_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FR_SEG(4);
#endif
    if constexpr (E3 != E3_NONE) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();  // x' complete
        // ---- phase 3: the wave's NB blocks of 16 output channels, c = 16 (NB w + b) + 4 q + t ----
        // (E3_QKV: this lane's rotary factors read here, their LDS latency under the MFMAs; the v
        // blocks read a harmless column too)
        f16x4 rc[E3 == E3_QKV ? NBP : 1], rs[E3 == E3_QKV ? NBP : 1];
        if constexpr (E3 == E3_QKV) {
#pragma unroll
            for (int b = 0; b < NBP; ++b) {
                const int d = (16 * (NB * wave + part * NBP + b) + 4 * q) % kD;
                rc[b] = *(__attribute__((address_space(3))) f16x4*)(lds + kCS + r * kCSP + d * 2);
                rs[b] = *(__attribute__((address_space(3))) f16x4*)(lds + kCS + (MT + r) * kCSP + d * 2);
            }
        }
        f32x4 a3[NBP] = {};
        f16x8 xf = *(lds_f16x8*)(lds + kX + x_unit(r, q));
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            f16x8 w3[NBP];
#pragma unroll
            for (int b = 0; b < NBP; ++b) w3[b] = take(96 + NBP * s + b);
            const f16x8 xn = s + 1 < 8 ? *(lds_f16x8*)(lds + kX + x_unit(r, 4 * (s + 1) + q)) : xf;
#pragma unroll
            for (int b = 0; b < NBP; ++b) a3[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w3[b], xf, a3[b], 0, 0, 0);
            xf = xn;
            __builtin_amdgcn_sched_barrier(0);
        }
        FR_SEG(5);  // (the projection's MFMA loop; its epilogue: segment 6)
        // epilogue: fp16(acc + b3) (+ rotary for q, k) into the staging rows, then one 16-B unit a thread
        // (row, unit u: channels 8 u .. + 7, one head of one part) to its destination
#pragma unroll
        for (int b = 0; b < NBP; ++b) {
            const int c = 16 * (NB * wave + part * NBP + b) + 4 * q;
            const f16x4 b4 = *(__attribute__((address_space(3))) f16x4*)(lds + kB3 + c * 2);
            f16x4 v = f16x4{lin_val(a3[b][0], b4[0]), lin_val(a3[b][1], b4[1]), lin_val(a3[b][2], b4[2]),
                            lin_val(a3[b][3], b4[3])};
            // (a declaration, not the bare test in the `if`: without one here the compiler swaps the operands
            // of phase 2's v_pk_add_f16 in the SPLIT2 forms — same results, but not the recorded instructions)
            constexpr bool ROT = E3 == E3_QKV;
            if constexpr (ROT) {
                if (c < 2 * NO) {  // q, k: rotary pairs (d, d + 1) from this row's tables
#pragma unroll
                    for (int t = 0; t < 4; t += 2) rot_pair(v, t, rc[b][t], rs[b][t], rc[b][t + 1], rs[b][t + 1]);
                }
            }
            *(__attribute__((address_space(3))) f16x4*)(lds + kS3 + r * (U3 * 16) + (((c >> 3) ^ r) << 4) + 8 * (q & 1)) = v;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        {  // thread -> row tid / 32, units t + 32 j (t = tid % 32): part j, head t / 8 — one row
           // lookup per thread, and 32 consecutive threads write a row's 512 B of one part
            const int row = tid >> 5, t = tid & 31, grow = m0 + row;
            if (grow < p.m) {
                if constexpr (E3 == E3_PLAIN) {
#pragma unroll
                    for (int j = 0; j < U3 / 32; ++j) {
                        const int u = t + 32 * j;
                        if (SP > 1 && ((8 * u) % (16 * NB)) / (16 * NBP) != part) continue;  // (another part's)
                        if (8 * u < q3.n_store)
                            *reinterpret_cast<f16x8*>(q3.out[0] + (size_t)grow * q3.n_store + 8 * u) =
                                *(lds_f16x8*)(lds + kS3 + row * (U3 * 16) + ((u ^ row) << 4));
                    }
                } else {
                    const LinRow lr = lin_row(p, grow, t >> 3);
                    const size_t off = lr.off + (8 * t) % kD;
#pragma unroll
                    for (int j = 0; j < U3 / 32; ++j) {
                        const int u = t + 32 * j;
                        if (SP > 1 && ((8 * u) % (16 * NB)) / (16 * NBP) != part) continue;  // (another part's)
                        const f16x8 v = *(lds_f16x8*)(lds + kS3 + row * (U3 * 16) + ((u ^ row) << 4));
                        f16* const dst = q3.out[E3 == E3_QKV ? (lr.first ? 0 : 3) + j : (lr.first ? 0 : 1) + 2 * j] + off;
                        *reinterpret_cast<f16x8*>(dst) = v;
                    }
                }
            }
        }
    }
#ifdef LG_FR_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    FR_SEG(6);
    if (lane == 0 && blockIdx.x < 256) {  // (slot 6: the phase-3 epilogue, not the entry time)
        unsigned long long* d = g_fr_stamps + ((size_t)blockIdx.x * 8 + wave) * 8;
        for (int i = 0; i < 5; ++i) d[i] = fr_[i];
        d[5] = fr_last_ - fr_entry_;
        d[6] = fr_[6];
        d[7] = fr_[5];
    }
#endif
}

// lg_ffn_pack: one thread per 16-B fragment of the packed stream (layout: include/lightglue_glue.h);
// wave w's stream: 64 W1 pieces, 32 W2 pieces, then NB3 x 16 W3 pieces (NB3 = n3 / 256). form 0: the
// 32-row kernel's fragments (32 channels x k16 a piece), form 1: the 16-row kernel's (16 x k32)
__global__ __launch_bounds__(256) void ffn_pack_kernel(const f16* __restrict__ w1, const f16* __restrict__ w2,
                                                       const f16* __restrict__ w3, int nb3, int form, f16* packed) {
    const int np = 96 + 16 * nb3;                  // pieces per wave
    const int f = blockIdx.x * 256 + threadIdx.x;  // fragment: wave w, piece i, lane l
    if (f >= 8 * np * 64) return;
    const int w = f / (np * 64), i = (f % (np * 64)) / 64, l = f % 64;
    const f16* src;
    if (form == 0) {
        const int r = l % 32, hh = l / 32;
        if (i < 64) src = w1 + (size_t)(64 * w + 32 * (i & 1) + r) * 512 + 16 * (i >> 1) + 8 * hh;
        else if (i < 96) src = w2 + (size_t)(32 * w + r) * 512 + 16 * (i - 64) + 8 * hh;
        else {
            const int j = (i - 96) / nb3, b = (i - 96) % nb3;
            src = w3 + (size_t)(32 * (nb3 * w + b) + r) * 256 + 16 * j + 8 * hh;
        }
    } else {
        const int r = l % 16, q = l / 16;
        if (i < 64) src = w1 + (size_t)(64 * w + 16 * (i & 3) + r) * 512 + 32 * (i >> 2) + 8 * q;
        else if (i < 96) src = w2 + (size_t)(32 * w + 16 * ((i - 64) & 1) + r) * 512 + 32 * ((i - 64) >> 1) + 8 * q;
        else {
            const int j = (i - 96) / (2 * nb3), b = (i - 96) % (2 * nb3);
            src = w3 + (size_t)(16 * (2 * nb3 * w + b) + r) * 256 + 32 * j + 8 * q;
        }
    }
    *reinterpret_cast<f16x8*>(packed + (size_t)f * 8) = *reinterpret_cast<const f16x8*>(src);
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

namespace {

// lg_linear_cat_ffn's form (lg_linear_set_ffn_fused): 1 (default) the one-launch ffn_rows_kernel when
// the caller passes the packed weight stream, 0 always its two calls (lg_linear_cat_ln_gelu, then
// lg_linear with the residual). Measured against the
// two calls (profiles/r06/ffn_rows_*_ab.jsonl, op alone, us): P = 1 (2,048 rows) 15.5 -> 12.1, P = 4
// 31.0 -> 14.4, P = 8 32.4 -> 23.4, P = 16 53.6 -> 46.5, P = 32 94.0 -> 87.3; forwards P = 1 / 8 / 16 / 32
// 0.546 / 1.471 / 2.336 / 4.295 -> 0.501 / 1.204 / 2.145 / 4.029 ms. (Round 5's 128-row one-launch form,
// ffn_kernel, GELU output in LDS and W2 fragments per 128-row tile from L2: 56 vs 52.7 us at P = 16, not
// adopted, and removed in round 6: profiles/r05/ffn_one_launch_ab.jsonl.)
std::atomic<int> g_ffn_fused{1};
}  // namespace
extern "C" int32_t lg_linear_set_ffn_fused(int32_t mode) { return g_ffn_fused.exchange(mode >= 0 && mode <= 3 ? mode : 1); }

namespace {
// ffn_rows_kernel's weight-stream depth: k16 steps of fragments in flight per wave (measured flat over
// 6..20 at 2,048 and 8,192 rows: the stream is throughput-bound, profiles/r06/ffn_rows_rowmajor_w_ab.jsonl)
constexpr int kFrDepth = 12;
// The one-launch FFN by size (lg_linear_set_ffn_fused 1): 16-row workgroups up to one round of them
// (ffn_rows16_kernel: the most workgroups and the least vector work per CU, for latency), 32-row up
// to one round, 64-row beyond (half the weight bytes per row); 2 / 3: the 32/64-row / 16-row kernel at
// every size (A/B). wp: lg_ffn_pack's two layouts, the 32-row kernel's first. (Tried and dropped: the
// 32-row kernel two workgroups per CU (128 VGPRs, an 8-piece ring, staging over h), for one workgroup's
// A-tile latency under the other's stream — 46.0 -> 47.1 us at 32,768 rows, 23.0 -> 24.1 at 16,384,
// equal bits; profiles/r06/ffn_rows_occ2_ab.jsonl.)
// The 16-row kernel's projection split over two workgroups per tile (ffn_rows16_kernel<…, SP = 2>):
// up to 64 tiles (LG_FFN_SPLIT=0: never, =2: while 2 x tiles fill at most one round). Measured
// (profiles/r06/ffn_phase3_split_ab.jsonl, single-pair forwards, ms): n = 512 (64 tiles) 0.368 -> 0.353;
// n = 1024 (128 tiles) 0.427-0.431 -> 0.434 split, kept whole. Three / four parts (one or two blocks
// per wave, an A/B build) : n = 512 0.351-0.354 -> 0.355-0.359, n = 256 0.334 -> 0.325.
int ffn_split_parts(int tiles) {
    static const int env = [] {
        const char* e = std::getenv("LG_FFN_SPLIT");
        return e ? std::atoi(e) : -1;
    }();
    if (env == 0) return 1;
    return (env == 2 ? 2 * tiles <= kTileGrid : tiles <= 64) ? 2 : 1;
}
template <int E3, int NB3>
void launch_ffn_rows(const LinArgs& p, const f16* gamma, const f16* beta, float eps, const f16* wp, const f16* b2,
                     const Proj3& q3, hipStream_t stream) {
    const int mode = g_ffn_fused.load();
    if (mode == 3 || (mode != 2 && p.m <= 16 * kTileGrid)) {
        const f16* wp16 = wp + (size_t)8 * (96 + 16 * NB3) * 1024 / 2;
        const int tiles = (p.m + 15) / 16;
        if constexpr (E3 != E3_NONE) {
            const int sp = ffn_split_parts(tiles);
            if (sp == 2) {
                hipLaunchKernelGGL((ffn_rows16_kernel<kFrDepth, E3, NB3, 2>), dim3(2 * tiles), dim3(512), 0, stream, p,
                                   gamma, beta, eps, wp16, b2, q3);
                return;
            }
        }
        hipLaunchKernelGGL((ffn_rows16_kernel<kFrDepth, E3, NB3>), dim3(tiles), dim3(512), 0, stream, p, gamma, beta, eps,
                           wp16, b2, q3);
    } else if (p.m <= 32 * kTileGrid)
        hipLaunchKernelGGL((ffn_rows_kernel<1, kFrDepth, E3, NB3>), dim3((p.m + 31) / 32), dim3(512), 0, stream, p, gamma, beta,
                           eps, wp, b2, q3);
    else
        hipLaunchKernelGGL((ffn_rows_kernel<2, kFrDepth, E3, NB3>), dim3((p.m + 63) / 64), dim3(512), 0, stream, p, gamma, beta,
                           eps, wp, b2, q3);
}
}  // namespace

extern "C" {

int32_t lg_linear_cat_ffn(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                          int32_t pairs, const void* w1, const void* b1, const void* gamma, const void* beta, float eps,
                          const void* w2, const void* b2, const void* w_packed, void* h, void* out, hipStream_t stream) {
    const int d = heads * kD, k = 2 * d, m = pairs * (n0 + n1);
    if (heads <= 0 || n0 < 0 || n1 < 0 || pairs < 0 || !shape_ok(m, k, k) || !x || !w1 || !b1 || !gamma || !beta || !w2 ||
        !b2 || !h || !out || out == x || !aligned16(x) || (n0 && !aligned16(ctx0)) || (n1 && !aligned16(ctx1)) ||
        !aligned16(w1) || !aligned16(w2) || !aligned8(b1) || !aligned8(b2) || !aligned16(h) || !aligned8(out) || !(eps >= 0.f) ||
        (w_packed && !aligned16(w_packed)))
        return bad("lg_linear_cat_ffn");
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;
    const bool one = g_ffn_fused.load() != 0 && w_packed && k == kLnN && d == kFfnOut && aligned16(b1) && aligned16(gamma) &&
                     aligned16(beta) && aligned16(b2) && aligned16(out);
    if (!one) {  // h in the caller's buffer, then the output projection with the residual
        const int32_t st = lg_linear_cat_ln_gelu(x, ctx0, ctx1, heads, n0, n1, pairs, w1, b1, gamma, beta, eps, h, stream);
        if (st != MHA_HD64_STATUS_SUCCESS) return st;
        return lg_linear(h, w2, b2, x, m, d, k, out, stream);
    }
    const LinArgs p = gather_args(x, ctx0, ctx1, w1, b1, out, heads, n0, n1, pairs, k, k);
    launch_ffn_rows<E3_NONE, 0>(p, (const f16*)gamma, (const f16*)beta, eps, (const f16*)w_packed, (const f16*)b2, Proj3{}, stream);
    return launched("lg_linear_cat_ffn");
}

size_t lg_ffn_packed_bytes(int32_t heads, int32_t n3) {  // both layouts, the 32-row kernel's first
    return heads == 4 && (n3 == 0 || n3 == 512 || n3 == 768) ? (size_t)2 * 8 * (96 + n3 / 16) * 1024 : 0;
}

int32_t lg_ffn_pack(const void* w1, const void* w2, const void* w3, int32_t n3, int32_t heads, void* packed, hipStream_t stream) {
    if (!lg_ffn_packed_bytes(heads, n3) || !w1 || !w2 || !packed || !aligned16(w1) || !aligned16(w2) || !aligned16(packed) ||
        (n3 && (!w3 || !aligned16(w3))))
        return bad("lg_ffn_pack");
    const int nb3 = n3 / 256, frags = 8 * (96 + 16 * nb3) * 64;
    for (int form = 0; form < 2; ++form)
        hipLaunchKernelGGL(ffn_pack_kernel, dim3((frags + 255) / 256), dim3(256), 0, stream, (const f16*)w1, (const f16*)w2,
                           (const f16*)w3, nb3, form, (f16*)packed + (size_t)form * frags * 8);
    return launched("lg_ffn_pack");
}

int32_t lg_linear_cat_ffn_proj(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                               int32_t pairs, const void* b1, const void* gamma, const void* beta, float eps, const void* b2,
                               const void* w_packed, int32_t kind, const void* b3, const void* cosv, const void* sinv,
                               int32_t n_store, void* const* outs3, void* out, hipStream_t stream) {
    const int d = heads * kD, k = 2 * d, m = pairs * (n0 + n1);
    const int nouts = kind == LG_PROJ_SPLIT2 ? 4 : kind == LG_PROJ_QKV ? 6 : kind == LG_PROJ_PLAIN ? 1 : 0;
    bool ok = heads == 4 && n0 >= 0 && n1 >= 0 && pairs >= 0 && nouts && x && b1 && gamma && beta && b2 && w_packed && b3 && outs3 &&
              out && out != x && aligned16(x) && (!n0 || aligned16(ctx0)) && (!n1 || aligned16(ctx1)) && aligned16(b1) &&
              aligned16(gamma) && aligned16(beta) && aligned16(b2) && aligned16(w_packed) && aligned8(b3) && aligned16(out) &&
              eps >= 0.f && (kind != LG_PROJ_QKV || (cosv && sinv && aligned8(cosv) && aligned8(sinv))) &&
              (kind != LG_PROJ_PLAIN || (n_store > 0 && n_store <= 512 && n_store % 8 == 0)) &&
              (kind == LG_PROJ_PLAIN || (long long)m * heads * kD < (1LL << 31));
    for (int i = 0; ok && i < nouts; ++i) ok = outs3[i] && aligned16(outs3[i]);
    if (!ok) return bad("lg_linear_cat_ffn_proj");
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;
    const LinArgs p = gather_args(x, ctx0, ctx1, nullptr, b1, out, heads, n0, n1, pairs, k, k);  // (W1 in w_packed)
    Proj3 q3{};
    q3.b3 = (const f16*)b3, q3.cosv = (const f16*)cosv, q3.sinv = (const f16*)sinv, q3.n_store = n_store;
    for (int i = 0; i < nouts; ++i) q3.out[i] = (f16*)outs3[i];
    const f16 *g = (const f16*)gamma, *be = (const f16*)beta, *wp = (const f16*)w_packed, *bb2 = (const f16*)b2;
    if (kind == LG_PROJ_SPLIT2) launch_ffn_rows<E3_SPLIT2, 2>(p, g, be, eps, wp, bb2, q3, stream);
    else if (kind == LG_PROJ_QKV) launch_ffn_rows<E3_QKV, 3>(p, g, be, eps, wp, bb2, q3, stream);
    else launch_ffn_rows<E3_PLAIN, 2>(p, g, be, eps, wp, bb2, q3, stream);
    return launched("lg_linear_cat_ffn_proj");
}

#ifdef LG_LN_STAMPS
int32_t lg_diag_ln_stamps(void* host_dst) {  // (diagnostic build only: not in the header)
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_ln_stamps), sizeof(g_ln_stamps)) == hipSuccess ? 0 : 1;
}
#endif
#ifdef LG_FR_STAMPS
int32_t lg_diag_fr_stamps(void* host_dst) {  // (diagnostic build only: not in the header)
    return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_fr_stamps), sizeof(g_fr_stamps)) == hipSuccess ? 0 : 1;
}
#endif

}  // extern "C"
