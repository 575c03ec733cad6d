// lightglue_linear.hip — the matcher's projections as gfx950 MFMA kernels with their neighbours
// fused in (include/lightglue_glue.h, lg_linear_*). fp16 in/out, fp32 accumulation.
//
// The LightGlue layer (lightglue_pytorch_no_plugin/lightglue.py:88-194) is a chain of small
// GEMMs (M = both images' keypoints, K = 256 or 512, N = 256..768) separated by layout and
// elementwise steps; at matcher sizes every one of them is a few-microsecond, latency-bound
// launch. These kernels do the GEMM and the step either side in one launch:
//   * lg_linear           : out = A·Wᵀ + b (+ residual)                  (FFN layers, residual add)
//   * lg_linear_cat       : A = [x | merge_heads(ctx0, ctx1)] gathered on load (FFN input of
//                           both blocks, lightglue.py:104/181; the message projection is folded
//                           into W by the caller)
//   * lg_linear_qkv_rotary: SelfBlock Wqkv + rotary + per-image head-major q/k/v (:111-134; W's
//                           rows pre-permuted to [q|k|v][head][dim] order by the caller)
//   * lg_linear_split2    : CrossBlock to_qk | to_v as one GEMM + per-image head split (:158-166)
//
// Workgroup: 64 rows (m) x 64 output channels (n), 4 waves as 2 x 2 tiles of 32 x 32. The
// product is computed transposed, Cᵀ = W·Aᵀ on v_mfma_f32_32x32x16_f16 (A-operand = W rows,
// B-operand = activation rows, both K-contiguous), so a lane ends up owning one activation row
// and 4 runs of 4 consecutive output channels: epilogue stores are 8-B row segments and a rotary
// pair (2d, 2d+1) sits in one lane. Both 64 x K tiles reach LDS by LDS-DMA in 128-column
// chunks ([chunk][row][256 B], 16-B units XOR-swizzled by row & 15 on the source address:
// conflict-free ds_read_b128 of 16 rows at one k); the MFMAs of chunk c start once c has
// landed (counted vmcnt + barrier) while the later chunks stream in.
//
// The FFN's own kernels are in lightglue_ffn_ln.hip (lg_linear_cat_ln_gelu) and lightglue_ffn.hip (lg_linear_cat_ffn*), the
// assignment and match heads in lightglue_assign.hip; what they share with this file (LinArgs, the
// A-gather, the output arithmetic, the tile forms' DMA sources) is in lightglue_device.h.
#include <stdlib.h>

#include <atomic>
#include <cstdlib>

#include "lightglue_device.h"

namespace {

constexpr int kBM = 64, kBN = 64, kKC = 128;
// tile rows, tile channels, K columns per LDS chunk
constexpr int kChunkBytes = 64 * kKC * 2;     // one [64 rows][128 k] fp16 chunk = 16 KiB

enum { EPI_BIAS = 0, EPI_QKV_ROTARY = 1, EPI_SPLIT2 = 2 };

template <int EPI, bool GATHER, int KC>
__global__ __launch_bounds__(256) void linear_kernel(LinArgs p) {
    static_assert(KC == 2 || KC == 4, "k = 256 or 512");
    __shared__ __attribute__((aligned(16))) char smem[2 * KC * kChunkBytes];  // W, A tiles (64 / 128 KiB)
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave & 1, wn = wave >> 1;  // this wave's 32 x 32 tile of the 64 x 64
    const int r = lane & 31, hh = lane >> 5;
    // XCD-aware order: consecutive j (one XCD) = consecutive m tiles of one n tile (W tile in L2)
    int j;
    {
        const int T = p.total, L = blockIdx.x, q8 = T >> 3, r8 = T & 7, xcd = L & 7;
        j = xcd * q8 + min(xcd, r8) + (L >> 3);
    }
    const int mt = j % p.mtiles, nt = j / p.mtiles;
    const int m0 = mt * kBM, n0 = nt * kBN;
    const unsigned wbase = 0, abase = KC * kChunkBytes;
    const int wrow = wn * 32 + r, arow = wm * 32 + r;
    const int m = min(m0 + arow, p.m - 1);  // this lane's output row (clamped; stores are guarded)

    // Epilogue operands first (plain loads, older than every DMA below, so the counted waits
    // of the main loop stay exact): bias, residual / rotary tables of the lane's 4 x 4 channels.
    f16x4 bias4[4], aux0[4], aux1[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 32 + 8 * g + 4 * hh;
        bias4[g] = *reinterpret_cast<const f16x4*>(p.bias + n);
        if constexpr (EPI == EPI_BIAS) {
            if (p.res) aux0[g] = *reinterpret_cast<const f16x4*>(p.res + (size_t)m * p.n + n);
        } else if constexpr (EPI == EPI_QKV_ROTARY) {
            aux0[g] = *reinterpret_cast<const f16x4*>(p.cosv + (size_t)m * kD + n % kD);
            aux1[g] = *reinterpret_cast<const f16x4*>(p.sinv + (size_t)m * kD + n % kD);
        }
    }

    __builtin_amdgcn_sched_barrier(0);  // (they stay ahead of the DMAs)

    // ---- loads: per chunk c, W rows n0.. and A rows m0.. ; one DMA = 4 rows x 256 B ----
    // lane -> (row 4i + lane/16, LDS unit lane%16 <- global unit (lane%16) ^ (row & 15))
    // Wave w issues DMA instructions i = w, w+4, w+8, w+12 of each 16-instruction chunk tile.
#pragma unroll
    for (int c = 0; c < KC; ++c) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int i = wave + 4 * s;
            const int row = 4 * i + (lane >> 4), pu = lane & 15;
            const int gc = c * (kKC / 8) + (pu ^ (row & 15));
            const int wr = min(n0 + row, p.n - 1);
            __builtin_amdgcn_global_load_lds((const void*)(p.w + (size_t)wr * p.k + gc * 8),
                                             (__attribute__((address_space(3))) void*)(smem + wbase + c * kChunkBytes + i * 1024),
                                             16, 0, 0);
            const int ar = min(m0 + row, p.m - 1);
            __builtin_amdgcn_global_load_lds((const void*)a_src<GATHER>(p, ar, gc),
                                             (__attribute__((address_space(3))) void*)(smem + abase + c * kChunkBytes + i * 1024),
                                             16, 0, 0);
        }
    }

    f32x16 acc = {};
#pragma unroll
    for (int c = 0; c < KC; ++c) {
        // chunk c landed for this wave's DMAs (8 per chunk, in issue order), then for everyone's
        switch (KC - 1 - c) {
            case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
            case 1: asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); break;
            case 2: asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); break;
            default: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
        }
        __builtin_amdgcn_s_barrier();
        const unsigned wc = wbase + c * kChunkBytes + wrow * 256, ac = abase + c * kChunkBytes + arow * 256;
        // all 8 k-steps' fragments of the chunk first (one LDS latency per chunk, not per step)
        f16x8 wf[kKC / 16], af[kKC / 16];
#pragma unroll
        for (int s = 0; s < kKC / 16; ++s) {
            const int u = 2 * s + hh;  // 16-B unit of the k-step
            wf[s] = *(lds_f16x8*)(lds + wc + ((u ^ (wrow & 15)) << 4));
            af[s] = *(lds_f16x8*)(lds + ac + ((u ^ (arow & 15)) << 4));
        }
#pragma unroll
        for (int s = 0; s < kKC / 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[s], af[s], acc, 0, 0, 0);
    }

    // ---- epilogue: lane = activation row m; acc[4g + t] = channel n0 + wn*32 + 8g + 4hh + t ----
    if (m0 + arow >= p.m) return;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn * 32 + 8 * g + 4 * hh;  // 4 consecutive channels n..n+3
        f16x4 v;
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = lin_val(acc[4 * g + t], bias4[g][t]);
        if constexpr (EPI == EPI_BIAS) {
            if (p.res) {
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = res_add(v[t], aux0[g][t]);
            }
            *reinterpret_cast<f16x4*>(p.out[0] + (size_t)m * p.n + n) = v;
        } else {
            const int hd = p.heads * kD;
            const int part = n / hd, h = (n % hd) / kD, d = n % kD;
            const LinRow lr = lin_row(p, m, h);
            const bool first = lr.first;
            if constexpr (EPI == EPI_QKV_ROTARY) {
                if (part < 2) {  // q, k: (x0, x1) -> (x0 c - x1 s, x1 c + x0 s), pairs (d, d+1)
                    const f16x4 cc = aux0[g], ss = aux1[g];
#pragma unroll
                    for (int t = 0; t < 4; t += 2) rot_pair(v, t, cc[t], ss[t], cc[t + 1], ss[t + 1]);
                }
            }
            f16* dst = p.out[(first ? 0 : (EPI == EPI_QKV_ROTARY ? 3 : 1)) + (EPI == EPI_QKV_ROTARY ? part : 2 * part)];
            *reinterpret_cast<f16x4*>(dst + lr.off + d) = v;
        }
    }
}

// ---- the tile form, for launches with many rows (several image pairs per forward) ----
// Persistent tiles of MT rows x NT channels (128 x 128 on 4 waves is the one instantiated), NWV waves as WM (m) x
// WN (n) tiles of 64 rows x NT / WN channels (2 x NB MFMA blocks of 32 x 32), K in BK-deep steps through
// an NST-stage LDS-DMA ring (16-B units XOR-swizzled on the source address: conflict-free
// ds_read_b128), NST - 1 steps in flight; the ring runs on across tile seams, so the next tile's
// first steps load during the current tile's last ones. XCD-aware: the workgroups of XCD x walk the
// contiguous tile range [jb, je) (tile j = m tile j / ntiles, n tile j % ntiles: the n tiles of one
// m tile run side by side on one XCD and read its A rows through one L2).
//
// Epilogue (round 5): the MFMA layout puts one activation row on each lane, so stores straight from
// the accumulators write 32 rows x 16-32 B per wave instruction; measured (ablations of the round-4
// forms, profiles/r05/linear_ablations.jsonl) those stores cost more than the GEMM: lg_linear_qkv_rotary
// 53.6 us with them, 15.9 without. Here each wave rounds (acc + bias) to fp16 into its own 4 KiB
// region of the ring stage its tile's last K step has just freed (one barrier per tile), 32 rows x
// 64 channels a round, reads it back row-major and writes whole 128-B row segments: 8 rows x 128 B
// per wave instruction, the residual / rotary tables loaded in the same coalesced layout (prefetched
// at the tile's last K step). The stores stay in flight into the next tile: its first NST - 1 waits
// count them (every lane stores; rows past m are computed on the clamped last A row and write that
// row's own bytes again, so the count is exact).
// RES (EPI_BIAS): p.res is added (a compile-time form: its prefetch holds registers).
template <int EPI, bool GATHER, bool RES, int KS, int MT, int NT, int BK, int NST, int NWV = 8>
__global__ __launch_bounds__(64 * NWV, NWV == 4 ? 2 : 1) void linear_tile_kernel(LinArgs p) {
    constexpr int WM = MT / 64, WN = NWV / WM, WTN = NT / WN, NB = WTN / 32, NP = WTN / 64;
    constexpr int SB = (MT + NT) * BK * 2;                               // one ring stage
    constexpr int NWP = NT * BK * 2 / (NWV * 1024), NAP = MT * BK * 2 / (NWV * 1024);  // 1-KiB DMA pieces per wave, step
    constexpr int D = NWP + NAP;
    constexpr int SPW = 2 * NP * 4;                                      // output stores per wave and tile
    // epilogue operands loaded per wave and tile (at its first K step): bias, residual / cos + sin rows
    constexpr int PF = NB * 4 + (RES ? 2 * NP * 4 : 0) + (EPI == EPI_QKV_ROTARY ? 16 : 0);
    static_assert(SB >= NWV * 4096, "a staging region per wave inside one ring stage");
    static_assert(KS >= NST - 1 && NB % 2 == 0 && (NST - 2) * D + SPW + PF <= 63, "shape");
    static_assert(NB == 2 || (EPI != EPI_QKV_ROTARY && !RES), "64 x 128 wave tiles: no room for the prefetched tables");
    __shared__ __attribute__((aligned(16))) char smem[NST * SB];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int r = lane & 31, hh = lane >> 5;
    const int T = p.total, xcd = blockIdx.x & 7, loc = blockIdx.x >> 3;
    const int q8 = T >> 3, r8 = T & 7;
    const int jb = xcd * q8 + min(xcd, r8), je = jb + q8 + (xcd < r8 ? 1 : 0);
    const int G = ((int)gridDim.x - xcd + 7) >> 3;
    const int ntiles = p.n / NT;
    const int j0 = jb + loc;
    if (j0 >= je) return;
    const int ntile_w = (je - j0 + G - 1) / G;
    const int nsteps = ntile_w * KS;

    auto src_of = [&](int t) {
        const int jt = j0 + G * t, mt = jt / ntiles;
        return tile_src<GATHER, BK, NWP, NAP, NWV>(p, mt * MT, (jt - mt * ntiles) * NT, wave, lane);
    };
    TileSrc<NWP, NAP> cur = src_of(0), nxt = cur;
#pragma unroll
    for (int i = 0; i < NST - 1; ++i)
        tile_issue<GATHER, BK, KS, NT, NWV>(cur, i, smem + i * SB, wave);

    // fragment rows of this lane: W rows wn * WTN + 32 b + r, A rows wm * 64 + 32 b + r
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
    // coalesced phase: lane -> (row 8 i + lane / 8 of a 32-row round, 16-B chunk lane % 8 of 64 channels)
    const int cr = lane >> 3, cc = lane & 7;
    int st = 0;
    for (int t = 0; t < ntile_w; ++t) {
        const int jt = j0 + G * t;
        const int mt = jt / ntiles, m0 = mt * MT, n0 = (jt - mt * ntiles) * NT;
        const int nw0 = n0 + wn * WTN;  // this wave's first channel
        const bool more = t + 1 < ntile_w;
        if (more) nxt = src_of(t + 1);
        f32x16 acc[NB][2] = {};
        f16x4 bias4[NB][4];
        f16x8 aux[2][NP][4];  // residual rows (EPI_BIAS) / cos rows (QKV) of the coalesced phase
        f16x8 aux2[2][4];     // sin rows (QKV)
        int st_last = 0;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int gs = t * KS + ks;
            // step gs landed (this wave's pieces: younger ones = the later steps' DMAs in flight,
            // plus the previous tile's output stores while they are younger), then everyone's; past
            // this barrier every wave is done with step gs - 1's stage
            // Younger than step gs's pieces: the later steps' DMA in flight; the previous tile's output
            // stores while issued after gs's DMA (ks < NST - 1); this tile's epilogue operands,
            // loaded at ks = 0 after that step's wait (1 <= ks <= NST - 2). (The workgroup's last
            // NST - 2 steps have fewer later steps in flight: drain all.)
            const bool pfk = ks >= 1 && ks <= NST - 2;  // (folded after unrolling)
            if (gs + NST - 2 > nsteps - 1) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            else if (ks < NST - 1 && t > 0) {
                if (pfk) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D + SPW + PF) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D + SPW) : "memory");
            } else {
                if (pfk) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D + PF) : "memory");
                else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"((NST - 2) * D) : "memory");
            }
            __builtin_amdgcn_s_barrier();
            if (ks == 0) {
                // the epilogue's operands, a whole tile ahead of their use (rows clamped to m - 1, as
                // the A rows are; the rotary tables for the v part too: a fixed count for the waits)
#pragma unroll
                for (int b = 0; b < NB; ++b)
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        bias4[b][g] = *reinterpret_cast<const f16x4*>(p.bias + nw0 + 32 * b + 8 * g + 4 * hh);
#pragma unroll
                for (int mb = 0; mb < 2; ++mb)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = min(m0 + wm * 64 + 32 * mb + 8 * i + cr, p.m - 1);
                        if constexpr (EPI == EPI_BIAS && RES) {
#pragma unroll
                            for (int np = 0; np < NP; ++np)
                                aux[mb][np][i] = *reinterpret_cast<const f16x8*>(p.res + (size_t)row * p.n + nw0 + 64 * np + 8 * cc);
                        } else if constexpr (EPI == EPI_QKV_ROTARY) {
                            aux[mb][0][i] = *reinterpret_cast<const f16x8*>(p.cosv + (size_t)row * kD + 8 * cc);
                            aux2[mb][i] = *reinterpret_cast<const f16x8*>(p.sinv + (size_t)row * kD + 8 * cc);
                        }
                    }
            }
            {
                char* const fb = smem + (st == 0 ? NST - 1 : st - 1) * SB;
                if (ks + NST - 1 < KS) tile_issue<GATHER, BK, KS, NT, NWV>(cur, ks + NST - 1, fb, wave);
                else if (more) tile_issue<GATHER, BK, KS, NT, NWV>(nxt, ks + NST - 1 - KS, fb, wave);
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

        // ---- epilogue: the operands loaded at ks = 0 landed (younger: this tile's KS DMA issues when
        // another tile follows; a count capped at 63 only waits for more); every wave's fragment reads
        // of the last stage done (barrier) ----
        if (more) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(KS * D < 63 ? KS * D : 63) : "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        lds_char* const stg = lds + st_last * SB + wave * 4096;
        const int hd = p.heads * kD;
        // Head-major outputs (QKV / SPLIT2): rows rb + 32 mb + 8 i of the coalesced phase, split
        // into (pair, row of the pair) with one division per tile and a step per row (pairs of
        // more than 56 rows here, tile_form: one wrap at most); rows past m take row m - 1's
        // place, as their A rows did.
        const int ntot = p.n0 + p.n1;
        const int rb = m0 + wm * 64 + cr;
        const int pr0 = rb / ntot, l0 = rb - pr0 * ntot;
        const int prl = (p.m - 1) / ntot, ll = p.m - 1 - prl * ntot;
        auto split_row = [&](int o, int& pr, int& l) {
            pr = pr0, l = l0 + o;
            if (l >= ntot) l -= ntot, ++pr;
            if (rb + o > p.m - 1) pr = prl, l = ll;
        };
        // (the common tile: no lane's rows rb .. rb + 56 cross an image, pair or m boundary, so row
        // o's offset is row 0's + 64 o in the same image: wave-uniform)
        const bool img0 = l0 < p.n0;
        const bool span = (img0 ? l0 + 56 < p.n0 : l0 + 56 < ntot) && rb + 56 <= p.m - 1;
        const bool easy = __builtin_amdgcn_ballot_w64(!span) == 0;
#pragma unroll
        for (int mb = 0; mb < 2; ++mb)
#pragma unroll
            for (int np = 0; np < NP; ++np) {
                // (acc + bias) -> fp16, rows r of the round, 16-B chunk (4 nbl + g) ^ (r & 7), half hh
#pragma unroll
                for (int nbl = 0; nbl < 2; ++nbl)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const f32x16& a = acc[2 * np + nbl][mb];
                        const f16x4 b4 = bias4[2 * np + nbl][g];
                        const f16x4 v = f16x4{lin_val(a[4 * g], b4[0]), lin_val(a[4 * g + 1], b4[1]),
                                              lin_val(a[4 * g + 2], b4[2]), lin_val(a[4 * g + 3], b4[3])};
                        *(__attribute__((address_space(3))) f16x4*)(stg + r * 128 + (((4 * nbl + g) ^ (r & 7)) << 4) + 8 * hh) = v;
                    }
                f16x8 o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int rl = 8 * i + cr;
                    o[i] = *(lds_f16x8*)(stg + rl * 128 + ((cc ^ (rl & 7)) << 4));
                }
                if constexpr (EPI == EPI_BIAS) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = min(m0 + wm * 64 + 32 * mb + 8 * i + cr, p.m - 1);
                        const int n = nw0 + 64 * np + 8 * cc;  // 8 consecutive channels n..n+7
                        f16x8 v = o[i];
                        if constexpr (RES) {
#pragma unroll
                            for (int e = 0; e < 8; ++e) v[e] = res_add(v[e], aux[mb][np][i][e]);
                        }
                        st_out(p.out[0] + (size_t)row * p.n + n, v);
                    }
                } else {
                    // the wave's 64 channels lie in one head of one part (nw0 + 64 np and hd are
                    // multiples of 64): part, head and the two images' destinations are wave-uniform
                    const int nu = __builtin_amdgcn_readfirstlane(nw0 + 64 * np);
                    const int part = nu / hd, h = (nu - part * hd) / kD;
                    f16* d0;
                    f16* d1;
                    if constexpr (EPI == EPI_QKV_ROTARY) {
                        d0 = part == 0 ? p.out[0] : part == 1 ? p.out[1] : p.out[2];
                        d1 = part == 0 ? p.out[3] : part == 1 ? p.out[4] : p.out[5];
                    } else {
                        d0 = part == 0 ? p.out[0] : p.out[2];
                        d1 = part == 0 ? p.out[1] : p.out[3];
                    }
                    // element offsets in [pairs, heads, ni, 64]: pair stride, head h's first row + d
                    const unsigned ps0 = (unsigned)(p.heads * p.n0 * kD), ps1 = (unsigned)(p.heads * p.n1 * kD);
                    const unsigned hb0 = (unsigned)(h * p.n0 * kD + 8 * cc), hb1 = (unsigned)(h * p.n1 * kD + 8 * cc);
                    f16* const db = img0 ? d0 : d1;
                    const unsigned ob = img0 ? (unsigned)pr0 * ps0 + (unsigned)l0 * kD + hb0
                                             : (unsigned)pr0 * ps1 + (unsigned)(l0 - p.n0) * kD + hb1;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f16x8 v = o[i];
                        if constexpr (EPI == EPI_QKV_ROTARY) {
                            if (part < 2) {
#pragma unroll
                                for (int e = 0; e < 8; e += 2)
                                    rot_pair(v, e, aux[mb][0][i][e], aux2[mb][i][e], aux[mb][0][i][e + 1], aux2[mb][i][e + 1]);
                            }
                        }
                        if (easy) {
                            st_out(db + ob + (unsigned)((32 * mb + 8 * i) * kD), v);
                            continue;
                        }
                        int pr, l;
                        split_row(32 * mb + 8 * i, pr, l);
                        const bool first = l < p.n0;
                        const unsigned off = first ? (unsigned)pr * ps0 + (unsigned)l * kD + hb0
                                                   : (unsigned)pr * ps1 + (unsigned)(l - p.n0) * kD + hb1;
                        st_out((first ? d0 : d1) + off, v);
                    }
                }
            }
        cur = nxt;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// The tile form (tile_form below): lg_linear_set_wide or LG_LINEAR_WIDE, 0 = the 64 x 64 form, 1..5 = the
// 128 x 128 form (where n allows), for tests and timing; -1 (the default) chooses by size.
std::atomic<int> g_wide{-2};
}  // namespace
int lightglue::wide_mode() {
    int v = g_wide.load();
    if (v == -2) {
        const char* e = std::getenv("LG_LINEAR_WIDE");
        long m = -1;  // unset or unparsable: chosen by size
        if (e && *e) {
            char* end = nullptr;
            const long x = std::strtol(e, &end, 10);
            if (end != e) m = x < -1 ? -1 : (x > 5 ? 5 : x);
        }
        int expect = -2;
        g_wide.compare_exchange_strong(expect, (int)m);
        v = g_wide.load();
    }
    return v;
}
extern "C" int32_t lg_linear_set_wide(int32_t mode) {
    lightglue::wide_mode();
    return g_wide.exchange(mode < 0 ? -1 : (mode > 5 ? 5 : mode));
}

namespace {
// The tile form (linear_tile_kernel): 128 x 128 on 4 waves, two workgroups per CU, 64-deep K steps through 2
// stages. (Tried and dropped: 256 x 128 and 256 x 256 on 8 waves, 128 x 256, and 32-deep K steps through 4
// stages; profiles/r05/tile_form4_ab.jsonl, form_fwd_ab.jsonl: qkv 18.5 / 26.6 / 48.8 -> 15.9 / 25.1 / 46.5 us
// at P = 8 / 16 / 32 against 256 x 128, which leaves half the CUs idle at P = 8.)
// True: the 128 x 128 form; false: the 64 x 64 form (linear_kernel).
bool tile_form(const LinArgs& p, int epi) {
    bool al = aligned16(p.bias);
    const int nout = epi == EPI_BIAS ? 1 : epi == EPI_QKV_ROTARY ? 6 : 4;
    for (int i = 0; i < nout; ++i) al = al && aligned16(p.out[i]);
    if (p.res) al = al && aligned16(p.res);
    if (epi == EPI_QKV_ROTARY) al = al && aligned16(p.cosv) && aligned16(p.sinv);
    if (!al) return false;
    // (the head-major epilogue's element offsets are 32-bit: every per-image output below 2^32 elements;
    // (and it steps through the rows of a tile with one wrap at most: pairs of more than 56 rows)
    if (epi != EPI_BIAS && ((long long)p.m * p.heads * kD >= (1LL << 32) || p.n0 + p.n1 <= 56)) return false;
    // forced (wide_mode 0, or 1..5), else by size: from 128 of its tiles and 8,192 rows on
    // (profiles/r05/tile_form4_ab.jsonl: at 128 tiles it wins linear+res at P = 4 and lg_linear_cat at
    // P = 2, loses split2 at P = 2 by 1 us; from 192 tiles on it wins or ties every op the matcher calls.
    // Whole forwards, form_fwd_ab_final.jsonl: P = 2 (4,096 rows) 2 % faster with the 64 x 64 form)
    const int w = lightglue::wide_mode();
    const bool wide = w >= 0 ? w >= 1 : (p.m >= 8192 && (long)((p.m + 127) / 128) * (p.n / 128) >= 128);
    return wide && p.n % 128 == 0;
}

template <int EPI, bool GATHER, bool RES, int MT, int NT, int BK, int NST, int NWV>
void launch_tile_r(LinArgs& p, hipStream_t stream) {
    p.mtiles = (p.m + MT - 1) / MT;
    p.total = p.mtiles * (p.n / NT);
    constexpr int cap = kTileGrid * 8 / NWV;  // persistent: one round (4 waves: two workgroups per CU)
    const int grid = p.total < cap ? p.total : cap;
    if (p.k == 256)
        hipLaunchKernelGGL((linear_tile_kernel<EPI, GATHER, RES, 256 / BK, MT, NT, BK, NST, NWV>), dim3(grid), dim3(64 * NWV), 0, stream, p);
    else
        hipLaunchKernelGGL((linear_tile_kernel<EPI, GATHER, RES, 512 / BK, MT, NT, BK, NST, NWV>), dim3(grid), dim3(64 * NWV), 0, stream, p);
}
template <int EPI, bool GATHER, int MT, int NT, int BK, int NST, int NWV>
void launch_tile(LinArgs& p, hipStream_t stream) {
    if constexpr (EPI == EPI_BIAS && !GATHER) {
        if (p.res) return launch_tile_r<EPI, GATHER, true, MT, NT, BK, NST, NWV>(p, stream);
    }
    launch_tile_r<EPI, GATHER, false, MT, NT, BK, NST, NWV>(p, stream);
}

template <int EPI, bool GATHER>
int32_t launch(LinArgs& p, hipStream_t stream, const char* what) {
    if (tile_form(p, EPI)) {
        launch_tile<EPI, GATHER, 128, 128, 64, 2, 4>(p, stream);
    } else {
        p.mtiles = (p.m + kBM - 1) / kBM;
        p.total = p.mtiles * (p.n / kBN);
        if (p.k == 256)
            hipLaunchKernelGGL((linear_kernel<EPI, GATHER, 2>), dim3(p.total), dim3(256), 0, stream, p);
        else
            hipLaunchKernelGGL((linear_kernel<EPI, GATHER, 4>), dim3(p.total), dim3(256), 0, stream, p);
    }
    return launched(what);
}

}  // namespace

extern "C" {

int32_t lg_linear(const void* a, const void* w, const void* bias, const void* res, int32_t m, int32_t n, int32_t k,
                  void* out, hipStream_t stream) {
    if (!shape_ok(m, n, k) || !a || !w || !bias || !out || !aligned16(a) || !aligned16(w) || !aligned8(bias) ||
        !aligned8(out) || (res && !aligned8(res)))
        return bad("lg_linear");
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;
    LinArgs p{};
    p.a = (const f16*)a, p.w = (const f16*)w, p.bias = (const f16*)bias, p.res = (const f16*)res;
    p.out[0] = (f16*)out;
    p.m = m, p.n = n, p.k = k, p.n0 = m, p.n1 = 0;
    return launch<EPI_BIAS, false>(p, stream, "lg_linear");
}

int32_t lg_linear_cat(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                      int32_t pairs, const void* w, const void* bias, int32_t n, void* out, hipStream_t stream) {
    const int k = 2 * heads * kD, m = pairs * (n0 + n1);
    if (heads <= 0 || n0 < 0 || n1 < 0 || pairs < 0 || !shape_ok(m, n, k) || !x || !w || !bias || !out || !aligned16(x) ||
        (n0 && !aligned16(ctx0)) || (n1 && !aligned16(ctx1)) || !aligned16(w) || !aligned8(bias) || !aligned8(out))
        return bad("lg_linear_cat");
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;
    LinArgs p = gather_args(x, ctx0, ctx1, w, bias, out, heads, n0, n1, pairs, n, k);
    return launch<EPI_BIAS, true>(p, stream, "lg_linear_cat");
}

int32_t lg_linear_qkv_rotary(const void* x, const void* w_perm, const void* b_perm, const void* cosv,
                             const void* sinv, int32_t heads, int32_t n0, int32_t n1, int32_t pairs, int32_t k,
                             void* q0, void* k0, void* v0, void* q1, void* k1, void* v1, hipStream_t stream) {
    const int m = pairs * (n0 + n1), n = 3 * heads * kD;
    if (heads <= 0 || n0 < 0 || n1 < 0 || pairs < 0 || !shape_ok(m, n, k) || !x || !w_perm || !b_perm || !cosv || !sinv ||
        !aligned16(x) || !aligned16(w_perm) || !aligned8(b_perm) || !aligned8(cosv) || !aligned8(sinv))
        return bad("lg_linear_qkv_rotary");
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;
    LinArgs p{};
    p.a = (const f16*)x, p.w = (const f16*)w_perm, p.bias = (const f16*)b_perm;
    p.cosv = (const f16*)cosv, p.sinv = (const f16*)sinv;
    f16* outs[6] = {(f16*)q0, (f16*)k0, (f16*)v0, (f16*)q1, (f16*)k1, (f16*)v1};
    for (int i = 0; i < 6; ++i) p.out[i] = outs[i];
    p.m = m, p.n = n, p.k = k, p.heads = heads, p.n0 = n0, p.n1 = n1;
    return launch<EPI_QKV_ROTARY, false>(p, stream, "lg_linear_qkv_rotary");
}

int32_t lg_linear_split2(const void* x, const void* w, const void* bias, int32_t heads, int32_t n0, int32_t n1,
                         int32_t pairs, int32_t k, void* a0, void* a1, void* b0, void* b1, hipStream_t stream) {
    const int m = pairs * (n0 + n1), n = 2 * heads * kD;
    if (heads <= 0 || n0 < 0 || n1 < 0 || pairs < 0 || !shape_ok(m, n, k) || !x || !w || !bias || !aligned16(x) ||
        !aligned16(w) || !aligned8(bias))
        return bad("lg_linear_split2");
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;
    LinArgs p{};
    p.a = (const f16*)x, p.w = (const f16*)w, p.bias = (const f16*)bias;
    f16* outs[4] = {(f16*)a0, (f16*)a1, (f16*)b0, (f16*)b1};
    for (int i = 0; i < 4; ++i) p.out[i] = outs[i];
    p.m = m, p.n = n, p.k = k, p.heads = heads, p.n0 = n0, p.n1 = n1;
    return launch<EPI_SPLIT2, false>(p, stream, "lg_linear_split2");
}

int32_t lg_glue_abi_version(void) { return LG_GLUE_ABI_VERSION; }

}  // extern "C"
