// lightglue_ffn.hip — the matcher's whole FFN in one launch, as gfx950 MFMA kernels that own whole rows
// (include/lightglue_glue.h: lg_linear_cat_ffn, lg_ffn_pack, lg_linear_cat_ffn_proj). fp16 in/out, fp32
// accumulation. LinArgs, the A-gather and the output arithmetic are shared with the projections
// (lightglue_linear.hip) through lightglue_device.h, the steps that both rows kernels take are in
// lightglue_ffn_device.h; the two-call fallback calls lg_linear_cat_ln_gelu (lightglue_ffn_ln.hip) and
// lg_linear through the C ABI.
#ifdef LG_FR_STAMPS
#define FFN_STAMPS
#endif
#include <atomic>

#include "lightglue_ffn_device.h"

namespace {

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
// (Tried and dropped: a workgroup barrier every few 1-KiB pieces of the weight stream, so that no wave
// runs ahead of the others' streams; P = 1 / 4 / 16 FFN 10.0 / 14.6 / 46.0 us without, 10.1 / 15.1 / 46.4
// with one every 8: the CU's stream is bandwidth-bound either way, profiles/r06/ffn_wave_sync_ab.jsonl.)
// Diagnostic build (-DLG_FR_STAMPS, tools/fr_stamps.py; never shipped): per wave of the first 256
// workgroups, the stamps of lightglue_ffn_device.h by chained segment (0 entry -> A in LDS, 1 phase 1,
// 2 LayerNorm + GELU, 3 phase 2, 4 epilogue; slot 6: the entry time, 7: phase 3 and its epilogue), read
// back by lg_diag_fr_stamps.
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
    using L = FfnLds<MT, E3, NB3, (MB == 1 ? kStg + 8 * MT * kSP : 2 * kH)>;  // the vectors, partials, phase 3's
    constexpr int kPar = L::kPar, kRed = L::kRed, kB3 = L::kB3, kCS = L::kCS, kCSP = L::kCSP;
    constexpr int NS1 = K / 16, NS = 2 * NS1;      // k16 steps per GEMM; the stream: phase 1, then 2
    constexpr int NS3 = NO / 16;                   // phase 3: k16 steps over x' (K = 256)
    constexpr int NP = 96 + NB3 * NS3;             // the wave's stream: pieces of 1 KiB
    constexpr int R = 2 * D;                       // pieces in flight (a register ring)
    static_assert(D >= 1 && D <= NS1 && (MB == 1 || MB == 2) && (E3 == E3_NONE) == (NB3 == 0), "shape");
    static_assert(MB == 1 || 8 * MT * kSP <= kH, "staging over h");
    __shared__ __attribute__((aligned(16))) char smem[L::kEnd];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int m0 = blockIdx.x * MT;
    FFN_STAMPS_BEGIN();

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
    const __amdgpu_buffer_rsrc_t wrs = wstream_rsrc(wp, NP);
    const unsigned wo = (unsigned)(wave * NP * 1024 + lane * 16);
    auto piece = [&](int i) { return wstream_load(wrs, wo, i * 1024); };
    WRing<R, NP> ring(piece);
    auto take = [&](int i) { return ring.take(i, piece); };
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
    FFN_SEG(0);

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

    FFN_SEG(1);
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
                for (int u = 0; u < 2; ++u)
                    hp[b][mb][2 * g + u] = h_sum2(acc[b][mb][4 * g + 2 * u], acc[b][mb][4 * g + 2 * u + 1], b4[u], s1);
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
    // GELU(LN(h)) -> fp16 into the h tile (unit 8 w + 4 b + g of the row, half hh)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int row = 32 * mb + r;
        const RowStats st = row_stats(lds + kRed, MT, row, eps);
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
                    const f32x2 gl = ln_gelu2(hp[b][mb][2 * g + u], rstd, nmr, g4[u], be4[u]);
                    o[2 * u] = (f16)gl[0];
                    o[2 * u + 1] = (f16)gl[1];
                }
                *(__attribute__((address_space(3))) f16x4*)(lds + kH + row * 1024 + (((8 * wave + 4 * b + g) ^ (row & 15)) << 4) + 8 * hh) = o;
            }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // h complete
    FFN_SEG(2);

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
    FFN_SEG(3);
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
            const f16x4 v = lin_val4(o2[mb], 4 * g, b4);
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
    FFN_SEG_VM(4);
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
                    f16x4 v = lin_val4(a3[b][mb], 4 * g, b4);
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
                        dst = proj3_out<E3>(q3, lr.first, part) + lr.off + cb % kD + 16 * half;
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
    FFN_SEG_VM(5);  // (phase 3 and its epilogue; segment 4 then ends at phase 2's stores)
    FFN_STAMPS_WRITE(wave, stamps_.entry, stamps_.seg[5]);
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
    using L = FfnLds<MT, E3, NB3, kS3 + MT * U3 * 16>;  // the vectors, partials, phase 3's vectors
    constexpr int kPar = L::kPar, kRed = L::kRed, kB3 = L::kB3, kCS = L::kCS, kCSP = L::kCSP;
    static_assert(D >= 1 && D <= 16 && (E3 == E3_NONE) == (NB3 == 0), "shape");
    static_assert(SP == 1 || (E3 != E3_NONE && NB % SP == 0), "parts");
    __shared__ __attribute__((aligned(16))) char smem[L::kEnd];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    // SP > 1: SP workgroups per 16-row tile, each running phases 1 and 2 whole and 1/SP of phase 3
    // (at a few hundred tiles the chip has the CUs; the projection's weight stream and epilogue halve)
    const int part = SP > 1 ? (int)blockIdx.x % SP : 0;
    const int m0 = (SP > 1 ? (int)blockIdx.x / SP : (int)blockIdx.x) * MT;
    FFN_STAMPS_BEGIN();
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

    const __amdgpu_buffer_rsrc_t wrs = wstream_rsrc(wp, NP);
    const unsigned wo = (unsigned)(wave * NP * 1024 + lane * 16);
    // stream position i -> packed piece (phase 3: this part's NBP blocks of each k32 step)
    const int p3off = __builtin_amdgcn_readfirstlane(part * NBP * 1024);
    auto piece = [&](int i) {
        return wstream_load(wrs, wo, i < 96 ? i * 1024 : (96 + NB * ((i - 96) / NBP) + (i - 96) % NBP) * 1024 + p3off);
    };
    WRing<R, NPS> ring(piece);
    auto take = [&](int i) { return ring.take(i, piece); };
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
    FFN_SEG(0);

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
    FFN_SEG(1);

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
        for (int u = 0; u < 2; ++u) hp[b][u] = h_sum2(acc[b][2 * u], acc[b][2 * u + 1], b4[u], s1);
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
    {
        const RowStats st = row_stats(lds + kRed, MT, r, eps);
        const float rstd = st.rstd, nmr = -st.mean * rstd;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int n = 64 * wave + 16 * b + 4 * q;
            const u32x2 g4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + K * 2 + n * 2);
            const u32x2 be4 = *(__attribute__((address_space(3))) u32x2*)(lds + kPar + 2 * K * 2 + n * 2);
            f16x4 o;
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const f32x2 gl = ln_gelu2(hp[b][u], rstd, nmr, g4[u], be4[u]);
                o[2 * u] = (f16)gl[0];
                o[2 * u + 1] = (f16)gl[1];
            }
            *(__attribute__((address_space(3))) f16x4*)(lds + kH + tile_unit(r, n >> 3) + 8 * (q & 1)) = o;
        }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // h complete
    FFN_SEG(2);

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
    FFN_SEG(3);
    // ---- out = fp16(fp16(acc + b2) + x): fp16(acc + b2) into the x' tile, then one 16-B unit a thread
    // (row tid / 32, unit tid % 32) with x from the A tile, to memory and back into the x' tile ----
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int c = 32 * wave + 16 * b + 4 * q;
        const f16x4 b4 = *(__attribute__((address_space(3))) f16x4*)(lds + kPar + 3 * K * 2 + c * 2);
        const f16x4 v = lin_val4(o2[b], 0, b4);
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
    FFN_SEG_VM(4);
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
        FFN_SEG(5);  // (the projection's MFMA loop; its epilogue: segment 6)
        // epilogue: fp16(acc + b3) (+ rotary for q, k) into the staging rows, then one 16-B unit a thread
        // (row, unit u: channels 8 u .. + 7, one head of one part) to its destination
#pragma unroll
        for (int b = 0; b < NBP; ++b) {
            const int c = 16 * (NB * wave + part * NBP + b) + 4 * q;
            const f16x4 b4 = *(__attribute__((address_space(3))) f16x4*)(lds + kB3 + c * 2);
            f16x4 v = lin_val4(a3[b], 0, b4);
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
                        *reinterpret_cast<f16x8*>(proj3_out<E3>(q3, lr.first, j) + off) = v;
                    }
                }
            }
        }
    }
    FFN_SEG_VM(6);
    FFN_STAMPS_WRITE(wave, stamps_.seg[6], stamps_.seg[5]);  // (slot 6: the phase-3 epilogue, not the entry time)
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

// lg_linear_cat_ffn's form (lg_linear_set_ffn_fused): 1 (default) the one-launch ffn_rows_kernel when
// the caller passes the packed weight stream, 0 always its two calls (lg_linear_cat_ln_gelu, then
// lg_linear with the residual). Measured against the
// two calls (profiles/r06/ffn_rows_*_ab.jsonl, op alone, us): P = 1 (2,048 rows) 15.5 -> 12.1, P = 4
// 31.0 -> 14.4, P = 8 32.4 -> 23.4, P = 16 53.6 -> 46.5, P = 32 94.0 -> 87.3; forwards P = 1 / 8 / 16 / 32
// 0.546 / 1.471 / 2.336 / 4.295 -> 0.501 / 1.204 / 2.145 / 4.029 ms. (Round 5's 128-row one-launch form,
// ffn_kernel, GELU output in LDS and W2 fragments per 128-row tile from L2: 56 vs 52.7 us at P = 16, not
// adopted, and removed in round 6: profiles/r05/ffn_one_launch_ab.jsonl.)
std::atomic<int> g_ffn_fused{1};
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
constexpr int kRows16Round = 16 * kTileGrid;  // the rows of one round of 16-row tiles (4,096)
constexpr int kRows32Round = 32 * kTileGrid;  // ... of 32-row tiles (8,192)
// The 16-row kernel's projection split over two workgroups per tile (ffn_rows16_kernel<…, SP = 2>):
// up to 64 tiles. Measured, never / up to 64 tiles / while 2 x tiles fill at most one round
// (profiles/r06/ffn_phase3_split_ab.jsonl, single-pair forwards, ms): n = 512 (64 tiles) 0.368 -> 0.353;
// n = 1024 (128 tiles) 0.427-0.431 -> 0.434 split, kept whole. Three / four parts (one or two blocks
// per wave, an A/B build) : n = 512 0.351-0.354 -> 0.355-0.359, n = 256 0.334 -> 0.325.
int ffn_split_parts(int tiles) { return tiles <= 64 ? 2 : 1; }
template <int E3, int NB3>
void launch_ffn_rows(const LinArgs& p, const f16* gamma, const f16* beta, float eps, const f16* wp, const f16* b2,
                     const Proj3& q3, hipStream_t stream) {
    const int mode = g_ffn_fused.load();
    if (mode == 3 || (mode != 2 && p.m <= kRows16Round)) {
        const f16* wp16 = wp + (size_t)8 * (96 + 16 * NB3) * 1024 / 2;
        const int tiles = (p.m + 15) / 16;
        if constexpr (E3 != E3_NONE) {
            if (ffn_split_parts(tiles) == 2) {
                hipLaunchKernelGGL((ffn_rows16_kernel<kFrDepth, E3, NB3, 2>), dim3(2 * tiles), dim3(512), 0, stream, p,
                                   gamma, beta, eps, wp16, b2, q3);
                return;
            }
        }
        hipLaunchKernelGGL((ffn_rows16_kernel<kFrDepth, E3, NB3>), dim3(tiles), dim3(512), 0, stream, p, gamma, beta, eps,
                           wp16, b2, q3);
    } else if (p.m <= kRows32Round)
        hipLaunchKernelGGL((ffn_rows_kernel<1, kFrDepth, E3, NB3>), dim3((p.m + 31) / 32), dim3(512), 0, stream, p, gamma, beta,
                           eps, wp, b2, q3);
    else
        hipLaunchKernelGGL((ffn_rows_kernel<2, kFrDepth, E3, NB3>), dim3((p.m + 63) / 64), dim3(512), 0, stream, p, gamma, beta,
                           eps, wp, b2, q3);
}
}  // namespace

extern "C" {

int32_t lg_linear_set_ffn_fused(int32_t mode) { return g_ffn_fused.exchange(mode >= 0 && mode <= 3 ? mode : 1); }

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

}  // extern "C"
FFN_STAMPS_READBACK(lg_diag_fr_stamps)
