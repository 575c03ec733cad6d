// mha_hd64_ring.hip — fused FlashAttention-v2 forward, head_dim = 64, for gfx950 (MI355X, CDNA4).
//
// Computes, per (batch, head):  O = softmax(Q·Kᵀ · 0.125) · V
// the operator of the reference's TensorRT plugin "MHAHeadDim64"
// (lightglue_attention_plugin/attention_headdim_64_fp16in_fp16out.cu:253-733 and
//  attention_headdim_64_fp16in_fp32out.cu:253-703; oracle
//  lightglue_pytorch_no_plugin/lightglue.py:75-85).
//
// Design (MI355X-first, not a translation of the CuTe/SM80 kernel):
//  * Workgroup = QW x KW wave64s. Each wave owns 32 query rows: QW waves split the query
//    block, KW waves split the keys of every iteration (intra-workgroup split-KV, merged
//    through LDS at the end). 8-wave workgroups put two waves on every SIMD so one wave's
//    softmax (VALU) runs beside the other's MFMAs. An optional cross-workgroup KV split
//    (`splits`) writes fp32 partials + (m, l) to the workspace and a combine kernel merges
//    them; this is what fills the 256 CUs for a single 1x4x1024x1024 call.
//  * Swapped QKᵀ on v_mfma_f32_32x32x16_f16: Sᵀ = K·Qᵀ puts one query per lane (column)
//    and 16 keys per lane in registers, so the softmax row max / row sum is an in-register
//    reduction plus one v_permlane32_swap.
//  * The score scale 0.125·log2(e) is folded into Q once (fp16), and the running row max
//    is folded into the MFMA's C operand (C = -m, a register block that only changes on a
//    rescale), so the MFMA emits s·c - m directly and a probability is ONE v_exp_f32.
//  * Lazy rescale (max moves only when a tile's max exceeds it by > 8 in log2 units, P
//    stays <= 256 which fp16 carries exactly as well as 1.0): the O accumulators are
//    untouched by VALU in the steady state.
//  * P never touches LDS: the Sᵀ accumulators, packed to f16, are directly the B operand
//    of Oᵀ = Vᵀ·Pᵀ (also 32x32x16 f16); Vᵀ comes from LDS with the gfx950 transposing
//    read ds_read_b64_tr_b16. Oᵀ keeps one query per lane, so alpha is per-lane.
//  * K/V tiles (64 keys x 64 dims fp16 = 8 KiB) are register-staged into a double-buffered
//    LDS ring: global loads for iteration t+1 are issued before the MFMAs of iteration t and
//    written to LDS after them (one barrier per iteration). XOR swizzles keep ds_read_b128
//    (K) and ds_read_b64_tr_b16 (V) conflict-free.
//  * Tails (N % 64 != 0) are masked inside the kernel: no pad / unpad launches (replaces
//    the reference's a4/a5/a7 helper kernels). fp32 inputs are rounded to fp16 (RN) on load
//    (replaces the reference's a6 convert kernel).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "mha_hd64_device.h"
#include "mha_hd64_internal.h"

namespace mha_hd64 {
namespace {


// ----------------------------------------------------------------------------------------
// Main kernel. Grid: x = query blocks of 32*QW rows, y = batch*heads, z = KV splits.
//
// Software pipeline per wave (tile t = this wave's 64 keys of super-tile t):
//   phase A:  QKᵀ MFMAs of tile t+1            ‖ exp / row-sum / f16-pack of tile t (VALU)
//   phase B:  PV MFMAs of tile t               ‖ tail mask + row max of tile t+1 (VALU)
// so the matrix pipe and the vector pipe of a SIMD work on independent data. LDS is a
// 3-stage ring of super-tiles: iteration t reads V(t) and K(t+1) and fills stage t+2
// (loaded into registers at the start of the iteration, written after phase B), one
// barrier per iteration.
// ----------------------------------------------------------------------------------------
// MULTI = false: a launch of one call (plugin enqueue, L0 launchers) reads only c[0], so the
// prologue's kernarg loads issue in one scalar round; MULTI = true: grouped launches.
// RB = 32-row query blocks per wave: RB = 2 shares every K/V fragment read between two
// query blocks (half the LDS read traffic per FLOP), at twice the registers per wave.
template <typename TIn, typename TOut, int QW, int KW, int RB, bool MULTI>
__global__ __launch_bounds__(64 * QW * KW, 1) void mha_hd64_fwd_kernel(FwdArgs a) {
    constexpr int NT = 64 * QW * KW;                // threads
    constexpr int BLOCK_M = 32 * QW * RB;           // query rows per workgroup
    constexpr int SUPER = kTileKV * KW;             // keys per iteration
    constexpr int STAGE_BYTES = KW * 2 * kTileBytes;
    // LDS ring of super-tiles: step t reads K(t+1) and V(t) and refills super-tile t + NSTAGE-1,
    // one barrier per step with the LDS work spread over the step.
    // (Tried and dropped: a ping-pong form of the 8-wave workgroups, load and compute segments of the
    // two waves of a SIMD offset by a barrier and a fourth stage; neutral on the steady loop, which
    // is vector-issue bound, and the fp32-input kernel spilled.)
    // KW = 4 workgroups are the single-super-tile shape: every split is one super-tile (the
    // planner guarantees it), so one stage suffices.
    constexpr int NSTAGE = KW >= 4 ? 1 : 3;
    constexpr int NLOAD = (2 * KW * 512) / NT;      // 16-B chunks staged per thread per iteration
    constexpr unsigned SZ = sizeof(TIn);
    static_assert(NLOAD * NT == 2 * KW * 512, "staging must divide evenly");
    constexpr int OROW = 68;  // epilogue: fp32 row pitch in LDS (64 dims + 4 pad: rows r, r+1 on different banks)
    constexpr int EPI_BYTES = (KW * BLOCK_M * OROW + KW * BLOCK_M * 2) * 4 + 16;  // + the last-arriver word
    constexpr int LDS_BYTES = NSTAGE * STAGE_BYTES > EPI_BYTES ? NSTAGE * STAGE_BYTES : EPI_BYTES;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS exceeds 160 KiB");
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];
    lds_char* const lds = (lds_char*)smem;

    STAMP(0);
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int r = lane & 31;   // query column of the MFMA tiles
    const int hh = lane >> 5;  // half-wave
    const int qw = wave % QW;
    const int kw = wave / QW;
    // XCD-aware order (T1): the dispatcher deals consecutive blocks round-robin over the 8 XCDs;
    // renumber (bijectively, any count) so that the blocks sharing one XCD are consecutive in
    // j = block_begin(call) + split + S*(qtile + qtiles*bh): the KV splits and neighbouring query
    // blocks of one (batch, head) run on one XCD, read its K/V through one L2 and leave their
    // split partials there for the combine kernel (which maps its blocks to the same XCD).
    int qtile, bh, split, j;
    {
        // branch-free (one basic block, so every kernarg load issues in one round):
        // XCD x holds j in [x*q8 + min(x, r8), ...)
        const int T = a.total_blocks, L = blockIdx.x;
        const int q8 = T >> 3, r8 = T & 7, xcd = L & 7;
        j = xcd * q8 + min(xcd, r8) + (L >> 3);
    }
    int ci = 0;
    if constexpr (MULTI) {
#pragma unroll
        for (int i = 1; i < kMaxCalls; ++i) ci += (int)((i < a.n_calls) & (j >= a.c[i].block_begin));
    }
    const CallArgs ca = MULTI ? pick_call(a, ci) : a.c[0];
    {
        const int jl = j - ca.block_begin;
        split = jl % ca.splits;
        const int g = jl / ca.splits;
        qtile = g % ca.qtiles;
        bh = g / ca.qtiles;
    }
    const int nq = ca.nq, nkv = ca.nkv;
    const TIn* Qb = reinterpret_cast<const TIn*>(ca.q) + (size_t)bh * nq * kHeadDim;
    const TIn* Kb = reinterpret_cast<const TIn*>(ca.k) + (size_t)bh * nkv * kHeadDim;
    const TIn* Vb = reinterpret_cast<const TIn*>(ca.v) + (size_t)bh * nkv * kHeadDim;
    const __amdgpu_buffer_rsrc_t q_rs = make_rsrc(Qb, (unsigned)nq * kHeadDim * SZ);
    const __amdgpu_buffer_rsrc_t k_rs = make_rsrc(Kb, (unsigned)nkv * kHeadDim * SZ);
    const __amdgpu_buffer_rsrc_t v_rs = make_rsrc(Vb, (unsigned)nkv * kHeadDim * SZ);
    const int q_row0 = qtile * BLOCK_M + qw * 32 * RB + r;  // + 32 * rb

    const int super_total = (nkv + SUPER - 1) / SUPER;
    const int st_begin = split * ca.tiles_per_split;
    const int st_end = min(super_total, st_begin + ca.tiles_per_split);
    const int n_iter = max(0, st_end - st_begin);

    // Staging: load i of this thread covers tile-tensor tt = i / PER (tile tt/2, K or V by tt&1),
    // row (i % PER) * (NT/8) + tid/8, 16-B chunk tid%8. tt is compile-time, so the K/V descriptor
    // choice stays scalar (no waterfall loop around the buffer load).
    constexpr int PER = 512 / NT;  // loads per thread per 8 KiB tile-tensor
    static_assert(PER * NT == 512, "workgroup size must divide a tile");
    // Two staging register sets: the loads of super-tile t+NSTAGE are issued at step t while the
    // set holding super-tile t+NSTAGE-1 is written to LDS.
    Raw8<TIn> stgA[NLOAD], stgB[NLOAD];
    auto issue = [&](int it, Raw8<TIn>(&stg)[NLOAD]) {
        const unsigned soff = (unsigned)(st_begin + it) * SUPER * kHeadDim * SZ;
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int tt = i / PER;
            const int row = (i % PER) * (NT / 8) + (tid >> 3);
            const unsigned voff = (unsigned)(((tt >> 1) * kTileKV + row) * kHeadDim + (tid & 7) * 8) * SZ;
            bload8(stg[i], (tt & 1) ? v_rs : k_rs, voff, soff);
        }
    };
    auto write = [&](int stage, const Raw8<TIn>(&stg)[NLOAD]) {
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) {
            const int tt = i / PER;
            const int row = (i % PER) * (NT / 8) + (tid >> 3);
            const int ch = tid & 7;
            lds_write16(lds, stage * STAGE_BYTES + tt * kTileBytes + ((tt & 1) ? v_off(row, ch) : k_off(row, ch)),
                        to_f16(stg[i]));
        }
    };

    // Q fragments (B operand of Sᵀ = K·Qᵀ): lane holds Q[q_row][16s + 8hh .. +7] * 0.125*log2(e), fp16.
    f16x8 qf[RB][4];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            Raw8<TIn> t;
            bload8(t, q_rs, (unsigned)((q_row0 + 32 * rb) * kHeadDim + 16 * s + 8 * hh) * SZ, 0);
            const f16x8 h = to_f16(t);
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[rb][s][e] = (f16)((float)h[e] * kScaleLog2);
        }
    // queries with a non-finite Q: fragments zeroed here, their O rows poisoned to NaN before the
    // merge (q_nonfinite_fix, mha_hd64_device.h), so every merge and combine downstream carries it
    unsigned qbad[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) qbad[rb] = q_nonfinite_fix(qf[rb]);

    // Prologue: stage 0 is published first so QKᵀ(0) starts while the next stage(s) are in flight
    // (published right after it).
    // (single-stage ring, KW = 4: every split is one super-tile, so the body is straight-line and
    // the second staging set never exists)
    if (n_iter > 0) issue(0, stgA);
    if constexpr (NSTAGE > 1) {
        if (n_iter > 1) issue(1, stgB);
    }
    if (n_iter > 0) write(0, stgA);
    if constexpr (NSTAGE > 1) {
        if (n_iter > 2) issue(2, stgA);
    }
    __syncthreads();
    STAMP(1);

    // Per-lane LDS addressing (compile-time parts are added as immediates).
    unsigned k_addr[4];  // + (kw * 2) * kTileBytes: this wave's K tile inside a stage
#pragma unroll
    for (int s = 0; s < 4; ++s) k_addr[s] = k_off(r, 2 * s + hh) + (kw * 2) * kTileBytes;
    // V tr-read: lane (group g, idx 4qq+pp) supplies row (4hh + qq) + const, columns
    // 32dt + 16(g&1) + 4pp. Swizzle bit b = (qq>>1)&1 flips the 64-B half (dt).
    const int g16 = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const int vb = (qq >> 1) & 1;
    const int v_lane = 128 * (4 * hh + qq) + 16 * (2 * (g16 & 1) + (pp >> 1)) + 8 * (pp & 1);
    const unsigned v_addr0 = v_lane + 64 * vb + (kw * 2 + 1) * kTileBytes;        // dims 0..31
    const unsigned v_addr1 = v_lane + 64 * (1 - vb) + (kw * 2 + 1) * kTileBytes;  // dims 32..63

    float m_run[RB];          // reference max of this lane's query, log2 units (s·c)
    // Row sums on the matrix pipe: l_acc = ones_sel · P over every k-step (16x16x32 MFMA), so the
    // 31 adds per tile leave the vector pipe. P (the 32x32x16 B operand) read as a 16x16x32 B
    // operand puts query n (lanes 0-15, 32-47) and n+16 (lanes 16-31, 48-63) in column n; the
    // selector row m takes k-group g when ((m>>2)&1) == (g&1), so lane l's four D rows all hold
    // the sum of query l&31 over the step's 16 keys (both half-waves) — the lane's own query.
    const f16 sel = (((lane & 15) >> 2) & 1) == ((lane >> 4) & 1) ? (f16)1.f : (f16)0.f;
    const f16x8 a_sum = f16x8{sel, sel, sel, sel, sel, sel, sel, sel};
    f32x4 l_acc[RB];
    // Bias k-step of the QKᵀ chains: A (key side) = [1, 1, mask] per key row, B (query side) =
    // [-m_hi, -m_lo, 1] per query, in k-slots 0..2 of the lower half-wave (zeros elsewhere).
    // One extra MFMA per chain adds -m (fp16 hi + lo, error ~|m|·2^-22) and the tail mask, so
    // the chain starts from an inline-zero C (no register copy) and the softmax needs no
    // subtraction and no masking VALU.
    const f16 one_h = hh == 0 ? (f16)1.f : (f16)0.f;
    const f16x8 a_bias = f16x8{one_h, one_h, 0, 0, 0, 0, 0, 0};
    f16x8 b_bias[RB];
    auto set_bias = [&](int rb) {
        const f16 hi = (f16)(-m_run[rb]);
        const f16 lo = (f16)(-m_run[rb] - (float)hi);
        b_bias[rb] = hh == 0 ? f16x8{hi, lo, (f16)1.f, 0, 0, 0, 0, 0} : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    };
    f32x16 o0[RB], o1[RB];  // Oᵀ tiles: dims 0..31 and 32..63, query on the lane
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        m_run[rb] = 0.f;
        l_acc[rb] = f32x4{0.f, 0.f, 0.f, 0.f};
        b_bias[rb] = f16x8{0, 0, one_h, 0, 0, 0, 0, 0};  // m_run = 0
        o0[rb] = f32x16{};
        o1[rb] = f32x16{};
    }

    // K fragments of the tile in stage kstage (A operand of Sᵀ = K·Qᵀ, 8 x ds_read_b128).
    auto read_k = [&](unsigned kstage, f16x8(&kf)[8]) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const unsigned ka = k_addr[s] + kstage;
            kf[2 * s] = lds_read16(lds, ka);
            kf[2 * s + 1] = lds_read16(lds, ka + 32 * 128);
        }
    };
    // QKᵀ chain step i (0..9) of the tile: i = 0,1 are the bias k-steps of the two 32-key halves,
    // then K·Qᵀ over the 4 dim k-steps alternating halves. Scores s·c - m (log2 units), masked
    // keys at ~-65504. Split per MFMA so the caller can interleave vector work between them.
    auto qk_step = [&](int i, const f16x8(&kf)[8], const f16x8& ab0, const f16x8& ab1, f32x16& s0, f32x16& s1,
                       int rb) {
        const f32x16 zero = {};
        if (i == 0) s0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ab0, b_bias[rb], zero, 0, 0, 0);
        else if (i == 1) s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(ab1, b_bias[rb], zero, 0, 0, 0);
        else if ((i & 1) == 0)
            s0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[i - 2], qf[rb][(i - 2) >> 1], s0, 0, 0, 0);
        else s1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[i - 2], qf[rb][(i - 2) >> 1], s1, 0, 0, 0);
    };
    auto qk = [&](unsigned kstage, const f16x8& ab0, const f16x8& ab1, f32x16(&s0)[RB], f32x16(&s1)[RB]) {
        f16x8 kf[8];
        read_k(kstage, kf);
#pragma unroll
        for (int i = 0; i < 10; ++i)
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) qk_step(i, kf, ab0, ab1, s0[rb], s1[rb], rb);
    };
    // Tail mask (reference: last KV tile only, …fp16out.cu:475-494): the bias A operand of the
    // tile carries kMaskBias in k-slot 2 for key rows >= nkv. Only the last super-tile of the
    // call can hold such keys; the steady-state loop below never runs it.
    auto a_bias_tile = [&](int t, int half) -> f16x8 {
        const int key = (st_begin + t) * SUPER + kw * kTileKV + 32 * half + r;
        const f16 mk = (hh == 0 && key >= nkv) ? (f16)kMaskBias : (f16)0.f;
        return f16x8{one_h, one_h, mk, 0, 0, 0, 0, 0};
    };
    const bool tail = (st_begin + n_iter) * SUPER > nkv;  // last super-tile of this split is partial

    // Ring stage of tile `it` (scalar, advanced once per step).
    int st_cur = 0;
    // Step `it` writes super-tile it+3 from set `wr` and issues super-tile it+4 into set `is`.
#ifdef MHA_STEPSTAMPS
    unsigned long long ck[4] = {}, ck_prev[4] = {}, ck_sum[4] = {};
    bool ck_first = true;
#endif
    auto step = [&](int it, f32x16(&c0)[RB], f32x16(&c1)[RB], const float(&mxc)[RB], f32x16(&n0)[RB],
                    f32x16(&n1)[RB], float(&mxn)[RB],
                    auto has_next_c, bool mask_next, Raw8<TIn>(&wr)[NLOAD], Raw8<TIn>(&is)[NLOAD],
                    bool may_issue, bool may_write) {
        constexpr bool HAS_NEXT = decltype(has_next_c)::value;
        const int st_nxt = st_cur == NSTAGE - 1 ? 0 : st_cur + 1;
        const int st_fill = st_cur == 0 ? NSTAGE - 1 : st_cur - 1;  // (st_cur + NSTAGE-1) mod NSTAGE
        // In the steady loop the refill is unconditional (may_issue = true at compile time): a
        // super-tile past this split's last one lands in a stage nobody reads, and past nkv the
        // buffer descriptor returns zeros. A conditional load would make the compiler's vmcnt
        // analysis drain every load at the next LDS write.
        if (may_issue) issue(it + NSTAGE, is);
        TCLK(ck[0]);

        // Fragment reads first: K of tile it+1 (phase A) and Vᵀ of tile it (phase B); both stages
        // are complete since the last barrier, and the reads land while the bias MFMAs run.
        f16x8 kf[8];
        // (8-wave workgroups with fp32 staging registers read Vᵀ in phase B instead: the early
        // reads' 32 VGPRs would spill there.)
        constexpr bool kEarlyV = !(NT == 512 && SZ == 4);
        f16x8 vfa[2][2], vfb[2][2];
        auto read_v = [&]() {
            const unsigned va0 = v_addr0 + (unsigned)st_cur * STAGE_BYTES;
            const unsigned va1 = v_addr1 + (unsigned)st_cur * STAGE_BYTES;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int ss = 0; ss < 2; ++ss) {
                    const unsigned rowc = 128 * (32 * j + 16 * ss);
                    vfa[j][ss] = cat8(tr_read(lds, va0 + rowc), tr_read(lds, va0 + rowc + 8 * 128));
                    vfb[j][ss] = cat8(tr_read(lds, va1 + rowc), tr_read(lds, va1 + rowc + 8 * 128));
                }
        };
        // online-softmax decision for tile `it` (first tile: set the max exactly; later tiles:
        // move it only when some query's tile max exceeds it by > kRescaleThr)
        const bool first = (it == 0);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            if (first || __builtin_amdgcn_ballot_w64(mxc[rb] > kRescaleThr) != 0) {  // wave-uniform, rare
                const float d = first ? ((mxc[rb] < kEmptyMax) ? 0.f : mxc[rb])  // fully masked tile: m = 0
                                      : fmaxf(mxc[rb], 0.f);
                const float alpha = first ? 0.f : __builtin_amdgcn_exp2f(-d);
                o0[rb] *= alpha;
                o1[rb] *= alpha;
                l_acc[rb] *= alpha;
                m_run[rb] += d;
                c0[rb] -= d;
                c1[rb] -= d;
                set_bias(rb);
            }
        }

        if constexpr (HAS_NEXT) read_k((unsigned)st_nxt * STAGE_BYTES, kf);
        if constexpr (kEarlyV && !HAS_NEXT) read_v();

        // phase A: QKᵀ(it+1) on the matrix pipe ‖ exp(it) on the vector pipe, pinned as one MFMA
        // followed by three v_exp_f32 per gap (8 + 3·8 issue cycles fill the MFMA's 32).
        auto exp_at = [&](int e) {  // e in [0, 32*RB): query block e/32, score e%32
            const int rb = e >> 5, i = e & 31;
            if (i < 16) c0[rb][i] = __builtin_amdgcn_exp2f(c0[rb][i]);
            else c1[rb][i - 16] = __builtin_amdgcn_exp2f(c1[rb][i - 16]);
        };
        if constexpr (HAS_NEXT) {
            const f16x8 ab0 = mask_next ? a_bias_tile(it + 1, 0) : a_bias;
            const f16x8 ab1 = mask_next ? a_bias_tile(it + 1, 1) : a_bias;
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < 10; ++i)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    qk_step(i, kf, ab0, ab1, n0[rb], n1[rb], rb);
                    // Vᵀ reads queue behind the K reads (phase A carries all fragment reads).
                    if (kEarlyV && i == 2 && rb == 0) read_v();
                    const int g = i * RB + rb;
                    exp_at(3 * g);
                    exp_at(3 * g + 1);
                    exp_at(3 * g + 2);
                    __builtin_amdgcn_sched_barrier(0);
                }
            TCLK(ck[1]);
#pragma unroll
            for (int e = 30 * RB; e < 32 * RB; ++e) exp_at(e);
        } else {
#pragma unroll
            for (int e = 0; e < 32 * RB; ++e) exp_at(e);
        }
        f16x8 p[RB][2][2];  // P (f16) as the B operand: registers 8ss..8ss+7 of a 32x32 tile = k-step ss
#pragma unroll
        for (int rb = 0; rb < RB; ++rb)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                p[rb][0][0][e] = (f16)c0[rb][e];
                p[rb][0][1][e] = (f16)c0[rb][8 + e];
                p[rb][1][0][e] = (f16)c1[rb][e];
                p[rb][1][1][e] = (f16)c1[rb][8 + e];
            }

        // phase B: Oᵀ += Vᵀ·Pᵀ (it) and the row sums on the matrix pipe ‖ row max (it+1) and the
        // LDS refill of super-tile it+NSTAGE-1 (its stage held tile it-1).
        if constexpr (!kEarlyV) read_v();
        if (may_write) write(st_fill, wr);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss)
#pragma unroll
                for (int rb = 0; rb < RB; ++rb) {
                    o0[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vfa[j][ss], p[rb][j][ss], o0[rb], 0, 0, 0);
                    o1[rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vfb[j][ss], p[rb][j][ss], o1[rb], 0, 0, 0);
                    l_acc[rb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a_sum, p[rb][j][ss], l_acc[rb], 0, 0, 0);
                }
        if constexpr (HAS_NEXT) {
#pragma unroll
            for (int rb = 0; rb < RB; ++rb) mxn[rb] = xhalf_max(tree_max(n0[rb], n1[rb]));
        }

        TCLK(ck[2]);
#ifdef MHA_STEPSTAMPS
        if (HAS_NEXT) {  // previous full step's phases (its clocks have returned by now)
            ck_sum[0] += ck_prev[1] - ck_prev[0];
            ck_sum[1] += ck_prev[2] - ck_prev[1];
            ck_sum[2] += ck_prev[3] - ck_prev[2];
            ck_sum[3] += 1;
        }
#endif
        __syncthreads();
        TCLK(ck[3]);
#ifdef MHA_STEPSTAMPS
        if (HAS_NEXT) {
            for (int i = 0; i < 4; ++i) ck_prev[i] = ck[i];
        }
#endif
        st_cur = st_nxt;
    };

    // Scores ping-pong between two named register sets (no runtime-indexed arrays, no copies).
    f32x16 sA0[RB], sA1[RB], sB0[RB], sB1[RB];
    float mxA[RB], mxB[RB];
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) mxA[rb] = mxB[rb] = 0.f;
    using T_ = std::true_type;
    using F_ = std::false_type;
    if (n_iter > 0) {
        if (tail && n_iter == 1)
            qk(0u, a_bias_tile(0, 0), a_bias_tile(0, 1), sA0, sA1);
        else
            qk(0u, a_bias, a_bias, sA0, sA1);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) mxA[rb] = xhalf_max(tree_max(sA0[rb], sA1[rb]));
    }
    if constexpr (NSTAGE == 1) {
        if (n_iter > 0) step(0, sA0, sA1, mxA, sB0, sB1, mxB, F_{}, false, stgA, stgA, false, false);
    } else {
    if (n_iter > 1) write(1, stgB);
    if (n_iter > 1) __syncthreads();
    // The first step writes super-tile NSTAGE-1 from stgA and issues into stgB.
    int it = 0;
    // Steady state: tiles it+1 and it+2 exist and neither is the (possibly partial) last one.
    // Refill issue / write are unconditional here (see step).
    for (; it + 3 < n_iter; it += 2) {
        step(it, sA0, sA1, mxA, sB0, sB1, mxB, T_{}, false, stgA, stgB, true, true);
        step(it + 1, sB0, sB1, mxB, sA0, sA1, mxA, T_{}, false, stgB, stgA, true, true);
    }
    // Tail (at most 3 iterations): same step with the mask flag live; scores and the pending
    // staging set move back after each step.
    for (; it + 1 < n_iter; ++it) {
        step(it, sA0, sA1, mxA, sB0, sB1, mxB, T_{}, tail && (it + 2 == n_iter), stgA, stgB, it + NSTAGE < n_iter,
             it + NSTAGE - 1 < n_iter);
#pragma unroll
        for (int rb = 0; rb < RB; ++rb) {
            sA0[rb] = sB0[rb];
            sA1[rb] = sB1[rb];
            mxA[rb] = mxB[rb];
        }
#pragma unroll
        for (int i = 0; i < NLOAD; ++i) stgA[i] = stgB[i];
    }
    if (it < n_iter) step(it, sA0, sA1, mxA, sB0, sB1, mxB, F_{}, false, stgA, stgB, false, false);
    }  // NSTAGE > 1
    STAMP(2);

    // ---- epilogue ----
    // Every wave stages its Oᵀ accumulators as fp32 rows (at its own max) plus (m, l) in LDS;
    // then all threads merge the KW key-split partials of a row and write whole 16-byte row
    // chunks (a wave stores complete rows: coalesced, few store instructions).
    // A wave that saw no key (all of its tiles past nkv) gets m = -inf (weight 0). The test uses
    // the cross-half total: the halves hold disjoint keys but the SAME query's m and O dims.
    float* ol = reinterpret_cast<float*>(smem);     // [KW][BLOCK_M][OROW]
    float* mlb = ol + KW * BLOCK_M * OROW;          // [KW][BLOCK_M][2]
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
        if (qbad[rb]) {  // wave-uniform, rare
            const float pois = inv_or_nan(1.f, qbad[rb], r);  // NaN on a bad query's lanes, else 1
            o0[rb] *= pois;
            o1[rb] *= pois;
        }
        const float L_w = l_acc[rb][0];  // the row-sum MFMA already spans both half-waves
        const float m_w = (L_w > 0.f) ? m_run[rb] : -INFINITY;
        const int row = qw * 32 * RB + 32 * rb + r;
        float* dst = ol + (kw * BLOCK_M + row) * OROW;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
            const int d = 8 * g4 + 4 * hh;
            *reinterpret_cast<f32x4*>(dst + d) =
                f32x4{o0[rb][4 * g4], o0[rb][4 * g4 + 1], o0[rb][4 * g4 + 2], o0[rb][4 * g4 + 3]};
            *reinterpret_cast<f32x4*>(dst + 32 + d) =
                f32x4{o1[rb][4 * g4], o1[rb][4 * g4 + 1], o1[rb][4 * g4 + 2], o1[rb][4 * g4 + 3]};
        }
        if (hh == 0) *reinterpret_cast<float2*>(mlb + (kw * BLOCK_M + row) * 2) = make_float2(m_w, L_w);
    }
    __syncthreads();
    STAMP(3);

    // Thread -> (row, chunk of 8 dims); 8 threads per row, NT/8 rows per pass. Stores are 16-B
    // buffer stores through per-head descriptors.
    const int q_base = qtile * BLOCK_M;
    const __amdgpu_buffer_rsrc_t o_rs =
        make_rsrc(reinterpret_cast<TOut*>(ca.o) + (size_t)bh * nq * kHeadDim, (unsigned)(nq * kHeadDim * sizeof(TOut)));
    const __amdgpu_buffer_rsrc_t po_rs =
        make_rsrc(reinterpret_cast<TOut*>(ca.part_o) + (size_t)bh * ca.splits * nq * kHeadDim,
                  (unsigned)(ca.splits * nq * kHeadDim * sizeof(TOut)));
    // In-launch combine: every split's workgroup publishes its partial write-through (sc1) and
    // takes a ticket; the group's last arriver reads all the group's partials back and writes O
    // (same arithmetic and order as the combine kernel, so both forms give the same bits). Visibility follows MI355X_MICROARCH.md "Valid forms" (table
    // row 1): all partial bytes stored sc1 and drained (vmcnt(0)) before one lane's agent-scope
    // add, every load of them an sc1 buffer load, the other waves behind a barrier.
    const bool fused = a.tickets != nullptr && ca.splits > 1;
    const __amdgpu_buffer_rsrc_t pml_rs =
        make_rsrc(ca.part_ml + (size_t)bh * ca.splits * nq, (unsigned)(ca.splits * nq * sizeof(float2)));
    // Epilogue items: (row, chunk of DPT dims). DPT = 8 while a pass has no more threads than
    // items; workgroups with twice as many threads as 8-dim items (32-row (1,8)) use 4-dim chunks
    // so every thread merges and stores.
    constexpr int DPT = BLOCK_M * 8 >= NT ? 8 : 4;
    constexpr int CPR = kHeadDim / DPT;  // chunks per row
    constexpr int EITEMS = BLOCK_M * CPR;
    constexpr int EPASS = (EITEMS + NT - 1) / NT;
    static_assert(EITEMS % NT == 0, "epilogue items must tile the workgroup");
    using RawD = typename std::conditional<DPT == 8, Raw8<TOut>, Raw4<TOut>>::type;
    // merge of the KW key-wave partials of (row, dims c..c+DPT-1) staged in LDS
    auto merge_waves = [&](int row, int c, float& M, float& L, f32x4& acc0, f32x4& acc1) {
        M = -INFINITY;
        float2 ml[KW];
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            ml[k] = *reinterpret_cast<const float2*>(mlb + (k * BLOCK_M + row) * 2);
            M = fmaxf(M, ml[k].x);
        }
        acc0 = f32x4{0.f, 0.f, 0.f, 0.f};
        acc1 = f32x4{0.f, 0.f, 0.f, 0.f};
        L = 0.f;
#pragma unroll
        for (int k = 0; k < KW; ++k) {
            const float w = (ml[k].x == -INFINITY) ? 0.f : __builtin_amdgcn_exp2f(ml[k].x - M);
            L += w * ml[k].y;
            const float* src = ol + (k * BLOCK_M + row) * OROW + c;
            acc0 += w * *reinterpret_cast<const f32x4*>(src);
            if constexpr (DPT == 8) acc1 += w * *reinterpret_cast<const f32x4*>(src + 4);
        }
    };
#pragma unroll
    for (int pass = 0; pass < EPASS; ++pass) {
        const int idx = pass * NT + tid;
        const int row = idx / CPR;
        const int chunk = idx % CPR;
        const int c = chunk * DPT;
        const int q = q_base + row;
        float M, L;
        f32x4 acc0, acc1;
        merge_waves(row, c, M, L, acc0, acc1);
        if (q < nq) {
            if (ca.splits == 1) {
                const float inv = 1.f / L;
                store_dims<TOut, DPT, 0>(o_rs, (unsigned)((q * kHeadDim + c) * sizeof(TOut)), acc0 * inv, acc1 * inv);
            } else {
                // Partial O_s / l_s in the output precision (fp16 halves the partial traffic of
                // the fp16 path; the fp32-output path keeps fp32), merged with weights l_s·2^(m_s-M).
                const unsigned prow = (unsigned)(split * nq + q);
                const float inv = (L > 0.f) ? 1.f / L : 0.f;
                const unsigned poff = prow * (unsigned)(kHeadDim * sizeof(TOut)) + c * (unsigned)sizeof(TOut);
                if (fused) {
                    store_dims<TOut, DPT, kSC1>(po_rs, poff, acc0 * inv, acc1 * inv);
                    if (chunk == 0)
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, make_float2(M, L)), pml_rs,
                                                              prow * (unsigned)sizeof(float2), 0, kSC1);
                } else {
                    store_dims<TOut, DPT, 0>(po_rs, poff, acc0 * inv, acc1 * inv);
                    if (chunk == 0) ca.part_ml[((size_t)bh * ca.splits) * nq + prow] = make_float2(M, L);
                }
            }
        }
    }
    if (fused) {  // workgroup-uniform
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        unsigned* last_word = reinterpret_cast<unsigned*>(smem + EPI_BYTES - 16);
        if (tid == 0) {
            unsigned* t = a.tickets + (j - split);
            const unsigned old = __hip_atomic_fetch_add(t, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned last = old + 1 == (unsigned)ca.splits;
            if (last) __hip_atomic_store(t, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *last_word = last;
        }
        __syncthreads();
        STAMP(5);
        if (*last_word) {
#pragma unroll
            for (int pass = 0; pass < EPASS; ++pass) {
                const int idx = pass * NT + tid;
                const int row = idx / CPR;
                const int c = (idx % CPR) * DPT;
                const int q = q_base + row;
                if (q >= nq) continue;
                // every split's partial as stored (its own too), merged in split order exactly as
                // the combine kernel does: the result does not depend on which split came last
                float2 ml[kMaxSplits];
                RawD pv[kMaxSplits];
#pragma unroll
                for (int s2 = 0; s2 < kMaxSplits; ++s2) {
                    if (s2 < ca.splits) {
                        const unsigned prow = (unsigned)(s2 * nq + q);
                        ml[s2] = __builtin_bit_cast(
                            float2, __builtin_amdgcn_raw_buffer_load_b64(pml_rs, prow * (unsigned)sizeof(float2), 0, kSC1));
                        const unsigned off = prow * (unsigned)(kHeadDim * sizeof(TOut)) + c * (unsigned)sizeof(TOut);
                        if constexpr (DPT == 8) bload8_aux<kSC1>(pv[s2], po_rs, off);
                        else bload4_aux<kSC1>(pv[s2], po_rs, off);
                    }
                }
                float Mt = -INFINITY;
#pragma unroll
                for (int s2 = 0; s2 < kMaxSplits; ++s2)
                    if (s2 < ca.splits) Mt = fmaxf(Mt, ml[s2].x);
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                float L = 0.f;
#pragma unroll
                for (int s2 = 0; s2 < kMaxSplits; ++s2) {
                    if (s2 < ca.splits) {
                        const float w = split_weight(ml[s2], Mt);
                        L += w;
                        if constexpr (DPT == 8) {
                            f32x4 lo, hi;
                            raw8_to_f32(pv[s2], lo, hi);
                            split_accumulate(acc0, w, lo);
                            split_accumulate(acc1, w, hi);
                        } else {
                            split_accumulate(acc0, w, raw4_to_f32(pv[s2]));
                        }
                    }
                }
                const float inv = 1.f / L;
                store_dims<TOut, DPT, 0>(o_rs, (unsigned)((q * kHeadDim + c) * sizeof(TOut)), split_scale(acc0, inv),
                                         split_scale(acc1, inv));
            }
        }
    }
    STAMP(4);
#ifdef MHA_STEPSTAMPS
    if (lane == 0) {
        unsigned long long* dst = a.stamps + (1 << 16) + ((size_t)blockIdx.x * 8 + wave) * 4;
        // the first accumulated step has zero deltas (ck_prev unset): subtract it out on the host
        for (int i = 0; i < 4; ++i) dst[i] = ck_sum[i];
    }
    (void)ck_first;
#endif
}

// ----------------------------------------------------------------------------------------
// Split-KV combine: O = Σ_s w_s Ô_s / Σ_s w_s with w_s = l_s·2^(m_s - M) (m in log2 units) and
// Ô_s = O_s / l_s the partial as stored (TOut precision). One thread per (row, 4-dim chunk).
// Block b serves XCD b % 8: it combines rows whose partials the main kernel produced on that same XCD (same bijective block order), so the reads hit L2. All
// partials of a row are loaded in one round trip (S <= kMaxSplits).
// ----------------------------------------------------------------------------------------

struct CombineCall {
    const void* part_o;
    const float2* part_ml;
    void* out;
    int nq;
    int splits;
    int qtiles;       // query blocks per (batch, head) of the main kernel
    int pad_;
};
// Block b of the combine grid serves XCD x = b % 8 (k = b / 8): blocks k in
// [kbeg[x][i], kbeg[x][i+1]) serve call i, starting at query group gbeg[x][i] (the first group
// whose first split block ran on XCD x). A block is 16 rows of one query group (block_m is a
// multiple of 16), so the call, the group and its (batch*head, query block) are block-uniform.
struct CombineArgs {
    CombineCall c[kMaxCalls];
    int kbeg[8][kMaxCalls + 1];
    int gbeg[8][kMaxCalls];
    int n_calls;
    int block_m_log2;  // rows per query block = 1 << block_m_log2
    int per_xcd;       // combine blocks per XCD
    int main_blocks;   // single-call form: grid of the main kernel
    int groups0;       // single-call form: query groups of call 0
};

template <typename T>
__device__ __forceinline__ f32x4 load4f(const T* p) {
    if constexpr (sizeof(T) == 2) {
        const f16x4 h = *reinterpret_cast<const f16x4*>(p);
        return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
    } else {
        return *reinterpret_cast<const f32x4*>(p);
    }
}

// MULTI = false (one call): the XCD's first group is computed from the main grid in scalar
// arithmetic (no dependent kernarg table lookups); MULTI = true reads the per-XCD table.
template <typename TOut, bool MULTI>
__global__ __launch_bounds__(256) void mha_hd64_combine_kernel(CombineArgs c) {
    const int x = blockIdx.x & 7, k = blockIdx.x >> 3;
    CombineCall cc = c.c[0];
    int kb = 0, gb;
    if constexpr (MULTI) {
        int ci = -1;
#pragma unroll
        for (int i = 0; i < kMaxCalls; ++i)
            if (i < c.n_calls && k >= c.kbeg[x][i] && k < c.kbeg[x][i + 1]) ci = i;
        if (ci < 0) return;
        kb = c.kbeg[x][0];
        gb = c.gbeg[x][0];
#pragma unroll
        for (int i = 1; i < kMaxCalls; ++i)
            if (ci == i) {
                cc = c.c[i];
                kb = c.kbeg[x][i];
                gb = c.gbeg[x][i];
            }
    } else {
        const int T = c.main_blocks, q8 = T >> 3, r8 = T & 7;
        const int jlo = x * q8 + min(x, r8), jhi = (x + 1) * q8 + min(x + 1, r8);
        const int groups = c.groups0;
        const int glo = min(groups, (jlo + cc.splits - 1) / cc.splits);
        const int ghi = min(groups, (jhi + cc.splits - 1) / cc.splits);
        if (k >= ((ghi - glo) << c.block_m_log2) / 16) return;
        gb = glo;
    }
    const int row0 = (k - kb) * 16;                       // first row of this block in the segment
    const int g = gb + (row0 >> c.block_m_log2);          // block-uniform query group
    const int bh = g / cc.qtiles, qt = g - bh * cc.qtiles;
    const int q = (qt << c.block_m_log2) + (row0 & ((1 << c.block_m_log2) - 1)) + ((int)threadIdx.x >> 4);
    if (q >= cc.nq) return;
    const int chunk = threadIdx.x & 15;
    const size_t base = (size_t)bh * cc.splits * cc.nq + q;
    const TOut* po = reinterpret_cast<const TOut*>(cc.part_o);
    float2 ml[kMaxSplits];
    f32x4 v[kMaxSplits];
#pragma unroll
    for (int s = 0; s < kMaxSplits; ++s) {
        if (s < cc.splits) {
            const size_t pr = base + (size_t)s * cc.nq;
            ml[s] = cc.part_ml[pr];
            v[s] = load4f<TOut>(po + pr * kHeadDim + chunk * 4);
        }
    }
    float M = -INFINITY;
#pragma unroll
    for (int s = 0; s < kMaxSplits; ++s)
        if (s < cc.splits) M = fmaxf(M, ml[s].x);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float L = 0.f;
#pragma unroll
    for (int s = 0; s < kMaxSplits; ++s) {
        if (s < cc.splits) {
            const float w = split_weight(ml[s], M);
            L += w;
            split_accumulate(acc, w, v[s]);
        }
    }
    const f32x4 o = split_scale(acc, 1.f / L);
    TOut* out = reinterpret_cast<TOut*>(cc.out) + ((size_t)bh * cc.nq + q) * kHeadDim + chunk * 4;
    store4<TOut>(out, o[0], o[1], o[2], o[3]);
}

template <typename TIn, typename TOut, int QW, int KW, int RB, bool MULTI>
hipError_t launch_fwd(const FwdArgs& a, int grid, hipStream_t stream) {
    hipLaunchKernelGGL((mha_hd64_fwd_kernel<TIn, TOut, QW, KW, RB, MULTI>), dim3(grid), dim3(64 * QW * KW), 0, stream,
                       a);
    return hipGetLastError();
}

// Grouped launches (several calls) exist for the shapes the planner picks on its own.
template <typename TIn, typename TOut>
hipError_t launch_fwd_shape(const FwdArgs& a, int grid, int qw, int kw, int rb, hipStream_t stream) {
    if (a.n_calls > 1) {
        switch (rb * 64 + qw * 8 + kw) {
            case 64 + 4 * 8 + 1: return launch_fwd<TIn, TOut, 4, 1, 1, true>(a, grid, stream);  // > 256 128-row blocks
            case 64 + 2 * 8 + 2: return launch_fwd<TIn, TOut, 2, 2, 1, true>(a, grid, stream);
            case 64 + 4 * 8 + 2: return launch_fwd<TIn, TOut, 4, 2, 1, true>(a, grid, stream);
            case 128 + 2 * 8 + 2: return launch_fwd<TIn, TOut, 2, 2, 2, true>(a, grid, stream);
            case 64 + 2 * 8 + 4: return launch_fwd<TIn, TOut, 2, 4, 1, true>(a, grid, stream);
            case 64 + 1 * 8 + 8: return launch_fwd<TIn, TOut, 1, 8, 1, true>(a, grid, stream);
            default: return hipErrorInvalidValue;
        }
    }
    switch (rb * 64 + qw * 8 + kw) {
        case 64 + 4 * 8 + 1: return launch_fwd<TIn, TOut, 4, 1, 1, false>(a, grid, stream);
        case 64 + 2 * 8 + 2: return launch_fwd<TIn, TOut, 2, 2, 1, false>(a, grid, stream);
        case 64 + 1 * 8 + 2: return launch_fwd<TIn, TOut, 1, 2, 1, false>(a, grid, stream);
        case 64 + 4 * 8 + 2: return launch_fwd<TIn, TOut, 4, 2, 1, false>(a, grid, stream);
        case 64 + 2 * 8 + 4: return launch_fwd<TIn, TOut, 2, 4, 1, false>(a, grid, stream);
        case 64 + 1 * 8 + 4: return launch_fwd<TIn, TOut, 1, 4, 1, false>(a, grid, stream);
        case 64 + 1 * 8 + 8: return launch_fwd<TIn, TOut, 1, 8, 1, false>(a, grid, stream);
        case 128 + 2 * 8 + 2: return launch_fwd<TIn, TOut, 2, 2, 2, false>(a, grid, stream);
        default: return hipErrorInvalidValue;
    }
}

template <typename TOut>
hipError_t launch_combine(const CombineArgs& c, hipStream_t stream) {
    if (c.n_calls > 1)
        hipLaunchKernelGGL((mha_hd64_combine_kernel<TOut, true>), dim3(8 * c.per_xcd), dim3(256), 0, stream, c);
    else
        hipLaunchKernelGGL((mha_hd64_combine_kernel<TOut, false>), dim3(8 * c.per_xcd), dim3(256), 0, stream, c);
    return hipGetLastError();
}


// ---- Float boundary onto the single-pass kernels ----
// fp32 Q/K/V of launches the single-pass kernels take (as fp16) are rounded to fp16 (RNE, the
// reference's convert kernel …fp16in_fp32out.cu:706-804 without its padding) into the caller's
// workspace by one elementwise launch, then run there; the LDS-ring kernel converts on load instead.
struct ConvArgs {
    const float* src[kConvMax];
    f16* dst[kConvMax];
    unsigned end8[kConvMax];  // prefix sums of each tensor's element count / 8
    int count;
};

__global__ __launch_bounds__(256) void convert_f32_f16_kernel(ConvArgs c) {
    const unsigned g = blockIdx.x * 256u + threadIdx.x;
    int t = 0;
#pragma unroll
    for (int i = 0; i < kConvMax - 1; ++i) t += (int)((i < c.count - 1) & (g >= c.end8[i]));
    if (g >= c.end8[t]) return;
    const unsigned idx = g - (t ? c.end8[t - 1] : 0u);
    const f32x4* s = reinterpret_cast<const f32x4*>(c.src[t]) + 2 * (size_t)idx;
    const f32x4 lo = s[0], hi = s[1];
    const f16x4 a = __builtin_convertvector(lo, f16x4), b = __builtin_convertvector(hi, f16x4);
    reinterpret_cast<f16x8*>(c.dst[t])[idx] = f16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

}  // namespace

// The launchers below are what the host side (mha_hd64_launch.hip) sees of this file; the kernels'
// argument structs stay in the anonymous namespace (their names are part of the kernels' symbols).
bool valid_shape(int qw, int kw, int rb) {
    if (rb == 2) return qw == 2 && kw == 2;
    return rb == 1 && ((qw == 4 && kw == 1) || (qw == 2 && kw == 2) || (qw == 1 && kw == 2) || (qw == 4 && kw == 2) ||
                       (qw == 2 && kw == 4) || (qw == 1 && kw == 4) || (qw == 1 && kw == 8));
}

hipError_t launch_ring(const FwdArgs& a, int grid, int qw, int kw, int rb, bool in_f32, bool out_f32,
                       hipStream_t stream) {
    if (!in_f32)
        return out_f32 ? launch_fwd_shape<f16, float>(a, grid, qw, kw, rb, stream)
                       : launch_fwd_shape<f16, f16>(a, grid, qw, kw, rb, stream);
    return out_f32 ? launch_fwd_shape<float, float>(a, grid, qw, kw, rb, stream)
                   : launch_fwd_shape<float, f16>(a, grid, qw, kw, rb, stream);
}

hipError_t launch_combine(const FwdArgs& a, int block_m, bool out_f32, hipStream_t stream) {
    CombineArgs cb{};
    for (int i = 0; i < a.n_calls; ++i) {
        const CallArgs& ca = a.c[i];
        cb.c[i] = CombineCall{ca.part_o, ca.part_ml, ca.o, ca.nq, ca.splits, ca.qtiles, 0};
    }
    // Combine grid: for every XCD x, the groups (of calls that split) whose first split block
    // ran on x (same bijective order as the main kernel), 16 rows per block.
    const int blocks = a.total_blocks, n_live = a.n_calls;
    cb.n_calls = n_live;
    cb.block_m_log2 = block_m == 32 ? 5 : (block_m == 64 ? 6 : 7);
    auto xb = [&](int xx) {
        const int q8 = blocks >> 3, r8 = blocks & 7;
        return xx < r8 ? xx * (q8 + 1) : r8 * (q8 + 1) + (xx - r8) * q8;
    };
    auto fg = [](int j, int b0, int S) { return j <= b0 ? 0 : (j - b0 + S - 1) / S; };
    int per_xcd = 0;
    for (int x = 0; x < 8; ++x) {
        const int jlo = xb(x), jhi = xb(x + 1);
        int kk = 0;
        for (int i = 0; i < n_live; ++i) {
            cb.kbeg[x][i] = kk;
            const CallArgs& ca = a.c[i];
            if (ca.splits <= 1) {
                cb.gbeg[x][i] = 0;
                continue;
            }
            const int groups = ca.qtiles * ca.bh;
            const int glo = std::min(groups, fg(jlo, ca.block_begin, ca.splits));
            const int ghi = std::min(groups, fg(jhi, ca.block_begin, ca.splits));
            cb.gbeg[x][i] = glo;
            kk += (ghi - glo) * block_m / 16;
        }
        for (int i = n_live; i <= kMaxCalls; ++i) cb.kbeg[x][i] = kk;
        per_xcd = std::max(per_xcd, kk);
    }
    cb.per_xcd = std::max(1, per_xcd);
    cb.main_blocks = blocks;
    cb.groups0 = a.c[0].qtiles * a.c[0].bh;
    return out_f32 ? launch_combine<float>(cb, stream) : launch_combine<f16>(cb, stream);
}

hipError_t launch_convert(const void* const* src, void* const* dst, const unsigned* end8, int count,
                          hipStream_t stream) {
    ConvArgs cv{};
    for (int i = 0; i < count; ++i) {
        cv.src[i] = reinterpret_cast<const float*>(src[i]);
        cv.dst[i] = reinterpret_cast<f16*>(dst[i]);
        cv.end8[i] = end8[i];
    }
    cv.count = count;
    hipLaunchKernelGGL(convert_f32_f16_kernel, dim3((end8[count - 1] + 255) / 256), dim3(256), 0, stream, cv);
    return hipGetLastError();
}

}  // namespace mha_hd64
