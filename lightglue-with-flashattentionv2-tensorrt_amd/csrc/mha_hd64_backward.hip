// mha_hd64_backward.hip — gradient of O = softmax(Q·Kᵀ/8)·V, head_dim = 64, for gfx950 (MI355X, CDNA4).
//
// Per (batch, head), with S = Q·Kᵀ/8 and P the row softmax of S:
//   D_i = Σ_d dO_id·O_id,  dV = Pᵀ·dO,  dP = dO·Vᵀ,  dS = P∘(dP − D),  dQ = dS·K/8,  dK = dSᵀ·Q/8.
// The forward kernels save no row statistics, so the backward recomputes the row log-sum-exp L_i and
// P = exp2(S·log2e − L). No floating-point atomics: every output element has one owner, and where
// several workgroups hold partial sums (the column kernel's query split) they are added in split
// order by a reduce kernel, so results are bitwise reproducible.
//
// Two kernels of 2 wave64s, both on v_mfma_f32_32x32x16_f16 with fp16 operands and fp32 accumulators:
//  * rows (64 queries per workgroup, one query per lane, all keys streamed twice through LDS):
//    pass one  Sᵀ = K·Qᵀ, online max and sum -> L;  D from dO and O as the block is loaded;
//    pass two  Sᵀ again, P, dPᵀ = V·dOᵀ, dSᵀ = Pᵀ∘(dPᵀ − D), and dQᵀ += Kᵀ·dSᵀ: the dSᵀ accumulators
//    rounded to fp16 are directly the B operand, Kᵀ comes from LDS by ds_read_b64_tr_b16 (the forward's
//    P·V scheme with K in V's place). Writes dQ, and L and D ([B, H, nq] fp32) to the workspace.
//  * cols (64 keys per workgroup, one key per lane, K and V fragments resident in registers, blocks of
//    64 queries streamed through LDS with their L and D): S = Q·Kᵀ and dP = dO·Vᵀ put the key on the
//    lane and 16 queries in registers, so P and dS rounded to fp16 are the B operands of
//    dVᵀ += dOᵀ·P and dKᵀ += Qᵀ·dS; dOᵀ and Qᵀ are transposing LDS reads. With a query split the
//    partial dK / dV go to the workspace in fp32 and bwd_reduce adds them in split order.
// P and dS are rounded to fp16 once, where they become MFMA operands; everything else stays fp32 until
// the final store. Tails are masked in the kernels: loads past nq / nkv return zeros (buffer
// descriptors sized per head), masked keys and queries get P = 0 exactly, and no row past the end is stored.
//
// The grouped form (mha_hd64_backward_grouped_lens) runs up to 4 calls of different shapes, each item with
// its own query and key count, as one rows, one cols and at most one reduce launch. The tile code is the
// same (the bodies below are templates over LENS); what differs is where a workgroup gets its shape from:
// it finds its call by comparing its index with the calls' prefix sums in the kernel arguments, reads its
// item's two counts by scalar loads, ends its buffer descriptors at the counts (padding is never read),
// streams only the tiles below them, and writes zeros into the padded rows of dQ, dK and dV. A workgroup
// with nothing below its counts writes its zeros and leaves before the first barrier.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "mha_hd64_device.h"
#include "mha_hd64_internal.h"

namespace mha_hd64 {
namespace {

constexpr int kBwdThreads = 128;          // 2 waves of 32 queries (rows) or 32 keys (cols)
constexpr float kMaskedScore = -1e30f;    // a masked key's score in the running max (finite: no inf - inf)
constexpr int kRowStage = 3 * kTileBytes;         // rows kernel: K by rows, K for transposing reads, V by rows
constexpr int kColStage = 4 * kTileBytes + 512;   // cols kernel: Q and dO, both images each, then L and D

struct BwdArgs {
    const f16* q;
    const f16* k;
    const f16* v;
    const f16* o;
    const f16* dout;
    void* dq;
    void* dk;
    void* dv;
    float* lse;    // [bh][nq] row log-sum-exp of S·log2e (log2 units)
    float* delta;  // [bh][nq] D
    float* part;   // [2 (dK, dV)][splits][bh][nkv][64] fp32 partials (splits > 1 only)
    int nq;
    int nkv;
    int bh;
    int qtiles;           // 64-row query blocks per (batch, head)
    int ktiles;           // 64-key blocks per (batch, head)
    int splits;           // query splits of the cols kernel
    int tiles_per_split;  // query blocks per split
};

// One launch of n <= kGroupCalls calls: call i owns workgroups [end[i - 1], end[i]) of the rows and of the cols
// grid (end[i] of an unused slot = the grid, so that no workgroup selects it). q_lens / kv_lens: per call a
// device table of `batch` int32 counts, or null (every row); heads turns a workgroup's batch·head into its item.
struct BwdGroupArgs {
    BwdArgs c[kGroupCalls];
    const int* q_lens[kGroupCalls];
    const int* kv_lens[kGroupCalls];
    int heads[kGroupCalls];
    int rows_end[kGroupCalls];
    int cols_end[kGroupCalls];
};
// A workgroup's call and its index inside it, from the prefix sums (wave-uniform compares and selects).
__device__ __forceinline__ int group_call(const int (&end)[kGroupCalls], int block, int& local) {
    const int ci = (block >= end[0]) + (block >= end[1]) + (block >= end[2]);
    local = block - (ci == 0 ? 0 : ci == 1 ? end[0] : ci == 2 ? end[1] : end[2]);
    return ci;
}
template <typename T>
__device__ __forceinline__ T group_pick(const T (&tab)[kGroupCalls], int ci) {
    T x = tab[0];
#pragma unroll
    for (int i = 1; i < kGroupCalls; ++i)
        if (ci == i) x = tab[i];
    return x;
}
// An item's count: one scalar load (a uniform address in the constant address space), clamped into [1, n];
// a null table means n.
__device__ __forceinline__ int group_len(const int* tab, int item, int n) {
    typedef const __attribute__((address_space(4))) int* const_int_t;
    int len = n;
    if (tab) len = ((const_int_t)(uintptr_t)tab)[__builtin_amdgcn_readfirstlane(item)];
    return min(max(len, 1), n);
}

__device__ __forceinline__ float xhalf_sum(float x) {
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ f32x16 mfma32(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}
// row of accumulator register i of a 32x32 tile on half-wave hh
__device__ __forceinline__ int acc_row(int i, int hh) { return 8 * (i >> 2) + 4 * hh + (i & 3); }

// One 64-row x 64-dim fp16 tile, 4 chunks of 16 B per thread: rows row0.. of the head behind rs
// (rows past its end read as zeros), written as the row image (k_off) and / or the image the
// transposing reads take (v_off).
__device__ __forceinline__ void tile_issue(Raw8<f16> (&st)[4], __amdgpu_buffer_rsrc_t rs, int row0, int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
        bload8(st[i], rs, (unsigned)((row0 + 16 * i + (tid >> 3)) * kHeadDim + (tid & 7) * 8) * 2u, 0);
}
template <bool ROWS, bool TRANS>
__device__ __forceinline__ void tile_write(lds_char* lds, unsigned rows_at, unsigned trans_at, const Raw8<f16> (&st)[4],
                                           int tid) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = 16 * i + (tid >> 3), ch = tid & 7;
        if constexpr (ROWS) lds_write16(lds, rows_at + k_off(row, ch), st[i].x);
        if constexpr (TRANS) lds_write16(lds, trans_at + v_off(row, ch), st[i].x);
    }
}
// Byte offsets of this lane's transposing reads inside a v_off tile (the forward's Vᵀ scheme): lane
// (16-lane group g, index 4qq + pp) supplies row 4hh + qq, columns 16(g&1) + 4pp of dims 0..31
// (half 0) or 32..63 (half 1).
__device__ __forceinline__ void trans_lane(int lane, unsigned& at0, unsigned& at1) {
    const int hh = lane >> 5, g16 = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const int vb = (qq >> 1) & 1;
    const int base = 128 * (4 * hh + qq) + 16 * (2 * (g16 & 1) + (pp >> 1)) + 8 * (pp & 1);
    at0 = base + 64 * vb;
    at1 = base + 64 * (1 - vb);
}
// A operand Xᵀ[dim][16 rows] of k-step (j, ss) of a 64-row v_off tile: the rows in the order the
// 32x32 accumulator registers 8ss..8ss+7 of row half j hold them.
__device__ __forceinline__ f16x8 trans_frag(lds_char* lds, unsigned at, int j, int ss) {
    const unsigned rowc = 128u * (32 * j + 16 * ss);
    return cat8(tr_read(lds, at + rowc), tr_read(lds, at + rowc + 8 * 128));
}
// registers 8ss..8ss+7 of an accumulator, rounded to fp16: the B operand of k-step ss
__device__ __forceinline__ f16x8 acc_frag(const f32x16& c, int ss) {
    f16x8 b;
#pragma unroll
    for (int e = 0; e < 8; ++e) b[e] = (f16)c[8 * ss + e];
    return b;
}

// One query row of dQᵀ (dims 0..31 in dq0, 32..63 in dq1, times 1/8): this lane's 4-dim groups.
template <typename TOut>
__device__ __forceinline__ void store_dq_row(TOut* dst, const f32x16& dq0, const f32x16& dq1) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        store4<TOut>(dst + 8 * g, dq0[4 * g] * 0.125f, dq0[4 * g + 1] * 0.125f, dq0[4 * g + 2] * 0.125f,
                     dq0[4 * g + 3] * 0.125f);
        store4<TOut>(dst + 32 + 8 * g, dq1[4 * g] * 0.125f, dq1[4 * g + 1] * 0.125f, dq1[4 * g + 2] * 0.125f,
                     dq1[4 * g + 3] * 0.125f);
    }
}

// ----------------------------------------------------------------------------------------
// rows: grid = qtiles * bh. Lane = query (r = lane & 31 of the wave's 32), registers = keys.
// `block` is the workgroup's index inside its call. LENS: the item has q_len real query rows and kv_len
// real keys inside its [a.nq] / [a.nkv] slabs (the strides stay the padded sizes).
// ----------------------------------------------------------------------------------------
template <typename TOut, bool LENS>
__device__ __forceinline__ void bwd_rows_body(const BwdArgs& a, int block, int q_len, int kv_len, lds_char* lds) {
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = block / a.qtiles, qtile = block % a.qtiles;
    const int nq = LENS ? q_len : a.nq, nkv = LENS ? kv_len : a.nkv;
    const size_t qo = (size_t)bh * a.nq * kHeadDim, ko = (size_t)bh * a.nkv * kHeadDim;
    const auto q_rs = make_rsrc(a.q + qo, (unsigned)nq * 128u), o_rs = make_rsrc(a.o + qo, (unsigned)nq * 128u);
    const auto do_rs = make_rsrc(a.dout + qo, (unsigned)nq * 128u);
    const auto k_rs = make_rsrc(a.k + ko, (unsigned)nkv * 128u), v_rs = make_rsrc(a.v + ko, (unsigned)nkv * 128u);
    const int q = qtile * 64 + 32 * wave + r;
    TOut* const dq_row = reinterpret_cast<TOut*>(a.dq) + qo + (size_t)q * kHeadDim + 4 * hh;
    if constexpr (LENS) {
        if (qtile * 64 >= nq) {  // (workgroup-uniform) a block of padding: zeros, and no barrier was reached
            if (q < a.nq) store_dq_row<TOut>(dq_row, f32x16{}, f32x16{});
            return;
        }
    }

    // Q and dO fragments (B operands: lane holds dims 16s + 8hh .. +7 of its query) and D
    f16x8 qf[4], dof[4];
    float dpart = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const unsigned at = (unsigned)(q * kHeadDim + 16 * s + 8 * hh) * 2u;
        Raw8<f16> tq, td, to;
        bload8(tq, q_rs, at, 0);
        bload8(td, do_rs, at, 0);
        bload8(to, o_rs, at, 0);
        qf[s] = tq.x;
        dof[s] = td.x;
#pragma unroll
        for (int e = 0; e < 8; ++e) dpart += (float)td.x[e] * (float)to.x[e];
    }
    const float D = xhalf_sum(dpart);

    unsigned tr0, tr1;
    trans_lane(lane, tr0, tr1);
    const int nt = LENS ? (nkv + 63) / 64 : a.ktiles;

    // Sᵀ·log2e/8 of the tile at `base`, masked keys at kMaskedScore; ok bit 16h + i = key of register i, half h, is real
    auto scores = [&](unsigned base, int t, f32x16 (&x)[2], unsigned& ok) {
        x[0] = f32x16{};
        x[1] = f32x16{};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const unsigned ka = base + k_off(r, 2 * s + hh);
            x[0] = mfma32(lds_read16(lds, ka), qf[s], x[0]);
            x[1] = mfma32(lds_read16(lds, ka + 32 * 128), qf[s], x[1]);
        }
        ok = 0xffffffffu;
        const bool tail = (t + 1) * 64 > nkv;  // wave-uniform: the last tile only
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                x[h][i] *= kScaleLog2;
                if (tail && t * 64 + 32 * h + acc_row(i, hh) >= nkv) {
                    x[h][i] = kMaskedScore;
                    ok &= ~(1u << (16 * h + i));
                }
            }
    };
    // The K/V stream: tile t+1 is loaded into registers while tile t is computed from LDS, and written
    // to the other stage after it; one barrier per tile. FULL also stages V and K's transposable image.
    auto stream = [&](auto full_c, auto&& body) {
        constexpr bool FULL = decltype(full_c)::value;
        Raw8<f16> kst[4], vst[4];
        auto issue = [&](int t) {
            tile_issue(kst, k_rs, t * 64, tid);
            if constexpr (FULL) tile_issue(vst, v_rs, t * 64, tid);
        };
        auto write = [&](unsigned base) {
            tile_write<true, FULL>(lds, base, base + kTileBytes, kst, tid);
            if constexpr (FULL) tile_write<true, false>(lds, base + 2 * kTileBytes, 0, vst, tid);
        };
        issue(0);
        write(0);
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const unsigned base = (t & 1) * kRowStage;
            issue(t + 1);  // (past the last tile: zeros into a stage nobody reads)
            body(t, base);
            write(kRowStage - base);
            __syncthreads();
        }
    };

    // pass one: the row log-sum-exp (log2 units)
    float m = kMaskedScore, l = 0.f;
    stream(std::false_type{}, [&](int t, unsigned base) {
        f32x16 x[2];
        unsigned ok;
        scores(base, t, x, ok);
        const float m_new = fmaxf(m, tree_max(x[0], x[1]));
        l *= __builtin_amdgcn_exp2f(m - m_new);
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = __builtin_amdgcn_exp2f(x[h][i] - m_new);
                l += ((ok >> (16 * h + i)) & 1u) ? p : 0.f;
            }
        m = m_new;
    });
    const float M = xhalf_max(m);  // (a half-wave that saw masked keys only has l = 0)
    const float L = M + __builtin_amdgcn_logf(xhalf_sum(l * __builtin_amdgcn_exp2f(m - M)));

    // pass two: dQᵀ (dims 0..31 and 32..63, query on the lane)
    f32x16 dq0 = {}, dq1 = {};
    stream(std::true_type{}, [&](int t, unsigned base) {
        f32x16 x[2], dp[2] = {f32x16{}, f32x16{}};
        unsigned ok;
        scores(base, t, x, ok);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const unsigned va = base + 2 * kTileBytes + k_off(r, 2 * s + hh);
            dp[0] = mfma32(lds_read16(lds, va), dof[s], dp[0]);
            dp[1] = mfma32(lds_read16(lds, va + 32 * 128), dof[s], dp[1]);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                float p = __builtin_amdgcn_exp2f(x[h][i] - L);
                p = ((ok >> (16 * h + i)) & 1u) ? p : 0.f;
                x[h][i] = p * (dp[h][i] - D);
            }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const f16x8 ds = acc_frag(x[j], ss);
                dq0 = mfma32(trans_frag(lds, base + kTileBytes + tr0, j, ss), ds, dq0);
                dq1 = mfma32(trans_frag(lds, base + kTileBytes + tr1, j, ss), ds, dq1);
            }
    });

    if (q < nq) {
        store_dq_row<TOut>(dq_row, dq0, dq1);
        if (hh == 0) {
            a.lse[(size_t)bh * a.nq + q] = L;
            a.delta[(size_t)bh * a.nq + q] = D;
        }
    } else if (LENS && q < a.nq) {  // padded rows of a live block (their L and D are never read)
        store_dq_row<TOut>(dq_row, f32x16{}, f32x16{});
    }
}

template <typename TOut>
__global__ __launch_bounds__(kBwdThreads) void mha_hd64_bwd_rows_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kRowStage];
    bwd_rows_body<TOut, false>(a, blockIdx.x, 0, 0, (lds_char*)smem);
}
// grouped: grid = the calls' qtiles * bh, one after the other
template <typename TOut>
__global__ __launch_bounds__(kBwdThreads) void mha_hd64_bwd_rows_group_kernel(BwdGroupArgs g) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kRowStage];
    int block;
    const int ci = group_call(g.rows_end, blockIdx.x, block);
    const BwdArgs a = group_pick(g.c, ci);
    const int item = (block / a.qtiles) / group_pick(g.heads, ci);
    bwd_rows_body<TOut, true>(a, block, group_len(group_pick(g.q_lens, ci), item, a.nq),
                              group_len(group_pick(g.kv_lens, ci), item, a.nkv), (lds_char*)smem);
}

// ----------------------------------------------------------------------------------------
// cols: grid = splits * ktiles * bh. Lane = key (r of the wave's 32), registers = queries.
// `block` and LENS as for the rows. LENS: a split's query blocks end at ceil(q_len / 64); a workgroup whose
// keys or query blocks all lie past the counts runs no tile and stores zeros (outputs or partials alike, so
// the reduce needs no condition), and so do the padded keys of a live block.
// ----------------------------------------------------------------------------------------
template <typename TOut, bool LENS>
__device__ __forceinline__ void bwd_cols_body(const BwdArgs& a, int block, int q_len, int kv_len, lds_char* lds) {
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = block % a.splits, ktile = (block / a.splits) % a.ktiles;
    const int bh = block / (a.splits * a.ktiles);
    const int nq = LENS ? q_len : a.nq, nkv = LENS ? kv_len : a.nkv;
    const size_t qo = (size_t)bh * a.nq * kHeadDim, ko = (size_t)bh * a.nkv * kHeadDim;
    const auto q_rs = make_rsrc(a.q + qo, (unsigned)nq * 128u), do_rs = make_rsrc(a.dout + qo, (unsigned)nq * 128u);
    const auto k_rs = make_rsrc(a.k + ko, (unsigned)nkv * 128u), v_rs = make_rsrc(a.v + ko, (unsigned)nkv * 128u);
    const auto l_rs = make_rsrc(a.lse + (size_t)bh * a.nq, (unsigned)nq * 4u);
    const auto d_rs = make_rsrc(a.delta + (size_t)bh * a.nq, (unsigned)nq * 4u);
    const int key = ktile * 64 + 32 * wave + r;
    const bool key_ok = key < nkv;

    // K and V fragments, resident (B operands: lane holds dims 16s + 8hh .. +7 of its key)
    f16x8 kf[4], vf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const unsigned at = (unsigned)(key * kHeadDim + 16 * s + 8 * hh) * 2u;
        Raw8<f16> tk, tv;
        bload8(tk, k_rs, at, 0);
        bload8(tv, v_rs, at, 0);
        kf[s] = tk.x;
        vf[s] = tv.x;
    }
    unsigned tr0, tr1;
    trans_lane(lane, tr0, tr1);

    // The Q/dO stream, as the rows kernel's: stage = Q rows, Qᵀ image, dO rows, dOᵀ image, L[64], D[64]
    const int t_begin = split * a.tiles_per_split;
    const int t_end = min(LENS ? (nq + 63) / 64 : a.qtiles, t_begin + a.tiles_per_split);
    const bool live = !LENS || (ktile * 64 < nkv && t_begin < t_end);  // (workgroup-uniform)
    Raw8<f16> qst[4], dst[4];
    unsigned ldst;
    auto issue = [&](int t) {
        tile_issue(qst, q_rs, t * 64, tid);
        tile_issue(dst, do_rs, t * 64, tid);
        ldst = __builtin_amdgcn_raw_buffer_load_b32(wave == 0 ? l_rs : d_rs, (unsigned)(t * 64 + (tid & 63)) * 4u, 0, 0);
    };
    auto write = [&](unsigned base) {
        tile_write<true, true>(lds, base, base + kTileBytes, qst, tid);
        tile_write<true, true>(lds, base + 2 * kTileBytes, base + 3 * kTileBytes, dst, tid);
        *(__attribute__((address_space(3))) unsigned*)(lds + base + 4 * kTileBytes + 4 * tid) = ldst;
    };
    f32x16 dk0 = {}, dk1 = {}, dv0 = {}, dv1 = {};  // dKᵀ, dVᵀ: dims 0..31 and 32..63, key on the lane
    if (live) {
        issue(t_begin);
        write(0);
        __syncthreads();
    }
    for (int t = t_begin; live && t < t_end; ++t) {
        const unsigned base = ((t - t_begin) & 1) * kColStage;
        issue(t + 1);  // (past the last block: a stage nobody reads)
        const bool qtail = (t + 1) * 64 > nq;  // wave-uniform: the last block only
#pragma unroll
        for (int j = 0; j < 2; ++j) {  // 32 queries each
            f32x16 s = {}, dp = {};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const unsigned at = base + k_off(32 * j + r, 2 * c + hh);
                s = mfma32(lds_read16(lds, at), kf[c], s);
                dp = mfma32(lds_read16(lds, at + 2 * kTileBytes), vf[c], dp);
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
                const unsigned at = base + 4 * kTileBytes + 4 * (32 * j + 8 * g + 4 * hh);
                const f32x4 L4 = *(lds_f32x4*)(lds + at), D4 = *(lds_f32x4*)(lds + at + 256);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = 4 * g + e;
                    float p = __builtin_amdgcn_exp2f(s[i] * kScaleLog2 - L4[e]);
                    p = key_ok ? p : 0.f;
                    if (qtail && t * 64 + 32 * j + acc_row(i, hh) >= nq) p = 0.f;
                    s[i] = p;
                    dp[i] = p * (dp[i] - D4[e]);
                }
            }
#pragma unroll
            for (int ss = 0; ss < 2; ++ss) {
                const f16x8 pb = acc_frag(s, ss), dsb = acc_frag(dp, ss);
                dv0 = mfma32(trans_frag(lds, base + 3 * kTileBytes + tr0, j, ss), pb, dv0);
                dv1 = mfma32(trans_frag(lds, base + 3 * kTileBytes + tr1, j, ss), pb, dv1);
                dk0 = mfma32(trans_frag(lds, base + kTileBytes + tr0, j, ss), dsb, dk0);
                dk1 = mfma32(trans_frag(lds, base + kTileBytes + tr1, j, ss), dsb, dk1);
            }
        }
        write(kColStage - base);
        __syncthreads();
    }

    if constexpr (LENS) {
        if (key >= a.nkv) return;
        if (!key_ok) dk0 = dk1 = dv0 = dv1 = f32x16{};  // a padded key: zeros, whatever the tiles gave
    } else {
        if (!key_ok) return;
    }
    auto store_row = [&](auto* out, size_t at) {
        typedef std::remove_pointer_t<decltype(out)> T;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            store4<T>(out + at + 8 * g, dk0[4 * g], dk0[4 * g + 1], dk0[4 * g + 2], dk0[4 * g + 3]);
            store4<T>(out + at + 32 + 8 * g, dk1[4 * g], dk1[4 * g + 1], dk1[4 * g + 2], dk1[4 * g + 3]);
        }
    };
    dk0 *= 0.125f;
    dk1 *= 0.125f;
    const size_t row = ko + (size_t)key * kHeadDim + 4 * hh;
    if (a.splits == 1) {
        store_row(reinterpret_cast<TOut*>(a.dk), row);
        dk0 = dv0;
        dk1 = dv1;
        store_row(reinterpret_cast<TOut*>(a.dv), row);
    } else {
        const size_t tensor = (size_t)a.bh * a.nkv * kHeadDim;
        store_row(a.part + (size_t)split * tensor, row);
        dk0 = dv0;
        dk1 = dv1;
        store_row(a.part + ((size_t)a.splits + split) * tensor, row);
    }
}

template <typename TOut>
__global__ __launch_bounds__(kBwdThreads) void mha_hd64_bwd_cols_kernel(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kColStage];
    bwd_cols_body<TOut, false>(a, blockIdx.x, 0, 0, (lds_char*)smem);
}
// grouped: grid = the calls' splits * ktiles * bh, one after the other
template <typename TOut>
__global__ __launch_bounds__(kBwdThreads) void mha_hd64_bwd_cols_group_kernel(BwdGroupArgs g) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kColStage];
    int block;
    const int ci = group_call(g.cols_end, blockIdx.x, block);
    const BwdArgs a = group_pick(g.c, ci);
    const int item = (block / (a.splits * a.ktiles)) / group_pick(g.heads, ci);
    bwd_cols_body<TOut, true>(a, block, group_len(group_pick(g.q_lens, ci), item, a.nq),
                              group_len(group_pick(g.kv_lens, ci), item, a.nkv), (lds_char*)smem);
}

// Partial dK / dV of the query splits, added in split order: grid = (blocks of 256 x 4 elements, 2).
template <typename TOut>
__device__ __forceinline__ void bwd_reduce_body(const BwdArgs& a) {
    const size_t tensor = (size_t)a.bh * a.nkv * kHeadDim;
    const size_t at = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (at >= tensor) return;
    const float* p = a.part + (size_t)blockIdx.y * a.splits * tensor + at;
    f32x4 acc = *reinterpret_cast<const f32x4*>(p);
    for (int s = 1; s < a.splits; ++s) acc += *reinterpret_cast<const f32x4*>(p + (size_t)s * tensor);
    store4<TOut>(reinterpret_cast<TOut*>(blockIdx.y ? a.dv : a.dk) + at, acc[0], acc[1], acc[2], acc[3]);
}
template <typename TOut>
__global__ __launch_bounds__(256) void mha_hd64_bwd_reduce_kernel(BwdArgs a) {
    bwd_reduce_body<TOut>(a);
}
// grouped: grid = (the largest splitting call's blocks, 2, calls); a call without a split wrote its outputs itself
template <typename TOut>
__global__ __launch_bounds__(256) void mha_hd64_bwd_reduce_group_kernel(BwdGroupArgs g) {
    const BwdArgs a = group_pick(g.c, (int)blockIdx.z);
    if (a.splits > 1) bwd_reduce_body<TOut>(a);
}

template <typename TOut>
hipError_t launch_kernels(const BwdArgs& a, hipStream_t stream) {
    hipLaunchKernelGGL(mha_hd64_bwd_rows_kernel<TOut>, dim3((unsigned)(a.qtiles * a.bh)), dim3(kBwdThreads), 0, stream, a);
    hipLaunchKernelGGL(mha_hd64_bwd_cols_kernel<TOut>, dim3((unsigned)(a.splits * a.ktiles * a.bh)), dim3(kBwdThreads), 0,
                       stream, a);
    if (a.splits > 1) {
        const size_t quads = (size_t)a.bh * a.nkv * kHeadDim / 4;
        hipLaunchKernelGGL(mha_hd64_bwd_reduce_kernel<TOut>, dim3((unsigned)((quads + 255) / 256), 2), dim3(256), 0, stream,
                           a);
    }
    return hipGetLastError();
}

}  // namespace

// The cols kernel's query split: while the launch's 64-key workgroups (`groups`: this call's, or all of its
// chunk's in a grouped launch, since the calls of a launch fill the chip together) number at most half of
// `target`, the query blocks are dealt to up to 16 splits so that about `target` workgroups run. A lone call
// aims at 256 (one per CU); a grouped launch at 512, which measured faster there (2 calls of P x 4 x 1024 x 1024:
// P = 1 4 splits 69.7 us against 72.4 with 2, P = 2 2 splits 77.0 against 82.8 with 1, P = 4 1 split 98.9 against
// 111.4 with 2; profiles/attention_backward/INDEX.md).
static BwdPlan plan_call(int batch, int heads, int nq, int nkv, InType in, long long groups, int target) {
    BwdPlan p{};
    const long long bh = (long long)batch * heads;
    p.qtiles = (nq + 63) / 64;
    p.ktiles = (nkv + 63) / 64;
    int splits = groups > target / 2 ? 1 : (int)std::min<long long>(std::min(p.qtiles, 16), target / groups);
    // measurement hook (tools/attention_backward_ab.py): MHA_HD64_BWD_SPLITS=n forces up to n splits
    if (const char* e = std::getenv("MHA_HD64_BWD_SPLITS"))
        if (std::atoi(e) >= 1) splits = std::min(std::min(p.qtiles, 16), std::atoi(e));
    p.tiles_per_split = (p.qtiles + splits - 1) / splits;
    p.splits = (p.qtiles + p.tiles_per_split - 1) / p.tiles_per_split;
    p.stats_bytes = align256((size_t)bh * nq * 4);
    const size_t qb = align256((size_t)bh * nq * kHeadDim * 2), kb = align256((size_t)bh * nkv * kHeadDim * 2);
    p.copy_bytes = in == InType::F32 ? 3 * qb + 2 * kb : 0;  // fp16 copies of Q, O, dO and K, V
    p.part_bytes = p.splits > 1 ? (size_t)2 * p.splits * bh * nkv * kHeadDim * 4 : 0;
    p.ws_bytes = 2 * p.stats_bytes + p.copy_bytes + p.part_bytes;
    return p;
}

BwdPlan plan_backward(int batch, int heads, int nq, int nkv, InType in) {
    return plan_call(batch, heads, nq, nkv, in, (long long)batch * heads * ((nkv + 63) / 64), 256);
}

BwdGroupPlan plan_backward_group(const BwdCall* calls, int n) {
    BwdGroupPlan g{};
    long long groups = 0;
    for (int i = 0; i < n; ++i) groups += (long long)calls[i].batch * calls[i].heads * ((calls[i].nkv + 63) / 64);
    for (int i = 0; i < n; ++i) {
        g.call[i] = plan_call(calls[i].batch, calls[i].heads, calls[i].nq, calls[i].nkv, InType::F16, groups, 512);
        g.ws_offset[i] = g.ws_bytes;
        g.ws_bytes += g.call[i].ws_bytes;
    }
    return g;
}

hipError_t launch_backward_group(const BwdCall* calls, const int* const* q_lens, const int* const* kv_lens, int n,
                                 void* workspace, hipStream_t stream) {
    const BwdGroupPlan gp = plan_backward_group(calls, n);
    BwdGroupArgs g{};
    int rows = 0, cols = 0;
    size_t reduce_quads = 0;
    for (int i = 0; i < n; ++i) {
        const BwdCall& c = calls[i];
        const BwdPlan& p = gp.call[i];
        char* ws = reinterpret_cast<char*>(workspace) + gp.ws_offset[i];
        BwdArgs& a = g.c[i];
        a.q = reinterpret_cast<const f16*>(c.q);
        a.k = reinterpret_cast<const f16*>(c.k);
        a.v = reinterpret_cast<const f16*>(c.v);
        a.o = reinterpret_cast<const f16*>(c.o);
        a.dout = reinterpret_cast<const f16*>(c.dout);
        a.dq = c.dq;
        a.dk = c.dk;
        a.dv = c.dv;
        a.lse = reinterpret_cast<float*>(ws);
        a.delta = reinterpret_cast<float*>(ws + p.stats_bytes);
        a.part = reinterpret_cast<float*>(ws + 2 * p.stats_bytes);
        a.nq = c.nq;
        a.nkv = c.nkv;
        a.bh = c.batch * c.heads;
        a.qtiles = p.qtiles;
        a.ktiles = p.ktiles;
        a.splits = p.splits;
        a.tiles_per_split = p.tiles_per_split;
        g.q_lens[i] = q_lens ? q_lens[i] : nullptr;
        g.kv_lens[i] = kv_lens ? kv_lens[i] : nullptr;
        g.heads[i] = c.heads;
        rows += a.qtiles * a.bh;
        cols += a.splits * a.ktiles * a.bh;
        g.rows_end[i] = rows;
        g.cols_end[i] = cols;
        if (p.splits > 1) reduce_quads = std::max(reduce_quads, (size_t)a.bh * a.nkv * kHeadDim / 4);
    }
    for (int i = n; i < kGroupCalls; ++i) {  // unused slots: a copy of the last call that no workgroup selects
        g.c[i] = g.c[n - 1];
        g.heads[i] = g.heads[n - 1];
        g.rows_end[i] = rows;
        g.cols_end[i] = cols;
    }
    hipLaunchKernelGGL(mha_hd64_bwd_rows_group_kernel<f16>, dim3((unsigned)rows), dim3(kBwdThreads), 0, stream, g);
    hipLaunchKernelGGL(mha_hd64_bwd_cols_group_kernel<f16>, dim3((unsigned)cols), dim3(kBwdThreads), 0, stream, g);
    if (reduce_quads)
        hipLaunchKernelGGL(mha_hd64_bwd_reduce_group_kernel<f16>, dim3((unsigned)((reduce_quads + 255) / 256), 2, (unsigned)n),
                           dim3(256), 0, stream, g);
    return hipGetLastError();
}

hipError_t launch_backward(const BwdCall& c, InType in, void* workspace, hipStream_t stream) {
    const BwdPlan p = plan_backward(c.batch, c.heads, c.nq, c.nkv, in);
    char* ws = reinterpret_cast<char*>(workspace);
    BwdArgs a{};
    a.lse = reinterpret_cast<float*>(ws);
    a.delta = reinterpret_cast<float*>(ws + p.stats_bytes);
    ws += 2 * p.stats_bytes;
    const void* t16[5] = {c.q, c.o, c.dout, c.k, c.v};
    if (in == InType::F32) {  // the forward's Float boundary: one convert launch, then the fp16 kernels
        const size_t bh = (size_t)c.batch * c.heads;
        const void* src[5] = {c.q, c.o, c.dout, c.k, c.v};
        void* dst[5];
        unsigned end8[5], total8 = 0;
        for (int i = 0; i < 5; ++i) {
            const size_t elems = bh * (i < 3 ? c.nq : c.nkv) * kHeadDim;
            total8 += (unsigned)(elems / 8);
            end8[i] = total8;
            dst[i] = ws;
            t16[i] = ws;
            ws += align256(elems * 2);
        }
        const hipError_t e = launch_convert(src, dst, end8, 5, stream);
        if (e != hipSuccess) return e;
    }
    a.q = reinterpret_cast<const f16*>(t16[0]);
    a.o = reinterpret_cast<const f16*>(t16[1]);
    a.dout = reinterpret_cast<const f16*>(t16[2]);
    a.k = reinterpret_cast<const f16*>(t16[3]);
    a.v = reinterpret_cast<const f16*>(t16[4]);
    a.part = reinterpret_cast<float*>(ws);
    a.dq = c.dq;
    a.dk = c.dk;
    a.dv = c.dv;
    a.nq = c.nq;
    a.nkv = c.nkv;
    a.bh = c.batch * c.heads;
    a.qtiles = p.qtiles;
    a.ktiles = p.ktiles;
    a.splits = p.splits;
    a.tiles_per_split = p.tiles_per_split;
    return in == InType::F32 ? launch_kernels<float>(a, stream) : launch_kernels<f16>(a, stream);
}

}  // namespace mha_hd64
