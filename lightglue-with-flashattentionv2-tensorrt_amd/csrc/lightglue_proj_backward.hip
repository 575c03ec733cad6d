// lightglue_proj_backward.hip — the backward of the matcher's fused projections on gfx950
// (include/lightglue_glue.h: lg_proj_backward): lg_linear_qkv_rotary (Wqkv + rotary, head-major q/k/v per image),
// lg_linear_split2 (to_qk | to_v, head-major) and the head's lg_linear with [W_final / scale ; w_match ; 0].
// fp16 operands, fp32 accumulators, an fp16 data gradient and fp32 parameter gradients; 4 heads of 64, k = 256.
//
// For Y [M, n] = X [M, 256] Wᵀ + b leaving through a layout epilogue, G [M, n] = dL/dY in W's row order is never
// handed in: it is gathered by kind through the forward's epilogue in reverse,
//   QKV    (n = 768): q0 k0 v0 q1 k1 v1 head-major [pairs, 4, ni, 64]; the q and k parts through the transposed rotary,
//                     (g0, g1) -> (g0 c0 + g1 s1, g1 c1 - g0 s0) in fp32, rounded once; the v part copied
//   SPLIT2 (n = 512): a0 a1 b0 b1 head-major, G = [merge(da) | merge(db)]
//   PLAIN  (n = n_store): one fp32 gradient [M, ld], G = fp16 of its first n_store columns
// and  dx = fp16(G W (+ dx_add)),  dW = Gᵀ X,  db = column sums of G  (fp32 sums; dx one rounding).
// Launches:
//  1. proj_bw_pack_kernel: Wᵀ re-laid per call as the rows kernel's fragment streams (8 wave streams of 1-KiB
//     pieces: piece s of wave w, lane l = W[16 s + 8 (l / 32) ..][32 w + l % 32]), so that the product contracts over
//     n with one contiguous KiB per load, straight into registers. (The other route, staging W tiles in LDS and
//     reading them transposed, would pass all of W, up to 384 KiB, through every workgroup's LDS beside the G tile's
//     own reads, which by instruction counts already match the MFMA time (an estimate); the pack is one small launch.)
//  2. proj_bw_rows_kernel, the hot path: a workgroup of 8 waves owns 64 whole rows. Its prologue gathers the rows' G
//     tile into LDS (row pitch 2 n + 16 B: 16-B reads of 16 rows conflict-free), 128 B per (row, head), the un-rotate
//     in registers. With parameter gradients wanted the tile leaves once by 16-B row-major stores to the workspace
//     G [M, n], and its column sums are MFMAs against ones through transposing reads (one fp32 partial per column
//     and workgroup). dx is taken swapped, D[channel][row] by v_mfma_f32_32x32x16_f16 with the packed Wᵀ as A and
//     the tile as B: wave w owns channels 32 w .. 32 w + 31 of all 64 rows. The fp32 result passes through the
//     tile's LDS so that dx_add is added in fp32 and dx leaves in 16-B stores. X is not staged: dx does not need it.
//  3. proj_bw_weight_kernel: dW in 128 x 128 output tiles (n / 128 x 2) times a split of the rows
//     (proj_bw_splits). Both operands contract over rows: 32-row tiles of G and X, register-staged into two LDS
//     stages (64-B blocks XOR (row & 3)), both read by ds_read_b64_tr_b16. fp32 partials per split.
//  4. proj_bw_reduce_kernel: the weight partials in split order; proj_bw_colreduce_kernel: the column partials in
//     workgroup order, in fp64, 16 threads a column.
// No atomics, no exchange between workgroups inside a launch: a call is bitwise reproducible and capturable.
// (rows_gemm's stream loop, col_sums and the weight kernel's tile loop have lg_ffn_backward's shape; they are
// written out here and not shared, so that lightglue_ffn_backward.hip compiles to the code it had.)
#include "lightglue_device.h"
#include "mha_hd64_device.h"

#include <algorithm>
#include <cstdlib>

namespace {

typedef __attribute__((address_space(3))) f32x4 lds_f32x4;

constexpr int kPbRows = 64;             // rows of a rows-kernel workgroup
constexpr int kPbK = 256;               // the projections' input width
constexpr int kPbOutP = 4 * kPbK + 16;  // the fp32 output rows' pitch in the tile's place (1040 B)

struct PbArgs {
    LinArgs p;         // a = x, w, cosv, sinv, m, n, heads, n0, n1
    const void* g[6];  // the kind's gradients (null: zeros)
    int gld;           // PLAIN: the fp32 gradient's row pitch in elements
    const f16* dx_add;
    f16* dx;
    float *dw, *db;
    f16* pack;       // workspace: Wᵀ's streams [8][n / 16][64 lanes][8]
    f16* G;          // [M, n]
    float* colpart;  // [nwg][n]
    float* wpart;    // [S][n * 256]
    int S, nwg, full;
};

__global__ __launch_bounds__(256) void proj_bw_pack_kernel(PbArgs q) {
    const int f = blockIdx.x * 256 + threadIdx.x;  // fragment: piece f / 64, lane f % 64
    const int steps = q.p.n / 16;
    if (f >= 8 * steps * 64) return;
    const int piece = f >> 6, l = f & 63, w = piece / steps, s = piece - w * steps;
    const int n0 = 16 * s + 8 * (l >> 5), k = 32 * w + (l & 31);
    f16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = q.p.w[(size_t)(n0 + e) * kPbK + k];
    *reinterpret_cast<f16x8*>(q.pack + (size_t)f * 8) = v;
}

// the sums over the tile's 64 rows of its channels cbase .. cbase + 31 (MFMA against ones, the tile read
// transposed) -> dst[0..31], written by lanes 0 and 32
__device__ __forceinline__ void col_sums(lds_char* lds, int pitch, int cbase, float* dst, int lane) {
    const int hh = lane >> 5, qq = (lane & 15) >> 2, pp = lane & 3, gh = (lane >> 4) & 1;
    const f16 one = (f16)1.f;
    const f16x8 ones = {one, one, one, one, one, one, one, one};
    f32x16 a = f32x16{};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const unsigned at = (16 * ks + 8 * hh + qq) * pitch + (cbase + 16 * gh + 4 * pp) * 2;
        const f16x8 af = mha_hd64::cat8(mha_hd64::tr_read(lds, at), mha_hd64::tr_read(lds, at + 4 * pitch));
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, ones, a, 0, 0, 0);
    }
    if ((lane & 31) == 0) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
            *reinterpret_cast<f32x4*>(dst + 8 * gq + 4 * hh) = f32x4{a[4 * gq], a[4 * gq + 1], a[4 * gq + 2], a[4 * gq + 3]};
    }
}

__device__ __forceinline__ f16x8 ld8(const void* base, size_t at) {
    return base ? *reinterpret_cast<const f16x8*>((const f16*)base + at) : f16x8{};
}

// (cos, sin: 8-B aligned as the forward takes them, so two 8-B loads)
__device__ __forceinline__ f16x8 ld8_halves(const f16* p) {
    return mha_hd64::cat8(*reinterpret_cast<const f16x4*>(p), *reinterpret_cast<const f16x4*>(p + 4));
}

// One 16-B unit of G: row `row` (< M), channels 8 un .. 8 un + 7, gathered through the kind's epilogue in reverse.
// fetch: the loads; finish: the un-rotate (QKV's q and k parts).
struct PbUnit {
    f16x8 v, c, s;
};
template <int KIND>
__device__ __forceinline__ PbUnit pb_fetch(const PbArgs& q, int row, int un) {
    PbUnit t{};
    if constexpr (KIND == LG_PROJ_PLAIN) {
        if (!q.g[0]) return t;
        const float* src = (const float*)q.g[0] + (size_t)row * q.gld + 8 * un;
        const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
        t.v = f16x8{(f16)a[0], (f16)a[1], (f16)a[2], (f16)a[3], (f16)b[0], (f16)b[1], (f16)b[2], (f16)b[3]};
    } else {
        const int col = 8 * un, part = col >> 8, h = (col >> 6) & 3, d = col & 63;
        const LinRow lr = lin_row(q.p, row, h);
        if constexpr (KIND == LG_PROJ_QKV) {  // q0 k0 v0 q1 k1 v1
            const void* const src = lr.first ? (part == 0 ? q.g[0] : part == 1 ? q.g[1] : q.g[2])
                                             : (part == 0 ? q.g[3] : part == 1 ? q.g[4] : q.g[5]);
            t.v = ld8(src, lr.off + d);
            if (part < 2) {
                t.c = ld8_halves(q.p.cosv + (size_t)row * kD + d);
                t.s = ld8_halves(q.p.sinv + (size_t)row * kD + d);
            }
        } else {  // a0 a1 b0 b1
            const void* const src = lr.first ? (part == 0 ? q.g[0] : q.g[2]) : (part == 0 ? q.g[1] : q.g[3]);
            t.v = ld8(src, lr.off + d);
        }
    }
    return t;
}
template <int KIND>
__device__ __forceinline__ f16x8 pb_finish(const PbUnit& t, int un) {
    if (KIND != LG_PROJ_QKV || un >= 64) return t.v;
    f16x8 o;  // the forward's (x0 c0 - x1 s0, x1 c1 + x0 s1), transposed; the products are exact in fp32
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        const float g0 = (float)t.v[e], g1 = (float)t.v[e + 1];
        o[e] = (f16)(g0 * (float)t.c[e] + g1 * (float)t.s[e + 1]);
        o[e + 1] = (f16)(g1 * (float)t.c[e + 1] - g0 * (float)t.s[e]);
    }
    return o;
}

template <int KIND>
__global__ __launch_bounds__(512) void proj_bw_rows_kernel(PbArgs q) {
    constexpr int NMAX = KIND == LG_PROJ_QKV ? 768 : 512;
    __shared__ __attribute__((aligned(16))) char smem[kPbRows * (2 * NMAX + 16)];
    static_assert(sizeof(smem) >= kPbRows * kPbOutP && sizeof(smem) <= 160 * 1024, "LDS");
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = q.p.m, row0 = blockIdx.x * kPbRows;
    const int n = KIND == LG_PROJ_PLAIN ? q.p.n : NMAX, U = n / 8, pitch = 2 * n + 16;

    // the G tile, four units a lane in flight; rows past M: zeros (so dx's unused rows and every sum's share are zero)
    for (int u0 = tid; u0 < kPbRows * U; u0 += 4 * 512) {
        PbUnit t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = u0 + 512 * i, row = u / U;
            t[i] = PbUnit{};
            if (u < kPbRows * U && row0 + row < M) t[i] = pb_fetch<KIND>(q, row0 + row, u - row * U);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = u0 + 512 * i, row = u / U, un = u - row * U;
            if (u < kPbRows * U) *(lds_f16x8*)(lds + row * pitch + un * 16) = pb_finish<KIND>(t[i], un);
        }
    }
    __syncthreads();
    if (q.full) {  // G's rows that exist, row-major, 16 B a lane; the column sums
        for (int u = tid; u < kPbRows * U; u += 512) {
            const int row = u / U, un = u - row * U;
            if (row0 + row < M)
                *reinterpret_cast<f16x8*>(q.G + (size_t)(row0 + row) * n + un * 8) = *(lds_f16x8*)(lds + row * pitch + un * 16);
        }
        for (int cb = wave; cb < n / 32; cb += 8) col_sums(lds, pitch, 32 * cb, q.colpart + (size_t)blockIdx.x * n + 32 * cb, lane);
    }

    // dx = G W, swapped: acc[rb][4 gq + e] = channel 32 wave + 8 gq + 4 hh + e of row 32 rb + r. The stream runs one
    // chunk of 4 k16 steps ahead in registers (n / 16 is a multiple of 4).
    constexpr int CH = 4;
    const int chunks = n / (16 * CH);
    const f16x8* const src = reinterpret_cast<const f16x8*>(q.pack) + (size_t)wave * (n / 16) * 64 + lane;
    const unsigned boff = r * pitch + 16 * hh;
    f32x16 acc[2] = {f32x16{}, f32x16{}};
    f16x8 cur[CH], nxt[CH];
#pragma unroll
    for (int i = 0; i < CH; ++i) cur[i] = src[i * 64];
    for (int c = 0; c < chunks; ++c) {
        const int cn = min(c + 1, chunks - 1);  // (the last chunk is loaded again and not used)
#pragma unroll
        for (int i = 0; i < CH; ++i) nxt[i] = src[(cn * CH + i) * 64];
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            const unsigned at = boff + 32 * (c * CH + s);
            const f16x8 b0 = *(lds_f16x8*)(lds + at), b1 = *(lds_f16x8*)(lds + at + 32 * pitch);
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[s], b0, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[s], b1, acc[1], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < CH; ++i) cur[i] = nxt[i];
    }
    __syncthreads();  // (the tile is read: its place takes the fp32 rows)
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
            *(lds_f32x4*)(lds + (32 * rb + r) * kPbOutP + (32 * wave + 8 * gq + 4 * hh) * 4) =
                f32x4{acc[rb][4 * gq], acc[rb][4 * gq + 1], acc[rb][4 * gq + 2], acc[rb][4 * gq + 3]};
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = i * 512 + tid, row = u >> 5, un = u & 31;
        if (row0 + row >= M) continue;
        const size_t at = (size_t)(row0 + row) * kPbK + un * 8;
        const f32x4 a = *(lds_f32x4*)(lds + row * kPbOutP + un * 32), b = *(lds_f32x4*)(lds + row * kPbOutP + un * 32 + 16);
        const f16x8 ad = ld8(q.dx_add, at);
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (f16)(a[e] + (float)ad[e]), o[4 + e] = (f16)(b[e] + (float)ad[4 + e]);
        *reinterpret_cast<f16x8*>(q.dx + at) = o;
    }
}

// ---- the weight gradient ----
constexpr int kWgOp = 32 * 256;      // one operand's tile: [32 rows][128 channels], 64-B blocks XOR (row & 3)
constexpr int kWgStage = 2 * kWgOp;  // G then X

__global__ __launch_bounds__(256) void proj_bw_weight_kernel(PbArgs q) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kWgStage];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int qq = (lane & 15) >> 2, pp = lane & 3, gh = (lane >> 4) & 1;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wi = wave >> 1, wj = wave & 1;
    const int M = q.p.m, n = q.p.n, sp = blockIdx.y;
    const int ti = blockIdx.x >> 1, tj = blockIdx.x & 1;  // dW rows 128 ti .., columns 128 tj ..
    const int stages = (M + 31) / 32, tps = (stages + q.S - 1) / q.S;
    const int t_begin = sp * tps, t_end = min(t_begin + tps, stages);

    f16x8 xs[2], ys[2];
    auto issue = [&](int t) {  // rows past M and G's channels past n: zeros
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = i * 256 + tid, row = 32 * t + (u >> 4), un = u & 15;
            xs[i] = ys[i] = f16x8{};
            if (row < M) {
                if (128 * ti + 8 * un < n) xs[i] = *reinterpret_cast<const f16x8*>(q.G + (size_t)row * n + 128 * ti + 8 * un);
                ys[i] = *reinterpret_cast<const f16x8*>(q.p.a + (size_t)row * kPbK + 128 * tj + 8 * un);
            }
        }
    };
    auto write = [&](unsigned base) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = i * 256 + tid, row = u >> 4, un = u & 15;
            const unsigned off = row * 256 + ((((un >> 2) ^ (row & 3)) << 6) | ((un & 3) << 4));
            *(lds_f16x8*)(lds + base + off) = xs[i];
            *(lds_f16x8*)(lds + base + kWgOp + off) = ys[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = f32x16{};
    issue(t_begin);
    write(0);
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
        const unsigned base = ((t - t_begin) & 1) * kWgStage;
        issue(t + 1);  // (past t_end - 1: written and never read)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int rq = 16 * ks + 8 * hh + qq;
            f16x8 xa[2], yb[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const unsigned ax = base + rq * 256 + (((2 * wi + b) ^ qq) << 6) + 32 * gh + 8 * pp;
                const unsigned ay = base + kWgOp + rq * 256 + (((2 * wj + b) ^ qq) << 6) + 32 * gh + 8 * pp;
                xa[b] = mha_hd64::cat8(mha_hd64::tr_read(lds, ax), mha_hd64::tr_read(lds, ax + 4 * 256));
                yb[b] = mha_hd64::cat8(mha_hd64::tr_read(lds, ay), mha_hd64::tr_read(lds, ay + 4 * 256));
            }
#pragma unroll
            for (int bi = 0; bi < 2; ++bi)
#pragma unroll
                for (int bj = 0; bj < 2; ++bj)
                    acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(xa[bi], yb[bj], acc[bi][bj], 0, 0, 0);
        }
        write(kWgStage - base);
        __syncthreads();
    }
    // acc[bi][bj][4 gq + e] = dW[128 ti + 64 wi + 32 bi + 8 gq + 4 hh + e][128 tj + 64 wj + 32 bj + r]
    float* const dst = q.wpart + (size_t)sp * n * kPbK;
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = 128 * ti + 64 * wi + 32 * bi + 8 * (i >> 2) + 4 * hh + (i & 3);
                if (row < n) dst[(size_t)row * kPbK + 128 * tj + 64 * wj + 32 * bj + r] = acc[bi][bj][i];
            }
}

// dW: the weight partials added in split order
__global__ __launch_bounds__(256) void proj_bw_reduce_kernel(PbArgs q) {
    const int at = blockIdx.x * 256 + threadIdx.x, wn = q.p.n * kPbK;  // (wn is a multiple of 256)
    float s = 0.f;
    for (int i = 0; i < q.S; ++i) s += q.wpart[(size_t)i * wn + at];
    q.dw[at] = s;
}
// db: a block owns 16 columns; 16 threads a column add a 16th of the workgroups' partials each, in workgroup order
// and in fp64 (up to 16,384 workgroups: their order costs no bits), then the 16 in order
__global__ __launch_bounds__(256) void proj_bw_colreduce_kernel(PbArgs q) {
    __shared__ double part[16][16];
    const int col = threadIdx.x & 15, chunk = threadIdx.x >> 4, c = blockIdx.x * 16 + col;
    const int per = (q.nwg + 15) / 16, end = min((chunk + 1) * per, q.nwg);
    double s = 0.0;
    for (int i = chunk * per; i < end; ++i) s += (double)q.colpart[(size_t)i * q.p.n + c];
    part[chunk][col] = s;
    __syncthreads();
    if (chunk != 0) return;
    for (int j = 1; j < 16; ++j) s += part[j][col];
    q.db[c] = (float)s;
}

size_t pb_up256(size_t x) { return (x + 255) / 256 * 256; }
int pb_width(int32_t kind, int32_t n_store) {
    return kind == LG_PROJ_QKV ? 768 : kind == LG_PROJ_SPLIT2 ? 512 : kind == LG_PROJ_PLAIN ? n_store : 0;
}
// The weight kernel's split of the rows: one split per 256 rows, 32 at the most (its 2 n / 128 = 12 / 8 / 6 output
// tiles are few, so the split fills the chip: 32 splits are 384 / 256 / 192 workgroups of 4 waves on 256 CUs).
// Measured (profiles/proj_backward/ab.jsonl, the whole QKV call, us): S = 1 / 4 / 8 / 16 / 20 / 32 / 40 / 64 at 2,048
// rows 73 / 48 / 48 / 51 / 51 / 55 / 55 / 65, at 32,768 rows 656 / 221 / 149 / 115 / 109 / 105 / 105 / 114; S = 1 / 2 /
// 4 / 10 / 20 at 320 rows 42 / 40 / 40 / 42 / 50, at 640 rows 48 / 43 / 42 / 44 / 51. The other two kinds order the
// candidates alike. The rule takes the table's best, or within 1 us of it, at each of the four sizes.
int proj_bw_splits(int32_t m) {
    int S = std::min(32, (m + 255) / 256);
    // measurement hook (tools/proj_backward_ab.py): LG_PROJ_BACKWARD_SPLITS=s forces s splits
    if (const char* e = std::getenv("LG_PROJ_BACKWARD_SPLITS"))
        if (std::atoi(e) >= 1) S = std::min(std::atoi(e), 64);
    return S;
}

}  // namespace

extern "C" {

// the packed stream, G [m, n] fp16, the column partials, the split partials
size_t lg_proj_backward_workspace(int32_t kind, int32_t m_rows, int32_t n_store) {
    const int n = pb_width(kind, n_store);
    if (m_rows <= 0 || n <= 0 || n > 768 || n % 64) return 0;
    const size_t m = (size_t)m_rows, nwg = (m + kPbRows - 1) / kPbRows;
    return pb_up256((size_t)n * kPbK * 2) + pb_up256(m * n * 2) + pb_up256(nwg * n * 4) +
           (size_t)proj_bw_splits(m_rows) * n * kPbK * 4;
}

int32_t lg_proj_backward(int32_t kind, const void* x, const void* w, const void* cosv, const void* sinv,
                         const void* const* grads, int32_t grad_ld, int32_t n_store, int32_t heads, int32_t n0,
                         int32_t n1, int32_t pairs, const void* dx_add, void* dx, float* dw, float* db, void* workspace,
                         hipStream_t stream) {
    const char* const who = "lg_proj_backward";
    const int ng = kind == LG_PROJ_QKV ? 6 : kind == LG_PROJ_SPLIT2 ? 4 : kind == LG_PROJ_PLAIN ? 1 : 0;
    const long long m = (long long)pairs * ((long long)n0 + n1);
    if (ng == 0 || heads != 4 || n0 < 0 || n1 < 0 || pairs < 0 || m > (1 << 20) || !aligned16(dw) || !aligned16(db) ||
        (kind == LG_PROJ_PLAIN && (n_store < 64 || n_store > 512 || n_store % 64 || grad_ld < n_store || grad_ld % 4)) ||
        (kind == LG_PROJ_QKV && (!cosv || !sinv || !aligned8(cosv) || !aligned8(sinv))) || !grads)
        return bad(who);
    // dx's bytes may meet none of x's or a gradient's; dx_add may be dx itself, not a shifted overlap
    const size_t dxb = (size_t)m * kPbK * 2;
    auto meets = [&](const void* q, size_t bytes) {
        const uintptr_t a = (uintptr_t)dx, b = (uintptr_t)q;
        return q && a < b + bytes && b < a + dxb;
    };
    for (int i = 0; i < ng; ++i) {
        const int ni = kind == LG_PROJ_QKV ? (i < 3 ? n0 : n1) : (i & 1) ? n1 : n0;
        const size_t bytes = kind == LG_PROJ_PLAIN ? (size_t)m * grad_ld * 4 : (size_t)pairs * 4 * ni * kD * 2;
        if (!aligned16(grads[i]) || (m > 0 && meets(grads[i], bytes))) return bad(who);
    }
    if (!aligned16(x) || !aligned16(w) || !aligned16(dx) || !aligned16(dx_add) || !aligned16(workspace) ||
        (m > 0 && (!x || !w || !dx || !workspace || meets(x, dxb) || (dx_add != dx && meets(dx_add, dxb)))))
        return bad(who);
    if (m == 0) return MHA_HD64_STATUS_SUCCESS;  // no rows: nothing is launched (dw and db are the caller's to clear)
    PbArgs q{};
    q.p.a = (const f16*)x, q.p.w = (const f16*)w, q.p.cosv = (const f16*)cosv, q.p.sinv = (const f16*)sinv;
    q.p.m = (int)m, q.p.n = pb_width(kind, n_store), q.p.k = kPbK, q.p.heads = heads, q.p.n0 = n0, q.p.n1 = n1;
    for (int i = 0; i < ng; ++i) q.g[i] = grads[i];
    q.gld = grad_ld, q.dx_add = (const f16*)dx_add, q.dx = (f16*)dx, q.dw = dw, q.db = db;
    q.full = dw || db, q.S = proj_bw_splits((int32_t)m), q.nwg = (int)((m + kPbRows - 1) / kPbRows);
    const size_t n = (size_t)q.p.n;
    char* ws = (char*)workspace;
    q.pack = (f16*)ws, ws += pb_up256(n * kPbK * 2);
    q.G = (f16*)ws, ws += pb_up256((size_t)m * n * 2);
    q.colpart = (float*)ws, ws += pb_up256((size_t)q.nwg * n * 4);
    q.wpart = (float*)ws;
    hipLaunchKernelGGL(proj_bw_pack_kernel, dim3((unsigned)(n * 32 + 255) / 256), dim3(256), 0, stream, q);
    if (kind == LG_PROJ_QKV) hipLaunchKernelGGL(proj_bw_rows_kernel<LG_PROJ_QKV>, dim3(q.nwg), dim3(512), 0, stream, q);
    else if (kind == LG_PROJ_SPLIT2) hipLaunchKernelGGL(proj_bw_rows_kernel<LG_PROJ_SPLIT2>, dim3(q.nwg), dim3(512), 0, stream, q);
    else hipLaunchKernelGGL(proj_bw_rows_kernel<LG_PROJ_PLAIN>, dim3(q.nwg), dim3(512), 0, stream, q);
    if (dw) {
        hipLaunchKernelGGL(proj_bw_weight_kernel, dim3(2 * (unsigned)((n + 127) / 128), q.S), dim3(256), 0, stream, q);
        hipLaunchKernelGGL(proj_bw_reduce_kernel, dim3((unsigned)n), dim3(256), 0, stream, q);
    }
    if (db) hipLaunchKernelGGL(proj_bw_colreduce_kernel, dim3((unsigned)n / 16), dim3(256), 0, stream, q);
    return launched(who);
}

}  // extern "C"
