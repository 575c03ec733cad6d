// lightglue_ffn_backward.hip — the backward of the matcher's FFN block on gfx950
// (include/lightglue_glue.h: lg_ffn_backward). fp16 operands, fp32 accumulators, fp16 data gradients and
// fp32 parameter gradients. The forward (lg_linear_cat_ffn) saves nothing: everything is recomputed.
//
// With c = [x | merge_heads(ctx0, ctx1)] [M, 512]:
//   a = fp16(c W1ᵀ + b1);  mu, rstd over a (fp32, the variance from the squares about the mean);
//   n = (a - mu) rstd;  u = n gamma + beta;  g = fp16(GELU(u))
//   dg = dy W2;  du = dg (Phi(u) + u phi(u));  dn = du gamma;  da = rstd (dn - mean(dn) - n mean(dn n))
//   dc = da W1;  dx = fp16(dy + dc[:, :256]);  dctx = fp16(dc[:, 256:]) head-major
//   dW2 = dyᵀ g, db2 = sum dy, dW1 = daᵀ c, db1 = sum da, dgamma = sum du n, dbeta = sum du
// Rounding points: a and g to fp16 as the forward rounds them; da to fp16 where it becomes the operand of dc
// and dW1 (db1 sums the same rounded da); du and du n to fp16 where they become the operands of the column
// sums dbeta and dgamma; dx in one rounding of the fp32 sum; everything else fp32 (the erf is gelu_as's).
// Launches:
//  1. ffn_bw_pack_kernel: W1, W2ᵀ and W1ᵀ re-laid per call as the rows kernel's three fragment streams
//     (8 wave streams of 1-KiB pieces, piece (k16 step s, block b) lane l = B[64 w + 32 b + l % 32][16 s + 8 (l / 32) ..]),
//     so that all three products read their weights alike: one contiguous KiB per load, straight into registers.
//  2. ffn_bw_rows_kernel, the hot path: a workgroup of 8 waves owns 64 whole rows. Every product is taken
//     swapped, D[channel][row] by v_mfma_f32_32x32x16_f16 with the weights as A and the rows' tile in LDS as B,
//     so a lane owns one row (two: 32 rb + lane % 32) and wave w the channels 64 w .. 64 w + 63 of every product:
//     LayerNorm statistics and the two row means are in-lane sums, a cross-half swap and 8 partials in LDS.
//     One 65-KiB tile T (row pitch 1040 B: 16-B reads of 32 rows conflict-free by halves) holds in turn c, g,
//     du, du n, da and the output rows; the dy tile stays throughout. g and da leave T by 16-B row-major stores
//     for the weight kernel; dx and the head-major dctx leave it the same way. The column sums (dbeta, dgamma,
//     db1, db2) are MFMAs of the tile against ones through transposing reads (ds_read_b64_tr_b16): one fp32
//     partial per column and workgroup.
//  3. ffn_bw_weight_kernel: dW1 and dW2 in 128 x 128 output tiles (16 + 8) times a split of the rows
//     (ffn_bw_splits). Both operands contract over rows: 32-row tiles of da | c (gathered as the forward
//     gathers it) or dy | g, register-staged into two LDS stages (64-B blocks XOR (row & 3)), both read by
//     ds_read_b64_tr_b16. fp32 partials per split.
//  4. ffn_bw_reduce_kernel: the weight partials in split order; ffn_bw_colreduce_kernel: the column partials in
//     workgroup order, in fp64, 16 threads a column.
// No atomics, no exchange between workgroups inside a launch: a call is bitwise reproducible.
#include "lightglue_ffn_device.h"
#include "mha_hd64_device.h"

#include <algorithm>
#include <cstdlib>

namespace {

typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
typedef __attribute__((address_space(3))) f16x4 lds_f16x4;
typedef __attribute__((address_space(3))) float lds_f32;

constexpr int kBwRows = 64;                     // rows of a rows-kernel workgroup
constexpr int kTP = 2 * kLnN + 16;              // T's row pitch (1040 B)
constexpr int kDP = 2 * kFfnOut + 16;           // the dy tile's (528 B)
constexpr int kT = 0;
constexpr int kDyT = kBwRows * kTP;
constexpr int kRed = kDyT + kBwRows * kDP;      // row partials [2 slots][64 rows][8 waves] fp32
constexpr int kBwLds = kRed + 2 * kBwRows * 8 * 4;
static_assert(kBwLds <= 160 * 1024, "LDS");
// the packed streams (fp16 elements): W1 (a), W2ᵀ (dg), W1ᵀ (dc)
constexpr int kPkW1 = 0, kPkW2t = kLnN * kLnN, kPkW1t = kPkW2t + kFfnOut * kLnN, kPkEnd = kPkW1t + kLnN * kLnN;
// a workgroup's column partials: dbeta, dgamma, db1 [512], db2 [256]
constexpr int kColBeta = 0, kColGamma = kLnN, kColB1 = 2 * kLnN, kColB2 = 3 * kLnN, kColN = 3 * kLnN + kFfnOut;
constexpr int kW1N = kLnN * kLnN, kWN = kW1N + kFfnOut * kLnN;  // a split's weight partials: dW1 then dW2

struct FbArgs {
    LinArgs p;  // x, ctx0, ctx1, m, k = 512, heads, n0, n1
    const f16 *w1, *w2, *b1, *gamma, *beta, *dy;
    float eps;
    f16 *dx, *dctx0, *dctx1;
    float *dw1, *db1, *dgamma, *dbeta, *dw2, *db2;
    f16* pack;       // workspace: the three streams
    f16* g;          // [M, 512]
    f16* da;         // [M, 512]
    float* colpart;  // [nwg][kColN]
    float* wpart;    // [S][kWN]
    int S, nwg, full;
};

__global__ __launch_bounds__(256) void ffn_bw_pack_kernel(FbArgs q) {
    const int f = blockIdx.x * 256 + threadIdx.x;  // fragment: piece f / 64, lane f % 64
    if (f >= kPkEnd / 8) return;
    const int piece = f >> 6, l = f & 63;
    const int which = piece < 512 ? 0 : piece < 768 ? 1 : 2;
    const int pi = piece - (which == 0 ? 0 : which == 1 ? 512 : 768), ks = which == 1 ? 16 : 32;
    const int w = pi / (2 * ks), s = (pi >> 1) % ks, b = pi & 1;
    const int n = 64 * w + 32 * b + (l & 31), k0 = 16 * s + 8 * (l >> 5);
    f16x8 v;
    if (which == 0) {
        v = *reinterpret_cast<const f16x8*>(q.w1 + (size_t)n * kLnN + k0);
    } else {
        const f16* src = which == 1 ? q.w2 : q.w1;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = src[(size_t)(k0 + e) * kLnN + n];
    }
    *reinterpret_cast<f16x8*>(q.pack + (size_t)f * 8) = v;
}

// Phi(x) + x phi(x) with gelu_as's erf: t = Phi(-|x|) = (y / 2) e^{-x^2 / 2}
__device__ __forceinline__ float gelu_grad_as(float x) {
    const float ax = fabsf(x);
    const float r = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752f, ax, 1.f));
    float p = fmaf(0.5f * 1.061405429f, r, 0.5f * -1.453152027f);
    p = fmaf(p, r, 0.5f * 1.421413741f);
    p = fmaf(p, r, 0.5f * -0.284496736f);
    p = fmaf(p, r, 0.5f * 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(x * x * (-0.5f * 1.4426950408889634f));
    const float t = p * r * e;
    return fmaf(x * 0.3989422804014327f, e, x >= 0.f ? 1.f - t : t);
}

// acc[b][rb] += B[64 w + 32 b ..][k] · tile[32 rb ..][k] over KS k16 steps: ws this wave's stream, the tile
// row-major in LDS; the stream runs 2 steps ahead in registers
template <int KS>
__device__ __forceinline__ void rows_gemm(f32x16 (&acc)[2][2], const f16* ws, lds_char* lds, unsigned tile, int pitch,
                                          int lane) {
    constexpr int CH = 2;
    const f16x8* const src = reinterpret_cast<const f16x8*>(ws) + lane;
    const unsigned boff = tile + (lane & 31) * pitch + 16 * (lane >> 5);
    f16x8 cur[2 * CH], nxt[2 * CH];
#pragma unroll
    for (int i = 0; i < 2 * CH; ++i) cur[i] = src[i * 64];
#pragma unroll
    for (int c = 0; c < KS / CH; ++c) {
        if (c + 1 < KS / CH) {
#pragma unroll
            for (int i = 0; i < 2 * CH; ++i) nxt[i] = src[((c + 1) * 2 * CH + i) * 64];
        }
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            const unsigned at = boff + 32 * (c * CH + s);
            const f16x8 b0 = *(lds_f16x8*)(lds + at), b1 = *(lds_f16x8*)(lds + at + 32 * pitch);
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * s], b0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * s + 1], b0, acc[1][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * s], b1, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(cur[2 * s + 1], b1, acc[1][1], 0, 0, 0);
        }
        if (c + 1 < KS / CH) {
#pragma unroll
            for (int i = 0; i < 2 * CH; ++i) cur[i] = nxt[i];
        }
        __builtin_amdgcn_sched_barrier(0);  // (the unrolled stream is not hoisted past its depth: registers)
    }
}

// s[rb]: this lane's share of a sum over the 512 channels of row 32 rb + lane % 32 -> the row's sum, the 8
// waves' partials added in wave order (one barrier; `slot` free since the barrier before last)
__device__ __forceinline__ void row_reduce(float (&s)[2], lds_char* lds, unsigned slot, int wave, int lane) {
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        s[rb] += __shfl_xor(s[rb], 32, 64);
        if (lane < 32) *(lds_f32*)(lds + slot + ((32 * rb + lane) * 8 + wave) * 4) = s[rb];
    }
    __syncthreads();
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const unsigned at = slot + (32 * rb + (lane & 31)) * 32;
        const f32x4 a = *(lds_f32x4*)(lds + at), c = *(lds_f32x4*)(lds + at + 16);
        s[rb] = ((a[0] + a[1]) + (a[2] + a[3])) + ((c[0] + c[1]) + (c[2] + c[3]));
    }
}

// the sums over the tile's 64 rows of its channels cbase .. cbase + 31 (MFMA against ones, the tile read
// transposed) -> dst[0..31], written by lanes 0 and 32
__device__ __forceinline__ void col_sums(lds_char* lds, unsigned tile, int pitch, int cbase, float* dst, int lane) {
    const int hh = lane >> 5, qq = (lane & 15) >> 2, pp = lane & 3, gh = (lane >> 4) & 1;
    const f16 one = (f16)1.f;
    const f16x8 ones = {one, one, one, one, one, one, one, one};
    f32x16 a = f32x16{};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const unsigned at = tile + (16 * ks + 8 * hh + qq) * pitch + (cbase + 16 * gh + 4 * pp) * 2;
        const f16x8 af = mha_hd64::cat8(mha_hd64::tr_read(lds, at), mha_hd64::tr_read(lds, at + 4 * pitch));
        a = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, ones, a, 0, 0, 0);
    }
    if ((lane & 31) == 0) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
            *reinterpret_cast<f32x4*>(dst + 8 * gq + 4 * hh) = f32x4{a[4 * gq], a[4 * gq + 1], a[4 * gq + 2], a[4 * gq + 3]};
    }
}

__device__ __forceinline__ f16x4 ld4(const f16* p) { return *reinterpret_cast<const f16x4*>(p); }
// an opaque copy: what is computed from it is computed where it is used, not at entry and kept in registers
__device__ __forceinline__ int fresh(int v) {
    asm volatile("" : "+v"(v));
    return v;
}

__global__ __launch_bounds__(512) void ffn_bw_rows_kernel(FbArgs q) {
    __shared__ __attribute__((aligned(16))) char smem[kBwLds];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = q.p.m, row0 = blockIdx.x * kBwRows;
    float* const cpart = q.colpart + (size_t)blockIdx.x * kColN;

    // c and dy tiles; rows past M: c clamped (finite, unused), dy zero (so that du, da and every sum are zero)
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int u = i * 512 + tid, row = u >> 6, un = u & 63;
        *(lds_f16x8*)(lds + kT + row * kTP + un * 16) =
            *reinterpret_cast<const f16x8*>(a_src<true>(q.p, min(row0 + row, M - 1), un));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int u = i * 512 + tid, row = u >> 5, un = u & 31;
        f16x8 v = f16x8{};
        if (row0 + row < M) v = *reinterpret_cast<const f16x8*>(q.dy + (size_t)(row0 + row) * kFfnOut + un * 8);
        *(lds_f16x8*)(lds + kDyT + row * kDP + un * 16) = v;
    }
    __syncthreads();
    if (q.full) col_sums(lds, kDyT, kDP, 32 * wave, cpart + kColB2 + 32 * wave, lane);

    // a = fp16(c W1ᵀ + b1): acc[b][rb][4 gq + e] = channel 64 wave + 32 b + 8 gq + 4 hh + e of row 32 rb + r
    f32x16 acc[2][2];
    auto clear = [&]() {
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) acc[b][rb] = f32x16{};
    };
    auto chan = [&](int b, int gq) { return 64 * wave + 32 * b + 8 * gq + 4 * hh; };
    auto t_at = [&](int b, int gq, int rb) { return (unsigned)(kT + (32 * rb + r) * kTP + chan(b, gq) * 2); };
    clear();
    rows_gemm<32>(acc, q.pack + kPkW1 + (size_t)wave * (kLnN * 64), lds, kT, kTP, lane);

    f16x2 ap[2][2][8];  // a, packed
    float mean[2], rstd[2];
    {
        float s[2] = {0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f16x4 bb = ld4(q.b1 + chan(b, gq));
#pragma unroll
                for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const f16 a = lin_val(acc[b][rb][4 * gq + e], bb[e]);
                        ap[b][rb][2 * gq + (e >> 1)][e & 1] = a;
                        s[rb] += (float)a;
                    }
            }
        row_reduce(s, lds, kRed, wave, lane);  // (its barrier: every wave is past its reads of c)
        mean[0] = s[0] * (1.f / kLnN), mean[1] = s[1] * (1.f / kLnN);
        float v[2] = {0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb)
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float d = (float)ap[b][rb][i >> 1][i & 1] - mean[rb];
                    v[rb] = fmaf(d, d, v[rb]);
                }
        row_reduce(v, lds, kRed + kBwRows * 32, wave, lane);
        rstd[0] = 1.f / sqrtf(v[0] * (1.f / kLnN) + q.eps), rstd[1] = 1.f / sqrtf(v[1] * (1.f / kLnN) + q.eps);
    }
    auto n_of = [&](int b, int rb, int i) { return ((float)ap[b][rb][i >> 1][i & 1] - mean[rb]) * rstd[rb]; };
    // T's rows that exist -> dst [M, 512] row-major, 16 B a lane
    auto t_out = [&](f16* dst) {
        const int td = fresh(tid);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int u = i * 512 + td, row = u >> 6, un = u & 63;
            if (row0 + row < M)
                *reinterpret_cast<f16x8*>(dst + (size_t)(row0 + row) * kLnN + un * 8) = *(lds_f16x8*)(lds + kT + row * kTP + un * 16);
        }
    };

    if (q.full) {  // g = fp16(GELU(u)) through T to the workspace
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                const f16x4 ga = ld4(q.gamma + chan(b, gq)), be = ld4(q.beta + chan(b, gq));
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    f16x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (f16)gelu_as(fmaf(n_of(b, rb, 4 * gq + e), (float)ga[e], (float)be[e]));
                    *(lds_f16x4*)(lds + t_at(b, gq, rb)) = o;
                }
                __builtin_amdgcn_sched_barrier(0);  // (8 values at a time: registers)
            }
        __syncthreads();
        t_out(q.g);
    }

    // dg = dy W2, then du = dg GELU'(u) in its place
    clear();
    rows_gemm<16>(acc, q.pack + kPkW2t + (size_t)wave * (kFfnOut * 64), lds, kDyT, kDP, lane);
    __syncthreads();  // (T's rows of g are out)
    float m1[2] = {0.f, 0.f}, m2[2] = {0.f, 0.f};
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const f16x4 ga = ld4(q.gamma + chan(b, gq)), be = ld4(q.beta + chan(b, gq));
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                f16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float n = n_of(b, rb, 4 * gq + e);
                    const float du = acc[b][rb][4 * gq + e] * gelu_grad_as(fmaf(n, (float)ga[e], (float)be[e]));
                    const float dn = du * (float)ga[e];
                    acc[b][rb][4 * gq + e] = du;
                    m1[rb] += dn;
                    m2[rb] = fmaf(dn, n, m2[rb]);
                    o[e] = (f16)du;
                }
                if (q.full) *(lds_f16x4*)(lds + t_at(b, gq, rb)) = o;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    row_reduce(m1, lds, kRed, wave, lane);  // (its barrier: T = du)
    if (q.full) {
        col_sums(lds, kT, kTP, 64 * wave, cpart + kColBeta + 64 * wave, lane);
        col_sums(lds, kT, kTP, 64 * wave + 32, cpart + kColBeta + 64 * wave + 32, lane);
    }
    row_reduce(m2, lds, kRed + kBwRows * 32, wave, lane);  // (its barrier: T read)
    if (q.full) {  // T = du n
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    f16x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (f16)(acc[b][rb][4 * gq + e] * n_of(b, rb, 4 * gq + e));
                    *(lds_f16x4*)(lds + t_at(b, gq, rb)) = o;
                }
        __syncthreads();
        col_sums(lds, kT, kTP, 64 * wave, cpart + kColGamma + 64 * wave, lane);
        col_sums(lds, kT, kTP, 64 * wave + 32, cpart + kColGamma + 64 * wave + 32, lane);
        __syncthreads();
    }
    // T = da = rstd (dn - mean(dn) - n mean(dn n))
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) m1[rb] *= 1.f / kLnN, m2[rb] *= 1.f / kLnN;
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const f16x4 ga = ld4(q.gamma + chan(b, gq));
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                f16x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dn = acc[b][rb][4 * gq + e] * (float)ga[e];
                    o[e] = (f16)(rstd[rb] * ((dn - m1[rb]) - n_of(b, rb, 4 * gq + e) * m2[rb]));
                }
                *(lds_f16x4*)(lds + t_at(b, gq, rb)) = o;
            }
        }
    __syncthreads();
    if (q.full) {
        col_sums(lds, kT, kTP, 64 * wave, cpart + kColB1 + 64 * wave, lane);
        col_sums(lds, kT, kTP, 64 * wave + 32, cpart + kColB1 + 64 * wave + 32, lane);
        t_out(q.da);
    }

    // dc = da W1: waves 0..3 own dx's channels, wave 4 + h head h of dctx
    clear();
    rows_gemm<32>(acc, q.pack + kPkW1t + (size_t)wave * (kLnN * 64), lds, kT, kTP, lane);
    __syncthreads();  // (T read)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int gq = 0; gq < 4; ++gq)
#pragma unroll
            for (int rb = 0; rb < 2; ++rb) {
                f16x4 o;
                if (wave < 4) {
                    const f16x4 d4 = *(lds_f16x4*)(lds + kDyT + (32 * rb + r) * kDP + chan(b, gq) * 2);
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (f16)((float)d4[e] + acc[b][rb][4 * gq + e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (f16)acc[b][rb][4 * gq + e];
                }
                *(lds_f16x4*)(lds + t_at(b, gq, rb)) = o;
            }
    __syncthreads();
    const int td = fresh(tid);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int u = i * 512 + td, row = u >> 6, un = u & 63;
        if (row0 + row >= M) continue;
        const f16x8 v = *(lds_f16x8*)(lds + kT + row * kTP + un * 16);
        if (un < 32) {
            *reinterpret_cast<f16x8*>(q.dx + (size_t)(row0 + row) * kFfnOut + un * 8) = v;
        } else {
            const int c2 = un * 8 - kFfnOut;
            const LinRow lr = lin_row(q.p, row0 + row, c2 / kD);
            *reinterpret_cast<f16x8*>((lr.first ? q.dctx0 : q.dctx1) + lr.off + c2 % kD) = v;
        }
    }
}

// ---- the weight gradients ----
constexpr int kWgOp = 32 * 256;       // one operand's tile: [32 rows][128 channels], 64-B blocks XOR (row & 3)
constexpr int kWgStage = 2 * kWgOp;   // X (da | dy) then Y (c | g)

__global__ __launch_bounds__(256) void ffn_bw_weight_kernel(FbArgs q) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kWgStage];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, hh = lane >> 5;
    const int qq = (lane & 15) >> 2, pp = lane & 3, gh = (lane >> 4) & 1;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wi = wave >> 1, wj = wave & 1;
    const int M = q.p.m, sp = blockIdx.y;
    const bool one = blockIdx.x < 16;  // dW1 = daᵀ c (16 tiles), else dW2 = dyᵀ g (8)
    const int tt = one ? (int)blockIdx.x : (int)blockIdx.x - 16, ti = tt >> 2, tj = tt & 3;
    const f16* const X = one ? q.da : q.dy;
    const int xld = one ? kLnN : kFfnOut;
    const int stages = (M + 31) / 32, tps = (stages + q.S - 1) / q.S;
    const int t_begin = sp * tps, t_end = min(t_begin + tps, stages);

    f16x8 xs[2], ys[2];
    auto issue = [&](int t) {  // rows past M: zeros in both operands
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = i * 256 + tid, row = 32 * t + (u >> 4), un = u & 15;
            xs[i] = ys[i] = f16x8{};
            if (row < M) {
                xs[i] = *reinterpret_cast<const f16x8*>(X + (size_t)row * xld + 128 * ti + 8 * un);
                ys[i] = *reinterpret_cast<const f16x8*>(one ? a_src<true>(q.p, row, 16 * tj + un)
                                                            : q.g + (size_t)row * kLnN + 128 * tj + 8 * un);
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
    float* const dst = q.wpart + (size_t)sp * kWN + (one ? 0 : kW1N);
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int row = 128 * ti + 64 * wi + 32 * bi + 8 * (i >> 2) + 4 * hh + (i & 3);
                dst[(size_t)row * kLnN + 128 * tj + 64 * wj + 32 * bj + r] = acc[bi][bj][i];
            }
}

// dW1 and dW2: the weight partials added in split order
__global__ __launch_bounds__(256) void ffn_bw_reduce_kernel(FbArgs q) {
    const int at = blockIdx.x * 256 + threadIdx.x;
    if (at >= kWN) return;
    float s = 0.f;
    for (int i = 0; i < q.S; ++i) s += q.wpart[(size_t)i * kWN + at];
    (at < kW1N ? q.dw1 + at : q.dw2 + (at - kW1N))[0] = s;
}
// dbeta, dgamma, db1, db2: a block owns 16 columns; 16 threads a column add a 16th of the workgroups' partials
// each, in workgroup order and in fp64 (up to 16,384 workgroups: their order costs no bits), then the 16 in order
__global__ __launch_bounds__(256) void ffn_bw_colreduce_kernel(FbArgs q) {
    __shared__ double part[16][16];
    const int col = threadIdx.x & 15, chunk = threadIdx.x >> 4, c = blockIdx.x * 16 + col;
    const int per = (q.nwg + 15) / 16, end = min((chunk + 1) * per, q.nwg);
    double s = 0.0;
    for (int i = chunk * per; i < end; ++i) s += (double)q.colpart[(size_t)i * kColN + c];
    part[chunk][col] = s;
    __syncthreads();
    if (chunk != 0) return;
    for (int j = 1; j < 16; ++j) s += part[j][col];
    float* const out = c < kColGamma ? q.dbeta + c
                       : c < kColB1  ? q.dgamma + (c - kColGamma)
                       : c < kColB2  ? q.db1 + (c - kColB1)
                                     : q.db2 + (c - kColB2);
    out[0] = (float)s;
}

size_t fb_up256(size_t x) { return (x + 255) / 256 * 256; }
// The weight kernel's split of the rows: its 24 output tiles alone up to 320 rows, 20 splits beyond (480
// workgroups of 4 waves, resident at once on the chip's 256 CUs; twenty partials of 1.5 MiB whatever M).
// Measured (profiles/ffn_backward/ab.jsonl, the whole call, us): S = 1 / 4 / 8 / 10 / 16 / 20 at 2,048 rows
// 109 / 74 / 70 / 70 / 71 / 73, at 32,768 rows 891 / 326 / 232 / 215 / 194 / 186; S = 1 / 2 / 4 / 10 / 20 at 320
// rows 64 / 61 / 62 / 68 / 74, at 640 rows 71 / 65 / 64 / 69 / 73. The two values are the table's best at its
// ends; between about 640 and a few thousand rows 2 to 10 splits are 3 to 8 us ahead of this rule.
int ffn_bw_splits(int32_t m) {
    int S = m <= 320 ? 1 : 20;
    // measurement hook (tools/ffn_backward_ab.py): LG_FFN_BACKWARD_SPLITS=s forces s splits
    if (const char* e = std::getenv("LG_FFN_BACKWARD_SPLITS"))
        if (std::atoi(e) >= 1) S = std::min(std::atoi(e), 32);
    return S;
}

}  // namespace

extern "C" {

// the three packed streams, g and da [m, 512] fp16, the column partials, the split partials
size_t lg_ffn_backward_workspace(int32_t m_rows) {
    if (m_rows <= 0) return 0;
    const size_t m = (size_t)m_rows, nwg = (m + kBwRows - 1) / kBwRows;
    return fb_up256((size_t)kPkEnd * 2) + 2 * fb_up256(m * kLnN * 2) + fb_up256(nwg * kColN * 4) +
           (size_t)ffn_bw_splits(m_rows) * kWN * 4;
}

int32_t lg_ffn_backward(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0, int32_t n1,
                        int32_t pairs, const void* w1, const void* b1, const void* gamma, const void* beta, float eps,
                        const void* w2, const void* dy, void* dx, void* dctx0, void* dctx1, float* dw1, float* db1,
                        float* dgamma, float* dbeta, float* dw2, float* db2, void* workspace, hipStream_t stream) {
    const char* const who = "lg_ffn_backward";
    const long long m = (long long)pairs * ((long long)n0 + n1);
    const int grads = !!dw1 + !!db1 + !!dgamma + !!dbeta + !!dw2 + !!db2;
    if (heads != 4 || n0 < 0 || n1 < 0 || pairs < 0 || m > (1 << 20) || !(eps >= 0.f) || (grads != 0 && grads != 6) ||
        !aligned16(dw1) || !aligned16(db1) || !aligned16(dgamma) || !aligned16(dbeta) || !aligned16(dw2) || !aligned16(db2) ||
        (m > 0 && (!x || !w1 || !b1 || !gamma || !beta || !w2 || !dy || !dx || !workspace || (n0 && (!ctx0 || !dctx0)) ||
                   (n1 && (!ctx1 || !dctx1)) || dx == x || dx == dy || (n0 && dctx0 == ctx0) || (n1 && dctx1 == ctx1) || !aligned16(x) || !aligned16(ctx0) || !aligned16(ctx1) ||
                   !aligned16(w1) || !aligned16(w2) || !aligned8(b1) || !aligned8(gamma) || !aligned8(beta) || !aligned16(dy) ||
                   !aligned16(dx) || !aligned16(dctx0) || !aligned16(dctx1) || !aligned16(workspace))))
        return bad(who);
    FbArgs q{};
    q.p = gather_args(x, ctx0, ctx1, w1, b1, dx, heads, n0, n1, pairs, kLnN, kLnN);
    q.w1 = (const f16*)w1, q.w2 = (const f16*)w2, q.b1 = (const f16*)b1, q.gamma = (const f16*)gamma, q.beta = (const f16*)beta;
    q.dy = (const f16*)dy, q.eps = eps, q.dx = (f16*)dx, q.dctx0 = (f16*)dctx0, q.dctx1 = (f16*)dctx1;
    q.dw1 = dw1, q.db1 = db1, q.dgamma = dgamma, q.dbeta = dbeta, q.dw2 = dw2, q.db2 = db2;
    q.full = grads == 6, q.S = ffn_bw_splits((int32_t)m), q.nwg = (int)((m + kBwRows - 1) / kBwRows);
    if (m == 0) {  // no rows: the parameter gradients are zeros
        q.S = 0;
        if (!q.full) return MHA_HD64_STATUS_SUCCESS;
        {
            hipLaunchKernelGGL(ffn_bw_reduce_kernel, dim3(kWN / 256), dim3(256), 0, stream, q);
            hipLaunchKernelGGL(ffn_bw_colreduce_kernel, dim3(kColN / 16), dim3(256), 0, stream, q);
        }
        return launched(who);
    }
    char* ws = (char*)workspace;
    q.pack = (f16*)ws, ws += fb_up256((size_t)kPkEnd * 2);
    q.g = (f16*)ws, ws += fb_up256((size_t)m * kLnN * 2);
    q.da = (f16*)ws, ws += fb_up256((size_t)m * kLnN * 2);
    q.colpart = (float*)ws, ws += fb_up256((size_t)q.nwg * kColN * 4);
    q.wpart = (float*)ws;
    hipLaunchKernelGGL(ffn_bw_pack_kernel, dim3((kPkEnd / 8 + 255) / 256), dim3(256), 0, stream, q);
    hipLaunchKernelGGL(ffn_bw_rows_kernel, dim3(q.nwg), dim3(512), 0, stream, q);
    if (q.full) {
        hipLaunchKernelGGL(ffn_bw_weight_kernel, dim3(24, q.S), dim3(256), 0, stream, q);
        hipLaunchKernelGGL(ffn_bw_reduce_kernel, dim3(kWN / 256), dim3(256), 0, stream, q);
        hipLaunchKernelGGL(ffn_bw_colreduce_kernel, dim3(kColN / 16), dim3(256), 0, stream, q);
    }
    return launched(who);
}

}  // extern "C"
