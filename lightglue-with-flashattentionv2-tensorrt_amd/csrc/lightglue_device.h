// lightglue_device.h — what more than one of the matcher's kernel files uses (lightglue_linear.hip: the
// projections, lightglue_ffn_ln.hip and lightglue_ffn.hip: the FFN (what only they share: lightglue_ffn_device.h),
// lightglue_assign.hip: the assignment and match heads, lightglue_glue.hip: the layout / normalisation
// kernels): the vector types, the projections' argument block and A-gather, their output arithmetic, the
// 256-row forms' DMA sources, the entry points' argument-check and launch-status helpers. All in an unnamed
// namespace: each file compiles its own copy, and the kernels' mangled names do not depend on their file.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lightglue_glue.h"
#include "mha_hd64.h"
#include "mha_hd64_internal.h"

namespace lightglue {
// The projections' tile form, forced (0..5) or -1 = chosen by size: lg_linear_set_wide / LG_LINEAR_WIDE
// (lightglue_linear.hip; lg_linear_cat_ln_gelu in lightglue_ffn_ln.hip reads it too)
__attribute__((visibility("hidden"))) int wide_mode();
}  // namespace lightglue

namespace {

typedef _Float16 f16;
typedef f16 f16x8 __attribute__((ext_vector_type(8)));
typedef f16 f16x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) char lds_char;
typedef __attribute__((address_space(3))) f16x8 lds_f16x8;

__device__ __forceinline__ void st_out(f16* dst, f16x8 v) { *reinterpret_cast<f16x8*>(dst) = v; }
constexpr int kD = 64;  // head dim

struct LinArgs {
    const f16* a;      // [m, k] activations (A-gather: x [m, k/2])
    const f16* ctx0;   // A-gather: head-major attention outputs of image 0 / 1 [heads, ni, 64]
    const f16* ctx1;
    const f16* w;      // [n, k]
    const f16* bias;   // [n]
    const f16* res;    // [m, n] residual (EPI_BIAS, nullable)
    const f16* cosv;   // [m, 64] rotary tables (EPI_QKV_ROTARY)
    const f16* sinv;
    f16* out[6];       // EPI_BIAS: out[0] [m, n]; QKV: q0 k0 v0 q1 k1 v1; SPLIT2: a0 a1 b0 b1
    int m, n, k;
    int heads, n0, n1; // per-image split: m = pairs x (n0 + n1) rows, pair-major (n0 of image 0, n1 of image 1)
    int mtiles, total;
};

// Row `row` of the stacked rows -> its image and the offset of its head-h segment in that image's
// [pairs, heads, ni, 64] tensor
struct LinRow {
    bool first;
    size_t off;
};
__device__ __forceinline__ LinRow lin_row(const LinArgs& p, int row, int h) {
    const int ntot = p.n0 + p.n1;
    const int pr = row / ntot, l = row - pr * ntot;
    const bool first = l < p.n0;
    const int r = first ? l : l - p.n0, nn = first ? p.n0 : p.n1;
    return {first, (((size_t)pr * p.heads + h) * nn + r) * kD};
}

// global source of A row `row`, 16-B unit `gc` (8 k values)
template <bool GATHER>
__device__ __forceinline__ const f16* a_src(const LinArgs& p, int row, int gc) {
    if constexpr (!GATHER) {
        return p.a + (size_t)row * p.k + gc * 8;
    } else {
        const int half = p.k / 2, col = gc * 8;
        if (col < half) return p.a + (size_t)row * half + col;  // x
        const int c2 = col - half, h = c2 / kD, d = c2 % kD;
        const LinRow lr = lin_row(p, row, h);
        return (lr.first ? p.ctx0 : p.ctx1) + lr.off + d;
    }
}

// The projections' output arithmetic, shared by every form (so every form gives the same bits): the
// GEMM value plus bias is rounded to fp16 once (F.linear's fp16 output, lightglue.py:97-122); the
// residual add and the rotary (lightglue.py:124-134) then work from that value, as the reference's
// fp16 model does (x + ffn(...): fp32 with one rounding; q * cos + rotate(q) * sin: fp16 products
// and sum, rot_pair).
__device__ __forceinline__ f16 lin_val(float acc, f16 b) { return (f16)(acc + (float)b); }
__device__ __forceinline__ f16 res_add(f16 v, f16 r) { return (f16)((float)v + (float)r); }
// Exact (erf) GELU for the fp16 FFN with erf from Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7, far
// below the fp16 rounding of the output), folded: with z = |x| / sqrt(2), r = 1 / (1 + p z) and
// erf(z) = 1 - y(r) e^{-z^2}, x Phi(x) = max(x, 0) - |x| (y / 2) e^{-x^2 / 2} for either sign of x (no
// 1 + erf cancellation for negative x); one v_rcp_f32 and one v_exp_f32, the 1/2 and 1/sqrt(2) in
// the constants. (lightglue_glue.hip and the FFN's files compute it alike: this definition.)
__device__ __forceinline__ float gelu_as(float x) {
    const float ax = fabsf(x);
    const float r = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752f, ax, 1.f));
    float p = fmaf(0.5f * 1.061405429f, r, 0.5f * -1.453152027f);
    p = fmaf(p, r, 0.5f * 1.421413741f);
    p = fmaf(p, r, 0.5f * -0.284496736f);
    p = fmaf(p, r, 0.5f * 0.254829592f);
    const float w = p * r * ax;
    const float e = __builtin_amdgcn_exp2f(x * x * (-0.5f * 1.4426950408889634f));
    return fmaf(-w, e, fmaxf(x, 0.f));
}
// The same on a pair of values, written on float2 so that the FMAs and products issue as packed
// v_pk_fma_f32 / v_pk_mul_f32 (two values per instruction: the vector pipe's full fp32 rate; the
// rcp, exp, abs and max stay per value)
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 gelu_as2(f32x2 x) {
    const f32x2 ax = f32x2{fabsf(x[0]), fabsf(x[1])};
    const f32x2 den = ax * (0.3275911f * 0.70710678118654752f) + 1.f;
    const f32x2 r = f32x2{__builtin_amdgcn_rcpf(den[0]), __builtin_amdgcn_rcpf(den[1])};
    f32x2 p = r * (0.5f * 1.061405429f) + (0.5f * -1.453152027f);
    p = p * r + (0.5f * 1.421413741f);
    p = p * r + (0.5f * -0.284496736f);
    p = p * r + (0.5f * 0.254829592f);
    const f32x2 w = p * r * ax;
    const f32x2 a = x * x * (-0.5f * 1.4426950408889634f);
    const f32x2 e = f32x2{__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
    return f32x2{fmaxf(x[0], 0.f), fmaxf(x[1], 0.f)} - w * e;
}

// (x0, x1) of a rotary pair (d, d + 1) -> (x0 c0 - x1 s0, x1 c1 + x0 s1), elements e, e + 1 of v,
// in fp16 arithmetic as the reference's fp16 model evaluates t * cos + rotate_half(t) * sin
// (lightglue.py:124-134): each product and the sum rounded to fp16 (packed v_pk_mul_f16 /
// v_pk_add_f16, no contraction into an fma)
typedef f16 f16x2 __attribute__((ext_vector_type(2)));
template <typename V>
__device__ __forceinline__ void rot_pair(V& v, int e, f16 c0, f16 s0, f16 c1, f16 s1) {
#pragma clang fp contract(off)
    const f16x2 x = f16x2{v[e], v[e + 1]};
    const f16x2 xr = f16x2{-v[e + 1], v[e]};
    const f16x2 o = x * f16x2{c0, c1} + xr * f16x2{s0, s1};
    v[e] = o[0];
    v[e + 1] = o[1];
}

// Mixed-precision FMAs for the one-launch LayerNorm epilogue (fp16 operands read in place, halves
// chosen by op_sel): mixf(x, g, b) = x * g + b in fp32 with g, b the HI-th halves of packed fp16
// words; mixh(acc, b) = fp16(acc + b), rounded once (the two-launch path's lin_val rounds to fp32
// first: the forms agree within the rare double-rounding ulp, not in every bit).
template <int HI>
__device__ __forceinline__ float mixf(float x, unsigned g2, unsigned b2) {
    float r;
    if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[0,1,1] op_sel_hi:[0,1,1]" : "=v"(r) : "v"(x), "v"(g2), "v"(b2));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[0,1,1]" : "=v"(r) : "v"(x), "v"(g2), "v"(b2));
    return r;
}
// The packed forms (round 6): h2 = (fp16(acc0 + b.lo), fp16(acc1 + b.hi)) in one register, each half
// rounded once as mixh does; mixn(h2, a, c) = h2's HI-th half * a + c in fp32 (the LayerNorm's
// normalisation read straight from the packed fp16 values)
__device__ __forceinline__ unsigned mixh2(float acc0, float acc1, unsigned b2) {
    unsigned h;
    asm("v_fma_mixlo_f16 %0, %1, 1.0, %2 op_sel_hi:[0,0,1]\n\t"
        "v_fma_mixhi_f16 %0, %3, 1.0, %2 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
        : "=&v"(h)
        : "v"(acc0), "v"(b2), "v"(acc1));
    return h;
}
template <int HI>
__device__ __forceinline__ float mixn(unsigned h2, float a, float c) {
    float r;
    if constexpr (HI) asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h2), "v"(a), "v"(c));
    else asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h2), "v"(a), "v"(c));
    return r;
}
// the row sum of one packed pair: s1 += h.lo + h.hi (v_dot2_f32_f16)
__device__ __forceinline__ void row_sum2(unsigned h2, float& s1) {
    const f16x2 h = __builtin_bit_cast(f16x2, h2);
    s1 = __builtin_amdgcn_fdot2(h, f16x2{(f16)1.f, (f16)1.f}, s1, false);
}
template <int HI>
__device__ __forceinline__ float mixh(float acc, unsigned b2) {
    unsigned h;
    if constexpr (HI) asm("v_fma_mixlo_f16 %0, %1, 1.0, %2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "=v"(h) : "v"(acc), "v"(b2));
    else asm("v_fma_mixlo_f16 %0, %1, 1.0, %2 op_sel_hi:[0,0,1]" : "=v"(h) : "v"(acc), "v"(b2));
    return (float)__builtin_bit_cast(f16x2, h)[0];
}

// ---- per-tile DMA sources of the 256-row forms: each wave's W and A pieces of a tile, computed once
// per tile (row clamps, the swizzled unit, the A-gather's image and head-major offset) so that a K
// step's DMA is one address add per piece. BK-deep steps: a 1-KiB piece is 1024 / (2 BK) rows; lane
// -> (row RP i + lane / U, LDS unit lane % U <- global unit (lane % U) ^ swz(row)), U = BK / 8 units a row
template <int NWP, int NAP>
struct TileSrc {
    const f16* w[NWP];
    const f16* a[NAP];  // A rows (the gather: x rows)
    const f16* c[NAP];  // the gather: head 0 of the row in its image's [pairs, heads, ni, 64] tensor
    int hs[NAP];        // the gather: elements between heads there (ni * 64)
};
template <int BK>
__device__ __forceinline__ int src_unit(int row, int pos) {
    return BK == 64 ? (pos ^ ((row >> 1) & 7)) : (pos ^ ((row >> 2) & 3));
}
// (LW waves issue a stage's DMA pieces: piece wave + LW h)
template <bool GATHER, int BK, int NWP, int NAP, int LW>
__device__ __forceinline__ TileSrc<NWP, NAP> tile_src(const LinArgs& p, int m0, int n0, int wave, int lane) {
    constexpr int U = BK / 8, RP = 1024 / (2 * BK);
    TileSrc<NWP, NAP> t;
#pragma unroll
    for (int h = 0; h < NWP; ++h) {
        const int row = RP * (wave + LW * h) + lane / U;
        const int wr = min(n0 + row, p.n - 1);
        t.w[h] = p.w + (size_t)wr * p.k + src_unit<BK>(row, lane % U) * 8;
    }
#pragma unroll
    for (int h = 0; h < NAP; ++h) {
        const int row = RP * (wave + LW * h) + lane / U;
        const int ar = min(m0 + row, p.m - 1);
        const int gu8 = src_unit<BK>(row, lane % U) * 8;
        if constexpr (!GATHER) {
            t.a[h] = p.a + (size_t)ar * p.k + gu8;
        } else {
            t.a[h] = p.a + (size_t)ar * (p.k / 2) + gu8;
            const LinRow lr = lin_row(p, ar, 0);
            t.c[h] = (lr.first ? p.ctx0 : p.ctx1) + lr.off + gu8;
            t.hs[h] = (lr.first ? p.n0 : p.n1) * kD;
        }
    }
    return t;
}
// K step ks (compile-time after unrolling; K = KS BK) of a tile into the stage at sb: W pieces
// wave + LW h at sb, A pieces at sb + BN BK 2
template <bool GATHER, int BK, int KS, int BN, int LW, int NWP, int NAP>
__device__ __forceinline__ void tile_issue(const TileSrc<NWP, NAP>& t, int ks, char* sb, int wave) {
#pragma unroll
    for (int h = 0; h < NWP; ++h)
        __builtin_amdgcn_global_load_lds((const void*)(t.w[h] + ks * BK),
                                         (__attribute__((address_space(3))) void*)(sb + (wave + LW * h) * 1024), 16, 0, 0);
#pragma unroll
    for (int h = 0; h < NAP; ++h) {
        const f16* src;
        if constexpr (!GATHER) {
            src = t.a[h] + ks * BK;
        } else {
            constexpr int half = KS * BK / 2;
            const int col = ks * BK;
            src = col < half ? t.a[h] + col : t.c[h] + ((col - half) / kD) * t.hs[h] + (col - half) % kD;
        }
        __builtin_amdgcn_global_load_lds((const void*)src,
                                         (__attribute__((address_space(3))) void*)(sb + BN * BK * 2 + (wave + LW * h) * 1024),
                                         16, 0, 0);
    }
}

// ---- host side: the entry points' argument checks and launch status ----
constexpr int kTileGrid = 256;  // the 256-row forms: one workgroup per CU
bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
bool aligned8(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) == 0; }
bool aligned4(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 3) == 0; }
bool aligned2(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 1) == 0; }
bool dtype_ok(int32_t dt) { return dt == MHA_HD64_DT_FLOAT || dt == MHA_HD64_DT_HALF; }
// aligned for elements of a dtype that dtype_ok accepts
bool aligned_as(int32_t dtype, const void* q) { return dtype == MHA_HD64_DT_HALF ? aligned2(q) : aligned4(q); }
// batch images of h x w pixels: grid z / y and 32-bit pixel counts
bool image_ok(int64_t h, int64_t w, int64_t batch) {
    return h >= 1 && w >= 1 && batch >= 0 && batch <= 65535 && h * w <= (1 << 26) && h * w * (batch ? batch : 1) <= (1 << 30);
}
// (n: whole 64-channel tiles)
bool shape_ok(int m, int n, int k) { return m >= 0 && n > 0 && n % 64 == 0 && (k == 256 || k == 512); }

int32_t bad(const char* what) { return mha_hd64::report_error(MHA_HD64_STATUS_BAD_PARAM, what, "bad arguments"); }
// the status of the launches an entry point has just made
int32_t launched(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return MHA_HD64_STATUS_SUCCESS;
    return mha_hd64::report_error(MHA_HD64_STATUS_LAUNCH_FAILED, what, hipGetErrorString(e));
}

// The gather entry points' arguments: A = [x | merge_heads(ctx0, ctx1)] of `pairs` image pairs, one
// [m, n] output
LinArgs gather_args(const void* x, const void* ctx0, const void* ctx1, const void* w, const void* bias, void* out,
                    int heads, int n0, int n1, int pairs, int n, int k) {
    LinArgs p{};
    p.a = (const f16*)x, p.ctx0 = (const f16*)ctx0, p.ctx1 = (const f16*)ctx1, p.w = (const f16*)w;
    p.bias = (const f16*)bias, p.out[0] = (f16*)out;
    p.m = pairs * (n0 + n1), p.n = n, p.k = k, p.heads = heads, p.n0 = n0, p.n1 = n1;
    return p;
}

}  // namespace
