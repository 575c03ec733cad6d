// lightglue_ffn_device.h — what the FFN's kernel files share (lightglue_ffn_ln.hip: linear_ln_kernel;
// lightglue_ffn.hip: the rows kernels): the FFN's widths, the diagnostic builds' stamps, and the steps
// that ffn_rows_kernel and ffn_rows16_kernel both take, each written once (the ones that could not move
// without changing a kernel's instructions: profiles/ffn_split/INDEX.md). Unnamed namespace, as lightglue_device.h.
#pragma once

#include "lightglue_device.h"

namespace {

constexpr int kLnN = 512;     // the FFN's width: its input [x | heads] and its hidden channels (2d)
constexpr int kFfnOut = 256;  // the FFN's output channels (d)

// ---- stamps of the diagnostic builds (never shipped): per wave, s_memtime cycles by chained segment ----
// A file turns them on for its kernels by defining FFN_STAMPS ahead of this header. FFN_SEG(k) ends
// segment k: the wave's LDS and scalar traffic drained, the clock read, the cycles since the last stamp
// added to slot k. FFN_SEG_VM(k) drains the wave's loads and stores first. FFN_STAMPS_WRITE(wave, s6, s7):
// lane 0 of each wave of the first 256 workgroups writes its 8 slots — 0..4 those segments, 5 entry to
// the last stamp, 6 and 7 as given. FFN_STAMPS_READBACK(name): the entry point that copies the slots to
// the host (diagnostic build only: not in the header). In the shipped build all of them are empty.
#ifdef FFN_STAMPS
__device__ unsigned long long g_ffn_stamps[256 * 8 * 8];
struct FfnStamps {
    unsigned long long seg[7] = {0, 0, 0, 0, 0, 0, 0}, last, entry;
    __device__ __forceinline__ FfnStamps() {
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(entry)::"memory");
        last = entry;
    }
    __device__ __forceinline__ void mark(int k, bool vm = false) {
        unsigned long long t;
        if (vm) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
        seg[k] += t - last;
        last = t;
    }
    __device__ __forceinline__ void write(int wave, unsigned long long s6, unsigned long long s7) const {
        if ((threadIdx.x & 63) != 0 || blockIdx.x >= 256) return;
        unsigned long long* d = g_ffn_stamps + ((size_t)blockIdx.x * 8 + wave) * 8;
        for (int k = 0; k < 5; ++k) d[k] = seg[k];
        d[5] = last - entry, d[6] = s6, d[7] = s7;
    }
};
#define FFN_STAMPS_BEGIN() FfnStamps stamps_
#define FFN_SEG(k) stamps_.mark(k)
#define FFN_SEG_VM(k) stamps_.mark(k, true)
#define FFN_STAMPS_WRITE(wave, s6, s7) stamps_.write(wave, s6, s7)
#define FFN_STAMPS_READBACK(name)                                                                              \
    extern "C" int32_t name(void* host_dst) {                                                                   \
        return hipMemcpyFromSymbol(host_dst, HIP_SYMBOL(g_ffn_stamps), sizeof(g_ffn_stamps)) == hipSuccess ? 0 : 1; \
    }
#else
#define FFN_STAMPS_BEGIN() do {} while (0)
#define FFN_SEG(k) do {} while (0)
#define FFN_SEG_VM(k) do {} while (0)
#define FFN_STAMPS_WRITE(wave, s6, s7) do {} while (0)
#define FFN_STAMPS_READBACK(name)
#endif

// ---- the rows kernels (lightglue_ffn.hip) ----
// phase 3 (lg_linear_cat_ffn_proj): the next attention's projection of the FFN output x'
enum { E3_NONE = 0, E3_SPLIT2 = 1, E3_QKV = 2, E3_PLAIN = 3 };
struct Proj3 {
    const f16* b3;      // [n3] bias
    const f16* cosv;    // E3_QKV: rotary tables [m, 64]
    const f16* sinv;
    f16* out[6];        // SPLIT2: a0 a1 b0 b1; QKV: q0 k0 v0 q1 k1 v1 (per-image head-major); PLAIN: [m, n_store]
    int n_store;        // E3_PLAIN: channels stored per row (the first n_store of 32 NB3 8)
};
// a row's destination among them (SPLIT2, QKV): its image (first: image 0) and the part its channels lie in
template <int E3>
__device__ __forceinline__ f16* proj3_out(const Proj3& q3, bool first, int part) {
    return q3.out[E3 == E3_QKV ? (first ? 0 : 3) + part : (first ? 0 : 1) + 2 * part];
}

// LDS behind the kernel's tiles, from PAR on: the vectors, the LayerNorm's partials and phase 3's vectors
template <int MT, int E3, int NB3, int PAR>
struct FfnLds {
    static constexpr int kPar = PAR;                              // b1, gamma, beta [512], b2 [256] fp16
    static constexpr int kRed = kPar + (3 * kLnN + kFfnOut) * 2;  // row partials [2][MT][8 waves] fp32
    static constexpr int kB3 = kRed + 2 * MT * 8 * 4;             // b3 [32 NB3 8] fp16
    // E3_QKV: this tile's rows of cos / sin, [2][MT] rows of 64 fp16 at a 144-B pitch (36 banks a row
    // apart: a column read by 32 rows is 2-way and by 16 rows conflict-free, where a 128-B pitch was 16-
    // and 8-way)
    static constexpr int kCS = kB3 + NB3 * 256 * 2, kCSP = 144;
    static constexpr int kEnd = kCS + (E3 == E3_QKV ? 2 * MT * kCSP : 0);
    static_assert(kEnd <= 160 * 1024, "LDS");
};

// The wave's weight stream through a ring of R registers: piece i sits in slot i % R, and taking piece i
// (compile-time after unrolling) issues piece i + R behind it, up to the N pieces the wave consumes.
// piece(i): the load of stream position i (passed in, not kept: as a member it changed the 16-row forms).
template <int R, int N>
struct WRing {
    f16x8 q[R];
    template <typename Piece>
    __device__ __forceinline__ explicit WRing(const Piece& piece) {
#pragma unroll
        for (int i = 0; i < R; ++i) {  // (in stream order: the loops' counted waits assume it)
            q[i] = piece(i);
            if (i & 1) __builtin_amdgcn_sched_barrier(0);
        }
    }
    template <typename Piece>
    __device__ __forceinline__ f16x8 take(int i, const Piece& piece) {
        const f16x8 w = q[i % R];
        if (i + R < N) q[i % R] = piece(i + R);
        return w;
    }
};
// the 8 waves' packed streams of np pieces of 1 KiB, and the load of this lane's 16 B at wo + so
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wstream_rsrc(const f16* wp, int np) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(wp), (short)0, 8 * np * 1024, 0x00020000);
}
__device__ __forceinline__ f16x8 wstream_load(__amdgpu_buffer_rsrc_t wrs, unsigned wo, int so) {
    return __builtin_bit_cast(f16x8, __builtin_amdgcn_raw_buffer_load_b128(wrs, wo, so, 0));
}

// h of one packed pair, fp16(acc + b1) in one rounding each (mixh2), added to the row sum s1
__device__ __forceinline__ unsigned h_sum2(float acc0, float acc1, unsigned b2, float& s1) {
    const unsigned h2 = mixh2(acc0, acc1, b2);
    row_sum2(h2, s1);
    return h2;
}
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
// ... of row `row`, from the partials red = [2][MT][8 waves] in LDS, in a fixed order
__device__ __forceinline__ RowStats row_stats(const lds_char* red, int MT, int row, float eps) {
    auto part = [&](int i) { return *(const __attribute__((address_space(3))) f32x4*)(red + (i + row * 8) * 4); };
    return ln_merge(part(0), part(4), part(MT * 8), part(MT * 8 + 4), eps);
}
// GELU(LN(h)) of one packed pair, in fp32: h * rstd + nmr (nmr = -mean * rstd), times gamma plus beta
// (g2, be2: their packed fp16 pairs)
__device__ __forceinline__ f32x2 ln_gelu2(unsigned h2, float rstd, float nmr, unsigned g2, unsigned be2) {
    const float x0 = mixn<0>(h2, rstd, nmr), x1 = mixn<1>(h2, rstd, nmr);
    return gelu_as2(f32x2{mixf<0>(x0, g2, be2), mixf<1>(x1, g2, be2)});
}
// fp16(acc + b) (lin_val) of the accumulator's elements e .. e + 3
template <typename V>
__device__ __forceinline__ f16x4 lin_val4(const V& acc, int e, f16x4 b) {
    return f16x4{lin_val(acc[e], b[0]), lin_val(acc[e + 1], b[1]), lin_val(acc[e + 2], b[2]), lin_val(acc[e + 3], b[3])};
}

}  // namespace
