// lightglue_assign_device.h — what lightglue_assign.hip (the assignment and match heads) and
// lightglue_assign_nll.hip (the assignment loss) share: the argument block, the statistics kernel
// (similarity in fp16 plus the (max, sum) partials of every row and column), the close of those partials,
// and the workspace layout and launch of that kernel. In an unnamed namespace, as lightglue_device.h.
#pragma once

#include "lightglue_device.h"
#include "mha_hd64_device.h"  // (lds_dma16: the inline-asm LDS-DMA piece)

namespace {

// ---- the assignment head: similarity + dual log-softmax in two launches (lg_assign_scores, round 6) ----
// MatchAssignment (lightglue.py:208-233) on the fp16 model: sim = m0 · m1ᵀ (fp16 out, the reference's
// bmm), scores = log_softmax(sim, 2) + log_softmax(sim, 1) + logsig(z0) + logsig(z1)ᵀ. Round 5 ran the
// similarity as a framework GEMM and three glue launches (row pass, column pass, combine: ~31 us per
// single-pair forward at n = 1,024, profiles/r05/single_pair_timelines.txt). Here:
//  * assign_lse_kernel: a workgroup owns 32 rows of ONE image and computes their similarity against
//    1/S of the OTHER image's rows by MFMA (own rows in LDS, the other image streamed per wave through
//    a 2-slot LDS-DMA ring of 128-deep K halves, whole 256-B row pieces), then the (max, sum of
//    exponentials) of each own row over that share, reduced over the 8 waves through LDS. Image-0
//    workgroups give the row partials (and write sim in fp16 for the combine), image-1 workgroups the
//    column partials: no cross-workgroup exchange. (An image-1 workgroup recomputes its columns of sim
//    with the operands swapped: the same products in the same k-step order.) S splits of the other
//    image fill the chip at a single pair (each workgroup then streams 1/S of it).
//  * assign_combine_kernel closes the S partials of its rows and columns (fixed order) into the terms
//    logsig(z) - logsumexp and writes scores = 2 sim + row term + column term.
struct AsArgs {
    const f16* v;     // [batch][m + n][ld]: image 0's rows then image 1's; channels 0..255 the scaled
                      // final projection, channel zc the matchability logit
    long ps;          // pair stride of v (elements)
    int ld, zc, m, n, rb0, S;
    f16* sim;         // workspace [batch][m][n]
    float2* rpart;    // workspace [batch][S][m]: (max, sum of exp) of row i over split s
    float2* cpart;    // workspace [batch][S][n]: the same for column j
    float* rterm;     // workspace [batch][m] (round 6's separate close; kept in the workspace layout)
    float* cterm;     // workspace [batch][n]
    float* scores;    // [batch][m][n]
    // Ragged batches (lg_assign_scores_lens / lg_assign_matches_lens): pair p's leading mlen[p] rows and
    // nlen[p] columns are real, the rest padding (null: all m / n). m and n stay the strides and the
    // launch bounds. No kernel reads a padded row of v, and every use of a padded slot of the workspace
    // is a select, never arithmetic.
    const int* mlen;
    const int* nlen;
};
__device__ __forceinline__ float log_sigmoid_f(float z) { return fminf(z, 0.f) - log1pf(__expf(-fabsf(z))); }
// pair p's valid count, clamped into [1, full] (null table: full)
__device__ __forceinline__ int assign_len(const int* lens, int p, int full) {
    return lens ? min(max(lens[p], 1), full) : full;
}

template <int BPW>  // 32-row blocks of the other image per wave
__global__ __launch_bounds__(512, 1) void assign_lse_kernel(AsArgs a) {
    constexpr int kOwn = 0;                       // own rows [32][512 B], units XOR (row & 15)
    constexpr int kRing = 32 * 512;               // per wave 2 slots of [32][256 B]
    constexpr int kRed = kRing + 8 * 2 * 8192;    // [32 rows][8 waves] fp32
    __shared__ __attribute__((aligned(16))) char smem[kRed + 32 * 8 * 4];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int p = blockIdx.y, sp = blockIdx.z;
    const bool side = (int)blockIdx.x >= a.rb0;
    const int o0 = (side ? (int)blockIdx.x - a.rb0 : (int)blockIdx.x) * 32;
    // the pair's valid rows of both images: every bound below (loads, the other image's descriptor, the
    // key mask, the partials' store) is the valid count, so padded rows are never read
    const int nown = assign_len(side ? a.nlen : a.mlen, p, side ? a.n : a.m);
    const int noth = assign_len(side ? a.mlen : a.nlen, p, side ? a.m : a.n);
    if (o0 >= nown) return;  // (ragged only) a workgroup wholly in padding: its partials are never read
    const f16* const vp = a.v + (size_t)p * a.ps;
    const f16* const own = vp + (size_t)(side ? a.m : 0) * a.ld;
    const f16* const oth = vp + (size_t)(side ? 0 : a.m) * a.ld;

    // own rows: 32 rows x 32 units, two per thread
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int u = i * 512 + tid, row = u >> 5, un = u & 31;
        const f16x8 x = *reinterpret_cast<const f16x8*>(own + (size_t)min(o0 + row, nown - 1) * a.ld + un * 8);
        *(lds_f16x8*)(lds + kOwn + row * 512 + ((un ^ (row & 15)) << 4)) = x;
    }
    // the other image's rows, streamed per wave: block t of this wave = other rows 32 ((t S + sp) 8 + w);
    // chunk c = (block t, K half hk) -> slot c & 1
    const __amdgpu_buffer_rsrc_t ors = __builtin_amdgcn_make_buffer_rsrc(const_cast<f16*>(oth), (short)0,
                                                                         (int)((size_t)noth * a.ld * 2), 0x00020000);
    auto blk_row0 = [&](int t) { return ((t * a.S + sp) * 8 + wave) * 32; };
    auto issue = [&](int c) {  // 8 pieces of 4 rows x 256 B; lane -> (row 4 i + lane / 16, unit lane % 16)
        const int t = c >> 1, hk = c & 1;
        const unsigned m0 = mha_hd64::lds_addr(smem + kRing + wave * 16384 + (c & 1) * 8192);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = 4 * i + (lane >> 4), pu = lane & 15;
            const int grow = min(blk_row0(t) + row, noth - 1);
            const unsigned voff = (unsigned)(grow * a.ld * 2 + hk * 256 + ((pu ^ (row & 15)) << 4));
            mha_hd64::lds_dma16(m0 + i * 1024, voff, ors, 0);
        }
    };
    constexpr int nch = 2 * BPW;
    auto live = [&](int t) { return blk_row0(t) < noth; };  // (wave-uniform)
    if (live(0)) issue(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // own rows in LDS

    f16 sv[BPW][16];
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < BPW; ++t) {
        f32x16 acc = {};
        if (live(t)) {
#pragma unroll
            for (int hk = 0; hk < 2; ++hk) {
                const int c = 2 * t + hk;
                // the next chunk in flight, then this one landed (this wave's own pieces: no barrier)
                if (c + 1 < nch && live((c + 1) >> 1)) {
                    issue(c + 1);
                    asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                const unsigned sb = kRing + wave * 16384 + (c & 1) * 8192;
#pragma unroll
                for (int s = 0; s < 8; ++s) {
                    const int u = 2 * s + hh;
                    const f16x8 af = *(lds_f16x8*)(lds + sb + r * 256 + ((u ^ (r & 15)) << 4));
                    const int uo = 16 * hk + u;
                    const f16x8 bf = *(lds_f16x8*)(lds + kOwn + r * 512 + ((uo ^ (r & 15)) << 4));
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, bf, acc, 0, 0, 0);
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // (the slot is refilled next chunk)
            }
        }
        // lane (r, hh): acc[4 g + e] = sim of own row o0 + r with other row blk_row0(t) + 8 g + 4 hh + e
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int j0 = blk_row0(t) + 8 * g + 4 * hh;
            f16x4 h4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const f16 h = (f16)acc[4 * g + e];
                h4[e] = h;
                sv[t][4 * g + e] = (j0 + e < noth) ? h : (f16)-INFINITY;
                mx = fmaxf(mx, (float)sv[t][4 * g + e]);
            }
            if (!side && o0 + r < a.m && j0 < a.n)
                *reinterpret_cast<f16x4*>(a.sim + ((size_t)p * a.m + o0 + r) * a.n + j0) = h4;
        }
    }
    // (max, sum of exp) of each own row over this split: the max over the 8 waves, then the sum
    float* const red = (float*)(void*)(smem + kRed);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    if (hh == 0) red[r * 8 + wave] = mx;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    float M = red[r * 8];
#pragma unroll
    for (int w = 1; w < 8; ++w) M = fmaxf(M, red[r * 8 + w]);
    float s = 0.f;
    if (M != -INFINITY) {
#pragma unroll
        for (int t = 0; t < BPW; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) s += __expf((float)sv[t][e] - M);
    }
    s += __shfl_xor(s, 32, 64);
    __builtin_amdgcn_s_barrier();  // (every wave has read the maxima)
    if (hh == 0) red[r * 8 + wave] = s;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (wave == 0 && hh == 0 && o0 + r < nown) {
        float tot = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) tot += red[r * 8 + w];
        (side ? a.cpart + ((size_t)p * a.S + sp) * a.n : a.rpart + ((size_t)p * a.S + sp) * a.m)[o0 + r] = make_float2(M, tot);
    }
}

// the logsumexp of S (max, sum) partials, merged in split order; every partial's load issued before
// the merge (round 6's first combine-side close walked them one dependent load at a time: 18-38 us)
__device__ __forceinline__ float lse_close(const float2* part, size_t stride, int S) {
    float2 q[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = k < S ? part[k * stride] : make_float2(-INFINITY, 0.f);
    float mx = -INFINITY, s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        if (q[k].x == -INFINITY) continue;
        if (q[k].x > mx) {
            s = s * __expf(mx - q[k].x) + q[k].y;
            mx = q[k].x;
        } else {
            s += q[k].y * __expf(q[k].x - mx);
        }
    }
    return mx + __logf(s);
}

// lg_assign_scores' split of the other image: enough workgroups for one round of the chip (256)
int assign_splits(int32_t m, int32_t n, int32_t batch) {
    const long base = (long)((m + 31) / 32 + (n + 31) / 32) * batch;
    int S = 1;
    while (S < 8 && base * S * 2 <= 256) S *= 2;
    return S;
}
size_t up256(size_t x) { return (x + 255) / 256 * 256; }
// the workspace both heads share (sim, the lse partials, the terms' slots) and assign_lse_kernel's launch
void assign_layout(AsArgs& a, char* ws, int32_t batch) {
    const size_t b = (size_t)batch, S = (size_t)a.S, m = (size_t)a.m, n = (size_t)a.n;
    a.sim = (f16*)ws;
    a.rpart = (float2*)(ws + up256(b * m * n * 2));
    a.cpart = (float2*)((char*)a.rpart + up256(b * S * m * 8));
    a.rterm = (float*)((char*)a.cpart + up256(b * S * n * 8));
    a.cterm = (float*)((char*)a.rterm + up256(b * m * 4));
}
void launch_assign_lse(const AsArgs& a, int32_t batch, hipStream_t stream) {
    const int m = a.m, n = a.n;
    const dim3 g1(a.rb0 + (n + 31) / 32, batch, a.S);
    const int oth = m > n ? m : n;  // other-image blocks per wave: ceil(blocks / (8 S))
    const int bpw = ((oth + 31) / 32 + 8 * a.S - 1) / (8 * a.S);
    if (bpw <= 1) hipLaunchKernelGGL(assign_lse_kernel<1>, g1, dim3(512), 0, stream, a);
    else if (bpw <= 2) hipLaunchKernelGGL(assign_lse_kernel<2>, g1, dim3(512), 0, stream, a);
    else if (bpw <= 4) hipLaunchKernelGGL(assign_lse_kernel<4>, g1, dim3(512), 0, stream, a);
    else hipLaunchKernelGGL(assign_lse_kernel<8>, g1, dim3(512), 0, stream, a);
}

}  // namespace
