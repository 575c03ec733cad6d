// lightglue_assign.hip — the matcher's assignment head and match head as gfx950 MFMA kernels
// (include/lightglue_glue.h: lg_assign_scores*, lg_assign_matches*). fp16 in, fp32 scores.
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

// The closed terms logsig(z) - logsumexp of a block's 8 W rows (rts) and 512 columns (cts) from the S
// partials, by 256 threads (every partial and z load in flight at once); ends in the block's barrier.
// Shared by the combine and the match head's best kernel, so both see the same bits.
template <int W>
__device__ __forceinline__ void assign_close_terms(const AsArgs& a, int p, int ib, int jb, float* rts, float* cts) {
    const int tid = threadIdx.x;
    const f16* const vp = a.v + (size_t)p * a.ps;
    // (ragged: the terms of valid rows and columns only; the other slots of rts / cts stay unwritten)
    const int ml = assign_len(a.mlen, p, a.m), nl = assign_len(a.nlen, p, a.n);
    if (tid < 8 * W && ib + tid < ml) {
        const float z = (float)vp[(size_t)(ib + tid) * a.ld + a.zc];
        rts[tid] = log_sigmoid_f(z) - lse_close(a.rpart + (size_t)p * a.S * a.m + ib + tid, a.m, a.S);
    }
#pragma unroll
    for (int c = tid; c < 512; c += 256) {
        if (jb + c < nl) {
            const float z = (float)vp[(size_t)(a.m + jb + c) * a.ld + a.zc];
            cts[c] = log_sigmoid_f(z) - lse_close(a.cpart + (size_t)p * a.S * a.n + jb + c, a.n, a.S);
        }
    }
    __syncthreads();
}

// scores = 2 sim + rterm[i] + cterm[j] (fp32), the terms logsig(z) - logsumexp closed here from the S
// partials (round 6: a separate close launch cost ~4.7 us at a single pair): the block's 8 W rows'
// and 512 columns' terms into LDS (256 threads; every partial and z load in flight at once), then each
// of the W combine waves writes 8 rows, a lane 8 columns (16-B loads, 2 x 16-B stores)
template <int W>
__global__ __launch_bounds__(256) void assign_combine_kernel(AsArgs a) {
    __shared__ float rts[8 * W], cts[512];
    const int p = blockIdx.z, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int ib = blockIdx.x * 8 * W, jb = blockIdx.y * 512;
    assign_close_terms<W>(a, p, ib, jb, rts, cts);
    const int i0 = ib + wave * 8, j = jb + lane * 8;
    if (wave >= W || i0 >= a.m || j >= a.n) return;
    const int i1 = min(i0 + 8, a.m);
    // (ragged) padded rows and columns are written too, as -inf, by select: what sim, rts and cts hold
    // there (unwritten workspace and LDS) never enters a written value
    const int ml = assign_len(a.mlen, p, a.m), nl = assign_len(a.nlen, p, a.n);
    const f16* sim = a.sim + (size_t)p * a.m * a.n;
    float* out = a.scores + (size_t)p * a.m * a.n;
    f16x8 x[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) x[b] = *reinterpret_cast<const f16x8*>(sim + (size_t)min(i0 + b, i1 - 1) * a.n + j);
    float cl[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cl[e] = cts[lane * 8 + e];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        if (i0 + b >= i1) break;
        const float rt = rts[wave * 8 + b];
        const int nv = i0 + b < ml ? nl - j : 0;  // this lane's valid columns of the row (<= 0: none)
        f32x4 o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o0[e] = e < nv ? 2.f * (float)x[b][e] + rt + cl[e] : -INFINITY;
            o1[e] = e + 4 < nv ? 2.f * (float)x[b][e + 4] + rt + cl[e + 4] : -INFINITY;
        }
        *reinterpret_cast<f32x4*>(out + (size_t)(i0 + b) * a.n + j) = o0;
        *reinterpret_cast<f32x4*>(out + (size_t)(i0 + b) * a.n + j + 4) = o1;
    }
}

// ---- the match head: mutual nearest neighbours without the scores tensor (lg_assign_matches) ----
// filter_matches (lightglue.py:235-258, its commented-out dense outputs included) on the scores the
// combine would write, in two launches after assign_lse_kernel:
//  * assign_best_kernel takes the combine's place (blocks of 32 rows x 512 columns, the same closes and
//    16-B loads of sim, each score evaluated as the combine evaluates it) and keeps, instead of the
//    scores, each row's (max, column) over the block's columns (rbest, one slab per column block) and
//    each column's (max, row) over the block's rows (cbest, one slab per 32-row strip).
//  * assign_finish_kernel, one workgroup per pair: closes the slabs in ascending order, the mutual and
//    threshold logic of both sides, and the compact list by a prefix sum over the pair's rows.
// Ties go to the lowest index everywhere (strict > in ascending order; the wave reduction compares
// (value, index)); no atomics and no exchange between workgroups inside a launch, so a call is
// bitwise reproducible.
struct AmArgs {
    AsArgs a;
    int RB, CB, K;      // 32-row strips, 512-column blocks, list rows per pair = min(m, n)
    float thr;
    float2* rbest;      // workspace [batch][CB][m]: (max, column as int bits) of row i over column block c
    float2* cbest;      // workspace [batch][RB][n]: (max, row as int bits) of column j over row strip r
    int *m0, *m1, *mt, *cnt;
    float *s0, *s1, *ms;
};

__global__ __launch_bounds__(256) void assign_best_kernel(AmArgs q) {
    const AsArgs& a = q.a;
    __shared__ float rts[32], cts[512];
    __shared__ __attribute__((aligned(16))) float cbv[4][512];
    __shared__ __attribute__((aligned(16))) int cbi[4][512];
    const int p = blockIdx.z, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int ib = blockIdx.x * 32, jb = blockIdx.y * 512;
    // (ragged) the pair's valid rows and columns bound everything; a block wholly in padding leaves its
    // slabs unwritten, and the finish kernel reads the slabs of blocks with a valid row and column only
    const int ml = assign_len(a.mlen, p, a.m), nl = assign_len(a.nlen, p, a.n);
    if (ib >= ml || jb >= nl) return;
    assign_close_terms<4>(a, p, ib, jb, rts, cts);
    const int i0 = ib + wave * 8, j = jb + lane * 8;
    const int i1 = min(i0 + 8, ml);           // (<= i0: a wave past the last row)
    const bool act = j < nl && i0 < i1;       // this lane holds >= 1 column of >= 1 row
    const f16* sim = a.sim + (size_t)p * a.m * a.n;
    f16x8 x[8] = {};
    float cl[8] = {};
    if (act) {
#pragma unroll
        for (int b = 0; b < 8; ++b) x[b] = *reinterpret_cast<const f16x8*>(sim + (size_t)min(i0 + b, i1 - 1) * a.n + j);
#pragma unroll
        for (int e = 0; e < 8; ++e) cl[e] = cts[lane * 8 + e];
    }
    float cv[8];
    int ci[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) cv[e] = -INFINITY, ci[e] = ib;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const int i = i0 + b;
        if (i >= i1) break;  // (wave-uniform)
        float bv = -INFINITY;
        int bj = j < nl ? j : 0x7fffffff;
        if (act) {
            const float rt = rts[wave * 8 + b];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                // (a padded column of a ragged pair: -inf by select, never above any best)
                const float s = j + e < nl ? 2.f * (float)x[b][e] + rt + cl[e] : -INFINITY;
                if (s > bv) bv = s, bj = j + e;
                if (s > cv[e]) cv[e] = s, ci[e] = i;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oj = __shfl_xor(bj, off, 64);
            if (ov > bv || (ov == bv && oj < bj)) bv = ov, bj = oj;
        }
        if (lane == 0) q.rbest[((size_t)p * q.CB + blockIdx.y) * a.m + i] = make_float2(bv, __int_as_float(bj));
    }
    // the block's columns over its 4 waves' rows, in wave (= row) order
#pragma unroll
    for (int e = 0; e < 8; ++e) cbv[wave][lane * 8 + e] = cv[e], cbi[wave][lane * 8 + e] = ci[e];
    __syncthreads();
#pragma unroll
    for (int c = tid; c < 512; c += 256) {
        if (jb + c >= nl) continue;
        float v = cbv[0][c];
        int i = cbi[0][c];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (cbv[w][c] > v) v = cbv[w][c], i = cbi[w][c];
        q.cbest[((size_t)p * q.RB + blockIdx.x) * a.n + jb + c] = make_float2(v, __int_as_float(i));
    }
}

__global__ __launch_bounds__(1024) void assign_finish_kernel(AmArgs q) {
    const AsArgs& a = q.a;
    __shared__ int js[2048], is[2048];   // j*(i), i*(j)
    __shared__ float sc[2048];           // row i's best score, then mscores0[i]
    __shared__ unsigned char vld[2048];  // valid0[i]
    __shared__ int wsum[16];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m, n = a.n;
    // (ragged) ml x nl is the pair's valid sub-matrix: the slabs of its blocks only (cbn column blocks, rbn
    // strips: the ones assign_best_kernel wrote), its rows and columns only; the padded rows and
    // columns get -1 / 0 below. The slabs' strides stay q.CB, q.RB, m, n.
    const int ml = assign_len(a.mlen, p, m), nl = assign_len(a.nlen, p, n);
    const int cbn = (nl + 511) / 512, rbn = (ml + 31) / 32;
    for (int i = tid; i < ml; i += 1024) {
        float2 r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = k < cbn ? q.rbest[((size_t)p * q.CB + k) * m + i] : make_float2(-INFINITY, 0.f);
        float bv = r[0].x;
        int bj = __float_as_int(r[0].y);
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (k < cbn && r[k].x > bv) bv = r[k].x, bj = __float_as_int(r[k].y);
        js[i] = min(max(bj, 0), nl - 1);
        sc[i] = bv;
    }
    for (int j = tid; j < nl; j += 1024) {
        float bv = -INFINITY;
        int bi = 0;
        for (int k0 = 0; k0 < rbn; k0 += 8) {
            float2 c[8];
#pragma unroll
            for (int k = 0; k < 8; ++k)
                c[k] = k0 + k < rbn ? q.cbest[((size_t)p * q.RB + k0 + k) * n + j] : make_float2(-INFINITY, 0.f);
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (k0 + k < rbn && c[k].x > bv) bv = c[k].x, bi = __float_as_int(c[k].y);
        }
        is[j] = min(max(bi, 0), ml - 1);
    }
    __syncthreads();
    // the row side; a thread owns rows 2 tid and 2 tid + 1, so the list keeps ascending i
    bool val[2] = {false, false};
    float ms[2] = {0.f, 0.f};
    int jj[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int i = 2 * tid + k;
        if (i >= m) continue;
        if (i >= ml) {  // (ragged) a padded row: no match
            q.m0[(size_t)p * m + i] = -1;
            q.s0[(size_t)p * m + i] = 0.f;
            continue;
        }
        jj[k] = js[i];
        const bool mutual = is[jj[k]] == i;
        ms[k] = mutual ? expf(sc[i]) : 0.f;
        val[k] = ms[k] > q.thr;
        sc[i] = ms[k];
        vld[i] = val[k];
        q.m0[(size_t)p * m + i] = val[k] ? jj[k] : -1;
        q.s0[(size_t)p * m + i] = ms[k];
    }
    const int cnt = (int)val[0] + (int)val[1];
    int inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();  // (also: sc and vld of every row written)
    for (int j = tid; j < n; j += 1024) {
        if (j >= nl) {  // (ragged) a padded column: no match
            q.s1[(size_t)p * n + j] = 0.f;
            q.m1[(size_t)p * n + j] = -1;
            continue;
        }
        const int i = is[j];
        const bool mutual = js[i] == j;
        q.s1[(size_t)p * n + j] = mutual ? sc[i] : 0.f;
        q.m1[(size_t)p * n + j] = (mutual && vld[i]) ? i : -1;
    }
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        if (w < wave) base += wsum[w];
        total += wsum[w];
    }
    int pos = base + inc - cnt;
    int* const mt = q.mt + (size_t)p * q.K * 2;
    float* const mso = q.ms + (size_t)p * q.K;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        if (!val[k] || pos >= q.K) continue;  // (pos < K always: valid rows map to distinct columns)
        mt[2 * pos] = 2 * tid + k, mt[2 * pos + 1] = jj[k];
        mso[pos] = ms[k];
        ++pos;
    }
    total = min(total, q.K);
    for (int r = total + tid; r < q.K; r += 1024) mt[2 * r] = -1, mt[2 * r + 1] = -1, mso[r] = 0.f;
    if (tid == 0) q.cnt[p] = total;
}

}  // namespace

extern "C" {

namespace {
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

size_t lg_assign_scores_workspace(int32_t m, int32_t n, int32_t batch) {
    if (m <= 0 || n <= 0 || batch <= 0) return 0;
    const size_t b = (size_t)batch, S = (size_t)assign_splits(m, n, batch);
    return up256(b * m * n * 2) + up256(b * S * m * 8) + up256(b * S * n * 8) + up256(b * m * 4) + up256(b * n * 4);
}

// lg_assign_scores' layout, then rbest [batch][CB][m] and cbest [batch][RB][n] (8 B each)
size_t lg_assign_matches_workspace(int32_t m, int32_t n, int32_t batch) {
    if (m <= 0 || n <= 0 || batch <= 0) return 0;
    const size_t b = (size_t)batch, cb = (size_t)(n + 511) / 512, rb = (size_t)(m + 31) / 32;
    return lg_assign_scores_workspace(m, n, batch) + up256(b * cb * m * 8) + up256(b * rb * n * 8);
}

namespace {
// lg_assign_matches and lg_assign_matches_lens (m_len / n_len: device tables of per-pair valid counts, or
// null = all m / n; `who` names the entry point in errors)
int32_t assign_matches_run(const char* who, const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n,
                           int32_t batch, const int32_t* m_len, const int32_t* n_len, float threshold, int32_t* matches0,
                           int32_t* matches1, float* mscores0, float* mscores1, int32_t* matches, float* mscores,
                           int32_t* counts, void* workspace, hipStream_t stream) {
    const bool work = m > 0 && n > 0 && batch > 0;
    if (m < 0 || n < 0 || batch < 0 || m > 2048 || n > 2048 || n % 8 != 0 || ld < 256 || ld % 8 != 0 || zc < 256 ||
        zc >= ld || pair_stride < (int64_t)(m + n) * ld || !(threshold >= 0.f) || !aligned4(counts) || !aligned4(m_len) ||
        !aligned4(n_len) ||
        (work && (!v || !workspace || !aligned16(v) || !aligned16(workspace) || !matches0 || !matches1 || !mscores0 ||
                  !mscores1 || !matches || !mscores || !counts || !aligned4(matches0) || !aligned4(matches1) ||
                  !aligned4(mscores0) || !aligned4(mscores1) || !aligned4(matches) || !aligned4(mscores))))
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    if (m == 0 || n == 0) {  // no rows or no columns: no match in any pair
        if (!counts) return MHA_HD64_STATUS_SUCCESS;
        const hipError_t e = hipMemsetAsync(counts, 0, (size_t)batch * 4, stream);
        return e == hipSuccess ? MHA_HD64_STATUS_SUCCESS
                               : mha_hd64::report_error(MHA_HD64_STATUS_LAUNCH_FAILED, who, hipGetErrorString(e));
    }
    AmArgs q{};
    AsArgs& a = q.a;
    a.v = (const f16*)v, a.ps = (long)pair_stride, a.ld = ld, a.zc = zc, a.m = m, a.n = n, a.rb0 = (m + 31) / 32;
    a.S = assign_splits(m, n, batch);
    a.mlen = m_len, a.nlen = n_len;
    assign_layout(a, (char*)workspace, batch);
    q.RB = (m + 31) / 32, q.CB = (n + 511) / 512, q.K = m < n ? m : n, q.thr = threshold;
    q.rbest = (float2*)((char*)workspace + lg_assign_scores_workspace(m, n, batch));
    q.cbest = (float2*)((char*)q.rbest + up256((size_t)batch * q.CB * m * 8));
    q.m0 = matches0, q.m1 = matches1, q.mt = matches, q.cnt = counts, q.s0 = mscores0, q.s1 = mscores1, q.ms = mscores;
    launch_assign_lse(a, batch, stream);
    hipLaunchKernelGGL(assign_best_kernel, dim3(q.RB, q.CB, batch), dim3(256), 0, stream, q);
    hipLaunchKernelGGL(assign_finish_kernel, dim3(batch), dim3(1024), 0, stream, q);
    return launched(who);
}
}  // namespace

int32_t lg_assign_matches(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n, int32_t batch,
                          float threshold, int32_t* matches0, int32_t* matches1, float* mscores0, float* mscores1,
                          int32_t* matches, float* mscores, int32_t* counts, void* workspace, hipStream_t stream) {
    return assign_matches_run("lg_assign_matches", v, pair_stride, ld, zc, m, n, batch, nullptr, nullptr, threshold, matches0,
                              matches1, mscores0, mscores1, matches, mscores, counts, workspace, stream);
}

int32_t lg_assign_matches_lens(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n,
                               int32_t batch, const int32_t* m_len, const int32_t* n_len, float threshold,
                               int32_t* matches0, int32_t* matches1, float* mscores0, float* mscores1, int32_t* matches,
                               float* mscores, int32_t* counts, void* workspace, hipStream_t stream) {
    return assign_matches_run("lg_assign_matches_lens", v, pair_stride, ld, zc, m, n, batch, m_len, n_len, threshold,
                              matches0, matches1, mscores0, mscores1, matches, mscores, counts, workspace, stream);
}

namespace {
int32_t assign_scores_run(const char* who, const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n,
                          int32_t batch, const int32_t* m_len, const int32_t* n_len, float* scores, void* workspace,
                          hipStream_t stream) {
    if (((uintptr_t)m_len & 3) || ((uintptr_t)n_len & 3) ||
        m < 0 || n < 0 || batch < 0 || m > 2048 || n > 2048 || n % 8 != 0 || ld < 256 || ld % 8 != 0 || zc < 256 ||
        zc >= ld || pair_stride < (int64_t)(m + n) * ld ||
        ((m > 0 && n > 0 && batch > 0) && (!v || !scores || !workspace || !aligned16(v) || !aligned16(scores) ||
                                          !aligned16(workspace))))
        return bad(who);
    if (m == 0 || n == 0 || batch == 0) return MHA_HD64_STATUS_SUCCESS;
    AsArgs a{};
    a.v = (const f16*)v, a.ps = (long)pair_stride, a.ld = ld, a.zc = zc, a.m = m, a.n = n, a.rb0 = (m + 31) / 32;
    a.S = assign_splits(m, n, batch);
    a.mlen = m_len, a.nlen = n_len;
    assign_layout(a, (char*)workspace, batch);
    a.scores = scores;
    launch_assign_lse(a, batch, stream);
    // combine (with the row / column closes): blocks of 8 W rows x 512 columns (W = 4: 32 rows; 1 where
    // that leaves the chip idle)
    const int cb = (n + 511) / 512;
    if ((long)((m + 31) / 32) * cb * batch >= 128)
        hipLaunchKernelGGL(assign_combine_kernel<4>, dim3((m + 31) / 32, cb, batch), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(assign_combine_kernel<1>, dim3((m + 7) / 8, cb, batch), dim3(256), 0, stream, a);
    return launched(who);
}
}  // namespace

int32_t lg_assign_scores(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n, int32_t batch,
                         float* scores, void* workspace, hipStream_t stream) {
    return assign_scores_run("lg_assign_scores", v, pair_stride, ld, zc, m, n, batch, nullptr, nullptr, scores, workspace,
                             stream);
}

int32_t lg_assign_scores_lens(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n, int32_t batch,
                              const int32_t* m_len, const int32_t* n_len, float* scores, void* workspace,
                              hipStream_t stream) {
    return assign_scores_run("lg_assign_scores_lens", v, pair_stride, ld, zc, m, n, batch, m_len, n_len, scores, workspace,
                             stream);
}

}  // extern "C"
