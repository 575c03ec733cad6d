// lightglue_assign_nll.hip — the matcher's training loss and its gradient on gfx950
// (include/lightglue_glue.h: lg_assign_nll). fp16 v in, fp32 loss per pair and fp32 dL/dv out.
//
// Per pair, with sim = fp16(m0 · m1ᵀ) (the similarity lg_assign_scores uses), Lr / Lc its row / column
// logsumexps over the valid block, W[i][j] = [gt0[i] == j], r = W·1, c = Wᵀ·1:
//   loss = -0.5/Pn Σ_pos (2 sim - Lr[i] - Lc[j] + logsig(z0[i]) + logsig(z1[j]))
//          -0.5/Nn (Σ_{gt0 == -1} logsig(-z0[i]) + Σ_{gt1 == -1} logsig(-z1[j]))
//   G[i][j] = r[i] exp(sim - Lr[i]) + c[j] exp(sim - Lc[j]) - 2 W[i][j]
//   dm0 = (0.5/Pn) G · m1,   dm1 = (0.5/Pn) Gᵀ · m0,   dz from r, c and the negatives.
// Launches:
//  1. assign_lse_kernel (lightglue_assign_device.h), unchanged: fp16 sim and the (max, sum) partials.
//  2. assign_nll_terms_kernel, one workgroup per pair: closes Lr and Lc, counts Pn, Nn and c (an integer
//     LDS count), sums the loss in a fixed order and leaves one float4 (L, count, gt0, dz) per row and
//     column plus 0.5/Pn for the gradient.
//  3. assign_nll_grad_kernel, the hot path. A workgroup of 2 waves owns 64 rows of ONE image (a wave 32,
//     one per lane) and all 256 channels of their gradient in 8 fp32 32x32 accumulators per wave; the OTHER
//     image streams past in tiles of 32 rows x 256 channels (register-staged, two LDS stages, one barrier
//     per tile). Per tile and 16-row k-step a lane forms 8 entries of G from sim with two exponentials
//     each, rounds them unscaled to fp16 and has them as the B operand of 8 MFMAs (v_mfma_f32_32x32x16_f16)
//     whose A operand is the streamed tile transposed, channel on the lane: ds_read_b64_tr_b16 on the
//     row-major tile. The contraction runs over the streamed rows, so G needs 8 consecutive streamed rows
//     per lane: row-owning workgroups read exactly that from sim with one 16-B load per k-step (8 columns
//     of the lane's row); column-owning workgroups stage the 32 x 64 sim tile in LDS and take it by the same
//     transposing read. With a split of the streamed image (G > 1) the unscaled fp32 partials go to the
//     workspace and assign_nll_reduce_kernel adds them in split order.
// No atomics on floats, no exchange between workgroups inside a launch: a call is bitwise reproducible.
#include "lightglue_assign_device.h"

#include <algorithm>
#include <cstdlib>

namespace {

struct NlArgs {
    AsArgs a;
    const int* gt0;   // [batch][m]
    const int* gt1;   // [batch][n]
    float* loss;      // [batch]
    float* dv;        // [batch][m + n][ld] fp32 (null: loss only)
    f32x4* coef;      // workspace [batch][m + n]: rows (Lr, r, gt0 as bits, dz0), columns (Lc, c, -, dz1)
    float* scal;      // workspace [batch]: 0.5 / Pn
    float* part;      // workspace [G][batch][m + n][256] fp32 (G > 1)
    int G, rb64, batch;
};

__device__ __forceinline__ int block_sum(int x, int* red, int tid) {  // (1024 threads; ends in a barrier)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    __syncthreads();  // (red free again)
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    return t;
}
// sum over the block in a fixed order: a wave tree, then the waves in order
__device__ __forceinline__ double block_sum(double x, double* red, int tid) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = x;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) t += red[w];
    return t;
}
// (σ(z), σ(-z)); expf, not the fast form: dz is compared at fp32 precision and this is off the hot path
__device__ __forceinline__ float2 sigmoid_pair(float z) {
    const float e = expf(-fabsf(z)), hi = 1.f / (1.f + e), lo = e / (1.f + e);
    return z >= 0.f ? make_float2(hi, lo) : make_float2(lo, hi);
}

__global__ __launch_bounds__(1024) void assign_nll_terms_kernel(NlArgs q) {
    const AsArgs& a = q.a;
    __shared__ int cnt[2048];
    __shared__ float cterm[2048];  // logsig(z1[j]) - Lc[j]
    __shared__ int ired[16];
    __shared__ double dred[16];
    const int p = blockIdx.x, tid = threadIdx.x, m = a.m, n = a.n;
    const int ml = assign_len(a.mlen, p, m), nl = assign_len(a.nlen, p, n);
    const f16* const vp = a.v + (size_t)p * a.ps;
    const int* const g0 = q.gt0 + (size_t)p * m;
    const int* const g1 = q.gt1 + (size_t)p * n;
    f32x4* const coef = q.coef + (size_t)p * (m + n);
    for (int j = tid; j < n; j += 1024) cnt[j] = 0;
    __syncthreads();
    int np = 0, nn = 0;
    for (int i = tid; i < ml; i += 1024) {
        const int g = g0[i];
        if (g >= 0 && g < nl) atomicAdd(&cnt[g], 1), ++np;
        else if (g == -1) ++nn;
    }
    for (int j = tid; j < nl; j += 1024) nn += g1[j] == -1;
    np = block_sum(np, ired, tid);
    nn = block_sum(nn, ired, tid);  // (its barriers: cnt complete)
    const float wp = 0.5f / (float)max(np, 1), wn = 0.5f / (float)max(nn, 1);
    double spos = 0.0, sneg = 0.0;
    for (int j = tid; j < n; j += 1024) {
        f32x4 c4 = {0.f, 0.f, 0.f, 0.f};
        if (j < nl) {
            const float z = (float)vp[(size_t)(m + j) * a.ld + a.zc];
            const float L = lse_close(a.cpart + (size_t)p * a.S * n + j, n, a.S);
            const float c = (float)cnt[j];
            const bool neg = g1[j] == -1;
            const float2 sg = sigmoid_pair(z);
            cterm[j] = log_sigmoid_f(z) - L;
            if (neg) sneg += (double)log_sigmoid_f(-z);
            c4 = f32x4{L, c, 0.f, -wp * c * sg.y + (neg ? wn * sg.x : 0.f)};
        }
        coef[m + j] = c4;
    }
    __syncthreads();
    for (int i = tid; i < m; i += 1024) {
        f32x4 c4 = {0.f, 0.f, __int_as_float(-2), 0.f};
        if (i < ml) {
            const int g = g0[i];
            const bool pos = g >= 0 && g < nl, neg = g == -1;
            const float z = (float)vp[(size_t)i * a.ld + a.zc];
            const float L = lse_close(a.rpart + (size_t)p * a.S * m + i, m, a.S);
            const float2 sg = sigmoid_pair(z);
            if (pos) {
                const float s = (float)a.sim[((size_t)p * m + i) * n + g];
                spos += (double)(2.f * s + (log_sigmoid_f(z) - L) + cterm[g]);
            }
            if (neg) sneg += (double)log_sigmoid_f(-z);
            c4 = f32x4{L, pos ? 1.f : 0.f, __int_as_float(g), (pos ? -wp * sg.y : 0.f) + (neg ? wn * sg.x : 0.f)};
        }
        coef[i] = c4;
    }
    spos = block_sum(spos, dred, tid);
    sneg = block_sum(sneg, dred, tid);
    if (tid == 0) {
        q.loss[p] = (float)(-(double)wp * spos - (double)wn * sneg);
        q.scal[p] = wp;
    }
}

// channels 256..ld-1 of one dv row: zeros, dz at zc; quads qd0, qd0 + step, ...
__device__ __forceinline__ void nll_tail(float* row, int ld, int zc, float dz, int qd0, int step) {
    for (int qd = 64 + qd0; qd < ld / 4; qd += step) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
        if (qd == zc >> 2) o[zc & 3] = dz;
        *reinterpret_cast<f32x4*>(row + 4 * qd) = o;
    }
}

typedef __attribute__((address_space(3))) f32x4 lds_f32x4;
constexpr int kNlV = 0;                  // the streamed tile [32 rows][512 B], 64-B blocks XOR (row & 3)
constexpr int kNlCoef = 32 * 512;        // [32] float4
constexpr int kNlSim = kNlCoef + 512;    // (column side) sim tile [32 rows][128 B], 64-B halves XOR (row >> 1) & 1
constexpr int kNlStage = kNlSim + 32 * 128;

template <int SIDE>  // 0: owns rows of image 0 (dm0), image 1 streamed; 1: owns columns (dm1), image 0 streamed
__device__ __forceinline__ void nll_grad_body(const NlArgs& q, lds_char* lds) {
    const AsArgs& a = q.a;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int qq = (lane & 15) >> 2, pp = lane & 3, gh = (lane >> 4) & 1;
    const int p = blockIdx.y, sp = blockIdx.z, m = a.m, n = a.n;
    const int o0 = (SIDE ? (int)blockIdx.x - q.rb64 : (int)blockIdx.x) * 64;
    const int ml = assign_len(a.mlen, p, m), nl = assign_len(a.nlen, p, n);
    const int nown = SIDE ? nl : ml, noth = SIDE ? ml : nl, fown = SIDE ? n : m, foth = SIDE ? m : n;
    const int base_own = SIDE ? m : 0, base_oth = SIDE ? 0 : m;
    const f16* const voth = a.v + (size_t)p * a.ps + (size_t)base_oth * a.ld;
    const f16* const sim = a.sim + (size_t)p * m * n;
    const f32x4* const coef = q.coef + (size_t)p * (m + n);

    const int own = o0 + 32 * wave + r;
    const bool own_ok = own < nown;
    const int ownc = min(own, nown - 1);
    const f32x4 co = coef[base_own + ownc];
    const float Lo = co[0], cno = co[1];
    const int gto = __float_as_int(co[2]);

    // this split's tiles of the streamed image (none for a workgroup wholly in padding)
    const int tps = ((foth + 31) / 32 + q.G - 1) / q.G;
    const int t_begin = sp * tps;
    const int t_end = o0 < nown ? min(t_begin + tps, (noth + 31) / 32) : t_begin;

    // The stream: tile t + 1 into registers while tile t is computed from LDS, written to the other stage
    // after it. Every row index is clamped into the valid block: no padded row of v or sim is read.
    f16x8 vst[8], sst[2];
    f32x4 cst;
    auto issue = [&](int t) {
        const int R0 = 32 * t;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int u = i * 128 + tid, row = u >> 5, un = u & 31;
            vst[i] = *reinterpret_cast<const f16x8*>(voth + (size_t)min(R0 + row, noth - 1) * a.ld + un * 8);
        }
        if (tid < 32) cst = coef[base_oth + min(R0 + tid, noth - 1)];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            sst[i] = f16x8{};
            if constexpr (SIDE) {  // sim[R0 + row][o0 + 8 un ..]
                const int u = i * 128 + tid, row = u >> 3, j = o0 + 8 * (u & 7);
                if (j < n) sst[i] = *reinterpret_cast<const f16x8*>(sim + (size_t)min(R0 + row, ml - 1) * n + j);
            } else {  // this lane's 8 columns of k-step i of its own row
                const int j = R0 + 16 * i + 8 * hh;
                if (j < n) sst[i] = *reinterpret_cast<const f16x8*>(sim + (size_t)ownc * n + j);
            }
        }
    };
    auto write = [&](unsigned base) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int u = i * 128 + tid, row = u >> 5, un = u & 31;
            *(lds_f16x8*)(lds + base + kNlV + row * 512 + ((((un >> 2) ^ (row & 3)) << 6) | ((un & 3) << 4))) = vst[i];
        }
        if (tid < 32) *(lds_f32x4*)(lds + base + kNlCoef + 16 * tid) = cst;
        if constexpr (SIDE) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int u = i * 128 + tid, row = u >> 3, un = u & 7;
                *(lds_f16x8*)(lds + base + kNlSim + row * 128 + ((16 * un) ^ (((row >> 1) & 1) << 6))) = sst[i];
            }
        }
    };

    f32x16 acc[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[b] = f32x16{};

    issue(t_begin);
    write(0);
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
        const unsigned base = ((t - t_begin) & 1) * kNlStage;
        const f16x8 sd0 = sst[0], sd1 = sst[1];  // (row side: tile t's entries of sim)
        issue(t + 1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int rq = 16 * ks + 8 * hh + qq;  // this lane's source row of the transposing reads
            f16x8 s8;
            if constexpr (SIDE) {
                const unsigned at = base + kNlSim + rq * 128 + ((64 * wave + 32 * gh + 8 * pp) ^ (((qq >> 1) & 1) << 6));
                s8 = mha_hd64::cat8(mha_hd64::tr_read(lds, at), mha_hd64::tr_read(lds, at + 4 * 128));
            } else {
                s8 = ks ? sd1 : sd0;
            }
            // entry e: streamed row (column) 32 t + 16 ks + 8 hh + e against this lane's own row
            f16x8 g8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int idx = 16 * ks + 8 * hh + e, sidx = 32 * t + idx;
                const f32x4 cf = *(lds_f32x4*)(lds + base + kNlCoef + 16 * idx);
                const float s = (float)s8[e];
                const float to = cno * __expf(s - Lo), ts = cf[1] * __expf(s - cf[0]);
                const bool hit = SIDE ? __float_as_int(cf[2]) == own : gto == sidx;
                const float g = (SIDE ? ts + to : to + ts) - (hit ? 2.f : 0.f);
                g8[e] = (f16)((own_ok && sidx < noth) ? g : 0.f);
            }
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const unsigned at = base + kNlV + rq * 512 + ((b ^ qq) << 6) + 32 * gh + 8 * pp;
                const f16x8 af = mha_hd64::cat8(mha_hd64::tr_read(lds, at), mha_hd64::tr_read(lds, at + 4 * 512));
                acc[b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af, g8, acc[b], 0, 0, 0);
            }
        }
        write(kNlStage - base);
        __syncthreads();
    }

    // lane (own row, hh): acc[b][4 g + e] = channel 32 b + 8 g + 4 hh + e
    if (own >= fown) return;
    if (q.G == 1) {
        const float sc = q.scal[p];
        float* const row = q.dv + ((size_t)p * (m + n) + base_own + own) * a.ld;
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<f32x4*>(row + 32 * b + 8 * g + 4 * hh) =
                    f32x4{acc[b][4 * g] * sc, acc[b][4 * g + 1] * sc, acc[b][4 * g + 2] * sc, acc[b][4 * g + 3] * sc};
        nll_tail(row, a.ld, a.zc, own_ok ? co[3] : 0.f, hh, 2);
    } else {
        float* const row = q.part + (((size_t)sp * q.batch + p) * (m + n) + base_own + own) * 256;
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<f32x4*>(row + 32 * b + 8 * g + 4 * hh) =
                    f32x4{acc[b][4 * g], acc[b][4 * g + 1], acc[b][4 * g + 2], acc[b][4 * g + 3]};
    }
}

__global__ __launch_bounds__(128) void assign_nll_grad_kernel(NlArgs q) {
    __shared__ __attribute__((aligned(16))) char smem[2 * kNlStage];
    if ((int)blockIdx.x >= q.rb64) nll_grad_body<1>(q, (lds_char*)smem);
    else nll_grad_body<0>(q, (lds_char*)smem);
}

// dv rows from the G partials, added in split order and scaled; a thread = 4 channels of a row
// (grid: ((m + n) ld / 4 / 256, batch)); padded rows and the channels past 255 as nll_tail writes them
__global__ __launch_bounds__(256) void assign_nll_reduce_kernel(NlArgs q) {
    const AsArgs& a = q.a;
    const int p = blockIdx.y, rows = a.m + a.n, qpr = a.ld / 4;
    const int at = blockIdx.x * 256 + threadIdx.x;
    if (at >= rows * qpr) return;
    const int row = at / qpr, qd = at - row * qpr;
    const int ml = assign_len(a.mlen, p, a.m), nl = assign_len(a.nlen, p, a.n);
    const bool ok = row < a.m ? row < ml : row - a.m < nl;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (qd >= 64) {
        if (qd == a.zc >> 2) o[a.zc & 3] = q.coef[(size_t)p * rows + row][3];
    } else if (ok) {
        const size_t split = (size_t)q.batch * rows * 256;
        const float* src = q.part + ((size_t)p * rows + row) * 256 + 4 * qd;
        for (int s = 0; s < q.G; ++s) o += *reinterpret_cast<const f32x4*>(src + s * split);
        o *= q.scal[p];
    }
    *reinterpret_cast<f32x4*>(q.dv + ((size_t)p * rows + row) * a.ld + 4 * qd) = o;
}

// The gradient kernel's split of the streamed image: while its 64-row workgroups number at most half a
// round of the chip, the streamed tiles are dealt to up to 8 splits (the timings behind it).
int nll_splits(int32_t m, int32_t n, int32_t batch) {
    const long base = (long)((m + 63) / 64 + (n + 63) / 64) * batch;
    int G = 1;
    while (G < 8 && base * G * 2 <= 256) G *= 2;
    // measurement hook (tools/assign_nll_ab.py): LG_ASSIGN_NLL_SPLITS=g forces g splits
    if (const char* e = std::getenv("LG_ASSIGN_NLL_SPLITS"))
        if (std::atoi(e) >= 1) G = std::min(std::atoi(e), 8);
    const int tiles = ((m > n ? m : n) + 31) / 32;
    return G < tiles ? G : tiles;
}

}  // namespace

extern "C" {

// lg_assign_scores' layout, then coef [batch][m + n] float4, 0.5 / Pn [batch] and the split partials
size_t lg_assign_nll_workspace(int32_t m, int32_t n, int32_t batch) {
    if (m <= 0 || n <= 0 || batch <= 0) return 0;
    const size_t b = (size_t)batch, rows = (size_t)m + n, G = (size_t)nll_splits(m, n, batch);
    return lg_assign_scores_workspace(m, n, batch) + up256(b * rows * 16) + up256(b * 4) +
           (G > 1 ? G * b * rows * 256 * 4 : 0);
}

int32_t lg_assign_nll(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m, int32_t n, int32_t batch,
                      const int32_t* m_len, const int32_t* n_len, const int32_t* gt0, const int32_t* gt1, float* loss,
                      float* dv, void* workspace, hipStream_t stream) {
    const char* const who = "lg_assign_nll";
    if (m < 1 || n < 1 || batch < 0 || batch > 65535 || m > 2048 || n > 2048 || n % 8 != 0 || ld < 256 || ld % 8 != 0 ||
        zc < 256 || zc >= ld || pair_stride < (int64_t)(m + n) * ld || !aligned4(m_len) || !aligned4(n_len) ||
        (batch > 0 && (!v || !workspace || !gt0 || !gt1 || !loss || !aligned16(v) || !aligned16(workspace) ||
                       !aligned16(dv) || !aligned4(gt0) || !aligned4(gt1) || !aligned4(loss))))
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    NlArgs q{};
    AsArgs& a = q.a;
    a.v = (const f16*)v, a.ps = (long)pair_stride, a.ld = ld, a.zc = zc, a.m = m, a.n = n, a.rb0 = (m + 31) / 32;
    a.S = assign_splits(m, n, batch);
    a.mlen = m_len, a.nlen = n_len;
    assign_layout(a, (char*)workspace, batch);
    q.gt0 = gt0, q.gt1 = gt1, q.loss = loss, q.dv = dv, q.batch = batch;
    q.G = nll_splits(m, n, batch), q.rb64 = (m + 63) / 64;
    q.coef = (f32x4*)((char*)workspace + lg_assign_scores_workspace(m, n, batch));
    q.scal = (float*)((char*)q.coef + up256((size_t)batch * (m + n) * 16));
    q.part = (float*)((char*)q.scal + up256((size_t)batch * 4));
    launch_assign_lse(a, batch, stream);
    hipLaunchKernelGGL(assign_nll_terms_kernel, dim3(batch), dim3(1024), 0, stream, q);
    if (dv) {
        hipLaunchKernelGGL(assign_nll_grad_kernel, dim3(q.rb64 + (n + 63) / 64, batch, q.G), dim3(128), 0, stream, q);
        if (q.G > 1)
            hipLaunchKernelGGL(assign_nll_reduce_kernel, dim3(((m + n) * (ld / 4) + 255) / 256, batch), dim3(256), 0, stream,
                               q);
    }
    return launched(who);
}

}  // extern "C"
