// lightglue_adaptive.hip — adaptive depth and width for the fp16 matcher (include/lightglue_glue.h):
// lg_token_scores (per-row token confidence and matchability, the keep flags and the per-pair counts the
// host decides on), lg_compact_rows (the stable gather of the kept rows of x / cos / sin and of the
// running index maps) and lg_matches_scatter (the surviving rows' MatchResult back in original index
// space). Bandwidth kernels: a row of x is 512 B = 32 lanes x 16 B, so a wave reads two rows per load;
// counters are integer LDS / global vector atomics (order-independent: bitwise reproducible).
#include "lightglue_device.h"

namespace {

constexpr int kTile = 64;        // rows per workgroup (256 threads)
constexpr int kMaxRows = 2048;   // lg_matches_scatter's inverse map in LDS (the heads' limit)

// a pair's valid rows of one image: the table's value clamped into [1, limit] (every lens form's rule)
__device__ __forceinline__ int seg_len(const int32_t* tab, int p, int limit) {
    return tab ? min(max(tab[p], 1), limit) : limit;
}

__device__ __forceinline__ float sigmoid32(float z) { return 1.f / (1.f + expf(-z)); }

struct TsArgs {
    const f16* x;
    const int32_t* mlen;
    const int32_t* nlen;
    const f16* wtok;
    const f16* btok;
    const f16* wmat;
    const f16* bmat;
    float tconf, tkeep;
    int flags, m, n, tiles0;
    float* conf;
    float* mtch;
    uint8_t* keep;
    int32_t* stats;
};

// grid (tiles of image 0 + tiles of image 1, pairs); wave w takes rows 16 w .. 16 w + 15 of the tile,
// two at a time (lanes 0..31 / 32..63, lane % 32 = the row's 16-B unit)
__global__ __launch_bounds__(256) void token_scores_kernel(const TsArgs a) {
    __shared__ int cnt[3];  // kept, unconfident, valid of this tile
    const int tid = threadIdx.x, p = blockIdx.y;
    const bool first = (int)blockIdx.x < a.tiles0;
    const int tile = first ? blockIdx.x : blockIdx.x - a.tiles0;
    const int dim = first ? a.m : a.n;
    const int len = seg_len(first ? a.mlen : a.nlen, p, dim);
    const size_t seg = (size_t)p * (a.m + a.n) + (first ? 0 : a.m);
    const bool width = (a.flags & (first ? LG_ADAPT_WIDTH0 : LG_ADAPT_WIDTH1)) != 0;
    const bool depth = (a.flags & LG_ADAPT_DEPTH) != 0;
    const int lane = tid & 63, wave = tid >> 6, unit = lane & 31, sub = lane >> 5;
    if (tid < 3) cnt[tid] = 0;
    __syncthreads();
    const f16x8 wt = *reinterpret_cast<const f16x8*>(a.wtok + unit * 8);
    const f16x8 wm = *reinterpret_cast<const f16x8*>(a.wmat + unit * 8);
    const float bt = (float)a.btok[0], bm = (float)a.bmat[0];
    int kept = 0, unc = 0, valid = 0;
#pragma unroll 2
    for (int it = 0; it < 8; ++it) {
        const int r = tile * kTile + wave * 16 + it * 2 + sub;
        float c = 0.f, t = 0.f;
        if (r < len) {  // (rows past the count are never read)
            const f16x8 xv = *reinterpret_cast<const f16x8*>(a.x + (seg + r) * 256 + unit * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                c = fmaf((float)xv[e], (float)wt[e], c);
                t = fmaf((float)xv[e], (float)wm[e], t);
            }
        }
#pragma unroll
        for (int s = 16; s >= 1; s >>= 1) {  // the 32 lanes of a row (the xor stays inside its half)
            c += __shfl_xor(c, s);
            t += __shfl_xor(t, s);
        }
        if (unit == 0 && r < dim) {
            float cf = 0.f, mt = 0.f;
            bool k = false;
            if (r < len) {
                cf = sigmoid32(c + bt), mt = sigmoid32(t + bm);
                k = !width || mt > a.tkeep || (depth && cf <= a.tconf);
                kept += k, unc += cf < a.tconf, ++valid;
            }
            a.conf[seg + r] = cf, a.mtch[seg + r] = mt, a.keep[seg + r] = k;
        }
    }
    if (unit == 0 && valid) {
        atomicAdd(&cnt[0], kept);
        atomicAdd(&cnt[1], unc);
        atomicAdd(&cnt[2], valid);
    }
    __syncthreads();
    if (tid == 0 && cnt[0]) atomicAdd(a.stats + p * 4 + (first ? 0 : 1), cnt[0]);
    if (tid == 1 && cnt[1]) atomicAdd(a.stats + p * 4 + 2, cnt[1]);
    if (tid == 2 && cnt[2]) atomicAdd(a.stats + p * 4 + 3, cnt[2]);
}

// The min-one rule: a pruned segment that kept no row keeps its row of highest matchability (the lowest
// index on ties). grid (2, pairs); reads the counts token_scores_kernel left.
__global__ __launch_bounds__(256) void token_min_one_kernel(const TsArgs a) {
    __shared__ float bv[256];
    __shared__ int bi[256];
    const int tid = threadIdx.x, p = blockIdx.y;
    const bool first = blockIdx.x == 0;
    if (!(a.flags & (first ? LG_ADAPT_WIDTH0 : LG_ADAPT_WIDTH1))) return;
    int32_t* kept = a.stats + p * 4 + (first ? 0 : 1);
    if (*kept != 0) return;  // (uniform over the workgroup)
    const int dim = first ? a.m : a.n;
    const int len = seg_len(first ? a.mlen : a.nlen, p, dim);
    const size_t seg = (size_t)p * (a.m + a.n) + (first ? 0 : a.m);
    float v = -1.f;  // (a sigmoid is >= 0)
    int idx = 0x7fffffff;
    for (int r = tid; r < len; r += 256) {
        const float t = a.mtch[seg + r];
        if (t > v) v = t, idx = r;  // (ascending r: the first of equal values stays)
    }
    bv[tid] = v, bi[tid] = idx;
    __syncthreads();
    for (int s = 128; s >= 1; s >>= 1) {
        if (tid < s) {
            const float ov = bv[tid + s];
            const int oi = bi[tid + s];
            if (ov > bv[tid] || (ov == bv[tid] && oi < bi[tid])) bv[tid] = ov, bi[tid] = oi;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int r = bi[0] < len ? bi[0] : 0;
        a.keep[seg + r] = 1;
        *kept = 1;
    }
}

struct CpArgs {
    const f16* x;
    const f16* cosv;
    const f16* sinv;
    const uint8_t* keep;
    const int32_t* ind0;
    const int32_t* ind1;
    const int32_t* mlen;
    const int32_t* nlen;
    int m, n, mo, no, tiles0;
    f16* xo;
    f16* coso;
    f16* sino;
    int32_t* ind0o;
    int32_t* ind1o;
    int32_t* mleno;
    int32_t* nleno;
    int32_t* prune0;
    int32_t* prune1;
    int pm, pn, layers;
};

// grid (tiles of image 0 + tiles of image 1, pairs): a workgroup counts its segment's flags before its
// tile (the tile's first destination row), ranks its own 64 flags by a ballot, then copies the kept rows
// 16 B a lane (x: units 0..31, cos: 32..39, sin: 40..47 of a 64-lane group, four rows per pass).
__global__ __launch_bounds__(256) void compact_rows_kernel(const CpArgs a) {
    __shared__ int before, here;
    __shared__ int dest[kTile];
    const int tid = threadIdx.x, p = blockIdx.y;
    const bool first = (int)blockIdx.x < a.tiles0;
    const int tile = first ? blockIdx.x : blockIdx.x - a.tiles0;
    const int dim = first ? a.m : a.n, dimo = first ? a.mo : a.no;
    const int len = seg_len(first ? a.mlen : a.nlen, p, dim);
    const int r0 = tile * kTile;
    if (r0 >= len) return;  // (no valid row: nothing kept, no count to write)
    const size_t seg = (size_t)p * (a.m + a.n) + (first ? 0 : a.m);
    const size_t sego = (size_t)p * (a.mo + a.no) + (first ? 0 : a.mo);
    const uint8_t* flag = a.keep + seg;
    const int32_t* ind = first ? a.ind0 : a.ind1;
    if (tid == 0) before = 0;
    __syncthreads();
    int c = 0;
    for (int r = tid; r < r0; r += 256) c += flag[r] != 0;  // (r0 < len)
    if (c) atomicAdd(&before, c);
    __syncthreads();
    if (tid < kTile) {
        const int r = r0 + tid;
        const bool f = r < len && flag[r] != 0;
        const unsigned long long mask = __ballot(f);
        const int d = before + __popcll(mask & ((1ull << tid) - 1ull));
        dest[tid] = f && d < dimo ? d : -1;
        if (r < len) {
            const int orig = ind ? ind[(size_t)p * dim + r] : r;
            if (f && d < dimo) (first ? a.ind0o : a.ind1o)[(size_t)p * dimo + d] = orig;
            int32_t* prune = first ? a.prune0 : a.prune1;
            const int pd = first ? a.pm : a.pn;
            if (!f && prune && orig >= 0 && orig < pd) prune[(size_t)p * pd + orig] = a.layers;
        }
        if (tid == 0) here = __popcll(mask);
    }
    __syncthreads();
    if (tid == 0 && len - 1 < r0 + kTile)  // the segment's last tile knows its total
        (first ? a.mleno : a.nleno)[p] = min(before + here, dimo);
    const int u = tid & 63;
    if (u >= 48) return;
#pragma unroll 4
    for (int it = 0; it < kTile / 4; ++it) {
        const int rr = it * 4 + (tid >> 6);
        const int d = dest[rr];
        if (d < 0) continue;
        const size_t src = seg + r0 + rr, dst = sego + d;
        if (u < 32)
            reinterpret_cast<uint4*>(a.xo)[dst * 32 + u] = reinterpret_cast<const uint4*>(a.x)[src * 32 + u];
        else if (u < 40)
            reinterpret_cast<uint4*>(a.coso)[dst * 8 + (u - 32)] = reinterpret_cast<const uint4*>(a.cosv)[src * 8 + (u - 32)];
        else
            reinterpret_cast<uint4*>(a.sino)[dst * 8 + (u - 40)] = reinterpret_cast<const uint4*>(a.sinv)[src * 8 + (u - 40)];
    }
}

struct ScArgs {
    const int32_t* m0;
    const int32_t* m1;
    const float* s0;
    const float* s1;
    const int32_t* mt;
    const float* ms;
    const int32_t* cnt;
    const int32_t* ind0;
    const int32_t* ind1;
    const int32_t* mlen;
    const int32_t* nlen;
    int mc, nc, m, n, stop;
    int32_t* om0;
    int32_t* om1;
    float* os0;
    float* os1;
    int32_t* omt;
    float* oms;
    int32_t* ocnt;
    int32_t* prune0;
    int32_t* prune1;
};

// current row / column index -> original, or -1 outside either range
__device__ __forceinline__ int to_orig(const int32_t* ind, size_t base, int j, int cur, int orig_dim) {
    if (j < 0 || j >= cur) return -1;
    const int o = ind ? ind[base + j] : j;
    return o >= 0 && o < orig_dim ? o : -1;
}

// grid (3, pairs): x = 0 / 1 the dense outputs of image 0 / 1 (an inverse map original -> surviving row in
// LDS, so every output element is written once), x = 2 the list and its count
__global__ __launch_bounds__(256) void matches_scatter_kernel(const ScArgs a) {
    __shared__ int inv[kMaxRows];
    const int tid = threadIdx.x, p = blockIdx.y;
    if (blockIdx.x == 2) {
        const int K = min(a.m, a.n), kc = min(a.mc, a.nc);
        const int c = min(max(a.cnt[p], 0), kc);
        for (int k = tid; k < K; k += 256) {
            int i = -1, j = -1;
            float s = 0.f;
            if (k < c) {
                i = to_orig(a.ind0, (size_t)p * a.mc, a.mt[((size_t)p * kc + k) * 2], a.mc, a.m);
                j = to_orig(a.ind1, (size_t)p * a.nc, a.mt[((size_t)p * kc + k) * 2 + 1], a.nc, a.n);
                s = a.ms[(size_t)p * kc + k];
            }
            a.omt[((size_t)p * K + k) * 2] = i, a.omt[((size_t)p * K + k) * 2 + 1] = j, a.oms[(size_t)p * K + k] = s;
        }
        if (tid == 0) a.ocnt[p] = c;
        return;
    }
    const bool first = blockIdx.x == 0;
    const int dim = first ? a.m : a.n, cur = first ? a.mc : a.nc;
    const int odim = first ? a.n : a.m, ocur = first ? a.nc : a.mc;
    const int len = seg_len(first ? a.mlen : a.nlen, p, cur);
    const int32_t* ind = first ? a.ind0 : a.ind1;
    const int32_t* oind = first ? a.ind1 : a.ind0;
    const int32_t* mi = (first ? a.m0 : a.m1) + (size_t)p * cur;
    const float* si = (first ? a.s0 : a.s1) + (size_t)p * cur;
    int32_t* om = (first ? a.om0 : a.om1) + (size_t)p * dim;
    float* os = (first ? a.os0 : a.os1) + (size_t)p * dim;
    int32_t* prune = first ? a.prune0 : a.prune1;
    for (int o = tid; o < dim; o += 256) inv[o] = -1;
    __syncthreads();
    for (int r = tid; r < len; r += 256) {
        const int o = to_orig(ind, (size_t)p * cur, r, cur, dim);
        if (o >= 0) inv[o] = r;
    }
    __syncthreads();
    for (int o = tid; o < dim; o += 256) {
        const int r = inv[o];
        int mm = -1;
        float ss = 0.f;
        if (r >= 0) {
            mm = to_orig(oind, (size_t)p * ocur, mi[r], ocur, odim);
            ss = si[r];
            if (prune) prune[(size_t)p * dim + o] = a.stop;
        }
        om[o] = mm, os[o] = ss;
    }
}

// pairs of (m + n) rows: grid y and 32-bit row counts
bool rows_ok(int32_t m, int32_t n, int32_t pairs) {
    return m >= 1 && n >= 1 && pairs >= 0 && pairs <= 65535 && (int64_t)pairs * ((int64_t)m + n) <= (1 << 24);
}

}  // namespace

extern "C" {

int32_t lg_token_scores(const void* x, int32_t m, int32_t n, int32_t pairs, const int32_t* m_len, const int32_t* n_len,
                        const void* w_tok, const void* b_tok, const void* w_match, const void* b_match, float t_conf,
                        float t_keep, int32_t flags, float* conf, float* mtch, uint8_t* keep, int32_t* stats,
                        hipStream_t stream) {
    const char* who = "lg_token_scores";
    if (!rows_ok(m, n, pairs) || !(t_conf >= 0.f && t_conf <= 1.f) || !(t_keep == t_keep) || flags < 0 ||
        flags > (LG_ADAPT_DEPTH | LG_ADAPT_WIDTH0 | LG_ADAPT_WIDTH1) || !aligned4(m_len) || !aligned4(n_len) || !x ||
        !aligned16(x) || !w_tok || !aligned16(w_tok) || !w_match || !aligned16(w_match) || !b_tok || !aligned2(b_tok) ||
        !b_match || !aligned2(b_match) || !conf || !aligned4(conf) || !mtch || !aligned4(mtch) || !keep || !stats ||
        !aligned4(stats))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    const hipError_t e = hipMemsetAsync(stats, 0, (size_t)pairs * 16, stream);
    if (e != hipSuccess) return mha_hd64::report_error(MHA_HD64_STATUS_LAUNCH_FAILED, who, hipGetErrorString(e));
    TsArgs a{};
    a.x = (const f16*)x, a.mlen = m_len, a.nlen = n_len;
    a.wtok = (const f16*)w_tok, a.btok = (const f16*)b_tok, a.wmat = (const f16*)w_match, a.bmat = (const f16*)b_match;
    a.tconf = t_conf, a.tkeep = t_keep, a.flags = flags, a.m = m, a.n = n, a.tiles0 = (m + kTile - 1) / kTile;
    a.conf = conf, a.mtch = mtch, a.keep = keep, a.stats = stats;
    hipLaunchKernelGGL(token_scores_kernel, dim3(a.tiles0 + (n + kTile - 1) / kTile, pairs), dim3(256), 0, stream, a);
    if (flags & (LG_ADAPT_WIDTH0 | LG_ADAPT_WIDTH1))
        hipLaunchKernelGGL(token_min_one_kernel, dim3(2, pairs), dim3(256), 0, stream, a);
    return launched(who);
}

int32_t lg_compact_rows(const void* x, const void* cosv, const void* sinv, const uint8_t* keep, const int32_t* ind0,
                        const int32_t* ind1, int32_t m, int32_t n, int32_t pairs, const int32_t* m_len, const int32_t* n_len,
                        int32_t m_out, int32_t n_out, void* x_out, void* cos_out, void* sin_out, int32_t* ind0_out,
                        int32_t* ind1_out, int32_t* m_len_out, int32_t* n_len_out, int32_t* prune0, int32_t* prune1,
                        int32_t m_orig, int32_t n_orig, int32_t layers, hipStream_t stream) {
    const char* who = "lg_compact_rows";
    const bool pr = prune0 || prune1;
    if (!rows_ok(m, n, pairs) || m_out < 1 || n_out < 1 || m_out > m || n_out > n || !x || !cosv || !sinv || !keep ||
        !x_out || !cos_out || !sin_out || !ind0_out || !ind1_out || !m_len_out || !n_len_out || !aligned16(x) ||
        !aligned16(cosv) || !aligned16(sinv) || !aligned16(x_out) || !aligned16(cos_out) || !aligned16(sin_out) ||
        !aligned4(ind0) || !aligned4(ind1) || !aligned4(m_len) || !aligned4(n_len) || !aligned4(ind0_out) ||
        !aligned4(ind1_out) || !aligned4(m_len_out) || !aligned4(n_len_out) || !aligned4(prune0) || !aligned4(prune1) ||
        x_out == x || cos_out == cosv || sin_out == sinv || (pr && (!prune0 || !prune1 || m_orig < 1 || n_orig < 1 || layers < 1)))
        return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    CpArgs a{};
    a.x = (const f16*)x, a.cosv = (const f16*)cosv, a.sinv = (const f16*)sinv, a.keep = keep, a.ind0 = ind0, a.ind1 = ind1;
    a.mlen = m_len, a.nlen = n_len, a.m = m, a.n = n, a.mo = m_out, a.no = n_out, a.tiles0 = (m + kTile - 1) / kTile;
    a.xo = (f16*)x_out, a.coso = (f16*)cos_out, a.sino = (f16*)sin_out, a.ind0o = ind0_out, a.ind1o = ind1_out;
    a.mleno = m_len_out, a.nleno = n_len_out, a.prune0 = prune0, a.prune1 = prune1, a.pm = m_orig, a.pn = n_orig;
    a.layers = layers;
    hipLaunchKernelGGL(compact_rows_kernel, dim3(a.tiles0 + (n + kTile - 1) / kTile, pairs), dim3(256), 0, stream, a);
    return launched(who);
}

int32_t lg_matches_scatter(const int32_t* matches0, const int32_t* matches1, const float* mscores0, const float* mscores1,
                           const int32_t* matches, const float* mscores, const int32_t* counts, const int32_t* ind0,
                           const int32_t* ind1, const int32_t* m_len, const int32_t* n_len, int32_t m_cur, int32_t n_cur,
                           int32_t m, int32_t n, int32_t pairs, int32_t stop, int32_t* out_matches0, int32_t* out_matches1,
                           float* out_mscores0, float* out_mscores1, int32_t* out_matches, float* out_mscores,
                           int32_t* out_counts, int32_t* prune0, int32_t* prune1, hipStream_t stream) {
    const char* who = "lg_matches_scatter";
    const void* need[] = {matches0, matches1, mscores0, mscores1, matches, mscores, counts, out_matches0, out_matches1,
                          out_mscores0, out_mscores1, out_matches, out_mscores, out_counts};
    const void* opt[] = {ind0, ind1, m_len, n_len, prune0, prune1};
    bool ok = m_cur >= 1 && n_cur >= 1 && m_cur <= m && n_cur <= n && m <= kMaxRows && n <= kMaxRows && pairs >= 0 &&
              pairs <= 65535 && stop >= 0;
    for (const void* q : need) ok = ok && q && aligned4(q);
    for (const void* q : opt) ok = ok && aligned4(q);
    if (!ok) return bad(who);
    if (pairs == 0) return MHA_HD64_STATUS_SUCCESS;
    ScArgs a{};
    a.m0 = matches0, a.m1 = matches1, a.s0 = mscores0, a.s1 = mscores1, a.mt = matches, a.ms = mscores, a.cnt = counts;
    a.ind0 = ind0, a.ind1 = ind1, a.mlen = m_len, a.nlen = n_len, a.mc = m_cur, a.nc = n_cur, a.m = m, a.n = n, a.stop = stop;
    a.om0 = out_matches0, a.om1 = out_matches1, a.os0 = out_mscores0, a.os1 = out_mscores1, a.omt = out_matches;
    a.oms = out_mscores, a.ocnt = out_counts, a.prune0 = prune0, a.prune1 = prune1;
    hipLaunchKernelGGL(matches_scatter_kernel, dim3(3, pairs), dim3(256), 0, stream, a);
    return launched(who);
}

}  // extern "C"
