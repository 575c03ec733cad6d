// lightglue_frontend.hip — the keypoint front end (include/lightglue_glue.h, "keypoint front end"):
// SuperPoint's two dense heads to the matcher's inputs without a host synchronisation.
//   lg_kp_heatmap   softmax over the 65 detector channels + the 8 x 8 depth-to-space, one pass
//   lg_kp_nms       simple_nms (superpoint.py:52-69) in one launch: tile + halo in LDS, five separable pools
//   lg_kp_select    threshold / border compaction, then the K best per image in a pinned order
//   lg_kp_describe  bilinear descriptor sampling, both normalisations, keypoint normalisation
// Hand-offs between the stages are kernel boundaries on the stream; atomics are integer counters and slot
// allocators in LDS only (the selected set does not depend on slot order: bitwise reproducible), and no
// state outlives a launch: nothing is zeroed between calls.
#include "lightglue_device.h"

#include <math.h>

namespace {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------------------------------
// heatmap: one thread per 8 x 8 cell. Lanes run along Wc, so each channel's load is contiguous across the
// wave and each of a cell's eight 32-B row segments sits next to its neighbour lane's.
template <typename T>
__global__ __launch_bounds__(256) void kp_heatmap_kernel(const T* __restrict__ logits, float* __restrict__ out, int hc,
                                                         int wc, int cells) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= cells) return;
    const int plane = hc * wc;
    const int b = idx / plane, c = idx - b * plane;
    const int i = c / wc, j = c - i * wc;
    const T* src = logits + (size_t)b * 65 * plane + c;
    float v[65];
#pragma unroll
    for (int ch = 0; ch < 65; ++ch) v[ch] = (float)src[(size_t)ch * plane];
    float mx = v[0];
#pragma unroll
    for (int ch = 1; ch < 65; ++ch) mx = fmaxf(mx, v[ch]);
    float sum = 0.f;
#pragma unroll
    for (int ch = 0; ch < 65; ++ch) {
        v[ch] = expf(v[ch] - mx);
        sum += v[ch];
    }
    const int w = wc * 8;
    float* dst = out + ((size_t)b * hc * 8 + (size_t)i * 8) * w + (size_t)j * 8;
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
        f32x4 lo, hi;
#pragma unroll
        for (int e = 0; e < 4; ++e) lo[e] = v[rr * 8 + e] / sum, hi[e] = v[rr * 8 + 4 + e] / sum;
        *reinterpret_cast<f32x4*>(dst + (size_t)rr * w) = lo;
        *reinterpret_cast<f32x4*>(dst + (size_t)rr * w + 4) = hi;
    }
}

// ---------------------------------------------------------------------------------------------------
// NMS. A pixel's result depends on scores up to 5 r away: r for the first maximum mask, and per round r
// for the dilation of the mask, r for the pool of the suppressed scores (2 r), twice. So a tile's region is
// the tile plus 5 r on every side, every pool is clipped to the region, and an intermediate at distance d
// from the tile is exact while d is at most (4, 3, 3, 2, 1, 1, 0) r for (mask0, supp1, ss1, mask1, supp2,
// ss2, mask2). Pixels outside the image hold -inf and are in no mask: the pools' implicit padding.
constexpr int kNmsTile = 32;
constexpr int kNmsMaxR = 4;
constexpr int kNmsRun = 8;  // outputs per work item: 8 + 2 r loads for 8 window maxima

// One separable pass over the R x R region (row pitch PITCH, odd: an item's column reads and a wave's row
// reads both spread over the banks): COL = false, item (y, 8 consecutive x) takes the row maximum; COL = true,
// item (x, 8 consecutive y) the column maximum. Consecutive threads take consecutive y (x): conflict-free.
// ld(y, x) -> float (outside the region: -inf), st(y, x, max).
template <int RAD, int R, bool COL, typename Ld, typename St>
__device__ __forceinline__ void nms_pass(int tid, Ld ld, St st) {
    constexpr int RUNS = (R + kNmsRun - 1) / kNmsRun, W = kNmsRun + 2 * RAD;
    for (int it = tid; it < R * RUNS; it += 256) {
        const int a = it % R, b0 = (it / R) * kNmsRun;  // a: the fixed coordinate, b0: the run's first
        float v[W];
#pragma unroll
        for (int j = 0; j < W; ++j) {
            const int b = b0 - RAD + j;
            v[j] = (b >= 0 && b < R) ? (COL ? ld(b, a) : ld(a, b)) : -INFINITY;
        }
#pragma unroll
        for (int i = 0; i < kNmsRun; ++i) {
            float m = v[i];
#pragma unroll
            for (int k = 1; k <= 2 * RAD; ++k) m = fmaxf(m, v[i + k]);
            if (b0 + i < R) {
                if (COL) st(b0 + i, a, m);
                else st(a, b0 + i, m);
            }
        }
    }
    __syncthreads();
}

template <int RAD>
__global__ __launch_bounds__(256) void kp_nms_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w) {
    constexpr int halo = 5 * RAD, R = kNmsTile + 2 * halo, PITCH = R | 1, n = R * R;
    __shared__ float S[R * PITCH];
    __shared__ float T[R * PITCH];
    __shared__ uint8_t M[R * PITCH];
    __shared__ uint8_t P[R * PITCH];
    const int tid = threadIdx.x;
    const int y0 = (int)blockIdx.y * kNmsTile - halo, x0 = (int)blockIdx.x * kNmsTile - halo;
    const float* img = in + (size_t)blockIdx.z * h * w;
    auto inside = [&](int y, int x) { return y0 + y >= 0 && y0 + y < h && x0 + x >= 0 && x0 + x < w; };
    auto stT = [&](int y, int x, float m) { T[y * PITCH + x] = m; };
    auto ldT = [&](int y, int x) { return T[y * PITCH + x]; };

    for (int idx = tid; idx < n; idx += 256) {
        const int y = idx / R, x = idx - y * R;
        S[y * PITCH + x] = inside(y, x) ? img[(size_t)(y0 + y) * w + (x0 + x)] : -INFINITY;
    }
    __syncthreads();
    // first mask: s == pool(s)
    nms_pass<RAD, R, false>(tid, [&](int y, int x) { return S[y * PITCH + x]; }, stT);
    nms_pass<RAD, R, true>(tid, ldT, [&](int y, int x, float m) { M[y * PITCH + x] = inside(y, x) && S[y * PITCH + x] == m; });
    for (int round = 0; round < 2; ++round) {
        // supp = pool(mask) > 0 (outside the image: not suppressed, the score stays -inf)
        nms_pass<RAD, R, false>(tid, [&](int y, int x) { return (float)M[y * PITCH + x]; }, stT);
        nms_pass<RAD, R, true>(tid, ldT, [&](int y, int x, float m) { P[y * PITCH + x] = m > 0.f && inside(y, x); });
        // ss = supp ? 0 : s; mask |= (ss == pool(ss)) & ~supp
        nms_pass<RAD, R, false>(tid, [&](int y, int x) { return P[y * PITCH + x] ? 0.f : S[y * PITCH + x]; }, stT);
        nms_pass<RAD, R, true>(tid, ldT, [&](int y, int x, float m) {
            if (!P[y * PITCH + x] && inside(y, x) && S[y * PITCH + x] == m) M[y * PITCH + x] = 1;
        });
    }
    float* dst = out + (size_t)blockIdx.z * h * w;
    for (int idx = tid; idx < kNmsTile * kNmsTile; idx += 256) {
        const int ty = idx / kNmsTile, tx = idx - ty * kNmsTile;
        const int gy = (int)blockIdx.y * kNmsTile + ty, gx = (int)blockIdx.x * kNmsTile + tx;
        if (gy >= h || gx >= w) continue;
        const int li = (ty + halo) * PITCH + tx + halo;
        dst[(size_t)gy * w + gx] = M[li] ? S[li] : 0.f;
    }
}

// ---------------------------------------------------------------------------------------------------
// select. A candidate's key is (score bits << 32) | ~pixel: scores above a threshold >= 0 are positive, so
// their bits order as the values do, and among equal scores the lower pixel index has the larger key.
// Descending keys = descending score, ties by ascending row-major index. Keys are unique.
constexpr int kSelMaxK = 2048;
constexpr int kSelThreads = 1024;

// The image is cut into `segs` segments of `chunk` pixels (a multiple of 256); each segment's candidates
// go to its own slice of the workspace and its count is stored, so no counter outlives a launch and none
// has to be zeroed before one.
constexpr int kSelMaxSegs = 2048;
struct SegLayout {
    int segs, chunk;
};
__host__ __device__ inline SegLayout seg_layout(int hw) {
    SegLayout l;
    const int want = (hw + 4095) / 4096;
    l.segs = want < 1 ? 1 : want > kSelMaxSegs ? kSelMaxSegs : want;
    l.chunk = ((hw + l.segs - 1) / l.segs + 255) / 256 * 256;
    return l;
}

// grid (segments, batch): a workgroup compacts its segment through an LDS slot counter (one atomic per wave)
__global__ __launch_bounds__(256) void kp_compact_kernel(const float* __restrict__ nms, int h, int w, int border,
                                                         float threshold, int32_t* segcnt, u64* segkeys) {
    __shared__ int slots;
    const int hw = h * w, b = blockIdx.y, s = blockIdx.x;
    const SegLayout l = seg_layout(hw);
    const int lane = threadIdx.x & 63;
    u64* dst = segkeys + ((size_t)b * l.segs + s) * l.chunk;
    if (threadIdx.x == 0) slots = 0;
    __syncthreads();
    for (int off = 0; off < l.chunk; off += 256) {
        const int i = s * l.chunk + off + threadIdx.x;
        bool cand = false;
        float v = 0.f;
        if (i < hw) {
            const int y = i / w, x = i - y * w;
            v = nms[(size_t)b * hw + i];
            cand = y >= border && y < h - border && x >= border && x < w - border && v > threshold;
        }
        const u64 mask = __ballot(cand);
        int base = 0;
        if (lane == 0 && mask) base = atomicAdd(&slots, (int)__popcll(mask));
        base = __shfl(base, 0);
        const int slot = base + (int)__popcll(mask & ((1ull << lane) - 1ull));
        if (cand && slot >= 0 && slot < l.chunk) dst[slot] = ((u64)__float_as_uint(v) << 32) | (u64)(~(unsigned)i);
    }
    __syncthreads();
    if (threadIdx.x == 0) segcnt[(size_t)b * l.segs + s] = slots;
}

// grid (batch): the segments' lists copied into one (a wave per segment), the K-th largest key by an 8-bit
// radix select over it, the keys >= it gathered into LDS and sorted by a bitonic network.
__global__ __launch_bounds__(kSelThreads) void kp_select_kernel(const int32_t* segcnt, const u64* segkeys, u64* lists, int hw,
                                                                int K, int32_t* count, int32_t* pix, float* score) {
    __shared__ unsigned hist[256];
    __shared__ u64 sk[kSelMaxK];
    __shared__ int pre[kSelMaxSegs + 1];
    __shared__ u64 s_prefix;
    __shared__ unsigned s_remain, s_slot, s_bin;
    const int tid = threadIdx.x, b = blockIdx.x;
    const SegLayout l = seg_layout(hw);
    for (int s = tid; s < l.segs; s += kSelThreads) pre[s + 1] = min(max(segcnt[(size_t)b * l.segs + s], 0), l.chunk);
    __syncthreads();
    if (tid == 0) {
        pre[0] = 0;
        for (int s = 0; s < l.segs; ++s) pre[s + 1] += pre[s];
    }
    __syncthreads();
    const int n = min(pre[l.segs], hw);
    u64* list = lists + (size_t)b * hw;
    for (int s = tid >> 6; s < l.segs; s += kSelThreads / 64) {
        const u64* src = segkeys + ((size_t)b * l.segs + s) * l.chunk;
        const int at = pre[s], c = pre[s + 1] - at;
        for (int j = tid & 63; j < c; j += 64)
            if (at + j < hw) list[at + j] = src[j];
    }
    __threadfence_block();
    __syncthreads();
    const int take = min(n, K);
    u64 kth = 0;
    if (n > K) {  // (uniform over the workgroup)
        u64 prefix = 0, pmask = 0;
        unsigned remain = K;
        const int lane = tid & 63;
        for (int shift = 56; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0;
            __syncthreads();
            for (int base = 0; base < n; base += kSelThreads) {  // (uniform trip count: ballots below)
                const int i = base + tid;
                const u64 k = i < n ? list[i] : 0;
                bool act = i < n && (k & pmask) == prefix;
                const unsigned d = (unsigned)(k >> shift) & 255u;
                // the high bytes of most keys agree: up to three digits are counted once per wave
                for (int rep = 0; rep < 3; ++rep) {
                    const u64 todo = __ballot(act);
                    if (!todo) break;
                    const int leader = __ffsll((long long)todo) - 1;
                    const unsigned dl = __shfl(d, leader);
                    const u64 same = __ballot(act && d == dl);
                    if (lane == leader) atomicAdd(&hist[dl], (unsigned)__popcll(same));
                    act = act && d != dl;
                }
                if (act) atomicAdd(&hist[d], 1u);
            }
            __syncthreads();
            // digits in descending order: position q <-> digit 255 - q, lane l of wave 0 owns q = 4 l .. 4 l + 3
            if (tid < 64) {
                if (lane == 0) s_prefix = prefix, s_remain = remain, s_bin = 0;  // (unreachable default)
                unsigned c[4], tot = 0;
#pragma unroll
                for (int q = 0; q < 4; ++q) c[q] = hist[255 - (4 * lane + q)], tot += c[q];
                unsigned inc = tot;
#pragma unroll
                for (int sft = 1; sft < 64; sft <<= 1) {
                    const unsigned o = __shfl_up(inc, sft);
                    if (lane >= sft) inc += o;
                }
                unsigned acc = inc - tot;
                if (acc < remain && inc >= remain) {  // the lane whose digits hold the remain-th key from the top
                    int q = 0;
                    while (q < 3 && acc + c[q] < remain) acc += c[q], ++q;
                    s_prefix = prefix | ((u64)(255 - (4 * lane + q)) << shift);
                    s_remain = remain - acc;
                    s_bin = c[q];
                }
            }
            __syncthreads();
            prefix = s_prefix, remain = s_remain;
            pmask |= (u64)255 << shift;
            // every key with this prefix is wanted: the bytes below cannot change the set (k >= prefix)
            if (s_bin == remain) break;
        }
        kth = prefix;
    }
    int npad = 1;
    while (npad < take) npad <<= 1;
    for (int i = tid; i < npad; i += kSelThreads) sk[i] = 0;  // (below every key: a candidate's score bits are > 0)
    if (tid == 0) s_slot = 0;
    __syncthreads();
    for (int i = tid; i < n; i += kSelThreads) {
        const u64 k = list[i];
        if (k >= kth) {
            const unsigned s = atomicAdd(&s_slot, 1u);
            if (s < (unsigned)take) sk[s] = k;
        }
    }
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int i = tid; i < npad; i += kSelThreads) {
                const int o = i ^ j;
                if (o > i) {
                    const u64 a = sk[i], c = sk[o];
                    const bool desc = (i & k) == 0;
                    if (desc ? a < c : a > c) sk[i] = c, sk[o] = a;
                }
            }
            __syncthreads();
        }
    }
    for (int k = tid; k < K; k += kSelThreads) {
        int p = -1;
        float s = 0.f;
        if (k < take) {
            const u64 key = sk[k];
            p = min((int)(~(unsigned)key & 0x7fffffffu), hw - 1);
            s = __uint_as_float((unsigned)(key >> 32));
        }
        pix[(size_t)b * K + k] = p, score[(size_t)b * K + k] = s;
    }
    if (tid == 0) count[b] = take;
}

// ---------------------------------------------------------------------------------------------------
// describe: one wave per keypoint, lane l holds channels l, l + 64, l + 128, l + 192.
struct DsArgs {
    const void* dense;
    long long sb, sc, sy, sx;
    int hc, wc, K, normalized;
    const int32_t* count;
    const int32_t* pix;
    void* desc;
    int32_t* kpx;
    void* kpts;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s);
    return v;
}

template <typename T, typename O>
__global__ __launch_bounds__(256) void kp_describe_kernel(const DsArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63;
    const int kp = blockIdx.x * 4 + (threadIdx.x >> 6);  // (the grid is batch * K / 4: K % 8 == 0)
    const int b = kp / a.K, k = kp - b * a.K;
    const int h = a.hc * 8, w = a.wc * 8;
    const int cnt = min(max(a.count[b], 0), a.K);
    O* d = reinterpret_cast<O*>(a.desc) + (size_t)kp * 256;
    O* kn = reinterpret_cast<O*>(a.kpts) + (size_t)kp * 2;
    if (k >= cnt) {  // (uniform over the wave) a padded row: all zero
#pragma unroll
        for (int i = 0; i < 4; ++i) d[lane + 64 * i] = (O)0.f;
        if (lane < 2) kn[lane] = (O)0.f, a.kpx[(size_t)kp * 2 + lane] = 0;
        return;
    }
    const int p = min(max(a.pix[kp], 0), h * w - 1);
    const int y = p / w, x = p - y * w;
    // sample_descriptors (superpoint.py:72-87) then grid_sample's align_corners=True unnormalisation, in
    // the reference's order of fp32 operations
    const float gx = ((float)x - 4.f + 0.5f) / ((float)w - 4.f - 0.5f) * 2.f - 1.f;
    const float gy = ((float)y - 4.f + 0.5f) / ((float)h - 4.f - 0.5f) * 2.f - 1.f;
    const float ix = (gx + 1.f) / 2.f * (float)(a.wc - 1), iy = (gy + 1.f) / 2.f * (float)(a.hc - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    const int cx0 = (int)fx, cy0 = (int)fy;
    const float wx1 = ix - fx, wx0 = (fx + 1.f) - ix, wy1 = iy - fy, wy0 = (fy + 1.f) - iy;
    const T* dense = reinterpret_cast<const T*>(a.dense) + (size_t)b * a.sb;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int cy = cy0 + (c >> 1), cx = cx0 + (c & 1);
        const float wt = ((c & 1) ? wx1 : wx0) * ((c >> 1) ? wy1 : wy0);
        if (cy < 0 || cy >= a.hc || cx < 0 || cx >= a.wc) continue;  // zero padding (uniform over the wave)
        const T* src = dense + (size_t)cy * a.sy + (size_t)cx * a.sx;
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)src[(size_t)(lane + 64 * i) * a.sc];
        if (!a.normalized) {  // F.normalize over channels (superpoint.py:173) on this corner alone
            const float ss = wave_sum(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
            const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = v[i] / den;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] += v[i] * wt;
    }
    const float ss = wave_sum(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2] + acc[3] * acc[3]);
    const float den = fmaxf(sqrtf(ss), 1e-12f);
#pragma unroll
    for (int i = 0; i < 4; ++i) d[lane + 64 * i] = (O)(acc[i] / den);
    if (lane < 2) {
        const int xy = lane ? y : x;
        const float half = lane ? (float)h / 2.f : (float)w / 2.f;
        a.kpx[(size_t)kp * 2 + lane] = xy;
        kn[lane] = (O)(((float)xy - half) / ((float)max(w, h) / 2.f));
    }
}

// lg_kp_select's workspace: the segments' counts, their key slices (at .keys), the images' lists (at .lists)
struct SelWs {
    size_t keys, lists;
};
SelWs sel_ws(int hw, int batch) {
    const SegLayout l = seg_layout(hw);
    SelWs ws;
    ws.keys = ((size_t)batch * l.segs * 4 + 255) & ~(size_t)255;
    ws.lists = ws.keys + (size_t)batch * l.segs * l.chunk * sizeof(u64);
    return ws;
}

}  // namespace

extern "C" {

int32_t lg_kp_heatmap(int32_t dtype, const void* logits, int32_t hc, int32_t wc, int32_t batch, float* scores,
                      hipStream_t stream) {
    const char* who = "lg_kp_heatmap";
    if (!dtype_ok(dtype) || hc < 1 || wc < 1 || !image_ok((int64_t)hc * 8, (int64_t)wc * 8, batch) || !logits || !scores ||
        !aligned16(scores) || !aligned_as(dtype, logits))
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    const int cells = batch * hc * wc;
    const dim3 grid((cells + 255) / 256), block(256);
    if (dtype == MHA_HD64_DT_HALF)
        hipLaunchKernelGGL(kp_heatmap_kernel<f16>, grid, block, 0, stream, (const f16*)logits, scores, hc, wc, cells);
    else
        hipLaunchKernelGGL(kp_heatmap_kernel<float>, grid, block, 0, stream, (const float*)logits, scores, hc, wc, cells);
    return launched(who);
}

int32_t lg_kp_nms(const float* scores, int32_t h, int32_t w, int32_t batch, int32_t radius, float* out,
                  hipStream_t stream) {
    const char* who = "lg_kp_nms";
    if (!image_ok(h, w, batch) || radius < 0 || radius > kNmsMaxR || !scores || !out || !aligned4(scores) || !aligned4(out) ||
        scores == out)
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    const dim3 grid((w + kNmsTile - 1) / kNmsTile, (h + kNmsTile - 1) / kNmsTile, batch);
    if (grid.y > 65535) return bad(who);
    switch (radius) {
        case 0: hipLaunchKernelGGL(kp_nms_kernel<0>, grid, dim3(256), 0, stream, scores, out, h, w); break;
        case 1: hipLaunchKernelGGL(kp_nms_kernel<1>, grid, dim3(256), 0, stream, scores, out, h, w); break;
        case 2: hipLaunchKernelGGL(kp_nms_kernel<2>, grid, dim3(256), 0, stream, scores, out, h, w); break;
        case 3: hipLaunchKernelGGL(kp_nms_kernel<3>, grid, dim3(256), 0, stream, scores, out, h, w); break;
        default: hipLaunchKernelGGL(kp_nms_kernel<4>, grid, dim3(256), 0, stream, scores, out, h, w); break;
    }
    return launched(who);
}

size_t lg_kp_select_workspace(int32_t h, int32_t w, int32_t batch) {
    if (!image_ok(h, w, batch) || batch == 0) return 0;
    const SelWs ws = sel_ws(h * w, batch);
    return ws.lists + (size_t)batch * h * w * sizeof(u64);
}

int32_t lg_kp_select(const float* nms, int32_t h, int32_t w, int32_t batch, int32_t border, float threshold, int32_t k,
                     int32_t* count, int32_t* pix, float* score, void* workspace, hipStream_t stream) {
    const char* who = "lg_kp_select";
    if (!image_ok(h, w, batch) || border < 0 || !(threshold >= 0.f) || !(threshold < INFINITY) || k < 1 || k > kSelMaxK ||
        k % 8 != 0 || !nms || !count || !pix || !score || !workspace || !aligned4(nms) || !aligned4(count) || !aligned4(pix) ||
        !aligned4(score) || !aligned16(workspace))
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    const SelWs ws = sel_ws(h * w, batch);
    int32_t* segcnt = (int32_t*)workspace;
    u64* segkeys = (u64*)((char*)workspace + ws.keys);
    u64* lists = (u64*)((char*)workspace + ws.lists);
    hipLaunchKernelGGL(kp_compact_kernel, dim3(seg_layout(h * w).segs, batch), dim3(256), 0, stream, nms, h, w, border,
                       threshold, segcnt, segkeys);
    hipLaunchKernelGGL(kp_select_kernel, dim3(batch), dim3(kSelThreads), 0, stream, segcnt, segkeys, lists, h * w, k, count, pix,
                       score);
    return launched(who);
}

int32_t lg_kp_describe(int32_t dense_dtype, const void* dense, int64_t stride_b, int64_t stride_c, int64_t stride_y,
                       int64_t stride_x, int32_t hc, int32_t wc, int32_t batch, int32_t k, const int32_t* count,
                       const int32_t* pix, int32_t dense_normalized, int32_t out_dtype, void* desc, int32_t* kpts_px,
                       void* kpts, hipStream_t stream) {
    const char* who = "lg_kp_describe";
    const int64_t lim = (int64_t)1 << 40;
    if (!dtype_ok(dense_dtype) || !dtype_ok(out_dtype) || hc < 1 || wc < 1 || !image_ok((int64_t)hc * 8, (int64_t)wc * 8, batch) ||
        k < 1 || k > kSelMaxK || k % 8 != 0 || stride_b < 0 || stride_c < 0 || stride_y < 0 || stride_x < 0 || stride_b > lim ||
        stride_c > lim || stride_y > lim || stride_x > lim || (dense_normalized != 0 && dense_normalized != 1) || !dense ||
        !count || !pix || !desc || !kpts_px || !kpts || !aligned4(count) || !aligned4(pix) || !aligned4(kpts_px) ||
        !aligned4(desc) || !aligned4(kpts) || !aligned_as(dense_dtype, dense))
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    DsArgs a{};
    a.dense = dense, a.sb = stride_b, a.sc = stride_c, a.sy = stride_y, a.sx = stride_x, a.hc = hc, a.wc = wc, a.K = k;
    a.normalized = dense_normalized, a.count = count, a.pix = pix, a.desc = desc, a.kpx = kpts_px, a.kpts = kpts;
    const dim3 grid(batch * (k / 4)), block(256);
    const bool dh = dense_dtype == MHA_HD64_DT_HALF, oh = out_dtype == MHA_HD64_DT_HALF;
    if (dh && oh) hipLaunchKernelGGL((kp_describe_kernel<f16, f16>), grid, block, 0, stream, a);
    else if (dh) hipLaunchKernelGGL((kp_describe_kernel<f16, float>), grid, block, 0, stream, a);
    else if (oh) hipLaunchKernelGGL((kp_describe_kernel<float, f16>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((kp_describe_kernel<float, float>), grid, block, 0, stream, a);
    return launched(who);
}

}  // extern "C"
