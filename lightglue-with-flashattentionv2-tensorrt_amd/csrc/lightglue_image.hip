// lightglue_image.hip — image input (include/lightglue_glue.h, "image input"): uint8 images of any size,
// channel count and strides to the encoder's grey [batch, Ht, Wt] input in one launch, and the keypoints
// back to each source image's pixels. What the reference does on the host before its network sees a frame
// (demo/demo_mono.cpp:151-152, 232-233; lightglue_pytorch_no_plugin/utils.py:30-76, 94-97).
//
// lg_img_prepare / lg_img_prepare_batch share one body. A thread owns one output pixel; the 64 lanes of a wave
// are 64 adjacent output columns of one row, so a wave's reads of a source row are one contiguous run of
// bytes (ratio x channels bytes per lane) and its store is one contiguous run. An area axis takes its taps four
// or eight at a time, and where a row's pixels and channels are adjacent bytes it reads them as dwords; every
// form gives the same bits. Every source position and
// overlap is an exact integer rational; a weight is one fp32 division of two integers below 2^24. The grey
// weights carry the 1 / 255, so every partial result is at most 1.
#include "lightglue_device.h"

namespace {

constexpr int kImgMaxSide = 16384;
constexpr int kImgCols = 64, kImgRows = 4;  // a workgroup's output tile (one wave per row)
constexpr int kKpThreads = 256;

// One axis of one output pixel: `count` source pixels from `first` on (indices clamped by the reader), the
// first weighing w_first, the last w_last, those between w_mid.
struct Taps {
    int first, count;
    float w_first, w_mid, w_last;
};

// Output index o of n_dst along a source axis of n_src pixels.
// area (only where n_src > n_dst): o covers [o n_src, (o + 1) n_src) in units of 1 / n_dst of a source pixel;
// pixel i, [i n_dst, (i + 1) n_dst), weighs its overlap / n_src. The interval is longer than a pixel, so it
// touches at least two, every overlap is positive and they sum to n_src.
// linear: the source position ((2 o + 1) n_src - n_dst) / (2 n_dst) = i0 + r / (2 n_dst), weights
// (2 n_dst - r) / (2 n_dst) and r / (2 n_dst) on i0 and i0 + 1 (INTER_LINEAR, bilinear align_corners=False).
__device__ __forceinline__ Taps axis_taps(int o, int n_src, int n_dst, bool area) {
    Taps t;
    if (area) {
        const int lo = o * n_src, hi = lo + n_src;     // <= 2^28
        const int first = lo / n_dst, last = (hi - 1) / n_dst;
        const float den = (float)n_src;
        t.first = first, t.count = last - first + 1;
        t.w_first = (float)((first + 1) * n_dst - lo) / den;
        t.w_mid = (float)n_dst / den;
        t.w_last = (float)(hi - last * n_dst) / den;
    } else {
        const int p = (2 * o + 1) * n_src - n_dst;      // >= -(n_dst - 1), < 2^29
        const int d = 2 * n_dst;
        const int i0 = p >= 0 ? p / d : -1;             // floor: p > -d
        const int r = p - i0 * d;                       // [0, d)
        t.first = i0, t.count = 2;
        t.w_first = (float)(d - r) / (float)d;
        t.w_mid = 0.f;
        t.w_last = (float)r / (float)d;
    }
    return t;
}
__device__ __forceinline__ float tap_weight(const Taps& t, int i) {
    return i == 0 ? t.w_first : (i == t.count - 1 ? t.w_last : t.w_mid);
}

// The descriptor as the kernel uses it: sides clamped into [1, 16384], the channel offsets resolved.
struct Src {
    const uint8_t* data;
    int h, w;
    bool color, bgr;
    int packed;  // bytes per pixel (1, 3, 4) where a row's pixels and channels are adjacent bytes, >= 4 a row; else 0
    int64_t sy, sx, off_r, off_g, off_b;
};
__device__ __forceinline__ Src make_src(const void* data, int h, int w, int channels, int bgr, int64_t sy, int64_t sx,
                                        int64_t sc) {
    Src s;
    s.data = (const uint8_t*)data;
    s.h = min(max(h, 1), kImgMaxSide), s.w = min(max(w, 1), kImgMaxSide);
    s.color = channels == 3 || channels == 4;  // (a fourth channel is ignored)
    s.bgr = bgr != 0;
    const int bpp = s.color ? channels : 1;
    s.packed = sx == bpp && (!s.color || sc == 1) && s.w * bpp >= 4 ? bpp : 0;
    s.sy = sy, s.sx = sx;
    s.off_r = bgr ? 2 * sc : 0, s.off_g = sc, s.off_b = bgr ? 0 : 2 * sc;
    return s;
}

// grey / 255 = 0.299 R + 0.587 G + 0.114 B (utils.py:72-76) with the 1 / 255 in the constants
constexpr float kGreyR = (float)(0.299 / 255.0), kGreyG = (float)(0.587 / 255.0), kGreyB = (float)(0.114 / 255.0);
constexpr float kGrey1 = (float)(1.0 / 255.0);

__device__ __forceinline__ float grey_at(const Src& s, const uint8_t* px) {
    if (s.color) return fmaf(kGreyB, (float)px[s.off_b], fmaf(kGreyG, (float)px[s.off_g], kGreyR * (float)px[s.off_r]));
    return kGrey1 * (float)px[0];
}

// One source row's weighted sum, the taps in ascending x, CH at a time: their loads are issued together (a
// lane's taps are dependent on nothing but the address), and a tap past the count is a clamped load weighing
// 0, which leaves the sum's bits as they are. So the result does not depend on CH.
template <int CH>
__device__ __forceinline__ float row_sum(const Src& s, const uint8_t* row, const Taps& tx) {
    float rs = 0.f;
#pragma unroll 1
    for (int i0 = 0; i0 < tx.count; i0 += CH) {
        float g[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) g[u] = grey_at(s, row + min(max(tx.first + i0 + u, 0), s.w - 1) * s.sx);
#pragma unroll
        for (int u = 0; u < CH; ++u) rs = fmaf(i0 + u < tx.count ? tap_weight(tx, i0 + u) : 0.f, g[u], rs);
    }
    return rs;
}

// The same sum (the same bits) for an area axis of a packed row (Src::packed == BPP): the CH taps of a chunk
// are CH BPP adjacent bytes, read as dwords (a byte load costs the texture path as many cycles as a dword
// load). The hardware takes a dword at any byte address; one that would end past the row's last byte is
// read 4 bytes before that end and shifted down, so no byte outside the row is touched. What it then lacks
// belongs to taps past the count.
template <int BPP, int CH>
__device__ __forceinline__ float row_sum_packed(const Src& s, const uint8_t* row, const Taps& tx) {
    constexpr int ND = CH * BPP / 4;
    const int last = s.w * BPP - 4;  // the last dword of the row
    float rs = 0.f;
#pragma unroll 1
    for (int i0 = 0; i0 < tx.count; i0 += CH) {
        const int a = (tx.first + i0) * BPP;  // the chunk's first byte: a valid tap's, 0 <= a <= last + 3
        unsigned v[ND];
#pragma unroll
        for (int k = 0; k < ND; ++k) {
            const int want = a + 4 * k, off = min(want, last), sh = want - off;
            unsigned d;
            __builtin_memcpy(&d, row + off, 4);
            v[k] = sh >= 4 ? 0u : d >> (8 * (sh & 3));
        }
        float g[CH];
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            float c[3];
#pragma unroll
            for (int e = 0; e < (BPP == 1 ? 1 : 3); ++e) c[e] = (float)((v[(u * BPP + e) / 4] >> (8 * ((u * BPP + e) % 4))) & 0xffu);
            if constexpr (BPP == 1) g[u] = kGrey1 * c[0];
            else g[u] = fmaf(kGreyB, s.bgr ? c[0] : c[2], fmaf(kGreyG, c[1], kGreyR * (s.bgr ? c[2] : c[0])));
        }
#pragma unroll
        for (int u = 0; u < CH; ++u) rs = fmaf(i0 + u < tx.count ? tap_weight(tx, i0 + u) : 0.f, g[u], rs);
    }
    return rs;
}

template <int CH>
__device__ __forceinline__ float row_sum_area(const Src& s, const uint8_t* row, const Taps& tx) {
    switch (s.packed) {  // (the same for the whole image)
        case 1: return row_sum_packed<1, CH>(s, row, tx);
        case 3: return row_sum_packed<3, CH>(s, row, tx);
        case 4: return row_sum_packed<4, CH>(s, row, tx);
        default: return row_sum<CH>(s, row, tx);
    }
}

template <typename TOut>
__device__ __forceinline__ void img_prepare_body(const Src& s, int ht, int wt, int interp, TOut* out /* [ht, wt] */) {
    const int ox = blockIdx.x * kImgCols + threadIdx.x, oy = blockIdx.y * kImgRows + threadIdx.y;
    if (ox >= wt || oy >= ht) return;
    const bool area_x = interp == LG_IMG_AREA && s.w > wt;
    const Taps ty = axis_taps(oy, s.h, ht, interp == LG_IMG_AREA && s.h > ht);
    const Taps tx = axis_taps(ox, s.w, wt, area_x);
    const int chunk = !area_x ? 2 : (s.w > 4 * wt ? 8 : 4);  // (the same for the whole image)
    float acc = 0.f;
    if (chunk == 2) {  // two taps a row: two rows at a time (linear in y: all four pixels in flight at once)
#pragma unroll 1
        for (int j = 0; j < ty.count; j += 2) {
            const float rs0 = row_sum<2>(s, s.data + min(max(ty.first + j, 0), s.h - 1) * s.sy, tx);
            const float rs1 = row_sum<2>(s, s.data + min(max(ty.first + j + 1, 0), s.h - 1) * s.sy, tx);
            acc = fmaf(tap_weight(ty, j), rs0, acc);
            acc = fmaf(j + 1 < ty.count ? tap_weight(ty, j + 1) : 0.f, rs1, acc);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < ty.count; ++j) {
            const uint8_t* row = s.data + min(max(ty.first + j, 0), s.h - 1) * s.sy;
            acc = fmaf(tap_weight(ty, j), chunk == 4 ? row_sum_area<4>(s, row, tx) : row_sum_area<8>(s, row, tx), acc);
        }
    }
    out[(size_t)oy * wt + ox] = (TOut)acc;
}

template <typename TOut>
__global__ __launch_bounds__(kImgCols* kImgRows) void img_prepare_table_kernel(const lg_img_src* __restrict__ table, int ht,
                                                                                int wt, int interp, TOut* __restrict__ out) {
    const lg_img_src d = table[blockIdx.z];
    const Src s = make_src(d.data, d.h, d.w, d.channels, d.bgr, d.stride_y, d.stride_x, d.stride_c);
    img_prepare_body<TOut>(s, ht, wt, interp, out + (size_t)blockIdx.z * ht * wt);
}

template <typename TOut>
__global__ __launch_bounds__(kImgCols* kImgRows) void img_prepare_batch_kernel(lg_img_src d, int64_t stride_b, int ht, int wt,
                                                                                int interp, TOut* __restrict__ out) {
    const Src s = make_src((const uint8_t*)d.data + blockIdx.z * stride_b, d.h, d.w, d.channels, d.bgr, d.stride_y,
                           d.stride_x, d.stride_c);
    img_prepare_body<TOut>(s, ht, wt, interp, out + (size_t)blockIdx.z * ht * wt);
}

// (2 px + 1) n_src / (2 n_dst) - 1/2 = ((2 px + 1) n_src - n_dst) / (2 n_dst) = q + r / (2 n_dst), |r| < 2 n_dst:
// q and r exact, one division and one sum in fp32 (n_src == n_dst: r = 0 and q = px).
__device__ __forceinline__ float kp_axis(int px, int n_src, int n_dst) {
    px = min(max(px, 0), n_dst - 1);
    n_src = min(max(n_src, 1), kImgMaxSide);
    const int m = (2 * px + 1) * n_src - n_dst, d = 2 * n_dst;
    const int q = m / d, r = m - q * d;
    return (float)q + (float)r / (float)d;
}

__global__ __launch_bounds__(kKpThreads) void kp_to_source_kernel(const int32_t* __restrict__ kpts_px,
                                                                   const int32_t* __restrict__ counts,
                                                                   const int32_t* __restrict__ src_sizes, int ht, int wt, int k,
                                                                   int total, float* __restrict__ out) {
    const int i = blockIdx.x * kKpThreads + threadIdx.x;  // one keypoint
    if (i >= total) return;
    const int b = i / k, row = i - b * k;
    const int n = min(max(counts[b], 0), k);
    float x = 0.f, y = 0.f;
    if (row < n) {
        x = kp_axis(kpts_px[2 * (size_t)i], src_sizes[2 * b + 1], wt);
        y = kp_axis(kpts_px[2 * (size_t)i + 1], src_sizes[2 * b], ht);
    }
    out[2 * (size_t)i] = x;
    out[2 * (size_t)i + 1] = y;
}

bool side_ok(int32_t n) { return n >= 1 && n <= kImgMaxSide; }
// what both prepare calls share: the target, the interpolation, the output
bool target_ok(int32_t batch, int32_t ht, int32_t wt, int32_t interp, int32_t out_dtype, const void* out) {
    return batch >= 0 && batch <= 65535 && side_ok(ht) && side_ok(wt) && (interp == LG_IMG_LINEAR || interp == LG_IMG_AREA) &&
           dtype_ok(out_dtype) && out && aligned_as(out_dtype, out);
}
dim3 prepare_grid(int batch, int ht, int wt) {
    return dim3((wt + kImgCols - 1) / kImgCols, (ht + kImgRows - 1) / kImgRows, batch);
}

}  // namespace

extern "C" {

size_t lg_img_src_bytes(void) { return sizeof(lg_img_src); }

int32_t lg_img_prepare(const lg_img_src* table, int32_t batch, int32_t ht, int32_t wt, int32_t interp, int32_t out_dtype,
                       void* out, hipStream_t stream) {
    const char* who = "lg_img_prepare";
    if (!target_ok(batch, ht, wt, interp, out_dtype, out) || !table || !aligned8(table)) return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    const dim3 grid = prepare_grid(batch, ht, wt), block(kImgCols, kImgRows);
    if (out_dtype == MHA_HD64_DT_HALF)
        hipLaunchKernelGGL(img_prepare_table_kernel<f16>, grid, block, 0, stream, table, ht, wt, interp, (f16*)out);
    else
        hipLaunchKernelGGL(img_prepare_table_kernel<float>, grid, block, 0, stream, table, ht, wt, interp, (float*)out);
    return launched(who);
}

int32_t lg_img_prepare_batch(const void* data, int32_t batch, int32_t h, int32_t w, int32_t channels, int32_t bgr,
                             int64_t stride_b, int64_t stride_y, int64_t stride_x, int64_t stride_c, int32_t ht, int32_t wt,
                             int32_t interp, int32_t out_dtype, void* out, hipStream_t stream) {
    const char* who = "lg_img_prepare_batch";
    const int64_t lim = (int64_t)1 << 40;
    if (!target_ok(batch, ht, wt, interp, out_dtype, out) || !data || !side_ok(h) || !side_ok(w) ||
        (channels != 1 && channels != 3 && channels != 4) || (bgr != 0 && bgr != 1) || stride_b < 0 || stride_y < 0 ||
        stride_x < 0 || stride_c < 0 || stride_b > lim || stride_y > lim || stride_x > lim || stride_c > lim)
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    lg_img_src d{};
    d.data = data, d.h = h, d.w = w, d.channels = channels, d.bgr = bgr;
    d.stride_y = stride_y, d.stride_x = stride_x, d.stride_c = stride_c;
    const dim3 grid = prepare_grid(batch, ht, wt), block(kImgCols, kImgRows);
    if (out_dtype == MHA_HD64_DT_HALF)
        hipLaunchKernelGGL(img_prepare_batch_kernel<f16>, grid, block, 0, stream, d, stride_b, ht, wt, interp, (f16*)out);
    else
        hipLaunchKernelGGL(img_prepare_batch_kernel<float>, grid, block, 0, stream, d, stride_b, ht, wt, interp, (float*)out);
    return launched(who);
}

int32_t lg_kp_to_source(const int32_t* kpts_px, const int32_t* counts, const int32_t* src_sizes, int32_t ht, int32_t wt,
                        int32_t batch, int32_t k, float* out, hipStream_t stream) {
    const char* who = "lg_kp_to_source";
    if (batch < 0 || k < 1 || (int64_t)batch * k > (1 << 28) || !side_ok(ht) || !side_ok(wt) || !kpts_px || !counts ||
        !src_sizes || !out || !aligned4(kpts_px) || !aligned4(counts) || !aligned4(src_sizes) || !aligned4(out))
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    const int total = batch * k;
    hipLaunchKernelGGL(kp_to_source_kernel, dim3((total + kKpThreads - 1) / kKpThreads), dim3(kKpThreads), 0, stream, kpts_px,
                       counts, src_sizes, ht, wt, k, total, out);
    return launched(who);
}

}  // extern "C"
