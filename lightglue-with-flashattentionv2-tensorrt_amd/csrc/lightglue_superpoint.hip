// lightglue_superpoint.hip — the SuperPoint encoder and its two heads (include/lightglue_glue.h, "SuperPoint
// encoder"; superpoint.py:143-172): images to the keypoint front end's inputs in ten launches.
//   lg_sp_conv1     conv1a, 1 -> 64 channels, on the vector pipe (nine FMAs per output, store-bound)
//   lg_sp_conv3x3   every other 3 x 3 layer as an implicit GEMM on v_mfma_f32_32x32x16_f16
//   lg_sp_heads     convPb (256 -> 65) and convDb (256 -> 256) in one launch, in the front end's layouts
// Activations are NHWC fp16; a layer accumulates in fp32, adds the bias in fp32, applies ReLU and rounds to
// fp16 once. No launch synchronises, keeps state or uses atomics.
//
// The 3 x 3 kernel. As in lightglue_linear.hip the product is computed transposed, Cᵀ = W·Aᵀ: the MFMA's A
// operand is a weight fragment (32 output channels x 16 input channels of one tap), its B operand 32 pixels
// x the same 16 channels, so a lane owns one pixel and 4 runs of 4 consecutive output channels. A workgroup
// owns an 8 x 16 tile of output pixels and 64 (cout <= 256) or 128 (cout = 512) output channels; its 4 waves
// are 2 (pixel halves: 2 blocks of 2 rows x 16 pixels each) x 2 (channel halves). The tile's 10 x 18 input
// patch is loaded into LDS once, zero outside the image (each image of the batch is addressed on its own,
// so a patch never holds a neighbour's rows), and all nine taps read it at shifted addresses: no im2col.
// A pixel's channels take CIN * 2 + 16 bytes and a patch row 18 pixels + 224 bytes: with either CIN the
// 16-B slot of pixel (y, x) is then (x + 16 y) * odd mod 16, and each of ds_read_b128's 16-lane groups
// (lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} of a half) reads 16 distinct slots: conflict-free.
// The weights come straight from global memory in the fragment-major order the host packed once
// ([cout / 32][tap][cin / 16][lane][8]): a wave's stream is contiguous, 1 KiB per fragment, prefetched a
// group of four k-steps ahead. The epilogue stages the tile through the (dead) patch's LDS so that the optional
// 2 x 2 max-pool and the stores work on whole 16-B channel groups of a pixel.
#include "lightglue_device.h"

namespace {

constexpr int kTH = 8, kTW = 16;             // output pixels of a workgroup's tile
constexpr int kPH = kTH + 2, kPW = kTW + 2;  // its input patch
constexpr int kRowPad = 224;                 // bytes after a patch row's 18 pixels (see above)

struct ConvArgs {
    const f16* in;    // [batch, h, w, CIN]
    const f16* wp;    // packed weights
    const f16* bias;  // [cout]
    f16* out;         // [batch, h, w, cout], or [batch, h / 2, w / 2, cout] with pool
    int h, w, cout, tiles_x, relu, pool;
};

template <int CIN, int NCB>
__global__ __launch_bounds__(256) void sp_conv3x3_kernel(const ConvArgs a) {
    constexpr int NPB = kTH * kTW / 64;  // pixel blocks per wave
    constexpr int PP = CIN * 2 + 16, RP = kPW * PP + kRowPad, PATCH = kPH * RP;
    constexpr int KS = CIN / 16, CB = 64 * NCB, SP = CB * 2 + 16, STAGE = kTH * kTW * SP;
    // weight prefetch: groups of G k-steps, NB - 1 groups in flight (a whole tap per group and two groups in
    // flight measured 3 % slower at every batch size: the compiler schedules the loads early either way)
    constexpr int G = 4, NB = 2;
    constexpr int STEPS = 9 * KS, NG = STEPS / G;
    static_assert(KS % G == 0 && NG >= NB, "a prefetch group stays inside one tap");
    __shared__ __attribute__((aligned(16))) char smem[PATCH > STAGE ? PATCH : STAGE];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wp = wave & 1, wc = wave >> 1;
    const int r = lane & 31, hh = lane >> 5;
    const int tx0 = ((int)blockIdx.x % a.tiles_x) * kTW, ty0 = ((int)blockIdx.x / a.tiles_x) * kTH;
    const int c0 = (int)blockIdx.y * CB, b = blockIdx.z;
    const f16* img = a.in + (size_t)b * a.h * a.w * CIN;

    // this wave's weight streams (one per 32-channel block) and the first group, under the patch load
    const f16* wsrc[NCB];
#pragma unroll
    for (int i = 0; i < NCB; ++i) wsrc[i] = a.wp + (size_t)(c0 / 32 + wc * NCB + i) * (STEPS * 512) + lane * 8;
    f16x8 wbuf[NB][G][NCB];
#pragma unroll
    for (int g = 0; g < NB - 1; ++g)
#pragma unroll
        for (int s = 0; s < G; ++s)
#pragma unroll
            for (int i = 0; i < NCB; ++i) wbuf[g][s][i] = *reinterpret_cast<const f16x8*>(wsrc[i] + (g * G + s) * 512);
    f16x4 bias4[NCB][4];
#pragma unroll
    for (int i = 0; i < NCB; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g)
            bias4[i][g] = *reinterpret_cast<const f16x4*>(a.bias + c0 + (wc * NCB + i) * 32 + 8 * g + 4 * hh);

    // the patch: pixel (ty0 - 1 + py, tx0 - 1 + px), 16-B units of its channels; zero outside the image
    constexpr int U = CIN / 8;
    for (int idx = tid; idx < kPH * kPW * U; idx += 256) {
        const int pix = idx / U, u = idx - pix * U;
        const int py = pix / kPW, px = pix - py * kPW;
        const int gy = ty0 + py - 1, gx = tx0 + px - 1;
        f16x8 v = {};
        if (gy >= 0 && gy < a.h && gx >= 0 && gx < a.w)
            v = *reinterpret_cast<const f16x8*>(img + ((size_t)gy * a.w + gx) * CIN + u * 8);
        *reinterpret_cast<f16x8*>(smem + py * RP + px * PP + u * 16) = v;
    }
    __syncthreads();

    // pixel block NPB wp + j: lane r -> tile pixel p = 32 (NPB wp + j) + r, row-major in the tile
    unsigned pbase[NPB];
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
        const int p = (NPB * wp + j) * 32 + r;
        pbase[j] = (p / kTW) * RP + (p % kTW) * PP + hh * 16;
    }

    f32x16 acc[NPB][NCB] = {};
#pragma unroll
    for (int g = 0; g < NG; ++g) {  // (fully unrolled: every buffer index below is a compile-time constant)
        if (g + NB - 1 < NG) {
#pragma unroll
            for (int s = 0; s < G; ++s)
#pragma unroll
                for (int i = 0; i < NCB; ++i)
                    wbuf[(g + NB - 1) % NB][s][i] = *reinterpret_cast<const f16x8*>(wsrc[i] + ((g + NB - 1) * G + s) * 512);
        }
        const int t = g * G / KS, ks0 = g * G % KS;
        const unsigned toff = (t / 3) * RP + (t % 3) * PP + ks0 * 32;
#pragma unroll
        for (int s = 0; s < G; ++s) {
            f16x8 af[NPB];
#pragma unroll
            for (int j = 0; j < NPB; ++j) af[j] = *(lds_f16x8*)(lds + pbase[j] + toff + s * 32);
#pragma unroll
            for (int j = 0; j < NPB; ++j)
#pragma unroll
                for (int i = 0; i < NCB; ++i)
                    acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wbuf[g % NB][s][i], af[j], acc[j][i], 0, 0, 0);
        }
    }

    // ---- epilogue: bias, ReLU, one rounding; the tile staged as [pixel][CB channels] in the patch's LDS ----
    __syncthreads();  // (every wave is done with the patch)
#pragma unroll
    for (int j = 0; j < NPB; ++j) {
        const int p = (NPB * wp + j) * 32 + r;
#pragma unroll
        for (int i = 0; i < NCB; ++i)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f16x4 v;
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    float x = acc[j][i][4 * g + t] + (float)bias4[i][g][t];
                    if (a.relu) x = fmaxf(x, 0.f);
                    v[t] = (f16)x;
                }
                *reinterpret_cast<f16x4*>(smem + p * SP + ((wc * NCB + i) * 32 + 8 * g + 4 * hh) * 2) = v;
            }
    }
    __syncthreads();
    constexpr int UO = CB / 8;
    if (!a.pool) {
        f16* dst = a.out + (size_t)b * a.h * a.w * a.cout + c0;
        for (int idx = tid; idx < kTH * kTW * UO; idx += 256) {
            const int p = idx / UO, u = idx - p * UO;
            const int gy = ty0 + p / kTW, gx = tx0 + p % kTW;
            if (gy < a.h && gx < a.w)
                *reinterpret_cast<f16x8*>(dst + ((size_t)gy * a.w + gx) * a.cout + u * 8) =
                    *reinterpret_cast<const f16x8*>(smem + p * SP + u * 16);
        }
    } else {  // 2 x 2 / stride 2 (h, w even: a window whose first pixel is inside the image is whole)
        const int oh = a.h / 2, ow = a.w / 2;
        f16* dst = a.out + (size_t)b * oh * ow * a.cout + c0;
        for (int idx = tid; idx < (kTH / 2) * (kTW / 2) * UO; idx += 256) {
            const int q = idx / UO, u = idx - q * UO;
            const int qy = q / (kTW / 2), qx = q % (kTW / 2);
            const int gy = ty0 / 2 + qy, gx = tx0 / 2 + qx;
            if (gy >= oh || gx >= ow) continue;
            const char* src = smem + (2 * qy * kTW + 2 * qx) * SP + u * 16;
            const f16x8 v0 = *reinterpret_cast<const f16x8*>(src), v1 = *reinterpret_cast<const f16x8*>(src + SP);
            const f16x8 v2 = *reinterpret_cast<const f16x8*>(src + kTW * SP);
            const f16x8 v3 = *reinterpret_cast<const f16x8*>(src + (kTW + 1) * SP);
            *reinterpret_cast<f16x8*>(dst + ((size_t)gy * ow + gx) * a.cout + u * 8) =
                __builtin_elementwise_max(__builtin_elementwise_max(v0, v1), __builtin_elementwise_max(v2, v3));
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// conv1a: a thread computes 8 channels of 4 consecutive pixels of a row from a 3 x 6 window; the 8 threads
// of a pixel write its 128 B as eight 16-B stores.
template <typename T>
__global__ __launch_bounds__(256) void sp_conv1_kernel(const T* __restrict__ img, const f16* __restrict__ wt,
                                                       const f16* __restrict__ bias, f16* __restrict__ out, int h, int w,
                                                       int runs, long long total, int relu) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int cg = (int)(gid & 7);
    const long long run = gid >> 3;
    const int rx = (int)(run % runs);
    const long long row = run / runs;  // b * h + y
    const int y = (int)(row % h);
    const int x0 = rx * 4;
    // this thread's 8 channels: 72 contiguous weights (nine 16-B loads) and 8 biases (one)
    float k[8][9], bs[8];
    {
        f16x8 wv[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) wv[i] = *reinterpret_cast<const f16x8*>(wt + cg * 72 + i * 8);
        const f16x8 bv = *reinterpret_cast<const f16x8*>(bias + cg * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            bs[c] = (float)bv[c];
#pragma unroll
            for (int t = 0; t < 9; ++t) k[c][t] = (float)wv[(c * 9 + t) / 8][(c * 9 + t) % 8];
        }
    }
    float v[3][6];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = y + dy - 1;
#pragma unroll
        for (int dx = 0; dx < 6; ++dx) {
            const int xx = x0 + dx - 1;
            v[dy][dx] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? (float)img[(size_t)(row + dy - 1) * w + xx] : 0.f;
        }
    }
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        if (x0 + px >= w) break;
        f16x8 o;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 9; ++t) s = fmaf(v[t / 3][px + t % 3], k[c][t], s);
            s += bs[c];
            if (relu) s = fmaxf(s, 0.f);
            o[c] = (f16)s;
        }
        *reinterpret_cast<f16x8*>(out + ((size_t)row * w + x0 + px) * 64 + cg * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------------
// The heads: a workgroup takes 64 pixels' 512 channels (cPa | cDa) into LDS (a pixel's row is 1024 + 16
// bytes: consecutive pixels sit one 16-B slot apart, conflict-free as above) and its waves share the 11
// blocks of 32 output channels: 0..2 convPb's 65 (padded with zero weights to 96) on channels 0..255, 3..10
// convDb's 256 on channels 256..511. Wave w takes blocks w, w + 4, w + 8. A lane owns a pixel: its logits
// go to 65 channel planes (consecutive lanes, consecutive pixels), its descriptors to 8-B runs of its row.
constexpr int kHeadPix = 64, kHeadPitch = 1024 + 16, kHeadBlocks = 11;

struct HeadArgs {
    const f16* in;    // [M, 512]
    const f16* wp;    // packed [11][16][64][8]
    const f16* bias;  // [96 + 256]
    f16* logits;      // [batch, 65, hw]
    f16* dense;       // [M, 256]
    int M, hw;
};

__global__ __launch_bounds__(256) void sp_heads_kernel(const HeadArgs a) {
    __shared__ __attribute__((aligned(16))) char smem[kHeadPix * kHeadPitch];
    lds_char* const lds = (lds_char*)smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int m0 = (int)blockIdx.x * kHeadPix;
    for (int idx = tid; idx < kHeadPix * 64; idx += 256) {
        const int row = idx >> 6, u = idx & 63;
        f16x8 v = {};
        if (m0 + row < a.M) v = *reinterpret_cast<const f16x8*>(a.in + (size_t)(m0 + row) * 512 + u * 8);
        *reinterpret_cast<f16x8*>(smem + row * kHeadPitch + u * 16) = v;
    }
    __syncthreads();

    f32x16 acc[2][3] = {};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int cb = wave + 4 * i;
        if (cb >= kHeadBlocks) break;  // (uniform over the wave)
        const f16* wsrc = a.wp + (size_t)cb * (16 * 512) + lane * 8;
        const unsigned koff = (cb < 3 ? 0 : 512) + hh * 16;  // byte offset of the block's input channels
        f16x8 wf[16];
#pragma unroll
        for (int ks = 0; ks < 16; ++ks) wf[ks] = *reinterpret_cast<const f16x8*>(wsrc + ks * 512);
#pragma unroll
        for (int ks = 0; ks < 16; ++ks)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f16x8 af = *(lds_f16x8*)(lds + (j * 32 + r) * kHeadPitch + koff + ks * 32);
                acc[j][i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[ks], af, acc[j][i], 0, 0, 0);
            }
    }

#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int cb = wave + 4 * i;
        if (cb >= kHeadBlocks) break;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + j * 32 + r;
            if (m >= a.M) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = cb * 32 + 8 * g + 4 * hh;  // 4 consecutive rows of the bias table
                const f16x4 b4 = *reinterpret_cast<const f16x4*>(a.bias + n);
                f16x4 v;
#pragma unroll
                for (int t = 0; t < 4; ++t) v[t] = (f16)(acc[j][i][4 * g + t] + (float)b4[t]);
                if (cb < 3) {
                    const int bi = m / a.hw, pi = m - bi * a.hw;
#pragma unroll
                    for (int t = 0; t < 4; ++t)
                        if (n + t < 65) a.logits[((size_t)bi * 65 + n + t) * a.hw + pi] = v[t];
                } else {
                    *reinterpret_cast<f16x4*>(a.dense + (size_t)m * 256 + (n - 96)) = v;
                }
            }
        }
    }
}

bool cin_ok(int cin) { return cin == 64 || cin == 128; }
bool cout_ok(int cout) { return cout == 64 || cout == 128 || cout == 256 || cout == 512; }

template <int CIN, int NCB>
void launch_conv(const ConvArgs& a, int batch, hipStream_t stream) {
    const dim3 grid(a.tiles_x * ((a.h + kTH - 1) / kTH), a.cout / (64 * NCB), batch);
    hipLaunchKernelGGL((sp_conv3x3_kernel<CIN, NCB>), grid, dim3(256), 0, stream, a);
}

}  // namespace

extern "C" {

size_t lg_sp_packed_bytes(int32_t taps, int32_t cin, int32_t cout) {
    if (taps == 9) return cin_ok(cin) && cout_ok(cout) ? (size_t)9 * cin * cout * 2 : 0;
    if (taps == 1) return cin == 256 && cout == 32 * kHeadBlocks ? (size_t)cin * cout * 2 : 0;
    return 0;
}

int32_t lg_sp_conv1(int32_t image_dtype, const void* image, const void* weight, const void* bias, int32_t h, int32_t w,
                    int32_t batch, int32_t flags, void* out, hipStream_t stream) {
    const char* who = "lg_sp_conv1";
    const bool half = image_dtype == MHA_HD64_DT_HALF;
    if (!dtype_ok(image_dtype) || !image_ok(h, w, batch) || (flags & ~LG_SP_RELU) || !image || !weight || !bias || !out ||
        !aligned_as(image_dtype, image) || !aligned16(weight) || !aligned16(bias) || !aligned16(out) || image == out)
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    const int runs = (w + 3) / 4;
    const long long total = (long long)batch * h * runs * 8;
    const dim3 grid((unsigned)((total + 255) / 256)), block(256);
    const int relu = flags & LG_SP_RELU;
    if (half)
        hipLaunchKernelGGL(sp_conv1_kernel<f16>, grid, block, 0, stream, (const f16*)image, (const f16*)weight, (const f16*)bias,
                           (f16*)out, h, w, runs, total, relu);
    else
        hipLaunchKernelGGL(sp_conv1_kernel<float>, grid, block, 0, stream, (const float*)image, (const f16*)weight,
                           (const f16*)bias, (f16*)out, h, w, runs, total, relu);
    return launched(who);
}

int32_t lg_sp_conv3x3(const void* in, const void* w_packed, const void* bias, int32_t cin, int32_t cout, int32_t h, int32_t w,
                      int32_t batch, int32_t flags, void* out, hipStream_t stream) {
    const char* who = "lg_sp_conv3x3";
    const bool pool = flags & LG_SP_POOL2;
    if (!cin_ok(cin) || !cout_ok(cout) || !image_ok(h, w, batch) || (flags & ~(LG_SP_RELU | LG_SP_POOL2)) ||
        (pool && (h % 2 || w % 2)) || !in || !w_packed || !bias || !out || !aligned16(in) || !aligned16(w_packed) ||
        !aligned8(bias) || !aligned16(out) || in == out)
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    ConvArgs a{};
    a.in = (const f16*)in, a.wp = (const f16*)w_packed, a.bias = (const f16*)bias, a.out = (f16*)out;
    a.h = h, a.w = w, a.cout = cout, a.tiles_x = (w + kTW - 1) / kTW, a.relu = flags & LG_SP_RELU, a.pool = pool;
    // 128 channels per workgroup for the widest layer only (convPa | convDa: 4 x fewer patch loads); 64
    // elsewhere, so that a 60 x 80 map still makes 80 workgroups per 64 channels. (8 x 32 tiles for the
    // 64 -> 64 layers, a weight fragment feeding four MFMAs: 256 VGPRs, two workgroups per CU, 0.6 x the rate.)
    if (cin == 64) {
        if (cout == 512) launch_conv<64, 2>(a, batch, stream);
        else launch_conv<64, 1>(a, batch, stream);
    } else {
        if (cout == 512) launch_conv<128, 2>(a, batch, stream);
        else launch_conv<128, 1>(a, batch, stream);
    }
    return launched(who);
}

int32_t lg_sp_heads(const void* in, const void* w_packed, const void* bias, int32_t hc, int32_t wc, int32_t batch,
                    void* logits, void* dense, hipStream_t stream) {
    const char* who = "lg_sp_heads";
    if (hc < 1 || wc < 1 || !image_ok((int64_t)hc * 8, (int64_t)wc * 8, batch) || !in || !w_packed || !bias || !logits || !dense ||
        !aligned16(in) || !aligned16(w_packed) || !aligned8(bias) || !aligned2(logits) ||
        !aligned8(dense) || in == dense || in == logits || logits == dense)
        return bad(who);
    if (batch == 0) return MHA_HD64_STATUS_SUCCESS;
    HeadArgs a{};
    a.in = (const f16*)in, a.wp = (const f16*)w_packed, a.bias = (const f16*)bias, a.logits = (f16*)logits;
    a.dense = (f16*)dense, a.hw = hc * wc, a.M = batch * hc * wc;
    hipLaunchKernelGGL(sp_heads_kernel, dim3((a.M + kHeadPix - 1) / kHeadPix), dim3(256), 0, stream, a);
    return launched(who);
}

}  // extern "C"
