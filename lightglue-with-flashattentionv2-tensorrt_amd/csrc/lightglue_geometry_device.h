// lightglue_geometry_device.h — what the RANSAC kernel files share on the device and in their entry points
// (csrc/lightglue_geometry.hip: the fundamental matrix and the homography; csrc/lightglue_essential.hip: the
// calibrated five-point): the launch shapes, a pair's arguments and its correspondences into LDS, the ordered block
// sum, the wave tree of the normal matrix's 45 sums, the round-robin Jacobi on the 9 x 9 in LDS, and the argument
// checks. The per-lane arithmetic is in lightglue_geometry_math.h.
#pragma once

#include "lightglue_device.h"
#include "lightglue_geometry_math.h"

namespace {

using namespace lg_geom;

constexpr int kHypLanes = 64;    // hypotheses a workgroup
constexpr int kHypSplit = 4;     // adjacent lanes that share a hypothesis' scoring pass (every fourth correspondence each)
constexpr int kHypThreads = kHypLanes * kHypSplit;
constexpr int kFinThreads = 256;

struct PairArgs {
    const int32_t* matches;  // [pairs, kmax, 2]
    const int32_t* counts;   // [pairs]
    const float* kpts0;      // [pairs, k0, 2]
    const float* kpts1;      // [pairs, k1, 2]
    int kmax, k0, k1;
};

__device__ __forceinline__ int pair_count(const PairArgs& a, int p) { return min(max(a.counts[p], 0), a.kmax); }

// The pair's correspondences (x0, y0, x1, y1) into LDS, indices clamped into range.
__device__ __forceinline__ void stage_pair(const PairArgs& a, int p, int count, float4* pts, int tid, int nthreads) {
    for (int k = tid; k < count; k += nthreads) {
        const size_t m = ((size_t)p * a.kmax + k) * 2;
        const int i0 = min(max(a.matches[m], 0), a.k0 - 1), i1 = min(max(a.matches[m + 1], 0), a.k1 - 1);
        const float2 u = *reinterpret_cast<const float2*>(a.kpts0 + ((size_t)p * a.k0 + i0) * 2);
        const float2 v = *reinterpret_cast<const float2*>(a.kpts1 + ((size_t)p * a.k1 + i1) * 2);
        pts[k] = make_float4(u.x, u.y, v.x, v.y);
    }
}

// The sum over the workgroup of one double per thread, in a fixed order (a tree over the thread index); every
// thread gets it. buf: NT doubles.
template <int NT>
__device__ __forceinline__ double block_sum(double v, double* buf, int tid) {
    __syncthreads();
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if (tid < s) buf[tid] += buf[tid + s];
        __syncthreads();
    }
    return buf[0];
}

// The 45 sums of a thread's inliers (the upper triangle of the normal matrix) added over each wave's lanes in a tree;
// lane 0 of wave w leaves them in part[w].
__device__ __forceinline__ void wave_sums(const double acc[45], double (*part)[45], int tid) {
    #pragma unroll
                    for (int e = 0; e < 45; ++e) {
                        double v = acc[e];
    #pragma unroll
                        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
                        if (tid % 64 == 0) part[tid / 64][e] = v;
                    }
}

// Jacobi on the symmetric 9 x 9 am with the eigenvectors accumulated in vm (both row-major in LDS, vm the identity
// at entry, the workgroup synchronised at entry and at exit): kJacobiSweeps sweeps of 9 steps, 4 disjoint rotations
// a step; A <- Jᵀ A J, V <- V J. rot: [4][2] in LDS.
__device__ __forceinline__ void jacobi9(double* am, double* vm, double (*rot)[2], int tid) {
                #pragma unroll 1
                for (int step = 0; step < 9 * kJacobiSweeps; ++step) {
                    if (tid < 4) {
                        int pp, qq;
                        jacobi_pair(step, tid, pp, qq);
                        double cc, ss;
                        jacobi_cs(am[9 * pp + pp], am[9 * qq + qq], am[9 * pp + qq], cc, ss);
                        rot[tid][0] = cc, rot[tid][1] = ss;
                    }
                    __syncthreads();
                    if (tid < 72) {  // columns p, q of row k of A and of V
                        const int g = tid / 18, w = tid % 18, k = w % 9;
                        double* m = w < 9 ? am : vm;
                        int pp, qq;
                        jacobi_pair(step, g, pp, qq);
                        const double cc = rot[g][0], ss = rot[g][1];
                        const double mp = m[9 * k + pp], mq = m[9 * k + qq];
                        m[9 * k + pp] = cc * mp - ss * mq, m[9 * k + qq] = ss * mp + cc * mq;
                    }
                    __syncthreads();
                    if (tid < 36) {  // rows p, q of column k of A
                        const int g = tid / 9, k = tid % 9;
                        int pp, qq;
                        jacobi_pair(step, g, pp, qq);
                        const double cc = rot[g][0], ss = rot[g][1];
                        const double mp = am[9 * pp + k], mq = am[9 * qq + k];
                        am[9 * pp + k] = cc * mp - ss * mq, am[9 * qq + k] = ss * mp + cc * mq;
                    }
                    __syncthreads();
                }
}

bool pair_args_ok(const int32_t* matches, const int32_t* counts, const float* kpts0, const float* kpts1, int32_t pairs,
                  int32_t kmax, int32_t k0, int32_t k1) {
    const int64_t lim = 1 << 28;
    return pairs >= 0 && pairs <= 65535 && kmax >= 1 && kmax <= kMaxPoints && k0 >= 1 && k1 >= 1 &&
           (int64_t)pairs * kmax <= lim && (int64_t)pairs * k0 <= lim && (int64_t)pairs * k1 <= lim && matches && counts &&
           kpts0 && kpts1 && aligned8(matches) && aligned4(counts) && aligned8(kpts0) && aligned8(kpts1);
}
bool threshold_ok(float t) { return t > 0.f && t <= 1e6f; }  // (NaN fails; t² stays finite)
dim3 hyp_grid(int32_t n, int32_t pairs) { return dim3((n + kHypLanes - 1) / kHypLanes, pairs); }

// lg_ransac_samples, lg_ransac_samples4, lg_ransac_samples5: a lane is a hypothesis.
template <int N>
__global__ __launch_bounds__(kHypLanes) void ransac_samples_kernel(int count, int hypotheses, uint32_t seed,
                                                                    int32_t* __restrict__ out) {
    const int h = blockIdx.x * kHypLanes + threadIdx.x;
    if (h >= hypotheses) return;
    int idx[N];
    sample<N>(seed, h, count, idx);
#pragma unroll
    for (int j = 0; j < N; ++j) out[(size_t)h * N + j] = idx[j];
}

}  // namespace
