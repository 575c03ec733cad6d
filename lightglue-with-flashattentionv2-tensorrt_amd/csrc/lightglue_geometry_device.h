// lightglue_geometry_device.h — what the RANSAC kernel files share on the device and in their entry points
// (csrc/lightglue_geometry.hip: the fundamental matrix and the homography; csrc/lightglue_essential.hip: the
// calibrated five-point; csrc/lightglue_absolute.hip: the absolute pose's P3P): the launch shapes, a pair's arguments and its correspondences into LDS, the ordered block
// sum, the refit's steps (the Hartley normalisation, the normal matrix's eigenvectors: the wave tree of its 45 sums
// and the round-robin Jacobi on the 9 x 9 in LDS), the samples' entry point and the argument checks. The per-lane arithmetic is in lightglue_geometry_math.h.
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

// A correspondence as the fundamental matrix and the homography take it: in pixels.
struct PixelCoord {
    __device__ __forceinline__ void operator()(const float4 q, double c[4]) const {
        c[0] = (double)q.x, c[1] = (double)q.y, c[2] = (double)q.z, c[3] = (double)q.w;
    }
};

// Hartley normalisation over the correspondences k < count with use[k] != 0 (use == nullptr: all), in the
// coordinates coord(pts[k], ·) gives: centroid and sqrt(2) / mean distance per image, each thread's share summed in
// ascending k, the shares by block_sum. n: the number of correspondences used (> 0).
template <int NT, class Coord>
__device__ __forceinline__ void hartley(const float4* pts, const uint8_t* use, int count, double n, double* buf, int tid,
                                        double c[4], double s[2], const Coord& coord) {
    double sum[4] = {0.0, 0.0, 0.0, 0.0};
    for (int k = tid; k < count; k += NT) {
        if (use && !use[k]) continue;
        double q[4];
        coord(pts[k], q);
#pragma unroll
        for (int i = 0; i < 4; ++i) sum[i] += q[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = block_sum<NT>(sum[i], buf, tid) / n;
    double dist[2] = {0.0, 0.0};
    for (int k = tid; k < count; k += NT) {
        if (use && !use[k]) continue;
        double q[4];
        coord(pts[k], q);
        const double ax = q[0] - c[0], ay = q[1] - c[1], bx = q[2] - c[2], by = q[3] - c[3];
        dist[0] += sqrt(ax * ax + ay * ay), dist[1] += sqrt(bx * bx + by * by);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) s[i] = 1.4142135623730951 / (block_sum<NT>(dist[i], buf, tid) / n);
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

// The refit's eigenvectors from every thread's 45 sums acc (kFinThreads threads): a wave adds its lanes in a tree
// (wave_sums), the four waves in order into the normal matrix am, vm the identity, jacobi9; the eigenvector of the
// smallest eigenvalue is then the column of vm at am's smallest diagonal entry. part, am, vm, rot: in LDS.
__device__ __forceinline__ void normal_eigenvector(const double acc[45], double (*part)[45], double* am, double* vm,
                                                   double (*rot)[2], int tid) {
    wave_sums(acc, part, tid);
    __syncthreads();
    if (tid < 45) {
        int i, j;
        tri_index(tid, i, j);
        const double v = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
        am[9 * i + j] = v, am[9 * j + i] = v;
    }
    if (tid < 81) vm[tid] = tid / 9 == tid % 9 ? 1.0 : 0.0;
    __syncthreads();
    jacobi9(am, vm, rot, tid);
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

// What lg_ransac_fundamental, lg_ransac_homography and lg_ransac_essential check alike, after pair_args_ok (m: the
// model's matrix; need: the workspace's bytes).
bool ransac_args_ok(float threshold, int32_t hypotheses, int32_t refits, const void* workspace, size_t workspace_bytes,
                    size_t need, const float* m, const uint8_t* inliers, const int32_t* num_inliers, const int32_t* valid,
                    const int32_t* best) {
    return threshold_ok(threshold) && hypotheses >= 1 && hypotheses <= kMaxHypotheses && refits >= 0 && refits <= kMaxRefits &&
           workspace && aligned16(workspace) && workspace_bytes >= need && m && inliers && num_inliers && valid && best &&
           aligned4(m) && aligned4(num_inliers) && aligned4(valid) && aligned4(best);
}
// lg_ransac_solve7, lg_ransac_solve4, lg_ransac_solve5.
bool solve_args_ok(int32_t hypotheses, const int32_t* samples, const float* candidates, const int32_t* num) {
    return hypotheses >= 1 && hypotheses <= kMaxHypotheses && samples && candidates && num && aligned4(samples) &&
           aligned4(candidates) && aligned4(num);
}
// lg_ransac_score, lg_ransac_score_homography.
bool score_args_ok(float threshold, int32_t num_candidates, const float* candidates, const int32_t* inlier_counts) {
    return threshold_ok(threshold) && num_candidates >= 1 && num_candidates <= kMaxHypotheses && candidates && inlier_counts &&
           aligned4(candidates) && aligned4(inlier_counts);
}

// lg_ransac_samples, lg_ransac_samples4, lg_ransac_samples5, lg_ransac_samples3: a lane is a hypothesis.
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

template <int N>
int32_t samples_call(const char* who, int32_t count, int32_t hypotheses, int32_t seed, int32_t* samples, hipStream_t stream) {
    if (count < N || count > kMaxPoints || hypotheses < 1 || hypotheses > kMaxHypotheses || !samples || !aligned4(samples))
        return bad(who);
    hipLaunchKernelGGL(ransac_samples_kernel<N>, dim3((hypotheses + kHypLanes - 1) / kHypLanes), dim3(kHypLanes), 0, stream, count,
                       hypotheses, (uint32_t)seed, samples);
    return launched(who);
}

}  // namespace
