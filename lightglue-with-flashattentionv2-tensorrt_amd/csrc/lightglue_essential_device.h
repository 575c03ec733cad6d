// lightglue_essential_device.h — what the calibrated kernels share on the device (csrc/lightglue_essential.hip: the
// five-point RANSAC; csrc/lightglue_polish.hip: the pose polish and the triangulation): a pair's intrinsics, a
// correspondence in camera coordinates and the inlier mask of an F in pixels.
#pragma once

#include "lightglue_geometry_device.h"
#include "lightglue_essential_math.h"

namespace {

__device__ __forceinline__ Intrinsics load_intrinsics(const float* intr, int p) {
    const float* k = intr + (size_t)p * 8;
    return Intrinsics{k[0], k[1], k[2], k[3], k[4], k[5], k[6], k[7]};
}

__device__ __forceinline__ void camera(const float4 q, const Intrinsics& k, double c[4]) {
    c[0] = ((double)q.x - k.cx0) / k.fx0, c[1] = ((double)q.y - k.cy0) / k.fy0;
    c[2] = ((double)q.z - k.cx1) / k.fx1, c[3] = ((double)q.w - k.cy1) / k.fy1;
}

// hartley's coordinates for the essential matrix's refit: camera(q, kk, ·).
struct CameraCoord {
    const Intrinsics& kk;
    __device__ __forceinline__ void operator()(const float4 q, double c[4]) const { camera(q, kk, c); }
};

// Marks the inliers of f into m and returns their number (every thread).
__device__ __forceinline__ int mark_inliers(const float f[9], const float4* pts, int count, float thr2, uint8_t* m, double* buf,
                                            int tid) {
    int mine = 0;
    for (int k = tid; k < count; k += kFinThreads) {
        const float4 q = pts[k];
        const bool in = is_inlier(f, q.x, q.y, q.z, q.w, thr2);
        m[k] = in ? 1 : 0;
        mine += in ? 1 : 0;
    }
    return (int)block_sum<kFinThreads>((double)mine, buf, tid);  // (exact: integers below 2^53)
}

}  // namespace
