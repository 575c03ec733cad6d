// lightglue_window.hip — the sequence window (include/lightglue_glue.h, "the sequence window"): what turns the matcher's
// V - 1 consecutive pair results into lg_bundle_adjust's window. Tracks chained through the shared images, each track's
// point from all of its posed views, and the 2D-3D rows that give the next frame its pose. The contract is restated in
// lightglue_amd/geometry_contract.py (window_tracks_reference: plain loops over integers; window_points_reference: the
// fixed-round scheme in float64; window_points_converged: scipy per track, another route); the arithmetic is in
// lightglue_window_math.h.
//
// window_tracks_kernel: one workgroup of 256 threads per window. The per-pair next / prev tables sit in LDS as 16-bit
// keypoint indices (2 x 7 x 2,048 x 2 B = 56 KiB). A pair at a time, the owners of both sides' keypoints are built in
// two int tables (16 KiB, reused by every pair) by an integer atomicMin over the live rows: the lowest row wins, whatever
// the order. A row that owns both of its keypoints is a link, so a keypoint has at most one link out and one in: the
// tracks are simple paths. The start flags over the (V - 1) x 2,048 candidates (view, keypoint), a thread's candidates
// adjacent, go through the workgroup prefix sum (block_prefix, lg_link_landmarks'), which numbers the tracks in ascending
// (start view, start keypoint) order; the first lmax starts go to LDS over the owner tables, and one thread per kept
// track walks its at most V - 1 links, so adjacent threads write adjacent entries of a view's row.
//
// window_points_kernel: grid (tiles of 32 tracks, windows), 256 threads; the lane layout is bundle_adjust_kernel's: thread
// tid is view tid % 8 of track tid / 8 of the tile, the 8 views of a track 8 adjacent lanes. The window's poses (fp64,
// entered as lg_bundle_adjust enters them) and cameras sit in LDS. The 6 + 3 sums of the normal equations, and of JᵀJ
// and Jᵀr in each Gauss-Newton round, go round an xor butterfly in a fixed order, so every lane of the group holds the
// same bits and solves the 3 x 3 system alike: no LDS traffic in the rounds, no atomics. There is no MFMA here: the
// widest product is a track's 3 x 3 block from at most 8 rows of 2 x 3.
//
// window_landmarks_kernel: one workgroup per window; a stable compaction by the same prefix sum.
// No floating-point atomics, no allocation, no scratch, no host synchronisation.
#include "lightglue_geometry_device.h"
#include "lightglue_window_math.h"

namespace {

constexpr int kWinThreads = 256;
constexpr int kWinTile = kWinThreads / kMaxViews;  // tracks a workgroup of window_points_kernel
constexpr int kWinPairs = kMaxViews - 1;
constexpr int kNoOwnerRow = 0x7fffffff;

struct TrackArgs {
    const int32_t* matches;    // [B, V-1, Kmax, 2]
    const int32_t* counts;     // [B, V-1]
    const uint8_t* mask;       // [B, V-1, Kmax]
    const int32_t* kp_counts;  // [B, V]
    int views, kmax, lmax;
};

struct TrackShared {
    uint16_t next[kWinPairs][kMaxPoints];  // keypoint i of view v -> its keypoint of view v + 1
    uint16_t prev[kWinPairs][kMaxPoints];  // keypoint j of view v + 1 -> its keypoint of view v
    int own[2][kMaxPoints];                // a pair's owners, column 0's then column 1's; then the kept tracks' starts
    int scan[kWinThreads];
};

__global__ __launch_bounds__(kWinThreads) void window_tracks_kernel(TrackArgs a, int32_t* __restrict__ track_kp,
                                                                     int32_t* __restrict__ kept_out, int32_t* __restrict__ found_out) {
    __shared__ TrackShared sh;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pairs = a.views - 1;
    for (int e = tid; e < pairs * kMaxPoints; e += kWinThreads) (&sh.next[0][0])[e] = kNoLink, (&sh.prev[0][0])[e] = kNoLink;  // (the window's pairs' rows: no other is read)
#pragma unroll 1
    for (int v = 0; v < kWinPairs; ++v) {
        if (v >= pairs) break;
        for (int e = tid; e < 2 * kMaxPoints; e += kWinThreads) (&sh.own[0][0])[e] = kNoOwnerRow;
        __syncthreads();
        const size_t pair = (size_t)b * pairs + v;
        const int count = min(max(a.counts[pair], 0), a.kmax);
        const int k0 = min(max(a.kp_counts[(size_t)b * a.views + v], 0), kMaxPoints);
        const int k1 = min(max(a.kp_counts[(size_t)b * a.views + v + 1], 0), kMaxPoints);
        for (int r = tid; r < count; r += kWinThreads) {
            const size_t row = pair * a.kmax + r;
            const int i = a.matches[2 * row], j = a.matches[2 * row + 1];
            if (!a.mask[row] || i < 0 || i >= k0 || j < 0 || j >= k1) continue;  // (not live)
            atomicMin(&sh.own[0][i], r);  // (an integer minimum in LDS: the same whatever the order)
            atomicMin(&sh.own[1][j], r);
        }
        __syncthreads();
        for (int r = tid; r < count; r += kWinThreads) {
            const size_t row = pair * a.kmax + r;
            const int i = a.matches[2 * row], j = a.matches[2 * row + 1];
            if (!a.mask[row] || i < 0 || i >= k0 || j < 0 || j >= k1) continue;
            if (sh.own[0][i] == r && sh.own[1][j] == r) sh.next[v][i] = (uint16_t)j, sh.prev[v][j] = (uint16_t)i;
        }
        __syncthreads();  // (the owners are read before the next pair clears them)
    }
    // a thread's candidates (view, keypoint) are adjacent, so the threads' counts scanned in thread order give the order
    const int chunk = pairs * (kMaxPoints / kWinThreads), lo = tid * chunk;
    int mine = 0;
#pragma unroll 1
    for (int e = 0; e < kWinPairs * (kMaxPoints / kWinThreads); ++e) {
        if (e >= chunk) break;
        const int v = (lo + e) / kMaxPoints, i = (lo + e) % kMaxPoints;
        mine += sh.next[v][i] != kNoLink && (v == 0 || sh.prev[v - 1][i] == kNoLink) ? 1 : 0;
    }
    int total;
    int pos = block_prefix<kWinThreads>(mine, sh.scan, tid, total);
    int* starts = &sh.own[0][0];
#pragma unroll 1
    for (int e = 0; e < kWinPairs * (kMaxPoints / kWinThreads); ++e) {
        if (e >= chunk) break;
        const int v = (lo + e) / kMaxPoints, i = (lo + e) % kMaxPoints;
        if (sh.next[v][i] == kNoLink || (v != 0 && sh.prev[v - 1][i] != kNoLink)) continue;
        if (pos < a.lmax) starts[pos] = lo + e;
        ++pos;
    }
    __syncthreads();
    const int kept = min(total, a.lmax);
    for (int l = tid; l < a.lmax; l += kWinThreads) {
        const int start = l < kept ? starts[l] : 0;
        const int v0 = l < kept ? start / kMaxPoints : kMaxViews;
        int cur = -1;
#pragma unroll
        for (int v = 0; v < kMaxViews; ++v) {
            if (v >= a.views) break;
            if (v == v0) {
                cur = start % kMaxPoints;
            } else if (v > v0 && cur >= 0) {
                const int nx = sh.next[v - 1][cur];
                cur = nx == kNoLink ? -1 : nx;
            }
            track_kp[((size_t)b * a.views + v) * a.lmax + l] = cur;
        }
    }
    if (tid == 0) kept_out[b] = kept, found_out[b] = total;
}

struct PointArgs {
    const int32_t* track_kp;  // [B, V, L]
    const int32_t* kept;      // [B]
    const float* kpts;        // [B, V, Kp, 2]
    const float* intr;        // [B, V, 4]
    const float* r;           // [B, V, 3, 3]
    const float* t;           // [B, V, 3]
    const uint8_t* posed;     // [B, V]
    int views, lmax, kp;
};

__global__ __launch_bounds__(kWinThreads) void window_points_kernel(PointArgs a, double thr2, float* __restrict__ obs,
                                                                     uint8_t* __restrict__ seen, int32_t* __restrict__ counts,
                                                                     float* __restrict__ points, uint8_t* __restrict__ ok_out,
                                                                     uint8_t* __restrict__ seen_all) {
    __shared__ double pose[kMaxViews][12];
    __shared__ float cams[kMaxViews][4];
    __shared__ int usable[kMaxViews];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int v = tid % kMaxViews, l = blockIdx.x * kWinTile + tid / kMaxViews;
    if (tid < kMaxViews) {  // thread v enters view v: the pose, and whether the view counts
        bool ok = false;
        float p[12] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
        float kk[4] = {1.f, 1.f, 0.f, 0.f};
        if (tid < a.views) {
            const size_t at = (size_t)b * a.views + tid;
#pragma unroll
            for (int k = 0; k < 4; ++k) kk[k] = a.intr[at * 4 + k];
            ok = a.posed[at] != 0 && camera_ok(Camera{kk[0], kk[1], kk[2], kk[3]});
            if (tid >= 1) {
#pragma unroll
                for (int k = 0; k < 9; ++k) p[k] = a.r[at * 9 + k];
#pragma unroll
                for (int k = 0; k < 3; ++k) p[9 + k] = a.t[at * 3 + k];
            }
        }
        Pose q;
        ok = absolute_enter(p, q) && ok;
#pragma unroll
        for (int k = 0; k < 9; ++k) pose[tid][k] = q.r[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) pose[tid][9 + k] = q.t[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) cams[tid][k] = kk[k];
        usable[tid] = ok ? 1 : 0;
    }
    __syncthreads();
    const int kept = min(max(a.kept[b], 0), a.lmax);
    if (tid == 0 && blockIdx.x == 0) counts[b] = kept;
    const bool inb = l < a.lmax && v < a.views;
    const size_t at = ((size_t)b * a.views + (v < a.views ? v : 0)) * a.lmax + (l < a.lmax ? l : 0);
    const int kp = inb && l < kept ? a.track_kp[at] : -1;
    const bool has = kp >= 0 && kp < a.kp;
    float2 px = make_float2(0.f, 0.f);
    if (has) px = *reinterpret_cast<const float2*>(a.kpts + (((size_t)b * a.views + v) * a.kp + kp) * 2);
    Pose q;
#pragma unroll
    for (int k = 0; k < 9; ++k) q.r[k] = pose[v][k];
#pragma unroll
    for (int k = 0; k < 3; ++k) q.t[k] = pose[v][9 + k];
    const Camera cam{cams[v][0], cams[v][1], cams[v][2], cams[v][3]};
    bool set = has && usable[v] != 0;  // the track's posed views; after the first pass, those kept
    bool solved = false, all_pass = false;
    int nset = 0;
    double x[3] = {0.0, 0.0, 0.0}, piv = 0.0;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        double s[kWindowSums], res[2], jx[2][3];
        window_ray(q, cam, (double)px.x, (double)px.y, s);
#pragma unroll
        for (int e = 0; e < kWindowSums; ++e) s[e] = lanes_sum<kMaxViews>(set ? s[e] : 0.0);
        nset = lanes_sum<kMaxViews>(set ? 1 : 0);
        solved = window_start(s, x, piv);
#pragma unroll 1
        for (int round = 0; round < kWindowGnRounds; ++round) {
            const bool row_ok = window_row(q, cam, x, (double)px.x, (double)px.y, res, jx);
            window_row_sums(set && row_ok, res, jx, s);
#pragma unroll
            for (int e = 0; e < kWindowSums; ++e) s[e] = lanes_sum<kMaxViews>(s[e]);
            window_step(s, x);
        }
        const bool row_ok = window_row(q, cam, x, (double)px.x, (double)px.y, res, jx);
        const bool pass_v = window_pass(set, row_ok, res, thr2);
        all_pass = lanes_sum<kMaxViews>(set && !pass_v ? 1 : 0) == 0;
        if (pass == 0) set = pass_v;
    }
    const bool ok = window_ok(solved, nset, all_pass, x, piv);
    if (inb) {
        obs[2 * at] = px.x, obs[2 * at + 1] = px.y;
        seen[at] = set && ok ? 1 : 0;
        seen_all[at] = has ? 1 : 0;
    }
    if (v == 0 && l < a.lmax) {
        const size_t row = (size_t)b * a.lmax + l;
#pragma unroll
        for (int k = 0; k < 3; ++k) points[3 * row + k] = ok ? (float)x[k] : 0.f;
        ok_out[row] = ok ? 1 : 0;
    }
}

struct MarkArgs {
    const int32_t* track_kp;  // [B, V, L]
    const int32_t* kept;      // [B]
    const uint8_t* ok;        // [B, L]
    const float* points;      // [B, L, 3]
    const float* kpts;        // [B, Kp, 2]: the one view's
    int views, lmax, kp, view;
};

__global__ __launch_bounds__(kWinThreads) void window_landmarks_kernel(MarkArgs a, float* __restrict__ points,
                                                                        float* __restrict__ image, int32_t* __restrict__ rows,
                                                                        int32_t* __restrict__ n_out) {
    __shared__ int scan[kWinThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int kept = min(max(a.kept[b], 0), a.lmax);
    const int32_t* kps = a.track_kp + ((size_t)b * a.views + a.view) * a.lmax;
    // a thread's tracks are adjacent, so that the threads' counts scanned in thread order give the tracks' order
    const int chunk = (a.lmax + kWinThreads - 1) / kWinThreads;
    const int lo = tid * chunk, hi = min(lo + chunk, kept);
    int mine = 0;
    for (int l = lo; l < hi; ++l) mine += a.ok[(size_t)b * a.lmax + l] != 0 && kps[l] >= 0 && kps[l] < a.kp ? 1 : 0;
    int total;
    int pos = block_prefix<kWinThreads>(mine, scan, tid, total);
    for (int l = lo; l < hi; ++l) {
        const int kp = kps[l];
        if (a.ok[(size_t)b * a.lmax + l] == 0 || kp < 0 || kp >= a.kp) continue;
        const size_t dst = (size_t)b * a.lmax + pos, src = (size_t)b * a.lmax + l;
        points[3 * dst] = a.points[3 * src], points[3 * dst + 1] = a.points[3 * src + 1], points[3 * dst + 2] = a.points[3 * src + 2];
        image[2 * dst] = a.kpts[((size_t)b * a.kp + kp) * 2], image[2 * dst + 1] = a.kpts[((size_t)b * a.kp + kp) * 2 + 1];
        rows[dst] = l;
        ++pos;
    }
    for (int k = total + tid; k < a.lmax; k += kWinThreads) {
        const size_t dst = (size_t)b * a.lmax + k;
        points[3 * dst] = 0.f, points[3 * dst + 1] = 0.f, points[3 * dst + 2] = 0.f;
        image[2 * dst] = 0.f, image[2 * dst + 1] = 0.f;
        rows[dst] = -1;
    }
    if (tid == 0) n_out[b] = total;
}

bool window_shape_ok(int32_t windows, int32_t views, int32_t lmax) {
    return windows >= 0 && windows <= 65535 && views >= 2 && views <= kMaxViews && lmax >= 1 && lmax <= kMaxPoints;
}

}  // namespace

extern "C" {

int32_t lg_window_tracks(const int32_t* matches, const int32_t* counts, const uint8_t* mask, const int32_t* kp_counts,
                         int32_t windows, int32_t views, int32_t kmax, int32_t lmax, int32_t* track_kp, int32_t* kept,
                         int32_t* found, hipStream_t stream) {
    const char* who = "lg_window_tracks";
    if (!window_shape_ok(windows, views, lmax) || kmax < 1 || kmax > kMaxPoints || !matches || !counts || !mask || !kp_counts ||
        !track_kp || !kept || !found || !aligned4(matches) || !aligned4(counts) || !aligned4(kp_counts) || !aligned4(track_kp) ||
        !aligned4(kept) || !aligned4(found))
        return bad(who);
    if (windows == 0) return MHA_HD64_STATUS_SUCCESS;
    const TrackArgs a{matches, counts, mask, kp_counts, views, kmax, lmax};
    hipLaunchKernelGGL(window_tracks_kernel, dim3(windows), dim3(kWinThreads), 0, stream, a, track_kp, kept, found);
    return launched(who);
}

int32_t lg_window_points(const int32_t* track_kp, const int32_t* kept, const float* kpts, const float* intrinsics, const float* r,
                         const float* t, const uint8_t* posed, int32_t windows, int32_t views, int32_t lmax, int32_t kp,
                         float threshold, float* obs, uint8_t* seen, int32_t* counts, float* points, uint8_t* ok, uint8_t* seen_all,
                         hipStream_t stream) {
    const char* who = "lg_window_points";
    if (!window_shape_ok(windows, views, lmax) || kp < 1 || (int64_t)windows * views * kp > (1 << 28) || !threshold_ok(threshold) ||
        !track_kp || !kept || !kpts || !intrinsics || !r || !t || !posed || !obs || !seen || !counts || !points || !ok || !seen_all ||
        !aligned4(track_kp) || !aligned4(kept) || !aligned8(kpts) || !aligned4(intrinsics) || !aligned4(r) || !aligned4(t) ||
        !aligned4(obs) || !aligned4(counts) || !aligned4(points))
        return bad(who);
    if (windows == 0) return MHA_HD64_STATUS_SUCCESS;
    const PointArgs a{track_kp, kept, kpts, intrinsics, r, t, posed, views, lmax, kp};
    hipLaunchKernelGGL(window_points_kernel, dim3((lmax + kWinTile - 1) / kWinTile, windows), dim3(kWinThreads), 0, stream, a,
                       (double)threshold * (double)threshold, obs, seen, counts, points, ok, seen_all);
    return launched(who);
}

int32_t lg_window_landmarks(const int32_t* track_kp, const int32_t* kept, const uint8_t* ok, const float* points,
                            const float* kpts_view, int32_t windows, int32_t views, int32_t lmax, int32_t kp, int32_t view,
                            float* out_points, float* image, int32_t* rows, int32_t* n, hipStream_t stream) {
    const char* who = "lg_window_landmarks";
    if (!window_shape_ok(windows, views, lmax) || kp < 1 || (int64_t)windows * kp > (1 << 28) || view < 0 || view >= views ||
        !track_kp || !kept || !ok || !points || !kpts_view || !out_points || !image || !rows || !n || !aligned4(track_kp) ||
        !aligned4(kept) || !aligned4(points) || !aligned4(kpts_view) || !aligned4(out_points) || !aligned4(image) || !aligned4(rows) ||
        !aligned4(n))
        return bad(who);
    if (windows == 0) return MHA_HD64_STATUS_SUCCESS;
    const MarkArgs a{track_kp, kept, ok, points, kpts_view, views, lmax, kp, view};
    hipLaunchKernelGGL(window_landmarks_kernel, dim3(windows), dim3(kWinThreads), 0, stream, a, out_points, image, rows, n);
    return launched(who);
}

}  // extern "C"
