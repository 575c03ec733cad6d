"""The synthetic image pairs of the geometric verification's tests and tools, from synth.uniform24 alone (numpy, no
GPU): ``two_view_scene`` (random 3D points, for the fundamental matrix), ``planar_scene`` (one plane, or a camera
that only turns, for the homography), and ``calibrated_scene`` / ``calibrated_planar_scene``, the same pairs bit for
bit with their cameras (K, R, t) for the essential matrix and the pose polish. The errors that place the outliers are
the float64 contract's (geometry_contract.py). ``absolute_scene`` is a map of 3D points and one camera that sees it (the
absolute pose), ``three_view_scene`` three cameras in a row and the match rows of the two pairs that share the middle
one (the chain from a relative pose to the next camera's pose in the first pair's frame)."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

from . import synth
from .geometry_contract import _epi, _reproject, _transfer, _unit


def _scene_camera(cam: np.ndarray, h: int, w: int):
    """The scenes' intrinsics (focal length w, the centre of the image) and the second camera's rotation from the
    first draws of the stream."""
    kk = np.array([[w, 0.0, w / 2.0], [0.0, w, h / 2.0], [0.0, 0.0, 1.0]])
    ang = (cam[:3] - 0.5) * np.array([0.12, 0.5, 0.12]) + np.array([0.0, 0.15, 0.0])  # radians about x, y, z
    cx, cy, cz = np.cos(ang)
    sx, sy, sz = np.sin(ang)
    rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return kk, rz @ ry @ rx


def _scene_shift(cam: np.ndarray) -> np.ndarray:
    """The second camera's translation (X1 = R X0 + t): sideways."""
    return np.array([-1.0 - cam[3], 0.3 * (cam[4] - 0.5), 0.3 * (cam[5] - 0.5)])


def _split(who: str, k: int, outlier_fraction: float, noise_px: float):
    """(inliers, outliers, the pool of draws a stream) of a scene of k rows."""
    n_out = int(round(k * outlier_fraction))
    n_in = k - n_out
    if k < 1 or n_in < 0 or n_out < 0 or noise_px < 0:
        raise ValueError(f"{who}: bad k / outlier_fraction / noise_px {k}, {outlier_fraction}, {noise_px}")
    return n_in, n_out, 16 * k + 64


def _rows_of(who: str, seed: int, n_in: int, n_out: int, noise_px: float, p0, p1, ok, o0, o1, noise_u, error, model):
    """What the scenes share once the true model is known: the first n_in projections (p0 -> p1 where ok) moved by at
    most noise_px in each image (noise_u: two streams), the first n_out of the outlier draws (o0, o1) further than
    12 px under error(o0, o1) (squared pixels), concatenated and shuffled -> (kpts0, kpts1, gt_mask, model)."""
    k = n_in + n_out
    keep = np.nonzero(ok)[0][:n_in]
    with np.errstate(all="ignore"):
        far = np.nonzero(np.sqrt(error(o0, o1)) > 12.0)[0][:n_out]
    if len(keep) < n_in or len(far) < n_out:
        raise ValueError(f"{who}: the pool ran out (a seed whose second view sees too little)")
    a = noise_px / np.sqrt(2.0)
    noise = (noise_u[:, :2 * n_in].reshape(2, 2, n_in) * 2.0 - 1.0) * a
    k0 = np.concatenate([p0[keep] + noise[0].T, o0[far]])
    k1 = np.concatenate([p1[keep] + noise[1].T, o1[far]])
    gt = np.concatenate([np.ones(n_in, dtype=bool), np.zeros(n_out, dtype=bool)])
    order = np.argsort(synth.uniform24(int(seed) + 0x5EED, k), kind="stable")
    return (torch.from_numpy(k0[order].astype(np.float32)), torch.from_numpy(k1[order].astype(np.float32)),
            torch.from_numpy(gt[order]), torch.from_numpy(model))


def two_view_scene(seed: int, k: int, outlier_fraction: float, noise_px: float, size=(480, 640)):
    """Two pinhole views (size = (h, w), focal length w, the second camera turned and moved sideways) of random
    3D points, from synth.uniform24: (kpts0 [k, 2] fp32, kpts1 [k, 2] fp32, gt_mask [k] bool, F_true [3, 3]
    float64 at unit norm). round(k outlier_fraction) rows are outliers: both ends uniform in the images, redrawn
    until their error under F_true exceeds 12 px; the inliers are projections moved by at most noise_px in each
    image; the rows are shuffled."""
    h, w = int(size[0]), int(size[1])
    n_in, n_out, pool = _split("two_view_scene", k, outlier_fraction, noise_px)
    u = synth.uniform24(int(seed), 16 + 9 * pool).astype(np.float64)
    cam, u = u[:16], u[16:].reshape(9, pool)
    kk, rot = _scene_camera(cam, h, w)
    t = _scene_shift(cam)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    kinv = np.linalg.inv(kk)
    f_true = kinv.T @ tx @ rot @ kinv
    f_true = _unit(f_true)
    # inliers: a pixel of image 0 at a depth, seen in image 1
    p0 = np.stack([u[0] * (w - 1), u[1] * (h - 1)], 1)
    depth = 4.0 + 8.0 * u[2]
    xyz = (np.concatenate([p0, np.ones((pool, 1))], 1) @ kinv.T) * depth[:, None]
    q = (xyz @ rot.T + t) @ kk.T
    p1 = q[:, :2] / q[:, 2:3]
    ok = (q[:, 2] > 0.5) & (p1[:, 0] >= 0) & (p1[:, 0] <= w - 1) & (p1[:, 1] >= 0) & (p1[:, 1] <= h - 1)
    o0 = np.stack([u[3] * (w - 1), u[4] * (h - 1)], 1)
    o1 = np.stack([u[5] * (w - 1), u[6] * (h - 1)], 1)
    return _rows_of("two_view_scene", seed, n_in, n_out, noise_px, p0, p1, ok, o0, o1, u[7:9],
                    lambda a, b: _epi(f_true, a, b), f_true)


def planar_scene(seed: int, k: int, outlier_fraction: float, noise_px: float, size=(480, 640),
                 rotation_only: bool = False):
    """two_view_scene's twin for the homography: two pinhole views (size = (h, w), focal length w) of points on one
    random plane (a depth of 5 to 9 at the image centre, tilted by up to 0.3 in x and in y), the second camera
    turned and moved sideways as two_view_scene's is; rotation_only: the second camera only turned, the points at
    any depth. From synth.uniform24: (kpts0 [k, 2] fp32, kpts1 [k, 2] fp32, gt_mask [k] bool, H_true [3, 3] float64
    at unit norm, x1 ~ H_true x0). round(k outlier_fraction) rows are outliers: both ends uniform in the images,
    redrawn until their transfer error under H_true exceeds 12 px; the inliers are projections moved by at most
    noise_px in each image; the rows are shuffled."""
    h, w = int(size[0]), int(size[1])
    n_in, n_out, pool = _split("planar_scene", k, outlier_fraction, noise_px)
    u = synth.uniform24(int(seed) + (0x9A7A if rotation_only else 0x91A9), 16 + 8 * pool).astype(np.float64)
    cam, u = u[:16], u[16:].reshape(8, pool)
    kk, rot = _scene_camera(cam, h, w)
    kinv = np.linalg.inv(kk)
    if rotation_only:
        h_true = kk @ rot @ kinv
    else:  # the plane n · X = d in the first camera's frame, X' = R X + t: H = K (R + t nᵀ / d) K⁻¹
        t = _scene_shift(cam)
        n = np.array([-0.6 * (cam[6] - 0.5), -0.6 * (cam[7] - 0.5), 1.0])
        d = 5.0 + 4.0 * cam[8]
        h_true = kk @ (rot + np.outer(t, n) / d) @ kinv
    h_true = _unit(h_true)
    # inliers: a pixel of image 0 through H_true
    p0 = np.stack([u[0] * (w - 1), u[1] * (h - 1)], 1)
    q = np.concatenate([p0, np.ones((pool, 1))], 1) @ h_true.T
    p1 = q[:, :2] / q[:, 2:3]
    ok = (q[:, 2] * h_true[2, 2] > 0) & (p1[:, 0] >= 0) & (p1[:, 0] <= w - 1) & (p1[:, 1] >= 0) & (p1[:, 1] <= h - 1)
    o0 = np.stack([u[2] * (w - 1), u[3] * (h - 1)], 1)
    o1 = np.stack([u[4] * (w - 1), u[5] * (h - 1)], 1)
    return _rows_of("planar_scene", seed, n_in, n_out, noise_px, p0, p1, ok, o0, o1, u[6:8],
                    lambda a, b: _transfer(h_true, a, b), h_true)


def _scene_pose(seed: int, k: int, size, stream_seed: int, rows: int):
    h, w = int(size[0]), int(size[1])
    cam = synth.uniform24(stream_seed, 16 + rows * (16 * k + 64)).astype(np.float64)[:16]
    kk, rot = _scene_camera(cam, h, w)
    t = _scene_shift(cam)
    return torch.from_numpy(kk), torch.from_numpy(rot), torch.from_numpy(t / np.linalg.norm(t))


def calibrated_scene(seed: int, k: int, outlier_fraction: float, noise_px: float, size=(480, 640)):
    """two_view_scene(seed, k, outlier_fraction, noise_px, size) with its cameras: (kpts0, kpts1, gt_mask, F_true,
    K [3, 3] float64 (both images'), R [3, 3], t [3] at unit length: X1 = R X0 + t). The first four are two_view_scene's
    own, bit for bit: the same random stream."""
    return two_view_scene(seed, k, outlier_fraction, noise_px, size) + _scene_pose(seed, k, size, int(seed), 9)


def calibrated_planar_scene(seed: int, k: int, outlier_fraction: float, noise_px: float, size=(480, 640)):
    """planar_scene(seed, k, outlier_fraction, noise_px, size) (the moved camera, not the rotation-only one) with its
    cameras: (kpts0, kpts1, gt_mask, H_true, K, R, t) as calibrated_scene's."""
    return planar_scene(seed, k, outlier_fraction, noise_px, size) + _scene_pose(seed, k, size, int(seed) + 0x91A9, 8)


def _inside(q: np.ndarray, h: int, w: int):
    """(pixels, seen) of camera points q [n, 3] already multiplied by K."""
    with np.errstate(all="ignore"):
        p = q[:, :2] / q[:, 2:3]
    return p, (q[:, 2] > 0.5) & (p[:, 0] >= 0) & (p[:, 0] <= w - 1) & (p[:, 1] >= 0) & (p[:, 1] <= h - 1)


def absolute_scene(seed: int, k: int, outlier_fraction: float, noise_px: float, planar: bool = False, size=(480, 640)):
    """A map and a pinhole camera that sees it (size = (h, w), focal length w; the camera turned and moved sideways from
    the map's frame as two_view_scene's second camera is), from synth.uniform24: (points [k, 3] fp32, kpts [k, 2] fp32,
    gt_mask [k] bool, K [3, 3], R [3, 3], t [3] float64: X_c = R X + t, t at the map's scale, not normalised). The map
    points lie at depths 4 to 12 along the rays of the map frame's own camera; planar: on one plane (a depth of 5 to 9 at
    the image centre, tilted by up to 0.3 in x and in y). round(k outlier_fraction) rows are outliers: a map point paired
    with a uniform pixel further than 12 px from its projection; the inliers are projections moved by at most noise_px;
    the rows are shuffled."""
    h, w = int(size[0]), int(size[1])
    n_in, n_out, pool = _split("absolute_scene", k, outlier_fraction, noise_px)
    u = synth.uniform24(int(seed) + (0xAB51 if planar else 0xAB50), 16 + 10 * pool).astype(np.float64)
    cam, u = u[:16], u[16:].reshape(10, pool)
    kk, rot = _scene_camera(cam, h, w)
    t = _scene_shift(cam)
    kinv = np.linalg.inv(kk)
    normal, dist = np.array([-0.6 * (cam[6] - 0.5), -0.6 * (cam[7] - 0.5), 1.0]), 5.0 + 4.0 * cam[8]

    def lift(ux, uy, ud):
        rays = np.concatenate([np.stack([ux * (w - 1), uy * (h - 1)], 1), np.ones((pool, 1))], 1) @ kinv.T
        depth = dist / (rays @ normal) if planar else 4.0 + 8.0 * ud
        return rays * depth[:, None]

    xin, xout = lift(u[0], u[1], u[2]), lift(u[3], u[4], u[5])
    pin, ok = _inside((xin @ rot.T + t) @ kk.T, h, w)
    pix = np.stack([u[6] * (w - 1), u[7] * (h - 1)], 1)
    intr = np.array([kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]])
    with np.errstate(all="ignore"):
        far = np.nonzero(np.sqrt(_reproject(rot, t, xout, pix, intr)) > 12.0)[0][:n_out]
    keep = np.nonzero(ok)[0][:n_in]
    if len(keep) < n_in or len(far) < n_out:
        raise ValueError("absolute_scene: the pool ran out (a seed whose camera sees too little)")
    noise = (u[8:10, :n_in] * 2.0 - 1.0) * (noise_px / np.sqrt(2.0))
    pts = np.concatenate([xin[keep], xout[far]])
    kp = np.concatenate([pin[keep] + noise.T, pix[far]])
    gt = np.concatenate([np.ones(n_in, dtype=bool), np.zeros(n_out, dtype=bool)])
    order = np.argsort(synth.uniform24(int(seed) + 0x5EED, k), kind="stable")
    return (torch.from_numpy(pts[order].astype(np.float32)), torch.from_numpy(kp[order].astype(np.float32)),
            torch.from_numpy(gt[order]), torch.from_numpy(kk), torch.from_numpy(rot), torch.from_numpy(t))


class ThreeViews(NamedTuple):
    """three_view_scene's result. kpts0, kpts1, kpts2 [k, 2] fp32: the keypoints of the three images; matches_a [k, 2]
    int32: the rows of pair A = (image 0, image 1); matches_b [k, 2] int32: the rows of pair B = (image 1, image 2), column
    0 indexing the shared image 1; gt_a, gt_b [k] bool: the rows that are true correspondences; K [3, 3]; R1, t1 and R2, t2
    float64: X1 = R1 X0 + t1 with |t1| = 1 and X2 = R2 X0 + t2 at that scale."""
    kpts0: torch.Tensor
    kpts1: torch.Tensor
    kpts2: torch.Tensor
    matches_a: torch.Tensor
    matches_b: torch.Tensor
    gt_a: torch.Tensor
    gt_b: torch.Tensor
    K: torch.Tensor
    R1: torch.Tensor
    t1: torch.Tensor
    R2: torch.Tensor
    t2: torch.Tensor


def three_view_scene(seed: int, k: int, outlier_fraction: float, noise_px: float, size=(480, 640)) -> ThreeViews:
    """Three pinhole views in a row (size = (h, w), focal length w; camera 1 turned and moved sideways from camera 0 as
    two_view_scene's second camera is, camera 2 turned again and moved about as far again) of random 3D points, from
    synth.uniform24, the world scaled so that |t1| = 1. Keypoint j of every image belongs to track j. The first
    k - round(k outlier_fraction) tracks are 3D points seen in all three images, each projection moved by at most
    noise_px; the others have uniform pixels in images 0 and 1, further than 12 px from each other's epipolar line:
    pair A's outliers. In pair B the outlier tracks get a uniform pixel in image 2, and so do the last
    round(k outlier_fraction) of the true tracks, further than 12 px from the track's projection: pair B's outliers that
    carry a 3D point. The rows of each pair are the tracks in an order of its own."""
    h, w = int(size[0]), int(size[1])
    n_in, n_out, pool = _split("three_view_scene", k, outlier_fraction, noise_px)
    if n_in - n_out < 4:
        raise ValueError(f"three_view_scene: k and outlier_fraction leave fewer than 4 true rows in pair B: {k}, {outlier_fraction}")
    u = synth.uniform24(int(seed) + 0x3E57, 16 + 15 * pool).astype(np.float64)
    cam, u = u[:16], u[16:].reshape(15, pool)
    kk, r1 = _scene_camera(cam, h, w)
    t1 = _scene_shift(cam)
    _, turn = _scene_camera(cam[6:], h, w)
    r2, t2 = turn @ r1, turn @ t1 + _scene_shift(cam[6:])
    scale = 1.0 / np.linalg.norm(t1)
    t1, t2 = t1 * scale, t2 * scale
    kinv = np.linalg.inv(kk)
    p0 = np.stack([u[0] * (w - 1), u[1] * (h - 1)], 1)
    xyz = (np.concatenate([p0, np.ones((pool, 1))], 1) @ kinv.T) * ((4.0 + 8.0 * u[2]) * scale)[:, None]
    p1, ok1 = _inside((xyz @ r1.T + t1) @ kk.T, h, w)
    p2, ok2 = _inside((xyz @ r2.T + t2) @ kk.T, h, w)
    keep = np.nonzero(ok1 & ok2)[0][:n_in]
    tx = np.array([[0, -t1[2], t1[1]], [t1[2], 0, -t1[0]], [-t1[1], t1[0], 0]])
    f01 = _unit(kinv.T @ tx @ r1 @ kinv)
    o0, o1 = np.stack([u[3] * (w - 1), u[4] * (h - 1)], 1), np.stack([u[5] * (w - 1), u[6] * (h - 1)], 1)
    with np.errstate(all="ignore"):
        far_a = np.nonzero(np.sqrt(_epi(f01, o0, o1)) > 12.0)[0][:n_out]
    if len(keep) < n_in or len(far_a) < n_out:
        raise ValueError("three_view_scene: the pool ran out (a seed whose later views see too little)")
    noise = (u[9:15, :n_in].reshape(3, 2, n_in) * 2.0 - 1.0) * (noise_px / np.sqrt(2.0))
    k0 = np.concatenate([p0[keep] + noise[0].T, o0[far_a]])
    k1 = np.concatenate([p1[keep] + noise[1].T, o1[far_a]])
    k2 = np.concatenate([p2[keep] + noise[2].T, np.zeros((n_out, 2))])
    # image 2's wrong pixels: the last n_out true tracks, then the outlier tracks; each a draw far from the track's own
    # projection (an outlier track has none: any draw serves)
    o2 = np.stack([u[7] * (w - 1), u[8] * (h - 1)], 1)
    draw = 0
    for j in list(range(n_in - n_out, n_in)) + list(range(n_in, k)):
        while j < n_in and np.linalg.norm(o2[draw] - p2[keep[j]]) <= 12.0:
            draw += 1
        k2[j] = o2[draw]
        draw += 1
    order_a = np.argsort(synth.uniform24(int(seed) + 0x5EED, k), kind="stable")
    order_b = np.argsort(synth.uniform24(int(seed) + 0x5EEE, k), kind="stable")
    as32 = lambda a: torch.from_numpy(a.astype(np.float32))  # noqa: E731
    rows = lambda o: torch.from_numpy(np.stack([o, o], 1).astype(np.int32))  # noqa: E731
    return ThreeViews(as32(k0), as32(k1), as32(k2), rows(order_a), rows(order_b), torch.from_numpy(order_a < n_in),
                      torch.from_numpy(order_b < n_in - n_out), torch.from_numpy(kk), torch.from_numpy(r1), torch.from_numpy(t1),
                      torch.from_numpy(r2), torch.from_numpy(t2))
