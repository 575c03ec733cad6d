"""The synthetic image pairs of the geometric verification's tests and tools, from synth.uniform24 alone (numpy, no
GPU): ``two_view_scene`` (random 3D points, for the fundamental matrix), ``planar_scene`` (one plane, or a camera
that only turns, for the homography), and ``calibrated_scene`` / ``calibrated_planar_scene``, the same pairs bit for
bit with their cameras (K, R, t) for the essential matrix and the pose polish. The errors that place the outliers are
the float64 contract's (geometry_contract.py). ``absolute_scene`` is a map of 3D points and one camera that sees it (the
absolute pose), ``three_view_scene`` three cameras in a row and the match rows of the two pairs that share the middle
one (the chain from a relative pose to the next camera's pose in the first pair's frame), ``multi_view_scene`` a window of
up to 8 cameras in a row with a perturbed start (the bundle adjustment), ``sequence_scene`` those cameras and points as
per-view keypoints and per-pair match rows (the sequence window)."""
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


def _rodrigues(w: np.ndarray) -> np.ndarray:
    """exp([w]x)."""
    th = np.linalg.norm(w)
    kx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    a, b = (1.0, 0.5) if th == 0 else (np.sin(th) / th, (1.0 - np.cos(th)) / th ** 2)
    return np.eye(3) + a * kx + b * kx @ kx


class MultiViews(NamedTuple):
    """multi_view_scene's result. obs [V, k, 2] fp32 and seen [V, k] uint8: the observations; K [3, 3]; R [V, 3, 3], t [V, 3]
    and points [k, 3] float64: the true poses (X_v = R_v X + t_v, view 0 the frame, |t1| = 1) and landmarks; R0, t0, points0
    fp32: the perturbed start."""
    obs: torch.Tensor
    seen: torch.Tensor
    K: torch.Tensor
    R: torch.Tensor
    t: torch.Tensor
    points: torch.Tensor
    R0: torch.Tensor
    t0: torch.Tensor
    points0: torch.Tensor


def multi_view_scene(seed: int, views: int, k: int, noise_px: float, miss_fraction: float, size=(480, 640)) -> MultiViews:
    """`views` pinhole cameras in a row (size = (h, w), focal length w), each turned and moved sideways from the one before
    as three_view_scene's are (in smaller steps, so that the last still sees the first's points), the world scaled so that
    |t1| = 1; k random 3D points seen in view 0, from synth.uniform24. Each projection is moved by at most noise_px; seen is
    cleared where the point is out of the image or not in front of the camera, and on a hashed miss_fraction of the rest
    (never in view 0). The start: every pose from 1 on turned by up to 0.01 rad about a seeded axis and shifted by up to
    0.02 (t1 then back at unit length, so the start's gauge is the truth's), every point moved by up to 0.05."""
    h, w = int(size[0]), int(size[1])
    if not 2 <= views <= 8 or k < 1 or noise_px < 0 or not 0.0 <= miss_fraction < 1.0:
        raise ValueError(f"multi_view_scene: bad views / k / noise_px / miss_fraction {views}, {k}, {noise_px}, {miss_fraction}")
    u = synth.uniform24(int(seed) + 0xBA5E, 64 * views + (8 + 3 * views) * k).astype(np.float64)
    cam, u = u[:64 * views].reshape(views, 64), u[64 * views:].reshape(8 + 3 * views, k)
    kk = np.array([[w, 0.0, w / 2.0], [0.0, w, h / 2.0], [0.0, 0.0, 1.0]])
    kinv = np.linalg.inv(kk)
    rs, ts = [np.eye(3)], [np.zeros(3)]
    for v in range(1, views):
        ang = (cam[v, :3] - 0.5) * np.array([0.04, 0.04, 0.04]) + np.array([0.0, 0.05, 0.0])
        step = np.array([-0.5 - 0.2 * cam[v, 3], 0.1 * (cam[v, 4] - 0.5), 0.1 * (cam[v, 5] - 0.5)])
        cx, cy, cz = np.cos(ang)
        sx, sy, sz = np.sin(ang)
        turn = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
                np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
        rs.append(turn @ rs[-1])
        ts.append(turn @ ts[-1] + step)
    scale = 1.0 / np.linalg.norm(ts[1])
    r, t = np.stack(rs), np.stack(ts) * scale
    p0 = np.stack([u[0] * (w - 1), u[1] * (h - 1)], 1)
    xyz = (np.concatenate([p0, np.ones((k, 1))], 1) @ kinv.T) * ((4.0 + 8.0 * u[2]) * scale)[:, None]
    a = noise_px / np.sqrt(2.0)
    obs, seen = np.zeros((views, k, 2)), np.zeros((views, k), dtype=np.uint8)
    for v in range(views):
        p, ok = _inside((xyz @ r[v].T + t[v]) @ kk.T, h, w)
        miss = (u[3 + v] < miss_fraction) & (v > 0)
        obs[v] = np.where(ok[:, None], p, 0.0) + (u[3 + views + 2 * v:5 + views + 2 * v].T * 2.0 - 1.0) * a
        seen[v] = ok & ~miss
    r0, t0 = r.copy(), t.copy()
    for v in range(1, views):
        r0[v] = _rodrigues((cam[v, 8:11] - 0.5) * 0.02 / np.sqrt(3.0) * 2.0) @ r[v]
        t0[v] = t[v] + (cam[v, 11:14] - 0.5) * 0.04 / np.sqrt(3.0)
    t0[1] /= np.linalg.norm(t0[1])
    x0 = xyz + (u[3 + 3 * views:6 + 3 * views].T - 0.5) * 0.1 / np.sqrt(3.0)
    f32 = lambda m: torch.from_numpy(m.astype(np.float32))  # noqa: E731
    return MultiViews(f32(obs), torch.from_numpy(seen), torch.from_numpy(kk), torch.from_numpy(r), torch.from_numpy(t),
                      torch.from_numpy(xyz), f32(r0), f32(t0), f32(x0))


class SequenceViews(NamedTuple):
    """sequence_scene's result. kpts [V, k, 2] fp32: every view's keypoints; matches [V-1, k, 2] int32, counts [V-1] int32 and
    mask [V-1, k] uint8: the rows of pair v = (view v, view v + 1); kp_counts [V] int32; K [3, 3]; R [V, 3, 3], t [V, 3] and
    points [n_true, 3] float64: the truth (multi_view_scene's); n_true: keypoint j < n_true of every view belongs to point
    j; seen [V, n_true] bool: the point is matched in the view; wrong [V, n_true] bool: its pixel there is a wrong one."""
    kpts: torch.Tensor
    matches: torch.Tensor
    counts: torch.Tensor
    mask: torch.Tensor
    kp_counts: torch.Tensor
    K: torch.Tensor
    R: torch.Tensor
    t: torch.Tensor
    points: torch.Tensor
    n_true: int
    seen: torch.Tensor
    wrong: torch.Tensor


def sequence_scene(seed: int, views: int, k: int, outlier_fraction: float, noise_px: float, miss_fraction: float,
                   size=(480, 640)) -> SequenceViews:
    """multi_view_scene(seed, views, n_true, noise_px, miss_fraction)'s cameras and points as a sequence's inputs: k keypoints
    a view and up to k match rows a pair, from synth.uniform24. Keypoint j < n_true = k - round(k outlier_fraction) of every
    view is point j's observation, the others uniform pixels. Pair v's rows: (j, j) for every point seen in both views (a
    miss splits a point's track in two; about one point in seven first appears in a later view); (o, o) for every other
    keypoint, the outlier rows, which chain into tracks of no point; round(k outlier_fraction) / 2 rows that name a
    keypoint some other row names too, with another keypoint on the other side (duplicates, non-mutual rows); from 16
    keypoints on, two rows with an index out of range. From 4 views on, about one point in twenty has a wrong pixel in one
    view from 2 on, 12.5 to 15 px from its observation (further, and a least-squares point leaves every view's threshold): an
    observation its track must drop. The rows of each pair are
    in an order of its own, cut at k, and padded past the count with indices out of range; the mask clears about one row in
    twenty, and every other outlier row."""
    h, w = int(size[0]), int(size[1])
    n_out = int(round(k * outlier_fraction))
    n_true = k - n_out
    if k < 1 or n_true < 1 or n_out < 0:
        raise ValueError(f"sequence_scene: bad k / outlier_fraction {k}, {outlier_fraction}")
    mv = multi_view_scene(seed, views, n_true, noise_px, miss_fraction, size)
    u = synth.uniform24(int(seed) + 0x5E90, 8 * k + 4 * views * k).astype(np.float64)
    pt, u = u[:8 * k].reshape(8, k), u[8 * k:].reshape(4, views, k)
    seen = mv.seen.numpy().astype(bool)
    kpts = np.zeros((views, k, 2))
    kpts[:, :n_true] = mv.obs.numpy()
    kpts[:, n_true:] = np.stack([u[0, :, n_true:] * (w - 1), u[1, :, n_true:] * (h - 1)], -1)
    wrong = np.zeros((views, n_true), dtype=bool)
    for j in range(n_true):
        if views >= 3 and pt[0, j] < 0.15:  # the point first appears in a later view
            seen[:1 + int(pt[1, j] * (views - 2)), j] = False
        v = 2 + int(pt[3, j] * (views - 2))
        if views >= 4 and pt[2, j] < 0.05 and seen[v, j]:
            turn, far = 2.0 * np.pi * u[0, v, j], 12.5 + 2.5 * u[1, v, j]
            kpts[v, j], wrong[v, j] = kpts[v, j] + far * np.array([np.cos(turn), np.sin(turn)]), True
    matches = np.zeros((views - 1, k, 2), dtype=np.int64)
    counts, mask = np.zeros(views - 1, dtype=np.int32), np.ones((views - 1, k), dtype=np.uint8)
    for v in range(views - 1):
        rows = [(j, j) for j in range(n_true) if seen[v, j] and seen[v + 1, j]] + [(o, o) for o in range(n_true, k)]
        first_out = len(rows) - n_out
        rows += [(int(u[2, v, d] * k), int(u[3, v, d] * k)) for d in range(n_out // 2)]
        if k >= 16:
            rows += [(k + 3, 0), (1, -2)]
        order = np.argsort(synth.uniform24(int(seed) + 0x5EED + v, len(rows)), kind="stable")
        clear = np.array([(first_out <= i < first_out + n_out and i % 2 == 0) for i in range(len(rows))]) | (u[2, v, np.arange(len(rows)) % k] < 0.05)
        n = min(len(rows), k)
        matches[v, :n], mask[v, :n], counts[v] = np.array(rows).reshape(-1, 2)[order][:n], ~clear[order][:n], n
        matches[v, n:] = (-1, 1 << 20)
    return SequenceViews(torch.from_numpy(kpts.astype(np.float32)), torch.from_numpy(matches.astype(np.int32)), torch.from_numpy(counts),
                         torch.from_numpy(mask), torch.full((views,), k, dtype=torch.int32), mv.K, mv.R, mv.t, mv.points, n_true,
                         torch.from_numpy(seen), torch.from_numpy(wrong))
