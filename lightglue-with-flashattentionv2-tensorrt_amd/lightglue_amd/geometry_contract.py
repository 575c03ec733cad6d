

"""The float64 contract of the geometric verification (geometry.py's kernels), on the CPU in numpy and scipy: nothing
here touches a GPU or the library.

The fundamental matrix: ``ransac_samples`` (the minimal samples, which the kernel equals bitwise),
``epipolar_error``, ``solve7_reference`` (an SVD null space and ``numpy.roots``, deliberately not the kernel's
elimination and closed form), ``fundamental_refit`` and ``ransac_reference`` (the whole).

The homography x1 ~ H x0: ``ransac_samples(size=4)``, ``transfer_error``, ``solve4_reference`` (an SVD null vector
scaled to the canonical one, not the kernel's elimination), ``homography_refit`` and ``homography_reference``.

The essential matrix and the pose: ``ransac_samples5``, ``solve5_reference`` (an SVD null space, the ten constraints
by generic polynomial products, the eigenvalues of the cubic matrix pencil in the hidden variable: not the kernel's
elimination and degree-10 polynomial), ``essential_refit``, ``pose_from_essential_reference`` and
``essential_reference``.

The three ``*_reference`` are one scheme (``_ransac_pair``: sample, solve, score, the strict winner, the refit rounds)
over a model of a few callables each.

The pose polish and the triangulation: ``sampson_error``, ``polish_pose_reference``
(``scipy.optimize.least_squares(method="lm")`` on a global rotation vector and two angles of t with a numeric
Jacobian, deliberately not the kernel's route: the converged minimiser is what is compared), ``polish_reference`` (a
batch of it) and ``triangulate_reference``.

The absolute pose (a camera against 3D points): ``ransac_samples3``, ``reprojection_error``, ``solve3_reference``
(Grunert's quartic by ``numpy.roots``, the third distance from a quadratic, the pose by an SVD absolute orientation:
not the kernel's bracketed roots, rational third distance and triangle frames), ``absolute_refit_reference`` (scipy's
least squares to its tolerance floor on a global rotation vector and t), ``absolute_pose_reference`` (the whole, a
fourth model of ``_ransac_pair``) and ``link_landmarks_reference`` (the 3D points of one pair onto the rows of the next).
"""
from __future__ import annotations

from typing import NamedTuple, Tuple

import numpy as np
import torch

MAX_HYPOTHESES = 4096
MAX_REFITS = 8
MIN_POLISH_ROWS = 5     # the polish's fixed set needs as many rows as there are parameters
MIN_INLIERS = 8         # a fundamental matrix, and its refit, needs 8 correspondences
MIN_INLIERS_H = 4       # a homography, and its refit, needs 4
MIN_INLIERS_E = 5       # an essential matrix needs 5 (its refit 8, as the fundamental matrix's)
MIN_INLIERS_A = 4       # an absolute pose, and its refit, needs 4 correspondences
MIN_ABSOLUTE_ROWS = 3   # the refit's fixed set needs as many residuals as there are parameters
AREA_EPS = 1e-6         # a P3P sample triangle's area over its longest side squared below this: no candidate
MAX_POINTS = 2048       # kmax, and the keypoints of a shared image
PIVOT_EPS = 1e-6        # a pivot of the 7 x 9 (8 x 9) elimination below this: no candidate
_M32 = 0xFFFFFFFF


class GeometryResult(NamedTuple):
    """F [P, 3, 3] (x1ᵀ F x0 = 0, unit Frobenius norm, the entry of the largest magnitude positive; zeros where
    valid == 0), inliers [P, Kmax] uint8 aligned with the rows of MatchResult.matches (0 past the count),
    num_inliers, valid, best [P] int32 (best: the winning hypothesis, -1 where valid == 0)."""
    F: torch.Tensor
    inliers: torch.Tensor
    num_inliers: torch.Tensor
    valid: torch.Tensor
    best: torch.Tensor


class HomographyResult(NamedTuple):
    """H [P, 3, 3] (x1 ~ H x0, unit Frobenius norm, the entry of the largest magnitude positive; zeros where
    valid == 0), inliers [P, Kmax] uint8 aligned with the rows of MatchResult.matches (0 past the count),
    num_inliers, valid, best [P] int32 (best: the winning hypothesis, -1 where valid == 0). A pair is valid from 4
    inliers on, and a 4-inlier winner is only its own sample: threshold num_inliers before trusting H."""
    H: torch.Tensor
    inliers: torch.Tensor
    num_inliers: torch.Tensor
    valid: torch.Tensor
    best: torch.Tensor


class PoseResult(NamedTuple):
    """E [P, 3, 3] (x1ᵀ E x0 = 0 in camera coordinates, canonical: unit Frobenius norm, the entry of the largest
    magnitude positive), R [P, 3, 3] and t [P, 3] (X1 = R X0 + t, det R = +1, |t| = 1, E ∝ [t]× R), inliers [P, Kmax]
    uint8 aligned with the rows of MatchResult.matches (0 past the count), num_inliers, num_front (the inliers that
    triangulate in front of both cameras under (R, t)), valid, best [P] int32 (best: the winning hypothesis, -1 where
    valid == 0; every other output is zeros there). A pair is valid from 5 inliers on, and a 5-inlier winner is
    only its own sample: threshold num_inliers (and num_front) before trusting the pose."""
    E: torch.Tensor
    R: torch.Tensor
    t: torch.Tensor
    inliers: torch.Tensor
    num_inliers: torch.Tensor
    num_front: torch.Tensor
    valid: torch.Tensor
    best: torch.Tensor


class PolishResult(NamedTuple):
    """The pose polish's outputs. E, R, t, inliers, num_inliers, num_front as PoseResult's; cost [P, 2] fp32: the sum of
    squared Sampson residuals (px²) over the fixed set (the given inliers with a finite residual) under the given
    and under the returned pose; kept [P] int32: 1 where the polished pose is returned (its mask, recomputed over all
    the pair's correspondences, has at least as many inliers as the given one), 0 where the given pose and mask are
    passed through (both costs are then the entering one; every output but R, t and the mask is zeros where the
    given pose was invalid)."""
    E: torch.Tensor
    R: torch.Tensor
    t: torch.Tensor
    inliers: torch.Tensor
    num_inliers: torch.Tensor
    num_front: torch.Tensor
    cost: torch.Tensor
    kept: torch.Tensor


class AbsolutePoseResult(NamedTuple):
    """R [P, 3, 3] and t [P, 3] (X_c = R X + t, det R = +1; t is not normalised: the scale is the map's), inliers
    [P, Kmax] uint8 aligned with the rows of the correspondences (0 past the count), num_inliers, valid, best [P] int32
    (best: the winning hypothesis, -1 where valid == 0; every other output is zeros there). A pair is valid from 4
    inliers on, and a 4-inlier winner is little more than its own sample: threshold num_inliers before trusting the
    pose."""
    R: torch.Tensor
    t: torch.Tensor
    inliers: torch.Tensor
    num_inliers: torch.Tensor
    valid: torch.Tensor
    best: torch.Tensor


class Landmarks(NamedTuple):
    """The 2D-3D correspondences link_landmarks makes of two pairs that share an image: points [P, Kmax_b, 3] (pair A's
    3D points), image [P, Kmax_b, 2] (the new image's keypoints, pixels), rows [P, Kmax_b] int32 (the row of pair B's
    matches each came from, ascending; -1 past the count), counts [P] int32. Points and image are zeros past the
    count."""
    points: torch.Tensor
    image: torch.Tensor
    rows: torch.Tensor
    counts: torch.Tensor


# ---- the minimal samples --------------------------------------------------------------------------------------
def _hash32(seed: int, h: np.ndarray, j: int) -> np.ndarray:
    """The counter-based hash of (seed, hypothesis, draw), uint32 arithmetic: the key folded by odd multipliers,
    then the lowbias32 finaliser."""
    x = ((seed & _M32) * 0x9E3779B1 + h.astype(np.uint64) * 0x85EBCA77 + j * 0xC2B2AE3D + 0x27D4EB2F) & _M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & _M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & _M32
    x ^= x >> 16
    return x


def ransac_samples(seed: int, hypotheses: int, count: int, size: int = 7) -> torch.Tensor:
    """[H, size] int32: hypothesis h's `size` (7: the fundamental matrix, 4: the homography) distinct indices in
    [0, count), in draw order. Draw j is hash32(seed, h, j) % (count - j), moved past the earlier draws in
    ascending order (one more for each earlier draw <= it, the smallest first): for count >= 7 the 4-sample is the
    first four columns of the 7-sample. The pair is not in the key: a pair's result does not depend on its place
    in a batch."""
    seed, hypotheses, count, size = int(seed), int(hypotheses), int(count), int(size)
    if size not in (4, 7):
        raise ValueError(f"ransac_samples: size is 4 or 7, got {size}")
    if count < size or hypotheses < 1:
        raise ValueError(f"ransac_samples: count >= {size} and hypotheses >= 1, got {count} and {hypotheses}")
    return _samples(seed, hypotheses, count, size)


def _samples(seed: int, hypotheses: int, count: int, size: int) -> torch.Tensor:
    h = np.arange(hypotheses, dtype=np.uint64)
    out = np.zeros((hypotheses, size), dtype=np.int64)
    for j in range(size):
        r = (_hash32(seed, h, j) % np.uint64(count - j)).astype(np.int64)
        earlier = np.sort(out[:, :j], axis=1)
        for e in range(j):
            r = r + (r >= earlier[:, e])
        out[:, j] = r
    return torch.from_numpy(out.astype(np.int32))


def ransac_samples5(seed: int, hypotheses: int, count: int) -> torch.Tensor:
    """[H, 5] int32: hypothesis h's five distinct indices in [0, count) for the essential matrix, by
    ransac_samples' rule (count >= 5): for count >= 7 the first five columns of its 7-sample."""
    seed, hypotheses, count = int(seed), int(hypotheses), int(count)
    if count < 5 or hypotheses < 1:
        raise ValueError(f"ransac_samples5: count >= 5 and hypotheses >= 1, got {count} and {hypotheses}")
    return _samples(seed, hypotheses, count, 5)


def ransac_samples3(seed: int, hypotheses: int, count: int) -> torch.Tensor:
    """[H, 3] int32: hypothesis h's three distinct indices in [0, count) for the absolute pose, by ransac_samples'
    rule (count >= 3): for count >= 7 the first three columns of its 7-sample."""
    seed, hypotheses, count = int(seed), int(hypotheses), int(count)
    if count < 3 or hypotheses < 1:
        raise ValueError(f"ransac_samples3: count >= 3 and hypotheses >= 1, got {count} and {hypotheses}")
    return _samples(seed, hypotheses, count, 3)


# ---- the contract's pieces in float64 ---------------------------------------------------------------------------
def _np(t) -> np.ndarray:
    return (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)).astype(np.float64)


def _epi(f: np.ndarray, x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        h0 = np.concatenate([x0, np.ones((len(x0), 1))], 1)
        h1 = np.concatenate([x1, np.ones((len(x1), 1))], 1)
        l1, l0 = h0 @ f.T, h1 @ f
        d2 = (h1 * l1).sum(1) ** 2
        return np.maximum(d2 / (l1[:, 0] ** 2 + l1[:, 1] ** 2), d2 / (l0[:, 0] ** 2 + l0[:, 1] ** 2))


def epipolar_error(F, x0, x1) -> torch.Tensor:
    """The error of each correspondence (x0 [n, 2], x1 [n, 2]) under F [3, 3], in squared pixels, float64 [n]:
    l1 = F x0, l0 = Fᵀ x1, d = x1 · l1, max(d² / (l1x² + l1y²), d² / (l0x² + l0y²)) (OpenCV's for FM_RANSAC).
    An inlier has error <= threshold²; NaN (a degenerate line, a non-finite coordinate) is none."""
    return torch.from_numpy(_epi(_np(F).reshape(3, 3), _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2)))


def _hartley(pts: np.ndarray) -> np.ndarray:
    """T [3, 3]: centroid to 0, mean distance sqrt 2."""
    with np.errstate(all="ignore"):
        c = pts.mean(0)
        s = np.sqrt(2.0) / np.sqrt(((pts - c) ** 2).sum(1)).mean()
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def _apply(t: np.ndarray, pts: np.ndarray) -> np.ndarray:
    return pts * t[0, 0] + t[:2, 2]


def _rows(x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
    """The rows of x1ᵀ F x0 = 0 for F row-major: (x1 x0, x1 y0, x1, y1 x0, y1 y0, y1, x0, y0, 1)."""
    one = np.ones(len(x0))
    return np.stack([x1[:, 0] * x0[:, 0], x1[:, 0] * x0[:, 1], x1[:, 0], x1[:, 1] * x0[:, 0], x1[:, 1] * x0[:, 1],
                     x1[:, 1], x0[:, 0], x0[:, 1], one], 1)


def _unit(f: np.ndarray):
    """f at unit Frobenius norm with the sign rule (the entry of the largest magnitude positive, the lowest index
    among equals), or None where it is zero or not finite."""
    with np.errstate(all="ignore"):
        n = np.sqrt((f * f).sum())
        if not np.isfinite(n) or n == 0.0 or not np.isfinite(1.0 / n):
            return None
        f = f / n
    return -f if f.flat[int(np.argmax(np.abs(f)))] < 0 else f


def elimination_pivots(a: np.ndarray) -> float:
    """The smallest pivot magnitude of the Gauss-Jordan elimination with partial (row) pivoting on the n x 9
    system (7 rows: the 7-point solve, 8: the 4-point), columns 0..n-1 in order: the quantity the contract's
    epsilon is about. NaN where not finite."""
    a = np.array(a, dtype=np.float64)
    low = np.inf
    rows = len(a)
    with np.errstate(all="ignore"):
        for c in range(rows):
            piv = c + int(np.argmax(np.abs(a[c:, c])))
            best = abs(a[piv, c])
            if not best > 0.0:
                return float(best)
            low = min(low, best)
            a[[c, piv]] = a[[piv, c]]
            a[c] /= a[c, c]
            for r in range(rows):
                if r != c:
                    a[r] -= a[r, c] * a[c]
    return float(low)


class Solve7(NamedTuple):
    """candidates [n, 3, 3] float64 in pixels (unit norm, sign rule), in ascending root; roots: the cubic's three
    complex roots (fewer where its leading coefficients vanish); pivot: elimination_pivots of the system."""
    candidates: np.ndarray
    roots: np.ndarray
    pivot: float


def _det_poly(g: np.ndarray, d: np.ndarray) -> np.ndarray:
    """Coefficients (highest first) of det(g + l d) for 3 x 3 g, d: each a sum of determinants of mixed rows."""
    det = np.linalg.det

    def mixed(mask):
        return det(np.stack([d[i] if mask >> i & 1 else g[i] for i in range(3)]))

    return np.array([mixed(7), mixed(3) + mixed(5) + mixed(6), mixed(1) + mixed(2) + mixed(4), mixed(0)])


def solve7_reference(x0, x1, sample) -> Solve7:
    """The 7-point solve of the contract in float64: x0, x1 [n, 2] all correspondences of the pair (the Hartley
    normalisation is over all of them), sample 7 indices. The null space by SVD, brought to the canonical basis
    f1 = (.., 1, 0), f2 = (.., 0, 1) (which fixes the parameter l whatever found the null space), the roots of
    det(l f1 + (1 - l) f2) by numpy.roots, the real ones in ascending order de-normalised to unit norm. A pivot
    below PIVOT_EPS, or anything non-finite, gives no candidate."""
    x0, x1 = _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2)
    idx = np.asarray(sample, dtype=np.int64).reshape(7)
    t0, t1 = _hartley(x0), _hartley(x1)
    a = _rows(_apply(t0, x0[idx]), _apply(t1, x1[idx]))
    none = Solve7(np.zeros((0, 3, 3)), np.zeros((0,), dtype=complex), float("nan"))
    if not np.isfinite(a).all():
        return none
    pivot = elimination_pivots(a)
    null = np.linalg.svd(a)[2][7:9]
    with np.errstate(all="ignore"):
        try:
            basis = np.linalg.solve(null[:, 7:9], null)  # rows end (1, 0) and (0, 1)
        except np.linalg.LinAlgError:
            return Solve7(none.candidates, none.roots, pivot)
    if not np.isfinite(basis).all():
        return Solve7(none.candidates, none.roots, pivot)
    g, d = basis[1].reshape(3, 3), (basis[0] - basis[1]).reshape(3, 3)
    roots = np.roots(_det_poly(g, d)).astype(complex)
    real = sorted(float(r.real) for r in roots if abs(r.imag) <= 1e-12 * max(1.0, abs(r)))
    cands = []
    if pivot >= PIVOT_EPS:
        for lam in real:
            f = _unit(t1.T @ (g + lam * d) @ t0)
            if f is not None:
                cands.append(f)
    return Solve7(np.array(cands).reshape(-1, 3, 3), roots, pivot)


def _refit(x0: np.ndarray, x1: np.ndarray):
    t0, t1 = _hartley(x0), _hartley(x1)
    a = _rows(_apply(t0, x0), _apply(t1, x1))
    if not (np.isfinite(a).all() and np.isfinite(t0).all() and np.isfinite(t1).all()):
        return None
    f = np.linalg.eigh(a.T @ a)[1][:, 0].reshape(3, 3)
    v = np.linalg.svd(f)[2][2]
    return _unit(t1.T @ (f - np.outer(f @ v, v)) @ t0)


def fundamental_refit(x0, x1) -> torch.Tensor:
    """One refit round of the contract on the given correspondences (x0, x1 [n, 2], n >= 8), float64 [3, 3]:
    Hartley normalisation over them, the eigenvector of the smallest eigenvalue of the 9 x 9 normal matrix, rank
    2 by F <- F (I - v vᵀ) with v the smallest right-singular direction, de-normalised to unit norm with the
    sign rule."""
    x0, x1 = _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2)
    if len(x0) < MIN_INLIERS or len(x0) != len(x1):
        raise ValueError(f"fundamental_refit: two sets of n >= {MIN_INLIERS} points, got {len(x0)} and {len(x1)}")
    f = _refit(x0, x1)
    if f is None:
        raise ValueError("fundamental_refit: the correspondences give no finite matrix")
    return torch.from_numpy(f)


# ---- the homography's pieces in float64 -------------------------------------------------------------------------
def _transfer(h: np.ndarray, x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        q = np.concatenate([x0, np.ones((len(x0), 1))], 1) @ h.T
        return (x1[:, 0] - q[:, 0] / q[:, 2]) ** 2 + (x1[:, 1] - q[:, 1] / q[:, 2]) ** 2


def transfer_error(H, x0, x1) -> torch.Tensor:
    """The error of each correspondence (x0 [n, 2], x1 [n, 2]) under H [3, 3] (x1 ~ H x0), in squared pixels,
    float64 [n]: (X, Y, W) = H x0, (x1 - X/W)² + (y1 - Y/W)² (OpenCV's for findHomography with RANSAC). An inlier
    has error <= threshold²; a non-finite error (W = 0, a non-finite coordinate, a zero or NaN H) is none."""
    return torch.from_numpy(_transfer(_np(H).reshape(3, 3), _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2)))


def _rows_h(x0: np.ndarray, x1: np.ndarray) -> np.ndarray:
    """The two rows a point of x1 ~ H x0 for H row-major: (-x0, -y0, -1, 0, 0, 0, x1 x0, x1 y0, x1) and
    (0, 0, 0, -x0, -y0, -1, y1 x0, y1 y0, y1); [2 n, 9], a point's pair adjacent."""
    one, zero = np.ones(len(x0)), np.zeros(len(x0))
    ra = np.stack([-x0[:, 0], -x0[:, 1], -one, zero, zero, zero, x1[:, 0] * x0[:, 0], x1[:, 0] * x0[:, 1], x1[:, 0]], 1)
    rb = np.stack([zero, zero, zero, -x0[:, 0], -x0[:, 1], -one, x1[:, 1] * x0[:, 0], x1[:, 1] * x0[:, 1], x1[:, 1]], 1)
    return np.stack([ra, rb], 1).reshape(-1, 9)


_TRIPLES = ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3))


def _orientations(p: np.ndarray) -> np.ndarray:
    """The 2 x 2 orientation determinant of each of the four triples of four points [4, 2]."""
    return np.array([(p[j, 0] - p[i, 0]) * (p[k, 1] - p[i, 1]) - (p[j, 1] - p[i, 1]) * (p[k, 0] - p[i, 0])
                     for i, j, k in _TRIPLES])


class Solve4(NamedTuple):
    """candidates [n, 3, 3] float64 in pixels (unit norm, sign rule), n 0 or 1; pivot: elimination_pivots of the
    8 x 9 system; orientation: the smallest magnitude of the eight orientation determinants (four triples, two
    images) in normalised coordinates."""
    candidates: np.ndarray
    pivot: float
    orientation: float


def solve4_reference(x0, x1, sample) -> Solve4:
    """The 4-point solve of the contract in float64: x0, x1 [n, 2] all correspondences of the pair (the Hartley
    normalisation is over all of them), sample 4 indices. The null vector of the 8 x 9 system by SVD, scaled to
    the canonical one (h8 = 1 in the normalised frame, which fixes it whatever found the null space),
    de-normalised by T1⁻¹ Hn T0 to unit norm with the sign rule. A pivot of the elimination below PIVOT_EPS (three
    collinear points, a repeated index, a true h8 of 0), a sample whose four triples are not oriented alike in
    both images (the products of the two orientation determinants all positive or all negative: OpenCV's
    checkSubset), or anything non-finite gives no candidate."""
    x0, x1 = _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2)
    idx = np.asarray(sample, dtype=np.int64).reshape(4)
    t0, t1 = _hartley(x0), _hartley(x1)
    n0, n1 = _apply(t0, x0[idx]), _apply(t1, x1[idx])
    a = _rows_h(n0, n1)
    none = np.zeros((0, 3, 3))
    if not np.isfinite(a).all():
        return Solve4(none, float("nan"), float("nan"))
    pivot = elimination_pivots(a)
    d0, d1 = _orientations(n0), _orientations(n1)
    orientation = float(min(np.abs(d0).min(), np.abs(d1).min()))
    prod = np.sign(d0) * np.sign(d1)
    if not (pivot >= PIVOT_EPS and ((prod > 0).all() or (prod < 0).all())):
        return Solve4(none, pivot, orientation)
    v = np.linalg.svd(a)[2][8]
    with np.errstate(all="ignore"):
        hn = (v / v[8]).reshape(3, 3)
        h = _unit(np.linalg.inv(t1) @ hn @ t0) if np.isfinite(hn).all() else None
    return Solve4(none if h is None else h[None], pivot, orientation)


def _refit_h(x0: np.ndarray, x1: np.ndarray):
    t0, t1 = _hartley(x0), _hartley(x1)
    a = _rows_h(_apply(t0, x0), _apply(t1, x1))
    if not (np.isfinite(a).all() and np.isfinite(t0).all() and np.isfinite(t1).all()):
        return None
    hn = np.linalg.eigh(a.T @ a)[1][:, 0].reshape(3, 3)
    with np.errstate(all="ignore"):
        return _unit(np.linalg.inv(t1) @ hn @ t0)


def homography_refit(x0, x1) -> torch.Tensor:
    """One refit round of the homography's contract on the given correspondences (x0, x1 [n, 2], n >= 4), float64
    [3, 3]: Hartley normalisation over them, two rows a point, the eigenvector of the smallest eigenvalue of the
    9 x 9 normal matrix (no rank step), de-normalised by T1⁻¹ Hn T0 to unit norm with the sign rule."""
    x0, x1 = _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2)
    if len(x0) < MIN_INLIERS_H or len(x0) != len(x1):
        raise ValueError(f"homography_refit: two sets of n >= {MIN_INLIERS_H} points, got {len(x0)} and {len(x1)}")
    h = _refit_h(x0, x1)
    if h is None:
        raise ValueError("homography_refit: the correspondences give no finite matrix")
    return torch.from_numpy(h)


# ---- the essential matrix's pieces in float64 -------------------------------------------------------------------
def _intrinsics_ok(k: np.ndarray) -> bool:
    return bool(np.isfinite(k).all() and (k[:, :2] > 0).all())


def camera_coordinates(pts, intrinsics) -> np.ndarray:
    """pts [n, 2] in pixels under (fx, fy, cx, cy) -> ((x - cx) / fx, (y - cy) / fy), float64 [n, 2]."""
    p, k = _np(pts).reshape(-1, 2), _np(intrinsics).reshape(4)
    with np.errstate(all="ignore"):
        return (p - k[2:4]) / k[0:2]


def _kinv(k: np.ndarray) -> np.ndarray:
    return np.array([[1.0 / k[0], 0.0, -k[2] / k[0]], [0.0, 1.0 / k[1], -k[3] / k[1]], [0.0, 0.0, 1.0]])


def essential_to_fundamental(E, intrinsics) -> torch.Tensor:
    """F = K1⁻ᵀ E K0⁻¹ at unit Frobenius norm with the sign rule, float64 [3, 3]: the matrix a candidate E (camera
    coordinates, intrinsics [2, 4] = (fx, fy, cx, cy) of image 0 then image 1) is scored with in pixels."""
    k = _np(intrinsics).reshape(2, 4)
    f = _unit(_kinv(k[1]).T @ _np(E).reshape(3, 3) @ _kinv(k[0]))
    if f is None:
        raise ValueError("essential_to_fundamental: the matrix is zero or not finite")
    return torch.from_numpy(f)


def _f_of_e(e: np.ndarray, k: np.ndarray):
    with np.errstate(all="ignore"):
        return _unit(_kinv(k[1]).T @ e @ _kinv(k[0]))


def _pmul(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """The product of two polynomials in (x, y, z), each an array indexed by the three exponents."""
    out = np.zeros(tuple(i + j - 1 for i, j in zip(a.shape, b.shape)))
    for idx in np.ndindex(*a.shape):
        if a[idx] != 0.0:
            out[idx[0]:idx[0] + b.shape[0], idx[1]:idx[1] + b.shape[1], idx[2]:idx[2] + b.shape[2]] += a[idx] * b
    return out


def essential_constraints(basis: np.ndarray):
    """The ten cubic constraints on E = x basis[0] + y basis[1] + z basis[2] + basis[3] (basis [4, 3, 3]): det E = 0
    and the nine entries of 2 E Eᵀ E - tr(E Eᵀ) E = 0, each a polynomial [4, 4, 4] indexed by the exponents of
    (x, y, z), by generic polynomial products."""
    e = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            p = np.zeros((2, 2, 2))
            p[1, 0, 0], p[0, 1, 0], p[0, 0, 1], p[0, 0, 0] = basis[0, i, j], basis[1, i, j], basis[2, i, j], basis[3, i, j]
            e[i][j] = p
    eet = [[sum(_pmul(e[i][k], e[j][k]) for k in range(3)) for j in range(3)] for i in range(3)]
    tr = eet[0][0] + eet[1][1] + eet[2][2]
    out = [_pmul(e[0][0], _pmul(e[1][1], e[2][2]) - _pmul(e[1][2], e[2][1]))
           - _pmul(e[0][1], _pmul(e[1][0], e[2][2]) - _pmul(e[1][2], e[2][0]))
           + _pmul(e[0][2], _pmul(e[1][0], e[2][1]) - _pmul(e[1][1], e[2][0]))]
    for i in range(3):
        for j in range(3):
            out.append(sum(_pmul(2.0 * eet[i][k] - (tr if i == k else 0.0), e[k][j]) for k in range(3)))
    return out


def essential_residuals(E) -> Tuple[float, float]:
    """(|det E|, the largest magnitude among the entries of 2 E Eᵀ E - tr(E Eᵀ) E) of a 3 x 3 matrix."""
    e = _np(E).reshape(3, 3)
    return float(abs(np.linalg.det(e))), float(np.abs(2.0 * e @ e.T @ e - np.trace(e @ e.T) * e).max())


_XY_MONOMIALS = ((3, 0), (2, 1), (1, 2), (0, 3), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0))


class Solve5(NamedTuple):
    """candidates [n, 3, 3] float64 in camera coordinates (canonical: unit norm, sign rule), ascending in their
    entry [0, 0]; eigenvalues: the finite eigenvalues of the pencil, complex (the hidden variable at every
    solution, real or not); pivot: elimination_pivots of the 5 x 9 system; ratio: its smallest singular value over
    its largest."""
    candidates: np.ndarray
    eigenvalues: np.ndarray
    pivot: float
    ratio: float


def solve5_reference(q0, q1, sample) -> Solve5:
    """The five-point solve of the contract in float64: q0, q1 [n, 2] the pair's correspondences in camera
    coordinates, sample 5 indices. The 4-dimensional null space by SVD; the ten cubic constraints by generic
    polynomial products (essential_constraints); z hidden: C(z) m = 0 for the ten monomials m of (x, y) up to degree
    3, a cubic matrix pencil whose real finite eigenvalues (scipy.linalg.eig on its linearisation) are the
    solutions' z, with (x, y) read off the eigenvector. Deliberately not the kernel's elimination and degree-10
    polynomial. A pivot of the 5 x 9 elimination below PIVOT_EPS, or anything non-finite, gives no candidate."""
    from scipy.linalg import eig

    q0, q1 = _np(q0).reshape(-1, 2), _np(q1).reshape(-1, 2)
    idx = np.asarray(sample, dtype=np.int64).reshape(5)
    a = _rows(q0[idx], q1[idx])
    none = np.zeros((0, 3, 3))
    if not np.isfinite(a).all():
        return Solve5(none, np.zeros((0,), dtype=complex), float("nan"), float("nan"))
    pivot = elimination_pivots(a)
    _, sv, vt = np.linalg.svd(a)
    ratio = float(sv[4] / sv[0]) if sv[0] > 0 else 0.0
    basis = vt[5:9].reshape(4, 3, 3)
    cons = essential_constraints(basis)
    c = np.zeros((4, 10, 10))
    for r, poly in enumerate(cons):
        for m, (ex, ey) in enumerate(_XY_MONOMIALS):
            for d in range(4 - ex - ey):
                c[d, r, m] = poly[ex, ey, d]
    eye, zero = np.eye(10), np.zeros((10, 10))
    lhs = np.block([[zero, eye, zero], [zero, zero, eye], [-c[0], -c[1], -c[2]]])
    rhs = np.block([[eye, zero, zero], [zero, eye, zero], [zero, zero, c[3]]])
    with np.errstate(all="ignore"):
        (alpha, beta), vec = eig(lhs, rhs, homogeneous_eigvals=True)
        finite = np.abs(beta) > 1e-9 * np.abs(alpha)
        values = (alpha[finite] / beta[finite]).astype(complex)
        vec = vec[:, finite]
    cands = []
    if pivot >= PIVOT_EPS:
        for z, v in zip(values, vec.T):
            if abs(z.imag) > 1e-9 * max(1.0, abs(z)):
                continue
            with np.errstate(all="ignore"):
                m = v[:10] / v[9]
                x, y = float(m[7].real), float(m[8].real)
                e = _unit(x * basis[0] + y * basis[1] + float(z.real) * basis[2] + basis[3])
            if e is not None:
                cands.append(e)
    cands.sort(key=lambda e: e[0, 0])
    return Solve5(np.array(cands).reshape(-1, 3, 3), values, pivot, ratio)


def _project_essential(e: np.ndarray) -> np.ndarray:
    u, _, vt = np.linalg.svd(e)
    return u @ np.diag([1.0, 1.0, 0.0]) @ vt


def _refit_e(q0: np.ndarray, q1: np.ndarray):
    t0, t1 = _hartley(q0), _hartley(q1)
    a = _rows(_apply(t0, q0), _apply(t1, q1))
    if not (np.isfinite(a).all() and np.isfinite(t0).all() and np.isfinite(t1).all()):
        return None
    e = t1.T @ np.linalg.eigh(a.T @ a)[1][:, 0].reshape(3, 3) @ t0
    if not np.isfinite(e).all():
        return None
    return _unit(_project_essential(e))


def essential_refit(q0, q1) -> torch.Tensor:
    """One refit round of the essential matrix's contract on the given correspondences in camera coordinates (q0,
    q1 [n, 2], n >= 8), float64 [3, 3]: Hartley normalisation over them, the eigenvector of the smallest eigenvalue
    of the 9 x 9 normal matrix, de-normalised, then the nearest essential matrix (singular values (1, 1, 0)),
    canonical (unit norm, sign rule)."""
    q0, q1 = _np(q0).reshape(-1, 2), _np(q1).reshape(-1, 2)
    if len(q0) < MIN_INLIERS or len(q0) != len(q1):
        raise ValueError(f"essential_refit: two sets of n >= {MIN_INLIERS} points, got {len(q0)} and {len(q1)}")
    e = _refit_e(q0, q1)
    if e is None:
        raise ValueError("essential_refit: the correspondences give no finite matrix")
    return torch.from_numpy(e)


def _depths(r: np.ndarray, t: np.ndarray, q0: np.ndarray, q1: np.ndarray):
    """The depths (d0, d1) of each correspondence's midpoint triangulation under X1 = R X0 + t: the least-squares
    solution of d0 R a - d1 b = -t for the rays a = (q0, 1), b = (q1, 1)."""
    a = np.concatenate([q0, np.ones((len(q0), 1))], 1) @ r.T
    b = np.concatenate([q1, np.ones((len(q1), 1))], 1)
    with np.errstate(all="ignore"):
        aa, bb, ab, at, bt = (a * a).sum(1), (b * b).sum(1), (a * b).sum(1), a @ t, b @ t
        det = aa * bb - ab * ab
        return (ab * bt - bb * at) / det, (aa * bt - ab * at) / det


def pose_candidates(E):
    """The four (R, t) of an essential matrix: E = U diag(1, 1, 0) Vᵀ with det U and det V positive, W the quarter
    turn about z: (U W Vᵀ, +u3), (U W Vᵀ, -u3), (U Wᵀ Vᵀ, +u3), (U Wᵀ Vᵀ, -u3)."""
    u, _, vt = np.linalg.svd(_np(E).reshape(3, 3))
    if np.linalg.det(u) < 0:
        u[:, 2] = -u[:, 2]
    if np.linalg.det(vt) < 0:
        vt[2] = -vt[2]
    w = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ra, rb, u3 = u @ w @ vt, u @ w.T @ vt, u[:, 2].copy()
    return [(ra, u3), (ra, -u3), (rb, u3), (rb, -u3)]


def pose_from_essential_reference(E, q0, q1):
    """(R [3, 3], t [3], num_front, the four counts) in float64: of pose_candidates(E), the one under which the
    most correspondences (q0, q1 [n, 2], camera coordinates) triangulate (_depths: the midpoint method) to a
    positive depth in both cameras; the lowest index among equals. X1 = R X0 + t, |t| = 1, det R = +1."""
    q0, q1 = _np(q0).reshape(-1, 2), _np(q1).reshape(-1, 2)
    cands = pose_candidates(E)
    counts = []
    for r, t in cands:
        d0, d1 = _depths(r, t, q0, q1)
        counts.append(int(((d0 > 0) & (d1 > 0)).sum()))
    i = int(np.argmax(counts))
    return torch.from_numpy(cands[i][0].copy()), torch.from_numpy(cands[i][1].copy()), counts[i], counts


# ---- the pose polish and the triangulation in float64 --------------------------------------------------------------
def _skew(t: np.ndarray) -> np.ndarray:
    return np.array([[0.0, -t[2], t[1]], [t[2], 0.0, -t[0]], [-t[1], t[0], 0.0]])


def _sampson(e: np.ndarray, x0: np.ndarray, x1: np.ndarray, k: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        q0 = np.concatenate([(x0 - k[0, 2:4]) / k[0, 0:2], np.ones((len(x0), 1))], 1)
        q1 = np.concatenate([(x1 - k[1, 2:4]) / k[1, 0:2], np.ones((len(x1), 1))], 1)
        l1, l0 = q0 @ e.T, q1 @ e
        d = (q1 * l1).sum(1)
        n2 = (l1[:, 0] / k[1, 0]) ** 2 + (l1[:, 1] / k[1, 1]) ** 2 + (l0[:, 0] / k[0, 0]) ** 2 + (l0[:, 1] / k[0, 1]) ** 2
        return d / np.sqrt(n2)


def sampson_error(E, x0, x1, intrinsics) -> torch.Tensor:
    """The signed Sampson distance in pixels of each correspondence (x0, x1 [n, 2] in pixels) under E [3, 3] (camera
    coordinates, any scale; intrinsics [2, 4]), float64 [n]: with q the camera coordinates, (a, b, .) = E q0,
    (a', b', .) = Eᵀ q1 and d = q1ᵀ E q0, d / sqrt((a / fx1)² + (b / fy1)² + (a' / fx0)² + (b' / fy0)²): the first-order
    distance to the epipolar constraint in the pixels of both images. The polish's cost is the sum of its squares."""
    return torch.from_numpy(_sampson(_np(E).reshape(3, 3), _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2),
                                     _np(intrinsics).reshape(2, 4)))


def _axis_order(t: np.ndarray):
    i = int(np.argmin(np.abs(t)))  # (the lowest index among equals)
    return i, (i + 1) % 3, (i + 2) % 3


def polish_pose_reference(R, t, x0, x1, intrinsics, mask, threshold: float = 3.0) -> PolishResult:
    """PosePolish.refine's contract for one valid pair in float64, run to convergence: R [3, 3], t [3], the pair's
    correspondences x0, x1 [n, 2] in pixels, intrinsics [2, 4], mask [n] (its non-zeros: the given inliers) ->
    PolishResult without the batch dimension (E, R, t, cost float64). The fixed set is the given inliers with a finite
    sampson_error under the given pose; with fewer than 5 of them, bad intrinsics, a non-finite R or t or a zero t
    the pair is passed through. Else the sum of squared sampson_error over the fixed set is minimised by
    scipy.optimize.least_squares(method="lm") at its tolerance floor over a global rotation vector and the two
    angles of t about the axis of its smallest component, with a numeric Jacobian (not the kernel's route: a local
    rotation, a tangent step of t, an analytic Jacobian and a fixed number of rounds). The mask is then recomputed
    over all n correspondences as essential_reference scores a candidate; with at least as many inliers as given the
    polished pose, its mask and its counts are returned (kept = 1), else the given ones (kept = 0, both costs the
    entering one, E = canonical([t]x R) of the given pose)."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation

    r, t = _np(R).reshape(3, 3), _np(t).reshape(3)
    x0, x1, kk = _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2), _np(intrinsics).reshape(2, 4)
    given = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).reshape(-1) != 0
    n_in, thr2 = int(given.sum()), float(threshold) ** 2
    with np.errstate(all="ignore"):
        e_given = _unit(_skew(t) @ r) if np.isfinite(r).all() and np.isfinite(t).all() else None
        length = float(np.linalg.norm(t))
    good = _intrinsics_ok(kk)

    def front_of(rr, tt, rows):
        if not good:
            return 0
        d0, d1 = _depths(rr, tt, camera_coordinates(x0[rows], kk[0]), camera_coordinates(x1[rows], kk[1]))
        return int(((d0 > 0) & (d1 > 0)).sum())

    def result(e, rr, tt, rows, costs, kept):
        return PolishResult(torch.from_numpy(np.zeros((3, 3)) if e is None else e.copy()), torch.from_numpy(rr.copy()),
                            torch.from_numpy(tt.copy()), torch.from_numpy(rows.astype(np.uint8)),
                            torch.tensor(int(rows.sum()), dtype=torch.int32), torch.tensor(front_of(rr, tt, rows), dtype=torch.int32),
                            torch.tensor(costs, dtype=torch.float64), torch.tensor(kept, dtype=torch.int32))

    if not (good and e_given is not None and np.isfinite(length) and length > 0.0):
        return result(e_given, r, t, given, [0.0, 0.0], 0)
    t0 = t / length
    rows = np.nonzero(given)[0]
    rows = rows[np.isfinite(_sampson(_skew(t0) @ r, x0[rows], x1[rows], kk))]
    rot0 = Rotation.from_matrix(r)  # (the nearest rotation: a pose rounded to fp32 is 1e-7 off)
    cost0 = float((_sampson(_skew(t0) @ rot0.as_matrix(), x0[rows], x1[rows], kk) ** 2).sum())
    if len(rows) < MIN_POLISH_ROWS or not np.isfinite(cost0):
        return result(e_given, r, t, given, [cost0, cost0], 0)
    i, j, k = _axis_order(t0)

    def pose(p):
        tt = np.zeros(3)
        tt[i], tt[j], tt[k] = np.cos(p[3]), np.sin(p[3]) * np.cos(p[4]), np.sin(p[3]) * np.sin(p[4])
        return Rotation.from_rotvec(p[:3]).as_matrix(), tt

    def residuals(p):
        rr, tt = pose(p)
        return _sampson(_skew(tt) @ rr, x0[rows], x1[rows], kk)

    p0 = np.concatenate([rot0.as_rotvec(), [np.arccos(np.clip(t0[i], -1.0, 1.0)), np.arctan2(t0[k], t0[j])]])
    sol = least_squares(residuals, p0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
    cost1 = float((sol.fun ** 2).sum())
    r1, t1 = pose(sol.x) if np.isfinite(cost1) and cost1 < cost0 else pose(p0)
    cost1 = cost1 if np.isfinite(cost1) and cost1 < cost0 else cost0
    e1 = _unit(_skew(t1) @ r1)
    f1 = None if e1 is None else _f_of_e(e1, kk)
    again = np.zeros(len(x0), dtype=bool) if f1 is None else _epi(f1, x0, x1) <= thr2
    if f1 is None or int(again.sum()) < n_in:
        return result(e_given, r, t, given, [cost0, cost0], 0)
    return result(e1, r1, t1, again, [cost0, cost1], 1)


def polish_reference(pose, matches, counts, kpts0, kpts1, intrinsics, threshold: float = 3.0) -> PolishResult:
    """PosePolish(threshold).refine for a batch in float64, run to convergence: polish_pose_reference on every pair
    with pose.valid != 0 (over its gathered correspondences and pose.inliers); a pair with valid == 0 returns R, t
    and the mask as given and zeros elsewhere. E, R, t, cost float64."""
    pr, kmax = int(matches.shape[0]), int(matches.shape[1])
    out = PolishResult(torch.zeros((pr, 3, 3), dtype=torch.float64), _as64(pose.R).clone(), _as64(pose.t).clone(),
                       torch.zeros((pr, kmax), dtype=torch.uint8), torch.zeros((pr,), dtype=torch.int32),
                       torch.zeros((pr,), dtype=torch.int32), torch.zeros((pr, 2), dtype=torch.float64),
                       torch.zeros((pr,), dtype=torch.int32))
    for p in range(pr):
        x0, x1 = gather_correspondences(matches[p], int(counts[p]), kpts0[p], kpts1[p])
        n = len(x0)
        given = pose.inliers[p, :n].cpu()
        if not int(pose.valid[p]):
            out.inliers[p, :n] = (given != 0).to(torch.uint8)
            continue
        one = polish_pose_reference(pose.R[p], pose.t[p], x0, x1, intrinsics[p], given, threshold)
        out.E[p], out.R[p], out.t[p], out.cost[p] = one.E, one.R, one.t, one.cost
        out.inliers[p, :n] = one.inliers
        out.num_inliers[p], out.num_front[p], out.kept[p] = one.num_inliers, one.num_front, one.kept
    return out


def _as64(t) -> torch.Tensor:
    return torch.from_numpy(_np(t))


def triangulate_reference(R, t, x0, x1, intrinsics, mask):
    """triangulate's contract for one pair in float64: (points [n, 3], ok [n] uint8). For a row with mask != 0 the
    midpoint method of pose_from_essential_reference: the depths (d0, d1) of _depths, and X = (d0 a + Rᵀ (d1 b - t)) / 2
    in camera 0's frame for the rays a = (q0, 1), b = (q1, 1), at the scale |t| = 1; ok where both depths are
    positive and X is finite. Every other entry is zeros."""
    r, t = _np(R).reshape(3, 3), _np(t).reshape(3)
    x0, x1, kk = _np(x0).reshape(-1, 2), _np(x1).reshape(-1, 2), _np(intrinsics).reshape(2, 4)
    rows = np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask).reshape(-1) != 0
    pts, ok = np.zeros((len(x0), 3)), np.zeros(len(x0), dtype=bool)
    if _intrinsics_ok(kk):
        q0, q1 = camera_coordinates(x0, kk[0]), camera_coordinates(x1, kk[1])
        d0, d1 = _depths(r, t, q0, q1)
        with np.errstate(all="ignore"):
            a = np.concatenate([q0, np.ones((len(q0), 1))], 1)
            b = np.concatenate([q1, np.ones((len(q1), 1))], 1)
            x = 0.5 * (d0[:, None] * a + (d1[:, None] * b - t) @ r)
            ok = rows & (d0 > 0) & (d1 > 0) & np.isfinite(x).all(1)
        pts[ok] = x[ok]
    return torch.from_numpy(pts), torch.from_numpy(ok.astype(np.uint8))


def rotation_angle_deg(ra, rb) -> float:
    """The angle of the rotation Raᵀ Rb in degrees: |Ra - Rb| = 2 sqrt 2 sin(angle / 2) in the Frobenius norm (exact
    for small angles, where the arc cosine of the trace is not)."""
    d = np.linalg.norm(_np(ra).reshape(3, 3) - _np(rb).reshape(3, 3))
    return float(np.degrees(2.0 * np.arcsin(min(1.0, d / (2.0 * np.sqrt(2.0))))))


def direction_angle_deg(ta, tb) -> float:
    """The angle between two directions in degrees: |a - b| = 2 sin(angle / 2) at unit length."""
    a, b = _np(ta).reshape(3), _np(tb).reshape(3)
    return float(np.degrees(2.0 * np.arcsin(min(1.0, np.linalg.norm(a / np.linalg.norm(a) - b / np.linalg.norm(b)) / 2.0))))


def _check_params(threshold, hypotheses, refits) -> None:
    if not 0.0 < float(threshold) <= 1e6:
        raise ValueError(f"threshold must be in (0, 1e6] pixels, got {threshold}")
    if not 1 <= int(hypotheses) <= MAX_HYPOTHESES:
        raise ValueError(f"hypotheses must be in [1, {MAX_HYPOTHESES}], got {hypotheses}")
    if not 0 <= int(refits) <= MAX_REFITS:
        raise ValueError(f"refits must be in [0, {MAX_REFITS}], got {refits}")


def gather_correspondences(matches, count: int, kpts0, kpts1) -> Tuple[np.ndarray, np.ndarray]:
    """One pair's correspondences as the kernels read them: matches [Kmax, 2], kpts0 [K0, 2], kpts1 [K1, 2] ->
    (x0, x1) float64 [count, 2], the count clamped into [0, Kmax] and the indices into range."""
    m = np.asarray(matches.cpu() if isinstance(matches, torch.Tensor) else matches).astype(np.int64)
    k0, k1 = _np(kpts0), _np(kpts1)
    n = min(max(int(count), 0), len(m))
    return k0[np.clip(m[:n, 0], 0, len(k0) - 1)], k1[np.clip(m[:n, 1], 0, len(k1) - 1)]


# ---- the scheme -------------------------------------------------------------------------------------------------------
def _ransac_pair(samples, solve, mask_of, refit, min_valid: int, min_refit: int, refits: int, drop_worse: bool,
                 refit_from_model: bool = False):
    """One pair's RANSAC -> (model, mask, the winning hypothesis), or None where the winner has fewer than min_valid
    inliers. samples: the table, a row a hypothesis; solve(sample): its candidates in scoring order; mask_of(model): the
    inliers [n] bool; refit(mask): a model or None. The winner is the highest count, strictly: the first hypothesis,
    then the first candidate, among equals. Then `refits` rounds over the current inliers: a round with fewer than
    min_refit of them, or without a model, ends them; with drop_worse so does one whose model counts fewer. With
    refit_from_model the refit is iterative and starts at the current model: refit(mask, model)."""
    best_n, best_h, best_m = -1, -1, None
    for h, sample in enumerate(samples):
        for m in solve(sample):
            got = int(mask_of(m).sum())
            if got > best_n:
                best_n, best_h, best_m = got, h, m
    if best_n < min_valid:
        return None
    m, mask = best_m, mask_of(best_m)
    for _ in range(int(refits)):
        if int(mask.sum()) < min_refit:
            break
        again = refit(mask, m) if refit_from_model else refit(mask)
        if again is None:
            break
        mask_again = mask_of(again)
        if drop_worse and int(mask_again.sum()) < int(mask.sum()):
            break
        m, mask = again, mask_again
    return m, mask, best_h


def _blank(result, pr: int, kmax: int, *shapes):
    """A reference's result tuple for pr pairs: float64 zeros [pr, *shape] per shape, the mask, int32 zeros, best = -1."""
    counts = len(result._fields) - len(shapes) - 2
    return result(*(torch.zeros((pr,) + s, dtype=torch.float64) for s in shapes), torch.zeros((pr, kmax), dtype=torch.uint8),
                  *(torch.zeros((pr,), dtype=torch.int32) for _ in range(counts)), torch.full((pr,), -1, dtype=torch.int32))


def ransac_reference(matches, counts, kpts0, kpts1, threshold: float = 3.0, hypotheses: int = 512, refits: int = 2,
                     seed: int = 888) -> GeometryResult:
    """FundamentalRansac(threshold, hypotheses, refits, seed).verify in float64 on the CPU: matches [P, Kmax, 2],
    counts [P], kpts0 [P, K0, 2], kpts1 [P, K1, 2] -> GeometryResult (F float64). The steps are the header's:
    gather and normalise, ransac_samples, solve7_reference, every candidate scored in pixels (the winner: the
    highest count, then the lowest hypothesis, then the lowest root), `refits` rounds of fundamental_refit's
    arithmetic over the current inliers (a round with fewer than 8 keeps F and mask)."""
    _check_params(threshold, hypotheses, refits)
    pr, kmax = int(matches.shape[0]), int(matches.shape[1])
    out = _blank(GeometryResult, pr, kmax, (3, 3))
    thr2 = float(threshold) ** 2
    for p in range(pr):
        x0, x1 = gather_correspondences(matches[p], int(counts[p]), kpts0[p], kpts1[p])
        n = len(x0)
        if n < MIN_INLIERS:
            continue
        won = _ransac_pair(ransac_samples(seed, hypotheses, n).numpy(), lambda s: solve7_reference(x0, x1, s).candidates,
                           lambda f: _epi(f, x0, x1) <= thr2, lambda mask: _refit(x0[mask], x1[mask]),
                           MIN_INLIERS, MIN_INLIERS, refits, False)
        if won is None:
            continue
        f, mask, best_h = won
        out.F[p] = torch.from_numpy(f)
        out.inliers[p, :n] = torch.from_numpy(mask.astype(np.uint8))
        out.num_inliers[p], out.valid[p], out.best[p] = int(mask.sum()), 1, best_h
    return out


def homography_reference(matches, counts, kpts0, kpts1, threshold: float = 3.0, hypotheses: int = 512, refits: int = 2,
                         seed: int = 888) -> HomographyResult:
    """HomographyRansac(threshold, hypotheses, refits, seed).verify in float64 on the CPU: matches [P, Kmax, 2],
    counts [P], kpts0 [P, K0, 2], kpts1 [P, K1, 2] -> HomographyResult (H float64). The steps are the header's:
    gather and normalise, ransac_samples(size=4), solve4_reference, the candidate scored in pixels (the winner: the
    highest count, then the lowest hypothesis), `refits` rounds of homography_refit's arithmetic over the current
    inliers (a round with fewer than 4 keeps H and mask). No Levenberg-Marquardt polish."""
    _check_params(threshold, hypotheses, refits)
    pr, kmax = int(matches.shape[0]), int(matches.shape[1])
    out = _blank(HomographyResult, pr, kmax, (3, 3))
    thr2 = float(threshold) ** 2
    for p in range(pr):
        x0, x1 = gather_correspondences(matches[p], int(counts[p]), kpts0[p], kpts1[p])
        n = len(x0)
        if n < MIN_INLIERS_H:
            continue
        won = _ransac_pair(ransac_samples(seed, hypotheses, n, size=4).numpy(),
                           lambda s: solve4_reference(x0, x1, s).candidates, lambda m: _transfer(m, x0, x1) <= thr2,
                           lambda mask: _refit_h(x0[mask], x1[mask]), MIN_INLIERS_H, MIN_INLIERS_H, refits, False)
        if won is None:
            continue
        m, mask, best_h = won
        out.H[p] = torch.from_numpy(m)
        out.inliers[p, :n] = torch.from_numpy(mask.astype(np.uint8))
        out.num_inliers[p], out.valid[p], out.best[p] = int(mask.sum()), 1, best_h
    return out


def essential_reference(matches, counts, kpts0, kpts1, intrinsics, threshold: float = 3.0, hypotheses: int = 512,
                        refits: int = 2, seed: int = 888) -> PoseResult:
    """EssentialRansac(threshold, hypotheses, refits, seed).verify in float64 on the CPU: matches [P, Kmax, 2],
    counts [P], kpts0 [P, K0, 2], kpts1 [P, K1, 2], intrinsics [P, 2, 4] -> PoseResult (E, R, t float64). The steps
    are the header's: gather, camera coordinates, ransac_samples5, solve5_reference, every candidate scored in
    pixels as essential_to_fundamental's F (the winner: the highest count, then the lowest hypothesis, then the
    candidate whose canonical E has the smallest entry [0, 0]), `refits` rounds of essential_refit's arithmetic over
    the current inliers (a round with fewer than 8 stops; a round whose E counts fewer inliers than the current one
    is dropped and the rounds stop: on a planar scene the 8-point fit is degenerate and the five-point winner
    stays), the pose by pose_from_essential_reference over the inliers. A pair with fewer than 5 correspondences, or with an intrinsic
    that is not finite or a focal length <= 0, is invalid."""
    _check_params(threshold, hypotheses, refits)
    pr, kmax = int(matches.shape[0]), int(matches.shape[1])
    out = _blank(PoseResult, pr, kmax, (3, 3), (3, 3), (3,))
    thr2 = float(threshold) ** 2
    for p in range(pr):
        x0, x1 = gather_correspondences(matches[p], int(counts[p]), kpts0[p], kpts1[p])
        kk = _np(intrinsics[p]).reshape(2, 4)
        n = len(x0)
        if n < MIN_INLIERS_E or not _intrinsics_ok(kk):
            continue
        q0, q1 = camera_coordinates(x0, kk[0]), camera_coordinates(x1, kk[1])

        def mask_of(e):
            f = _f_of_e(e, kk)
            return np.zeros(n, dtype=bool) if f is None else _epi(f, x0, x1) <= thr2

        won = _ransac_pair(ransac_samples5(seed, hypotheses, n).numpy(), lambda s: solve5_reference(q0, q1, s).candidates,
                           mask_of, lambda mask: _refit_e(q0[mask], q1[mask]), MIN_INLIERS_E, MIN_INLIERS, refits, True)
        if won is None:
            continue
        e, mask, best_h = won
        r, t, front, _ = pose_from_essential_reference(e, q0[mask], q1[mask])
        out.E[p], out.R[p], out.t[p] = torch.from_numpy(e), r, t
        out.inliers[p, :n] = torch.from_numpy(mask.astype(np.uint8))
        out.num_inliers[p], out.num_front[p], out.valid[p], out.best[p] = int(mask.sum()), front, 1, best_h
    return out


# ---- the absolute pose in float64 ----------------------------------------------------------------------------------------
def _camera_ok(k: np.ndarray) -> bool:
    return bool(np.isfinite(k).all() and (k[:2] > 0).all())


def _reproject(r: np.ndarray, t: np.ndarray, pts: np.ndarray, img: np.ndarray, k: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        c = pts @ r.T + t
        err = (k[0] * c[:, 0] / c[:, 2] + k[2] - img[:, 0]) ** 2 + (k[1] * c[:, 1] / c[:, 2] + k[3] - img[:, 1]) ** 2
        return np.where(c[:, 2] > 0, err, np.inf)


def reprojection_error(R, t, X, x, intrinsics) -> torch.Tensor:
    """The error of each 2D-3D correspondence (X [n, 3], x [n, 2] in pixels) under the pose (R [3, 3], t [3]:
    X_c = R X + t) and the camera intrinsics [4] = (fx, fy, cx, cy), in squared pixels, float64 [n]:
    (fx X_c / Z_c + cx - x)² + (fy Y_c / Z_c + cy - y)², +inf at a depth Z_c <= 0. An inlier has error <= threshold²; a NaN
    (a non-finite coordinate) is none."""
    return torch.from_numpy(_reproject(_np(R).reshape(3, 3), _np(t).reshape(3), _np(X).reshape(-1, 3), _np(x).reshape(-1, 2),
                                       _np(intrinsics).reshape(4)))


class Solve3(NamedTuple):
    """R [n, 3, 3], t [n, 3] float64: the candidates in ascending |R X_s0 + t|; roots: the quartic's four complex roots
    (fewer where its leading coefficients vanish); area: the sample triangle's area over its longest side squared."""
    R: np.ndarray
    t: np.ndarray
    roots: np.ndarray
    area: float


def _absolute_orientation(a: np.ndarray, b: np.ndarray):
    """(R, t) with b ~ R a + t for point sets [n, 3], det R = +1 (Kabsch / Umeyama without scale, by SVD)."""
    ca, cb = a.mean(0), b.mean(0)
    u, _, vt = np.linalg.svd((b - cb).T @ (a - ca))
    d = np.diag([1.0, 1.0, np.sign(np.linalg.det(u @ vt))])
    r = u @ d @ vt
    return r, cb - r @ ca


def solve3_reference(points, image, intrinsics, sample) -> Solve3:
    """The P3P solve of the contract in float64: points [n, 3], image [n, 2] (pixels) all correspondences of the pair,
    intrinsics [4], sample 3 indices. Bearings f_i: the unit vectors of ((x - cx) / fx, (y - cy) / fy, 1). With the
    camera distances s1, s2 = u s1, s3 = v s1 and the law of cosines on the three sides, Grunert's quartic in u by
    generic polynomial products, its roots by numpy.roots; for each real root u > 0 the two v of the quadratic
    v² - 2 c13 v + 1 - E q(u) = 0, the one that fits the third side better, (u, v) then polished by three Newton steps on the
    two conics; s1 = |X1 - X2| / sqrt(q(u)); the pose by an SVD
    absolute orientation of the three camera points s_i f_i onto the map points. Deliberately not the kernel's
    bracketed root finding, rational v and triangle frames. No candidate: anything non-finite, a sample triangle whose
    area over its longest side squared is below AREA_EPS, u or v <= 0, or a sample point at depth <= 0 under the
    candidate. The candidates are in ascending |R X_s0 + t|."""
    pts, img, k = _np(points).reshape(-1, 3), _np(image).reshape(-1, 2), _np(intrinsics).reshape(4)
    idx = np.asarray(sample, dtype=np.int64).reshape(3)
    x, px = pts[idx], img[idx]
    none = Solve3(np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros((0,), dtype=complex), float("nan"))
    with np.errstate(all="ignore"):
        f = np.concatenate([(px - k[2:4]) / k[0:2], np.ones((3, 1))], 1)
        f = f / np.linalg.norm(f, axis=1, keepdims=True)
        sides = np.array([((x[1] - x[0]) ** 2).sum(), ((x[2] - x[0]) ** 2).sum(), ((x[2] - x[1]) ** 2).sum()])
        area = 0.5 * np.linalg.norm(np.cross(x[1] - x[0], x[2] - x[0])) / sides.max()
    if not (np.isfinite(f).all() and np.isfinite(x).all() and np.isfinite(area)):
        return none
    if not area >= AREA_EPS:
        return Solve3(none.R, none.t, none.roots, float(area))
    c12, c13, c23 = float(f[0] @ f[1]), float(f[0] @ f[2]), float(f[1] @ f[2])
    ee, ff = sides[1] / sides[0], sides[2] / sides[0]
    q = np.array([1.0, -2.0 * c12, 1.0])                      # q(u), highest power first
    n = np.polyadd(np.array([1.0, 0.0, -1.0]), (ee - ff) * q)  # N(u)
    d = np.array([2.0 * c23, -2.0 * c13])                     # D(u)
    quartic = np.polyadd(np.polysub(np.polymul(n, n), 2.0 * c13 * np.polymul(n, d)),
                         np.polymul(np.polysub([1.0], ee * q), np.polymul(d, d)))
    if not np.isfinite(quartic).all():
        return Solve3(none.R, none.t, none.roots, float(area))
    roots = np.roots(quartic).astype(complex)
    cands = []
    for z in roots:
        if abs(z.imag) > 1e-9 * max(1.0, abs(z)) or not z.real > 0.0:
            continue
        u = float(z.real)
        qu = 1.0 - 2.0 * c12 * u + u * u
        disc = c13 * c13 - (1.0 - ee * qu)
        both = [c13 + sg * np.sqrt(max(disc, 0.0)) for sg in (1.0, -1.0)]
        v = min(both, key=lambda w: abs(w * w - 2.0 * c23 * u * w + u * u - ff * qu))
        for _ in range(3):  # Newton on the two conics in (u, v): the square root loses digits where the two v are close
            qu, dq = 1.0 - 2.0 * c12 * u + u * u, 2.0 * u - 2.0 * c12
            fa, fb = v * v - 2.0 * c13 * v + 1.0 - ee * qu, v * v - 2.0 * c23 * u * v + u * u - ff * qu
            jac = np.array([[-ee * dq, 2.0 * v - 2.0 * c13], [-2.0 * c23 * v + 2.0 * u - ff * dq, 2.0 * v - 2.0 * c23 * u]])
            with np.errstate(all="ignore"):
                try:
                    step = np.linalg.solve(jac, [fa, fb])
                except np.linalg.LinAlgError:
                    break
            if not np.isfinite(step).all():
                break
            u, v = u - step[0], v - step[1]
        qu = 1.0 - 2.0 * c12 * u + u * u
        with np.errstate(all="ignore"):
            s1 = np.sqrt(sides[0] / qu)
            y = np.array([s1, u * s1, v * s1])[:, None] * f
        if not (v > 0.0 and np.isfinite(y).all()):
            continue
        r, t = _absolute_orientation(x, y)
        if not (np.isfinite(r).all() and np.isfinite(t).all() and ((x @ r.T + t)[:, 2] > 0).all()):
            continue
        cands.append((float(np.linalg.norm(r @ x[0] + t)), r, t))
    cands.sort(key=lambda c: c[0])
    return Solve3(np.array([c[1] for c in cands]).reshape(-1, 3, 3), np.array([c[2] for c in cands]).reshape(-1, 3), roots,
                  float(area))


def absolute_refit_reference(R, t, X, x, intrinsics):
    """One refit round of the absolute pose's contract in float64, run to convergence: from the pose (R, t) over the
    given correspondences (X [n, 3], x [n, 2]: the round's current inliers) -> (R, t), or None. The fixed set is the rows
    with a finite residual at a positive depth under the given pose; with fewer than 3 of them, or a pose that is not
    finite, there is no refit. Else Σ squared reprojection error in px² over the fixed set is minimised by
    scipy.optimize.least_squares(method="lm") at its tolerance floor over a global rotation vector and t with a numeric
    Jacobian (not the kernel's route: a local rotation, an analytic Jacobian and a fixed number of rounds); the given
    pose comes back where the minimiser's cost is not below it."""
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation

    r, t = _np(R).reshape(3, 3), _np(t).reshape(3)
    pts, img, k = _np(X).reshape(-1, 3), _np(x).reshape(-1, 2), _np(intrinsics).reshape(4)
    if not (np.isfinite(r).all() and np.isfinite(t).all()):
        return None
    rows = np.isfinite(_reproject(r, t, pts, img, k))
    if int(rows.sum()) < MIN_ABSOLUTE_ROWS:
        return None
    pts, img = pts[rows], img[rows]

    def residuals(p):
        c = pts @ Rotation.from_rotvec(p[:3]).as_matrix().T + p[3:]
        with np.errstate(all="ignore"):
            return np.concatenate([k[0] * c[:, 0] / c[:, 2] + k[2] - img[:, 0], k[1] * c[:, 1] / c[:, 2] + k[3] - img[:, 1]])

    rot0 = Rotation.from_matrix(r)  # (the nearest rotation)
    p0 = np.concatenate([rot0.as_rotvec(), t])
    cost0 = float((residuals(p0) ** 2).sum())
    if not np.isfinite(cost0):
        return None
    sol = least_squares(residuals, p0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=4000)
    cost1 = float((sol.fun ** 2).sum())
    p1 = sol.x if np.isfinite(cost1) and cost1 < cost0 else p0
    return Rotation.from_rotvec(p1[:3]).as_matrix(), p1[3:].copy()


def absolute_pose_reference(points, image, counts, intrinsics, threshold: float = 3.0, hypotheses: int = 512,
                            refits: int = 2, seed: int = 888) -> AbsolutePoseResult:
    """AbsolutePoseRansac(threshold, hypotheses, refits, seed).localize in float64 on the CPU: points [P, Kmax, 3],
    image [P, Kmax, 2], counts [P], intrinsics [P, 4] -> AbsolutePoseResult (R, t float64). The steps are the header's:
    ransac_samples3, solve3_reference, every candidate scored by reprojection_error with a positive depth (the winner:
    the highest count, then the lowest hypothesis, then the candidates' order), `refits` rounds of
    absolute_refit_reference from the current pose over the current inliers (a round with fewer than 4 stops; a round
    whose pose counts fewer inliers than the current one is dropped and the rounds stop). A pair with fewer than 4
    correspondences, or with an intrinsic that is not finite or a focal length <= 0, is invalid."""
    _check_params(threshold, hypotheses, refits)
    pr, kmax = int(points.shape[0]), int(points.shape[1])
    out = _blank(AbsolutePoseResult, pr, kmax, (3, 3), (3,))
    thr2 = float(threshold) ** 2
    for p in range(pr):
        n = min(max(int(counts[p]), 0), kmax)
        pts, img, kk = _np(points[p])[:n].reshape(-1, 3), _np(image[p])[:n].reshape(-1, 2), _np(intrinsics[p]).reshape(4)
        if n < MIN_INLIERS_A or not _camera_ok(kk):
            continue

        def solve(s):
            got = solve3_reference(pts, img, kk, s)
            return list(zip(got.R, got.t))

        def mask_of(m):
            with np.errstate(all="ignore"):
                return _reproject(m[0], m[1], pts, img, kk) <= thr2

        won = _ransac_pair(ransac_samples3(seed, hypotheses, n).numpy(), solve, mask_of,
                           lambda mask, m: absolute_refit_reference(m[0], m[1], pts[mask], img[mask], kk),
                           MIN_INLIERS_A, MIN_INLIERS_A, refits, True, refit_from_model=True)
        if won is None:
            continue
        (r, t), mask, best_h = won
        out.R[p], out.t[p] = torch.from_numpy(np.array(r)), torch.from_numpy(np.array(t))
        out.inliers[p, :n] = torch.from_numpy(mask.astype(np.uint8))
        out.num_inliers[p], out.valid[p], out.best[p] = int(mask.sum()), 1, best_h
    return out


def link_landmarks_reference(matches_a, counts_a, points_a, ok_a, matches_b, counts_b, kpts_b1, side_a: int = 1,
                             num_shared: int = MAX_POINTS) -> Landmarks:
    """link_landmarks' contract on the CPU: matches_a [P, Ka, 2], counts_a [P], points_a [P, Ka, 3], ok_a [P, Ka]
    (triangulate's outputs for pair A), matches_b [P, Kb, 2], counts_b [P], kpts_b1 [P, K1, 2] -> Landmarks. A row r of
    A below its count with ok_a != 0 owns the shared keypoint matches_a[r, side_a] (clamped into [0, num_shared)), the
    lowest row where several name one; a row k of B below its count is linked iff its shared keypoint matches_b[k, 0]
    (clamped) has an owner. The linked rows in ascending k: the owner's point (the same bits), the new image's keypoint
    kpts_b1[matches_b[k, 1]] (clamped), and k; zeros and -1 past their number."""
    ma, mb = np.asarray(matches_a).astype(np.int64), np.asarray(matches_b).astype(np.int64)
    pa, oka, kb1 = np.asarray(points_a), np.asarray(ok_a), np.asarray(kpts_b1)
    pr, ka, kb = ma.shape[0], ma.shape[1], mb.shape[1]
    points, image = np.zeros((pr, kb, 3), dtype=pa.dtype), np.zeros((pr, kb, 2), dtype=kb1.dtype)
    rows, n = np.full((pr, kb), -1, dtype=np.int32), np.zeros((pr,), dtype=np.int32)
    for p in range(pr):
        owner = {}
        for r in range(min(max(int(counts_a[p]), 0), ka)):
            if oka[p, r]:
                owner.setdefault(int(np.clip(ma[p, r, int(side_a)], 0, int(num_shared) - 1)), r)
        pos = 0
        for k in range(min(max(int(counts_b[p]), 0), kb)):
            r = owner.get(int(np.clip(mb[p, k, 0], 0, int(num_shared) - 1)))
            if r is None:
                continue
            points[p, pos], image[p, pos], rows[p, pos] = pa[p, r], kb1[p, int(np.clip(mb[p, k, 1], 0, kb1.shape[1] - 1))], k
            pos += 1
        n[p] = pos
    return Landmarks(torch.from_numpy(points), torch.from_numpy(image), torch.from_numpy(rows), torch.from_numpy(n))
