"""What tests/test_essential.py and tests/test_gpu_essential.py share: the calibrated two-view scenes (the scenes of
geometry_scenes.py with their cameras: the keypoints are the same bits, so its pair() and batch() serve here), their
intrinsics, the float64 reference of each (computed once), the calibrated planar scenes and the solve-5 cases. A
plain module: no fixtures, no GPU."""
import functools

import numpy as np
import torch

from geometry_scenes import (ALT_SEEDS, FORMAT_LIMIT, HYPOTHESES, NOISE, OUTLIERS, REFITS, SCENE_SEEDS, SEED,  # noqa: F401
                             THRESHOLD, batch, pair)
from scene_common import plant_dirty_rows

# The seeds are geometry_scenes.py's: on each the float64 five-point reference returns exactly gt_mask with every
# inlier below 1.5 px and every outlier above 6 px (test_essential.py asserts it), so none had to be replaced.
# (k, seed) of calibrated_planar_scene. Seed 2 at k = 24 was tried and replaced: its reference loses one ground-truth
# inlier at 256 hypotheses.
PLANAR_SEEDS = ((24, 1), (24, 3), (64, 2), (64, 3))


@functools.lru_cache(maxsize=None)
def scene(k, alt=False):
    """(kpts0, kpts1, gt_mask, F_true, K, R, t) of calibrated_scene."""
    from lightglue_amd import calibrated_scene

    return calibrated_scene((ALT_SEEDS if alt else SCENE_SEEDS)[k], k, OUTLIERS, NOISE)


def intrinsics_of(kk):
    """K [3, 3] -> [2, 4] fp32: (fx, fy, cx, cy) of image 0 then image 1 (the scenes' cameras are alike)."""
    return torch.tensor([[kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]]] * 2, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def intrinsics(k=None):
    """The scenes' intrinsics (the same for every k: the image size is)."""
    return intrinsics_of(scene(24)[4])


def batch_intrinsics(pairs):
    return intrinsics()[None].repeat(pairs, 1, 1).contiguous()


def reference_of(m, counts, kp0, kp1, intr=None, hypotheses=HYPOTHESES):
    from lightglue_amd import essential_reference

    intr = batch_intrinsics(m.shape[0]) if intr is None else intr
    return essential_reference(m, counts, kp0, kp1, intr, THRESHOLD, hypotheses, REFITS, SEED)


@functools.lru_cache(maxsize=None)
def reference(k, alt=False):
    """essential_reference of the whole scene as one pair."""
    return reference_of(*batch(((k, k),), k, alt))


def errors_px(e, k, alt=False):
    """The epipolar error in pixels of each row of the scene under E (camera coordinates)."""
    from lightglue_amd import epipolar_error, essential_to_fundamental

    k0, k1 = scene(k, alt)[:2]
    return epipolar_error(essential_to_fundamental(e, intrinsics()), k0, k1).sqrt()


def pose_errors_deg(r, t, r_want, t_want):
    from lightglue_amd.geometry import direction_angle_deg, rotation_angle_deg

    return rotation_angle_deg(r, r_want), direction_angle_deg(t, t_want)


def true_essential(r, t):
    """[t]x R at unit norm, float64 numpy."""
    t = np.asarray(t, dtype=np.float64)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    e = tx @ np.asarray(r, dtype=np.float64)
    return e / np.linalg.norm(e)


# ---- the planar scenes ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def planar(k, seed):
    """(matches [1, k, 2], counts, kpts0, kpts1 [1, k, 2], gt_mask, intrinsics [1, 2, 4]) of calibrated_planar_scene,
    the matches the identity."""
    from lightglue_amd import calibrated_planar_scene

    k0, k1, gt, _, kk, _, _ = calibrated_planar_scene(seed, k, OUTLIERS, NOISE)
    m = torch.arange(k, dtype=torch.int32)[None, :, None].repeat(1, 1, 2)
    return m, torch.tensor([k], dtype=torch.int32), k0[None], k1[None], gt, intrinsics_of(kk)[None]


@functools.lru_cache(maxsize=None)
def planar_reference(k, seed):
    from lightglue_amd import essential_reference

    m, counts, kp0, kp1, _, intr = planar(k, seed)
    return essential_reference(m, counts, kp0, kp1, intr, THRESHOLD, HYPOTHESES, REFITS, SEED)


# ---- lg_ransac_solve5's cases -------------------------------------------------------------------------------------
SOLVE_K, SOLVE_H = 64, 64
SEPARATION = 1e-3     # relative: a complex eigenvalue this far off the real axis, real ones this far apart
SINGULAR_RATIO = 1e-3  # the 5 x 9 system's smallest singular value over its largest


@functools.lru_cache(maxsize=None)
def solve_pairs():
    """P = 2 on the k = 64 scene: its rows as they are, and reversed (other samples hit other points)."""
    k0, k1 = scene(SOLVE_K)[:2]
    return (k0, k1), (k0.flip(0).contiguous(), k1.flip(0).contiguous())


def kept(ref, x0, x1, s, intr):
    """Whether the reference keeps a hypothesis (a Solve5): ten finite eigenvalues, each real or at least SEPARATION
    (relative) off the real axis, the real ones pairwise further apart than SEPARATION (relative), a singular ratio of
    at least SINGULAR_RATIO, and every candidate rounded to fp32 within FORMAT_LIMIT of its sample points."""
    from lightglue_amd import epipolar_error, essential_to_fundamental

    ev = ref.eigenvalues
    if len(ev) != 10 or not ref.ratio >= SINGULAR_RATIO:
        return False
    real = []
    for z in ev:
        scale = max(1.0, abs(z))
        if abs(z.imag) <= 1e-9 * scale:
            real.append(z.real)
        elif abs(z.imag) < SEPARATION * scale:
            return False
    real.sort()
    if any(b - a <= SEPARATION * max(1.0, abs(a), abs(b)) for a, b in zip(real, real[1:])):
        return False
    if len(ref.candidates) != len(real):
        return False
    for e in ref.candidates:
        e32 = torch.from_numpy(e.astype(np.float32)).double()
        if not float(epipolar_error(essential_to_fundamental(e32, intr), x0[s], x1[s]).sqrt().max()) <= FORMAT_LIMIT:
            return False
    return True


@functools.lru_cache(maxsize=None)
def solve_cases():
    """(samples [H, 5], per pair and hypothesis (sample, Solve5, kept))."""
    from lightglue_amd import camera_coordinates, ransac_samples5, solve5_reference

    samples = ransac_samples5(SEED, SOLVE_H, SOLVE_K)
    intr = intrinsics()
    out = []
    for x0, x1 in solve_pairs():
        q0, q1 = camera_coordinates(x0, intr[0]), camera_coordinates(x1, intr[1])
        rows = []
        for s in samples.numpy():
            ref = solve5_reference(q0, q1, s)
            rows.append((s, ref, kept(ref, x0, x1, s, intr)))
        out.append(rows)
    return samples, out


# ---- the ragged batch ---------------------------------------------------------------------------------------------
RAGGED_SPECS = ((24, 0), (24, 4), (24, 5), (24, 7), (24, 8), (24, 24), (64, 64), (200, 200), (200, 200), (64, 64))
RAGGED_KMAX = 208
RAGGED_DIRTY, RAGGED_BAD = 8, 9  # the pair with untrusted indices and keypoints, the pair with a bad intrinsic


@functools.lru_cache(maxsize=None)
def ragged():
    """(matches [10, 208, 2], counts, kpts0, kpts1 [10, 208, 2], intrinsics [10, 2, 4]): counts 0, 4, 5, 7, 8, 24, 64,
    200 under kmax 208; pair 8 is the k = 200 scene with match indices out of range on both sides (the kernel clamps
    them, and so does the reference) and NaN and Inf keypoints (never inliers); pair 9 the k = 64 scene with a
    focal length of 0."""
    m, counts, kp0, kp1 = batch(RAGGED_SPECS, RAGGED_KMAX)
    pad = torch.zeros((len(RAGGED_SPECS), 8, 2))
    kp0, kp1 = torch.cat([kp0, pad], 1), torch.cat([kp1, pad], 1)
    plant_dirty_rows(m[RAGGED_DIRTY], kp0[RAGGED_DIRTY], kp1[RAGGED_DIRTY], 200)
    intr = batch_intrinsics(len(RAGGED_SPECS)).clone()
    intr[RAGGED_BAD, 1, 0] = 0.0
    return m, counts, kp0, kp1, intr


@functools.lru_cache(maxsize=None)
def ragged_reference():
    m, counts, kp0, kp1, intr = ragged()
    return reference_of(m, counts, kp0, kp1, intr)
