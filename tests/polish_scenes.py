"""What tests/test_pose_polish.py, tests/test_gpu_pose_polish.py and tools/polish_host_check.py share: the calibrated
scenes at 1 px of noise (where a polish has something to do; essential_scenes.py's are at 0.25 px) through the matcher's
layout, the batch of the six, the float64 references of each (computed once), the turned true pose and the full-width
pair. A plain module: no fixtures, no GPU."""
import functools

import numpy as np
import torch

from geometry_scenes import ALT_SEEDS, HYPOTHESES, OUTLIERS, REFITS, SCENE_SEEDS, SEED, THRESHOLD  # noqa: F401
from essential_scenes import batch_intrinsics, intrinsics, pose_errors_deg  # noqa: F401  (the cameras are the same)
from scene_common import batch_of, shuffled_pair

NOISE = 1.0
POLISH = 10
# (k, alt): on each the float64 reference's mask equals gt_mask before and after the polish, every inlier within
# 1.5 px and every outlier further than 6 px (test_pose_polish.py asserts it)
SIX = ((24, False), (64, False), (200, False), (24, True), (64, True), (200, True))
SIX_KMAX = 200
TURN_R_DEG, TURN_T_DEG = 0.5, 1.0  # the second start: the true pose turned by these
FULL_K = 2048


@functools.lru_cache(maxsize=None)
def scene(k, alt=False):
    """(kpts0, kpts1, gt_mask, F_true, K, R, t) of calibrated_scene at NOISE."""
    from lightglue_amd import calibrated_scene

    seed = 1 if k == FULL_K else (ALT_SEEDS if alt else SCENE_SEEDS)[k]
    return calibrated_scene(seed, k, OUTLIERS, NOISE)


@functools.lru_cache(maxsize=None)
def pair(k, alt=False):
    """The scene through the matcher's layout: (matches [k, 2] int32, kpts0 [k, 2], kpts1 [k, 2]) with the keypoints of
    each image in a shuffled order of their own; correspondence j is the scene's row j."""
    k0, k1 = scene(k, alt)[:2]
    return shuffled_pair(k0, k1, 2000 + k)


def batch(specs, kmax):
    """specs: (k, alt) per pair, each whole -> (matches [P, kmax, 2] with -1 past the count, counts [P], kpts0, kpts1
    [P, max k, 2] zero-padded, intrinsics [P, 2, 4])."""
    return batch_of(lambda s: pair(*s), [((k, alt), k) for k, alt in specs], kmax) + (batch_intrinsics(len(specs)),)


@functools.lru_cache(maxsize=None)
def six():
    return batch(SIX, SIX_KMAX)


@functools.lru_cache(maxsize=None)
def six_ransac():
    """essential_reference of the six."""
    from lightglue_amd import essential_reference

    m, counts, kp0, kp1, intr = six()
    return essential_reference(m, counts, kp0, kp1, intr, THRESHOLD, HYPOTHESES, REFITS, SEED)


def polished(pose, m, counts, kp0, kp1, intr):
    from lightglue_amd import polish_reference

    return polish_reference(pose, m, counts, kp0, kp1, intr, THRESHOLD)


@functools.lru_cache(maxsize=None)
def six_polished():
    """polish_reference of six_ransac()."""
    return polished(six_ransac(), *six())


def turned_pose(r, t, r_deg=TURN_R_DEG, t_deg=TURN_T_DEG):
    """(R, t) float64 numpy: R turned by r_deg about (1, 2, 3), t turned by t_deg about an axis across it."""
    from scipy.spatial.transform import Rotation

    r, t = np.asarray(r, dtype=np.float64), np.asarray(t, dtype=np.float64)
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    across = np.cross(t, [0.0, 0.0, 1.0])
    across /= np.linalg.norm(across)
    return (Rotation.from_rotvec(np.radians(r_deg) * axis).as_matrix() @ r,
            Rotation.from_rotvec(np.radians(t_deg) * across).as_matrix() @ t)


def given_pose(r, t, mask, valid=1):
    """A one-pair PoseResult (fp32 R and t, as the kernel takes them) of a pose and a mask [n]."""
    from lightglue_amd import PoseResult

    mask = torch.as_tensor(mask).to(torch.uint8)[None]
    return PoseResult(torch.zeros((1, 3, 3)), torch.as_tensor(np.asarray(r)).float()[None], torch.as_tensor(np.asarray(t)).float()[None],
                      mask, torch.tensor([int(mask.sum())], dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                      torch.tensor([valid], dtype=torch.int32), torch.zeros(1, dtype=torch.int32))


@functools.lru_cache(maxsize=None)
def full_width():
    """K = 2048: ((matches, counts, kpts0, kpts1, intrinsics), the given pose: gt_mask and the turned true pose)."""
    b = batch(((FULL_K, False),), FULL_K)
    _, _, gt, _, _, r, t = scene(FULL_K)
    return b, given_pose(*turned_pose(r, t), gt)


@functools.lru_cache(maxsize=None)
def full_width_polished():
    b, pose = full_width()
    return polished(pose, *b)


@functools.lru_cache(maxsize=None)
def keep_rule():
    """The k = 64 scene under an all-ones mask (its 16 outliers among the rows) and the reference's pose: the polish
    of that set loses inliers, so the pose comes back as given."""
    b = batch(((64, False),), 64)
    ref = six_ransac()
    return b, given_pose(ref.R[1], ref.t[1], torch.ones(64, dtype=torch.uint8))


def rounded(pose):
    """A float64 PoseResult as the kernel takes it: R and t in fp32."""
    return pose._replace(R=pose.R.float(), t=pose.t.float())


@functools.lru_cache(maxsize=None)
def ragged_given():
    """essential_scenes.ragged() and the pose to polish on it: ragged_reference()'s, rounded to fp32."""
    import essential_scenes as es

    return es.ragged(), rounded(es.ragged_reference())


@functools.lru_cache(maxsize=None)
def ragged_polished():
    b, pose = ragged_given()
    return polished(pose, *b)


RAGGED_FIVE = 2  # the pair of 5 rows: as many residuals as parameters, so no minimiser to compare
