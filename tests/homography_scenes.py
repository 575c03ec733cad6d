"""What tests/test_homography.py and tests/test_gpu_homography.py share: the seeded planar scenes, their matches
through shuffled keypoint tables, the float64 reference of each (computed once), batches of them, the solve-4
cases and the scoring inputs. A plain module: no fixtures, no GPU. Written like geometry_scenes.py, whose
constants it uses."""
import functools

import numpy as np
import torch

import scene_common
from geometry_scenes import (FORMAT_LIMIT, HYPOTHESES, NOISE, OUTLIERS, PIVOT_MARGIN, REFITS, SCORE_MARGIN, SEED,  # noqa: F401
                             THRESHOLD)

# k -> the scene's seed: picked by a CPU search so that the float64 reference returns exactly gt_mask with every
# inlier below 1.5 px and every outlier above 6 px (test_homography.py asserts it for each)
SCENE_SEEDS = {8: 1, 24: 1, 64: 1, 200: 1, 2048: 1}
ALT_SEEDS = {8: 2, 24: 2, 64: 2, 200: 2}  # a second scene per size (capture and replay), under the same precondition
ROTATION_K, ROTATION_SEED = 64, 1        # the scene of a purely rotated camera


@functools.lru_cache(maxsize=None)
def scene(k, alt=False, rotation=False):
    from lightglue_amd import planar_scene

    seed = ROTATION_SEED if rotation else (ALT_SEEDS if alt else SCENE_SEEDS)[k]
    return planar_scene(seed, k, OUTLIERS, NOISE, rotation_only=rotation)


@functools.lru_cache(maxsize=None)
def pair(k, alt=False, rotation=False):
    """The scene through the matcher's layout: (matches [k, 2] int32, kpts0 [k, 2], kpts1 [k, 2]) with the
    keypoints of each image in a shuffled order of their own; correspondence j is the scene's row j."""
    k0, k1, _, _ = scene(k, alt, rotation)
    return scene_common.shuffled_pair(k0, k1, 2000 + k)


def batch(specs, kmax, alt=False, rotation=False):
    """specs: (scene k, count) per pair -> (matches [P, kmax, 2] with -1 past the count, counts [P], kpts0, kpts1
    [P, max k, 2] zero-padded)."""
    return scene_common.batch_of(lambda k: pair(k, alt, rotation), specs, kmax)


@functools.lru_cache(maxsize=None)
def reference(k, alt=False, rotation=False):
    """homography_reference of the whole scene as one pair."""
    from lightglue_amd import homography_reference

    m, counts, kp0, kp1 = batch(((k, k),), k, alt, rotation)
    return homography_reference(m, counts, kp0, kp1, THRESHOLD, HYPOTHESES, REFITS, SEED)


def errors_px(h, k, alt=False, rotation=False):
    """The transfer error in pixels of each row of the scene under H."""
    from lightglue_amd import transfer_error

    k0, k1, _, _ = scene(k, alt, rotation)
    return transfer_error(h, k0, k1).sqrt()


# ---- lg_ransac_solve4's cases -------------------------------------------------------------------------------------
SOLVE_K, SOLVE_H = 64, 64
ORIENTATION_MARGIN = 1e-3  # the eight orientation determinants (normalised coordinates, O(1)) at least this


@functools.lru_cache(maxsize=None)
def solve_pairs():
    """P = 2 on the k = 64 scene: its rows as they are, and reversed (other samples hit other points)."""
    k0, k1, _, _ = scene(SOLVE_K)
    return (k0, k1), (k0.flip(0).contiguous(), k1.flip(0).contiguous())


@functools.lru_cache(maxsize=None)
def solve_cases():
    """Per pair and hypothesis: (sample, Solve4, kept). kept: the reference does not call the hypothesis
    borderline: a pivot of at least PIVOT_MARGIN, orientation determinants of at least ORIENTATION_MARGIN, and,
    where there is a candidate, one representable in the output's fp32 (its rounding alone keeps the sample
    points' transfer error within FORMAT_LIMIT)."""
    from lightglue_amd import ransac_samples, solve4_reference, transfer_error

    samples = ransac_samples(SEED, SOLVE_H, SOLVE_K, size=4)
    out = []
    for x0, x1 in solve_pairs():
        rows = []
        for s in samples.numpy():
            ref = solve4_reference(x0, x1, s)
            kept = ref.pivot >= PIVOT_MARGIN and ref.orientation >= ORIENTATION_MARGIN
            for h in ref.candidates:
                h32 = torch.from_numpy(h.astype(np.float32))
                kept = kept and float(transfer_error(h32, x0[s], x1[s]).sqrt().max()) <= FORMAT_LIMIT
            rows.append((s, ref, bool(kept)))
        out.append(rows)
    return samples, out


# ---- lg_ransac_score_homography's inputs --------------------------------------------------------------------------
SCORE_COUNTS = (1, 3, 4, 5, 63, 64, 65, 300, 2048)
W0_POINT = (128.0, 64.0)  # a keypoint of image 0 on the line W = 0 of the candidate built for it


@functools.lru_cache(maxsize=None)
def score_inputs():
    """(matches [9, 2048, 2], counts, kpts0, kpts1 [9, 2056, 2], candidates [9, C, 9] fp32, want [9, C] int32): the
    k = 2048 scene per pair (each pair its own shift of the rows), counts SCORE_COUNTS; some match indices out of
    range on both sides (the kernel clamps them, and so does the reference), NaN and Inf keypoints (never
    inliers); candidates: the true H, the refit on the true inliers, 4-point candidates of all-inlier samples, a
    zero matrix, a NaN matrix and a matrix whose W is exactly 0 at W0_POINT (the identity's first two rows over 2,
    the third (2^-10, 0, -128 / 2^10): exact in fp32 and float64 alike), which row 20 of each pair from 63 rows on
    is moved to. Rows whose float64 error under a candidate lies within SCORE_MARGIN of the threshold are moved
    until none does."""
    from lightglue_amd import homography_refit, solve4_reference, transfer_error

    k0, k1, gt, h_true = scene(2048)
    cands = [h_true.numpy(), homography_refit(k0[gt], k1[gt]).numpy()]
    inl = torch.nonzero(gt)[:, 0]
    for i in range(16):
        if len(cands) < 6:
            cands.extend(solve4_reference(k0, k1, inl[4 * i:4 * i + 4].numpy()).candidates[:1])
    assert len(cands) == 6, "score_inputs: the all-inlier samples gave too few candidates"
    w0 = np.array([[0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [2.0 ** -10, 0.0, -W0_POINT[0] * 2.0 ** -10]])
    cands = np.stack(cands + [np.zeros((3, 3)), np.full((3, 3), np.nan), w0]).astype(np.float32)

    def to_w0(p, m, kp0):
        kp0[p, int(m[p, 20, 0])] = torch.tensor(W0_POINT)

    return scene_common.score_inputs(k0, k1, cands, SCORE_COUNTS, transfer_error, THRESHOLD, SCORE_MARGIN, plant=to_w0)
