"""What tests/test_geometry.py and tests/test_gpu_geometry.py share: the seeded two-view scenes, their matches
through shuffled keypoint tables, the float64 reference of each (computed once), batches of them, the solve-7
cases and the scoring inputs. A plain module: no fixtures, no GPU."""
import functools

import numpy as np
import torch

import scene_common

OUTLIERS, NOISE, HYPOTHESES, REFITS, THRESHOLD, SEED = 0.25, 0.25, 256, 2, 3.0, 888
# k -> the scene's seed: picked so that the float64 reference returns exactly gt_mask with every inlier below
# 1.5 px and every outlier above 6 px (test_geometry.py asserts it for each)
SCENE_SEEDS = {24: 2, 64: 5, 200: 3, 2048: 1}
ALT_SEEDS = {24: 3, 64: 1, 200: 5}  # a second scene per size (capture and replay), under the same precondition


@functools.lru_cache(maxsize=None)
def scene(k, alt=False):
    from lightglue_amd import two_view_scene

    return two_view_scene((ALT_SEEDS if alt else SCENE_SEEDS)[k], k, OUTLIERS, NOISE)


@functools.lru_cache(maxsize=None)
def pair(k, alt=False):
    """The scene through the matcher's layout: (matches [k, 2] int32, kpts0 [k, 2], kpts1 [k, 2]) with the
    keypoints of each image in a shuffled order of their own; correspondence j is the scene's row j."""
    k0, k1, _, _ = scene(k, alt)
    return scene_common.shuffled_pair(k0, k1, 1000 + k)


def batch(specs, kmax, alt=False):
    """specs: (scene k, count) per pair -> (matches [P, kmax, 2] with -1 past the count, counts [P], kpts0, kpts1
    [P, max k, 2] zero-padded)."""
    return scene_common.batch_of(lambda k: pair(k, alt), specs, kmax)


@functools.lru_cache(maxsize=None)
def reference(k, alt=False):
    """ransac_reference of the whole scene as one pair."""
    from lightglue_amd import ransac_reference

    m, counts, kp0, kp1 = batch(((k, k),), k, alt)
    return ransac_reference(m, counts, kp0, kp1, THRESHOLD, HYPOTHESES, REFITS, SEED)


def errors_px(f, k, alt=False):
    """The error in pixels of each row of the scene under F."""
    from lightglue_amd import epipolar_error

    k0, k1, _, _ = scene(k, alt)
    return epipolar_error(f, k0, k1).sqrt()


# ---- lg_ransac_solve7's cases -------------------------------------------------------------------------------------
SOLVE_K, SOLVE_H = 64, 64
ROOT_SEPARATION = 1e-3   # the cubic's roots (all three, complex ones too) pairwise further apart than this
PIVOT_MARGIN = 1e-3      # "well above" PIVOT_EPS = 1e-6
FORMAT_LIMIT = 5e-3      # px: the float64 candidate rounded to fp32 keeps its sample points within this


@functools.lru_cache(maxsize=None)
def solve_pairs():
    """P = 2 on the k = 64 scene: its rows as they are, and reversed (other samples hit other points)."""
    k0, k1, _, _ = scene(SOLVE_K)
    return (k0, k1), (k0.flip(0).contiguous(), k1.flip(0).contiguous())


@functools.lru_cache(maxsize=None)
def solve_cases():
    """Per pair and hypothesis: (sample, Solve7, kept). kept: the reference does not call the hypothesis
    degenerate: three roots pairwise separated by more than ROOT_SEPARATION, a pivot of at least PIVOT_MARGIN, and
    every candidate representable in the output's fp32 (its rounding alone moves no sample point's error past
    FORMAT_LIMIT: a sample point next to a candidate's epipole makes its line direction a difference of rounded
    entries)."""
    from lightglue_amd import epipolar_error, ransac_samples, solve7_reference

    samples = ransac_samples(SEED, SOLVE_H, SOLVE_K)
    out = []
    for x0, x1 in solve_pairs():
        rows = []
        for s in samples.numpy():
            ref = solve7_reference(x0, x1, s)
            r = ref.roots
            kept = len(r) == 3 and min(abs(r[i] - r[j]) for i in range(3) for j in range(i)) > ROOT_SEPARATION
            kept = kept and ref.pivot >= PIVOT_MARGIN and len(ref.candidates) >= 1
            for f in ref.candidates:
                f32 = torch.from_numpy(f.astype(np.float32))
                kept = kept and float(epipolar_error(f32, x0[s], x1[s]).sqrt().max()) <= FORMAT_LIMIT
            rows.append((s, ref, bool(kept)))
        out.append(rows)
    return samples, out


# ---- lg_ransac_score's inputs -------------------------------------------------------------------------------------
SCORE_COUNTS = (1, 63, 64, 65, 300, 2048)
SCORE_MARGIN = 0.02  # px: no float64 error this close to the threshold


@functools.lru_cache(maxsize=None)
def score_inputs():
    """(matches [6, 2048, 2], counts, kpts0, kpts1 [6, 2056, 2], candidates [6, C, 9] fp32, want [6, C] int32): the
    k = 2048 scene per pair (each pair its own shift of the rows), counts SCORE_COUNTS; some match indices out of
    range on both sides (the kernel clamps them, and so does the reference), NaN and Inf keypoints (never
    inliers); candidates: the true F, the refit on the true inliers, 7-point candidates of all-inlier samples, a
    zero matrix and a NaN matrix. Rows whose float64 error under a candidate lies within SCORE_MARGIN of the
    threshold are moved until none does."""
    from lightglue_amd import epipolar_error, fundamental_refit, solve7_reference

    k0, k1, gt, f_true = scene(2048)
    cands = [f_true.numpy(), fundamental_refit(k0[gt], k1[gt]).numpy()]
    inl = torch.nonzero(gt)[:, 0]
    for i in range(4):
        cands.extend(solve7_reference(k0, k1, inl[7 * i:7 * i + 7].numpy()).candidates[:1])
    cands = np.stack(cands + [np.zeros((3, 3)), np.full((3, 3), np.nan)]).astype(np.float32)
    return scene_common.score_inputs(k0, k1, cands, SCORE_COUNTS, epipolar_error, THRESHOLD, SCORE_MARGIN)
