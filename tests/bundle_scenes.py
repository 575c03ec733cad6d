"""The scenes of the bundle adjustment's tests (test_bundle.py, test_gpu_bundle.py) and of tools/bundle_host_check.py, with
their float64 references computed once: multi_view_scene windows against bundle_adjust_reference. numpy and scipy, no GPU."""
import functools

import numpy as np
import torch

from lightglue_amd import bundle_adjust_reference, bundle_fixed_set, multi_view_scene
from lightglue_amd.geometry_contract import rotation_angle_deg

CASES = ((2, 7), (3, 64), (3, 200), (8, 37), (8, 200))  # (views, k): the 5-parameter camera alone, a partial tile, several
NOISE, MISS = 0.5, 0.2                                  # tiles, and 41 parameters in the padded 48
SEEDS = {2: 23}  # (two views of 7 points: a seed whose window has 6 live landmarks, 24 residuals for 23 parameters)
ITERATIONS = 10
WIDE = (8, 2048)


@functools.lru_cache(maxsize=None)
def scene(views, k, noise=NOISE, miss=MISS):
    return multi_view_scene(SEEDS.get(views, 11), views, k, noise, miss)


def window(s):
    """The call's arguments for one scene, without the batch dimension: (obs, seen, count, intrinsics, R0, t0, points0)."""
    kk = s.K
    intr = torch.tensor([kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]], dtype=torch.float32).repeat(s.obs.shape[0], 1)
    return [s.obs.clone(), s.seen.clone(), torch.tensor(s.obs.shape[1], dtype=torch.int32), intr, s.R0.clone(), s.t0.clone(), s.points0.clone()]


def batch(windows):
    return tuple(torch.stack([w[i] for w in windows]).contiguous() for i in range(7))


@functools.lru_cache(maxsize=None)
def reference(views, k):
    return bundle_adjust_reference(*window(scene(views, k)))


def errors(r, t, x, ref_r, ref_t, ref_x, live):
    """(the worst rotation difference in degrees, the worst |t - t_ref| in units of |t1|, the worst point entry difference
    over the live landmarks)."""
    r, t, x, ref_r, ref_t, ref_x = (np.asarray(a, dtype=np.float64) for a in (r, t, x, ref_r, ref_t, ref_x))
    unit = np.linalg.norm(ref_t[1])
    rot = max(rotation_angle_deg(r[v], ref_r[v]) for v in range(len(r)))
    return rot, float(np.linalg.norm(t - ref_t, axis=1).max() / unit), float(np.abs(x - ref_x)[live].max())


def live_of(w):
    mask, usable, _ = bundle_fixed_set(*w)
    return mask, usable


def dirty_windows():
    """The ragged, dirty batch at V = 3, Lmax = 64: counts 0, 1 and full; a view with 3 observations; a window with a NaN
    pixel, a point behind a camera and a landmark seen once; a focal length of 0."""
    base = lambda: window(scene(3, 64))  # noqa: E731
    out = [base() for _ in range(6)]
    out[0][2] = torch.tensor(0, dtype=torch.int32)
    out[1][2] = torch.tensor(1, dtype=torch.int32)
    keep = torch.nonzero(out[3][1][2])[:3, 0]
    out[3][1][2] = 0
    out[3][1][2, keep] = 1
    d = out[4]
    rows = torch.nonzero(d[1].all(0))[:3, 0].tolist()  # three landmarks seen in every view
    d[0][1, rows[0], 0] = float("nan")
    d[6][rows[1]] = torch.tensor([0.0, 0.0, -5.0])
    d[1][1:, rows[2]] = 0
    out[5][3][1, 0] = 0.0
    return out, rows


@functools.lru_cache(maxsize=None)
def chain_reference():
    """The float64 chain of absolute_scenes.chain_reference with the bundle adjustment appended (window_from_chain ->
    bundle_adjust_reference): (view 2's (deg, |t - t_true|) against the truth without it, the same with it, the window)."""
    import absolute_scenes as ab
    from lightglue_amd import triangulate_reference, window_from_chain
    from lightglue_amd.geometry import gather_correspondences
    from lightglue_amd.matches import MatchResult

    tv, k = ab.three_views(), ab.CHAIN_K
    fine, marks, got, on_b = ab.chain_reference()
    pair_intr, cam_intr = ab.chain_intrinsics()
    cnt = torch.tensor([k], dtype=torch.int32)
    res = lambda m: MatchResult(None, None, None, None, m[None], None, cnt)  # noqa: E731
    x0, x1 = gather_correspondences(tv.matches_a, k, tv.kpts0, tv.kpts1)
    pts, ok = triangulate_reference(fine.R[0], fine.t[0], x0, x1, pair_intr[0], fine.inliers[0, :k])
    w = window_from_chain(res(tv.matches_a), res(tv.matches_b), tv.kpts0[None], tv.kpts1[None], tv.kpts2[None], fine, pts[None],
                          ok[None], marks, got, on_b[None])
    w = [w[0][0], w[1][0], w[2][0], cam_intr.repeat(3, 1), w[3][0], w[4][0], w[5][0]]
    ref = bundle_adjust_reference(*w)
    return ab.pose_errors(got.R[0], got.t[0], tv.R2, tv.t2), ab.pose_errors(ref.R[2], ref.t[2], tv.R2, tv.t2), w, ref
