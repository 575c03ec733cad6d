"""What tests/test_absolute.py, tests/test_gpu_absolute.py and tools/absolute_host_check.py share: the absolute pose's
scenes (a map and a camera that sees it), their intrinsics, batches of them, the float64 reference of each (computed
once), the solve-3 cases, the ragged batch, the scoring poses, the link cases and the three-view chain. A plain module:
no fixtures, no GPU."""
import functools

import numpy as np
import torch

from geometry_scenes import FORMAT_LIMIT, HYPOTHESES, NOISE, OUTLIERS, REFITS, SEED, THRESHOLD  # noqa: F401

# k -> the scene's seed: on each the float64 reference returns exactly gt_mask with every inlier below 1.5 px and every
# outlier above 6 px (test_absolute.py asserts it). Seeds 1, 2, 3, .. were tried in order per size and none had to be
# replaced.
SCENE_SEEDS = {24: 1, 64: 1, 200: 1, 2048: 1}
ALT_SEEDS = {24: 2, 64: 2, 200: 2}  # a second scene per size (capture and replay), under the same precondition
PLANAR_SEEDS = ((24, 1), (64, 1))   # (k, seed) of absolute_scene(planar=True)
WIDE_HYPOTHESES = 512                # the class's default, at kmax = 2048
FULL_HYPOTHESES = 4096               # the full grid, on the k = 64 scene
CHAIN_SEED, CHAIN_K, CHAIN_POLISH = 1, 200, 10


@functools.lru_cache(maxsize=None)
def scene(k, alt=False, planar_seed=None):
    """(points [k, 3], kpts [k, 2], gt_mask, K, R, t) of absolute_scene."""
    from lightglue_amd import absolute_scene

    if planar_seed is not None:
        return absolute_scene(planar_seed, k, OUTLIERS, NOISE, planar=True)
    return absolute_scene((ALT_SEEDS if alt else SCENE_SEEDS)[k], k, OUTLIERS, NOISE)


def intrinsics_of(kk):
    """K [3, 3] -> [4] fp32: (fx, fy, cx, cy)."""
    return torch.tensor([kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]], dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def intrinsics():
    """The scenes' intrinsics (the same for every k: the image size is)."""
    return intrinsics_of(scene(24)[3])


def batch_intrinsics(pairs):
    return intrinsics()[None].repeat(pairs, 1).contiguous()


def batch_of(scenes, counts, kmax):
    """scenes: (points, kpts, ..) per pair -> (points [P, kmax, 3], image [P, kmax, 2] zero-padded, counts [P])."""
    pts, img = torch.zeros((len(scenes), kmax, 3)), torch.zeros((len(scenes), kmax, 2))
    for p, s in enumerate(scenes):
        k = min(len(s[0]), kmax)
        pts[p, :k], img[p, :k] = s[0][:k], s[1][:k]
    return pts, img, torch.tensor(list(counts), dtype=torch.int32)


def batch(specs, kmax, alt=False):
    """specs: (scene k, count) per pair."""
    return batch_of([scene(k, alt) for k, _ in specs], [c for _, c in specs], kmax)


def reference_of(points, image, counts, intr=None, hypotheses=HYPOTHESES):
    from lightglue_amd import absolute_pose_reference

    intr = batch_intrinsics(points.shape[0]) if intr is None else intr
    return absolute_pose_reference(points, image, counts, intr, THRESHOLD, hypotheses, REFITS, SEED)


@functools.lru_cache(maxsize=None)
def reference(k, alt=False, hypotheses=HYPOTHESES, planar_seed=None):
    """absolute_pose_reference of the whole scene as one pair."""
    s = scene(k, alt, planar_seed)
    return reference_of(*batch_of([s], [k], k), hypotheses=hypotheses)


def errors_px(r, t, s):
    """The reprojection error in pixels of each row of the scene s under (R, t); +inf behind the camera."""
    from lightglue_amd import reprojection_error

    return reprojection_error(r, t, s[0], s[1], intrinsics_of(s[3])).sqrt()


def pose_errors(r, t, r_want, t_want):
    """(the rotation between R and R_want in degrees, |t - t_want| in the map's units)."""
    from lightglue_amd.geometry import rotation_angle_deg

    a = t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else np.asarray(t, dtype=np.float64)
    b = t_want.detach().cpu().double().numpy() if isinstance(t_want, torch.Tensor) else np.asarray(t_want, dtype=np.float64)
    return rotation_angle_deg(r, r_want), float(np.linalg.norm(a.reshape(3) - b.reshape(3)))


# ---- lg_ransac_solve3's cases -------------------------------------------------------------------------------------
SOLVE_K, SOLVE_H = 64, 64
SEPARATION = 1e-3  # relative: the quartic's roots pairwise this far apart, complex ones this far off the real axis,
                   # no real one this near 0
AREA_MARGIN = 1e-3  # "well above" AREA_EPS = 1e-6


@functools.lru_cache(maxsize=None)
def solve_pairs():
    """P = 2 on the k = 64 scene: its rows as they are, and reversed (other samples hit other points)."""
    pts, kp = scene(SOLVE_K)[:2]
    return (pts, kp), (pts.flip(0).contiguous(), kp.flip(0).contiguous())


def kept(ref, pts, kp, s, intr):
    """Whether the reference keeps a hypothesis (a Solve3): four quartic roots pairwise further apart than SEPARATION
    (relative), the complex ones at least that far off the real axis, no real root within SEPARATION of 0, an area ratio
    above AREA_MARGIN, and every candidate rounded to fp32 within FORMAT_LIMIT of its sample points."""
    from lightglue_amd import reprojection_error

    z = ref.roots
    if len(z) != 4 or not ref.area > AREA_MARGIN:
        return False
    for i in range(4):
        scale = max(1.0, abs(z[i]))
        real = abs(z[i].imag) <= 1e-9 * scale
        if not real and abs(z[i].imag) < SEPARATION * scale:
            return False
        if real and abs(z[i].real) < SEPARATION:
            return False
        for j in range(i):
            if abs(z[i] - z[j]) <= SEPARATION * max(1.0, abs(z[i]), abs(z[j])):
                return False
    for r, t in zip(ref.R, ref.t):
        r32, t32 = torch.from_numpy(r.astype(np.float32)).double(), torch.from_numpy(t.astype(np.float32)).double()
        if not float(reprojection_error(r32, t32, pts[s], kp[s], intr).sqrt().max()) <= FORMAT_LIMIT:
            return False
    return True


@functools.lru_cache(maxsize=None)
def solve_cases():
    """(samples [H, 3], per pair and hypothesis (sample, Solve3, kept))."""
    from lightglue_amd import ransac_samples3, solve3_reference

    samples = ransac_samples3(SEED, SOLVE_H, SOLVE_K)
    intr = intrinsics()
    out = []
    for pts, kp in solve_pairs():
        rows = []
        for s in samples.numpy():
            ref = solve3_reference(pts, kp, intr, s)
            rows.append((s, ref, kept(ref, pts, kp, s, intr)))
        out.append(rows)
    return samples, out


# ---- the ragged batch ---------------------------------------------------------------------------------------------
RAGGED_SPECS = ((24, 0), (24, 3), (24, 4), (24, 5), (24, 24), (64, 64), (200, 200), (200, 200), (64, 64))
RAGGED_KMAX = 208
RAGGED_DIRTY, RAGGED_BAD = 7, 8  # the pair with planted rows, the pair with a focal length of 0


def plant_dirty(points, image, s):
    """Into one pair's rows of the k = 200 scene s, on outlier rows only (the ground-truth mask stays): NaN and Inf
    points and pixels, and three points mirrored through the camera centre onto an inlier's pixel (an inlier but for
    its depth). Returns the planted rows."""
    gt, r, t = s[2].numpy(), s[4].numpy(), s[5].numpy()
    out_rows, in_rows = np.nonzero(~gt)[0], np.nonzero(gt)[0]
    a, b, c, d = (int(x) for x in out_rows[:4])
    points[a, 0] = float("nan")
    points[b, 2] = float("inf")
    image[c, 1] = float("nan")
    image[d, 0] = float("-inf")
    behind = [int(x) for x in out_rows[4:7]]
    for row, src in zip(behind, in_rows[:3]):
        xc = r @ s[0][src].double().numpy() + t
        points[row] = torch.from_numpy(r.T @ (-xc - t)).float()
        image[row] = s[1][src]
    return [a, b, c, d] + behind


@functools.lru_cache(maxsize=None)
def ragged():
    """(points [9, 208, 3], image [9, 208, 2], counts, intrinsics [9, 4]): counts 0, 3, 4, 5, 24, 64, 200, 200 under kmax
    208 (pairs 2 and 3: the k = 24 scene's first inliers, so that 4 and 5 rows make a valid pair); pair 7 is the k = 200 scene with plant_dirty's rows (never inliers); pair 8 the k = 64 scene with a focal
    length of 0."""
    pts, img, counts = batch(RAGGED_SPECS, RAGGED_KMAX)
    first = torch.argsort(~scene(24)[2], stable=True)  # the k = 24 scene's inliers first: 4 and 5 rows that are a pose's
    for p in (2, 3):
        pts[p, :24], img[p, :24] = scene(24)[0][first], scene(24)[1][first]
    plant_dirty(pts[RAGGED_DIRTY], img[RAGGED_DIRTY], scene(200))
    intr = batch_intrinsics(len(RAGGED_SPECS)).clone()
    intr[RAGGED_BAD, 0] = 0.0
    return pts, img, counts, intr


@functools.lru_cache(maxsize=None)
def ragged_reference():
    pts, img, counts, intr = ragged()
    return reference_of(pts, img, counts, intr)


# ---- the scoring poses --------------------------------------------------------------------------------------------
SCORE_K = 200
SCORE_MARGIN_PX = 1e-2


@functools.lru_cache(maxsize=None)
def score_poses():
    """[4, 12] fp32 on the k = 200 scene: the reference's winning pose rounded to fp32, and three perturbed ones: the
    camera rolled about its axis by 0.008, 0.02 and 0.04 rad (a row's error grows with its distance from the image
    centre, so the inliers leave one by one; the three angles are those of a scan that leave every row more than
    SCORE_MARGIN_PX from the threshold)."""
    ref = reference(SCORE_K)
    r, t = ref.R[0].numpy(), ref.t[0].numpy()
    out = [np.concatenate([r.reshape(9), t])]
    for a in (0.008, 0.02, 0.04):
        turn = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
        out.append(np.concatenate([(turn @ r).reshape(9), turn @ t]))
    return torch.from_numpy(np.stack(out).astype(np.float32))


def score_errors(pose):
    """The reprojection error in pixels of each row of the k = 200 scene under a pose [12] (as the kernel gets it)."""
    p = pose.double()
    return errors_px(p[:9].reshape(3, 3), p[9:], scene(SCORE_K))


# ---- the link cases -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def link_hand_made():
    """(matches_a [6, 12, 2], counts_a, points_a [6, 12, 3], ok_a [6, 12], matches_b [6, 10, 2], counts_b, kpts_b1
    [6, 5, 2], num_shared = 7), hand-made: pair 0 duplicates (several rows of A name one shared keypoint: the lowest
    owns it); pair 1 the same with ok == 0 on the lowest; pair 2 indices out of range on both sides of both pairs (clamped);
    pair 3 count_a = 0; pair 4 count_b = 0; pair 5 every row of B linked and counts past kmax (stability, clamping).
    Column 1 of matches_a is the shared side; column 0 holds other values, so that side_a = 0 links differently."""
    ka, kb, k1, shared = 12, 10, 5, 7
    ma = torch.zeros((6, ka, 2), dtype=torch.int32)
    ma[..., 0] = (torch.arange(ka, dtype=torch.int32) * 5 % shared)[None]
    ma[..., 1] = torch.tensor([3, 3, 5, 1, 3, 6, 5, 0, 1, 2, 2, 4], dtype=torch.int32)[None]
    ca = torch.tensor([12, 12, 12, 0, 9, 40], dtype=torch.int32)
    pa = (torch.arange(6 * ka * 3, dtype=torch.float32).reshape(6, ka, 3) * 0.25 + 1.0)
    ok = torch.ones((6, ka), dtype=torch.uint8)
    ok[1, 0], ok[1, 2], ok[1, 7] = 0, 0, 0
    ok[0, 5], ok[2, 3] = 0, 0
    mb = torch.zeros((6, kb, 2), dtype=torch.int32)
    mb[..., 0] = torch.tensor([6, 3, 0, 5, 3, 1, 4, 2, 6, 5], dtype=torch.int32)[None]
    mb[..., 1] = torch.tensor([0, 1, 2, 3, 4, 4, 3, 2, 1, 0], dtype=torch.int32)[None]
    ma[2, 1] = torch.tensor([-4, 99]).int()
    ma[2, 6] = torch.tensor([50, -1]).int()
    mb[2, 0] = torch.tensor([-3, 77]).int()
    mb[2, 4] = torch.tensor([1000, -9]).int()
    cb = torch.tensor([10, 10, 10, 10, 0, 55], dtype=torch.int32)
    kb1 = torch.arange(6 * k1 * 2, dtype=torch.float32).reshape(6, k1, 2) * 1.5 + 0.5
    return ma, ca, pa, ok, mb, cb, kb1, shared


@functools.lru_cache(maxsize=None)
def three_views():
    from lightglue_amd import three_view_scene

    return three_view_scene(CHAIN_SEED, CHAIN_K, OUTLIERS, NOISE)


@functools.lru_cache(maxsize=None)
def link_wide():
    """The k = 200 three-view scene's two pairs with a point per row of A and every third row of A ok == 0."""
    tv = three_views()
    k = CHAIN_K
    pa = torch.from_numpy(np.random.default_rng(5).standard_normal((1, k, 3)).astype(np.float32))
    ok = torch.ones((1, k), dtype=torch.uint8)
    ok[0, ::3] = 0
    cnt = torch.tensor([k], dtype=torch.int32)
    return tv.matches_a[None].contiguous(), cnt, pa, ok, tv.matches_b[None].contiguous(), cnt.clone(), tv.kpts2[None].contiguous(), k


# ---- the three-view chain -----------------------------------------------------------------------------------------
def chain_intrinsics():
    """(pair intrinsics [1, 2, 4], camera intrinsics [1, 4]) of the three-view scene."""
    one = intrinsics_of(three_views().K)
    return one[None, None].repeat(1, 2, 1).contiguous(), one[None].contiguous()


@functools.lru_cache(maxsize=None)
def chain_reference():
    """The chain in float64, the references chained: essential_reference -> polish_reference -> triangulate_reference ->
    link_landmarks_reference -> absolute_pose_reference -> the mask on pair B's rows. Returns (pose A, landmarks, pose 2,
    mask on B's rows [k] bool)."""
    from lightglue_amd import (absolute_pose_reference, essential_reference, link_landmarks_reference, polish_reference,
                               triangulate_reference)
    from lightglue_amd.geometry import gather_correspondences

    tv, k = three_views(), CHAIN_K
    pair_intr, cam_intr = chain_intrinsics()
    ma, mb, cnt = tv.matches_a[None], tv.matches_b[None], torch.tensor([k], dtype=torch.int32)
    kp0, kp1, kp2 = tv.kpts0[None], tv.kpts1[None], tv.kpts2[None]
    pose = essential_reference(ma, cnt, kp0, kp1, pair_intr, THRESHOLD, HYPOTHESES, REFITS, SEED)
    fine = polish_reference(pose, ma, cnt, kp0, kp1, pair_intr, THRESHOLD)
    x0, x1 = gather_correspondences(ma[0], k, kp0[0], kp1[0])
    pts, ok = triangulate_reference(fine.R[0], fine.t[0], x0, x1, pair_intr[0], fine.inliers[0, :k])
    marks = link_landmarks_reference(ma, cnt, pts[None], ok[None], mb, cnt, kp2, 1, k)
    got = absolute_pose_reference(marks.points, marks.image, marks.counts, cam_intr, THRESHOLD, HYPOTHESES, REFITS, SEED)
    on_b = torch.zeros(k, dtype=torch.bool)
    n = int(marks.counts[0])
    on_b[marks.rows[0, :n].long()] = got.inliers[0, :n].bool()
    return fine, marks, got, on_b
