"""The absolute pose's float64 contract (lightglue_amd/geometry_contract.py) and scenes, on the CPU: the 3-samples, each
scene's precondition (the reference returns exactly the ground-truth mask, every inlier below 1.5 px and every outlier
above 6 px at threshold 3), the P3P reference on its own sample points and on noise-free samples, the planar scenes,
the scoring poses' margin, link_landmarks_reference on hand-made cases, the three-view chain in float64 (the yardstick of
the GPU chain test) and the argument checks of the classes. No GPU, no library.

The float64 chain on the three-view scene (seed 1, k = 200): pair B's mask is the ground truth, view 2's pose is
2.313e-2 deg and 9.898e-4 (|t - t_true| at the scale |t1| = 1) from the truth: CHAIN_ERROR below, which
tests/test_gpu_absolute.py takes its chain bound from.
"""
import numpy as np
import pytest
import torch

import absolute_scenes as ab

CHAIN_ERROR = (2.313e-2, 9.898e-4)  # the float64 chain's own error on the scene: (deg, |t - t_true|)


def test_samples3_are_the_first_three_columns_of_the_7_samples():
    from lightglue_amd import ransac_samples, ransac_samples3

    for count in (7, 8, 37, 2048):
        assert torch.equal(ransac_samples3(ab.SEED, 300, count), ransac_samples(ab.SEED, 300, count)[:, :3]), count
    for count in (3, 4, 5):
        s = ransac_samples3(ab.SEED, 300, count)
        assert s.shape == (300, 3) and int(s.min()) >= 0 and int(s.max()) < count
        assert all(len(set(row)) == 3 for row in s.tolist())
    with pytest.raises(ValueError):
        ransac_samples3(ab.SEED, 4, 2)
    with pytest.raises(ValueError):
        ransac_samples3(ab.SEED, 0, 9)


def precondition(s, ref, what):
    gt = s[2]
    err = ab.errors_px(ref.R[0], ref.t[0], s)
    rot, tra = ab.pose_errors(ref.R[0], ref.t[0], s[4], s[5])
    print(f"{what}: {int(ref.num_inliers[0])} inliers, best {int(ref.best[0])}, worst inlier {float(err[gt].max()):.3f} px, nearest "
          f"outlier {float(err[~gt].min()):.2f} px, the pose {rot:.3e} deg and {tra:.3e} from the truth")
    assert int(ref.valid[0]) == 1 and torch.equal(ref.inliers[0].bool(), gt) and int(ref.num_inliers[0]) == int(gt.sum()), what
    assert float(err[gt].max()) < 1.5 and float(err[~gt].min()) > 6.0, what
    assert abs(float(torch.linalg.det(ref.R[0])) - 1.0) < 1e-9, what
    return rot, tra


@pytest.mark.parametrize("k,alt", [(24, False), (64, False), (200, False), (24, True), (64, True), (200, True)])
def test_scene_precondition(k, alt):
    precondition(ab.scene(k, alt), ab.reference(k, alt), f"k {k}{' (alternate)' if alt else ''}")


def test_scene_precondition_at_full_width_and_at_the_full_grid():
    precondition(ab.scene(2048), ab.reference(2048, False, ab.WIDE_HYPOTHESES), "k 2048, 512 hypotheses")
    precondition(ab.scene(64), ab.reference(64, False, ab.FULL_HYPOTHESES), "k 64, 4096 hypotheses")


def test_planar_scenes_localise_as_well_as_the_others():
    """P3P has no planar degeneracy: the planar scenes meet the same precondition and their pose is of the non-planar
    scenes' order of magnitude from the truth (within ten times the worst of them)."""
    worst = [0.0, 0.0]
    for k in (24, 64):
        rot, tra = precondition(ab.scene(k), ab.reference(k), f"k {k}")
        worst = [max(worst[0], rot), max(worst[1], tra)]
    for k, seed in ab.PLANAR_SEEDS:
        s = ab.scene(k, planar_seed=seed)
        x = s[0][s[2]].double().numpy()
        sv = np.linalg.svd(x - x.mean(0), compute_uv=False)
        assert sv[2] < 1e-5 * sv[0], "the planar scene's inlier points lie on a plane"
        rot, tra = precondition(s, ab.reference(k, planar_seed=seed), f"planar, k {k} seed {seed}")
        print(f"planar k {k}: {rot:.3e} deg, {tra:.3e}; the non-planar scenes' worst {worst[0]:.3e} deg, {worst[1]:.3e}")
        assert rot < 10.0 * worst[0] and tra < 10.0 * worst[1]


def test_solve3_candidates_reproject_their_sample_points():
    from lightglue_amd import reprojection_error

    samples, cases = ab.solve_cases()
    intr = ab.intrinsics()
    worst, total, kept = 0.0, 0, 0
    for (pts, kp), rows in zip(ab.solve_pairs(), cases):
        for s, ref, ok in rows:
            kept += ok
            assert len(ref.R) <= 4 and ref.area > 0
            keys = [float(np.linalg.norm(r @ pts[s[0]].double().numpy() + t)) for r, t in zip(ref.R, ref.t)]
            assert keys == sorted(keys)
            for r, t in zip(ref.R, ref.t):
                total += 1
                assert abs(np.linalg.det(r) - 1.0) < 1e-9
                worst = max(worst, float(reprojection_error(r, t, pts[s], kp[s], intr).sqrt().max()))
    print(f"solve3_reference: {total} candidates on {2 * ab.SOLVE_H} hypotheses, {kept} kept; worst sample-point error {worst:.3e} px")
    assert worst < 1e-9 and total >= 2 * ab.SOLVE_H and kept >= 2 * ab.SOLVE_H * 3 // 4


def test_solve3_finds_the_true_pose_on_noise_free_samples():
    from lightglue_amd import absolute_scene, ransac_samples3, solve3_reference

    pts, kp, gt, kk, r, t = absolute_scene(3, 40, 0.0, 0.0)
    intr = ab.intrinsics_of(kk)
    worst = 0.0
    for s in ransac_samples3(ab.SEED, 32, 40).numpy():
        ref = solve3_reference(pts, kp, intr, s)
        assert len(ref.R) >= 1
        # the scene's points and pixels are rounded to fp32: 6e-8 relative on pixels of up to 640 and depths of up to 12
        near = min(max(*ab.pose_errors(rc, tc, r, t)) for rc, tc in zip(ref.R, ref.t))
        worst = max(worst, near)
    print(f"noise-free samples: the nearest candidate to the true pose, worst of 32: {worst:.3e} (deg, map units)")
    assert worst < 1e-2


def test_solve3_refuses_degenerate_samples():
    from lightglue_amd import solve3_reference

    pts, kp = (t.clone() for t in ab.scene(24)[:2])
    intr = ab.intrinsics()
    assert len(solve3_reference(pts, kp, intr, [3, 3, 5]).R) == 0          # a repeated point
    pts[2] = 0.5 * (pts[0] + pts[1])
    assert len(solve3_reference(pts, kp, intr, [0, 1, 2]).R) == 0          # three collinear points
    pts[4, 1] = float("nan")
    assert len(solve3_reference(pts, kp, intr, [4, 5, 6]).R) == 0
    kp[7, 0] = float("inf")
    assert len(solve3_reference(pts, kp, intr, [7, 8, 9]).R) == 0


def test_reprojection_error_and_the_refit():
    from lightglue_amd import absolute_refit_reference, reprojection_error

    s = ab.scene(64)
    pts, kp, gt, kk, r, t = s
    intr = ab.intrinsics_of(kk)
    err = reprojection_error(r, t, pts, kp, intr)
    assert float(err[gt].sqrt().max()) <= ab.NOISE + 1e-3 and float(err[~gt].sqrt().min()) > 12.0 - 1e-3
    behind = reprojection_error(r, -t - 20.0, pts, kp, intr)
    assert bool(torch.isinf(behind).all())
    turn = np.array([[np.cos(0.01), -np.sin(0.01), 0.0], [np.sin(0.01), np.cos(0.01), 0.0], [0.0, 0.0, 1.0]])
    r1, t1 = absolute_refit_reference(turn @ r.numpy(), t.numpy() + 0.02, pts[gt], kp[gt], intr)
    rot, tra = ab.pose_errors(r1, t1, r, t)
    cost = lambda a, b: float(reprojection_error(a, b, pts[gt], kp[gt], intr).sum())  # noqa: E731
    print(f"the refit from a pose 0.57 deg and 0.035 off: {rot:.3e} deg, {tra:.3e} from the truth, cost {cost(r1, t1):.4f} px² "
          f"(the truth's {cost(r, t):.4f})")
    assert cost(r1, t1) <= cost(r, t) and rot < 0.05 and tra < 0.01
    assert absolute_refit_reference(r, t, pts[:2], kp[:2], intr) is None


def test_invalid_pairs_of_the_reference():
    pts, img, counts, intr = ab.ragged()
    want = ab.ragged_reference()
    assert want.valid.tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0] and want.best.tolist()[0] == -1 and want.best.tolist()[-1] == -1
    for p in (0, 1, 8):
        assert not bool(want.R[p].any()) and not bool(want.t[p].any()) and not bool(want.inliers[p].any())
    gt = ab.scene(200)[2]
    assert torch.equal(want.inliers[ab.RAGGED_DIRTY, :200].bool(), gt), "the planted rows are outliers' and stay out"
    assert torch.equal(want.inliers[6], want.inliers[7])
    rows = ab.plant_dirty(pts[7].clone(), img[7].clone(), ab.scene(200))
    assert not bool(want.inliers[7, rows].any())


def test_scoring_poses_keep_every_row_off_the_threshold():
    poses = ab.score_poses()
    counts = []
    for i, pose in enumerate(poses):
        err = ab.score_errors(pose)
        gap = float((err - ab.THRESHOLD).abs().min())
        counts.append(int((err <= ab.THRESHOLD).sum()))
        print(f"scoring pose {i}: {counts[-1]} inliers, the nearest row {gap:.3e} px from the threshold")
        assert gap > (1.0 if i == 0 else ab.SCORE_MARGIN_PX)
    assert counts[0] == 150 and len(set(counts)) == 4 and counts[3] < counts[0]


def test_link_landmarks_reference_on_hand_made_cases():
    from lightglue_amd import link_landmarks_reference

    ma, ca, pa, ok, mb, cb, kb1, shared = ab.link_hand_made()
    got = link_landmarks_reference(ma, ca, pa, ok, mb, cb, kb1, 1, shared)
    # pair 0: shared keypoints (column 1 of A) 3, 3, 5, 1, 3, 6*, 5, 0, 1, 2, 2, 4 (* ok == 0): owners 3 -> row 0, 5 -> 2,
    # 1 -> 3, 0 -> 7, 2 -> 9, 4 -> 11, 6 -> none; B's shared keypoints 6, 3, 0, 5, 3, 1, 4, 2, 6, 5
    assert got.counts.tolist() == [8, 9, 10, 0, 0, 10]
    assert got.rows[0].tolist() == [1, 2, 3, 4, 5, 6, 7, 9, -1, -1]
    owners0 = [0, 7, 2, 0, 3, 11, 9, 2]
    assert torch.equal(got.points[0, :8], pa[0, owners0]) and not bool(got.points[0, 8:].any())
    assert torch.equal(got.image[0, :8], kb1[0, [1, 2, 3, 4, 4, 3, 2, 0]]) and not bool(got.image[0, 8:].any())
    # pair 1: rows 0, 2 and 7 of A are not ok (and row 5 is): 3 -> row 1, 5 -> row 6, 0 -> none, 6 -> row 5: nine rows
    owners1 = {6: 5, 3: 1, 5: 6, 1: 3, 4: 11, 2: 9}
    rows1 = [k for k in range(10) if int(mb[1, k, 0]) in owners1]
    assert got.rows[1, :len(rows1)].tolist() == rows1 and int(got.counts[1]) == len(rows1)
    assert torch.equal(got.points[1, :len(rows1)], pa[1, [owners1[int(mb[1, k, 0])] for k in rows1]])
    # pair 2: indices out of range are clamped: A's row 1 names 99 -> 6 and row 6 names -1 -> 0; B's row 0 names -3 -> 0
    # with the new image's 77 -> 4, row 4 names 1000 -> 6 with -9 -> 0
    assert int(got.counts[2]) == 10 and got.rows[2].tolist() == list(range(10))
    assert torch.equal(got.points[2, 0], pa[2, 6]) and torch.equal(got.image[2, 0], kb1[2, 4])
    assert torch.equal(got.points[2, 4], pa[2, 1]) and torch.equal(got.image[2, 4], kb1[2, 0])
    # pairs 3 and 4: an empty side links nothing; pair 5: counts past kmax are clamped
    assert got.rows[3].tolist() == [-1] * 10 and got.rows[4].tolist() == [-1] * 10
    assert got.rows[5].tolist() == list(range(10))
    # the other side of A links differently
    other = link_landmarks_reference(ma, ca, pa, ok, mb, cb, kb1, 0, shared)
    assert not torch.equal(other.rows, got.rows)
    wide = ab.link_wide()
    marks = link_landmarks_reference(*wide[:7], 1, wide[7])
    n = int(marks.counts[0])
    rows = marks.rows[0, :n]
    assert 100 < n < 200 and bool((rows[1:] > rows[:-1]).all()) and int(marks.rows[0, n:].max()) == -1


def test_three_view_chain_in_float64():
    """The references chained: pair A's mask and pair B's mask are the ground truth; view 2's pose against the truth
    is printed and is CHAIN_ERROR (the GPU chain's yardstick)."""
    tv = ab.three_views()
    fine, marks, got, on_b = ab.chain_reference()
    assert torch.equal(fine.inliers[0, :ab.CHAIN_K].bool(), tv.gt_a) and int(marks.counts[0]) == int(tv.gt_a.sum())
    assert int(got.valid[0]) == 1 and torch.equal(on_b, tv.gt_b)
    rot, tra = ab.pose_errors(got.R[0], got.t[0], tv.R2, tv.t2)
    rot1, tra1 = ab.pose_errors(fine.R[0], fine.t[0], tv.R1, tv.t1)
    print(f"the float64 chain: view 1 {rot1:.3e} deg, {tra1:.3e}; view 2 in view 0's frame {rot:.3e} deg, |t - t_true| {tra:.3e} "
          f"({int(got.num_inliers[0])} inliers of {int(marks.counts[0])} landmarks)")
    assert abs(rot - CHAIN_ERROR[0]) < 1e-3 * CHAIN_ERROR[0] + 1e-6 and abs(tra - CHAIN_ERROR[1]) < 1e-3 * CHAIN_ERROR[1] + 1e-7
    assert abs(float(np.linalg.norm(tv.t1)) - 1.0) < 1e-12


def test_class_and_argument_validation():
    from lightglue_amd import AbsolutePoseRansac, AbsolutePoseResult, Landmarks, inliers_on_matches, link_landmarks
    from lightglue_amd.matches import MatchResult

    for bad in (dict(threshold=0.0), dict(threshold=float("nan")), dict(hypotheses=0), dict(hypotheses=4097), dict(refits=-1),
                dict(refits=9)):
        with pytest.raises(ValueError):
            AbsolutePoseRansac(**bad)
    er = AbsolutePoseRansac()
    assert (er.threshold, er.hypotheses, er.refits, er.seed) == (3.0, 512, 2, 888)
    assert AbsolutePoseResult._fields == ("R", "t", "inliers", "num_inliers", "valid", "best")
    assert Landmarks._fields == ("points", "image", "rows", "counts")
    pts, img, counts = ab.batch(((24, 24),), 24)
    with pytest.raises((ValueError, TypeError, RuntimeError)):
        er.localize(pts, img, counts, ab.batch_intrinsics(1))  # (not on the device)
    with pytest.raises(TypeError):
        er.verify(None, None, None)
    ma, ca, pa, ok, mb, cb, kb1, shared = ab.link_hand_made()
    a, b = MatchResult(None, None, None, None, ma, None, ca), MatchResult(None, None, None, None, mb, None, cb)
    with pytest.raises((ValueError, TypeError, RuntimeError)):
        link_landmarks(a, pa, ok, b, kb1, num_shared=shared)  # (not on the device)
    marks = Landmarks(torch.zeros(1, 4, 3), torch.zeros(1, 4, 2), torch.tensor([[0, 2, 5, -1]], dtype=torch.int32), torch.tensor([3]))
    res = AbsolutePoseResult(None, None, torch.tensor([[1, 0, 1, 1]], dtype=torch.uint8), None, None, None)
    assert inliers_on_matches(marks, res, 7).tolist() == [[1, 0, 0, 0, 0, 1, 0]]
    with pytest.raises(ValueError):
        inliers_on_matches(marks, res, 3)
