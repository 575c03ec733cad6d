"""The calibrated five-point RANSAC, no GPU: the exports and their bindings, every argument check of the new
lg_ransac_essential / lg_ransac_samples5 / lg_ransac_solve5 / lg_pose_from_essential entry points (nothing reaches
the device), ransac_samples5, the float64 reference solver, refit and pose, the calibrated scenes, the preconditions
of the scenes the GPU tests use, the planar scenes and the keep rule, and EssentialRansac's own validation."""
import numpy as np
import pytest
import torch

import essential_scenes as es

A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below
NAMES = ("lg_ransac_essential_workspace", "lg_ransac_essential", "lg_ransac_samples5", "lg_ransac_solve5",
         "lg_pose_from_essential")
# The reference's own errors against the scenes' true pose after two refits, degrees (rotation, translation
# direction): k = 24: (0.101, 1.041), alternate (0.084, 0.266); 64: (0.025, 0.020), (0.056, 0.067); 200: (0.048, 0.044),
# (0.016, 0.086); 2048: (0.012, 0.004). The bounds are one and a half times the worst of each.
ROTATION_BOUND_DEG, TRANSLATION_BOUND_DEG = 0.15, 1.6
# The reference's candidates on the 128 solve cases: |det E| <= 4.9e-14, the cubic constraints' entries <= 1.3e-12, the
# sample equations <= 4.3e-16 (unit-norm E, camera coordinates of order 0.5). The bounds leave two orders of magnitude
# for another LAPACK; they are float64 rounding times the condition of the eigenproblem, nothing a wrong solver meets.
DET_BOUND, CUBIC_BOUND, SAMPLE_BOUND = 1e-11, 1e-10, 1e-13


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


# ---- exports, bindings, argument checks -----------------------------------------------------------------------
def test_exports_and_bindings(lib):
    import lightglue_amd
    from lightglue_amd import _lib

    assert lib.lg_glue_abi_version() == _lib.GLUE_ABI_VERSION == 4
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
    for name in ("EssentialRansac", "PoseResult", "essential_reference", "essential_refit", "solve5_reference",
                 "pose_from_essential_reference", "ransac_samples5", "calibrated_scene", "calibrated_planar_scene",
                 "camera_coordinates", "essential_to_fundamental", "verify_source_images"):
        assert name in lightglue_amd.__all__ and hasattr(lightglue_amd, name), name
    assert lightglue_amd.PoseResult._fields == ("E", "R", "t", "inliers", "num_inliers", "num_front", "valid", "best")


def _rejects(call, bads):
    for bad in bads:
        assert call(**bad) == 1, bad


PAIR_BADS = [dict(pairs=-1), dict(pairs=65536), dict(kmax=0), dict(kmax=2049), dict(kmax=-1), dict(k0=0), dict(k1=0),
             dict(pairs=65535, kmax=1 << 13), dict(pairs=65535, k0=1 << 13), dict(pairs=65535, k1=1 << 13), dict(matches=None),
             dict(counts=None), dict(kp0=None), dict(kp1=None), dict(matches=A + 4), dict(counts=A + 2), dict(kp0=A + 4),
             dict(kp1=A + 4), dict(intr=None), dict(intr=A + 2)]


def test_entry_points_validate_before_touching_the_device(lib):
    """An empty call returns success and every clause of every argument check rejects with the entry's name in the
    message, on fake addresses and without a device call."""
    from lightglue_amd import _lib

    def essential(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, intr=A, pairs=0, kmax=64, k0=64, k1=64, thr=3.0, hyp=512, refits=2,
                 seed=888, ws=A, ws_bytes=1 << 20, e=A, r=A, t=A, inl=A, num=A, front=A, valid=A, best=A)
        a.update(kw)
        return lib.lg_ransac_essential(a["matches"], a["counts"], a["kp0"], a["kp1"], a["intr"], a["pairs"], a["kmax"], a["k0"],
                                       a["k1"], a["thr"], a["hyp"], a["refits"], a["seed"], a["ws"], a["ws_bytes"], a["e"],
                                       a["r"], a["t"], a["inl"], a["num"], a["front"], a["valid"], a["best"], None)

    assert essential() == 0
    assert essential(kmax=2048, k0=1, k1=1, thr=1e-3, hyp=4096, refits=0, seed=-1, inl=A + 1, counts=A + 4, e=A + 4, intr=A + 4) == 0
    assert essential(kmax=1, hyp=1, refits=8, ws_bytes=0) == 0  # (an empty call needs no workspace)
    out_bads = [{name: bad} for name in ("e", "r", "t", "num", "front", "valid", "best") for bad in (None, A + 2)]
    _rejects(essential, PAIR_BADS + out_bads + [
        dict(thr=0.0), dict(thr=-3.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=2e6), dict(hyp=0),
        dict(hyp=4097), dict(hyp=-1), dict(refits=-1), dict(refits=9), dict(ws=None), dict(ws=A + 8),
        dict(pairs=2, ws_bytes=lib.lg_ransac_essential_workspace(2, 64, 512) - 1), dict(inl=None)])
    assert "lg_ransac_essential" in _lib.last_error()
    assert lib.lg_ransac_essential_workspace(2, 64, 512) == 2 * 512 * 80 > lib.lg_ransac_workspace(2, 64, 512)
    assert lib.lg_ransac_essential_workspace(0, 64, 512) == lib.lg_ransac_essential_workspace(2, 0, 512) == 0

    def samples5(**kw):
        a = dict(count=8, hyp=64, seed=888, out=None)
        a.update(kw)
        return lib.lg_ransac_samples5(a["count"], a["hyp"], a["seed"], a["out"], None)

    _rejects(samples5, [dict(), dict(out=A + 2), dict(out=A, count=4), dict(out=A, count=2049), dict(out=A, hyp=0),
                        dict(out=A, hyp=4097)])
    assert "lg_ransac_samples5" in _lib.last_error()

    def solve5(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, intr=A, pairs=0, kmax=64, k0=64, k1=64, smp=A, hyp=64, cand=A, num=A)
        a.update(kw)
        return lib.lg_ransac_solve5(a["matches"], a["counts"], a["kp0"], a["kp1"], a["intr"], a["pairs"], a["kmax"], a["k0"],
                                    a["k1"], a["smp"], a["hyp"], a["cand"], a["num"], None)

    assert solve5() == 0 and solve5(hyp=4096, smp=A + 4, cand=A + 4, num=A + 4) == 0
    _rejects(solve5, PAIR_BADS + [dict(hyp=0), dict(hyp=4097), dict(smp=None), dict(cand=None), dict(num=None),
                                  dict(smp=A + 2), dict(cand=A + 2), dict(num=A + 2)])
    assert "lg_ransac_solve5" in _lib.last_error()

    def pose(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, intr=A, pairs=0, kmax=64, k0=64, k1=64, e=A, inl=A, r=A, t=A, front=A)
        a.update(kw)
        return lib.lg_pose_from_essential(a["matches"], a["counts"], a["kp0"], a["kp1"], a["intr"], a["pairs"], a["kmax"],
                                          a["k0"], a["k1"], a["e"], a["inl"], a["r"], a["t"], a["front"], None)

    assert pose() == 0 and pose(e=A + 4, inl=A + 1, r=A + 4, t=A + 4, front=A + 4) == 0
    _rejects(pose, PAIR_BADS + [dict(inl=None)] + [{name: bad} for name in ("e", "r", "t", "front") for bad in (None, A + 2)])
    assert "lg_pose_from_essential" in _lib.last_error()


# ---- the samples ------------------------------------------------------------------------------------------------
def test_samples5_are_the_first_five_of_the_seven():
    from lightglue_amd import ransac_samples, ransac_samples5

    for count in (7, 8, 37, 2048):
        assert torch.equal(ransac_samples5(es.SEED, 300, count), ransac_samples(es.SEED, 300, count)[:, :5]), count
    for count in (5, 6):
        s = ransac_samples5(es.SEED, 300, count)
        assert s.shape == (300, 5) and s.dtype == torch.int32 and int(s.min()) >= 0 and int(s.max()) < count
        assert all(len(set(row)) == 5 for row in s.tolist()), count
        assert torch.equal(s, ransac_samples5(es.SEED, 300, count)) and not torch.equal(s, ransac_samples5(es.SEED + 1, 300, count))
    with pytest.raises(ValueError):
        ransac_samples(es.SEED, 8, 64, size=5)
    for bad in ((8, 4), (0, 8)):
        with pytest.raises(ValueError):
            ransac_samples5(es.SEED, *bad)


# ---- the float64 pieces -----------------------------------------------------------------------------------------
def test_reference_candidates_satisfy_the_constraints_and_their_samples():
    from lightglue_amd import camera_coordinates
    from lightglue_amd.geometry import essential_residuals
    from lightglue_amd.geometry_contract import _rows

    _, cases = es.solve_cases()
    intr = es.intrinsics()
    worst, total = [0.0, 0.0, 0.0], 0
    for p, (x0, x1) in enumerate(es.solve_pairs()):
        q0, q1 = camera_coordinates(x0, intr[0]), camera_coordinates(x1, intr[1])
        for s, ref, _ in cases[p]:
            assert len(ref.candidates) <= 10, (p, s)
            assert all(a[0, 0] <= b[0, 0] for a, b in zip(ref.candidates, ref.candidates[1:]))
            for e in ref.candidates:
                total += 1
                assert abs(float((e * e).sum()) - 1.0) < 1e-12 and e.flat[int(np.abs(e).argmax())] > 0
                det, cubic = essential_residuals(e)
                worst = [max(worst[0], det), max(worst[1], cubic), max(worst[2], float(np.abs(_rows(q0[s], q1[s]) @ e.reshape(9)).max()))]
    print(f"{total} candidates: |det E| <= {worst[0]:.2e}, cubic entries <= {worst[1]:.2e}, sample equations <= {worst[2]:.2e}")
    assert total > 400 and worst[0] < DET_BOUND and worst[1] < CUBIC_BOUND and worst[2] < SAMPLE_BOUND


true_essential = es.true_essential


def test_reference_solver_recovers_the_true_essential_matrix_and_pose():
    """A noise-free all-inlier scene: among the candidates of a sample is the true E = [t]x R up to sign (to the fp32
    rounding of the keypoints, 3e-5 px of 640), and the pose of the true E, of either sign, is the true pose with
    every point in front and fewer in front under each of the other three decompositions."""
    from lightglue_amd import calibrated_scene, camera_coordinates, pose_from_essential_reference, ransac_samples5, solve5_reference

    k0, k1, gt, _, kk, r, t = calibrated_scene(7, 40, 0.0, 0.0)
    assert bool(gt.all())
    intr = es.intrinsics_of(kk)
    q0, q1 = camera_coordinates(k0, intr[0]), camera_coordinates(k1, intr[1])
    e_true = true_essential(r, t)
    for s in ransac_samples5(es.SEED, 8, 40).numpy():
        c = solve5_reference(q0, q1, s).candidates
        assert len(c) >= 1 and min(min(np.abs(e - e_true).max(), np.abs(e + e_true).max()) for e in c) < 1e-5, s
    for sign in (1.0, -1.0):
        rr, tt, front, counts = pose_from_essential_reference(sign * e_true, q0, q1)
        assert front == 40 and sorted(counts)[2] < 40, counts
        rot, tra = es.pose_errors_deg(rr, tt, r, t)
        assert rot < 1e-6 and tra < 1e-6 and abs(float(torch.linalg.det(rr)) - 1.0) < 1e-12 and abs(float(tt.norm()) - 1.0) < 1e-12


def test_essential_refit_is_on_the_manifold_and_fits():
    from lightglue_amd import camera_coordinates, epipolar_error, essential_refit, essential_to_fundamental
    from lightglue_amd.geometry import essential_residuals

    k0, k1, gt = es.scene(64)[:3]
    intr = es.intrinsics()
    e = essential_refit(camera_coordinates(k0[gt], intr[0]), camera_coordinates(k1[gt], intr[1]))
    det, cubic = essential_residuals(e)
    sv = np.linalg.svd(e.numpy())[1]
    assert det < 1e-14 and cubic < 1e-14 and abs(sv[0] - sv[1]) < 1e-14 and sv[2] < 1e-14 and abs(float((e * e).sum()) - 1) < 1e-12
    err = epipolar_error(essential_to_fundamental(e, intr), k0, k1).sqrt()
    assert float(err[gt].max()) < 1.5 and float(err[~gt].min()) > 6.0
    with pytest.raises(ValueError):
        essential_refit(torch.zeros(7, 2), torch.zeros(7, 2))


# ---- the scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (24, 200))
def test_calibrated_scenes_are_the_uncalibrated_ones_with_their_cameras(k):
    from lightglue_amd import calibrated_planar_scene, calibrated_scene, planar_scene, two_view_scene

    for seed in (1, 5):
        a, b = calibrated_scene(seed, k, es.OUTLIERS, es.NOISE), two_view_scene(seed, k, es.OUTLIERS, es.NOISE)
        assert len(a) == 7 and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))
        kk, r, t = a[4:]
        assert kk.tolist() == [[640.0, 0.0, 320.0], [0.0, 640.0, 240.0], [0.0, 0.0, 1.0]]
        assert abs(float(torch.linalg.det(r)) - 1.0) < 1e-12 and abs(float(t.norm()) - 1.0) < 1e-12
        kinv = np.linalg.inv(kk.numpy())
        f = kinv.T @ true_essential(r, t) @ kinv
        f = f / np.linalg.norm(f)
        assert min(np.abs(f - a[3].numpy()).max(), np.abs(f + a[3].numpy()).max()) < 1e-12
        c, d = calibrated_planar_scene(seed, k, es.OUTLIERS, es.NOISE), planar_scene(seed, k, es.OUTLIERS, es.NOISE)
        assert len(c) == 7 and all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(c, d))
        # the plane's homography is of the returned pose: H ~ K (R + t nᵀ / d) K⁻¹, so K⁻¹ H K - s R has rank 1 for one s
        g = kinv @ c[3].numpy() @ kk.numpy()
        g = g / np.linalg.svd(g)[1][1]  # the middle singular value of R + t nᵀ / d is 1
        assert min(np.linalg.svd(g - c[5].numpy())[1][1], np.linalg.svd(g + c[5].numpy())[1][1]) < 1e-9


@pytest.mark.parametrize("k,alt", [(24, False), (64, False), (200, False), (2048, False), (24, True), (64, True), (200, True)])
def test_gpu_scene_preconditions(k, alt):
    """What tests/test_gpu_essential.py rests on: the float64 reference returns exactly gt_mask, every inlier below
    1.5 px and every outlier above 6 px under its E, and its pose is the scene's within the bounds above."""
    ref = es.reference(k, alt)
    k0, k1, gt, _, _, r, t = es.scene(k, alt)
    assert int(ref.valid[0]) == 1 and 0 <= int(ref.best[0]) < es.HYPOTHESES
    assert torch.equal(ref.inliers[0, :k].bool(), gt) and int(ref.num_inliers[0]) == int(gt.sum()) == int(ref.num_front[0])
    e = es.errors_px(ref.E[0], k, alt)
    rot, tra = es.pose_errors_deg(ref.R[0], ref.t[0], r, t)
    print(f"k {k} alt {alt}: inliers <= {float(e[gt].max()):.3f} px, outliers >= {float(e[~gt].min()):.2f} px, R {rot:.3f} deg, t {tra:.3f} deg")
    assert float(e[gt].max()) < 1.5 and float(e[~gt].min()) > 6.0
    assert rot < ROTATION_BOUND_DEG and tra < TRANSLATION_BOUND_DEG


def test_gpu_solve5_cases_keep_three_quarters():
    _, cases = es.solve_cases()
    kept = sum(ok for rows in cases for _, _, ok in rows)
    with_candidates = sum(ok and len(ref.candidates) >= 2 for rows in cases for _, ref, ok in rows)
    assert kept >= 2 * es.SOLVE_H * 3 // 4 and with_candidates >= kept // 2, (kept, with_candidates)


def test_ragged_reference():
    m, counts, kp0, kp1, intr = es.ragged()
    ref = es.ragged_reference()
    assert counts.tolist() == [0, 4, 5, 7, 8, 24, 64, 200, 200, 64] and m.shape[1] > 200
    assert int(m.min()) < -1 and int(m.max()) >= 208 and bool(torch.isnan(kp0).any()) and bool(torch.isinf(kp1).any())
    assert ref.valid.tolist()[:2] == [0, 0] and ref.valid.tolist()[5:] == [1, 1, 1, 1, 0] and ref.best.tolist()[:2] == [-1, -1]
    bad = es.RAGGED_BAD
    assert int(ref.best[bad]) == -1 and not bool(ref.E[bad].any()) and not bool(ref.R[bad].any()) and not bool(ref.inliers[bad].any())
    for p, k in ((5, 24), (6, 64), (7, 200)):  # the whole scenes: the same as alone
        one = es.reference(k)
        assert torch.equal(ref.inliers[p, :k], one.inliers[0]) and torch.equal(ref.E[p], one.E[0]) and int(ref.best[p]) == int(one.best[0])
    dirty = es.RAGGED_DIRTY  # the untrusted rows are no inliers, the rest of the scene's are
    gt = es.scene(200)[2].clone()
    assert not bool(ref.inliers[dirty, [5, 6, 10, 11, 12]].any())
    gt[[5, 6, 10, 11, 12]] = False
    assert torch.equal(ref.inliers[dirty, :200].bool(), gt)


# ---- the planar scenes --------------------------------------------------------------------------------------------
def test_planar_scenes_keep_their_five_point_winner():
    """On a plane the 8-point refit is degenerate. The reference's final mask contains every ground-truth inlier and
    counts no fewer than the winner did (the keep rule); the same rounds taken unconditionally lose inliers."""
    from lightglue_amd import (camera_coordinates, epipolar_error, essential_refit, essential_to_fundamental, ransac_samples5,
                               solve5_reference)

    thr2, lost = es.THRESHOLD ** 2, 0
    for k, seed in es.PLANAR_SEEDS:
        m, counts, kp0, kp1, gt, intr = es.planar(k, seed)
        ref = es.planar_reference(k, seed)
        final = ref.inliers[0].bool()
        assert int(ref.valid[0]) == 1 and bool((final | ~gt).all()), (k, seed)
        q0, q1 = camera_coordinates(kp0[0], intr[0, 0]), camera_coordinates(kp1[0], intr[0, 1])

        def mask_of(e):
            return epipolar_error(essential_to_fundamental(e, intr[0]), kp0[0], kp1[0]) <= thr2

        sample = ransac_samples5(es.SEED, es.HYPOTHESES, k)[int(ref.best[0])].numpy()
        winner = max((int(mask_of(e).sum()) for e in solve5_reference(q0, q1, sample).candidates))
        assert int(ref.num_inliers[0]) >= winner >= int(gt.sum()), (k, seed, winner)
        e = next(e for e in solve5_reference(q0, q1, sample).candidates if int(mask_of(e).sum()) == winner)
        mask, counts_free = mask_of(e), [winner]
        for _ in range(es.REFITS):
            if int(mask.sum()) < 8:
                break
            mask = mask_of(essential_refit(q0[mask], q1[mask]))
            counts_free.append(int(mask.sum()))
        print(f"planar k {k} seed {seed}: {int(gt.sum())} true inliers, the winner {winner}, the final mask {int(ref.num_inliers[0])}, "
              f"unconditional rounds {counts_free}")
        lost += counts_free[-1] < winner
    assert lost >= 1


# ---- EssentialRansac ----------------------------------------------------------------------------------------------
def test_reference_rejects_small_pairs_and_bad_intrinsics():
    from lightglue_amd import essential_reference

    m, counts, kp0, kp1 = es.batch(((24, 4), (24, 24), (24, 24), (24, 24)), 24)
    intr = es.batch_intrinsics(4).clone()
    intr[1, 0, 1], intr[2, 1, 2], intr[3, 0, 0] = -1.0, float("nan"), float("inf")
    r = essential_reference(m, counts, kp0, kp1, intr, es.THRESHOLD, 16, es.REFITS, es.SEED)
    assert r.valid.tolist() == [0] * 4 and r.best.tolist() == [-1] * 4 and not bool(r.E.any()) and not bool(r.inliers.any())
    assert not bool(r.R.any()) and not bool(r.t.any()) and r.num_front.tolist() == [0] * 4


def test_essential_ransac_validates():
    from lightglue_amd import EssentialRansac, FundamentalRansac, PluginError, verify_source_images
    from lightglue_amd.matches import MatchResult

    for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(hypotheses=0), dict(hypotheses=4097), dict(refits=-1),
                dict(refits=9)):
        with pytest.raises(ValueError):
            EssentialRansac(**bad)
    er = EssentialRansac()
    assert (er.threshold, er.hypotheses, er.refits, er.seed) == (3.0, 512, 2, 888)
    assert not isinstance(er, FundamentalRansac) and "num_inliers" in EssentialRansac.__doc__
    r = MatchResult.blank(2, 16, 16, "cpu")
    with pytest.raises(PluginError, match="GPU"):
        er.verify(r, torch.zeros(2, 16, 2), torch.zeros(2, 16, 2), torch.ones(2, 2, 4))
    # the intrinsics go with the calibrated estimator, and only with it: refused before anything runs
    with pytest.raises(ValueError, match="intrinsics"):
        verify_source_images(None, None, None, None, er, [], [])
    with pytest.raises(ValueError, match="intrinsics"):
        verify_source_images(None, None, None, None, FundamentalRansac(), [], [], intrinsics=torch.ones(2, 2, 4))
