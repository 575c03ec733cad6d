"""The pose polish and the triangulation, no GPU: the exports and their bindings, every argument check of
lg_pose_polish and lg_triangulate (nothing reaches the device), the float64 contract (sampson_error,
polish_pose_reference, triangulate_reference) on the scenes of polish_scenes.py with the preconditions the GPU tests
rely on, the keep rule, and the statements of csrc/lightglue_polish_math.h run on the CPU (tools/polish_host_check.py)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import polish_scenes as ps

A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below
# Two starts of the reference on one scene end within 3.6e-7 deg of each other (R and t, the six scenes): the
# numeric Jacobian's 1.5e-8 relative error times the residual at the minimum over the curvature. The bound leaves a
# factor of 30 for another MINPACK build; a start that ends in another minimum is off by 0.01 deg and more.
TWO_STARTS_BOUND_DEG = 1e-5


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def test_exports_and_bindings(lib):
    import lightglue_amd
    from lightglue_amd import _lib

    assert lib.lg_glue_abi_version() == _lib.GLUE_ABI_VERSION == 4
    for name in ("lg_pose_polish", "lg_triangulate"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
    for name in ("PosePolish", "PolishResult", "triangulate", "sampson_error", "polish_pose_reference", "polish_reference",
                 "triangulate_reference"):
        assert name in lightglue_amd.__all__ and hasattr(lightglue_amd, name), name
    assert lightglue_amd.PolishResult._fields == ("E", "R", "t", "inliers", "num_inliers", "num_front", "cost", "kept")
    assert lightglue_amd.PoseResult._fields == ("E", "R", "t", "inliers", "num_inliers", "num_front", "valid", "best")
    assert lightglue_amd.EssentialRansac().polish == 0 and lightglue_amd.EssentialRansac(polish=16).polish == 16
    for bad in (-1, 17):
        with pytest.raises(ValueError):
            lightglue_amd.EssentialRansac(polish=bad)
    for kw in (dict(iterations=0), dict(iterations=17), dict(threshold=0.0), dict(threshold=float("nan"))):
        with pytest.raises(ValueError):
            lightglue_amd.PosePolish(**kw)


PAIR_BADS = [dict(pairs=-1), dict(pairs=65536), dict(kmax=0), dict(kmax=2049), dict(kmax=-1), dict(k0=0), dict(k1=0),
             dict(pairs=65535, k0=1 << 13), dict(pairs=65535, k1=1 << 13), dict(matches=None), dict(counts=None), dict(kp0=None),
             dict(kp1=None), dict(matches=A + 4), dict(counts=A + 2), dict(kp0=A + 4), dict(kp1=A + 4), dict(intr=None),
             dict(intr=A + 2), dict(r=None), dict(r=A + 2), dict(t=None), dict(t=A + 2), dict(inl=None)]


def test_entry_points_validate_before_touching_the_device(lib):
    """An empty call returns success and every clause of every argument check rejects with the entry's name in the
    message, on fake addresses and without a device call."""
    from lightglue_amd import _lib

    def polish(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, intr=A, pairs=0, kmax=64, k0=64, k1=64, r=A, t=A, inl=A, valid=A, thr=3.0,
                 it=10, e=A, ro=A, to=A, io=A, num=A, front=A, cost=A, kept=A)
        a.update(kw)
        return lib.lg_pose_polish(a["matches"], a["counts"], a["kp0"], a["kp1"], a["intr"], a["pairs"], a["kmax"], a["k0"], a["k1"],
                                  a["r"], a["t"], a["inl"], a["valid"], a["thr"], a["it"], a["e"], a["ro"], a["to"], a["io"],
                                  a["num"], a["front"], a["cost"], a["kept"], None)

    assert polish() == 0
    assert polish(kmax=2048, k0=1, k1=1, thr=1e-3, it=1, inl=A + 1, io=A + 1, counts=A + 4, e=A + 4, intr=A + 4, r=A + 4) == 0
    assert polish(it=16, thr=1e6) == 0
    out_bads = [{name: bad} for name in ("valid", "e", "ro", "to", "num", "front", "cost", "kept") for bad in (None, A + 2)]
    for bad in PAIR_BADS + out_bads + [dict(io=None), dict(it=0), dict(it=17), dict(it=-1), dict(thr=0.0), dict(thr=-3.0),
                                       dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=2e6)]:
        assert polish(**bad) == 1, bad
    assert "lg_pose_polish" in _lib.last_error()

    def tri(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, intr=A, pairs=0, kmax=64, k0=64, k1=64, r=A, t=A, inl=A, points=A, ok=A)
        a.update(kw)
        return lib.lg_triangulate(a["matches"], a["counts"], a["kp0"], a["kp1"], a["intr"], a["pairs"], a["kmax"], a["k0"], a["k1"],
                                  a["r"], a["t"], a["inl"], a["points"], a["ok"], None)

    assert tri() == 0 and tri(kmax=2048, inl=A + 1, ok=A + 1, points=A + 4) == 0
    for bad in PAIR_BADS + [dict(points=None), dict(points=A + 2), dict(ok=None)]:
        assert tri(**bad) == 1, bad
    assert "lg_triangulate" in _lib.last_error()


# ---- the float64 contract ---------------------------------------------------------------------------------------
def test_sampson_error_is_the_first_order_distance():
    """The noise-free scene is at zero under the true E; the error is signed and does not depend on E's scale; and it
    is the definition written out in pixels: x1ᵀ F x0 over the length of its gradient in the four pixel coordinates,
    which never exceeds the distance a point was moved by."""
    from lightglue_amd import calibrated_scene, sampson_error

    k0, k1, _, _, kk, r, t = calibrated_scene(7, 40, 0.0, 0.0)
    intr = torch.tensor([[kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]]] * 2)
    import essential_scenes as es

    e = torch.from_numpy(es.true_essential(r, t))
    zero = sampson_error(e, k0, k1, intr)
    assert float(zero.abs().max()) < 1e-3  # (the keypoints' fp32 rounding: 3e-5 px)
    moved = k1.double().clone()
    moved[:, 0] += 0.5
    s = sampson_error(e, k0, moved, intr)
    assert torch.allclose(sampson_error(-3.5 * e, k0, moved, intr), -s, rtol=1e-12, atol=1e-12)
    # against the definition written out: d / |J| with J the gradient of x1ᵀ F x0 in the four pixel coordinates
    from lightglue_amd import essential_to_fundamental

    f = essential_to_fundamental(e, intr).numpy()
    h0 = np.concatenate([k0.double().numpy(), np.ones((40, 1))], 1)
    h1 = np.concatenate([moved.numpy(), np.ones((40, 1))], 1)
    l1, l0 = h0 @ f.T, h1 @ f
    want = (h1 * l1).sum(1) / np.sqrt(l1[:, 0] ** 2 + l1[:, 1] ** 2 + l0[:, 0] ** 2 + l0[:, 1] ** 2)
    assert np.allclose(np.abs(s.numpy()), np.abs(want), rtol=1e-9, atol=1e-12)
    assert 0.0 < float(s.abs().max()) < 0.5 + 1e-6


def test_scene_preconditions_and_the_final_cost():
    """On the six scenes the reference's mask equals gt_mask before and after the polish, every inlier within 1.5 px
    and every outlier further than 6 px of the polished E, the polish is kept and its final cost is at most the
    entering one."""
    from lightglue_amd import epipolar_error, essential_to_fundamental

    ref, pol = ps.six_ransac(), ps.six_polished()
    for p, (k, alt) in enumerate(ps.SIX):
        k0, k1, gt = ps.scene(k, alt)[:3]
        assert torch.equal(ref.inliers[p, :k].bool(), gt) and torch.equal(pol.inliers[p, :k].bool(), gt), (k, alt)
        assert int(pol.kept[p]) == 1 and int(pol.num_inliers[p]) == int(gt.sum()) == int(pol.num_front[p]), (k, alt)
        assert float(pol.cost[p, 1]) <= float(pol.cost[p, 0]), (k, alt, pol.cost[p])
        err = epipolar_error(essential_to_fundamental(pol.E[p], ps.intrinsics()), k0, k1).sqrt()
        assert float(err[gt].max()) < 1.5 and float(err[~gt].min()) > 6.0, (k, alt)
        print(f"k {k} alt {alt}: cost {float(pol.cost[p, 0]):.3f} -> {float(pol.cost[p, 1]):.3f} px²")


def test_two_starts_reach_one_minimiser():
    """The reference from the RANSAC pose and from the true pose turned by 0.5 deg (t by 1 deg) ends at the same pose."""
    from lightglue_amd import polish_pose_reference
    from lightglue_amd.geometry import gather_correspondences

    m, counts, kp0, kp1, intr = ps.six()
    pol, worst = ps.six_polished(), 0.0
    for p, (k, alt) in enumerate(ps.SIX):
        _, _, gt, _, _, r, t = ps.scene(k, alt)
        x0, x1 = gather_correspondences(m[p], k, kp0[p], kp1[p])
        other = polish_pose_reference(*ps.turned_pose(r, t), x0, x1, intr[p], gt, ps.THRESHOLD)
        rot, tra = ps.pose_errors_deg(other.R, other.t, pol.R[p], pol.t[p])
        worst = max(worst, rot, tra)
        print(f"k {k} alt {alt}: the two starts end {rot:.3e} deg (R), {tra:.3e} deg (t) apart; cost {float(other.cost[0]):.1f} -> "
              f"{float(other.cost[1]):.3f} against {float(pol.cost[p, 1]):.3f}")
        assert int(other.kept) == 1 and torch.equal(other.inliers, pol.inliers[p, :k])
    assert worst < TWO_STARTS_BOUND_DEG


def test_keep_rule_returns_the_pose_as_given():
    """An all-ones mask on the k = 64 scene puts its 16 outliers into the fixed set: the minimiser of that cost loses
    inliers at the threshold, so R, t and the mask come back as given with kept = 0 and equal costs."""
    b, pose = ps.keep_rule()
    out = ps.polished(pose, *b)
    assert int(out.kept[0]) == 0 and int(out.num_inliers[0]) == 64
    assert torch.equal(out.R[0], pose.R[0].double()) and torch.equal(out.t[0], pose.t[0].double())
    assert torch.equal(out.inliers, pose.inliers) and float(out.cost[0, 0]) == float(out.cost[0, 1]) > 1e3
    assert abs(float((out.E[0] ** 2).sum()) - 1.0) < 1e-12


def test_invalid_and_degenerate_pairs_pass_through():
    from lightglue_amd import polish_pose_reference

    b, pose = ps.ragged_given()
    out = ps.ragged_polished()
    for p in (0, 1, 9):  # too few rows, and the bad intrinsic: invalid
        assert int(pose.valid[p]) == 0 and int(out.kept[p]) == 0 and not bool(out.E[p].any()) and not bool(out.cost[p].any())
        assert int(out.num_inliers[p]) == int(out.num_front[p]) == 0
    k0, k1, gt = ps.scene(24)[:3]
    r, t = ps.six_ransac().R[0], ps.six_ransac().t[0]
    four = torch.zeros(24, dtype=torch.uint8)
    four[torch.nonzero(gt)[:4, 0]] = 1
    for rr, tt, mask in ((r, t, four), (r, torch.zeros(3), gt), (r * float("nan"), t, gt), (r, t * float("inf"), gt)):
        one = polish_pose_reference(rr, tt, k0, k1, ps.intrinsics(), mask, ps.THRESHOLD)
        assert int(one.kept) == 0 and int(one.num_inliers) == int(torch.as_tensor(mask).bool().sum()), (rr, tt)
        assert float(one.cost[0]) == float(one.cost[1])


def test_triangulation_reprojects_within_a_millipixel():
    """noise_px = 0 under the true pose: the midpoint of the two rays reprojects within 1e-3 px in both images (the
    keypoints' fp32 rounding is 3e-5 px), every true correspondence is ok, and the other rows are zeros."""
    from lightglue_amd import calibrated_scene, triangulate_reference

    k0, k1, gt, _, kk, r, t = calibrated_scene(7, 40, 0.25, 0.0)
    intr = torch.tensor([[kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]]] * 2)
    x, ok = triangulate_reference(r, t, k0, k1, intr, gt)
    assert torch.equal(ok.bool(), gt) and not bool(x[~gt].any()) and bool((x[gt][:, 2] > 0).all())
    k = kk.numpy()
    p0 = x[gt].numpy() @ k.T
    p1 = (x[gt].numpy() @ r.numpy().T + t.numpy()) @ k.T
    d0 = np.abs(p0[:, :2] / p0[:, 2:] - k0[gt].double().numpy()).max()
    d1 = np.abs(p1[:, :2] / p1[:, 2:] - k1[gt].double().numpy()).max()
    print(f"reprojection: {d0:.3e} px and {d1:.3e} px")
    assert d0 < 1e-3 and d1 < 1e-3
    behind, ok_behind = triangulate_reference(r, -t, k0, k1, intr, gt)  # the twisted pair's translation: nothing in front
    assert not bool(ok_behind.any()) and not bool(behind.any())


# ---- the statements on the CPU ----------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which(os.environ.get("CXX", "c++")) is None, reason="no C++ compiler")
def test_host_check_runs_within_its_bounds():
    """tools/polish_host_check.py on the k = 24 scene: csrc/lightglue_polish_math.h compiled by the host compiler, the
    RANSAC and ten rounds of the polish run serially, against the float64 reference."""
    tool = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "polish_host_check.py")
    run = subprocess.run([sys.executable, tool, "--scene", "24"], capture_output=True, text=True)
    print(run.stdout[-2000:], run.stderr[-2000:])
    assert run.returncode == 0 and "0 differ in mask, counts or kept" in run.stdout
