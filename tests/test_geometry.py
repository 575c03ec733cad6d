"""Geometric verification, no GPU: the exports and their bindings, every argument check of the lg_ransac_* entry
points (nothing reaches the device), ransac_samples, the float64 reference solver and refit, the scenes, the
preconditions of the scenes the GPU tests use, and FundamentalRansac's own validation."""
import numpy as np
import pytest
import torch

import geometry_scenes as gs

A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below
NAMES = ("lg_ransac_workspace", "lg_ransac_fundamental", "lg_ransac_samples", "lg_ransac_solve7", "lg_ransac_score")


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
    for name in ("FundamentalRansac", "GeometryResult", "ransac_reference", "ransac_samples", "epipolar_error",
                 "fundamental_refit", "solve7_reference", "two_view_scene", "verify_source_images"):
        assert name in lightglue_amd.__all__ and hasattr(lightglue_amd, name), name
    assert lightglue_amd.GeometryResult._fields == ("F", "inliers", "num_inliers", "valid", "best")
    assert lib.lg_ransac_workspace(0, 8, 8) == 0 and lib.lg_ransac_workspace(2, 0, 8) == 0
    assert lib.lg_ransac_workspace(3, 2048, 512) >= 3 * 512 * 11 * 4


def _rejects(call, bads):
    for bad in bads:
        assert call(**bad) == 1, bad


PAIR_BADS = [dict(pairs=-1), dict(pairs=65536), dict(kmax=0), dict(kmax=2049), dict(kmax=-1), dict(k0=0), dict(k1=0),
             dict(pairs=65535, k0=1 << 13), dict(pairs=65535, k1=1 << 13), dict(matches=None), dict(counts=None),
             dict(kp0=None), dict(kp1=None), dict(matches=A + 4), dict(counts=A + 2), dict(kp0=A + 4), dict(kp1=A + 4)]


def test_entry_points_validate_before_touching_the_device(lib):
    """An empty call returns success and every clause of every argument check rejects with the entry's name in the
    message, on fake addresses and without a device call."""
    from lightglue_amd import _lib

    def fundamental(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, pairs=0, kmax=64, k0=64, k1=64, thr=3.0, hyp=512, refits=2, seed=888,
                 ws=A, ws_bytes=1 << 20, f=A, inl=A, num=A, valid=A, best=A)
        a.update(kw)
        return lib.lg_ransac_fundamental(a["matches"], a["counts"], a["kp0"], a["kp1"], a["pairs"], a["kmax"], a["k0"], a["k1"],
                                         a["thr"], a["hyp"], a["refits"], a["seed"], a["ws"], a["ws_bytes"], a["f"], a["inl"],
                                         a["num"], a["valid"], a["best"], None)

    assert fundamental() == 0
    assert fundamental(kmax=2048, k0=1, k1=1, thr=1e-3, hyp=4096, refits=0, seed=-1, inl=A + 1, counts=A + 4, f=A + 4) == 0
    assert fundamental(kmax=1, hyp=1, refits=8, ws_bytes=0) == 0  # (an empty call needs no workspace)
    _rejects(fundamental, PAIR_BADS + [
        dict(thr=0.0), dict(thr=-3.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=2e6), dict(hyp=0),
        dict(hyp=4097), dict(hyp=-1), dict(refits=-1), dict(refits=9), dict(ws=None), dict(ws=A + 8),
        dict(pairs=2, ws_bytes=lib.lg_ransac_workspace(2, 64, 512) - 1), dict(f=None), dict(inl=None), dict(num=None),
        dict(valid=None), dict(best=None), dict(f=A + 2), dict(num=A + 2), dict(valid=A + 2), dict(best=A + 2)])
    assert "lg_ransac_fundamental" in _lib.last_error()

    def samples(**kw):
        a = dict(count=8, hyp=64, seed=888, out=None)
        a.update(kw)
        return lib.lg_ransac_samples(a["count"], a["hyp"], a["seed"], a["out"], None)

    _rejects(samples, [dict(), dict(out=A + 2), dict(out=A, count=6), dict(out=A, count=2049), dict(out=A, hyp=0),
                       dict(out=A, hyp=4097)])
    assert "lg_ransac_samples" in _lib.last_error()

    def solve7(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, pairs=0, kmax=64, k0=64, k1=64, smp=A, hyp=64, cand=A, roots=A)
        a.update(kw)
        return lib.lg_ransac_solve7(a["matches"], a["counts"], a["kp0"], a["kp1"], a["pairs"], a["kmax"], a["k0"], a["k1"],
                                    a["smp"], a["hyp"], a["cand"], a["roots"], None)

    assert solve7() == 0 and solve7(hyp=4096, smp=A + 4, cand=A + 4, roots=A + 4) == 0
    _rejects(solve7, PAIR_BADS + [dict(hyp=0), dict(hyp=4097), dict(smp=None), dict(cand=None), dict(roots=None),
                                  dict(smp=A + 2), dict(cand=A + 2), dict(roots=A + 2)])
    assert "lg_ransac_solve7" in _lib.last_error()

    def score(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, pairs=0, kmax=64, k0=64, k1=64, cand=A, n=8, thr=3.0, out=A)
        a.update(kw)
        return lib.lg_ransac_score(a["matches"], a["counts"], a["kp0"], a["kp1"], a["pairs"], a["kmax"], a["k0"], a["k1"],
                                   a["cand"], a["n"], a["thr"], a["out"], None)

    assert score() == 0 and score(n=4096, cand=A + 4, out=A + 4, thr=1e6) == 0
    _rejects(score, PAIR_BADS + [dict(n=0), dict(n=4097), dict(thr=0.0), dict(thr=float("nan")), dict(cand=None),
                                 dict(out=None), dict(cand=A + 2), dict(out=A + 2)])
    assert "lg_ransac_score" in _lib.last_error()


# ---- ransac_samples ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (7, 8, 9, 37, 2048))
def test_samples_are_in_range_distinct_and_deterministic(count):
    from lightglue_amd import ransac_samples

    s = ransac_samples(888, 4096, count)
    assert s.shape == (4096, 7) and s.dtype == torch.int32
    assert int(s.min()) >= 0 and int(s.max()) < count
    assert bool((s.sort(1).values.diff(dim=1) > 0).all())           # 7 distinct indices a row
    assert torch.equal(s, ransac_samples(888, 4096, count))
    assert torch.equal(s[:64], ransac_samples(888, 64, count))      # a hypothesis does not depend on H
    assert torch.equal(s, ransac_samples(888 + (1 << 32), 4096, count))  # the seed's low 32 bits
    assert not torch.equal(s, ransac_samples(889, 4096, count)) or count == 7
    if count == 8:  # the last draw is from 2 values: both occur, about evenly
        left = torch.tensor([sorted(set(range(8)) - set(r[:6].tolist())) for r in s])
        second = (s[:, 6] == left[:, 1]).float().mean()
        assert 0.45 < float(second) < 0.55
    if count == 2048:  # every draw covers the range
        assert int(s[:, 0].max()) > 2000 and int(s[:, 6].max()) > 2000 and int(s[:, 6].min()) < 48
    with pytest.raises(ValueError):
        ransac_samples(888, 64, 6)


# ---- the reference ----------------------------------------------------------------------------------------------
def test_reference_seven_point_solver():
    """Every candidate of a random 7-sample passes through its sample (error < 1e-9 px) and is singular
    (|det| < 1e-12 at unit norm); the candidates are in ascending root."""
    from lightglue_amd import epipolar_error, ransac_samples, solve7_reference

    k0, k1, _, _ = gs.scene(64)
    seen = 0
    for s in ransac_samples(7, 32, 64).numpy():
        ref = solve7_reference(k0, k1, s)
        assert ref.pivot > 0 and len(ref.roots) == 3 and len(ref.candidates) in (1, 3)
        for f in ref.candidates:
            assert abs(np.sqrt((f * f).sum()) - 1.0) < 1e-12 and f.flat[np.argmax(np.abs(f))] > 0
            assert float(epipolar_error(f, k0[s], k1[s]).sqrt().max()) < 1e-9
            assert abs(np.linalg.det(f)) < 1e-12
            seen += 1
    assert seen >= 32
    # a repeated point: a zero pivot, no candidate
    assert len(solve7_reference(k0, k1, [0, 1, 2, 3, 4, 5, 5]).candidates) == 0


def test_reference_error_and_refit():
    from lightglue_amd import epipolar_error, fundamental_refit

    k0, k1, gt, f_true = gs.scene(200)
    e = epipolar_error(f_true, k0, k1).sqrt()
    assert float(e[gt].max()) <= 2 * gs.NOISE and float(e[~gt].min()) > 12.0 - 1e-3  # (fp32 keypoints)
    f = fundamental_refit(k0[gt], k1[gt])
    assert f.dtype == torch.float64 and abs(float((f * f).sum()) - 1.0) < 1e-12 and abs(float(torch.linalg.det(f))) < 1e-15
    assert float(epipolar_error(f, k0, k1).sqrt()[gt].max()) < 0.75
    bad = k0.clone()
    bad[3, 0] = float("nan")
    assert bool(torch.isnan(epipolar_error(f_true, bad, k1)[3])) and not bool(torch.isnan(epipolar_error(f_true, bad, k1)[4]))
    assert bool(torch.isnan(epipolar_error(torch.zeros(3, 3), k0, k1)).all())  # a zero matrix: no inlier anywhere
    with pytest.raises(ValueError):
        fundamental_refit(k0[:7], k1[:7])


def test_two_view_scene():
    from lightglue_amd import two_view_scene

    k0, k1, gt, f = two_view_scene(11, 40, 0.25, 0.5, size=(240, 320))
    assert k0.shape == k1.shape == (40, 2) and k0.dtype == torch.float32 and gt.dtype == torch.bool and f.shape == (3, 3)
    assert int(gt.sum()) == 30 and not bool(gt[:30].all())  # shuffled
    for kp in (k0, k1):
        assert float(kp[:, 0].min()) >= -1 and float(kp[:, 0].max()) <= 320 and float(kp[:, 1].max()) <= 240
    again = two_view_scene(11, 40, 0.25, 0.5, size=(240, 320))
    assert all(torch.equal(a, b) for a, b in zip((k0, k1, gt, f), again))
    assert not torch.equal(k0, two_view_scene(12, 40, 0.25, 0.5, size=(240, 320))[0])


def test_reference_rejects_small_and_clamps():
    from lightglue_amd import ransac_reference

    m, counts, kp0, kp1 = gs.batch(((24, 0), (24, 7), (24, 24)), 24)
    counts[2] = 1000  # clamped to Kmax
    r = ransac_reference(m, counts, kp0, kp1, gs.THRESHOLD, 64, gs.REFITS, gs.SEED)
    assert r.valid.tolist() == [0, 0, 1] and r.best.tolist()[:2] == [-1, -1] and int(r.best[2]) >= 0
    assert r.num_inliers.tolist()[:2] == [0, 0] and not bool(r.inliers[:2].any()) and not bool(r.F[:2].any())
    assert int(r.num_inliers[2]) == int(r.inliers[2].sum()) >= 8
    for bad in (dict(threshold=0.0), dict(hypotheses=0), dict(hypotheses=4097), dict(refits=-1), dict(refits=9)):
        with pytest.raises(ValueError):
            ransac_reference(m, counts, kp0, kp1, **bad)


# ---- preconditions of the GPU tests' scenes ---------------------------------------------------------------------
@pytest.mark.parametrize("k,alt", [(k, False) for k in gs.SCENE_SEEDS] + [(k, True) for k in gs.ALT_SEEDS])
def test_gpu_scene_preconditions(k, alt):
    """The float64 reference returns exactly gt_mask, every inlier below 1.5 px and every outlier above 6 px under
    its final F (25 % outliers, 0.25 px noise, H = 256, R = 2, threshold 3)."""
    _, _, gt, _ = gs.scene(k, alt)
    r = gs.reference(k, alt)
    assert int(r.valid[0]) == 1 and 0 <= int(r.best[0]) < gs.HYPOTHESES
    assert torch.equal(r.inliers[0].bool(), gt) and int(r.num_inliers[0]) == int(gt.sum()) == k - round(k * gs.OUTLIERS)
    e = gs.errors_px(r.F[0], k, alt)
    print(f"k {k} alt {alt}: inliers <= {float(e[gt].max()):.3f} px, outliers >= {float(e[~gt].min()):.2f} px, best {int(r.best[0])}")
    assert float(e[gt].max()) < 1.5 and float(e[~gt].min()) > 6.0


def test_gpu_solve7_cases_leave_out_at_most_a_tenth():
    _, cases = gs.solve_cases()
    kept = [c[2] for rows in cases for c in rows]
    assert len(kept) == 2 * gs.SOLVE_H and kept.count(False) <= len(kept) // 10, kept.count(False)


def test_gpu_score_inputs_keep_the_margin():
    m, counts, kp0, kp1, cands, want = gs.score_inputs()
    assert counts.tolist() == list(gs.SCORE_COUNTS) and want.shape == (6, cands.shape[1])
    assert int(want[:, 0].max()) > 1000 and not bool(want[:, -2:].any())  # the zero and the NaN matrix: no inlier
    assert int(m.min()) < 0 and int(m.max()) >= 2048 + 8 and bool(torch.isnan(kp0).any()) and bool(torch.isinf(kp1).any())


# ---- FundamentalRansac ----------------------------------------------------------------------------------------
def test_fundamental_ransac_validates():
    from lightglue_amd import FundamentalRansac, PluginError
    from lightglue_amd.matches import MatchResult

    for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(hypotheses=0), dict(hypotheses=4097), dict(refits=-1), dict(refits=9)):
        with pytest.raises(ValueError):
            FundamentalRansac(**bad)
    fr = FundamentalRansac()
    assert (fr.threshold, fr.hypotheses, fr.refits, fr.seed) == (3.0, 512, 2, 888)
    r = MatchResult.blank(2, 16, 16, "cpu")
    with pytest.raises(PluginError, match="GPU"):
        fr.verify(r, torch.zeros(2, 16, 2), torch.zeros(2, 16, 2))
