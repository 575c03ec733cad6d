"""The homography's RANSAC, no GPU: the exports and their bindings, every argument check of the four new
lg_ransac_* entry points (nothing reaches the device), ransac_samples(size=4), the float64 reference solver and
refit, planar_scene, the preconditions of the scenes the GPU tests use, and HomographyRansac's own validation."""
import numpy as np
import pytest
import torch

import homography_scenes as hs

A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below
NAMES = ("lg_ransac_homography", "lg_ransac_samples4", "lg_ransac_solve4", "lg_ransac_score_homography")


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
    assert _lib.SIGNATURES["lg_ransac_homography"] == _lib.SIGNATURES["lg_ransac_fundamental"]
    for name in ("HomographyRansac", "HomographyResult", "homography_reference", "homography_refit", "solve4_reference",
                 "transfer_error", "planar_scene", "ransac_samples", "verify_source_images"):
        assert name in lightglue_amd.__all__ and hasattr(lightglue_amd, name), name
    assert lightglue_amd.HomographyResult._fields == ("H", "inliers", "num_inliers", "valid", "best")


def _rejects(call, bads):
    for bad in bads:
        assert call(**bad) == 1, bad


PAIR_BADS = [dict(pairs=-1), dict(pairs=65536), dict(kmax=0), dict(kmax=2049), dict(kmax=-1), dict(k0=0), dict(k1=0),
             dict(pairs=65535, kmax=1 << 13), dict(pairs=65535, k0=1 << 13), dict(pairs=65535, k1=1 << 13), dict(matches=None),
             dict(counts=None), dict(kp0=None), dict(kp1=None), dict(matches=A + 4), dict(counts=A + 2), dict(kp0=A + 4),
             dict(kp1=A + 4)]


def test_entry_points_validate_before_touching_the_device(lib):
    """An empty call returns success and every clause of every argument check rejects with the entry's name in the
    message, on fake addresses and without a device call."""
    from lightglue_amd import _lib

    def homography(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, pairs=0, kmax=64, k0=64, k1=64, thr=3.0, hyp=512, refits=2, seed=888,
                 ws=A, ws_bytes=1 << 20, h=A, inl=A, num=A, valid=A, best=A)
        a.update(kw)
        return lib.lg_ransac_homography(a["matches"], a["counts"], a["kp0"], a["kp1"], a["pairs"], a["kmax"], a["k0"], a["k1"],
                                        a["thr"], a["hyp"], a["refits"], a["seed"], a["ws"], a["ws_bytes"], a["h"], a["inl"],
                                        a["num"], a["valid"], a["best"], None)

    assert homography() == 0
    assert homography(kmax=2048, k0=1, k1=1, thr=1e-3, hyp=4096, refits=0, seed=-1, inl=A + 1, counts=A + 4, h=A + 4) == 0
    assert homography(kmax=1, hyp=1, refits=8, ws_bytes=0) == 0  # (an empty call needs no workspace)
    _rejects(homography, PAIR_BADS + [
        dict(thr=0.0), dict(thr=-3.0), dict(thr=float("nan")), dict(thr=float("inf")), dict(thr=2e6), dict(hyp=0),
        dict(hyp=4097), dict(hyp=-1), dict(refits=-1), dict(refits=9), dict(ws=None), dict(ws=A + 8),
        dict(pairs=2, ws_bytes=lib.lg_ransac_workspace(2, 64, 512) - 1), dict(h=None), dict(inl=None), dict(num=None),
        dict(valid=None), dict(best=None), dict(h=A + 2), dict(num=A + 2), dict(valid=A + 2), dict(best=A + 2)])
    assert "lg_ransac_homography" in _lib.last_error()

    def samples4(**kw):
        a = dict(count=8, hyp=64, seed=888, out=None)
        a.update(kw)
        return lib.lg_ransac_samples4(a["count"], a["hyp"], a["seed"], a["out"], None)

    _rejects(samples4, [dict(), dict(out=A + 2), dict(out=A, count=3), dict(out=A, count=2049), dict(out=A, hyp=0),
                        dict(out=A, hyp=4097)])
    assert "lg_ransac_samples4" in _lib.last_error()

    def solve4(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, pairs=0, kmax=64, k0=64, k1=64, smp=A, hyp=64, cand=A, num=A)
        a.update(kw)
        return lib.lg_ransac_solve4(a["matches"], a["counts"], a["kp0"], a["kp1"], a["pairs"], a["kmax"], a["k0"], a["k1"],
                                    a["smp"], a["hyp"], a["cand"], a["num"], None)

    assert solve4() == 0 and solve4(hyp=4096, smp=A + 4, cand=A + 4, num=A + 4) == 0
    _rejects(solve4, PAIR_BADS + [dict(hyp=0), dict(hyp=4097), dict(smp=None), dict(cand=None), dict(num=None),
                                  dict(smp=A + 2), dict(cand=A + 2), dict(num=A + 2)])
    assert "lg_ransac_solve4" in _lib.last_error()

    def score(**kw):
        a = dict(matches=A, counts=A, kp0=A, kp1=A, pairs=0, kmax=64, k0=64, k1=64, cand=A, n=8, thr=3.0, out=A)
        a.update(kw)
        return lib.lg_ransac_score_homography(a["matches"], a["counts"], a["kp0"], a["kp1"], a["pairs"], a["kmax"], a["k0"],
                                              a["k1"], a["cand"], a["n"], a["thr"], a["out"], None)

    assert score() == 0 and score(n=4096, cand=A + 4, out=A + 4, thr=1e6) == 0
    _rejects(score, PAIR_BADS + [dict(n=0), dict(n=4097), dict(thr=0.0), dict(thr=-1.0), dict(thr=float("nan")),
                                 dict(thr=2e6), dict(cand=None), dict(out=None), dict(cand=A + 2), dict(out=A + 2)])
    assert "lg_ransac_score_homography" in _lib.last_error()


# ---- ransac_samples(size=4) -------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", (4, 5, 6, 7, 37, 2048))
def test_samples4_are_in_range_distinct_deterministic_and_a_prefix(count):
    from lightglue_amd import ransac_samples

    s = ransac_samples(888, 4096, count, size=4)
    assert s.shape == (4096, 4) and s.dtype == torch.int32
    assert int(s.min()) >= 0 and int(s.max()) < count
    assert bool((s.sort(1).values.diff(dim=1) > 0).all())           # 4 distinct indices a row
    assert torch.equal(s, ransac_samples(888, 4096, count, size=4))
    assert torch.equal(s[:64], ransac_samples(888, 64, count, size=4))  # a hypothesis does not depend on H
    assert not torch.equal(s, ransac_samples(889, 4096, count, size=4))
    if count >= 7:
        assert torch.equal(s, ransac_samples(888, 4096, count)[:, :4])
        assert torch.equal(ransac_samples(888, 64, count), ransac_samples(888, 64, count, size=7))
    else:
        with pytest.raises(ValueError):
            ransac_samples(888, 64, count)  # the 7-sample is not defined below 7
    if count == 4:  # a permutation of 0..3 a row, every one of the 24 about evenly
        assert bool((s.sort(1).values == torch.arange(4)).all())
        seen = torch.unique(s, dim=0, return_counts=True)[1]
        assert len(seen) == 24 and int(seen.min()) > 4096 // 24 // 2
    if count == 2048:  # every draw covers the range
        assert int(s[:, 0].max()) > 2000 and int(s[:, 3].max()) > 2000 and int(s[:, 3].min()) < 48
    for bad in (dict(count=3), dict(size=5), dict(size=8), dict(hypotheses=0)):
        with pytest.raises(ValueError):
            ransac_samples(**dict(dict(seed=888, hypotheses=64, count=count, size=4), **bad))


# ---- the reference ----------------------------------------------------------------------------------------------
def _exact_pairs(n=40, seed=5):
    """Noise-free correspondences of a known homography, float64."""
    gen = np.random.default_rng(seed)
    h = np.array([[0.9, -0.12, 30.0], [0.08, 1.05, -12.0], [1.5e-4, -0.8e-4, 1.0]])
    x0 = gen.uniform([0, 0], [639, 479], size=(n, 2))
    q = np.concatenate([x0, np.ones((n, 1))], 1) @ h.T
    return h / np.linalg.norm(h), x0, q[:, :2] / q[:, 2:3]


def test_reference_four_point_solver_recovers_an_exact_homography():
    from lightglue_amd import ransac_samples, solve4_reference, transfer_error

    h, x0, x1 = _exact_pairs()
    seen = 0
    for s in ransac_samples(7, 32, len(x0), size=4).numpy():
        ref = solve4_reference(x0, x1, s)
        assert ref.pivot > 0 and ref.orientation >= 0 and len(ref.candidates) in (0, 1)
        for c in ref.candidates:
            assert abs(np.sqrt((c * c).sum()) - 1.0) < 1e-12 and c.flat[np.argmax(np.abs(c))] > 0
            assert float(np.abs(c - h).max()) < 1e-9
            assert float(transfer_error(c, x0, x1).sqrt().max()) < 1e-7
            seen += 1
    assert seen >= 28


def test_reference_four_point_solver_rejects_degenerate_samples():
    from lightglue_amd import solve4_reference

    h, x0, x1 = _exact_pairs()
    assert len(solve4_reference(x0, x1, [0, 1, 2, 3]).candidates) == 1
    assert len(solve4_reference(x0, x1, [0, 1, 2, 2]).candidates) == 0      # a repeated index: a zero pivot
    assert solve4_reference(x0, x1, [0, 1, 2, 2]).pivot < 1e-6
    # three collinear points (their images are collinear too: a homography keeps lines)
    a0, a1 = x0.copy(), x1.copy()
    a0[2] = 0.25 * a0[0] + 0.75 * a0[1]
    q = np.append(a0[2], 1.0) @ (h / h[2, 2]).T
    a1[2] = q[:2] / q[2]
    ref = solve4_reference(a0, a1, [0, 1, 2, 3])
    assert len(ref.candidates) == 0 and ref.orientation < 1e-9
    # a twisted quadrilateral: one point of image 1 mirrored across the line through two others flips the
    # orientation of the triples it is in, while the 8 x 9 system stays regular
    b1 = x1.copy()
    p, q_, r = b1[0], b1[1], b1[3]
    d = (q_ - p) / np.linalg.norm(q_ - p)
    b1[3] = p + 2.0 * np.dot(r - p, d) * d - (r - p)
    ref = solve4_reference(x0, b1, [0, 1, 2, 3])
    assert ref.pivot >= 1e-3 and ref.orientation > 1e-3 and len(ref.candidates) == 0


def test_reference_error_and_refit_against_an_svd_dlt():
    from lightglue_amd import homography_refit, transfer_error

    k0, k1, gt, h_true = hs.scene(200)
    e = transfer_error(h_true, k0, k1).sqrt()
    assert float(e[gt].max()) <= 3 * hs.NOISE and float(e[~gt].min()) > 12.0 - 1e-3  # (fp32 keypoints)
    h = homography_refit(k0[gt], k1[gt])
    assert h.dtype == torch.float64 and abs(float((h * h).sum()) - 1.0) < 1e-12 and float(h.flatten()[h.abs().argmax()]) > 0
    # an independent DLT: Hartley by hand, the smallest right-singular vector of the [2 n, 9] system
    x0, x1 = k0[gt].double().numpy(), k1[gt].double().numpy()

    def norm(p):
        c = p.mean(0)
        s = np.sqrt(2.0) / np.linalg.norm(p - c, axis=1).mean()
        return np.array([[s, 0, -s * c[0]], [0, s, -s * c[1]], [0, 0, 1.0]])

    t0, t1 = norm(x0), norm(x1)
    a0 = np.concatenate([x0, np.ones((len(x0), 1))], 1) @ t0.T
    a1 = np.concatenate([x1, np.ones((len(x1), 1))], 1) @ t1.T
    rows = []
    for (x, y, _), (u, v, _) in zip(a0, a1):
        rows += [[-x, -y, -1, 0, 0, 0, u * x, u * y, u], [0, 0, 0, -x, -y, -1, v * x, v * y, v]]
    hn = np.linalg.svd(np.array(rows))[2][-1].reshape(3, 3)
    want = np.linalg.inv(t1) @ hn @ t0
    want = want / np.linalg.norm(want)
    want = want if want.flat[np.argmax(np.abs(want))] > 0 else -want
    assert float(np.abs(h.numpy() - want).max()) < 1e-10
    assert float(transfer_error(h, k0, k1).sqrt()[gt].max()) < 0.75
    bad = k0.clone()
    bad[3, 0] = float("nan")
    assert bool(torch.isnan(transfer_error(h_true, bad, k1)[3])) and not bool(torch.isnan(transfer_error(h_true, bad, k1)[4]))
    assert not bool((transfer_error(torch.zeros(3, 3), k0, k1) <= 9.0).any())  # a zero matrix: no inlier anywhere
    w0 = torch.tensor([[1.0, 0, 0], [0, 1.0, 0], [1.0, 0, -float(k0[7, 0])]])
    assert not bool(torch.isfinite(transfer_error(w0, k0, k1)[7]))  # W = 0 at a point: not finite, no inlier
    with pytest.raises(ValueError):
        homography_refit(k0[:3], k1[:3])


@pytest.mark.parametrize("rotation", (False, True))
def test_planar_scene(rotation):
    from lightglue_amd import planar_scene, transfer_error

    k0, k1, gt, h = planar_scene(11, 40, 0.25, 0.5, size=(240, 320), rotation_only=rotation)
    assert k0.shape == k1.shape == (40, 2) and k0.dtype == torch.float32 and gt.dtype == torch.bool and h.shape == (3, 3)
    assert h.dtype == torch.float64 and abs(float((h * h).sum()) - 1.0) < 1e-12
    assert int(gt.sum()) == 30 and not bool(gt[:30].all())  # shuffled
    for kp in (k0, k1):
        assert float(kp[:, 0].min()) >= -1 and float(kp[:, 0].max()) <= 320 and float(kp[:, 1].max()) <= 240
    e = transfer_error(h, k0, k1).sqrt()
    # an inlier is moved by at most 0.5 px in each image; H stretches image 0's share by less than 2 on these views
    assert float(e[gt].max()) <= 0.5 * 3 and float(e[~gt].min()) > 12.0 - 1e-3
    again = planar_scene(11, 40, 0.25, 0.5, size=(240, 320), rotation_only=rotation)
    assert all(torch.equal(a, b) for a, b in zip((k0, k1, gt, h), again))
    assert not torch.equal(k0, planar_scene(12, 40, 0.25, 0.5, size=(240, 320), rotation_only=rotation)[0])
    assert not torch.equal(h, planar_scene(11, 40, 0.25, 0.5, size=(240, 320), rotation_only=not rotation)[3])
    if rotation:  # K R K⁻¹: K⁻¹ H K is a rotation up to scale
        kk = np.array([[320, 0, 160.0], [0, 320, 120.0], [0, 0, 1]])
        r = np.linalg.inv(kk) @ h.numpy() @ kk
        r = r / np.cbrt(np.linalg.det(r))
        assert float(np.abs(r @ r.T - np.eye(3)).max()) < 1e-9
    with pytest.raises(ValueError):
        planar_scene(11, 0, 0.25, 0.5)


def test_reference_rejects_small_and_clamps():
    from lightglue_amd import homography_reference

    m, counts, kp0, kp1 = hs.batch(((24, 0), (24, 3), (24, 24)), 24)
    counts[2] = 1000  # clamped to Kmax
    r = homography_reference(m, counts, kp0, kp1, hs.THRESHOLD, 64, hs.REFITS, hs.SEED)
    assert r.valid.tolist() == [0, 0, 1] and r.best.tolist()[:2] == [-1, -1] and int(r.best[2]) >= 0
    assert r.num_inliers.tolist()[:2] == [0, 0] and not bool(r.inliers[:2].any()) and not bool(r.H[:2].any())
    assert int(r.num_inliers[2]) == int(r.inliers[2].sum()) >= 4
    for bad in (dict(threshold=0.0), dict(hypotheses=0), dict(hypotheses=4097), dict(refits=-1), dict(refits=9)):
        with pytest.raises(ValueError):
            homography_reference(m, counts, kp0, kp1, **bad)


# ---- preconditions of the GPU tests' scenes ---------------------------------------------------------------------
@pytest.mark.parametrize("k,alt,rotation", [(k, False, False) for k in hs.SCENE_SEEDS] + [(k, True, False) for k in hs.ALT_SEEDS]
                         + [(hs.ROTATION_K, False, True)])
def test_gpu_scene_preconditions(k, alt, rotation):
    """The float64 reference returns exactly gt_mask, every inlier below 1.5 px and every outlier above 6 px under
    its final H (25 % outliers, 0.25 px noise, H = 256, R = 2, threshold 3)."""
    _, _, gt, _ = hs.scene(k, alt, rotation)
    r = hs.reference(k, alt, rotation)
    assert int(r.valid[0]) == 1 and 0 <= int(r.best[0]) < hs.HYPOTHESES
    assert torch.equal(r.inliers[0].bool(), gt) and int(r.num_inliers[0]) == int(gt.sum()) == k - round(k * hs.OUTLIERS)
    e = hs.errors_px(r.H[0], k, alt, rotation)
    print(f"k {k} alt {alt} rotation {rotation}: inliers <= {float(e[gt].max()):.3f} px, outliers >= {float(e[~gt].min()):.2f} px, "
          f"best {int(r.best[0])}")
    assert float(e[gt].max()) < 1.5 and float(e[~gt].min()) > 6.0


def test_gpu_solve4_cases_leave_out_at_most_a_tenth():
    _, cases = hs.solve_cases()
    kept = [c[2] for rows in cases for c in rows]
    assert len(kept) == 2 * hs.SOLVE_H and kept.count(False) <= len(kept) // 10, kept.count(False)
    assert sum(len(c[1].candidates) for rows in cases for c in rows if c[2]) >= len(kept) // 2  # most kept ones have a candidate


def test_gpu_score_inputs_keep_the_margin():
    m, counts, kp0, kp1, cands, want = hs.score_inputs()
    assert counts.tolist() == list(hs.SCORE_COUNTS) and want.shape == (len(hs.SCORE_COUNTS), cands.shape[1]) and cands.shape[1] == 9
    assert int(want[:, 0].max()) > 1000 and not bool(want[:, 6:8].any())  # the zero and the NaN matrix: no inlier
    assert int(m.min()) < 0 and int(m.max()) >= 2048 + 8 and bool(torch.isnan(kp0).any()) and bool(torch.isinf(kp1).any())
    assert bool((kp0[4:] == torch.tensor(hs.W0_POINT)).all(-1).any(1).all())  # the W = 0 point is in every pair from 63 rows on


# ---- HomographyRansac -------------------------------------------------------------------------------------------
def test_homography_ransac_validates():
    from lightglue_amd import FundamentalRansac, HomographyRansac, PluginError
    from lightglue_amd.matches import MatchResult

    for bad in (dict(threshold=0.0), dict(threshold=-1.0), dict(hypotheses=0), dict(hypotheses=4097), dict(refits=-1),
                dict(refits=9)):
        with pytest.raises(ValueError):
            HomographyRansac(**bad)
    hr = HomographyRansac()
    assert (hr.threshold, hr.hypotheses, hr.refits, hr.seed) == (3.0, 512, 2, 888)
    assert not isinstance(hr, FundamentalRansac) and "num_inliers" in HomographyRansac.__doc__
    r = MatchResult.blank(2, 16, 16, "cpu")
    with pytest.raises(PluginError, match="GPU"):
        hr.verify(r, torch.zeros(2, 16, 2), torch.zeros(2, 16, 2))
