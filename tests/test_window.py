"""The sequence window's float64 contract on the CPU (lightglue_amd/geometry_contract.py): the preconditions the GPU tests
(test_gpu_window.py) rest on, and the figures their bounds come from. Nothing here needs a GPU or the library."""
import numpy as np
import pytest

import window_scenes as ws


@pytest.mark.parametrize("views,k,lmax", ws.TRACK_CASES)
def test_scene_rows_are_dirty_and_tracks_are_simple_paths(views, k, lmax):
    s = ws.scene(views, k)
    tk, kept, found = ws.tracks(views, k, lmax)
    m, c = s.matches.numpy(), s.counts.numpy()
    if k >= 16:  # duplicates, masked rows, counts below Kmax and indices out of range, all below the count
        for v in range(views - 1):
            live = m[v, :c[v]]
            assert len(set(live[:, 0])) < len(live) and (s.mask[v, :c[v]] == 0).any() and c[v] < k
            assert (live >= k).any() and (live < 0).any()
    assert kept == min(found, lmax) and (tk[:, kept:] == -1).all()
    for v in range(views):  # no keypoint belongs to two tracks; every kept track has at least two consecutive views
        used = tk[v][tk[v] >= 0]
        assert len(set(used)) == len(used)
    has = tk[:, :kept] >= 0
    assert (has.sum(0) >= 2).all() and (np.abs(np.diff(has.astype(int), axis=0)).sum(0) <= 2).all()
    if (views, k, lmax) == (8, 300, 64):
        assert found > lmax


@pytest.mark.parametrize("views,k", list(ws.POINT_CASES))
def test_point_preconditions_and_bounds(views, k):
    """No error within 1e-3 px of the threshold, no pivot within a factor 2 of PARALLAX_EPS n, at least 90 % of the true
    tracks ok, some observation dropped where there are 4 views or more; the fixed rounds' distance from scipy's
    minimiser and the contract's sensitivity to the order of a track's sums are below the constants the GPU bounds use."""
    ref, true = ws.points(views, k), ws.true_tracks(views, k)
    ok = ref[4].astype(bool)
    frac = ok[true].sum() / len(true)
    dropped = int(((ref[5] != 0) & (ref[1] == 0) & ws.posed_of(views, k).numpy()[:, None].astype(bool) & ok[None, :]).sum())
    conv = ws.converged(views, k)
    dist = max(np.abs(ref[3][l] - x).max() for l, x in conv.items())
    serial = ws.points(views, k, order=lambda terms: sum(terms[1:], terms[0]))
    order = np.abs(serial[3] - ref[3]).max()
    print(f"V {views} k {k}: margins {ref[6]}, true tracks ok {frac:.3f}, dropped {dropped}, converged {dist:.3e}, order {order:.3e}")
    assert ref[6][0] > 1e-3 and ref[6][1] > 2.0 and frac >= 0.9
    assert views < 4 or dropped > 0
    assert (serial[1] == ref[1]).all() and (serial[4] == ref[4]).all()
    assert dist <= ws.CONVERGED and order <= ws.ORDER


def test_sequence_reference_ratio():
    """The float64 five-view sequence: views 3 and 4 get valid poses, the bundle adjustment is kept, and view 4's error
    against the truth falls by the ratios SEQUENCE_RATIO is half way to 1 from."""
    before, after, valid, kept = ws.sequence_reference()
    ratios = (after[0] / before[0], after[1] / before[1])
    print(f"view 4: {before[0]:.3e} deg, {before[1]:.3e} -> {after[0]:.3e} deg, {after[1]:.3e} (ratios {ratios[0]:.3f}, {ratios[1]:.3f})")
    assert valid == (1, 1) and kept == 1
    assert all(0.5 * (1.0 + r) <= b < 1.0 for r, b in zip(ratios, ws.SEQUENCE_RATIO))
