"""The bundle adjustment on the MI355X (csrc/lightglue_bundle.hip) against the float64 contract in
lightglue_amd/geometry_contract.py (bundle_adjust_reference: scipy's sparse least squares to convergence by another route).
The scenes and their preconditions are in bundle_scenes.py and test_bundle.py. Nothing here reads the reference tree.

The bounds are four times a worst measured with the same statements on the CPU (csrc/lightglue_bundle_math.h is
__host__ __device__; python tools/bundle_host_check.py; profiles/geometry/INDEX.md), not on a GPU; the margin is for the
fp32 rounding of the outputs and the MFMA's summation order:
    against the converged reference at 10 rounds (the table stops falling at 6): R 2.895e-4 deg, t 9.033e-5 |t1|, points
        1.415e-3, the final cost 1.260e-7 relative -> REF_BOUND = (1.16e-3, 3.62e-4, 5.66e-3), COST_BOUND = 5.04e-7;
    the full width at noise 0 against the truth: R 1.506e-6 deg, t 2.323e-7, points 2.684e-5, the cost falling by the factor
        1.746e-12 -> WIDE_BOUND = (6.03e-6, 9.30e-7, 1.08e-4), WIDE_FACTOR = 6.99e-12.
The chain: the float64 chain's view 2 error falls to 0.779 (deg) and 0.777 (t) of the unrefined chain's with the bundle
adjustment appended (test_bundle.py). CHAIN_RATIO = 0.89 is half way from that ratio to 1, no improvement: the margin is for
the fp32 map and poses the GPU chain enters with, which move the unrefined error (test_gpu_absolute.py allows it four times
the float64 chain's) but not the minimiser.
The tests print their figures before they assert.
"""
import numpy as np
import pytest
import torch

import bundle_scenes as bs
from gpu_common import GuardedOut, capture_on_side_stream, equal_results, same_bits

pytestmark = pytest.mark.gpu

REF_BOUND = (1.16e-3, 3.62e-4, 5.66e-3)
COST_BOUND = 5.04e-7
WIDE_BOUND = (6.03e-6, 9.30e-7, 1.08e-4)
WIDE_FACTOR = 6.99e-12
CHAIN_RATIO = 0.89


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def refine_raw(dev, windows):
    """lg_bundle_adjust through raw pointers into guarded outputs -> the outputs on the host."""
    from lightglue_amd import _lib
    from lightglue_amd._host import call

    args = tuple(x.to(dev) for x in bs.batch(windows))
    bw, views, lmax = args[0].shape[:3]
    nbytes = int(_lib.load().lg_bundle_adjust_workspace(bw, views, lmax))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((bw, views, 3, 3), torch.float32), ((bw, views, 3), torch.float32), ((bw, lmax, 3), torch.float32),
             ((bw, 2), torch.float32), ((bw,), torch.int32), ((bw,), torch.int32))]
    call("lg_bundle_adjust", *(x.data_ptr() for x in args), bw, views, lmax, bs.ITERATIONS, ws.data_ptr(), nbytes,
         *(o.ptr for o in outs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.check(n) for o, n in zip(outs, ("R", "t", "points", "cost", "num_obs", "kept"))]


@pytest.mark.parametrize("views,k", bs.CASES)
def test_against_the_converged_reference(dev, views, k):
    w, ref = bs.window(bs.scene(views, k)), bs.reference(views, k)
    r, t, x, cost, num, kept = refine_raw(dev, [w])
    live = bs.live_of(w)[0].any(0)
    e = bs.errors(r[0], t[0], x[0], ref.R, ref.t, ref.points, live)
    rel = abs(float(cost[0, 1]) - float(ref.cost[1])) / float(ref.cost[1])
    print(f"V {views} k {k}: R {e[0]:.3e} deg, t {e[1]:.3e}, points {e[2]:.3e}, cost {rel:.3e} relative, num_obs {int(num[0])}")
    assert int(kept[0]) == 1 and int(num[0]) == int(ref.num_obs)
    assert same_bits(x[0][~live], w[6][~live]) and torch.equal(r[0, 0], torch.eye(3)) and not t[0, 0].any()
    assert all(a <= b for a, b in zip(e, REF_BOUND)), e
    assert rel <= COST_BOUND + 2.0 ** -23, rel  # (the cost is an fp32 output)


def test_full_width_reaches_the_truth(dev):
    s = bs.scene(*bs.WIDE, 0.0, bs.MISS)
    w = bs.window(s)
    r, t, x, cost, num, kept = refine_raw(dev, [w])
    mask, usable = bs.live_of(w)
    e = bs.errors(r[0], t[0], x[0], s.R, s.t, s.points, mask.any(0))
    print(f"full width: R {e[0]:.3e} deg, t {e[1]:.3e}, points {e[2]:.3e}, cost {float(cost[0, 0]):.6e} -> {float(cost[0, 1]):.3e}")
    assert usable and int(kept[0]) == 1 and int(num[0]) == int(mask.sum())
    assert all(a <= b for a, b in zip(e, WIDE_BOUND)), e
    assert float(cost[0, 1]) <= WIDE_FACTOR * float(cost[0, 0])


def test_ragged_dirty_batch(dev):
    """Counts 0, 1 and full, a view with 3 observations, dirty observations, a focal length of 0: num_obs and kept are the
    reference's, the pass-through is the input's bits, and a window alone, the batch reversed and a second call agree
    bitwise."""
    from lightglue_amd import bundle_adjust_reference

    wins, _ = bs.dirty_windows()
    got = refine_raw(dev, wins)
    for i, w in enumerate(wins):
        ref = bundle_adjust_reference(*w)
        print(f"window {i}: num_obs {int(got[4][i])} kept {int(got[5][i])} cost {got[3][i].tolist()}")
        assert int(got[4][i]) == int(ref.num_obs) and int(got[5][i]) == int(ref.kept), i
        if not int(ref.kept):
            assert same_bits(got[0][i, 1:], w[4][1:]) and same_bits(got[1][i, 1:], w[5][1:]) and same_bits(got[2][i], w[6]), i
            assert torch.equal(got[0][i, 0], torch.eye(3)) and not got[1][i, 0].any() and float(got[3][i, 0]) == float(got[3][i, 1]), i
        else:
            e = bs.errors(got[0][i], got[1][i], got[2][i], ref.R, ref.t, ref.points, bs.live_of(w)[0].any(0))
            assert all(a <= b for a, b in zip(e, REF_BOUND)), (i, e)
    assert not got[3][5].any() and not got[3][0].any()
    again, flipped = refine_raw(dev, wins), refine_raw(dev, wins[::-1])
    alone = refine_raw(dev, [wins[4]])
    for a, b, c, d in zip(got, again, flipped, alone):
        assert same_bits(a, b) and same_bits(a, c.flip(0)) and same_bits(a[4:5], d)


def test_public_interface_matches_the_raw_call(dev):
    from lightglue_amd import BundleAdjust

    w = bs.window(bs.scene(3, 64))
    res = BundleAdjust(bs.ITERATIONS).refine(*(x.to(dev) for x in bs.batch([w])))
    torch.cuda.synchronize()
    for a, b in zip(res, refine_raw(dev, [w])):
        assert same_bits(a.cpu(), b)


def test_chain_with_bundle_adjustment_is_one_captured_piece(dev):
    """EssentialRansac(polish).verify -> triangulate -> link_landmarks -> localize_landmarks -> inliers_on_matches ->
    window_from_chain -> BundleAdjust.refine on the three-view scene: the replay equals the eager run bitwise, and view 2's
    error against the truth is at most CHAIN_RATIO of the unrefined chain's on the same run."""
    import absolute_scenes as ab
    from lightglue_amd import (AbsolutePoseRansac, BundleAdjust, EssentialRansac, inliers_on_matches, link_landmarks, triangulate,
                               window_from_chain)
    from lightglue_amd.matches import MatchResult

    tv, k = ab.three_views(), ab.CHAIN_K
    pair_intr, cam_intr = (t.to(dev) for t in ab.chain_intrinsics())
    intr3 = cam_intr[:, None].repeat(1, 3, 1).contiguous()
    cnt = torch.tensor([k], dtype=torch.int32, device=dev)
    ma, mb = tv.matches_a[None].contiguous().to(dev), tv.matches_b[None].contiguous().to(dev)
    kp0, kp1, kp2 = (t[None].contiguous().to(dev) for t in (tv.kpts0, tv.kpts1, tv.kpts2))
    ea = EssentialRansac(ab.THRESHOLD, ab.HYPOTHESES, ab.REFITS, ab.SEED, polish=ab.CHAIN_POLISH)
    er, ba = AbsolutePoseRansac(ab.THRESHOLD, ab.HYPOTHESES, ab.REFITS, ab.SEED), BundleAdjust(bs.ITERATIONS)

    def chain():
        a, b = MatchResult(None, None, None, None, ma, None, cnt), MatchResult(None, None, None, None, mb, None, cnt)
        pose = ea.verify(a, kp0, kp1, pair_intr)
        points, ok = triangulate(a, kp0, kp1, pair_intr, pose)
        marks = link_landmarks(a, points, ok, b, kp2, side_a=1, num_shared=k)
        got = er.localize_landmarks(marks, cam_intr)
        w = window_from_chain(a, b, kp0, kp1, kp2, pose, points, ok, marks, got, inliers_on_matches(marks, got, k))
        return got, ba.refine(w[0], w[1], w[2], intr3, w[3], w[4], w[5])

    with torch.no_grad():
        got, fine = chain()
    torch.cuda.synchronize()
    graph, captured = capture_on_side_stream(chain)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        equal_results(got, captured[0], "replay, the absolute pose")
        equal_results(fine, captured[1], "replay, the bundle adjustment")
    before = ab.pose_errors(got.R[0].cpu(), got.t[0].cpu(), tv.R2, tv.t2)
    after = ab.pose_errors(fine.R[0, 2].cpu(), fine.t[0, 2].cpu(), tv.R2, tv.t2)
    print(f"the chain: view 2 against the truth {before[0]:.3e} deg, {before[1]:.3e} -> {after[0]:.3e} deg, {after[1]:.3e} "
          f"(ratios {after[0] / before[0]:.3f}, {after[1] / before[1]:.3f}); {int(fine.num_obs[0])} observations, cost {fine.cost[0].tolist()}")
    assert int(fine.kept[0]) == 1
    assert after[0] <= CHAIN_RATIO * before[0] and after[1] <= CHAIN_RATIO * before[1]
