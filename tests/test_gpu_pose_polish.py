"""The pose polish and the triangulation on the MI355X (csrc/lightglue_polish.hip) against the float64 contract in
lightglue_amd/geometry_contract.py (polish_reference: scipy's least squares run to convergence in another parameterisation):
polish = 0 bitwise today's call, verify(polish = 10) on the six scenes in one call, the hook on a ragged batch with
untrusted inputs through raw pointers, the full width, the keep rule, the planar pairs, independence of the batch,
repeatability, capture and replay, and lg_triangulate. The scenes and their preconditions are in polish_scenes.py and
test_pose_polish.py. Nothing here reads the reference tree.

The three bounds are four times a worst measured with the same statements on the CPU (csrc/lightglue_polish_math.h
is __host__ __device__; python tools/polish_host_check.py over every pair these tests run;
profiles/geometry/INDEX.md), not on a GPU:
    R and t against polish_reference's: 1.771e-6 deg and 6.244e-7 deg (the fp32 rounding of the outputs; the
        reference's own two starts end 3.6e-7 deg apart) -> POSE_BOUND_DEG = 7.08e-6;
    the final E against polish_reference's on the same mask, per point: 1.286e-5 px -> E_BOUND_PX = 5.14e-5;
    triangulated points against triangulate_reference, relative to their depth: 5.710e-8 (the fp32 rounding of the
        output) -> POINT_BOUND = 2.28e-7.
The last accepted step of the ten rounds was at most 2.8e-11 rad there. The tests print their figures before they
assert."""
import numpy as np
import pytest
import torch

import essential_scenes as es
import polish_scenes as ps
from gpu_common import GuardedOut, capture_on_side_stream, equal_results, same_bits

pytestmark = pytest.mark.gpu

POSE_BOUND_DEG = 7.08e-6
E_BOUND_PX = 5.14e-5
POINT_BOUND = 2.28e-7


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def ransac(**kw):
    from lightglue_amd import EssentialRansac

    return EssentialRansac(ps.THRESHOLD, ps.HYPOTHESES, ps.REFITS, ps.SEED, **kw)


def as_result(matches, counts):
    from lightglue_amd.matches import MatchResult

    return MatchResult(None, None, None, None, matches, None, counts)


def verify(dev, batch, er):
    m, counts, kp0, kp1, intr = (t.to(dev) for t in batch)
    r = er.verify(as_result(m, counts), kp0, kp1, intr)
    torch.cuda.synchronize()
    return r


def on_device(pose, dev):
    return type(pose)(*(None if t is None else t.to(dev) for t in pose))


def refine(dev, batch, pose, iterations=ps.POLISH):
    from lightglue_amd import PosePolish

    m, counts, kp0, kp1, intr = (t.to(dev) for t in batch)
    r = PosePolish(ps.THRESHOLD, iterations).refine(as_result(m, counts), kp0, kp1, intr, on_device(pose, dev))
    torch.cuda.synchronize()
    return r


WORST = {"px": 0.0, "deg": 0.0}


def check_pair(got, p, want, q, batch_row, what):
    """Pair p of the GPU's PolishResult (or polished PoseResult) against pair q of polish_reference's: mask and counts
    exactly (and kept, where `got` has it); where the reference kept the polish, E per point in pixels over the finite
    correspondences and R, t in degrees; where it passed the pose through, R, t bitwise the given ones."""
    from lightglue_amd import epipolar_error, essential_to_fundamental
    from lightglue_amd.geometry import gather_correspondences

    m, count, kp0, kp1, intr = batch_row
    x0, x1 = gather_correspondences(m, int(count), kp0, kp1)
    n = len(x0)
    a, b = [int(got.num_inliers[p]), int(got.num_front[p])], [int(want.num_inliers[q]), int(want.num_front[q])]
    if hasattr(got, "kept"):
        a.append(int(got.kept[p])), b.append(int(want.kept[q]))
        assert float(got.cost[p, 1]) <= float(got.cost[p, 0]), (what, got.cost[p])
    assert a == b, (what, a, b)
    assert torch.equal(got.inliers[p, :n].cpu(), want.inliers[q, :n]) and not bool(got.inliers[p, n:].any()), what
    e, rr, tt = got.E[p].cpu().double(), got.R[p].cpu().double(), got.t[p].cpu().double()
    if not int(want.kept[q]):
        assert torch.equal(rr, want.R[q].double()) and torch.equal(tt, want.t[q].double()), what
        return
    assert abs(float((e * e).sum()) - 1.0) < 1e-6 and float(e.flatten()[e.abs().argmax()]) > 0, what
    assert abs(float(torch.linalg.det(rr)) - 1.0) < 1e-6 and abs(float(tt.norm()) - 1.0) < 1e-6, what
    fine = torch.from_numpy(np.isfinite(x0).all(1) & np.isfinite(x1).all(1))
    diff = float((epipolar_error(essential_to_fundamental(e, intr), x0[fine], x1[fine]).sqrt()
                  - epipolar_error(essential_to_fundamental(want.E[q], intr), x0[fine], x1[fine]).sqrt()).abs().max())
    rot, tra = ps.pose_errors_deg(rr, tt, want.R[q], want.t[q])
    WORST["px"], WORST["deg"] = max(WORST["px"], diff), max(WORST["deg"], rot, tra)
    print(f"{what}: {a[0]} inliers, {a[1]} in front, E against the reference {diff:.3e} px (bound {E_BOUND_PX}), R {rot:.3e} deg, "
          f"t {tra:.3e} deg (bound {POSE_BOUND_DEG}); worst so far {WORST['px']:.3e} px, {WORST['deg']:.3e} deg")
    assert diff < E_BOUND_PX and rot < POSE_BOUND_DEG and tra < POSE_BOUND_DEG, what


def row(batch, p):
    return tuple(t[p] for t in batch)


# ---- polish = 0 -------------------------------------------------------------------------------------------------
def test_polish_zero_is_bitwise_todays_call(dev):
    from lightglue_amd import EssentialRansac

    b = ps.six()
    today = verify(dev, b, EssentialRansac(ps.THRESHOLD, ps.HYPOTHESES, ps.REFITS, ps.SEED))
    equal_results(verify(dev, b, ransac(polish=0)), today, "polish = 0")
    assert not same_bits(verify(dev, b, ransac(polish=ps.POLISH)).R, today.R)


# ---- RANSAC and polish in one call ----------------------------------------------------------------------------------
def test_verify_with_polish_on_the_six_scenes(dev):
    """P = 6 in one call: masks, num_inliers, num_front, valid and best exactly essential_reference followed by
    polish_reference; R, t and E within the bounds; and through the hook the same bits with cost[1] <= cost[0]."""
    b = ps.six()
    got, want, first = verify(dev, b, ransac(polish=ps.POLISH)), ps.six_polished(), ps.six_ransac()
    assert torch.equal(got.valid.cpu(), first.valid) and torch.equal(got.best.cpu(), first.best)
    for p, (k, alt) in enumerate(ps.SIX):
        check_pair(got, p, want, p, row(b, p), f"the six, k {k} alt {alt}")
        assert torch.equal(got.inliers[p, :k].cpu().bool(), ps.scene(k, alt)[2])
    hook = refine(dev, b, verify(dev, b, ransac()))
    for name in ("E", "R", "t", "inliers", "num_inliers", "num_front"):
        assert same_bits(getattr(hook, name), getattr(got, name)), name
    cost = hook.cost.cpu()
    print("cost (px²):", [f"{float(a):.3f} -> {float(c):.3f}" for a, c in cost], "; the reference:",
          [f"{float(a):.3f} -> {float(c):.3f}" for a, c in want.cost])
    assert bool((cost[:, 1] <= cost[:, 0]).all()) and hook.kept.cpu().tolist() == [1] * 6
    # at the minimum the cost is flat: what is left is its fp32 rounding, 6e-8 relative
    assert torch.allclose(cost[:, 1].double(), want.cost[:, 1], rtol=1e-5, atol=0.0)


# ---- the hook -------------------------------------------------------------------------------------------------------
def test_hook_on_the_ragged_batch(dev):
    """Counts 0, 4, 5, 7, 8, 24, 64, 200 under kmax 208, a pair with match indices out of range and NaN / Inf keypoints,
    and a pair with a focal length of 0, the pose and mask ragged_reference()'s, through raw pointers into guarded
    outputs: every entry written, nothing outside; invalid pairs zeros and kept = 0; the 5-row pair (as many residuals
    as parameters: no minimiser to compare) finite; every other pair the reference's."""
    from lightglue_amd import PolishResult
    from lightglue_amd._host import call

    b, pose = ps.ragged_given()
    want = ps.ragged_polished()
    m, counts, kp0, kp1, intr = b
    pr, kmax = m.shape[0], m.shape[1]
    keep = tuple(x.to(dev).contiguous() for x in b) + tuple(x.to(dev).contiguous() for x in (pose.R, pose.t, pose.inliers, pose.valid))
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((pr, 3, 3), torch.float32), ((pr, 3, 3), torch.float32), ((pr, 3), torch.float32), ((pr, kmax), torch.uint8),
             ((pr,), torch.int32), ((pr,), torch.int32), ((pr, 2), torch.float32), ((pr,), torch.int32))]
    call("lg_pose_polish", *(x.data_ptr() for x in keep[:5]), pr, kmax, kp0.shape[1], kp1.shape[1],
         *(x.data_ptr() for x in keep[5:]), ps.THRESHOLD, ps.POLISH, *(o.ptr for o in outs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = PolishResult(*(o.check(f"output {i}") for i, o in enumerate(outs)))
    assert pose.valid.tolist()[:2] == [0, 0] and pose.valid.tolist()[-1] == 0 and int(got.inliers.max()) == 1
    for p in range(pr):
        what = f"ragged, pair {p} ({int(counts[p])} rows)"
        if not int(pose.valid[p]):
            assert not any(bool(t[p].any()) for t in got), what
            continue
        assert all(bool(torch.isfinite(t[p].double()).all()) for t in got), what
        if p == ps.RAGGED_FIVE:
            print(f"{what}: kept {int(got.kept[p])}, cost {got.cost[p].tolist()}")
            assert int(got.num_inliers[p]) >= int(pose.num_inliers[p]) and float(got.cost[p, 1]) <= float(got.cost[p, 0])
            continue
        check_pair(got, p, want, p, row(b, p), what)
    assert got.kept.tolist()[5:9] == [1, 1, 1, 1]
    equal_results(refine(dev, b, pose), PolishResult(*(t.to(dev) for t in got)), "the class against the raw call")


def test_full_width(dev):
    """K = 2048 through the hook: gt_mask and the true pose turned by 0.5 deg (t by 1 deg) as input."""
    b, pose = ps.full_width()
    got, want = refine(dev, b, pose), ps.full_width_polished()
    check_pair(got, 0, want, 0, row(b, 0), "full width")
    print(f"full width: cost {got.cost[0].tolist()} px², the reference {want.cost[0].tolist()}")
    assert int(got.kept[0]) == 1 and float(got.cost[0, 1]) < float(got.cost[0, 0])
    assert torch.allclose(got.cost[0, 1].cpu().double(), want.cost[0, 1], rtol=1e-5, atol=0.0)  # (flat at the minimum: fp32 rounding)


def test_keep_rule_returns_the_inputs_bitwise(dev):
    b, pose = ps.keep_rule()
    got = refine(dev, b, pose)
    assert int(got.kept[0]) == 0 and int(got.num_inliers[0]) == 64
    assert same_bits(got.R.cpu(), pose.R) and same_bits(got.t.cpu(), pose.t) and same_bits(got.inliers.cpu(), pose.inliers)
    assert float(got.cost[0, 0]) == float(got.cost[0, 1]) > 1e3
    check_pair(got, 0, ps.polished(pose, *b), 0, row(b, 0), "keep rule")


def test_planar_pairs_lose_no_inlier(dev):
    """On a plane chance outliers sit within 0.1 px of the model, so no exact mask is asked: the polish keeps at least
    the entering inliers or passes the pose through, the cost does not rise and every output is finite."""
    for k, seed in es.PLANAR_SEEDS:
        pl = es.planar(k, seed)
        b = pl[:4] + (pl[5],)
        given = verify(dev, b, ransac())
        got = refine(dev, b, given)
        print(f"planar k {k} seed {seed}: kept {int(got.kept[0])}, inliers {int(given.num_inliers[0])} -> {int(got.num_inliers[0])}, "
              f"cost {got.cost[0].tolist()} px²")
        assert int(got.kept[0]) == 0 or int(got.num_inliers[0]) >= int(given.num_inliers[0])
        assert float(got.cost[0, 1]) <= float(got.cost[0, 0])
        assert all(bool(torch.isfinite(t.double()).all()) for t in got)
        equal_results(verify(dev, b, ransac(polish=ps.POLISH)),
                      type(given)(got.E, got.R, got.t, got.inliers, got.num_inliers, got.num_front, given.valid, given.best), "one call")


# ---- independence, repeatability, capture ---------------------------------------------------------------------------
def test_pairs_are_independent_and_calls_repeat(dev):
    from lightglue_amd import PolishResult

    b, pose = ps.ragged_given()
    r = refine(dev, b, pose)
    equal_results(r, refine(dev, b, pose), "two calls")
    for p in (2, 4, 6, 8, 9):
        one = refine(dev, tuple(t[p:p + 1] for t in b), type(pose)(*(t[p:p + 1] for t in pose)))
        equal_results(PolishResult(*(t[p:p + 1] for t in r)), one, f"pair {p} alone")
    order = torch.arange(b[0].shape[0]).flip(0)
    back = refine(dev, tuple(t[order] for t in b), type(pose)(*(t[order] for t in pose)))
    equal_results(PolishResult(*(t.flip(0) for t in back)), r, "the batch reversed")


def test_capture_and_replay_on_new_matches(dev):
    """RANSAC and polish captured as one piece on the first three scenes, replayed on the alternates."""
    from lightglue_amd import PoseResult

    a, b = ps.batch(ps.SIX[:3], ps.SIX_KMAX), ps.batch(ps.SIX[3:], ps.SIX_KMAX)
    live = [t.to(dev).clone() for t in a]
    er = ransac(polish=ps.POLISH)
    graph, captured = capture_on_side_stream(lambda: er.verify(as_result(live[0], live[1]), live[2], live[3], live[4]))
    graph.replay()
    torch.cuda.synchronize()
    first = PoseResult(*(t.clone() for t in captured))
    equal_results(first, verify(dev, a, er), "replay, the captured scenes")
    for dst, src in zip(live, b):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    equal_results(captured, verify(dev, b, er), "replay, other scenes")
    assert not same_bits(captured.R, first.R)
    want = ps.six_polished()
    for p in range(3):
        check_pair(captured, p, want, 3 + p, row(b, p), f"replayed, k {ps.SIX[3 + p][0]}")


# ---- the triangulation ----------------------------------------------------------------------------------------------
def test_triangulate_on_the_ragged_batch(dev):
    """lg_triangulate through raw pointers into guarded outputs, under ragged_reference()'s pose and mask: ok and the
    zeros exactly triangulate_reference's, the points within POINT_BOUND of their depth; the function equals the call."""
    from lightglue_amd import triangulate, triangulate_reference
    from lightglue_amd._host import call
    from lightglue_amd.geometry import gather_correspondences

    b, pose = ps.ragged_given()
    m, counts, kp0, kp1, intr = b
    pr, kmax = m.shape[0], m.shape[1]
    keep = tuple(x.to(dev).contiguous() for x in b) + tuple(x.to(dev).contiguous() for x in (pose.R, pose.t, pose.inliers))
    points = GuardedOut((pr, kmax, 3), torch.float32, dev, fill=torch.full((pr, kmax, 3), 77.0))
    ok = GuardedOut((pr, kmax), torch.uint8, dev, fill=torch.full((pr, kmax), 77, dtype=torch.uint8))
    call("lg_triangulate", *(x.data_ptr() for x in keep[:5]), pr, kmax, kp0.shape[1], kp1.shape[1], *(x.data_ptr() for x in keep[5:]),
         points.ptr, ok.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    x, good = points.check("points"), ok.check("ok")
    worst, total = 0.0, 0
    for p in range(pr):
        x0, x1 = gather_correspondences(m[p], int(counts[p]), kp0[p], kp1[p])
        n = len(x0)
        want, want_ok = triangulate_reference(pose.R[p], pose.t[p], x0, x1, intr[p], pose.inliers[p, :n])
        assert torch.equal(good[p, :n], want_ok) and not bool(good[p, n:].any()) and not bool(x[p][~good[p].bool()].any()), p
        rows = want_ok.bool()
        total += int(rows.sum())
        if bool(rows.any()):
            worst = max(worst, float(((x[p, :n][rows].double() - want[rows]).abs().amax(1) / want[rows][:, 2]).max()))
    print(f"triangulation: {total} points, worst {worst:.3e} of the depth (bound {POINT_BOUND})")
    assert total == int(pose.num_front.sum()) > 200 and worst < POINT_BOUND
    px, pok = triangulate(as_result(keep[0], keep[1]), keep[2], keep[3], keep[4], on_device(pose, dev))
    torch.cuda.synchronize()
    assert same_bits(px.cpu(), x) and same_bits(pok.cpu(), good)
