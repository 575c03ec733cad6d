"""The absolute pose on the MI355X (csrc/lightglue_absolute.hip) against the float64 contract in
lightglue_amd/geometry_contract.py: the 3-samples bitwise, the P3P solve per hypothesis, the score hook, the whole call on
a ragged batch with untrusted inputs, the full width and the full grid, independence of the batch, capture and replay,
the planar scenes (whose pose is asserted: P3P has no planar degeneracy), lg_link_landmarks bitwise, and the chain from
a relative pose to the next view's pose as one captured piece. The scenes and their preconditions are in
absolute_scenes.py and test_absolute.py. Nothing here reads the reference tree.

The bounds are four times a worst measured with the same statements on the CPU (csrc/lightglue_absolute_math.h is
__host__ __device__; python tools/absolute_host_check.py; profiles/geometry/INDEX.md), not on a GPU:
    lg_ransac_solve3: a kept candidate's entries against the reference's, 9.424e-7 -> ENTRY_BOUND = 3.77e-6; its sample
        points' reprojection error, 3.073e-3 px (the fp32 rounding of the output: the reference's own candidates rounded
        to fp32 show the same 3.073e-3 px, below FORMAT_LIMIT = 5e-3) -> SOLVE_BOUND_PX = 1.23e-2, below the 0.05 px it
        must stay under;
    R and t of the whole call against absolute_pose_reference's: 1.582e-6 deg and 1.097e-7 map units (the fp32 rounding
        of the outputs) -> POSE_BOUND_DEG = 6.33e-6, POSE_BOUND_T = 4.39e-7.
The chain's bound is four times the float64 chain's own error against the ground truth on the scene (test_absolute.py:
2.313e-2 deg, 9.898e-4) -> CHAIN_BOUND = (9.25e-2 deg, 3.96e-3); the margin is for the fp32 map.
The tests print their figures before they assert.
"""
import numpy as np
import pytest
import torch

import absolute_scenes as ab
from gpu_common import GuardedOut, capture_on_side_stream, equal_results, same_bits

pytestmark = pytest.mark.gpu

ENTRY_BOUND = 3.77e-6
SOLVE_BOUND_PX = 1.23e-2
POSE_BOUND_DEG = 6.33e-6
POSE_BOUND_T = 4.39e-7
CHAIN_BOUND = (9.25e-2, 3.96e-3)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def ransac(hypotheses=ab.HYPOTHESES):
    from lightglue_amd import AbsolutePoseRansac

    return AbsolutePoseRansac(ab.THRESHOLD, hypotheses, ab.REFITS, ab.SEED)


def localize(dev, pts, img, counts, intr=None, er=None):
    intr = ab.batch_intrinsics(pts.shape[0]) if intr is None else intr
    r = (er or ransac()).localize(pts.to(dev), img.to(dev), counts.to(dev), intr.to(dev))
    torch.cuda.synchronize()
    return r


def abs_ptrs(dev, pts, img, counts, intr):
    t = tuple(x.to(dev).contiguous() for x in (pts, img, counts, intr))
    return t, tuple(x.data_ptr() for x in t) + (pts.shape[0], pts.shape[1])


def stream():
    return torch.cuda.current_stream().cuda_stream


def as_result(matches, counts):
    from lightglue_amd.matches import MatchResult

    return MatchResult(None, None, None, None, matches, None, counts)


# ---- the samples ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hypotheses", (1, 4096))
def test_samples3_are_bitwise_the_reference(dev, hypotheses):
    from lightglue_amd import ransac_samples3
    from lightglue_amd._host import call

    for count in (3, 4, 7, 37, 2048):
        out = GuardedOut((hypotheses, 3), torch.int32, dev, fill=torch.full((hypotheses, 3), -1, dtype=torch.int32))
        call("lg_ransac_samples3", count, hypotheses, ab.SEED, out.ptr, stream())
        torch.cuda.synchronize()
        assert torch.equal(out.check(f"samples {count}"), ransac_samples3(ab.SEED, hypotheses, count)), (count, hypotheses)


# ---- the P3P solve ----------------------------------------------------------------------------------------------
def test_solve3_against_the_reference_per_hypothesis(dev):
    """P = 2, H = 64 on the k = 64 scene. On every hypothesis the reference keeps (absolute_scenes.kept; at least three
    quarters): the same number of candidates, each GPU candidate one reference candidate's, one to one (paired by
    value, entries within ENTRY_BOUND), det R = 1 within 1e-5, and every sample point within SOLVE_BOUND_PX of its
    pixel under it."""
    from lightglue_amd import reprojection_error
    from lightglue_amd._host import call

    samples, cases = ab.solve_cases()
    pairs, h, k = ab.solve_pairs(), ab.SOLVE_H, ab.SOLVE_K
    intr = ab.intrinsics()
    keep, args = abs_ptrs(dev, torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs]),
                          torch.tensor([k, k], dtype=torch.int32), ab.batch_intrinsics(2))
    smp = samples.to(dev)
    cand = GuardedOut((2, h, 4, 12), torch.float32, dev)
    num = GuardedOut((2, h), torch.int32, dev, fill=torch.full((2, h), -1, dtype=torch.int32))
    call("lg_ransac_solve3", *args, smp.data_ptr(), h, cand.ptr, num.ptr, stream())
    torch.cuda.synchronize()
    cand, num = cand.check("candidates"), num.check("num")
    worst, worst_entry, worst_det, kept, total = 0.0, 0.0, 0.0, 0, 0
    for p, (pts, kp) in enumerate(pairs):
        for i, (s, ref, ok) in enumerate(cases[p]):
            n = int(num[p, i])
            assert 0 <= n <= 4 and not bool(cand[p, i, n:].any()) and bool(cand[p, i, :n].any(1).all()), (p, i, n)
            if not ok:
                continue
            kept += 1
            assert n == len(ref.R), (p, i, n, len(ref.R))
            got = cand[p, i, :n].double()
            refs = torch.from_numpy(np.concatenate([ref.R.reshape(-1, 9), ref.t.reshape(-1, 3)], 1))
            keys = [float((g[:9].reshape(3, 3) @ pts[s[0]].double() + g[9:]).norm()) for g in got]
            assert all(b >= a - 1e-5 for a, b in zip(keys, keys[1:])), (p, i, keys)
            taken = set()
            for g in got:
                total += 1
                dist = (refs - g).abs().amax(1)
                j = int(dist.argmin())
                worst_entry = max(worst_entry, float(dist[j]))
                assert float(dist[j]) < ENTRY_BOUND and j not in taken, (p, i, g, refs[j])
                taken.add(j)
                worst_det = max(worst_det, abs(float(torch.linalg.det(g[:9].reshape(3, 3))) - 1.0))
                worst = max(worst, float(reprojection_error(g[:9].reshape(3, 3), g[9:], pts[s], kp[s], intr).sqrt().max()))
    print(f"solve3: {kept} of {2 * h} hypotheses kept, {total} candidates, worst sample-point reprojection error {worst:.3e} px "
          f"(bound {SOLVE_BOUND_PX}), worst entry difference {worst_entry:.3e} (bound {ENTRY_BOUND}), worst |det R - 1| {worst_det:.3e}")
    assert kept >= 2 * h * 3 // 4 and total >= kept and worst < SOLVE_BOUND_PX < 0.05 and worst_det < 1e-5


# ---- the score hook ---------------------------------------------------------------------------------------------
def test_score_hook_counts_are_exact(dev):
    """The k = 200 scene under the reference's winning pose and three perturbed ones (test_absolute.py asserts that no
    row lies within 1e-2 px of the threshold under them), P = 2: the scene, and the scene with planted rows (NaN, Inf,
    points behind the camera: never inliers); a third pair with a NaN intrinsic counts nothing."""
    from lightglue_amd._host import call

    poses = ab.score_poses()
    s = ab.scene(ab.SCORE_K)
    pts, img, counts = ab.batch_of([s, s, s], [200, 200, 200], 208)
    planted = ab.plant_dirty(pts[1], img[1], s)
    intr = ab.batch_intrinsics(3).clone()
    intr[2, 3] = float("nan")
    keep, args = abs_ptrs(dev, pts, img, counts, intr)
    cand = poses[None].repeat(3, 1, 1).contiguous().to(dev)
    out = GuardedOut((3, 4), torch.int32, dev, fill=torch.full((3, 4), -1, dtype=torch.int32))
    call("lg_ransac_score_absolute", *args, cand.data_ptr(), 4, ab.THRESHOLD, out.ptr, stream())
    torch.cuda.synchronize()
    got = out.check("counts")
    want = [int((ab.score_errors(p) <= ab.THRESHOLD).sum()) for p in poses]
    dirty = []
    for p in poses:
        err = ab.score_errors(p)
        err[planted] = float("inf")
        dirty.append(int((err <= ab.THRESHOLD).sum()))
    print(f"score: {got.tolist()} against {want} and {dirty}")
    assert got[0].tolist() == want and got[1].tolist() == dirty and got[2].tolist() == [0, 0, 0, 0]


# ---- the whole call ---------------------------------------------------------------------------------------------
WORST = {"deg": 0.0, "t": 0.0}


def check_against(r, p, want, q, n, what):
    """Pair p of result r against pair q of the reference `want` over n rows: mask, counts, valid and best exactly, R in
    degrees and t in map units."""
    got = [int(r.num_inliers[p]), int(r.valid[p]), int(r.best[p])]
    ref = [int(want.num_inliers[q]), int(want.valid[q]), int(want.best[q])]
    assert got == ref, (what, got, ref)
    assert torch.equal(r.inliers[p, :n].cpu(), want.inliers[q, :n]) and not bool(r.inliers[p, n:].any()), what
    if not ref[1]:
        assert not bool(r.R[p].any()) and not bool(r.t[p].any()), what
        return
    rr, tt = r.R[p].cpu().double(), r.t[p].cpu().double()
    assert abs(float(torch.linalg.det(rr)) - 1.0) < 1e-5, what
    rot, tra = ab.pose_errors(rr, tt, want.R[q], want.t[q])
    WORST["deg"], WORST["t"] = max(WORST["deg"], rot), max(WORST["t"], tra)
    print(f"{what}: {got[0]} inliers, best {got[2]}, R {rot:.3e} deg (bound {POSE_BOUND_DEG}), t {tra:.3e} (bound {POSE_BOUND_T}); "
          f"worst so far {WORST['deg']:.3e} deg, {WORST['t']:.3e}")
    assert rot < POSE_BOUND_DEG and tra < POSE_BOUND_T, what


def test_ragged_batch_end_to_end(dev):
    """Counts 0, 3, 4, 5, 24, 64, 200, 200 under kmax 208, a pair with planted NaN / Inf points and pixels and points
    behind the camera, and a pair with a focal length of 0, through raw pointers into guarded outputs: every entry
    written, nothing outside; everything equals absolute_pose_reference's, R and t within the pose bounds; the class
    call equals the raw call bitwise."""
    from lightglue_amd import AbsolutePoseResult, _lib
    from lightglue_amd._host import call

    pts, img, counts, intr = ab.ragged()
    want = ab.ragged_reference()
    pr, kmax = pts.shape[0], pts.shape[1]
    keep, args = abs_ptrs(dev, pts, img, counts, intr)
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((pr, 3, 3), torch.float32), ((pr, 3), torch.float32), ((pr, kmax), torch.uint8), ((pr,), torch.int32),
             ((pr,), torch.int32), ((pr,), torch.int32))]
    n = _lib.load().lg_ransac_absolute_workspace(pr, kmax, ab.HYPOTHESES)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    call("lg_ransac_absolute", *args, ab.THRESHOLD, ab.HYPOTHESES, ab.REFITS, ab.SEED, ws.data_ptr(), n, *(o.ptr for o in outs),
         stream())
    torch.cuda.synchronize()
    r = AbsolutePoseResult(*(o.check(f"output {i}") for i, o in enumerate(outs)))
    assert r.valid.tolist() == [0, 0, 1, 1, 1, 1, 1, 1, 0] and int(r.inliers.max()) == 1
    assert r.num_inliers.tolist()[2:4] == [4, 5]
    for p in range(pr):
        check_against(r, p, want, p, min(int(counts[p]), kmax), f"ragged, pair {p} ({int(counts[p])} rows)")
    planted = ab.plant_dirty(pts[ab.RAGGED_DIRTY].clone(), img[ab.RAGGED_DIRTY].clone(), ab.scene(200))
    assert not bool(r.inliers[ab.RAGGED_DIRTY, planted].any())
    equal_results(localize(dev, pts, img, counts, intr), AbsolutePoseResult(*(t.to(dev) for t in r)), "the class against the raw call")


def test_full_width_and_full_grid(dev):
    """kmax = 2048 at the class's default hypotheses: the mask equals the ground truth and the reference; 4096
    hypotheses on the k = 64 scene equal the reference (the workspace and the winner's reduction at the full grid)."""
    from lightglue_amd import AbsolutePoseRansac

    pts, img, counts = ab.batch(((2048, 2048),), 2048)
    r = localize(dev, pts, img, counts, er=AbsolutePoseRansac())
    check_against(r, 0, ab.reference(2048, False, ab.WIDE_HYPOTHESES), 0, 2048, "full width")
    assert torch.equal(r.inliers[0].cpu().bool(), ab.scene(2048)[2])
    pts, img, counts = ab.batch(((64, 64),), 64)
    r = localize(dev, pts, img, counts, er=ransac(ab.FULL_HYPOTHESES))
    check_against(r, 0, ab.reference(64, False, ab.FULL_HYPOTHESES), 0, 64, "4096 hypotheses")


def test_pairs_are_independent_and_calls_deterministic(dev):
    from lightglue_amd import AbsolutePoseResult

    pts, img, counts, intr = ab.ragged()
    r = localize(dev, pts, img, counts, intr)
    equal_results(r, localize(dev, pts, img, counts, intr), "two calls")
    for p in (2, 4, 6, 7, 8):
        one = localize(dev, pts[p:p + 1], img[p:p + 1], counts[p:p + 1], intr[p:p + 1])
        equal_results(AbsolutePoseResult(*(t[p:p + 1] for t in r)), one, f"pair {p} alone")
    order = torch.arange(pts.shape[0]).flip(0)
    back = localize(dev, pts[order], img[order], counts[order], intr[order])
    equal_results(AbsolutePoseResult(*(t.flip(0) for t in back)), r, "the batch reversed")


def test_capture_and_replay_on_new_correspondences(dev):
    from lightglue_amd import AbsolutePoseResult

    specs = ((24, 24), (64, 64), (200, 200))
    a, b = ab.batch(specs, 200), ab.batch(specs, 200, alt=True)
    intr = ab.batch_intrinsics(3).to(dev)
    live = [t.to(dev).clone() for t in a]
    er = ransac()
    graph, captured = capture_on_side_stream(lambda: er.localize(live[0], live[1], live[2], intr))
    graph.replay()
    torch.cuda.synchronize()
    first = AbsolutePoseResult(*(t.clone() for t in captured))
    equal_results(first, localize(dev, *a), "replay, the captured scene")
    for dst, src in zip(live, b):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    equal_results(captured, localize(dev, *b), "replay, another scene")
    assert not same_bits(captured.R, first.R)
    for p, (k, _) in enumerate(specs):
        check_against(captured, p, ab.reference(k, True), 0, k, f"replayed, k {k}")
        assert torch.equal(captured.inliers[p, :k].cpu().bool(), ab.scene(k, True)[2])


def test_planar_landmarks_localise(dev):
    """P3P is not degenerate on a plane: mask and counts are the reference's and the pose is asserted."""
    for k, seed in ab.PLANAR_SEEDS:
        s = ab.scene(k, planar_seed=seed)
        pts, img, counts = ab.batch_of([s], [k], k)
        r = localize(dev, pts, img, counts)
        check_against(r, 0, ab.reference(k, planar_seed=seed), 0, k, f"planar, k {k} seed {seed}")
        assert torch.equal(r.inliers[0].cpu().bool(), s[2])


# ---- the link -------------------------------------------------------------------------------------------------------
def link_raw(dev, ma, ca, pa, ok, mb, cb, kb1, shared, side):
    from lightglue_amd import Landmarks
    from lightglue_amd._host import call

    pr, ka, kb = ma.shape[0], ma.shape[1], mb.shape[1]
    keep = tuple(t.to(dev).contiguous() for t in (ma, ca, pa, ok, mb, cb, kb1))
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((pr, kb, 3), torch.float32), ((pr, kb, 2), torch.float32), ((pr, kb), torch.int32), ((pr,), torch.int32))]
    call("lg_link_landmarks", keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), keep[3].data_ptr(), side, keep[4].data_ptr(),
         keep[5].data_ptr(), keep[6].data_ptr(), pr, ka, kb, shared, kb1.shape[1], *(o.ptr for o in outs), stream())
    torch.cuda.synchronize()
    return Landmarks(*(o.check(f"link output {i}") for i, o in enumerate(outs)))


@pytest.mark.parametrize("side", (1, 0))
def test_link_landmarks_is_bitwise_the_reference(dev, side):
    """The hand-made cases (duplicates, ok == 0, indices out of range, empty sides, counts past kmax) and the k = 200
    pair with every third row of A ok == 0, through raw pointers into guarded outputs: the compaction order and the
    -1 / zero padding included; the function equals the raw call."""
    from lightglue_amd import link_landmarks, link_landmarks_reference

    for name, case in (("hand-made", ab.link_hand_made()), ("k 200", ab.link_wide())):
        ma, ca, pa, ok, mb, cb, kb1, shared = case
        want = link_landmarks_reference(ma, ca, pa, ok, mb, cb, kb1, side, shared)
        got = link_raw(dev, ma, ca, pa, ok, mb, cb, kb1, shared, side)
        print(f"link, {name}, side {side}: linked {got.counts.tolist()}")
        equal_results(got, want, f"link, {name}")
        api = link_landmarks(as_result(ma.to(dev), ca.to(dev)), pa.to(dev), ok.to(dev), as_result(mb.to(dev), cb.to(dev)), kb1.to(dev),
                             side_a=side, num_shared=shared)
        torch.cuda.synchronize()
        equal_results(type(got)(*(t.cpu() for t in api)), got, f"link, {name}, the function")


# ---- the chain ------------------------------------------------------------------------------------------------------
def test_three_view_chain_is_one_captured_piece(dev):
    """EssentialRansac(polish=10).verify -> triangulate -> link_landmarks -> localize_landmarks -> inliers_on_matches on
    the three-view scene (k = 200): the replay equals the eager run bitwise, pair B's mask is the ground truth, and view
    2's pose is within CHAIN_BOUND of the truth."""
    from lightglue_amd import EssentialRansac, inliers_on_matches, link_landmarks, triangulate

    tv, k = ab.three_views(), ab.CHAIN_K
    pair_intr, cam_intr = (t.to(dev) for t in ab.chain_intrinsics())
    cnt = torch.tensor([k], dtype=torch.int32, device=dev)
    ma, mb = tv.matches_a[None].contiguous().to(dev), tv.matches_b[None].contiguous().to(dev)
    kp0, kp1, kp2 = (t[None].contiguous().to(dev) for t in (tv.kpts0, tv.kpts1, tv.kpts2))
    ea = EssentialRansac(ab.THRESHOLD, ab.HYPOTHESES, ab.REFITS, ab.SEED, polish=ab.CHAIN_POLISH)
    er = ransac()

    def chain():
        a, b = as_result(ma, cnt), as_result(mb, cnt)
        pose = ea.verify(a, kp0, kp1, pair_intr)
        points, ok = triangulate(a, kp0, kp1, pair_intr, pose)
        marks = link_landmarks(a, points, ok, b, kp2, side_a=1, num_shared=k)
        got = er.localize_landmarks(marks, cam_intr)
        return pose, marks, got, inliers_on_matches(marks, got, k)

    with torch.no_grad():
        pose, marks, got, on_b = chain()
    torch.cuda.synchronize()
    graph, captured = capture_on_side_stream(chain)
    graph.replay()
    torch.cuda.synchronize()
    for name, x, y in (("pose", pose, captured[0]), ("landmarks", marks, captured[1]), ("the absolute pose", got, captured[2])):
        equal_results(x, y, f"replay, {name}")
    assert same_bits(on_b, captured[3])
    rot, tra = ab.pose_errors(got.R[0].cpu(), got.t[0].cpu(), tv.R2, tv.t2)
    ref = ab.chain_reference()
    ref_rot, ref_tra = ab.pose_errors(ref[2].R[0], ref[2].t[0], tv.R2, tv.t2)
    print(f"the chain: {int(marks.counts[0])} landmarks, {int(got.num_inliers[0])} inliers; view 2 against the truth {rot:.3e} deg "
          f"(bound {CHAIN_BOUND[0]}), |t - t_true| {tra:.3e} (bound {CHAIN_BOUND[1]}); the float64 chain's {ref_rot:.3e} deg, {ref_tra:.3e}")
    assert int(got.valid[0]) == 1 and torch.equal(pose.inliers[0].cpu().bool(), tv.gt_a)
    assert on_b.shape == (1, k) and torch.equal(on_b[0].cpu().bool(), tv.gt_b)
    assert rot < CHAIN_BOUND[0] and tra < CHAIN_BOUND[1]
