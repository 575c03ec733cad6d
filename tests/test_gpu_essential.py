"""The calibrated five-point RANSAC on the MI355X (csrc/lightglue_essential.hip) against the float64 contract in
lightglue_amd/geometry_contract.py: the 5-samples bitwise, the five-point solve per hypothesis, the whole call on a ragged
batch with untrusted inputs, the pose hook, the full width, independence of the batch, capture and replay, the planar
scenes, and verify_source_images with intrinsics captured as one piece. The scenes and their preconditions are in
essential_scenes.py and test_essential.py. Nothing here reads the reference tree.

The three bounds are four times a worst measured with the same statements on the CPU (csrc/lightglue_essential_math.h
is __host__ __device__; python tools/essential_host_check.py; profiles/geometry/INDEX.md), not on a GPU:
    lg_ransac_solve5: the worst sample-point epipolar error under a kept candidate, 4.797e-3 px (the fp32 rounding of
        the output) -> SOLVE_BOUND_PX = 1.92e-2, below the 0.05 px it must stay under;
    the final E against essential_reference's on the same mask, per point: 2.045e-5 px -> REFIT_BOUND_PX = 8.18e-5;
    R and t against essential_reference's: 1.621e-6 deg and 8.061e-7 deg (the fp32 rounding of the outputs)
        -> POSE_BOUND_DEG = 6.48e-6.
The tests print their figures before they assert.
"""
import numpy as np
import pytest
import torch

import essential_scenes as es
from gpu_common import GuardedOut, capture_on_side_stream, equal_results, same_bits, seeded_matcher

pytestmark = pytest.mark.gpu

SOLVE_BOUND_PX = 1.92e-2
ENTRY_BOUND = 1.51e-4  # a candidate's entries against the reference's: four times the 3.765e-5 of the same host check
REFIT_BOUND_PX = 8.18e-5
POSE_BOUND_DEG = 6.48e-6


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def ransac():
    from lightglue_amd import EssentialRansac

    return EssentialRansac(es.THRESHOLD, es.HYPOTHESES, es.REFITS, es.SEED)


def as_result(matches, counts):
    from lightglue_amd.matches import MatchResult

    return MatchResult(None, None, None, None, matches, None, counts)


def verify(dev, m, counts, kp0, kp1, intr=None, er=None):
    intr = es.batch_intrinsics(m.shape[0]) if intr is None else intr
    r = (er or ransac()).verify(as_result(m.to(dev), counts.to(dev)), kp0.to(dev), kp1.to(dev), intr.to(dev))
    torch.cuda.synchronize()
    return r


def pair_ptrs(dev, m, counts, kp0, kp1, intr):
    t = tuple(x.to(dev).contiguous() for x in (m, counts, kp0, kp1, intr))
    return t, tuple(x.data_ptr() for x in t) + (m.shape[0], m.shape[1], kp0.shape[1], kp1.shape[1])


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the samples ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hypotheses", (1, 4096))
def test_samples5_are_bitwise_the_reference(dev, hypotheses):
    from lightglue_amd import ransac_samples5
    from lightglue_amd._host import call

    for count in (5, 6, 7, 37, 2048):
        out = GuardedOut((hypotheses, 5), torch.int32, dev, fill=torch.full((hypotheses, 5), -1, dtype=torch.int32))
        call("lg_ransac_samples5", count, hypotheses, es.SEED, out.ptr, stream())
        torch.cuda.synchronize()
        assert torch.equal(out.check(f"samples {count}"), ransac_samples5(es.SEED, hypotheses, count)), (count, hypotheses)


# ---- the five-point solve ---------------------------------------------------------------------------------------
def test_solve5_against_the_reference_per_hypothesis(dev):
    """P = 2, H = 64 on the k = 64 scene. On every hypothesis the reference keeps (essential_scenes.kept; at least
    three quarters): the same number of candidates, each GPU candidate canonical and one reference candidate's, one
    to one (entries within ENTRY_BOUND at unit norm, up to the sign where two entries tie for the largest; the kernel
    lists them in ascending root of its own polynomial, the reference ascending in entry [0, 0], so they are paired by
    value), and every sample point within SOLVE_BOUND_PX of its epipolar lines under it."""
    from lightglue_amd import epipolar_error, essential_to_fundamental
    from lightglue_amd._host import call

    samples, cases = es.solve_cases()
    pairs, h, k = es.solve_pairs(), es.SOLVE_H, es.SOLVE_K
    intr = es.intrinsics()
    m = torch.arange(k, dtype=torch.int32)[None, :, None].repeat(2, 1, 2)
    keep, args = pair_ptrs(dev, m, torch.tensor([k, k], dtype=torch.int32), torch.stack([p[0] for p in pairs]),
                           torch.stack([p[1] for p in pairs]), es.batch_intrinsics(2))
    smp = samples.to(dev)
    cand = GuardedOut((2, h, 10, 9), torch.float32, dev)
    num = GuardedOut((2, h), torch.int32, dev, fill=torch.full((2, h), -1, dtype=torch.int32))
    call("lg_ransac_solve5", *args, smp.data_ptr(), h, cand.ptr, num.ptr, stream())
    torch.cuda.synchronize()
    cand, num = cand.check("candidates"), num.check("num")
    worst, worst_entry, kept, total = 0.0, 0.0, 0, 0
    for p, (x0, x1) in enumerate(pairs):
        for i, (s, ref, ok) in enumerate(cases[p]):
            n = int(num[p, i])
            assert 0 <= n <= 10 and not bool(cand[p, i, n:].any()) and bool(cand[p, i, :n].any(1).all()), (p, i, n)
            if not ok:
                continue
            kept += 1
            assert n == len(ref.candidates), (p, i, n, len(ref.candidates))
            got, refs = cand[p, i, :n].double(), torch.from_numpy(ref.candidates).reshape(-1, 9)
            taken = set()
            for g in got:
                total += 1
                assert abs(float((g ** 2).sum()) - 1.0) < 1e-6 and float(g[g.abs().argmax()]) > 0, (p, i)
                dist = torch.minimum((refs - g).abs().amax(1), (refs + g).abs().amax(1))
                j = int(dist.argmin())
                worst_entry = max(worst_entry, float(dist[j]))
                assert float(dist[j]) < ENTRY_BOUND and j not in taken, (p, i, g, refs[j])
                taken.add(j)
                f = essential_to_fundamental(g.reshape(3, 3), intr)
                worst = max(worst, float(epipolar_error(f, x0[s], x1[s]).sqrt().max()))
    print(f"solve5: {kept} of {2 * h} hypotheses kept, {total} candidates, worst sample-point epipolar error {worst:.3e} px "
          f"(bound {SOLVE_BOUND_PX}), worst entry difference {worst_entry:.3e}")
    assert kept >= 2 * h * 3 // 4 and total >= kept and worst < SOLVE_BOUND_PX < 0.05


# ---- the whole call ---------------------------------------------------------------------------------------------
WORST = {"px": 0.0, "deg": 0.0}


def check_against(r, p, want, q, x0, x1, intr, what, pose=True):
    """Pair p of result r against pair q of the reference `want`: mask, counts, valid and best exactly, E per point in
    pixels over the finite correspondences (x0, x1), R and t in degrees."""
    from lightglue_amd import epipolar_error, essential_to_fundamental

    n = len(x0)
    got = [int(r.num_inliers[p]), int(r.num_front[p]), int(r.valid[p]), int(r.best[p])]
    ref = [int(want.num_inliers[q]), int(want.num_front[q]), int(want.valid[q]), int(want.best[q])]
    assert got[2:] == ref[2:] and got[0] == ref[0], (what, got, ref)
    assert torch.equal(r.inliers[p, :n].cpu(), want.inliers[q, :n]) and not bool(r.inliers[p, n:].any()), what
    if not ref[2]:
        assert not bool(r.E[p].any()) and not bool(r.R[p].any()) and not bool(r.t[p].any()) and got[1] == 0, what
        return
    e, rr, tt = r.E[p].cpu().double(), r.R[p].cpu().double(), r.t[p].cpu().double()
    assert abs(float((e * e).sum()) - 1.0) < 1e-6 and float(e.flatten()[e.abs().argmax()]) > 0, what
    assert abs(float(torch.linalg.det(rr)) - 1.0) < 1e-5 and abs(float(tt.norm()) - 1.0) < 1e-6, what
    fine = torch.from_numpy(np.isfinite(x0).all(1) & np.isfinite(x1).all(1))
    a = epipolar_error(essential_to_fundamental(e, intr), x0[fine], x1[fine]).sqrt()
    b = epipolar_error(essential_to_fundamental(want.E[q], intr), x0[fine], x1[fine]).sqrt()
    diff = float((a - b).abs().max())
    WORST["px"] = max(WORST["px"], diff)
    line = f"{what}: {got[0]} inliers, {got[1]} in front, E against the reference {diff:.3e} px (bound {REFIT_BOUND_PX})"
    if pose:
        assert got[1] == ref[1], (what, got, ref)
        rot, tra = es.pose_errors_deg(rr, tt, want.R[q], want.t[q])
        WORST["deg"] = max(WORST["deg"], rot, tra)
        line += f", R {rot:.3e} deg, t {tra:.3e} deg (bound {POSE_BOUND_DEG})"
    print(line + f"; worst so far {WORST['px']:.3e} px, {WORST['deg']:.3e} deg")
    assert diff < REFIT_BOUND_PX, what
    if pose:
        assert rot < POSE_BOUND_DEG and tra < POSE_BOUND_DEG, what


def gathered(m, count, kp0, kp1):
    from lightglue_amd.geometry import gather_correspondences

    return gather_correspondences(m, int(count), kp0, kp1)


def test_ragged_batch_end_to_end(dev):
    """Counts 0, 4, 5, 7, 8, 24, 64, 200 under kmax 208, a pair with match indices out of range and NaN / Inf
    keypoints, and a pair with a focal length of 0, through raw pointers into guarded outputs: every entry written,
    nothing outside; masks, num_inliers, valid and best exactly essential_reference's."""
    from lightglue_amd import PoseResult, _lib
    from lightglue_amd._host import call

    m, counts, kp0, kp1, intr = es.ragged()
    want = es.ragged_reference()
    pr, kmax = m.shape[0], m.shape[1]
    keep, args = pair_ptrs(dev, m, counts, kp0, kp1, intr)
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((pr, 3, 3), torch.float32), ((pr, 3, 3), torch.float32), ((pr, 3), torch.float32), ((pr, kmax), torch.uint8),
             ((pr,), torch.int32), ((pr,), torch.int32), ((pr,), torch.int32), ((pr,), torch.int32))]
    n = _lib.load().lg_ransac_essential_workspace(pr, kmax, es.HYPOTHESES)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    call("lg_ransac_essential", *args, es.THRESHOLD, es.HYPOTHESES, es.REFITS, es.SEED, ws.data_ptr(), n, *(o.ptr for o in outs),
         stream())
    torch.cuda.synchronize()
    r = PoseResult(*(o.check(f"output {i}") for i, o in enumerate(outs)))
    assert r.valid.tolist()[:2] == [0, 0] and r.valid.tolist()[-1] == 0 and int(r.inliers.max()) == 1
    for p in range(pr):
        x0, x1 = gathered(m[p], counts[p], kp0[p], kp1[p])
        check_against(r, p, want, p, x0, x1, intr[p], f"ragged, pair {p} ({int(counts[p])} rows)")
    equal_results(verify(dev, m, counts, kp0, kp1, intr), PoseResult(*(t.to(dev) for t in r)), "the class against the raw call")


def test_full_width(dev):
    m, counts, kp0, kp1 = es.batch(((2048, 2048),), 2048)
    r = verify(dev, m, counts, kp0, kp1)
    x0, x1 = gathered(m[0], 2048, kp0[0], kp1[0])
    check_against(r, 0, es.reference(2048), 0, x0, x1, es.intrinsics(), "full width")
    assert torch.equal(r.inliers[0].cpu().bool(), es.scene(2048)[2])


def test_pairs_are_independent_and_calls_deterministic(dev):
    from lightglue_amd import PoseResult

    m, counts, kp0, kp1, intr = es.ragged()
    r = verify(dev, m, counts, kp0, kp1, intr)
    equal_results(r, verify(dev, m, counts, kp0, kp1, intr), "two calls")
    for p in (2, 4, 6, 8, 9):
        one = verify(dev, m[p:p + 1], counts[p:p + 1], kp0[p:p + 1], kp1[p:p + 1], intr[p:p + 1])
        equal_results(PoseResult(*(t[p:p + 1] for t in r)), one, f"pair {p} alone")
    order = torch.arange(m.shape[0]).flip(0)
    back = verify(dev, m[order], counts[order], kp0[order], kp1[order], intr[order])
    equal_results(PoseResult(*(t.flip(0) for t in back)), r, "the batch reversed")


def test_capture_and_replay_on_new_matches(dev):
    from lightglue_amd import PoseResult

    specs = ((24, 24), (64, 64), (200, 200))
    a, b = es.batch(specs, 200), es.batch(specs, 200, alt=True)
    intr = es.batch_intrinsics(3).to(dev)
    live = [t.to(dev).clone() for t in a]
    er = ransac()
    graph, captured = capture_on_side_stream(lambda: er.verify(as_result(live[0], live[1]), live[2], live[3], intr))
    graph.replay()
    torch.cuda.synchronize()
    first = PoseResult(*(t.clone() for t in captured))
    equal_results(first, verify(dev, *a), "replay, the captured scene")
    for dst, src in zip(live, b):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    equal_results(captured, verify(dev, *b), "replay, another scene")
    assert not same_bits(captured.E, first.E)
    for p, (k, _) in enumerate(specs):
        x0, x1 = gathered(b[0][p], k, b[2][p], b[3][p])
        check_against(captured, p, es.reference(k, True), 0, x0, x1, es.intrinsics(), f"replayed, k {k}")
        assert torch.equal(captured.inliers[p, :k].cpu().bool(), es.scene(k, True)[2])


def test_planar_scenes_equal_the_reference(dev):
    """On a plane the refit's 8-point fit is degenerate and the keep rule holds the five-point winner: mask and counts
    are the reference's. The pose is not asserted: two solutions fit a plane."""
    for k, seed in es.PLANAR_SEEDS:
        m, counts, kp0, kp1, gt, intr = es.planar(k, seed)
        r = verify(dev, m, counts, kp0, kp1, intr)
        x0, x1 = gathered(m[0], k, kp0[0], kp1[0])
        check_against(r, 0, es.planar_reference(k, seed), 0, x0, x1, intr[0], f"planar, k {k} seed {seed}", pose=False)
        assert bool((r.inliers[0].cpu().bool() | ~gt).all())


# ---- the pose -----------------------------------------------------------------------------------------------------
def test_pose_from_essential_picks_the_pose_in_front(dev):
    """Noise-free all-inlier scenes (num_front is then the count), the true E with either sign and at another scale,
    and a scene whose second camera moved the other way (R and t inverted, the images swapped): R and t are the
    truth, and each of the other three decompositions puts fewer points in front. A zero E and a bad intrinsic give
    zeros; an empty mask counts nothing in front."""
    from lightglue_amd import calibrated_scene, camera_coordinates, pose_from_essential_reference
    from lightglue_amd._host import call

    true_essential = es.true_essential
    k = 40
    k0, k1, _, _, kk, r, t = calibrated_scene(7, k, 0.0, 0.0)
    intr = es.intrinsics_of(kk)
    e = torch.from_numpy(true_essential(r, t))
    r_back, t_back = r.T.contiguous(), -(r.T @ t)
    e_back = torch.from_numpy(true_essential(r_back, t_back))
    zero = torch.zeros(3, 3, dtype=torch.float64)
    cases = [(k0, k1, e, r, t), (k0, k1, -e, r, t), (k0, k1, 3.5 * e, r, t), (k1, k0, e_back, r_back, t_back),
             (k0, k1, zero, None, None), (k0, k1, e, None, None), (k0, k1, e, r, t)]
    pr = len(cases)
    m = torch.arange(k, dtype=torch.int32)[None, :, None].repeat(pr, 1, 2)
    intrs = intr[None].repeat(pr, 1, 1).clone()
    intrs[5, 0, 0] = float("nan")
    inl = torch.ones((pr, k), dtype=torch.uint8)
    inl[6] = 0
    inl[0, 3] = 0  # a row left out of the vote
    keep, args = pair_ptrs(dev, m, torch.full((pr,), k, dtype=torch.int32), torch.stack([c[0] for c in cases]),
                           torch.stack([c[1] for c in cases]), intrs)
    e_dev, inl_dev = torch.stack([c[2] for c in cases]).float().to(dev), inl.to(dev)
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((pr, 3, 3), torch.float32), ((pr, 3), torch.float32), ((pr,), torch.int32))]
    call("lg_pose_from_essential", *args, e_dev.data_ptr(), inl_dev.data_ptr(), *(o.ptr for o in outs), stream())
    torch.cuda.synchronize()
    rr, tt, front = (o.check(f"output {i}") for i, o in enumerate(outs))
    for p, (a, b, ee, r_want, t_want) in enumerate(cases):
        if r_want is None:
            assert not bool(rr[p].any()) and not bool(tt[p].any()) and int(front[p]) == 0, p
            continue
        if p == 6:  # nothing votes: the four tie at 0 and the first decomposition stands
            assert int(front[p]) == 0 and abs(float(torch.linalg.det(rr[p].double())) - 1.0) < 1e-5, p
            continue
        rows = inl[p].bool()
        q0, q1 = camera_coordinates(a[rows], intr[0]), camera_coordinates(b[rows], intr[1])
        _, _, front_want, others = pose_from_essential_reference(ee, q0, q1)
        rot, tra = es.pose_errors_deg(rr[p].double(), tt[p].double(), r_want, t_want)
        print(f"pose, case {p}: {int(front[p])} in front (the four decompositions: {others}), R {rot:.3e} deg, t {tra:.3e} deg")
        assert int(front[p]) == front_want == int(rows.sum()) and sorted(others)[2] < front_want, (p, others)
        # E is rounded to fp32 on the way in: 6e-8 an entry at unit norm is 3.4e-6 deg, times the nine entries and a
        # condition of the decomposition of a few: below 1e-4 deg
        assert rot < 1e-4 and tra < 1e-4, p


# ---- verify_source_images -------------------------------------------------------------------------------------------
def test_verify_source_images_with_intrinsics_is_one_captured_piece(dev):
    """Seeded weights and two small image pairs (the sizes tests/test_gpu_image_input.py uses), eager against its parts
    and captured as one graph. The seeded weights match nothing the five-point solve can use: what is checked is that
    the outputs are consistent with themselves and that the replay is the eager result."""
    from lightglue_amd import (EssentialRansac, ImageInput, KeypointFrontend, PoseResult, SuperPointEncoder, match_source_images,
                               seeded_superpoint_state_dict, verify_source_images)

    def rand_u8(seed, *shape):
        return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)

    encoder, model = SuperPointEncoder(seeded_superpoint_state_dict(3)), seeded_matcher(dev)
    fe, ii, er = KeypointFrontend(max_keypoints=64), ImageInput((40, 72)), EssentialRansac(hypotheses=128)
    s0 = [rand_u8(100, 50, 70, 3).to(dev), rand_u8(101, 96, 64).to(dev)]
    s1 = [rand_u8(110, 61, 83).to(dev), rand_u8(111, 40, 120, 3).to(dev)]
    intr = torch.tensor([[[70.0, 70.0, 35.0, 25.0], [83.0, 83.0, 41.5, 30.5]], [[96.0, 96.0, 32.0, 48.0], [120.0, 120.0, 60.0, 20.0]]]).to(dev)
    with torch.no_grad():
        result, kp0, kp1, geo = verify_source_images(ii, encoder, fe, model, er, s0, s1, intrinsics=intr)
        want, w0, w1 = match_source_images(ii, encoder, fe, model, s0, s1)
        torch.cuda.synchronize()
        equal_results(result, want, "the matches")
        assert same_bits(kp0, w0) and same_bits(kp1, w1)
        equal_results(geo, er.verify(want, w0, w1, intr), "the verification")
    assert isinstance(geo, PoseResult) and geo.E.shape == geo.R.shape == (2, 3, 3) and geo.t.shape == (2, 3)
    assert geo.inliers.shape == (2, result.matches.shape[1])
    counts = result.counts.cpu()
    for p in range(2):  # whatever the seeded weights match: the outputs are consistent with themselves
        assert int(geo.num_front[p]) <= int(geo.num_inliers[p]) == int(geo.inliers[p].sum()) <= max(int(counts[p]), 0)
        assert int(geo.valid[p]) == (1 if int(geo.best[p]) >= 0 else 0)
        assert bool(geo.E[p].any()) == bool(geo.R[p].any()) == bool(geo.valid[p])
    t0, t1 = ii.table(s0), ii.table(s1)  # (the tables are built once, before the capture)
    graph, captured = capture_on_side_stream(lambda: verify_source_images(ii, encoder, fe, model, er, t0, t1, intrinsics=intr))
    graph.replay()
    torch.cuda.synchronize()
    equal_results(captured[0], result, "replay, the matches")
    assert same_bits(captured[1], kp0) and same_bits(captured[2], kp1)
    equal_results(captured[3], geo, "replay, the verification")
