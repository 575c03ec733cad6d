"""Geometric verification on the MI355X (csrc/lightglue_geometry.hip) against the float64 contract in
lightglue_amd/geometry_contract.py: the samples bitwise, the 7-point solve per hypothesis, the scoring counts exactly, the
whole call on ragged batches and at full width, independence of the batch, determinism, capture and replay, and
verify_source_images against its parts. The scenes and their preconditions are in geometry_scenes.py and
test_geometry.py. Nothing here reads the reference tree.

Measured on the first run (profiles/geometry/INDEX.md) and pinned at four times that:
    lg_ransac_solve7: the worst sample-point error under a kept GPU candidate, 4.807e-3 px -> SOLVE_BOUND_PX =
        1.92e-2 (the fp32 rounding of the candidate alone reaches FORMAT_LIMIT = 5e-3 px on the kept hypotheses);
    the final F against fundamental_refit on the same mask, per point, 2.945e-5 px (the k = 24 scene) ->
        REFIT_BOUND_PX = 1.18e-4.
"""
import pytest
import torch

import geometry_scenes as gs
from gpu_common import GuardedOut, capture_on_side_stream, equal_results, same_bits, seeded_matcher

pytestmark = pytest.mark.gpu

SOLVE_BOUND_PX = 1.92e-2
REFIT_BOUND_PX = 1.18e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def ransac():
    from lightglue_amd import FundamentalRansac

    return FundamentalRansac(gs.THRESHOLD, gs.HYPOTHESES, gs.REFITS, gs.SEED)


def as_result(matches, counts):
    from lightglue_amd.matches import MatchResult

    return MatchResult(None, None, None, None, matches, None, counts)


def verify(dev, m, counts, kp0, kp1, fr=None):
    r = (fr or ransac()).verify(as_result(m.to(dev), counts.to(dev)), kp0.to(dev), kp1.to(dev))
    torch.cuda.synchronize()
    return r


def pair_ptrs(dev, m, counts, kp0, kp1):
    t = tuple(x.to(dev).contiguous() for x in (m, counts, kp0, kp1))
    return t, tuple(x.data_ptr() for x in t) + (m.shape[0], m.shape[1], kp0.shape[1], kp1.shape[1])


# ---- the samples ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hypotheses", (64, 4096))
def test_samples_are_bitwise_the_reference(dev, hypotheses):
    from lightglue_amd import ransac_samples
    from lightglue_amd._host import call

    for count in (8, 9, 37, 2048):
        out = GuardedOut((hypotheses, 7), torch.int32, dev, fill=torch.full((hypotheses, 7), -1, dtype=torch.int32))
        call("lg_ransac_samples", count, hypotheses, gs.SEED, out.ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert torch.equal(out.check(f"samples {count}"), ransac_samples(gs.SEED, hypotheses, count)), (count, hypotheses)


# ---- the 7-point solve ------------------------------------------------------------------------------------------
def test_solve7_against_the_reference_per_hypothesis(dev):
    """P = 2, H = 64 on the k = 64 scene. On every hypothesis the reference keeps (geometry_scenes.solve_cases: at most
    a tenth is left out): the same number of candidates, each GPU candidate nearest to a reference candidate of its
    own, and every sample point within SOLVE_BOUND_PX of the GPU candidate's epipolar lines."""
    from lightglue_amd import epipolar_error
    from lightglue_amd._host import call

    samples, cases = gs.solve_cases()
    pairs, h = gs.solve_pairs(), gs.SOLVE_H
    k = gs.SOLVE_K
    m = torch.arange(k, dtype=torch.int32)[None, :, None].repeat(2, 1, 2)
    keep, args = pair_ptrs(dev, m, torch.tensor([k, k], dtype=torch.int32), torch.stack([p[0] for p in pairs]),
                           torch.stack([p[1] for p in pairs]))
    smp = samples.to(dev)
    cand = GuardedOut((2, h, 3, 9), torch.float32, dev)
    roots = GuardedOut((2, h), torch.int32, dev, fill=torch.full((2, h), -1, dtype=torch.int32))
    call("lg_ransac_solve7", *args, smp.data_ptr(), h, cand.ptr, roots.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cand, roots = cand.check("candidates"), roots.check("num_roots")
    worst, kept = 0.0, 0
    for p, (x0, x1) in enumerate(pairs):
        for i, (s, ref, ok) in enumerate(cases[p]):
            n = int(roots[p, i])
            assert 0 <= n <= 3 and not bool(cand[p, i, n:].any()), (p, i)
            if not ok:
                continue
            kept += 1
            assert n == len(ref.candidates), (p, i, n, len(ref.candidates))
            got = cand[p, i, :n].double().reshape(n, 1, 9)
            want = torch.from_numpy(ref.candidates).reshape(1, n, 9)
            dist = torch.minimum((got - want).abs().amax(2), (got + want).abs().amax(2))  # (a candidate's sign is free)
            assert sorted(dist.argmin(1).tolist()) == list(range(n)), (p, i, dist)
            for c in cand[p, i, :n]:
                assert abs(float((c.double() ** 2).sum()) - 1.0) < 1e-6
                worst = max(worst, float(epipolar_error(c.reshape(3, 3), x0[s], x1[s]).sqrt().max()))
    print(f"solve7: {kept} of {2 * h} hypotheses kept, worst sample-point error {worst:.3e} px (bound {SOLVE_BOUND_PX})")
    assert kept >= 2 * h - 2 * h // 10 and worst < SOLVE_BOUND_PX < 0.05


def test_solve7_small_pairs_and_bad_samples_give_nothing(dev):
    """count < 8: zeros. Samples out of range are clamped; a repeated index is a zero pivot: no candidate."""
    from lightglue_amd._host import call

    mm, counts, kp0, kp1 = gs.batch(((24, 7), (24, 24)), 24)
    keep, args = pair_ptrs(dev, mm, counts, kp0, kp1)
    smp = torch.tensor([[0, 1, 2, 3, 4, 5, 5], [0, 1, 2, 3, 4, 5, 99], [-4, 1, 2, 3, 4, 5, 0], [3, 9, 1, 20, 7, 14, 11]],
                       dtype=torch.int32).to(dev)
    cand = GuardedOut((2, 4, 3, 9), torch.float32, dev)
    roots = GuardedOut((2, 4), torch.int32, dev, fill=torch.full((2, 4), -1, dtype=torch.int32))
    call("lg_ransac_solve7", *args, smp.data_ptr(), 4, cand.ptr, roots.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cand, roots = cand.check("candidates"), roots.check("num_roots")
    assert roots[0].tolist() == [0, 0, 0, 0] and not bool(cand[0].any())
    assert roots[1, 0] == 0 and roots[1, 2] == 0 and int(roots[1, 1]) in (1, 3) and int(roots[1, 3]) in (1, 3)


# ---- the scoring ------------------------------------------------------------------------------------------------
def test_score_counts_are_exactly_the_float64_counts(dev):
    """Ragged counts 1, 63, 64, 65, 300, 2048 in one launch, out-of-range match indices, NaN and Inf keypoints, a
    zero and a NaN candidate; no float64 error within 0.02 px of the threshold (geometry_scenes.score_inputs)."""
    from lightglue_amd._host import call

    m, counts, kp0, kp1, cands, want = gs.score_inputs()
    keep, args = pair_ptrs(dev, m, counts, kp0, kp1)
    c = cands.to(dev).contiguous()
    out = GuardedOut(tuple(want.shape), torch.int32, dev, fill=torch.full(tuple(want.shape), -1, dtype=torch.int32))
    call("lg_ransac_score", *args, c.data_ptr(), c.shape[1], gs.THRESHOLD, out.ptr, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = out.check("inlier counts")
    assert torch.equal(got, want), (got.tolist(), want.tolist())


# ---- the whole call ---------------------------------------------------------------------------------------------
def check_pair(r, p, k, count_rows, what, alt=False):
    """Pair p of result r is the whole scene k: the mask is gt_mask, F separates as the contract's preconditions
    say and agrees with fundamental_refit on that mask."""
    from lightglue_amd import fundamental_refit

    k0, k1, gt, _ = gs.scene(k, alt)
    f = r.F[p].cpu().double()
    assert int(r.valid[p]) == 1 and 0 <= int(r.best[p]) < gs.HYPOTHESES, what
    assert torch.equal(r.inliers[p, :k].cpu().bool(), gt) and int(r.num_inliers[p]) == int(gt.sum()), what
    assert not bool(r.inliers[p, k:].any()) and r.inliers.shape[1] == count_rows, what
    assert abs(float((f * f).sum()) - 1.0) < 1e-6 and float(f.flatten()[f.abs().argmax()]) > 0, what
    e = gs.errors_px(f, k, alt)
    refit = gs.errors_px(fundamental_refit(k0[gt], k1[gt]), k, alt)
    diff = float((e - refit).abs().max())
    print(f"{what}: inliers <= {float(e[gt].max()):.3f} px, outliers >= {float(e[~gt].min()):.2f} px, "
          f"against fundamental_refit {diff:.3e} px (bound {REFIT_BOUND_PX})")
    assert float(e[gt].max()) < 1.5 and float(e[~gt].min()) > 6.0 and diff < REFIT_BOUND_PX, what


def test_ragged_batch_end_to_end(dev):
    m, counts, kp0, kp1 = gs.batch(((24, 0), (24, 7), (64, 64), (200, 200)), 200)
    r = verify(dev, m, counts, kp0, kp1)
    assert r.F.shape == (4, 3, 3) and r.F.dtype == torch.float32 and r.inliers.shape == (4, 200) and r.inliers.dtype == torch.uint8
    assert r.valid.tolist() == [0, 0, 1, 1] and r.best.tolist()[:2] == [-1, -1] and r.num_inliers.tolist()[:2] == [0, 0]
    assert not bool(r.F[:2].any()) and not bool(r.inliers[:2].any())
    check_pair(r, 2, 64, 200, "ragged, k 64")
    check_pair(r, 3, 200, 200, "ragged, k 200")


def test_small_scene_and_untrusted_counts(dev):
    """k = 24 alone; a count beyond Kmax is clamped, a negative one is 0."""
    m, counts, kp0, kp1 = gs.batch(((24, 24), (24, 24), (24, 24)), 24)
    counts[1], counts[2] = 100000, -5
    r = verify(dev, m, counts, kp0, kp1)
    assert r.valid.tolist() == [1, 1, 0] and int(r.best[2]) == -1 and not bool(r.inliers[2].any())
    check_pair(r, 0, 24, 24, "k 24")
    assert same_bits(r.F[0], r.F[1]) and same_bits(r.inliers[0], r.inliers[1])


def test_full_width(dev):
    m, counts, kp0, kp1 = gs.batch(((2048, 2048),), 2048)
    check_pair(verify(dev, m, counts, kp0, kp1), 0, 2048, 2048, "full width")


def test_outputs_stay_inside_their_tensors(dev):
    """The call through raw pointers into guarded outputs: every entry written, nothing outside."""
    from lightglue_amd import _lib
    from lightglue_amd._host import call

    m, counts, kp0, kp1 = gs.batch(((24, 7), (64, 64)), 70)
    keep, args = pair_ptrs(dev, m, counts, kp0, kp1)
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((2, 3, 3), torch.float32), ((2, 70), torch.uint8), ((2,), torch.int32), ((2,), torch.int32), ((2,), torch.int32))]
    n = _lib.load().lg_ransac_workspace(2, 70, gs.HYPOTHESES)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    call("lg_ransac_fundamental", *args, gs.THRESHOLD, gs.HYPOTHESES, gs.REFITS, gs.SEED, ws.data_ptr(), n,
         *(o.ptr for o in outs), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    f, inl, num, valid, best = (o.check(f"output {i}") for i, o in enumerate(outs))
    assert valid.tolist() == [0, 1] and best[0] == -1 and num[0] == 0 and not bool(f[0].any()) and not bool(inl[0].any())
    assert int(inl.max()) == 1 and int(num[1]) == int(inl[1].sum()) == 48


def test_pairs_are_independent_and_calls_deterministic(dev):
    from lightglue_amd import GeometryResult

    specs = ((24, 0), (24, 7), (64, 64), (200, 200), (24, 24))
    m, counts, kp0, kp1 = gs.batch(specs, 200)
    r = verify(dev, m, counts, kp0, kp1)
    equal_results(r, verify(dev, m, counts, kp0, kp1), "two calls")
    for p in range(len(specs)):
        one = verify(dev, m[p:p + 1], counts[p:p + 1], kp0[p:p + 1], kp1[p:p + 1])
        equal_results(GeometryResult(*(t[p:p + 1] for t in r)), one, f"pair {p} alone")


def test_capture_and_replay_on_new_matches(dev):
    from lightglue_amd import GeometryResult

    specs = ((24, 24), (64, 64), (200, 200))
    a = gs.batch(specs, 200)
    b = gs.batch(specs, 200, alt=True)
    live = [t.to(dev).clone() for t in a]
    fr = ransac()
    graph, captured = capture_on_side_stream(lambda: fr.verify(as_result(live[0], live[1]), live[2], live[3]))
    graph.replay()
    torch.cuda.synchronize()
    first = GeometryResult(*(t.clone() for t in captured))
    equal_results(first, verify(dev, *a), "replay, the captured scene")
    for dst, src in zip(live, b):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    equal_results(captured, verify(dev, *b), "replay, another scene")
    assert not same_bits(captured.F, first.F)
    for p, (k, _) in enumerate(specs):
        check_pair(captured, p, k, 200, f"replayed, k {k}", alt=True)


# ---- verify_source_images -------------------------------------------------------------------------------------------
def test_verify_source_images_is_its_parts(dev):
    """Seeded weights and two small image pairs (the sizes tests/test_gpu_image_input.py uses)."""
    from lightglue_amd import (FundamentalRansac, ImageInput, KeypointFrontend, SuperPointEncoder, match_source_images,
                               seeded_superpoint_state_dict, verify_source_images)

    def rand_u8(seed, *shape):
        return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)

    encoder, model = SuperPointEncoder(seeded_superpoint_state_dict(3)), seeded_matcher(dev)
    fe, ii, fr = KeypointFrontend(max_keypoints=64), ImageInput((40, 72)), FundamentalRansac(hypotheses=128)
    s0 = [rand_u8(100, 50, 70, 3).to(dev), rand_u8(101, 96, 64).to(dev)]
    s1 = [rand_u8(110, 61, 83).to(dev), rand_u8(111, 40, 120, 3).to(dev)]
    with torch.no_grad():
        result, kp0, kp1, geo = verify_source_images(ii, encoder, fe, model, fr, s0, s1)
        want, w0, w1 = match_source_images(ii, encoder, fe, model, s0, s1)
        torch.cuda.synchronize()
        equal_results(result, want, "the matches")
        assert same_bits(kp0, w0) and same_bits(kp1, w1)
        equal_results(geo, fr.verify(want, w0, w1), "the verification")
    assert geo.F.shape == (2, 3, 3) and geo.inliers.shape == (2, result.matches.shape[1])
    counts = result.counts.cpu()
    for p in range(2):  # whatever the seeded weights match: the outputs are consistent with themselves
        assert int(geo.num_inliers[p]) == int(geo.inliers[p].sum()) <= max(int(counts[p]), 0)
        assert int(geo.valid[p]) == (1 if int(geo.best[p]) >= 0 else 0)
