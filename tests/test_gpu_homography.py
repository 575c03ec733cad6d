"""The homography's RANSAC on the MI355X (csrc/lightglue_geometry.hip, the HomographyModel instantiations) against
the float64 contract in lightglue_amd/geometry_contract.py: the 4-samples bitwise, the 4-point solve per hypothesis, the
scoring counts exactly, the whole call on ragged batches, small scenes, a rotation-only scene and at full width,
guarded outputs, independence of the batch, determinism, capture and replay, and verify_source_images with a
HomographyRansac against its parts. The scenes and their preconditions are in homography_scenes.py and
test_homography.py. Nothing here reads the reference tree.

The two bounds are four times a worst that was measured on the CPU, not on a GPU: no GPU figure of these kernels
is recorded (profiles/geometry/INDEX.md, "Open"). Both worsts are the fp32 rounding of the output, which is what
the F bounds measured on the GPU came to as well:
    lg_ransac_solve4: the worst sample-point transfer error under a kept candidate, the same statements on the CPU
        (tools/homography_host_check.py), 4.966e-3 px -> SOLVE_BOUND_PX = 1.99e-2 (a kept hypothesis is one whose
        float64 candidate, rounded to fp32, keeps its sample points within FORMAT_LIMIT = 5e-3 px);
    the final H against homography_refit on the same mask, per point: 4.355e-5 px (the k = 200 alternate scene), from
        the same statements on the CPU and equally from rounding homography_refit itself to fp32 ->
        REFIT_BOUND_PX = 1.74e-4.
The tests print their figures before they assert.
"""
import pytest
import torch

import homography_scenes as hs
from gpu_common import GuardedOut, capture_on_side_stream, equal_results, same_bits, seeded_matcher

pytestmark = pytest.mark.gpu

SOLVE_BOUND_PX = 1.99e-2
REFIT_BOUND_PX = 1.74e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def ransac():
    from lightglue_amd import HomographyRansac

    return HomographyRansac(hs.THRESHOLD, hs.HYPOTHESES, hs.REFITS, hs.SEED)


def as_result(matches, counts):
    from lightglue_amd.matches import MatchResult

    return MatchResult(None, None, None, None, matches, None, counts)


def verify(dev, m, counts, kp0, kp1, hr=None):
    r = (hr or ransac()).verify(as_result(m.to(dev), counts.to(dev)), kp0.to(dev), kp1.to(dev))
    torch.cuda.synchronize()
    return r


def pair_ptrs(dev, m, counts, kp0, kp1):
    t = tuple(x.to(dev).contiguous() for x in (m, counts, kp0, kp1))
    return t, tuple(x.data_ptr() for x in t) + (m.shape[0], m.shape[1], kp0.shape[1], kp1.shape[1])


def stream():
    return torch.cuda.current_stream().cuda_stream


# ---- the samples ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hypotheses", (1, 65, 4096))
def test_samples4_are_bitwise_the_reference(dev, hypotheses):
    from lightglue_amd import ransac_samples
    from lightglue_amd._host import call

    for count in (4, 5, 7, 37, 2048):
        out = GuardedOut((hypotheses, 4), torch.int32, dev, fill=torch.full((hypotheses, 4), -1, dtype=torch.int32))
        call("lg_ransac_samples4", count, hypotheses, hs.SEED, out.ptr, stream())
        torch.cuda.synchronize()
        assert torch.equal(out.check(f"samples {count}"), ransac_samples(hs.SEED, hypotheses, count, size=4)), (count, hypotheses)


# ---- the 4-point solve ------------------------------------------------------------------------------------------
def test_solve4_against_the_reference_per_hypothesis(dev):
    """P = 2, H = 64 on the k = 64 scene. On every hypothesis the reference keeps (homography_scenes.solve_cases: at
    most a tenth is left out): the same number of candidates, 0 or 1, the GPU candidate the reference's up to sign
    (entries within 1e-5 at unit norm: fp32 rounding is 6e-8), and every sample point within SOLVE_BOUND_PX of its
    image under the GPU candidate."""
    from lightglue_amd import transfer_error
    from lightglue_amd._host import call

    samples, cases = hs.solve_cases()
    pairs, h, k = hs.solve_pairs(), hs.SOLVE_H, hs.SOLVE_K
    m = torch.arange(k, dtype=torch.int32)[None, :, None].repeat(2, 1, 2)
    keep, args = pair_ptrs(dev, m, torch.tensor([k, k], dtype=torch.int32), torch.stack([p[0] for p in pairs]),
                           torch.stack([p[1] for p in pairs]))
    smp = samples.to(dev)
    cand = GuardedOut((2, h, 9), torch.float32, dev)
    num = GuardedOut((2, h), torch.int32, dev, fill=torch.full((2, h), -1, dtype=torch.int32))
    call("lg_ransac_solve4", *args, smp.data_ptr(), h, cand.ptr, num.ptr, stream())
    torch.cuda.synchronize()
    cand, num = cand.check("candidates"), num.check("num")
    worst, worst_entry, kept, with_candidate = 0.0, 0.0, 0, 0
    for p, (x0, x1) in enumerate(pairs):
        for i, (s, ref, ok) in enumerate(cases[p]):
            n = int(num[p, i])
            assert n in (0, 1) and (n == 1 or not bool(cand[p, i].any())), (p, i)
            if not ok:
                continue
            kept += 1
            assert n == len(ref.candidates), (p, i, n, len(ref.candidates))
            if n == 0:
                continue
            with_candidate += 1
            got, want = cand[p, i].double(), torch.from_numpy(ref.candidates[0]).reshape(9)
            assert abs(float((got ** 2).sum()) - 1.0) < 1e-6 and float(got[got.abs().argmax()]) > 0, (p, i)
            entry = min(float((got - want).abs().max()), float((got + want).abs().max()))
            worst_entry = max(worst_entry, entry)
            assert entry < 1e-5, (p, i, got, want)
            worst = max(worst, float(transfer_error(got.reshape(3, 3), x0[s], x1[s]).sqrt().max()))
    print(f"solve4: {kept} of {2 * h} hypotheses kept, {with_candidate} with a candidate, worst sample-point transfer error "
          f"{worst:.3e} px (bound {SOLVE_BOUND_PX}), worst entry difference {worst_entry:.3e}")
    assert kept >= 2 * h - 2 * h // 10 and with_candidate >= kept // 2 and worst < SOLVE_BOUND_PX < 0.05


def test_solve4_small_pairs_and_bad_samples_give_nothing(dev):
    """count < 4: zeros. Samples out of range are clamped; a repeated index, a collinear triple and a twisted sample
    (one triple's orientation flipped between the images): no candidate. A plain sample: one."""
    from lightglue_amd._host import call

    kp0 = torch.tensor([[10.0, 10.0], [200.0, 20.0], [220.0, 180.0], [30.0, 200.0], [105.0, 15.0], [120.0, 60.0]])
    kp1 = kp0 * 1.1 + torch.tensor([5.0, -3.0])
    kp1[5] = torch.tensor([400.0, 300.0])  # point 5 of image 1 outside the quadrilateral 0 1 2 3: twisted with 0 1 2
    ident = torch.arange(6, dtype=torch.int32)[:, None].repeat(1, 2)
    m = torch.stack([ident, ident])
    keep, args = pair_ptrs(dev, m, torch.tensor([3, 6], dtype=torch.int32), torch.stack([kp0, kp0]), torch.stack([kp1, kp1]))
    smp = torch.tensor([[0, 1, 2, 3], [0, 1, 2, 2], [0, 1, 2, 99], [-4, 1, 2, 0], [0, 1, 4, 2], [0, 2, 3, 5], [3, 2, 1, 0]],
                       dtype=torch.int32).to(dev)
    h = smp.shape[0]
    cand = GuardedOut((2, h, 9), torch.float32, dev)
    num = GuardedOut((2, h), torch.int32, dev, fill=torch.full((2, h), -1, dtype=torch.int32))
    call("lg_ransac_solve4", *args, smp.data_ptr(), h, cand.ptr, num.ptr, stream())
    torch.cuda.synchronize()
    cand, num = cand.check("candidates"), num.check("num")
    assert num[0].tolist() == [0] * h and not bool(cand[0].any())
    # plain; repeated; 99 clamped to 5: (0 1 2 5) is twisted; -4 clamped to 0: repeated; 0 1 4 collinear; twisted; plain
    assert num[1].tolist() == [1, 0, 0, 0, 0, 0, 1], num[1].tolist()
    assert not bool(cand[1, 1:6].any()) and bool(cand[1, 0].any())
    want = torch.tensor([[1.1, 0, 5.0], [0, 1.1, -3.0], [0, 0, 1.0]], dtype=torch.float64)
    want = (want / want.norm()).reshape(9)
    for i in (0, 6):
        assert float((cand[1, i].double() - want).abs().max()) < 1e-6, cand[1, i]


# ---- the scoring ------------------------------------------------------------------------------------------------
def test_score_counts_are_exactly_the_float64_counts(dev):
    """Ragged counts 1, 3, 4, 5, 63, 64, 65, 300, 2048 in one launch, out-of-range match indices, NaN and Inf
    keypoints, a zero and a NaN candidate and one with W = 0 at a point; no float64 error within 0.02 px of the
    threshold (homography_scenes.score_inputs)."""
    from lightglue_amd._host import call

    m, counts, kp0, kp1, cands, want = hs.score_inputs()
    keep, args = pair_ptrs(dev, m, counts, kp0, kp1)
    c = cands.to(dev).contiguous()
    out = GuardedOut(tuple(want.shape), torch.int32, dev, fill=torch.full(tuple(want.shape), -1, dtype=torch.int32))
    call("lg_ransac_score_homography", *args, c.data_ptr(), c.shape[1], hs.THRESHOLD, out.ptr, stream())
    torch.cuda.synchronize()
    got = out.check("inlier counts")
    assert torch.equal(got, want), (got.tolist(), want.tolist())


# ---- the whole call ---------------------------------------------------------------------------------------------
WORST_REFIT = [0.0]


def check_pair(r, p, k, count_rows, what, alt=False, rotation=False):
    """Pair p of result r is the whole scene k: the mask is gt_mask, H separates as the contract's preconditions
    say and agrees with homography_refit on that mask."""
    from lightglue_amd import homography_refit

    k0, k1, gt, _ = hs.scene(k, alt, rotation)
    h = r.H[p].cpu().double()
    assert int(r.valid[p]) == 1 and 0 <= int(r.best[p]) < hs.HYPOTHESES, what
    assert torch.equal(r.inliers[p, :k].cpu().bool(), gt) and int(r.num_inliers[p]) == int(gt.sum()), what
    assert not bool(r.inliers[p, k:].any()) and r.inliers.shape[1] == count_rows, what
    assert abs(float((h * h).sum()) - 1.0) < 1e-6 and float(h.flatten()[h.abs().argmax()]) > 0, what
    e = hs.errors_px(h, k, alt, rotation)
    refit = hs.errors_px(homography_refit(k0[gt], k1[gt]), k, alt, rotation)
    diff = float((e - refit).abs().max())
    WORST_REFIT[0] = max(WORST_REFIT[0], diff)
    print(f"{what}: inliers <= {float(e[gt].max()):.3f} px, outliers >= {float(e[~gt].min()):.2f} px, "
          f"against homography_refit {diff:.3e} px (bound {REFIT_BOUND_PX}; worst so far {WORST_REFIT[0]:.3e})")
    assert float(e[gt].max()) < 1.5 and float(e[~gt].min()) > 6.0 and diff < REFIT_BOUND_PX, what


def test_ragged_batch_end_to_end(dev):
    m, counts, kp0, kp1 = hs.batch(((24, 0), (24, 3), (24, 4), (64, 64), (200, 200)), 200)
    r = verify(dev, m, counts, kp0, kp1)
    assert r.H.shape == (5, 3, 3) and r.H.dtype == torch.float32 and r.inliers.shape == (5, 200) and r.inliers.dtype == torch.uint8
    assert r.valid.tolist()[:2] == [0, 0] and r.valid.tolist()[3:] == [1, 1]
    assert r.best.tolist()[:2] == [-1, -1] and r.num_inliers.tolist()[:2] == [0, 0]
    assert not bool(r.H[:2].any()) and not bool(r.inliers[:2].any())
    # four correspondences: every sample is all of them; valid only if the four pass the solve and fit themselves
    want = hs_reference_of(m[2:3], counts[2:3], kp0[2:3], kp1[2:3])
    assert int(r.valid[2]) == int(want.valid[0]) and int(r.num_inliers[2]) == int(want.num_inliers[0])
    assert int(r.best[2]) == int(want.best[0]) and torch.equal(r.inliers[2].cpu(), want.inliers[0])
    assert int(r.valid[2]) == (1 if int(r.num_inliers[2]) == 4 else 0) and not bool(r.inliers[2, 4:].any())
    check_pair(r, 3, 64, 200, "ragged, k 64")
    check_pair(r, 4, 200, 200, "ragged, k 200")


def hs_reference_of(m, counts, kp0, kp1):
    from lightglue_amd import homography_reference

    return homography_reference(m, counts, kp0, kp1, hs.THRESHOLD, hs.HYPOTHESES, hs.REFITS, hs.SEED)


@pytest.mark.parametrize("k", (8, 24))
def test_small_scenes_and_untrusted_counts(dev, k):
    """k = 8 and k = 24 alone; a count beyond Kmax is clamped, a negative one is 0."""
    m, counts, kp0, kp1 = hs.batch(((k, k), (k, k), (k, k)), k)
    counts[1], counts[2] = 100000, -5
    r = verify(dev, m, counts, kp0, kp1)
    assert r.valid.tolist() == [1, 1, 0] and int(r.best[2]) == -1 and not bool(r.inliers[2].any()) and not bool(r.H[2].any())
    check_pair(r, 0, k, k, f"k {k}")
    assert same_bits(r.H[0], r.H[1]) and same_bits(r.inliers[0], r.inliers[1])


def test_full_width(dev):
    m, counts, kp0, kp1 = hs.batch(((2048, 2048),), 2048)
    check_pair(verify(dev, m, counts, kp0, kp1), 0, 2048, 2048, "full width")


def test_rotation_only_scene(dev):
    k = hs.ROTATION_K
    m, counts, kp0, kp1 = hs.batch(((k, k),), k, rotation=True)
    check_pair(verify(dev, m, counts, kp0, kp1), 0, k, k, "rotation only", rotation=True)


def test_outputs_stay_inside_their_tensors(dev):
    """The call through raw pointers into guarded outputs: every entry written, nothing outside."""
    from lightglue_amd import _lib
    from lightglue_amd._host import call

    m, counts, kp0, kp1 = hs.batch(((24, 3), (64, 64)), 70)
    keep, args = pair_ptrs(dev, m, counts, kp0, kp1)
    outs = [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in
            (((2, 3, 3), torch.float32), ((2, 70), torch.uint8), ((2,), torch.int32), ((2,), torch.int32), ((2,), torch.int32))]
    n = _lib.load().lg_ransac_workspace(2, 70, hs.HYPOTHESES)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    call("lg_ransac_homography", *args, hs.THRESHOLD, hs.HYPOTHESES, hs.REFITS, hs.SEED, ws.data_ptr(), n,
         *(o.ptr for o in outs), stream())
    torch.cuda.synchronize()
    h, inl, num, valid, best = (o.check(f"output {i}") for i, o in enumerate(outs))
    assert valid.tolist() == [0, 1] and best[0] == -1 and num[0] == 0 and not bool(h[0].any()) and not bool(inl[0].any())
    assert int(inl.max()) == 1 and int(num[1]) == int(inl[1].sum()) == 48


def test_pairs_are_independent_and_calls_deterministic(dev):
    from lightglue_amd import HomographyResult

    specs = ((24, 0), (24, 3), (24, 4), (64, 64), (200, 200), (24, 24), (8, 8))
    m, counts, kp0, kp1 = hs.batch(specs, 200)
    r = verify(dev, m, counts, kp0, kp1)
    equal_results(r, verify(dev, m, counts, kp0, kp1), "two calls")
    for p in range(len(specs)):
        one = verify(dev, m[p:p + 1], counts[p:p + 1], kp0[p:p + 1], kp1[p:p + 1])
        equal_results(HomographyResult(*(t[p:p + 1] for t in r)), one, f"pair {p} alone")


def test_capture_and_replay_on_new_matches(dev):
    from lightglue_amd import HomographyResult

    specs = ((8, 8), (24, 24), (64, 64), (200, 200))
    a = hs.batch(specs, 200)
    b = hs.batch(specs, 200, alt=True)
    live = [t.to(dev).clone() for t in a]
    hr = ransac()
    graph, captured = capture_on_side_stream(lambda: hr.verify(as_result(live[0], live[1]), live[2], live[3]))
    graph.replay()
    torch.cuda.synchronize()
    first = HomographyResult(*(t.clone() for t in captured))
    equal_results(first, verify(dev, *a), "replay, the captured scene")
    for dst, src in zip(live, b):
        dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    equal_results(captured, verify(dev, *b), "replay, another scene")
    assert not same_bits(captured.H, first.H)
    for p, (k, _) in enumerate(specs):
        check_pair(captured, p, k, 200, f"replayed, k {k}", alt=True)


# ---- verify_source_images -------------------------------------------------------------------------------------------
def test_verify_source_images_with_a_homography_is_its_parts(dev):
    """Seeded weights and two small image pairs (the sizes tests/test_gpu_image_input.py uses)."""
    from lightglue_amd import (HomographyRansac, HomographyResult, ImageInput, KeypointFrontend, SuperPointEncoder,
                               match_source_images, seeded_superpoint_state_dict, verify_source_images)

    def rand_u8(seed, *shape):
        return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)

    encoder, model = SuperPointEncoder(seeded_superpoint_state_dict(3)), seeded_matcher(dev)
    fe, ii, hr = KeypointFrontend(max_keypoints=64), ImageInput((40, 72)), HomographyRansac(hypotheses=128)
    s0 = [rand_u8(100, 50, 70, 3).to(dev), rand_u8(101, 96, 64).to(dev)]
    s1 = [rand_u8(110, 61, 83).to(dev), rand_u8(111, 40, 120, 3).to(dev)]
    with torch.no_grad():
        result, kp0, kp1, geo = verify_source_images(ii, encoder, fe, model, hr, s0, s1)
        want, w0, w1 = match_source_images(ii, encoder, fe, model, s0, s1)
        torch.cuda.synchronize()
        equal_results(result, want, "the matches")
        assert same_bits(kp0, w0) and same_bits(kp1, w1)
        equal_results(geo, hr.verify(want, w0, w1), "the verification")
    assert isinstance(geo, HomographyResult) and geo.H.shape == (2, 3, 3) and geo.inliers.shape == (2, result.matches.shape[1])
    counts = result.counts.cpu()
    for p in range(2):  # whatever the seeded weights match: the outputs are consistent with themselves
        assert int(geo.num_inliers[p]) == int(geo.inliers[p].sum()) <= max(int(counts[p]), 0)
        assert int(geo.valid[p]) == (1 if int(geo.best[p]) >= 0 else 0)
        assert bool(geo.H[p].any()) == bool(geo.valid[p])
