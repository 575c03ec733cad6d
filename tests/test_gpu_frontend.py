"""Keypoint front end on the MI355X: each stage against the reference's golden output on that stage's own
golden input (tests/golden/frontend_*.npz, make_frontend_golden.py), then extract end to end, extract +
match_features against match_batch with host counts, and one captured extract + match replayed on new logits.
Nothing here reads the reference tree."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR
from gpu_common import capture_on_side_stream, equal_results, same_bits, seeded_matcher

pytestmark = pytest.mark.gpu

NAMES = ("8x8", "9x17", "11x10")
THR = 0.0005


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


_cache = {}


def load(name):
    if name not in _cache:
        with np.load(os.path.join(GOLDEN_DIR, f"frontend_{name}.npz"), allow_pickle=False) as z:
            _cache[name] = {k: z[k] for k in z.files}
    return _cache[name]


@pytest.fixture(scope="module", params=NAMES)
def g(request):
    return load(request.param)


def t(a, dev=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.to(dev) if dev is not None else x


# ---- heatmap ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_heatmap(g, dev, dtype):
    """Against an fp64 softmax of the logits the kernel reads. The reference's own fp32 result is within
    heat_err of fp64 on these fixtures (3.9e-8 at 8x8, 7.9e-8 at 9x17, 5.6e-8 at 11x10: about one ulp of the
    largest scores, ~0.5); the kernel, with another exponential and sum order, may have 4 x that."""
    from lightglue_amd import frontend

    logits = t(g["logits"]).to(dtype)
    exact = frontend.heatmap_reference(logits.double())
    got = frontend.heatmap(logits.to(dev))
    assert got.dtype == torch.float32 and got.shape == exact.shape
    err = float((got.cpu().double() - exact).abs().max())
    print(f"heatmap {dtype}: max abs error {err:.3e}, bound {4 * float(g['heat_err']):.3e}")
    assert err <= 4 * float(g["heat_err"])


# ---- NMS ----------------------------------------------------------------------------------------------
def nms_cases(g):
    heat = t(g["heat32"])
    for r in (0, 1, 4):
        yield f"heat r{r}", heat, r, (heat if r == 0 else t(g[f"nms_r{r}"]))
        for lv in (32, 64):  # plateaus and suppression chains
            yield f"q{lv} r{r}", t(g[f"q{lv}_levels"]).float() / lv, r, t(g[f"q{lv}_nms_r{r}"])
        yield f"special r{r}", t(g["special"]), r, t(g[f"special_nms_r{r}"])  # constant, edge maxima, edge plateaus


def test_nms_is_bitwise_the_reference(g, dev):
    from lightglue_amd import frontend

    for tag, x, r, want in nms_cases(g):
        got = frontend.nms(x.to(dev), r).cpu()
        assert same_bits(got, want), (tag, int((got != want).sum()))


def test_nms_odd_sizes(dev):
    """Sizes that are no multiple of 8 or of the tile, down to one pixel and one row (the entry point takes
    any h, w >= 1), against the framework restatement, which the CPU tests pin to the reference."""
    from lightglue_amd import frontend

    gen = torch.Generator().manual_seed(5)
    for h, w in ((1, 1), (1, 50), (33, 31), (65, 97)):
        x = torch.floor(torch.rand((3, h, w), generator=gen) * 16) / 16
        for r in (0, 2, 3, 4):
            assert same_bits(frontend.nms(x.to(dev), r).cpu(), frontend.nms_reference(x, r)), (h, w, r)


# ---- select -------------------------------------------------------------------------------------------
def test_select_matches_the_reference_exactly(g, dev):
    """Distinct scores (the generator asserts it): pix, score and count are the reference's topk order.
    Cases: border 0 and 4, K between the images' counts, K = 8, K = 2048 with few candidates, and (8x8) an
    image with no candidate at all."""
    from lightglue_amd import frontend

    nms4 = t(g["nms_r4"], dev)
    k = int(g["k_main"])
    for border, kk in ((4, k), (0, k), (4, 8), (4, 2048)):
        count, pix, score = frontend.select(nms4, kk, THR, border)
        tag = f"sel_b{border}_k{kk}"
        assert torch.equal(count.cpu(), t(g[tag + "_count"])), tag
        assert torch.equal(pix.cpu(), t(g[tag + "_pix"])), tag
        assert same_bits(score.cpu(), t(g[tag + "_score"])), tag
    if bool(g["has_empty_image"]):
        count, pix, score = frontend.select(nms4, 64, THR, 4)
        assert int(count[1]) == 0 and bool((pix[1] == -1).all()) and bool((score[1] == 0).all())


def test_select_tie_rule_and_determinism(g, dev):
    """Equal scores across the K cut (the quantised NMS map), and far more candidates than K with long runs of
    equal scores (the quantised map itself, threshold 0, border 0: every positive pixel): exactly
    frontend_reference's rule, and two runs bitwise equal."""
    from lightglue_amd import frontend

    q = t(g["q64_nms_r4"])
    raw = t(g["q64_levels"]).float() / 64
    for x, k, thr, border in ((q, int(g["tie_k"]), THR, 4), (raw, 2048, 0.0, 0), (raw, 8, 0.0, 1), (raw, 1024, 0.5, 4)):
        want = frontend.select_reference(x, k, thr, border)
        got = frontend.select(x.to(dev), k, thr, border)
        again = frontend.select(x.to(dev), k, thr, border)
        for a, b, c in zip(got, want, again):
            assert same_bits(a.cpu(), b), (k, thr, border)
            assert same_bits(a, c), (k, thr, border)


# ---- describe -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("normalized", [False, True])
def test_describe(g, dev, layout, normalized):
    """Against the fp64 restatement on the tensor the kernel reads. The reference's fp32 descriptors are
    within desc_err of it (1.3e-7 .. 2.7e-7 on these fixtures); the fp32 output may have 4 x that, the fp16
    output that plus 2^-12 (half an fp16 ulp for components of magnitude <= 1). border 0 puts corners
    outside the map (zero padding); padded rows are exactly zero; kpts_px and kpts are exact."""
    from lightglue_amd import frontend

    dense = t(g["dense"]).float()
    if normalized:
        dense = F.normalize(dense, p=2, dim=1)
    k = int(g["k_main"])
    h, w = g["heat32"].shape[1:]
    for bi, border in enumerate((0, 4)):
        count, pix = t(g[f"sel_b{border}_k{k}_count"]), t(g[f"sel_b{border}_k{k}_pix"])
        exact, px_want, kn_want = frontend.describe_reference(dense.double(), count, pix, normalized, compute=torch.float64)
        kn32 = frontend.describe_reference(dense, count, pix, normalized)[2]
        d = dense.to(dev)
        if layout == "channels_last":
            d = d.contiguous(memory_format=torch.channels_last)
            assert d.stride(1) == 1
        valid = torch.arange(k)[None, :] < count[:, None]
        bound = 4 * float(g["desc_err"][bi, int(normalized)])
        for dtype, extra in ((torch.float32, 0.0), (torch.float16, 2.0 ** -12)):
            desc, kpx, kpts = frontend.describe(d, count.to(dev), pix.to(dev), normalized, dtype)
            assert desc.dtype == dtype and kpts.dtype == dtype and kpx.dtype == torch.int32
            err = float((desc.cpu().double() - exact).abs().max())
            print(f"describe {layout} normalized={normalized} border={border} {dtype}: {err:.3e}, bound {bound + extra:.3e}")
            assert err <= bound + extra
            assert bool((desc.cpu()[~valid] == 0).all()) and bool((kpts.cpu()[~valid] == 0).all())
            assert torch.equal(kpx.cpu(), px_want)
            assert same_bits(kpts.cpu(), kn32.to(dtype))
    # fp16 dense input: the fixture's values are fp16-exact, so the raw path reads the same numbers
    if not normalized:
        a = frontend.describe(d.half(), count.to(dev), pix.to(dev), False, torch.float32)[0]
        b = frontend.describe(d, count.to(dev), pix.to(dev), False, torch.float32)[0]
        assert same_bits(a, b)


# ---- end to end ---------------------------------------------------------------------------------------
def test_extract_end_to_end(g, dev):
    """extract from logits: the keypoint set of each image, keyed by pixel, is the golden one (the fixture's
    gaps are >= 64 x the heatmap error, so the reference alone decides the set; order is select's test), with
    descriptors within the describe bound of the fp64 restatement at those pixels. from_scores on the golden
    heatmap reproduces the golden order exactly."""
    from lightglue_amd import KeypointFrontend, frontend

    k = int(g["k_main"])
    w = g["heat32"].shape[2]
    fe = KeypointFrontend(max_keypoints=k, dtype=torch.float32)
    dense = t(g["dense"], dev)
    f = fe.extract(t(g["logits"], dev), dense)
    want_count, want_pix = t(g[f"sel_b4_k{k}_count"]), t(g[f"sel_b4_k{k}_pix"])
    assert torch.equal(f.counts.cpu(), want_count)
    pix = (f.kpts_px[..., 1] * w + f.kpts_px[..., 0]).cpu()
    for i in range(2):
        n = int(want_count[i])
        assert set(pix[i, :n].tolist()) == set(want_pix[i, :n].tolist()) and len(set(pix[i, :n].tolist())) == n
        assert bool((f.scores[i, :max(n - 1, 0)] >= f.scores[i, 1:max(n, 1)]).all()) and bool((f.scores[i, n:] == 0).all())
    mine = torch.where(torch.arange(k)[None, :] < want_count[:, None], pix, -1).int()
    exact = frontend.describe_reference(t(g["dense"]).double(), want_count, mine, False, compute=torch.float64)
    assert float((f.desc.cpu().double() - exact[0]).abs().max()) <= 4 * float(g["desc_err"][1, 0])
    assert same_bits(f.kpts.cpu(), frontend.describe_reference(t(g["dense"]).float(), want_count, mine)[2])
    s = fe.from_scores(t(g["heat32"], dev), dense)
    assert torch.equal((s.kpts_px[..., 1] * w + s.kpts_px[..., 0]).cpu(), want_pix.clamp_min(0))
    assert same_bits(s.scores.cpu(), t(g[f"sel_b4_k{k}_score"]))
    n = fe.from_scores(t(g["nms_r4"], dev), dense.half(), nms_done=True)
    assert torch.equal(n.kpts_px, s.kpts_px) and torch.equal(n.counts, s.counts)


@pytest.fixture(scope="module")
def model(dev):
    return seeded_matcher(dev, n_layers=9)


def pair_inputs(dev, variant=0):
    """Three pairs from the 8x8 fixture, whose image 1 has no keypoint: a full pair, one with no keypoint in
    image 0, one with none in image 1."""
    g8 = load("8x8")
    lg, dn = t(g8["logits"], dev), t(g8["dense"], dev)
    moved = torch.roll(lg, 1 + variant, dims=3)
    la = torch.stack([lg[0], lg[1], lg[0]]) if variant == 0 else torch.stack([moved[0], lg[1], lg[0]])
    lb = torch.stack([moved[0], moved[0], lg[1]])
    da = torch.stack([dn[0], dn[1], dn[0]])
    db = torch.stack([dn[1], dn[0], dn[1]])
    return la.contiguous(), lb.contiguous(), da.contiguous(), db.contiguous()


def expected_match(model, f0, f1):
    """match_batch with host counts (a zero count clamped to 1, as the kernels do), the pairs with a zero
    count masked."""
    c0, c1 = f0.counts.tolist(), f1.counts.tolist()
    r = model.match_batch(f0.kpts, f1.kpts, f0.desc, f1.desc, counts0=[max(c, 1) for c in c0], counts1=[max(c, 1) for c in c1])
    out = [x.clone() for x in r]
    for p, (a, b) in enumerate(zip(c0, c1)):
        if a == 0 or b == 0:
            for x, fill in zip(out, (-1, -1, 0, 0, -1, 0, 0)):
                x[p] = fill
    return type(r)(*out), c0, c1


def test_match_features_equals_match_batch_with_host_counts(model, dev):
    from lightglue_amd import KeypointFrontend

    fe = KeypointFrontend(max_keypoints=40)
    la, lb, da, db = pair_inputs(dev)
    with torch.no_grad():
        f0, f1 = fe.extract(la, da), fe.extract(lb, db)
        got = model.match_features(f0, f1)
        want, c0, c1 = expected_match(model, f0, f1)
    assert c0 == [40, 0, 40] and c1[1] == 40 and c1[2] == 0 and c1[0] > 0
    equal_results(got, want, "match_features")
    assert int(got.counts[0]) > 0 and got.counts[1:].tolist() == [0, 0]
    assert bool((got.matches0[1:] == -1).all()) and bool((got.scores1[1:] == 0).all())


def test_captured_extract_and_match_replays_on_new_logits(model, dev):
    """One capture of extract + extract + match_features on a single stream; new logits written in place; the
    replay equals the eager result for them (no count ever reaches the host)."""
    from lightglue_amd import KeypointFrontend

    fe = KeypointFrontend(max_keypoints=40)
    la, lb, da, db = pair_inputs(dev)
    la2 = pair_inputs(dev, variant=1)[0]

    def run():
        f0, f1 = fe.extract(la, da), fe.extract(lb, db)
        return f0, f1, model.match_features(f0, f1)

    graph, (c0, c1, captured) = capture_on_side_stream(run, on_side=False)
    with torch.no_grad():
        graph.replay()
        torch.cuda.synchronize()
        e0, e1, eager = run()
        equal_results(captured, eager, "replay, the captured logits")
        assert torch.equal(c0.kpts_px, e0.kpts_px) and same_bits(c1.desc, e1.desc)
        la.copy_(la2)
        graph.replay()
        torch.cuda.synchronize()
        e0, e1, eager = run()
    assert not torch.equal(e0.kpts_px[0], torch.zeros_like(e0.kpts_px[0]))
    equal_results(captured, eager, "replay, new logits")
    assert torch.equal(c0.kpts_px, e0.kpts_px) and same_bits(c0.desc, e0.desc) and torch.equal(c0.counts, e0.counts)
