"""The SuperPoint encoder on the MI355X: every lg_sp_* kernel against exact (float64, CPU) arithmetic on the same
fp16 inputs under a derived bound, the whole encoder against the float64 forward within twice the fp16-storage
model's own error, then the plumbing (extract, match_images), one capture replayed on a new image pair, and
repeatability. Nothing here reads the reference tree; every reference is computed by this file on the CPU.

The per-layer bound, for out = fp16(relu(sum + bias)) with the sum of K products accumulated in fp32:
    |out - ref| <= 2^-10 |ref| + 2 K 2^-24 S + 2^-24,   S = conv(|input|, |weight|) + |bias|  (float64)
one fp16 rounding (2^-11 relative, factor 2), the worst-case error of an fp32 sum of K terms in any order (factor
2), and the rounding of an fp16 subnormal. A 2 x 2 maximum keeps it with S pooled the same way (ref >= 0 there).
The kernel's tile is 8 x 16 pixels: 9 x 17 is one pixel over it in each direction, 18 x 34 spans 3 x 3 ragged
tiles, and the heads' 64-pixel blocks straddle the images of a batch at every size but 8 x 8.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_common import capture_on_side_stream, equal_results, same_bits, seeded_matcher

pytestmark = pytest.mark.gpu

SIZES = ((1, 1), (3, 5), (8, 8), (9, 17), (18, 34))
POOL_SIZES = ((2, 2), (4, 6), (8, 8), (10, 18), (18, 34))
CHANNELS = ((64, 64), (64, 128), (128, 128), (128, 512))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def normal16(seed, shape, std=1.0):
    """fp16 values from synth's generator (what the kernel sees), as a CPU fp16 tensor."""
    from lightglue_amd import synth

    return torch.from_numpy(synth.normal(seed, shape, std)).half()


def batch_scales(b):
    """Batch 3: image 1 is large-valued, images 0 and 2 small, so a patch that picks up a neighbour's rows
    breaks the bound instead of hiding in noise."""
    return torch.tensor([1.0] if b == 1 else [1.0 / 16, 4.0, 1.0 / 16])[:b]


def check_bound(out, ref, s, k, what):
    out, ref, s = out.double(), ref.double(), s.double()
    bound = 2.0 ** -10 * ref.abs() + 2.0 * k * 2.0 ** -24 * s + 2.0 ** -24
    err = (out - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: max err {float(err.max()):.3e}, max err / bound {worst:.3f}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, (what, worst, float(err.max()))


# ---- lg_sp_conv3x3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_conv3x3_against_exact_arithmetic(dev, cin, cout, batch):
    from lightglue_amd import superpoint as sp

    seed = 1000 + cin + cout + batch
    w = normal16(seed, (cout, cin, 3, 3), float(np.sqrt(2.0 / (9 * cin))))
    bias = normal16(seed + 1, (cout,), 0.1)
    wp, bg = sp.pack_conv(w).to(dev), bias.to(dev)
    for n, (h, wd) in enumerate(sorted(set(SIZES + POOL_SIZES))):
        x = normal16(seed + 10 + n, (batch, h, wd, cin)) * batch_scales(batch).half()[:, None, None, None]
        xn = x.double().permute(0, 3, 1, 2)
        lin = F.conv2d(xn, w.double(), bias.double(), padding=1)
        s = F.conv2d(xn.abs(), w.double().abs(), bias.double().abs(), padding=1)
        xg = x.to(dev)
        if (h, wd) in SIZES:
            for relu in (True, False):
                got = sp.conv3x3(xg, wp, bg, relu=relu, pool=False)
                assert got.shape == (batch, h, wd, cout) and got.dtype == torch.float16 and got.is_contiguous()
                ref = F.relu(lin) if relu else lin
                check_bound(got.cpu().permute(0, 3, 1, 2), ref, s, 9 * cin, f"conv3x3 {cin}->{cout} {h}x{wd} b{batch} relu={relu}")
        if (h, wd) in POOL_SIZES:
            got = sp.conv3x3(xg, wp, bg, relu=True, pool=True)
            assert got.shape == (batch, h // 2, wd // 2, cout) and got.is_contiguous()
            check_bound(got.cpu().permute(0, 3, 1, 2), F.max_pool2d(F.relu(lin), 2, 2), F.max_pool2d(s, 2, 2), 9 * cin,
                        f"conv3x3+pool {cin}->{cout} {h}x{wd} b{batch}")


def test_conv3x3_other_widths_and_output_buffer(dev):
    """cout 256 and 512 from 64 channels (the other instantiations), into a caller's buffer."""
    from lightglue_amd import superpoint as sp

    for cin, cout in ((64, 256), (64, 512), (128, 256)):
        w = normal16(77 + cout, (cout, cin, 3, 3), float(np.sqrt(2.0 / (9 * cin))))
        bias = normal16(78 + cout, (cout,), 0.1)
        x = normal16(79 + cout, (2, 9, 17, cin))
        out = torch.full((2, 9, 17, cout), 7.0, dtype=torch.float16, device=dev)
        got = sp.conv3x3(x.to(dev), sp.pack_conv(w).to(dev), bias.to(dev), relu=True, out=out)
        assert got.data_ptr() == out.data_ptr()
        xn = x.double().permute(0, 3, 1, 2)
        check_bound(got.cpu().permute(0, 3, 1, 2), F.relu(F.conv2d(xn, w.double(), bias.double(), padding=1)),
                    F.conv2d(xn.abs(), w.double().abs(), bias.double().abs(), padding=1), 9 * cin, f"conv3x3 {cin}->{cout}")


# ---- lg_sp_conv1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (1, 3))
@pytest.mark.parametrize("dtype", (torch.float16, torch.float32))
def test_conv1_against_exact_arithmetic(dev, dtype, batch):
    from lightglue_amd import superpoint as sp, synth

    w = normal16(31, (64, 1, 3, 3), float(np.sqrt(2.0 / 9)))
    bias = normal16(32, (64,), 0.1)
    for n, (h, wd) in enumerate(SIZES):
        img = torch.from_numpy(synth.normal(40 + n, (batch, h, wd))) * batch_scales(batch)[:, None, None]
        img = img.to(dtype)
        xn = img.double()[:, None]
        lin = F.conv2d(xn, w.double(), bias.double(), padding=1)
        s = F.conv2d(xn.abs(), w.double().abs(), bias.double().abs(), padding=1)
        for relu in (True, False):
            got = sp.conv1(img.to(dev), w.to(dev), bias.to(dev), relu=relu)
            assert got.shape == (batch, h, wd, 64) and got.dtype == torch.float16
            check_bound(got.cpu().permute(0, 3, 1, 2), F.relu(lin) if relu else lin, s, 9, f"conv1 {dtype} {h}x{wd} b{batch} relu={relu}")


# ---- lg_sp_heads --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", (1, 3))
def test_heads_against_exact_arithmetic_and_layouts(dev, batch):
    from lightglue_amd import superpoint as sp

    wpb, bpb = normal16(51, (65, 256, 1, 1), float(np.sqrt(2.0 / 256))), normal16(52, (65,), 0.1)
    wdb, bdb = normal16(53, (256, 256, 1, 1), float(np.sqrt(2.0 / 256))), normal16(54, (256,), 0.1)
    wp, bs = sp.pack_heads(wpb, bpb, wdb, bdb)
    wp, bs = wp.to(dev), bs.to(dev)
    for n, (hc, wc) in enumerate(SIZES):
        x = normal16(60 + n, (batch, hc, wc, 512)) * batch_scales(batch).half()[:, None, None, None]
        logits, dense = sp.heads(x.to(dev), wp, bs)
        assert logits.shape == (batch, 65, hc, wc) and logits.dtype == torch.float16 and logits.is_contiguous()
        assert same_bits(logits, logits.contiguous()) and logits.contiguous().data_ptr() == logits.data_ptr()
        assert dense.shape == (batch, 256, hc, wc) and dense.dtype == torch.float16
        assert dense.stride() == (hc * wc * 256, 1, wc * 256, 256)  # channels-last: the layout describe reads in place
        xn = x.double().permute(0, 3, 1, 2)
        for got, cols, wt, b, what in ((logits, slice(0, 256), wpb, bpb, "logits"), (dense, slice(256, 512), wdb, bdb, "dense")):
            ref = F.conv2d(xn[:, cols], wt.double(), b.double())
            s = F.conv2d(xn[:, cols].abs(), wt.double().abs(), b.double().abs())
            back = torch.empty(got.shape, dtype=torch.float16)
            back.copy_(got)  # read through the strides
            check_bound(back, ref, s, 256, f"heads {what} {hc}x{wc} b{batch}")


# ---- the whole encoder --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    from lightglue_amd import seeded_superpoint_state_dict

    return seeded_superpoint_state_dict(3)


@pytest.fixture(scope="module")
def encoder(sd):
    from lightglue_amd import SuperPointEncoder

    return SuperPointEncoder(sd)


def images(seed, b, h, w, dtype=torch.float32):
    from lightglue_amd import synth

    return torch.from_numpy(synth.uniform24(seed, b * h * w).reshape(b, 1, h, w)).to(dtype)


@pytest.mark.parametrize("h,w,dtype", [(40, 72, torch.float32), (72, 104, torch.float16)])
def test_encoder_within_twice_the_storage_models_error(dev, sd, encoder, h, w, dtype):
    """exact: the float64 forward on the fp16-rounded weights; model: storage fp16, compute float64; E = max
    |model - exact|. The kernels implement model up to the order of their fp32 sums, which can flip single
    fp16 roundings of the size E already counts: max |ours - exact| <= 2 E, for logits and dense separately."""
    from lightglue_amd import superpoint_reference

    img = images(5, 2, h, w, dtype)
    sd16 = {k: v.half().double() for k, v in sd.items()}
    exact = superpoint_reference(sd16, img.double(), None, torch.float64)
    model = superpoint_reference(sd, img.double(), torch.float16, torch.float64)
    with torch.no_grad():
        logits, dense = encoder.heads(img.to(dev))
    assert logits.shape == (2, 65, h // 8, w // 8) and logits.is_contiguous() and dense.shape == (2, 256, h // 8, w // 8)
    assert dense.stride()[1] == 1
    ratios = []
    for name, got, e, m in zip(("logits", "dense"), (logits, dense), exact, model):
        big_e = float((m - e).abs().max())
        ours = float((got.cpu().double() - e).abs().max())
        print(f"encoder {h}x{w} {name}: E {big_e:.3e}, ours {ours:.3e}, ours / E {ours / big_e:.3f}")
        ratios.append(ours / big_e)
    assert max(ratios) <= 2.0, ratios


# ---- plumbing, capture, repeatability -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(dev):
    return seeded_matcher(dev)


def test_extract_and_match_images_are_their_parts(dev, encoder, model):
    from lightglue_amd import Features, KeypointFrontend, match_images

    fe = KeypointFrontend(max_keypoints=64)
    i0, i1 = images(21, 2, 40, 72).to(dev), images(22, 2, 40, 72).to(dev)
    with torch.no_grad():
        f = encoder.extract(i0, fe)
        g = fe.extract(*encoder.heads(i0))
        equal_results(f, g, "extract")
        assert int(f.counts.min()) > 0
        got = match_images(encoder, fe, model, i0, i1)
        both = fe.extract(*encoder.heads(torch.cat([i0, i1])))
        want = model.match_features(Features(*(t[:2] for t in both)), Features(*(t[2:] for t in both)))
        equal_results(got, want, "match_images")
        again = match_images(encoder, fe, model, i0, i1)  # repeatability: two eager runs, the same bits
        equal_results(got, again, "repeat")
        l0, d0 = encoder.heads(i0)
        l1, d1 = encoder.heads(i0)
        assert same_bits(l0, l1) and same_bits(d0, d1)


def test_extract_pairs_is_one_extract_split_in_two(dev, encoder, model):
    """40 x 72: 5 x 9 cells, a non-square map and a ragged last tile in lg_sp_conv3x3. Both halves equal one
    extract over the concatenated batch split by hand, bitwise on every field; batches that disagree in shape
    raise what match_images raises."""
    from lightglue_amd import Features, KeypointFrontend, extract_pairs, match_images

    fe = KeypointFrontend(max_keypoints=64)
    i0, i1 = images(21, 2, 40, 72).to(dev), images(22, 2, 40, 72).to(dev)
    with torch.no_grad():
        f0, f1 = extract_pairs(encoder, fe, i0, i1)
        both = fe.extract(*encoder.heads(torch.cat([i0, i1])))
    assert isinstance(f0, Features) and isinstance(f1, Features) and int(both.counts.min()) > 0
    equal_results(f0, Features(*(t[:2] for t in both)), "side 0")
    equal_results(f1, Features(*(t[2:] for t in both)), "side 1")
    errors = []
    for fn in (lambda: extract_pairs(encoder, fe, i0, i1[:1]), lambda: match_images(encoder, fe, model, i0, i1[:1])):
        with pytest.raises(ValueError, match="must agree in shape and dtype") as e:
            fn()
        errors.append(str(e.value))
    assert errors[0] == errors[1]


def test_captured_images_to_matches_replays_on_a_new_pair(dev, encoder, model):
    """heads + extract + match_features captured once on a side stream; a second image pair copied into the
    captured input buffers; the replay equals the eager result on that pair bitwise (features and matches) and
    differs from the first pair's (nothing is baked in at capture, no count reaches the host)."""
    from lightglue_amd import Features, KeypointFrontend

    fe = KeypointFrontend(max_keypoints=64)
    a0, a1 = images(31, 1, 40, 72).to(dev), images(32, 1, 40, 72).to(dev)
    b0, b1 = images(33, 1, 40, 72).to(dev), images(34, 1, 40, 72).to(dev)
    in0, in1 = a0.clone(), a1.clone()

    def run(i0, i1):
        f = fe.extract(*encoder.heads(torch.cat([i0, i1])))
        return f, model.match_features(Features(*(t[:1] for t in f)), Features(*(t[1:] for t in f)))

    graph, (cf, cm) = capture_on_side_stream(lambda: run(in0, in1))
    with torch.no_grad():
        graph.replay()
        torch.cuda.synchronize()
        first_f, first_m = type(cf)(*(t.clone() for t in cf)), type(cm)(*(t.clone() for t in cm))
        ef, em = run(a0, a1)
        equal_results(first_f, ef, "replay, the captured pair: features")
        equal_results(first_m, em, "replay, the captured pair: matches")
        in0.copy_(b0), in1.copy_(b1)
        graph.replay()
        torch.cuda.synchronize()
        ef, em = run(b0, b1)
    equal_results(cf, ef, "replay, a new pair: features")
    equal_results(cm, em, "replay, a new pair: matches")
    assert int(ef.counts.min()) > 0
    assert not torch.equal(cf.kpts_px, first_f.kpts_px) and not same_bits(cf.desc, first_f.desc)
    assert not same_bits(cm.scores0, first_m.scores0) or not torch.equal(cm.matches0, first_m.matches0)
