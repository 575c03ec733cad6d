"""The image input on the MI355X: lg_img_prepare against image_reference in float64 (CPU) under a derived bound,
for both interpolations, both output types and 1, 3 and 4 channels; a ragged batch whose middle image would
break the bound if a neighbour read it; layouts and strided views read in place; constants; the table-free form
bitwise the table form; lg_kp_to_source against float64; and match_source_images against its parts, captured
once and replayed on new pixels. Nothing here reads the reference tree.

The derived bound, with T = (taps in y) x (taps in x) x channels (taps: 2 for linear; for area on a shrinking axis
the most source pixels an output's interval [o n / nt, (o + 1) n / nt) touches):
    fp32 output: |out - ref| <= (2 T + 8) 2^-24
    fp16 output: that + 2^-11 ref + 2^-24
Each weight is one fp32 rounding of an exact rational, each product one rounding, the sum T roundings, and every
partial result is at most 1; the 8 covers the grey weights and the 1 / 255.
"""
import functools

import pytest
import torch

from gpu_common import capture_on_side_stream, equal_results, same_bits, seeded_matcher

pytestmark = pytest.mark.gpu

TARGET_PAIRS = (((1, 1), (8, 8)), ((3, 5), (8, 8)), ((37, 53), (16, 24)), ((100, 7), (8, 16)), ((481, 641), (16, 24)),
                ((16, 24), (16, 24)), ((64, 48), (16, 24)))
INTERPS = ("linear", "area")
DTYPES = (torch.float16, torch.float32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def rand_u8(seed, *shape, high=256):
    return torch.randint(0, high, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def taps(n_src, n_dst, interp):
    if interp == "area" and n_src > n_dst:
        return max(-((-(o + 1) * n_src) // n_dst) - (o * n_src) // n_dst for o in range(n_dst))
    return 2


def check_bound(out, ref, src, dst, channels, interp, what):
    """out [Ht, Wt] (GPU result, any float type) against ref (float64, CPU) for one image."""
    t = taps(src[0], dst[0], interp) * taps(src[1], dst[1], interp) * min(channels, 3)
    bound = torch.full_like(ref, (2 * t + 8) * 2.0 ** -24)
    if out.dtype == torch.float16:
        bound = bound + 2.0 ** -11 * ref + 2.0 ** -24
    err = (out.cpu().double() - ref).abs()
    worst = float((err / bound).max())
    print(f"{what}: T {t}, max err {float(err.max()):.3e}, max err / bound {worst:.3f}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0, (what, worst, float(err.max()))


@functools.lru_cache(maxsize=None)
def source(src, channels):
    """One seeded HWC image ([H, W] for one channel) per (size, channels), shared by every test that uses it."""
    shape = src if channels == 1 else src + (channels,)
    return rand_u8(src[0] * 7919 + src[1] * 31 + channels, *shape)


@functools.lru_cache(maxsize=None)
def reference(src, dst, channels, interp):
    from lightglue_amd import image_reference

    return image_reference([source(src, channels)], dst, interp, torch.float64)[0]


# ---- lg_img_prepare against the bound ------------------------------------------------------------------------
@pytest.mark.parametrize("channels", (1, 3, 4))
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("interp", INTERPS)
def test_prepare_within_the_derived_bound(dev, interp, dtype, channels):
    from lightglue_amd import ImageInput

    for src, dst in TARGET_PAIRS:
        p = ImageInput(dst, interp, dtype).prepare([source(src, channels).to(dev)])
        assert p.image.shape == (1,) + dst and p.image.dtype == dtype and p.image.is_contiguous()
        assert p.src_sizes.tolist() == [list(src)]
        check_bound(p.image[0], reference(src, dst, channels, interp), src, dst, channels, interp,
                    f"prepare {interp} {dtype} c{channels} {src}->{dst}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("interp", INTERPS)
def test_ragged_batch_keeps_each_image_to_itself(dev, interp, dtype):
    """Three sources of three sizes in one launch; the middle one is all 255, the outer two at most 16: a row or
    a descriptor taken from a neighbour breaks the bound instead of hiding."""
    from lightglue_amd import ImageInput, image_reference

    dst = (16, 24)
    imgs = [rand_u8(41, 3, 5, 3, high=17), torch.full((37, 53, 3), 255, dtype=torch.uint8), rand_u8(42, 64, 48, 3, high=17)]
    ref = image_reference(imgs, dst, interp, torch.float64)
    p = ImageInput(dst, interp, dtype).prepare([i.to(dev) for i in imgs])
    assert p.image.shape == (3,) + dst and p.src_sizes.tolist() == [[3, 5], [37, 53], [64, 48]]
    for b, img in enumerate(imgs):
        check_bound(p.image[b], ref[b], tuple(img.shape[:2]), dst, 3, interp, f"ragged {interp} {dtype} image {b}")
    assert float(p.image[0].max()) < 0.07 and float(p.image[2].max()) < 0.07 and float(p.image[1].min()) > 0.999


@pytest.mark.parametrize("src", ((37, 53), (40, 131)))
@pytest.mark.parametrize("interp", INTERPS)
def test_layouts_and_views_are_read_in_place(dev, interp, src):
    """HWC, CHW, bgr and a cropped view (row stride != w c): bitwise the result on contiguous copies. The kernel
    reads rows whose pixels and channels are adjacent bytes as dwords on an area axis (four taps at a time up to
    a ratio of 4: 53 -> 24; eight beyond: 131 -> 24) and any other layout byte by byte: the same bits."""
    from lightglue_amd import ImageInput

    dst = (16, 24)
    ii = ImageInput(dst, interp, torch.float32)
    hwc = source(src, 3).to(dev)
    base = ii.prepare([hwc]).image
    check_bound(base[0], reference(src, dst, 3, interp), src, dst, 3, interp, f"layouts {interp} hwc")
    chw = hwc.permute(2, 0, 1)
    assert not chw.is_contiguous()
    assert same_bits(ii.prepare([chw], layout="chw").image, base)               # a CHW view of HWC memory
    assert same_bits(ii.prepare([chw.contiguous()], layout="chw").image, base)  # planar memory
    assert same_bits(ii.prepare([hwc.flip(-1).contiguous()], bgr=True).image, base)
    assert not same_bits(ii.prepare([hwc], bgr=True).image, base)
    big = rand_u8(43, src[0] + 23, src[1] + 27, 4).to(dev)
    crop = big[11:11 + src[0], 20:20 + src[1]]
    assert not crop.is_contiguous() and crop.stride(0) != src[1] * 4
    got = ii.prepare([crop]).image
    assert same_bits(got, ii.prepare([crop.contiguous()]).image)
    assert same_bits(got, ii.prepare([crop[..., :3]]).image)                    # RGB at a pixel stride of 4
    assert same_bits(got, ii.prepare([crop[..., :3].contiguous()]).image)       # the fourth channel is ignored
    grey = source(src, 1).to(dev)
    assert same_bits(ii.prepare([grey]).image, ii.prepare([grey[..., None]]).image)
    assert same_bits(ii.prepare([grey.t().contiguous().t()]).image, ii.prepare([grey]).image)  # column-major


@pytest.mark.parametrize("interp", INTERPS)
def test_constant_images_are_exact(dev, interp):
    """fp16 output: 0 everywhere for a black image and 1.0 everywhere for a white one (normalised weights)."""
    from lightglue_amd import ImageInput

    ii = ImageInput((16, 24), interp, torch.float16)
    for shape in ((37, 53, 3), (37, 53), (3, 5, 4), (64, 48, 3), (481, 641)):
        for value, want in ((0, 0.0), (255, 1.0)):
            out = ii.prepare([torch.full(shape, value, dtype=torch.uint8, device=dev)]).image
            assert bool((out == want).all()), (shape, value, float(out.min()), float(out.max()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("interp", INTERPS)
def test_batch_form_is_bitwise_the_table_form(dev, interp, dtype):
    from lightglue_amd import ImageInput

    ii = ImageInput((16, 24), interp, dtype)
    frames = rand_u8(44, 3, 37, 53, 3).to(dev)
    want = ii.prepare(list(frames))
    got = ii.prepare(frames)
    assert same_bits(got.image, want.image) and torch.equal(got.src_sizes, want.src_sizes)
    assert same_bits(ii.prepare(frames.permute(0, 3, 1, 2), layout="chw").image, want.image)
    assert same_bits(ii.prepare(frames.flip(-1).contiguous(), bgr=True).image, want.image)
    view = frames[:, 2:30, 5:40]  # a crop of every frame: batch and row strides of the full frames
    assert same_bits(ii.prepare(view).image, ii.prepare([v.contiguous() for v in view]).image)
    grey = rand_u8(45, 2, 64, 48).to(dev)
    assert same_bits(ii.prepare(grey).image, ii.prepare(list(grey)).image)
    assert same_bits(ii.prepare(frames[1:2]).image, want.image[1:2])


# ---- lg_kp_to_source ------------------------------------------------------------------------------------------------
def ulps32(got, ref):
    """|got - ref| in fp32 ulps at ref's magnitude (ref float64)."""
    _, e = torch.frexp(ref.abs())
    return (got.double() - ref).abs() / torch.pow(2.0, (e - 24).double())


@pytest.mark.parametrize("target,sources", [((480, 640), ((3000, 4000), (480, 640), (16384, 1), (37, 16384), (1, 1))),
                                            ((16384, 16384), ((16384, 16384), (1, 1), (8000, 12345))),
                                            ((8, 8), ((16384, 16384), (8, 8), (3, 5)))])
def test_keypoints_to_source(dev, target, sources):
    from lightglue_amd import Features, ImageInput, PreparedImages

    ht, wt = target
    b, k = len(sources), 64
    gen = torch.Generator().manual_seed(ht + b)
    px = torch.stack([torch.randint(0, wt, (b, k), generator=gen), torch.randint(0, ht, (b, k), generator=gen)], -1).int()
    px[:, 0], px[:, 1] = 0, torch.tensor([wt - 1, ht - 1], dtype=torch.int32)  # both ends of both axes
    counts = torch.tensor([k, 5, 0, k - 1, 1][:b], dtype=torch.int32)
    sizes = torch.tensor(sources, dtype=torch.int32)
    f = Features(px.to(dev), None, None, None, counts.to(dev))
    got = ImageInput(target).keypoints(f, PreparedImages(None, sizes.to(dev))).cpu()
    assert got.shape == (b, k, 2) and got.dtype == torch.float32
    wh = sizes.flip(-1).double()[:, None, :]                       # (w, h) per image
    ref = (2 * px.double() + 1) * wh / (2 * torch.tensor([wt, ht]).double()) - 0.5
    valid = (torch.arange(k)[None, :] < counts[:, None])[..., None].expand_as(ref)
    worst = float(ulps32(got, ref)[valid].max())
    print(f"kp_to_source {target}: max error {worst:.3f} ulps")
    assert worst <= 4.0
    assert bool((got[~valid] == 0).all())                          # rows past the count: exact zeros
    for i, s in enumerate(sources):
        if s == target:                                            # the same size: exactly px
            assert torch.equal(got[i][valid[i]], px[i].float()[valid[i]])


# ---- match_source_images --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoder():
    from lightglue_amd import SuperPointEncoder, seeded_superpoint_state_dict

    return SuperPointEncoder(seeded_superpoint_state_dict(3))


@pytest.fixture(scope="module")
def model(dev):
    return seeded_matcher(dev)


TARGET = (40, 72)  # the size tests/test_gpu_superpoint.py's match_images test uses
SIDE0 = ((50, 70, 3), (96, 64))
SIDE1 = ((61, 83), (40, 120, 3))


def sides(seed, dev):
    return tuple([rand_u8(seed + 10 * s + i, *shape).to(dev) for i, shape in enumerate(side)] for s, side in enumerate((SIDE0, SIDE1)))


def check_source_keypoints(kp, features, prepared, what):
    """kp [P, K, 2] against (2 px + 1) w / (2 Wt) - 1/2 in float64; zeros past the counts."""
    px, counts, sizes = features.kpts_px.cpu(), features.counts.cpu(), prepared.src_sizes.cpu()
    ref = (2 * px.double() + 1) * sizes.flip(-1).double()[:, None, :] / (2 * torch.tensor([TARGET[1], TARGET[0]]).double()) - 0.5
    valid = (torch.arange(px.shape[1])[None, :] < counts[:, None])[..., None].expand_as(ref)
    assert float(ulps32(kp.cpu(), ref)[valid].max()) <= 4.0, what
    assert bool((kp.cpu()[~valid] == 0).all()), what


def test_match_source_images_is_its_parts(dev, encoder, model):
    from lightglue_amd import Features, ImageInput, KeypointFrontend, match_images, match_source_images

    fe, ii = KeypointFrontend(max_keypoints=64), ImageInput(TARGET)
    s0, s1 = sides(100, dev)
    with torch.no_grad():
        got, kp0, kp1 = match_source_images(ii, encoder, fe, model, s0, s1)
        p0, p1 = ii.prepare(s0), ii.prepare(s1)
        assert p0.src_sizes.tolist() == [[50, 70], [96, 64]] and p1.src_sizes.tolist() == [[61, 83], [40, 120]]
        equal_results(got, match_images(encoder, fe, model, p0.image, p1.image), "match_source_images")
        f = encoder.extract(torch.cat([p0.image, p1.image]), fe)
        assert int(f.counts.min()) > 0
        for kp, ft, p, what in ((kp0, Features(*(t[:2] for t in f)), p0, "side 0"), (kp1, Features(*(t[2:] for t in f)), p1, "side 1")):
            assert kp.shape == (2, 64, 2) and kp.dtype == torch.float32
            check_source_keypoints(kp, ft, p, what)
        again, a0, a1 = match_source_images(ii, encoder, fe, model, s0, s1)  # two eager runs, the same bits
        equal_results(got, again, "repeat")
        assert same_bits(kp0, a0) and same_bits(kp1, a1)


def test_captured_source_images_to_matches_replay_on_new_pixels(dev, encoder, model):
    """The tables are built once, before the capture; new pixels go into the same source tensors; the replay is
    bitwise the eager result on those pixels and differs from the first."""
    from lightglue_amd import ImageInput, KeypointFrontend, match_source_images

    fe, ii = KeypointFrontend(max_keypoints=64), ImageInput(TARGET)
    a0, a1 = sides(200, dev)
    b0, b1 = sides(300, dev)
    in0, in1 = [t.clone() for t in a0], [t.clone() for t in a1]
    t0, t1 = ii.table(in0), ii.table(in1)

    def run(x0, x1):
        return match_source_images(ii, encoder, fe, model, x0, x1)

    def cloned(r):
        return type(r[0])(*(t.clone() for t in r[0])), r[1].clone(), r[2].clone()

    def equal(x, y, what):
        equal_results(x[0], y[0], what)
        assert same_bits(x[1], y[1]) and same_bits(x[2], y[2]), what

    graph, captured = capture_on_side_stream(lambda: run(t0, t1))
    with torch.no_grad():
        graph.replay()
        torch.cuda.synchronize()
        first = cloned(captured)
        equal(first, run(a0, a1), "replay, the captured pixels")
        for dst, src in zip(in0 + in1, b0 + b1):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        equal(captured, run(b0, b1), "replay, new pixels")
    assert not same_bits(captured[1], first[1]) or not same_bits(captured[0].scores0, first[0].scores0)
