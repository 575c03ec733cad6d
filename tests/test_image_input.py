"""The image input's host side, no GPU: the pinned resampling (resample_matrix) against F.interpolate and
F.avg_pool2d, target_size, the framework restatement image_reference (grey weights, bgr, alpha, layouts, strided
views, constants), the descriptor's size, every lg_img_* / lg_kp_to_source argument check (nothing reaches the
device), and ImageInput's own validation."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below

SIZE_PAIRS = (((1, 1), (8, 8)), ((3, 5), (8, 8)), ((37, 53), (16, 24)), ((100, 7), (8, 16)), ((481, 641), (16, 24)))


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def rand_u8(seed, *shape):
    return torch.randint(0, 256, shape, generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---- resample_matrix ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", ("linear", "area"))
def test_rows_sum_to_one(interp):
    from lightglue_amd import resample_matrix

    for (h, w), (ht, wt) in SIZE_PAIRS + (((64, 48), (16, 24)), ((16, 24), (16, 24)), ((16384, 1), (8, 8)), ((4000, 3000), (640, 480))):
        for n_src, n_dst in ((h, ht), (w, wt)):
            m = resample_matrix(n_src, n_dst, interp)
            assert m.shape == (n_dst, n_src) and m.dtype == torch.float64
            assert float((m.sum(1) - 1.0).abs().max()) <= 1e-12, (n_src, n_dst, interp)
            assert float(m.min()) >= 0.0


@pytest.mark.parametrize("src,dst", SIZE_PAIRS)
def test_linear_is_bilinear_without_aligned_corners(src, dst):
    from lightglue_amd import resample_matrix

    x = torch.rand(src, generator=torch.Generator().manual_seed(src[0] * 1000 + src[1]), dtype=torch.float64)
    want = F.interpolate(x[None, None], size=dst, mode="bilinear", align_corners=False)[0, 0]
    got = resample_matrix(src[0], dst[0], "linear") @ x @ resample_matrix(src[1], dst[1], "linear").t()
    assert float((got - want).abs().max()) <= 1e-12
    # and area on axes that do not shrink is linear
    if src[0] <= dst[0]:
        assert torch.equal(resample_matrix(src[0], dst[0], "area"), resample_matrix(src[0], dst[0], "linear"))


def test_identity_is_the_identity():
    from lightglue_amd import resample_matrix

    for interp in ("linear", "area"):
        assert torch.equal(resample_matrix(24, 24, interp), torch.eye(24, dtype=torch.float64))


def test_area_is_the_mean_at_integer_ratios_and_the_overlap_elsewhere():
    from lightglue_amd import resample_matrix

    x = rand_u8(3, 64, 48).double()
    got = resample_matrix(64, 16, "area") @ x @ resample_matrix(48, 24, "area").t()
    assert torch.equal(got, F.avg_pool2d(x[None, None], (4, 2))[0, 0])  # sums of integers / 8: exact
    for n_src, n_dst in ((37, 16), (53, 24)):
        m = resample_matrix(n_src, n_dst, "area")
        assert float(m.min()) >= 0.0
        for o in range(n_dst):
            first, end = (o * n_src) // n_dst, -((-(o + 1) * n_src) // n_dst)  # floor, ceil
            support = torch.nonzero(m[o])[:, 0].tolist()
            assert support == list(range(first, end)), (n_src, n_dst, o)
            lo, hi = o * n_src / n_dst, (o + 1) * n_src / n_dst
            for i in support:  # the overlap of [i, i + 1) with [lo, hi), over the interval's length
                assert abs(float(m[o, i]) - (min(i + 1, hi) - max(i, lo)) / (n_src / n_dst)) <= 1e-12


def test_resample_matrix_rejects_bad_arguments():
    from lightglue_amd import resample_matrix

    for bad in ((0, 8, "linear"), (8, 0, "linear"), (16385, 8, "area"), (8, 16385, "area"), (8, 8, "cubic"), (8, 8, "nearest")):
        with pytest.raises(ValueError):
            resample_matrix(*bad)


# ---- target_size ------------------------------------------------------------------------------------------------
def test_target_size():
    from lightglue_amd import target_size

    assert target_size(480, 640, (480, 640)) == (480, 640) and target_size(3000, 4000, [240, 320]) == (240, 320)
    assert target_size(3000, 4000, 640) == (480, 640) and target_size(4000, 3000, 640) == (640, 480)
    assert target_size(1080, 1920, 640) == (360, 640)
    # round(h scale) first (utils.resize_image), then the nearest multiple of 8, a tie upwards
    assert target_size(1080, 1920, 1024) == (576, 1024)
    assert target_size(500, 700, 100) == (72, 104)    # 71 x 100: 71 -> 72, 100 -> 104 (a tie)
    assert target_size(300, 1000, 100) == (32, 104)   # 30 -> 32
    assert target_size(480, 640, 1280) == (960, 1280)  # enlarging
    assert target_size(1, 1000, 64) == (8, 64) and target_size(2, 2, 3) == (8, 8)  # never below 8
    for bad in ((480, 641), (481, 640), (0, 8), (8, 0), (-8, 8), (8,), (8, 8, 8), "640", 6.5, None, (8.0, 8)):
        with pytest.raises(ValueError):
            target_size(480, 640, bad)
    for h, w, r in ((0, 8, 64), (8, 0, 64), (8, 8, 0), (8, 8, -64)):
        with pytest.raises(ValueError):
            target_size(h, w, r)


# ---- image_reference ----------------------------------------------------------------------------------------------
def test_reference_grey_weights_bgr_and_alpha():
    from lightglue_amd import image_reference

    size, f64 = (16, 24), torch.float64
    rgb = rand_u8(5, 16, 24, 3)
    got = image_reference([rgb], size, "linear", f64)
    want = (0.299 * rgb[..., 0].double() + 0.587 * rgb[..., 1].double() + 0.114 * rgb[..., 2].double()) / 255.0
    assert got.shape == (1, 16, 24) and float((got[0] - want).abs().max()) <= 1e-15  # (identity resampling)
    for ch, weight in enumerate((0.299, 0.587, 0.114)):  # each channel alone
        one = torch.zeros_like(rgb)
        one[..., ch] = 255
        assert float((image_reference([one], size, "linear", f64) - weight).abs().max()) <= 1e-15
    assert torch.equal(image_reference([rgb.flip(-1)], size, "linear", f64, bgr=True), got)
    assert not torch.equal(image_reference([rgb], size, "linear", f64, bgr=True), got)
    rgba = torch.cat([rgb, rand_u8(6, 16, 24, 1)], -1)
    assert torch.equal(image_reference([rgba], size, "linear", f64), got)
    grey = rand_u8(7, 16, 24)
    for form in (grey, grey[..., None]):
        assert torch.equal(image_reference([form], size, "area", f64)[0], grey.double() / 255.0)


@pytest.mark.parametrize("interp", ("linear", "area"))
def test_reference_layouts_and_strided_views_are_bitwise(interp):
    from lightglue_amd import image_reference

    size, f64 = (16, 24), torch.float64
    hwc = rand_u8(8, 37, 53, 3)
    base = image_reference([hwc], size, interp, f64)
    assert torch.equal(image_reference([hwc.permute(2, 0, 1).contiguous()], size, interp, f64, layout="chw"), base)
    assert torch.equal(image_reference([hwc.permute(2, 0, 1)], size, interp, f64, layout="chw"), base)  # a CHW view of HWC
    big = rand_u8(9, 60, 80, 4)
    crop = big[11:48, 20:73]  # [37, 53, 4], row stride 320 != 53 * 4
    assert not crop.is_contiguous()
    assert torch.equal(image_reference([crop], size, interp, f64), image_reference([crop.contiguous()], size, interp, f64))
    # a [B, ...] tensor and a ragged list
    frames = rand_u8(10, 3, 37, 53, 3)
    both = image_reference(frames, size, interp, f64), image_reference(list(frames), size, interp, f64)
    assert float((both[0] - both[1]).abs().max()) <= 1e-14  # (one batched product against three)
    ragged = image_reference([hwc, rand_u8(11, 64, 48), crop], size, interp, f64)
    assert ragged.shape == (3, 16, 24) and torch.equal(ragged[:1], base)


@pytest.mark.parametrize("interp", ("linear", "area"))
@pytest.mark.parametrize("dtype", (torch.float16, torch.float32))
def test_reference_constants_are_exact(interp, dtype):
    from lightglue_amd import image_reference

    for shape in ((37, 53, 3), (37, 53), (3, 5, 4), (64, 48, 1)):
        for value, want in ((0, 0.0), (255, 1.0)):
            out = image_reference([torch.full(shape, value, dtype=torch.uint8)], (16, 24), interp, dtype)
            assert out.dtype == dtype and bool((out == want).all()), (shape, value, interp)


# ---- the C entry points ---------------------------------------------------------------------------------------------
def test_descriptor_size(lib):
    from lightglue_amd import _lib

    assert lib.lg_img_src_bytes() == ctypes.sizeof(_lib.ImgSrc) == 48
    assert _lib.ImgSrc.stride_y.offset == 24 and _lib.ImgSrc.data.offset == 0 and _lib.ImgSrc.bgr.offset == 20


def _rejects(call, bads):
    for bad in bads:
        assert call(**bad) == 1, bad


def test_entry_points_validate_before_touching_the_device(lib):
    """lg_img_prepare, lg_img_prepare_batch, lg_kp_to_source: an empty launch returns success and every clause of
    the argument check rejects with a message, on fake addresses and without a device call."""
    from lightglue_amd import _lib

    target = [dict(batch=-1), dict(batch=65536), dict(ht=0), dict(ht=-8), dict(ht=16385), dict(wt=0), dict(wt=-8),
              dict(wt=16385), dict(interp=-1), dict(interp=2), dict(dt=2), dict(dt=-1), dict(out=None), dict(out=2 * A + 1),
              dict(dt=0, out=2 * A + 2)]

    def prepare(**kw):
        a = dict(table=A, batch=0, ht=8, wt=8, interp=0, dt=1, out=2 * A)
        a.update(kw)
        return lib.lg_img_prepare(a["table"], a["batch"], a["ht"], a["wt"], a["interp"], a["dt"], a["out"], None)

    assert prepare() == 0 and prepare(ht=1, wt=16384, interp=1, dt=0, out=2 * A + 4, table=A + 8) == 0
    assert prepare(ht=13, wt=7, out=2 * A + 2) == 0  # multiples of nothing; fp16 output 2-B aligned
    _rejects(prepare, target + [dict(table=None), dict(table=A + 4), dict(table=A + 1)])
    assert "lg_img_prepare" in _lib.last_error() and "lg_img_prepare_batch" not in _lib.last_error()

    def batch(**kw):
        a = dict(data=A, batch=0, h=8, w=8, c=3, bgr=0, sb=192, sy=24, sx=3, sc=1, ht=8, wt=8, interp=0, dt=1, out=2 * A)
        a.update(kw)
        return lib.lg_img_prepare_batch(a["data"], a["batch"], a["h"], a["w"], a["c"], a["bgr"], a["sb"], a["sy"], a["sx"],
                                        a["sc"], a["ht"], a["wt"], a["interp"], a["dt"], a["out"], None)

    assert batch() == 0 and batch(data=A + 1, h=1, w=16384, c=1, bgr=1, sb=0, sy=0, sx=0, sc=0, interp=1, dt=0) == 0
    assert batch(c=4, sb=1 << 40, sy=1 << 40, sx=1 << 40, sc=1 << 40) == 0
    big = (1 << 40) + 1
    _rejects(batch, target + [dict(data=None), dict(h=0), dict(h=-1), dict(h=16385), dict(w=0), dict(w=-1), dict(w=16385),
                              dict(c=0), dict(c=2), dict(c=5), dict(c=-3), dict(bgr=2), dict(bgr=-1), dict(sb=-1), dict(sy=-1),
                              dict(sx=-1), dict(sc=-1), dict(sb=big), dict(sy=big), dict(sx=big), dict(sc=big)])
    assert "lg_img_prepare_batch" in _lib.last_error()

    def to_source(**kw):
        a = dict(kp=A, counts=A, sizes=A, ht=8, wt=8, batch=0, k=8, out=2 * A)
        a.update(kw)
        return lib.lg_kp_to_source(a["kp"], a["counts"], a["sizes"], a["ht"], a["wt"], a["batch"], a["k"], a["out"], None)

    assert to_source() == 0 and to_source(ht=1, wt=16384, k=1, kp=A + 4, counts=A + 4, sizes=A + 4, out=2 * A + 4) == 0
    _rejects(to_source, [dict(batch=-1), dict(k=0), dict(k=-8), dict(batch=1 << 14, k=(1 << 14) + 1), dict(ht=0), dict(ht=16385),
                         dict(wt=0), dict(wt=16385), dict(kp=None), dict(counts=None), dict(sizes=None), dict(out=None),
                         dict(kp=A + 2), dict(counts=A + 2), dict(sizes=A + 2), dict(out=2 * A + 2)])
    assert "lg_kp_to_source" in _lib.last_error()


# ---- ImageInput ---------------------------------------------------------------------------------------------------------
def test_image_input_validates():
    from lightglue_amd import Features, ImageInput, PluginError, PreparedImages

    for bad in ((480, 641), (12, 16), (0, 8), 640, (8, 8, 8), None):
        with pytest.raises(ValueError):
            ImageInput(bad)
    with pytest.raises(ValueError, match="interp"):
        ImageInput((8, 8), interp="cubic")
    with pytest.raises(ValueError, match="dtype"):
        ImageInput((8, 8), dtype=torch.float64)
    ii = ImageInput((16, 24), "area", torch.float32)
    assert ii.size == (16, 24) and ii.interp == "area" and ii.dtype == torch.float32
    good = rand_u8(1, 10, 12, 3)
    for call in (ii.table, ii.prepare):
        with pytest.raises(PluginError, match="GPU"):
            call([good])
        with pytest.raises(PluginError, match="GPU"):
            call([good.permute(2, 0, 1)], layout="chw")
        for bad, what in ((good.float(), "uint8"), (good.to(torch.int8), "uint8"), (rand_u8(2, 10, 12, 2), "channels"),
                          (rand_u8(2, 5, 10, 12, 3), "expected"), (torch.zeros(0, 12, 3, dtype=torch.uint8), "sides"),
                          (torch.zeros(10, 0, dtype=torch.uint8), "sides"), ([[1, 2], [3, 4]], "tensor")):
            with pytest.raises(ValueError, match=what):
                call([good, bad])
        with pytest.raises(ValueError, match="channels"):
            call([good], layout="chw")  # read as 10 channels
        with pytest.raises(ValueError, match="layout"):
            call([good], layout="nhwc")
        with pytest.raises(ValueError, match="no images"):
            call([])
    # one [B, ...] tensor
    with pytest.raises(PluginError, match="GPU"):
        ii.prepare(rand_u8(3, 2, 10, 12, 3))
    with pytest.raises(PluginError, match="GPU"):
        ii.prepare(rand_u8(3, 2, 10, 12))
    for bad, what in ((rand_u8(3, 2, 10, 12, 3).float(), "uint8"), (rand_u8(3, 2, 10, 12, 2), "channels"),
                      (torch.zeros(2, 10, 0, 3, dtype=torch.uint8), "sides"), (rand_u8(3, 10, 12), "expected"),
                      (torch.zeros(0, 10, 12, dtype=torch.uint8), "no images")):
        with pytest.raises(ValueError, match=what):
            ii.prepare(bad)
    f = Features(torch.zeros(1, 8, 2, dtype=torch.int32), None, None, None, torch.zeros(1, dtype=torch.int32))
    with pytest.raises(PluginError, match="GPU"):
        ii.keypoints(f, PreparedImages(None, torch.zeros(1, 2, dtype=torch.int32)))


def test_image_reference_validates():
    from lightglue_amd import image_reference

    good = rand_u8(1, 10, 12, 3)
    for bad in (good.float(), rand_u8(2, 10, 12, 2), torch.zeros(0, 12, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            image_reference([bad], (8, 8))
    with pytest.raises(ValueError, match="interp"):
        image_reference([good], (8, 8), "cubic")
    assert image_reference([good], (8, 8)).dtype == torch.float16
