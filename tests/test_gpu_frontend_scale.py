"""Keypoint front end on the MI355X at the size it was written for (480 x 640, K = 1024 and 2048) and at the sizes
where lg_kp_select's control flow changes (frontend_refs.SHAPES; test_frontend_scale_reference.py asserts the fact
each shape is there for). Select and NMS are exact operations: bitwise against select_reference / nms_reference on
the CPU, no case excluded. The heat map and the descriptors are judged against float64 under a bound the test takes
from the fp32 restatement's own error on the same input. Every input comes from a seed; no NaN or Inf in any map."""
import pytest
import torch
import torch.nn.functional as F

import frontend_refs as fr
from gpu_common import equal_results, same_bits

pytestmark = pytest.mark.gpu

THR, BORDER = 0.0005, 4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def assert_select(got, want, tag):
    """count, pix and score bitwise (so also -1 / 0 past the count)."""
    got = [t.cpu() for t in got]
    for name, a, b in zip(("count", "pix", "score"), got, want):
        if not same_bits(a, b):
            bad = torch.nonzero((a.view(torch.int32) != b.view(torch.int32)).reshape(a.shape[0], -1))
            first = bad[0].tolist()
            raise AssertionError(f"select {tag}: {name} differs in {bad.shape[0]} places, first at image {first[0]} "
                                 f"slot {first[1]}; counts {got[0].tolist()} want {want[0].tolist()}")


# ---- a. select ------------------------------------------------------------------------------------------
def dense_settings(shape):
    """(threshold, border, K): every pixel a candidate at K = 2048; threshold 0.5 inside the border at K = 1024; at
    480 x 640 both again at K = 8 and at K = 1000 (the sort pads to 1024)."""
    s = [(0.0, 0, 2048), (0.5, 4, 1024)]
    if shape == (480, 640):
        s += [(thr, border, k) for k in (8, 1000) for thr, border in ((0.0, 0), (0.5, 4))]
    return s


@pytest.mark.parametrize("name", fr.DENSE_MAPS)
@pytest.mark.parametrize("shape", fr.SELECT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_dense_maps(dev, shape, name):
    from lightglue_amd import frontend

    h, w = shape
    x = fr.assert_finite(fr.dense_map(name, 2, h, w, 1000 + 7 * h + w))
    xd = x.to(dev)
    for thr, border, k in dense_settings(shape):
        want = frontend.select_reference(x, k, thr, border)
        assert_select(frontend.select(xd, k, thr, border), want, f"{name} {h} x {w} thr {thr} border {border} K {k}")


@pytest.mark.parametrize("where", fr.PLACEMENTS)
@pytest.mark.parametrize("k", [8, 2048])
@pytest.mark.parametrize("shape", [(256, 257), (480, 640)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_select_sparse_maps(dev, shape, k, where):
    """n = 0, 1, K - 1, K, K + 1 candidates: both sides of the n > K branch, prefix sums over runs of empty segments."""
    from lightglue_amd import frontend

    h, w = shape
    for n in (0, 1, k - 1, k, k + 1):
        x = fr.assert_finite(fr.sparse(2, h, w, n, where, 31 * n + k))
        want = frontend.select_reference(x, k, THR, 0)
        assert want[0].tolist() == [min(n, k)] * 2
        assert_select(frontend.select(x.to(dev), k, THR, 0), want, f"sparse({n}, {where}) {h} x {w} K {k}")


def test_select_at_the_segment_cap(dev):
    """2049 x 4096: 2048 segments of 4352 pixels, segments 1929 and up start past the end of the image."""
    from lightglue_amd import frontend

    h, w = fr.CAP_SHAPE
    assert fr.seg_layout(h * w) == (2048, 4352) and fr.first_segment_past_end(h * w) == 1929
    x = fr.assert_finite(fr.sparse(1, h, w, 5000, "spread", 9))
    want = frontend.select_reference(x, 2048, THR, 0)
    assert int(want[0]) == 2048
    assert_select(frontend.select(x.to(dev), 2048, THR, 0), want, "sparse(5000, spread) at the cap")


def test_select_images_of_a_batch_are_independent(dev):
    """A dense image, an empty one and a sparse one in one call equal three single-image calls, bitwise."""
    from lightglue_amd import frontend

    h, w = 480, 640
    x = torch.cat([fr.distinct(1, h, w, 41), torch.zeros((1, h, w)), fr.sparse(1, h, w, 100, "spread", 42)])
    xd = x.to(dev)
    for k, thr, border in ((2048, 0.0, 0), (1024, THR, BORDER)):
        together = frontend.select(xd, k, thr, border)
        assert_select(together, frontend.select_reference(x, k, thr, border), f"batch of three, K {k}")
        assert int(together[0][1]) == 0 and bool((together[1][1] == -1).all()) and bool((together[2][1] == 0).all())
        for i in range(3):
            alone = frontend.select(xd[i:i + 1], k, thr, border)
            for a, b in zip(together, alone):
                assert same_bits(a[i:i + 1], b), (k, i)


def test_select_on_a_dirty_workspace(dev):
    """No state outlives a launch: a workspace of the reported size filled with 0xFF, then with 0x00, gives the
    reference's result, and a second run on what the first left behind gives it again."""
    from lightglue_amd import _lib, frontend

    h, w = 479, 641
    x = fr.levels16(2, h, w, 77)
    xd = x.to(dev)
    nbytes = _lib.load().lg_kp_select_workspace(h, w, 2)
    assert nbytes == fr.select_workspace_bytes(h, w, 2)
    for k, thr, border in ((2048, 0.0, 0), (1024, 0.5, 4)):
        want = frontend.select_reference(x, k, thr, border)
        for fill in (0xFF, 0x00):
            ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
            first = frontend.select(xd, k, thr, border, workspace=ws)
            second = frontend.select(xd, k, thr, border, workspace=ws)
            assert_select(first, want, f"workspace of {fill:#04x}, K {k}")
            for a, b in zip(first, second):
                assert same_bits(a, b), (fill, k)


# ---- b. NMS ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["distinct", "levels16"])
@pytest.mark.parametrize("radius", [1, 4])
@pytest.mark.parametrize("shape", [(480, 640), (479, 641)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_nms_at_working_size(dev, shape, radius, name):
    """15 x 20 (and 15 x 21) tiles: plateaus and suppression chains across every seam, bitwise."""
    from lightglue_amd import frontend

    h, w = shape
    x = fr.dense_map(name, 2, h, w, 300 + radius)
    want = frontend.nms_reference(x, radius)
    got = frontend.nms(x.to(dev), radius).cpu()
    assert same_bits(got, want), (name, shape, radius, int((got != want).sum()))
    assert 0 < int((want > 0).sum()) < x.numel()


# ---- c. heat map ----------------------------------------------------------------------------------------
def heat_bound(logits):
    """(float64 heat map, E): E = max |heatmap_reference in fp32 - in float64| on these logits."""
    from lightglue_amd import frontend

    exact = frontend.heatmap_reference(logits.double())
    return exact, float((frontend.heatmap_reference(logits).double() - exact).abs().max())


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("cells", [(3, 60, 80), (3, 1, 1), (3, 1, 300)], ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_heatmap_at_working_size(dev, cells, dtype):
    """14,400 cells (no multiple of 256, an image boundary inside a workgroup), one cell, one row of cells. The
    kernel may have 4 E: what the project grants another exponential and another order of the sum."""
    from lightglue_amd import frontend, synth

    b, hc, wc = cells
    logits = torch.from_numpy(synth.normal(50 + hc, (b, 65, hc, wc), 2.0)).to(dtype)
    exact, e = heat_bound(logits)
    got = frontend.heatmap(logits.to(dev))
    assert got.dtype == torch.float32 and got.shape == exact.shape
    err = float((got.cpu().double() - exact).abs().max())
    print(f"heatmap {b} x {hc} x {wc} cells {dtype}: E {e:.3e}, error {err:.3e}, error / (4 E) {err / (4 * e):.3f}")
    assert err <= 4 * e


# ---- d. describe ----------------------------------------------------------------------------------------
def describe_bound(dense, count, pix, normalized):
    """(float64 descriptors, kpts_px, fp32 kpts, E) on the tensor the kernel reads (fp16 read as fp32)."""
    from lightglue_amd import frontend

    d32 = dense.float()
    exact, kpx, _ = frontend.describe_reference(d32.double(), count, pix, normalized, compute=torch.float64)
    r32 = frontend.describe_reference(d32, count, pix, normalized)
    return exact, kpx, r32[2], float((r32[0].double() - exact).abs().max())


def check_describe(dev, dense_dev, dense_cpu, count, pix, normalized, tag):
    from lightglue_amd import frontend

    exact, kpx_want, kn32, e = describe_bound(dense_cpu, count, pix, normalized)
    k = pix.shape[1]
    valid = torch.arange(k)[None, :] < count[:, None]
    for dtype, extra in ((torch.float32, 0.0), (torch.float16, 2.0 ** -12)):
        desc, kpx, kpts = frontend.describe(dense_dev, count.to(dev), pix.to(dev), normalized, dtype)
        assert desc.dtype == dtype and kpts.dtype == dtype and kpx.dtype == torch.int32
        err = float((desc.cpu().double() - exact).abs().max())
        bound = 4 * e + extra
        print(f"describe {tag} normalized={normalized} {dtype}: E {e:.3e}, error {err:.3e}, error / bound {err / bound:.3f}")
        assert err <= bound
        assert bool((desc.cpu()[~valid] == 0).all()) and bool((kpts.cpu()[~valid] == 0).all()) and bool((kpx.cpu()[~valid] == 0).all())
        assert torch.equal(kpx.cpu(), kpx_want)
        assert same_bits(kpts.cpu(), kn32.to(dtype))


def working_size_pix(h, w, k, counts):
    """The four image corners, 128 pixels on each edge (sampling corners leave the map), random interior pixels;
    -1 past each image's count, as select leaves it."""
    g = torch.Generator().manual_seed(8)
    rows = []
    for n in counts:
        xs, ys = torch.randint(0, w, (4 * 128,), generator=g), torch.randint(0, h, (4 * 128,), generator=g)
        edges = torch.cat([xs[:128], (h - 1) * w + xs[128:256], ys[256:384] * w, ys[384:] * w + w - 1])
        corners = torch.tensor([0, w - 1, (h - 1) * w, h * w - 1])
        inner = torch.randint(1, h - 1, (k,), generator=g) * w + torch.randint(1, w - 1, (k,), generator=g)
        p = torch.cat([corners, edges, inner])[:k]
        p = p[torch.randperm(k, generator=g)]  # so that a short count still keeps corners and edges
        p[n:] = -1
        rows.append(p)
    return torch.stack(rows).int()


@pytest.fixture(scope="module")
def dense_working_size():
    from lightglue_amd import synth

    return torch.from_numpy(synth.normal(12, (3, 256, 60, 80), 1.0))


@pytest.mark.parametrize("normalized", [False, True])
@pytest.mark.parametrize("layout", ["fp16_channels_last", "fp32_nchw"])
def test_describe_at_working_size(dev, dense_working_size, layout, normalized):
    """60 x 80 cells, K = 2048, counts 2048, 1000 and 0."""
    dense = F.normalize(dense_working_size, p=2, dim=1) if normalized else dense_working_size
    count = torch.tensor([2048, 1000, 0], dtype=torch.int32)
    pix = working_size_pix(480, 640, 2048, count.tolist())
    for i in range(2):
        on_edge = (pix[i] >= 0) & ((pix[i] % 640 == 0) | (pix[i] % 640 == 639) | (pix[i] < 640) | (pix[i] >= 479 * 640))
        assert int(on_edge.sum()) > 100
    if layout == "fp16_channels_last":
        dense = dense.half()
        d = dense.to(dev).contiguous(memory_format=torch.channels_last)
        assert d.stride(1) == 1
    else:
        d = dense.to(dev)
        assert d.stride(3) == 1
    check_describe(dev, d, dense, count, pix, normalized, f"60 x 80 {layout}")


@pytest.mark.parametrize("cells", [(1, 1), (1, 3), (2, 1)], ids=lambda c: f"{c[0]}x{c[1]}")
def test_describe_on_degenerate_maps(dev, cells):
    """wc - 1 or hc - 1 is 0: the unnormalisation multiplies by 0 and every sample sits on cell row / column 0."""
    from lightglue_amd import synth

    hc, wc = cells
    h, w = hc * 8, wc * 8
    dense = torch.from_numpy(synth.normal(3, (2, 256, hc, wc), 1.0))
    pix = torch.tensor([[0, w - 1, h * w - 1, (h // 2) * w + w // 2, 5 % (h * w), -1, -1, -1]] * 2, dtype=torch.int32)
    count = torch.tensor([5, 2], dtype=torch.int32)
    pix[1, 2:] = -1
    for normalized in (False, True):
        d = F.normalize(dense, p=2, dim=1) if normalized else dense
        check_describe(dev, d.to(dev), d, count, pix, normalized, f"{hc} x {wc} cells")


def test_describe_of_all_zero_corner_cells_is_exactly_zero(dev, dense_working_size):
    from lightglue_amd import frontend

    h, w, hc, wc = 480, 640, 60, 80
    x, y = 168, 88
    ix, iy = (x - 3.5) / (w - 4.5) * (wc - 1), (y - 3.5) / (h - 4.5) * (hc - 1)
    assert 20.2 < ix < 20.8 and 10.2 < iy < 10.8  # the four corners are cells (10..11, 20..21)
    dense = dense_working_size[:1].clone()
    dense[:, :, 10:12, 20:22] = 0
    pix = torch.tensor([[y * w + x, y * w + x + 16, -1, -1, -1, -1, -1, -1]], dtype=torch.int32)
    count = torch.tensor([2], dtype=torch.int32)
    for normalized in (False, True):
        exact = frontend.describe_reference(dense.double(), count, pix, normalized, compute=torch.float64)[0]
        assert bool((exact[0, 0] == 0).all()) and float(exact[0, 1].norm()) > 0.99
        for d in (dense.to(dev), dense.half().to(dev).contiguous(memory_format=torch.channels_last)):
            for dtype in (torch.float32, torch.float16):
                desc = frontend.describe(d, count.to(dev), pix.to(dev), normalized, dtype)[0].cpu()
                assert bool((desc[0, 0] == 0).all()) and not bool(torch.isnan(desc).any())
                assert abs(float(desc[0, 1].float().norm()) - 1) < 1e-2


# ---- e. extract, each stage judged on the tensor it read -------------------------------------------------
@pytest.mark.parametrize("offset", fr.E2E_OFFSETS, ids=lambda o: f"offset{o:g}")
@pytest.mark.parametrize("k", [2048, 1024])
def test_extract_at_working_size(dev, k, offset):
    """480 x 640, two images. extract is bitwise heatmap -> nms -> select -> describe called one by one; then the
    GPU heat map against float64, nms and select bitwise on the GPU tensor each read, the descriptors against
    float64 at the selected pixels. No keypoint is left out, and the selected set never depends on how the kernel's
    heat map rounds relative to the reference's."""
    from lightglue_amd import Features, KeypointFrontend, frontend

    logits, dense = fr.e2e_logits(offset), fr.e2e_dense()
    lg = logits.to(dev)
    dn = dense.to(dev).contiguous(memory_format=torch.channels_last)
    assert dn.stride(1) == 1
    exact_heat, e_heat = heat_bound(logits)

    heat = frontend.heatmap(lg)
    nmap = frontend.nms(heat, 4)
    count, pix, score = frontend.select(nmap, k, THR, BORDER)
    heat_cpu, nmap_cpu = heat.cpu(), nmap.cpu()
    err = float((heat_cpu.double() - exact_heat).abs().max())
    print(f"extract K {k} offset {offset:g}: heat map E {e_heat:.3e}, error {err:.3e}, error / (4 E) {err / (4 * e_heat):.3f}")
    assert err <= 4 * e_heat
    assert same_bits(nmap_cpu, frontend.nms_reference(heat_cpu, 4))
    assert_select((count, pix, score), frontend.select_reference(nmap_cpu, k, THR, BORDER), f"extract K {k} offset {offset:g}")
    candidates = fr.candidate_counts(nmap_cpu, THR, BORDER)
    print(f"extract K {k} offset {offset:g}: candidates {candidates}, counts {count.tolist()}")
    if offset == fr.E2E_OFFSETS[0]:
        assert all(c > 2048 for c in candidates) and count.tolist() == [k, k]
    else:
        assert any(1 <= c <= 1023 for c in candidates) and count.tolist() == candidates

    exact, kpx_want, kn32, e_desc = describe_bound(dense, count.cpu(), pix.cpu(), False)
    for dtype, extra in ((torch.float16, 2.0 ** -12), (torch.float32, 0.0)):
        fe = KeypointFrontend(max_keypoints=k, dtype=dtype)
        desc, kpx, kpts = frontend.describe(dn, count, pix, False, dtype)
        steps = Features(kpx, kpts, desc, score, count)
        equal_results(fe.extract(lg, dn), steps, f"extract K {k} {dtype}")
        equal_results(fe.from_scores(heat, dn), steps, f"from_scores K {k} {dtype}")
        equal_results(fe.from_scores(nmap, dn, nms_done=True), steps, f"from_scores nms_done K {k} {dtype}")
        err = float((desc.cpu().double() - exact).abs().max())
        bound = 4 * e_desc + extra
        print(f"extract K {k} offset {offset:g} {dtype}: descriptors E {e_desc:.3e}, error {err:.3e}, error / bound {err / bound:.3f}")
        assert err <= bound
        assert torch.equal(kpx.cpu(), kpx_want) and same_bits(kpts.cpu(), kn32.to(dtype))
