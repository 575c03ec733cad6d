"""The front end's working-size tests, CPU side: what test_gpu_frontend_scale.py relies on, checked without a GPU.
The segment rule restated in frontend_refs.seg_layout against the library's (through lg_kp_select_workspace, which
needs no device), the fact each shape is there for, every generator's stated property, select_reference's tie
rule on the dense tie maps, and the candidate counts of the two end-to-end logit sets."""
import pytest
import torch

import frontend_refs as fr


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def test_seg_layout_is_the_librarys(lib):
    """The workspace size fixes segs * chunk (and, with the counts' padding, segs): equal for every shape used."""
    for (h, w), (pixels, segs, chunk, fact) in fr.SHAPES.items():
        assert h * w == pixels and fr.seg_layout(pixels) == (segs, chunk), (h, w, fact)
    for h, w in tuple(fr.SHAPES) + ((1, 1), (3, 5), (72, 136), (8, 8), (1, 300 * 8)):
        for b in (1, 2, 3, 65):
            if h * w * b > (1 << 30):
                continue
            got = lib.lg_kp_select_workspace(h, w, b)
            print(f"{h} x {w}, batch {b}: seg_layout {fr.seg_layout(h * w)}, workspace {got} B")
            assert got == fr.select_workspace_bytes(h, w, b), (h, w, b)


def test_the_facts_the_gpu_cases_rely_on():
    L = fr.seg_layout
    assert L(64 * 64) == (1, 4096) and fr.last_segment_pixels(64 * 64) == 4096          # one full segment
    assert L(17 * 241) == (2, 2304) and fr.last_segment_pixels(17 * 241) == 4097 - 2304  # second one partly empty
    assert L(256 * 257)[0] == fr.SEL_COPY_WAVES + 1                                     # a second trip of the copy loop
    assert L(480 * 640) == (75, 4096) and 75 * 4096 == 480 * 640                        # every chunk exactly full
    assert L(479 * 641) == (75, 4096) and fr.last_segment_pixels(479 * 641) == 3935
    assert L(2049 * 4096) == (fr.SEL_MAX_SEGS, 4352) and fr.first_segment_past_end(2049 * 4096) == 1929
    for hw in (1, 15, 4096, 4097, 65792, 307200, 307039):
        assert fr.first_segment_past_end(hw) is None
    print({f"{h}x{w}": (L(h * w), fr.last_segment_pixels(h * w), fr.first_segment_past_end(h * w)) for h, w in fr.SHAPES})


def test_no_uncapped_shape_has_a_segment_past_the_end():
    """Up to the cap segs = ceil(hw / 4096), so (segs - 1) * 4096 < hw, and chunk <= 4096 (ceil(hw / segs) <= 4096, a
    multiple of 256): the last segment starts inside the image. Checked on every size to 70,000, round every multiple
    of 4096 to the cap, and sampled; one pixel past the cap the chunk jumps to 4352 and empty segments appear."""
    cap = fr.SEL_MAX_SEGS * fr.SEL_SEG_PIXELS
    sizes = set(range(1, 70001))
    for m in range(1, fr.SEL_MAX_SEGS + 1):
        sizes.update(m * 4096 + d for d in (-257, -256, -255, -1, 0, 1, 255, 256, 257) if 0 < m * 4096 + d <= cap)
    sizes.update(torch.randint(1, cap + 1, (20000,), generator=torch.Generator().manual_seed(3)).tolist())
    for hw in sizes:
        segs, chunk = fr.seg_layout(hw)
        assert segs * chunk >= hw and chunk % 256 == 0
        assert (segs - 1) * chunk < hw and chunk <= fr.SEL_SEG_PIXELS, hw
    assert fr.first_segment_past_end(cap) is None and fr.first_segment_past_end(cap + 1) == 1928


@pytest.mark.parametrize("name", fr.DENSE_MAPS)
def test_dense_generators(name):
    h, w = 64, 65
    x = fr.assert_finite(fr.dense_map(name, 2, h, w, 5))
    assert x.dtype == torch.float32 and x.shape == (2, h, w) and bool((x > 0).all())
    assert torch.equal(x, fr.dense_map(name, 2, h, w, 5))  # the seed decides
    bits = x.view(torch.int32)
    if name == "distinct":
        assert all(torch.unique(x[i]).numel() == h * w for i in range(2)) and not torch.equal(x[0], x[1])
        assert 0.3 < float((x > 0.5).float().mean()) < 0.7
    elif name == "constant":
        assert torch.unique(x).numel() == 1 and float(x[0, 0, 0]) > 0.5
    elif name == "levels16":
        assert torch.unique(x).tolist() == [i / 16 for i in range(1, 17)]
        assert all(abs(float((x == i / 16).float().mean()) - 1 / 16) < 0.02 for i in range(1, 17))
    elif name == "wide":
        assert int(bits.min()) >= 1 and int(bits.max()) <= 0x3f800000
        top = torch.unique(bits >> 24)
        wave = bits.reshape(-1)[:64] >> 24   # one wave's first digits: more than the three a ballot round takes
        print("wide: top bytes", top.numel(), "in the first 64 pixels", torch.unique(wave).numel())
        assert top.numel() >= 60 and torch.unique(wave).numel() > 3
    else:
        assert int(bits.min()) >= 0x3f000000 and int(bits.max()) < 0x3f000000 + 4096
        assert torch.unique(bits >> 16).numel() == 1 and torch.unique(bits).numel() > 3000


@pytest.mark.parametrize("hw", [(256, 257), (480, 640)])
def test_sparse_generator(hw):
    h, w = hw
    segs, chunk = fr.seg_layout(h * w)
    for n in (0, 1, 7, 8, 9, 2047, 2048, 2049):
        for where in fr.PLACEMENTS:
            x = fr.assert_finite(fr.sparse(2, h, w, n, where, 100 + n))
            for i in range(2):
                pos = torch.nonzero(x[i].reshape(-1) > 0)[:, 0]
                vals = x[i].reshape(-1)[pos]
                assert pos.numel() == n and int((x[i] != 0).sum()) == n and torch.unique(vals).numel() == n
                if n == 0:
                    continue
                assert float(vals.min()) > 0.5 and float(vals.max()) <= 1.0
                lo, hi = fr.sparse_window(h * w, n, where)
                assert int(pos.min()) >= lo and int(pos.max()) < hi
                if where == "first":
                    assert int(pos.max()) < chunk
                elif where == "last":
                    last = (h * w - 1) // chunk
                    if fr.last_segment_pixels(h * w) >= n:
                        assert int(pos.min()) >= last * chunk
                    else:  # 256 x 257: 256 pixels in segment 16, the window reaches back by whole segments
                        assert lo % chunk == 0 and hi - (lo + chunk) < n and int(pos.max()) >= last * chunk - chunk
                else:
                    assert int(pos.max()) == h * w - 1 and (n < 2 or int(pos.min()) == 0)
                    assert n < 100 or torch.unique(pos // chunk).numel() > 16
    big = fr.sparse(1, *fr.CAP_SHAPE, 5000, "spread", 9)
    pos = torch.nonzero(big.reshape(-1) > 0)[:, 0]
    assert pos.numel() == 5000 and int(pos[0]) == 0 and int(pos[-1]) == 2049 * 4096 - 1
    assert int(pos.max()) // 4352 == 1928  # the last segment that holds pixels holds a candidate


def _check_tie_rule(x, k, thr, border):
    """test_select_reference_tie_rule's first principles on any map."""
    from lightglue_amd import frontend

    count, pix, score = frontend.select_reference(x, k, thr, border)
    b, h, w = x.shape
    inner = torch.zeros((h, w), dtype=torch.bool)
    if h > 2 * border and w > 2 * border:
        inner[border:h - border, border:w - border] = True
    for i in range(b):
        n = int(count[i])
        p, s = pix[i, :n].long(), score[i, :n]
        flat = x[i].reshape(-1)
        assert torch.equal(flat[p], s)
        assert bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (p[:-1] < p[1:]))).all())
        assert bool(inner.reshape(-1)[p].all()) and bool((s > thr).all())
        rest = flat.clone()
        rest[p] = 0
        left = (rest > thr) & inner.reshape(-1)
        if bool(left.any()):  # nothing left out beats the last one kept, and an equal one has a higher index
            assert n == k and float(rest[left].max()) <= float(s[-1])
            eq = torch.nonzero(left & (rest == s[-1]))[:, 0]
            assert eq.numel() == 0 or int(eq.min()) > int(p[s == s[-1]].max())
        else:
            assert n == min(k, int(((flat > thr) & inner.reshape(-1)).sum()))
        assert bool((pix[i, n:] == -1).all()) and bool((score[i, n:] == 0).all())
    return count, pix, score


def test_select_reference_on_constant_and_levels16():
    """constant: the first K row-major pixels inside the border. levels16: the tie rule from first principles, with
    the K cut inside a run of equal scores."""
    for h, w in ((64, 64), (17, 241), (479, 641)):
        for k, border in ((2048, 0), (1024, 4), (8, 4)):
            c = fr.constant(2, h, w)
            count, pix, score = _check_tie_rule(c, k, 0.5, border)
            ys, xs = torch.meshgrid(torch.arange(border, h - border), torch.arange(border, w - border), indexing="ij")
            want = (ys * w + xs).reshape(-1)[:k].int()
            assert count.tolist() == [want.numel()] * 2
            assert torch.equal(pix[:, :want.numel()], want.expand(2, -1)) and bool((score[:, :want.numel()] == 0.75).all())
            q = fr.levels16(2, h, w, 21)
            count, pix, score = _check_tie_rule(q, k, 0.0, border)
            n = int(count[0])
            tied = int((q[0] == score[0, n - 1]).sum())
            print(f"levels16 {h} x {w}, K {k}, border {border}: cut at level {float(score[0, n - 1])}, {tied} pixels hold it")
            assert n < k or tied > int((score[0] == score[0, n - 1]).sum())  # the cut leaves equal scores out
    for name in ("wide", "near"):
        _check_tie_rule(fr.dense_map(name, 1, 256, 257, 4), 1024, 0.5, 4)


def test_end_to_end_candidate_counts():
    """The two logit sets of test_gpu_frontend_scale's extract case (480 x 640, radius 4, threshold 0.0005, border 4):
    every image of the first has more than 2048 candidates (the radix select runs at K = 2048 and 1024), an image of
    the second between 1 and 1023 (padded rows at both K)."""
    from lightglue_amd import frontend

    counts = {}
    for off in (0.0, 13.0) + fr.E2E_OFFSETS[1:]:
        nmap = frontend.nms_reference(frontend.heatmap_reference(fr.e2e_logits(off)), 4)
        counts[off] = fr.candidate_counts(nmap)
        f = frontend.frontend_reference(fr.e2e_logits(off), fr.e2e_dense(), max_keypoints=2048)
        assert f.counts.tolist() == [min(c, 2048) for c in counts[off]]
        print(f"offset {off} on channel 64: candidates {counts[off]}")
    assert counts[0.0] == [7153, 7112] and counts[13.0] == [2274, 2186]
    assert all(c > 2048 for c in counts[fr.E2E_OFFSETS[0]])
    assert any(1 <= c <= 1023 for c in counts[fr.E2E_OFFSETS[1]])
    assert all(c >= 1 for c in counts[fr.E2E_OFFSETS[1]])


def test_describe_reference_on_degenerate_maps():
    """Maps of 1 x 1, 1 x 3 and 2 x 1 cells (wc - 1 or hc - 1 is 0): the float64 reference gives finite descriptors,
    unit where a sampling corner carries weight."""
    from lightglue_amd import frontend, synth

    for hc, wc in ((1, 1), (1, 3), (2, 1)):
        d = torch.from_numpy(synth.normal(3, (1, 256, hc, wc), 1.0)).double()
        h, w = hc * 8, wc * 8
        pix = torch.tensor([[0, w - 1, h * w - 1, (h // 2) * w + w // 2, 0, 0, 0, 0]], dtype=torch.int32)
        out = frontend.describe_reference(d, torch.tensor([4], dtype=torch.int32), pix, False, compute=torch.float64)[0]
        norm = out.norm(dim=-1)[0]
        print(f"{hc} x {wc} cells: norms {norm[:4].tolist()}")
        assert bool(torch.isfinite(out).all()) and bool(((norm[:4] - 1).abs() < 1e-12).all()) and bool((norm[4:] == 0).all())
