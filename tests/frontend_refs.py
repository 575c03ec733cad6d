"""What the front end's working-size tests share (test_frontend_scale_reference.py, test_gpu_frontend_scale.py):
lg_kp_select's segment rule restated, the shapes the tests use with the fact each one is there for, seeded
score-map generators, and the logits / descriptors of the end-to-end case. A plain module: no fixtures.

Every map is a CPU fp32 [B, H, W] tensor made from a torch.Generator seed; none holds a NaN or an Inf (select's
order among those is not pinned by these tests). The oracles are lightglue_amd.frontend's *_reference stages."""
import numpy as np
import torch

SEL_SEG_PIXELS = 4096   # lg_kp_select aims at segments of this many pixels ...
SEL_MAX_SEGS = 2048     # ... and never cuts an image into more than this many
SEL_COPY_WAVES = 16     # kp_select_kernel: 1024 threads, one wave per segment and trip


def seg_layout(hw):
    """(segs, chunk) of csrc/lightglue_frontend.hip's seg_layout: segs = clamp(ceil(hw / 4096), 1, 2048),
    chunk = ceil(hw / segs) rounded up to a multiple of 256."""
    segs = min(max(-(-hw // SEL_SEG_PIXELS), 1), SEL_MAX_SEGS)
    chunk = -(-(-(-hw // segs)) // 256) * 256
    return segs, chunk


def select_workspace_bytes(h, w, b):
    """lg_kp_select_workspace from seg_layout: the counts (padded to 256 B), the segments' key slices, the lists."""
    segs, chunk = seg_layout(h * w)
    return ((b * segs * 4 + 255) & ~255) + b * segs * chunk * 8 + b * h * w * 8


def first_segment_past_end(hw):
    """The first segment that starts at or past hw (it holds no pixel), or None."""
    segs, chunk = seg_layout(hw)
    return next((s for s in range(segs) if s * chunk >= hw), None)


def last_segment_pixels(hw):
    """How many pixels the last segment that holds any holds."""
    _, chunk = seg_layout(hw)
    return hw - (hw - 1) // chunk * chunk


# (h, w): (pixels, segs, chunk, the fact the GPU cases rely on)
SHAPES = {
    (64, 64): (4096, 1, 4096, "one full segment"),
    (17, 241): (4097, 2, 2304, "second segment partly empty"),
    (256, 257): (65792, 17, 4096, "one more segment than the 16 copying waves"),
    (480, 640): (307200, 75, 4096, "every chunk exactly full when every pixel is a candidate"),
    (479, 641): (307039, 75, 4096, "last segment holds 3,935 pixels"),
    (2049, 4096): (8392704, 2048, 4352, "first segment wholly past the end is 1929"),
}
CAP_SHAPE = (2049, 4096)
SELECT_SHAPES = ((1, 1), (3, 5)) + tuple(s for s in SHAPES if s != CAP_SHAPE)
DENSE_MAPS = ("distinct", "constant", "levels16", "wide", "near")
PLACEMENTS = ("first", "last", "spread")


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _distinct_values(n, gen, lo_half):
    """n pairwise distinct positive fp32 values in random order: (a permutation of 1..n) * 2^-p, every one exact.
    lo_half False: p = floor(log2 n), values in (0, 2). lo_half True: 1/2 is added, p such that they stay in (1/2, 1]."""
    if n == 0:
        return torch.zeros((0,), dtype=torch.float32)
    assert n < (1 << 23)
    ranks = (torch.randperm(n, generator=gen) + 1).to(torch.float64)
    if lo_half:
        v = 0.5 + ranks * 2.0 ** -(n.bit_length() + 1)
    else:
        v = ranks * 2.0 ** -(n.bit_length() - 1)
    out = v.to(torch.float32)
    assert torch.equal(out.to(torch.float64), v) and bool((out > 0).all())
    return out


def distinct(b, h, w, seed):
    """Positive, pairwise distinct scores per image (asserted), about half of them above 0.5."""
    g = _gen(seed)
    x = torch.stack([_distinct_values(h * w, g, False) for _ in range(b)]).reshape(b, h, w)
    for i in range(b):
        assert torch.unique(x[i]).numel() == h * w and bool((x[i] > 0).all())
    return x


def constant(b, h, w, seed=0, value=0.75):
    return torch.full((b, h, w), value, dtype=torch.float32)


def levels16(b, h, w, seed):
    """floor(16 u + 1) / 16: sixteen levels 1/16 .. 1, about 1/16 of the map tied at each."""
    return torch.floor(torch.rand((b, h, w), generator=_gen(seed)) * 16 + 1) / 16


def wide(b, h, w, seed):
    """Uniformly random positive bit patterns in [1, 0x3f800000]: subnormals to 1.0, about 64 different top bytes."""
    bits = torch.randint(1, 0x3f800000 + 1, (b, h, w), generator=_gen(seed), dtype=torch.int64)
    return bits.to(torch.int32).view(torch.float32)


def near(b, h, w, seed):
    """Bits 0x3f000000 + randint(0, 4096): the keys agree in their top bytes; the low score bytes and the pixel decide."""
    bits = 0x3f000000 + torch.randint(0, 4096, (b, h, w), generator=_gen(seed), dtype=torch.int64)
    return bits.to(torch.int32).view(torch.float32)


def sparse_window(hw, n, where):
    """[lo, hi): the pixels a placement draws from. first: segment 0. last: the last segment that holds pixels,
    grown backwards by whole segments while it holds fewer than n pixels (256 x 257's holds 256). spread: the map."""
    _, chunk = seg_layout(hw)
    if where == "first":
        lo, hi = 0, min(chunk, hw)
    elif where == "last":
        lo, hi = (hw - 1) // chunk * chunk, hw
        while hi - lo < n and lo > 0:
            lo -= chunk
    else:
        assert where == "spread"
        lo, hi = 0, hw
    assert hi - lo >= n, (hw, n, where)
    return lo, hi


def sparse(b, h, w, n, where, seed):
    """Exactly n positive, pairwise distinct pixels (in (1/2, 1]) per image and the rest 0. spread: pixel h*w - 1 is
    among them, and pixel 0 too from n = 2 on."""
    hw = h * w
    lo, hi = sparse_window(hw, n, where)
    g = _gen(seed)
    x = torch.zeros((b, hw), dtype=torch.float32)
    for i in range(b):
        if where == "spread":
            fixed = [hw - 1, 0][:n] if hw > 1 else [0][:n]
            m = n - len(fixed)
            if m > 0:  # distinct draws from 1 .. hw - 2: oversample, drop repeats, keep the first m in draw order
                draw = torch.randint(1, hw - 1, (2 * m + 64,), generator=g)
                _, first = np.unique(draw.numpy(), return_index=True)
                rest = draw[torch.from_numpy(np.sort(first))][:m]
                assert rest.numel() == m
            else:
                rest = torch.zeros((0,), dtype=torch.int64)
            pos = torch.cat([torch.tensor(fixed, dtype=torch.int64), rest])
        else:
            pos = lo + torch.randperm(hi - lo, generator=g)[:n]
        assert pos.numel() == n and torch.unique(pos).numel() == n
        x[i, pos] = _distinct_values(n, g, True)
        assert int((x[i] > 0).sum()) == n
    return x.reshape(b, h, w)


def dense_map(name, b, h, w, seed):
    return {"distinct": distinct, "constant": constant, "levels16": levels16, "wide": wide, "near": near}[name](b, h, w, seed)


def assert_finite(x):
    assert bool(torch.isfinite(x).all())
    return x


# ---- the end-to-end case: 480 x 640, two logit sets --------------------------------------------------
E2E_CELLS = (60, 80)
E2E_OFFSETS = (0.0, 15.0)   # added to channel 64 (the "no keypoint" bin): the second leaves an image under 1024


def e2e_logits(offset):
    """synth.normal(7, (2, 65, 60, 80), 2.0) with `offset` added to channel 64, fp32."""
    from lightglue_amd import synth

    x = torch.from_numpy(synth.normal(7, (2, 65) + E2E_CELLS, 2.0)).clone()
    x[:, 64] += offset
    return x


def e2e_dense():
    """fp16 descriptors [2, 256, 60, 80] of std 1 (channels-last is the caller's choice)."""
    from lightglue_amd import synth

    return torch.from_numpy(synth.normal(11, (2, 256) + E2E_CELLS, 1.0)).half()


def candidate_counts(nms_map, threshold=0.0005, border=4):
    """Candidates per image: inside the border and above the threshold."""
    b, h, w = nms_map.shape
    inner = torch.zeros((h, w), dtype=torch.bool)
    if h > 2 * border and w > 2 * border:
        inner[border:h - border, border:w - border] = True
    return [int(((nms_map[i] > threshold) & inner).sum()) for i in range(b)]
