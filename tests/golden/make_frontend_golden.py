"""Golden fixtures for the keypoint front end (lightglue_amd/frontend.py, csrc/lightglue_frontend.hip).

    python tests/golden/make_frontend_golden.py --reference <checkout of the reference project>

Runs on the CPU. Imports the reference's ``simple_nms`` and ``sample_descriptors`` from
``lightglue_pytorch_no_plugin/superpoint.py`` by path (the module needs only torch; ``SuperPoint()`` is never
constructed) and restates ``SuperPointMonoTRT::PostProcess`` (demo/superpoint_mono_trt.cpp:153-253) in torch,
line by line. Writes ``frontend_<Hc>x<Wc>.npz``: seeded inputs and the reference's outputs of every stage on
that stage's own input, plus the reference's fp32 error against fp64 where a test's tolerance derives from it.

Shapes (the smallest that can still go wrong): 8x8 cells (64 x 64 px: two 32 x 32 NMS tiles each way, image 1
with no candidate at all), 9x17 (72 x 136: two / four tiles and a remainder of 8) and 11x10 (88 x 80: two tiles
and remainders of 24 and 16). B = 2. K_main is a multiple of 8 strictly between the two images' candidate
counts. Seeds are searched until the conditions of ``check_conditions`` hold; tests re-check them from the
file.
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

THRESHOLD = 0.0005
RADIUS = 4
BORDER = 4
GAP_FACTOR = 64.0  # the end-to-end gaps, in units of the reference's own fp32 heatmap error
# name: (Hc, Wc, first seed tried)
SHAPES = {"8x8": (8, 8, 100), "9x17": (9, 17, 200), "11x10": (11, 10, 300)}


def heat_from_logits(logits: torch.Tensor) -> torch.Tensor:
    """superpoint.py:160-165 (softmax, dustbin dropped, 8 x 8 depth-to-space), in the logits' dtype."""
    b, _, hc, wc = logits.shape
    s = torch.softmax(logits, 1)[:, :-1]
    return s.permute(0, 2, 3, 1).reshape(b, hc, wc, 8, 8).permute(0, 1, 3, 2, 4).reshape(b, hc * 8, wc * 8)


def others_max(x: torch.Tensor, radius: int) -> torch.Tensor:
    """[H, W] -> the maximum of each pixel's (2r+1)^2 window without the pixel itself (-inf padding)."""
    k = 2 * radius + 1
    cols = F.unfold(F.pad(x[None, None], (radius,) * 4, value=float("-inf")), k)[0]  # [k*k, H*W]
    cols[k * k // 2] = float("-inf")
    return cols.max(0).values.reshape(x.shape)


def e2e_gaps(heat: torch.Tensor, k: int, radius: int = RADIUS, threshold: float = THRESHOLD, border: int = BORDER):
    """The three margins that make the selected set robust to a perturbation of the heatmap (each must be
    >= GAP_FACTOR x the reference's fp32 error): (a) every NMS survivor's distance from the threshold, (b) the
    gap between the K-th and (K+1)-th candidate, (c) at each of simple_nms' three equality tests, every
    unsuppressed pixel's distance from the best other value in its window (a local maximum's lead over its
    runner-up, and every other pixel's deficit)."""
    inf = float("inf")
    thr_gap, cut_gap, lead = inf, inf, inf
    for img in heat:
        h, w = img.shape
        if float(img.max()) < threshold / 2:  # no candidate whatever the NMS keeps (the empty image)
            continue
        keep = torch.zeros_like(img, dtype=torch.bool)
        near = torch.zeros_like(img, dtype=torch.bool)
        for _ in range(3):
            rest = img.masked_fill(near, 0.0)
            d = (rest - others_max(rest, radius)).abs()
            lead = min(lead, float(d[~near].min()))
            keep = keep | ((rest >= others_max(rest, radius)) & ~near)
            near = F.max_pool2d(keep[None, None].float(), 2 * radius + 1, 1, radius)[0, 0] > 0
        inner = torch.zeros_like(keep)
        inner[border:h - border, border:w - border] = True
        v = img[keep & inner]
        thr_gap = min(thr_gap, float((v - threshold).abs().min()))
        c = torch.sort(v[v > threshold], descending=True).values
        if c.numel() > k:
            cut_gap = min(cut_gap, float(c[k - 1] - c[k]))
    return thr_gap, cut_gap, lead


def candidates(nms_map: torch.Tensor, border: int, threshold: float = THRESHOLD) -> torch.Tensor:
    """One image's candidate scores (unordered)."""
    h, w = nms_map.shape
    inner = torch.zeros_like(nms_map, dtype=torch.bool)
    inner[border:h - border, border:w - border] = True
    return nms_map[inner & (nms_map > threshold)]


def check_conditions(g) -> None:
    """What the generator asserts about a fixture (g: the .npz as a dict of arrays), from its data alone."""
    heat = torch.from_numpy(g["heat32"])
    nms4 = torch.from_numpy(g["nms_r4"])
    k = int(g["k_main"])
    err = float(g["heat_err"])
    assert 0 < err < 1e-7
    counts = []
    for border in (0, BORDER):
        for i in range(heat.shape[0]):
            c = candidates(nms4[i], border)
            assert torch.unique(c).numel() == c.numel(), "candidate scores are not distinct"
            if border == BORDER:
                counts.append(int(c.numel()))
    assert min(counts) < k < max(counts) and k % 8 == 0, (counts, k)
    assert list(g[f"sel_b{BORDER}_k{k}_count"]) == [min(c, k) for c in counts]
    if bool(g["has_empty_image"]):
        assert 0 in counts
    gaps = e2e_gaps(heat, k)
    assert all(x >= GAP_FACTOR * err for x in gaps), (gaps, err)
    # the quantised map's K cut falls inside a run of equal scores (image 0)
    q = torch.from_numpy(g["q64_nms_r4"])[0]
    c = torch.sort(candidates(q, BORDER), descending=True).values
    tk = int(g["tie_k"])
    assert tk % 8 == 0 and c.numel() > tk and c[tk - 1] == c[tk]
    # border 0 puts sampling corners outside the descriptor map
    assert (g[f"sel_b0_k{k}_pix"][g[f"sel_b0_k{k}_pix"] >= 0] % heat.shape[2] < 4).any()


def post_process(nms_map, dense_n, k, border, sample_descriptors, threshold=THRESHOLD):
    """SuperPointMonoTRT::PostProcess for one image: nms_map [H, W] fp32, dense_n [256, Hc, Wc] fp32 already
    normalised (superpoint.py:173). -> (n, kpts_px [n, 2] (x, y), kpts [n, 2], desc [n, 256], scores [n])."""
    h, w = nms_map.shape
    s = nms_map.clone()
    if border:  # :167-194 (the reference's 4)
        s[:border, :] = -1.0
        s[:, :border] = -1.0
        s[h - border:, :] = -1.0
        s[:, w - border:] = -1.0
    mask = s > threshold                                                      # :196
    rc = mask.nonzero().to(torch.int32)                                       # :197 (row, col)
    vals = s.view(-1).index_select(0, mask.view(-1).nonzero().squeeze(1))     # :199-202
    if vals.numel() == 0:                                                     # :204-211
        z = torch.zeros
        return 0, z((0, 2), dtype=torch.int32), z((0, 2)), z((0, 256)), z((0,))
    kk = min(vals.numel(), k)                                                 # :213
    top, idx = torch.topk(vals, kk, 0, True, True)                            # :214
    kp = rc.index_select(0, idx).flip(1).to(torch.int32)                      # :217 (x, y)
    desc = sample_descriptors(kp.float()[None], dense_n[None], 8)[0].t()      # :219-236 (superpoint.py:72-87)
    shift = torch.tensor([w / 2.0, h / 2.0])
    kn = (kp.float() - shift) / (max(w, h) / 2.0)                             # :238-245
    return kk, kp, kn, desc.contiguous(), top


def special_maps(h: int, w: int, seed: int):
    """[3, H, W]: a constant map, one whose maxima sit in the first and last rows and columns, and one of
    plateaus touching the edges."""
    gen = torch.Generator().manual_seed(seed)
    const = torch.full((h, w), 0.25)
    edge = torch.floor(torch.rand((h, w), generator=gen) * 256) / 1024
    for y, x in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h - 1, w // 3), (h // 2, 0), (h // 3, w - 1),
                 (0, 5), (0, 7), (h - 1, w - 6), (5, 0), (h - 2, w - 1)):
        edge[y, x] = 1.0 + float(torch.rand((), generator=gen))
    plat = torch.floor(torch.rand((h, w), generator=gen) * 4) / 4
    plat[:3, :] = 1.0
    plat[:, w - 2:] = 1.0
    return torch.stack([const, edge, plat])


def build(name: str, sp) -> dict:
    hc, wc, seed0 = SHAPES[name]
    h, w = hc * 8, wc * 8
    empty = name == "8x8"
    for seed in range(seed0, seed0 + 200):
        gen = torch.Generator().manual_seed(seed)
        logits = torch.randn((2, 65, hc, wc), generator=gen)
        if empty:
            logits[1, 64] += 30.0  # image 1: everything in the dustbin, no score above the threshold
        heat32 = heat_from_logits(logits)
        heat_err = float((heat32.double() - heat_from_logits(logits.double())).abs().max())
        nms4 = sp.simple_nms(heat32, RADIUS)
        counts = [int(candidates(nms4[i], BORDER).numel()) for i in range(2)]
        ks = [k for k in range(8, 2048, 8) if min(counts) < k < max(counts)]
        if not ks:
            continue
        k = ks[len(ks) // 2]
        distinct = all(torch.unique(candidates(nms4[i], b)).numel() == candidates(nms4[i], b).numel()
                       for i in range(2) for b in (0, BORDER))
        if not distinct or min(e2e_gaps(heat32, k)) < GAP_FACTOR * heat_err:
            continue
        break
    else:
        raise SystemExit(f"{name}: no seed satisfies the conditions")
    g = {"seed": np.int64(seed), "logits": logits.numpy(), "heat32": heat32.numpy(), "heat_err": np.float64(heat_err),
         "k_main": np.int32(k), "has_empty_image": np.bool_(empty), "nms_r1": sp.simple_nms(heat32, 1).numpy(),
         "nms_r4": nms4.numpy()}
    # quantised maps: plateaus and suppression chains
    for levels in (32, 64):
        lv = torch.floor(torch.rand((2, h, w), generator=gen) * levels).to(torch.uint8)
        q = lv.float() / levels
        g[f"q{levels}_levels"] = lv.numpy()
        for r in (0, 1, 4):
            g[f"q{levels}_nms_r{r}"] = sp.simple_nms(q, r).numpy()
    sm = special_maps(h, w, seed)
    g["special"] = sm.numpy()
    for r in (0, 1, 4):
        g[f"special_nms_r{r}"] = sp.simple_nms(sm, r).numpy()
    c = torch.sort(candidates(torch.from_numpy(g["q64_nms_r4"])[0], BORDER), descending=True).values
    ties = [t for t in range(8, min(int(c.numel()), 2048), 8) if c[t - 1] == c[t]]
    assert ties, "no K cut inside a run of equal scores"
    g["tie_k"] = np.int32(ties[len(ties) // 2])
    # select and describe on the reference's NMS map
    dense = torch.randn((2, 256, hc, wc), generator=gen).half()
    g["dense"] = dense.numpy()
    dn = F.normalize(dense.float(), p=2, dim=1)  # superpoint.py:173
    sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))
    from lightglue_amd.frontend import describe_reference

    desc_err = np.zeros((2, 2))  # [border 0 / BORDER][raw / normalised dense input]
    for border, kk in ((BORDER, k), (0, k), (BORDER, 8), (BORDER, 2048)):
        count = np.zeros((2,), np.int32)
        pix = np.full((2, kk), -1, np.int32)
        score = np.zeros((2, kk), np.float32)
        desc = torch.zeros((2, kk, 256))
        for i in range(2):
            n, kp, _, d, top = post_process(nms4[i], dn[i], kk, border, sp.sample_descriptors)
            count[i], pix[i, :n], score[i, :n] = n, (kp[:, 1] * w + kp[:, 0]).numpy(), top.numpy()
            desc[i, :n] = d
        tag = f"sel_b{border}_k{kk}"
        g[tag + "_count"], g[tag + "_pix"], g[tag + "_score"] = count, pix, score
        if kk == k:  # the reference's fp32 descriptors against the fp64 restatement, on both forms of the input
            ct, px = torch.from_numpy(count), torch.from_numpy(pix)
            raw64 = describe_reference(dense.double(), ct, px, False, compute=torch.float64)[0]
            nrm64 = describe_reference(dn.double(), ct, px, True, compute=torch.float64)[0]
            bi = 0 if border == 0 else 1
            desc_err[bi, 0] = float((desc.double() - raw64).abs().max())
            desc_err[bi, 1] = float((desc.double() - nrm64).abs().max())
    g["desc_err"] = desc_err
    check_conditions(g)
    return g


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("names", nargs="*", default=sorted(SHAPES))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location(
        "ref_superpoint", os.path.join(args.reference, "lightglue_pytorch_no_plugin", "superpoint.py"))
    sp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sp)
    torch.set_num_threads(1)  # (one summation order whatever the host)
    for name in args.names:
        g = build(name, sp)
        path = os.path.join(HERE, f"frontend_{name}.npz")
        np.savez_compressed(path, **g)
        print(f"{name}: seed {int(g['seed'])}, K_main {int(g['k_main'])}, tie K {int(g['tie_k'])}, counts "
              f"{list(g['sel_b%d_k2048_count' % BORDER])}, heat_err {float(g['heat_err']):.3e}, desc_err "
              f"{g['desc_err'].tolist()}, {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
