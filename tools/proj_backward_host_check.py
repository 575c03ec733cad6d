"""The fused projections' backward restated on the CPU in framework ops, with the kernels' rounding points
(csrc/lightglue_proj_backward.hip): fp16 operands; G, the gradient in W's row order, rounded once to fp16 (the
transposed rotary of the q and k parts and the head's fp32 gradient; the other parts are copies); fp32 sums (the column
sums in the kernels' order: col_sum); dx one rounding.

Writes, per kind, case and tensor, max|x - ref| / max|ref| against float64 autograd of the unfused projection (F.linear,
layers._rotary, the head split) on sum(grad * output), then the worst per kind and tensor, to
profiles/proj_backward/host_check.txt: tests/test_gpu_proj_backward.py takes four times those as its bounds.

    python tools/proj_backward_host_check.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))

from lightglue_amd.layers import _rotary  # noqa: E402

SPLIT_ROWS, SPLITS, ROWS_WG = 256, 32, 64  # proj_bw_splits: one split per 256 rows, 32 at the most; rows per workgroup
KINDS = {"split2": 1, "qkv": 2, "plain": 3}  # LG_PROJ_*
WIDTH = {"split2": 512, "qkv": 768, "plain": 384}
LD = 384  # the head's rows (lg_assign_nll's dv)

# name -> (pairs, n0, n1)
CASES = {
    "one_row": (1, 1, 1),        # a single partial tile, both images
    "empty_image": (1, 0, 5),    # an image with no rows: its gradients are null pointers
    "tile": (1, 33, 40),         # the image boundary and a 64-row boundary inside the pair, a partial last tile
    "pairs": (3, 70, 72),        # pair boundaries inside tiles, n0 != n1; S 2
    "unsplit": (1, 120, 136),    # 256 rows: the last count with S 1
    "split": (1, 128, 129),      # 257 rows: S 2, 9 tiles of 32 as 5 + 4, one row in the last
}
NAMES = ("dx", "dw", "db")


def splits(m):
    """The host rule (proj_bw_splits)."""
    return max(1, min(SPLITS, (m + SPLIT_ROWS - 1) // SPLIT_ROWS))


def workspace_bytes(kind, m):
    """lg_proj_backward_workspace: the packed stream, G, the column partials, the split partials."""
    up = lambda v: (v + 255) // 256 * 256  # noqa: E731
    n = WIDTH[kind]
    return 0 if m <= 0 else up(n * 512) + up(m * n * 2) + up((m + ROWS_WG - 1) // ROWS_WG * n * 4) + splits(m) * n * 1024


def operands(kind, name):
    """Seeded Gaussians: x [1, M, 256] at unit scale, w [n, 256] at 1 / sqrt(256), b, dx_add, the gradients at 2^-4
    (fp16; head-major [P, 4, ni, 64] per output, or the head's fp32 [M, 384]), cos / sin [1, M, 64] of random angles,
    each repeated over its rotary pair -> dict (grads: a list in the kernel's order)."""
    pr, n0, n1 = CASES[name]
    m, n = pr * (n0 + n1), WIDTH[kind]
    g = torch.Generator().manual_seed(2000 + 10 * KINDS[kind] + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(x=rn(1, m, 256).half(), w=(rn(n, 256) / 16).half(), b=(0.1 * rn(n)).half(), dx_add=(rn(1, m, 256) / 16).half())
    head = lambda ni: (rn(pr, 4, ni, 64) / 16).half()  # noqa: E731
    if kind == "qkv":
        ang = 6.0 * rn(1, m, 32)
        t["cos"], t["sin"] = (f(ang).repeat_interleave(2, -1).half() for f in (torch.cos, torch.sin))
        t["grads"] = [head(ni) for ni in (n0, n0, n0, n1, n1, n1)]
    elif kind == "split2":
        t["grads"] = [head(ni) for ni in (n0, n1, n0, n1)]
    else:
        t["grads"] = [rn(m, LD) / 16]
    return t


def merge(g0, g1):
    """merge_heads of both images' head-major tensors, pair-major rows [M, 256]."""
    rows = [c[p].transpose(0, 1).reshape(c.shape[2], 256) for p in range(g0.shape[0]) for c in (g0, g1)]
    return torch.cat(rows, 0)


def row_grads(kind, t):
    """The incoming gradients as rows [M, 256] per part, in W's part order."""
    g = t["grads"]
    if kind == "qkv":
        return [merge(g[j], g[3 + j]) for j in range(3)]
    return [merge(g[0], g[1]), merge(g[2], g[3])] if kind == "split2" else [g[0][:, :WIDTH[kind]]]


def reference(kind, t):
    """float64 autograd of sum(grad * output) of the unfused projection -> (dx [M, 256], dw, db)."""
    x, w, b = (t[k].double().requires_grad_() for k in ("x", "w", "b"))
    y = F.linear(x[0], w, b)
    parts = list(y.split(256, 1)) if kind != "plain" else [y]
    if kind == "qkv":
        c, s = t["cos"][0].double()[:, None], t["sin"][0].double()[:, None]
        parts[:2] = [_rotary(p.view(-1, 4, 64), c, s).reshape(-1, 256) for p in parts[:2]]
    sum((g.double() * p).sum() for g, p in zip(row_grads(kind, t), parts)).backward()
    return x.grad[0], w.grad, b.grad


def col_sum(v):
    """The column sums as the rows kernel and the reduce add them: 16 rows per MFMA step, the steps of a 64-row
    workgroup added in fp32 in order, then the workgroups in fp64."""
    pad = torch.cat((v, v.new_zeros(((-v.shape[0]) % ROWS_WG, v.shape[1]))), 0)
    steps = pad.view(-1, ROWS_WG // 16, 16, v.shape[1]).double().sum(2).float()   # [workgroups, 4, C]
    total = v.new_zeros(v.shape[1]).double()
    for wg in steps:
        part = v.new_zeros(v.shape[1])
        for step in wg:
            part = part + step
        total = total + part.double()
    return total.float()


def gathered(kind, t):
    """G [M, n] as the rows kernel's prologue leaves it in LDS: fp16 values, here in fp32."""
    parts = [g.float() for g in row_grads(kind, t)]
    if kind == "qkv":
        c, s = (t[k][0].float().repeat(1, 4) for k in ("cos", "sin"))
        for j in range(2):  # (g0, g1) -> (g0 c0 + g1 s1, g1 c1 - g0 s0), one rounding
            g0, g1 = parts[j][:, 0::2], parts[j][:, 1::2]
            o = torch.stack((g0 * c[:, 0::2] + g1 * s[:, 1::2], g1 * c[:, 1::2] - g0 * s[:, 0::2]), -1)
            parts[j] = o.flatten(-2)
    return torch.cat(parts, 1).half().float()


def emulated(kind, t, dx_add=False):
    """The kernels' arithmetic in fp32 with their roundings -> (dx fp16, dw, db)."""
    G, x = gathered(kind, t), t["x"][0].float()
    dx = G @ t["w"].float()[:G.shape[1]]
    return (dx + t["dx_add"][0].float() if dx_add else dx).half(), G.T @ x, col_sum(G)


def rel(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def main():
    lines = []
    for kind in KINDS:
        worst = {}
        for name, shape in CASES.items():
            t = operands(kind, name)
            errs = [rel(a, r) for a, r in zip(emulated(kind, t), reference(kind, t))]
            for k, e in zip(NAMES, errs):
                worst[k] = max(worst.get(k, 0.0), e)
            m = shape[0] * (shape[1] + shape[2])
            lines.append(f"{kind:<6} {name:<11} {shape[0]}x({shape[1]}+{shape[2]}) S {splits(m):<2} " +
                         "  ".join(f"{k} {e:.3e}" for k, e in zip(NAMES, errs)))
        for k in NAMES:  # (rounded up, so that the printed figure bounds the computed one)
            exp = int(np.floor(np.log10(worst[k])))
            lines.append(f"worst {kind} {k} {np.ceil(worst[k] / 10.0 ** exp * 1000) / 1000:.3f}e{exp:+03d}")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.join(REPO, "profiles", "proj_backward"), exist_ok=True)
    with open(os.path.join(REPO, "profiles", "proj_backward", "host_check.txt"), "w") as f:
        f.write(text)
    print(text, end="")


if __name__ == "__main__":
    main()
