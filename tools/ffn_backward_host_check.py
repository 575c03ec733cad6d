"""The FFN backward's arithmetic restated on the CPU in framework ops, with the kernels' rounding points
(csrc/lightglue_ffn_backward.hip): fp16 operands; a and g rounded to fp16 as the forward rounds them; fp32 statistics,
GELU derivative and row means; da rounded to fp16 where it becomes the operand of dc, dW1 and db1; du and du n rounded
to fp16 where they become the operands of dbeta's and dgamma's sums; dx one rounding of dy + dc; fp32 sums (the
column sums in the kernels' order: col_sum).

Prints, per case and per tensor, max|x - ref| / max|ref| against float64 autograd of the unrounded formula (F.linear,
F.layer_norm, F.gelu, the residual), then the worst per tensor: tests/test_gpu_ffn_backward.py takes four times those
as its bounds. Output kept as profiles/ffn_backward/host_check.txt.

    python tools/ffn_backward_host_check.py > profiles/ffn_backward/host_check.txt
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
SPLIT_ROWS, SPLITS, ROWS_WG = 320, 20, 64  # ffn_bw_splits: one split up to 320 rows, twenty beyond; rows per workgroup

# name -> (pairs, n0, n1), with S the weight kernel's split of the rows (tiles of 32) and the rows kernel's 64-row
# workgroups:
CASES = {
    "one_row": (1, 1, 1),      # S 1: one row per image, a single partial tile
    "tile": (1, 33, 40),       # S 1: the image boundary and a 64-row boundary inside the pair, a partial last tile
    "pairs": (3, 70, 72),      # S 20 (14 tiles, one a split, the last splits empty): pair boundaries inside tiles
    "unsplit": (1, 150, 170),  # 320 rows: the last count with S 1
    "split": (1, 160, 161),    # 321 rows: S 20, 11 tiles of 32, one a split, one row in the last
}
NAMES = ("dx", "dctx", "dw1", "db1", "dgamma", "dbeta", "dw2", "db2")


def splits(m):
    """The host rule (ffn_bw_splits)."""
    return 1 if m <= SPLIT_ROWS else SPLITS


def workspace_bytes(m):
    """lg_ffn_backward_workspace: the packed streams, g and da, the column partials, the split partials."""
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    wn = 512 * 512 + 256 * 512
    return up(2 * (2 * 512 * 512 + 256 * 512)) + 2 * up(m * 1024) + up((m + ROWS_WG - 1) // ROWS_WG * 1792 * 4) + splits(m) * wn * 4


def operands(name):
    """Seeded Gaussians in fp16: x [1, M, 256] and ctx_i [P, 4, ni, 64] at unit scale, weights at 1 / sqrt(fan-in),
    gamma around 1, dy at 2^-4 -> dict."""
    pr, n0, n1 = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name))
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(x=rn(1, pr * (n0 + n1), 256), ctx0=rn(pr, 4, n0, 64), ctx1=rn(pr, 4, n1, 64), w1=rn(512, 512) / math.sqrt(512),
             b1=0.1 * rn(512), gamma=1 + 0.1 * rn(512), beta=0.1 * rn(512), w2=rn(256, 512) / math.sqrt(512), b2=0.1 * rn(256),
             dy=rn(1, pr * (n0 + n1), 256) / 16)
    return {k: v.half() for k, v in t.items()}


def merge(ctx0, ctx1):
    """merge_heads of both images' head-major tensors, pair-major rows [M, 256]."""
    rows = [c[p].transpose(0, 1).reshape(c.shape[2], 256) for p in range(ctx0.shape[0]) for c in (ctx0, ctx1)]
    return torch.cat(rows, 0)


def reference(t):
    """float64 autograd of out = x + W2 GELU(LN(W1 c + b1)) + b2 -> the NAMES tensors (dctx merged, [M, 256])."""
    d = {k: v.double().requires_grad_() for k, v in t.items() if k != "dy"}
    c = torch.cat((d["x"][0], merge(d["ctx0"], d["ctx1"])), 1)
    h = F.gelu(F.layer_norm(F.linear(c, d["w1"], d["b1"]), (512,), d["gamma"], d["beta"], EPS))
    out = d["x"][0] + F.linear(h, d["w2"], d["b2"])
    out.backward(t["dy"][0].double())
    return (d["x"].grad[0], merge(d["ctx0"].grad, d["ctx1"].grad), d["w1"].grad, d["b1"].grad, d["gamma"].grad, d["beta"].grad,
            d["w2"].grad, d["b2"].grad)


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


def emulated(t):
    """The kernels' arithmetic in fp32 with their roundings -> the NAMES tensors."""
    f = {k: v.float() for k, v in t.items()}
    c, dy, gamma = torch.cat((f["x"][0], merge(f["ctx0"], f["ctx1"])), 1), f["dy"][0], f["gamma"]
    a = (c @ f["w1"].T + f["b1"]).half().float()
    mu = a.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((a - mu) ** 2).mean(1, keepdim=True) + EPS)
    n = (a - mu) * rstd
    u = n * gamma + f["beta"]
    g = F.gelu(u).half().float()
    du = (dy @ f["w2"]) * (0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi))
    dn = du * gamma
    da = (rstd * (dn - dn.mean(1, keepdim=True) - n * (dn * n).mean(1, keepdim=True))).half().float()
    dc = da @ f["w1"]
    return ((dy + dc[:, :256]).half(), dc[:, 256:].half(), da.T @ c, col_sum(da), col_sum((du * n).half().float()),
            col_sum(du.half().float()), dy.T @ g, col_sum(dy))


def rel(x, ref):
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def main():
    worst = {}
    for name, shape in CASES.items():
        t = operands(name)
        errs = [rel(x, r) for x, r in zip(emulated(t), reference(t))]
        for k, e in zip(NAMES, errs):
            worst[k] = max(worst.get(k, 0.0), e)
        m = shape[0] * (shape[1] + shape[2])
        print(f"{name:<8} {shape[0]}x({shape[1]}+{shape[2]}) S {splits(m):<2} " + "  ".join(f"{k} {e:.3e}" for k, e in zip(NAMES, errs)))
    for k in NAMES:  # (rounded up, so that the printed figure bounds the computed one)
        exp = int(np.floor(np.log10(worst[k])))
        print(f"worst {k} {np.ceil(worst[k] / 10.0 ** exp * 1000) / 1000:.3f}e{exp:+03d}")


if __name__ == "__main__":
    main()
