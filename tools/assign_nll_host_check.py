"""The assignment loss's arithmetic restated on the CPU in framework ops, with the kernels' rounding points
(csrc/lightglue_assign_nll.hip): fp16 v; the similarity accumulated in fp32 and rounded to fp16; fp32 logsumexps
and exponentials; G rounded unscaled to fp16 where it becomes an MFMA operand; fp32 products, 0.5/Pn applied once
at the end; the loss's terms in fp32, summed in float64 and rounded to fp32.

Prints, per test case and per tensor (loss, dm0, dm1, dz), max|x - ref| / max|ref| against
assignment_nll_reference's float64 autograd, then the worst per tensor: tests/test_gpu_assign_nll.py takes four
times those as its bounds. Output kept as profiles/assign_nll/host_check.txt.

    python tools/assign_nll_host_check.py > profiles/assign_nll/host_check.txt
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import assignment_refs as refs  # noqa: E402

LD, ZC = 264, 259  # v's row stride and the matchability channel here (zc not a multiple of 4; channel 256 is ignored)

# name -> (kind, (P, m, n), ragged). With S the statistics kernel's split and G the gradient kernel's
# (nll_splits: G = 1 once (ceil(m/64) + ceil(n/64)) P > 128, and never more than ceil(max(m, n) / 32)):
CASES = {
    "one_row": ("exact", (1, 1, 8), False),        # S 8, G 1: one row, the positive in the last column
    "strip": ("exact", (1, 33, 40), False),        # S 8, G 2: crosses a 32-row strip, a partial column block
    "gauss": ("gauss", (1, 33, 40), False),        # the same shape on Gaussian operands
    "ragged": ("exact", (3, 70, 72), True),        # S 8, G 3: m_len cuts a strip, n_len % 8 != 0
    "stats1": ("exact", (9, 232, 232), False),     # S 1, G 2
    "split": ("exact", (14, 200, 264), False),     # 126 gradient workgroups: G 2, the last count that splits
    "nosplit": ("exact", (15, 200, 264), False),   # 135: G 1, nine streamed tiles per workgroup
}


def operands(name):
    """(v fp16 [P, m + n, LD], m, lens or None, gt0, gt1 int32) of a case. Ground truth per pair: half the rows
    positive on distinct columns, a quarter unmatchable, the rest ignored; rows 0 and 1 claim one column; the last
    valid row claims the last valid column; the unclaimed columns are unmatchable or ignored in turn. The ragged
    case's pair 0 has no positive, its pair 1 ignores everything, its pair 2 has entries at and past n_len."""
    kind, shape, ragged = CASES[name]
    pr, m, n = shape
    inp = refs.Inputs(kind, shape, ragged)
    v = inp.v[:, :, :LD].copy()
    v[:, :, ZC] = inp.v[:, :, refs.ZC]
    gt0, gt1 = np.full((pr, m), -2, np.int32), np.full((pr, n), -2, np.int32)
    for p in range(pr):
        rng = np.random.default_rng(refs.seed_of("gt", name, p))
        ml, nl = (m, n) if not ragged else (int(inp.mlen[p]), int(inp.nlen[p]))
        if ragged and p == 1:
            continue
        rows = rng.permutation(ml)
        npos = 0 if (ragged and p == 0) else min((ml + 1) // 2, nl)
        gt0[p, rows[:npos]] = rng.permutation(nl)[:npos]
        gt0[p, rows[npos:npos + max(ml // 4, 1 if npos == 0 else 0)]] = -1
        if npos:
            gt0[p, ml - 1] = nl - 1
            if ml >= 3:
                gt0[p, 0] = gt0[p, 1] = int(rng.integers(0, nl))
        if ragged and p == 2:
            gt0[p, 2], gt0[p, 3] = nl, n - 1
        free = np.setdiff1d(np.arange(nl), gt0[p][gt0[p] >= 0])
        gt1[p, free[::2]] = -1
    lens = None if not ragged else (torch.from_numpy(inp.mlen), torch.from_numpy(inp.nlen))
    return torch.from_numpy(v), m, lens, torch.from_numpy(gt0), torch.from_numpy(gt1)


def reference(v, m, lens, gt0, gt1):
    """float64 (loss [P], dm0 [P, m, 256], dm1 [P, n, 256], dz [P, m + n]) by autograd of assignment_nll_reference;
    the gradient of the sum over pairs, so each pair's block is that pair's own gradient."""
    from lightglue_amd import assignment_nll_reference

    leaf = torch.nan_to_num(v.double(), 0.0, 0.0, 0.0).requires_grad_()  # (padded rows hold NaN / Inf: never read)
    loss = assignment_nll_reference(leaf, m, ZC, gt0, gt1, lens)
    loss.sum().backward()
    g = leaf.grad
    return loss.detach(), g[:, :m, :256], g[:, m:, :256], g[:, :, ZC]


def closed_form(v, m, lens, gt0, gt1, emulate):
    """The issue's closed form per pair: in float64 (emulate False), or with the kernels' roundings."""
    pr, n = v.shape[0], v.shape[1] - m
    ft = torch.float32 if emulate else torch.float64
    loss, dm0 = torch.zeros(pr, dtype=torch.float64), torch.zeros((pr, m, 256), dtype=torch.float64)
    dm1, dz = torch.zeros((pr, n, 256), dtype=torch.float64), torch.zeros((pr, m + n), dtype=torch.float64)
    for p in range(pr):
        ml, nl = (m, n) if lens is None else (int(lens[0][p]), int(lens[1][p]))
        a, b = v[p, :ml, :256].to(ft), v[p, m:m + nl, :256].to(ft)
        z0, z1 = v[p, :ml, ZC].to(ft), v[p, m:m + nl, ZC].to(ft)
        g0, g1 = gt0[p, :ml].long(), gt1[p, :nl].long()
        sim = (a @ b.T).half().to(ft)

        def lse(x, dim):
            mx = x.amax(dim, keepdim=True)
            return (mx + torch.log(torch.exp(x - mx).sum(dim, keepdim=True))).squeeze(dim)

        lr, lc = lse(sim, 1), lse(sim, 0)
        pos = (g0 >= 0) & (g0 < nl)
        rows = torch.nonzero(pos)[:, 0]
        w = torch.zeros((ml, nl), dtype=ft)
        w[rows, g0[rows]] = 1.0
        r, c = w.sum(1), w.sum(0)
        n0, n1 = g0 == -1, g1 == -1
        wp = torch.tensor(0.5, dtype=ft) / max(len(rows), 1)
        wn = torch.tensor(0.5, dtype=ft) / max(int(n0.sum()) + int(n1.sum()), 1)
        g = r[:, None] * torch.exp(sim - lr[:, None]) + c[None, :] * torch.exp(sim - lc[None, :]) - 2.0 * w
        if emulate:
            g = g.half().float()
        dm0[p, :ml], dm1[p, :nl] = ((g @ b) * wp).double(), ((g.T @ a) * wp).double()
        dz[p, :ml] = (-wp * r * torch.sigmoid(-z0) + wn * n0.to(ft) * torch.sigmoid(z0)).double()
        dz[p, m:m + nl] = (-wp * c * torch.sigmoid(-z1) + wn * n1.to(ft) * torch.sigmoid(z1)).double()
        terms = 2.0 * sim[rows, g0[rows]] + (F.logsigmoid(z0) - lr)[rows] + (F.logsigmoid(z1) - lc)[g0[rows]]
        neg = F.logsigmoid(-z0)[n0].double().sum() + F.logsigmoid(-z1)[n1].double().sum()
        loss[p] = -wp.double() * terms.double().sum() - wn.double() * neg
        if emulate:
            loss[p] = loss[p].float().double()
    return loss, dm0, dm1, dz


def rel(x, ref):
    """max|x - ref| / max|ref| (0 where both are all zero: a case without a positive)."""
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


NAMES = ("loss", "dm0", "dm1", "dz")


def main():
    worst = {}
    for name, (kind, shape, ragged) in CASES.items():
        ops = operands(name)
        errs = [rel(x, r) for x, r in zip(closed_form(*ops, emulate=True), reference(*ops))]
        for k, e in zip(NAMES, errs):
            worst[k] = max(worst.get(k, 0.0), e)
        print(f"{name:<8} {kind:<6} {shape[0]}x{shape[1]}x{shape[2]:<4} " + "  ".join(f"{k} {e:.3e}" for k, e in zip(NAMES, errs)))
    for k in NAMES:  # (rounded up, so that the printed figure bounds the computed one)
        exp = int(np.floor(np.log10(worst[k])))
        print(f"worst {k} {np.ceil(worst[k] / 10.0 ** exp * 1000) / 1000:.3f}e{exp:+03d}")


if __name__ == "__main__":
    main()
