"""The attention backward's arithmetic restated on the CPU in framework ops, with the kernels' rounding
points (csrc/mha_hd64_backward.hip): fp16 inputs (the saved O included); fp32 S, L and D; P and dS rounded
to fp16 where they become MFMA operands; fp32 products; the output rounding (fp16 form only).

Prints, per test shape and per tensor, max|x - ref| / max|ref| against attention_backward_reference on
the fp16-rounded inputs, then the worst per tensor: tests/test_gpu_attention_backward.py takes four times
those as its bounds (the factor covers the kernels' summation order). Output kept as
profiles/attention_backward/host_check.txt.

    python tools/attention_backward_host_check.py > profiles/attention_backward/host_check.txt
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))

from lightglue_amd import attention_backward_reference, synth  # noqa: E402

BQ = BK = 64  # the row and column kernels' block sizes
SCALE_LOG2 = np.float32(0.18033688011112042)  # 0.125 * log2(e)

# (name, batch, heads, nq, nkv, kind): the GPU tests' cases. The column kernel splits the query blocks
# while batch * heads * ceil(nkv / 64) <= 128: split128 is the last shape that splits, nosplit160 the first
# that does not (and every single-block shape does not).
CASES = [
    ("1x1", 1, 4, 1, 1, "normal"),
    ("bq-1", 1, 4, BQ - 1, BK + 1, "normal"),
    ("bq", 1, 4, BQ, BK, "normal"),
    ("bq+1", 1, 4, BQ + 1, BK - 1, "normal"),
    ("3bq+5", 1, 4, 3 * BQ + 5, 2 * BK + 7, "normal"),
    ("2bq+3", 1, 4, 2 * BQ + 3, 5 * BK + 1, "normal"),
    ("b2h3", 2, 3, 70, 45, "normal"),
    ("split128", 8, 4, 2 * BQ + 2, 4 * BK, "normal"),
    ("nosplit160", 8, 4, 2 * BQ + 2, 4 * BK + 1, "normal"),
    ("peaked", 1, 4, 2 * BQ + 3, 2 * BK + 7, "peaked"),
    ("spike", 1, 4, 2 * BQ + 3, 2 * BK + 7, "spike"),
]


def inputs(case):
    """fp32 (q, k, v, dout) of a case: synth.qkv, a seeded normal dout; peaked: logits reach +-40;
    spike: one key dominates a row (logit 32 there)."""
    name, batch, heads, nq, nkv, kind = case
    seed = 1 + [c[0] for c in CASES].index(name)
    q, k, v = synth.qkv(seed, nq, nkv, q_std=10.0 if kind == "peaked" else 1.0, batch=batch, heads=heads)
    if kind == "spike":
        k = synth.spike(q, k, nq // 2, nkv - 3, 4.0)
    dout = synth.normal(seed * 3 + 100, q.shape, 1.0)
    return tuple(torch.from_numpy(x) for x in (q, k, v, dout))


def emulate(q, k, v, dout, out_dtype):
    q, k, v, do = (t.half().float() for t in (q, k, v, dout))
    o = torch.softmax(q.double() @ k.double().transpose(-1, -2) * 0.125, -1) @ v.double()
    o = o.half().float()  # the forward's output as the backward reads it
    x = (q @ k.transpose(-1, -2)) * SCALE_LOG2
    m = x.amax(-1, keepdim=True)
    lse = m + torch.log2(torch.exp2(x - m).sum(-1, keepdim=True))
    p = torch.exp2(x - lse)
    d = (do * o).sum(-1, keepdim=True)
    ds = p * (do @ v.transpose(-1, -2) - d)
    p16, ds16 = p.half().float(), ds.half().float()
    dq, dk, dv = (ds16 @ k) * 0.125, (ds16.transpose(-1, -2) @ q) * 0.125, p16.transpose(-1, -2) @ do
    return tuple(t.to(out_dtype).double() for t in (dq, dk, dv))


def rel(x, ref):
    """max|x - ref| / max|ref|, the denominator floored at 1: the inputs are unit-scale normals, and a gradient
    that is exactly zero (one key: P = 1, dS = 0, so dQ = dK = 0) is compared absolutely at that scale."""
    return float((x.double() - ref).abs().max() / ref.abs().max().clamp_min(1.0))


def main():
    worst = {}
    for case in CASES:
        q, k, v, dout = inputs(case)
        ref = attention_backward_reference(*(t.half() for t in (q, k, v, dout)))
        for dt, form in ((torch.float16, "fp16"), (torch.float32, "fp32")):
            errs = [rel(x, r) for x, r in zip(emulate(q, k, v, dout, dt), ref)]
            for name, e in zip(("dq", "dk", "dv"), errs):
                worst[form, name] = max(worst.get((form, name), 0.0), e)
            print(f"{case[0]:<11} {case[1]}x{case[2]}x{case[3]}x{case[4]:<4} {form}  " +
                  "  ".join(f"{n} {e:.3e}" for n, e in zip(("dq", "dk", "dv"), errs)))
    for (form, name), e in sorted(worst.items()):
        print(f"worst {form} {name} {e:.3e}")


if __name__ == "__main__":
    main()
