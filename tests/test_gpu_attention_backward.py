"""Attention backward on the GPU (csrc/mha_hd64_backward.hip): dQ, dK, dV against the float64 closed form on
the fp16-rounded inputs, bitwise reproducibility, autograd through both public entries, and graph capture."""
import importlib.util
import os

import pytest
import torch

from conftest import REPO
from gpu_common import capture_on_side_stream, same_bits

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("attention_backward_host_check",
                                               os.path.join(REPO, "tools", "attention_backward_host_check.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)

# Four times the host check's worst figure per tensor over these cases (profiles/attention_backward/INDEX.md,
# host_check.txt: fp16 dq 5.879e-04, dk 7.996e-04, dv 4.815e-04; fp32 dq 5.527e-04, dk 7.994e-04, dv 2.721e-04).
BOUND = {torch.float16: (4 * 5.879e-04, 4 * 7.996e-04, 4 * 4.815e-04),
         torch.float32: (4 * 5.527e-04, 4 * 7.994e-04, 4 * 2.721e-04)}
CASES = {c[0]: c for c in host.CASES}
_cache = {}


def case_data(name):
    """(fp32 inputs on the CPU, float64 reference on their fp16 rounding), computed once per case."""
    if name not in _cache:
        from lightglue_amd import attention_backward_reference

        x = host.inputs(CASES[name])
        _cache[name] = (x, attention_backward_reference(*(t.half() for t in x)))
    return _cache[name]


def run(name, dtype):
    """The C-ABI backward (through plugin.mha_hd64_backward) on the forward kernel's own output."""
    from lightglue_amd import mha_hd64_backward, mha_hd64_batched

    q, k, v, dout = (t.to("cuda", dtype) for t in case_data(name)[0])
    return mha_hd64_backward(q, k, v, mha_hd64_batched(q, k, v), dout)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_parity_with_float64(name, dtype):
    grads = [g.cpu() for g in run(name, dtype)]
    errs = [host.rel(g, ref) for g, ref in zip(grads, case_data(name)[1])]
    print(name, dtype, " ".join(f"{e:.3e}" for e in errs))
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    for what, e, bound in zip(("dq", "dk", "dv"), errs, BOUND[dtype]):
        assert e <= bound, (what, e, bound)


@pytest.mark.parametrize("name", ["3bq+5", "2bq+3", "split128"])
def test_reproducible(name):
    for a, b in zip(run(name, torch.float16), run(name, torch.float16)):
        assert same_bits(a, b)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("entry", ["function", "op"])
def test_autograd_is_the_c_abi_call(entry, dtype):
    from lightglue_amd import MHAHeadDim64, mha_hd64_backward

    fwd = MHAHeadDim64.apply if entry == "function" else torch.ops.lightglue_amd.mha_hd64
    q, k, v, dout = (t.to("cuda", dtype) for t in case_data("3bq+5")[0])
    plain = fwd(q, k, v)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    out = fwd(*leaves)
    assert same_bits(out.detach(), plain)
    out.backward(dout.transpose(2, 3).contiguous().transpose(2, 3))  # (a non-contiguous dout)
    for leaf, want in zip(leaves, mha_hd64_backward(q, k, v, plain, dout)):
        assert same_bits(leaf.grad, want)
    only_k = [q, k.clone().requires_grad_(), v]
    fwd(*only_k).backward(dout)
    assert same_bits(only_k[1].grad, leaves[1].grad) and q.grad is None and v.grad is None


def test_forward_and_backward_in_one_graph():
    from lightglue_amd import mha_hd64, mha_hd64_backward

    q, k, v, dout = (t.to("cuda", torch.float16) for t in case_data("3bq+5")[0])
    eager = mha_hd64_backward(q, k, v, mha_hd64(q, k, v), dout)

    def both():
        return mha_hd64_backward(q, k, v, mha_hd64(q, k, v), dout)

    graph, outs = capture_on_side_stream(both)
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert same_bits(a, b)
