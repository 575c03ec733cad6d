"""The FFN backward on the GPU (csrc/lightglue_ffn_backward.hip): every output against float64 autograd of the unrounded
block, bitwise reproducibility, graph capture, the data-only form, and autograd through layers.ffn_residual."""
import copy
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from gpu_common import capture_on_side_stream, same_bits

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("ffn_backward_host_check", os.path.join(REPO, "tools", "ffn_backward_host_check.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)

# Four times the host check's worst figure per tensor over these cases (profiles/ffn_backward/host_check.txt; the GPU's
# own ratios: profiles/ffn_backward/INDEX.md).
BOUND = dict(dx=4 * 4.156e-04, dctx=4 * 4.836e-04, dw1=4 * 3.171e-04, db1=4 * 2.839e-04, dgamma=4 * 5.063e-04,
             dbeta=4 * 2.881e-04, dw2=4 * 5.260e-04, db2=4 * 3.874e-08)
_cache = {}


def case_data(name):
    """(operands on the CPU, float64 reference), computed once per case."""
    if name not in _cache:
        t = host.operands(name)
        _cache[name] = (t, host.reference(t))
    return _cache[name]


def on_gpu(name):
    return {k: v.cuda() for k, v in case_data(name)[0].items()}


def run(name, need_params=True, nan=False, t=None):
    from lightglue_amd.glue import _Hip

    t = t if t is not None else on_gpu(name)
    ln = SimpleNamespace(weight=t["gamma"], bias=t["beta"], eps=host.EPS)
    out = None
    if nan:  # every element is written
        like = (t["x"], t["ctx0"], t["ctx1"], t["w1"], t["b1"], t["b1"], t["b1"], t["w2"], t["b2"])
        out = [torch.full(v.shape, float("nan"), dtype=torch.float16 if i < 3 else torch.float32, device="cuda")
               for i, v in enumerate(like)]
    return _Hip.ffn_backward(t["x"], t["ctx0"], t["ctx1"], t["w1"], t["b1"], ln, t["w2"], t["dy"], need_params, out)


@pytest.mark.parametrize("name", sorted(host.CASES))
def test_parity_with_float64(name):
    got = [v.cpu() for v in run(name, nan=True)]
    got = [got[0][0], host.merge(got[1], got[2])] + got[3:]
    errs = {k: host.rel(x, r) for k, x, r in zip(host.NAMES, got, case_data(name)[1])}
    print(name, " ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    for k, x in zip(host.NAMES, got):
        assert bool(torch.isfinite(x).all()), k
    for k, e in errs.items():
        assert e <= BOUND[k], (k, e, BOUND[k])


def test_reproducible():
    for a, b in zip(run("split"), run("split")):
        assert same_bits(a, b)


def test_data_only_has_the_full_call_s_bits():
    full, data = run("pairs"), run("pairs", need_params=False)
    assert all(v is None for v in data[3:])
    for a, b in zip(full[:3], data[:3]):
        assert same_bits(a, b)


def test_captured_call_equals_eager():
    eager = run("split")
    t = on_gpu("split")
    graph, outs = capture_on_side_stream(lambda: run("split", t=t))
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert same_bits(a, b)


@pytest.mark.parametrize("kind", ["self", "cross"])
def test_ffn_residual_trains_the_block(kind):
    """out is _Hip.ffn's; the gradients of x, the contexts and every parameter of the block against float64 autograd of
    finish(..., hip=False), each held to its tensor's bound; the un-folded parameters take dw1's / db1's. ffn[3].bias
    alone gets an allowance: db2's bound (1.5e-7) is below the cast of the gradient to the parameter's fp16, half an
    ulp, so at most 2^-11 of the largest entry is added to it (the fp32 db2 itself is held to the plain bound by the
    parity test). With the parameters frozen the backward is the data-only call and dx, dctx keep their bits."""
    from lightglue_amd import ffn_residual
    from lightglue_amd.glue import _Hip
    from lightglue_amd.layers import CrossBlock, SelfBlock
    from lightglue_amd.weights import _ffn_in_fused

    t = case_data("tile")[0]
    torch.manual_seed(11)
    block = (SelfBlock if kind == "self" else CrossBlock)(256, 4).half()
    with torch.no_grad():
        block.ffn[1].weight.add_(0.1 * torch.randn(512)), block.ffn[1].bias.add_(0.1 * torch.randn(512))
    ref = copy.deepcopy(block).double()
    block = block.cuda()
    proj = block.out_proj if kind == "self" else block.to_out
    leaves = [t[k].cuda().requires_grad_() for k in ("x", "ctx0", "ctx1")]
    out = ffn_residual(block, proj, *leaves)
    with torch.no_grad():
        w, b = _ffn_in_fused(block, proj, torch.float16)
        assert same_bits(out, _Hip.ffn(*leaves, w, b, block.ffn[1], block.ffn[3].weight, block.ffn[3].bias))
    out.backward(t["dy"].cuda())

    leaves64 = [t[k].double().requires_grad_() for k in ("x", "ctx0", "ctx1")]
    ref.finish(leaves64[0], leaves64[1:], hip=False).backward(t["dy"].double())
    bound = {"ffn.0.weight": "dw1", "ffn.0.bias": "db1", "ffn.1.weight": "dgamma", "ffn.1.bias": "dbeta", "ffn.3.weight": "dw2",
             "ffn.3.bias": "db2", "out_proj.weight": "dw1", "out_proj.bias": "db1", "to_out.weight": "dw1", "to_out.bias": "db1"}
    for a, r, k in zip(leaves, leaves64, ("dx", "dctx", "dctx")):
        assert host.rel(a.grad.cpu(), r.grad) <= BOUND[k], k
    want = dict(ref.named_parameters())
    for name, p in block.named_parameters():
        if name in bound:
            e = host.rel(p.grad.cpu(), want[name].grad)
            print(kind, name, f"{e:.3e}")
            assert e <= BOUND[bound[name]] + (2.0 ** -11 if name == "ffn.3.bias" else 0.0), (name, e)
        else:
            assert p.grad is None, name
    frozen = [v.detach().clone().requires_grad_() for v in leaves]
    for p in block.parameters():
        p.requires_grad_(False)
    ffn_residual(block, proj, *frozen).backward(t["dy"].cuda())
    for a, b in zip(frozen, leaves):
        assert same_bits(a.grad, b.grad)
