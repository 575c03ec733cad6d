"""The projections' backward on the GPU (csrc/lightglue_proj_backward.hip): every output against float64 autograd of the
unfused projection, dx_add, null gradients, the data-only form, bitwise reproducibility, graph capture, and autograd
through SelfBlock.qkv_train, CrossBlock.qk_v_train and MatchAssignment.loss_rows."""
import copy
import importlib.util
import os

import pytest
import torch

from conftest import REPO
from gpu_common import capture_on_side_stream, same_bits

pytestmark = pytest.mark.gpu


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REPO, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


host = _tool("proj_backward_host_check")

# Four times the host check's worst figure per kind and tensor over these cases (profiles/proj_backward/host_check.txt;
# the GPU's own ratios: profiles/proj_backward/INDEX.md).
BOUND = dict(split2=dict(dx=4 * 3.503e-04, dw=4 * 6.544e-07, db=4 * 5.274e-08),
             qkv=dict(dx=4 * 3.705e-04, dw=4 * 2.845e-04, db=4 * 2.542e-04),
             plain=dict(dx=4 * 5.202e-04, dw=4 * 2.840e-04, db=4 * 2.438e-04))
_cache = {}


def case_data(kind, name):
    """(operands on the CPU, float64 reference), computed once per kind and case."""
    if (kind, name) not in _cache:
        t = host.operands(kind, name)
        _cache[kind, name] = (t, host.reference(kind, t))
    return _cache[kind, name]


def on_gpu(kind, name):
    return {k: [g.cuda() for g in v] if k == "grads" else v.cuda() for k, v in case_data(kind, name)[0].items()}


def run(kind, name, need_params=True, nan=False, dx_add=None, grads=None, t=None):
    from lightglue_amd.glue import _Hip

    t = t if t is not None else on_gpu(kind, name)
    out = None
    if nan:  # every element is written
        out = [torch.full(s, float("nan"), dtype=dt, device="cuda")
               for s, dt in ((t["x"].shape, torch.float16), (t["w"].shape, torch.float32), (t["b"].shape, torch.float32))]
    pr, n0, n1 = host.CASES[name]
    return _Hip.proj_backward(host.KINDS[kind], t["x"], t["w"], grads if grads is not None else t["grads"], (n0, n1, pr),
                              t.get("cos"), t.get("sin"), host.WIDTH[kind], dx_add, need_params, out)


@pytest.mark.parametrize("name", sorted(host.CASES))
@pytest.mark.parametrize("kind", sorted(host.KINDS))
def test_parity_with_float64(kind, name):
    got = [v.cpu() for v in run(kind, name, nan=True)]
    got[0] = got[0][0]
    errs = {k: host.rel(x, r) for k, x, r in zip(host.NAMES, got, case_data(kind, name)[1])}
    print(kind, name, " ".join(f"{k} {e:.3e} ({e / BOUND[kind][k] * 4:.2f} of the host figure)" for k, e in errs.items()))
    for k, x in zip(host.NAMES, got):
        assert bool(torch.isfinite(x).all()), k
    for k, e in errs.items():
        assert e <= BOUND[kind][k], (k, e, BOUND[kind][k])


@pytest.mark.parametrize("kind", sorted(host.KINDS))
def test_dx_add_is_added_before_the_rounding(kind):
    t = on_gpu(kind, "tile")
    dx = run(kind, "tile", dx_add=t["dx_add"], t=t)[0]
    want = case_data(kind, "tile")[1][0] + t["dx_add"][0].cpu().double()
    assert host.rel(dx[0].cpu(), want) <= BOUND[kind]["dx"]
    assert same_bits(run(kind, "tile", t=t)[0], run(kind, "tile", dx_add=torch.zeros_like(t["dx_add"]), t=t)[0])


def test_null_gradients_are_zeros():
    t = on_gpu("qkv", "tile")
    g = t["grads"]
    null = run("qkv", "tile", grads=[g[0], g[1], None, g[3], g[4], None], t=t)
    zero = run("qkv", "tile", grads=[g[0], g[1], torch.zeros_like(g[2]), g[3], g[4], torch.zeros_like(g[5])], t=t)
    for a, b in zip(null, zero):
        assert same_bits(a, b)


@pytest.mark.parametrize("kind", sorted(host.KINDS))
def test_data_only_has_the_full_call_s_bits(kind):
    full, data = run(kind, "pairs"), run(kind, "pairs", need_params=False)
    assert data[1] is None and data[2] is None and same_bits(full[0], data[0])


@pytest.mark.parametrize("kind", sorted(host.KINDS))
def test_reproducible_and_captured_call_equals_eager(kind):
    t = on_gpu(kind, "split")
    eager = run(kind, "split", t=t)
    for a, b in zip(eager, run(kind, "split", t=t)):
        assert same_bits(a, b)
    graph, outs = capture_on_side_stream(lambda: run(kind, "split", t=t))
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert same_bits(a, b)


def _fp32_on_the_fp16_grid(module):
    """fp32 parameters with fp16 values: the ops' fp16 weights are exact, and .grad keeps the kernels' fp32."""
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(p.half().float())
    return module


@pytest.mark.parametrize("kind", ["qkv", "split2"])
def test_block_projection_trains(kind):
    """qkv_train / qk_v_train have the inference kernels' bits; the gradients of x and of Wqkv / to_qk, to_v against
    float64 autograd of the block's unfused projection (SelfBlock.qkv, CrossBlock.heads_of), each held to its tensor's
    bound; the block's other parameters get none. With the parameters frozen the backward is the data-only call."""
    from lightglue_amd.glue import _Hip
    from lightglue_amd.layers import CrossBlock, SelfBlock
    from lightglue_amd.weights import _cross_qkv, _qkv_perm

    t, splits = on_gpu(kind, "tile"), host.CASES["tile"][1:]
    torch.manual_seed(13)
    block = _fp32_on_the_fp16_grid((SelfBlock if kind == "qkv" else CrossBlock)(256, 4))
    ref = copy.deepcopy(block).double()
    block = block.cuda()
    x = t["x"].clone().requires_grad_()
    x64 = t["x"].cpu().double().requires_grad_()
    if kind == "qkv":
        outs = block.qkv_train(x, t["cos"], t["sin"], splits)
        with torch.no_grad():
            i0, i1 = _Hip.linear_qkv_rotary(x, *_qkv_perm(block, torch.float16), t["cos"], t["sin"], 4, splits)
            same = [*i0, *i1]
        i0, i1 = ref.qkv(x64, t["cos"].cpu().double(), t["sin"].cpu().double(), splits)
        outs64 = [*i0, *i1]
        trained = {"Wqkv.weight": "dw", "Wqkv.bias": "db"}
    else:
        outs = block.qk_v_train(x, splits)
        with torch.no_grad():
            (a0, a1), (b0, b1) = _Hip.linear_split2(x, *_cross_qkv(block, torch.float16), 4, splits)
            same = [a0, a1, b0, b1]
        outs64 = ref.heads_of(ref.to_qk(x64), splits) + ref.heads_of(ref.to_v(x64), splits)
        trained = {"to_qk.weight": "dw", "to_qk.bias": "db", "to_v.weight": "dw", "to_v.bias": "db"}
    for a, b in zip(outs, same):
        assert same_bits(a, b)
    sum((g * o.float()).sum() for g, o in zip(t["grads"], outs)).backward()
    sum((g.cpu().double() * o).sum() for g, o in zip(t["grads"], outs64)).backward()
    assert host.rel(x.grad.cpu(), x64.grad) <= BOUND[kind]["dx"]
    want = dict(ref.named_parameters())
    for name, p in block.named_parameters():
        if name in trained:
            e = host.rel(p.grad.cpu(), want[name].grad)
            print(kind, name, f"{e:.3e}")
            assert p.grad.dtype == torch.float32 and e <= BOUND[kind][trained[name]], (name, e)
        else:
            assert p.grad is None, name
    frozen = t["x"].clone().requires_grad_()
    for p in block.parameters():
        p.requires_grad_(False)
    outs = block.qkv_train(frozen, t["cos"], t["sin"], splits) if kind == "qkv" else block.qk_v_train(frozen, splits)
    sum((g * o.float()).sum() for g, o in zip(t["grads"], outs)).backward()
    assert same_bits(frozen.grad, x.grad)


def test_head_loss_rows_trains_final_proj_and_matchability():
    """loss_rows(...).sum().backward() against float64 autograd of assignment_nll_reference on the unfused head."""
    from lightglue_amd import assignment_nll_reference
    from lightglue_amd.layers import MatchAssignment

    nll = _tool("assign_nll_host_check")
    _, m, _, gt0, gt1 = nll.operands("gauss")
    n = gt1.shape[1]
    torch.manual_seed(19)
    head = _fp32_on_the_fp16_grid(MatchAssignment(256))
    ref = copy.deepcopy(head).double()
    head = head.cuda()
    x = (0.5 * torch.randn((1, m + n, 256))).half()
    head.loss_rows(x.cuda(), 1, m, n, gt0.cuda(), gt1.cuda()).sum().backward()
    x64 = x.double()
    v = torch.cat((ref.final_proj(x64) / ref.scale, ref.matchability(x64), x64.new_zeros((1, m + n, 127))), 2)
    assignment_nll_reference(v, m, 256, gt0, gt1).sum().backward()
    want = dict(ref.named_parameters())
    for name, p in head.named_parameters():
        e = host.rel(p.grad.cpu(), want[name].grad)
        print(name, f"{e:.3e}")
        assert e <= BOUND["plain"]["dw" if name.endswith("weight") else "db"], (name, e)
