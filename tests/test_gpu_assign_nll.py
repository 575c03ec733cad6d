"""The assignment loss on the GPU (csrc/lightglue_assign_nll.hip): loss, dm0, dm1 and dz against float64 autograd
of assignment_nll_reference, every other element of dv, bitwise reproducibility, autograd through both public
entries, and graph capture."""
import importlib.util
import os

import pytest
import torch

from conftest import REPO
from gpu_common import capture_on_side_stream, same_bits

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("assign_nll_host_check", os.path.join(REPO, "tools", "assign_nll_host_check.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)

# Four times the host check's worst figure per tensor over these cases (profiles/assign_nll/host_check.txt:
# loss 7.280e-08, dm0 2.375e-04, dm1 1.668e-04, dz 1.043e-07; the GPU's own ratios: profiles/assign_nll/INDEX.md).
BOUND = dict(loss=4 * 7.280e-08, dm0=4 * 2.375e-04, dm1=4 * 1.668e-04, dz=4 * 1.043e-07)
_cache = {}


def case_data(name):
    """(operands on the CPU, float64 reference), computed once per case."""
    if name not in _cache:
        ops = host.operands(name)
        _cache[name] = (ops, host.reference(*ops))
    return _cache[name]


def on_gpu(name):
    v, m, lens, gt0, gt1 = case_data(name)[0]
    return v.cuda(), m, host.ZC, gt0.cuda(), gt1.cuda(), None if lens is None else tuple(t.cuda() for t in lens)


def run(name):
    from lightglue_amd.glue import _Hip

    return _Hip.assign_nll(*on_gpu(name))


@pytest.mark.parametrize("name", sorted(host.CASES))
def test_parity_with_float64(name):
    from lightglue_amd.glue import _Hip

    (v, m, lens, gt0, gt1), ref = case_data(name)
    nan = [torch.full(s, float("nan"), device="cuda") for s in ((v.shape[0],), v.shape)]   # every element is written
    loss, dv = (t.cpu() for t in _Hip.assign_nll(*on_gpu(name), out=nan))
    got = (loss, dv[:, :m, :256], dv[:, m:, :256], dv[:, :, host.ZC])
    errs = {k: host.rel(x, r) for k, x, r in zip(host.NAMES, got, ref)}
    print(name, " ".join(f"{k} {e:.3e}" for k, e in errs.items()))
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dv).all())
    for k, e in errs.items():
        assert e <= BOUND[k], (k, e, BOUND[k])
    rest = [c for c in range(256, host.LD) if c != host.ZC]
    assert not dv[:, :, rest].any()
    for p in range(dv.shape[0]):
        ml, nl = (m, dv.shape[1] - m) if lens is None else (int(lens[0][p]), int(lens[1][p]))
        assert not dv[p, ml:m].any() and not dv[p, m + nl:].any()             # padded rows: exactly 0
        if not ((gt0[p, :ml] >= 0) & (gt0[p, :ml] < nl)).any():
            assert not dv[p, :, :256].any()                                   # no positive: dm exactly 0
            if not (gt0[p, :ml] == -1).any() and not (gt1[p, :nl] == -1).any():
                assert loss[p] == 0 and not dv[p].any()                       # everything ignored


@pytest.mark.parametrize("name", ["ragged", "split"])
def test_reproducible(name):
    for a, b in zip(run(name), run(name)):
        assert same_bits(a, b)


@pytest.mark.parametrize("entry", ["function", "op"])
def test_autograd_is_the_c_abi_call(entry):
    from lightglue_amd import assignment_nll

    v, m, zc, gt0, gt1, lens = on_gpu("ragged")
    loss, dv = run("ragged")
    leaf = v.clone().requires_grad_()
    if entry == "function":
        out = assignment_nll(leaf, m, zc, gt0, gt1, lens)
    else:
        out = torch.ops.lightglue_amd.assign_nll(leaf, m, zc, gt0, gt1, *lens)[0]
    assert same_bits(out.detach(), loss)
    g = torch.tensor([65536.0, 0.25, -3.0], device="cuda")   # (a 2^16 loss scale among them)
    out.backward(g)
    assert same_bits(leaf.grad, (dv * g[:, None, None]).half())


def test_loss_rows_is_assignment_nll_on_project_rows():
    from lightglue_amd import assignment_nll
    from lightglue_amd.layers import MatchAssignment

    _, m, _, gt0, gt1, lens = on_gpu("ragged")
    pr, n = gt0.shape[0], gt1.shape[1]
    torch.manual_seed(5)
    head = MatchAssignment(256).cuda().half()
    x = torch.randn((1, pr * (m + n), 256), device="cuda").half()
    with torch.no_grad():
        want = assignment_nll(head.project_rows(x, pr, m, n), m, 256, gt0, gt1, lens)
        assert same_bits(head.loss_rows(x, pr, m, n, gt0, gt1, lens), want)


def test_captured_call_equals_eager():
    from lightglue_amd.glue import _Hip

    args = on_gpu("split")
    eager = _Hip.assign_nll(*args)
    graph, outs = capture_on_side_stream(lambda: _Hip.assign_nll(*args))
    for _ in range(2):
        for o in outs:
            o.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert same_bits(a, b)
