"""The attention backward on the MI355X against tests/attention_backward_refs.py: operands on which every query and
every key counts exactly once (census_q0, census_k0, selector, two-level, mixed: numeric equality with the float64
reference rounded to the output type, on every element of dQ, dK and dV) and graded operands under the derived
elementwise bound, at shapes that cover the split planner's space: 16 splits, a short last split, splits of several
blocks that start at an odd block, the workload's own plan, and the last shape that splits next to the first that does
not. Each test asserts the restated plan for its shape (against the library's workspace query) and prints its worst
error / bound.

mha_hd64_backward_fp16 / _fp32 are called through the library directly: dq, dk and dv start as NaN between sentinel
bytes, the five inputs lie between NaN rows, and the workspace is exactly mha_hd64_backward_workspace_bytes inside a
larger buffer that is refilled with a byte pattern before every launch and whose bytes beyond the stated size must come
back unchanged. tests/test_attention_backward_reference.py shows, without a GPU, what these checks reject.
"""
import numpy as np
import pytest

import attention_backward_refs as B
from gpu_common import GuardedIn, GuardedOut

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

WS_GUARD = 4096
WS_PATTERN = 0x5A       # (0x5A5A5A5A as fp32 is 1.5e16: an L or D read before it is written cannot pass)
NAMES = ("dq", "dk", "dv")
DTYPES = [torch.float16, torch.float32]
IDS = ["fp16", "fp32"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from lightglue_amd import _lib

    return _lib.load()


def _name(shape):
    return "x".join(map(str, shape))


def _report(capsys, what, worst):
    with capsys.disabled():
        print(f"\n  {what}: worst error / bound " + " ".join(f"{n} {w:.3f}" for n, w in zip(NAMES, worst)), end="")


_inputs = {}


def _on_device(case, key, dtype, dev):
    """The five inputs of a case between NaN rows, kept per (case, dtype)."""
    if len(_inputs) > 12:
        _inputs.clear()
    if (key, dtype) not in _inputs:
        _inputs[key, dtype] = [GuardedIn(torch.from_numpy(np.ascontiguousarray(case[x])).to(dtype), dev)
                               for x in ("q", "k", "v", "o", "dout")]
    return _inputs[key, dtype]


def backward(lib, dev, case, ins, dtype, what):
    """One guarded call -> (dq, dk, dv) as numpy. Asserts the status, the output guards, that every element was
    written, and that the workspace buffer is untouched beyond the size the library states."""
    from lightglue_amd import _lib

    plan = case["plan"]
    batch, heads, nq, nkv = (plan[x] for x in ("batch", "heads", "nq", "nkv"))
    f32 = dtype == torch.float32
    need = lib.mha_hd64_backward_workspace_bytes(batch, heads, nq, nkv, B.FLOAT if f32 else B.HALF)
    assert need == B.plan_backward(batch, heads, nq, nkv, f32)["ws_bytes"]
    ws = torch.full((need + 2 * WS_GUARD,), WS_PATTERN, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 256 == 0
    outs = [GuardedOut((batch, heads, n, 64), dtype, dev) for n in (nq, nkv, nkv)]
    fn = lib.mha_hd64_backward_fp32 if f32 else lib.mha_hd64_backward_fp16
    st = fn(*[g.ptr for g in ins], *[g.ptr for g in outs], batch, heads, nq, nkv, ws.data_ptr() + WS_GUARD, need,
            torch.cuda.current_stream().cuda_stream)
    assert st == 0, (what, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((ws[:WS_GUARD] == WS_PATTERN).all()), f"{what}: wrote before the workspace"
    assert bool((ws[WS_GUARD + need:] == WS_PATTERN).all()), f"{what}: wrote past the workspace's stated size"
    return [o.check(f"{what} {n}").numpy() for o, n in zip(outs, NAMES)]


def _exact(lib, dev, fam, shape, dtype, claim=None):
    """One exact family through one call -> (worst error / bound per tensor, the outputs)."""
    case, ref = B.case_and_reference(lib, fam, shape)     # (the plan asserted, the family's conditions asserted)
    plan = case["plan"]
    if claim is not None:
        assert (plan["splits"], plan["tiles_per_split"]) == claim, (shape, plan)
    what = f"{_name(shape)} splits {plan['splits']} {fam} {'fp32' if dtype == torch.float32 else 'fp16'}"
    got = backward(lib, dev, case, _on_device(case, (fam, shape, plan["splits"]), dtype, dev), dtype, what)
    return [B.check_exact(g, r, dtype == torch.float16, f"{what} {n}") for g, r, n in zip(got, ref, NAMES)], got


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", B.CENSUS_SHAPES, ids=_name)
def test_census_families_exact(shape, dtype, lib, dev, capsys):
    """Q = 0 (each key once in dQ, each query once in dV) and K = 0 (each query once in dK, across blocks and splits)."""
    for fam in ("census_q0", "census_k0"):
        worst, _ = _exact(lib, dev, fam, shape, dtype, B.SHAPES[shape])
        assert max(worst) <= 1.0
        _report(capsys, f"{_name(shape)} {fam} {IDS[DTYPES.index(dtype)]}", worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", list(B.SHAPES), ids=_name)
def test_selector_twolevel_mixed_exact(shape, dtype, lib, dev, capsys):
    for fam in ("selector", "twolevel", "mixed"):
        worst, _ = _exact(lib, dev, fam, shape, dtype, B.SHAPES[shape])
        assert max(worst) <= 1.0
        _report(capsys, f"{_name(shape)} {fam} {IDS[DTYPES.index(dtype)]}", worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", B.GRADED_SHAPES, ids=_name)
def test_graded_families_within_the_derived_bound(shape, dtype, lib, dev, capsys):
    """gauss1, peaked and spike, every element of dQ, dK and dV against the float64 closed form (D from the supplied O)
    under attention_backward_refs.graded_bound."""
    out16 = dtype == torch.float16
    for fam in B.GRADED:
        case, _ = B.case_and_reference(lib, fam, shape)
        assert (case["plan"]["splits"], case["plan"]["tiles_per_split"]) == B.SHAPES[shape]
        what = f"{_name(shape)} {fam} {IDS[DTYPES.index(dtype)]}"
        got = backward(lib, dev, case, _on_device(case, (fam, shape, 0), dtype, dev), dtype, what)
        worst = [0.0, 0.0, 0.0]
        for b in range(shape[0]):
            for h in range(shape[1]):
                refs, bounds = B.graded_bound(case, b, h, out16)
                for i in range(3):
                    ratio = np.abs(got[i][b, h].astype(np.float64) - refs[i]) / bounds[i]
                    worst[i] = max(worst[i], float(ratio.max()) if np.isfinite(ratio).all() else float("inf"))
        _report(capsys, what, worst)    # (the figure first, then the assertion)
        assert max(worst) <= 1.0, (what, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_forced_split_counts_give_the_same_numbers(dtype, lib, dev, monkeypatch, capsys):
    """2050 x 64 with MHA_HD64_BWD_SPLITS forced to 1, 2 and 16 (the library reads it per call): one split of 33 blocks,
    two of 17 and 16 (the second starts at an odd block), eleven of 3. Exact every time, and since every sum of these
    families is order-free, the same numbers every time."""
    want = {1: (1, 33), 2: (2, 17), 16: (11, 3)}
    runs = []
    for forced in B.FORCED_SPLITS:
        monkeypatch.setenv("MHA_HD64_BWD_SPLITS", str(forced))
        outs = []
        for fam in B.families_of(B.FORCED_SHAPE):
            worst, got = _exact(lib, dev, fam, B.FORCED_SHAPE, dtype, want[forced])
            assert max(worst) <= 1.0
            outs += got
            _report(capsys, f"{_name(B.FORCED_SHAPE)} forced {forced} {fam} {IDS[DTYPES.index(dtype)]}", worst)
        runs.append(outs)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert (a == b).all()


def test_forward_output_feeds_the_backward_exactly(lib, dev, capsys):
    """The chain forward -> backward: on selector rows the forward kernel's own O is V[target] bit for bit, and the
    backward on that O is exact."""
    from lightglue_amd import mha_hd64_batched

    for shape in ((1, 4, 130, 129), (1, 4, 1024, 1024)):
        case, ref = B.case_and_reference(lib, "selector", shape)
        for dtype in DTYPES:
            q, k, v, o, dout = _on_device(case, ("selector", shape, case["plan"]["splits"]), dtype, dev)
            fwd = mha_hd64_batched(q.view, k.view, v.view)
            torch.cuda.synchronize()
            assert fwd.dtype == dtype and np.array_equal(fwd.cpu().numpy().view(np.uint8), o.view.cpu().numpy().view(np.uint8))
            chained = [q, k, v, GuardedIn(fwd, dev), dout]
            what = f"{_name(shape)} selector on the forward's O {IDS[DTYPES.index(dtype)]}"
            got = backward(lib, dev, case, chained, dtype, what)
            worst = [B.check_exact(g, r, dtype == torch.float16, f"{what} {n}") for g, r, n in zip(got, ref, NAMES)]
            assert max(worst) <= 1.0
            _report(capsys, what, worst)
