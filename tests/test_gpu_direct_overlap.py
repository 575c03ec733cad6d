"""Stale-slot screen for the single-pass kernels' PV under the V stream.

The one-pass forms read V(t) out of the LDS slot that K(t) went through, as soon as a counted
`s_waitcnt vmcnt` says V(t) has landed. A read issued too early returns what the slot held before:
K of the same tile, or V of the launch that ran on that CU before. So each case here launches
twice back to back on one stream, with the same Q and K and a second V that differs from the first
in every element by at least 2 (200 times the tolerance), from fresh allocations, and checks the
second output against the fp64 C oracle.

A pass does not prove the wait counts: an early read goes unnoticed whenever the DMA happens to
land first. The derivation next to each wait in csrc/mha_hd64_direct16.hip is the proof; this
test screens for the failure, it does not search for it (one run per case, no repeats).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-2          # fp16 output (the contract of tests/test_gpu_parity.py)
TOL_F32OUT = 5e-3   # fp32 output

# (nq, nkv): the smallest shapes that reach each wait of the 16-row kernel (4 waves; plan 21 runs
# the 32-row kernel, 8 waves, on the same shapes)
SHAPES = [
    (64, 1024),  # four full tiles per wave
    (64, 1000),  # partial last tile
    (64, 577),   # a wave with one tile, a wave with none
    (64, 512),   # the 2-tile form
    (64, 320),   # the 2-tile form, a wave with one tile, a wave with none
    (33, 257),   # partial query block, one key past a tile
]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(nq, nkv):
    """Host inputs (fp16 values) of one shape and the oracle's output for the SECOND V; shared by
    the plans and the grouped launch, never modified."""
    from lightglue_amd import synth
    from oracle import oracle

    oracle.build()
    qn, kn, vn = synth.qkv(1234 + nq + 7 * nkv, nq, nkv)
    q, k, v1 = (synth.round_f16(x) for x in (qn, kn, vn))
    v2 = synth.round_f16(np.where(v1 >= 0, -v1 - 2.0, -v1 + 2.0).astype(np.float32))
    assert np.abs(v2 - v1).min() >= 2.0
    ref = oracle.attention_c(q, k, v2)
    for a in (q, k, v1, v2, ref):
        a.setflags(write=False)
    return q, k, v1, v2, ref


def _up(x, dev):
    return torch.from_numpy(np.array(x, copy=True)).to(dev).half().contiguous()  # (the cached array is read-only)


def _maxdiff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.mark.parametrize("code", [22, 21])
@pytest.mark.parametrize("nq,nkv", SHAPES)
def test_second_launch_reads_its_own_v(nq, nkv, code, dev):
    from lightglue_amd import _lib

    lib = _lib.load()
    q, k, v1, v2, ref = _case(nq, nkv)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    for of, dt, tol in ((0, torch.float16, TOL), (1, torch.float32, TOL_F32OUT)):
        qa, ka, va = (_up(x, dev) for x in (q, k, v1))
        qb, kb, vb = (_up(x, dev) for x in (q, k, v2))  # fresh allocations for the second launch
        oa = torch.full(qa.shape, float("nan"), dtype=dt, device=dev)
        ob = torch.full(qa.shape, float("nan"), dtype=dt, device=dev)
        torch.cuda.synchronize()
        for qq, kk, vv, oo in ((qa, ka, va, oa), (qb, kb, vb, ob)):  # back to back, one stream
            st = lib.mha_hd64_launch_forced(qq.data_ptr(), kk.data_ptr(), vv.data_ptr(), oo.data_ptr(), 1, 4, nq, nkv,
                                            0, of, code, 0, 0, ws.data_ptr(), ws.numel(), s, 3)
            assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        got = ob.float().cpu().numpy()
        err = _maxdiff(got, ref) if np.isfinite(got).all() else float("inf")
        print(f"plan {code} {nq}x{nkv} {'f32' if of else 'f16'} out: max-abs {err:.3e} (bound {tol:g})")
        assert err <= tol


def test_second_grouped_launch_reads_its_own_v(dev):
    """Two calls in one launch, twice. The kernel is the planner's choice, which the wrapper does not
    report: at 32 blocks of 16 rows it is the 16-row kernel's table form today, and the screen holds
    for whichever kernel a later planner picks."""
    from lightglue_amd import mha_hd64_grouped

    cases = [_case(64, 1024), _case(64, 577)]
    for dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
        first = [tuple(_up(x, dev) for x in (q, k, v1)) for q, k, v1, _, _ in cases]
        second = [tuple(_up(x, dev) for x in (q, k, v2)) for q, k, _, v2, _ in cases]
        outs_a = [torch.full(c[0].shape, float("nan"), dtype=dt, device=dev) for c in first]
        outs_b = [torch.full(c[0].shape, float("nan"), dtype=dt, device=dev) for c in first]
        torch.cuda.synchronize()
        mha_hd64_grouped(first, out_dtype=dt, outs=outs_a)
        mha_hd64_grouped(second, out_dtype=dt, outs=outs_b)
        torch.cuda.synchronize()
        for (_, _, _, _, ref), o in zip(cases, outs_b):
            got = o.float().cpu().numpy()
            err = _maxdiff(got, ref) if np.isfinite(got).all() else float("inf")
            print(f"grouped {tuple(o.shape)} {dt}: max-abs {err:.3e} (bound {tol:g})")
            assert err <= tol
