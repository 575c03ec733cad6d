"""Attention backward without a GPU: the float64 reference against autograd, the C ABI's three symbols,
the workspace query and every argument check (include/mha_hd64.h "backward")."""
import pytest
import torch

A = 4096  # a fake 16-B aligned address: never dereferenced on these paths
HALF, FLOAT = 1, 0
SHAPE = (2, 3, 70, 45)  # batch, heads, nq, nkv


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


@pytest.mark.parametrize("seed,batch,heads,nq,nkv", [(1, 1, 4, 1, 1), (2, 2, 3, 9, 14), (3, 1, 2, 33, 7)])
def test_reference_equals_autograd(seed, batch, heads, nq, nkv):
    from lightglue_amd import attention_backward_reference

    g = torch.Generator().manual_seed(seed)
    q, dout = (torch.randn(batch, heads, nq, 64, generator=g, dtype=torch.float64) for _ in range(2))
    k, v = (torch.randn(batch, heads, nkv, 64, generator=g, dtype=torch.float64) for _ in range(2))
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]
    out = torch.softmax(leaves[0] @ leaves[1].transpose(-1, -2) / 8, -1) @ leaves[2]
    want = torch.autograd.grad(out, leaves, dout)
    scale = max(float(ref.abs().max()) for ref in want)  # (one key: dQ = dK = 0 exactly, so not each tensor's own)
    for got, ref in zip(attention_backward_reference(q, k, v, dout), want):
        assert float((got - ref).abs().max()) <= 1e-12 * scale


def test_symbols_and_workspace_query(lib):
    from lightglue_amd import _lib

    for name in ("mha_hd64_backward_fp16", "mha_hd64_backward_fp32", "mha_hd64_backward_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    ws = lib.mha_hd64_backward_workspace_bytes
    assert ws(*SHAPE, 7) == 0
    for empty in ((0, 3, 70, 45), (2, 0, 70, 45), (2, 3, 0, 45), (2, 3, 70, 0)):
        assert ws(*empty, HALF) == 0 and ws(*empty, FLOAT) == 0
    for b, h, nq, nkv in (SHAPE, (1, 4, 1, 1), (1, 4, 1024, 1024), (8, 4, 130, 257)):
        assert ws(b, h, nq, nkv, FLOAT) > ws(b, h, nq, nkv, HALF) >= 2 * 4 * b * h * nq


def call(lib, fn="mha_hd64_backward_fp16", short=0, **kw):
    a = dict(q=A, k=A, v=A, o=A, dout=A, dq=A, dk=A, dv=A, batch=SHAPE[0], heads=SHAPE[1], nq=SHAPE[2], nkv=SHAPE[3], ws=A)
    a.update(kw)
    need = lib.mha_hd64_backward_workspace_bytes(*SHAPE, HALF if fn.endswith("fp16") else FLOAT)
    return getattr(lib, fn)(a["q"], a["k"], a["v"], a["o"], a["dout"], a["dq"], a["dk"], a["dv"], a["batch"], a["heads"],
                            a["nq"], a["nkv"], a["ws"], need - short, None)


BAD = [{p: None} for p in ("q", "k", "v", "o", "dout", "dq", "dk", "dv", "ws")] + \
      [{p: A + 8} for p in ("q", "dout", "dv", "ws")] + [dict(batch=-1), dict(heads=-1), dict(nq=-1), dict(nkv=-1), dict(nkv=0)]


@pytest.mark.parametrize("fn", ["mha_hd64_backward_fp16", "mha_hd64_backward_fp32"])
@pytest.mark.parametrize("bad", BAD, ids=lambda b: "-".join(f"{k}={v}" for k, v in b.items()))
def test_bad_arguments_return_bad_param(lib, fn, bad):
    from lightglue_amd import _lib

    assert call(lib, fn, **bad) == _lib.STATUS_BAD_PARAM
    assert "assertion failed" in _lib.last_error()


@pytest.mark.parametrize("fn", ["mha_hd64_backward_fp16", "mha_hd64_backward_fp32"])
def test_short_workspace_and_empty_call(lib, fn):
    from lightglue_amd import _lib

    assert call(lib, fn, short=1) == _lib.STATUS_WORKSPACE and "workspace" in _lib.last_error()
    for empty in (dict(nq=0), dict(batch=0), dict(heads=0)):  # a successful no-op, whatever the pointers
        assert call(lib, fn, **empty, q=None, dq=None, ws=None) == _lib.STATUS_SUCCESS
