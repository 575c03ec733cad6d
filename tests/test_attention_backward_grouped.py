"""mha_hd64_backward_grouped_lens without a GPU: symbols, workspace query, argument checks (fake addresses, never read)."""
import ctypes

import pytest

from lightglue_amd import _lib

A, HALF, FLOAT = 4096, 1, 0  # A: a fake 16-B aligned address
SHAPES = [(3, 4, 70, 70), (3, 4, 45, 45), (3, 4, 70, 45), (3, 4, 45, 70)]  # batch, heads, nq, nkv
ODD = (ctypes.c_void_p * 4)(None, A + 2, None, None)  # a lens table that is not 4-B aligned


def descs(shapes, **kw):
    arr = (_lib.BwdCallDesc * max(len(shapes), 1))()
    for i, s in enumerate(shapes):
        arr[i] = _lib.BwdCallDesc(A, A, A, A, A, A, A, A, *s)
    for name, value in kw.items():  # (the override goes into call 1)
        setattr(arr[1], name, value)
    return arr


def call(arr, n=4, in_type=HALF, ws=A, short=0, q_lens=None, kv_lens=None):
    lib = _lib.load()
    need = lib.mha_hd64_backward_grouped_workspace_bytes(descs(SHAPES), 4, HALF)
    return lib.mha_hd64_backward_grouped_lens(arr, q_lens, kv_lens, n, in_type, ws, need - short, None)


def test_symbols_and_workspace_query():
    lib = _lib.load()
    for name in ("mha_hd64_backward_grouped_lens", "mha_hd64_backward_grouped_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    ws = lib.mha_hd64_backward_grouped_workspace_bytes
    stats = lambda shapes: sum(2 * 4 * b * h * nq for b, h, nq, _ in shapes)  # noqa: E731
    assert ws(descs(SHAPES), 0, HALF) == 0 and ws(None, 0, HALF) == 0
    assert ws(descs(SHAPES), 4, 7) == 0 and ws(descs(SHAPES), 4, FLOAT) == 0
    assert ws(descs(SHAPES), 4, HALF) >= stats(SHAPES)
    five = SHAPES + [(8, 4, 300, 300)]
    assert ws(descs(five), 5, HALF) == max(ws(descs(five[:4]), 4, HALF), ws(descs(five[4:]), 1, HALF)) >= stats(five[4:])


BAD = [{p: None} for p in ("q", "k", "v", "o", "dout", "dq", "dk", "dv")] + [{p: A + 8} for p in ("q", "dout", "dv")] + \
      [dict(batch=-1), dict(heads=-1), dict(nq=-1), dict(nkv=-1), dict(nkv=0)]
BAD_ARGS = [dict(in_type=FLOAT), dict(in_type=7), dict(ws=None), dict(ws=A + 8), dict(q_lens=ODD), dict(kv_lens=ODD), dict(n=-1)]


@pytest.mark.parametrize("bad", BAD + BAD_ARGS, ids=lambda b: "-".join(b))
def test_bad_param_before_any_device_call(bad):
    in_call = bad in BAD  # (a field of call 1, else an argument of the launch)
    assert call(descs(SHAPES, **(bad if in_call else {})), **({} if in_call else bad)) == _lib.STATUS_BAD_PARAM
    assert "assertion failed" in _lib.last_error()


def test_null_calls_short_workspace_and_empty_calls():
    assert call(None) == _lib.STATUS_BAD_PARAM
    assert call(descs(SHAPES), short=1) == _lib.STATUS_WORKSPACE and "workspace" in _lib.last_error()
    assert call(None, n=0, ws=None) == _lib.STATUS_SUCCESS
    for empty in ((0, 4, 70, 70), (3, 0, 70, 70), (3, 4, 0, 0)):  # successful no-ops, whatever the pointers
        assert call(descs([empty] * 4, q=None, dk=None), ws=None) == _lib.STATUS_SUCCESS
