"""The FFN backward without a GPU: the C ABI, the registered ops' fake implementations, the host rule for the split."""
import importlib.util
import os

import pytest
import torch

from conftest import REPO

_spec = importlib.util.spec_from_file_location("ffn_backward_host_check", os.path.join(REPO, "tools", "ffn_backward_host_check.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)


def test_symbols_in_header_and_signatures():
    from lightglue_amd import _lib

    with open(os.path.join(REPO, "include", "lightglue_glue.h")) as f:
        text = f.read()
    assert "size_t lg_ffn_backward_workspace(int32_t m_rows);" in text
    assert "int32_t lg_ffn_backward(const void* x, const void* ctx0, const void* ctx1, int32_t heads, int32_t n0" in text
    assert "#define LG_GLUE_ABI_VERSION 4" in text
    assert len(_lib.SIGNATURES["lg_ffn_backward"][0]) == 25 and len(_lib.SIGNATURES["lg_ffn_backward_workspace"][0]) == 1


def test_ops_have_fake_implementations():
    import lightglue_amd  # noqa: F401  (registers the ops)

    h = dict(dtype=torch.float16, device="meta")
    x, c0, c1 = torch.empty((1, 10, 256), **h), torch.empty((1, 4, 4, 64), **h), torch.empty((1, 4, 6, 64), **h)
    w1, v, w2, b2 = torch.empty((512, 512), **h), torch.empty((512,), **h), torch.empty((256, 512), **h), torch.empty((256,), **h)
    out = torch.ops.lightglue_amd.ffn(x, c0, c1, w1, v, v, v, 1e-5, w2, b2)
    assert out.shape == x.shape and out.dtype == torch.float16
    grads = torch.ops.lightglue_amd.ffn_backward(x, c0, c1, w1, v, v, v, 1e-5, w2, out)
    assert [g.shape for g in grads] == [t.shape for t in (x, c0, c1, w1, v, v, v, w2, b2)]
    assert [g.dtype for g in grads] == [torch.float16] * 3 + [torch.float32] * 6
    data = torch.ops.lightglue_amd.ffn_backward(x, c0, c1, w1, v, v, v, 1e-5, w2, out, False)
    assert [g.shape for g in data] == [t.shape for t in (x, c0, c1)]


def test_split_rule_agrees_with_the_library():
    from lightglue_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    for pr, n0, n1 in host.CASES.values():
        m = pr * (n0 + n1)
        assert lib.lg_ffn_backward_workspace(m) == host.workspace_bytes(m), m
    assert [host.splits(m) for m in (1, 320, 321, 65536)] == [1, 1, 20, 20] and lib.lg_ffn_backward_workspace(0) == 0


def test_arguments_are_checked_before_any_device_call():
    """Made-up aligned addresses, never dereferenced: a good call has no rows; dctx aliasing ctx, a partial set of
    parameter gradients, heads != 4 and a misaligned pointer are refused."""
    from lightglue_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    a = dict(x=0x1000, c0=0x2000, c1=0x3000, heads=4, n0=8, n1=8, pairs=1, w1=0x4000, b1=0x5000, g=0x6000, be=0x7000, eps=1e-5,
             w2=0x8000, dy=0x9000, dx=0xa000, d0=0xb000, d1=0xc000, dw1=None, db1=None, dg=None, dbe=None, dw2=None, db2=None,
             ws=0xd000, stream=None)
    call = lambda **kw: lib.lg_ffn_backward(*{**a, **kw}.values())  # noqa: E731
    assert call(pairs=0) == 0
    for bad in (dict(d0=a["c0"]), dict(d1=a["c1"]), dict(dx=a["x"]), dict(dx=a["dy"]), dict(dw1=0xe000), dict(heads=8),
                dict(dy=0x9002), dict(ws=None)):
        assert call(**bad) != 0, bad
