"""The projections' backward without a GPU: the C ABI, the argument checks, the host rule for the split, the registered
ops' fake implementations."""
import ctypes
import importlib.util
import os

import pytest
import torch

from conftest import REPO

_spec = importlib.util.spec_from_file_location("proj_backward_host_check", os.path.join(REPO, "tools", "proj_backward_host_check.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)


def test_symbols_in_header_and_signatures():
    from lightglue_amd import _lib

    with open(os.path.join(REPO, "include", "lightglue_glue.h")) as f:
        text = f.read()
    assert "size_t lg_proj_backward_workspace(int32_t kind, int32_t m_rows, int32_t n_store);" in text
    assert "int32_t lg_proj_backward(int32_t kind, const void* x, const void* w, const void* cosv, const void* sinv," in text
    assert "#define LG_GLUE_ABI_VERSION 4" in text
    assert len(_lib.SIGNATURES["lg_proj_backward"][0]) == 18 and len(_lib.SIGNATURES["lg_proj_backward_workspace"][0]) == 3


def test_split_rule_agrees_with_the_library():
    from lightglue_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    for kind, k in host.KINDS.items():
        for m in (1, 64, 65, host.SPLIT_ROWS, host.SPLIT_ROWS + 1, 32768):
            assert lib.lg_proj_backward_workspace(k, m, 384) == host.workspace_bytes(kind, m), (kind, m)
        assert lib.lg_proj_backward_workspace(k, 0, 384) == 0
    assert lib.lg_proj_backward_workspace(0, 64, 384) == 0 and lib.lg_proj_backward_workspace(3, 64, 100) == 0


def test_arguments_are_checked_before_any_device_call():
    """Made-up aligned addresses, never dereferenced: a good call has no rows; every clause of the header's list is
    refused with BAD_PARAM (1): dx inside x's bytes, across a gradient's, or a shifted dx_add among them."""
    from lightglue_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built")
    lib = _lib.load()
    a = dict(kind=2, x=0x1000, w=0x2000, cos=0x3008, sin=0x4008, grads=[0x5000, 0x6000, None, 0x7000, 0x8000, None], ld=0,
             n_store=0, heads=4, n0=8, n1=8, pairs=1, dx_add=0x10000, dx=0x20000, dw=None, db=None, ws=0x30000, stream=None)

    def call(**kw):
        v = {**a, **kw}
        v["grads"] = (ctypes.c_void_p * 6)(*v["grads"]) if v["grads"] is not None else None
        return lib.lg_proj_backward(*v.values())

    plain = dict(kind=3, grads=[0x5000] + [None] * 5, ld=384, n_store=384)
    assert call(pairs=0) == 0 and call(n0=0, n1=0) == 0 and call(pairs=0, **plain) == 0 and call(pairs=0, kind=1) == 0
    bad = [dict(kind=0), dict(kind=4), dict(heads=8), dict(n0=-1), dict(n1=-1), dict(pairs=-1), dict(x=0x1008), dict(w=0x2008),
           dict(dx=0x20008), dict(dx_add=0x10008), dict(ws=0x30008), dict(cos=0x3004), dict(sin=0x4004), dict(cos=None),
           dict(sin=None), dict(grads=[0x5008] + [None] * 5), dict(grads=None), dict(dx=a["x"]), dict(dx=0x7000), dict(dx=0x1010),
           dict(dx=0x6ff0), dict(dx_add=0x20010), dict(n0=1 << 20, n1=1), dict(x=None), dict(ws=None), dict(dw=0xc004), dict(db=0xc004)]
    bad += [{**plain, **kw} for kw in (dict(n_store=0), dict(n_store=100), dict(n_store=576), dict(ld=320), dict(ld=386))]
    for kw in bad:
        assert call(**kw) == 1, kw


def test_ops_have_fake_implementations():
    import lightglue_amd  # noqa: F401  (registers the ops)

    h = dict(dtype=torch.float16, device="meta")
    ops = torch.ops.lightglue_amd
    x, cs = torch.empty((1, 20, 256), **h), torch.empty((1, 20, 64), **h)
    heads = lambda *ns: [(2, 4, n, 64) for n in ns]  # noqa: E731
    out = ops.qkv_rotary(x, torch.empty((768, 256), **h), torch.empty((768,), **h), cs, cs, 4, 6, 2)
    assert [tuple(o.shape) for o in out] == heads(4, 4, 4, 6, 6, 6) and all(o.dtype == torch.float16 for o in out)
    out = ops.split2(x, torch.empty((512, 256), **h), torch.empty((512,), **h), 4, 6, 2)
    assert [tuple(o.shape) for o in out] == heads(4, 6, 4, 6)
    w = torch.empty((384, 256), dtype=torch.float32, device="meta")
    v = ops.project(x, w, torch.empty((384,), **h))
    assert tuple(v.shape) == (1, 20, 384) and v.dtype == torch.float16
    got = ops.proj_backward(3, x, w, [v.float()], 20, 0, 1)
    assert [tuple(g.shape) for g in got] == [(1, 20, 256), (384, 256), (384,)]
    assert [g.dtype for g in got] == [torch.float16, torch.float32, torch.float32]
    assert len(ops.proj_backward(1, x, w, [None] * 4, 4, 6, 2, need_params=False)) == 1
