"""The assignment loss without a GPU: the float64 reference's autograd against the closed form the kernels
evaluate, the host check (the kernels' roundings on the CPU) against its committed figures, and the C ABI."""
import importlib.util
import os

import pytest

from conftest import REPO

_spec = importlib.util.spec_from_file_location("assign_nll_host_check", os.path.join(REPO, "tools", "assign_nll_host_check.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)


@pytest.mark.parametrize("name", ["strip", "ragged"])
def test_reference_gradient_is_the_closed_form(name):
    ops = host.operands(name)
    for what, x, ref in zip(host.NAMES, host.closed_form(*ops, emulate=False), host.reference(*ops)):
        assert host.rel(x, ref) <= 1e-12, what   # float64 on both sides: summation order only


def test_host_check_within_committed_figures():
    with open(os.path.join(REPO, "profiles", "assign_nll", "host_check.txt")) as f:
        committed = {ln.split()[1]: float(ln.split()[2]) for ln in f if ln.startswith("worst")}
    assert sorted(committed) == sorted(host.NAMES)
    for name in host.CASES:
        ops = host.operands(name)
        for what, x, ref in zip(host.NAMES, host.closed_form(*ops, emulate=True), host.reference(*ops)):
            assert host.rel(x, ref) <= committed[what], (name, what)


def test_symbols_in_header():
    with open(os.path.join(REPO, "include", "lightglue_glue.h")) as f:
        text = f.read()
    assert "size_t lg_assign_nll_workspace(int32_t m, int32_t n, int32_t batch);" in text
    assert "int32_t lg_assign_nll(const void* v, int64_t pair_stride, int32_t ld, int32_t zc, int32_t m" in text
    assert "#define LG_GLUE_ABI_VERSION 4" in text
