"""The attention backward's operands, bounds and restatement (tests/attention_backward_refs.py), checked without a GPU:
the restated planner gives the plans the shapes are there for; the NumPy fp32 restatement of the three kernels passes
every exact family (equality with the rounded float64 reference) and the graded bound at every shape that
tests/test_gpu_attention_backward_exact.py runs; every mutant of it is rejected by at least one exact-family check; and
the criterion of tests/test_gpu_attention_backward.py (host.rel against BOUND, tensor-wide) is applied to the same
mutants on its own eleven cases, with what it accepts printed.
"""
import importlib.util
import os

import numpy as np
import pytest

import attention_backward_refs as B
from conftest import REPO

_spec = importlib.util.spec_from_file_location("attention_backward_host_check",
                                               os.path.join(REPO, "tools", "attention_backward_host_check.py"))
host = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(host)

# No existing case gives the cols kernel a split of more than one block that starts at an odd block: the stage_parity
# mutant cannot show there (test_old_criterion_on_the_mutants asserts that it changes nothing).
for _c in host.CASES:
    for _f32 in (False, True):
        assert not B.odd_multiblock_splits(B.plan_backward(*_c[1:5], _f32, forced=0)), _c

MUTANT_SHAPES = [(1, 4, 1, 1), (2, 3, 70, 45), (1, 4, 130, 129), (1, 1, 2050, 64), (1, 4, 313, 1024)]
NAMES = ("dq", "dk", "dv")


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def _both_types(case, mutant=None):
    """{out16: (dq, dk, dv)} of the restatement: computed once, the fp16 form is the fp32 form rounded (restate)."""
    got = B.restate(case, False, mutant=mutant)
    return {False: got, True: tuple(B.round_out(g, True) for g in got)}


def _rejects(got, ref, out16):
    """None if (dq, dk, dv) pass check_exact, else the first message."""
    for g, r, n in zip(got, ref, NAMES):
        try:
            B.check_exact(g, r, out16, n)
        except AssertionError as e:
            return str(e)
    return None


def test_plans_are_what_the_shapes_are_there_for(lib, monkeypatch):
    monkeypatch.delenv("MHA_HD64_BWD_SPLITS", raising=False)
    for shape, claim in B.SHAPES.items():
        plan = B.plan_for(lib, *shape)
        assert (plan["splits"], plan["tiles_per_split"]) == claim, (shape, plan)
        blocks = B.split_blocks(plan)
        assert blocks[0][0] == 0 and blocks[-1][1] == plan["qtiles"] and all(a < e for a, e in blocks)
        assert all(blocks[i][1] == blocks[i + 1][0] for i in range(len(blocks) - 1))
    short = B.split_blocks(B.plan_for(lib, 1, 1, 1025, 64))[-1]
    assert short[1] - short[0] == 1                                                   # the last split is short
    assert B.odd_multiblock_splits(B.plan_for(lib, *B.FORCED_SHAPE))[0] == (3, 6)     # odd starts, three blocks each
    assert max(p["splits"] for p in (B.plan_for(lib, *s) for s in B.SHAPES)) == 16
    assert B.plan_for(lib, 8, 4, 130, 256)["splits"] == 2 and B.plan_for(lib, 8, 4, 130, 257)["splits"] == 1
    for forced, want in zip(B.FORCED_SPLITS, ((1, 33), (2, 17), (11, 3))):
        monkeypatch.setenv("MHA_HD64_BWD_SPLITS", str(forced))
        plan = B.plan_for(lib, *B.FORCED_SHAPE)     # (asserted against the library, which reads the variable per call)
        assert (plan["splits"], plan["tiles_per_split"]) == want
    assert B.odd_multiblock_splits(plan) and B.odd_multiblock_splits(B.plan_backward(*B.FORCED_SHAPE, False, forced=2))


def test_seams_targets_and_runs(lib):
    for shape in B.SHAPES:
        plan = B.plan_for(lib, *shape)
        nq, nkv = shape[2:]
        s = B.seams(plan)
        assert s["q_block"][0][0] == 0 and s["q_block"][-1][1] == nq - 1 and s["k_block"][-1][1] == nkv - 1
        assert s["q_split"][0][0] == 0 and s["q_split"][-1][1] == nq - 1 and len(s["q_split"]) == plan["splits"]
        case = B.exact_case("selector", plan)
        hit = set(case["target"].ravel().tolist())
        want = {nkv - 1, 0} | {x for ab in s["k_block"] for x in ab}
        assert want <= hit or shape[1] * nq < len(want), (shape, want - hit)
        for r0, r1 in B.seam_query_pairs(plan):     # one key selected from both sides of every query seam
            assert (case["target"][..., r0] == case["target"][..., r1]).all()
        runs = B.key_runs(nkv)
        assert all(e - a in (2, 4) and 0 <= a < e <= nkv for a, e in runs) and (nkv < 2 or runs)
        assert nkv < 2 or any(e == nkv for _, e in runs)
        assert nkv <= 64 or any(a < 64 < e for a, e in runs)
        mixed = B.exact_case("mixed", plan)
        if runs and nq > 1:
            assert set(mixed["kind"].ravel().tolist()) == {b"s", b"t"}
            if shape[0] * shape[1] > 1:     # the kind of a row differs between neighbouring heads: so does its L
                k = mixed["kind"].reshape(-1, nq)
                assert (k[0] != k[1]).all()


@pytest.mark.parametrize("shape", list(B.SHAPES), ids=lambda s: "x".join(map(str, s)))
def test_restatement_passes_the_exact_families(shape, lib, capsys):
    lines = []
    for fam in B.families_of(shape):
        case, ref = B.case_and_reference(lib, fam, shape)     # (asserts the family's conditions)
        both = _both_types(case)
        for out16 in (True, False):
            w = [B.check_exact(g, r, out16, f"{shape} {fam} {n}") for g, r, n in zip(both[out16], ref, NAMES)]
            assert max(w) <= 1.0
            lines.append(f"  restatement {'x'.join(map(str, shape))} {fam:9s} {'fp16' if out16 else 'fp32'} out: equal to "
                         f"the rounded reference; worst error / bound dq {w[0]:.3f} dk {w[1]:.3f} dv {w[2]:.3f}")
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")


@pytest.mark.parametrize("shape", B.GRADED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_passes_the_graded_bound(shape, lib, capsys):
    lines = []
    for fam in B.GRADED:
        case, _ = B.case_and_reference(lib, fam, shape)
        for out16 in (True, False):
            got = B.restate(case, out16)
            worst = [0.0, 0.0, 0.0]
            for b in range(shape[0]):
                for h in range(shape[1]):
                    refs, bounds = B.graded_bound(case, b, h, out16)
                    for i, n in enumerate(NAMES):
                        worst[i] = max(worst[i], B.check_graded(got[i][b, h], refs[i], bounds[i], f"{shape} {fam} {n}"))
            lines.append(f"  restatement {'x'.join(map(str, shape))} {fam:6s} {'fp16' if out16 else 'fp32'} out: worst "
                         f"error / bound dq {worst[0]:.3f} dk {worst[1]:.3f} dv {worst[2]:.3f}")
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")


def test_every_mutant_is_rejected_by_an_exact_family(lib, capsys):
    """Each mutant through every exact family at MUTANT_SHAPES, both output types: the first check that rejects it is
    printed with the whole table, and every mutant must be rejected somewhere (the unmutated restatement nowhere)."""
    table, first = {}, {}
    for shape in MUTANT_SHAPES:
        for fam in B.families_of(shape):
            case, ref = B.case_and_reference(lib, fam, shape)
            for mutant in (None,) + B.MUTANTS:
                both = _both_types(case, mutant)
                for out16 in (True, False):
                    msg = _rejects(both[out16], ref, out16)
                    if mutant is None:
                        assert msg is None, msg
                        continue
                    table.setdefault((mutant, fam), []).append(msg is not None)
                    if msg is not None and mutant not in first:
                        first[mutant] = f"{fam} at {'x'.join(map(str, shape))}, {'fp16' if out16 else 'fp32'} out: {msg}"
    with capsys.disabled():
        print("\n  rejected anywhere over " + ", ".join("x".join(map(str, s)) for s in MUTANT_SHAPES) +
              " (R rejected, . accepted everywhere)")
        for mutant in B.MUTANTS:
            print(f"  {mutant:18s}" + "  ".join(f"{fam} {'R' if any(table.get((mutant, fam), [])) else '.'}"
                                               for fam in B.EXACT))
            print(f"  {'':18s}first rejected by {first.get(mutant, 'NOTHING')}")
    assert set(first) == set(B.MUTANTS), set(B.MUTANTS) - set(first)
    # what each family is there for
    for mutant, fams in {"drop_last_key": ("census_q0", "twolevel"), "drop_last_query": ("census_q0", "census_k0", "selector"),
                         "drop_split_first": ("census_k0", "selector"), "double_block": ("census_k0", "selector"),
                         "reduce_omits_last": ("census_k0", "selector"), "stage_parity": ("census_k0", "selector"),
                         "tail_in_L": ("census_q0",), "head0_stats": ("mixed",), "no_D": ("selector",),
                         "eighth_twice": ("census_q0", "census_k0", "twolevel"), "kv_shift": ("selector",)}.items():
        for fam in fams:
            assert any(table[mutant, fam]), (mutant, fam)


def test_old_criterion_on_the_mutants(lib, capsys):
    """The criterion of tests/test_gpu_attention_backward.py, host.rel against its BOUND, on its eleven cases (O = fp16
    of the float64 forward, as the host check takes it), applied to every mutant of the restatement. What it accepts is
    a finding and is printed; the unmutated restatement must pass, and stage_parity must change no bit there."""
    import torch

    import test_gpu_attention_backward as old
    from lightglue_amd import attention_backward_reference

    accepted = {m: [] for m in B.MUTANTS}
    for c in host.CASES:
        name, shape = c[0], tuple(c[1:5])
        x = [t.half().float() for t in host.inputs(c)]
        ref = attention_backward_reference(*(t.half() for t in x))
        q, k, v, dout = (t.numpy() for t in x)
        o, _ = B.R.softmax64(q, k, v)
        case = dict(q=q, k=k, v=v, o=B.f16(o), dout=dout, plan=B.plan_for(lib, *shape))
        results = {m: _both_types(case, m) for m in (None,) + B.MUTANTS}
        for dtype in (torch.float16, torch.float32):
            out16 = dtype == torch.float16
            clean = results[None][out16]
            for mutant in (None,) + B.MUTANTS:
                got = results[mutant][out16]
                errs = [host.rel(torch.from_numpy(g.astype(np.float64)), r) for g, r in zip(got, ref)]
                ok = all(np.isfinite(g).all() for g in got) and all(e <= b for e, b in zip(errs, old.BOUND[dtype]))
                if mutant is None:
                    assert ok, (name, dtype, errs)
                elif ok:    # (=: the mutant does not apply to this plan, the result is the unmutated one bit for bit)
                    same = all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, clean))
                    accepted[mutant].append(f"{name}/{'fp16' if out16 else 'fp32'}{'=' if same else ''}")
                if mutant == "stage_parity":
                    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, clean)), name
    with capsys.disabled():
        print("\n  the tensor-wide criterion (host.rel <= BOUND) accepts (=: the mutant changes no bit at that plan):")
        for m in B.MUTANTS:
            print(f"  {m:18s}{len(accepted[m]):2d} of 22: {' '.join(accepted[m]) or '-'}")
    assert len(accepted["stage_parity"]) == 2 * len(host.CASES)
