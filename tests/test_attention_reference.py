"""The attention tests' operands, bounds and restatement (tests/attention_refs.py), checked without a GPU: every
bound accepts the NumPy fp32 restatement of the kernels' arithmetic on every family and shape that
tests/test_gpu_attention_exact.py runs, rejects each mutant of it on the family meant to catch it, and the operands have
the properties the exact families rest on. The seams (splits, waves, passes, tiles) come from the library's own planner
(mha_hd64_plan_route, host code) with the plan fields each GPU test forces.

Two mutants no bound can separate, documented instead of tested:
  * P kept unrounded in one tile only (row sum and P V both from it): the tile's weights are then closer to the exact
    ones than the kernel's, so every bound that accepts the kernel accepts it (`unrounded_tile` in the table below).
  * the row sum taken from the fp32 P shows only where the fp16 roundings of a row's weights do not average out: on
    lazy7 through a slice that starts at tile 0 (a one-wave plan, the streaming kernel), fp32 output.
Under fp16 output a lost key moves a census output by 1 / n of itself against 2^-11 for the output rounding: the
separation of 16 bounds holds for lost, doubled and neighbour-replaced keys up to 2048 keys, at 4500 keys it is 10 to
21 bounds, and a zero row read past the end or a key replaced by one 48 further on separates only under fp32 output,
which every form also runs with (there the separation is unbounded: the bound is a few fp32 ulps).
"""
import numpy as np
import pytest

import attention_refs as R


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def _forms(lib):
    """(label, batch, nq, nkv, plan): every plan and shape of the GPU file (one head is restated)."""
    out = []
    for nq in R.Q_ROWS:
        for nkv, qw, kw, sp, plan in R.ring_forms(lib, nq):
            out.append((f"ring{qw}x{kw}s{plan['splits']}", 1, nq, nkv, plan))
    for nkv, qw, kw, sp, plan in R.ring_forms(lib, 16, keys=(4500,)):
        out.append((f"ring{qw}x{kw}s{plan['splits']}", 1, 16, nkv, plan))
    for code in (21, 22):
        for nq in R.Q_ROWS:
            for nkv in R.ONE_PASS_KEYS + R.TWO_PASS_KEYS:
                out.append((f"direct{code}", 1, nq, nkv, R.plan_of(lib, 1, 4, nq, nkv, code)))
    for nq in (1024, 1056):
        for nkv in (600, 1024) + R.FOUR_PASS_KEYS:
            out.append(("direct21x2", 2, nq, nkv, R.plan_of(lib, 2, 4, nq, nkv, 21)))
    for in_f32 in (0, 1):   # the planner's default, single calls and groups of four
        for b, nq, nkv in R.DEFAULT_SHAPES:
            ws = lib.mha_hd64_launch_workspace_bytes_typed(b, 4, nq, nkv, 0 if in_f32 else 1)
            out.append((f"default{in_f32}", b, nq, nkv, R.plan_of(lib, b, 4, nq, nkv, in_f32=in_f32, ws_bytes=ws)))
        for group in R.GROUPS:
            for (b, nq, nkv), plan in zip(group, R.group_plan(lib, group, in_f32)):
                out.append((f"group{in_f32}", b, nq, nkv, plan))
    for waves in (4, 8):
        b, nq, nkv, _ = R.STREAM_CASE
        out.append((f"stream{waves}", b, nq, nkv, R.plan_of(lib, b, 4, nq, nkv, 23, waves)))
    return out


def _restate_case(case, layout, out16, plan, n=None, mutant=None, at=None, b=0, h=0):
    return R.restate(case["q"][b, h], case["k"][b, h], case["v"][b, h], layout, n=n, out16=out16,
                     block_rows=16 if plan["code"] == 22 else 32, zero_first=plan["code"] == 23, mutant=mutant, at=at)


def _one_head(case, b=0, h=0):
    return {k: (v[b:b + 1, h:h + 1] if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def _as_out(x, out16):
    return x.astype(np.float16) if out16 else x


def test_forms_reach_what_they_name(lib):
    """Every listed plan is the plan that was forced, every layout visits every key once, and the multi-round shapes
    reach the forms they are there for: 2 x 4 x 1024 rows is 256 blocks of 32 rows, NOT past one round (it runs the
    two-pass form), 2 x 4 x 1056 rows is 264 and runs the two-per-CU forms, four passes past 1024 keys."""
    forms = _forms(lib)
    assert len(forms) > 400
    for label, batch, nq, nkv, plan in forms:
        layout = R.plan_layout(plan, nkv)
        assert (R.count_keys(layout, nkv) == 1).all(), (label, nq, nkv)
        assert len(layout) == plan["splits"] or plan["code"] < 21, (label, nq, nkv)
        if label.startswith("direct"):
            assert plan["code"] == int(label[6:8]) and plan["direct_tiles"] == max(1, R.cdiv(nkv, 512)), (label, nq, nkv)
        if label.startswith("stream"):
            assert (plan["code"], plan["kv_waves"]) == (23, int(label[6:]))
    form = lambda nq, nkv: R.direct_form(21, *[R.plan_of(lib, 2, 4, nq, nkv, 21)[k] for k in ("direct_tiles", "blocks")])
    assert form(1024, 2048) == (4, 4, 2) and form(1056, 2048) == (4, 2, 4) and form(1056, 1100) == (4, 2, 4)
    assert form(1056, 1024) == (4, 2, 2) and form(1024, 1024) == (4, 4, 1)
    assert R.direct_form(22, 4, 36) == (4, 4, 2) and R.direct_form(22, 2, 36) == (4, 4, 1)


def test_bounds_accept_the_restatement_exact_families(lib, capsys):
    """check_exact on the restatement: selector rows bit for bit, census and two-level rows inside their ulp bound, both
    output types, every form and shape (the large multi-round shapes: their first 130 rows)."""
    worst = {}
    for label, batch, nq, nkv, plan in _forms(lib):
        layout = R.plan_layout(plan, nkv)
        units = R.layout_units(layout)
        rows = min(nq, 130)
        for fam in ("mixed", "selector"):
            if label.startswith("stream"):
                counts = R.STREAM_CASE[3]
                case = R.exact_case(fam, rows, nkv, lambda n: R.layout_units(R.plan_layout(plan, n)), 11, batch=len(counts),
                                    heads=1, counts=counts)
                items = [(b, R.plan_layout(plan, n), n) for b, n in enumerate(case["counts"])]
            else:
                case = R.exact_case(fam, rows, nkv, units, 11, heads=1)
                items = [(0, layout, None)]
            for out16 in (True, False):
                for b, lay, n in items:
                    got = _restate_case(case, lay, out16, plan, n=n, b=b)
                    w = R.check_exact(_as_out(got, out16)[None, None], _one_head(case, b), len(lay), out16)
                    key = (label.rstrip("0123456789s") if label.startswith("ring") else label, fam, out16)
                    worst[key] = max(worst.get(key, 0.0), w)
    with capsys.disabled():
        for (label, fam, out16), w in sorted(worst.items()):
            print(f"\n  restatement {label:12s} {fam:9s} {'fp16' if out16 else 'fp32'} out: worst error / bound {w:.3f}", end="")
    assert max(worst.values()) <= 1.0


def test_bounds_accept_the_restatement_graded_families(lib, capsys):
    lines = []
    for qw, kw, sp, nq, nkv in R.GRADED_FORMS:
        plan = R.plan_of(lib, 1, 1, nq, nkv, qw, kw, sp)
        layout = R.plan_layout(plan, nkv)
        for name in R.GRADED:
            q, k, v = R.graded_case(name, nq, nkv, 3, heads=1)
            for out16 in (True, False):
                ref, bound = R.graded_bound(q[0, 0], k[0, 0], v[0, 0], out16, R.split_ranges(layout),
                                            3 if plan["code"] in (21, 22) else 1, 8.0 if plan["code"] == 23 else 0.0)
                got = _restate_case(dict(q=q, k=k, v=v), layout, out16, plan)
                w = R.check_graded(got, ref, bound)
                lines.append(f"  restatement plan {plan['code']:2d} x{plan['kv_waves']} s{plan['splits']} {nq}x{nkv} {name:6s} "
                             f"{'fp16' if out16 else 'fp32'} out: worst error / bound {w:.3f} (median bound {np.median(bound):.2e})")
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")


def test_lazy_operands_do_what_they_name():
    """lazy7: tile 0's maximum is 0 and no later tile lifts a row's maximum past 8 log2 units over it, but past 6 (P
    above 64); lazy8p: one tile lifts it by more than 8. Scores are exact in fp32: integers of 2^-14."""
    qt = float(R.f16(np.float32(8.0) * np.float32(R.SCALE_LOG2)))
    assert len(R.lazy_grades()) >= 8
    for nkv in (200, 257, 1000, 1024, 2048):
        for name, lo, hi in (("lazy7", 6.0, 8.0), ("lazy8p", 8.0, 9.0)):
            q, k, v = R.graded_case(name, 3, nkv, 3, heads=1)
            s = qt * k[0, 0, :, 0].astype(np.float64)
            assert (s[:64] == 0).all() and lo < s.max() < hi, (name, nkv, s.max())
            assert np.array_equal(np.float32(qt) * k[0, 0, :, 0], s.astype(np.float32))
            assert (q[..., 1:] == 0).all()


def test_census_sums_and_selector_gap(lib):
    """Every census partial sum is an integer far below 2^24 even under the largest stale weight 2^8; the constant
    column is 1; the gap assert holds at every key count used (and is what exact_case asserts on each call); the
    selector values hold the fp16 extremes and no negative zero."""
    for nkv in sorted(set(R.RING_KEYS + R.ONE_PASS_KEYS + R.TWO_PASS_KEYS + (4500,))):
        v = R.census_v(nkv, 3)
        assert (v == np.round(v)).all() and v.min() == 0 and 256 * v.sum(0).max() < 2 ** 24 and (v[:, 63] == 1).all()
        assert len({tuple(r) for r in v.astype(np.int8)}) == nkv    # every key's row is its own
        plan = R.plan_of(lib, 1, 4, 16, nkv)
        case = R.exact_case("selector", 16, nkv, R.layout_units(R.plan_layout(plan, nkv)), 11, heads=2)
        assert case["gap"] >= R.GAP_MIN
        vs = case["v"]
        assert not np.signbit(vs[vs == 0]).any()
        if nkv >= 257:
            assert vs.max() == 65504 and vs.min() == -65504 and (np.abs(vs[vs != 0]).min() == 2.0 ** -24)
    # at that gap every other P is 0 in fp16, and a rescale factor or split weight past it 0 in fp32
    assert np.float16(np.exp2(np.float32(-R.GAP_MIN))) == 0 and np.float32(2.0) ** np.float32(-R.GAP_MIN) == 0


def test_census_separates_its_mutants(lib, capsys):
    """A key lost, read twice, replaced by another or a zero row read past the end moves some output component of the
    census by at least 16 bounds (the module docstring says where fp16 output limits this). Applied to the float64
    reference."""
    lines = []
    for nkv in (1, 63, 64, 65, 129, 257, 513, 600, 1000, 1024, 1025, 1100, 2048, 4500):
        for splits in (1, 5, 16):
            for out16 in (False, True):
                v = R.census_v(nkv, 1).astype(np.float64)
                tot = v.sum(0)
                ref = tot / nkv
                bound = R.exact_bound(ref[None], np.array([b"c"]), splits, out16)[0]

                def moved(m):
                    with np.errstate(divide="ignore", invalid="ignore"):
                        r = np.abs(m - ref) / bound
                    return float(np.where(np.isnan(r), np.inf, r).max())

                js = np.unique(np.r_[0, 63, 64, 65, nkv - 1, np.arange(0, nkv, max(1, nkv // 37))])
                js = js[js < nkv]
                sep = {"zero row": moved(tot / (nkv + 1)), "doubled": min(moved((tot + v[j]) / (nkv + 1)) for j in js)}
                if nkv > 1:
                    sep["lost"] = min(moved((tot - v[j]) / (nkv - 1)) for j in js)
                    sep["replaced +-1"] = min(moved((tot - v[j] + v[j + d]) / nkv) for j in js for d in (-1, 1)
                                              if 0 <= j + d < nkv)
                if nkv > 64:
                    sep["replaced +-64"] = min(moved((tot - v[j] + v[j + d]) / nkv) for j in js for d in (-64, 64)
                                               if 0 <= j + d < nkv)
                if nkv > 48:
                    sep["replaced +-48"] = min(moved((tot - v[j] + v[j + d]) / nkv) for j in js for d in (-48, 48)
                                               if 0 <= j + d < nkv)
                if splits == 5:
                    lines.append(f"  census {nkv:4d} keys, 5 splits, {'fp16' if out16 else 'fp32'} out: "
                                 + ", ".join(f"{k} {x:.3g}" for k, x in sep.items()))
                if nkv == 1 and out16:
                    continue    # (the only key doubled leaves the mean where it was; fp32 output has no slack at all)
                if not out16:
                    assert min(sep.values()) >= 16, (nkv, splits, sep)
                elif nkv <= 2048 and splits <= 5:
                    assert min(sep[k] for k in sep if k in ("lost", "doubled", "replaced +-1", "replaced +-64")) >= 16, \
                        (nkv, splits, sep)
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")


def test_targets_and_runs_reach_their_seams(lib):
    """pi reaches keys 0, 63, 64, 65, nkv - 1 and the first and last key of every split, pass and wave of the plan (of
    every tile too where the rows suffice), early and late targets alternate between neighbouring rows, and each run B
    lies where its name says, for every form, with the seams taken from the plan."""
    for label, batch, nq, nkv, plan in _forms(lib):
        if label.startswith("stream"):
            continue
        layout = R.plan_layout(plan, nkv)
        units = R.layout_units(layout)
        rows = min(nq, 130)
        case = R.exact_case("selector", rows, nkv, units, 11, heads=4)
        tg = case["targets"][0]
        hit = set(case["target"].ravel().tolist())
        want = [t for t in [nkv - 1, 0, 63, 64, 65] if t < nkv]
        for kind in ("split", "pass", "wave"):
            want += [x for a, b in units[kind] for x in (a, b)]
        assert set(want) <= set(tg), (label, nq, nkv)
        assert hit == set(tg[:min(len(tg), 4 * rows)]), (label, nq, nkv)   # all of them, or the first by priority
        if 4 * rows >= len(set(want)):
            assert set(want) <= hit, (label, nq, nkv)
        t = case["target"][0, 0]
        if rows >= 17 and len(tg) >= 8:     # neighbours differ, and targets move both up and down along the rows
            assert (np.diff(t) != 0).all() and (np.diff(t) > 0).any() and (np.diff(t) < 0).any()
        mixed = R.exact_case("mixed", rows, nkv, units, 11, heads=4)
        runs = mixed["runs"][0]
        sp = units["split"]
        for name, (a, e) in runs.items():
            assert 0 <= a < e <= nkv
            if name == "tile":
                assert a < 64 < e
            if name == "split":
                seams = [x for kind in ("split", "pass", "wave") for x, _ in units[kind] if x > 0]
                assert any(a < x < e for x in seams), (label, nkv, runs)
            if name == "last" and len(sp) > 1:
                assert sp[-1][0] <= a and e - 1 <= sp[-1][1]
            if name == "first" and len(sp) > 1:
                assert e - 1 <= sp[0][1]
        if nkv >= 129:
            assert {"tile", "first"} <= set(runs) and ("last" in runs or runs["split"][1] == nkv), (label, nkv, runs)
        if nkv >= 257 and (len(sp) > 1 or len(units["wave"]) > 1):
            assert "split" in runs or min(x for x, _ in units["wave"] if x > 0) == 64, (label, nkv, runs)
        kinds = set(mixed["kind"].ravel().tolist())
        assert kinds == ({b"c", b"s", b"t"} if 4 * rows >= 3 else kinds)


# ---- the mutants ----------------------------------------------------------------------------------------------------
MEANT = {  # mutant -> the families meant to catch it
    "drop_last": ("census",), "drop_tile_first": ("census",), "double_key": ("census",),
    "zero_row_past_end": ("census",), "count_minus": ("census",), "count_plus": ("census",),
    "swap_v_seam": ("selector",), "kv_shift": ("selector",),
    "equal_weights": ("twolevel", "selector"), "no_rescale": ("selector", "lazy8p"),
    "rowsum_fp32": ("lazy7",), "unrounded_tile": (),
}


def test_every_mutant_fails_on_the_family_meant_for_it(lib, capsys):
    """Each mutant of the restatement through each family's check, at a split ring plan (1000 keys, 3 splits), a
    one-wave walk (the streaming kernel's, 257 keys, an item of 129 keys for the count mutants) and both output
    types: the table is printed, the entries of MEANT are asserted for BOTH output types (rowsum_fp32: fp32 output,
    see the module docstring)."""
    nq = 33
    ring = R.plan_of(lib, 1, 1, nq, 1000, 2, 2, 3)
    walk = R.plan_of(lib, 1, 1, nq, 257, 23, 4)
    table = {}
    for mutant in R.MUTANTS:
        for fam in ("census", "selector", "twolevel", "mixed") + R.GRADED:
            verdict = []
            for plan, nkv in ((ring, 1000), (walk, 257)):
                count = None
                if mutant in ("count_minus", "count_plus"):
                    if plan is ring or fam in R.GRADED:
                        continue
                    count = 129
                n = count or nkv
                layout = R.plan_layout(plan, n)
                for out16 in (True, False):
                    if fam in R.GRADED:
                        q, k, v = R.graded_case(fam, nq, nkv, 3, heads=1)
                        case = dict(q=q, k=k, v=v)
                        ref, bound = R.graded_bound(q[0, 0], k[0, 0], v[0, 0], out16, R.split_ranges(layout), 1,
                                                    8.0 if plan is walk else 0.0)
                    else:
                        case = R.exact_case(fam, nq, nkv, R.layout_units(layout), 11, heads=1,
                                            counts=None if count is None else [count])
                    at = None
                    if mutant == "kv_shift":    # the tile that holds the first target past tile 0 (census: any)
                        at = 64
                    got = _restate_case(case, layout, out16, plan, n=count, mutant=mutant, at=at)
                    clean = _restate_case(case, layout, out16, plan, n=count)
                    try:
                        if fam in R.GRADED:
                            R.check_graded(clean, ref, bound)
                        else:
                            R.check_exact(_as_out(clean, out16)[None, None], case, len(layout), out16)
                    except AssertionError as e:     # the unmutated restatement must pass
                        raise AssertionError(f"unmutated restatement fails on {fam}: {e}")
                    try:
                        if fam in R.GRADED:
                            R.check_graded(got, ref, bound)
                        else:
                            R.check_exact(_as_out(got, out16)[None, None], case, len(layout), out16)
                        verdict.append(False)
                    except AssertionError:
                        verdict.append(True)
            table[mutant, fam] = verdict
    with capsys.disabled():
        print("\n  rejected (ring 3 splits fp16, fp32 | one-wave walk fp16, fp32); R rejected, . accepted")
        for mutant in R.MUTANTS:
            print(f"  {mutant:18s}" + "  ".join(f"{fam} {''.join('R' if x else '.' for x in table[mutant, fam])}"
                                               for fam in ("census", "selector", "twolevel", "mixed") + R.GRADED))
    for mutant, fams in MEANT.items():
        for fam in fams:
            v = table[mutant, fam]
            if mutant == "rowsum_fp32":
                assert v[-1], (mutant, fam, v)           # the one-wave walk, fp32 output
            elif mutant == "equal_weights":
                assert v[0] and v[1], (mutant, fam, v)   # the split plan, both output types
            elif mutant == "no_rescale" and fam == "lazy8p":
                assert v[2] and v[3], (mutant, fam, v)   # the one-wave walk: the lift is a later tile of the same slice
            else:
                assert all(v), (mutant, fam, v)
    assert not any(table["unrounded_tile", fam][i] for fam in R.GRADED for i in range(4))   # documented above


# ---- the old contract on the same mutants ---------------------------------------------------------------------------
def test_old_contract_on_the_mutants_at_2048_keys(lib, capsys):
    """The suite's checks before this file, on the Gaussian operands at 2048 keys through the two-pass form: max-abs
    1e-2 on the ~48 sampled rows the plan tests look at (tests/test_gpu_parity.py), the 1.5e-3 guard of _regress16 on
    the same rows, and this file's graded bound on all rows. What passes is a finding, recorded in
    profiles/attention_exact/INDEX.md; only the unmutated restatement is a condition."""
    nq, nkv = 256, 2048
    plan = R.plan_of(lib, 1, 4, nq, nkv, 22)
    layout = R.plan_layout(plan, nkv)
    rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 48)), nq - 1])
    lines = []
    for seed in (91, 92, 93, 94):
        q, k, v = R.graded_case("gauss1", nq, nkv, seed, heads=1)
        ref, bound = R.graded_bound(q[0, 0], k[0, 0], v[0, 0], True, None, 3)
        for mutant in (None, "drop_last", "drop_tile_first", "double_key", "swap_v_seam"):
            got = R.restate(q[0, 0], k[0, 0], v[0, 0], layout, out16=True, block_rows=16, mutant=mutant).astype(np.float64)
            d = np.abs(got - ref)
            tol = d[rows].max() <= 1e-2
            guard = bool((d[rows] <= 1.5e-3 + np.abs(ref[rows]) * 2.0 ** -11).all())
            new = bool((d <= bound).all())
            lines.append(f"  2048 keys gauss1 seed {seed} {str(mutant):16s}: max error {d.max():.2e} (sampled rows "
                         f"{d[rows].max():.2e}); 1e-2 contract {'passes' if tol else 'FAILS'}, 1.5e-3 guard "
                         f"{'passes' if guard else 'FAILS'}, graded bound {'passes' if new else 'FAILS'} "
                         f"(worst ratio {float((d / bound).max()):.2f})")
            if mutant is None:
                assert tol and guard and new
    with capsys.disabled():
        print("\n" + "\n".join(lines), end="")
