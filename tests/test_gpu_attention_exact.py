"""The attention kernels on the MI355X against tests/attention_refs.py: operands on which every key counts exactly
once (census, selector, two-level and mixed rows: bitwise or a few fp32 ulps, no modelled term) and graded operands
under the derived elementwise bound, all rows, through every entry point and form: mha_hd64_launch_forced with every
ring plan (WG_SHAPES x realisable split counts), the single-pass kernels' one-, two- and four-pass forms and the
streaming kernel; mha_hd64_launch_stream_lens with key counts; mha_hd64_grouped with key and query counts and with four
calls in one launch; the planner's default through mha_hd64 and mha_hd64_batched, fp16 and fp32 inputs; both forms of
the split combine. Each test asserts the plan (mha_hd64_plan_route with the fields it forces, mha_hd64_plan for the
default) and the combine form (mha_hd64_last_combine_form) that ran, and takes its seams from that plan.

Guards as in tests/test_gpu_projections.py: outputs start as NaN between sentinel bytes, Q, K and V lie between NaN
rows, the workspace is filled with a byte pattern before every launch. Each test prints its worst error / bound.
tests/test_attention_reference.py shows, without a GPU, what these checks reject.
"""
import ctypes

import numpy as np
import pytest

import attention_refs as R
from gpu_common import SENTINEL_BYTE, GuardedIn, GuardedOut

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

HEADS = 4
WS_BYTES = 32 << 20
WS_PATTERN = 0x5A


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib(dev):
    from lightglue_amd import _lib

    return _lib.load()


@pytest.fixture(scope="module")
def ws(dev):
    return torch.empty(WS_BYTES, dtype=torch.uint8, device=dev)


@pytest.fixture
def fused_switch(lib):
    yield lib.mha_hd64_set_fused_combine
    lib.mha_hd64_set_fused_combine(1)


def _report(capsys, what, worst):
    with capsys.disabled():
        print(f"\n  {what}: worst error / bound {worst:.3f}", end="")


class Operands:
    """Q, K, V of one case on the device, each between NaN rows, as fp16 and (on demand) fp32."""

    def __init__(self, q, k, v, dev):
        self.host = (q, k, v)
        self.dev = dev
        self.by_type = {}

    def of(self, dtype):
        if dtype not in self.by_type:
            self.by_type[dtype] = [GuardedIn(torch.from_numpy(np.ascontiguousarray(x)).to(dtype), self.dev)
                                   for x in self.host]
        return self.by_type[dtype]


def _guards_ok(out, what):
    assert bool((out.buf[:out.lo] == SENTINEL_BYTE).all()), f"{what}: wrote before the output"
    assert bool((out.buf[out.hi:] == SENTINEL_BYTE).all()), f"{what}: wrote past the output"
    return out.view.cpu().numpy()


def _forced(lib, ws, ops, shape, in_f32, out_f32, qw, kw, sp, what):
    """One guarded mha_hd64_launch_forced -> (output as numpy, combine form)."""
    from lightglue_amd import _lib

    batch, nq, nkv = shape
    q, k, v = ops.of(torch.float32 if in_f32 else torch.float16)
    out = GuardedOut((batch, HEADS, nq, 64), torch.float32 if out_f32 else torch.float16, ops.dev)
    ws.fill_(WS_PATTERN)
    st = lib.mha_hd64_launch_forced(q.ptr, k.ptr, v.ptr, out.ptr, batch, HEADS, nq, nkv, int(in_f32), int(out_f32), qw, kw,
                                    sp, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream, 3)
    assert st == 0, (what, _lib.last_error())
    form = lib.mha_hd64_last_combine_form()
    torch.cuda.synchronize()
    return _guards_ok(out, what), form


def _exact_through_forced(lib, ws, dev, batch, nq, nkv, qw, kw, sp, families, types=((0, 0), (0, 1), (1, 1)), seed=11):
    """The exact families through one forced plan, every (in_f32, out_f32) of `types` that the plan takes -> the worst
    error / bound. Asserts the plan and the combine form that ran."""
    worst = 0.0
    if qw in (21, 22, 23):      # (the forced single-pass and streaming kernels take fp16 inputs only)
        types = tuple(t for t in types if not t[0])
    plans = {i32: R.plan_of(lib, batch, HEADS, nq, nkv, qw, kw, sp, in_f32=i32, ws_bytes=WS_BYTES) for i32, _ in types}
    plan = plans[0]
    for pl in plans.values():
        assert pl["code"] == qw and (kw == 0 or pl["kv_waves"] == kw or qw in (21, 22)), (pl, qw, kw)
        assert qw >= 21 or kw >= 4 or pl["splits"] == sp, (pl, sp)
        assert R.plan_layout(pl, nkv) == R.plan_layout(plan, nkv)
    units = R.layout_units(R.plan_layout(plan, nkv))
    for fam in families:
        case = R.exact_case(fam, nq, nkv, units, seed, batch=batch, heads=HEADS)
        ops = Operands(case["q"], case["k"], case["v"], dev)
        for i32, o32 in types:
            what = (f"plan {qw}x{kw} splits {plan['splits']} {batch}x{nq}x{nkv} {fam} in{'32' if i32 else '16'} "
                    f"out{'32' if o32 else '16'}")
            got, form = _forced(lib, ws, ops, (batch, nq, nkv), i32, o32, qw, kw, sp, what)
            assert form == (1 if plan["splits"] > 1 else 0), (what, form)
            try:
                worst = max(worst, R.check_exact(got, case, plan["splits"], not o32))
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from None
    return worst


# ---- mha_hd64_launch_forced: the ring plans -------------------------------------------------------------------------
@pytest.mark.parametrize("nkv", R.RING_KEYS)
def test_ring_plans_exact(nkv, lib, ws, dev, capsys):
    """Codes 1, 2, 4 and 12 with every kv-wave count of WG_SHAPES and every realisable split count, 1 to 130 query rows,
    fp16 and fp32 output, fp32 input: mixed rows (census, selector, two-level) and selector rows on Gaussian values."""
    worst, n = 0.0, 0
    for nq in R.Q_ROWS:
        for _, qw, kw, sp, _ in R.ring_forms(lib, nq, keys=(nkv,)):
            worst = max(worst, _exact_through_forced(lib, ws, dev, 1, nq, nkv, qw, kw, sp, ("mixed", "selector")))
            n += 1
    assert n >= 4 * len(R.WG_SHAPES)
    _report(capsys, f"ring plans, {nkv} keys, {n} plans", worst)


def test_ring_many_splits_exact(lib, ws, dev, capsys):
    """16 x 4500: up to 9 splits of one super-tile (1 x 8) and 5 of many (2 x 2)."""
    worst = 0.0
    forms = R.ring_forms(lib, 16, keys=(4500,))
    assert max(f[4]["splits"] for f in forms) >= 9
    for _, qw, kw, sp, _ in forms:
        worst = max(worst, _exact_through_forced(lib, ws, dev, 1, 16, 4500, qw, kw, sp, ("mixed", "selector")))
    _report(capsys, f"ring plans, 4500 keys, {len(forms)} plans", worst)


COMBINE_SHAPES = [(33, 257, 4, 1, 2), (130, 1000, 2, 2, 3), (130, 1000, 12, 2, 3), (17, 1000, 1, 8, 0), (33, 1000, 2, 4, 0),
                  (1, 129, 1, 2, 2), (16, 4500, 1, 8, 0), (16, 4500, 2, 2, 5)]


@pytest.mark.parametrize("out_f32", [0, 1])
def test_split_combine_both_forms_exact(out_f32, lib, ws, dev, fused_switch, capsys):
    """The in-launch combine (arrival tickets) and the combine kernel: each asserted as the form that ran, each inside
    the exact bounds, and the same bits."""
    worst = 0.0
    for nq, nkv, qw, kw, sp in COMBINE_SHAPES:
        plan = R.plan_of(lib, 1, HEADS, nq, nkv, qw, kw, sp, ws_bytes=WS_BYTES)
        assert plan["code"] == qw and plan["kv_waves"] == kw and plan["splits"] > 1
        units = R.layout_units(R.plan_layout(plan, nkv))
        for fam in ("mixed", "selector"):
            case = R.exact_case(fam, nq, nkv, units, 13, heads=HEADS)
            ops = Operands(case["q"], case["k"], case["v"], dev)
            outs = []
            for fused in (0, 1):
                fused_switch(fused)
                what = f"plan {qw}x{kw} splits {plan['splits']} {nq}x{nkv} {fam} fused {fused}"
                got, form = _forced(lib, ws, ops, (1, nq, nkv), 0, out_f32, qw, kw, sp, what)
                assert form == (1 if fused else 2), (what, form)
                worst = max(worst, R.check_exact(got, case, plan["splits"], not out_f32))
                outs.append(got)
            assert np.array_equal(outs[0].view(np.uint8), outs[1].view(np.uint8)), (nq, nkv, qw, kw, sp, fam)
    _report(capsys, f"split combine, both forms, {'fp32' if out_f32 else 'fp16'} output", worst)


# ---- mha_hd64_launch_forced: the single-pass kernels and the streaming kernel ---------------------------------------
@pytest.mark.parametrize("code", [21, 22])
@pytest.mark.parametrize("nkv", R.ONE_PASS_KEYS + R.TWO_PASS_KEYS)
def test_single_pass_kernels_exact(nkv, code, lib, ws, dev, capsys):
    """The 32-row (21) and 16-row (22) kernels, one-pass forms up to 1024 keys and two-pass forms past them."""
    worst = 0.0
    for nq in R.Q_ROWS:
        plan = R.plan_of(lib, 1, HEADS, nq, nkv, code)
        assert R.direct_form(code, plan["direct_tiles"], plan["blocks"])[2] == (2 if nkv > 1024 else 1)
        worst = max(worst, _exact_through_forced(lib, ws, dev, 1, nq, nkv, code, 0, 0, ("mixed", "selector"),
                                                 types=((0, 0), (0, 1))))
    _report(capsys, f"plan {code}, {nkv} keys", worst)


@pytest.mark.parametrize("nq,nkv,form", [(1024, 1100, (4, 4, 2)), (1024, 2048, (4, 4, 2)), (1056, 1100, (4, 2, 4)),
                                         (1056, 2048, (4, 2, 4)), (1056, 600, (4, 2, 2)), (1056, 1024, (4, 2, 2))])
def test_multi_round_forms_exact(nq, nkv, form, lib, ws, dev, capsys):
    """Plan 21 with batch 2: 1024 rows are exactly 256 blocks of 32 rows, one round, the two-pass form; 1056 rows are
    264 blocks, past one round: the two-workgroups-per-CU forms, four passes of 2 tiles past 1024 keys and two passes
    up to it. Census and selector rows (their references are one vector per head and a gather)."""
    plan = R.plan_of(lib, 2, HEADS, nq, nkv, 21)
    assert R.direct_form(21, plan["direct_tiles"], plan["blocks"]) == form
    worst = _exact_through_forced(lib, ws, dev, 2, nq, nkv, 21, 0, 0, ("census", "selector"), types=((0, 0), (0, 1)))
    _report(capsys, f"plan 21 form {form}, 2x{nq}x{nkv}", worst)


@pytest.mark.parametrize("waves", [4, 8])
def test_streaming_kernel_forced_exact(waves, lib, ws, dev, capsys):
    worst = 0.0
    for nq, nkv in ((1, 1), (17, 65), (33, 257), (130, 1000), (257, 200)):
        worst = max(worst, _exact_through_forced(lib, ws, dev, 1, nq, nkv, 23, waves, 0, ("mixed", "selector"),
                                                 types=((0, 0), (0, 1))))
    _report(capsys, f"plan 23, {waves} waves", worst)


# ---- key and query counts -------------------------------------------------------------------------------------------
def _counts_case(lib, fam, waves, counts, q_counts, nq, nkv, seed):
    plan = R.plan_of(lib, len(counts), HEADS, nq, nkv, 23, waves)
    assert (plan["code"], plan["kv_waves"]) == (23, waves)
    return R.exact_case(fam, nq, nkv, lambda n: R.layout_units(R.plan_layout(plan, n)), seed, batch=len(counts),
                        heads=HEADS, counts=counts, q_counts=q_counts)


@pytest.mark.parametrize("waves", [4, 8])
def test_stream_lens_exact(waves, lib, dev, capsys):
    """mha_hd64_launch_stream_lens on the counts of test_gpu_ragged.py's 5x257x200 case plus 0 and nkv + 5, which the
    kernel clamps to 1 and nkv. Keys past a count are poison: NaN values and codes that would win selector rows."""
    batch, nq, nkv, counts = R.STREAM_CASE
    counts = list(counts) + [0, nkv + 5]
    worst = 0.0
    for fam in ("mixed", "selector"):
        case = _counts_case(lib, fam, waves, counts, None, nq, nkv, 17)
        assert case["counts"] == [200, 129, 128, 64, 65, 1, 200]
        ops = Operands(case["q"], case["k"], case["v"], dev)
        q, k, v = ops.of(torch.float16)
        lens = torch.tensor(counts, dtype=torch.int32, device=dev)
        for out_f32 in (0, 1):
            out = GuardedOut((len(counts), HEADS, nq, 64), torch.float32 if out_f32 else torch.float16, dev)
            st = lib.mha_hd64_launch_stream_lens(q.ptr, k.ptr, v.ptr, out.ptr, len(counts), HEADS, nq, nkv, lens.data_ptr(),
                                                 out_f32, waves, torch.cuda.current_stream().cuda_stream)
            assert st == 0
            assert lib.mha_hd64_last_combine_form() == 0
            torch.cuda.synchronize()
            worst = max(worst, R.check_exact(_guards_ok(out, fam), case, 1, not out_f32))
    _report(capsys, f"stream lens, {waves} waves", worst)


def test_grouped_kv_and_q_lens_exact(lib, dev, capsys):
    """mha_hd64_grouped with kv_lens and q_lens: two calls in one launch, rows past a query count come out NaN (and
    hold queries that would score high), keys past a key count are poison."""
    from lightglue_amd import mha_hd64_grouped

    shapes = [(3, 130, 200, [200, 129, 1], [130, 17, 1]), (2, 33, 257, [65, 257], [33, 0])]
    worst = 0.0
    for fam in ("mixed", "selector"):
        for out_dt in (torch.float16, torch.float32):
            cases, calls, outs, kl, ql = [], [], [], [], []
            for i, (b, nq, nkv, kc, qc) in enumerate(shapes):
                plan = R.plan_of(lib, b, HEADS, nq, nkv, 23, 0)
                case = _counts_case(lib, fam, plan["kv_waves"], kc, qc, nq, nkv, 19 + i)
                ops = Operands(case["q"], case["k"], case["v"], dev)
                calls.append(tuple(g.view for g in ops.of(torch.float16)))
                outs.append(GuardedOut((b, HEADS, nq, 64), out_dt, dev))
                kl.append(torch.tensor(kc, dtype=torch.int32, device=dev))
                ql.append(torch.tensor(qc, dtype=torch.int32, device=dev))
                cases.append((case, ops))
            mha_hd64_grouped(calls, out_dtype=out_dt, outs=[o.view for o in outs], kv_lens=kl, q_lens=ql)
            assert lib.mha_hd64_last_combine_form() == 0
            torch.cuda.synchronize()
            for (case, _), out in zip(cases, outs):
                worst = max(worst, R.check_exact(_guards_ok(out, fam), case, 1, out_dt == torch.float16))
    _report(capsys, "grouped kv_lens and q_lens", worst)


# ---- grouped launches and the planner's default ---------------------------------------------------------------------
@pytest.mark.parametrize("group", range(len(R.GROUPS)))
def test_grouped_four_calls_exact(group, lib, dev, capsys):
    """Four calls of different shapes in one launch through mha_hd64_grouped, the planner's choice, fp16 and fp32
    inputs: every call against its own seams."""
    from lightglue_amd import mha_hd64_grouped

    shapes = R.GROUPS[group]
    worst = 0.0
    for in_dt, out_dt in ((torch.float16, torch.float16), (torch.float16, torch.float32), (torch.float32, torch.float32)):
        plans = R.group_plan(lib, shapes, in_dt == torch.float32)
        for fam in ("mixed", "selector"):
            cases, calls, outs = [], [], []
            for i, ((b, nq, nkv), plan) in enumerate(zip(shapes, plans)):
                case = R.exact_case(fam, nq, nkv, R.layout_units(R.plan_layout(plan, nkv)), 23 + i, batch=b, heads=HEADS)
                ops = Operands(case["q"], case["k"], case["v"], dev)
                calls.append(tuple(g.view for g in ops.of(in_dt)))
                outs.append(GuardedOut((b, HEADS, nq, 64), out_dt, dev))
                cases.append((case, ops))
            mha_hd64_grouped(calls, out_dtype=out_dt, outs=[o.view for o in outs])
            form = lib.mha_hd64_last_combine_form()
            assert (form != 0) == any(p["splits"] > 1 for p in plans), (form, plans)
            torch.cuda.synchronize()
            for (case, _), out, plan in zip(cases, outs, plans):
                worst = max(worst, R.check_exact(_guards_ok(out, fam), case, plan["splits"], out_dt == torch.float16))
    _report(capsys, f"grouped, four calls, plan {plans[0]['code']}", worst)


@pytest.mark.parametrize("batch,nq,nkv", R.DEFAULT_SHAPES)
def test_planner_default_exact(batch, nq, nkv, lib, dev, capsys):
    """mha_hd64 (the plugin's enqueue, batch 1) and mha_hd64_batched as the planner routes them, fp16 and fp32 inputs:
    the plan asserted with mha_hd64_plan and mha_hd64_plan_route, the seams taken from it."""
    from lightglue_amd import mha_hd64, mha_hd64_batched

    worst = 0.0
    for in_dt, out_dt in ((torch.float16, torch.float16), (torch.float16, torch.float32), (torch.float32, torch.float32)):
        in_f32 = in_dt == torch.float32
        ws_bytes = lib.mha_hd64_launch_workspace_bytes_typed(batch, HEADS, nq, nkv, 0 if in_f32 else 1)
        plan = R.plan_of(lib, batch, HEADS, nq, nkv, in_f32=in_f32, ws_bytes=ws_bytes)
        if not in_f32:
            out4 = (ctypes.c_int32 * 4)()
            lib.mha_hd64_plan(batch, HEADS, nq, nkv, ws_bytes, out4)
            assert (out4[0], out4[2]) == (plan["code"], plan["splits"]), (list(out4), plan)
        units = R.layout_units(R.plan_layout(plan, nkv))
        fams = ("census", "selector") if nq > 130 else ("mixed", "selector")
        for fam in fams:
            case = R.exact_case(fam, nq, nkv, units, 29, batch=batch, heads=HEADS)
            ops = Operands(case["q"], case["k"], case["v"], dev)
            q, k, v = (g.view for g in ops.of(in_dt))
            out = GuardedOut((batch, HEADS, nq, 64), out_dt, dev)
            mha_hd64_batched(q, k, v, out_dtype=out_dt, out=out.view)
            form = lib.mha_hd64_last_combine_form()
            assert (form != 0) == (plan["splits"] > 1), (form, plan)
            torch.cuda.synchronize()
            what = f"{batch}x{nq}x{nkv} plan {plan['code']} route {plan['route']} {fam}"
            try:
                worst = max(worst, R.check_exact(_guards_ok(out, what), case, plan["splits"], out_dt == torch.float16))
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from None
            if batch == 1 and in_dt == out_dt and nkv <= 2048:   # the plugin's enqueue: same plan, same bits
                o2 = mha_hd64(q, k, v)
                torch.cuda.synchronize()
                assert np.array_equal(o2.cpu().numpy().view(np.uint8), out.view.cpu().numpy().view(np.uint8)), what
    _report(capsys, f"planner default {batch}x{nq}x{nkv}", worst)


# ---- the graded families under the derived bound --------------------------------------------------------------------
@pytest.mark.parametrize("qw,kw,sp,nq,nkv", R.GRADED_FORMS)
def test_graded_families_within_the_derived_bound(qw, kw, sp, nq, nkv, lib, ws, dev, capsys):
    """gauss1, gauss3, lazy7 and lazy8p, every row and element against the float64 softmax under
    attention_refs.graded_bound (R = 3 for the single-pass kernels, F = 8 for the streaming kernel), fp16 and fp32
    output, fp32 input on the ring plans."""
    plan = R.plan_of(lib, 1, HEADS, nq, nkv, qw, kw, sp, ws_bytes=WS_BYTES)
    assert plan["code"] == qw and (qw >= 21 or kw >= 4 or plan["splits"] == sp)
    ranges = R.split_ranges(R.plan_layout(plan, nkv))
    r_p, f_u = (3 if qw in (21, 22) else 1), (8.0 if qw == 23 else 0.0)
    lines = []
    for name in R.GRADED:
        q, k, v = R.graded_case(name, nq, nkv, 31, heads=HEADS)
        terms = R.graded_terms(q, k, v)
        ops = Operands(q, k, v, dev)
        for in_f32, out_f32 in ((0, 0), (0, 1)) + (((1, 1),) if qw < 21 else ()):
            ref, bound = R.graded_bound(q, k, v, not out_f32, ranges, r_p, f_u, terms=terms)
            what = (f"plan {qw}x{kw} splits {plan['splits']} {nq}x{nkv} {name} in{'32' if in_f32 else '16'} "
                    f"out{'32' if out_f32 else '16'}")
            got, form = _forced(lib, ws, ops, (1, nq, nkv), in_f32, out_f32, qw, kw, sp, what)
            assert form == (1 if plan["splits"] > 1 else 0), (what, form)
            err = np.abs(got.astype(np.float64) - ref)
            ratio = float((err / bound).max()) if np.isfinite(err).all() else float("nan")
            lines.append(f"  {what}: worst error / bound {ratio:.3f} (max error {float(err.max()):.2e}, median bound "
                         f"{float(np.median(bound)):.2e})")
            with capsys.disabled():
                print("\n" + lines[-1], end="")
            try:
                R.check_graded(got, ref, bound)
            except AssertionError as e:
                raise AssertionError(f"{what}: {e}") from None
