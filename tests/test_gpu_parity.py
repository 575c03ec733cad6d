"""Parity of the MI355X HIP kernels with the oracle and the reference's golden outputs.

Tolerance (north_star, BASELINE.json): max-abs <= 1e-2 against the PyTorch fp32 reference
(lightglue_pytorch_no_plugin/lightglue.py:75-85). The fp16 paths are compared on the
fp16-rounded inputs (o_ref16), the Float path on the raw fp32 inputs (o_ref32; the
kernel rounds them to fp16 on load exactly like the reference's convert kernel).
Observed errors are ~1e-3 (fp16 output rounding + fp16 P); TOL_* below are the contract.
"""
import ctypes

import numpy as np
import pytest

from conftest import golden_cases, load_golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-2          # north_star contract, every path
TOL_F32OUT = 5e-3   # fp32 output: no output rounding, expect tighter
# Regression guards near the observed error, so a numerical regression far inside the contract
# still fails (observed on MI355X per fixture, tools/parity_errors.py -> profiles/r02/
# parity_errors.jsonl; logit std 1 cases / the spike case): fp16 output, beyond half an fp16 ulp of
# the reference value (the output rounding), <= 2.6e-4 / 7.0e-4; fp16-in fp32-out <= 4.1e-4 /
# 1.0e-3; the Float path against the raw fp32 inputs (fp16 input rounding included) <= 9.4e-4 /
# 1.8e-3. Bounds: 1.5e-3 / 1.5e-3 / 2.5e-3, times the fixture's logit scale max(1, q_std) (the
# peaky case, q_std 3: 1.5e-3 / 1.7e-3 / 2.8e-3 observed).
REG_F32OUT = 1.5e-3
REG_F16OUT_ABS = 1.5e-3
REG_FLOAT = 2.5e-3


def _scale(g):
    return max(1.0, float(g["q_std"]))


def _regress16(got, ref, scale=1.0):
    """Elementwise fp16-output regression bound: |got - ref| <= 1.5e-3 scale + 2^-11 |ref|."""
    d = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    bound = REG_F16OUT_ABS * scale + np.abs(ref.astype(np.float64)) * 2.0 ** -11
    worst = float((d - bound).max())
    assert worst <= 0, f"fp16 output regression: max excess {worst:.3e} (max-abs {float(d.max()):.3e})"

CASES = golden_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _t(x, dev, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dtype).contiguous()


def _maxdiff(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max())


@pytest.mark.parametrize("name", CASES)
def test_plugin_half_path_matches_reference(name, dev):
    from lightglue_amd import mha_hd64

    g = load_golden(name)
    q, k, v = (_t(x, dev, torch.float16) for x in (g["q"], g["k"], g["v"]))
    o = mha_hd64(q, k, v)
    torch.cuda.synchronize()
    assert o.dtype == torch.float16 and o.shape == q.shape
    got = o.float().cpu().numpy()[:, :, g["rows"]]
    assert np.isfinite(got).all()
    assert _maxdiff(got, g["o_ref16"]) <= TOL
    _regress16(got, g["o_ref16"], _scale(g))


@pytest.mark.parametrize("name", CASES)
def test_plugin_float_path_matches_reference(name, dev):
    from lightglue_amd import mha_hd64

    g = load_golden(name)
    q, k, v = (_t(x, dev, torch.float32) for x in (g["q"], g["k"], g["v"]))
    o = mha_hd64(q, k, v)
    torch.cuda.synchronize()
    assert o.dtype == torch.float32
    got = o.cpu().numpy()[:, :, g["rows"]]
    assert _maxdiff(got, g["o_ref32"]) <= TOL
    assert _maxdiff(got, g["o_ref32"]) <= REG_FLOAT * _scale(g)


@pytest.mark.parametrize("name", CASES)
def test_fp16in_fp32out_launcher(name, dev):
    from lightglue_amd import mha_hd64_batched

    g = load_golden(name)
    q, k, v = (_t(x, dev, torch.float16) for x in (g["q"], g["k"], g["v"]))
    o = mha_hd64_batched(q, k, v, out_dtype=torch.float32)
    torch.cuda.synchronize()
    got = o.cpu().numpy()[:, :, g["rows"]]
    assert _maxdiff(got, g["o_ref16"]) <= TOL_F32OUT
    assert _maxdiff(got, g["o_ref16"]) <= REG_F32OUT * _scale(g)


# ---- every launch plan (query-wave split x cross-workgroup KV split) against the C oracle ----
PLAN_SHAPES = [(1, 1), (33, 65), (100, 100), (64, 2048), (300, 129), (1024, 1024), (257, 1000), (16, 4500)]
# 12 = two 32-row query blocks per wave, 2 q-waves; (2, 4), (1, 4), (1, 8) = one super-tile of
# 64*kv_waves keys per split (the split count follows from nkv; past 16 super-tiles the planner
# falls back to (2, 2))
WG_SHAPES = [(4, 1), (2, 2), (1, 2), (4, 2), (12, 2), (2, 4), (1, 4), (1, 8)]


@pytest.mark.parametrize("nq,nkv", PLAN_SHAPES)
@pytest.mark.parametrize("wg", WG_SHAPES)
@pytest.mark.parametrize("splits", [1, 2, 3, 5])
def test_forced_plans_match_oracle(nq, nkv, wg, splits, dev, oracle_mod):
    from lightglue_amd import _lib, synth

    q_waves, kv_waves = wg
    super_total = -(-nkv // (64 * kv_waves))
    if kv_waves >= 4 and splits != 1:
        pytest.skip("single-super-tile shapes take one split per super-tile")
    if splits > super_total:
        pytest.skip("more splits than key tiles")
    if -(-super_total // -(-super_total // splits)) != splits:
        pytest.skip("split count not realisable for this length")
    lib = _lib.load()
    qn, kn, vn = synth.qkv(1000 + nq + 7 * nkv, nq, nkv)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 48)), nq - 1])
    ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    for out_f32, tol in ((0, TOL), (1, TOL_F32OUT)):
        o = torch.full(q.shape, float("nan"), dtype=torch.float32 if out_f32 else torch.float16, device=dev)
        st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1, 4, nq, nkv, 0,
                                        out_f32, q_waves, kv_waves, splits, ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream().cuda_stream, 3)
        assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        got = o.float().cpu().numpy()
        assert np.isfinite(got).all(), "unwritten or NaN output rows"
        assert _maxdiff(got[:, :, rows], ref) <= tol


@pytest.mark.parametrize("wg", WG_SHAPES)
def test_forced_plans_f32_input(wg, dev, oracle_mod):
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    nq, nkv = 200, 333
    qn, kn, vn = synth.qkv(4242, nq, nkv)
    ref = oracle_mod.attention_c(qn, kn, vn)
    q, k, v = (_t(x, dev, torch.float32) for x in (qn, kn, vn))
    o = torch.empty_like(q)
    ws = torch.empty(16 << 20, dtype=torch.uint8, device=dev)
    st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1, 4, nq, nkv, 1, 1,
                                    wg[0], wg[1], 2, ws.data_ptr(), ws.numel(),
                                    torch.cuda.current_stream().cuda_stream, 3)
    assert st == 0, _lib.last_error()
    torch.cuda.synchronize()
    assert _maxdiff(o.cpu().numpy(), ref) <= TOL


F32_SHAPES = [(1, 1), (33, 65), (100, 100), (300, 129), (512, 512), (777, 1000), (1024, 768), (1024, 1024),
              (64, 2048), (1024, 2048), (700, 1500), (16, 4500)]


@pytest.mark.parametrize("nq,nkv", F32_SHAPES)
@pytest.mark.parametrize("batch,heads", [(1, 4), (2, 3)])
def test_float_boundary_in_kernel_equals_convert_launch(nq, nkv, batch, heads, dev, oracle_mod):
    """fp32 Q/K/V rounded to fp16 inside the 16-row kernel (one launch) vs the convert launch +
    fp16 kernel: both round every input RNE and then run the same arithmetic, so the outputs are
    bitwise equal. The in-kernel form leaves the workspace untouched (no converted copy is
    written: one launch), the convert form fills it; other launches (nkv > 1024, more than 256
    blocks) take the convert form or the ring kernel either way."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    qn, kn, vn = synth.qkv(77 + nq + nkv, nq, nkv, batch=batch, heads=heads)
    q, k, v = (_t(x, dev, torch.float32) for x in (qn, kn, vn))
    plan = (ctypes.c_int32 * 4)()
    lib.mha_hd64_plan(batch, heads, nq, nkv, 64 << 20, plan)
    in_kernel = plan[0] == 22 and nkv <= 1024  # the 16-row kernel's one-pass forms take fp32 directly
    outs, touched = [], []
    for inkernel in (1, 0):
        lib.mha_hd64_set_f32_inkernel(inkernel)
        try:
            ws = torch.full((64 << 20,), 0x5A, dtype=torch.uint8, device=dev)
            o = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
            st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch, heads,
                                            nq, nkv, 1, 1, 0, 0, 0, ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream().cuda_stream, 3)
            assert st == 0, _lib.last_error()
            torch.cuda.synchronize()
        finally:
            lib.mha_hd64_set_f32_inkernel(1)
        outs.append(o)
        touched.append(bool((ws[: 1 << 20] != 0x5A).any()))
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1])
    if in_kernel:
        assert not touched[0], "in-kernel form wrote the workspace (a convert launch ran)"
        assert touched[1]
    rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 24)), nq - 1])
    ref = oracle_mod.attention_c(np.ascontiguousarray(qn[:, :, rows]), kn, vn)
    assert _maxdiff(outs[0].cpu().numpy()[:, :, rows], ref) <= TOL


def test_float_convert_route_falls_back_without_room(dev, oracle_mod):
    """fp32 1x4x16x1100: its fp16 plan is the 16-row kernel's two-pass form, so with the queried
    workspace the launch converts into it and runs that kernel (no split: combine form 0, which the
    ring kernel's split plan for this shape would not report). With 256 bytes less, or with no
    workspace at all, the fp16 copies have no room and the ring kernel rounds on load instead. All
    three match the oracle at the Float path's tolerance."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    nq, nkv, FLOAT = 16, 1100, 0
    qn, kn, vn = synth.qkv(1100, nq, nkv)
    ref = oracle_mod.attention_c(qn, kn, vn)
    q, k, v = (_t(x, dev, torch.float32) for x in (qn, kn, vn))
    need = lib.mha_hd64_launch_workspace_bytes_typed(1, 4, nq, nkv, FLOAT)
    assert need == 4 * (nq + 2 * nkv) * 64 * 2  # Q, K, V in fp16
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    call = (_lib.CallDesc * 1)(_lib.CallDesc(0, 0, 0, 0, 1, 4, nq, nkv))
    head, one, off = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 1)(), (ctypes.c_size_t * 1)()
    for ws_ptr, ws_bytes, route in ((ws.data_ptr(), need, 2), (ws.data_ptr(), need - 256, 0), (None, 0, 0)):
        lib.mha_hd64_plan_route(call, 1, FLOAT, ws_bytes, ws_ptr is not None, 0, 0, 0, head, one, one, off)
        assert head[0] == route and (route == 0) == (head[1] not in (21, 22, 23)), (ws_bytes, list(head))
        o = torch.full(q.shape, float("nan"), dtype=torch.float32, device=dev)
        st = lib.mha_hd64_launch_fp32in_fp32out(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1, 4, nq, nkv,
                                                ws_ptr, ws_bytes, torch.cuda.current_stream().cuda_stream)
        assert st == 0, _lib.last_error()
        form = lib.mha_hd64_last_combine_form()
        torch.cuda.synchronize()
        err = _maxdiff(o.cpu().numpy(), ref)
        print(f"ws {ws_bytes}: route {route}, combine form {form}, max-abs {err:.2e}")
        assert err <= TOL and err <= REG_FLOAT
        if route == 2:
            assert form == 0


@pytest.mark.parametrize("shapes", [[(1024, 1024)], [(512, 512), (300, 257)], [(33, 65), (777, 1000), (64, 128)],
                                    [(1024, 2048)], [(200, 1500), (64, 2048)]])
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
def test_float_inputs_equal_fp16_inputs_rounded_on_host(shapes, out_dtype, dev):
    """The in-kernel rounding of fp32 Q/K/V (single and grouped launches, fp32 or fp16 output)
    is the host's RNE rounding: the fp32-input launch equals the fp16-input launch on
    round_f16(inputs) bit for bit (same plan, same kernel, same arithmetic after the loads)."""
    from lightglue_amd import mha_hd64_grouped, synth

    calls32, calls16 = [], []
    for i, (nq, nkv) in enumerate(shapes):
        qn, kn, vn = synth.qkv(500 + 13 * i + nq, nq, nkv)
        calls32.append(tuple(_t(x, dev, torch.float32) for x in (qn, kn, vn)))
        calls16.append(tuple(_t(synth.round_f16(x), dev, torch.float16) for x in (qn, kn, vn)))
    o32 = mha_hd64_grouped(calls32, out_dtype=out_dtype)
    o16 = mha_hd64_grouped(calls16, out_dtype=out_dtype)
    torch.cuda.synchronize()
    for a, b in zip(o32, o16):
        assert torch.isfinite(a.float()).all()
        assert torch.equal(a, b)


def test_rescale_branch_forced(dev, oracle_mod):
    """Rule 26 (cdna_hip_programming.md §5.4): force the lazy-rescale branch at a chosen tile.

    Query row 5 meets a key row (600) scaled so its score jumps far past the running max
    of the first tiles; every other query keeps its max. Checked on the full tensor."""
    from lightglue_amd import mha_hd64, synth

    nq, nkv = 256, 1024
    qn, kn, vn = synth.qkv(606, nq, nkv)
    for gain in (0.5, 2.0, 6.0):
        k2 = synth.spike(qn, kn, 5, 600, gain)
        q16, k16, v16 = (synth.round_f16(x) for x in (qn, k2, vn))
        ref = oracle_mod.attention_c(q16, k16, v16)
        q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
        o = mha_hd64(q, k, v)
        torch.cuda.synchronize()
        assert _maxdiff(o.float().cpu().numpy(), ref) <= TOL, gain


def test_large_negative_logits(dev, oracle_mod):
    """Scores far below zero everywhere: the first tile must set the max exactly (no underflow to l = 0)."""
    from lightglue_amd import mha_hd64, synth

    nq, nkv = 64, 300
    qn, kn, vn = synth.qkv(808, nq, nkv)
    qn = np.abs(qn) * 4
    kn = -np.abs(kn) * 4  # every score strongly negative (~ -200 raw)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    ref = oracle_mod.attention_c(q16, k16, v16)
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    o = mha_hd64(q, k, v)
    torch.cuda.synchronize()
    got = o.float().cpu().numpy()
    assert np.isfinite(got).all()
    assert _maxdiff(got, ref) <= TOL


def test_batched_launcher_many_pairs(dev, oracle_mod):
    """B independent calls in one launch == B single calls (the batched-pairs stream)."""
    from lightglue_amd import mha_hd64, mha_hd64_batched, synth

    B, nq, nkv = 6, 300, 257
    qn, kn, vn = synth.qkv(77, nq, nkv, batch=B)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    ob = mha_hd64_batched(q, k, v)
    torch.cuda.synchronize()
    ref = oracle_mod.attention_c(q16, k16, v16)
    assert _maxdiff(ob.float().cpu().numpy(), ref) <= TOL
    for b in range(B):
        os_ = mha_hd64(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous())
        torch.cuda.synchronize()
        assert _maxdiff(os_.float().cpu().numpy(), ref[b:b + 1]) <= TOL


def test_deterministic_bitwise(dev):
    from lightglue_amd import mha_hd64, synth

    qn, kn, vn = synth.qkv(5, 1024, 1024)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    a = mha_hd64(q, k, v).clone()
    b = mha_hd64(q, k, v).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_full_size_properties(dev):
    """At the metric shape: outputs are convex combinations of V rows, and scaling V scales O."""
    from lightglue_amd import mha_hd64, synth

    qn, kn, vn = synth.qkv(9, 1024, 1024)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    o = mha_hd64(q, k, v).float()
    vmin = v.float().amin(dim=2, keepdim=True)
    vmax = v.float().amax(dim=2, keepdim=True)
    assert bool((o >= vmin - 1e-2).all()) and bool((o <= vmax + 1e-2).all())
    o2 = mha_hd64(q, k, (v * 2).contiguous()).float()   # exact power-of-two scaling of V
    assert float((o2 - 2 * o).abs().max()) <= 2e-3
    # a constant V gives a constant output
    vc = torch.full_like(v, 0.5)
    oc = mha_hd64(q, k, vc).float()
    assert float((oc - 0.5).abs().max()) <= 1e-3


def test_graph_capture_replay(dev):
    """enqueue is capturable (no host sync, no allocation): hipGraph replay gives the same bits."""
    from lightglue_amd import mha_hd64, synth

    qn, kn, vn = synth.qkv(3, 1024, 1024)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    out = torch.empty_like(q)
    eager = mha_hd64(q, k, v).clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mha_hd64(q, k, v, out=out)  # warm the per-stream workspace outside capture
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mha_hd64(q, k, v, out=out)
    from lightglue_amd import _lib

    # one launch either way: the single-pass kernel (0, no split) or splits merged in-launch (1)
    assert _lib.load().mha_hd64_last_combine_form() in (0, 1)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_bound_enqueue_matches_plugin_call(dev):
    """bench.py's timed steps: the plugin's enqueue with bindings prepared once gives the bits of
    mha_hd64(), on the stream it was bound on, eagerly and under graph capture."""
    from lightglue_amd import mha_hd64, plugin, synth

    qn, kn, vn = synth.qkv(11, 1024, 1024)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    ref = mha_hd64(q, k, v).clone()
    out = torch.empty_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step = plugin.bound_enqueue(q, k, v, out)
        for _ in range(3):
            step()
    s.synchronize()
    assert torch.equal(out, ref)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)


def test_attention_module_and_autograd_function(dev):
    from lightglue_amd import Attention, MHAHeadDim64, synth

    qn, kn, vn = synth.qkv(21, 128, 96)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    a = Attention()(q, k, v)
    b = MHAHeadDim64.apply(q, k, v)
    ref = torch.nn.functional.scaled_dot_product_attention(q.float(), k.float(), v.float())
    assert torch.equal(a, b)
    assert float((a.float() - ref).abs().max()) <= TOL


def test_streams_with_separate_workspaces(dev):
    """Concurrent enqueues on two streams (distinct workspaces, the reference's rule)."""
    from lightglue_amd import mha_hd64, synth

    qn, kn, vn = synth.qkv(31, 1024, 1024)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    ref = mha_hd64(q, k, v).clone()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    outs = []
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            outs.append(mha_hd64(q, k, v))
    torch.cuda.synchronize()
    for o in outs:
        assert torch.equal(o, ref)


# ---- grouped launcher: several calls of different shapes per launch ----
def _group_inputs(shapes, seed, dtype=np.float16):
    from lightglue_amd import synth

    out = []
    for i, (b, nq, nkv) in enumerate(shapes):
        qn, kn, vn = synth.qkv(seed + 17 * i, nq, nkv, batch=b)
        out.append(tuple(synth.round_f16(x) for x in (qn, kn, vn)) if dtype == np.float16 else (qn, kn, vn))
    return out


def test_grouped_lightglue_layer(dev, oracle_mod):
    """One LightGlue layer's four calls (self0, self1, cross0->1, cross1->0; lightglue.py:137-152,
    188-205) as two grouped launches and as one, each output against the oracle."""
    from lightglue_amd import mha_hd64_grouped

    n0, n1 = 700, 513
    (q0, k0, v0), (q1, k1, v1) = _group_inputs([(1, n0, n0), (1, n1, n1)], 31)
    host = [(q0, k0, v0), (q1, k1, v1), (q0, k1, v1), (q1, k0, v0)]
    dev_t = [tuple(_t(x, dev, torch.float16) for x in c) for c in host]
    refs = [oracle_mod.attention_c(*c) for c in host]
    for grouping in ([[0, 1], [2, 3]], [[0, 1, 2, 3]]):
        outs = [None] * 4
        for grp in grouping:
            res = mha_hd64_grouped([dev_t[i] for i in grp])
            for i, o in zip(grp, res):
                outs[i] = o
        torch.cuda.synchronize()
        for i in range(4):
            got = outs[i].float().cpu().numpy()
            assert np.isfinite(got).all()
            assert _maxdiff(got, refs[i]) <= TOL, (grouping, i)


@pytest.mark.parametrize("in_dt,out_dt,tol", [(torch.float16, torch.float16, TOL),
                                              (torch.float16, torch.float32, TOL_F32OUT),
                                              (torch.float32, torch.float32, TOL)])
def test_grouped_chunked_mixed_shapes(in_dt, out_dt, tol, dev, oracle_mod):
    """Six calls (chunked 4 + 2) with mixed batch, tails, 1-row queries, and calls that split their
    keys beside calls that do not (per-call split counts inside one launch + one combine)."""
    from lightglue_amd import mha_hd64_grouped

    shapes = [(1, 1, 1), (2, 100, 2048), (1, 1024, 64), (1, 33, 65), (3, 257, 1000), (1, 2048, 2048)]
    host = _group_inputs(shapes, 55, np.float16 if in_dt == torch.float16 else np.float32)
    dev_t = [tuple(_t(x, dev, in_dt) for x in c) for c in host]
    outs = mha_hd64_grouped(dev_t, out_dtype=out_dt)
    torch.cuda.synchronize()
    for i, (c, o) in enumerate(zip(host, outs)):
        rows = np.unique(np.r_[np.arange(0, c[0].shape[2], max(1, c[0].shape[2] // 40)), c[0].shape[2] - 1])
        ref = oracle_mod.attention_c(np.ascontiguousarray(c[0][:, :, rows]), c[1], c[2])
        got = o.float().cpu().numpy()
        assert o.dtype == out_dt and np.isfinite(got).all(), i
        assert _maxdiff(got[:, :, rows], ref) <= tol, i


def test_grouped_matches_single_calls_bitwise_when_plans_agree(dev):
    """A group of one is exactly the single-call launch (same plan, same kernel)."""
    from lightglue_amd import mha_hd64_batched, mha_hd64_grouped, synth

    qn, kn, vn = synth.qkv(9, 1024, 1024)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    a = mha_hd64_batched(q, k, v)
    (b,) = mha_hd64_grouped([(q, k, v)])
    torch.cuda.synchronize()
    assert torch.equal(a, b)


# ---- in-launch split combine (arrival tickets; csrc/mha_hd64_ring.hip epilogue; tickets: mha_hd64_launch.hip) ----
FUSED_SHAPES = [  # (nq, nkv, q_waves, kv_waves, splits)
    (1024, 1024, 2, 4, 0), (1024, 1024, 2, 2, 4), (300, 2048, 2, 2, 3), (100, 1000, 12, 2, 3),
    (64, 4000, 2, 4, 0), (33, 65, 4, 1, 2), (257, 1000, 4, 2, 2), (1024, 1024, 1, 8, 0), (300, 2000, 1, 8, 0),
    (100, 1000, 1, 4, 0)]


def _forced(lib, q, k, v, o, nq, nkv, qw, kw, sp, ws, stream=None):
    from lightglue_amd import _lib

    st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1, 4, nq, nkv,
                                    int(q.dtype == torch.float32), int(o.dtype == torch.float32), qw, kw, sp,
                                    ws.data_ptr(), ws.numel(),
                                    (stream or torch.cuda.current_stream()).cuda_stream, 3)
    assert st == 0, _lib.last_error()


@pytest.fixture
def fused_switch(dev):
    from lightglue_amd import _lib

    lib = _lib.load()
    yield lib.mha_hd64_set_fused_combine
    lib.mha_hd64_set_fused_combine(1)


@pytest.mark.parametrize("out_dt", [torch.float16, torch.float32])
def test_fused_combine_bitwise_equals_combine_kernel(out_dt, dev, fused_switch, oracle_mod):
    """The last-arriver combine reads every split back in split order: same bits as the kernel."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    for nq, nkv, qw, kw, sp in FUSED_SHAPES:
        qn, kn, vn = synth.qkv(77 + nq + nkv, nq, nkv)
        q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
        outs = []
        for fused in (0, 1):
            fused_switch(fused)
            o = torch.full(q.shape, float("nan"), dtype=out_dt, device=dev)
            _forced(lib, q, k, v, o, nq, nkv, qw, kw, sp, ws)
            assert lib.mha_hd64_last_combine_form() == (1 if fused else 2)
            outs.append(o)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), (nq, nkv, qw, kw, sp)
        rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 32)), nq - 1])
        ref = oracle_mod.attention_c(np.ascontiguousarray(synth.round_f16(qn)[:, :, rows]), synth.round_f16(kn),
                                     synth.round_f16(vn))
        assert _maxdiff(outs[1].float().cpu().numpy()[:, :, rows], ref) <= TOL


def test_fused_combine_tickets_reset_under_load(dev, fused_switch):
    """Many launches with different split counts on one stream reuse the same tickets (each
    launch leaves them at zero), while another stream keeps the chip busy (uneven load)."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    cases = []
    for nq, nkv, qw, kw, sp in FUSED_SHAPES:
        qn, kn, vn = synth.qkv(5 + nq + 3 * nkv, nq, nkv)
        q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
        fused_switch(0)
        o = torch.empty_like(q)
        _forced(lib, q, k, v, o, nq, nkv, qw, kw, sp, ws)
        cases.append((q, k, v, o, nq, nkv, qw, kw, sp))
    torch.cuda.synchronize()
    fused_switch(1)
    s = torch.cuda.Stream()
    busy = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device=dev, dtype=torch.float16)
    outs = []
    with torch.cuda.stream(busy):
        for _ in range(6):
            a = (a @ a).clamp_(-1, 1)
    with torch.cuda.stream(s):
        for r in range(8):
            for i, (q, k, v, _, nq, nkv, qw, kw, sp) in enumerate(cases):
                o = torch.full_like(q, float("nan"))
                _forced(lib, q, k, v, o, nq, nkv, qw, kw, sp, ws, stream=s)
                outs.append((i, o))
    torch.cuda.synchronize()
    for i, o in outs:
        assert torch.equal(o, cases[i][3]), i


def test_fused_combine_graphs_from_one_stream_replayed_concurrently(dev):
    """Two graphs captured on one stream own separate tickets: replaying them side by side on two
    streams (each graph with its own workspace, the reference's rule) gives the eager results."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    cap = torch.cuda.Stream()
    data = []
    for seed, (nq, nkv) in ((31, (1024, 1024)), (32, (512, 2048))):
        qn, kn, vn = synth.qkv(seed, nq, nkv)
        q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
        ws = torch.empty(16 << 20, dtype=torch.uint8, device=dev)
        ref = torch.empty_like(q)
        _forced(lib, q, k, v, ref, nq, nkv, 1, 8, 0, ws)  # the split plan (tickets)
        data.append((q, k, v, ref, torch.empty_like(q), ws, nq, nkv))
    torch.cuda.synchronize()
    graphs = []
    for q, k, v, _, out, ws, nq, nkv in data:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=cap):
            _forced(lib, q, k, v, out, nq, nkv, 1, 8, 0, ws, stream=cap)
        assert lib.mha_hd64_last_combine_form() == 1  # recorded with its own tickets
        graphs.append(g)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(20):
        for d, g, s in zip(data, graphs, streams):
            d[4].zero_()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                g.replay()
        for d, s in zip(data, streams):
            torch.cuda.current_stream().wait_stream(s)
            assert torch.equal(d[4], d[3])


# ---- single-pass kernels (csrc/mha_hd64_direct16.hip, forced plan 22: the planner's choice for
# fp16 launches of <= 256 16-row blocks with nkv <= 1024; csrc/mha_hd64_direct.hip, plan 21: <= 256
# 32-row blocks) ----
DIRECT_SHAPES = [(1, 1), (33, 65), (100, 77), (256, 256), (1000, 777), (1024, 1024), (64, 1024), (513, 513),
                 (2048, 1000), (300, 129), (97, 600), (5, 1024), (1024, 64), (130, 520)]


@pytest.mark.parametrize("code", [21, 22])
@pytest.mark.parametrize("nq,nkv", DIRECT_SHAPES)
def test_direct_kernel_matches_oracle(nq, nkv, code, dev, oracle_mod):
    """Every key-tile layout: waves wholly past nkv, partial tiles, one- and two-tile waves; the
    32-row (code 21) and 16-row (code 22) single-pass kernels."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    qn, kn, vn = synth.qkv(77 + nq + 3 * nkv, nq, nkv)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 48)), nq - 1])
    ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
        o = torch.full(q.shape, float("nan"), dtype=out_dt, device=dev)
        _forced(lib, q, k, v, o, nq, nkv, code, 0, 0, ws)
        assert lib.mha_hd64_last_combine_form() == 0
        torch.cuda.synchronize()
        got = o.float().cpu().numpy()
        assert np.isfinite(got).all(), "unwritten or NaN output rows"
        assert _maxdiff(got[:, :, rows], ref) <= tol


# nkv in (1024, 2048]: the single-pass kernels' two-pass forms (4 waves x 2 x 4 tiles through 4 slots)
DIRECT2_SHAPES = [(2048, 2048), (1000, 1500), (64, 2048), (300, 1025), (17, 1900), (1024, 1100), (513, 1537)]


@pytest.mark.parametrize("code", [21, 22])
@pytest.mark.parametrize("nq,nkv", DIRECT2_SHAPES)
def test_direct_kernel_two_pass_matches_oracle(nq, nkv, code, dev, oracle_mod):
    """Second-pass tiles partial or wholly past nkv, waves without keys, both output types."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    qn, kn, vn = synth.qkv(91 + nq + 5 * nkv, nq, nkv)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 48)), nq - 1])
    ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
        o = torch.full(q.shape, float("nan"), dtype=out_dt, device=dev)
        _forced(lib, q, k, v, o, nq, nkv, code, 0, 0, ws)
        assert lib.mha_hd64_last_combine_form() == 0
        torch.cuda.synchronize()
        got = o.float().cpu().numpy()
        assert np.isfinite(got).all(), "unwritten or NaN output rows"
        assert _maxdiff(got[:, :, rows], ref) <= tol


def test_direct_kernel_two_pass_rescale(dev, oracle_mod):
    """Spikes in the second pass's tiles move the running max after the first pass's PV (O and
    the row sums rescaled): key 300 (wave 0, pass 1), key 1900 (wave 3, pass 1), key 10 (pass 0,
    small gain: no move), and nkv = 1100 (wave 2 partial, wave 3 empty)."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    nq = 256
    for nkv, krow, gain in ((2048, 300, 6.0), (2048, 1900, 3.0), (1100, 1090, 6.0), (2048, 10, 0.5)):
        qn, kn, vn = synth.qkv(707 + nkv + krow, nq, nkv)
        kn = synth.spike(qn, kn, 5, krow, gain)
        q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
        ref = oracle_mod.attention_c(q16, k16, v16)
        q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
        for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
            for code in (21, 22):
                o = torch.empty(q.shape, dtype=out_dt, device=dev)
                _forced(lib, q, k, v, o, nq, nkv, code, 0, 0, ws)
                torch.cuda.synchronize()
                assert _maxdiff(o.float().cpu().numpy(), ref) <= tol, (nkv, krow, gain, out_dt, code)


def test_direct_kernel_four_pass_rescale(dev, oracle_mod):
    """The two-per-CU 4-pass form (forced plan 21, B = 2 so the launch has > 256 blocks): spikes in
    the third and fourth passes of a wave move the running max late (key 300: wave 0, pass 2; key
    480: wave 0, pass 3; key 1900: wave 3, pass 2), and nkv = 1100 leaves waves 2-3 short."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    nq, batch = 1024, 2
    for nkv, krow, gain in ((2048, 300, 6.0), (2048, 480, 3.0), (2048, 1900, 6.0), (1100, 1090, 6.0)):
        qn, kn, vn = synth.qkv(808 + nkv + krow, nq, nkv, batch=batch)
        kn = synth.spike(qn, kn, 5, krow, gain)
        q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
        rows = np.unique(np.r_[np.arange(0, nq, 37), 5, nq - 1])
        ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
        q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
        o = torch.full(q.shape, float("nan"), dtype=torch.float16, device=dev)
        st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch, 4, nq, nkv, 0,
                                        0, 21, 0, 0, ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream,
                                        3)
        assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert _maxdiff(o.float().cpu().numpy()[:, :, rows], ref) <= TOL, (nkv, krow, gain)


def test_direct_kernel_rescale_and_masked_waves(dev, oracle_mod):
    """A spike in a wave's second tile forces the rescale of the first tile's probabilities (key
    100: wave 0, tile 1; key 1000: wave 7, tile 1); nkv = 600 leaves waves 5-7 without keys."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    nq = 256
    for nkv, krow, gain in ((1024, 100, 6.0), (1024, 1000, 3.0), (600, 590, 6.0), (600, 10, 0.5)):
        qn, kn, vn = synth.qkv(606 + nkv + krow, nq, nkv)
        kn = synth.spike(qn, kn, 5, krow, gain)
        q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
        ref = oracle_mod.attention_c(q16, k16, v16)
        q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
        for code in (21, 22):
            o = torch.empty_like(q)
            _forced(lib, q, k, v, o, nq, nkv, code, 0, 0, ws)
            torch.cuda.synchronize()
            assert _maxdiff(o.float().cpu().numpy(), ref) <= TOL, (code, nkv, krow, gain)


def test_direct_kernel_grouped_and_batched(dev, oracle_mod):
    """The planner's single-pass launches: a LightGlue layer's pair of self calls at N=512 and
    N=1024 (two calls, one launch) and a batched call, against the oracle; group of one is
    bitwise the single launch."""
    from lightglue_amd import _lib, mha_hd64_batched, mha_hd64_grouped

    lib = _lib.load()
    for n0, n1 in ((512, 512), (1024, 1024), (1000, 777)):
        host = _group_inputs([(1, n0, n0), (1, n1, n1)], 41 + n0)
        dev_t = [tuple(_t(x, dev, torch.float16) for x in c) for c in host]
        outs = mha_hd64_grouped(dev_t)
        assert lib.mha_hd64_last_combine_form() == 0
        torch.cuda.synchronize()
        for c, o in zip(host, outs):
            assert _maxdiff(o.float().cpu().numpy(), oracle_mod.attention_c(*c)) <= TOL
    (c,) = _group_inputs([(2, 300, 900)], 3)
    q, k, v = (_t(x, dev, torch.float16) for x in c)
    a = mha_hd64_batched(q, k, v)
    (b,) = mha_hd64_grouped([(q, k, v)])
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert _maxdiff(a.float().cpu().numpy(), oracle_mod.attention_c(*c)) <= TOL


def test_direct_kernel_multi_round_shared_form(dev, oracle_mod):
    """Launches of more than 256 32-row blocks with 512 < nkv <= 1024 run the 4 x 2 x 2-tile two-pass
    form, two workgroups per CU: batched calls and a grouped layer against the oracle, both output
    types, sampled rows."""
    from lightglue_amd import _lib, mha_hd64_batched, mha_hd64_grouped

    lib = _lib.load()
    for batch, nq, nkv in ((3, 1024, 1024), (2, 2048, 1000), (5, 700, 600)):
        (c,) = _group_inputs([(batch, nq, nkv)], 17 + batch)
        q, k, v = (_t(x, dev, torch.float16) for x in c)
        rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 40)), nq - 1])
        ref = oracle_mod.attention_c(np.ascontiguousarray(c[0][:, :, rows]), c[1], c[2])
        for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
            o = mha_hd64_batched(q, k, v, out_dtype=out_dt)
            assert lib.mha_hd64_last_combine_form() == 0
            torch.cuda.synchronize()
            got = o.float().cpu().numpy()
            assert np.isfinite(got).all()
            assert _maxdiff(got[:, :, rows], ref) <= tol, (batch, nq, nkv, out_dt)
    # 1024 < nkv <= 2048 past one round (forced plan 21): the 4 x 4 passes x 2-tile form
    for batch, nq, nkv in ((2, 2048, 2048), (3, 1100, 1300)):
        (c,) = _group_inputs([(batch, nq, nkv)], 23 + batch)
        q, k, v = (_t(x, dev, torch.float16) for x in c)
        rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 40)), nq - 1])
        ref = oracle_mod.attention_c(np.ascontiguousarray(c[0][:, :, rows]), c[1], c[2])
        ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
        for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
            o = torch.full(q.shape, float("nan"), dtype=out_dt, device=dev)
            st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch, 4, nq, nkv,
                                            0, int(out_dt == torch.float32), 21, 0, 0, ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream().cuda_stream, 3)
            assert st == 0, _lib.last_error()
            torch.cuda.synchronize()
            got = o.float().cpu().numpy()
            assert np.isfinite(got).all()
            assert _maxdiff(got[:, :, rows], ref) <= tol, (batch, nq, nkv, out_dt)
    host = _group_inputs([(1, 2048, 1024), (1, 1024, 2048 - 1100), (1, 1500, 1024)], 29)
    dev_t = [tuple(_t(x, dev, torch.float16) for x in c) for c in host]
    outs = mha_hd64_grouped(dev_t)
    torch.cuda.synchronize()
    for c, o in zip(host, outs):
        assert _maxdiff(o.float().cpu().numpy(), oracle_mod.attention_c(*c)) <= TOL


def test_direct_kernel_forced_outside_its_range_is_rejected(dev):
    from lightglue_amd import _lib

    lib = _lib.load()
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    for nkv, dt, codes in ((2049, torch.float16, (21, 22)), (512, torch.float32, (21, 22))):
        q = torch.zeros(1, 4, 64, 64, dtype=dt, device=dev)
        k = torch.zeros(1, 4, nkv, 64, dtype=dt, device=dev)
        o = torch.empty_like(q)
        for code in codes:
            st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), k.data_ptr(), o.data_ptr(), 1, 4, 64, nkv,
                                            int(dt == torch.float32), int(dt == torch.float32), code, 0, 0,
                                            ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream, 3)
            assert st == 1, (code, nkv, dt)


def test_direct_kernel_deterministic_and_capturable(dev):
    from lightglue_amd import mha_hd64, synth

    qn, kn, vn = synth.qkv(12, 1024, 1024)
    q, k, v = (_t(x, dev, torch.float16) for x in (qn, kn, vn))
    a = mha_hd64(q, k, v).clone()
    b = mha_hd64(q, k, v).clone()
    out = torch.empty_like(q)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        mha_hd64(q, k, v, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        mha_hd64(q, k, v, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(out, a)


@pytest.mark.parametrize("nq,nkv", [(1, 2048), (2048, 1), (2048, 1025), (1025, 2048), (17, 1537), (1536, 1536),
                                     (2047, 2047), (1024, 1088)])
def test_planner_default_edges(nq, nkv, dev, oracle_mod):
    """Edges of the planner's single-pass ranges (1024 / 2048 keys, 256 / 768 blocks) through the
    default plan, both output types, against the C oracle on sampled rows."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    qn, kn, vn = synth.qkv(4242 + nq + 7 * nkv, nq, nkv)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 24)), nq - 1])
    ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    ws = torch.empty(5242880, dtype=torch.uint8, device=dev)
    for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
        o = torch.full(q.shape, float("nan"), dtype=out_dt, device=dev)
        st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1, 4, nq, nkv, 0,
                                        int(out_dt == torch.float32), 0, 0, 0, ws.data_ptr(), ws.numel(),
                                        torch.cuda.current_stream().cuda_stream, 3)
        assert st == 0, _lib.last_error()
        torch.cuda.synchronize()
        got = o.float().cpu().numpy()
        assert np.isfinite(got).all(), (nq, nkv)
        assert _maxdiff(got[:, :, rows], ref) <= tol, (nq, nkv, out_dt)


def test_planner_default_random_shapes(dev, oracle_mod):
    """Seeded random shapes through the planner's default plan (single-pass kernel or LDS ring,
    split or not) for both output types, against the C oracle on sampled rows."""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    rng = np.random.default_rng(2024)
    ws = torch.empty(5242880, dtype=torch.uint8, device=dev)
    for case in range(12):
        batch = int(rng.integers(1, 3))
        nq = int(rng.integers(1, 2049))
        nkv = int(rng.integers(1, 2049))
        qn, kn, vn = synth.qkv(900 + case, nq, nkv, batch=batch)
        q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
        rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 24)), nq - 1])
        ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
        q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
        for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
            o = torch.full(q.shape, float("nan"), dtype=out_dt, device=dev)
            st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), batch, 4, nq, nkv,
                                            0, int(out_dt == torch.float32), 0, 0, 0, ws.data_ptr(), ws.numel(),
                                            torch.cuda.current_stream().cuda_stream, 3)
            assert st == 0, _lib.last_error()
            torch.cuda.synchronize()
            got = o.float().cpu().numpy()
            assert np.isfinite(got).all(), (batch, nq, nkv)
            assert _maxdiff(got[:, :, rows], ref) <= tol, (batch, nq, nkv, out_dt)


@pytest.mark.parametrize("n", [1024, 2048])
def test_full_tensor_at_metric_shapes(n, dev, oracle_mod):
    """Every element of the 1x4xNxN output (the metric shape and the max length) against the C
    oracle (fp64, lightglue_pytorch_no_plugin/lightglue.py:82-84) on the same fp16 inputs: the Half
    path, the Float path (raw fp32 inputs) and fp16-in/fp32-out, with the contract and the
    regression bounds."""
    from lightglue_amd import mha_hd64, mha_hd64_batched, synth

    qn, kn, vn = synth.qkv(9000 + n, n, n)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    ref16 = oracle_mod.attention_c(q16, k16, v16)
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    o = mha_hd64(q, k, v)
    o32 = mha_hd64_batched(q, k, v, out_dtype=torch.float32)
    torch.cuda.synchronize()
    got = o.float().cpu().numpy()
    assert np.isfinite(got).all()
    assert _maxdiff(got, ref16) <= TOL
    _regress16(got, ref16)
    assert _maxdiff(o32.cpu().numpy(), ref16) <= REG_F32OUT
    ref32 = oracle_mod.attention_c(qn, kn, vn)
    of = mha_hd64(*(_t(x, dev, torch.float32) for x in (qn, kn, vn)))
    torch.cuda.synchronize()
    assert _maxdiff(of.cpu().numpy(), ref32) <= REG_FLOAT


def test_outputs_bitwise_identical_on_every_device():
    """SURVEY.md §4 layer 4 / §8e: one pair's call gives the same bits on every GPU of the node."""
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs")
    from lightglue_amd import _lib, mha_hd64, synth

    _lib.load()
    qn, kn, vn = synth.qkv(31337, 1024, 1024)
    outs = []
    for d in range(torch.cuda.device_count()):
        dv = torch.device("cuda", d)
        with torch.cuda.device(dv):
            q, k, v = (_t(x, dv, torch.float16) for x in (qn, kn, vn))
            outs.append(mha_hd64(q, k, v).cpu())
            of = mha_hd64(*(_t(x, dv, torch.float32) for x in (qn, kn, vn))).cpu()
            outs[-1] = (outs[-1], of)
    for a, b in outs[1:]:
        assert torch.equal(a, outs[0][0]) and torch.equal(b, outs[0][1])


@pytest.mark.parametrize("where", ["q", "k", "v"])
@pytest.mark.parametrize("n", [100, 1024])
def test_nan_inputs_propagate_like_the_reference(where, n, dev):
    """The kernels are built with -fno-honor-nans (no NaN-canonicalising max), yet a NaN in Q, K or V
    must still reach the same outputs as in the reference's PyTorch math: a NaN query row gives a
    NaN output row; a NaN key row poisons every row's softmax; a NaN value element poisons its
    output column."""
    from lightglue_amd import mha_hd64, synth

    qn, kn, vn = synth.qkv(4711 + n, n, n)
    x = {"q": qn, "k": kn, "v": vn}[where]
    x[0, 1, n // 3, 5] = np.nan
    qf, kf, vf = (torch.from_numpy(a) for a in (qn, kn, vn))
    ref = torch.softmax((qf @ kf.transpose(-1, -2)) * 0.125, -1) @ vf
    for dt in (torch.float16, torch.float32):
        o = mha_hd64(*(_t(a, dev, dt) for a in (qn, kn, vn)))
        torch.cuda.synchronize()
        assert torch.equal(torch.isnan(o.float().cpu()), torch.isnan(ref)), (where, dt)


@pytest.mark.parametrize("hint", [2, 3, 4])
@pytest.mark.parametrize("nq,nkv", [(1024, 1024), (1000, 777), (512, 2048), (100, 100)])
def test_concurrency_hint_plans_match_oracle(hint, nq, nkv, dev, oracle_mod):
    """mha_hd64_set_concurrency_hint(>= 2): single calls take 32-row blocks (half the CUs; the
    two-per-CU form from 3) so independent streams overlap; same results within the contract."""
    import ctypes

    import lightglue_amd
    from lightglue_amd import _lib, mha_hd64, synth

    qn, kn, vn = synth.qkv(777 + nq + nkv, nq, nkv)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    ref = oracle_mod.attention_c(q16, k16, v16)
    q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
    prev = lightglue_amd.set_concurrency_hint(hint)
    try:
        plan = (ctypes.c_int32 * 4)()
        _lib.load().mha_hd64_plan(1, 4, nq, nkv, 5242880, plan)
        assert plan[0] != 22  # never the whole-chip 16-row kernel under the hint
        a = mha_hd64(q, k, v)
        b = mha_hd64(q, k, v)
        torch.cuda.synchronize()
    finally:
        lightglue_amd.set_concurrency_hint(prev)
    got = a.float().cpu().numpy()
    assert torch.equal(a, b)
    assert _maxdiff(got, ref) <= TOL
    _regress16(got, ref)


@pytest.mark.parametrize("in_dt,out_dt,tol", [(torch.float16, torch.float16, TOL), (torch.float16, torch.float32, TOL_F32OUT),
                                              (torch.float32, torch.float32, TOL)])
def test_grouped_past_one_round_of_128_row_blocks(in_dt, out_dt, tol, dev, oracle_mod):
    """Grouped launches whose calls carry more than 256 128-row blocks and more 32-row blocks than
    the single-pass kernels take: the planner's ring shape (4,1) in its multi-call form (a
    regression: that form was not instantiated and the launch failed with 'invalid argument')."""
    from lightglue_amd import _lib, mha_hd64_grouped

    lib = _lib.load()
    for shapes in ([(8, 1024, 1024), (8, 1024, 1024)], [(12, 1024, 1024), (6, 512, 700), (3, 1000, 77), (9, 200, 1500)]):
        host = _group_inputs(shapes, 61 + len(shapes), np.float16 if in_dt == torch.float16 else np.float32)
        dev_t = [tuple(_t(x, dev, in_dt) for x in c) for c in host]
        outs = mha_hd64_grouped(dev_t, out_dtype=out_dt)
        torch.cuda.synchronize()
        for (qh, kh, vh), o in zip(host, outs):
            b, nq = qh.shape[0], qh.shape[2]
            rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 24)), nq - 1])
            bsel = sorted({0, b - 1})
            q16, k16, v16 = (np.ascontiguousarray(x[bsel]).astype(np.float16).astype(np.float32) for x in (qh, kh, vh))
            ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
            got = o.float().cpu().numpy()
            assert np.isfinite(got).all()
            d = _maxdiff(got[bsel][:, :, rows], ref)
            assert d <= tol, (shapes, qh.shape, d)


# every kernel form (forced plan codes: q_waves, kv_waves, splits as mha_hd64_launch_forced)
NONFINITE_PLANS = [(21, 0, 0), (22, 0, 0), (23, 0, 0), (4, 2, 0), (4, 1, 0), (2, 2, 2), (1, 8, 0), (12, 2, 0), (2, 4, 0)]


@pytest.mark.parametrize("val,where", [(np.nan, "q"), (np.nan, "k"), (np.nan, "v"), (np.inf, "q"), (np.inf, "v")])
def test_nonfinite_inputs_every_plan(val, where, dev):
    """A NaN or Inf in one element reaches exactly the outputs it reaches in the reference's PyTorch
    math, in every kernel form: a query row -> that row only (the matrix-pipe row sums pair each
    query with a partner under a 0 selector, and 0 * NaN would also poison the partner: such a
    query's Q is zeroed in the kernel and its row written as NaN, q_nonfinite_fix); a key row ->
    every row of the head; a value element -> its output column. (An Inf in K is not covered: the
    queries whose score goes to +Inf give NaN rows as in the reference, and their row-sum partners
    can go NaN with them)"""
    from lightglue_amd import _lib, synth

    lib = _lib.load()
    ws = torch.empty(1 << 22, dtype=torch.uint8, device=dev)
    for b, n in ((1, 100), (2, 300)):
        qn, kn, vn = synth.qkv(4711 + n, n, n, batch=b)
        x = {"q": qn, "k": kn, "v": vn}[where]
        x[b - 1, 1, n // 3, 5] = val
        q16, k16, v16 = (synth.round_f16(a) for a in (qn, kn, vn))
        qf, kf, vf = (torch.from_numpy(a).double() for a in (q16, k16, v16))
        ref = torch.softmax((qf @ kf.transpose(-1, -2)) * 0.125, -1) @ vf
        q, k, v = (_t(a, dev, torch.float16) for a in (q16, k16, v16))
        for code, kw, sp in NONFINITE_PLANS:
            for out_dt in (torch.float16, torch.float32):
                o = torch.zeros(q.shape, dtype=out_dt, device=dev)
                st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), b, 4, n, n, 0,
                                                int(out_dt == torch.float32), code, kw, sp, ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream().cuda_stream, 3)
                if st != 0:  # a forced shape this size does not take (e.g. no split for one tile)
                    continue
                torch.cuda.synchronize()
                got = o.double().cpu()
                assert torch.equal(torch.isnan(got), torch.isnan(ref)), (where, val, b, n, code, kw, sp, out_dt)
                fin = torch.isfinite(ref)
                d = float((got[fin] - ref[fin]).abs().max()) if fin.any() else 0.0
                assert d <= TOL, (where, val, b, n, code, kw, sp, out_dt, d)


@pytest.mark.parametrize("batch,nq,nkv", [(2, 1024, 1024), (4, 1024, 1024), (4, 512, 512), (1, 1024, 2048), (3, 1000, 777)])
def test_float_routes_batched_equals_grouped(batch, nq, nkv, dev, oracle_mod):
    """fp32 inputs past the 16-row one-pass forms: the batched launcher sizes its workspace per
    input type (mha_hd64_launch_workspace_bytes_typed), so it takes the same route as the grouped
    launcher (convert + single-pass kernel, or the ring kernel rounding on load past one round of
    32-row blocks / at nkv <= 512): bitwise-equal outputs, within the contract of the oracle on
    the fp16-rounded inputs."""
    from lightglue_amd import mha_hd64_batched, mha_hd64_grouped

    (c,) = _group_inputs([(batch, nq, nkv)], 71 + batch, np.float32)
    q, k, v = (_t(x, dev, torch.float32) for x in c)
    a = mha_hd64_batched(q, k, v)
    (b,) = mha_hd64_grouped([(q, k, v)])
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 24)), nq - 1])
    q16, k16, v16 = (x[[0, batch - 1]].astype(np.float16).astype(np.float32) for x in c)
    ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), np.ascontiguousarray(k16),
                                 np.ascontiguousarray(v16))
    d = _maxdiff(a.cpu().numpy()[[0, batch - 1]][:, :, rows], ref)
    assert d <= TOL_F32OUT, d


@pytest.mark.parametrize("mode", ["default", "hint3", "stream"])
def test_grouped_random_groups(mode, dev, oracle_mod):
    """Seeded random groups through mha_hd64_grouped: 1-6 calls (chunked past 4), batch 1-12,
    nq/nkv 1-2048, fp16 or fp32 inputs, fp16 or fp32 outputs, under the default planner, the
    concurrency hint 3 and stream mode 1 -- every launch form the planner can pick for a group
    (single-pass 16/32-row, their multi-round forms, the ring kernel with or without a split, the
    convert route, the streaming kernel). NaN-filled outputs must be fully written; sampled rows of
    the first and last batch entry against the C oracle on the fp16-rounded inputs."""
    import lightglue_amd
    from lightglue_amd import _lib, mha_hd64_grouped, synth

    lib = _lib.load()
    rng = np.random.default_rng({"default": 31, "hint3": 32, "stream": 33}[mode])
    prev_hint = lightglue_amd.set_concurrency_hint(3) if mode == "hint3" else None
    prev_stream = lib.mha_hd64_set_stream_mode(1 if mode == "stream" else 0)
    try:
        for case in range(10):
            n_calls = int(rng.integers(1, 7))
            in_dt = torch.float32 if rng.random() < 0.3 else torch.float16
            out_dt = torch.float32 if rng.random() < 0.5 else torch.float16
            host, dev_calls, outs = [], [], []
            for i in range(n_calls):
                b = int(rng.integers(1, 13)) if rng.random() < 0.5 else 1
                nq, nkv = int(rng.integers(1, 2049)), int(rng.integers(1, 2049))
                qn, kn, vn = synth.qkv(3100 + 97 * case + 13 * i, nq, nkv, batch=b)
                if in_dt == torch.float16:
                    qn, kn, vn = (synth.round_f16(x) for x in (qn, kn, vn))
                host.append((qn, kn, vn))
                dev_calls.append(tuple(_t(x, dev, in_dt) for x in (qn, kn, vn)))
                outs.append(torch.full((b, 4, nq, 64), float("nan"), dtype=out_dt, device=dev))
            mha_hd64_grouped(dev_calls, out_dtype=out_dt, outs=outs)
            torch.cuda.synchronize()
            tol = TOL if (out_dt == torch.float16 or in_dt == torch.float32) else TOL_F32OUT
            for (qn, kn, vn), o in zip(host, outs):
                b, nq = qn.shape[0], qn.shape[2]
                got = o.float().cpu().numpy()
                assert np.isfinite(got).all(), (mode, case, qn.shape, kn.shape, in_dt, out_dt)
                rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 16)), nq - 1])
                bsel = sorted({0, b - 1})
                q16, k16, v16 = (np.ascontiguousarray(x[bsel]).astype(np.float16).astype(np.float32)
                                 for x in (qn, kn, vn))
                ref = oracle_mod.attention_c(np.ascontiguousarray(q16[:, :, rows]), k16, v16)
                d = _maxdiff(got[bsel][:, :, rows], ref)
                assert d <= tol, (mode, case, qn.shape, kn.shape, in_dt, out_dt, d)
    finally:
        if prev_hint is not None:
            lightglue_amd.set_concurrency_hint(prev_hint)
        lib.mha_hd64_set_stream_mode(prev_stream)


@pytest.mark.parametrize("heads", [1, 2, 3, 8])
def test_batched_launcher_other_head_counts(heads, dev, oracle_mod):
    """The L0 launchers accept any heads (the plugin fixes H = 4): heads 1/2/3/8 at shapes that
    put the planner on each kernel form (16-row single pass, 32-row, ring with and without a
    split, the streaming kernel under stream mode), both output types, against the C oracle."""
    import lightglue_amd
    from lightglue_amd import mha_hd64_batched, synth

    shapes = [(1, 1024, 1024), (2, 1000, 777), (1, 100, 2048), (12, 1024, 1024), (1, 33, 65)]
    for mode in (0, 1):
        prev_stream = lightglue_amd.set_stream_mode(mode)
        try:
            for i, (b, nq, nkv) in enumerate(shapes):
                qn, kn, vn = synth.qkv(7100 + 31 * i + heads, nq, nkv, batch=b, heads=heads)
                q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
                q, k, v = (_t(x, dev, torch.float16) for x in (q16, k16, v16))
                rows = np.unique(np.r_[np.arange(0, nq, max(1, nq // 16)), nq - 1])
                bsel = sorted({0, b - 1})
                ref = oracle_mod.attention_c(np.ascontiguousarray(q16[bsel][:, :, rows]),
                                             np.ascontiguousarray(k16[bsel]), np.ascontiguousarray(v16[bsel]))
                for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
                    o = mha_hd64_batched(q, k, v, out_dtype=out_dt)
                    torch.cuda.synchronize()
                    got = o.float().cpu().numpy()
                    assert np.isfinite(got).all(), (heads, b, nq, nkv, mode)
                    d = _maxdiff(got[bsel][:, :, rows], ref)
                    assert d <= tol, (heads, b, nq, nkv, mode, out_dt, d)
        finally:
            lightglue_amd.set_stream_mode(prev_stream)
