"""The bounds of tests/test_gpu_projections.py checked on the CPU, without a GPU: each accepts a float32 restatement
of the arithmetic the kernels state and rejects arithmetic that is wrong in a way a kernel could be.

Accepted (worst error / bound <= 1 on every input set the GPU tests use): the projection summed in fp32 in ascending
and in descending k with lin_val's fp16(acc + bias); res_add's fp16(fp16(lin) + res); rot_pair's fp16 products and
sum; LayerNorm + exact GELU with fp32 statistics in two passes, and as the one-launch FFN kernels merge them (each
64-channel share's sum and squares about its own mean, then the shares); at mean / spread up to 128.

Rejected (worst error / bound > 1): partial sums rounded to fp16 every 16 columns; a dropped 8-column k-slice; a
residual row taken from the neighbouring pair (pair scales 1/16, 4, 1/16); the one-pass variance E[x^2] - mean^2 at
mean / spread 64.

Not separable, so not a mutant here: the rotary evaluated in fp32 with one rounding. include/lightglue_glue.h pins
fp16 products and an fp16 sum for lg_linear_qkv_rotary, but an upper bound on the error cannot reject arithmetic that
rounds less; the rotary bound is a sum of the roundings rot_pair makes, and the fp32 form lies inside it (asserted
below, as a statement of what the bound does not see). The exact integer cases of the GPU tests do not see it either
(quarter-turn tables make both forms exact).

The integer cases' precondition (every partial sum below 2^11, so fp32 sums are exact in any order and the result is
an fp16 integer) is asserted here on the float64 reference of every shape and seed the GPU tests run.
"""
import numpy as np
import pytest
import torch

import projection_refs as R

F16, F32 = np.float16, np.float32


def gemm_f32(a, w, order, chunk16=False):
    """sum over k in `order` of a[:, k] w[:, k] in fp32, one rounding per addition (the fp16 products are exact in
    fp32). chunk16: the mutant that rounds the running sum to fp16 after every 16 columns."""
    a32, w32 = a.float().numpy(), w.float().numpy()
    acc = np.zeros((a32.shape[0], w32.shape[0]), F32)
    part = np.zeros_like(acc)
    for i, kk in enumerate(order):
        part += a32[:, kk, None] * w32[None, :, kk]
        if chunk16 and i % 16 == 15:
            acc = (acc + part).astype(F16).astype(F32)
            part[:] = 0
    return acc if chunk16 else part


def restate(c, order, chunk16=False, a=None, res=None, rotary32=False):
    """Case c through the kernels' stated output arithmetic on the CPU -> [m, n] fp16 values as a float64 tensor."""
    acc = gemm_f32(c.a if a is None else a, c.w, order, chunk16)
    v = (acc + c.b.float().numpy()[None, :]).astype(F16)  # lin_val
    if c.ep == "linear_res":
        r = (c.res if res is None else res).float().numpy()
        v = (v.astype(F32) + r).astype(F16)  # res_add
    elif c.ep == "qkv":
        hd2 = 2 * c.heads * 64
        rep = hd2 // 64
        cs, sn = np.tile(c.cos.numpy(), (1, rep)), np.tile(c.sin.numpy(), (1, rep))
        x = v[:, :hd2]
        xr = np.stack((-x[:, 1::2], x[:, 0::2]), -1).reshape(x.shape)  # rotate_half
        if rotary32:
            o = (x.astype(F32) * cs.astype(F32) + xr.astype(F32) * sn.astype(F32)).astype(F16)
        else:  # rot_pair: each product and the sum rounded to fp16
            o = ((x * cs).astype(F16) + (xr * sn).astype(F16)).astype(F16)
        v = np.concatenate((o, v[:, hd2:]), 1)
    return torch.from_numpy(v.astype(np.float64))


def small_case(ep, kind, k=512):
    heads = {"linear": 0, "linear_res": 0, "cat": k // 128, "split2": 1, "qkv": 1}[ep]
    n = {"linear": 192, "linear_res": 192, "cat": 192, "split2": 128, "qkv": 192}[ep]
    p, n0, n1 = (1, 3 * 107, 0) if heads == 0 else (3, 37, 70)
    return R.ProjCase(ep, p, n0, n1, heads, k, n, kind, R.seed_of("cpu", ep, kind, k))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("ep", R.EPILOGUES)
def test_bounds_accept_the_stated_arithmetic(ep, kind):
    worst = 0.0
    for k in (256, 512):
        c = small_case(ep, kind, k)
        r = R.proj_ref(c)
        for order in (range(k), range(k - 1, -1, -1)):
            got = restate(c, order)
            if kind == "int":
                assert torch.equal(got, r["ref"]), (c, "the integer case is not exact")
            worst = max(worst, R.worst_ratio(got, r["ref"], r["bound"]))
        if ep == "qkv":  # (the docstring: inside the bound, hence no mutant)
            assert R.worst_ratio(restate(c, range(k), rotary32=True), r["ref"], r["bound"]) <= 1.0
    print(f"{ep} {kind}: fp32 restatement, both k orders, worst err / bound {worst:.3f}")
    assert worst <= 1.0, (ep, kind, worst)


@pytest.mark.parametrize("ep", R.EPILOGUES)
def test_bounds_reject_wrong_sums(ep):
    c = small_case(ep, "gauss")
    r = R.proj_ref(c)
    half = R.worst_ratio(restate(c, range(c.k), chunk16=True), r["ref"], r["bound"])
    a = c.a.clone()
    a[:, 8:16] = 0
    dropped = R.worst_ratio(restate(c, range(c.k), a=a), r["ref"], r["bound"])
    print(f"{ep}: fp16 partial sums every 16 k {half:.2f}, a dropped 8-column k-slice {dropped:.1f} (err / bound)")
    assert half > 1.0 and dropped > 1.0, (ep, half, dropped)


def test_bound_rejects_a_residual_row_of_the_neighbouring_pair():
    c = R.ProjCase("linear_res", 3, 37, 70, 0, 512, 192, "pairscale", R.seed_of("cpu", "neighbour"))
    r = R.proj_ref(c)
    assert R.worst_ratio(restate(c, range(c.k)), r["ref"], r["bound"]) <= 1.0
    worst = R.worst_ratio(restate(c, range(c.k), res=torch.roll(c.res, 107, 0)), r["ref"], r["bound"])
    print(f"residual rows from the neighbouring pair: worst err / bound {worst:.1f}")
    assert worst > 1.0


# ---- LayerNorm + GELU ---------------------------------------------------------------------------------------------
def ln_f32(x, gamma, beta, form, eps=R.LN_EPS):
    """fp32 LayerNorm + erf GELU on fp16 rows. form: 'two' (sum, then squares about the mean), 'merge' (per 64-channel
    share: sum, squares about the share's own mean; then variance = (sum M2 + 64 sum (share mean - mean)^2) / dim),
    'one' (E[x^2] - mean^2)."""
    x = x.float().numpy()
    dim = x.shape[1]
    inv = F32(1.0 / dim)
    mean = (x.sum(1, dtype=F32) * inv)[:, None]
    if form == "two":
        d = x - mean
        var = (d * d).sum(1, dtype=F32)[:, None] * inv
    elif form == "merge":
        sh = x.reshape(x.shape[0], dim // 64, 64)
        s = sh.sum(2, dtype=F32)
        dd = sh - (s * F32(1.0 / 64))[:, :, None]
        m2 = (dd * dd).sum(2, dtype=F32)
        db = s * F32(1.0 / 64) - mean
        var = ((db * db).sum(1, dtype=F32) * F32(64) + m2.sum(1, dtype=F32))[:, None] * inv
    else:
        var = np.maximum((x * x).sum(1, dtype=F32)[:, None] * inv - mean * mean, F32(0))
    rstd = (F32(1) / np.sqrt(var + F32(eps))).astype(F32)
    t = torch.from_numpy((x - mean) * rstd * gamma.float().numpy() + beta.float().numpy())
    return (0.5 * t * (1.0 + torch.erf(t * 0.70710678118654752))).float()


def offset_rows(ratio, dim, seed):
    """fp16 rows of spread 0.125 and mean 0.125 * ratio."""
    g = torch.Generator().manual_seed(seed)
    return (0.125 * ratio + 0.125 * torch.randn(64, dim, generator=g)).half()


@pytest.mark.parametrize("dim", (64, 128, 256, 512, 1024))
def test_layernorm_bound_accepts_two_pass_and_merged_statistics(dim):
    gamma, beta = R.ln_params(dim, 3)
    sets = [(f"mean/spread {ratio}", offset_rows(ratio, dim, R.seed_of("ln", dim, ratio))) for ratio in (0, 8, 16, 64, 128)]
    sets += [(kind, R.ln_rows(kind, 5, dim, R.seed_of("lnk", dim, kind))) for kind in R.LN_KINDS]
    for name, x in sets:
        ref, t = R.ln_gelu_ref(x, gamma, beta)
        for form in ("two", "merge"):
            y = ln_f32(x, gamma, beta, form)
            w16 = R.worst_ratio(y.half(), ref, R.ln_bound(ref, t))
            w32 = R.worst_ratio(y, ref, R.ln_bound(ref, t, fp32_out=True))
            print(f"dim {dim} {name} {form}: worst err / bound fp16 out {w16:.3f}, fp32 out {w32:.3f}")
            assert w16 <= 1.0 and w32 <= 1.0, (dim, name, form, w16, w32)


def test_layernorm_bound_rejects_one_pass_variance_at_offset_rows():
    gamma, beta = R.ln_params(512, 3)
    out = {}
    for ratio in (8, 64):
        x = offset_rows(ratio, 512, R.seed_of("ln", 512, ratio))
        ref, t = R.ln_gelu_ref(x, gamma, beta)
        out[ratio] = R.worst_ratio(ln_f32(x, gamma, beta, "one").half(), ref, R.ln_bound(ref, t))
    x = R.ln_rows("off64", 5, 512, R.seed_of("lnk", 512, "off64"))
    ref, t = R.ln_gelu_ref(x, gamma, beta)
    rows5 = R.worst_ratio(ln_f32(x, gamma, beta, "one").half(), ref, R.ln_bound(ref, t))
    print(f"one-pass variance, worst err / bound: mean/spread 8 {out[8]:.2f}, 64 {out[64]:.1f} (the GPU test's rows {rows5:.1f})")
    assert out[8] <= 1.0 and out[64] > 1.0 and rows5 > 1.0


# ---- the integer cases' precondition ------------------------------------------------------------------------------
@pytest.mark.parametrize("ep", R.EPILOGUES)
def test_integer_cases_are_exact_in_fp32_and_fp16(ep):
    worst = 0.0
    for wide in (0, 1):
        for shape in R.proj_shapes(ep, wide):
            c = R.ProjCase(ep, *shape, "int", R.seed_of(ep, wide, shape))
            r = R.proj_ref(c)
            worst = max(worst, r["exact_sum"])
            assert r["exact_sum"] <= 2048, (c, r["exact_sum"])
            assert torch.equal(r["ref"].half().double(), r["ref"]), c
    c = R.large_case(ep, "int")
    r = R.proj_ref(c, R.sample_rows(c.m, c.pairs, c.n0, c.n1))
    assert max(worst, r["exact_sum"]) <= 2048
    print(f"{ep}: max sum |a||w| + |b| + |res| over every integer case {max(worst, r['exact_sum']):.0f} (<= 2048)")


def test_ffn_integer_model_has_an_exact_hidden_row():
    shapes = {R.split_m(m) for ms in R.FFN_SMALL_M.values() for m in ms} | {R.split_m(m) for m in R.FFN_PROJ_M} | {R.FFN_LARGE}
    for b1 in R.FFN_B1:
        for shape in sorted(shapes):
            c = R.FfnCase(*shape, b1, R.seed_of("ffn", shape, b1))
            rows = R.sample_rows(c.m, *shape, tile=64) if c.m > 2000 else None
            mo = c.model(rows)
            assert mo["exact_sum"] <= 2048 and float(mo["h"].abs().max()) <= 2048, (shape, b1)
            assert torch.equal(mo["h"].half().double(), mo["h"])
            if b1:  # the offset rows: mean / spread ~ 64 and a sum of squares past 2^24
                h = mo["h"]
                ratio = (h.mean(1).abs() / h.std(1, unbiased=False)) if h.shape[1] > 1 else None
                assert float((h * h).sum(1).min()) > 2.0 ** 24 and 40 <= float(ratio.median()) <= 100, (shape, float(ratio.median()))


def test_ulp_bound_is_the_matcher_tests_own():
    """The FFN model is compared under tests/test_matcher.py's _ulp_bound(k=2): 2 fp16 ulps of max(|out|, |out - x|, 1/4)."""
    from test_matcher import _ulp_bound

    out, x = torch.tensor([0.0, 1.0, -3.0, 100.0]).half(), torch.tensor([0.0, 0.5, 2.0, -100.0]).half()
    assert torch.equal(_ulp_bound(out, x), torch.tensor([0.25, 1.0, 5.0, 200.0]) * 2.0 ** -9)
