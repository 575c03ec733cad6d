"""The fp16 projection, LayerNorm + GELU and FFN kernels on the MI355X (csrc/lightglue_linear.hip, lightglue_ffn_ln.hip,
lightglue_ffn.hip, the row kernels of lightglue_glue.hip, with lightglue_device.h) against exact arithmetic: every reference is float64 on the
CPU, computed here (tests/projection_refs.py) from the fp16 operands the kernel reads. Nothing reads the reference
tree and no reference comes from a GPU GEMM. tests/test_projections_reference.py shows on the CPU that each bound
below accepts the stated arithmetic in fp32 and rejects fp16 partial sums, a dropped k-slice, a neighbour's residual
row and the one-pass variance.

Calls go through lightglue_amd._host.call on raw pointers. Every output (each head-major tensor on its own, and the h
scratch of lg_linear_cat_ffn) is a view inside a larger allocation with 4 KiB of a sentinel byte on both sides and NaN
inside: after the call the guards are unchanged and no NaN is left (gpu_common.GuardedOut). Every row-indexed input
(A / x, ctx0, ctx1, res, cos, sin) has NaN before and 4 KiB of NaN behind it (GuardedIn): a read past row m - 1 that
reaches a result shows there.

(a) Exact integer cases, no tolerance. A, W, ctx, res in {-2..2}, bias in {-8..8}: sum |a||w| + |b| + |res| <= 2048
(asserted on the float64 reference, for every shape and seed, by the CPU tests), so every partial sum is an integer
below 2^11: exact in fp32 in any order and exact in fp16. The rotary tables are quarter turns (one of cos, sin is 0,
the other +-1): rot_pair's fp16 products and sum are exact too. The kernel equals the float64 result in every element
(as fp16 numbers: the sign of an exact zero follows the order of a sum, which nothing pins), which covers every
k-slot, every swizzled LDS unit, the A-gather, the head-major scatter, bias and residual columns.
The FFN: x, ctx, W1 in {-1, 0, 1} and one integer b1 give an exact h (|h| <= 512 + 960), so the LayerNorm's input is
the model's bit for bit and only its arithmetic can differ: out is compared with g = fp16(GELU(LN(h))), v = fp16(W2 g +
b2), out = fp16(x + v) under tests/test_matcher.py's _ulp_bound(k=2) (one GELU output may move by an fp16 ulp, and
with it the rounding of v and of x + v), and the two-call form's g (left in the h buffer) under the LayerNorm bound of
(c). b1 = 960 with a spread of ~15 is a row of mean / spread ~ 64 whose sum of squares passes 2^24.

(b) Gaussian cases, every element under a derived bound. S = |A| |W|^T + |b| in float64, K the GEMM's depth.
  projection (lin_val: fp16(acc + b), acc an fp32 sum of K exact products in the kernel's order):
      E_lin = 2^-10 |lin| + 2 (K + 1) 2^-24 S + 2^-24
    an fp32 sum of K + 1 terms errs by at most (K + 1) 2^-24 S to first order whatever its order (factor 2 for the
    higher orders and the MFMA's internal order); one fp16 rounding is 2^-11 of the rounded value (2^-10 |lin| covers
    it and the error it is applied to); 2^-24 is the spacing of fp16 subnormals.
  residual (res_add: fp16(fp16(lin) + res), the sum exact in fp32): E_lin + 2^-10 |ref| + 2^-24, one more fp16 rounding.
  rotary (rot_pair: o = fp16(fp16(x0 c) +- fp16(x1 s)) on the fp16 x): the inputs' errors scaled by |c| and |s|, one
      rounding per product, one for the sum:
      |c| E(x0) + |s| E(x1) + 2^-10 (|x0 c| + |x1 s|) + 2^-10 |ref| + 3 2^-24
  the v part of lg_linear_qkv_rotary: E_lin.
Input sets: the existing tests' scales (x 0.5, W 0.05, b 0.1); near-constant rows against weights of alternating sign
(S >> |ref|: the absolute term is the bound); pair scales 1/16, 4, 1/16 and image 1 at 16 x image 0, so that a row
taken from a neighbour breaks the bound instead of hiding in it.

(c) LayerNorm + GELU, y = GELU(t), t = (x - mean) rstd gamma + beta:
      |y - ref| <= 2^-10 |ref| + 2^-20 (1 + |t|)        (fp32 outputs: 2^-22 |ref| + the same)
The relative term is the output's rounding. The absolute term: the rows are fp16 values (also where the call is fp32),
so the row sum is exact in fp32 when the values share a binade (the offset rows) and otherwise |mean| is of the order
of the spread; x - mean then carries one fp32 rounding; the sum of dim <= 1024 squares is 16 serial additions and a
6-level tree (or 8 waves' partials), a relative error of some 2^-20 in the variance and half that in rstd, beside the
hardware's 1-ulp v_rsq_f32 (2^-23): together below 2^-20 |t| with the two products and the addition of gamma and beta;
GELU's slope is at most 1.13, gelu_as's erf is within 1.5e-7 (~2^-22.7) and its v_rcp_f32 / v_exp_f32 within 1 ulp of
factors of order 1: below 2^-20 in all. None of this depends on mean / spread, which is the point: the one-pass
variance E[x^2] - mean^2 loses log2((mean / spread)^2) bits before it subtracts and misses this bound 5- to 17-fold at
64 (CPU tests), as the kernels did before they formed the variance from squares about a mean.

(d) Shapes: the smallest that reach each path (projection_refs.proj_shapes and the constants after it): rows either side
of the 64- and 128-row tiles, both K, one / a ragged number of / several channel tiles, n = 192 under the 128 x 128
setting (falls back), pairs that straddle tiles with 1-row and empty images, 1 / 2 / 4 / 8 heads, 8-B aligned
bias / out / res / cos / sin against the aligned call's bits, one persistent case per epilogue (10,900 rows x 768
channels: more tiles than resident workgroups), linear_ln_kernel's 64- and 128-row forms, the FFN's 16-, 32- and 64-row
forms, lg_linear_cat_ffn_proj's three kinds with the projection split over two workgroups and whole. The large cases
run every row on the GPU and compare sampled rows (projection_refs.sample_rows).
"""
import ctypes
import math

import pytest
import torch

import projection_refs as R
from gpu_common import SENTINEL_BYTE, GuardedIn, GuardedOut, same_bits

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


class forced:
    """with forced(lib, "lg_linear_set_wide", 0): the hook set for the block, the previous value restored after it."""

    def __init__(self, lib, hook, value):
        self.fn, self.value = getattr(lib, hook), value

    def __enter__(self):
        self.prev = self.fn(self.value)

    def __exit__(self, *exc):
        self.fn(self.prev)


def call(name, *args):
    from lightglue_amd import _host

    _host.call(name, *args, torch.cuda.current_stream().cuda_stream)


def head_outs(dev, c, count, shift):
    """`count` head-major outputs per image: [image][j] -> GuardedOut [pairs, heads, ni, 64]."""
    return [[GuardedOut((c.pairs, c.heads, ni, 64), F16, dev, shift) for _ in range(count)] for ni in (c.n0, c.n1)]


def merged(outs, what):
    """Head-major outputs checked and put back into rows: [m, count * heads * 64] in the GEMM's channel order."""
    o0, o1 = ([o.check(f"{what} image {i} output {j}") for j, o in enumerate(os_)] for i, os_ in enumerate(outs))
    return torch.cat([R.merge_heads(a, b) for a, b in zip(o0, o1)], 1)


def run_proj(dev, c, shift=0):
    """Case c through its entry point; bias / out / res / cos / sin `shift` bytes off 16-B alignment -> rows [m, n]."""
    w, b = c.w.to(dev), GuardedIn(c.b, dev, shift)
    if c.ep in ("linear", "linear_res"):
        a, out = GuardedIn(c.a, dev), GuardedOut((c.m, c.n), F16, dev, shift)
        res = GuardedIn(c.res, dev, shift) if c.ep == "linear_res" else None
        call("lg_linear", a.ptr, w.data_ptr(), b.ptr, res.ptr if res else None, c.m, c.n, c.k, out.ptr)
        return out.check(repr(c))
    if c.ep == "cat":
        x = GuardedIn(c.a[:, :c.k // 2].contiguous(), dev)
        c0, c1 = (GuardedIn(t, dev) for t in R.split_heads(c.a[:, c.k // 2:], c.pairs, c.n0, c.n1))
        out = GuardedOut((c.m, c.n), F16, dev, shift)
        call("lg_linear_cat", x.ptr, c0.ptr, c1.ptr, c.heads, c.n0, c.n1, c.pairs, w.data_ptr(), b.ptr, c.n, out.ptr)
        return out.check(repr(c))
    a = GuardedIn(c.a, dev)
    if c.ep == "split2":
        o = head_outs(dev, c, 2, shift)
        call("lg_linear_split2", a.ptr, w.data_ptr(), b.ptr, c.heads, c.n0, c.n1, c.pairs, c.k, o[0][0].ptr, o[1][0].ptr,
             o[0][1].ptr, o[1][1].ptr)
    else:
        cos, sin = GuardedIn(c.cos, dev, shift), GuardedIn(c.sin, dev, shift)
        o = head_outs(dev, c, 3, shift)
        call("lg_linear_qkv_rotary", a.ptr, w.data_ptr(), b.ptr, cos.ptr, sin.ptr, c.heads, c.n0, c.n1, c.pairs, c.k,
             *(t.ptr for t in o[0]), *(t.ptr for t in o[1]))
    return merged(o, repr(c))


def equal_values(a, b):
    """Equal element for element as numbers, in one dtype (a NaN equals nothing; -0 equals +0: the sign of an exact zero
    depends on the order of a sum, which no kernel pins)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


def check_proj(dev, c, rows=None, shift=0):
    """Run c; integer cases bit for bit, the others under their bound, on `rows` (all if None). -> (ratio, GPU rows)."""
    got = run_proj(dev, c, shift)
    r = R.proj_ref(c, rows)
    sel = got if rows is None else got[rows]
    if c.kind == "int":
        assert r["exact_sum"] <= 2048, (c, r["exact_sum"])
        assert equal_values(sel, r["ref"].half()), (c, "differs from the exact result", R.worst_ratio(sel, r["ref"], r["bound"]))
        return 0.0, got
    worst = R.worst_ratio(sel, r["ref"], r["bound"])
    assert worst <= 1.0, (c, worst)
    return worst, got


# ---- (a), (b), (d): the four projection entry points ------------------------------------------------------------------
@pytest.mark.parametrize("wide", (0, 1))
@pytest.mark.parametrize("ep", R.EPILOGUES)
def test_projection_small_shapes_exact_and_bounded(dev, lib, ep, wide):
    """Every small shape of (d) in both tile settings: the integer case bit for bit, the Gaussian case under (b)."""
    worst = 0.0
    with forced(lib, "lg_linear_set_wide", wide):
        for shape in R.proj_shapes(ep, wide):
            for kind in ("int", "gauss"):
                worst = max(worst, check_proj(dev, R.ProjCase(ep, *shape, kind, R.seed_of(ep, wide, shape)))[0])
    print(f"{ep} wide={wide}: {len(R.proj_shapes(ep, wide))} shapes exact on integers; Gaussian worst err / bound {worst:.3f}")


@pytest.mark.parametrize("wide", (0, 1))
@pytest.mark.parametrize("ep", R.EPILOGUES)
def test_projection_input_sets(dev, lib, ep, wide):
    """Cancellation-heavy operands, pair scales 1/16, 4, 1/16 and image 1 at 16 x image 0, three pairs of 37 + 70 rows
    (and 2 x (29 + 28): pairs that straddle a tile more than once)."""
    worst = {}
    with forced(lib, "lg_linear_set_wide", wide):
        for p, n0, n1 in ((3, 37, 70), (2, 29, 28)):
            for kind in ("cancel", "pairscale", "imgscale"):
                if ep in ("linear", "linear_res"):
                    c = R.ProjCase(ep, p, n0, n1, 0, 512, 768 if wide else 192, kind, R.seed_of(ep, wide, kind, p))
                else:
                    heads = 4
                    n = {"cat": 512, "split2": 2 * heads * 64, "qkv": 3 * heads * 64}[ep]
                    c = R.ProjCase(ep, p, n0, n1, heads, 512 if ep == "cat" else 256, n, kind, R.seed_of(ep, wide, kind, p))
                worst[kind] = max(worst.get(kind, 0.0), check_proj(dev, c)[0])
    print(f"{ep} wide={wide}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("ep", R.EPILOGUES)
def test_projection_eight_byte_alignment_gives_the_aligned_bits(dev, lib, ep):
    """bias / out / res / cos / sin 8-B but not 16-B aligned (the documented minimum) route to the 64 x 64 form also
    where the 128 x 128 form is asked for: the same bits as the aligned call, and exact on integers."""
    shape = (1, 129, 0, 0, 512, 768) if ep in ("linear", "linear_res") else (3, 37, 70, 4, 512 if ep == "cat" else 256,
                                                                            {"cat": 512, "split2": 512, "qkv": 768}[ep])
    worst = 0.0
    with forced(lib, "lg_linear_set_wide", 1):
        for kind in ("int", "gauss"):
            c = R.ProjCase(ep, *shape, kind, R.seed_of(ep, "align", kind))
            (w0, aligned), (w8, off) = check_proj(dev, c), check_proj(dev, c, shift=8)
            assert same_bits(aligned, off), (c, "8-B aligned pointers change the result")
            worst = max(worst, w0, w8)
    print(f"{ep} 8-B aligned: the aligned call's bits; worst err / bound {worst:.3f}")


@pytest.mark.parametrize("ep", R.EPILOGUES)
def test_projection_persistent_tiles(dev, lib, ep):
    """10,900 rows x 768 channels in the 128 x 128 form: 516 tiles for 512 resident workgroups, so a workgroup walks
    over a tile seam with its ring running. Every row on the GPU (all outputs guarded), sampled rows against float64."""
    worst = 0.0
    with forced(lib, "lg_linear_set_wide", 1):
        for kind in ("int", "gauss"):
            c = R.large_case(ep, kind)
            assert (c.m + 127) // 128 * (c.n // 128) > 512
            worst = max(worst, check_proj(dev, c, R.sample_rows(c.m, c.pairs, c.n0, c.n1))[0])
    print(f"{ep} {c.m} rows x {c.n}: exact on integers; Gaussian worst err / bound {worst:.3f} on sampled rows")


# ---- (a): the layout kernels ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (F16, F32))
def test_layout_kernels_move_every_element(dev, dtype):
    """lg_qkv_rotary_split (quarter-turn tables: exact in either arithmetic), lg_split_heads2_ld on column views of one
    wider tensor, lg_merge_heads_cat: small integers, bit for bit, on the head-major shapes with 1, 2 and 4 heads."""
    from lightglue_amd import _host

    dt = _host.DT[dtype]
    n_cases = 0
    for p, n0, n1 in R.HEAD_SHAPES:
        for heads in (1, 2, 4):
            m, hd = p * (n0 + n1), heads * 64
            g = torch.Generator().manual_seed(R.seed_of("layout", p, n0, n1, heads))
            ri = lambda *s: torch.randint(-9, 10, s, generator=g).to(dtype)  # noqa: E731
            c = R.ProjCase("qkv", p, n0, n1, heads, 256, 3 * hd, "int", R.seed_of("layout-tables", p, n0, n1))
            cos, sin = c.cos.to(dtype), c.sin.to(dtype)
            what = f"{dtype} P={p} {n0}+{n1} heads={heads}"
            # qkv [m, hd * 3] with channel (h * 64 + d) * 3 + j
            qkv = ri(m, hd, 3)
            outs = [[GuardedOut((p, heads, ni, 64), dtype, dev) for _ in range(3)] for ni in (n0, n1)]
            ins = [GuardedIn(t, dev) for t in (qkv, cos, sin)]
            call("lg_qkv_rotary_split", dt, ins[0].ptr, ins[1].ptr, ins[2].ptr, heads, n0, n1, p,
                 *(t.ptr for t in outs[0]), *(t.ptr for t in outs[1]))
            got = merged(outs, "lg_qkv_rotary_split " + what)
            q, k, v = (qkv[:, :, j].double() for j in range(3))
            ref = torch.cat((R.rotary(q, cos.double(), sin.double()), R.rotary(k, cos.double(), sin.double()), v), 1)
            assert equal_values(got, ref.to(dtype)), ("lg_qkv_rotary_split", what)
            # a | b: column views of one [m, 2 hd] tensor
            ab = ri(m, 2 * hd)
            src = GuardedIn(ab, dev)
            outs = [[GuardedOut((p, heads, ni, 64), dtype, dev) for _ in range(2)] for ni in (n0, n1)]
            call("lg_split_heads2_ld", dt, src.ptr, src.ptr + hd * ab.element_size(), 2 * hd, heads, n0, n1, p, outs[0][0].ptr,
                 outs[1][0].ptr, outs[0][1].ptr, outs[1][1].ptr)
            assert same_bits(merged(outs, "lg_split_heads2_ld " + what), ab), ("lg_split_heads2_ld", what)
            # [x | merge_heads(x0, x1)]
            x, ctx = ri(m, hd), ri(m, hd)
            xi = GuardedIn(x, dev)
            c0, c1 = (GuardedIn(t, dev) for t in R.split_heads(ctx, p, n0, n1))
            out = GuardedOut((m, 2 * hd), dtype, dev)
            call("lg_merge_heads_cat", dt, xi.ptr, c0.ptr, c1.ptr, heads, n0, n1, p, out.ptr)
            assert same_bits(out.check("lg_merge_heads_cat " + what), torch.cat((x, ctx), 1)), ("lg_merge_heads_cat", what)
            n_cases += 3
    print(f"layout kernels {dtype}: {n_cases} calls bit for bit (worst err / bound 0.000: exact)")


# ---- (c): LayerNorm + GELU --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (F16, F32))
@pytest.mark.parametrize("dim", (64, 128, 256, 512, 1024))
def test_layernorm_gelu_against_float64(dev, dim, dtype):
    """lg_layernorm_gelu on 1, 3, 4 and 5 rows (a block is 4 rows), out of place and in place, 16-B aligned and 8 B off
    it (dim 512 in fp16 then takes the generic kernel), on Gaussian rows, rows of mean / spread 8 and 64, and all-equal
    rows (variance 0: the eps path). The rows are fp16 values in either dtype."""
    from lightglue_amd import _host

    gamma, beta = (t.to(dtype) for t in R.ln_params(dim, R.seed_of("ln-params", dim)))
    worst = {}
    for kind in R.LN_KINDS:
        x5 = R.ln_rows(kind, 5, dim, R.seed_of("ln-rows", dim, kind)).to(dtype)
        ref5, t5 = R.ln_gelu_ref(x5, gamma, beta)
        bound5 = R.ln_bound(ref5, t5, fp32_out=dtype == F32)
        for rows in (1, 3, 4, 5):
            for shift in (0, 8):
                for in_place in (False, True):
                    what = f"lg_layernorm_gelu {dtype} dim {dim} {kind} rows {rows} shift {shift} in place {in_place}"
                    gi, bi = GuardedIn(gamma, dev, shift), GuardedIn(beta, dev, shift)
                    out = GuardedOut((rows, dim), dtype, dev, shift, fill=x5[:rows] if in_place else None)
                    xin = out if in_place else GuardedIn(x5[:rows], dev, shift)
                    call("lg_layernorm_gelu", _host.DT[dtype], xin.ptr, gi.ptr, bi.ptr, rows, dim, R.LN_EPS, out.ptr)
                    ratio = R.worst_ratio(out.check(what), ref5[:rows], bound5[:rows])
                    assert ratio <= 1.0, (what, ratio)
                    worst[kind] = max(worst.get(kind, 0.0), ratio)
    print(f"lg_layernorm_gelu {dtype} dim {dim}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def ln_fused_case(pairs, n0, n1, kind, seed):
    """lg_linear_cat_ln_gelu's operands for a row kind of (c), with an exact acc + b — integers in A, multiples of 2^-8
    (2^-6) in W and b, every partial sum below 2^24 of that unit — so that the one-launch form's h = fp16(acc + b), rounded
    once (mixh), and lg_linear_cat's, rounded through fp32 (lin_val), are the same single rounding: with a rounded
    acc + b a few elements in 10^5 are the other fp16 neighbour, and one fp16 ulp of h is far outside any bound on the
    LayerNorm's arithmetic. 'gauss': A = round(2 z), W = round(1.5 z) 2^-6, b = round(6.4 z) 2^-6 (h of unit spread, a
    sum of 512 terms); 'off8' / 'off64': A in {-2..2}, W = +-2^-8 (spread 0.125) under a constant bias 1 / 8; 'const':
    W = 0 under a constant bias (all-equal rows). 'rounded': the existing tests' Gaussian operands (for the two-launch
    form, whose h is lg_linear_cat's)."""
    c = R.ProjCase("cat", pairs, n0, n1, 4, 512, 512, "gauss", seed)
    if kind == "rounded":
        return c
    g = torch.Generator().manual_seed(seed + 1)
    z = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    if kind == "gauss":
        c.a, c.w, c.b = torch.round(2.0 * z(c.m, 512)).half(), (torch.round(1.5 * z(512, 512)) / 64).half(), (torch.round(6.4 * z(512)) / 64).half()
    else:
        c.a = torch.randint(-2, 3, (c.m, 512), generator=g).half()
        c.w = ((2.0 * torch.randint(0, 2, (512, 512), generator=g) - 1.0) * (0.0 if kind == "const" else 2.0 ** -8)).half()
        c.b = torch.full((512,), {"off8": 1.0, "off64": 8.0, "const": 3.0}[kind]).half()
    return c


def run_cat_ln_gelu(dev, c, gamma, beta):
    """-> (lg_linear_cat's h, lg_linear_cat_ln_gelu's output) on the same operands, both guarded."""
    x = GuardedIn(c.a[:, :256].contiguous(), dev)
    c0, c1 = (GuardedIn(t, dev) for t in R.split_heads(c.a[:, 256:], c.pairs, c.n0, c.n1))
    w, b, g, be = (t.to(dev) for t in (c.w, c.b, gamma, beta))
    h, out = GuardedOut((c.m, 512), F16, dev), GuardedOut((c.m, 512), F16, dev)
    call("lg_linear_cat", x.ptr, c0.ptr, c1.ptr, 4, c.n0, c.n1, c.pairs, w.data_ptr(), b.data_ptr(), 512, h.ptr)
    call("lg_linear_cat_ln_gelu", x.ptr, c0.ptr, c1.ptr, 4, c.n0, c.n1, c.pairs, w.data_ptr(), b.data_ptr(), g.data_ptr(),
         be.data_ptr(), R.LN_EPS, out.ptr)
    return h.check(f"lg_linear_cat {c}"), out.check(f"lg_linear_cat_ln_gelu {c}")


@pytest.mark.parametrize("form", (0, 2))
def test_linear_cat_ln_gelu_forms_against_float64(dev, lib, form):
    """lg_linear_cat_ln_gelu forced to two launches (0: lg_linear_cat, then ln_gelu_512_f16_kernel in place) and to one
    (2: linear_ln_kernel, 64-row tiles; 128-row tiles at 32,769 rows) against float64 GELU(LN(h)) on the kernel's own
    h = lg_linear_cat's output on the same operands, under the bound of (c): operands with an exact acc + b
    (ln_fused_case: every form's h is then the same bits, asserted against the float64 sum), and for the two-launch
    form also the existing tests' Gaussian operands."""
    gamma, beta = R.ln_params(512, R.seed_of("ln-params", 512))
    shapes = [R.split_m(m) if m != 130 else (2, 30, 35) for m in R.LN_FUSED_M] + [R.LN_FUSED_LARGE]
    worst = {}
    with forced(lib, "lg_linear_set_ln_fused", form), forced(lib, "lg_linear_set_wide", -1):
        for shape in shapes:
            for kind in R.LN_KINDS + (("rounded",) if form == 0 else ()):
                if shape == R.LN_FUSED_LARGE and kind in ("off8", "const"):
                    continue  # (the large case: the Gaussian and the mean / spread 64 rows)
                c = ln_fused_case(*shape, kind, R.seed_of("ln-fused", shape, kind))
                h, out = run_cat_ln_gelu(dev, c, gamma, beta)
                rows = R.sample_rows(c.m, *shape) if c.m > 30000 else torch.arange(c.m)
                if kind != "rounded":  # acc + b is exact: h is its one rounding
                    lin = c.a[rows].double() @ c.w.double().t() + c.b.double()
                    assert torch.equal(lin.float().double(), lin) and equal_values(h[rows], lin.half()), (c, kind, "h is not exact")
                if kind in ("off8", "off64"):  # the rows are what they are meant to be
                    ratio = float((h[rows].double().mean(1).abs() / h[rows].double().std(1)).median())
                    assert (6 if kind == "off8" else 48) <= ratio <= (11 if kind == "off8" else 85), (c, ratio)
                ref, t = R.ln_gelu_ref(h[rows], gamma, beta)
                r = R.worst_ratio(out[rows], ref, R.ln_bound(ref, t))
                assert r <= 1.0, (form, c, kind, r)
                worst[kind] = max(worst.get(kind, 0.0), r)
    print(f"lg_linear_cat_ln_gelu form {form}: worst err / bound " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ---- (a): the FFN against its integer model ---------------------------------------------------------------------------
def run_ffn(dev, c, packed=True):
    """lg_linear_cat_ffn on FfnCase c -> (out, the h scratch's GuardedOut: checked by the caller where it is written)."""
    x = GuardedIn(c.a[:, :256].contiguous(), dev)
    c0, c1 = (GuardedIn(t, dev) for t in R.split_heads(c.a[:, 256:], c.pairs, c.n0, c.n1))
    w1, b1, g, be, w2, b2 = (t.to(dev) for t in (c.w1, c.b1, c.gamma, c.beta, c.w2, c.b2))
    wp = None
    if packed:
        from lightglue_amd import matcher as mt

        wp = mt.ffn_pack(w1, w2)
    h, out = GuardedOut((c.m, 512), F16, dev), GuardedOut((c.m, 256), F16, dev)
    call("lg_linear_cat_ffn", x.ptr, c0.ptr, c1.ptr, 4, c.n0, c.n1, c.pairs, w1.data_ptr(), b1.data_ptr(), g.data_ptr(),
         be.data_ptr(), R.LN_EPS, w2.data_ptr(), b2.data_ptr(), wp.data_ptr() if packed else None, h.ptr, out.ptr)
    return out.check(f"lg_linear_cat_ffn P={c.pairs} {c.n0}+{c.n1}"), h


def check_ffn_out(c, out, rows, what):
    """out[rows] against the integer model under _ulp_bound(k=2) -> (worst err / bound, the model)."""
    from test_matcher import _ulp_bound

    mo = c.model(rows)
    assert mo["exact_sum"] <= 2048
    x = c.a[rows][:, :256]
    bound = _ulp_bound(mo["out"], x, k=2.0).double()
    ratio = R.worst_ratio(out[rows], mo["out"].double(), bound)
    assert ratio <= 1.0, (what, ratio)
    return ratio, mo


@pytest.mark.parametrize("b1", R.FFN_B1)
@pytest.mark.parametrize("mode", (0, 2, 3))
def test_ffn_forms_against_the_integer_model(dev, lib, mode, b1):
    """lg_linear_cat_ffn forced to its two calls (0), the 32 / 64-row kernel (2) and the 16-row kernel (3) on an exact h:
    rows either side of each form's tile and 8,201 rows (the 64-row form under 2, sampled rows), b1 = 0 and the offset
    rows of b1 = 960. The two-call form leaves g = GELU(LN(h)) in the h buffer: checked under the bound of (c)."""
    shapes = [R.split_m(m) for m in R.FFN_SMALL_M[mode]] + [R.FFN_LARGE]
    worst, worst_g = 0.0, 0.0
    with forced(lib, "lg_linear_set_ffn_fused", mode), forced(lib, "lg_linear_set_ln_fused", 1):
        for shape in shapes:
            c = R.FfnCase(*shape, b1, R.seed_of("ffn", shape, b1))
            out, h = run_ffn(dev, c)
            rows = R.sample_rows(c.m, *shape, tile=64) if c.m > 2000 else torch.arange(c.m)
            ratio, mo = check_ffn_out(c, out, rows, (mode, shape, b1))
            worst = max(worst, ratio)
            if mode == 0:
                g = h.check("the h scratch of the two-call form")[rows]
                rg = R.worst_ratio(g, mo["g64"], R.ln_bound(mo["g64"], mo["t"]))
                assert rg <= 1.0, (mode, shape, b1, "g", rg)
                worst_g = max(worst_g, rg)
            else:  # (the one-launch forms leave the scratch alone: its guards at least)
                assert bool((h.buf[:h.lo] == SENTINEL_BYTE).all()) and bool((h.buf[h.hi:] == SENTINEL_BYTE).all())
    print(f"lg_linear_cat_ffn mode {mode} b1 {b1}: worst err / bound {worst:.3f} under _ulp_bound(k=2)"
          + (f", g under the LayerNorm bound {worst_g:.3f}" if mode == 0 else ""))


@pytest.mark.parametrize("kind", (1, 2, 3))
def test_ffn_proj_kinds_against_float64(dev, lib, kind):
    """lg_linear_cat_ffn_proj (the 16-row kernel by size: its projection split over two workgroups up to 1,024 rows, whole
    at 1,040) with kinds SPLIT2, QKV and PLAIN (n_store 8, 384, 512): the FFN output against the integer model under
    _ulp_bound(k=2), the projection against float64 on the kernel's own FFN output under the bounds of (b), K = 256."""
    from lightglue_amd import matcher as mt

    ep = {1: "split2", 2: "qkv", 3: "linear"}[kind]
    n3 = 768 if kind == 2 else 512
    worst_x, worst_p = 0.0, 0.0
    for b1 in R.FFN_B1:
        for m in R.FFN_PROJ_M:
            for n_store in ((8, 384, 512) if kind == 3 else (0,)):
                shape = R.split_m(m)
                c = R.FfnCase(*shape, b1, R.seed_of("ffn", shape, b1))
                p = R.ProjCase(ep, *shape, 4, 256, n3, "gauss", R.seed_of("ffn-proj", kind, m, b1))  # (W3, b3, cos, sin)
                if kind == 3:
                    p.w[n_store:], p.b[n_store:] = 0, 0
                x = GuardedIn(c.a[:, :256].contiguous(), dev)
                c0, c1 = (GuardedIn(t, dev) for t in R.split_heads(c.a[:, 256:], *shape))
                b1d, g, be, b2, b3 = (t.to(dev) for t in (c.b1, c.gamma, c.beta, c.b2, p.b))
                wp = mt.ffn_pack(c.w1.to(dev), c.w2.to(dev), p.w.to(dev))
                cos, sin = GuardedIn(p.cos, dev), GuardedIn(p.sin, dev)
                out = GuardedOut((c.m, 256), F16, dev)
                if kind == 3:
                    o3 = [GuardedOut((c.m, n_store), F16, dev)]
                    ptrs = [o3[0].ptr]
                else:
                    o3 = head_outs(dev, p, kind + 1, 0)
                    ptrs = ([o3[0][0].ptr, o3[1][0].ptr, o3[0][1].ptr, o3[1][1].ptr] if kind == 1
                            else [t.ptr for t in o3[0]] + [t.ptr for t in o3[1]])
                arr = (ctypes.c_void_p * 6)(*(ptrs + [None] * (6 - len(ptrs))))
                call("lg_linear_cat_ffn_proj", x.ptr, c0.ptr, c1.ptr, 4, c.n0, c.n1, c.pairs, b1d.data_ptr(), g.data_ptr(),
                     be.data_ptr(), R.LN_EPS, b2.data_ptr(), wp.data_ptr(), kind, b3.data_ptr(),
                     cos.ptr if kind == 2 else None, sin.ptr if kind == 2 else None, n_store, arr, out.ptr)
                what = f"lg_linear_cat_ffn_proj kind {kind} m {m} b1 {b1} n_store {n_store}"
                xo = out.check(what)
                worst_x = max(worst_x, check_ffn_out(c, xo, torch.arange(c.m), what)[0])
                got = o3[0].check(what) if kind == 3 else merged(o3, what)
                p.a = xo  # the projection's input: the kernel's own FFN output
                r = R.proj_ref(p)
                ncol = n_store if kind == 3 else n3
                ratio = R.worst_ratio(got, r["ref"][:, :ncol], r["bound"][:, :ncol])
                assert ratio <= 1.0, (what, ratio)
                worst_p = max(worst_p, ratio)
    print(f"lg_linear_cat_ffn_proj kind {kind}: FFN output worst err / bound {worst_x:.3f} under _ulp_bound(k=2), projection "
          f"{worst_p:.3f}")
