"""What tests/test_gpu_projections.py (the kernels on the MI355X) and tests/test_projections_reference.py (the
bounds themselves, no GPU) share: the input sets, the float64 references and the bounds of the fp16 projection,
LayerNorm + GELU and FFN kernels. A plain module: no fixtures, nothing here touches a GPU. Every reference is
float64 arithmetic on the fp16 operands the kernel reads; the derivation of each bound is in the docstring of
tests/test_gpu_projections.py.
"""
import math
import zlib

import torch

F64 = torch.float64
U16, U24 = 2.0 ** -10, 2.0 ** -24  # twice the unit roundoff of fp16 / fp32


# ---- layouts ------------------------------------------------------------------------------------------------------
def merge_heads(c0, c1):
    """[pairs, heads, n0, 64], [pairs, heads, n1, 64] -> rows [pairs * (n0 + n1), heads * 64], pair-major."""
    p, h, n0, _ = c0.shape
    n1 = c1.shape[2]
    return torch.cat((c0.permute(0, 2, 1, 3).reshape(p, n0, h * 64), c1.permute(0, 2, 1, 3).reshape(p, n1, h * 64)),
                     1).reshape(p * (n0 + n1), h * 64)


def split_heads(rows, pairs, n0, n1):
    """The inverse: rows [pairs * (n0 + n1), heads * 64] -> the two per-image head-major tensors."""
    h = rows.shape[1] // 64
    r = rows.reshape(pairs, n0 + n1, h, 64)
    return r[:, :n0].permute(0, 2, 1, 3).contiguous(), r[:, n0:].permute(0, 2, 1, 3).contiguous()


def sample_rows(m, pairs, n0, n1, tile=128):
    """The rows a large case is checked on: the first tile, both sides of the first four tile seams, the rows either
    side of every pair and image boundary, and the last (ragged) tile."""
    nt = n0 + n1
    rows = set(range(min(tile, m)))
    for j in range(1, 5):
        rows.update((j * tile - 1, j * tile))
    for p in range(pairs):
        rows.update((p * nt - 1, p * nt, p * nt + n0 - 1, p * nt + n0))
    rows.update(range((m - 1) // tile * tile, m))
    return torch.tensor(sorted(r for r in rows if 0 <= r < m))


# ---- the projections' cases -----------------------------------------------------------------------------------------
EPILOGUES = ("linear", "linear_res", "cat", "split2", "qkv")
KINDS = ("int", "gauss", "cancel", "pairscale", "imgscale")


class ProjCase:
    """One call of an entry point: a [m, k] (lg_linear_cat's [x | merge_heads(ctx0, ctx1)]), w [n, k], b [n], res
    [m, n], cos / sin [m, 64], all fp16 on the CPU."""

    def __init__(self, ep, pairs, n0, n1, heads, k, n, kind, seed):
        assert ep in EPILOGUES and kind in KINDS
        self.ep, self.pairs, self.n0, self.n1, self.heads, self.k, self.n, self.kind = ep, pairs, n0, n1, heads, k, n, kind
        m = self.m = pairs * (n0 + n1)
        g = torch.Generator().manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        if kind == "int":  # every partial sum an integer below 2^11: exact in fp32 in any order, exact in fp16
            ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()  # noqa: E731
            a, w, b, res = ri(-2, 2, m, k), ri(-2, 2, n, k), ri(-8, 8, n), ri(-2, 2, m, n)
            q = torch.randint(0, 4, (m, 32), generator=g)  # quarter turns: one of (cos, sin) is 0, the other +-1
            cos, sin = torch.tensor([1.0, 0.0, -1.0, 0.0])[q], torch.tensor([0.0, 1.0, 0.0, -1.0])[q]
        else:
            a, w, b, res = rnd(m, k) * 0.5, rnd(n, k) * 0.05, rnd(n) * 0.1, rnd(m, n) * 0.5
            if ep == "cat":
                a[:, k // 2:] *= 2.0  # (the attention outputs: unit scale, as the existing tests have them)
            if kind == "cancel":  # S >> |ref|: near-constant rows against weights of alternating sign
                a = (0.5 + rnd(m, 1)) * (1.0 + 0.01 * rnd(m, k))
                w = 0.05 * (1.0 + 0.1 * rnd(n, k)) * (1.0 - 2.0 * (torch.arange(k) % 2))
            ang = rnd(m, 32)
            cos, sin = torch.cos(ang), torch.sin(ang)
            scale = torch.ones(pairs, n0 + n1)
            if kind == "pairscale":  # a row taken from the neighbouring pair breaks the bound
                scale *= torch.tensor([1.0 / 16, 4.0, 1.0 / 16]).repeat((pairs + 2) // 3)[:pairs, None]
            if kind == "imgscale":  # image 1 at 16 x image 0
                scale[:, :n0], scale[:, n0:] = 0.25, 4.0
            a, res = a * scale.reshape(m, 1), res * scale.reshape(m, 1)
        self.a, self.w, self.b, self.res = a.half(), w.half(), b.half(), res.half()
        self.cos = cos.repeat_interleave(2, -1).half().contiguous()
        self.sin = sin.repeat_interleave(2, -1).half().contiguous()

    def __repr__(self):
        return f"{self.ep} {self.kind} P={self.pairs} {self.n0}+{self.n1} heads={self.heads} k={self.k} n={self.n}"


def e_lin(lin, s, k):
    return U16 * lin.abs() + 2.0 * (k + 1) * U24 * s + U24


def rotary(x, cos, sin, e=None):
    """Channels [.., 2 hd] of q | k rows x [r, C] (C a multiple of 64): (x0, x1) -> (x0 c0 - x1 s0, x1 c1 + x0 s1) with
    the tables' column ch % 64; with e (the bound of x) also the bound of the result."""
    rep = x.shape[1] // 64
    c, s = cos.repeat(1, rep), sin.repeat(1, rep)
    x0, x1, c0, c1, s0, s1 = x[:, 0::2], x[:, 1::2], c[:, 0::2], c[:, 1::2], s[:, 0::2], s[:, 1::2]
    o = torch.stack((x0 * c0 - x1 * s0, x1 * c1 + x0 * s1), -1).reshape(x.shape)
    if e is None:
        return o
    e0, e1 = e[:, 0::2], e[:, 1::2]
    b0 = c0.abs() * e0 + s0.abs() * e1 + U16 * ((x0 * c0).abs() + (x1 * s0).abs())
    b1 = c1.abs() * e1 + s1.abs() * e0 + U16 * ((x1 * c1).abs() + (x0 * s1).abs())
    return o, torch.stack((b0, b1), -1).reshape(x.shape) + U16 * o.abs() + 3 * U24


def proj_ref(c, rows=None):
    """float64 reference and bound of case c on `rows` (all rows if None), channels in the GEMM's order (split2: a | b,
    qkv: q | k | v): dict(ref, bound, lin, s, exact_sum) — exact_sum the integer-exactness figure max(sum |a||w| + |b|
    + |res|) of section (a)."""
    rows = torch.arange(c.m) if rows is None else rows
    a, w, b = c.a[rows].double(), c.w.double(), c.b.double()
    lin, s = a @ w.t() + b, a.abs() @ w.abs().t() + b.abs()
    e = e_lin(lin, s, c.k)
    ref, bound, exact = lin, e, s
    if c.ep == "linear_res":
        ref = lin + c.res[rows].double()
        bound = e + U16 * ref.abs() + U24
        exact = s + c.res[rows].double().abs()
    elif c.ep == "qkv":
        hd2 = 2 * c.heads * 64
        o, bo = rotary(lin[:, :hd2], c.cos[rows].double(), c.sin[rows].double(), e[:, :hd2])
        ref, bound = torch.cat((o, lin[:, hd2:]), 1), torch.cat((bo, e[:, hd2:]), 1)
    return dict(ref=ref, bound=bound, lin=lin, s=s, exact_sum=float(exact.max()) if exact.numel() else 0.0)


def worst_ratio(out, ref, bound):
    """max |out - ref| / bound over every element (0 for an empty tensor); NaN or Inf in out counts as infinite."""
    if out.numel() == 0:
        return 0.0
    out = out.double()
    if not bool(torch.isfinite(out).all()):
        return math.inf
    return float(((out - ref).abs() / bound).max())


# ---- LayerNorm + GELU ---------------------------------------------------------------------------------------------
LN_KINDS = ("gauss", "off8", "off64", "const")
LN_EPS = 1e-5


def ln_rows(kind, rows, dim, seed):
    """fp16 rows: Gaussian; mean 1 / 8 at spread 0.125 (mean / spread 8 / 64); all-equal (variance 0: the eps path)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(rows, dim, generator=g)
    x = {"gauss": z, "off8": 1.0 + 0.125 * z, "off64": 8.0 + 0.125 * z, "const": torch.full((rows, dim), 3.0)}[kind]
    return x.half()


def ln_params(dim, seed):
    g = torch.Generator().manual_seed(seed)
    return (1.0 + 0.1 * torch.randn(dim, generator=g)).half(), (0.1 * torch.randn(dim, generator=g)).half()


def ln_gelu_ref(x, gamma, beta, eps=LN_EPS):
    """float64 GELU(LayerNorm(x) gamma + beta) (exact erf) -> (ref, t = the GELU's argument)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    d = x - x.mean(-1, keepdim=True)
    t = d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps) * gamma + beta
    return 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0))), t


def ln_bound(ref, t, fp32_out=False):
    return (2.0 ** -22 if fp32_out else U16) * ref.abs() + 2.0 ** -20 * (1.0 + t.abs())


# ---- the FFN's integer model ----------------------------------------------------------------------------------------
class FfnCase:
    """lg_linear_cat_ffn's operands with an exact h: x, ctx and W1 in {-1, 0, 1}, b1 one integer in every channel (0, or
    960 for rows of mean / spread ~ 64: sum h^2 > 2^24), gamma / beta / W2 / b2 at the existing tests' scales."""

    def __init__(self, pairs, n0, n1, b1, seed):
        self.pairs, self.n0, self.n1, self.m = pairs, n0, n1, pairs * (n0 + n1)
        g = torch.Generator().manual_seed(seed)
        ri = lambda *s: torch.randint(-1, 2, s, generator=g).half()  # noqa: E731
        rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
        self.a, self.w1 = ri(self.m, 512), ri(512, 512)
        self.b1 = torch.full((512,), float(b1)).half()
        self.gamma, self.beta = (1.0 + 0.1 * rnd(512)).half(), (0.1 * rnd(512)).half()
        self.w2, self.b2 = (rnd(256, 512) * 0.05).half(), (rnd(256) * 0.1).half()

    def model(self, rows=None):
        """h exact; g = fp16(GELU(LN(h))); v = fp16(W2 g + b2); out = fp16(x + v): dict(h, exact_sum, g64, t, g, v, out)."""
        rows = torch.arange(self.m) if rows is None else rows
        a = self.a[rows].double()
        h = a @ self.w1.double().t() + self.b1.double()
        exact = float((a.abs() @ self.w1.double().abs().t() + self.b1.double().abs()).max()) if len(rows) else 0.0
        g64, t = ln_gelu_ref(h, self.gamma, self.beta)
        g = g64.half()
        v = (g.double() @ self.w2.double().t() + self.b2.double()).half()
        out = (a[:, :256] + v.double()).half()
        return dict(h=h, exact_sum=exact, g64=g64, t=t, g=g, v=v, out=out)


# ---- the shapes of section (d), shared so that the CPU tests can assert the integer precondition on each ------------
HEAD_SHAPES = ((1, 1, 63), (1, 56, 1), (2, 29, 28), (3, 37, 70), (1, 0, 70), (1, 70, 0))  # (pairs, n0, n1)


def seed_of(*key):
    return zlib.crc32(repr(key).encode())


def proj_shapes(ep, wide):
    """(pairs, n0, n1, heads, k, n) of every small case of entry point `ep` under lg_linear_set_wide(wide): the 64 x 64
    form's and the 128 x 128 form's row counts either side of a tile, both K, channel counts of one tile, a ragged
    number of 128-wide tiles (192: the 64 x 64 form under either setting), several tiles; the head-major epilogues on
    HEAD_SHAPES with 1, 2, 4 and 8 heads."""
    if ep in ("linear", "linear_res"):
        ms, ns = ((1, 63, 64, 65), (64, 192, 512, 768)) if wide == 0 else ((1, 127, 128, 129, 257), (128, 512, 768, 192))
        return [(1, m, 0, 0, k, n) for m in ms for k in (256, 512) for n in ns]
    if ep == "cat":
        ns = (64, 192, 512) if wide == 0 else (128, 192, 512, 768)
        return [(p, n0, n1, h, 128 * h, n) for p, n0, n1 in HEAD_SHAPES for h in (2, 4) for n in ns]
    per = 2 if ep == "split2" else 3
    return [(p, n0, n1, h, k, per * h * 64) for p, n0, n1 in HEAD_SHAPES for h in (1, 2, 4, 8) for k in (256, 512)]


LARGE_M = (5, 1000, 1180)  # 10,900 rows: 86 x 6 tiles of 128 x 128 at n = 768, more than the 512 resident workgroups


def large_case(ep, kind="gauss"):
    p, n0, n1 = LARGE_M
    if ep in ("linear", "linear_res"):
        return ProjCase(ep, 1, p * (n0 + n1), 0, 0, 512, 768, kind, seed_of("large", ep))
    heads, k = {"cat": (4, 512), "split2": (6, 512), "qkv": (4, 256)}[ep]
    return ProjCase(ep, p, n0, n1, heads, k, 768, kind, seed_of("large", ep))


def split_m(m):
    """m rows as one pair: (pairs, n0, n1) with n0 = m // 2 (m = 1: an empty image 0)."""
    return 1, m // 2, m - m // 2


FFN_SMALL_M = {0: (1, 17, 33, 65), 2: (1, 31, 33, 65), 3: (1, 15, 17, 33)}  # by lg_linear_set_ffn_fused mode
FFN_LARGE = (59, 70, 69)            # 8,201 rows: ffn_rows_kernel's 64-row form (past 8,192), a ragged last workgroup
FFN_PROJ_M = (17, 1000, 1040)       # the 16-row kernel: split over two workgroups up to 1,024 rows, whole past it
FFN_B1 = (0, 960)
LN_FUSED_M = (1, 63, 65, 130)
LN_FUSED_LARGE = (3, 5000, 5923)    # 32,769 rows: linear_ln_kernel's 128-row form (from 32,768 on)
