"""What tests/test_gpu_assignment.py (the kernels on the MI355X) and tests/test_assignment_reference.py (the bound
itself, no GPU) share: the input sets, the float64 references and the error bound of the assignment head
(csrc/lightglue_assign.hip: lg_assign_scores[_lens], lg_assign_matches[_lens]) and of the two dual log-softmax entry
points of csrc/lightglue_glue.hip (lg_log_double_softmax, lg_log_double_softmax_f16), and the float64 reference of
lg_pair_inputs' rotary tables. A plain module: numpy only, no fixtures, nothing here touches a GPU.

The operation, in float64 on the operands the kernel reads:

    scores[i][j] = 2 x[i][j] - L[i] - C[j] + g(z0[i]) + g(z1[j]),   g(z) = min(z, 0) - log1p(exp(-|z|))

L the logsumexp of row i of x, C of column j. For the v entry points x = fp16(m0 . m1^T) of the fp16 rows (the float64
dot product rounded once to fp16); for the other two x is the sim operand as given. On a ragged pair both logsumexps
run over the valid [m_len, n_len] block and every other score is -inf. NaN and -inf follow IEEE: a NaN in x makes its
row's L and its column's C NaN; a -inf entry adds 0 to both sums and is -inf itself.

The bound, per element (U = 2^-24, the fp32 unit roundoff; eps_h = 2^-22, the modelled relative error of one hardware
__expf / __logf call: the one constant nothing documents, measured in profiles/assignment_exact/INDEX.md):

  x.   Where x is exactly representable (asserted in float64 for the `exact`, `peaky`, `ramp`, `z`, `neg_inf` and `nan`
       sets) it carries no error. Elsewhere (`gauss`) the kernel's fp32 accumulation errs by at most
       tol = 2 * 257 * U * (|m0| . |m1|^T), so it rounds to another fp16 value only where the float64 dot product
       lies within tol of an fp16 rounding boundary; there x may move by dx = tol + ulp16(x) (tol exceeds the ulp
       where x is small), 2 x by 2 dx, and L and C by the element's share of their sums times dx. Everywhere else
       dx = 0: the kernel's fp16 similarity is the reference's.
  L, C. A kernel forms Lhat = M + log(s), s = sum_j exp(x_j - M) in fp32, through a chain of at most A additions and at
       most R exponential factors per term (the term's own exponential and one more for every rescale of the partial
       sum that holds it; R and A are counted from the code, per kernel and shape, in `chain_*` below). The maxima along
       a chain only rise, so the arguments of a term's R exponentials add up to d_j = x_j - M: their roundings (the
       fp32 subtraction and the scaling by log2 e inside __expf) are 2 |d_j| U relative to the term, whatever the
       chain. With w_j = exp(d_j) / s the term's share:
           rel_s = R (eps_h + U) + A U + 2 U sum_j w_j |d_j|
           E_L   = rel_s + (eps_h + U) |log s| + U |L|
       ((eps_h + U) |log s|: __logf and its scaling by ln 2; U |L|: the addition M + log s).
  g.   t = exp(-|z|) carries eps_h + |z| U, log1p two fp32 ulps, the subtraction one:
           E_g = t / (1 + t) (eps_h + |z| U) + 2 U log1p(t) + U |g|
  combine. N fp32 additions (3 for the fp16 kernels: g - L, then 2 x + rterm, then + cterm; 4 for dual_combine_kernel's
       left-to-right sum) on the magnitudes they see: N U (|2 x| + |L| + |C| + |g0| + |g1|).
  2^-126 on top: a kernel may flush an fp32 subnormal (g(100) = -3.7e-44) to zero.

  E[i][j] = 2 dx[i][j] + sum_j' w_ij' dx[i][j'] + sum_i' w_i'j dx[i'][j]
            + E_L[i] + E_C[j] + E_g(z0[i]) + E_g(z1[j]) + combine + 2^-126

The match head: expf(score) of the best entry carries the score's error through exp and the expf's own rounding:
|mscore - exp(s)| <= exp(s) (E + eps_h (1 + |s|)).
"""
import math

import numpy as np

U = 2.0 ** -24
EPS_H = 2.0 ** -22      # relative error granted to one hardware exp / log (tests/test_gpu_match_head.py's figure for expf)
TINY = 2.0 ** -126
LD, ZC = 384, 256       # v's row stride and the matchability channel, as the matcher lays them out
NINF = -np.inf
Z_VALUES = (0.0, 0.5, -0.5, 3.0, -3.0, 12.0, -12.0, 100.0, -100.0, 65504.0, -65504.0)
PAIR_SCALES = (1.0 / 16, 4.0, 1.0 / 16)   # batches of 3 (batch_scales of tests/test_gpu_superpoint.py)

# ---- the shapes (P, m, n): the smallest that reach each path, from the launch rules of the two .hip files -------------
ASSIGN_SHAPES = {            # -> (S, BPW, combine W)
    (1, 1, 8): (8, 1, 1),        # S = 8, every share but the first empty
    (1, 33, 72): (8, 1, 1),      # S = 8, a row tail past a 32-row strip
    (3, 300, 296): (4, 1, 1),    # S = 4, one block per wave, two live splits, three pairs
    (1, 8, 1032): (4, 2, 1),     # S = 4, two blocks per wave, all four splits live on the row side
    (1, 40, 2048): (2, 4, 1),
    (3, 8, 2048): (1, 8, 1),     # one split, 8 blocks per wave; the 8-row combine
    (2, 2048, 8): (1, 8, 4),     # the 32-row combine
    (1, 70, 520): (8, 1, 1),     # more than one 512-column block
}
F32_SHAPES = ((1, 1, 1), (1, 3, 5), (1, 129, 65), (3, 130, 257))
F16_SHAPES = {               # -> (small form, CPL)
    (1, 9, 8): (True, 1), (1, 9, 520): (True, 2), (1, 9, 1032): (True, 4),
    (1, 1032, 8): (True, 1),     # col_lse_kernel walks 129 row blocks: more than 16 groups x 8
    (64, 65, 8): (False, 1),     # the 64-row form, a second block of one row
    (4, 1025, 8): (False, 1),    # 17 partials per column: combine16_kernel<.., false>'s second batch of 16
}
MATCH_SHAPES = ((1, 1, 8), (1, 33, 72), (3, 300, 296), (1, 70, 520))


def cdiv(a, b):
    return -(-a // b)


def up256(x):
    return cdiv(x, 256) * 256


def assign_plan(m, n, batch):
    """assign_splits, launch_assign_lse's BPW and assign_scores_run's combine width, restated."""
    base, s = (cdiv(m, 32) + cdiv(n, 32)) * batch, 1
    while s < 8 and base * s * 2 <= 256:
        s *= 2
    bpw = cdiv(cdiv(max(m, n), 32), 8 * s)
    bpw = 1 if bpw <= 1 else 2 if bpw <= 2 else 4 if bpw <= 4 else 8
    return s, bpw, 4 if cdiv(m, 32) * cdiv(n, 512) * batch >= 128 else 1


def assign_workspace(m, n, batch, s):
    return up256(batch * m * n * 2) + up256(batch * s * m * 8) + up256(batch * s * n * 8) + up256(batch * m * 4) + up256(batch * n * 4)


def f16_plan(m, n, batch):
    small = cdiv(m, 64) * batch < 64
    return small, 1 if n <= 512 else 2 if n <= 1024 else 4


def f16_workspace(m, n, batch, small):
    rb = cdiv(m, 8 if small else 64)
    return up256(batch * m * 4) + up256(batch * rb * n * 8) + (batch * n * 4 if small else 0)


def f32_workspace(m, n, batch):
    return up256(cdiv(m * 4, 16) * 16 + cdiv(m, 128) * n * 8) * batch


class Chain:
    """The longest chain of fp32 additions (A) and exponential factors (R) behind a row's and a column's logsumexp."""

    def __init__(self, a_row, r_row, a_col, r_col, n_comb):
        self.a_row, self.r_row, self.a_col, self.r_col, self.n_comb = a_row, r_row, a_col, r_col, n_comb


def chain_assign(m, n, batch):
    """assign_lse_kernel<BPW>: 16 BPW additions per lane, one shuffle, 8 waves, then lse_close's S merges (each one
    addition and at most one more exponential factor on every term)."""
    s, bpw, _ = assign_plan(m, n, batch)
    a, r = 16 * bpw + 1 + 8 + s, 1 + s
    return Chain(a, r, a, r, 3)


def chain_f32(m, n):
    """lse_kernel: a row is ceil(n / 64) additions per lane and 6 shuffle levels, one exponential; a column is up to 32
    online steps per thread, 3 merges in the block and one per 128-row chunk in dual_combine_kernel."""
    c = cdiv(m, 128)
    return Chain(cdiv(n, 64) + 6, 1, 32 + 3 + c, 32 + 3 + c + 1, 4)


def chain_f16(m, n, batch):
    """lse16_kernel: a row is 8 CPL additions per lane and 6 levels; a column is one batch (the carried sum and 8 rows),
    W - 1 merges in the block, then col_lse_kernel's ceil(rblocks / 16) + 15 merges (small form) or combine16's rblocks."""
    small, cpl = f16_plan(m, n, batch)
    merges = (cdiv(cdiv(m, 8), 16) + 15) if small else (7 + cdiv(m, 64))
    return Chain(8 * cpl + 6, 1, 9 + merges, 2 + merges, 3)


# ---- float64 reference -------------------------------------------------------------------------------------------------
def logsig(z):
    z = np.asarray(z, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(z, 0.0) - np.log1p(np.exp(-np.abs(z)))


def _lse(x, axis):
    """(logsumexp, max, sum_j w_j |d_j|) along axis; NaN propagates, -inf entries add nothing."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        mx = np.max(x, axis=axis, keepdims=True)          # (np.max propagates NaN)
        d = x - mx
        e = np.exp(d)
        s = e.sum(axis=axis, keepdims=True)
        wd = np.where(e > 0, e * np.abs(np.where(np.isfinite(d), d, 0.0)), 0.0).sum(axis=axis, keepdims=True) / s
        wd = np.where(np.isnan(s), np.nan, wd)
        return (mx + np.log(s)).squeeze(axis), mx.squeeze(axis), wd.squeeze(axis), e / s


def ulp16(x):
    """The fp16 spacing at |x| (the larger neighbour distance)."""
    h = np.abs(np.asarray(x, np.float64)).astype(np.float16)
    return (np.nextafter(h, np.float16(np.inf)).astype(np.float64) - h.astype(np.float64))


def ref_scores(x, z0, z1, chain, mlen=None, nlen=None, doubt=None):
    """x [P, m, n], z0 [P, m], z1 [P, n] (any float dtype, taken as exact), doubt: dx [P, m, n] or None -> (scores,
    bound) float64 [P, m, n]."""
    x, z0, z1 = (np.asarray(t, np.float64) for t in (x, z0, z1))
    pr, m, n = x.shape
    scores, bound = np.full(x.shape, NINF), np.zeros(x.shape)
    for p in range(pr):
        ml, nl = (m if mlen is None else int(mlen[p])), (n if nlen is None else int(nlen[p]))
        xs, a, b = x[p, :ml, :nl], z0[p, :ml], z1[p, :nl]
        row, rmx, rwd, rw = _lse(xs, 1)
        col, cmx, cwd, cw = _lse(xs, 0)
        g0, g1 = logsig(a), logsig(b)
        with np.errstate(invalid="ignore", over="ignore"):
            scores[p, :ml, :nl] = 2.0 * xs - row[:, None] - col[None, :] + g0[:, None] + g1[None, :]

            def e_lse(l, mx, wd, a_n, r_n):
                return r_n * (EPS_H + U) + a_n * U + 2.0 * U * wd + (EPS_H + U) * np.abs(l - mx) + U * np.abs(l)

            def e_g(z, g):
                t = np.exp(-np.abs(z))
                return t / (1.0 + t) * (EPS_H + np.abs(z) * U) + 2.0 * U * np.log1p(t) + U * np.abs(g)

            el, ec = e_lse(row, rmx, rwd, chain.a_row, chain.r_row), e_lse(col, cmx, cwd, chain.a_col, chain.r_col)
            e = (el[:, None] + ec[None, :] + e_g(a, g0)[:, None] + e_g(b, g1)[None, :] + TINY +
                 chain.n_comb * U * (np.abs(2.0 * xs) + np.abs(row)[:, None] + np.abs(col)[None, :] + np.abs(g0)[:, None] +
                                     np.abs(g1)[None, :]))
            if doubt is not None:
                du = doubt[p, :ml, :nl]
                e = e + 2.0 * du + (rw * du).sum(1, keepdims=True) + (cw * du).sum(0, keepdims=True)
        bound[p, :ml, :nl] = e
    return scores, bound


def compare(got, ref, bound):
    """-> (worst |got - ref| / bound over the finite entries of ref, a message or None). Where ref is NaN got must be
    NaN, where ref is infinite got must equal it, elsewhere got is finite and within the bound."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return math.inf, f"shape {got.shape} != {ref.shape}"
    nan, inf = np.isnan(ref), np.isinf(ref)
    fin = ~(nan | inf)
    if not np.isnan(got[nan]).all():
        return math.inf, f"{int((~np.isnan(got[nan])).sum())} entries not NaN where the reference is"
    if not (got[inf] == ref[inf]).all():
        return math.inf, f"{int((got[inf] != ref[inf]).sum())} entries differ where the reference is infinite"
    if not np.isfinite(got[fin]).all():
        k = np.argwhere(fin & ~np.isfinite(got))[0]
        return math.inf, f"{int((~np.isfinite(got[fin])).sum())} entries not finite where the reference is, first at {tuple(k)}"
    if not fin.any():
        return 0.0, None
    ratio = np.abs(got[fin] - ref[fin]) / bound[fin]
    worst = float(ratio.max())
    if worst > 1.0:
        k = np.argwhere(fin)[int(ratio.argmax())]
        return worst, f"error / bound {worst:.3g} at {tuple(k)}: got {got[tuple(k)]!r}, reference {ref[tuple(k)]!r}"
    return worst, None


# ---- float64 filter_matches_dense (include/lightglue_glue.h, lg_assign_matches[_lens]) -------------------------------------
def ref_matches(scores, th, mlen=None, nlen=None):
    """scores [P, m, n] float64 -> dict of matches0, matches1, scores0, scores1, matches, match_scores, counts and, for the
    tests' own assertions, arg0 / arg1 (each valid row's best column, each valid column's best row), best0 (the row's best
    score) and gap0 / gap1 (best minus second best; inf where there is one entry)."""
    pr, m, n = scores.shape
    k = min(m, n)
    o = dict(matches0=np.full((pr, m), -1, np.int32), matches1=np.full((pr, n), -1, np.int32), scores0=np.zeros((pr, m)),
             scores1=np.zeros((pr, n)), matches=np.full((pr, k, 2), -1, np.int32), match_scores=np.zeros((pr, k)),
             counts=np.zeros(pr, np.int32), best0=np.full((pr, m), np.nan), gap0=np.full((pr, m), np.inf),
             gap1=np.full((pr, n), np.inf), arg0=np.zeros((pr, m), np.int64), arg1=np.zeros((pr, n), np.int64))
    for p in range(pr):
        ml, nl = (m if mlen is None else int(mlen[p])), (n if nlen is None else int(nlen[p]))
        s = scores[p, :ml, :nl]
        j0, i1 = s.argmax(1), s.argmax(0)                 # the lowest index among equals
        best = s[np.arange(ml), j0]
        if nl > 1:
            o["gap0"][p, :ml] = best - np.sort(s, 1)[:, -2]
        if ml > 1:
            o["gap1"][p, :nl] = s[i1, np.arange(nl)] - np.sort(s, 0)[-2, :]
        mutual0 = i1[j0] == np.arange(ml)
        ms0 = np.where(mutual0, np.exp(best), 0.0)
        valid0 = ms0 > th
        mutual1 = j0[i1] == np.arange(nl)
        o["best0"][p, :ml] = best
        o["arg0"][p, :ml], o["arg1"][p, :nl] = j0, i1
        o["matches0"][p, :ml] = np.where(valid0, j0, -1)
        o["scores0"][p, :ml] = ms0
        o["matches1"][p, :nl] = np.where(mutual1 & valid0[i1], i1, -1)
        o["scores1"][p, :nl] = np.where(mutual1, ms0[i1], 0.0)
        idx = np.nonzero(valid0)[0]
        c = len(idx)
        o["matches"][p, :c, 0], o["matches"][p, :c, 1] = idx, j0[idx]
        o["match_scores"][p, :c] = ms0[idx]
        o["counts"][p] = c
    return o


def mscore_bound(best, e_best):
    """|expf(shat) - exp(s)| for |shat - s| <= e_best."""
    return np.exp(best) * (e_best + EPS_H * (1.0 + np.abs(best)))


# ---- input sets ------------------------------------------------------------------------------------------------------------
V_SETS = ("exact", "gauss", "peaky", "ramp", "ramp_desc", "z", "nan")
SIM_SETS = V_SETS + ("neg_inf",)


def seed_of(*key):
    import zlib

    return zlib.crc32(repr(key).encode())


def _pm_rows(rng, rows, nch, nnz, amp):
    """`rows` rows of 256 channels: nnz entries of +-amp among the first nch channels, the rest 0."""
    out = np.zeros((rows, 256))
    pos = np.argsort(rng.random((rows, nch)), 1)[:, :nnz]
    np.put_along_axis(out, pos, amp * rng.choice((-1.0, 1.0), (rows, nnz)), 1)
    return out, pos


def _exact_pair(rng, ml, nl, nch=256, nnz=96, amp=0.5):
    """Image 0: ml rows of nnz entries +-amp. Image 1: nl such rows, half of them (as far as image 0 has rows) copies of
    distinct rows of image 0 with 0 to 11 signs flipped. Every similarity is a multiple of amp^2 below 2^11 of them."""
    a, pos = _pm_rows(rng, ml, nch, nnz, amp)
    b, _ = _pm_rows(rng, nl, nch, nnz, amp)
    k = min(ml, nl // 2)
    src, dst = rng.permutation(ml)[:k], rng.permutation(nl)[:k]
    for s, d in zip(src, dst):
        row = a[s].copy()
        flips = rng.permutation(pos[s])[:int(rng.integers(0, 12))]
        row[flips] *= -1.0
        b[d] = row
    return a, b


def _z_normal(rng, k):
    return np.clip(np.round(rng.normal(size=k) * 2.0 * 4.0) / 4.0, -8.0, 8.0)


class Inputs:
    """One call's operands: v [P, m + n, LD] fp16 (channels 0..255 and ZC; padded rows of a ragged pair hold NaN / Inf),
    mlen / nlen int arrays or None. x_exact: every similarity is exactly representable in fp16 (asserted by x())."""

    def __init__(self, kind, shape, ragged=False, seed=0, scales=PAIR_SCALES):
        assert kind in V_SETS
        self.kind, self.shape, self.ragged = kind, shape, ragged
        pr, m, n = shape
        self.x_exact = kind != "gauss"
        self.mlen = self.nlen = None
        if ragged:
            self.mlen, self.nlen = ragged_counts(shape)
        v = np.zeros((pr, m + n, LD))
        self.peaks = []
        for p in range(pr):
            rng = np.random.default_rng(seed_of(kind, shape, ragged, seed, p))
            ml, nl = (m if not ragged else int(self.mlen[p])), (n if not ragged else int(self.nlen[p]))
            z = _z_normal(rng, ml + nl)
            if kind == "gauss":
                a, b = rng.normal(size=(ml, 256)) * 0.25, rng.normal(size=(nl, 256)) * 0.25
                z = rng.normal(size=ml + nl) * 2.0
            elif kind in ("exact", "z", "nan"):
                a, b = _exact_pair(rng, ml, nl)
                if kind == "z":
                    z = np.array([Z_VALUES[(5 * i + 3 * p) % len(Z_VALUES)] for i in range(ml + nl)])
            elif kind == "peaky":
                # background: 40 + multiples of 1/16 within +-3; peaks: one channel each, p q in 20..60, on distinct rows and
                # columns: the first 8 columns, the last 8 valid ones (a ragged tail when the pair is ragged) and the
                # last 8 of the padded width
                a, b = _exact_pair(rng, ml, nl, 128, 48, 0.25)
                a[:, 255], b[:, 255] = 8.0, 5.0   # every similarity 40 up: exp(x) without the max overflows at a peak
                cols = list(dict.fromkeys([j for j in list(range(8)) + list(range(nl - 8, nl)) + list(range(n - 8, n))
                                           if 0 <= j < nl] + [int(j) for j in rng.permutation(nl)]))
                kp = min(ml, len(cols), 120)
                rows = rng.permutation(ml)[:kp]
                for c, (i, j) in enumerate(zip(rows, cols[:kp])):
                    pq = [(6, 10), (4, 5), (5, 6), (6, 7), (5, 9), (4, 7), (5, 8)][c % 7]
                    a[i, 128 + c], b[j, 128 + c] = pq
                    self.peaks.append((p, int(i), int(j)))
            else:  # ramp: x[i][j] = a_i + b_j, a ascending (descending) in i, multiples of 1/32 below 33
                ai = (np.arange(ml) * 1024 // max(ml, 1)) / 32.0
                if kind == "ramp_desc":
                    ai = ai[::-1]
                a, b = np.zeros((ml, 256)), np.zeros((nl, 256))
                a[:, 0], a[:, 1] = ai, 1.0
                b[:, 0], b[:, 1] = 1.0, (np.arange(nl) * 7 % 32) / 32.0
            if pr == 3:  # a term or a partial of the neighbouring pair breaks the bound
                a = a * scales[p]
            v[p, :ml, :256], v[p, m:m + nl, :256] = a, b
            v[p, :ml, ZC], v[p, m:m + nl, ZC] = z[:ml], z[ml:]
            if kind == "nan" and p == pr // 2:
                v[p, ml - 1, :] = np.nan   # the last valid row: alone in its strip, chunk or 8-row batch where m = 32 k + 1
            if ragged:  # no kernel may read a padded row
                v[p, ml:m, :], v[p, m + nl:, :] = np.nan, np.inf
                v[p, ml:m:2, :] = -np.inf
        self.v = v.astype(np.float16)
        assert kind == "nan" or ragged or np.array_equal(self.v.astype(np.float64), v) or kind == "gauss"

    def operands(self):
        """(x float64 [P, m, n] = fp16(m0 . m1^T), z0, z1 float64, dx [P, m, n] (how far the kernel's fp16 similarity
        may lie from x: 0 almost everywhere) or None where x is exact), padded entries 0."""
        pr, m, n = self.shape
        v = self.v.astype(np.float64)
        x, doubt = np.zeros((pr, m, n)), (None if self.x_exact else np.zeros((pr, m, n)))
        z0, z1 = np.zeros((pr, m)), np.zeros((pr, n))
        for p in range(pr):
            ml, nl = (m if self.mlen is None else int(self.mlen[p])), (n if self.nlen is None else int(self.nlen[p]))
            a, b = v[p, :ml, :256], v[p, m:m + nl, :256]
            with np.errstate(invalid="ignore"):
                dot = a @ b.T
                h = dot.astype(np.float16)
            x[p, :ml, :nl] = h.astype(np.float64)
            z0[p, :ml], z1[p, :nl] = v[p, :ml, ZC], v[p, m:m + nl, ZC]
            if self.x_exact:
                ok = (h.astype(np.float64) == dot) | np.isnan(dot)
                assert ok.all(), (self.kind, self.shape, "a similarity is not exact in fp16")
            else:
                tol = 2.0 * 257 * U * (np.abs(a) @ np.abs(b).T)
                lo = (np.nextafter(h, np.float16(-np.inf)).astype(np.float64) + h) / 2.0
                hi = (np.nextafter(h, np.float16(np.inf)).astype(np.float64) + h) / 2.0
                doubt[p, :ml, :nl] = np.where(np.minimum(np.abs(dot - lo), np.abs(dot - hi)) <= tol, tol + ulp16(h), 0.0)
        return x, z0, z1, doubt


def ragged_counts(shape):
    """Per-pair valid counts: m_len cuts a 32-row strip, n_len cuts a lane's 8 columns (n_len % 8 != 0) and, where the
    width allows, leaves whole 32-column blocks (a wave's, and at the S > 1 shapes a whole split's share) in padding."""
    pr, m, n = shape
    mlen = np.array([max(1, m - 1 - (7 * p) % max(1, min(m, 40))) for p in range(pr)], np.int32)
    nlen = np.array([max(1, (n * (3 + p)) // (5 + p) - 3 - p) for p in range(pr)], np.int32)
    nlen = np.where(nlen % 8 == 0, nlen - 1, nlen).clip(1, n).astype(np.int32)
    return mlen, nlen


def sim_inputs(kind, shape, seed=0):
    """The operands of the two lg_log_double_softmax* entry points: (sim [P, m, n], z0 [P, m], z1 [P, n]) float64, every
    value exact in fp16 (and fp32) except `gauss` (fp32 values; the fp16 entry point rounds them first)."""
    pr, m, n = shape
    if kind == "gauss":
        rng = np.random.default_rng(seed_of("sim", kind, shape, seed))
        x = rng.normal(size=shape).astype(np.float32).astype(np.float64)
        if pr == 3:
            x = x * np.array(PAIR_SCALES)[:, None, None]
        return x, (rng.normal(size=(pr, m)) * 2).astype(np.float16).astype(np.float64), \
            (rng.normal(size=(pr, n)) * 2).astype(np.float16).astype(np.float64)
    x, z0, z1, _ = Inputs("exact" if kind == "neg_inf" else kind, shape, False, seed).operands()
    if kind == "neg_inf":  # never a whole row or column
        if m > 128:
            x[:, :128, ::3] = NINF                      # a whole 128-row chunk (two 64-row blocks) above finite rows
        if m >= 2:
            x[:, 0:min(4, m - 1), 0::2] = NINF          # the head of every thread's column walk (rows 0..3 of a chunk)
            x[:, 0, 1::4] = NINF                        # (more of row 0)
        if n >= 2:
            x[:, m - 1, n - max(1, n // 3):] = NINF     # a row's tail
        if m > 2:
            x[:, m // 2, 0] = NINF                      # one in the middle of a walk
        for p in range(pr):  # put a finite entry back into every row and column that lost all of them
            for i in np.nonzero(np.isinf(x[p]).all(1))[0]:
                x[p, i, (i * 5) % n] = float(i % 7)
            for j in np.nonzero(np.isinf(x[p]).all(0))[0]:
                x[p, m - 1 - (j % min(m, 3)), j] = float(j % 5)
        assert not np.isinf(x).all(1).any() and not np.isinf(x).all(2).any()
    return x, z0, z1


# ---- lg_pair_inputs ---------------------------------------------------------------------------------------------------------
def pair_inputs_ref(kp, wr):
    """kp [rows, 2], wr [32, 2] fp16 -> (proj fp16 as float64 [rows, 32], cos, sin float64 of it). proj is the float64
    Wr . kpt (exact: two 22-bit products) rounded once to fp16; `single` says where rounding through fp32 first (the
    kernel's order) gives the same fp16, which the tests assert for their keypoints."""
    kp, wr = np.asarray(kp, np.float16).astype(np.float64), np.asarray(wr, np.float16).astype(np.float64)
    exact = kp @ wr.T
    proj = exact.astype(np.float16)
    single = exact.astype(np.float32).astype(np.float16) == proj
    p64 = proj.astype(np.float64)
    return p64, np.cos(p64), np.sin(p64), single


def f16_candidates(val, err):
    """val float64, err >= 0 -> (lo, hi) fp16: the correctly rounded fp16 of val - err and val + err (equal unless val
    lies within err of an fp16 rounding boundary)."""
    return (val - err).astype(np.float16), (val + err).astype(np.float16)


# ---- the match head's inputs ----------------------------------------------------------------------------------------------
MATCH_SCALES = (1.0, 4.0, 1.0)   # at 1/16 a pair's scores lie within the bound of each other: no row could be called
MARGIN = 16.0                    # every decision clears the bound this many times over
THRESHOLDS = (0.0, 0.1, 1.0)


def match_margins(inp, ths=THRESHOLDS):
    """-> (scores, bound, smallest (gap / bound) over rows and columns, smallest |exp(best) - th| / mscore bound over rows
    and thresholds), in float64."""
    x, z0, z1, doubt = inp.operands()
    pr, m, n = inp.shape
    sc, bd = ref_scores(x, z0, z1, chain_assign(m, n, pr), inp.mlen, inp.nlen, doubt)
    r = ref_matches(sc, 0.0, inp.mlen, inp.nlen)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = min(float(np.nanmin(r["gap0"] / bd.max(2))), float(np.nanmin(r["gap1"] / bd.max(1))))
        best, eb = r["best0"], bd.max(2)
        t = min(float(np.nanmin(np.abs(np.exp(best) - th) / mscore_bound(best, eb))) for th in ths)
    return sc, bd, g, t


_match_cache = {}


def match_inputs(kind, shape, ragged=False):
    """The first seed whose pair(s) leave no row, column or threshold decision within MARGIN bounds of a tie (a choice
    made in float64 on the CPU, before any kernel runs) -> (Inputs, scores, bound)."""
    key = (kind, shape, ragged)
    if key not in _match_cache:
        for seed in range(64):
            inp = Inputs(kind, shape, ragged, seed, MATCH_SCALES)
            sc, bd, g, t = match_margins(inp)
            if g >= MARGIN and t >= MARGIN:
                _match_cache[key] = (inp, sc, bd)
                break
        else:
            raise AssertionError(("no seed separates", key))
    return _match_cache[key]


def pair_inputs_operands(rows):
    """(kp [rows, 2], wr [32, 2]) fp16: keypoints at 0, +-1 (the largest magnitude (xy - centre) / (max(W, H) / 2) takes)
    and uniform in between; Wr of unit spread. The first seed for which rounding the projection through fp32 (the
    kernel's order) equals rounding it once."""
    corners = np.array([(0, 0), (1, 1), (-1, -1), (1, -1), (-1, 1), (0, 1), (-1, 0), (1, 0), (0, -1)], np.float64)
    for seed in range(64):
        rng = np.random.default_rng(seed_of("pair_inputs", rows, seed))
        kp = rng.uniform(-1.0, 1.0, (rows, 2))
        k = min(rows, len(corners))
        kp[:k] = corners[:k]
        kp, wr = kp.astype(np.float16), rng.normal(size=(32, 2)).astype(np.float16)
        if pair_inputs_ref(kp, wr)[3].all():
            return kp, wr
    raise AssertionError("no seed rounds once")
