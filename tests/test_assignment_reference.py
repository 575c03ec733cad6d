"""The bound of tests/assignment_refs.py itself, without a GPU: each kernel's arithmetic restated in numpy fp32 in the
kernel's own order (assign_lse_kernel's lanes, waves and splits with lse_close and the combine; lse_kernel's 4-row
interleave, 128-row chunks and dual_combine_kernel; lse16_kernel's 8-row batches with col_lse_kernel's groups or
combine16_kernel's merge) stays within the bound on every input set and shape, and each plausible wrong kernel misses it:

    mutant                                   shown on (the smallest shape of the table where it changes anything)
    a dropped tail column                    all three kernels: gauss (1, 1, 8) / (1, 3, 5) / (1, 9, 8)
    a dropped last split / chunk / block     assign: gauss (1, 8, 1032) (the first shape whose last split holds columns);
                                             fp32: ramp (1, 129, 65) (the second chunk is the column's largest row);
                                             fp16: ramp (1, 9, 8) (the second 8-row block likewise)
    a partial merged without its rescale     the same three cases
    a logsumexp without the max subtraction  peaky: inf, or an error of the order of the peak
    log(sigmoid(z)) at z = -100              the `z` set: -inf where g(z) = -100
    a row term of the neighbouring pair      the three-pair shapes (pair scales 1/16, 4, 1/16)
    lse_kernel's walk started from -inf      neg_inf (1, 3, 5): NaN down the column where the reference is finite;
                                             nan (1, 3, 5): a NaN alone in its share dropped, finite where the reference is NaN

Not separable under an error bound, and so not tested: a split's partials merged in another order, a shuffle tree of
another shape, the fp16 head's rterm added after cterm: each changes roundings only, by less than the bound grants.

The same file confirms through the workspace-size entry points that the shapes reach the paths the table names, and
asserts the match head's inputs in float64: every row's and column's best entry leads the second by at least 16 bounds
and no exp(score) lies within 16 bounds of a threshold, so no row is left to either side.
"""
import numpy as np
import pytest

import assignment_refs as R

F = np.float32
NINF = F(-np.inf)
FMAX = np.finfo(np.float32).max


def quiet(fn):
    def run(*a, **k):
        with np.errstate(all="ignore"):
            return fn(*a, **k)
    run.__name__ = fn.__name__
    run.__doc__ = fn.__doc__
    return run


# ---- fp32 pieces -----------------------------------------------------------------------------------------------------------
def logsig32(z, naive=False):
    z = np.asarray(z, F)
    if naive:
        return np.log(F(1) / (F(1) + np.exp(-z)))
    return np.minimum(z, F(0)) - np.log1p(np.exp(-np.abs(z)))


def merge32(mx, s, m2, s2, guard=True, rescale=True):
    """lse_merge / lse_close's step on arrays: (mx, s) <- (mx, s) merged with (m2, s2)."""
    gt = m2 > mx
    if rescale:
        s_new = np.where(gt, s * np.exp(np.where(gt, mx - m2, F(0))) + s2, s + s2 * np.exp(np.where(gt, F(0), m2 - mx)))
    else:
        s_new = s + s2
    m_new = np.where(gt, m2, mx)
    if guard:
        skip = m2 == NINF
        return np.where(skip, mx, m_new), np.where(skip, s, s_new)
    return m_new, s_new


def wave_sum32(v):
    """The xor-shuffle tree over the last axis (64 lanes): every lane ends with the same sum; lane 0's is returned."""
    idx = np.arange(64)
    for k in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ k]
    return v[..., 0]


def seq_sum32(e):
    """A sequential fp32 sum over the last axis, from 0."""
    s = np.zeros(e.shape[:-1], F)
    for k in range(e.shape[-1]):
        s = s + e[..., k]
    return s


# ---- assign_lse_kernel + lse_close + assign_combine_kernel ----------------------------------------------------------------------
def assign_partials(xs, noth, s_n, bpw, mutant):
    """xs [own, oth_full] fp32 -> the S (max, sum) partials of every own row: [S][own] each."""
    out = []
    lim = noth - 1 if mutant == "drop_col" else noth
    for sp in range(s_n):
        idx = np.full((8, 2, bpw * 16), -1)
        for w in range(8):
            for t in range(bpw):
                b0 = ((t * s_n + sp) * 8 + w) * 32
                for g in range(4):
                    for hh in range(2):
                        for e in range(4):
                            j = b0 + 8 * g + 4 * hh + e
                            idx[w, hh, t * 16 + 4 * g + e] = j if j < lim else -1
        vals = np.where(idx >= 0, xs[:, idx.clip(0, xs.shape[1] - 1)], NINF)       # [own, 8, 2, 16 BPW]
        mx = np.fmax.reduce(vals.reshape(len(xs), -1), axis=1)                     # (fmaxf drops NaN)
        ref = np.zeros_like(mx) if mutant == "no_max" else mx
        e = np.exp(vals - ref[:, None, None, None])
        lane = seq_sum32(e)                                                        # [own, 8, 2]
        tot = seq_sum32(lane[:, :, 0] + lane[:, :, 1])                             # the 8 waves in order
        tot = np.where(mx == NINF, F(0), tot)
        out.append((ref if mutant == "no_max" else mx, tot))
    return out


def lse_close32(parts, mutant):
    mx, s = np.full_like(parts[0][0], NINF), np.zeros_like(parts[0][1])
    live = [k for k in range(len(parts)) if (parts[k][0] != NINF).any()]
    for k in range(len(parts)):
        if mutant == "drop_last" and k == live[-1]:
            continue
        mx, s = merge32(mx, s, parts[k][0], parts[k][1], True, mutant != "no_rescale")
    return mx + np.log(s)


@quiet
def assign_restated(inp, mutant=None):
    """lg_assign_scores[_lens] on inp in fp32, in the kernels' order -> scores [P, m, n]."""
    pr, m, n = inp.shape
    s_n, bpw, _ = R.assign_plan(m, n, pr)
    x, z0, z1, _ = inp.operands()
    out = np.full((pr, m, n), NINF, F)
    terms = []
    for p in range(pr):
        ml, nl = (m if inp.mlen is None else int(inp.mlen[p])), (n if inp.nlen is None else int(inp.nlen[p]))
        xs = x[p, :ml, :nl].astype(F)
        row = lse_close32(assign_partials(xs, nl, s_n, bpw, mutant), mutant)
        col = lse_close32(assign_partials(np.ascontiguousarray(xs.T), ml, s_n, bpw, None if mutant == "drop_col" else mutant), mutant)
        naive = mutant == "naive_logsig"
        terms.append((xs, logsig32(z0[p, :ml], naive) - row, logsig32(z1[p, :nl], naive) - col))
    for p in range(pr):
        xs, rt, ct = terms[p]
        if mutant == "neighbour":
            q = terms[(p + 1) % pr][1]
            rt = np.resize(q, rt.shape)
        out[p, :xs.shape[0], :xs.shape[1]] = (F(2) * xs + rt[:, None]) + ct[None, :]
    return out


# ---- lse_kernel + dual_combine_kernel (fp32) ---------------------------------------------------------------------------------------
@quiet
def f32_restated(x, z0, z1, mutant=None, guard=True):
    pr, m, n = x.shape
    out = np.zeros((pr, m, n), F)
    rows, cols = [], []
    for p in range(pr):
        xs = x[p].astype(F)
        nn = n - 1 if mutant == "drop_col" else n
        # rows: lane l takes columns l, l + 64, ...; the max, then the sum of exponentials, by the xor tree
        pad = np.full((m, R.cdiv(n, 64) * 64), NINF, F)
        pad[:, :nn] = xs[:, :nn]
        lanes = pad.reshape(m, -1, 64)                                # [m, k, lane]
        mx = np.fmax.reduce(pad, axis=1)
        ref = np.zeros_like(mx) if mutant == "no_max" else mx
        e = np.where(lanes == NINF, F(0), np.exp(lanes - ref[:, None, None]))
        e = np.where(np.isnan(lanes), F(np.nan), e)
        row = ref + np.log(wave_sum32(seq_sum32(np.moveaxis(e, 1, 2))))
        # columns: 128-row chunks, thread r4 walks rows i0 + r4, + 4, ...; merged r4 = 1..3 into 0; chunks in order
        chunks = R.cdiv(m, 128)
        parts = []
        for c in range(chunks):
            i0, i1 = c * 128, min(m, c * 128 + 128)
            th = []
            for r4 in range(4):
                cm, cs = np.full(n, -FMAX if guard else NINF, F), np.zeros(n, F)   # (guard: the walk starts at -FLT_MAX)
                for i in range(i0 + r4, i1, 4):
                    v = xs[i]
                    if mutant == "no_max":
                        cm, cs = np.zeros(n, F), cs + np.exp(v)
                        continue
                    gt = v > cm
                    new = np.where(gt, cs * np.exp(np.where(gt, cm - v, F(0))) + F(1), cs + np.exp(np.where(gt, F(0), v - cm)))
                    if mutant == "no_rescale":
                        new = np.where(gt, cs + F(1), new)
                    cm, cs = np.where(gt, v, cm), new
                th.append((cm, cs))
            cm, cs = th[0]
            for k in range(1, 4):
                cm, cs = merge32(cm, cs, th[k][0], th[k][1], True, mutant != "no_rescale")
            parts.append((cm, cs))
        if mutant == "drop_last":
            parts = parts[:-1]
        cm, cs = np.full(n, NINF, F), np.zeros(n, F)
        for q in parts:
            cm, cs = merge32(cm, cs, q[0], q[1], True, mutant != "no_rescale")
        rows.append(row)
        cols.append(np.log(cs) + cm)
    for p in range(pr):
        naive = mutant == "naive_logsig"
        row = rows[(p + 1) % pr] if mutant == "neighbour" else rows[p]
        out[p] = F(2) * x[p].astype(F) - row[:, None] - cols[p][None, :] + logsig32(z0[p], naive)[:, None] + logsig32(z1[p], naive)[None, :]
    return out


# ---- lse16_kernel (+ col_lse_kernel) + combine16_kernel (fp16 sim) -----------------------------------------------------------------
@quiet
def f16_restated(x, z0, z1, mutant=None):
    pr, m, n = x.shape
    small, cpl = R.f16_plan(m, n, pr)
    w_n = 1 if small else 8
    out = np.zeros((pr, m, n), F)
    rows, cols = [], []
    for p in range(pr):
        xs = x[p].astype(F)
        nn = n - 1 if mutant == "drop_col" else n
        # rows: lane l holds the 8-column groups c * 64 + l, summed over (c, e) in order, then the xor tree
        pad = np.full((m, cpl * 512), NINF, F)
        pad[:, :nn] = xs[:, :nn]
        mx = np.fmax.reduce(pad, axis=1)
        ref = np.zeros_like(mx) if mutant == "no_max" else mx
        e = np.where(pad == NINF, F(0), np.exp(pad - ref[:, None]))
        e = np.where(np.isnan(pad), F(np.nan), e).reshape(m, cpl, 64, 8)
        lane = seq_sum32(np.moveaxis(e, 2, 1).reshape(m, 64, cpl * 8))
        rows.append(ref + np.log(wave_sum32(lane)))
        # columns: one 8-row batch per wave, W waves merged per block, then the blocks
        nb = R.cdiv(m, 8)
        batch = []
        for b in range(nb):
            blk = xs[b * 8:min(m, b * 8 + 8)]
            if mutant == "no_max":
                batch.append((np.zeros(n, F), seq_sum32(np.exp(blk).T)))
                continue
            bm = np.fmax.reduce(blk, axis=0)                                  # (fmaxf drops a NaN ...
            nm = np.maximum(np.where(np.isnan(bm), NINF, bm), -FMAX)          # ... and the max starts at -FLT_MAX)
            t = np.zeros(n, F)
            for r in blk:
                t = t + np.exp(r - nm)                                        # (... the sum keeps it)
            batch.append((nm, t))
        blocks = []
        for b0 in range(0, nb, w_n):
            cm, cs = batch[b0]
            for q in batch[b0 + 1:b0 + w_n]:
                cm, cs = merge32(cm, cs, q[0], q[1], True, mutant != "no_rescale")
            blocks.append((cm, cs))
        if mutant == "drop_last":
            blocks = blocks[:-1]
        if small:   # col_lse_kernel: group g takes blocks g, g + 16, ...; then groups 1..15 into group 0
            groups = []
            for g in range(16):
                cm, cs = np.full(n, NINF, F), np.zeros(n, F)
                for q in blocks[g::16]:
                    cm, cs = merge32(cm, cs, q[0], q[1], True, mutant != "no_rescale")
                groups.append((cm, cs))
            cm, cs = groups[0]
            for q in groups[1:]:
                cm, cs = merge32(cm, cs, q[0], q[1], True, mutant != "no_rescale")
        else:
            cm, cs = np.full(n, NINF, F), np.zeros(n, F)
            for q in blocks:
                cm, cs = merge32(cm, cs, q[0], q[1], True, mutant != "no_rescale")
        cols.append(np.log(cs) + cm)
    for p in range(pr):
        naive = mutant == "naive_logsig"
        row = rows[(p + 1) % pr] if mutant == "neighbour" else rows[p]
        rt = logsig32(z0[p], naive) - row
        ct = logsig32(z1[p], naive) - cols[p]
        out[p] = (F(2) * x[p].astype(F) + rt[:, None]) + ct[None, :]
    return out


def sim16(kind, shape):
    """sim_inputs as the fp16 entry point reads them: the sim rounded to fp16 (only `gauss` changes)."""
    x, z0, z1 = R.sim_inputs(kind, shape)
    return x.astype(np.float16).astype(np.float64), z0, z1


# ---- the bound accepts the stated arithmetic -------------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", (False, True))
@pytest.mark.parametrize("shape", sorted(R.ASSIGN_SHAPES))
def test_bound_accepts_the_assignment_head(shape, ragged):
    pr, m, n = shape
    for kind in R.V_SETS:
        inp = R.Inputs(kind, shape, ragged)
        x, z0, z1, doubt = inp.operands()
        ref, bound = R.ref_scores(x, z0, z1, R.chain_assign(m, n, pr), inp.mlen, inp.nlen, doubt)
        worst, msg = R.compare(assign_restated(inp), ref, bound)
        assert msg is None, (kind, shape, ragged, msg)
        assert np.isnan(ref).any() == (kind == "nan")


@pytest.mark.parametrize("shape", R.F32_SHAPES)
def test_bound_accepts_the_fp32_dual_softmax(shape):
    pr, m, n = shape
    for kind in R.SIM_SETS:
        x, z0, z1 = R.sim_inputs(kind, shape)
        ref, bound = R.ref_scores(x, z0, z1, R.chain_f32(m, n))
        worst, msg = R.compare(f32_restated(x, z0, z1), ref, bound)
        assert msg is None, (kind, shape, msg)
        if kind == "neg_inf" and m > 1:
            assert np.isinf(ref).any() and np.isfinite(ref).any()


@pytest.mark.parametrize("shape", sorted(R.F16_SHAPES))
def test_bound_accepts_the_fp16_dual_softmax(shape):
    pr, m, n = shape
    for kind in R.SIM_SETS:
        x, z0, z1 = sim16(kind, shape)
        ref, bound = R.ref_scores(x, z0, z1, R.chain_f16(m, n, pr))
        worst, msg = R.compare(f16_restated(x, z0, z1), ref, bound)
        assert msg is None, (kind, shape, msg)


# ---- ... and rejects the wrong kernels -----------------------------------------------------------------------------------------------
def _rejects(got, ref, bound, what):
    worst, msg = R.compare(got, ref, bound)
    assert msg is not None and worst > 1.0, (what, "passes the bound", worst)
    return worst


ASSIGN_MUTANTS = (("drop_col", "gauss", (1, 1, 8)), ("drop_last", "gauss", (1, 8, 1032)), ("no_rescale", "gauss", (1, 8, 1032)),
                  ("no_max", "peaky", (1, 1, 8)), ("naive_logsig", "z", (1, 33, 72)), ("neighbour", "exact", (3, 8, 2048)))


@pytest.mark.parametrize("mutant,kind,shape", ASSIGN_MUTANTS)
def test_bound_rejects_a_wrong_assignment_head(mutant, kind, shape):
    pr, m, n = shape
    inp = R.Inputs(kind, shape)
    x, z0, z1, doubt = inp.operands()
    ref, bound = R.ref_scores(x, z0, z1, R.chain_assign(m, n, pr), None, None, doubt)
    assert R.compare(assign_restated(inp), ref, bound)[1] is None
    _rejects(assign_restated(inp, mutant), ref, bound, (mutant, kind, shape))


F32_MUTANTS = (("drop_col", "gauss", (1, 3, 5)), ("drop_last", "ramp", (1, 129, 65)), ("no_rescale", "ramp", (1, 129, 65)),
               ("no_max", "peaky", (1, 3, 5)), ("naive_logsig", "z", (1, 3, 5)), ("neighbour", "exact", (3, 130, 257)))


@pytest.mark.parametrize("mutant,kind,shape", F32_MUTANTS)
def test_bound_rejects_a_wrong_fp32_dual_softmax(mutant, kind, shape):
    x, z0, z1 = R.sim_inputs(kind, shape)
    ref, bound = R.ref_scores(x, z0, z1, R.chain_f32(shape[1], shape[2]))
    assert R.compare(f32_restated(x, z0, z1), ref, bound)[1] is None
    _rejects(f32_restated(x, z0, z1, mutant), ref, bound, (mutant, kind, shape))


def test_bound_rejects_the_column_walk_started_from_inf():
    """lse_kernel's walk as it stood (its running max from -inf, not -FLT_MAX): a thread whose first element is -inf adds
    exp(-inf - -inf) = NaN, and the whole column of scores is NaN where the reference is finite."""
    shape = (1, 3, 5)
    x, z0, z1 = R.sim_inputs("neg_inf", shape)
    ref, bound = R.ref_scores(x, z0, z1, R.chain_f32(3, 5))
    assert np.isfinite(ref).any() and np.isinf(ref).any()
    assert R.compare(f32_restated(x, z0, z1), ref, bound)[1] is None
    got = f32_restated(x, z0, z1, guard=False)
    assert np.isnan(got[np.isfinite(ref)]).any()
    _rejects(got, ref, bound, "the walk from -inf")


def test_bound_rejects_a_dropped_nan():
    """The walk from -inf again, on the `nan` set: the NaN row is alone in its thread's walk, fmaxf and v > mx ignore it,
    the share ends as (-inf, NaN) and lse_merge skips it as empty: finite scores down every column where the reference
    is NaN. (From -FLT_MAX the share is (-FLT_MAX, NaN) and every merge takes it.)"""
    x, z0, z1 = R.sim_inputs("nan", (1, 3, 5))
    ref, bound = R.ref_scores(x, z0, z1, R.chain_f32(3, 5))
    assert np.isnan(ref).all()
    assert R.compare(f32_restated(x, z0, z1), ref, bound)[1] is None
    got = f32_restated(x, z0, z1, guard=False)
    assert np.isfinite(got[0, :2]).all()
    _rejects(got, ref, bound, "a dropped NaN")


F16_MUTANTS = (("drop_col", "gauss", (1, 9, 8)), ("drop_last", "ramp", (1, 9, 8)), ("no_rescale", "ramp", (1, 9, 8)),
               ("no_max", "peaky", (1, 9, 8)), ("naive_logsig", "z", (1, 9, 8)), ("neighbour", "exact", (4, 1025, 8)),
               ("drop_last", "ramp", (4, 1025, 8)))


@pytest.mark.parametrize("mutant,kind,shape", F16_MUTANTS)
def test_bound_rejects_a_wrong_fp16_dual_softmax(mutant, kind, shape):
    x, z0, z1 = sim16(kind, shape)
    ref, bound = R.ref_scores(x, z0, z1, R.chain_f16(shape[1], shape[2], shape[0]))
    assert R.compare(f16_restated(x, z0, z1), ref, bound)[1] is None
    _rejects(f16_restated(x, z0, z1, mutant), ref, bound, (mutant, kind, shape))


# ---- the shapes reach the paths ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def test_shapes_reach_their_paths(lib):
    """The workspace sizes reveal S (lg_assign_scores) and the small / 64-row form (lg_log_double_softmax_f16); BPW, the
    combine's width and CPL follow from the launch rules restated in assignment_refs, which must give the table."""
    for (pr, m, n), (s_n, bpw, w_n) in R.ASSIGN_SHAPES.items():
        assert R.assign_plan(m, n, pr) == (s_n, bpw, w_n), (pr, m, n)
        got = lib.lg_assign_scores_workspace(m, n, pr)
        assert [s for s in (1, 2, 4, 8) if R.assign_workspace(m, n, pr, s) == got] == [s_n], (pr, m, n, got)
        extra = R.up256(pr * R.cdiv(n, 512) * m * 8) + R.up256(pr * R.cdiv(m, 32) * n * 8)
        assert lib.lg_assign_matches_workspace(m, n, pr) == got + extra
    assert {k[:2] for k in ((v[0], v[1]) for v in R.ASSIGN_SHAPES.values())} == {(8, 1), (4, 1), (4, 2), (2, 4), (1, 8)}
    assert {v[2] for v in R.ASSIGN_SHAPES.values()} == {1, 4}
    for (pr, m, n), (small, cpl) in R.F16_SHAPES.items():
        assert R.f16_plan(m, n, pr) == (small, cpl)
        got = lib.lg_log_double_softmax_f16_workspace(m, n, pr)
        assert got == R.f16_workspace(m, n, pr, small) != R.f16_workspace(m, n, pr, not small), (pr, m, n)
    assert {v for v in R.F16_SHAPES.values()} >= {(True, 1), (True, 2), (True, 4), (False, 1)}
    for pr, m, n in R.F32_SHAPES:
        assert lib.lg_log_double_softmax_workspace(m, n, pr) == R.f32_workspace(m, n, pr)
    for shape in R.MATCH_SHAPES:
        assert shape in R.ASSIGN_SHAPES


def test_ragged_counts_cut_what_they_should():
    cut_strip = cut_lane = pad_block = False
    for shape in R.ASSIGN_SHAPES:
        ml, nl = R.ragged_counts(shape)
        assert (1 <= ml).all() and (ml <= shape[1]).all() and (1 <= nl).all() and (nl <= shape[2]).all()
        cut_strip |= bool((ml % 32 != 0).any() and shape[1] > 32)
        cut_lane |= bool((nl % 8 != 0).all()) if shape[2] > 8 else False
        pad_block |= bool((shape[2] - nl >= 64).any())
    assert cut_strip and cut_lane and pad_block


# ---- the match head's inputs: no row left to either side ------------------------------------------------------------------------------
@pytest.mark.parametrize("ragged", (False, True))
@pytest.mark.parametrize("kind", ("exact", "peaky"))
@pytest.mark.parametrize("shape", R.MATCH_SHAPES)
def test_match_inputs_are_separated(shape, kind, ragged):
    inp, sc, bd = R.match_inputs(kind, shape, ragged)
    assert inp.x_exact
    _, _, gap, thr = R.match_margins(inp)
    assert gap >= R.MARGIN and thr >= R.MARGIN, (gap, thr)
    r = R.ref_matches(sc, 0.1, inp.mlen, inp.nlen)
    kept, mutual = int(r["counts"].sum()), int((r["scores0"] > 0).sum())
    assert mutual >= 1
    if shape[1] >= 8:   # matches on both sides of the threshold
        assert 0 < kept < mutual
    assert int(R.ref_matches(sc, 0.0, inp.mlen, inp.nlen)["counts"].sum()) == mutual
    assert int(R.ref_matches(sc, 1.0, inp.mlen, inp.nlen)["counts"].sum()) == 0
    if kind == "peaky":  # every peak is its row's and its column's best entry
        for p, i, j in inp.peaks:
            assert sc[p, i].argmax() == j and sc[p, :, j].argmax() == i


def test_reference_filter_is_the_packages_filter():
    """ref_matches against lightglue_amd.matches.filter_matches_dense on the same float64 scores (ties included)."""
    torch = pytest.importorskip("torch")
    from lightglue_amd.matches import filter_matches_dense

    inp, sc, _ = R.match_inputs("exact", (1, 33, 72))
    sc = sc.copy()
    sc[0, 5, :] = sc[0, 5].max()          # a row of ties: the lowest column
    sc[0, :, 9] = sc[0, :, 9].max()       # a column of ties: the lowest row
    for th in R.THRESHOLDS:
        want, got = R.ref_matches(sc, th), filter_matches_dense(torch.from_numpy(sc), th)
        for f in ("matches0", "matches1", "matches", "counts"):
            assert (getattr(got, f).numpy() == want[f]).all(), (th, f)
        assert np.allclose(got.scores0.numpy(), want["scores0"], rtol=1e-12, atol=0)
        assert np.allclose(got.match_scores.numpy(), want["match_scores"], rtol=1e-12, atol=0)


# ---- lg_pair_inputs' reference --------------------------------------------------------------------------------------------------------
def test_pair_inputs_keypoints_round_once():
    """The kernel rounds Wr . kpt to fp32, then fp16; the reference rounds the exact float64 value once. For the tests'
    keypoints and weights the two agree in every element, so the projection itself is not in doubt."""
    kp, wr = R.pair_inputs_operands(2 * (9 + 7) * 3)
    proj, c, s, single = R.pair_inputs_ref(kp, wr)
    assert single.all()
    assert (np.abs(kp.astype(np.float64)).max() == 1.0) and (kp == 0).any()
