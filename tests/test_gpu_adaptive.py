"""Adaptive depth and width on the MI355X: lg_token_scores, lg_compact_rows, lg_matches_scatter
(include/lightglue_glue.h) and LightGlueMatcher.match_adaptive on the fp16 fast path.

Bounds. conf / mtch against float64 numpy on the same fp16 inputs: the products of two fp16 values are
exact in fp32, so the logit's error is that of summing 256 terms (and the bias) in fp32 in some order,
at most 256 * 2^-24 * (sum_k |w_k x_k| + |b|), doubled because the kernel's order (8 sequential FMAs a
lane, then a 5-level tree) is not numpy's; the sigmoid's slope is at most 1/4, and evaluating
1 / (1 + exp(-z)) in fp32 adds one relative rounding each for the exponential (~1 ulp), the sum and the
quotient on a value <= 1: 8 * 2^-24 covers them. Everything else (keep flags from the kernel's own conf
/ mtch bits, stats, compaction, scatter, reruns, poisoned padding) is exact.

The matcher's knobs were chosen beforehand with adaptive_reference on the CPU (fp32, the oracle
attention) on exactly this model and these pairs, seeded_confidence_state_dict(54, 9):
  depth only (0.4, -1): the confident shares per pair are <= 0.21 up to layer 4 and 0.88 / 0.70 / 0.85 at
    layer 5, so the forward stops after 6 layers (68 / 50 / 33 matches from log_assignment[5]);
  width only (-1, 0.98): layer 2 drops a few rows (150 x 136 -> 145 x 128) and layer 6, whose matchability
    has its median near 0.02, about 59 % (145 -> 60 rows of pair 0's image 0); 22 / 14 / 8 matches;
  both (0.4, 0.5): layer 2 prunes its confident rows of low matchability (150 -> 119 rows, 21 %), the
    forward stops after 6 layers; 53 / 34 / 23 matches.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

FIELDS = ("matches0", "matches1", "scores0", "scores1", "matches", "match_scores", "counts")
SIZES = [(150, 136), (120, 97), (64, 120)]   # tests/test_gpu_ragged.py _matcher_case
SWEEP_RECALL = 0.9                           # tests/test_matcher.py
L = 9
CONF_SEED = 54
DEPTH_ONLY, WIDTH_ONLY, BOTH = (0.4, -1.0), (-1.0, 0.98), (0.4, 0.5)
RAGGED = (3, 150, 136, ([150, 120, 33], [136, 97, 120]))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _lens_dev(lens, dev):
    return None if lens is None else tuple(torch.tensor(v, dtype=torch.int32, device=dev) for v in lens)


# =========================================================================================
# lg_token_scores
# =========================================================================================
TOKEN_CASES = {
    "3x150x136 ragged": RAGGED,
    "3x150x136": (3, 150, 136, None),
    "1x2048x2048": (1, 2048, 2048, None),
    "2x1x8": (2, 1, 8, None),
}
T_CONF = float(np.float32(0.8 + 0.1 * np.exp(-4.0 * 3 / 9)))


@functools.lru_cache(maxsize=None)
def _token_inputs(name):
    """(x fp16 [P*(m+n), 256], w_tok, b_tok, w_match, b_match as fp16 numpy): logits of std ~2."""
    from lightglue_amd import synth

    pr, m, n, _ = TOKEN_CASES[name]
    seed = 900 + sorted(TOKEN_CASES).index(name)
    x = synth.round_f16(2.0 * synth.normal(seed, (pr * (m + n), 256))).astype(np.float16)
    wt = synth.round_f16(synth.normal(seed + 50, (256,), 1.0 / 16)).astype(np.float16)
    wm = synth.round_f16(synth.normal(seed + 60, (256,), 1.0 / 16)).astype(np.float16)
    return x, wt, np.float16([0.25]), wm, np.float16([-0.125])


def _token_run(name, flags, t_keep, dev, x=None):
    from lightglue_amd import matcher as mt

    pr, m, n, lens = TOKEN_CASES[name]
    xs, wt, bt, wm, bm = _token_inputs(name)
    x = torch.from_numpy(xs).to(dev) if x is None else x
    g = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    out = mt._Hip.token_scores(x[None], m, n, pr, _lens_dev(lens, dev), g(wt), g(bt), g(wm), g(bm), T_CONF, t_keep, flags)
    torch.cuda.synchronize()
    return out


def _valid_mask(pr, m, n, lens):
    v = np.zeros((pr, m + n), dtype=bool)
    for p in range(pr):
        a, b = (lens[0][p], lens[1][p]) if lens is not None else (m, n)
        v[p, :a] = v[p, m:m + b] = True
    return v


def _keep_rule(conf, mtch, valid, m, flags, t_keep):
    """The header's rule applied to the kernel's own conf / mtch (numpy fp32), min-one included."""
    pr = conf.shape[0]
    keep = np.zeros(conf.shape, dtype=np.uint8)
    for p in range(pr):
        for lo, hi, bit in ((0, m, 2), (m, conf.shape[1], 4)):
            v = valid[p, lo:hi]
            cnt = int(v.sum())
            if not flags & bit:
                k = v.copy()
            else:
                k = v & ((mtch[p, lo:hi] > np.float32(t_keep)) | (bool(flags & 1) & (conf[p, lo:hi] <= np.float32(T_CONF))))
                if not k.any():
                    k[int(np.argmax(mtch[p, lo:lo + cnt]))] = True   # (numpy: the first of equal maxima)
            keep[p, lo:hi] = k
    return keep


@pytest.mark.parametrize("name", sorted(TOKEN_CASES))
def test_token_scores(dev, name):
    pr, m, n, lens = TOKEN_CASES[name]
    xs, wt, bt, wm, bm = _token_inputs(name)
    valid = _valid_mask(pr, m, n, lens)
    x64 = xs.astype(np.float64).reshape(pr, m + n, 256)
    worst = 0.0
    for flags, t_keep in ((7, 0.5), (6, 0.5), (1, 0.5), (2, 0.7), (4, 0.3), (6, 1.0), (7, 1.0), (0, 0.5)):
        conf, mtch, keep, stats = (t.cpu().numpy() for t in _token_run(name, flags, t_keep, dev))
        for got, w, b in ((conf, wt, bt), (mtch, wm, bm)):
            z = x64 @ w.astype(np.float64) + float(b[0])
            ref = 1.0 / (1.0 + np.exp(-z))
            mag = np.abs(x64 * w.astype(np.float64)).sum(-1) + abs(float(b[0]))
            bound = 0.25 * 2.0 * 256 * 2.0 ** -24 * mag + 8 * 2.0 ** -24
            err = np.abs(got.astype(np.float64) - ref)
            worst = max(worst, float((err / bound)[valid].max()))
            assert (err[valid] <= bound[valid]).all(), (name, flags, float((err / bound)[valid].max()))
            assert (got[~valid] == 0).all()
        want = _keep_rule(conf, mtch, valid, m, flags, t_keep)
        assert np.array_equal(keep, want), (name, flags, t_keep, int((keep != want).sum()))
        unc = ((conf < np.float32(T_CONF)) & valid).sum(1)
        assert np.array_equal(stats, np.stack([keep[:, :m].sum(1), keep[:, m:].sum(1), unc, valid.sum(1)], 1)), (name, flags)
        if t_keep == 1.0 and flags == 6:   # nothing passes: the min-one rule in every segment
            assert (stats[:, :2] == 1).all()
    print(f"lg_token_scores {name}: max error / bound {worst:.3f}")


def test_token_scores_min_one_tie_break(dev):
    """Identical rows have identical scores: the kept row of an emptied segment is its first."""
    name = "2x1x8"
    pr, m, n, _ = TOKEN_CASES[name]
    xs = _token_inputs(name)[0]
    x = torch.from_numpy(np.tile(xs[:1], (pr * (m + n), 1))).to(dev)
    conf, mtch, keep, stats = (t.cpu().numpy() for t in _token_run(name, 6, 1.0, dev, x=x))
    assert len(np.unique(mtch)) == 1
    want = np.zeros((pr, m + n), dtype=np.uint8)
    want[:, 0] = want[:, m] = 1
    assert np.array_equal(keep, want) and (stats[:, :2] == 1).all()


def test_token_scores_poison_and_rerun(dev):
    name = "3x150x136 ragged"
    pr, m, n, lens = TOKEN_CASES[name]
    a = _token_run(name, 7, 0.5, dev)
    b = _token_run(name, 7, 0.5, dev)
    x = torch.from_numpy(_token_inputs(name)[0]).to(dev).view(pr, m + n, 256).clone()
    for p in range(pr):
        x[p, lens[0][p]:m] = float("nan")
        x[p, m + lens[1][p]:] = float("nan")
    c = _token_run(name, 7, 0.5, dev, x=x.view(pr * (m + n), 256))
    for u, v, w in zip(a, b, c):
        assert _same_bits(u, v) and _same_bits(u, w)


# =========================================================================================
# lg_compact_rows
# =========================================================================================
def _flag_patterns(pr, m, n, lens, seed):
    rng = np.random.RandomState(seed)
    valid = _valid_mask(pr, m, n, lens)
    pats = {"all": np.ones((pr, m + n), dtype=np.uint8), "alternating": (np.arange(m + n)[None] % 2 == 0).repeat(pr, 0),
            "random 30 %": rng.rand(pr, m + n) < 0.3}
    first, last = np.zeros((pr, m + n), dtype=np.uint8), np.zeros((pr, m + n), dtype=np.uint8)
    for p in range(pr):
        a, b = (lens[0][p], lens[1][p]) if lens is not None else (m, n)
        first[p, 0] = first[p, m] = 1
        last[p, a - 1] = last[p, m + b - 1] = 1
    pats["first only"], pats["last only"] = first, last
    # (flags past a pair's count are set too: the kernel must not read them)
    return {k: np.where(valid, v, 1).astype(np.uint8) for k, v in pats.items()}, valid


def _compact_check(dev, pr, m, n, lens, seed, with_maps):
    from lightglue_amd import matcher as mt

    rng = np.random.RandomState(seed)
    rows = pr * (m + n)
    def bits(c):   # any fp16 bit pattern, NaN and Inf included: the copies are bitwise
        return torch.from_numpy(rng.randint(-32768, 32767, size=(1, rows, c)).astype(np.int16)).to(dev).view(torch.float16)

    x, cos, sin = bits(256), bits(64), bits(64)
    pats, valid = _flag_patterns(pr, m, n, lens, seed)
    ind = (None, None)
    if with_maps:   # running maps of an earlier compaction: increasing original indices in [0, 3 m)
        ind = tuple(torch.from_numpy((3 * np.arange(k)[None] + rng.randint(0, 3, size=(pr, k))).astype(np.int32)).to(dev)
                    for k in (m, n))
    for pname, flags in pats.items():
        k0 = [int((flags[p, :m] & valid[p, :m]).sum()) for p in range(pr)]
        k1 = [int((flags[p, m:] & valid[p, m:]).sum()) for p in range(pr)]
        mo, no = mt.compact_dims(k0, k1)
        no = min(no, n)
        prune = tuple(torch.zeros((pr, 3 * k), dtype=torch.int32, device=dev) for k in (m, n))
        xo, co, so, (i0, i1), (l0, l1) = mt._Hip.compact_rows(x, cos, sin, torch.from_numpy(flags).to(dev), ind, m, n, pr,
                                                              _lens_dev(lens, dev), mo, no, prune, 5)
        torch.cuda.synchronize()
        assert l0.tolist() == k0 and l1.tolist() == k1, (pname, l0.tolist(), k0)
        if pname != "all":
            assert mo < m
        for p in range(pr):
            for img, (lo, dim, dimo, kept, io, imap, pru) in enumerate(((0, m, mo, k0[p], i0, ind[0], prune[0]),
                                                                        (m, n, no, k1[p], i1, ind[1], prune[1]))):
                sel = np.nonzero(flags[p, lo:lo + dim] & valid[p, lo:lo + dim])[0]
                idx = torch.from_numpy(sel).to(dev)
                src, dst = p * (m + n) + lo, p * (mo + no) + (0 if img == 0 else mo)
                for t, o in ((x, xo), (cos, co), (sin, so)):
                    want = t[0, src:src + dim].index_select(0, idx)
                    assert torch.equal(_bits(o[0, dst:dst + kept]), _bits(want)), (pname, p, img)
                orig = imap[p].long() if imap is not None else torch.arange(dim, device=dev)
                assert torch.equal(io[p, :kept].long(), orig[idx]), (pname, p, img)
                want = torch.zeros_like(pru[p])
                gone = np.nonzero(valid[p, lo:lo + dim] & ~flags[p, lo:lo + dim].astype(bool))[0]
                want[orig[torch.from_numpy(gone).to(dev)]] = 5
                assert torch.equal(pru[p], want), (pname, p, img)


def test_compact_rows_ragged(dev):
    pr, m, n, lens = RAGGED
    _compact_check(dev, pr, m, n, lens, 11, with_maps=True)
    _compact_check(dev, pr, m, n, None, 12, with_maps=False)


def test_compact_rows_2048(dev):
    _compact_check(dev, 1, 2048, 2048, None, 13, with_maps=False)
    _compact_check(dev, 1, 2048, 2048, ([2047], [1985]), 14, with_maps=True)


# =========================================================================================
# lg_matches_scatter
# =========================================================================================
def test_matches_scatter(dev):
    """Exact against scatter_matches_reference on a hand-built survivors' MatchResult: 3 pairs, layout
    40 x 48 of 150 x 136, rows pruned at different layers (prune pre-filled as lg_compact_rows leaves it)."""
    from lightglue_amd import matcher as mt

    rng = np.random.RandomState(5)
    pr, m, n, mc, nc, stop = 3, 150, 136, 40, 48, 7
    orig0, orig1 = [150, 120, 64], [136, 97, 120]
    len0, len1 = [40, 33, 17], [48, 40, 9]
    kc = min(mc, nc)
    r = dict(m0=np.full((pr, mc), -1, np.int32), m1=np.full((pr, nc), -1, np.int32), s0=np.zeros((pr, mc), np.float32),
             s1=np.zeros((pr, nc), np.float32), mt=np.full((pr, kc, 2), -1, np.int32), ms=np.zeros((pr, kc), np.float32),
             cnt=np.zeros((pr,), np.int32))
    ind0, ind1 = np.zeros((pr, mc), np.int32), np.zeros((pr, nc), np.int32)
    prune0, prune1 = np.zeros((pr, m), np.int32), np.zeros((pr, n), np.int32)
    for p in range(pr):
        for ind, ln, orig, prune in ((ind0, len0[p], orig0[p], prune0), (ind1, len1[p], orig1[p], prune1)):
            live = np.sort(rng.permutation(orig)[:ln])
            ind[p, :ln] = live
            ind[p, ln:] = 10 ** 6            # (past the count: never read)
            prune[p, :orig] = rng.randint(1, stop, size=orig)   # dropped at layers 1 .. stop - 1
        k = min(len0[p], len1[p]) // 2
        rows, cols = np.sort(rng.permutation(len0[p])[:k]), rng.permutation(len1[p])[:k]
        sc = rng.rand(k).astype(np.float32) + 0.1
        r["m0"][p, rows], r["m1"][p, cols], r["s0"][p, rows], r["s1"][p, cols] = cols, rows, sc, sc
        r["s0"][p, (rows[0] + 1) % len0[p]] += 0.05   # (a mutual score below the threshold keeps its value with -1)
        r["mt"][p, :k, 0], r["mt"][p, :k, 1], r["ms"][p, :k], r["cnt"][p] = rows, cols, sc, k
    g = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    res = mt.MatchResult(*(g(r[k]) for k in ("m0", "m1", "s0", "s1", "mt", "ms", "cnt")))
    lens = _lens_dev((len0, len1), dev)
    got_p, want_p = (g(prune0), g(prune1)), (g(prune0), g(prune1))
    got = mt._Hip.matches_scatter(res, (g(ind0), g(ind1)), lens, m, n, stop, got_p)
    torch.cuda.synchronize()
    want = mt.scatter_matches_reference(res, g(ind0), g(ind1), len0, len1, m, n, stop, *want_p)
    for f in FIELDS:
        assert _same_bits(getattr(got, f), getattr(want, f)), f
    assert torch.equal(got_p[0], want_p[0]) and torch.equal(got_p[1], want_p[1])
    assert int((got_p[0] == stop).sum()) == sum(len0) and int((want.matches0 >= 0).sum()) == int(r["cnt"].sum())
    # identity maps (nothing was ever compacted) and full counts: the input itself, padded
    full = mt.MatchResult(*(g(r[k]) for k in ("m0", "m1", "s0", "s1", "mt", "ms", "cnt")))
    same = mt._Hip.matches_scatter(full, None, lens, mc, nc, stop, None)
    ident = tuple(torch.arange(k, device=dev, dtype=torch.int32).repeat(pr, 1) for k in (mc, nc))
    want = mt.scatter_matches_reference(full, *ident, len0, len1, mc, nc)
    for f in FIELDS:
        assert _same_bits(getattr(same, f), getattr(want, f)), f


# =========================================================================================
# the matcher, 9 layers, fp16
# =========================================================================================
def _match_set(m):
    return {(int(a), int(b)) for a, b in np.asarray(m)}


@functools.lru_cache(maxsize=None)
def _inputs():
    """The padded batch [3, 150 | 136, .] of tests/test_gpu_ragged.py's _matcher_case, and the counts."""
    from lightglue_amd import matcher

    dev = torch.device("cuda:0")
    pairs = [tuple(t.to(dev, torch.float16) for t in matcher.synthetic_pair(300 + i, m, n, overlap=min(m, n) // 2))
             for i, (m, n) in enumerate(SIZES)]
    m, n = max(a for a, _ in SIZES), max(b for _, b in SIZES)
    batch = []
    for j, size in enumerate((m, n, m, n)):
        t = torch.zeros((len(pairs), size, pairs[0][j].shape[-1]), dtype=torch.float16, device=dev)
        for p, pair in enumerate(pairs):
            t[p, :pair[j].shape[1]] = pair[j][0]
        batch.append(t)
    return tuple(batch), [a for a, _ in SIZES], [b for _, b in SIZES]


@functools.lru_cache(maxsize=None)
def _model(knobs, glue="hip"):
    from lightglue_amd import matcher

    model = matcher.LightGlueMatcher(n_layers=L, glue=glue, depth_confidence=knobs[0], width_confidence=knobs[1]).eval()
    sd = matcher.seeded_state_dict(7, L)
    if model.adaptive:
        sd.update(matcher.seeded_confidence_state_dict(CONF_SEED, L))
    model.load_state_dict(sd, strict=True)
    return model.to(torch.device("cuda:0"), torch.float16)


@functools.lru_cache(maxsize=None)
def _adaptive_run(knobs):
    """(AdaptiveResult, trace) of match_adaptive on the fast path: computed once per knob pair, read-only."""
    batch, c0, c1 = _inputs()
    trace = []
    with torch.no_grad():
        res = _model(knobs).match_adaptive(*batch, counts0=c0, counts1=c1, trace=trace)
    torch.cuda.synchronize()
    return res, trace


def _equal_adaptive(a, b, what):
    assert a.stop == b.stop, what
    for f in FIELDS:
        assert _same_bits(getattr(a.result, f), getattr(b.result, f)), (what, f)
    assert torch.equal(a.prune0, b.prune0) and torch.equal(a.prune1, b.prune1), what


def test_matcher_knobs_off_is_match_batch(dev):
    batch, c0, c1 = _inputs()
    model = _model((-1.0, -1.0))
    assert not hasattr(model, "token_confidence")
    with torch.no_grad():
        want = model.match_batch(*batch, counts0=c0, counts1=c1)
        got = model.match_adaptive(*batch, counts0=c0, counts1=c1)
    torch.cuda.synchronize()
    assert got.stop == L and got.prune0 is None and got.prune1 is None and int(want.counts.min()) >= 1
    for f in FIELDS:
        assert _same_bits(getattr(got.result, f), getattr(want, f)), f


def test_matcher_full_depth_loop_is_match_batch(dev):
    """depth_confidence = 1.0 with width off: the exit (1 - unconfident / valid > 1.0) never holds and
    nothing is pruned, so match_adaptive's own loop runs all L layers on the fast path; it launches the
    layer step match_batch launches, so the bits are match_batch's, whichever projections that one folds."""
    batch, c0, c1 = _inputs()
    model = _model((1.0, -1.0))
    trace = []
    with torch.no_grad():
        got = model.match_adaptive(*batch, counts0=c0, counts1=c1, trace=trace)
        want = model.match_batch(*batch, counts0=c0, counts1=c1)
        model.chain_kinds = "sh"
        try:
            want_sh = model.match_batch(*batch, counts0=c0, counts1=c1)
        finally:
            del model.chain_kinds
    torch.cuda.synchronize()
    assert model.adaptive and got.stop == L and len(trace) == L - 1 and all(e["stop"] is False for e in trace)
    for prune, counts in ((got.prune0, c0), (got.prune1, c1)):
        valid = torch.arange(prune.shape[1], device=dev)[None] < torch.tensor(counts, device=dev)[:, None]
        assert torch.equal(prune, torch.where(valid, L, 0).to(torch.int32))
    assert int(want.counts.min()) >= 1
    for f in FIELDS:
        assert _same_bits(getattr(got.result, f), getattr(want, f)), f
        assert _same_bits(getattr(got.result, f), getattr(want_sh, f)), (f, "sh")


def _check_decisions(knobs, res, trace, c0, c1):
    """The recorded decisions are the rules applied to the recorded stats."""
    from lightglue_amd.matcher import adaptive_thresholds, compact_dims, exit_passes

    depth, width = knobs[0] > 0, knobs[1] > 0
    thr = adaptive_thresholds(L)
    dims, lens = (max(c0), max(c1)), (list(c0), list(c1))
    assert [e["layer"] for e in trace] == list(range(len(trace)))
    for e in trace:
        st = e["stats"]
        assert e["threshold"] == thr[e["layer"]]
        assert [s[3] for s in st] == [a + b for a, b in zip(*lens)]
        assert e["stop"] == (depth and all(exit_passes(s[2], s[3], knobs[0]) for s in st))
        if not width:
            assert [s[:2] for s in st] == [list(t) for t in zip(*lens)]
        if not e["stop"] and any(s[0] + s[1] < s[3] for s in st):
            dims, lens = compact_dims([s[0] for s in st], [s[1] for s in st]), ([s[0] for s in st], [s[1] for s in st])
        assert e["dims"] == dims
        assert [len(k) for k in e["kept0"]] == lens[0] and [len(k) for k in e["kept1"]] == lens[1]
        for k in e["kept0"] + e["kept1"]:
            assert bool((k[1:] > k[:-1]).all())                  # stable: original indices stay ascending
    assert res.stop == (trace[-1]["layer"] + 1 if trace[-1]["stop"] else L)
    assert len(trace) == (res.stop if trace[-1]["stop"] else L - 1)
    return lens


def _lost_shares(trace, c0, c1):
    out, prev = [], (list(c0), list(c1))
    for e in trace:
        if e["stop"]:
            break
        cur = ([len(k) for k in e["kept0"]], [len(k) for k in e["kept1"]])
        out += [1 - c / p for img in (0, 1) for c, p in zip(cur[img], prev[img])]
        prev = cur
    return out


@pytest.mark.parametrize("case", ["width", "depth", "both"])
def test_matcher_adaptive(dev, case):
    from lightglue_amd import matcher

    knobs = dict(width=WIDTH_ONLY, depth=DEPTH_ONLY, both=BOTH)[case]
    batch, c0, c1 = _inputs()
    res, trace = _adaptive_run(knobs)
    lens = _check_decisions(knobs, res, trace, c0, c1)
    lost = _lost_shares(trace, c0, c1)
    print(f"match_adaptive {case}: stop {res.stop}, surviving rows {lens}, largest share of a segment lost at one layer "
          f"{max(lost, default=0.0):.2f}, matches {res.result.counts.tolist()}")
    # the run is not trivial
    if case in ("width", "both"):
        assert any(0.1 <= x <= 0.9 for x in lost), lost
    if case in ("depth", "both"):
        assert 2 <= res.stop <= L - 1
    if case == "depth":
        assert not any(lost) and lens == (c0, c1)
    # the framework path, following the recorded decisions
    with torch.no_grad():
        ref = matcher.adaptive_reference(_model(knobs, "torch"), *batch, counts0=c0, counts1=c1, decisions=trace)
    torch.cuda.synchronize()
    assert ref.stop == res.stop and torch.equal(ref.prune0, res.prune0) and torch.equal(ref.prune1, res.prune1)
    for p, (a, b) in enumerate(zip(c0, c1)):
        want = _match_set(ref.result.matches[p, :int(ref.result.counts[p])].cpu().numpy())
        mine = _match_set(res.result.matches[p, :int(res.result.counts[p])].cpu().numpy())
        print(f"  pair {p}: {len(mine)} matches, {len(mine & want)} of the framework path's {len(want)}")
        assert len(want) >= 1 and len(mine & want) >= SWEEP_RECALL * len(want)
        # original index space: pruned and padded rows hold -1 / 0, the rest is mutually consistent
        live0, live1 = trace[-1]["kept0"][p].to(dev), trace[-1]["kept1"][p].to(dev)
        dead0 = torch.ones(batch[0].shape[1], dtype=torch.bool, device=dev)
        dead1 = torch.ones(batch[1].shape[1], dtype=torch.bool, device=dev)
        dead0[live0], dead1[live1] = False, False
        r = res.result
        assert (r.matches0[p][dead0] == -1).all() and (r.scores0[p][dead0] == 0).all()
        assert (r.matches1[p][dead1] == -1).all() and (r.scores1[p][dead1] == 0).all()
        i = torch.nonzero(r.matches0[p] >= 0)[:, 0]
        assert torch.equal(r.matches1[p][r.matches0[p][i].long()].long(), i) and not dead1[r.matches0[p][i].long()].any()
        assert torch.equal(r.matches[p, :len(i), 0].long(), i) and len(i) == int(r.counts[p])
        assert (res.prune0[p][live0] == res.stop).all() and (res.prune0[p, :a] >= 1).all() and (res.prune0[p, a:] == 0).all()
        assert (res.prune1[p][live1] == res.stop).all() and (res.prune1[p, :b] >= 1).all() and (res.prune1[p, b:] == 0).all()
        assert int(res.prune0[p].max()) <= res.stop and int(res.prune1[p].max()) <= res.stop


@pytest.mark.parametrize("case", ["width", "depth", "both"])
def test_matcher_adaptive_rerun_and_poison(dev, case):
    knobs = dict(width=WIDTH_ONLY, depth=DEPTH_ONLY, both=BOTH)[case]
    batch, c0, c1 = _inputs()
    res, _ = _adaptive_run(knobs)
    model = _model(knobs)
    bad = [t.clone() for t in batch]
    for p, (a, b) in enumerate(SIZES):
        bad[0][p, a:] = bad[2][p, a:] = float("nan")
        bad[1][p, b:] = bad[3][p, b:] = float("nan")
    with torch.no_grad():
        again = model.match_adaptive(*batch, counts0=c0, counts1=c1)
        dev_counts = model.match_adaptive(*batch, counts0=torch.tensor(c0, dtype=torch.int32, device=dev),
                                          counts1=torch.tensor(c1, dtype=torch.int32, device=dev))
        poisoned = model.match_adaptive(*bad, counts0=c0, counts1=c1)
    torch.cuda.synchronize()
    _equal_adaptive(again, res, "same input twice")
    _equal_adaptive(dev_counts, res, "counts on the device")
    _equal_adaptive(poisoned, res, "poisoned padding")
