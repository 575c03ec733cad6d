"""lg_assign_matches on the MI355X (the match head: mutual nearest neighbours, scores and the compacted
list of all P pairs without the fp32 scores tensor) against the semantics of include/lightglue_glue.h
applied in numpy to the scores lg_assign_scores writes for the same input, and
LightGlueMatcher.match_batch end to end.

Expected values: `_Hip.assign_scores` on the same v, copied to the host; numpy's argmax takes the
lowest index among equals, the rule the kernel states. Indices, counts, the -1 / 0 padding and which
score entries are zero must be exactly equal. Non-zero scores: within relative 2^-22 (4 + |s|) of
np.exp(s) in fp32 — a few fp32 ulps plus what an exponential adds by rounding s log2(e), which grows
with |s|. A row whose exp(s) lies within that distance of the threshold may fall on either side; such
rows take the kernel's side, and there may be at most 0.5 % of them per case (rounded down: none for
the small cases).
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 8), (1, 8, 8), (2, 33, 72), (1, 70, 520), (1, 520, 72), (3, 300, 296), (1, 2048, 2048)]
FIELDS = ("matches0", "matches1", "scores0", "scores1", "matches", "match_scores", "counts")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _pair_rows(sd, m, n):
    """One pair's v [m + n, 384] (fp32 values, before the fp16 rounding)."""
    from lightglue_amd import synth

    d0 = synth.normal(sd * 8 + 0, (m, 256))
    d1 = synth.normal(sd * 8 + 1, (n, 256))
    d0 = d0 / np.linalg.norm(d0, axis=-1, keepdims=True)
    ov = min(m, n) // 2
    if ov:
        src = np.argsort(synth.uniform24(sd * 8 + 2, m), kind="stable")[:ov]
        d1[:ov] = d0[src] + 0.2 * synth.normal(sd * 8 + 3, (ov, 256)) / 16
    d1 = d1 / np.linalg.norm(d1, axis=-1, keepdims=True)
    v = np.zeros((m + n, 384), dtype=np.float32)
    v[:m, :256], v[m:, :256] = 4 * d0, 4 * d1
    v[:, 256] = synth.normal(sd * 8 + 4, (m + n,), 2.0)
    return v


@functools.lru_cache(maxsize=None)
def _case(pairs, m, n):
    """(v [P, m + n, 384] fp16 on the GPU, the scores lg_assign_scores gives for it on the host):
    computed once per shape and shared (read-only) by the tests below."""
    from lightglue_amd import matcher as mt

    dev = torch.device("cuda:0")
    v = torch.from_numpy(np.stack([_pair_rows(7 * 16 + p, m, n) for p in range(pairs)])).to(dev, torch.float16)
    scores = mt._Hip.assign_scores(v, m, 256).cpu().numpy()
    scores.setflags(write=False)
    return v, scores


def _rel(s):
    return 2.0 ** -22 * (4.0 + np.abs(s.astype(np.float64)))


def _check(got, scores, th, label):
    """got: MatchResult on the GPU; scores [P, m, n] fp32 (numpy)."""
    pr, m, n = scores.shape
    k = min(m, n)
    g = {f: getattr(got, f).cpu().numpy() for f in FIELDS}
    assert g["matches0"].shape == (pr, m) and g["matches1"].shape == (pr, n) and g["matches"].shape == (pr, k, 2)
    assert g["scores0"].shape == (pr, m) and g["scores1"].shape == (pr, n) and g["match_scores"].shape == (pr, k)
    assert g["counts"].shape == (pr,)
    assert all(g[f].dtype == np.int32 for f in ("matches0", "matches1", "matches", "counts"))
    j0, i1 = scores.argmax(2), scores.argmax(1)              # lowest index among equals
    s = np.take_along_axis(scores, j0[..., None], 2)[..., 0]
    e = np.exp(s)                                            # fp32
    rows, cols = np.arange(m)[None], np.arange(n)[None]
    mutual0 = np.take_along_axis(i1, j0, 1) == rows
    mutual1 = np.take_along_axis(j0, i1, 1) == cols
    band = mutual0 & (np.abs(e.astype(np.float64) - th) <= _rel(s) * e)   # exp(s) too close to th to call
    n_band = int(band.sum())
    n_mutual, n_valid = int(mutual0.sum()), int((g["matches0"] >= 0).sum())
    print(f"match head {label} th={th}: mutual {n_mutual}, kept {n_valid}, rows within the band of th {n_band}")
    assert n_band <= (pr * m * 5) // 1000
    valid0 = np.where(band, g["matches0"] >= 0, mutual0 & (e > th))
    valid1 = mutual1 & np.take_along_axis(valid0, i1, 1)
    assert (g["matches0"] == np.where(valid0, j0, -1)).all()
    assert (g["matches1"] == np.where(valid1, i1, -1)).all()
    assert (g["counts"] == valid0.sum(1)).all()
    # scores: zero exactly where not mutual, else exp(s) within the bound; the column side copies the row side
    assert ((g["scores0"] == 0) == ~mutual0).all() and ((g["scores1"] == 0) == ~mutual1).all()
    err = np.abs(g["scores0"].astype(np.float64) - e) / e
    worst = float((err / _rel(s))[mutual0].max(initial=0.0))
    print(f"   mscores0 vs np.exp: worst error {worst:.3f} of the bound")
    assert (err <= _rel(s))[mutual0].all()
    assert (g["scores1"][mutual1] == np.take_along_axis(g["scores0"], i1, 1)[mutual1]).all()
    for p in range(pr):  # the list: the valid rows in ascending i, then -1 / 0
        idx = np.nonzero(valid0[p])[0]
        c = len(idx)
        assert c <= k
        assert (g["matches"][p, :c, 0] == idx).all() and (g["matches"][p, :c, 1] == j0[p, idx]).all()
        assert (g["match_scores"][p, :c] == g["scores0"][p, idx]).all()
        assert (g["matches"][p, c:] == -1).all() and (g["match_scores"][p, c:] == 0).all()
    return n_mutual, n_valid


@pytest.mark.parametrize("pairs,m,n,th", [c + (0.1,) for c in CASES] + [(2, 33, 72, 0.0), (2, 33, 72, 1.0)])
def test_assign_matches_kernel(pairs, m, n, th):
    """Each shape is the smallest that takes one of the kernels' paths: one row and one lane's 8
    columns; a row tail past a 32-row strip with a column tail inside a wave's 512 and two pairs; more
    than one 512-column block and many strips, m < n and m > n; batch offsets with partial blocks both
    ways; the limits (64 strips, 4 column blocks, compaction over 2048 rows)."""
    _need_gpu()
    from lightglue_amd import matcher as mt

    v, scores = _case(pairs, m, n)
    got = mt._Hip.assign_matches(v, m, 256, th)
    n_mutual, n_valid = _check(got, scores, th, f"P={pairs} {m}x{n}")
    assert n_mutual >= 1
    if th == 1.0:       # exp(s) <= 1: nothing is kept
        assert n_valid == 0 and (got.matches.cpu() == -1).all()
    elif th == 0.0:     # every mutual row is kept
        assert n_valid == n_mutual
    elif m >= 8:        # matches on both sides of the threshold: no case is vacuous
        assert 0 < n_valid < n_mutual


def test_guaranteed_ties_go_to_the_lowest_index():
    """v = 0 but a constant matchability logit: every score has the same bits, so every row's best
    column and every column's best row are ties over the whole row / column."""
    dev = _need_gpu()
    from lightglue_amd import matcher as mt

    m, n = 40, 72
    v = torch.zeros((1, m + n, 384), dtype=torch.float16, device=dev)
    v[:, :, 256] = 0.5
    scores = mt._Hip.assign_scores(v, m, 256).cpu().numpy()
    assert (scores.view(np.uint32) == scores.view(np.uint32)[0, 0, 0]).all()
    got = mt._Hip.assign_matches(v, m, 256, 0.0)
    _check(got, scores, 0.0, "all-equal 40x72")
    m0, m1 = got.matches0.cpu().numpy()[0], got.matches1.cpu().numpy()[0]
    assert m0[0] == 0 and (m0[1:] == -1).all() and m1[0] == 0 and (m1[1:] == -1).all()
    assert got.counts.tolist() == [1] and got.matches[0, 0].tolist() == [0, 0]
    s = float(scores[0, 0, 0])
    assert abs(float(got.match_scores[0, 0]) - np.exp(s)) <= float(_rel(np.float32(s))) * np.exp(s)


def test_duplicated_column_ties():
    """Image 1's row 9 is a copy of its row 5 (inside the overlap, so some row's best column): two
    equal columns, and the lower one must win in that row and in the list."""
    _need_gpu()
    from lightglue_amd import matcher as mt

    m, n = 70, 520
    v = _case(1, m, n)[0].clone()
    v[0, m + 9] = v[0, m + 5]
    scores = mt._Hip.assign_scores(v, m, 256).cpu().numpy()
    top = scores.max(2, keepdims=True)
    print(f"duplicated column: columns 5 and 9 bitwise equal: {bool((scores[0, :, 5] == scores[0, :, 9]).all())}; "
          f"rows whose maximum is held twice: {int(((scores == top).sum(2) > 1).sum())}")
    _check(mt._Hip.assign_matches(v, m, 256, 0.1), scores, 0.1, "70x520, column 9 = column 5")
    _check(mt._Hip.assign_matches(v, m, 256, 0.0), scores, 0.0, "70x520, column 9 = column 5")


def _equal_bits(a, b, label):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32), y.view(torch.int32)), (label, f)


def test_pairs_are_independent_and_calls_reproducible():
    """(1) Two calls on one input give the same bits. (2) A pair's results do not depend on its slot
    in the batch: the batch in another order gives the same bits, reordered. (3) P = 3 stacked equals
    three P = 1 calls bit for bit — at a shape where both sizes of batch split the other image the same
    way: lg_assign_scores picks its number of splits S from the whole launch's workgroup count, and
    another S sums a row's exponentials in other groups, so its scores (and so these) may differ in the
    last bit between batch sizes elsewhere. 150 x 136: S = 8 at P = 1 and at P = 3."""
    _need_gpu()
    from lightglue_amd import matcher as mt

    v, _ = _case(3, 300, 296)
    a = mt._Hip.assign_matches(v, 300, 256, 0.1)
    b = mt._Hip.assign_matches(v, 300, 256, 0.1)
    _equal_bits(a, b, "same input twice")
    order = [2, 0, 1]
    c = mt._Hip.assign_matches(v[order].contiguous(), 300, 256, 0.1)
    _equal_bits(mt.MatchResult(*(t[order] for t in a)), c, "pairs reordered")
    m, n = 150, 136
    v, scores = _case(3, m, n)
    whole = mt._Hip.assign_matches(v, m, 256, 0.1)
    _check(whole, scores, 0.1, "P=3 150x136")
    for p in range(3):
        one = mt._Hip.assign_matches(v[p:p + 1].contiguous(), m, 256, 0.1)
        _equal_bits(mt.MatchResult(*(t[p:p + 1] for t in whole)), one, f"pair {p} alone")


def test_match_batch_end_to_end():
    """LightGlueMatcher.match_batch on the fp16 hip path (the forward through the last FFN, then
    lg_assign_matches) for the 512 x 512 sweep fixture's pair inside a P = 2 batch: the same set of
    matches as match() from the same model, and the recall of the reference's matches the batched
    forward test asks; on an fp32 copy of the model (the framework path: filter_matches_dense on the
    scores) the same fields, equal to filter_matches on that model's scores."""
    import os

    from test_matcher import GOLD, SWEEP, SWEEP_RECALL, _match_set, _sweep_model

    dev = _need_gpu()
    from lightglue_amd import matcher

    name = "sweep_l9_512x512"
    meta = SWEEP[name]
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    model, pair = _sweep_model(name)
    at = 1
    ps = [matcher.synthetic_pair(meta["seed"] + 100, meta["m"], meta["n"], overlap=meta["overlap"]), pair]
    for dt in (torch.float32, torch.float16):  # (.to converts in place: fp32 first, from the unrounded weights)
        mod = model.to(dev, dt)
        batch = tuple(torch.cat([p[j] for p in ps], 0).to(dev, dt) for j in range(4))
        with torch.no_grad():
            res = mod.match_batch(*batch)
            old = mod.match(*batch)
            scores = mod(*batch)[2]
        assert isinstance(res, matcher.MatchResult) and res.counts.shape == (2,)
        assert res.matches.dtype == torch.int32 and res.matches.shape == (2, 512, 2)
        for p in range(2):
            c = int(res.counts[p])
            got = _match_set(res.matches[p, :c].cpu().numpy())
            assert len(got) == c and got == _match_set(old[p][0].cpu().numpy()), (dt, p)
            assert (res.matches[p, c:] == -1).all()
        c = int(res.counts[at])
        ref = _match_set(g["matches"])
        hit = len(_match_set(res.matches[at, :c].cpu().numpy()) & ref)
        print(f"match_batch {dt}: {c} matches, recall {hit} / {len(ref)}")
        assert hit >= SWEEP_RECALL * len(ref)
        if dt == torch.float32:
            for p in range(2):
                mm, ss = matcher.filter_matches(scores[p:p + 1], mod.filter_threshold)
                c = int(res.counts[p])
                assert c == len(mm) and (res.matches[p, :c].long() == mm).all() and (res.match_scores[p, :c] == ss).all()
