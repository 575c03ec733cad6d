"""Ragged batches on the MI355X: per-item key counts in the streaming attention kernel
(mha_hd64_launch_grouped_lens / mha_hd64_launch_stream_lens), per-pair row and column counts in the
assignment head and the match head (lg_assign_scores_lens / lg_assign_matches_lens), and
LightGlueMatcher.forward / match_batch / match_pairs with counts on the fp16 fast path.

The rule all of it is held to: a valid row's result depends on no padded row, whatever it holds. So
beside the oracle comparisons every layer has a bitwise test (the lens form with full counts equals
the form without; a uniform count equals the same call on the truncated tensors) and a poison test
(NaN in every padded row changes no bit of any valid result).

Bounds: attention, tests/test_gpu_stream.py's TOL / TOL_F32OUT (the project's contract); the scores,
test_assign_scores_kernel's 2e-5 * scale * 4 against the restatement on the kernel's own similarity (empirical;
tests/test_gpu_assignment.py holds both _lens heads to a float64 reference under the derived bound of
tests/assignment_refs.py);
the matches, tests/test_gpu_match_head.py's _check (indices, counts and padding exact, non-zero
scores within 2^-22 (4 + |s|) relative, at most 0.5 % of rows in the threshold's band) applied to the
scores lg_assign_scores_lens wrote for the same input; the matcher, BATCHED_VS_SINGLE["float16"] and
SWEEP_RECALL of tests/test_matcher.py.
"""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

TOL = 1e-2          # tests/test_gpu_stream.py
TOL_F32OUT = 5e-3
STREAM = 23
FIELDS = ("matches0", "matches1", "scores0", "scores1", "matches", "match_scores", "counts")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib

    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


# =========================================================================================
# attention
# =========================================================================================
def _lens_launch(q, k, v, lens, out_dt, waves):
    """mha_hd64_launch_stream_lens; lens: an int32 device tensor [batch] or None."""
    from lightglue_amd import _lib

    b, h, nq, _ = q.shape
    o = torch.full(q.shape, float("nan"), dtype=out_dt, device=q.device)
    st = _lib.load().mha_hd64_launch_stream_lens(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), b, h, nq,
                                                 k.shape[2], lens.data_ptr() if lens is not None else None,
                                                 int(out_dt == torch.float32), waves,
                                                 torch.cuda.current_stream().cuda_stream)
    assert st == 0, _lib.last_error()
    return o


def _forced_launch(q, k, v, out_dt, waves):
    """The streaming kernel without counts (mha_hd64_launch_forced, code 23, the same wave form)."""
    from lightglue_amd import _lib

    b, h, nq, _ = q.shape
    o = torch.full(q.shape, float("nan"), dtype=out_dt, device=q.device)
    st = _lib.load().mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), b, h, nq, k.shape[2], 0,
                                            int(out_dt == torch.float32), STREAM, waves, 0, None, 0,
                                            torch.cuda.current_stream().cuda_stream, 3)
    assert st == 0, _lib.last_error()
    return o


def _rows(nq, n=40):
    return np.unique(np.r_[np.arange(0, nq, max(1, nq // n)), nq - 1])


# (batch, nq, nkv, lens): a partial tile, one key, one tile; tile edges (64, 65, 128, 129: odd tile
# counts are rounded up to even) over three 128-row query blocks; 640 items, so a workgroup walks 2-3
# items of different tile counts across seams
ATTN = {
    "3x100x77": (3, 100, 77, [77, 1, 40]),
    "5x257x200": (5, 257, 200, [200, 129, 128, 64, 65]),
    "40x512x300": (40, 512, 300, [64 + (37 * b) % 237 for b in range(40)]),
}


@functools.lru_cache(maxsize=None)
def _attn_case(name):
    """(q, k, v fp16 on the GPU, lens on the GPU, the oracle on each item's K[:len], V[:len] for a
    subset of query rows, those rows): computed once per shape, read-only."""
    from lightglue_amd import synth
    from oracle import oracle

    oracle.build()
    batch, nq, nkv, lens = ATTN[name]
    qn, kn, vn = synth.qkv(4100 + 7 * batch + nq + 3 * nkv, nq, nkv, batch=batch)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    rows = _rows(nq)
    ref = np.stack([oracle.attention_c(np.ascontiguousarray(q16[b:b + 1][:, :, rows]),
                                       np.ascontiguousarray(k16[b:b + 1, :, :n]),
                                       np.ascontiguousarray(v16[b:b + 1, :, :n]))[0] for b, n in enumerate(lens)])
    ref.setflags(write=False)
    dev = torch.device("cuda:0")
    q, k, v = (torch.from_numpy(x).to(dev, torch.float16).contiguous() for x in (q16, k16, v16))
    return q, k, v, torch.tensor(lens, dtype=torch.int32, device=dev), ref, rows


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("name", sorted(ATTN))
def test_attention_lens_matches_oracle(name, waves, dev):
    q, k, v, lens, ref, rows = _attn_case(name)
    for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
        o = _lens_launch(q, k, v, lens, out_dt, waves)
        torch.cuda.synchronize()
        got = o.float().cpu().numpy()
        assert np.isfinite(got).all(), "unwritten or NaN output rows"   # (query rows are not masked)
        d = float(np.abs(got[:, :, rows].astype(np.float64) - ref).max())
        print(f"attention lens {name} waves {waves} {out_dt}: max-abs {d:.2e}")
        assert d <= tol, (name, waves, out_dt, d)


@pytest.mark.parametrize("out_dt,tol", [(torch.float16, TOL), (torch.float32, TOL_F32OUT)])
def test_attention_lens_two_calls_one_launch(out_dt, tol, dev):
    """One grouped launch of two calls with different nkv (the MULTI form): one with counts, one
    with a null table, through the Python wrapper and torch.ops."""
    import lightglue_amd
    from lightglue_amd import synth
    from oracle import oracle

    oracle.build()
    lens0 = [40, 77]
    qa, ka, va = (synth.round_f16(x) for x in synth.qkv(4201, 100, 77, batch=2))
    qb, kb, vb = (synth.round_f16(x) for x in synth.qkv(4202, 77, 100, batch=2))
    ref_a = np.stack([oracle.attention_c(qa[b:b + 1], np.ascontiguousarray(ka[b:b + 1, :, :n]),
                                         np.ascontiguousarray(va[b:b + 1, :, :n]))[0] for b, n in enumerate(lens0)])
    ref_b = oracle.attention_c(qb, kb, vb)
    t = lambda x: torch.from_numpy(x).to(dev, torch.float16).contiguous()  # noqa: E731
    calls = [(t(qa), t(ka), t(va)), (t(qb), t(kb), t(vb))]
    lens = torch.tensor(lens0, dtype=torch.int32, device=dev)
    oa, ob = lightglue_amd.mha_hd64_grouped(calls, out_dtype=out_dt, kv_lens=[lens, None])
    torch.cuda.synchronize()
    da = float(np.abs(oa.float().cpu().numpy() - ref_a).max())
    db = float(np.abs(ob.float().cpu().numpy() - ref_b).max())
    print(f"two calls, one launch ({out_dt}): {da:.2e} (with counts) {db:.2e} (null table)")
    assert da <= tol and db <= tol
    if out_dt == torch.float16:
        pa, pb = torch.ops.lightglue_amd.mha_hd64_grouped_lens([c[0] for c in calls], [c[1] for c in calls],
                                                               [c[2] for c in calls], [lens, lens.new_full((2,), 100)])
        assert _same_bits(pa, oa) and _same_bits(pb, ob)   # (a full table = a null one)


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("out_dt", [torch.float16, torch.float32])
def test_attention_lens_bitwise(out_dt, waves, dev):
    """(1) every count = nkv (or a null table): the bits of the streaming launch without counts;
    (2) one count L for every item: the bits of that launch on the contiguous K[:, :, :L], V[:, :, :L]
    (same items, same walk: only the strides differ); (3) counts 0 and nkv + 5 are clamped to 1 and
    nkv."""
    q, k, v, _, _, _ = _attn_case("5x257x200")
    batch, nkv = q.shape[0], k.shape[2]
    full = _forced_launch(q, k, v, out_dt, waves)
    i32 = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)  # noqa: E731
    assert _same_bits(_lens_launch(q, k, v, i32([nkv] * batch), out_dt, waves), full)
    assert _same_bits(_lens_launch(q, k, v, None, out_dt, waves), full)
    for L in (129, 64, 1):
        cut = _forced_launch(q, k[:, :, :L].contiguous(), v[:, :, :L].contiguous(), out_dt, waves)
        assert _same_bits(_lens_launch(q, k, v, i32([L] * batch), out_dt, waves), cut), L
    a = _lens_launch(q, k, v, i32([0, nkv + 5, -7, 1 << 30, 100]), out_dt, waves)
    b = _lens_launch(q, k, v, i32([1, nkv, 1, nkv, 100]), out_dt, waves)
    assert _same_bits(a, b)


@pytest.mark.parametrize("waves", [4, 8])
def test_attention_lens_poison(waves, dev):
    """NaN in every K/V row at or past an item's count: no output bit changes (those rows are never
    read). NaN query rows change their own output rows only."""
    q, k, v, lens, _, _ = _attn_case("5x257x200")
    for out_dt in (torch.float16, torch.float32):
        clean = _lens_launch(q, k, v, lens, out_dt, waves)
        kp, vp = k.clone(), v.clone()
        for b, n in enumerate(lens.tolist()):
            kp[b, :, n:] = float("nan")
            vp[b, :, n:] = float("nan")
        assert _same_bits(_lens_launch(q, kp, vp, lens, out_dt, waves), clean)
        qp = q.clone()
        bad = [(1, 3), (1, 130), (4, 256)]
        for b, r in bad:
            qp[b, :, r] = float("nan")
        got = _lens_launch(qp, kp, vp, lens, out_dt, waves)
        keep = torch.ones(q.shape[:3], dtype=torch.bool, device=dev)
        for b, r in bad:
            keep[b, :, r] = False
        assert torch.equal(_bits(got)[keep], _bits(clean)[keep])


@pytest.mark.parametrize("batch,nq,nkv", [(5, 257, 200), (24, 512, 200)])
def test_attention_query_counts(batch, nq, nkv, dev):
    """mha_hd64_launch_grouped_qkv_lens: query rows at or past an item's q count are padding. A wave
    decides for its 32 rows together when to move their running maxima, so without the counts a real
    row's rounding depends on its padded neighbours; with them the padded rows are written as NaN and
    every real row keeps its bits whatever the padded rows hold. Logits of std ~ 5 (log2 units), so the
    lazy rescale fires; the planner takes the 4-wave form for the first shape, the 8-wave form for
    the second (its last round of 256-row items is 3/4 full)."""
    import lightglue_amd
    from lightglue_amd import synth
    from oracle import oracle

    oracle.build()
    qn, kn, vn = synth.qkv(4300 + batch, nq, nkv, q_std=3.5, batch=batch)
    q16, k16, v16 = (synth.round_f16(x) for x in (qn, kn, vn))
    ql = [1 + (53 * b + 140) % nq for b in range(batch)]
    kl = [1 + (31 * b + 100) % nkv for b in range(batch)]
    t = lambda x: torch.from_numpy(x).to(dev, torch.float16).contiguous()  # noqa: E731
    q, k, v = t(q16), t(k16), t(v16)
    qlt, klt = torch.tensor(ql, dtype=torch.int32, device=dev), torch.tensor(kl, dtype=torch.int32, device=dev)
    real = torch.zeros(q.shape[:3], dtype=torch.bool, device=dev)
    for b, n in enumerate(ql):
        real[b, :, :n] = True
    for out_dt, tol in ((torch.float16, TOL), (torch.float32, TOL_F32OUT)):
        base = lightglue_amd.mha_hd64_grouped([(q, k, v)], out_dtype=out_dt, kv_lens=[klt], q_lens=[qlt])[0]
        assert torch.isfinite(base[real]).all() and torch.isnan(base[~real]).all()
        for b in sorted({0, batch // 2, batch - 1}):
            rows = _rows(ql[b], 10)
            ref = oracle.attention_c(np.ascontiguousarray(q16[b:b + 1][:, :, rows]), np.ascontiguousarray(k16[b:b + 1, :, :kl[b]]),
                                     np.ascontiguousarray(v16[b:b + 1, :, :kl[b]]))
            d = float(np.abs(base[b:b + 1][:, :, rows].float().cpu().numpy() - ref).max())
            assert d <= tol, (b, out_dt, d)
        for fill in (0.0, 40.0, float("nan"), float("inf")):
            qp, kp, vp = q.clone(), k.clone(), v.clone()
            qp[~real] = fill
            for b, n in enumerate(kl):
                kp[b, :, n:] = fill
                vp[b, :, n:] = fill
            got = lightglue_amd.mha_hd64_grouped([(qp, kp, vp)], out_dtype=out_dt, kv_lens=[klt], q_lens=[qlt])[0]
            assert torch.equal(_bits(got)[real], _bits(base)[real]), (out_dt, fill)
            assert torch.isnan(got[~real]).all()
    # a null q table and a full one: the bits of the key counts alone
    only_k = lightglue_amd.mha_hd64_grouped([(q, k, v)], kv_lens=[klt])[0]
    assert _same_bits(lightglue_amd.mha_hd64_grouped([(q, k, v)], kv_lens=[klt], q_lens=[None])[0], only_k)
    assert _same_bits(lightglue_amd.mha_hd64_grouped([(q, k, v)], kv_lens=[klt], q_lens=[qlt.new_full((batch,), nq)])[0], only_k)


# =========================================================================================
# the assignment head and the match head
# =========================================================================================
# (P, M, N, ((m_len, n_len), ...)): one valid entry; a full pair beside a nearly empty one; one valid
# column in the second 512-column block; whole strips and column blocks empty, and a 31-row pair;
# the limits
HEAD = {
    "1x8x8": (1, 8, 8, ((1, 1),)),
    "2x33x72": (2, 33, 72, ((33, 72), (1, 5))),
    "1x70x520": (1, 70, 520, ((70, 513),)),
    "3x300x296": (3, 300, 296, ((300, 296), (257, 100), (31, 290))),
    "1x2048x2048": (1, 2048, 2048, ((2047, 2041),)),
}


def _pair_rows(sd, m, n):
    """One pair's v [m + n, 384] (fp32 values, before the fp16 rounding); as tests/test_gpu_match_head.py."""
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


def _head_rows(name):
    """v [P, M + N, 384] fp32 (numpy): each pair's valid rows from _pair_rows at its own size, every
    padded row a loud finite one (descriptor 4 x a valid row of the pair, logit +6: unmasked it would be
    every row's best partner)."""
    pairs, m, n, lens = HEAD[name]
    v = np.zeros((pairs, m + n, 384), dtype=np.float32)
    for p, (ml, nl) in enumerate(lens):
        rows = _pair_rows(9 * 16 + 5 * p + m, ml, nl)
        v[p, :ml], v[p, m:m + nl] = rows[:ml], rows[ml:]
        loud = 4 * rows[0]
        loud[256] = 6.0
        v[p, ml:m], v[p, m + nl:] = loud, loud
    return v


@functools.lru_cache(maxsize=None)
def _head_case(name):
    """(v fp16 on the GPU, m_len, n_len on the GPU, the scores lg_assign_scores_lens gives on the host,
    the kernel's own similarity): computed once per case, read-only."""
    from lightglue_amd import matcher as mt

    pairs, m, n, lens = HEAD[name]
    dev = torch.device("cuda:0")
    v = torch.from_numpy(_head_rows(name)).to(dev, torch.float16)
    ml = torch.tensor([a for a, _ in lens], dtype=torch.int32, device=dev)
    nl = torch.tensor([b for _, b in lens], dtype=torch.int32, device=dev)
    scores = mt._Hip.assign_scores(v, m, 256, (ml, nl))
    sim = mt._Hip._last_assign_ws[:pairs * m * n * 2].view(torch.float16).view(pairs, m, n).clone()
    scores = scores.cpu().numpy()
    scores.setflags(write=False)
    return v, ml, nl, scores, sim


def _rel(s):
    return 2.0 ** -22 * (4.0 + np.abs(s.astype(np.float64)))


def _check(got, scores, th, label):
    """tests/test_gpu_match_head.py's _check (got: MatchResult on the GPU; scores [P, m, n] fp32, numpy,
    here with -inf on padded rows and columns: such a row's best is column 0 at -inf, never mutual).
    Returns per pair (mutual, kept)."""
    pr, m, n = scores.shape
    k = min(m, n)
    g = {f: getattr(got, f).cpu().numpy() for f in FIELDS}
    assert g["matches0"].shape == (pr, m) and g["matches1"].shape == (pr, n) and g["matches"].shape == (pr, k, 2)
    assert g["scores0"].shape == (pr, m) and g["scores1"].shape == (pr, n) and g["match_scores"].shape == (pr, k)
    assert g["counts"].shape == (pr,)
    assert all(g[f].dtype == np.int32 for f in ("matches0", "matches1", "matches", "counts"))
    j0, i1 = scores.argmax(2), scores.argmax(1)              # lowest index among equals
    s = np.take_along_axis(scores, j0[..., None], 2)[..., 0]
    with np.errstate(all="ignore"):                          # (padded rows: s = -inf, e = 0)
        e = np.exp(s)                                        # fp32
        rows, cols = np.arange(m)[None], np.arange(n)[None]
        mutual0 = (np.take_along_axis(i1, j0, 1) == rows) & np.isfinite(s)
        mutual1 = (np.take_along_axis(j0, i1, 1) == cols) & np.isfinite(scores.max(1))
        band = mutual0 & (np.abs(e.astype(np.float64) - th) <= _rel(s) * e)   # exp(s) too close to th to call
        err = np.abs(g["scores0"].astype(np.float64) - e) / e
    n_band = int(band.sum())
    n_mutual, n_valid = int(mutual0.sum()), int((g["matches0"] >= 0).sum())
    print(f"match head {label} th={th}: mutual {n_mutual}, kept {n_valid}, rows within the band of th {n_band}")
    assert n_band <= (pr * m * 5) // 1000
    valid0 = np.where(band, g["matches0"] >= 0, mutual0 & (e > th))
    valid1 = mutual1 & np.take_along_axis(valid0, i1, 1)
    assert (g["matches0"] == np.where(valid0, j0, -1)).all()
    assert (g["matches1"] == np.where(valid1, i1, -1)).all()
    assert (g["counts"] == valid0.sum(1)).all()
    assert ((g["scores0"] == 0) == ~mutual0).all() and ((g["scores1"] == 0) == ~mutual1).all()
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
    return [(int(mutual0[p].sum()), int((g["matches0"][p] >= 0).sum())) for p in range(pr)]


def _check_padding(got, lens, m, n):
    """matches -1 and scores 0 on every padded row and column; the list within min(m_len, n_len)."""
    for p, (ml, nl) in enumerate(lens):
        assert (got.matches0[p, ml:] == -1).all() and (got.scores0[p, ml:] == 0).all()
        assert (got.matches1[p, nl:] == -1).all() and (got.scores1[p, nl:] == 0).all()
        assert (got.matches0[p] < nl).all() and (got.matches1[p] < ml).all()
        assert int(got.counts[p]) <= min(ml, nl)


@pytest.mark.parametrize("name", sorted(HEAD))
def test_assign_scores_lens(name, dev):
    from lightglue_amd import matcher as mt

    pairs, m, n, lens = HEAD[name]
    v, _, _, scores, sim = _head_case(name)
    got = torch.from_numpy(np.array(scores))
    for p, (ml, nl) in enumerate(lens):
        assert (got[p, ml:] == float("-inf")).all() and (got[p, :, nl:] == float("-inf")).all()   # exactly
        own = sim[p:p + 1, :ml, :nl].float()
        z0, z1 = v[p:p + 1, :ml, 256:257].float(), v[p:p + 1, m:m + nl, 256:257].float()
        ref = mt.log_double_softmax(own, z0, z1).cpu()
        scale = max(1.0, float(own.abs().max()))
        e = float((got[p:p + 1, :ml, :nl] - ref).abs().max())
        print(f"assign scores lens {name} pair {p} ({ml} x {nl}): vs the restatement on its own sim {e:.2e} "
              f"(bound {2e-5 * scale * 4:.2e})")
        assert torch.isfinite(got[p, :ml, :nl]).all() and e <= 2e-5 * scale * 4


def _restated_band_rows(name, th):
    """Rows whose exp(score) lies in the band of th, by the fp32 torch restatement on the CPU."""
    from lightglue_amd import matcher as mt

    pairs, m, n, lens = HEAD[name]
    v = torch.from_numpy(_head_rows(name)).half()
    total = 0
    for p, (ml, nl) in enumerate(lens):
        m0, m1 = v[p, :ml, :256].float(), v[p, m:m + nl, :256].float()
        sim = (m0 @ m1.T).half().float()[None]
        sc = mt.log_double_softmax(sim, v[p:p + 1, :ml, 256:257].float(), v[p:p + 1, m:m + nl, 256:257].float())[0].numpy()
        j0, i1 = sc.argmax(1), sc.argmax(0)
        s = sc[np.arange(ml), j0]
        e = np.exp(s)
        mutual = i1[j0] == np.arange(ml)
        total += int((mutual & (np.abs(e.astype(np.float64) - th) <= 4 * _rel(s) * e)).sum())   # (4 x the band)
    return total


@pytest.mark.parametrize("name,th", [(c, 0.1) for c in sorted(HEAD)] + [("2x33x72", 0.0), ("2x33x72", 1.0)])
def test_assign_matches_lens(name, th, dev):
    from lightglue_amd import matcher as mt

    pairs, m, n, lens = HEAD[name]
    if m <= 300:   # the chosen inputs put no row near the threshold (restated in fp32 on the CPU)
        assert _restated_band_rows(name, th) == 0
    v, ml, nl, scores, _ = _head_case(name)
    got = mt._Hip.assign_matches(v, m, 256, th, (ml, nl))
    per_pair = _check(got, scores, th, name)
    _check_padding(got, lens, m, n)
    assert sum(a for a, _ in per_pair) >= 1                  # at least one mutual match
    for (a, b), (n_mutual, n_valid) in zip(lens, per_pair):
        if th == 1.0:       # exp(s) <= 1: nothing is kept
            assert n_valid == 0
        elif th == 0.0:     # every mutual row is kept
            assert n_valid == n_mutual
        elif a >= 8:        # matches on both sides of the threshold: no pair is vacuous
            assert 0 < n_valid < n_mutual, (a, b, n_mutual, n_valid)


def _equal_results(a, b, label):
    for f in FIELDS:
        assert _same_bits(getattr(a, f), getattr(b, f)), (label, f)


def test_head_lens_full_counts_equal_the_equal_size_head(dev):
    """Full counts (and null tables): both new functions equal lg_assign_scores / lg_assign_matches in
    every bit."""
    from lightglue_amd import matcher as mt

    pairs, m, n, _ = HEAD["3x300x296"]
    v = _head_case("3x300x296")[0]
    full = (torch.full((pairs,), m, dtype=torch.int32, device=dev), torch.full((pairs,), n, dtype=torch.int32, device=dev))
    ref_s, ref_m = mt._Hip.assign_scores(v, m, 256), mt._Hip.assign_matches(v, m, 256, 0.1)
    assert _same_bits(mt._Hip.assign_scores(v, m, 256, full), ref_s)
    _equal_results(mt._Hip.assign_matches(v, m, 256, 0.1, full), ref_m, "full counts")
    # over-long counts are clamped to the full sizes
    over = (full[0] + 9, full[1] + 100)
    assert _same_bits(mt._Hip.assign_scores(v, m, 256, over), ref_s)
    _equal_results(mt._Hip.assign_matches(v, m, 256, 0.1, over), ref_m, "clamped counts")


@pytest.mark.parametrize("name", ["2x33x72", "3x300x296", "1x70x520"])
def test_head_lens_poison(name, dev):
    """NaN in every padded row of v (all 384 channels): every bit of the scores and of the matches is
    the clean run's."""
    from lightglue_amd import matcher as mt

    pairs, m, n, lens = HEAD[name]
    v, ml, nl, scores, _ = _head_case(name)
    vp = v.clone()
    for p, (a, b) in enumerate(lens):
        vp[p, a:m] = float("nan")
        vp[p, m + b:] = float("nan")
    assert torch.equal(_bits(mt._Hip.assign_scores(vp, m, 256, (ml, nl))).cpu(), torch.from_numpy(np.array(scores)).view(torch.int32))
    _equal_results(mt._Hip.assign_matches(vp, m, 256, 0.1, (ml, nl)), mt._Hip.assign_matches(v, m, 256, 0.1, (ml, nl)), "poison")


def test_head_lens_reproducible_and_pairs_independent(dev):
    from lightglue_amd import matcher as mt

    pairs, m, n, _ = HEAD["3x300x296"]
    v, ml, nl, scores, _ = _head_case("3x300x296")
    a = mt._Hip.assign_matches(v, m, 256, 0.1, (ml, nl))
    b = mt._Hip.assign_matches(v, m, 256, 0.1, (ml, nl))
    _equal_results(a, b, "same input twice")
    order = [2, 0, 1]
    c = mt._Hip.assign_matches(v[order].contiguous(), m, 256, 0.1, (ml[order].contiguous(), nl[order].contiguous()))
    _equal_results(mt.MatchResult(*(t[order] for t in a)), c, "pairs reordered")
    s = mt._Hip.assign_scores(v[order].contiguous(), m, 256, (ml[order].contiguous(), nl[order].contiguous()))
    assert torch.equal(_bits(s).cpu(), torch.from_numpy(np.array(scores[order])).view(torch.int32))


# =========================================================================================
# the matcher, 9 layers, fp16
# =========================================================================================
SIZES = [(150, 136), (120, 97), (64, 120)]
BATCHED_VS_SINGLE_F16 = (6e-2, 0.6)   # tests/test_matcher.py BATCHED_VS_SINGLE["float16"]
SWEEP_RECALL = 0.9                    # tests/test_matcher.py


def _match_set(m):
    return {(int(a), int(b)) for a, b in np.asarray(m)}


@functools.lru_cache(maxsize=None)
def _matcher_case():
    """(model, the pairs on the GPU, the padded batch [3, 150 | 136, .], each pair's own forward and
    match_batch through the equal-size code): computed once, read-only."""
    from lightglue_amd import matcher

    dev = torch.device("cuda:0")
    model = matcher.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(matcher.seeded_state_dict(7, 9), strict=True)
    model = model.to(dev, torch.float16)
    pairs = [tuple(t.to(dev, torch.float16) for t in matcher.synthetic_pair(300 + i, m, n, overlap=min(m, n) // 2))
             for i, (m, n) in enumerate(SIZES)]
    m, n = max(a for a, _ in SIZES), max(b for _, b in SIZES)
    assert n % 8 == 0
    batch = []
    for j, size in enumerate((m, n, m, n)):
        t = torch.zeros((len(pairs), size, pairs[0][j].shape[-1]), dtype=torch.float16, device=dev)
        for p, pair in enumerate(pairs):
            t[p, :pair[j].shape[1]] = pair[j][0]
        batch.append(t)
    with torch.no_grad():
        fwd = [model(*p) for p in pairs]
        res = [model.match_batch(*p) for p in pairs]
    torch.cuda.synchronize()
    return model, pairs, tuple(batch), fwd, res


def test_matcher_forward_counts_equals_single_pairs(dev):
    model, pairs, batch, fwd, _ = _matcher_case()
    c0, c1 = [a for a, _ in SIZES], [b for _, b in SIZES]
    with torch.no_grad():
        d0, d1, sc = model(*batch, counts0=c0, counts1=c1)
    torch.cuda.synchronize()
    assert sc.shape == (3, 150, 136) and sc.dtype == torch.float32
    tol_d, tol_s = BATCHED_VS_SINGLE_F16
    for p, ((a, b), (e0, e1, es)) in enumerate(zip(SIZES, fwd)):
        assert (sc[p, a:] == float("-inf")).all() and (sc[p, :, b:] == float("-inf")).all()
        ed = max(float((d0[p, :a].float() - e0[0].float()).abs().max()), float((d1[p, :b].float() - e1[0].float()).abs().max()))
        es_ = float((sc[p, :a, :b] - es[0].float()).abs().max())
        print(f"ragged forward vs the pair alone, pair {p} ({a} x {b}): desc {ed:.3e} scores {es_:.3e}")
        assert torch.isfinite(sc[p, :a, :b]).all() and ed <= tol_d and es_ <= tol_s, (p, ed, es_)


def test_matcher_match_batch_counts(dev):
    """match_batch(counts) equals the semantics applied to forward(counts)'s own scores, match_pairs
    equals it, and each pair keeps at least SWEEP_RECALL of the matches it gets alone."""
    model, pairs, batch, _, res = _matcher_case()
    c0, c1 = [a for a, _ in SIZES], [b for _, b in SIZES]
    with torch.no_grad():
        sc = model(*batch, counts0=c0, counts1=c1)[2]
        got = model.match_batch(*batch, counts0=torch.tensor(c0), counts1=torch.tensor(c1))
        via_pairs, r0, r1 = model.match_pairs([tuple(t[0] for t in p) for p in pairs])
    torch.cuda.synchronize()
    _check(got, sc.cpu().numpy(), model.filter_threshold, "matcher 3 ragged pairs")
    _check_padding(got, SIZES, 150, 136)
    assert (r0, r1) == (c0, c1)
    _equal_results(via_pairs, got, "match_pairs")
    for p, one in enumerate(res):
        alone = _match_set(one.matches[0, :int(one.counts[0])].cpu().numpy())
        mine = _match_set(got.matches[p, :int(got.counts[p])].cpu().numpy())
        print(f"ragged match_batch pair {p}: {len(mine)} matches, {len(mine & alone)} of the {len(alone)} it gets alone")
        assert len(alone) >= 1 and len(mine & alone) >= SWEEP_RECALL * len(alone)


def test_matcher_single_pair_off_size_reaches_the_fast_path(dev):
    """A single pair with n % 8 != 0 through match_pairs: padded to 104 columns with its count, the
    chained fp16 path and lg_assign_matches_lens (its own scores are the oracle)."""
    model, pairs, _, _, res = _matcher_case()
    pair = tuple(t[0] for t in pairs[1])   # 120 x 97
    with torch.no_grad():
        got, c0, c1 = model.match_pairs([pair])
    assert (c0, c1) == ([120], [97]) and got.matches1.shape == (1, 104)
    _check_padding(got, [(120, 97)], 120, 104)
    alone = _match_set(res[1].matches[0, :int(res[1].counts[0])].cpu().numpy())
    mine = _match_set(got.matches[0, :int(got.counts[0])].cpu().numpy())
    assert len(mine & alone) >= SWEEP_RECALL * len(alone)


def test_matcher_poison(dev):
    """NaN in every padded descriptor and keypoint row: a bitwise-equal MatchResult and bitwise-equal
    valid descriptors."""
    model, _, batch, _, _ = _matcher_case()
    c0, c1 = [a for a, _ in SIZES], [b for _, b in SIZES]
    bad = [t.clone() for t in batch]
    for p, (a, b) in enumerate(SIZES):
        bad[0][p, a:] = bad[2][p, a:] = float("nan")
        bad[1][p, b:] = bad[3][p, b:] = float("nan")
    with torch.no_grad():
        d0, d1, sc = model(*batch, counts0=c0, counts1=c1)
        e0, e1, esc = model(*bad, counts0=c0, counts1=c1)
        _equal_results(model.match_batch(*bad, counts0=c0, counts1=c1), model.match_batch(*batch, counts0=c0, counts1=c1),
                       "poisoned padding")
    assert _same_bits(esc, sc)
    for p, (a, b) in enumerate(SIZES):
        assert _same_bits(e0[p, :a], d0[p, :a]) and _same_bits(e1[p, :b], d1[p, :b])


def test_matcher_counts_are_read_on_the_device(dev):
    """One capture of match_batch with counts in device tensors, one replay after new counts were
    written into the same tensors: the eager result for the new counts (the counts are kernel inputs
    read at run time; nothing in the forward depends on their values on the host)."""
    model, _, batch, _, _ = _matcher_case()
    old = ([150, 120, 64], [136, 97, 120])
    new = ([97, 150, 33], [136, 50, 111])
    c0 = torch.tensor(old[0], dtype=torch.int32, device=dev)
    c1 = torch.tensor(old[1], dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):   # warm-up off the capture: caches, workspaces
        model.match_batch(*batch, counts0=c0, counts1=c1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        captured = model.match_batch(*batch, counts0=c0, counts1=c1)
    with torch.no_grad():
        graph.replay()
        torch.cuda.synchronize()
        _equal_results(captured, model.match_batch(*batch, counts0=old[0], counts1=old[1]), "replay, the captured counts")
        c0.copy_(torch.tensor(new[0], dtype=torch.int32))
        c1.copy_(torch.tensor(new[1], dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want = model.match_batch(*batch, counts0=new[0], counts1=new[1])
    _equal_results(captured, want, "replay, new counts")
    assert captured.counts.tolist() != [0, 0, 0]
