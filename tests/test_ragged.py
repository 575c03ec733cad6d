"""Ragged batches, host side (no GPU): per-pair keypoint counts through LightGlueMatcher.forward /
match_batch / match_pairs on the framework path (pairs one at a time on their valid slices, results
padded), the dense oracle on padded scores, count validation, and the argument checks of the new C
entry points (include/mha_hd64.h: mha_hd64_launch_grouped_lens, mha_hd64_launch_stream_lens;
include/lightglue_glue.h: lg_assign_scores_lens, lg_assign_matches_lens), which all happen before
any device call. (The kernels: tests/test_gpu_ragged.py.)
"""
import ctypes
import functools

import pytest

torch = pytest.importorskip("torch")

SIZES = [(5, 7), (9, 4), (3, 3)]   # (m_p, n_p): M = 9, N = 7 -> 8 after match_pairs' rounding
FIELDS = ("matches0", "matches1", "scores0", "scores1", "matches", "match_scores", "counts")
A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below


def _oracle_attention(calls):
    from oracle import oracle

    return [oracle.attention_torch(q, k, v) for q, k, v in calls]


@functools.lru_cache(maxsize=None)
def _setup():
    """(model, the pairs, each pair's own forward and match_batch): computed once, read-only."""
    from lightglue_amd import matcher

    model = matcher.LightGlueMatcher(n_layers=2, attention=_oracle_attention, glue="torch").eval()
    model.load_state_dict(matcher.seeded_state_dict(11, 2), strict=True)
    pairs = [matcher.synthetic_pair(40 + i, m, n, overlap=min(m, n) // 2 + 1) for i, (m, n) in enumerate(SIZES)]
    with torch.no_grad():
        fwd = [model(*p) for p in pairs]
        res = [model.match_batch(*p) for p in pairs]
    return model, pairs, fwd, res


def _padded(pairs, m, n):
    """The four inputs zero-padded to [P, m or n, .]."""
    out = []
    for j, size in enumerate((m, n, m, n)):
        t = torch.zeros((len(pairs), size, pairs[0][j].shape[-1]))
        for p, pair in enumerate(pairs):
            t[p, :pair[j].shape[1]] = pair[j][0]
        out.append(t)
    return out


def _check_result(got, singles, m, n):
    """got (a MatchResult of the padded batch) equals each pair's own, padded with -1 / 0."""
    k = min(m, n)
    assert got.matches0.shape == (len(SIZES), m) and got.matches1.shape == (len(SIZES), n)
    assert got.matches.shape == (len(SIZES), k, 2) and got.match_scores.shape == (len(SIZES), k)
    for p, ((a, b), one) in enumerate(zip(SIZES, singles)):
        kk = min(a, b)
        assert torch.equal(got.matches0[p, :a], one.matches0[0]) and (got.matches0[p, a:] == -1).all()
        assert torch.equal(got.matches1[p, :b], one.matches1[0]) and (got.matches1[p, b:] == -1).all()
        assert torch.equal(got.scores0[p, :a], one.scores0[0]) and (got.scores0[p, a:] == 0).all()
        assert torch.equal(got.scores1[p, :b], one.scores1[0]) and (got.scores1[p, b:] == 0).all()
        assert torch.equal(got.matches[p, :kk], one.matches[0]) and (got.matches[p, kk:] == -1).all()
        assert torch.equal(got.match_scores[p, :kk], one.match_scores[0]) and (got.match_scores[p, kk:] == 0).all()
        assert int(got.counts[p]) == int(one.counts[0])
    assert all(getattr(got, f).dtype == getattr(singles[0], f).dtype for f in FIELDS)


def test_per_pair_loop_equals_single_pairs():
    """glue='torch' with a substituted attention is not the fast path: match_pairs and forward(counts)
    run the pairs one at a time on their valid slices and pad the results."""
    model, pairs, fwd, res = _setup()
    assert sum(int(r.counts[0]) for r in res) >= 1   # (not vacuous: some pair has a match)
    with torch.no_grad():
        got, c0, c1 = model.match_pairs([tuple(t[0] for t in p) for p in pairs])
    assert c0 == [a for a, _ in SIZES] and c1 == [b for _, b in SIZES]   # the counts, as given
    _check_result(got, res, 9, 8)                     # N = 7 rounded up to 8
    m, n = 9, 7
    batch = _padded(pairs, m, n)
    for counts in ((c0, c1), (torch.tensor(c0), torch.tensor(c1, dtype=torch.int32))):
        with torch.no_grad():
            d0, d1, sc = model(*batch, counts0=counts[0], counts1=counts[1])
            mb = model.match_batch(*batch, counts0=counts[0], counts1=counts[1])
        assert d0.shape == (3, m, 256) and d1.shape == (3, n, 256) and sc.shape == (3, m, n) and sc.dtype == torch.float32
        for p, ((a, b), (e0, e1, es)) in enumerate(zip(SIZES, fwd)):
            assert torch.equal(d0[p, :a], e0[0]) and torch.equal(d1[p, :b], e1[0]) and torch.equal(sc[p, :a, :b], es[0])
            assert (d0[p, a:] == 0).all() and (d1[p, b:] == 0).all()
            assert (sc[p, a:] == float("-inf")).all() and (sc[p, :, b:] == float("-inf")).all()
        _check_result(mb, res, m, n)
    # one side's counts only: the other side is full
    with torch.no_grad():
        full1 = model.match_batch(*_padded(pairs[2:], 3, 3), counts0=[3])
    for f in FIELDS:
        assert torch.equal(getattr(full1, f), getattr(res[2], f)), f
    # no counts: today's call, unchanged
    with torch.no_grad():
        same = model.match_batch(*pairs[0])
    for f in FIELDS:
        assert torch.equal(getattr(same, f), getattr(res[0], f)), f


def test_dense_oracle_on_padded_scores():
    """filter_matches_dense on scores padded with -inf gives each pair's own result (padded rows and
    columns: -1 / 0): the oracle the GPU tests apply to lg_assign_scores_lens' output."""
    from lightglue_amd.matcher import filter_matches_dense

    model, pairs, fwd, res = _setup()
    m, n = 9, 8
    sc = torch.full((len(SIZES), m, n), float("-inf"))
    for p, ((a, b), f) in enumerate(zip(SIZES, fwd)):
        sc[p, :a, :b] = f[2][0]
    _check_result(filter_matches_dense(sc, model.filter_threshold), res, m, n)
    _check_result(filter_matches_dense(sc, 0.0), [filter_matches_dense(f[2], 0.0) for f in fwd], m, n)


def test_count_validation():
    model, pairs, _, _ = _setup()
    batch = _padded(pairs, 9, 8)
    good0, good1 = [5, 9, 3], [7, 4, 3]
    bads = [dict(counts0=[0, 9, 3], counts1=good1), dict(counts0=good0, counts1=[7, 0, 3]),
            dict(counts0=[5, 10, 3], counts1=good1), dict(counts0=good0, counts1=[7, 4, 9]),
            dict(counts0=[5, 9], counts1=good1), dict(counts0=good0, counts1=[7, 4, 3, 3]),
            dict(counts0=torch.tensor([5, 9, 3, 1]), counts1=good1), dict(counts0=torch.tensor([5.0, 9.0, 3.0]), counts1=good1),
            dict(counts0=[-1, 9, 3])]
    for bad in bads:
        for fn in (model.forward, model.match_batch):
            with pytest.raises(ValueError):
                fn(*batch, **bad)
    with pytest.raises(ValueError):
        model.match_pairs([])


# ---- the C entry points ----
@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def _calls(n=1, **kw):
    from lightglue_amd import _lib

    a = dict(q=A, k=A, v=A, o=A, batch=2, heads=4, nq=8, nkv=8)
    a.update(kw)
    arr = (_lib.CallDesc * n)()
    for i in range(n):
        arr[i] = _lib.CallDesc(a["q"], a["k"], a["v"], a["o"], a["batch"], a["heads"], a["nq"], a["nkv"])
    return arr


def _lens(n=1, value=A):
    return (ctypes.c_void_p * n)(*([value] * n))


def test_attention_lens_rejects_before_touching_the_device(lib):
    """Every reject returns BAD_PARAM before a device call (this host has no GPU: a launch would fail
    with another status)."""
    from lightglue_amd import _lib

    HALF, FLOAT, BAD = _lib.DT_HALF, _lib.DT_FLOAT, _lib.STATUS_BAD_PARAM
    f = lib.mha_hd64_launch_grouped_lens
    assert f(_calls(), _lens(), 1, FLOAT, FLOAT, None, 0, None) == BAD          # fp16 inputs only
    assert f(_calls(), _lens(), 1, FLOAT, HALF, None, 0, None) == BAD
    assert f(_calls(), _lens(), 1, HALF, 2, None, 0, None) == BAD               # no such output type
    assert f(_calls(), None, 1, HALF, HALF, None, 0, None) == BAD               # a null kv_lens array
    assert f(None, _lens(), 1, HALF, HALF, None, 0, None) == BAD                # null calls
    assert f(_calls(), _lens(value=A + 2), 1, HALF, HALF, None, 0, None) == BAD  # a misaligned table
    for name in ("q", "k", "v", "o"):
        assert f(_calls(**{name: A + 8}), _lens(), 1, HALF, HALF, None, 0, None) == BAD, name
        assert f(_calls(**{name: None}), _lens(), 1, HALF, HALF, None, 0, None) == BAD, name
    assert f(_calls(nkv=0), _lens(), 1, HALF, HALF, None, 0, None) == BAD
    assert f(_calls(batch=-1), _lens(), 1, HALF, HALF, None, 0, None) == BAD
    assert f(_calls(5), _lens(5), -1, HALF, HALF, None, 0, None) == BAD
    assert "mha_hd64" in _lib.last_error()
    # nothing to compute: success without a launch (null per-call tables are legal: all nkv keys)
    assert f(None, None, 0, HALF, HALF, None, 0, None) == 0
    assert f(_calls(nq=0), _lens(value=None), 1, HALF, FLOAT, None, 0, None) == 0
    assert f(_calls(6, batch=0), _lens(6), 6, HALF, HALF, None, 0, None) == 0
    # with query-row counts: the same checks; the q_lens array itself may be null
    h = lib.mha_hd64_launch_grouped_qkv_lens
    assert h(_calls(), _lens(), _lens(), 1, FLOAT, FLOAT, None, 0, None) == BAD
    assert h(_calls(), _lens(), None, 1, HALF, HALF, None, 0, None) == BAD
    assert h(None, None, _lens(), 1, HALF, HALF, None, 0, None) == BAD
    assert h(_calls(), _lens(value=A + 1), _lens(), 1, HALF, HALF, None, 0, None) == BAD
    assert h(_calls(o=A + 4), None, _lens(), 1, HALF, HALF, None, 0, None) == BAD
    assert h(_calls(nq=0), None, _lens(value=None), 1, HALF, HALF, None, 0, None) == 0
    assert h(_calls(batch=0), _lens(), _lens(), 1, HALF, FLOAT, None, 0, None) == 0
    # the test hook: the same checks, and the wave form
    g = lib.mha_hd64_launch_stream_lens
    assert g(A, A, A, A, 2, 4, 8, 8, A, 0, 5, None) == BAD                       # waves: 0, 4 or 8
    assert g(A, A, A, A + 8, 2, 4, 8, 8, A, 0, 4, None) == BAD
    assert g(None, A, A, A, 2, 4, 8, 8, A, 1, 8, None) == BAD
    assert g(A, A, A, A, 2, 4, 8, 8, A + 1, 0, 0, None) == BAD
    assert g(A, A, A, A, 2, 4, 8, 0, A, 0, 0, None) == BAD
    assert g(A, A, A, A, 2, 4, 0, 8, None, 0, 4, None) == 0


def _scores(lib, **kw):
    a = dict(v=A, ps=16 * 384, ld=384, zc=256, m=8, n=8, batch=1, ml=A, nl=A, sc=A, ws=A)
    a.update(kw)
    return lib.lg_assign_scores_lens(a["v"], a["ps"], a["ld"], a["zc"], a["m"], a["n"], a["batch"], a["ml"], a["nl"], a["sc"],
                                     a["ws"], None)


def _matches(lib, **kw):
    a = dict(v=A, ps=16 * 384, ld=384, zc=256, m=8, n=8, batch=1, ml=A, nl=A, th=0.1, m0=A, m1=A, s0=A, s1=A, mt=A, ms=A,
             cnt=A, ws=A)
    a.update(kw)
    return lib.lg_assign_matches_lens(a["v"], a["ps"], a["ld"], a["zc"], a["m"], a["n"], a["batch"], a["ml"], a["nl"], a["th"],
                                      a["m0"], a["m1"], a["s0"], a["s1"], a["mt"], a["ms"], a["cnt"], a["ws"], None)


def test_head_lens_validate_before_touching_the_device(lib):
    from lightglue_amd import _lib

    bads = [dict(n=12), dict(m=2049, ps=(2049 + 8) * 384), dict(n=2056, ps=(8 + 2056) * 384), dict(zc=255), dict(zc=384),
            dict(ld=380), dict(v=None), dict(v=A + 8), dict(ws=None), dict(ws=A + 8), dict(ps=16 * 384 - 1), dict(m=-1),
            dict(batch=-1), dict(ml=A + 2), dict(nl=A + 1)]
    for bad in bads:
        assert _scores(lib, **bad) == _lib.STATUS_BAD_PARAM, bad
        assert "lg_assign_scores_lens" in _lib.last_error(), bad
        assert _matches(lib, **bad) == _lib.STATUS_BAD_PARAM, bad
        assert "lg_assign_matches_lens" in _lib.last_error(), bad
    assert _scores(lib, sc=None) == _lib.STATUS_BAD_PARAM and _scores(lib, sc=A + 4) == _lib.STATUS_BAD_PARAM
    for bad in [dict(th=-0.5), dict(th=float("nan"))] + [{k: None} for k in ("m0", "m1", "s0", "s1", "mt", "ms", "cnt")] + \
            [{k: A + 2} for k in ("m0", "m1", "s0", "s1", "mt", "ms", "cnt")]:
        assert _matches(lib, **bad) == _lib.STATUS_BAD_PARAM, bad


def test_null_lens_pass_the_workspace_free_checks(lib):
    """Null m_len / n_len mean "every pair is full": the calls that need no workspace and launch
    nothing accept them like any other table, and the workspace queries are the equal-size ones."""
    for kw in (dict(ml=None, nl=None), dict(ml=None), dict(nl=None), dict()):
        assert _scores(lib, batch=0, **kw) == 0
        assert _scores(lib, batch=0, v=None, ws=None, sc=None, **kw) == 0
        assert _scores(lib, m=0, ps=8 * 384, **kw) == 0
        assert _scores(lib, n=0, ps=8 * 384, v=None, ws=None, sc=None, **kw) == 0
        assert _matches(lib, batch=0, **kw) == 0
        assert _matches(lib, batch=0, v=None, ws=None, m0=None, cnt=None, **kw) == 0
        assert _matches(lib, m=0, ps=8 * 384, cnt=None, **kw) == 0      # (counts null: no device call)
        assert _matches(lib, m=0, n=0, ps=0, cnt=None, v=None, ws=None, **kw) == 0
        # ... but the limits still hold for an empty call
        assert _scores(lib, batch=0, n=12, **kw) == 1 and _matches(lib, batch=0, n=12, **kw) == 1


def test_library_exports_and_binds_the_new_symbols(lib):
    import re
    import subprocess

    from lightglue_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T ((?:lg|mha_hd64)_\w+)", out))
    for name in ("mha_hd64_launch_grouped_lens", "mha_hd64_launch_grouped_qkv_lens", "mha_hd64_launch_stream_lens",
                 "lg_assign_scores_lens", "lg_assign_matches_lens"):
        assert name in exported, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
    assert lib.lg_glue_abi_version() == _lib.GLUE_ABI_VERSION == 4   # new symbols only


def test_grouped_lens_op_is_registered_with_a_fake():
    """torch.ops.lightglue_amd.mha_hd64_grouped_lens traces on meta tensors (shapes and dtypes of the
    queries) and has no CPU kernel."""
    import lightglue_amd  # noqa: F401

    q = torch.empty((2, 4, 9, 64), dtype=torch.float16, device="meta")
    k = torch.empty((2, 4, 8, 64), dtype=torch.float16, device="meta")
    lens = torch.empty((2,), dtype=torch.int32, device="meta")
    out = torch.ops.lightglue_amd.mha_hd64_grouped_lens([q, k], [k, q], [k, q], [lens, lens])
    assert [tuple(o.shape) for o in out] == [(2, 4, 9, 64), (2, 4, 8, 64)] and out[0].dtype == torch.float16
    with pytest.raises((NotImplementedError, RuntimeError)):
        c = torch.zeros((1, 4, 8, 64), dtype=torch.float16)
        torch.ops.lightglue_amd.mha_hd64_grouped_lens([c], [c], [c], [torch.ones(1, dtype=torch.int32)])
