"""Adaptive depth and width, host side (no GPU): the published LightGlue rules (per-layer thresholds,
the exit ratio, the keep flags and the min-one rule), adaptive_reference on the framework path with the
oracle attention (a 3-layer seeded model, pairs of 64 x 48 and 120 x 97 with overlap), the state-dict
contract, the mapping back to original indices, and the argument checks of the three C entry points
(include/lightglue_glue.h: lg_token_scores, lg_compact_rows, lg_matches_scatter), which all happen
before any device call. (The kernels and match_adaptive's fast path: tests/test_gpu_adaptive.py.)

The knobs below were found with adaptive_reference itself on this model (fp32, CPU): with the
confidence weights of seed 10, layer 1 leaves 84 of 112 and 180 of 217 rows unconfident (confident shares
0.25 and 0.17, none at layer 0), so depth_confidence = 0.1 stops after two layers; the matchability of
layer 0 has its median near 0.4, so width_confidence = 0.6 (keep mtch > 0.4) drops 10-20 % of every
segment at layer 0 and again at layer 1. With both knobs and depth_confidence = 0.3 no pair passes the
exit and layer 1 prunes its confident rows of low matchability (64 x 48 -> 62 x 44, 120 x 97 -> 112 x 94).
"""
import ctypes
import functools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

SIZES = [(64, 48), (120, 97)]
L = 3
CONF_SEED = 10
DEPTH, WIDTH = 0.1, 0.6
BOTH_DEPTH = 0.3   # (both knobs: above layer 1's confident shares, so that its confident rows are pruned, not an exit)
FIELDS = ("matches0", "matches1", "scores0", "scores1", "matches", "match_scores", "counts")
A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below


def _oracle_attention(calls):
    from oracle import oracle

    return [oracle.attention_torch(q, k, v) for q, k, v in calls]


@functools.lru_cache(maxsize=None)
def _batch():
    from lightglue_amd import matcher

    pairs = [matcher.synthetic_pair(70 + i, m, n, overlap=min(m, n) // 2) for i, (m, n) in enumerate(SIZES)]
    m, n = max(a for a, _ in SIZES), max(b for _, b in SIZES)
    out = []
    for j, size in enumerate((m, n, m, n)):
        t = torch.zeros((len(pairs), size, pairs[0][j].shape[-1]))
        for p, pair in enumerate(pairs):
            t[p, :pair[j].shape[1]] = pair[j][0]
        out.append(t)
    return tuple(out), [a for a, _ in SIZES], [b for _, b in SIZES]


@functools.lru_cache(maxsize=None)
def _run(depth, width):
    """(model, AdaptiveResult, trace) of adaptive_reference: computed once per knob pair, read-only."""
    from lightglue_amd import matcher

    model = matcher.LightGlueMatcher(n_layers=L, attention=_oracle_attention, glue="torch", depth_confidence=depth,
                                     width_confidence=width).eval()
    sd = matcher.seeded_state_dict(11, L)
    if model.adaptive:
        sd.update(matcher.seeded_confidence_state_dict(CONF_SEED, L))
    model.load_state_dict(sd, strict=True)
    batch, c0, c1 = _batch()
    trace = []
    with torch.no_grad():
        res = matcher.adaptive_reference(model, *batch, counts0=c0, counts1=c1, trace=trace)
    return model, res, trace


def test_threshold_table():
    from lightglue_amd.matcher import adaptive_thresholds

    for n_layers in (1, 3, 9):
        got = adaptive_thresholds(n_layers)
        assert len(got) == n_layers
        for i, t in enumerate(got):
            assert t == min(max(0.8 + 0.1 * math.exp(-4.0 * i / n_layers), 0.0), 1.0)
    assert adaptive_thresholds(9)[0] == 0.9 and all(0.8 < t <= 0.9 for t in adaptive_thresholds(9))


def test_exit_ratio_is_strict():
    from lightglue_amd.matcher import exit_passes

    # 1 - unconfident / valid > depth_confidence, strictly
    assert exit_passes(1, 4, 0.7) and not exit_passes(1, 4, 0.75) and not exit_passes(2, 4, 0.5)
    assert exit_passes(0, 5, 0.99) and not exit_passes(5, 5, 0.0 + 1e-9)
    # "unconfident" is conf < t, strictly: a row exactly at the threshold counts as confident
    t = float(np.float32(0.9))
    conf = torch.tensor([t, np.nextafter(np.float32(t), np.float32(0)), 0.95], dtype=torch.float32)
    assert int((conf < t).sum()) == 1


def test_keep_rule():
    from lightglue_amd.matcher import keep_rule

    f = lambda *v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    lim = float(np.float32(1.0 - 0.75))  # keep mtch > float32(0.25), strictly
    mtch = f(0.1, lim, float(np.nextafter(np.float32(lim), np.float32(1))), 0.9)
    conf = f(0.5, 0.95, 0.95, 0.5)
    # width only: the matchability alone
    assert keep_rule(conf, mtch, 0.9, -1.0, 0.75).tolist() == [False, False, True, True]
    # with depth: an unconfident row (conf <= t, the threshold itself included) is kept whatever its matchability
    t = float(np.float32(0.9))
    conf = f(0.5, t, float(np.nextafter(np.float32(t), np.float32(1))), 0.95)
    assert keep_rule(conf, f(0.1, 0.1, 0.1, 0.9), 0.9, 0.5, 0.75).tolist() == [True, True, False, True]
    # min-one: nothing kept -> the highest matchability, the lowest index on ties
    assert keep_rule(f(1, 1, 1, 1), f(0.1, 0.2, 0.2, 0.05), 0.9, 0.5, 0.75).tolist() == [False, True, False, False]
    assert keep_rule(f(1, 1), f(0.0, 0.0), 0.9, -1.0, 0.75).tolist() == [True, False]
    assert keep_rule(f(1.0), f(0.0), 0.9, -1.0, 0.75).tolist() == [True]


def test_compact_dims():
    from lightglue_amd.matcher import compact_dims

    assert compact_dims([5, 9, 3], [7, 4, 3]) == (9, 8) and compact_dims([1], [8]) == (1, 8) and compact_dims([1], [9]) == (1, 16)


def test_knobs_off_equals_match_batch():
    from lightglue_amd import matcher

    model, res, trace = _run(-1.0, -1.0)
    batch, c0, c1 = _batch()
    with torch.no_grad():
        want = model.match_batch(*batch, counts0=c0, counts1=c1)
        via = model.match_adaptive(*batch, counts0=c0, counts1=c1)
    assert res.stop == via.stop == L and res.prune0 is None and via.prune1 is None and trace == []
    assert int(want.counts.sum()) >= 1
    for f in FIELDS:
        assert torch.equal(getattr(res.result, f), getattr(want, f)), f
        assert torch.equal(getattr(via.result, f), getattr(want, f)), f
    assert isinstance(res, matcher.AdaptiveResult) and res.result._fields == FIELDS


def test_full_depth_loop_equals_match_batch():
    """depth_confidence = 1.0 with width off: 1 - unconfident / valid > 1.0 never holds and nothing is
    pruned, so the adaptive loop (not the knobs-off shortcut) runs all L layers and must give match_batch."""
    from lightglue_amd import matcher

    model, res, trace = _run(1.0, -1.0)
    batch, c0, c1 = _batch()
    m, n = batch[0].shape[1], batch[1].shape[1]
    with torch.no_grad():
        want = model.match_batch(*batch, counts0=c0, counts1=c1)
        via = model.match_adaptive(*batch, counts0=c0, counts1=c1)
    assert model.adaptive and res.stop == via.stop == L == 3
    assert len(trace) == 2 and all(e["stop"] is False and e["dims"] == (120, 97) for e in trace)
    for r in (res, via):
        for prune, counts, size in ((r.prune0, c0, m), (r.prune1, c1, n)):
            valid = torch.arange(size)[None] < torch.tensor(counts)[:, None]
            assert torch.equal(prune, torch.where(valid, 3, 0).to(torch.int32))
        for f in FIELDS:
            assert torch.equal(getattr(r.result, f), getattr(want, f)), f
    assert int(want.counts.sum()) >= 1
    assert isinstance(via, matcher.AdaptiveResult)


def test_state_dict_contract():
    from lightglue_amd import matcher

    plain = matcher.LightGlueMatcher(n_layers=L)
    assert not any("token_confidence" in k for k in plain.state_dict())
    assert set(plain.state_dict()) == set(matcher.seeded_state_dict(11, L))
    for kw in (dict(depth_confidence=0.9), dict(width_confidence=0.9), dict(depth_confidence=0.9, width_confidence=0.9)):
        keys = [k for k in matcher.LightGlueMatcher(n_layers=L, **kw).state_dict() if "token_confidence" in k]
        want = [f"token_confidence.{i}.token.0.{w}" for i in range(L - 1) for w in ("weight", "bias")]
        assert sorted(keys) == sorted(want)
    sd = matcher.seeded_confidence_state_dict(CONF_SEED, L)
    assert sorted(sd) == sorted(want) and tuple(sd[want[0]].shape) == (1, 256) and tuple(sd[want[1]].shape) == (1,)
    again = matcher.seeded_confidence_state_dict(CONF_SEED, L)
    assert all(torch.equal(sd[k], again[k]) for k in sd)
    assert not torch.equal(sd[want[0]], matcher.seeded_confidence_state_dict(CONF_SEED + 1, L)[want[0]])


def _check_mapping(res, trace, c0, c1):
    r, stop = res.result, res.stop
    m, n = r.matches0.shape[1], r.matches1.shape[1]
    for p, (a, b) in enumerate(zip(c0, c1)):
        live0 = set(trace[-1]["kept0"][p].tolist()) if trace else set(range(a))
        live1 = set(trace[-1]["kept1"][p].tolist()) if trace else set(range(b))
        assert live0 <= set(range(a)) and live1 <= set(range(b))
        m0, m1 = r.matches0[p].tolist(), r.matches1[p].tolist()
        for i in range(m):
            if i not in live0:   # pruned or padded: -1 / 0
                assert m0[i] == -1 and float(r.scores0[p, i]) == 0.0
            elif m0[i] >= 0:     # mutually consistent, and between surviving rows
                assert m0[i] in live1 and m1[m0[i]] == i and float(r.scores0[p, i]) == float(r.scores1[p, m0[i]])
        for j in range(n):
            if j not in live1:
                assert m1[j] == -1 and float(r.scores1[p, j]) == 0.0
            elif m1[j] >= 0:
                assert m1[j] in live0 and m0[m1[j]] == j
        c = int(r.counts[p])
        lst = r.matches[p, :c].tolist()
        assert lst == [[i, m0[i]] for i in range(m) if m0[i] >= 0] and (r.matches[p, c:] == -1).all()
        assert (r.match_scores[p, c:] == 0).all()
        # prune: the layers a point took part in
        p0, p1 = res.prune0[p].tolist(), res.prune1[p].tolist()
        assert all(p0[i] == stop for i in live0) and all(p1[j] == stop for j in live1)
        assert all(1 <= p0[i] <= stop for i in range(a)) and all(1 <= p1[j] <= stop for j in range(b))
        assert all(v == 0 for v in p0[a:]) and all(v == 0 for v in p1[b:])
        for e in trace:          # a point dropped at layer i took part in i + 1 layers
            if e["stop"]:
                continue
            gone0 = [i for i in range(a) if p0[i] == e["layer"] + 1]
            assert not set(gone0) & set(e["kept0"][p].tolist())
            assert len(e["kept0"][p]) == e["stats"][p][0] and len(e["kept1"][p]) == e["stats"][p][1]


def test_width_only_prunes_and_maps_back():
    _, res, trace = _run(-1.0, WIDTH)
    _, c0, c1 = _batch()
    assert res.stop == L and len(trace) == L - 1 and not any(e["stop"] for e in trace)
    lost = [1 - e["stats"][p][0] / (c0[p] if e["layer"] == 0 else trace[e["layer"] - 1]["stats"][p][0])
            for e in trace for p in range(len(SIZES))]
    assert all(0.05 <= x <= 0.9 for x in lost), lost    # (not vacuous: every layer drops rows of image 0)
    assert int(res.result.counts.min()) >= 1
    assert {1, 2, 3} <= set(res.prune0[1].tolist())    # rows pruned at different layers, and survivors
    _check_mapping(res, trace, c0, c1)


def test_depth_only_stops_early():
    from lightglue_amd.matcher import exit_passes

    model, res, trace = _run(DEPTH, -1.0)
    _, c0, c1 = _batch()
    assert res.stop == 2 and [e["stop"] for e in trace] == [False, True]
    for e in trace:
        assert e["stop"] == all(exit_passes(s[2], s[3], DEPTH) for s in e["stats"])
        assert [s[:2] + s[3:] for s in e["stats"]] == [[a, b, a + b] for a, b in zip(c0, c1)]   # nothing pruned
    assert int(res.result.counts.min()) >= 1
    _check_mapping(res, trace, c0, c1)
    # the head is the stop layer's: the plain model cut to two layers gives the same matches
    from lightglue_amd import matcher

    cut = matcher.LightGlueMatcher(n_layers=2, attention=_oracle_attention, glue="torch").eval()
    cut.load_state_dict({k: v for k, v in model.state_dict().items() if k in cut.state_dict()}, strict=True)
    batch, _, _ = _batch()
    with torch.no_grad():
        want = cut.match_batch(*batch, counts0=c0, counts1=c1)
    for f in FIELDS:
        assert torch.equal(getattr(res.result, f), getattr(want, f)), f


def test_both_knobs_and_following_a_trace():
    from lightglue_amd import matcher

    model, res, trace = _run(BOTH_DEPTH, WIDTH)
    batch, c0, c1 = _batch()
    # with depth on an unconfident row is never pruned: layer 0 (no confident row) keeps everything that
    # width alone drops there, layer 1 drops confident rows of low matchability; no pair passes the exit
    assert res.stop == L and [s[:2] for s in trace[0]["stats"]] == [list(t) for t in zip(c0, c1)]
    assert all(s[0] < a and s[1] < b for s, a, b in zip(trace[1]["stats"], c0, c1))
    assert _run(-1.0, WIDTH)[2][0]["stats"][1][0] < c0[1]
    _check_mapping(res, trace, c0, c1)
    # decisions=: the recorded keep sets and stop layer instead of the run's own scores
    with torch.no_grad():
        again = matcher.adaptive_reference(model, *batch, counts0=c0, counts1=c1, decisions=trace)
    assert again.stop == res.stop and torch.equal(again.prune0, res.prune0) and torch.equal(again.prune1, res.prune1)
    for f in FIELDS:
        assert torch.equal(getattr(again.result, f), getattr(res.result, f)), f
    # match_adaptive off the fast path (glue='torch', a substituted attention) is adaptive_reference
    with torch.no_grad():
        via = model.match_adaptive(*batch, counts0=c0, counts1=c1)
    for f in FIELDS:
        assert torch.equal(getattr(via.result, f), getattr(res.result, f)), f


def test_scatter_restatement_by_hand():
    """scatter_matches_reference on a hand-built case: 2 surviving rows x 3 surviving columns of 5 x 4."""
    from lightglue_amd.matcher import MatchResult, scatter_matches_reference

    i32 = lambda v: torch.tensor(v, dtype=torch.int32)   # noqa: E731
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)  # noqa: E731
    r = MatchResult(i32([[2, -1, 7]]), i32([[-1, -1, 0, 9]]), f32([[0.5, 0.0, 9.0]]), f32([[0.0, 0.0, 0.5, 9.0]]),
                    i32([[[0, 2], [-1, -1], [-1, -1]]]), f32([[0.5, 0.0, 0.0]]), i32([1]))
    p0, p1 = torch.tensor([[0, 1, 0, 2, 0]], dtype=torch.int32), torch.zeros((1, 4), dtype=torch.int32)
    out = scatter_matches_reference(r, i32([[1, 4, 0]]), i32([[0, 2, 3, 1]]), [2], [3], 5, 4, 3, p0, p1)
    assert out.matches0.tolist() == [[-1, 3, -1, -1, -1]] and out.matches1.tolist() == [[-1, -1, -1, 1]]
    assert out.scores0.tolist() == [[0, 0.5, 0, 0, 0]] and out.scores1.tolist() == [[0, 0, 0, 0.5]]
    assert out.matches.tolist() == [[[1, 3], [-1, -1], [-1, -1], [-1, -1]]] and out.counts.tolist() == [1]
    assert p0.tolist() == [[0, 3, 0, 2, 3]] and p1.tolist() == [[3, 0, 3, 3]]


# ---- the C entry points ----
@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def _scores(lib, **kw):
    a = dict(x=A, m=8, n=8, pairs=1, ml=A, nl=A, wt=A, bt=A, wm=A, bm=A, tc=0.9, tk=0.5, flags=7, conf=A, mtch=A, keep=A,
             stats=A)
    a.update(kw)
    return lib.lg_token_scores(a["x"], a["m"], a["n"], a["pairs"], a["ml"], a["nl"], a["wt"], a["bt"], a["wm"], a["bm"],
                               a["tc"], a["tk"], a["flags"], a["conf"], a["mtch"], a["keep"], a["stats"], None)


def _compact(lib, **kw):
    a = dict(x=A, cos=A, sin=A, keep=A, i0=A, i1=A, m=8, n=8, pairs=1, ml=A, nl=A, mo=4, no=8, xo=2 * A, co=2 * A, so=2 * A,
             i0o=A, i1o=A, mlo=A, nlo=A, p0=A, p1=A, pm=8, pn=8, layers=1)
    a.update(kw)
    return lib.lg_compact_rows(a["x"], a["cos"], a["sin"], a["keep"], a["i0"], a["i1"], a["m"], a["n"], a["pairs"], a["ml"],
                               a["nl"], a["mo"], a["no"], a["xo"], a["co"], a["so"], a["i0o"], a["i1o"], a["mlo"], a["nlo"],
                               a["p0"], a["p1"], a["pm"], a["pn"], a["layers"], None)


_SC_IN = ("m0", "m1", "s0", "s1", "mt", "ms", "cnt")
_SC_OUT = ("om0", "om1", "os0", "os1", "omt", "oms", "ocnt")


def _scatter(lib, **kw):
    a = dict({k: A for k in _SC_IN + _SC_OUT}, i0=A, i1=A, ml=A, nl=A, mc=4, nc=8, m=8, n=8, pairs=1, stop=3, p0=A, p1=A)
    a.update(kw)
    return lib.lg_matches_scatter(*(a[k] for k in _SC_IN), a["i0"], a["i1"], a["ml"], a["nl"], a["mc"], a["nc"], a["m"], a["n"],
                                  a["pairs"], a["stop"], *(a[k] for k in _SC_OUT), a["p0"], a["p1"], None)


def test_entry_points_validate_before_touching_the_device(lib):
    """Every reject returns BAD_PARAM before a device call (this host has no GPU: a launch would fail
    with another status); pairs == 0 is a no-op."""
    from lightglue_amd import _lib

    BAD = _lib.STATUS_BAD_PARAM
    bads = [dict(m=0), dict(n=-1), dict(pairs=-1), dict(pairs=70000), dict(tc=1.5), dict(tc=-0.1), dict(tc=float("nan")),
            dict(tk=float("nan")), dict(flags=8), dict(flags=-1), dict(ml=A + 2), dict(nl=A + 1), dict(conf=A + 2),
            dict(mtch=A + 1),
            dict(stats=A + 2), dict(x=A + 8), dict(wt=A + 8), dict(wm=A + 4), dict(bt=A + 1), dict(bm=A + 1)]
    bads += [{k: None} for k in ("x", "wt", "bt", "wm", "bm", "conf", "mtch", "keep", "stats")]
    for bad in bads:
        assert _scores(lib, **bad) == BAD, bad
        assert "lg_token_scores" in _lib.last_error(), bad
    assert _scores(lib, pairs=0) == 0 and _scores(lib, pairs=0, ml=None, nl=None) == 0

    bads = [dict(m=0), dict(n=0), dict(pairs=-1), dict(mo=0), dict(no=0), dict(mo=9), dict(no=9), dict(xo=A), dict(co=A),
            dict(so=A), dict(p0=None), dict(p1=None), dict(pm=0), dict(pn=0), dict(layers=0), dict(ml=A + 2), dict(nl=A + 2),
            dict(i0=A + 2), dict(i1=A + 1), dict(p0=A + 2)]
    bads += [{k: None} for k in ("x", "cos", "sin", "keep", "xo", "co", "so", "i0o", "i1o", "mlo", "nlo")]
    bads += [{k: A + 8} for k in ("x", "cos", "sin")] + [{k: 2 * A + 8} for k in ("xo", "co", "so")]
    bads += [{k: A + 2} for k in ("i0o", "i1o", "mlo", "nlo")]
    for bad in bads:
        assert _compact(lib, **bad) == BAD, bad
        assert "lg_compact_rows" in _lib.last_error(), bad
    assert _compact(lib, pairs=0) == 0 and _compact(lib, pairs=0, i0=None, i1=None, ml=None, nl=None, p0=None, p1=None) == 0

    bads = [dict(mc=0), dict(nc=0), dict(mc=9), dict(nc=16), dict(m=2049, mc=2049), dict(n=2056), dict(pairs=-1), dict(stop=-1)]
    bads += [{k: None} for k in _SC_IN + _SC_OUT] + [{k: A + 2} for k in _SC_IN + _SC_OUT]
    bads += [{k: A + 2} for k in ("i0", "i1", "ml", "nl", "p0", "p1")]
    for bad in bads:
        assert _scatter(lib, **bad) == BAD, bad
        assert "lg_matches_scatter" in _lib.last_error(), bad
    assert _scatter(lib, pairs=0) == 0 and _scatter(lib, pairs=0, i0=None, i1=None, ml=None, nl=None, p0=None, p1=None) == 0


def test_library_exports_and_binds_the_new_symbols(lib):
    import re
    import subprocess

    from lightglue_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T ((?:lg|mha_hd64)_\w+)", out))
    for name in ("lg_token_scores", "lg_compact_rows", "lg_matches_scatter"):
        assert name in exported, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0] and getattr(lib, name).restype is ctypes.c_int32
    assert lib.lg_glue_abi_version() == _lib.GLUE_ABI_VERSION == 4   # new symbols only
    assert (_lib.ADAPT_DEPTH, _lib.ADAPT_WIDTH0, _lib.ADAPT_WIDTH1) == (1, 2, 4)


def test_package_exports():
    import lightglue_amd

    for name in ("AdaptiveResult", "adaptive_reference", "adaptive_thresholds", "seeded_confidence_state_dict"):
        assert name in lightglue_amd.__all__ and hasattr(lightglue_amd, name)
