"""The match head's host side: the C ABI of lg_assign_matches (include/lightglue_glue.h) and the
framework restatement filter_matches_dense against the reference's golden matches.

Runs without a GPU: the argument checks of lg_assign_matches happen before any device call, and
filter_matches_dense runs on CPU tensors. (The kernels: tests/test_gpu_match_head.py.)
"""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
INDEX = json.load(open(os.path.join(GOLD, "matcher_index.json")))
CASES = sorted(INDEX)

A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def _call(lib, **kw):
    a = dict(v=A, ps=16 * 384, ld=384, zc=256, m=8, n=8, batch=1, th=0.1, m0=A, m1=A, s0=A, s1=A, mt=A, ms=A, cnt=A, ws=A)
    a.update(kw)
    return lib.lg_assign_matches(a["v"], a["ps"], a["ld"], a["zc"], a["m"], a["n"], a["batch"], a["th"], a["m0"], a["m1"],
                                 a["s0"], a["s1"], a["mt"], a["ms"], a["cnt"], a["ws"], None)


def test_library_exports_and_binds_the_match_head(lib):
    import re
    import subprocess

    from lightglue_amd import _lib

    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (lg_\w+)", out))
    for name in ("lg_assign_matches", "lg_assign_matches_workspace"):
        assert name in exported, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][0]
    assert lib.lg_glue_abi_version() == _lib.GLUE_ABI_VERSION == 4  # additions keep the version


def test_assign_matches_validates_before_touching_the_device(lib):
    """Every reject returns before a device call (this host has no GPU: a launch would fail with
    another status) and names the function in mha_hd64_last_error()."""
    from lightglue_amd import _lib

    bads = [dict(n=12), dict(m=2049, ps=(2049 + 8) * 384), dict(n=2056, ps=(8 + 2056) * 384), dict(zc=255), dict(zc=384),
            dict(zc=400), dict(ld=380), dict(v=None), dict(v=A + 8), dict(ws=None), dict(ws=A + 8), dict(ps=16 * 384 - 1),
            dict(m=-1), dict(batch=-1), dict(th=-0.5), dict(th=float("nan"))]
    bads += [{k: None} for k in ("m0", "m1", "s0", "s1", "mt", "ms", "cnt")]
    bads += [{k: A + 2} for k in ("m0", "m1", "s0", "s1", "mt", "ms", "cnt")]
    for bad in bads:
        assert _call(lib, **bad) == _lib.STATUS_BAD_PARAM, bad
        assert "lg_assign_matches" in _lib.last_error(), bad
    # nothing to do: success without a launch (m or n == 0 only zeroes counts: null here, so no device call)
    assert _call(lib, batch=0) == 0
    assert _call(lib, batch=0, v=None, ws=None, m0=None, cnt=None) == 0
    assert _call(lib, m=0, ps=8 * 384, cnt=None) == 0
    assert _call(lib, n=0, ps=8 * 384, cnt=None) == 0
    assert _call(lib, m=0, n=0, ps=0, cnt=None, v=None, ws=None) == 0
    # ... but the limits still hold for an empty call
    assert _call(lib, batch=0, n=12) == _lib.STATUS_BAD_PARAM


def test_assign_matches_workspace(lib):
    ws, base = lib.lg_assign_matches_workspace, lib.lg_assign_scores_workspace
    for m, n in ((1, 8), (33, 72), (300, 296), (520, 72), (2048, 2048)):
        prev = 0
        for batch in (1, 2, 3, 16):
            got = ws(m, n, batch)
            # the lg_assign_scores layout first (assign_lse_kernel runs unchanged), then per pair a (max, index)
            # of 8 B per row and 512-column block and per column and 32-row strip
            extra = batch * 8 * (-(-n // 512) * m + -(-m // 32) * n)
            assert base(m, n, batch) + extra <= got <= base(m, n, batch) + extra + 512, (m, n, batch)
            assert got % 16 == 0 and got > prev, (m, n, batch)
            prev = got
    for m, n, batch in ((0, 8, 1), (8, 0, 1), (8, 8, 0), (-1, 8, 1), (8, -8, 1), (8, 8, -1)):
        assert ws(m, n, batch) == 0


# ---- filter_matches_dense against the reference's matches ----
def _gold(name):
    return np.load(os.path.join(GOLD, f"{name}.npz"))


def _consistent(r, p=0):
    """matches0 / matches1 point at each other and scores1 follows scores0."""
    m0, m1, s0, s1 = (t[p].numpy() for t in (r.matches0, r.matches1, r.scores0, r.scores1))
    i = np.nonzero(m0 >= 0)[0]
    assert (m1[m0[i]] == i).all()
    assert int((m0 >= 0).sum()) == int((m1 >= 0).sum()) == int(r.counts[p])
    j = np.nonzero(m1 >= 0)[0]
    assert (s1[j] == s0[m1[j]]).all()
    assert ((m0 >= -1) & (m0 < len(m1))).all() and ((m1 >= -1) & (m1 < len(m0))).all()


@pytest.mark.parametrize("name", CASES)
def test_filter_matches_dense_matches_reference(name):
    from lightglue_amd.matcher import MatchResult, filter_matches_dense

    g = _gold(name)
    sc = torch.from_numpy(g["scores"])
    for th, key, skey in ((0.1, "matches", "mscores"), (0.0, "matches_all", "mscores_all")):
        r = filter_matches_dense(sc, th)
        assert isinstance(r, MatchResult) and r._fields == ("matches0", "matches1", "scores0", "scores1", "matches",
                                                            "match_scores", "counts")
        k = min(sc.shape[1], sc.shape[2])
        assert r.matches.shape == (1, k, 2) and r.match_scores.shape == (1, k) and r.counts.shape == (1,)
        assert all(t.dtype == torch.int32 for t in (r.matches0, r.matches1, r.matches, r.counts))
        c = int(r.counts[0])
        assert c == len(g[key])
        assert (r.matches[0, :c].numpy() == g[key]).all()                      # in order (ascending i)
        assert np.abs(r.match_scores[0, :c].numpy() - g[skey]).max(initial=0.0) <= 1e-6
        assert (r.matches[0, c:] == -1).all() and (r.match_scores[0, c:] == 0).all()
        _consistent(r)
        # the dense row side restates the list
        m0 = r.matches0[0].numpy()
        assert (np.nonzero(m0 >= 0)[0] == g[key][:, 0]).all() and (m0[m0 >= 0] == g[key][:, 1]).all()


@pytest.mark.parametrize("name", CASES)
def test_filter_matches_dense_batched_equals_per_pair(name):
    """P = 2 in one call equals filter_matches pair by pair. (The fixtures have three different
    shapes, so the second pair is the fixture's assignment with rows and columns reversed: another
    assignment of the same shape, with other matches at other positions.)"""
    from lightglue_amd.matcher import filter_matches, filter_matches_dense

    sc = torch.from_numpy(_gold(name)["scores"])
    both = torch.cat([sc, sc.flip(1, 2)], 0).contiguous()
    for th in (0.1, 0.0):
        r = filter_matches_dense(both, th)
        for p in range(2):
            m, s = filter_matches(both[p:p + 1], th)
            c = int(r.counts[p])
            assert c == len(m)
            assert (r.matches[p, :c].long() == m).all() and (r.match_scores[p, :c] == s).all()
            assert (r.matches[p, c:] == -1).all() and (r.match_scores[p, c:] == 0).all()
            _consistent(r, p)
    assert int(r.counts[0]) == int(r.counts[1]) > 0   # (th = 0: the reversed pair has the mirrored matches)


def test_ties_go_to_the_lowest_index_and_padding():
    from lightglue_amd.matcher import filter_matches_dense

    r = filter_matches_dense(torch.full((1, 40, 72), -3.0), 0.0)
    want0 = np.full(40, -1)
    want1 = np.full(72, -1)
    want0[0] = want1[0] = 0
    assert (r.matches0[0].numpy() == want0).all() and (r.matches1[0].numpy() == want1).all()
    assert int(r.counts[0]) == 1 and r.matches[0, 0].tolist() == [0, 0]
    assert float(r.match_scores[0, 0]) == float(torch.tensor(-3.0).exp()) == float(r.scores0[0, 0]) == float(r.scores1[0, 0])
    assert (r.matches[0, 1:] == -1).all() and (r.match_scores[0, 1:] == 0).all()
    assert (r.scores0[0, 1:] == 0).all() and (r.scores1[0, 1:] == 0).all()
    # a tie inside a row and inside a column, away from index 0
    sc = torch.full((1, 5, 8), -9.0)
    sc[0, 3, 2] = sc[0, 3, 6] = sc[0, 4, 2] = -1.0
    r = filter_matches_dense(sc, 0.0)
    assert r.matches0[0].tolist() == [0, -1, -1, 2, -1] and int(r.counts[0]) == 2
    assert r.matches[0].tolist() == [[0, 0], [3, 2], [-1, -1], [-1, -1], [-1, -1]]
    assert r.matches1[0].tolist() == [0, -1, 3, -1, -1, -1, -1, -1]
    # nothing above the threshold, and empty sides
    r = filter_matches_dense(sc, 1.0)
    assert int(r.counts[0]) == 0 and (r.matches == -1).all() and (r.matches0 == -1).all() and (r.matches1 == -1).all()
    r = filter_matches_dense(torch.zeros((2, 0, 8)), 0.1)
    assert r.counts.tolist() == [0, 0] and r.matches.shape == (2, 0, 2) and (r.matches1 == -1).all()
    with pytest.raises(ValueError):
        filter_matches_dense(sc, -0.1)
