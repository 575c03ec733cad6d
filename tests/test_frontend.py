"""Keypoint front end, CPU side: frontend_reference (the GPU tests' oracle) against the reference's golden
outputs, the fixtures' asserted conditions re-checked from the files, the C exports and every entry point's
argument refusals (checked before any device call, so they run without a GPU)."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR, REPO

NAMES = ("8x8", "9x17", "11x10")
ENTRY_POINTS = ("lg_kp_heatmap", "lg_kp_nms", "lg_kp_select_workspace", "lg_kp_select", "lg_kp_describe")
A = 4096  # a fake 16-B aligned address: never dereferenced on the paths below


def load(name):
    with np.load(os.path.join(GOLDEN_DIR, f"frontend_{name}.npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module", params=NAMES)
def g(request):
    return load(request.param)


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("make_frontend_golden",
                                                  os.path.join(GOLDEN_DIR, "make_frontend_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from lightglue_amd import _lib

    return _lib.load()


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def test_fixture_conditions_hold(g, gen):
    """Distinct candidate scores, K_main strictly between the two images' counts, the three end-to-end gaps
    >= 64 x the reference's fp32 heatmap error, the tie K inside a run of equal scores, border-0 keypoints
    whose sampling corners leave the map."""
    gen.check_conditions(g)


def test_fixtures_stay_small():
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN_DIR, f"frontend_{name}.npz")) < 512 * 1024


def test_heatmap_reference(g):
    from lightglue_amd import frontend

    logits = t(g["logits"])
    exact = frontend.heatmap_reference(logits.double())
    assert float((t(g["heat32"]).double() - exact).abs().max()) == pytest.approx(float(g["heat_err"]), rel=1e-6)
    got = frontend.heatmap_reference(logits)
    assert got.dtype == torch.float32 and float((got.double() - exact).abs().max()) <= 4 * float(g["heat_err"])
    half = frontend.heatmap_reference(logits.half())
    assert half.dtype == torch.float32 and float((half - got).abs().max()) < 2e-3


def test_nms_reference_is_bitwise_the_reference(g):
    from lightglue_amd import frontend

    heat = t(g["heat32"])
    assert torch.equal(frontend.nms_reference(heat, 0), heat)
    for r in (1, 4):
        assert torch.equal(frontend.nms_reference(heat, r), t(g[f"nms_r{r}"])), r
    for r in (0, 1, 4):
        for lv in (32, 64):
            q = t(g[f"q{lv}_levels"]).float() / lv
            assert torch.equal(frontend.nms_reference(q, r), t(g[f"q{lv}_nms_r{r}"])), (lv, r)
        assert torch.equal(frontend.nms_reference(t(g["special"]), r), t(g[f"special_nms_r{r}"])), r


def select_cases(g):
    k = int(g["k_main"])
    return ((4, k), (0, k), (4, 8), (4, 2048))


def test_select_reference(g):
    from lightglue_amd import frontend

    nms4 = t(g["nms_r4"])
    for border, k in select_cases(g):
        count, pix, score = frontend.select_reference(nms4, k, 0.0005, border)
        tag = f"sel_b{border}_k{k}"
        assert torch.equal(count, t(g[tag + "_count"])) and torch.equal(pix, t(g[tag + "_pix"])), tag
        assert torch.equal(score, t(g[tag + "_score"])), tag


def test_select_reference_tie_rule(g):
    """On the quantised map the K cut falls inside a run of equal scores: descending score, ties by
    ascending pixel index, checked from first principles."""
    from lightglue_amd import frontend

    q = t(g["q64_nms_r4"])
    k = int(g["tie_k"])
    count, pix, score = frontend.select_reference(q, k, 0.0005, 4)
    for i in range(q.shape[0]):
        n = int(count[i])
        p, s = pix[i, :n].long(), score[i, :n]
        assert torch.equal(q[i].reshape(-1)[p], s)
        assert bool(((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (p[:-1] < p[1:]))).all())
        y, x = p // q.shape[2], p % q.shape[2]
        assert bool(((y >= 4) & (y < q.shape[1] - 4) & (x >= 4) & (x < q.shape[2] - 4)).all())
        inner = torch.zeros_like(q[i], dtype=torch.bool)
        inner[4:-4, 4:-4] = True
        rest = q[i].clone()
        rest.reshape(-1)[p] = 0
        left = rest[inner & (rest > 0.0005)]
        if left.numel():  # nothing left out beats the last one kept, and an equal one has a higher index
            assert n == k and float(left.max()) <= float(s[-1])
            eq = torch.nonzero((rest.reshape(-1) == s[-1]) & inner.reshape(-1))[:, 0]
            assert eq.numel() == 0 or int(eq.min()) > int(p[s == s[-1]].max())
        assert bool((pix[i, n:] == -1).all()) and bool((score[i, n:] == 0).all())


def test_describe_reference(g):
    """fp32 against the fp64 restatement within 4 x the reference's own fp32 error; padded rows zero; kpts
    and kpts_px exact."""
    from lightglue_amd import frontend

    dense = t(g["dense"]).float()
    k = int(g["k_main"])
    h, w = g["heat32"].shape[1:]
    for bi, border in enumerate((0, 4)):
        count, pix = t(g[f"sel_b{border}_k{k}_count"]), t(g[f"sel_b{border}_k{k}_pix"])
        for ni, dn in enumerate((False, True)):
            src = F.normalize(dense, p=2, dim=1) if dn else dense
            exact = frontend.describe_reference(src.double(), count, pix, dn, compute=torch.float64)
            got = frontend.describe_reference(src, count, pix, dn)
            assert float((got[0].double() - exact[0]).abs().max()) <= 4 * float(g["desc_err"][bi, ni])
            valid = torch.arange(k)[None, :] < count[:, None]
            assert bool((got[0][~valid] == 0).all()) and bool((got[1][~valid] == 0).all()) and bool((got[2][~valid] == 0).all())
            p = pix.clamp_min(0).long()
            xy = torch.stack([p % w, p // w], -1)
            assert torch.equal(got[1][valid], xy[valid].int())
            want = (xy.float() - torch.tensor([w / 2, h / 2])) / (max(w, h) / 2)
            assert torch.equal(got[2][valid], want[valid])


def test_frontend_reference_end_to_end(g):
    from lightglue_amd import frontend

    k = int(g["k_main"])
    f = frontend.frontend_reference(t(g["logits"]), t(g["dense"]), max_keypoints=k, dtype=torch.float32)
    w = g["heat32"].shape[2]
    assert torch.equal(f.counts, t(g[f"sel_b4_k{k}_count"]))
    assert torch.equal(f.kpts_px[..., 1] * w + f.kpts_px[..., 0], t(g[f"sel_b4_k{k}_pix"]).clamp_min(0))
    assert f.desc.shape == (2, k, 256) and f.desc.dtype == torch.float32
    norm = f.desc.norm(dim=-1)
    valid = torch.arange(k)[None, :] < f.counts[:, None]
    assert bool(((norm[valid] - 1).abs() < 1e-5).all()) and bool((norm[~valid] == 0).all())
    f16 = frontend.frontend_reference(None, t(g["dense"]), scores=t(g["heat32"]), max_keypoints=k)
    assert f16.desc.dtype == torch.float16 and torch.equal(f16.kpts_px, f.kpts_px)


def test_exports_are_declared_and_bound(lib):
    from lightglue_amd import _lib
    import lightglue_amd

    header = open(os.path.join(REPO, "include", "lightglue_glue.h")).read()
    src = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in lightglue_glue.h"
    assert "#define LG_GLUE_ABI_VERSION 4" in header and lib.lg_glue_abi_version() == 4
    for name in ("Features", "KeypointFrontend", "frontend_reference"):
        assert hasattr(lightglue_amd, name)
    assert lightglue_amd.Features._fields == ("kpts_px", "kpts", "desc", "scores", "counts")
    assert hasattr(lightglue_amd.matcher.LightGlueMatcher, "match_features")


def _rejects(lib, who, call, bads):
    from lightglue_amd import _lib

    for bad in bads:
        assert call(**bad) == 1, (who, bad)
        assert who in _lib.last_error(), (who, bad, _lib.last_error())


def test_entry_points_validate_before_touching_the_device(lib):
    """batch == 0 is a no-op (even with every other argument valid only in form); every clause of the
    argument checks rejects with last_error naming the function, without a device call."""
    def heat(**kw):
        a = dict(dt=0, x=A, hc=8, wc=8, b=0, out=A)
        a.update(kw)
        return lib.lg_kp_heatmap(a["dt"], a["x"], a["hc"], a["wc"], a["b"], a["out"], None)

    assert heat() == 0 and heat(dt=1, x=A + 2) == 0
    _rejects(lib, "lg_kp_heatmap", heat, [dict(dt=2), dict(dt=-1), dict(x=None), dict(out=None), dict(out=A + 4),
                                         dict(x=A + 2), dict(dt=1, x=A + 1), dict(hc=0), dict(wc=0), dict(hc=-1),
                                         dict(b=-1), dict(b=65536), dict(hc=2048, wc=2048), dict(b=1, x=None)])

    def nms(**kw):
        a = dict(x=A, h=64, w=64, b=0, r=4, out=A + 16)
        a.update(kw)
        return lib.lg_kp_nms(a["x"], a["h"], a["w"], a["b"], a["r"], a["out"], None)

    assert nms() == 0 and nms(r=0, h=1, w=7) == 0
    _rejects(lib, "lg_kp_nms", nms, [dict(x=None), dict(out=None), dict(x=A + 2), dict(out=A + 2), dict(out=A), dict(r=-1),
                                     dict(r=5), dict(h=0), dict(w=0), dict(b=-1), dict(b=65536), dict(h=8192, w=8193)])

    def sel(**kw):
        a = dict(x=A, h=64, w=64, b=0, border=4, thr=0.0005, k=1024, cnt=A, pix=A, sc=A, ws=A)
        a.update(kw)
        return lib.lg_kp_select(a["x"], a["h"], a["w"], a["b"], a["border"], a["thr"], a["k"], a["cnt"], a["pix"], a["sc"],
                                a["ws"], None)

    assert sel() == 0 and sel(border=0, thr=0.0, k=8) == 0 and sel(k=2048) == 0
    _rejects(lib, "lg_kp_select", sel, [dict(x=None), dict(cnt=None), dict(pix=None), dict(sc=None), dict(ws=None),
                                        dict(x=A + 2), dict(cnt=A + 2), dict(pix=A + 2), dict(sc=A + 2), dict(ws=A + 8),
                                        dict(border=-1), dict(thr=-0.1), dict(thr=float("nan")), dict(thr=float("inf")),
                                        dict(k=0), dict(k=4), dict(k=12), dict(k=2056), dict(h=0), dict(w=0), dict(b=-1)])
    assert lib.lg_kp_select_workspace(64, 64, 0) == 0 and lib.lg_kp_select_workspace(0, 64, 1) == 0
    assert lib.lg_kp_select_workspace(72, 136, 2) == 256 + 2 * 3 * 3328 * 8 + 2 * 72 * 136 * 8  # 3 segments of 3328
    assert lib.lg_kp_select_workspace(480, 640, 65) == 19712 + 2 * 65 * 480 * 640 * 8  # 75 segments of 4096

    def desc(**kw):
        a = dict(dd=1, x=A, sb=256 * 64, sc=64, sy=8, sx=1, hc=8, wc=8, b=0, k=1024, cnt=A, pix=A, dn=0, od=1, out=A, kpx=A,
                 kp=A)
        a.update(kw)
        return lib.lg_kp_describe(a["dd"], a["x"], a["sb"], a["sc"], a["sy"], a["sx"], a["hc"], a["wc"], a["b"], a["k"],
                                  a["cnt"], a["pix"], a["dn"], a["od"], a["out"], a["kpx"], a["kp"], None)

    assert desc() == 0 and desc(dd=0, od=0, dn=1, sc=1, sx=256, sy=256 * 8, k=8) == 0
    _rejects(lib, "lg_kp_describe", desc, [dict(dd=2), dict(od=2), dict(x=None), dict(cnt=None), dict(pix=None), dict(out=None),
                                          dict(kpx=None), dict(kp=None), dict(x=A + 1), dict(dd=0, x=A + 2), dict(cnt=A + 2),
                                          dict(pix=A + 2), dict(out=A + 2), dict(kpx=A + 2), dict(kp=A + 2), dict(sb=-1),
                                          dict(sc=-1), dict(sy=-1), dict(sx=-1), dict(dn=2), dict(dn=-1), dict(k=0),
                                          dict(k=12), dict(k=2056), dict(hc=0), dict(wc=0), dict(b=-1)])


def test_python_wrappers_refuse_cpu_tensors_and_bad_settings():
    from lightglue_amd import KeypointFrontend, PluginError

    fe = KeypointFrontend(max_keypoints=64)
    with pytest.raises(PluginError):
        fe.extract(torch.zeros(1, 65, 8, 8), torch.zeros(1, 256, 8, 8))
    with pytest.raises(PluginError):
        fe.from_scores(torch.zeros(1, 64, 64), torch.zeros(1, 256, 8, 8))
    for kw in (dict(max_keypoints=12), dict(max_keypoints=4096), dict(max_keypoints=0), dict(nms_radius=5),
               dict(nms_radius=-1), dict(threshold=-1.0), dict(remove_borders=-1), dict(dtype=torch.float64)):
        with pytest.raises(ValueError):
            KeypointFrontend(**kw)
