"""The LightGlue matcher around the op against the reference model.

Fixtures (tests/golden/match_*.npz, tests/golden/make_matcher_golden.py) hold the outputs of the
reference ``LightGlue(features=None, n_layers=L)`` (lightglue_pytorch_no_plugin/lightglue.py) in
fp32 on CPU, with weights and inputs regenerated bit-exactly from seeds.

Tolerances (stated per path):
* CPU, oracle attention, fp32: the restated model must reproduce the reference to float32
  round-off: max-abs <= 1e-4 on descriptors and log-scores.
* GPU, kernel attention, fp32 model: the kernel rounds q/k/v to fp16 on load (the reference's
  Float-boundary plugin does the same, …fp32out.cu:706-804) and uses fp16 P, so errors compound
  over the layers: max-abs <= TOL_DESC32 on descriptors, TOL_SCORE32 on log-scores.
* GPU, fp16 model (weights, activations and attention in fp16): TOL_DESC16 / TOL_SCORE16.
Matches are compared as sets of mutual nearest neighbours: the GPU paths must recover at least
MATCH_RECALL of the reference's mutual matches (near-ties may flip).
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

TOL_CPU = 1e-4
# observed on MI355X (tools/matcher_errors.py): fp32 <= 3.6e-3 / 3.4e-2, fp16 <= 2.6e-2 / 0.28 at 9 layers
TOL_DESC32, TOL_SCORE32 = 1e-2, 1e-1
TOL_DESC16, TOL_SCORE16 = 1e-1, 0.6
MATCH_RECALL = 0.9


def _model(name, attention=None, glue="hip"):
    from lightglue_amd import matcher

    meta = INDEX[name]
    m = matcher.LightGlueMatcher(n_layers=meta["n_layers"], attention=attention, glue=glue).eval()
    sd = matcher.seeded_state_dict(meta["seed"], meta["n_layers"])
    m.load_state_dict(sd, strict=True)
    pair = matcher.synthetic_pair(meta["seed"], meta["m"], meta["n"])
    return m, sd, pair


def _oracle_attention(calls):
    from oracle import oracle

    return [oracle.attention_torch(q, k, v) for q, k, v in calls]


def _match_set(m):
    return {(int(a), int(b)) for a, b in np.asarray(m)}


@pytest.mark.parametrize("name", CASES)
def test_seeded_inputs_reproduce(name):
    import hashlib

    _, sd, pair = _model(name)
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].numpy().tobytes())
    for t in pair:
        h.update(t.numpy().tobytes())
    assert h.hexdigest() == INDEX[name]["inputs_sha256"]


@pytest.mark.parametrize("name", CASES)
def test_cpu_restatement_matches_reference(name):
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    model, _, pair = _model(name, attention=_oracle_attention, glue="torch")
    with torch.no_grad():
        d0, d1, sc = model(*pair)
    assert float((d0 - torch.from_numpy(g["desc0"])).abs().max()) <= TOL_CPU
    assert float((d1 - torch.from_numpy(g["desc1"])).abs().max()) <= TOL_CPU
    assert float((sc - torch.from_numpy(g["scores"])).abs().max()) <= TOL_CPU


@pytest.mark.parametrize("name", CASES)
def test_filter_matches_restatement(name):
    from lightglue_amd.matcher import filter_matches

    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    sc = torch.from_numpy(g["scores"])
    for th, key in ((0.1, "matches"), (0.0, "matches_all")):
        m, s = filter_matches(sc, th)
        assert _match_set(m.numpy()) == _match_set(g[key])
        ref_scores = dict(zip(map(tuple, g[key].tolist()), g["mscores" if th else "mscores_all"].tolist()))
        for (a, b), v in zip(m.tolist(), s.tolist()):
            assert abs(ref_scores[(a, b)] - v) <= 1e-6


@pytest.mark.parametrize("glue", ["hip", "torch"])
def test_default_attention_refuses_cpu(glue):
    from lightglue_amd import PluginError

    model, _, pair = _model(CASES[0], glue=glue)
    with pytest.raises(PluginError):
        with torch.no_grad():
            model(*pair)


def test_pair_inputs_fast_path_needs_every_operand_fp16():
    """lg_pair_inputs reads desc0/desc1/kpts0/kpts1/posenc.Wr as raw fp16: the fast path is taken only
    when all five are fp16 (and 256 / 2 wide); any fp32 operand takes the framework path."""
    from lightglue_amd import matcher

    m = matcher.LightGlueMatcher(n_layers=1, attention=_oracle_attention).eval()
    k0, k1, d0, d1 = (t.half() for t in matcher.synthetic_pair(3, 16, 12))
    assert not m.pair_inputs_ok(k0, k1, d0, d1)            # fp32 model: Wr is fp32
    m = m.half()
    assert m.pair_inputs_ok(k0, k1, d0, d1)
    for i in range(4):
        args = [k0, k1, d0, d1]
        args[i] = args[i].float()
        assert not m.pair_inputs_ok(*args), i
    assert not m.pair_inputs_ok(k0, k1, d0, d1[..., :128])


def test_ffn_pack_layout():
    """ffn_pack (the one-launch FFN's weight streams, include/lightglue_glue.h lg_ffn_pack), two layouts
    back to back. 32-row kernel: wave w's 96 KiB = W1 pieces i = 2j + b, then W2 pieces 64 + j, then
    W3 pieces 96 + nb3 j + b; lane l of a piece = W[row0 + 32b + l % 32][16j + 8(l // 32) : + 8].
    16-row kernel: W1 pieces 4j + b, W2 64 + 2j + b, W3 96 + 2 nb3 j + b; lane l = W[row0 + 16b + l % 16]
    [32j + 8(l // 16) : + 8]. Every fragment checked against those definitions."""
    from lightglue_amd import matcher

    w1 = torch.arange(512 * 512, dtype=torch.float32).reshape(512, 512)
    w2 = -torch.arange(256 * 512, dtype=torch.float32).reshape(256, 512)
    e = torch.arange(8)

    def expected(w3, form):
        nb3 = 0 if w3 is None else w3.shape[0] // 256
        np_ = 96 + 16 * nb3
        w, i, l = torch.meshgrid(torch.arange(8), torch.arange(np_), torch.arange(64), indexing="ij")
        if form == 32:
            r, g = l % 32, l // 32
            j1, b1 = i // 2, i % 2
            j2, b2 = i - 64, 0 * i
            j3, b3 = (i - 96) // max(nb3, 1), (i - 96) % max(nb3, 1)
            row1, k1 = 64 * w + 32 * b1 + r, 16 * j1 + 8 * g
            row2, k2 = 32 * w + r, 16 * j2 + 8 * g
            row3, k3 = 32 * (nb3 * w + b3) + r, 16 * j3 + 8 * g
        else:
            r, g = l % 16, l // 16
            j1, b1 = i // 4, i % 4
            j2, b2 = (i - 64) // 2, (i - 64) % 2
            j3, b3 = (i - 96) // max(2 * nb3, 1), (i - 96) % max(2 * nb3, 1)
            row1, k1 = 64 * w + 16 * b1 + r, 32 * j1 + 8 * g
            row2, k2 = 32 * w + 16 * b2 + r, 32 * j2 + 8 * g
            row3, k3 = 16 * (2 * nb3 * w + b3) + r, 32 * j3 + 8 * g
        out = torch.zeros(8, np_, 64, 8)
        m1, m2, m3 = i < 64, (i >= 64) & (i < 96), i >= 96
        out[m1] = w1[row1[m1][:, None], k1[m1][:, None] + e]
        out[m2] = w2[row2[m2][:, None], k2[m2][:, None] + e]
        if nb3:
            out[m3] = w3[row3[m3][:, None], k3[m3][:, None] + e]
        return out

    for n3 in (0, 512, 768):
        w3 = None if n3 == 0 else torch.arange(n3 * 256, dtype=torch.float32).reshape(n3, 256) + 0.5
        got = matcher.ffn_pack(w1, w2, w3).reshape(2, 8, 96 + n3 // 16, 64, 8)
        assert torch.equal(got[0], expected(w3, 32)), n3
        assert torch.equal(got[1], expected(w3, 16)), n3


def _gpu_run(name, dtype, glue="hip"):
    model, _, pair = _model(name, glue=glue)
    dev = torch.device("cuda:0")
    model = model.to(dev, dtype)
    with torch.no_grad():
        k0, k1, x0, x1 = (t.to(dev, dtype) for t in pair)
        d0, d1, sc = model(k0, k1, x0, x1)
        torch.cuda.synchronize()
    return model, d0.float().cpu(), d1.float().cpu(), sc.float().cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("glue", ["hip", "torch"])
@pytest.mark.parametrize("dtype,tol_d,tol_s", [("float32", TOL_DESC32, TOL_SCORE32),
                                               ("float16", TOL_DESC16, TOL_SCORE16)])
def test_gpu_matcher_matches_reference(name, glue, dtype, tol_d, tol_s):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd.matcher import filter_matches

    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    _, d0, d1, sc = _gpu_run(name, getattr(torch, dtype), glue)
    assert torch.isfinite(sc).all()
    assert float((d0 - torch.from_numpy(g["desc0"])).abs().max()) <= tol_d
    assert float((d1 - torch.from_numpy(g["desc1"])).abs().max()) <= tol_d
    assert float((sc - torch.from_numpy(g["scores"])).abs().max()) <= tol_s
    got = _match_set(filter_matches(sc, 0.0)[0].numpy())
    ref = _match_set(g["matches_all"])
    assert len(got & ref) >= MATCH_RECALL * len(ref)


def _check_fused_linear(mt, blk, dev, rnd, n0, n1, h):
    """lg_linear* against framework GEMMs (fp32 math on the same fp16 operands), tolerances for
    fp16 outputs of K = 256 / 512 dot products."""
    F = torch.nn.functional
    dt = torch.float16
    f32 = lambda t: t.float()  # noqa: E731
    x = rnd(1, n0 + n1, 256) * 0.5
    tol = 2e-2
    # plain + residual (K = 512)
    a, res = rnd(1, n0 + n1, 512) * 0.5, rnd(1, n0 + n1, 256)
    w, b = rnd(256, 512) * 0.05, rnd(256) * 0.1
    ref = F.linear(f32(a), f32(w), f32(b))
    assert float((mt._Hip.linear(a, w, b).float() - ref).abs().max()) <= tol
    assert float((mt._Hip.linear(a, w, b, res=res).float() - (ref + f32(res))).abs().max()) <= tol
    # [x | merged heads] gathered on load (K = 512, N = 512)
    c0, c1 = rnd(1, h, n0, 64), rnd(1, h, n1, 64)
    w, b = rnd(512, 512) * 0.05, rnd(512) * 0.1
    merged = torch.cat([c[0].transpose(0, 1).reshape(c.shape[2], -1) for c in (c0, c1)], 0)[None]
    ref = F.linear(torch.cat((f32(x), f32(merged)), -1), f32(w), f32(b))
    assert float((mt._Hip.linear_cat(x, c0, c1, w, b).float() - ref).abs().max()) <= tol
    # self-block projection + rotary + head split (K = 256, N = 768)
    ang = rnd(1, n0 + n1, 32).float()
    cos = torch.cos(ang).repeat_interleave(2, -1).to(dt).contiguous()
    sin = torch.sin(ang).repeat_interleave(2, -1).to(dt).contiguous()
    blk32 = mt.SelfBlock(256, h).to(dev)
    with torch.no_grad():
        blk16 = mt.SelfBlock(256, h).to(dev, dt)
        blk16.load_state_dict(blk.state_dict())
        blk32.load_state_dict(blk.state_dict())
        ref = blk32.qkv(f32(x), f32(cos), f32(sin), (n0, n1), hip=False)
        wq, bq = mt._qkv_perm(blk16, dt)
        got = mt._Hip.linear_qkv_rotary(x, wq, bq, cos, sin, h, (n0, n1))
    for r3, g3 in zip(ref, got):
        for r_, g_ in zip(r3, g3):
            assert float((r_ - g_.float()).abs().max()) <= tol
    # cross-block to_qk | to_v + head split (K = 256, N = 512)
    cb = mt.CrossBlock(256, h).to(dev)
    with torch.no_grad():
        wc = torch.cat((cb.to_qk.weight, cb.to_v.weight), 0).to(dt)
        bc = torch.cat((cb.to_qk.bias, cb.to_v.bias), 0).to(dt)
        (a0, a1), (b0, b1) = mt._Hip.linear_split2(x, wc, bc, h, (n0, n1))
        xs = f32(x)
        refs = cb.heads_of(F.linear(xs, f32(wc[:256]), f32(bc[:256])), (n0, n1)) + \
            cb.heads_of(F.linear(xs, f32(wc[256:]), f32(bc[256:])), (n0, n1))
    for r_, g_ in zip(refs, (a0, a1, b0, b1)):
        assert float((r_ - g_.float()).abs().max()) <= tol


# ---- the glue kernels one by one against the torch restatement (include/lightglue_glue.h) ----
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_glue_kernels_match_torch(dtype):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import matcher as mt

    dt = getattr(torch, dtype)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    tol = 2e-3 if dtype == "float16" else 1e-5
    n0, n1, h = 37, 70, 4
    blk = mt.SelfBlock(256, h).to(dev, dt)
    x = rnd(1, n0 + n1, 256)
    ang = rnd(1, n0 + n1, 32).float()
    cos = torch.cos(ang).repeat_interleave(2, -1).to(dt)
    sin = torch.sin(ang).repeat_interleave(2, -1).to(dt)
    with torch.no_grad():
        ref = blk.qkv(x, cos, sin, (n0, n1), hip=False)
        got = blk.qkv(x, cos.contiguous(), sin.contiguous(), (n0, n1), hip=True)
        for r3, g3 in zip(ref, got):
            for r, g_ in zip(r3, g3):
                assert float((r.float() - g_.float()).abs().max()) <= tol * 4
        a, b = rnd(1, n0 + n1, 256), rnd(1, n0 + n1, 256)
        cb = mt.CrossBlock(256, h)
        (a0, a1), (b0, b1) = mt._Hip.split_heads2(a, b, h, (n0, n1))
        for r, g_ in zip(cb.heads_of(a, (n0, n1)) + cb.heads_of(b, (n0, n1)), (a0, a1, b0, b1)):
            assert torch.equal(r, g_)
        merged = mt._Hip.merge_heads(a0, a1)
        assert torch.equal(merged, a)
        # strided split of one [a | b] projection; [x | merge] concatenation
        ab = torch.cat((a, b), -1).contiguous()
        (c0, c1), (d0_, d1_) = mt._Hip.split_heads2_ld(ab, h, (n0, n1))
        for r, g_ in zip((a0, a1, b0, b1), (c0, c1, d0_, d1_)):
            assert torch.equal(r, g_)
        assert torch.equal(mt._Hip.merge_heads_cat(b, a0, a1), torch.cat((b, a), -1))
        # out_proj folded into ffn[0] (fp32 fold of the weights): same pre-activation
        w, bias = mt._ffn_in_fused(blk, blk.out_proj, dt)
        xm = torch.cat((x, a), -1)
        ref_h = blk.ffn[0](torch.cat((x, blk.out_proj(a)), -1)).float()
        got_h = torch.nn.functional.linear(xm, w, bias).float()
        assert float((ref_h - got_h).abs().max()) <= (5e-2 if dtype == "float16" else 1e-4)
        ln = torch.nn.LayerNorm(512).to(dev, dt)
        with torch.no_grad():
            ln.weight.copy_(rnd(512) * 0.1 + 1)
            ln.bias.copy_(rnd(512) * 0.1)
        hx = rnd(1, 300, 512)
        ref = torch.nn.functional.gelu(ln(hx).float()).to(dt)
        tol_ln = 2e-2 if dtype == "float16" else 1e-4
        assert float((mt._Hip.layernorm_gelu(hx, ln).float() - ref.float()).abs().max()) <= tol_ln
        if dtype == "float16":  # the fused projections (csrc/lightglue_linear.hip, lightglue_ffn_ln.hip, lightglue_ffn.hip, fp16 only)
            _check_fused_linear(mt, blk, dev, rnd, n0, n1, h)
            _check_fused_linear(mt, blk, dev, rnd, 700, 1301, h)
        for m_, n_ in ((130, 211), (1024, 777), (1, 2000), (2000, 5)):  # column pass: 128-row chunks
            sim = rnd(1, m_, n_).float() * 5
            z0, z1 = rnd(1, m_, 1).float(), rnd(1, n_, 1).float()
            ref = mt.log_double_softmax(sim, z0, z1)
            got = mt._Hip.log_double_softmax(sim, z0, z1)
            torch.cuda.synchronize()
            assert float((ref - got).abs().max()) <= 1e-4, (m_, n_)


# ---- BASELINE configs[3] sweep size (512 x 512, 9 layers) on a pair with true correspondences ----
SWEEP = json.load(open(os.path.join(GOLD, "matcher_sweep_index.json")))
# fp16 path at 9 layers (weights, activations and attention in fp16): log-scores are sums of two
# log-softmaxes over 512 entries of a similarity built from fp16 descriptors; an fp16 descriptor
# error e moves a similarity by ~|d| e, and both softmax normalisers by a weighted mean of such
# moves, so per-element errors stay near the descriptor error times the similarity scale. Observed on
# MI355X (the test prints them): fp32 3.2e-3 / 2.6e-2 / 1.3e-4, fp16 1.8e-2 / 0.22 / 1.1e-3
# (descriptors / log-scores / relative row and column sums); bounds ~3-4x those.
SWEEP_TOL = {"float32": (1e-2, 1e-1, 5e-4), "float16": (6e-2, 0.6, 5e-3)}
SWEEP_RECALL = 0.9
# |log-score - reference| on the reference's mutual nearest neighbours (every threshold-0 match: the
# entries that decide matching). The fp16 value is not a property of one attention plan: nine fp16
# layers amplify any rounding difference, and perturbing each attention output by +-1 fp16 ulp on a
# random 10 % of its elements (tools/matcher_plan_errors.py, profiles/r05/matcher_plan_errors*.jsonl,
# 1024 x 1024 fixture) moves this error over 0.14-0.26 across 8 seeds; one pair per forward under
# other attention plans 0.15-0.21, the fixture pair inside P = 4 / 8 pairs per forward (stream modes
# 0 and 1) 0.135-0.20. fp32: 0.011-0.022. Bounds ~2x the largest of those.
SWEEP_TOL_MATCHED = {"float32": 6e-2, "float16": 0.5}
SWEEP_TOL_MATCHED_BATCHED = SWEEP_TOL_MATCHED
# A batched forward against the same pair's own forward, every element: two fp16 forwards differ by
# what a 1-ulp attention perturbation alone moves (same tool: descriptors 0.039, log-scores 0.525 over
# 8 seeds; batched vs single measured 0.031 / 0.511, round 6 0.031 / 0.514 at P = 4 and 8); fp32 ~10x
# tighter. fp16 bounds ~1.2x the measured, fp32 ~2-4x.
BATCHED_VS_SINGLE = {"float32": (1e-2, 1e-1), "float16": (6e-2, 0.6)}


def _sweep_model(name, attention=None, glue="hip"):
    from lightglue_amd import matcher

    meta = SWEEP[name]
    m = matcher.LightGlueMatcher(n_layers=meta["n_layers"], attention=attention, glue=glue).eval()
    m.load_state_dict(matcher.seeded_state_dict(meta["seed"], meta["n_layers"]), strict=True)
    return m, matcher.synthetic_pair(meta["seed"], meta["m"], meta["n"], overlap=meta["overlap"])


def _check_sweep(g, d0, d1, sc, tol_d, tol_s, tol_rowsum_rel):
    rows = g["rows"]
    assert torch.isfinite(sc).all()
    err_d = max(float((d0[0, rows] - torch.from_numpy(g["desc0_rows"])).abs().max()),
                float((d1[0, rows] - torch.from_numpy(g["desc1_rows"])).abs().max()))
    err_s = max(float((sc[0, rows] - torch.from_numpy(g["scores_rows"])).abs().max()),
                float((sc[0, :, 0] - torch.from_numpy(g["scores_col0"])).abs().max()))
    rs = sc[0].double().sum(1).numpy()
    cs = sc[0].double().sum(0).numpy()
    err_sum = max(float(np.abs(rs - g["scores_row_sums"]).max() / np.abs(g["scores_row_sums"]).max()),
                  float(np.abs(cs - g["scores_col_sums"]).max() / np.abs(g["scores_col_sums"]).max()))
    # the entries that decide the matches: the reference's mutual nearest neighbours (threshold 0)
    mi, mj = g["matches_all"][:, 0], g["matches_all"][:, 1]
    err_m = float((sc[0, mi, mj].double() - torch.from_numpy(np.log(g["mscores_all"].astype(np.float64)))).abs().max())
    print(f"sweep errors: desc {err_d:.3e} scores {err_s:.3e} row/col-sum rel {err_sum:.3e} matched entries {err_m:.3e}")
    assert err_d <= tol_d and err_s <= tol_s and err_sum <= tol_rowsum_rel
    return err_d, err_s, err_m


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_sweep_inputs_reproduce_and_have_matches(name):
    import hashlib

    from lightglue_amd import matcher

    meta = SWEEP[name]
    _, pair = _sweep_model(name)
    sd = matcher.seeded_state_dict(meta["seed"], meta["n_layers"])
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].numpy().tobytes())
    for t in pair:
        h.update(t.numpy().tobytes())
    assert h.hexdigest() == meta["inputs_sha256"]
    assert meta["n_matches"] >= 50   # a recall check on this fixture is not vacuous


@pytest.mark.parametrize("name", sorted(SWEEP))
def test_sweep_cpu_restatement_matches_reference(name):
    from lightglue_amd.matcher import filter_matches

    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    model, pair = _sweep_model(name, attention=_oracle_attention, glue="torch")
    with torch.no_grad():
        d0, d1, sc = model(*pair)
    _check_sweep(g, d0, d1, sc, TOL_CPU, TOL_CPU, 1e-6)
    assert _match_set(filter_matches(sc, 0.1)[0].numpy()) == _match_set(g["matches"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SWEEP))
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_sweep_gpu_matcher_matches_reference(name, dtype):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd.matcher import filter_matches

    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    model, pair = _sweep_model(name)
    dev = torch.device("cuda:0")
    dt = getattr(torch, dtype)
    model = model.to(dev, dt)
    with torch.no_grad():
        d0, d1, sc = model(*(t.to(dev, dt) for t in pair))
        torch.cuda.synchronize()
    d0, d1, sc = d0.float().cpu(), d1.float().cpu(), sc.float().cpu()
    _, _, err_m = _check_sweep(g, d0, d1, sc, *SWEEP_TOL[dtype])
    assert err_m <= SWEEP_TOL_MATCHED[dtype], err_m
    got = _match_set(filter_matches(sc, 0.1)[0].numpy())
    ref = _match_set(g["matches"])
    assert len(ref) >= 50
    print(f"recall {len(got & ref)} / {len(ref)}")
    assert len(got & ref) >= SWEEP_RECALL * len(ref), (len(got & ref), len(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float16", "float32"])
@pytest.mark.parametrize("pairs", [4, 8])
def test_batched_pairs_equal_single_pair_forwards(pairs, dtype):
    """P image pairs in one forward (pair-major rows through every projection and glue kernel, one
    grouped attention launch of P-batch calls per block; lightglue.py:328-353 batched, the demo's
    pair loop demo_mono.cpp:194-418 folded into the batch): each pair's outputs equal that pair's
    own forward within the fixture bounds, and the fixture pair inside the batch still matches the
    reference (BASELINE configs[3]/[4] at 1024 x 1024)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import matcher

    name = "sweep_l9_1024x1024"
    meta = SWEEP[name]
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    model, pair = _sweep_model(name)
    dev = torch.device("cuda:0")
    dt = getattr(torch, dtype)
    model = model.to(dev, dt)
    at = pairs // 2  # the fixture pair's slot in the batch
    ps = [matcher.synthetic_pair(meta["seed"] + 100 + i, meta["m"], meta["n"], overlap=meta["overlap"])
          for i in range(pairs)]
    ps[at] = pair
    batch = tuple(torch.cat([p[j] for p in ps], 0).to(dev, dt) for j in range(4))
    with torch.no_grad():
        bd0, bd1, bsc = model(*batch)
        singles = [model(*(t.to(dev, dt) for t in p)) for p in ps]
        torch.cuda.synchronize()
    assert bsc.shape == (pairs, meta["m"], meta["n"])
    tol_d, tol_s = BATCHED_VS_SINGLE[dtype]
    worst = [0.0, 0.0]
    for i, (d0, d1, sc) in enumerate(singles):
        ed = max(float((bd0[i] - d0[0]).abs().max()), float((bd1[i] - d1[0]).abs().max()))
        es = float((bsc[i] - sc[0]).abs().max())
        worst = [max(worst[0], ed), max(worst[1], es)]
        assert ed <= tol_d and es <= tol_s, (i, ed, es)
    print(f"batched vs single forwards (P={pairs}, {dtype}): desc {worst[0]:.3e} scores {worst[1]:.3e}")
    d0, d1, sc = (t[at:at + 1].float().cpu() for t in (bd0, bd1, bsc))
    _, _, err_m = _check_sweep(g, d0, d1, sc, *SWEEP_TOL[dtype])
    assert err_m <= SWEEP_TOL_MATCHED_BATCHED[dtype], err_m
    matches = model.match(*batch)
    assert isinstance(matches, list) and len(matches) == pairs
    got = _match_set(matches[at][0].cpu().numpy())
    ref = _match_set(g["matches"])
    assert len(got & ref) >= SWEEP_RECALL * len(ref), (len(got & ref), len(ref))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_glue_kernels_with_pairs_equal_per_pair_calls(dtype):
    """Every pair-aware glue kernel (include/lightglue_glue.h, `pairs`) on P = 3 pairs stacked
    pair-major gives, for each pair, the bits its own P = 1 call gives; the dual log-softmax on a
    [P, m, n] batch equals its per-pair launches."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import matcher as mt

    dt = getattr(torch, dtype)
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    P, n0, n1, h = 3, 37, 70, 4
    nt = n0 + n1
    rows = lambda t, i: t[:, i * nt:(i + 1) * nt].contiguous()  # noqa: E731  pair i's rows
    with torch.no_grad():
        qkv = rnd(1, P * nt, 3 * h * 64)
        ang = rnd(1, P * nt, 32).float()
        cos = torch.cos(ang).repeat_interleave(2, -1).to(dt).contiguous()
        sin = torch.sin(ang).repeat_interleave(2, -1).to(dt).contiguous()
        got = mt._Hip.qkv_rotary_split(qkv, cos, sin, h, (n0, n1, P))
        for i in range(P):
            one = mt._Hip.qkv_rotary_split(rows(qkv, i), rows(cos, i), rows(sin, i), h, (n0, n1))
            for g3, o3 in zip(got, one):
                for g_, o_ in zip(g3, o3):
                    assert torch.equal(g_[i:i + 1], o_)
        a, b = rnd(1, P * nt, h * 64), rnd(1, P * nt, h * 64)
        (a0, a1), (b0, b1) = mt._Hip.split_heads2(a, b, h, (n0, n1, P))
        assert a0.shape == (P, h, n0, 64) and a1.shape == (P, h, n1, 64)
        ab = torch.cat((a, b), -1).contiguous()
        (c0, c1), (d0_, d1_) = mt._Hip.split_heads2_ld(ab, h, (n0, n1, P))
        for r, g_ in zip((a0, a1, b0, b1), (c0, c1, d0_, d1_)):
            assert torch.equal(r, g_)
        for i in range(P):
            (e0, e1), (f0, f1) = mt._Hip.split_heads2(rows(a, i), rows(b, i), h, (n0, n1))
            for g_, o_ in zip((a0, a1, b0, b1), (e0, e1, f0, f1)):
                assert torch.equal(g_[i:i + 1], o_)
        assert torch.equal(mt._Hip.merge_heads(a0, a1), a)
        assert torch.equal(mt._Hip.merge_heads_cat(b, a0, a1), torch.cat((b, a), -1))
        if dtype == "float16":  # fused projections: per-row math, so the batched rows are bitwise
            x = rnd(1, P * nt, 256) * 0.5
            blk = mt.SelfBlock(256, h).to(dev, dt)
            wq, bq = mt._qkv_perm(blk, dt)
            got = mt._Hip.linear_qkv_rotary(x, wq, bq, cos, sin, h, (n0, n1, P))
            w2, b2 = rnd(512, 256) * 0.05, rnd(512) * 0.1
            (s0, s1), (t0, t1) = mt._Hip.linear_split2(x, w2, b2, h, (n0, n1, P))
            w3, b3 = rnd(512, 512) * 0.05, rnd(512) * 0.1
            lc = mt._Hip.linear_cat(x, a0, a1, w3, b3)
            for i in range(P):
                one = mt._Hip.linear_qkv_rotary(rows(x, i), wq, bq, rows(cos, i), rows(sin, i), h, (n0, n1))
                for g3, o3 in zip(got, one):
                    for g_, o_ in zip(g3, o3):
                        assert torch.equal(g_[i:i + 1], o_)
                (u0, u1), (v0, v1) = mt._Hip.linear_split2(rows(x, i), w2, b2, h, (n0, n1))
                for g_, o_ in zip((s0, s1, t0, t1), (u0, u1, v0, v1)):
                    assert torch.equal(g_[i:i + 1], o_)
                assert torch.equal(rows(lc, i), mt._Hip.linear_cat(rows(x, i), a0[i:i + 1].contiguous(),
                                                                   a1[i:i + 1].contiguous(), w3, b3))
        sim = rnd(P, 300, 257).float() * 5
        z0, z1 = rnd(P, 300, 1).float(), rnd(P, 257, 1).float()
        got = mt._Hip.log_double_softmax(sim, z0, z1)
        for i in range(P):
            one = mt._Hip.log_double_softmax(sim[i:i + 1].contiguous(), z0[i:i + 1].contiguous(),
                                             z1[i:i + 1].contiguous())
            assert torch.equal(got[i:i + 1], one)
        torch.cuda.synchronize()


def test_torch_glue_runs_pairs_one_by_one():
    """glue='torch' (the CPU restatement) takes P pairs by looping: the same outputs as P forwards."""
    from lightglue_amd import matcher

    m = matcher.LightGlueMatcher(n_layers=2, attention=_oracle_attention, glue="torch").eval()
    m.load_state_dict(matcher.seeded_state_dict(1, 2), strict=True)
    ps = [matcher.synthetic_pair(s, 40, 33) for s in (1, 2)]
    batch = tuple(torch.cat([p[j] for p in ps], 0) for j in range(4))
    with torch.no_grad():
        got = m(*batch)
        for i, p in enumerate(ps):
            one = m(*p)
            for g_, o_ in zip(got, one):
                assert torch.equal(g_[i:i + 1], o_)


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,n0,n1", [(3, 37, 70), (2, 1000, 777), (16, 1024, 1024), (9, 1000, 1011), (40, 20, 30), (5, 1, 63),
                                         (4, 56, 1)])
def test_wide_projections_equal_narrow(pairs, n0, n1):
    """The projections' tile form (csrc/lightglue_linear.hip linear_tile_kernel: 128 x 128 on 4 waves,
    modes 1, 2 and 4 alike, with the LDS-staged coalesced epilogue, taken for launches of at least one
    round of tiles: several image pairs per forward) gives the bits of the 64 x 64 form on
    every fused entry point — ragged row counts (rows past m in a tile: computed on the clamped last
    row, their stores rewrite that row's bytes), both K (256 and 512), residual on and off, the
    A-gather of lg_linear_cat, the per-image scatters. The head-major epilogue's row paths: the
    per-tile row step (1024-row images), the per-row split where a lane's rows cross an image or
    pair boundary (37 + 70, 1 + 63, 56 + 1: the shortest pair it takes), and the 64 x 64 fallback for
    pairs of <= 56 rows (20 + 30)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib
    from lightglue_amd import matcher as mt

    lib = _lib.load()
    dev, dt, h = torch.device("cuda:0"), torch.float16, 4
    gen = torch.Generator().manual_seed(11)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    nt = n0 + n1
    sp = (n0, n1, pairs)
    with torch.no_grad():
        x = rnd(1, pairs * nt, 256) * 0.5
        hx = rnd(1, pairs * nt, 512) * 0.5
        ang = rnd(1, pairs * nt, 32).float()
        cos = torch.cos(ang).repeat_interleave(2, -1).to(dt).contiguous()
        sin = torch.sin(ang).repeat_interleave(2, -1).to(dt).contiguous()
        c0, c1 = rnd(pairs, h, n0, 64), rnd(pairs, h, n1, 64)
        blk = mt.SelfBlock(256, h).to(dev, dt)
        wq, bq = mt._qkv_perm(blk, dt)
        w2, b2 = rnd(512, 256) * 0.05, rnd(512) * 0.1
        w3, b3 = rnd(512, 512) * 0.05, rnd(512) * 0.1
        w4, b4 = rnd(256, 512) * 0.05, rnd(256) * 0.1

        def run():
            return [mt._Hip.linear_qkv_rotary(x, wq, bq, cos, sin, h, sp),
                    mt._Hip.linear_split2(x, w2, b2, h, sp),
                    mt._Hip.linear_cat(x, c0, c1, w3, b3),
                    mt._Hip.linear(hx, w4, b4, x), mt._Hip.linear(hx, w4, b4)]

        flat = lambda o: [t for t in (o if isinstance(o, torch.Tensor) else  # noqa: E731
                                      [u for v in o for u in (v if isinstance(v, (tuple, list)) else [v])])]
        prev = lib.lg_linear_set_wide(0)
        try:
            narrow = [flat(o) for o in run()]
            forms = []
            for mode in (1, 2, 4):  # all the 128 x 128 form on 4 waves (1 and 2 once named 256-row forms)
                lib.lg_linear_set_wide(mode)
                forms.append([flat(o) for o in run()])
            torch.cuda.synchronize()
        finally:
            lib.lg_linear_set_wide(prev)
        for f, form in enumerate(forms):
            for i, (a, b) in enumerate(zip(narrow, form)):
                for ta, tb in zip(a, b):
                    assert torch.equal(ta, tb), (f + 1, i, float((ta.float() - tb.float()).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,n0,n1", [(16, 1024, 1024), (9, 1000, 1011), (1, 700, 1301)])
def test_linear_cat_ln_gelu_matches_torch(pairs, n0, n1):
    """lg_linear_cat_ln_gelu (the FFN's Linear -> LayerNorm -> GELU, lightglue.py:101-106) against
    the torch restatement on the same fp16 operands: F.linear rounded to fp16 (as the fp16 model
    rounds h), then layer_norm and exact GELU in fp32; both forms, forced (lg_linear_set_ln_fused 0:
    two launches, 2: the one-launch form, tiles owning whole rows, statistics in the workgroup), and
    the default's choice by size (one launch from 16,384 rows on — 128-row tiles for 16 x 2048 rows,
    64-row tiles for 9 x 2011 — two launches for 2001 rows). Bound: a few fp16 ulps of the O(1)
    outputs."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib
    from lightglue_amd import matcher as mt

    F = torch.nn.functional
    dev, dt, h = torch.device("cuda:0"), torch.float16, 4
    lib = _lib.load()
    gen = torch.Generator().manual_seed(5 + pairs)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    with torch.no_grad():
        x = rnd(1, pairs * (n0 + n1), 256) * 0.5
        c0, c1 = rnd(pairs, h, n0, 64), rnd(pairs, h, n1, 64)
        w, b = rnd(512, 512) * 0.05, rnd(512) * 0.1
        ln = torch.nn.LayerNorm(512).to(dev, dt)
        ln.weight.copy_(1 + 0.1 * rnd(512))
        ln.bias.copy_(0.1 * rnd(512))
        got = mt._Hip.linear_cat_ln_gelu(x, c0, c1, w, b, ln)  # the default
        prev = lib.lg_linear_set_ln_fused(0)
        try:
            two = mt._Hip.linear_cat_ln_gelu(x, c0, c1, w, b, ln)
            lib.lg_linear_set_ln_fused(2)
            fused = mt._Hip.linear_cat_ln_gelu(x, c0, c1, w, b, ln)
        finally:
            lib.lg_linear_set_ln_fused(prev)
        hh = mt._Hip.linear_cat(x, c0, c1, w, b)  # the projection alone (bits of every form)
        ref = F.gelu(F.layer_norm(hh.float(), (512,), ln.weight.float(), ln.bias.float(), ln.eps))
        unf = mt._Hip.layernorm_gelu(hh, ln)  # the two-launch path
        torch.cuda.synchronize()
    err = float((two.float() - ref).abs().max())
    err_f = float((fused.float() - ref).abs().max())
    print(f"cat+LN+GELU P={pairs}: max-abs {err:.3e} (one-launch form {err_f:.3e})")
    assert torch.isfinite(two).all() and torch.isfinite(fused).all()
    assert torch.equal(two, unf)  # the two-launch form is lg_linear_cat + lg_layernorm_gelu
    assert torch.equal(got, fused if pairs * (n0 + n1) >= 256 * 64 else two)  # the default's choice by size
    assert err <= 8e-3 and err_f <= 8e-3


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,n0,n1", [(16, 1024, 1024), (17, 1000, 977), (1, 300, 257), (2, 64, 1)])
def test_linear_cat_ffn_equals_two_calls(pairs, n0, n1):
    """lg_linear_cat_ffn without the packed stream (or with lg_linear_set_ffn_fused(0)) is exactly its
    two calls: lg_linear_cat_ln_gelu then lg_linear(h, W2, b2, res = x) (lightglue.py:101-106 +
    :150-151), bitwise, under each of lg_linear_cat_ln_gelu's forms (lg_linear_set_ln_fused 1: by size,
    2: one launch, 0: two launches)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib
    from lightglue_amd import matcher as mt

    dev, dt, h = torch.device("cuda:0"), torch.float16, 4
    lib = _lib.load()
    gen = torch.Generator().manual_seed(11 + pairs)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    with torch.no_grad():
        x = rnd(1, pairs * (n0 + n1), 256) * 0.5
        c0, c1 = rnd(pairs, h, n0, 64), rnd(pairs, h, n1, 64)
        w, b = rnd(512, 512) * 0.05, rnd(512) * 0.1
        w2, b2 = rnd(256, 512) * 0.05, rnd(256) * 0.1
        ln = torch.nn.LayerNorm(512).to(dev, dt)
        ln.weight.copy_(1 + 0.1 * rnd(512))
        ln.bias.copy_(0.1 * rnd(512))
        wp = mt.ffn_pack(w, w2)
        outs = {}
        for mode in (1, 2, 0):
            prev = lib.lg_linear_set_ln_fused(mode)
            try:
                outs[mode] = mt._Hip.ffn(x, c0, c1, w, b, ln, w2, b2)           # no packed stream
                prev_f = lib.lg_linear_set_ffn_fused(0)
                try:
                    outs[(mode, "off")] = mt._Hip.ffn(x, c0, c1, w, b, ln, w2, b2, wp)  # one-launch form off
                finally:
                    lib.lg_linear_set_ffn_fused(prev_f)
                hh = mt._Hip.linear_cat_ln_gelu(x, c0, c1, w, b, ln)
                outs[(mode, "two")] = mt._Hip.linear(hh, w2, b2, res=x)
            finally:
                lib.lg_linear_set_ln_fused(prev)
        torch.cuda.synchronize()
    for mode in (1, 2, 0):
        assert torch.isfinite(outs[mode]).all(), mode
        assert torch.equal(outs[mode], outs[(mode, "two")]), mode
        assert torch.equal(outs[(mode, "off")], outs[(mode, "two")]), mode


def _ffn_torch(x, c0, c1, w, b, ln, w2, b2):
    """The FFN with its residual as the fp16 model rounds it (lightglue.py:101-106, 150-151): F.linear
    outputs rounded to fp16, LayerNorm and exact GELU in fp32 rounded to fp16, x + that in fp32 rounded."""
    F = torch.nn.functional
    a = torch.cat((x[0], torch.cat([torch.cat([ci[p].transpose(0, 1).reshape(ci.shape[2], -1) for ci in (c0, c1)], 0)
                                     for p in range(c0.shape[0])], 0)), 1).float()
    h = (a @ w.float().t() + b.float()).half().float()
    g = F.gelu(F.layer_norm(h, (512,), ln.weight.float(), ln.bias.float(), ln.eps)).half().float()
    o = (g @ w2.float().t() + b2.float()).half().float()
    return (x[0].float() + o).half()[None]


# |ffn_rows_kernel - two calls|: h before the LayerNorm is bitwise the two-call path's; the statistics
# differ in the order of their fp32 sums only (lg_layernorm_gelu: two passes over the row in one wave;
# the rows kernels: each wave's sum and squares about its own mean, merged over 8 waves; neither forms
# E[h^2] - mean^2), so a GELU output can move by one fp16 ulp, and with it the rounding of
# v = fp16(W2 g + b2) and of x + v. Bound: 2 ulp of the larger of |out| and |v| = |out - x| (and 2^-11
# near 0).
def _ulp_bound(out, x, k=2.0):
    mag = torch.maximum(out.float().abs(), (out.float() - x.float()).abs())
    return k * torch.clamp(mag, min=2.0 ** -2) * 2.0 ** -10


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,n0,n1", [(1, 512, 512), (1, 1024, 1024), (1, 2048, 2048), (1, 700, 1301), (1, 1, 63),
                                         (3, 37, 70), (4, 1024, 1024), (5, 1000, 1011), (1, 3, 2), (8, 1024, 1024),
                                         (9, 1000, 1011)])
def test_ffn_rows_kernel(pairs, n0, n1):
    """lg_linear_cat_ffn's one-launch forms — ffn_rows16_kernel (16 rows per workgroup, the default up
    to one round of them, 4,096 rows; lg_linear_set_ffn_fused(3) at every size) and ffn_rows_kernel
    (32 rows up to 8,192, 64 beyond; the default there, and (2) at every size) — against its two calls
    (lg_linear_set_ffn_fused(0)) and the torch restatement of the fp16 model (_ffn_torch): single pairs
    of 512 / 1024 / 2048 keypoints, ragged rows (a partial last workgroup, images of 1..3 rows), 4 pairs
    (8,192 rows: the last 32-row size), 5 pairs (64-row tiles, a partial last one), 8 and 9 pairs."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib
    from lightglue_amd import matcher as mt

    dev, dt, h = torch.device("cuda:0"), torch.float16, 4
    lib = _lib.load()
    gen = torch.Generator().manual_seed(21 + pairs + n0)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    m = pairs * (n0 + n1)
    with torch.no_grad():
        x = rnd(1, m, 256) * 0.5
        c0, c1 = rnd(pairs, h, n0, 64), rnd(pairs, h, n1, 64)
        w, b = rnd(512, 512) * 0.05, rnd(512) * 0.1
        w2, b2 = rnd(256, 512) * 0.05, rnd(256) * 0.1
        ln = torch.nn.LayerNorm(512).to(dev, dt)
        ln.weight.copy_(1 + 0.1 * rnd(512))
        ln.bias.copy_(0.1 * rnd(512))
        wp = mt.ffn_pack(w, w2)
        packed_c = torch.empty(lib.lg_ffn_packed_bytes(h, 0) // 2, dtype=dt, device=dev)
        assert lib.lg_ffn_pack(w.data_ptr(), w2.data_ptr(), None, 0, h, packed_c.data_ptr(), None) == 0
        outs = {}
        for mode in (0, 2, 3):
            prev = lib.lg_linear_set_ffn_fused(mode)
            try:
                outs[mode] = mt._Hip.ffn(x, c0, c1, w, b, ln, w2, b2, wp)
            finally:
                lib.lg_linear_set_ffn_fused(prev)
        default = mt._Hip.ffn(x, c0, c1, w, b, ln, w2, b2, wp)
        no_pack = mt._Hip.ffn(x, c0, c1, w, b, ln, w2, b2)  # (without the packed stream: the two calls)
        ref = _ffn_torch(x, c0, c1, w, b, ln, w2, b2)
        torch.cuda.synchronize()
    two = outs[0].float()
    err_two = float((two - ref.float()).abs().max())
    for mode, name in ((2, "rows32"), (3, "rows16")):
        rows = outs[mode].float()
        assert torch.isfinite(rows).all(), name
        d = (rows - two).abs()
        err_rows = float((rows - ref.float()).abs().max())
        print(f"ffn {name} P={pairs} {n0}x{n1}: |rows - two| max {float(d.max()):.3e} ({int((d > 0).sum())} of "
              f"{d.numel()} differ), vs torch: rows {err_rows:.3e}, two calls {err_two:.3e}")
        assert bool((d <= _ulp_bound(two, x)).all()), (name, float(d.max()))
        assert err_rows <= 2e-2 and err_two <= 2e-2
    assert torch.equal(default, outs[3] if m <= 4096 else outs[2])  # the default: one launch, by size
    assert torch.equal(no_pack, outs[0]) and torch.equal(packed_c, wp)  # lg_ffn_pack == ffn_pack


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,n0,n1", [(1, 512, 512), (1, 1024, 1024), (1, 700, 1301), (3, 37, 70), (5, 1000, 1011),
                                         (16, 1024, 1024), (1, 1, 63), (2, 60, 1)])
def test_ffn_proj_equals_ffn_then_projection(pairs, n0, n1):
    """lg_linear_cat_ffn_proj (the FFN and, in the same launch, the projection of its output that the next
    attention needs) against lg_linear_cat_ffn followed by that projection's own call on the FFN's
    output — lg_linear_split2 (to_qk | to_v), lg_linear_qkv_rotary (Wqkv + rotary), lg_linear (the
    assignment head's 384 channels of a 512-row W3) — in the 32 / 64-row forms (lg_linear_set_ffn_fused(2))
    bitwise: the same k-step order and output arithmetic; in the 16-row form (3: each k32 step of the
    projection one v_mfma_f32_16x16x32_f16, the separate call's two k16 MFMAs) within 2 fp16 ulps (the
    rotary's products and sum can carry a 1-ulp difference of its input twice), its
    FFN output bitwise lg_linear_cat_ffn's in that form. Ragged rows, pairs whose rows cross workgroup and
    image boundaries."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import matcher as mt

    dev, dt, h = torch.device("cuda:0"), torch.float16, 4
    gen = torch.Generator().manual_seed(31 + pairs + n0)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    m = pairs * (n0 + n1)
    sp = (n0, n1, pairs)
    with torch.no_grad():
        x = rnd(1, m, 256) * 0.5
        c0, c1 = rnd(pairs, h, n0, 64), rnd(pairs, h, n1, 64)
        w, b = rnd(512, 512) * 0.05, rnd(512) * 0.1
        w2, b2 = rnd(256, 512) * 0.05, rnd(256) * 0.1
        ln = torch.nn.LayerNorm(512).to(dev, dt)
        ln.weight.copy_(1 + 0.1 * rnd(512))
        ln.bias.copy_(0.1 * rnd(512))
        ang = rnd(1, m, 32).float()
        cos = torch.cos(ang).repeat_interleave(2, -1).to(dt).contiguous()
        sin = torch.sin(ang).repeat_interleave(2, -1).to(dt).contiguous()
        w3s, b3s = rnd(512, 256) * 0.06, rnd(512) * 0.1
        w3q, b3q = rnd(768, 256) * 0.06, rnd(768) * 0.1
        w3h, b3h = rnd(512, 256) * 0.06, rnd(512) * 0.1
        w3h[384:], b3h[384:] = 0, 0
        res = {}
        for mode in (2, 3):
            prev = mt._lib.load().lg_linear_set_ffn_fused(mode)
            try:
                ref_x = mt._Hip.ffn(x, c0, c1, w, b, ln, w2, b2, mt.ffn_pack(w, w2))
                got_s = mt._Hip.ffn_proj(x, c0, c1, b, ln, b2, mt.ffn_pack(w, w2, w3s), 1, b3s, sp)
                got_q = mt._Hip.ffn_proj(x, c0, c1, b, ln, b2, mt.ffn_pack(w, w2, w3q), 2, b3q, sp, cos, sin)
                got_h = mt._Hip.ffn_proj(x, c0, c1, b, ln, b2, mt.ffn_pack(w, w2, w3h), 3, b3h, sp, n_store=384)
            finally:
                mt._lib.load().lg_linear_set_ffn_fused(prev)
            ref_s = mt._Hip.linear_split2(ref_x, w3s, b3s, h, sp)
            ref_q = mt._Hip.linear_qkv_rotary(ref_x, w3q, b3q, cos, sin, h, sp)
            ref_h = mt._Hip.linear(ref_x, w3h[:384].contiguous(), b3h[:384].contiguous())
            res[mode] = (ref_x, got_s, got_q, got_h, ref_s, ref_q, ref_h)
        torch.cuda.synchronize()
    flat = lambda o: [t for u in o for t in u]  # noqa: E731
    for mode, (ref_x, got_s, got_q, got_h, ref_s, ref_q, ref_h) in res.items():
        for got in (got_s, got_q, got_h):
            assert torch.equal(got[0], ref_x), mode
        worst = 0.0
        for a_, b_ in zip(flat(got_s[1]) + flat(got_q[1]) + [got_h[1]], flat(ref_s) + flat(ref_q) + [ref_h]):
            d = (a_.float() - b_.float()).abs()
            worst = max(worst, float(d.max()))
            if mode == 2:
                assert torch.equal(a_, b_), float(d.max())
            else:
                assert bool((d <= torch.clamp(b_.float().abs(), min=2.0 ** -2) * 2.0 ** -9).all()), float(d.max())
        print(f"ffn_proj form {mode} P={pairs} {n0}x{n1}: projections vs separate calls max {worst:.3e}")


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,m,n", [(1, 64, 48), (3, 300, 256), (1, 130, 216), (1, 1024, 1024), (16, 1024, 1024),
                                     (2, 2048, 2000), (1, 2048, 2048), (1, 1003, 1016), (1, 1, 8), (5, 37, 1024)])
def test_assign_scores_kernel(pairs, m, n):
    """lg_assign_scores (the fp16 assignment head: sim = m0 · m1ᵀ by MFMA and each row's / column's exact
    logsumexp in one launch, the combine in a second; lightglue.py:208-233) against (1) torch's fp16 bmm
    for sim (fp32 accumulation, fp16 out: within one fp16 ulp, the accumulation order differing), (2)
    the torch restatement of the dual log-softmax on the kernel's own sim (the workspace copy: 2e-5 of
    the scale) and (3) that restatement on torch's sim (2 ulps of the similarity scale). These figures
    are empirical and kept for continuity at the matcher's sizes; the derived per-element bound against a
    float64 reference of the operands (tests/assignment_refs.py) is held by tests/test_gpu_assignment.py."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import _lib
    from lightglue_amd import matcher as mt

    lib = _lib.load()
    dev, dt = torch.device("cuda:0"), torch.float16
    gen = torch.Generator().manual_seed(pairs * 11 + m + n)
    with torch.no_grad():
        v = (torch.randn(pairs, m + n, 384, generator=gen) * 0.25).to(dev, dt)
        got = mt._Hip.assign_scores(v, m, 256)
        ws_sim = mt._Hip._last_assign_ws[:pairs * m * n * 2].view(dt).view(pairs, m, n).clone()
        sim_t = torch.bmm(v[:, :m, :256], v[:, m:, :256].transpose(1, 2))
        z0, z1 = v[:, :m, 256:257].float(), v[:, m:, 256:257].float()
        ref_own = mt.log_double_softmax(ws_sim.float(), z0, z1)
        ref_t = mt.log_double_softmax(sim_t.float(), z0, z1)
        torch.cuda.synchronize()
    d_sim = (ws_sim.float() - sim_t.float()).abs()
    ulp = torch.clamp(sim_t.float().abs(), min=2.0 ** -14) * 2.0 ** -10
    scale = max(1.0, float(sim_t.float().abs().max()))
    e_own, e_t = float((got - ref_own).abs().max()), float((got - ref_t).abs().max())
    print(f"assign scores P={pairs} {m}x{n}: sim differs in {int((d_sim > 0).sum())} of {d_sim.numel()} (max "
          f"{float(d_sim.max()):.2e}); scores vs restatement on own sim {e_own:.2e}, on torch's sim {e_t:.2e}")
    assert bool((d_sim <= ulp).all())
    assert torch.isfinite(got).all() and e_own <= 2e-5 * scale * 4 and e_t <= 2 * scale * 2.0 ** -10 * 4


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,m,n", [(1, 64, 48), (3, 300, 256), (1, 130, 211), (16, 1024, 1024), (2, 2048, 2000),
                                     (1, 2048, 2048), (1, 1003, 1016)])
def test_fp16_head_and_inputs_kernels(pairs, m, n):
    """The fp16 forward's own kernels around the layers: lg_pair_inputs (pair-major x = the torch cat
    bit for bit; cos / sin = the fp16 FourierPositionalEncoding within one fp16 ulp) and
    lg_log_double_softmax_f16 (fp16 sim and strided fp16 matchability logits read directly) against
    the torch restatement of lightglue.py:197-205 on the same fp16 inputs — both of its launch
    shapes: 64-row blocks (16 x 1024, 2 x 2048) and, below 64 of those, 8-row blocks with the
    separate column pass (single pairs up to 2048 x 2048, three pairs of 300 rows). The figures below
    (1e-3 on cos / sin, 1e-4 and 2e-4 max(1, |ref| / 16) on the scores) are empirical; both kernels are held
    to float64 references under derived bounds by tests/test_gpu_assignment.py (tests/assignment_refs.py)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import matcher as mt

    dev, dt = torch.device("cuda:0"), torch.float16
    gen = torch.Generator().manual_seed(pairs * 7 + m)
    rnd = lambda *s: torch.randn(*s, generator=gen).to(dev, dt)  # noqa: E731
    with torch.no_grad():
        d0, d1 = rnd(pairs, m, 256), rnd(pairs, n, 256)
        k0, k1 = rnd(pairs, m, 2), rnd(pairs, n, 2)
        pe = mt.FourierPositionalEncoding(2, 64).to(dev, dt)
        x, cos, sin = mt._Hip.pair_inputs(d0, d1, k0, k1, pe.Wr.weight)
        rc, rs = pe(torch.cat((k0, k1), 1))
        assert torch.equal(x.view(pairs, m + n, 256), torch.cat((d0, d1), 1))
        for got, ref in ((cos, rc), (sin, rs)):
            assert float((got.view(pairs, m + n, 64).float() - ref.reshape(pairs, m + n, 64).float()).abs().max()) <= 1e-3
        if n % 8:
            return
        v = rnd(pairs, m + n, 384) * 2
        sim = rnd(pairs, m, n) * 4
        got = mt._Hip.log_double_softmax_f16(sim, v, m, 256)
        ref = mt.log_double_softmax(sim.float(), v[:, :m, 256:257].float(), v[:, m:, 256:257].float())
        torch.cuda.synchronize()
    err = float((got - ref).abs().max())
    print(f"dual log-softmax f16 P={pairs} {m}x{n}: max-abs {err:.3e}")
    assert err <= 2e-4 * max(1.0, float(ref.abs().max()) / 16)


# Random shapes through the chained fp16 forward (round 6): the 16-row FFN kernel with and without its
# split projection, the 32 / 64-row kernels, ragged row counts (partial tiles, images of a few rows,
# pairs whose rows cross tiles), every chain kind's fused projection and the two-launch head — against
# the same fp16 model with the framework's ops around our attention (glue='torch', one pair at a time),
# every element, at the batched-vs-single bound (two fp16 forwards' rounding spread).
RANDOM_SHAPES = int(os.environ.get("LG_RANDOM_SHAPES", "12"))  # (LG_RANDOM_SHAPES=n widens it, one-off)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(RANDOM_SHAPES))
def test_matcher_random_shapes_chained_vs_torch_glue(case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from lightglue_amd import matcher

    rng = np.random.default_rng(9000 + case)
    pairs = int(rng.choice([1, 1, 1, 2, 3, 5]))
    n0 = int(rng.choice([int(rng.integers(1, 64)), int(rng.integers(64, 1100)), int(rng.integers(1100, 2049))],
                        p=[0.2, 0.6, 0.2]))
    n1 = 8 * int(rng.integers(1, 256))  # (the fp16 head kernel takes n1 % 8 == 0)
    dev, dt = torch.device("cuda:0"), torch.float16
    sd = matcher.seeded_state_dict(7, 9)
    outs = {}
    for glue in ("hip", "torch"):
        m = matcher.LightGlueMatcher(n_layers=9, glue=glue).eval()
        m.load_state_dict(sd, strict=True)
        m = m.to(dev, dt)
        ps = [matcher.synthetic_pair(500 + 13 * case + i, n0, n1) for i in range(pairs)]
        batch = tuple(torch.cat([p[j] for p in ps], 0).to(dev, dt) for j in range(4))
        with torch.no_grad():
            outs[glue] = m(*batch)
    torch.cuda.synchronize()
    tol_d, tol_s = BATCHED_VS_SINGLE["float16"]
    (d0, d1, sc), (r0, r1, rs) = outs["hip"], outs["torch"]
    assert sc.shape == (pairs, n0, n1) and torch.isfinite(sc).all()
    ed = max(float((d0 - r0).abs().max()), float((d1 - r1).abs().max()))
    es = float((sc - rs).abs().max())
    print(f"random shape {case}: P={pairs} {n0}x{n1} rows {pairs * (n0 + n1)}: desc {ed:.3e} scores {es:.3e}")
    assert ed <= tol_d and es <= tol_s, (pairs, n0, n1, ed, es)
