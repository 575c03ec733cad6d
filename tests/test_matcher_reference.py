"""The float64 layer of tests/matcher_refs.py, on the CPU: that its exact form IS the model's layer and head, that the
criterion of tests/test_gpu_matcher_exact.py (max |ours - exact| <= 2 E per layer and pair, E the storage model's own
error from the same fp16 input) accepts fp32 arithmetic with the kernels' stores, and that it rejects every wiring
mutant by a factor of ten at a layer named here. No GPU, and nothing is read from the reference tree: the module this
pins the restatement to reproduces the reference's golden outputs (test_matcher.py, and once more below).

Inputs: the GPU test's cases a (one pair 40 x 24) and b (three pairs 150 x 136 at descriptor scales 1/16, 4, 1/16),
weights seeded_state_dict(7, 9). Each layer's input is the fp32 proxy's own previous output rounded to fp16 (a stand-in
for the GPU's), the same for exact, model, proxy and mutants: teacher-forced, as on the GPU.
"""
import json
import os

import numpy as np
import pytest
import torch

import matcher_refs as R

L = 9
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL_CPU = 1e-4          # test_matcher.py's, for the module against the golden outputs
PIN = 1e-12             # restatement against the module, float64
FACTOR = 2.0            # the criterion's
MARGIN = 10.0           # every mutant misses the criterion by at least this, where MUTANT_AT says
# (case, layer) at which the mutant must miss 2 E by MARGIN, on every pair of the case but for cross_next, whose last
# pair of case b reads pair 0 (the same scale) and is judged on pairs 0 and 1. fold_bias shows where the biases
# matter against x (layer 0); the rotary mutants where the attention has become selective.
MUTANT_AT = {"fold_bias": ("a", 0), "rot_shift": ("a", 4), "rot_v": ("a", 4), "self_all": ("a", 8), "cross_own": ("a", 4),
             "no_residual": ("a", 4), "no_scale": ("a", 0), "cross_next": ("b", 4), "rot_other": ("a", 4)}


def softmax64(calls):
    return [torch.matmul((q / 8 @ k.transpose(-1, -2)).softmax(-1), v) for q, k, v in calls]


@pytest.fixture(scope="module")
def sd():
    from lightglue_amd import matcher

    return matcher.seeded_state_dict(7, L)


@pytest.fixture(scope="module")
def module64(sd):
    from lightglue_amd import matcher

    m = matcher.LightGlueMatcher(n_layers=L, glue="torch", attention=softmax64).eval().double()
    m.load_state_dict({k: v.half().double() for k, v in sd.items()}, strict=True)
    return m


def case_pairs(sd, name):
    pr, m, n, _ = R.CASES[name]
    k0, k1, d0, d1 = R.case_batch(name)
    ins = [R.pair_inputs(sd, k0[p], k1[p], d0[p], d1[p]) for p in range(pr)]
    return [i[0] for i in ins], [(i[1], i[2]) for i in ins], [(m, n)] * pr


@pytest.fixture(scope="module")
def runs(sd):
    """Per case: per layer the proxy's ratio and every mutant's, per pair (computed once for all tests)."""
    torch.manual_seed(0)
    out = {}
    w64 = [R.layer_weights(sd, li) for li in range(L)]
    w32 = [R.layer_weights(sd, li, torch.float32) for li in range(L)]
    with torch.no_grad():
        for name in ("a", "b"):
            xs, tabs, dims = case_pairs(sd, name)
            tabs32 = [(c.float(), s.float()) for c, s in tabs]
            rows = []
            for li in range(L):
                xs = [R.half(x) for x in xs]
                exact = R.layer(w64[li], xs, tabs, dims)
                model = R.layer(w64[li], xs, tabs, dims, R.half)
                proxy = R.layer(w32[li], [x.float() for x in xs], tabs32, dims, R.half)
                e = [R.max_err(a, b) for a, b in zip(model, exact)]
                rec = {"E": e, "proxy": [R.max_err(a, b) / ee for a, b, ee in zip(proxy, exact, e)]}
                for mut in R.MUTANTS:
                    got = R.layer(w64[li], xs, tabs, dims, R.half, mut)
                    rec[mut] = [R.max_err(a, b) / (FACTOR * ee) for a, b, ee in zip(got, exact, e)]
                rows.append(rec)
                xs = [p.double() for p in proxy]
            out[name] = rows
    return out


def test_exact_form_is_the_modules_layer_and_head(sd, module64):
    """rnd = ident: every layer's output and the scores equal LightGlueMatcher(glue='torch', float64 softmax
    attention).double() on the fp16-rounded weights to 1e-12, layer by layer from the module's own x."""
    xs, tabs, dims = case_pairs(sd, "a")
    (m, n), x, (cos, sin) = dims[0], xs[0], tabs[0]
    worst = 0.0
    with torch.no_grad():
        for li, lay in enumerate(module64.transformers):
            want = lay(x[None], cos[None], sin[None], (m, n, 1), softmax64, False)[0]
            got = R.layer(R.layer_weights(sd, li), [x], [(cos, sin)], [(m, n)])[0]
            worst = max(worst, R.max_err(got, want))
            x = want
        # (MatchAssignment.forward casts the similarity to fp32: its own steps here, left in float64)
        from lightglue_amd.layers import log_double_softmax

        ha = module64.log_assignment[L - 1]
        m0, m1 = ha.final_proj(x[None, :m]) / ha.scale, ha.final_proj(x[None, m:]) / ha.scale
        want = log_double_softmax(m0 @ m1.transpose(1, 2), ha.matchability(x[None, :m]), ha.matchability(x[None, m:]))[0]
        got = R.head(R.head_weights(sd, L - 1), x, m)
        assert R.max_err(want, ha(x[None, :m], x[None, m:])[0]) <= 1e-4  # (and those steps are its forward, to fp32)
    print(f"restatement vs module: layers {worst:.2e}, scores {R.max_err(got, want):.2e}")
    assert worst <= PIN and R.max_err(got, want) <= PIN * max(1.0, float(want.abs().max()))


def test_the_module_reproduces_the_reference(module64):
    """The same module class with the float64 softmax on the fp32 weights of the smallest golden case."""
    from lightglue_amd import matcher

    name = "match_l2_64x48"
    meta = json.load(open(os.path.join(GOLD, "matcher_index.json")))[name]
    g = np.load(os.path.join(GOLD, f"{name}.npz"))
    m = matcher.LightGlueMatcher(n_layers=meta["n_layers"], glue="torch", attention=softmax64).eval()
    m.load_state_dict(matcher.seeded_state_dict(meta["seed"], meta["n_layers"]), strict=True)
    with torch.no_grad():
        d0, d1, sc = m(*matcher.synthetic_pair(meta["seed"], meta["m"], meta["n"]))
    for got, key in ((d0, "desc0"), (d1, "desc1"), (sc, "scores")):
        assert R.max_err(got, torch.from_numpy(g[key])) <= TOL_CPU, key


def test_bound_accepts_fp32_arithmetic_with_the_kernels_stores(runs):
    worst = 0.0
    for name, rows in runs.items():
        for li, rec in enumerate(rows):
            print(f"case {name} layer {li}: E " + " ".join(f"{e:.2e}" for e in rec["E"]) + " | fp32 proxy / E " +
                  " ".join(f"{r:.2f}" for r in rec["proxy"]))
            worst = max(worst, max(rec["proxy"]))
    assert worst <= FACTOR, worst


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bound_rejects(runs, mutant):
    """max |mutant - exact| / (2 E): at least MARGIN at the layer MUTANT_AT names (printed for every layer)."""
    for name, rows in runs.items():
        for li, rec in enumerate(rows):
            print(f"{mutant} case {name} layer {li}: err / 2E " + " ".join(f"{r:.1f}" for r in rec[mutant]))
    name, li = MUTANT_AT[mutant]
    got = runs[name][li][mutant]
    if mutant == "cross_next":
        got = got[:2]
    assert min(got) >= MARGIN, (mutant, name, li, got)


def test_storage_model_differs_from_exact_only_by_stores(sd):
    """The model with rnd = a float64 no-op wrapper (not `ident`: the stored forms, folded weights and the log2
    domain) stays within the fold's and q~'s own fp16 roundings of exact: the two code paths state one layer."""
    xs, tabs, dims = case_pairs(sd, "a")
    w = R.layer_weights(sd, 0)
    with torch.no_grad():
        exact = R.layer(w, xs, tabs, dims)[0]
        model = R.layer(w, xs, tabs, dims, R.half)[0]
        folded = R.layer(w, xs, tabs, dims, lambda t: t)[0]
    e, f = R.max_err(model, exact), R.max_err(folded, exact)
    print(f"layer 0: stores {e:.2e}, folded weights alone {f:.2e}")
    assert f < e
