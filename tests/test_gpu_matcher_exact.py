"""The matcher's composed fp16 forward on the MI355X (LightGlueMatcher._forward_chain -> TransformerLayer.fused_step
-> the derived weights of weights.py), layer by layer against the float64 layer of tests/matcher_refs.py.

The criterion is test_gpu_superpoint.py's (test_encoder_within_twice_the_storage_models_error), per layer and per
pair: with exact = the float64 layer and model = the same layer with the kernels' fp16 stores, BOTH computed from the
GPU's own fp16 input to that layer (so nothing compounds and every layer is judged at its own scale),
    max |ours - exact| <= 2 E,   E = max |model - exact|   (maxima over the pair's valid rows and all channels).
The kernels implement the model up to the order of their fp32 sums, which flips single fp16 roundings of the size E
already counts. tests/test_matcher_reference.py shows on the CPU that this accepts fp32 arithmetic (ratios 0.85-1.16)
and rejects nine wiring mutants by 10 x and more. The per-layer x comes from driving fused_step with _forward_chain's
folding decisions; that loop's final x and scores must be, bit for bit, what model(*batch) returns, which also pins
_forward_chain to the loop. Every ratio is printed (pytest -s).

Cases (matcher_refs.CASES), by the one-launch FFN kernel the row count selects (launch_ffn_rows, kTileGrid = 256; no
route reporter exists, so the arithmetic is matcher_refs.ffn_rows_form's): a 64 rows and b 858 rows: 16-row tiles,
at most 64 of them, the projection split over two workgroups; c 1430 rows: 90 tiles, the whole 16-row kernel; d 4216
rows > 4096: the 32-row kernel; e 8432 rows > 8192: the 64-row kernel.
"""
import pytest
import torch

import matcher_refs as R
from gpu_common import equal_results, same_bits, seeded_matcher

pytestmark = pytest.mark.gpu

L = 9
FACTOR = 2.0
FFN_FORM = {"a": "rows16 split", "b": "rows16 split", "c": "rows16", "d": "rows32", "e": "rows64"}
CHECKED_LAYERS = {"a": range(L), "b": range(L), "c": range(2), "d": range(2), "e": range(2)}
FORMS = ("", "s", "h", "sh", "sqh")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    return seeded_matcher(dev, L, 7)


@pytest.fixture(scope="module")
def refs():
    from lightglue_amd import matcher

    sd = matcher.seeded_state_dict(7, L)
    return [R.layer_weights(sd, li) for li in range(L)], R.head_weights(sd, L - 1)


def chain_loop(model, batch, lens=None):
    """_forward_chain's loop, keeping every layer's x: (xs [L + 1] of [1, P (m + n), 256], cos, sin, scores)."""
    from lightglue_amd.glue import _Hip
    from lightglue_amd.layers import _lens_attention

    pr, m, n = batch[2].shape[0], batch[2].shape[1], batch[3].shape[1]
    x, cos, sin = model._inputs(*batch, True)
    assert model.chain_ok(x, m, n)
    kinds, layers = model._chain_kinds(), model.transformers
    head = model.log_assignment[L - 1]
    attn_self, attn_cross = (model.attention, model.attention) if lens is None else _lens_attention(lens)
    xs, qkv = [x], None
    for li, layer in enumerate(layers):
        last = li + 1 == L
        then = (head if last else layers[li + 1].self_attn) if ("h" if last else "q") in kinds else None
        x, qkv, v = layer.fused_step(x, cos, sin, (m, n, pr), qkv, attn_self, attn_cross, "s" in kinds, then)
        xs.append(x)
    v = v.view(pr, m + n, 384) if v is not None else head.project_rows(x, pr, m, n)
    return xs, cos, sin, _Hip.assign_scores(v, m, x.shape[-1], lens)


_RUNS = {}


def run_case(model, dev, name):
    """The loop on a case (or 'ragged': case b with RAGGED_COUNTS and NaN padding), once per session, on the CPU:
    dict(xs, cos, sin float64 [P, m + n, .], scores, counts, batch, lens)."""
    if name in _RUNS:
        return _RUNS[name]
    case = "b" if name == "ragged" else name
    pr, m, n, _ = R.CASES[case]
    batch = [t.clone() for t in R.case_batch(case)]
    counts, lens = ([m] * pr, [n] * pr), None
    if name == "ragged":
        counts = R.RAGGED_COUNTS
        for p in range(pr):
            for t, c in ((batch[0], counts[0][p]), (batch[1], counts[1][p]), (batch[2], counts[0][p]), (batch[3], counts[1][p])):
                t[p, c:] = float("nan")
        lens = tuple(torch.tensor(c, dtype=torch.int32, device=dev) for c in counts)
    batch = tuple(t.to(dev) for t in batch)
    with torch.no_grad():
        xs, cos, sin, scores = chain_loop(model, batch, lens)
        torch.cuda.synchronize()
    cpu = lambda t: t.cpu().double().view(pr, m + n, -1)
    _RUNS[name] = dict(xs=[cpu(x) for x in xs], x_last=xs[-1], cos=cpu(cos), sin=cpu(sin), scores=scores, counts=counts,
                       batch=batch, lens=lens, dims=(pr, m, n))
    return _RUNS[name]


def valid_rows(t, p, m, counts):
    """Pair p's valid rows of t [P, m + n, C]: image 0's, then image 1's."""
    return torch.cat((t[p, :counts[0][p]], t[p, m:m + counts[1][p]]), 0)


def pair_lists(run, x):
    pr, m, _ = run["dims"]
    c = run["counts"]
    return ([valid_rows(x, p, m, c) for p in range(pr)],
            [(valid_rows(run["cos"], p, m, c), valid_rows(run["sin"], p, m, c)) for p in range(pr)],
            [(c[0][p], c[1][p]) for p in range(pr)])


def check_teacher_forced(name, run, refs, layers):
    """Every layer of `layers` from the GPU's own input to it: ours / E per pair, printed; all <= FACTOR."""
    pr, m, _ = run["dims"]
    worst = []
    with torch.no_grad():
        for li in layers:
            ins, tabs, dims = pair_lists(run, run["xs"][li])
            assert all(bool(torch.isfinite(x).all()) for x in ins), (name, li)
            exact = R.layer(refs[0][li], ins, tabs, dims)
            stored = R.layer(refs[0][li], ins, tabs, dims, R.half)
            ours = [valid_rows(run["xs"][li + 1], p, m, run["counts"]) for p in range(pr)]
            e = [R.max_err(a, b) for a, b in zip(stored, exact)]
            ratio = [R.max_err(a, b) / ee for a, b, ee in zip(ours, exact, e)]
            head = f"case {name} layer {li}: ours / E"
            es = " ".join(f"{v:.2e}" for v in e) if pr <= 5 else f"{min(e):.2e} .. {max(e):.2e}"
            print(head + " " + " ".join(f"{r:.2f}" for r in ratio) + " | E " + es)
            worst.append(max(ratio))
    assert max(worst) <= FACTOR, (name, [round(w, 3) for w in worst])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_layers_within_twice_the_storage_models_error(dev, model, refs, name):
    pr, m, n, _ = R.CASES[name]
    assert R.ffn_rows_form(pr * (m + n)) == FFN_FORM[name]
    run = run_case(model, dev, name)
    with torch.no_grad():
        d0, d1, scores = model(*run["batch"])
    x = run["x_last"].view(pr, m + n, 256)
    assert same_bits(d0, x[:, :m]) and same_bits(d1, x[:, m:]) and same_bits(scores, run["scores"]), "loop != model(*batch)"
    check_teacher_forced(name, run, refs, CHECKED_LAYERS[name])


def test_ragged_batch_with_poisoned_padding(dev, model, refs):
    """Case b with counts ([150, 120, 33], [136, 97, 120]) as device tensors and NaN in every padded descriptor and
    keypoint row; the float64 side sees the valid rows only."""
    run = run_case(model, dev, "ragged")
    pr, m, n = run["dims"]
    c0, c1 = run["counts"]
    with torch.no_grad():
        d0, d1, scores = model(*run["batch"], counts0=run["lens"][0], counts1=run["lens"][1])
    x = run["x_last"].view(pr, m + n, 256)
    for p in range(pr):
        assert same_bits(d0[p, :c0[p]], x[p, :c0[p]]) and same_bits(d1[p, :c1[p]], x[p, m:m + c1[p]]), "loop != model(*batch)"
        assert bool(torch.isfinite(scores[p, :c0[p], :c1[p]]).all())
    assert same_bits(scores, run["scores"])
    check_teacher_forced("ragged", run, refs, range(L))


@pytest.mark.parametrize("name", ("a", "b"))
def test_head_scores_from_the_chained_path(dev, model, refs, name):
    """The scores of the chained path (the head's projection folded into the last FFN launch, kind 3) against the
    float64 head on the GPU's final x, under the same rule, on finite entries."""
    run = run_case(model, dev, name)
    assert "h" in model._chain_kinds()
    pr, m, _ = run["dims"]
    ratios = []
    with torch.no_grad():
        for p in range(pr):
            x = run["xs"][L][p]
            exact, stored = R.head(refs[1], x, m), R.head(refs[1], x, m, R.half)
            ours = run["scores"][p].cpu().double()
            ok = torch.isfinite(exact) & torch.isfinite(stored)
            assert bool(ok.any()) and bool(torch.isfinite(ours[ok]).all())
            e = R.max_err(stored[ok], exact[ok])
            ratios.append(R.max_err(ours[ok], exact[ok]) / e)
            print(f"case {name} head pair {p}: E {e:.2e}, ours / E {ratios[-1]:.2f}")
    assert max(ratios) <= FACTOR, ratios


@pytest.mark.parametrize("name", ("b", "ragged"))
def test_folded_forms_give_the_same_bits(dev, model, name):
    """chain_kinds '', 's', 'h', 'sh', 'sqh' (the attribute, not the environment): final x, scores and match_batch's
    result bit for bit equal; on the ragged batch the descriptors on valid rows (padded rows are unspecified)."""
    run = run_case(model, dev, name)
    pr, m, n = run["dims"]
    kw = {} if run["lens"] is None else dict(counts0=run["lens"][0], counts1=run["lens"][1])
    outs = {}
    try:
        for kinds in FORMS:
            model.chain_kinds = kinds
            with torch.no_grad():
                outs[kinds] = (model(*run["batch"], **kw), model.match_batch(*run["batch"], **kw))
    finally:
        del model.chain_kinds
    torch.cuda.synchronize()
    (d0, d1, sc), res = outs[FORMS[0]]
    # (the pairs at descriptor scale 1/16 have no match above the threshold; pair 1 has some)
    assert int(res.counts.max()) >= 1
    for kinds in FORMS[1:]:
        (e0, e1, es), eres = outs[kinds]
        for p in range(pr):
            a, b = run["counts"][0][p], run["counts"][1][p]
            assert same_bits(d0[p, :a], e0[p, :a]) and same_bits(d1[p, :b], e1[p, :b]), (kinds, p)
        assert same_bits(sc, es), kinds
        equal_results(res, eres, f"match_batch, chain_kinds {kinds!r}")


@pytest.mark.parametrize("name", ("a", "b"))
def test_free_running_ratio_is_recorded(dev, model, refs, name):
    """Nine layers free-running from the GPU's layer-0 input: |ours - exact| against the free-running model's E.
    Printed, NOT asserted: rounding differences amplify from layer to layer by a factor nobody has derived (the CPU's
    fp32 proxy gave 0.78-1.18, which is no bound for the GPU); the teacher-forced checks are the assertions."""
    run = run_case(model, dev, name)
    pr, m, _ = run["dims"]
    ins, tabs, dims = pair_lists(run, run["xs"][0])
    with torch.no_grad():
        ex, es = R.forward(refs[0], refs[1], ins, tabs, dims)
        mx, ms = R.forward(refs[0], refs[1], ins, tabs, dims, R.half)
    for p in range(pr):
        e, es_ = R.max_err(mx[p], ex[p]), R.max_err(ms[p], es[p])
        ours = R.max_err(run["xs"][L][p], ex[p])
        ours_s = R.max_err(run["scores"][p].cpu(), es[p])
        print(f"case {name} free-running pair {p}: x E {e:.2e} ours / E {ours / e:.2f} | scores E {es_:.2e} ours / E {ours_s / es_:.2f}")
        assert bool(torch.isfinite(run["xs"][L][p]).all())
