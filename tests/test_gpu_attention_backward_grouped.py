"""mha_hd64_backward_grouped_lens on ragged groups with NaN in every padded row, and as the grouped ops' autograd."""
import pytest
import torch

from gpu_common import capture_on_side_stream, same_bits
from lightglue_amd import attention_backward_reference, mha_hd64_backward, mha_hd64_backward_grouped, mha_hd64_batched
from test_gpu_attention_backward import BOUND, host

pytestmark = pytest.mark.gpu

L0, L1 = [70, 1, 33], [45, 40, 9]  # the layer group's image counts, mapped as the matcher maps them
# name -> (batch, heads, [(nq, nkv)], q_lens, kv_lens); a table of None: all rows; 0 and 999 are clamped into [1, n]
GROUPS = {
    "layer": (3, 4, [(70, 70), (45, 45), (70, 45), (45, 70)], [L0, L1, L0, L1], [L0, L1, L1, L0]),
    "tiles": (4, 1, [(130, 130)], [[130, 65, 64, 1]], [[1, 63, 130, 66]]),
    "chunked": (1, 2, [(9, 33), (17, 9), (33, 20), (25, 25), (12, 31)], [[5], None, [999], [25], [0]],
                [None, [9], [7], [999], [30]]),
}
_cache = {}


def table(lens):
    return [None if t is None else torch.tensor(t, dtype=torch.int32, device="cuda") for t in lens]


def group(name, pad=float("nan")):
    """(calls, outs, douts, clamped q_lens, kv_lens): O from the forward on each item's slices, `pad` in padded rows; built once."""
    if (name, pad) not in _cache:
        batch, heads, shapes, q_lens, kv_lens = GROUPS[name]
        g = torch.Generator().manual_seed(len(name))
        calls, outs, douts, ql, kl = [], [], [], [], []
        for (nq, nkv), qt, kt in zip(shapes, q_lens, kv_lens):
            q, do = (torch.randn(batch, heads, nq, 64, generator=g).half().cuda() for _ in range(2))
            k, v = (torch.randn(batch, heads, nkv, 64, generator=g).half().cuda() for _ in range(2))
            o = torch.empty_like(q)
            ql.append([min(max(c, 1), nq) for c in (qt or [nq] * batch)])
            kl.append([min(max(c, 1), nkv) for c in (kt or [nkv] * batch)])
            for b, (a, c) in enumerate(zip(ql[-1], kl[-1])):
                o[b:b + 1, :, :a] = mha_hd64_batched(*(t[b:b + 1, :, :r].contiguous() for t, r in ((q, a), (k, c), (v, c))))
                for t, r in ((q, a), (o, a), (do, a), (k, c), (v, c)):
                    t[b, :, r:] = pad
            calls.append((q, k, v)), outs.append(o), douts.append(do)
        _cache[name, pad] = (calls, outs, douts, ql, kl)
    return _cache[name, pad]


def run(name, q_lens=None, kv_lens=None):
    calls, outs, douts, _, _ = group(name)
    return mha_hd64_backward_grouped(calls, outs, douts, kv_lens=kv_lens or table(GROUPS[name][4]),
                                     q_lens=q_lens or table(GROUPS[name][3]))


def items(name, grads):
    """Per item: (its five input slices, contiguous; its gradients' valid regions; its gradients' padded rows)."""
    calls, outs, douts, ql, kl = group(name)
    for (q, k, v), o, do, g, qs, ks in zip(calls, outs, douts, grads, ql, kl):
        for b, (a, c) in enumerate(zip(qs, ks)):
            rows = (a, c, c)
            yield ([t[b:b + 1, :, :r].contiguous() for t, r in ((q, a), (k, c), (v, c), (o, a), (do, a))],
                   [t[b:b + 1, :, :r] for t, r in zip(g, rows)], [t[b:b + 1, :, r:] for t, r in zip(g, rows)])


@pytest.mark.parametrize("splits", ["1", None], ids=["one_split_bits", "planned_float64"])
@pytest.mark.parametrize("name", sorted(GROUPS))
def test_every_item_on_its_slices(name, splits, monkeypatch):
    """One split: the single-call backward's bits on the slices. Planned splits: float64 under that call's bounds."""
    monkeypatch.setenv("MHA_HD64_BWD_SPLITS", splits) if splits else monkeypatch.delenv("MHA_HD64_BWD_SPLITS", raising=False)
    for i, (ins, valid, padded) in enumerate(items(name, run(name))):
        assert all(bool(torch.isfinite(g).all()) for g in valid) and all(bool((p == 0).all()) for p in padded)
        if splits:
            assert all(same_bits(got, want) for got, want in zip(valid, mha_hd64_backward(*ins))), i
            continue
        q, k, v, _, do = (t.cpu() for t in ins)
        errs = [host.rel(g.cpu(), ref) for g, ref in zip(valid, attention_backward_reference(q, k, v, do))]
        print(name, i, tuple(q.shape), tuple(k.shape), " ".join(f"{e:.3e}" for e in errs))
        assert all(e <= b for e, b in zip(errs, BOUND[torch.float16])), (i, errs)


def test_reproducible_and_replayed_with_new_counts():
    q_lens, kv_lens = table(GROUPS["layer"][3]), table(GROUPS["layer"][4])
    first = run("layer", q_lens, kv_lens)
    for a, b in zip(first, run("layer", q_lens, kv_lens)):
        assert all(same_bits(x, y) for x, y in zip(a, b))
    graph, outs = capture_on_side_stream(lambda: run("layer", q_lens, kv_lens))
    new = {0: [5, 1, 33], 1: [45, 3, 9]}  # the images' new counts (at most the old: the rows past those hold NaN)
    for t, img in zip(q_lens + kv_lens, (0, 1, 0, 1, 0, 1, 1, 0)):
        t.copy_(torch.tensor(new[img], dtype=torch.int32))
    eager = run("layer", q_lens, kv_lens)
    for _ in range(2):
        for t in (t for g in outs for t in g):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert all(same_bits(x, y) for x, y in zip(a, b))
    assert not all(same_bits(x, y) for a, b in zip(first, eager) for x, y in zip(a, b))


@pytest.mark.parametrize("op", ["mha_hd64_grouped", "mha_hd64_grouped_lens", "mha_hd64_grouped_qkv_lens"])
def test_autograd_of_the_grouped_ops_is_the_c_abi_call(op):
    calls, _, douts, _, _ = group("layer", pad=0.5)  # (finite padding: two of the ops read padded rows)
    q_lens, kv_lens = table(GROUPS["layer"][3]), table(GROUPS["layer"][4])
    lens = {"mha_hd64_grouped": [], "mha_hd64_grouped_lens": [kv_lens], "mha_hd64_grouped_qkv_lens": [q_lens, kv_lens]}[op]
    fwd = getattr(torch.ops.lightglue_amd, op)
    leaves = [[t.clone().requires_grad_() for t in ts] for ts in zip(*calls)]
    outs = fwd(*leaves, *lens)
    strided = [d.transpose(2, 3).contiguous().transpose(2, 3) for d in douts]  # (non-contiguous gradients)
    torch.autograd.backward(outs, strided)
    want = mha_hd64_backward_grouped(calls, [o.detach() for o in outs], douts, kv_lens=lens[-1] if lens else None,
                                     q_lens=lens[0] if len(lens) == 2 else None)
    for i, triple in enumerate(want):
        assert all(same_bits(leaves[j][i].grad, triple[j]) for j in range(3))
    only = [list(ts) for ts in zip(*calls)]
    only[1][2] = only[1][2].clone().requires_grad_()
    torch.autograd.backward(fwd(*only, *lens), strided)
    assert same_bits(only[1][2].grad, want[2][1]) and all(t.grad is None for ts in (only[0], only[2]) for t in ts)
