"""A/B timing of the attention backward (csrc/mha_hd64_backward.hip) against the framework's, by graph replay.

Arms, alternated in one process, medians of 9 replays after warm-up, each replay CALLS calls:
  ours            mha_hd64_backward alone (Q, K, V, the saved O and dO given)
  sdpa_fwd        F.scaled_dot_product_attention forward, fp16
  sdpa_fwd_bwd    the same forward plus its backward; the baseline is sdpa_fwd_bwd - sdpa_fwd
and, with --splits, ours once per forced query split of the column kernel (MHA_HD64_BWD_SPLITS), each next
to the default, for the split decision in DESIGN.md. Appends one JSON line per shape to --out.

--grouped: a matcher layer's backward instead, its four attention calls (self0, self1, cross 0->1, cross 1->0) of
P x 4 x n x n at P = 1, 4, 16, n = 1024, as autograd issues them (the self pair, then the cross pair), per replay:
  grouped         two mha_hd64_backward_grouped calls of two calls each, every count n
  single          four mha_hd64_backward calls (the code before the grouped call existed)
  grouped_ragged  the grouped calls with per-pair counts drawn in [n/2, n]

    python tools/attention_backward_ab.py [--shapes 1x4x1024x1024,...] [--splits 1,2,4,8,16] [--out ...]
    python tools/attention_backward_ab.py --grouped [--out profiles/attention_backward/grouped_ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"))

import lightglue_amd  # noqa: E402

CALLS = 10


def captured(run):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(CALLS):
            run()
    return graph


def replay_ms(graph):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / CALLS


def measure(shape, splits):
    b, h, nq, nkv = shape
    g = torch.Generator(device="cuda").manual_seed(1)
    q, dout = (torch.randn(b, h, nq, 64, generator=g, device="cuda", dtype=torch.float16) for _ in range(2))
    k, v = (torch.randn(b, h, nkv, 64, generator=g, device="cuda", dtype=torch.float16) for _ in range(2))
    o = lightglue_amd.mha_hd64_batched(q, k, v)
    leaves = [t.clone().requires_grad_() for t in (q, k, v)]

    def sdpa_fwd():
        with torch.no_grad():
            return F.scaled_dot_product_attention(q, k, v)

    def sdpa_fwd_bwd():
        return torch.autograd.grad(F.scaled_dot_product_attention(*leaves), leaves, dout)

    arms = {"ours": captured(lambda: lightglue_amd.mha_hd64_backward(q, k, v, o, dout)),
            "sdpa_fwd": captured(sdpa_fwd), "sdpa_fwd_bwd": captured(sdpa_fwd_bwd)}
    for s in splits:
        os.environ["MHA_HD64_BWD_SPLITS"] = str(s)
        arms[f"ours_splits{s}"] = captured(lambda: lightglue_amd.mha_hd64_backward(q, k, v, o, dout))
        del os.environ["MHA_HD64_BWD_SPLITS"]
    times = {name: [] for name in arms}
    for rep in range(3 + 9):  # 3 warm-up rounds, then 9 timed, the arms alternating
        for name, graph in arms.items():
            t = replay_ms(graph)
            if rep >= 3:
                times[name].append(t)
    rec = {"shape": list(shape), "calls_per_replay": CALLS}
    for name, t in times.items():
        rec[name + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4), "max": round(max(t), 4)}
    rec["sdpa_bwd_median_ms"] = round(rec["sdpa_fwd_bwd_ms"]["median"] - rec["sdpa_fwd_ms"]["median"], 4)
    rec["ours_over_sdpa_bwd"] = round(rec["ours_ms"]["median"] / rec["sdpa_bwd_median_ms"], 3)
    return rec


def timed(arms):
    """{arm: min / median / max ms} of 9 replays after 3 warm-up rounds, the arms alternating."""
    times = {name: [] for name in arms}
    for rep in range(3 + 9):
        for name, graph in arms.items():
            t = replay_ms(graph)
            if rep >= 3:
                times[name].append(t)
    return {name + "_ms": {"min": round(min(t), 4), "median": round(statistics.median(t), 4), "max": round(max(t), 4)}
            for name, t in times.items()}


def measure_grouped(pairs, n):
    g = torch.Generator(device="cuda").manual_seed(pairs)
    rand = lambda: torch.randn(pairs, 4, n, 64, generator=g, device="cuda", dtype=torch.float16)  # noqa: E731
    full = [torch.full((pairs,), n, dtype=torch.int32, device="cuda") for _ in range(2)]
    some = [torch.randint(n // 2, n + 1, (pairs,), generator=g, device="cuda", dtype=torch.int32) for _ in range(2)]
    calls = [tuple(rand() for _ in range(3)) for _ in range(4)]
    douts = [rand() for _ in range(4)]
    outs = lightglue_amd.mha_hd64_grouped(calls)

    def grouped(c):
        for at, lens in ((0, (c[0], c[1])), (2, (c[1], c[0]))):  # self: own counts; cross i -> j: rows i, keys j
            lightglue_amd.mha_hd64_backward_grouped(calls[at:at + 2], outs[at:at + 2], douts[at:at + 2], kv_lens=list(lens),
                                                    q_lens=[c[0], c[1]])

    def single():
        for (q, k, v), o, do in zip(calls, outs, douts):
            lightglue_amd.mha_hd64_backward(q, k, v, o, do)

    rec = {"pairs": pairs, "n": n, "calls_per_replay": CALLS, "counts": [t.tolist() for t in some]}
    rec.update(timed({"grouped": captured(lambda: grouped(full)), "single": captured(single),
                      "grouped_ragged": captured(lambda: grouped(some))}))
    rec["grouped_over_single"] = round(rec["grouped_ms"]["median"] / rec["single_ms"]["median"], 3)
    rec["ragged_over_grouped"] = round(rec["grouped_ragged_ms"]["median"] / rec["grouped_ms"]["median"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x4x1024x1024,1x4x2048x2048,16x4x1024x1024")
    ap.add_argument("--splits", default="", help="forced splits to time as well, on the first and last shape")
    ap.add_argument("--grouped", action="store_true", help="time a layer's four calls: grouped against four single calls")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.out = args.out or os.path.join(REPO, "profiles", "attention_backward", "grouped_ab.jsonl" if args.grouped else "ab.jsonl")
    if args.grouped:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        for pairs in (1, 4, 16):
            rec = measure_grouped(pairs, 1024)
            print(json.dumps(rec))
            with open(args.out, "a") as f:
                f.write(json.dumps(rec) + "\n")
        return
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    splits = [int(s) for s in args.splits.split(",") if s]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for i, shape in enumerate(shapes):
        rec = measure(shape, splits if i in (0, len(shapes) - 1) else [])
        print(json.dumps(rec))
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
