"""A/B timing of the attention backward (csrc/mha_hd64_backward.hip) against the framework's, by graph replay.

Arms, alternated in one process, medians of 9 replays after warm-up, each replay CALLS calls:
  ours            mha_hd64_backward alone (Q, K, V, the saved O and dO given)
  sdpa_fwd        F.scaled_dot_product_attention forward, fp16
  sdpa_fwd_bwd    the same forward plus its backward; the baseline is sdpa_fwd_bwd - sdpa_fwd
and, with --splits, ours once per forced query split of the column kernel (MHA_HD64_BWD_SPLITS), each next
to the default, for the split decision in DESIGN.md. Appends one JSON line per shape to --out.

    python tools/attention_backward_ab.py [--shapes 1x4x1024x1024,...] [--splits 1,2,4,8,16] [--out ...]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1x4x1024x1024,1x4x2048x2048,16x4x1024x1024")
    ap.add_argument("--splits", default="", help="forced splits to time as well, on the first and last shape")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attention_backward", "ab.jsonl"))
    args = ap.parse_args()
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
