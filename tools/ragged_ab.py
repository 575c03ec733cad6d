"""A/B on one GPU: a ragged batch of 16 image pairs through LightGlueMatcher.match_pairs (one padded
forward with per-pair counts: lens forms of the streaming attention kernel and of the match head)
against (a) 16 single-pair match_batch calls on the routing every pair takes without counts (n % 8 != 0
pairs take the per-layer path and framework ops) and (b) an equal-size P = 16 batch at 1024 x 1024
(what the padded forward would cost if no key were masked, and the figure to compare between commits:
it runs the streaming instantiation without counts). fp16, 9 layers, seeded weights; the 16 pairs'
keypoint counts are drawn, seeded, from [600, 1024] for each image.

Method (tools/match_head_ab.py's): one process; every form warmed up; per repeat the forms alternate,
each timed by a host clock around a window of calls that ends in a device synchronise, the window
sized from the warm-up to last at least --window seconds; the comparison repeated --repeats times, so
every figure comes with its spread (min / median / max of the per-call time over the repeats).

    python tools/ragged_ab.py [--pairs 16] [--lo 600] [--hi 1024] [--repeats 5] [--window 0.3]
                              [--out profiles/ragged/ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd")]
import torch  # noqa: E402

from lightglue_amd import matcher as mt  # noqa: E402
from lightglue_amd import synth  # noqa: E402


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--lo", type=int, default=600)
    ap.add_argument("--hi", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ragged", "ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ragged_ab.py: needs a GPU (timings from anywhere else mean nothing)")
    dev, dt = torch.device("cuda:0"), torch.float16
    model = mt.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(mt.seeded_state_dict(7, 9), strict=True)
    model = model.to(dev, dt)
    P = args.pairs
    u = synth.uniform24(20260, 2 * P)
    sizes = [(args.lo + int(u[2 * p] * (args.hi - args.lo + 1)), args.lo + int(u[2 * p + 1] * (args.hi - args.lo + 1)))
             for p in range(P)]
    pairs = [tuple(t.to(dev, dt) for t in mt.synthetic_pair(300 + p, m, n, overlap=min(m, n) // 2))
             for p, (m, n) in enumerate(sizes)]
    flat = [tuple(t[0] for t in p) for p in pairs]
    full = [mt.synthetic_pair(300 + p, args.hi, args.hi, overlap=args.hi // 2) for p in range(P)]
    equal = tuple(torch.cat([p[j] for p in full], 0).to(dev, dt) for j in range(4))
    forms = {
        "ragged_match_pairs": lambda: model.match_pairs(flat),
        "per_pair_loop": lambda: [model.match_batch(*p) for p in pairs],
        "equal_size_batch": lambda: model.match_batch(*equal),
    }
    with torch.no_grad():
        calls = {}
        for name, fn in forms.items():   # warm-up, and the window's length from it
            _window(fn, 3)
            calls[name] = max(3, int(args.window / _window(fn, 3)) + 1)
        # the ragged batch finds the matches the pairs get alone (its own tests check every field)
        got = model.match_pairs(flat)[0]
        alone = [model.match_batch(*p) for p in pairs]
        hit = tot = 0
        for p in range(P):
            a = {tuple(x) for x in alone[p].matches[0, :int(alone[p].counts[0])].tolist()}
            g = {tuple(x) for x in got.matches[p, :int(got.counts[p])].tolist()}
            hit, tot = hit + len(a & g), tot + len(a)
        ms = {name: [] for name in forms}
        for _ in range(args.repeats):
            for name, fn in forms.items():
                ms[name].append(1e3 * _window(fn, calls[name]))
    rec = {"P": P, "sizes": sizes, "padded_to": [max(m for m, _ in sizes), (max(n for _, n in sizes) + 7) // 8 * 8],
           "dtype": "float16", "repeats": args.repeats, "calls_per_window": calls,
           "matches_alone": tot, "of_them_in_the_ragged_batch": hit}
    for name, t in ms.items():
        rec[name + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4), "max": round(max(t), 4)}
    # faster by more than the spread: the slowest ragged window under the fastest per-pair window
    rec["ragged_faster_than_loop_beyond_spread"] = max(ms["ragged_match_pairs"]) < min(ms["per_pair_loop"])
    rec["speedup_median_vs_loop"] = round(statistics.median(ms["per_pair_loop"]) / statistics.median(ms["ragged_match_pairs"]), 3)
    rec["ragged_over_equal_size_median"] = round(statistics.median(ms["ragged_match_pairs"]) /
                                                 statistics.median(ms["equal_size_batch"]), 3)
    rec["pairs_per_s_ragged"] = round(P / (statistics.median(ms["ragged_match_pairs"]) * 1e-3), 1)
    line = json.dumps(rec)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as out:
        out.write(line + "\n")


if __name__ == "__main__":
    main()
