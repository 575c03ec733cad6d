"""A/B on one GPU: LightGlueMatcher.match_adaptive (adaptive depth and width: one host wait per checked
layer, fewer layers and fewer rows) against match_batch on the same inputs and stream. match_batch's
code and launches are what they were before match_adaptive existed, so it is the baseline. fp16, 9 layers,
seeded weights (seeded_state_dict(7) + seeded_confidence_state_dict(54)); P = 1 at 512 / 1024 / 2048
keypoints and P = 16 at 1024, `overlap` at half the points. Forms: match_batch, match_adaptive with the
knobs off (the same launches: the only timing condition is that it stays within match_batch's spread),
depth only, width only and both, with the knobs of tests/test_gpu_adaptive.py.

The seeded weights are not trained: where these runs stop and how many rows they drop says nothing about
real image pairs. What the lines measure is the price of the mechanism (token scores, the copy of the
stats and the wait for it, the compaction, the unfolded Wqkv projection) against the layers and rows it
removed in that run; each line reports the stop layer and the surviving counts next to both times.

Method (tools/ragged_ab.py's): one process; every form warmed up; per repeat the forms alternate, each
timed by a host clock around a window of calls that ends in a device synchronise, the window sized from
the warm-up to last at least --window seconds; --repeats repeats, so every figure comes with its spread.

    python tools/adaptive_ab.py [--repeats 5] [--window 0.3] [--out profiles/adaptive/ab.jsonl]
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

CASES = [(1, 512), (1, 1024), (1, 2048), (16, 1024)]
KNOBS = {"off": (-1.0, -1.0), "depth": (0.4, -1.0), "width": (-1.0, 0.98), "both": (0.4, 0.5)}
CONF_SEED = 54


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def _model(knobs, dev):
    model = mt.LightGlueMatcher(n_layers=9, depth_confidence=knobs[0], width_confidence=knobs[1]).eval()
    sd = mt.seeded_state_dict(7, 9)
    if model.adaptive:
        sd.update(mt.seeded_confidence_state_dict(CONF_SEED, 9))
    model.load_state_dict(sd, strict=True)
    return model.to(dev, torch.float16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adaptive", "ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adaptive_ab.py: needs a GPU (timings from anywhere else mean nothing)")
    dev = torch.device("cuda:0")
    models = {name: _model(k, dev) for name, k in KNOBS.items()}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for P, n in CASES:
        pairs = [mt.synthetic_pair(300 + p, n, n, overlap=n // 2) for p in range(P)]
        batch = tuple(torch.cat([p[j] for p in pairs], 0).to(dev, torch.float16) for j in range(4))
        forms = {"match_batch": lambda: models["off"].match_batch(*batch)}
        for name in KNOBS:
            forms["adaptive_" + name] = lambda name=name: models[name].match_adaptive(*batch)
        rec = {"P": P, "n": n, "overlap": n // 2, "dtype": "float16", "repeats": args.repeats, "knobs": KNOBS}
        with torch.no_grad():
            for name in ("depth", "width", "both"):   # what each adaptive run did
                trace = []
                res = models[name].match_adaptive(*batch, trace=trace)
                rec[name] = {"stop": res.stop, "rows_after_each_check": [list(e["dims"]) for e in trace],
                             "surviving0": [len(k) for k in trace[-1]["kept0"]],
                             "surviving1": [len(k) for k in trace[-1]["kept1"]],
                             "matches": res.result.counts.tolist()}
            rec["match_batch_matches"] = models["off"].match_batch(*batch).counts.tolist()
            calls = {}
            for name, fn in forms.items():   # warm-up, and the window's length from it
                _window(fn, 3)
                calls[name] = max(3, int(args.window / _window(fn, 3)) + 1)
            ms = {name: [] for name in forms}
            for _ in range(args.repeats):
                for name, fn in forms.items():
                    ms[name].append(1e3 * _window(fn, calls[name]))
        rec["calls_per_window"] = calls
        for name, t in ms.items():
            rec[name + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4), "max": round(max(t), 4)}
        base = ms["match_batch"]
        rec["knobs_off_within_match_batch_spread"] = min(ms["adaptive_off"]) <= max(base) and max(ms["adaptive_off"]) >= min(base)
        for name in ("depth", "width", "both"):
            rec[name + "_over_match_batch_median"] = round(statistics.median(ms["adaptive_" + name]) / statistics.median(base), 3)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as out:
            out.write(line + "\n")


if __name__ == "__main__":
    main()
