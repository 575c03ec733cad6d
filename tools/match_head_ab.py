"""A/B on one GPU: LightGlueMatcher.match() (forward, then filter_matches pair by pair in framework
ops, one host synchronisation per pair) against match_batch() (the forward through the last FFN, then
lg_assign_matches: no scores tensor, no framework op, no synchronisation), and forward() alone for
reference. fp16, 9 layers, seeded weights, synthetic_pair(..., overlap=n // 2) inputs.

Method: one process; every shape and form warmed up; per repeat the forms alternate, each timed by a
host clock around a window of calls that ends in a device synchronise, the window sized from the
warm-up to last at least --window seconds; the whole comparison repeated --repeats times, so every
figure comes with its spread (min / median / max of the per-call time over the repeats).

    python tools/match_head_ab.py [--pairs 1,16] [--sizes 512,1024,2048] [--repeats 5] [--window 0.3]
                                  [--out profiles/match_head/ab.jsonl]

    python tools/match_head_ab.py --once 1x1024     one warmed-up match_batch call between two
                                                    synchronises (for a kernel trace in a run of its own:
                                                    rocprofv3 --kernel-trace --stats ... -- python ...)
    python tools/match_head_ab.py --timeline <dir>/..._kernel_trace.csv
                                                    that trace's last call, kernel by kernel
                                                    (profiles/match_head/timeline_1x1024.txt)
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


def _batch(P, n, dev, dt):
    ps = [mt.synthetic_pair(300 + i, n, n, overlap=n // 2) for i in range(P)]
    return tuple(torch.cat([p[j] for p in ps], 0).to(dev, dt) for j in range(4))


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def timeline(path):
    """The last match_batch call of a rocprofv3 kernel trace of --once (kernel_trace.csv), cut after
    the previous call's last kernel (assign_finish_kernel, once per call): every kernel in order."""
    import csv

    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    marks = [i for i, r in enumerate(rows) if "assign_finish_kernel" in r["Kernel_Name"]]
    if len(marks) < 2:
        sys.exit("no two match_batch calls in this trace")
    last = rows[marks[-2] + 1:marks[-1] + 1]
    t0 = int(last[0]["Start_Timestamp"])
    ours = ("mha_hd64", "linear", "ffn_rows", "assign_", "pair_inputs")
    other = [r["Kernel_Name"] for r in last if not any(k in r["Kernel_Name"] for k in ours)]
    busy = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in last) / 1e3
    print(f"one match_batch call: {len(last)} kernels, {(int(last[-1]['End_Timestamp']) - t0) / 1e3:.1f} us from the first "
          f"kernel's start to the last one's end, {busy:.1f} us in kernels; kernels that are not this library's: "
          f"{len(other)} {other}")
    print("   #  start us   dur us  kernel")
    for i, r in enumerate(last):
        s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        name = r["Kernel_Name"].removeprefix("void ").replace("(anonymous namespace)::", "").split("(")[0]
        print(f"{i + 1:4d} {(s - t0) / 1e3:9.1f} {(e - s) / 1e3:8.1f}  {name[:110]}")


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--timeline":
        return timeline(sys.argv[2])
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", default="1,16")
    ap.add_argument("--sizes", default="512,1024,2048")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "match_head", "ab.jsonl"))
    ap.add_argument("--once", default=None, metavar="PxN")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("match_head_ab.py: needs a GPU (timings from anywhere else mean nothing)")
    dev, dt = torch.device("cuda:0"), torch.float16
    model = mt.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(mt.seeded_state_dict(7, 9), strict=True)
    model = model.to(dev, dt)
    forms = {"match": model.match, "match_batch": model.match_batch, "forward": model.forward}
    with torch.no_grad():
        if args.once:
            P, n = (int(x) for x in args.once.split("x"))
            batch = _batch(P, n, dev, dt)
            for _ in range(3):
                model.match_batch(*batch)
            torch.cuda.synchronize()
            res = model.match_batch(*batch)   # the traced call: the last 38 + 3 kernels of the run
            torch.cuda.synchronize()
            print(json.dumps({"P": P, "n": n, "counts": res.counts.tolist()}))
            return
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as out:
            for P in (int(x) for x in args.pairs.split(",")):
                for n in (int(x) for x in args.sizes.split(",")):
                    batch = _batch(P, n, dev, dt)
                    calls = {}
                    for name, fn in forms.items():   # warm-up, and the window's length from it
                        call = lambda fn=fn: fn(*batch)  # noqa: E731
                        _window(call, 3)
                        calls[name] = max(5, int(args.window / _window(call, 5)) + 1)
                    # the two forms give the same matches (match_batch's own tests check every field)
                    old, new = model.match(*batch), model.match_batch(*batch)
                    old = [old] if P == 1 else old
                    same = all(torch.equal(new.matches[p, :int(new.counts[p])].long(), old[p][0]) for p in range(P))
                    ms = {name: [] for name in forms}
                    for _ in range(args.repeats):
                        for name, fn in forms.items():
                            ms[name].append(1e3 * _window(lambda fn=fn: fn(*batch), calls[name]))
                    rec = {"P": P, "n": n, "dtype": "float16", "repeats": args.repeats, "calls_per_window": calls,
                           "matches_equal": same, "matches": int(new.counts.sum())}
                    for name, t in ms.items():
                        rec[name + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4),
                                             "max": round(max(t), 4)}
                    # faster by more than the spread: the slowest match_batch window under the fastest match window
                    rec["match_batch_faster_beyond_spread"] = max(ms["match_batch"]) < min(ms["match"])
                    rec["speedup_median"] = round(statistics.median(ms["match"]) / statistics.median(ms["match_batch"]), 3)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    out.write(line + "\n")
                    out.flush()


if __name__ == "__main__":
    main()
