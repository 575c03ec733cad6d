"""A/B on one GPU: KeypointFrontend.extract (gfx950 kernels: heatmap, NMS, select, describe; no host
synchronisation) against frontend_reference on the same device (the reference's post-processing in framework
ops: softmax + depth-to-space, five 9 x 9 max-pools, nonzero per image, sort, grid_sample, two normalisations),
and extract x 2 + match_features against frontend_reference x 2 + match_batch with the counts it returns.
480 x 640 images (the reference's size: 60 x 80 cells), B = 1, 2, 16 images per side, K = 1024, fp16 outputs,
9 layers, seeded weights (seeded_state_dict(7)).

The inputs are seeded random logits and descriptors, not a trained SuperPoint's: every image has far more
than K candidates (reported per case), so select's radix path runs and every slot is filled; what the
matcher then finds says nothing about real image pairs. Each line also reports whether the two front ends
chose the same pixels per image (they may differ where the kernel's and the framework's softmax round a
score differently across the threshold, the K cut or a local maximum).

Method (tools/adaptive_ab.py's): one process; every form warmed up; per repeat the forms alternate, each
timed by a host clock around a window of calls that ends in a device synchronise, the window sized from the
warm-up to last at least --window seconds; --repeats repeats, so every figure comes with its spread.

    python tools/frontend_ab.py [--repeats 5] [--window 0.5] [--out profiles/frontend/ab.jsonl]
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

from lightglue_amd import KeypointFrontend, frontend_reference  # noqa: E402
from lightglue_amd import matcher as mt  # noqa: E402

HC, WC, K = 60, 80, 1024
BATCHES = (1, 2, 16)


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def _inputs(seed, b, dev):
    gen = torch.Generator().manual_seed(seed)
    logits = torch.randn((b, 65, HC, WC), generator=gen)
    dense = torch.randn((b, 256, HC, WC), generator=gen).half()
    return logits.to(dev), dense.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frontend", "ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frontend_ab.py: needs a GPU (timings from anywhere else mean nothing)")
    dev = torch.device("cuda:0")
    model = mt.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(mt.seeded_state_dict(7, 9), strict=True)
    model = model.to(dev, torch.float16)
    fe = KeypointFrontend(max_keypoints=K)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for b in BATCHES:
        (l0, d0), (l1, d1) = _inputs(500 + b, b, dev), _inputs(600 + b, b, dev)

        def ref(lg, dn):
            return frontend_reference(lg, dn, max_keypoints=K)

        def match_ref():
            f0, f1 = ref(l0, d0), ref(l1, d1)
            return model.match_batch(f0.kpts, f1.kpts, f0.desc, f1.desc, counts0=f0.counts, counts1=f1.counts)

        forms = {"extract": lambda: fe.extract(l0, d0), "reference": lambda: ref(l0, d0),
                 "extract_match": lambda: model.match_features(fe.extract(l0, d0), fe.extract(l1, d1)),
                 "reference_match": match_ref}
        rec = {"B": b, "h": HC * 8, "w": WC * 8, "K": K, "dtype": "float16", "repeats": args.repeats,
               "window_s": args.window, "device": torch.cuda.get_device_name(0)}
        with torch.no_grad():
            mine, theirs = fe.extract(l0, d0), ref(l0, d0)
            from lightglue_amd import frontend as fr
            rec["candidates"] = fr.select_reference(fr.nms_reference(fr.heatmap_reference(l0)), 2048, fe.threshold,
                                                    fe.remove_borders)[0].tolist()  # (capped at 2048)
            w = WC * 8
            pm, pt = (f.kpts_px[..., 1] * w + f.kpts_px[..., 0] for f in (mine, theirs))
            rec["counts"] = mine.counts.tolist()
            rec["same_counts"] = bool(torch.equal(mine.counts, theirs.counts))
            rec["images_with_the_same_pixels"] = sum(set(pm[i].tolist()) == set(pt[i].tolist()) for i in range(b))
            rec["desc_max_abs_diff"] = float((mine.desc.float() - theirs.desc.float()).abs().max()) \
                if bool(torch.equal(pm, pt)) else None
            rec["matches_extract"] = forms["extract_match"]().counts.tolist()
            rec["matches_reference"] = match_ref().counts.tolist()
            calls = {}
            for name, fn in forms.items():  # warm-up, and the window's length from it
                _window(fn, 3)
                calls[name] = max(3, int(args.window / _window(fn, 3)) + 1)
            ms = {name: [] for name in forms}
            for _ in range(args.repeats):
                for name, fn in forms.items():
                    ms[name].append(1e3 * _window(fn, calls[name]))
        rec["calls_per_window"] = calls
        for name, t in ms.items():
            rec[name + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4), "max": round(max(t), 4)}
        med = {name: statistics.median(t) for name, t in ms.items()}
        rec["reference_over_extract_median"] = round(med["reference"] / med["extract"], 2)
        rec["reference_match_over_extract_match_median"] = round(med["reference_match"] / med["extract_match"], 2)
        rec["extract_ms_per_image"] = round(med["extract"] / b, 4)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as out:
            out.write(line + "\n")


if __name__ == "__main__":
    main()
