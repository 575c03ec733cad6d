"""A/B on one GPU: SuperPointEncoder.heads (gfx950 kernels: lg_sp_conv1, lg_sp_conv3x3, lg_sp_heads; ten launches)
against superpoint_reference on the same device in fp16 (the framework's convolutions: MIOpen), the reference in
both layouts (NCHW, and weights and activations in channels_last), and each side followed by extract +
match_features (images to matches; B / 2 pairs, so not at B = 1). 480 x 640 images (the reference's size), B = 1,
2, 16 images per encoder pass, uniform [0, 1) pixels, seeded_superpoint_state_dict(3), K = 1024, 9 matcher layers
(seeded_state_dict(7)). Seeded weights, not trained ones: the times do not depend on the values, and what the
matcher finds says nothing about real image pairs.

Every line also times each of our ten launches on its own, at that layer's size, against its algorithmic FLOPs
and bytes (input + output + weights, each once).

Method (tools/frontend_ab.py's): one process; every form warmed up (MIOpen's find step runs in the warm-up, outside
every timed window); per repeat the forms alternate, each timed by a host clock around a window of calls that ends
in a device synchronise, the window sized from the warm-up to last at least --window seconds. If the framework
cannot run a form here, the line records the error instead of a time.

    python tools/superpoint_ab.py [--repeats 5] [--window 0.3] [--out profiles/superpoint/ab.jsonl]

Per-kernel statistics come from a run of their own under the profiler, 50 encoder passes at batch B:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o run -- python tools/superpoint_ab.py --profile B

(profiles/superpoint/kernel_stats_b*.csv).
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

from lightglue_amd import (  # noqa: E402
    Features, KeypointFrontend, SuperPointEncoder, match_images, seeded_superpoint_state_dict, superpoint_reference, synth)
from lightglue_amd import matcher as mt  # noqa: E402
from lightglue_amd import superpoint as sp  # noqa: E402

H, W, K = 480, 640, 1024
BATCHES = (1, 2, 16)
# our launches: (name, cin, cout, divisor of H and W at its input, pooled)
CONVS = (("conv1b", 64, 64, 1, True), ("conv2a", 64, 64, 2, False), ("conv2b", 64, 64, 2, True), ("conv3a", 64, 128, 4, False),
         ("conv3b", 128, 128, 4, True), ("conv4a", 128, 128, 8, False), ("conv4b", 128, 128, 8, False),
         ("convPa|convDa", 128, 512, 8, False))


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def _images(seed, b, dev):
    return torch.from_numpy(synth.uniform24(seed, b * H * W).reshape(b, 1, H, W)).half().to(dev)


def _layer_forms(enc, b, dev):
    """name -> (callable, flop, bytes): each launch on buffers of its own size (values do not matter)."""
    p = enc._weights(dev)
    img = _images(9, b, dev)
    forms = {}
    x1 = torch.empty((b, H, W, 64), dtype=torch.float16, device=dev)
    forms["conv1a"] = (lambda: sp.conv1(img[:, 0], *p["conv1a"], out=x1), 2 * 9 * 64 * H * W * b, b * H * W * (2 + 128))
    for name, cin, cout, div, pool in CONVS:
        h, w = H // div, W // div
        x = torch.randn((b, h, w, cin), device=dev).half()
        oh, ow = (h // 2, w // 2) if pool else (h, w)
        out = torch.empty((b, oh, ow, cout), dtype=torch.float16, device=dev)
        wp, bias = p["convPDa" if "|" in name else name]
        forms[name] = (lambda x=x, wp=wp, bias=bias, pool=pool, out=out: sp.conv3x3(x, wp, bias, True, pool, out=out),
                       2 * 9 * cin * cout * h * w * b, 2 * (x.numel() + out.numel() + wp.numel()))
    xh = torch.randn((b, H // 8, W // 8, 512), device=dev).half()
    wp, bias = p["heads"]
    forms["convPb+convDb"] = (lambda: sp.heads(xh, wp, bias), 2 * 256 * (65 + 256) * (H // 8) * (W // 8) * b,
                              2 * (xh.numel() + b * (H // 8) * (W // 8) * 321 + wp.numel()))
    return forms


def profile(b):
    dev = torch.device("cuda:0")
    enc = SuperPointEncoder(seeded_superpoint_state_dict(3))
    img = _images(700 + b, b, dev)
    for _ in range(50):
        enc.heads(img)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "superpoint", "ab.jsonl"))
    ap.add_argument("--profile", type=int, default=0, metavar="B", help="only run 50 encoder passes at batch B (for rocprofv3)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("superpoint_ab.py: needs a GPU (timings from anywhere else mean nothing)")
    if args.profile:
        return profile(args.profile)
    dev = torch.device("cuda:0")
    sd = seeded_superpoint_state_dict(3)
    enc = SuperPointEncoder(sd)
    sd_nchw = {k: v.to(dev, torch.float16) for k, v in sd.items()}
    sd_cl = {k: (v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v) for k, v in sd_nchw.items()}
    model = mt.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(mt.seeded_state_dict(7, 9), strict=True)
    model = model.to(dev, torch.float16)
    fe = KeypointFrontend(max_keypoints=K)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for b in BATCHES:
        img = _images(700 + b, b, dev)
        img_cl = img.contiguous(memory_format=torch.channels_last)
        pairs = b // 2

        def ref_nchw():
            return superpoint_reference(sd_nchw, img, None, torch.float16)

        def ref_cl():
            return superpoint_reference(sd_cl, img_cl, None, torch.float16)

        def match_after(heads_fn):
            f = fe.extract(*heads_fn())
            return model.match_features(Features(*(t[:pairs] for t in f)), Features(*(t[pairs:] for t in f)))

        forms = {"heads": lambda: enc.heads(img), "reference_nchw": ref_nchw, "reference_channels_last": ref_cl}
        if pairs:
            forms["images_to_matches"] = lambda: match_images(enc, fe, model, img[:pairs], img[pairs:])
            forms["reference_nchw_to_matches"] = lambda: match_after(ref_nchw)
            forms["reference_channels_last_to_matches"] = lambda: match_after(ref_cl)
        rec = {"B": b, "h": H, "w": W, "K": K, "dtype": "float16", "repeats": args.repeats, "window_s": args.window,
               "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
        with torch.no_grad():
            errors, calls = {}, {}
            for name, fn in list(forms.items()):  # warm-up (MIOpen's find step), and the window's length from it
                try:
                    _window(fn, 3)
                    calls[name] = max(3, int(args.window / _window(fn, 3)) + 1)
                except Exception as e:  # the framework cannot run this form here: recorded, not worked around
                    errors[name] = f"{type(e).__name__}: {e}"[:300]
                    del forms[name]
            rec["not_run"] = errors
            if "reference_channels_last" in forms:
                lg, dn = ref_cl()
                rec["channels_last_outputs"] = [bool(t.is_contiguous(memory_format=torch.channels_last)) for t in (lg, dn)]
            if "reference_nchw" in forms:
                ours, theirs = enc.heads(img), ref_nchw()
                rec["max_abs_diff_to_reference_nchw"] = [float((a.float() - r.float()).abs().max()) for a, r in zip(ours, theirs)]
            ms = {name: [] for name in forms}
            for _ in range(args.repeats):
                for name, fn in forms.items():
                    ms[name].append(1e3 * _window(fn, calls[name]))
            layers = {}
            for name, (fn, flop, nbytes) in _layer_forms(enc, b, dev).items():
                _window(fn, 3)
                n = max(3, int(0.05 / _window(fn, 3)) + 1)
                t = statistics.median(_window(fn, n) for _ in range(3))
                layers[name] = {"us": round(1e6 * t, 2), "gflop": round(flop / 1e9, 3), "tflops": round(flop / t / 1e12, 1),
                                "mbytes": round(nbytes / 1e6, 2), "gbytes_per_s": round(nbytes / t / 1e9, 1)}
        rec["calls_per_window"] = calls
        for name, t in ms.items():
            rec[name + "_ms"] = {"min": round(min(t), 4), "median": round(statistics.median(t), 4), "max": round(max(t), 4)}
        med = {name: statistics.median(t) for name, t in ms.items()}
        for other in ("reference_nchw", "reference_channels_last"):
            if other in med:
                rec[other + "_over_heads_median"] = round(med[other] / med["heads"], 2)
            if other + "_to_matches" in med:
                rec[other + "_to_matches_over_ours_median"] = round(med[other + "_to_matches"] / med["images_to_matches"], 2)
        rec["layers"] = layers
        rec["layers_sum_us"] = round(sum(v["us"] for v in layers.values()), 1)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as out:
            out.write(line + "\n")


if __name__ == "__main__":
    main()
