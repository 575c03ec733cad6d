"""A/B on one GPU: ImageInput.prepare (one gfx950 launch: uint8 sources of any size, channels and strides to the
encoder's grey [B, Ht, Wt] fp16 input) against image_reference(compute=torch.float32) on the same device (the same
contract in framework ops: three conversions, the grey sum, two matrix products with cached weight matrices and a
division; a Python loop over the images when their sizes differ).

Cases (target 480 x 640, the reference demo's size): 480 x 640 grey -> itself; 1080 x 1920 RGB, linear and area;
3000 x 4000 RGB, area; each at B = 1, 2, 16 equal-sized frames (one [B, H, W, C] tensor: lg_img_prepare_batch, and
the same frames through a prebuilt table: lg_img_prepare), plus one ragged batch of six mixed sources (table).
Bytes: every source byte once plus the output (what a resize that looks at every pixel must move; `linear` at a
ratio above 2 touches fewer source bytes than that, `area` all of them), over the median time.

Method (tools/frontend_ab.py's): one process; every form warmed up; per repeat the forms alternate, each timed by
a host clock around a window of calls that ends in a device synchronise, the window sized from the warm-up to last
at least --window seconds; --repeats repeats, so every figure comes with its spread.

    python tools/image_ab.py [--repeats 5] [--window 0.3] [--out profiles/image/ab.jsonl]
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

from lightglue_amd import ImageInput, image_reference  # noqa: E402

TARGET = (480, 640)
BATCHES = (1, 2, 16)
CASES = (("grey480", (480, 640), 1, "linear"), ("rgb1080", (1080, 1920), 3, "linear"), ("rgb1080", (1080, 1920), 3, "area"),
         ("rgb3000", (3000, 4000), 3, "area"))
RAGGED = ((480, 640, 1), (1080, 1920, 3), (3000, 4000, 3), (720, 1280, 4), (600, 800, 3), (2160, 3840, 3))


def _window(fn, calls):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def _image(seed, shape, dev):
    gen = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8).to(dev)


def _measure(forms, rec, args, nbytes):
    calls = {}
    for name, fn in forms.items():  # warm-up, and the window's length from it
        _window(fn, 3)
        calls[name] = max(3, int(args.window / _window(fn, 3)) + 1)
    ms = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, fn in forms.items():
            ms[name].append(1e3 * _window(fn, calls[name]))
    rec["calls_per_window"] = calls
    rec["bytes"] = nbytes
    for name, t in ms.items():
        med = statistics.median(t)
        rec[name + "_ms"] = {"min": round(min(t), 4), "median": round(med, 4), "max": round(max(t), 4)}
        rec[name + "_GBps"] = round(nbytes / (med * 1e-3) / 1e9, 1)
    rec["reference_over_prepare_median"] = round(statistics.median(ms["reference"]) / statistics.median(ms["prepare"]), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "image", "ab.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("image_ab.py: needs a GPU (timings from anywhere else mean nothing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    base = {"target": list(TARGET), "dtype": "float16", "repeats": args.repeats, "window_s": args.window,
            "device": torch.cuda.get_device_name(0)}
    out_bytes = TARGET[0] * TARGET[1] * 2
    runs = [(name, (h, w), c, interp, b) for name, (h, w), c, interp in CASES for b in BATCHES] + [("ragged", None, None, "area", len(RAGGED))]
    for name, hw, c, interp, b in runs:
        ii = ImageInput(TARGET, interp)
        with torch.no_grad():
            if hw is not None:
                frames = _image(700 + b, (b,) + hw + ((c,) if c > 1 else ()), dev)
                table = ii.table(list(frames))
                forms = {"prepare": lambda: ii.prepare(frames), "prepare_table": lambda: ii.prepare(table),
                         "reference": lambda: image_reference(frames, TARGET, interp, torch.float16, torch.float32)}
                nbytes = frames.numel() + b * out_bytes
                rec = dict(base, case=name, B=b, h=hw[0], w=hw[1], channels=c, interp=interp)
            else:
                imgs = [_image(800 + i, (h, w) + ((ch,) if ch > 1 else ()), dev) for i, (h, w, ch) in enumerate(RAGGED)]
                table = ii.table(imgs)
                forms = {"prepare": lambda: ii.prepare(table),
                         "reference": lambda: image_reference(imgs, TARGET, interp, torch.float16, torch.float32)}
                nbytes = sum(i.numel() for i in imgs) + b * out_bytes
                rec = dict(base, case=name, B=b, sources=[list(s) for s in RAGGED], interp=interp)
            mine, theirs = forms["prepare"]().image, forms["reference"]()
            rec["max_abs_diff"] = float((mine.float() - theirs.float()).abs().max())
            _measure(forms, rec, args, nbytes)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as out:
            out.write(line + "\n")
        del forms, table
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
