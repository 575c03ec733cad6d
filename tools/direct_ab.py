"""Per-launch graph-replay times of the single-pass kernels' forms for one build, one JSON line;
run it once per build and alternate the builds (A/B/A/B) from the calling script.

    python tools/direct_ab.py <lib.so> [label]
Single 1x4xNxN calls on forced plan 22 (16-row kernel: N = 1024 and 768 the 4-tile form, 512 and
320 the 2-tile form) and plan 21 (32-row kernel), fp16 output; plan 22 at 1024 with fp32 output;
and the planner's grouped launch of two 512x1024 calls (256 blocks of the 16-row kernel's table form).
"""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"), os.path.join(REPO, "tools")]
import torch  # noqa: E402

from lightglue_amd import _lib, synth  # noqa: E402

_lib.LIB_PATH = os.path.abspath(sys.argv[1])
from direct_check import forced, per_launch_us  # noqa: E402


def main():
    lib = _lib.load()
    from lightglue_amd import mha_hd64_grouped

    dev = torch.device("cuda:0")
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
    res = {"lib": sys.argv[2] if len(sys.argv) > 2 else os.path.basename(sys.argv[1])}
    for n in (1024, 768, 512, 320):
        qn, kn, vn = synth.qkv(5, n, n)
        q, k, v = (torch.from_numpy(x).to(dev).half().contiguous() for x in (qn, kn, vn))
        o = torch.empty_like(q)
        for code in (22, 21):
            res[f"p{code}_{n}"] = round(per_launch_us(lambda: forced(lib, q, k, v, o, n, n, code, 0, 0, ws)), 3)
        if n == 1024:
            o32 = torch.empty(q.shape, dtype=torch.float32, device=dev)
            res["p22_1024_f32out"] = round(per_launch_us(lambda: forced(lib, q, k, v, o32, n, n, 22, 0, 0, ws)), 3)
            q2 = q[:, :, :512].contiguous()
            calls = [(q2, k, v), (q2.clone(), k.clone(), v.clone())]
            outs = [torch.empty_like(q2), torch.empty_like(q2)]
            res["grouped_2x512x1024"] = round(per_launch_us(lambda: mha_hd64_grouped(calls, outs=outs)), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
