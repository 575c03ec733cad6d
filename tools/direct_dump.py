"""Bitwise comparison of two builds' single-pass kernels (a schedule change must not move a bit).

    python tools/direct_dump.py dump <lib.so> <out.npz>   # on the GPU, one build per process
    python tools/direct_dump.py compare <a.npz> <b.npz>   # on the CPU; exit status 1 on a difference

`dump` runs every shape of DIRECT_SHAPES (tests/test_gpu_parity.py) on forced plans 21 (32-row
kernel) and 22 (16-row kernel) with fp16 and fp32 output, one grouped launch of two calls per
output type, and stores the raw output bytes.
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd"), os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402


def dump(lib_path, out_path):
    import torch

    from lightglue_amd import _lib, synth
    from test_gpu_parity import DIRECT_SHAPES

    _lib.LIB_PATH = os.path.abspath(lib_path)
    lib = _lib.load()
    from lightglue_amd import mha_hd64_grouped

    dev = torch.device("cuda:0")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    out = {}
    for nq, nkv in DIRECT_SHAPES:
        qn, kn, vn = synth.qkv(77 + nq + 3 * nkv, nq, nkv)
        q, k, v = (torch.from_numpy(synth.round_f16(x)).to(dev).half().contiguous() for x in (qn, kn, vn))
        for of, dt in ((0, torch.float16), (1, torch.float32)):
            for code in (21, 22):
                o = torch.full(q.shape, float("nan"), dtype=dt, device=dev)
                st = lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1, 4, nq, nkv,
                                                0, of, code, 0, 0, ws.data_ptr(), ws.numel(), s, 3)
                assert st == 0, _lib.last_error()
                torch.cuda.synchronize()
                out[f"p{code}_{nq}x{nkv}_{'f32' if of else 'f16'}"] = o.cpu().numpy().view(np.uint8)
    calls = []
    # the planner's grouped single-pass launch (240 16-row blocks: the 16-row kernel's table form)
    for i, (nq, nkv) in enumerate(((512, 1024), (448, 1000))):
        qn, kn, vn = synth.qkv(41 + i, nq, nkv)
        calls.append(tuple(torch.from_numpy(synth.round_f16(x)).to(dev).half().contiguous() for x in (qn, kn, vn)))
    for dt in (torch.float16, torch.float32):
        outs = mha_hd64_grouped(calls, out_dtype=dt)
        torch.cuda.synchronize()
        for i, o in enumerate(outs):
            out[f"grouped{i}_{'f32' if dt == torch.float32 else 'f16'}"] = o.cpu().numpy().view(np.uint8)
    np.savez(out_path, **out)
    print(f"{len(out)} outputs -> {out_path}")


def compare(a_path, b_path):
    with np.load(a_path) as a, np.load(b_path) as b:
        assert sorted(a.files) == sorted(b.files), "different sets of outputs"
        bad = [n for n in a.files if a[n].shape != b[n].shape or not np.array_equal(a[n], b[n])]
        print(f"{len(a.files)} outputs compared; {len(bad)} differ" + (": " + ", ".join(bad) if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
