"""Diagnostic: phase timestamps of the single-pass kernels from a -DMHA_STAMPS build
(make -C lightglue-with-flashattentionv2-tensorrt_amd variant SRC='mha_hd64_direct mha_hd64_direct16 mha_hd64_plugin'
NAME=stamps DEFS=-DMHA_STAMPS).
    python tools/dstamps.py <lib.so> nq nkv [plan code: 21 (32-row kernel, default) | 22 (16-row)]
Plan 21, 8 slots per workgroup (wave 0, s_memtime cycles): 0 entry, 1 Q + K(0) landed, 2 scores and
probabilities of every tile done, 3 V(0) landed, 4 PV done, 5 after the epilogue barrier,
6 output stores acknowledged. Prints medians / maxima of each segment and of the start spread.
Plan 22, 16 slots per workgroup: 0 entry, 1 Q + K(0) landed, 2 last score done, 3 later tiles'
exponentials done, 4 PV done, 5 barrier, 6 stores acknowledged, 7 rows 0-31 of the last V tile
landed, 8 + t V(t) landed. Prints each event's median / maximum cycles since the workgroup's entry
(in time order), and the tail: PV done, barrier and stores acknowledged since the last V landed."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd")]
import torch  # noqa: E402

from lightglue_amd import _lib, synth  # noqa: E402

_lib.LIB_PATH = os.path.abspath(sys.argv[1])
lib = _lib.load()
nq, nkv = int(sys.argv[2]), int(sys.argv[3])
code = int(sys.argv[4]) if len(sys.argv) > 4 else 21
rows = 16 if code == 22 else 32
slots = 16 if code == 22 else 8
dev = torch.device("cuda:0")
qn, kn, vn = synth.qkv(3, nq, nkv)
q, k, v = (torch.from_numpy(x).to(dev).half().contiguous() for x in (qn, kn, vn))
o = torch.empty_like(q)
ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
st = torch.zeros(1 << 16, dtype=torch.int64, device=dev)
lib.mha_hd64_set_stamp_buffer(st.data_ptr())
s = torch.cuda.current_stream().cuda_stream
res = []
for rep in range(30):  # back-to-back launches (clocks up); keep the last
    lib.mha_hd64_launch_forced(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), 1, 4, nq, nkv, 0, 0, code, 0, 0,
                               ws.data_ptr(), ws.numel(), s, 3)
torch.cuda.synchronize()
nwg = -(-nq // rows) * 4
t = st[: nwg * slots].view(nwg, slots).cpu().numpy().astype("int64")
t0 = t[:, 0].min()
d = {"nq": nq, "nkv": nkv, "plan": code, "wgs": nwg, "start_spread_cyc": int(t[:, 0].max() - t0),
     "span_cyc": int(t[:, 6].max() - t0)}
if code == 22:
    assert nkv <= 1024, "plan 22 stamps: the one-pass forms (the two-pass form stamps V(0) only)"
    tiles = 4 if nkv > 512 else 2  # 64-key tiles per wave of the one-pass forms
    events = [("qk0_landed", 1), ("last_score", 2), ("later_exps", 3)]
    events += [(f"v{i}_landed", 8 + i) for i in range(tiles - 1)]
    events += [("vlast_rows0_31_landed", 7), (f"v{tiles - 1}_landed", 8 + tiles - 1), ("pv_done", 4), ("barrier", 5),
               ("stores_acked", 6)]
    events = [e for e in events if t[:, e[1]].any()]  # (a schedule without that wait leaves its slot 0)
    for name, slot in sorted(events, key=lambda e: statistics.median(t[:, e[1]] - t[:, 0])):
        seg = t[:, slot] - t[:, 0]
        d[name + "_med"] = int(statistics.median(seg))
        d[name + "_max"] = int(seg.max())
    last = t[:, 8 + tiles - 1]
    for name, slot in (("pv_done", 4), ("barrier", 5), ("stores_acked", 6)):
        d[f"tail_{name}_after_last_v_med"] = int(statistics.median(t[:, slot] - last))
    d["end_med_from_t0"] = int(statistics.median(t[:, 6] - t0))
    print(json.dumps(d))
    sys.exit(0)
names = ["qk0_landed", "scores", "v0_landed", "pv", "epi_barrier", "merge_store"]
for i, n in enumerate(names):
    seg = t[:, i + 1] - t[:, i]
    d[n + "_med"] = int(statistics.median(seg))
    d[n + "_max"] = int(seg.max())
d["end_med_from_t0"] = int(statistics.median(t[:, 6] - t0))
if nkv > 1024 and code == 21:  # two-pass form: slot 7 = second pass starts (first pass's PVs done)
    d["pass1_start_med_from_t0"] = int(statistics.median(t[:, 7] - t0))
    d["pass1_med"] = int(statistics.median(t[:, 4] - t[:, 7]))
    d["v0_to_pass1_med"] = int(statistics.median(t[:, 7] - t[:, 3]))
print(json.dumps(d))
