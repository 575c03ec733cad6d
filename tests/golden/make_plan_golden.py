"""Record tests/golden/plan_routes.json: how the attention launcher routes and plans a table of launches
(mha_hd64_plan_route), taken from a build of the commit named in the fixture's header. The table pins the
planner, the fp32 routes and the workspace each uses, so that a change to the host side of the attention
operator that is meant to keep them shows any drift (tests/test_abi.py replays it; no GPU).

    MHA_HD64_LIB=path/to/libmha_hd64.so python tests/golden/make_plan_golden.py "<recorded from ...>"

The library must export mha_hd64_plan_route; a commit older than the hook gets it patched into its
mha_hd64_plugin.cpp for the recording (the hook only reads the planner). Environment switches
(MHA_HD64_*) unset.
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HALF, FLOAT = 1, 0
UNLIMITED = -1  # ws_bytes = (size_t)-1
FIELDS = ("route", "plan_code", "kv_waves", "rows_per_wave", "direct_tiles", "splits", "tiles_per_split",
          "ws_offset", "ws_needed")
A = 4096  # a fake 16-B aligned address for the workspace query's argument checks: never dereferenced

BATCHES = (1, 2, 3, 4, 6, 8, 16, 64)
LENGTHS = (1, 16, 17, 64, 100, 512, 513, 1024, 1025, 1536, 2048)
GROUPS = (
    [(1, 4, 1024, 1024)] * 2,                                                      # a LightGlue pair: self
    [(1, 4, 1000, 777), (1, 4, 777, 1000)],                                        # ... and cross
    [(2, 4, 2048, 2048), (1, 4, 1536, 1536)],
    [(1, 4, 512, 2048), (1, 4, 2048, 512)],
    [(4, 4, 1024, 1024)] * 2,
    [(1, 4, 100, 1100), (1, 4, 16, 1100)],
    [(1, 4, 1024, 1024)] * 4,
    [(1, 4, 512, 512), (1, 4, 100, 2048), (2, 4, 17, 1025), (1, 4, 1536, 64)],
    [(8, 4, 1024, 1024)] * 4,
    [(1, 4, 64, 64), (1, 4, 1, 1), (1, 4, 16, 17), (1, 4, 513, 100)],
    [(1, 4, 1024, 1024)] * 5,                                                      # 5: a second chunk
    [(1, 4, 2048, 2048), (1, 4, 1000, 777), (1, 4, 777, 1000), (2, 4, 512, 1536), (1, 4, 1025, 513)],
    [(16, 4, 1024, 1024)] * 4 + [(1, 4, 100, 100)],
)
SWITCHES = [(h, s, k) for h in (1, 2) for s in (1, 0) for k in (1, 0, 2)]  # (hint, stream mode, f32 in-kernel)
FORCED = ([(q, k, s) for (q, k) in ((4, 1), (2, 2), (1, 8), (2, 4)) for s in (0, 3)] +
          [(12, 2, 0), (21, 0, 0), (22, 0, 0), (23, 0, 0), (23, 4, 0), (23, 8, 0)])


def singles():
    """One in 13 of BATCHES x LENGTHS x LENGTHS (heads = 4), spread over every value of every axis."""
    return [[(b, 4, nq, nkv)] for ib, b in enumerate(BATCHES) for iq, nq in enumerate(LENGTHS)
            for ik, nkv in enumerate(LENGTHS) if (ib + 2 * iq + 3 * ik) % 13 == 0]


def entries():
    """(calls, in_type, switches, forced) of every table entry, in the fixture's order."""
    one, groups = singles(), [list(g) for g in GROUPS]
    for calls in one + groups:
        for t in (HALF, FLOAT):
            yield calls, t, SWITCHES[0], (0, 0, 0)
    for calls in one[::25] + groups[1::2]:  # the switches (fp16 inputs never look at the fp32 one)
        for sw in SWITCHES[1:]:
            for t in (HALF, FLOAT) if sw[2] == 1 else (FLOAT,):
                yield calls, t, sw, (0, 0, 0)
    for calls in one[7::30] + groups[::4]:
        for f in FORCED:
            for t in (HALF, FLOAT):
                yield calls, t, SWITCHES[0], f


def call_array(calls):
    from lightglue_amd._lib import CallDesc

    return (CallDesc * len(calls))(*[CallDesc(A, A, A, A, *c) for c in calls])


def query(lib, calls, in_type):
    return lib.mha_hd64_grouped_workspace_bytes_typed(call_array(calls), len(calls), in_type)


def route(lib, calls, in_type, ws, has_ws, forced):
    """One [route, plan_code, ..., ws_needed] (FIELDS) per chunk of four calls."""
    out = []
    for i in range(0, len(calls), 4):
        chunk = calls[i:i + 4]
        n = len(chunk)
        head, sp, tp = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * n)(), (ctypes.c_int32 * n)()
        off = (ctypes.c_size_t * n)()
        need = lib.mha_hd64_plan_route(call_array(chunk), n, in_type, ws % (1 << 64), has_ws, *forced, head, sp, tp, off)
        assert need != (1 << 64) - 1, (calls, "bad arguments")
        out.append(list(head) + [list(sp), list(tp), list(off), need])
    return out


def workspaces(need):
    sizes = sorted({0, need, max(0, need - 256), 5 << 20, 1 << 30})
    return [(ws, has) for ws in sizes for has in (1, 0)] + [(UNLIMITED, 1)]


class switches:
    """Set (hint, stream mode, f32 in-kernel) for a block; put back what was there."""

    def __init__(self, lib, sw):
        self.lib, self.sw = lib, sw

    def __enter__(self):
        self.hint = self.lib.mha_hd64_set_concurrency_hint(self.sw[0])
        self.stream = self.lib.mha_hd64_set_stream_mode(self.sw[1])
        self.lib.mha_hd64_set_f32_inkernel(self.sw[2])

    def __exit__(self, *exc):
        self.lib.mha_hd64_set_concurrency_hint(self.hint)
        self.lib.mha_hd64_set_stream_mode(self.stream)
        self.lib.mha_hd64_set_f32_inkernel({"0": 0, "2": 2}.get(os.environ.get("MHA_HD64_F32_INKERNEL", "1")[:1], 1))


def record(lib):
    table = []
    for calls, t, sw, forced in entries():
        with switches(lib, sw):
            need = query(lib, calls, t)
            rows, results = [], []
            for ws, has in workspaces(need):
                r = route(lib, calls, t, ws, has, forced)
                if r not in results:
                    results.append(r)
                rows.append(results.index(r))
            if forced == (0, 0, 0):  # the workspace query is the route at its best
                assert need == max(c[-1] for c in route(lib, calls, t, UNLIMITED, 1, forced)), (calls, t, sw)
        table.append([[list(c) for c in calls], t, list(sw), list(forced), need, rows, results])
    return table


def main():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lightglue-with-flashattentionv2-tensorrt_amd"))
    from lightglue_amd import _lib

    table = record(_lib.load())
    doc = {"header": {"recorded_from": sys.argv[1], "recipe": "tests/golden/make_plan_golden.py", "fields": FIELDS,
                      "entry": "[calls [batch, heads, nq, nkv], in_type, switches (hint, stream mode, f32 in-kernel), "
                               "forced (q_waves, kv_waves, splits), workspace query, index into results for each of "
                               "workspaces(query), results]; a result is one list of fields per chunk of four calls"},
           "entries": table}
    path = os.path.join(HERE, "plan_routes.json")
    with open(path, "w") as f:
        f.write("{\"header\": " + json.dumps(doc["header"]) + ",\n\"entries\": [\n")
        f.write(",\n".join(json.dumps(e, separators=(",", ":")) for e in table))
        f.write("\n]}\n")
    print(path, len(table), "entries,", sum(len(e[5]) for e in table), "rows,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
