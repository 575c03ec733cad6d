"""The bundle adjustment's statements on the CPU, before any GPU run: csrc/lightglue_bundle_math.h is __host__ __device__,
tools/bundle_host.cpp wraps the whole of lg_bundle_adjust for one window serially (the Schur product as plain loops), and
this script compares it with the float64 contract in lightglue_amd/geometry_contract.py (bundle_adjust_reference) on the
scenes of tests/bundle_scenes.py. It prints the table the default `iterations` is chosen from (the distance to the
converged reference per number of rounds), the worsts the bounds of tests/test_gpu_bundle.py are pinned from (four times
each), the full-width window against the truth with the factor its cost falls by, and the dirty batch's num_obs and kept
against the reference. The figures are in profiles/geometry/INDEX.md. No GPU.

    python tools/bundle_host_check.py
"""
import ctypes
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd")
sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402

import bundle_scenes as bs  # noqa: E402
from lightglue_amd import bundle_adjust_reference  # noqa: E402


def build(tmp):
    so = os.path.join(tmp, "libbundle_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "bundle_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.host_bundle.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 3 + [ctypes.c_void_p] * 5
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host(lib, w, iterations):
    obs, seen, count, intr, r, t, pts = (np.ascontiguousarray(x.numpy()) for x in w)
    views, lmax = obs.shape[0], obs.shape[1]
    ro, to, po = np.zeros((views, 3, 3), np.float32), np.zeros((views, 3), np.float32), np.zeros((lmax, 3), np.float32)
    cost, out = np.zeros(2), np.zeros(2, np.int32)
    lib.host_bundle(ptr(obs), ptr(seen), int(count), ptr(intr), ptr(r), ptr(t), ptr(pts), views, lmax, iterations, ptr(ro), ptr(to),
                    ptr(po), ptr(cost), ptr(out))
    return ro, to, po, cost, out


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        print("rounds against bundle_adjust_reference, worst of the scenes " + ", ".join(f"V {v} k {k}" for v, k in bs.CASES) + ":")
        for rounds in (1, 2, 3, 4, 5, 6, 8, 10, 12, 16):
            worst = np.zeros(4)
            for views, k in bs.CASES:
                w, ref = bs.window(bs.scene(views, k)), bs.reference(views, k)
                ro, to, po, cost, out = host(lib, w, rounds)
                live = bs.live_of(w)[0].any(0)
                assert out[0] == int(ref.num_obs) and out[1] == 1 == int(ref.kept), (views, k, out)
                e = bs.errors(ro, to, po, ref.R, ref.t, ref.points, live)
                worst = np.maximum(worst, e + (abs(cost[1] - float(ref.cost[1])) / float(ref.cost[1]),))
            print(f"  {rounds:2d} rounds: R {worst[0]:.3e} deg, t {worst[1]:.3e}, points {worst[2]:.3e}, cost {worst[3]:.3e} relative")
        s = bs.scene(*bs.WIDE, 0.0, bs.MISS)
        w = bs.window(s)
        ro, to, po, cost, out = host(lib, w, bs.ITERATIONS)
        e = bs.errors(ro, to, po, s.R, s.t, s.points, bs.live_of(w)[0].any(0))
        print(f"full width V {bs.WIDE[0]} k {bs.WIDE[1]}, noise 0, {bs.ITERATIONS} rounds against the truth: R {e[0]:.3e} deg, t {e[1]:.3e}, "
              f"points {e[2]:.3e}; cost {cost[0]:.6e} -> {cost[1]:.3e} px² (factor {cost[1] / cost[0]:.3e}), num_obs {out[0]}")
        wins, _ = bs.dirty_windows()
        for i, w in enumerate(wins):
            ref = bundle_adjust_reference(*w)
            ro, to, po, cost, out = host(lib, w, bs.ITERATIONS)
            line = f"dirty window {i}: num_obs {out[0]} (reference {int(ref.num_obs)}), kept {out[1]} (reference {int(ref.kept)})"
            if out[1]:
                e = bs.errors(ro, to, po, ref.R, ref.t, ref.points, bs.live_of(w)[0].any(0))
                line += f", R {e[0]:.3e} deg, t {e[1]:.3e}, points {e[2]:.3e}"
            print(line)


if __name__ == "__main__":
    main()
