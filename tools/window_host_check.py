"""The sequence window's point statements on the CPU, before any GPU run: csrc/lightglue_window_math.h is __host__
__device__, tools/window_host.cpp wraps lg_window_points for one window serially (the 8 lanes of a track as arrays, their
sums in the butterfly's order), and this script compares it with the float64 contract in lightglue_amd/geometry_contract.py
(window_points_reference) on the scenes of tests/window_scenes.py and on the dirty batch: the decisions must be equal, and
it prints the worst point difference next to the bound of tests/test_gpu_window.py, and the table kWindowGnRounds is chosen
from on those scenes. The figures are in profiles/geometry/INDEX.md. No GPU.

    python tools/window_host_check.py

The same source as a stand-alone program under the sanitizers (nothing loaded into Python runs under one):

    c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -DWINDOW_HOST_MAIN \\
        -Ilightglue-with-flashattentionv2-tensorrt_amd/csrc tools/window_host.cpp -o window_host_san && ./window_host_san
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

import window_scenes as ws  # noqa: E402
from lightglue_amd import window_points_reference, window_tracks_reference  # noqa: E402


def build(tmp):
    so = os.path.join(tmp, "libwindow_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "window_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.host_window_points.argtypes = ([ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5 + [ctypes.c_int] * 3 + [ctypes.c_float] +
                                       [ctypes.c_void_p] * 5)
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host(lib, tk, kept, kpts, intr, r, t, posed):
    tk = np.ascontiguousarray(tk, dtype=np.int32)
    kpts, intr, r, t, posed = (np.ascontiguousarray(x.numpy()) for x in (kpts, intr, r, t, posed))
    views, lmax = tk.shape
    obs, seen = np.zeros((views, lmax, 2), np.float32), np.zeros((views, lmax), np.uint8)
    pts, ok, seen_all = np.zeros((lmax, 3), np.float32), np.zeros(lmax, np.uint8), np.zeros((views, lmax), np.uint8)
    lib.host_window_points(ptr(tk), int(kept), ptr(kpts), ptr(intr), ptr(r), ptr(t), ptr(posed), views, lmax, kpts.shape[1], ws.THRESHOLD,
                           ptr(obs), ptr(seen), ptr(pts), ptr(ok), ptr(seen_all))
    return obs, seen, pts, ok, seen_all


def same_decisions(got, ref):
    return all(np.array_equal(a, b) for a, b in ((got[0], ref[0]), (got[1], ref[1]), (got[3], ref[4]), (got[4], ref[5])))


def main():
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        print("(V, k): host against the contract (bound), against scipy's minimiser (bound); the contract against scipy per rounds 0..4")
        for (views, k), (lmax, _) in ws.POINT_CASES.items():
            s, ref = ws.scene(views, k), ws.points(views, k)
            tk, kept, _ = ws.tracks(views, k, lmax)
            args = (s.kpts, *ws.cameras(s), ws.posed_of(views, k))
            got = host(lib, tk, kept, *args)
            diff = float(np.abs(got[2].astype(np.float64) - ref[3]).max())
            bound = 2.0 ** -23 * float(np.abs(ref[3]).max()) + 4.0 * ws.ORDER
            conv = ws.converged(views, k)
            far = max(float(np.abs(got[2][l] - x).max()) for l, x in conv.items())
            sweep = []
            for rounds in range(5):
                alt = window_points_reference(tk, kept, *args, ws.THRESHOLD, rounds=rounds)
                sweep.append(max(float(np.abs(alt[3][l] - x).max()) for l, x in conv.items() if alt[4][l] and (alt[1][:, l] == ref[1][:, l]).all()))
            good = same_decisions(got, ref) and diff <= bound and far <= 4.0 * ws.CONVERGED
            bad += 0 if good else 1
            print(f"({views}, {k}): decisions {'equal' if same_decisions(got, ref) else 'DIFFER'}, points {diff:.3e} ({bound:.3e}), converged {far:.3e} "
                  f"({4.0 * ws.CONVERGED:.3e}); rounds " + " ".join(f"{x:.3e}" for x in sweep))
        for i, w in enumerate(ws.dirty_windows()):
            tk, kept, _ = window_tracks_reference(w[0], w[1], w[2], w[3], 64)
            ref = window_points_reference(tk, kept, *w[4:], ws.THRESHOLD)
            good = same_decisions(host(lib, tk, kept, *w[4:]), ref)
            bad += 0 if good else 1
            print(f"dirty window {i}: kept {kept}, ok {int(ref[4].sum())}, decisions {'equal' if good else 'DIFFER'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
