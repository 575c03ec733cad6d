"""The pose polish's and the triangulation's statements on the CPU, before any GPU run: csrc/lightglue_polish_math.h
is __host__ __device__, tools/polish_host.cpp wraps pose_polish_kernel for one pair with the workgroup's rows run
serially (and tools/essential_host.cpp the RANSAC before it), and this script compares them with the float64 contract
in lightglue_amd/geometry_contract.py (polish_reference: scipy's least squares run to convergence in another
parameterisation) on every pair tests/test_gpu_pose_polish.py runs: the six scenes of tests/polish_scenes.py through
RANSAC and POLISH rounds, the hook on essential_scenes.ragged(), the full width, the keep rule's pair and the planar
pairs. Masks, counts and kept must equal the reference's; it prints the worsts the GPU bounds are pinned from (four
times each): R and t in degrees, E per point in pixels on the same mask, triangulated points relative to their depth,
and the length of the last accepted step per pair. The figures are in profiles/geometry/INDEX.md. No GPU.

    python tools/polish_host_check.py [--scene K]      (--scene: only the k = K scene of the six)
"""
import argparse
import ctypes
import os
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd")
sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import essential_scenes as es  # noqa: E402
import polish_scenes as ps  # noqa: E402
from lightglue_amd import PolishResult, PoseResult, epipolar_error, essential_to_fundamental, triangulate_reference  # noqa: E402
from lightglue_amd.geometry import gather_correspondences  # noqa: E402

# the tool's own bounds (what --scene asserts): far above the fp32 rounding of the outputs, far below a wrong step
TOOL_BOUND_DEG, TOOL_BOUND_PX, TOOL_BOUND_REL = 1e-4, 1e-3, 1e-5


def build(tmp):
    so = os.path.join(tmp, "libpolish_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "polish_host.cpp"),
                    os.path.join(REPO, "tools", "essential_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_rows(m, count, kp0, kp1):
    x0, x1 = gather_correspondences(m, count, kp0, kp1)
    return x0, x1, np.ascontiguousarray(np.concatenate([x0, x1], 1).astype(np.float32).reshape(-1, 4))


def host_polish(lib, batch, pose, iterations=ps.POLISH):
    """lg_pose_polish's statements on every pair of a batch -> (PolishResult (fp32, as the kernel's), the last accepted
    step of each pair)."""
    m, counts, kp0, kp1, intr = batch
    pr, kmax = m.shape[0], m.shape[1]
    out = PolishResult(torch.zeros((pr, 3, 3)), torch.zeros((pr, 3, 3)), torch.zeros((pr, 3)), torch.zeros((pr, kmax), dtype=torch.uint8),
                       torch.zeros(pr, dtype=torch.int32), torch.zeros(pr, dtype=torch.int32), torch.zeros((pr, 2)),
                       torch.zeros(pr, dtype=torch.int32))
    last = []
    for p in range(pr):
        _, _, pts = host_rows(m[p], int(counts[p]), kp0[p], kp1[p])
        n = len(pts)
        kk = np.ascontiguousarray(intr[p].numpy().astype(np.float32).reshape(8))
        r = np.ascontiguousarray(pose.R[p].numpy().astype(np.float32).reshape(9))
        t = np.ascontiguousarray(pose.t[p].numpy().astype(np.float32).reshape(3))
        inl = np.ascontiguousarray(pose.inliers[p, :max(n, 1)].numpy().astype(np.uint8))
        e, ro, to = np.zeros(9, dtype=np.float32), np.zeros(9, dtype=np.float32), np.zeros(3, dtype=np.float32)
        io, o3, cost = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(3, dtype=np.int32), np.zeros(2, dtype=np.float32)
        steps = np.zeros(iterations, dtype=np.float64)
        lib.host_polish(ptr(pts), n, ptr(kk), ptr(r), ptr(t), ptr(inl), int(pose.valid[p]), ctypes.c_float(ps.THRESHOLD), iterations,
                        ptr(e), ptr(ro), ptr(to), ptr(io), ptr(o3), ptr(cost), ptr(steps))
        out.E[p], out.R[p], out.t[p] = torch.from_numpy(e).reshape(3, 3), torch.from_numpy(ro).reshape(3, 3), torch.from_numpy(to)
        out.inliers[p, :n] = torch.from_numpy(io[:n])
        out.num_inliers[p], out.num_front[p], out.kept[p] = int(o3[0]), int(o3[1]), int(o3[2])
        out.cost[p] = torch.from_numpy(cost)
        taken = steps[steps >= 0]
        last.append(float(taken[-1]) if len(taken) else 0.0)
    return out, last


def host_ransac(lib, batch):
    """lg_ransac_essential's statements on every pair of a batch (tools/essential_host.cpp) -> PoseResult (fp32)."""
    m, counts, kp0, kp1, intr = batch
    pr, kmax = m.shape[0], m.shape[1]
    out = PoseResult(torch.zeros((pr, 3, 3)), torch.zeros((pr, 3, 3)), torch.zeros((pr, 3)), torch.zeros((pr, kmax), dtype=torch.uint8),
                     torch.zeros(pr, dtype=torch.int32), torch.zeros(pr, dtype=torch.int32), torch.zeros(pr, dtype=torch.int32),
                     torch.zeros(pr, dtype=torch.int32))
    for p in range(pr):
        _, _, pts = host_rows(m[p], int(counts[p]), kp0[p], kp1[p])
        n = len(pts)
        kk = np.ascontiguousarray(intr[p].numpy().astype(np.float32).reshape(8))
        e, r, t = np.zeros(9, dtype=np.float32), np.zeros(9, dtype=np.float32), np.zeros(3, dtype=np.float32)
        inl, o4 = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(4, dtype=np.int32)
        lib.host_essential(ptr(pts), n, ptr(kk), ctypes.c_float(ps.THRESHOLD), ps.HYPOTHESES, ps.REFITS, ps.SEED, ptr(e), ptr(r), ptr(t),
                           ptr(inl), ptr(o4))
        out.E[p], out.R[p], out.t[p] = torch.from_numpy(e).reshape(3, 3), torch.from_numpy(r).reshape(3, 3), torch.from_numpy(t)
        out.inliers[p, :n] = torch.from_numpy(inl[:n])
        out.num_inliers[p], out.num_front[p], out.valid[p], out.best[p] = (int(v) for v in o4)
    return out


class Worst:
    def __init__(self):
        self.rot = self.tra = self.px = self.rel = self.step = 0.0
        self.pairs = self.bad = 0


def compare(name, batch, got, want, w, skip=(), pose=True, last=None):
    """Pair by pair: mask, counts and kept exactly; where kept, E per point in pixels and R, t in degrees; where passed
    through, R and t bitwise the given ones (which `want` holds too)."""
    m, counts, kp0, kp1, intr = batch
    for p in range(m.shape[0]):
        if p in skip:
            continue
        w.pairs += 1
        n = min(max(int(counts[p]), 0), m.shape[1])
        a = [int(got.num_inliers[p]), int(got.num_front[p]), int(got.kept[p])]
        b = [int(want.num_inliers[p]), int(want.num_front[p]), int(want.kept[p])]
        if a != b or not torch.equal(got.inliers[p], want.inliers[p]):
            w.bad += 1
            print(f"  {name}, pair {p}: (num, front, kept) {a} against {b}")
            continue
        if not b[2]:
            assert torch.equal(got.R[p].double(), want.R[p].double()) and torch.equal(got.t[p].double(), want.t[p].double()), (name, p)
            assert float(got.cost[p, 0]) == float(got.cost[p, 1]), (name, p)
            continue
        assert float(got.cost[p, 1]) <= float(got.cost[p, 0]), (name, p)
        x0, x1 = gather_correspondences(m[p], n, kp0[p], kp1[p])
        keep = np.isfinite(x0).all(1) & np.isfinite(x1).all(1)
        e_got = epipolar_error(essential_to_fundamental(got.E[p].double(), intr[p]), x0[keep], x1[keep]).sqrt()
        e_ref = epipolar_error(essential_to_fundamental(want.E[p], intr[p]), x0[keep], x1[keep]).sqrt()
        w.px = max(w.px, float((e_got - e_ref).abs().max()))
        if pose:
            rot, tra = ps.pose_errors_deg(got.R[p].double(), got.t[p].double(), want.R[p], want.t[p])
            w.rot, w.tra = max(w.rot, rot), max(w.tra, tra)
        if last is not None:
            w.step = max(w.step, last[p])


def triangulation(lib, batch, pose, w):
    """lg_triangulate's statements on a batch against triangulate_reference: ok and the zeros exactly, the points
    relative to their depth."""
    m, counts, kp0, kp1, intr = batch
    for p in range(m.shape[0]):
        x0, x1, pts = host_rows(m[p], int(counts[p]), kp0[p], kp1[p])
        n = len(pts)
        kk = np.ascontiguousarray(intr[p].numpy().astype(np.float32).reshape(8))
        r = np.ascontiguousarray(pose.R[p].numpy().astype(np.float32).reshape(9))
        t = np.ascontiguousarray(pose.t[p].numpy().astype(np.float32).reshape(3))
        inl = np.ascontiguousarray(pose.inliers[p, :max(n, 1)].numpy().astype(np.uint8))
        out, ok = np.zeros((max(n, 1), 3), dtype=np.float32), np.zeros(max(n, 1), dtype=np.uint8)
        lib.host_triangulate(ptr(pts), n, ptr(kk), ptr(r), ptr(t), ptr(inl), ptr(out), ptr(ok))
        want, want_ok = triangulate_reference(torch.from_numpy(r).double(), torch.from_numpy(t).double(), x0, x1, intr[p], inl[:n])
        assert np.array_equal(ok[:n], want_ok.numpy()), ("triangulation", p)
        rows = want_ok.numpy().astype(bool)
        assert not out[:n][~rows].any(), ("triangulation", p)
        if rows.any():
            w.rel = max(w.rel, float((np.abs(out[:n][rows] - want.numpy()[rows]).max(1) / want.numpy()[rows, 2]).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", type=int, default=0)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        w = Worst()
        if args.scene:
            b = ps.batch(((args.scene, False),), args.scene)
            from lightglue_amd import essential_reference

            ref = essential_reference(*b, ps.THRESHOLD, ps.HYPOTHESES, ps.REFITS, ps.SEED)
            got, last = host_polish(lib, b, host_ransac(lib, b))
            compare(f"k {args.scene}", b, got, ps.polished(ref, *b), w, last=last)
            triangulation(lib, b, got, w)
        else:
            b = ps.six()
            got, last = host_polish(lib, b, host_ransac(lib, b))
            compare("the six", b, got, ps.six_polished(), w, last=last)
            b, pose = ps.ragged_given()
            got, last = host_polish(lib, b, pose)
            compare("ragged", b, got, ps.ragged_polished(), w, skip=(ps.RAGGED_FIVE,), last=last)
            assert all(bool(torch.isfinite(t[ps.RAGGED_FIVE].double()).all()) for t in got), "the 5-row pair"
            triangulation(lib, b, pose, w)
            triangulation(lib, b, got, w)
            b, pose = ps.full_width()
            got, last = host_polish(lib, b, pose)
            compare("full width", b, got, ps.full_width_polished(), w, last=last)
            b, pose = ps.keep_rule()
            got, _ = host_polish(lib, b, pose)
            compare("keep rule", b, got, ps.polished(pose, *b), w)
            assert int(got.kept[0]) == 0
            for k, seed in es.PLANAR_SEEDS:
                pl = es.planar(k, seed)
                b = pl[:4] + (pl[5],)
                given = host_ransac(lib, b)
                got, _ = host_polish(lib, b, given)
                ok = int(got.kept[0]) == 0 or int(got.num_inliers[0]) >= int(given.num_inliers[0])
                ok = ok and float(got.cost[0, 1]) <= float(got.cost[0, 0]) and all(bool(torch.isfinite(t.double()).all()) for t in got)
                print(f"  planar k {k} seed {seed}: kept {int(got.kept[0])}, inliers {int(given.num_inliers[0])} -> "
                      f"{int(got.num_inliers[0])}, cost {float(got.cost[0, 0]):.4f} -> {float(got.cost[0, 1]):.4f} px²")
                assert ok, (k, seed)
        print(f"the polish against polish_reference, {w.pairs} pairs: {w.bad} differ in mask, counts or kept; R {w.rot:.3e} deg, "
              f"t {w.tra:.3e} deg; E per point {w.px:.3e} px; triangulated points {w.rel:.3e} of their depth; the longest last "
              f"accepted step {w.step:.3e} rad")
        assert w.bad == 0 and w.rot < TOOL_BOUND_DEG and w.tra < TOOL_BOUND_DEG and w.px < TOOL_BOUND_PX and w.rel < TOOL_BOUND_REL


if __name__ == "__main__":
    main()
