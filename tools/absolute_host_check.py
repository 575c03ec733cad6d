"""The absolute pose's statements on the CPU, before any GPU run: csrc/lightglue_absolute_math.h is __host__ __device__,
tools/absolute_host.cpp wraps its 3-sample, P3P solve (the four lanes of a hypothesis run in turn), fp32 score, one
Levenberg-Marquardt refit as the finalize kernel orders it and the whole call, and this script compares them with the
float64 contract in lightglue_amd/geometry_contract.py on the scenes of tests/absolute_scenes.py. It prints the worsts the
bounds of tests/test_gpu_absolute.py are pinned from (four times each): a candidate's entries against the reference's
(ENTRY_BOUND) and its sample points' reprojection error (SOLVE_BOUND_PX) on the hypotheses the reference keeps (k = 24,
64, 200 and the alternates, rows as they are and reversed, 64 hypotheses each); R and t of the whole call against
absolute_pose_reference's (POSE_BOUND_DEG, POSE_BOUND_T) on every pair the GPU tests run, where masks, counts, valid
and best must equal the reference's; and the table kAbsoluteLmRounds is chosen from: the worst difference of one refit
from the RANSAC winner to absolute_refit_reference's converged pose, per number of rounds. The figures are in
profiles/geometry/INDEX.md. ABSOLUTE_HOST_VERBOSE=1 prints each disagreement. No GPU.

    python tools/absolute_host_check.py
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
import torch  # noqa: E402

import absolute_scenes as ab  # noqa: E402
from lightglue_amd import (absolute_refit_reference, ransac_samples3, reprojection_error, solve3_reference)  # noqa: E402

VERBOSE = bool(os.environ.get("ABSOLUTE_HOST_VERBOSE"))


def build(tmp):
    so = os.path.join(tmp, "libabsolute_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "absolute_host.cpp"), "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.host_score.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]
    lib.host_absolute.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int,
                                  ctypes.c_int32, ctypes.c_int] + [ctypes.c_void_p] * 4
    return lib


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def rows5(points, image, n):
    return np.ascontiguousarray(torch.cat([points[:n], image[:n]], 1).numpy().astype(np.float32))


def check_samples(lib):
    for count in (3, 4, 7, 37, 2048):
        got = np.zeros((64, 3), dtype=np.int32)
        lib.host_samples3(ab.SEED, 64, count, ptr(got))
        assert np.array_equal(got, ransac_samples3(ab.SEED, 64, count).numpy()), count
    print("samples: host statements equal ransac_samples3 at count 3, 4, 7, 37, 2048")


def check_solve(lib):
    hyp, intr = 64, ab.intrinsics()
    kk = np.ascontiguousarray(intr.numpy())
    st = dict(kept=0, total=0, count_diff=0, worst=0.0, entry=0.0, fmt=0.0, det=0.0, cands=0)
    for k in (24, 64, 200):
        for alt in (False, True):
            pts0, kp0 = ab.scene(k, alt)[:2]
            for flip in (False, True):
                pts, kp = (pts0.flip(0), kp0.flip(0)) if flip else (pts0, kp0)
                rows = rows5(pts, kp, k)
                samples = np.ascontiguousarray(ransac_samples3(ab.SEED, hyp, k).numpy())
                cands, num = np.zeros((hyp, 4, 12), dtype=np.float32), np.zeros((hyp,), dtype=np.int32)
                lib.host_solve3(ptr(rows), k, ptr(kk), ptr(samples), hyp, ptr(cands), ptr(num))
                for s, c, n in zip(samples, cands, num):
                    ref = solve3_reference(pts, kp, intr, s)
                    st["total"] += 1
                    if not ab.kept(ref, pts, kp, s, intr):
                        continue
                    st["kept"] += 1
                    if int(n) != len(ref.R):
                        st["count_diff"] += 1
                        if VERBOSE:
                            print(f"  k {k} alt {alt} flip {flip} sample {s.tolist()}: {int(n)} against {len(ref.R)}, roots {ref.roots}")
                        continue
                    want = np.concatenate([ref.R.reshape(-1, 9), ref.t.reshape(-1, 3)], 1)
                    for i in range(n):  # (the same order: ascending |R X_s0 + t|)
                        st["cands"] += 1
                        st["entry"] = max(st["entry"], float(np.abs(c[i].astype(np.float64) - want[i]).max()))
                        g = torch.from_numpy(c[i]).double()
                        st["det"] = max(st["det"], abs(float(torch.linalg.det(g[:9].reshape(3, 3))) - 1.0))
                        st["worst"] = max(st["worst"], float(reprojection_error(g[:9].reshape(3, 3), g[9:], pts[s], kp[s], intr).sqrt().max()))
                        w32 = torch.from_numpy(want[i].astype(np.float32)).double()
                        st["fmt"] = max(st["fmt"], float(reprojection_error(w32[:9].reshape(3, 3), w32[9:], pts[s], kp[s], intr).sqrt().max()))
    print(f"solve3: {st['kept']} of {st['total']} hypotheses kept, {st['count_diff']} candidate-count disagreements, {st['cands']} "
          f"candidates; worst sample-point reprojection error {st['worst']:.3e} px (the reference's own candidates rounded to fp32: "
          f"{st['fmt']:.3e} px), worst entry difference to the reference's candidate {st['entry']:.3e}, worst |det R - 1| {st['det']:.3e}")


def whole_cases():
    cases = [("ragged", ab.ragged(), ab.ragged_reference(), ab.HYPOTHESES)]
    for k in (24, 64, 200):
        cases.append((f"alternate k {k}", ab.batch(((k, k),), k, True) + (ab.batch_intrinsics(1),), ab.reference(k, True), ab.HYPOTHESES))
    cases.append(("k 2048", ab.batch(((2048, 2048),), 2048) + (ab.batch_intrinsics(1),), ab.reference(2048, False, ab.WIDE_HYPOTHESES),
                  ab.WIDE_HYPOTHESES))
    cases.append(("k 64, 4096 hypotheses", ab.batch(((64, 64),), 64) + (ab.batch_intrinsics(1),),
                  ab.reference(64, False, ab.FULL_HYPOTHESES), ab.FULL_HYPOTHESES))
    for k, seed in ab.PLANAR_SEEDS:
        s = ab.scene(k, planar_seed=seed)
        cases.append((f"planar k {k} seed {seed}", ab.batch_of([s], [k], k) + (ab.batch_intrinsics(1),),
                      ab.reference(k, planar_seed=seed), ab.HYPOTHESES))
    _, marks, got, _ = ab.chain_reference()
    cases.append(("the chain's landmarks", (marks.points.float(), marks.image.float(), marks.counts, ab.chain_intrinsics()[1]), got,
                  ab.HYPOTHESES))
    return cases


def host_absolute(lib, points, image, count, intr, hypotheses, rounds):
    n = min(max(int(count), 0), len(points))
    rows = rows5(points, image, n) if n else np.zeros((1, 5), dtype=np.float32)
    kk = np.ascontiguousarray(intr.numpy().astype(np.float32))
    r, t = np.zeros(9, dtype=np.float32), np.zeros(3, dtype=np.float32)
    inl, out = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(3, dtype=np.int32)
    lib.host_absolute(ptr(rows), n, ptr(kk), ab.THRESHOLD, hypotheses, ab.REFITS, ab.SEED, rounds, ptr(r), ptr(t), ptr(inl), ptr(out))
    return r.reshape(3, 3), t, inl[:n], out


def check_whole(lib):
    rounds = lib.host_lm_rounds()
    worst_rot, worst_t, pairs, bad = 0.0, 0.0, 0, 0
    for name, (points, image, counts, intr), want, hypotheses in whole_cases():
        for p in range(points.shape[0]):
            r, t, inl, out = host_absolute(lib, points[p], image[p], counts[p], intr[p], hypotheses, rounds)
            n = len(inl)
            ref = [int(want.num_inliers[p]), int(want.valid[p]), int(want.best[p])]
            pairs += 1
            if not (out.tolist() == ref and np.array_equal(inl, want.inliers[p, :n].numpy())):
                bad += 1
                print(f"  {name}, pair {p}: (num, valid, best) {out.tolist()} against {ref}")
                continue
            if not out[1]:
                assert not r.any() and not t.any()
                continue
            rot, tra = ab.pose_errors(r, t, want.R[p], want.t[p])
            if VERBOSE:
                print(f"  {name}, pair {p}: {out[0]} inliers, R {rot:.3e} deg, t {tra:.3e}")
            worst_rot, worst_t = max(worst_rot, rot), max(worst_t, tra)
    print(f"the whole call ({rounds} LM rounds a refit) against absolute_pose_reference, {pairs} pairs (the ragged batch, the "
          f"alternates, k = 2048, 4096 hypotheses, the planar scenes, the chain's landmarks): {bad} differ in mask, counts, valid or "
          f"best; R {worst_rot:.3e} deg, t {worst_t:.3e} (map units)")


def check_rounds(lib):
    """One refit from the RANSAC winner (refits = 0) over its mask, per number of LM rounds, against the converged
    reference: the worst over the scenes of the rotation difference, of |t - t_ref| and of the cost's excess."""
    cases = []
    for name, (points, image, counts, intr), _, hypotheses in whole_cases():
        for p in range(points.shape[0]):
            r, t, inl, out = host_absolute(lib, points[p], image[p], counts[p], intr[p], hypotheses, 0)
            if not out[1]:
                continue
            n = len(inl)
            pose = np.ascontiguousarray(np.concatenate([r.reshape(9), t]).astype(np.float32))
            rows = inl.astype(bool)
            ref = absolute_refit_reference(pose[:9].reshape(3, 3).astype(np.float64), pose[9:].astype(np.float64),
                                           points[p][:n][rows], image[p][:n][rows], intr[p])
            if ref is None:
                continue
            cases.append((rows5(points[p], image[p], n), np.ascontiguousarray(inl), n,
                          np.ascontiguousarray(intr[p].numpy().astype(np.float32)), pose, ref))
    print(f"LM rounds a refit, one refit from the RANSAC winner against absolute_refit_reference, worst of {len(cases)} pairs:")
    for rounds in range(1, 13):
        worst_rot, worst_t, worst_cost = 0.0, 0.0, 0.0
        for rows, mask, n, kk, pose, (r_ref, t_ref) in cases:
            out, cost = np.zeros(12, dtype=np.float32), np.zeros(2, dtype=np.float64)
            assert lib.host_refit(ptr(rows), ptr(mask), n, ptr(kk), ptr(pose), rounds, ptr(out), ptr(cost)) == 1
            rot, tra = ab.pose_errors(out[:9].reshape(3, 3), out[9:], r_ref, t_ref)
            pts, img = torch.from_numpy(rows[:, :3]).double(), torch.from_numpy(rows[:, 3:]).double()
            ref_cost = float(reprojection_error(r_ref, t_ref, pts[mask.astype(bool)], img[mask.astype(bool)], torch.from_numpy(kk)).sum())
            worst_rot, worst_t = max(worst_rot, rot), max(worst_t, tra)
            worst_cost = max(worst_cost, (cost[1] - ref_cost) / ref_cost)
        print(f"  {rounds:2d} rounds: R {worst_rot:.3e} deg, t {worst_t:.3e}, cost above the reference's {worst_cost:.3e} relative")


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        check_samples(lib)
        check_solve(lib)
        check_rounds(lib)
        check_whole(lib)


if __name__ == "__main__":
    main()
