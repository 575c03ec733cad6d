"""The five-point RANSAC's statements on the CPU, before any GPU run: csrc/lightglue_essential_math.h is
__host__ __device__, tools/essential_host.cpp wraps its 5-sample, five-point solve (the four lanes of a hypothesis
run in turn), one refit round as the finalize kernel orders it and the pose, and this script compares them with the
float64 contract in lightglue_amd/geometry_contract.py on the calibrated scenes of tests/essential_scenes.py (k = 24, 64, 200
and the alternates, rows as they are and reversed, 64 hypotheses each). It prints the worsts the bounds of
tests/test_gpu_essential.py are pinned from (four times each): the sample-point epipolar error of a kept candidate
(SOLVE_BOUND_PX), the refit against essential_refit per point on the ground-truth mask (REFIT_BOUND_PX), R and t
against essential_reference's in degrees (POSE_BOUND_DEG), the last two from the whole call run serially on every
pair the GPU tests run, where masks, counts, valid and best must equal the reference's. The figures are in
profiles/geometry/INDEX.md. ESSENTIAL_HOST_VERBOSE=1 prints each disagreement. No GPU.

    python tools/essential_host_check.py
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

import essential_scenes as es  # noqa: E402
from lightglue_amd import (camera_coordinates, epipolar_error, essential_refit, essential_to_fundamental,  # noqa: E402
                           pose_from_essential_reference, ransac_samples5, solve5_reference)


def build(tmp):
    so = os.path.join(tmp, "libessential_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "essential_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def canonical_match(got, want):
    """The largest entry difference after pairing each candidate of got [n, 9] with its nearest of want [n, 9], up to
    sign (two entries of nearly the largest magnitude: the sign rule may pick either)."""
    worst = 0.0
    for g in got:
        worst = max(worst, float(np.minimum(np.abs(want - g).max(1), np.abs(want + g).max(1)).min()))
    return worst


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        hyp = 64
        for count in (5, 6, 7, 37, 2048):
            got = np.zeros((hyp, 5), dtype=np.int32)
            lib.host_samples5(es.SEED, hyp, count, ptr(got))
            assert np.array_equal(got, ransac_samples5(es.SEED, hyp, count).numpy()), count
        print("samples: host statements equal ransac_samples5 at count 5, 6, 7, 37, 2048")
        intr = es.intrinsics()
        kk = np.ascontiguousarray(intr.numpy().reshape(8))
        st = dict(kept=0, total=0, count_diff=0, worst=0.0, entry=0.0, low=np.inf, low_all=np.inf)
        scenes = [(k, alt) for k in (24, 64, 200) for alt in (False, True)]
        for k, alt in scenes:
            k0, k1 = es.scene(k, alt)[:2]
            for flip in (False, True):
                x0, x1 = (k0.flip(0), k1.flip(0)) if flip else (k0, k1)
                q0, q1 = camera_coordinates(x0, intr[0]), camera_coordinates(x1, intr[1])
                pts = np.ascontiguousarray(torch.cat([x0, x1], 1).numpy().astype(np.float32))
                samples = np.ascontiguousarray(ransac_samples5(es.SEED, hyp, k).numpy())
                cands, num = np.zeros((hyp, 10, 9), dtype=np.float32), np.zeros((hyp,), dtype=np.int32)
                low = np.zeros((hyp,), dtype=np.float64)
                lib.host_solve5(ptr(pts), k, ptr(kk), ptr(samples), hyp, ptr(cands), ptr(num), ptr(low))
                for s, c, n, lo in zip(samples, cands, num, low):
                    ref = solve5_reference(q0, q1, s)
                    st["total"] += 1
                    st["low_all"] = min(st["low_all"], lo)
                    if not es.kept(ref, x0, x1, s, intr):
                        continue
                    st["kept"] += 1
                    st["low"] = min(st["low"], lo)
                    if int(n) != len(ref.candidates):
                        st["count_diff"] += 1
                        if os.environ.get("ESSENTIAL_HOST_VERBOSE"):
                            print(f"  k {k} alt {alt} flip {flip} sample {s.tolist()}: {int(n)} against {len(ref.candidates)}, "
                                  f"eigenvalues {np.sort_complex(ref.eigenvalues)}")
                        continue
                    if n:
                        st["entry"] = max(st["entry"], canonical_match(c[:n].astype(np.float64), ref.candidates.reshape(-1, 9)))
                    for e in c[:n]:
                        f = essential_to_fundamental(torch.from_numpy(e).double(), intr)
                        st["worst"] = max(st["worst"], float(epipolar_error(f, x0[s], x1[s]).sqrt().max()))
        print(f"solve5: {st['kept']} of {st['total']} hypotheses kept, {st['count_diff']} candidate-count disagreements, worst "
              f"sample-point epipolar error {st['worst']:.3e} px, worst entry difference to the reference's candidate "
              f"{st['entry']:.3e}; smallest pivot of the 10 x 20 elimination {st['low']:.3e} on the kept, {st['low_all']:.3e} on all")
        worst_px, worst_rot, worst_t = 0.0, 0.0, 0.0
        for k, alt in scenes + [(2048, False)]:
            k0, k1, gt = es.scene(k, alt)[:3]
            pts = np.ascontiguousarray(torch.cat([k0, k1], 1).numpy().astype(np.float32))
            mask = np.ascontiguousarray(gt.numpy().astype(np.uint8))
            got = np.zeros((9,), dtype=np.float32)
            assert lib.host_refit_e(ptr(pts), ptr(mask), k, ptr(kk), ptr(got)) == 1
            q0, q1 = camera_coordinates(k0[gt], intr[0]), camera_coordinates(k1[gt], intr[1])
            want = essential_refit(q0, q1)
            e = epipolar_error(essential_to_fundamental(torch.from_numpy(got).double(), intr), k0, k1).sqrt()
            worst_px = max(worst_px, float((e - epipolar_error(essential_to_fundamental(want, intr), k0, k1).sqrt()).abs().max()))
            r, t, fronts = np.zeros((9,), dtype=np.float32), np.zeros((3,), dtype=np.float32), np.zeros((4,), dtype=np.int32)
            front = lib.host_pose(ptr(got), ptr(pts), ptr(mask), k, ptr(kk), ptr(r), ptr(t), ptr(fronts))
            r_want, t_want, front_want, _ = pose_from_essential_reference(want, q0, q1)
            assert front == front_want == int(gt.sum()) and sorted(fronts.tolist())[2] < front, (k, alt, fronts, front_want)
            rot, tra = es.pose_errors_deg(r.reshape(3, 3), t, r_want, t_want)
            worst_rot, worst_t = max(worst_rot, rot), max(worst_t, tra)
        print(f"refit (camera coordinates, normal_accumulate_f, the Jacobi ordering, denormalise64, project_essential, fp32 "
              f"output) against essential_refit on the ground-truth mask: worst per-point difference {worst_px:.3e} px; the "
              f"pose of it (svd3, pose_candidate, in_front, fp32 output) against pose_from_essential_reference: R {worst_rot:.3e} "
              f"deg, t {worst_t:.3e} deg, over {len(scenes) + 1} scenes")
        check_whole(lib)


def host_essential(lib, m, count, kp0, kp1, intr):
    """lg_ransac_essential's statements for one pair on the CPU -> (e, r, t, inliers [count], num, front, valid, best)."""
    from lightglue_amd.geometry import gather_correspondences

    x0, x1 = gather_correspondences(m, count, kp0, kp1)
    n = len(x0)
    pts = np.ascontiguousarray(np.concatenate([x0, x1], 1).astype(np.float32).reshape(-1, 4))
    kk = np.ascontiguousarray(intr.numpy().astype(np.float32).reshape(8))
    e, r, t = np.zeros(9, dtype=np.float32), np.zeros(9, dtype=np.float32), np.zeros(3, dtype=np.float32)
    inl, out = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(4, dtype=np.int32)
    lib.host_essential(ptr(pts), n, ptr(kk), ctypes.c_float(es.THRESHOLD), es.HYPOTHESES, es.REFITS, es.SEED, ptr(e), ptr(r),
                       ptr(t), ptr(inl), ptr(out))
    return e.reshape(3, 3), r.reshape(3, 3), t, inl[:n], out


def check_whole(lib):
    """The whole call on the CPU against essential_reference on every pair the GPU tests run: masks, counts, valid and
    best exactly; E per point in pixels, R and t in degrees."""
    cases = [("ragged", es.ragged(), es.ragged_reference())]
    for k in (24, 64, 200):
        cases.append((f"alternate k {k}", es.batch(((k, k),), k, True) + (es.batch_intrinsics(1),), es.reference(k, True)))
    cases.append(("k 2048", es.batch(((2048, 2048),), 2048) + (es.batch_intrinsics(1),), es.reference(2048)))
    for k, seed in es.PLANAR_SEEDS:
        cases.append((f"planar k {k} seed {seed}", es.planar(k, seed)[:4] + (es.planar(k, seed)[5],), es.planar_reference(k, seed)))
    worst_px, worst_rot, worst_t, pairs, bad = 0.0, 0.0, 0.0, 0, 0
    for name, (m, counts, kp0, kp1, intr), want in cases:
        for p in range(m.shape[0]):
            e, r, t, inl, out = host_essential(lib, m[p], int(counts[p]), kp0[p], kp1[p], intr[p])
            n = len(inl)
            same = (out.tolist() == [int(want.num_inliers[p]), int(want.num_front[p]), int(want.valid[p]), int(want.best[p])]
                    and np.array_equal(inl, want.inliers[p, :n].numpy()))
            pairs += 1
            if not same:
                bad += 1
                print(f"  {name}, pair {p}: (num, front, valid, best) {out.tolist()} against "
                      f"{[int(want.num_inliers[p]), int(want.num_front[p]), int(want.valid[p]), int(want.best[p])]}")
                continue
            if not out[2]:
                assert not e.any() and not r.any() and not t.any()
                continue
            from lightglue_amd.geometry import gather_correspondences

            x0, x1 = gather_correspondences(m[p], int(counts[p]), kp0[p], kp1[p])
            keep = np.isfinite(x0).all(1) & np.isfinite(x1).all(1)
            got = epipolar_error(essential_to_fundamental(torch.from_numpy(e).double(), intr[p]), x0[keep], x1[keep]).sqrt()
            ref = epipolar_error(essential_to_fundamental(want.E[p], intr[p]), x0[keep], x1[keep]).sqrt()
            worst_px = max(worst_px, float((got - ref).abs().max()))
            if "planar" in name:
                continue  # two poses fit a plane
            rot, tra = es.pose_errors_deg(r, t, want.R[p], want.t[p])
            worst_rot, worst_t = max(worst_rot, rot), max(worst_t, tra)
    print(f"the whole call against essential_reference, {pairs} pairs (the ragged batch, the alternates, k = 2048, the planar "
          f"scenes): {bad} differ in mask, counts, valid or best; E per point {worst_px:.3e} px; R {worst_rot:.3e} deg, "
          f"t {worst_t:.3e} deg (the planar scenes' poses left out)")


if __name__ == "__main__":
    main()
