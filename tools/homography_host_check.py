"""The homography's per-lane statements on the CPU, before any GPU run: csrc/lightglue_geometry_math.h is
__host__ __device__, tools/homography_host.cpp wraps its 4-sample, 4-point solve (in double and in float) and
transfer-error test, and this script compares them with the float64 contract in lightglue_amd/geometry_contract.py on the
planar scenes of tests/homography_scenes.py (k = 8, 24, 64, 200, the alternates and the rotation scene, rows as
they are and reversed, 64 hypotheses each). Per real type: the hypotheses the reference keeps (a pivot >= 1e-3,
orientation determinants >= 1e-3, its own candidate rounded to fp32 within 5e-3 px of its sample), disagreements
on whether there is a candidate, and the worst transfer error of a sample point under the candidate; then one
refit round as the finalize kernel orders it against homography_refit, and the error test's counts on the score
inputs. The figures are in profiles/geometry/INDEX.md. No GPU.

    python tools/homography_host_check.py
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

import homography_scenes as hs  # noqa: E402
from lightglue_amd import homography_refit, ransac_samples, solve4_reference, transfer_error  # noqa: E402


def build(tmp):
    so = os.path.join(tmp, "libhomography_host.so")
    subprocess.run([os.environ.get("CXX", "c++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off",
                    "-I" + os.path.join(PKG, "csrc"), os.path.join(REPO, "tools", "homography_host.cpp"), "-o", so], check=True)
    return ctypes.CDLL(so)


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        lib = build(tmp)
        hyp = 64
        for count in (4, 5, 7, 37, 2048):
            got = np.zeros((hyp, 4), dtype=np.int32)
            lib.host_samples4(hs.SEED, hyp, count, ptr(got))
            assert np.array_equal(got, ransac_samples(hs.SEED, hyp, count, size=4).numpy()), count
        print("samples: host statements equal ransac_samples(size=4) at count 4, 5, 7, 37, 2048")
        stats = {0: dict(kept=0, total=0, count_diff=0, worst=0.0), 1: dict(kept=0, total=0, count_diff=0, worst=0.0)}
        scenes = [(k, alt, False) for k in (8, 24, 64, 200) for alt in (False, True)] + [(hs.ROTATION_K, False, True)]
        for k, alt, rot in scenes:
            k0, k1, _, _ = hs.scene(k, alt, rot)
            for flip in (False, True):
                x0, x1 = (k0.flip(0), k1.flip(0)) if flip else (k0, k1)
                pts = np.ascontiguousarray(torch.cat([x0, x1], 1).numpy().astype(np.float32))
                samples = np.ascontiguousarray(ransac_samples(hs.SEED, hyp, k, size=4).numpy())
                refs = [solve4_reference(x0, x1, s) for s in samples]
                fits = [all(float(transfer_error(torch.from_numpy(h.astype(np.float32)), x0[s], x1[s]).sqrt().max())
                            <= hs.FORMAT_LIMIT for h in ref.candidates) for s, ref in zip(samples, refs)]
                for use_float in (0, 1):
                    cands, num = np.zeros((hyp, 9), dtype=np.float32), np.zeros((hyp,), dtype=np.int32)
                    lib.host_solve4(use_float, ptr(pts), k, ptr(samples), hyp, ptr(cands), ptr(num))
                    st = stats[use_float]
                    for s, ref, fit, c, n in zip(samples, refs, fits, cands, num):
                        st["total"] += 1
                        if not (ref.pivot >= hs.PIVOT_MARGIN and ref.orientation >= hs.ORIENTATION_MARGIN and fit):
                            continue
                        st["kept"] += 1
                        if int(n) != len(ref.candidates):
                            st["count_diff"] += 1
                        elif n:
                            st["worst"] = max(st["worst"], float(transfer_error(torch.from_numpy(c), x0[s], x1[s]).sqrt().max()))
        for use_float, name in ((0, "double"), (1, "float")):
            st = stats[use_float]
            print(f"solve4<{name}>: {st['kept']} of {st['total']} hypotheses kept, {st['count_diff']} candidate-count "
                  f"disagreements, worst sample-point transfer error {st['worst']:.3e} px")
        worst = 0.0
        for k, alt, rot in scenes + [(2048, False, False)]:
            k0, k1, gt, _ = hs.scene(k, alt, rot)
            pts = np.ascontiguousarray(torch.cat([k0, k1], 1).numpy().astype(np.float32))
            mask = np.ascontiguousarray(gt.numpy().astype(np.uint8))
            got = np.zeros((9,), dtype=np.float32)
            assert lib.host_refit_h(ptr(pts), ptr(mask), k, ptr(got)) == 1
            e = transfer_error(torch.from_numpy(got), k0, k1).sqrt()
            worst = max(worst, float((e - transfer_error(homography_refit(k0[gt], k1[gt]), k0, k1).sqrt()).abs().max()))
        print(f"refit (normal_accumulate_h, the Jacobi ordering, denormalise_h, fp32 output) against homography_refit on the "
              f"ground-truth mask: worst per-point difference {worst:.3e} px over {len(scenes) + 1} scenes")
        m, counts, kp0, kp1, cands, want = hs.score_inputs()
        from lightglue_amd.geometry import gather_correspondences

        bad = 0
        for p in range(len(counts)):
            x0, x1 = gather_correspondences(m[p], int(counts[p]), kp0[p], kp1[p])
            pts = np.ascontiguousarray(np.concatenate([x0, x1], 1).astype(np.float32))
            c = np.ascontiguousarray(cands[p].numpy())
            got = np.zeros((c.shape[0],), dtype=np.int32)
            lib.host_score_h(ptr(pts), len(pts), ptr(c), c.shape[0], ctypes.c_float(hs.THRESHOLD ** 2), ptr(got))
            bad += int((got != want[p].numpy()).sum())
        print(f"is_inlier_h: {bad} of {want.numel()} counts differ from the float64 counts on score_inputs")


if __name__ == "__main__":
    main()
