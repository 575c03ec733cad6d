"""A/B on one GPU: FundamentalRansac.verify (two gfx950 launches) against the same contract restated as batched
framework ops on the same device (ransac_reference's stages: the samples gathered, an SVD null space per
hypothesis, the cubic's roots as companion eigenvalues, every candidate scored by products over all
correspondences, refits by eigh / svd), and the share verify adds to verify_source_images over match_source_images.

Cases: K in {256, 1024, 2048} correspondences a pair (all pairs full), P in {1, 16} pairs, H = 512, R = 2, 25 %
outliers. verify is timed as graph replays (N calls captured back to back, replay time / N, events on the
stream); the framework arm is timed eagerly, by a host clock around two calls that end in a device synchronise:
its SVD and eigenvalue routines synchronise with the host, which a capture refuses (framework_mode in the
record; verify_eager_us is our arm under the same clock). Arms alternate; --repeats repeats, median [min, max].

The pipeline part: 480 x 640 grey sources at the target size, 512 keypoints a side, the seeded 9-layer matcher,
P = 1 and 2: match_source_images and verify_source_images each captured as one graph, replayed alternately.

--model homography: the same method for HomographyRansac.verify on planar scenes (the framework arm: an SVD null
vector per hypothesis, the orientation rule, the transfer error, refits by eigh), with FundamentalRansac.verify
re-measured at the same K, P and H on the same points in the same repeats, the three arms alternating
(fundamental_us in the record; the two estimators run the same launches, so the comparison is of the models'
arithmetic). The pipeline part is the fundamental matrix's alone.

--model essential: EssentialRansac.verify on calibrated_scene's pairs (the scenes of the fundamental matrix with
their cameras) and FundamentalRansac.verify on the same points in the same repeats, alternating, and the
lg_ransac_solve5 hook alone on the call's own samples under the same method (solve5_us: the sample, the solve and the
candidates of every hypothesis without the scoring pass, the finalize launch and the pose). No framework arm: batched
framework ops have no five-point solve to put next to it.

--model essential --polish N: what the pose polish adds. EssentialRansac.verify at polish = 0 and at polish = N on
calibrated_scene's pairs at 1 px of noise, alternating in the same repeats, and the PosePolish.refine hook alone on
the call's own pose at N rounds and at 1 round (added_us: the medians' difference of the two verify arms;
per_round_us: the hook's (N rounds - 1 round) / (N - 1); hook_one_round_us holds the launch, the staging, the first
pass, the mask and the outputs). Written to profiles/geometry/ab_polish.jsonl unless --out is given.

--model absolute: AbsolutePoseRansac.localize on absolute_scene's 2D-3D correspondences: the whole call, the call
without refits, lg_ransac_solve3 alone and lg_link_landmarks, all by graph replay (-> ab_absolute.jsonl).

    python tools/geometry_ab.py [--model fundamental|homography|essential|absolute] [--repeats 5] [--part all|verify|pipeline]
                                [--polish N] [--out profiles/geometry/ab.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "lightglue-with-flashattentionv2-tensorrt_amd")]
import torch  # noqa: E402

from lightglue_amd import (EssentialRansac, FundamentalRansac, HomographyRansac, ImageInput, KeypointFrontend, PosePolish,  # noqa: E402
                           SuperPointEncoder,
                           calibrated_scene, match_source_images, matcher, planar_scene, ransac_samples, ransac_samples5,
                           seeded_superpoint_state_dict, two_view_scene, verify_source_images)
from lightglue_amd._host import call  # noqa: E402
from lightglue_amd.matches import MatchResult  # noqa: E402

H, R, THR, SEED = 512, 2, 3.0, 888
CALLS = 20  # calls a graph


def _rows(x0, x1):
    one = torch.ones_like(x0[..., 0])
    return torch.stack([x1[..., 0] * x0[..., 0], x1[..., 0] * x0[..., 1], x1[..., 0], x1[..., 1] * x0[..., 0],
                        x1[..., 1] * x0[..., 1], x1[..., 1], x0[..., 0], x0[..., 1], one], -1)


def _hartley(x, w):
    """x [P, K, 2], weights w [P, K] -> T [P, 3, 3] float64."""
    n = w.sum(1, keepdim=True)
    c = (x * w[..., None]).sum(1) / n
    d = (((x - c[:, None]) ** 2).sum(-1).sqrt() * w).sum(1) / n[:, 0]
    s = 2.0 ** 0.5 / d
    t = torch.zeros((x.shape[0], 3, 3), dtype=x.dtype, device=x.device)
    t[:, 0, 0], t[:, 1, 1], t[:, 2, 2] = s, s, 1.0
    t[:, 0, 2], t[:, 1, 2] = -s * c[:, 0], -s * c[:, 1]
    return t


def _apply(t, x):
    return x * t[:, None, 0, 0, None] + t[:, None, :2, 2]


def _inliers(f, x0, x1, thr2):
    """f [P, C, 3, 3], x [P, K, 2] (fp32) -> [P, C, K] bool."""
    h0 = torch.cat([x0, torch.ones_like(x0[..., :1])], -1)
    h1 = torch.cat([x1, torch.ones_like(x1[..., :1])], -1)
    l1 = torch.einsum("pcij,pkj->pcki", f, h0)
    l0 = torch.einsum("pcji,pkj->pcki", f, h1)
    d2 = (l1 * h1[:, None]).sum(-1) ** 2
    err = torch.maximum(d2 / (l1[..., 0] ** 2 + l1[..., 1] ** 2), d2 / (l0[..., 0] ** 2 + l0[..., 1] ** 2))
    return err <= thr2


def framework_ransac(x0, x1, samples):
    """x0, x1 [P, K, 2] fp32 on the GPU, samples [H, 7] -> (F [P, 3, 3] fp32, mask [P, K])."""
    pr, k, _ = x0.shape
    a0, a1 = x0.double(), x1.double()
    ones = torch.ones((pr, k), dtype=torch.float64, device=x0.device)
    t0, t1 = _hartley(a0, ones), _hartley(a1, ones)
    n0, n1 = _apply(t0, a0), _apply(t1, a1)
    a = _rows(n0[:, samples], n1[:, samples])                         # [P, H, 7, 9]
    null = torch.linalg.svd(a, full_matrices=True)[2][..., 7:9, :]    # [P, H, 2, 9]
    basis = torch.linalg.solve(null[..., 7:9], null)
    g, d = basis[..., 1, :].reshape(pr, -1, 3, 3), (basis[..., 0, :] - basis[..., 1, :]).reshape(pr, -1, 3, 3)
    det = torch.linalg.det

    def mixed(mask):
        return det(torch.stack([d[..., i, :] if mask >> i & 1 else g[..., i, :] for i in range(3)], -2))

    c3, c2, c1, c0 = mixed(7), mixed(3) + mixed(5) + mixed(6), mixed(1) + mixed(2) + mixed(4), mixed(0)
    comp = torch.zeros(c3.shape + (3, 3), dtype=torch.float64, device=x0.device)
    comp[..., 0, 0], comp[..., 0, 1], comp[..., 0, 2] = -c2 / c3, -c1 / c3, -c0 / c3
    comp[..., 1, 0], comp[..., 2, 1] = 1.0, 1.0
    lam = torch.linalg.eigvals(comp)                                  # [P, H, 3] complex
    real = lam.imag.abs() <= 1e-9 * lam.abs().clamp(min=1.0)
    fn = g[:, :, None] + lam.real[..., None, None] * d[:, :, None]    # [P, H, 3, 3, 3]
    f = torch.einsum("pji,phrjk,pkl->phril", t1, fn, t0)
    f = (f / f.flatten(-2).norm(dim=-1)[..., None, None]).reshape(pr, -1, 3, 3).float()
    inl = _inliers(f, x0, x1, THR * THR)
    counts = torch.where(real.reshape(pr, -1), inl.sum(-1), -1)
    best = counts.argmax(1)
    fb = f[torch.arange(pr, device=x0.device), best]
    mask = inl[torch.arange(pr, device=x0.device), best]
    for _ in range(R):
        w = mask.double()
        t0, t1 = _hartley(a0, w), _hartley(a1, w)
        rows = _rows(_apply(t0, a0), _apply(t1, a1)) * w[..., None]
        fe = torch.linalg.eigh(rows.transpose(1, 2) @ rows)[1][..., 0].reshape(pr, 3, 3)
        v = torch.linalg.svd(fe)[2][:, 2]
        fe = fe - (fe @ v[..., None]) * v[:, None]
        fb = t1.transpose(1, 2) @ fe @ t0
        fb = (fb / fb.flatten(1).norm(dim=1)[:, None, None]).float()
        mask = _inliers(fb[:, None], x0, x1, THR * THR)[:, 0]
    return fb, mask


def _rows_h(x0, x1):
    """[..., n, 2] x 2 -> [..., 2 n, 9]: the two rows a point of x1 ~ H x0."""
    one, zero = torch.ones_like(x0[..., 0]), torch.zeros_like(x0[..., 0])
    ra = torch.stack([-x0[..., 0], -x0[..., 1], -one, zero, zero, zero, x1[..., 0] * x0[..., 0], x1[..., 0] * x0[..., 1],
                      x1[..., 0]], -1)
    rb = torch.stack([zero, zero, zero, -x0[..., 0], -x0[..., 1], -one, x1[..., 1] * x0[..., 0], x1[..., 1] * x0[..., 1],
                      x1[..., 1]], -1)
    return torch.stack([ra, rb], -2).flatten(-3, -2)


def _inliers_h(h, x0, x1, thr2):
    """h [P, C, 3, 3], x [P, K, 2] (fp32) -> [P, C, K] bool."""
    q = torch.einsum("pcij,pkj->pcki", h, torch.cat([x0, torch.ones_like(x0[..., :1])], -1))
    err = (x1[:, None, :, 0] - q[..., 0] / q[..., 2]) ** 2 + (x1[:, None, :, 1] - q[..., 1] / q[..., 2]) ** 2
    return err <= thr2


def _orient(p):
    """p [P, H, 4, 2] -> the orientation determinants of the four triples [P, H, 4]."""
    out = []
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        a, b = p[..., j, :] - p[..., i, :], p[..., k, :] - p[..., i, :]
        out.append(a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0])
    return torch.stack(out, -1)


def framework_homography(x0, x1, samples):
    """x0, x1 [P, K, 2] fp32 on the GPU, samples [H, 4] -> (H [P, 3, 3] fp32, mask [P, K])."""
    pr, k, _ = x0.shape
    a0, a1 = x0.double(), x1.double()
    ones = torch.ones((pr, k), dtype=torch.float64, device=x0.device)
    t0, t1 = _hartley(a0, ones), _hartley(a1, ones)
    n0, n1 = _apply(t0, a0)[:, samples], _apply(t1, a1)[:, samples]              # [P, H, 4, 2]
    v = torch.linalg.svd(_rows_h(n0, n1), full_matrices=True)[2][..., 8, :]      # [P, H, 9]
    hn = (v / v[..., 8:9]).reshape(pr, -1, 3, 3)
    prod = torch.sign(_orient(n0)) * torch.sign(_orient(n1))
    good = (prod > 0).all(-1) | (prod < 0).all(-1)
    h = torch.linalg.inv(t1)[:, None] @ hn @ t0[:, None]
    h = (h / h.flatten(-2).norm(dim=-1)[..., None, None]).float()
    inl = _inliers_h(h, x0, x1, THR * THR)
    counts = torch.where(good, inl.sum(-1), -1)
    best = counts.argmax(1)
    hb = h[torch.arange(pr, device=x0.device), best]
    mask = inl[torch.arange(pr, device=x0.device), best]
    for _ in range(R):
        w = mask.double()
        t0, t1 = _hartley(a0, w), _hartley(a1, w)
        rows = _rows_h(_apply(t0, a0), _apply(t1, a1)) * w.repeat_interleave(2, 1)[..., None]
        he = torch.linalg.eigh(rows.transpose(1, 2) @ rows)[1][..., 0].reshape(pr, 3, 3)
        hb = torch.linalg.inv(t1) @ he @ t0
        hb = (hb / hb.flatten(1).norm(dim=1)[:, None, None]).float()
        mask = _inliers_h(hb[:, None], x0, x1, THR * THR)[:, 0]
    return hb, mask


def graph_of(fn, stream, calls):
    with torch.cuda.stream(stream):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(calls):
                fn()
    return g


def time_graph(g, stream, calls):
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        s.record(stream)
        g.replay()
        e.record(stream)
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / calls  # us a call


def time_eager(fn, calls):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def spread(v):
    return {"min": round(min(v), 2), "median": round(statistics.median(v), 2), "max": round(max(v), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--polish", type=int, default=0, help="with --model essential: the A/B of verify at polish 0 and N")
    ap.add_argument("--part", choices=("all", "verify", "pipeline"), default="all")
    ap.add_argument("--model", choices=("fundamental", "homography", "essential", "absolute"), default="fundamental")
    args = ap.parse_args()
    if args.polish and args.model != "essential":
        sys.exit("geometry_ab.py: --polish goes with --model essential")
    if args.out is None:
        name = "ab_polish.jsonl" if args.polish else ("ab_absolute.jsonl" if args.model == "absolute" else "ab.jsonl")
        args.out = os.path.join(REPO, "profiles", "geometry", name)
    if not torch.cuda.is_available():
        sys.exit("geometry_ab.py: needs a GPU (timings from anywhere else mean nothing)")
    dev = torch.device("cuda:0")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    stream = torch.cuda.Stream(dev)
    base = {"H": H, "refits": R, "threshold": THR, "repeats": args.repeats, "device": torch.cuda.get_device_name(0)}

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as out:
            out.write(line + "\n")

    fr = FundamentalRansac(THR, H, R, SEED)
    if args.model == "homography":
        homography_part(args, dev, stream, base, emit, fr)
        return
    if args.model == "absolute":
        absolute_part(args, dev, stream, base, emit)
        return
    if args.model == "essential":
        if args.polish:
            polish_part(args, dev, stream, base, emit)
        else:
            essential_part(args, dev, stream, base, emit, fr)
        return
    for k in (256, 1024, 2048) if args.part != "pipeline" else ():
        k0, k1, gt, _ = two_view_scene(k, k, 0.25, 0.25)
        samples = ransac_samples(SEED, H, k).long().to(dev)
        for pr in (1, 16):
            x0, x1 = k0.to(dev)[None].repeat(pr, 1, 1), k1.to(dev)[None].repeat(pr, 1, 1)
            m = torch.arange(k, dtype=torch.int32, device=dev)[None, :, None].repeat(pr, 1, 2).contiguous()
            counts = torch.full((pr,), k, dtype=torch.int32, device=dev)
            res = MatchResult(None, None, None, None, m, None, counts)
            with torch.no_grad():
                ours = lambda: fr.verify(res, x0, x1)              # noqa: E731
                theirs = lambda: framework_ransac(x0, x1, samples)  # noqa: E731
                mine, (_, their_mask) = ours(), theirs()
                torch.cuda.synchronize()
                rec = dict(base, part="verify", K=k, P=pr,
                           ours_mask_is_gt=bool((mine.inliers.bool().cpu() == gt[None]).all()),
                           framework_mask_is_gt=bool((their_mask.cpu() == gt[None]).all()))
                g = graph_of(ours, stream, CALLS)
                t_ours, t_theirs = [], []
                for _ in range(args.repeats):
                    t_ours.append(time_graph(g, stream, CALLS))
                    t_theirs.append(time_eager(theirs, 2))
                rec.update(verify_us=spread(t_ours), framework_us=spread(t_theirs), framework_mode="eager",
                           verify_eager_us=round(time_eager(ours, 50), 2),
                           framework_over_verify_median=round(statistics.median(t_theirs) / statistics.median(t_ours), 1))
            emit(rec)
            del g
    if args.part == "verify":
        return
    encoder = SuperPointEncoder(seeded_superpoint_state_dict(3))
    model = matcher.LightGlueMatcher(n_layers=9).eval()
    model.load_state_dict(matcher.seeded_state_dict(7, 9), strict=True)
    model = model.to(dev, torch.float16)
    fe, ii = KeypointFrontend(max_keypoints=512), ImageInput((480, 640))
    for pr in (1, 2):
        gen = torch.Generator().manual_seed(40 + pr)
        s0 = torch.randint(0, 256, (pr, 480, 640), generator=gen, dtype=torch.uint8).to(dev)
        s1 = torch.randint(0, 256, (pr, 480, 640), generator=gen, dtype=torch.uint8).to(dev)
        with torch.no_grad():
            a = lambda: match_source_images(ii, encoder, fe, model, s0, s1)          # noqa: E731
            b = lambda: verify_source_images(ii, encoder, fe, model, fr, s0, s1)     # noqa: E731
            counts = b()[0].counts.cpu().tolist()
            ga, gb = graph_of(a, stream, 1), graph_of(b, stream, 1)
            ta, tb = [], []
            for _ in range(args.repeats):
                ta.append(time_graph(ga, stream, 1))
                tb.append(time_graph(gb, stream, 1))
        ma, mb = statistics.median(ta), statistics.median(tb)
        emit(dict(base, part="pipeline", P=pr, source=[480, 640], max_keypoints=512, match_counts=counts,
                  match_source_images_us=spread(ta), verify_source_images_us=spread(tb),
                  verify_adds_us=round(mb - ma, 2), verify_share_of_total=round((mb - ma) / mb, 3)))


def homography_part(args, dev, stream, base, emit, fr):
    hr = HomographyRansac(THR, H, R, SEED)
    for k in (256, 1024, 2048):
        k0, k1, gt, _ = planar_scene(k, k, 0.25, 0.25)
        samples = ransac_samples(SEED, H, k, size=4).long().to(dev)
        for pr in (1, 16):
            x0, x1 = k0.to(dev)[None].repeat(pr, 1, 1), k1.to(dev)[None].repeat(pr, 1, 1)
            m = torch.arange(k, dtype=torch.int32, device=dev)[None, :, None].repeat(pr, 1, 2).contiguous()
            counts = torch.full((pr,), k, dtype=torch.int32, device=dev)
            res = MatchResult(None, None, None, None, m, None, counts)
            with torch.no_grad():
                ours = lambda: hr.verify(res, x0, x1)                   # noqa: E731
                fund = lambda: fr.verify(res, x0, x1)                   # noqa: E731
                theirs = lambda: framework_homography(x0, x1, samples)  # noqa: E731
                mine, (_, their_mask) = ours(), theirs()
                torch.cuda.synchronize()
                rec = dict(base, part="verify", model="homography", K=k, P=pr,
                           ours_mask_is_gt=bool((mine.inliers.bool().cpu() == gt[None]).all()),
                           framework_mask_is_gt=bool((their_mask.cpu() == gt[None]).all()))
                g, gf = graph_of(ours, stream, CALLS), graph_of(fund, stream, CALLS)
                t_ours, t_fund, t_theirs = [], [], []
                for _ in range(args.repeats):
                    t_ours.append(time_graph(g, stream, CALLS))
                    t_fund.append(time_graph(gf, stream, CALLS))
                    t_theirs.append(time_eager(theirs, 2))
                rec.update(verify_us=spread(t_ours), fundamental_us=spread(t_fund), framework_us=spread(t_theirs),
                           framework_mode="eager", verify_eager_us=round(time_eager(ours, 50), 2),
                           homography_over_fundamental_median=round(statistics.median(t_ours) / statistics.median(t_fund), 3),
                           framework_over_verify_median=round(statistics.median(t_theirs) / statistics.median(t_ours), 1))
            emit(rec)
            del g, gf


def essential_part(args, dev, stream, base, emit, fr):
    er = EssentialRansac(THR, H, R, SEED)
    for k in (256, 1024, 2048):
        k0, k1, gt, _, kk, _, _ = calibrated_scene(k, k, 0.25, 0.25)
        samples = ransac_samples5(SEED, H, k).to(dev)
        for pr in (1, 16):
            x0, x1 = k0.to(dev)[None].repeat(pr, 1, 1), k1.to(dev)[None].repeat(pr, 1, 1)
            m = torch.arange(k, dtype=torch.int32, device=dev)[None, :, None].repeat(pr, 1, 2).contiguous()
            counts = torch.full((pr,), k, dtype=torch.int32, device=dev)
            intr = torch.tensor([[kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]]] * 2, dtype=torch.float32, device=dev)[None].repeat(pr, 1, 1)
            res = MatchResult(None, None, None, None, m, None, counts)
            cand = torch.empty((pr, H, 10, 9), dtype=torch.float32, device=dev)
            num = torch.empty((pr, H), dtype=torch.int32, device=dev)

            def solve():
                call("lg_ransac_solve5", m.data_ptr(), counts.data_ptr(), x0.data_ptr(), x1.data_ptr(), intr.data_ptr(), pr, k, k, k,
                     samples.data_ptr(), H, cand.data_ptr(), num.data_ptr(), torch.cuda.current_stream().cuda_stream)

            with torch.no_grad():
                ours = lambda: er.verify(res, x0, x1, intr)  # noqa: E731
                fund = lambda: fr.verify(res, x0, x1)        # noqa: E731
                mine = ours()
                torch.cuda.synchronize()
                rec = dict(base, part="verify", model="essential", K=k, P=pr,
                           ours_mask_is_gt=bool((mine.inliers.bool().cpu() == gt[None]).all()),
                           num_front_is_num_inliers=bool((mine.num_front == mine.num_inliers).all()))
                g, gf, gs = graph_of(ours, stream, CALLS), graph_of(fund, stream, CALLS), graph_of(solve, stream, CALLS)
                t_ours, t_fund, t_solve = [], [], []
                for _ in range(args.repeats):
                    t_ours.append(time_graph(g, stream, CALLS))
                    t_fund.append(time_graph(gf, stream, CALLS))
                    t_solve.append(time_graph(gs, stream, CALLS))
                rec.update(verify_us=spread(t_ours), fundamental_us=spread(t_fund), solve5_us=spread(t_solve),
                           verify_eager_us=round(time_eager(ours, 50), 2), candidates_per_hypothesis=round(float(num.float().mean()), 2),
                           essential_over_fundamental_median=round(statistics.median(t_ours) / statistics.median(t_fund), 3),
                           solve5_share_of_verify=round(statistics.median(t_solve) / statistics.median(t_ours), 3))
            emit(rec)
            del g, gf, gs


def polish_part(args, dev, stream, base, emit):
    n = args.polish
    plain, fine = EssentialRansac(THR, H, R, SEED), EssentialRansac(THR, H, R, SEED, polish=n)
    hook, hook1 = PosePolish(THR, n), PosePolish(THR, 1)
    for k in (256, 1024, 2048):
        k0, k1, gt, _, kk, _, _ = calibrated_scene(k, k, 0.25, 1.0)
        for pr in (1, 16):
            x0, x1 = k0.to(dev)[None].repeat(pr, 1, 1), k1.to(dev)[None].repeat(pr, 1, 1)
            m = torch.arange(k, dtype=torch.int32, device=dev)[None, :, None].repeat(pr, 1, 2).contiguous()
            counts = torch.full((pr,), k, dtype=torch.int32, device=dev)
            intr = torch.tensor([[kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]]] * 2, dtype=torch.float32, device=dev)[None].repeat(pr, 1, 1)
            res = MatchResult(None, None, None, None, m, None, counts)
            with torch.no_grad():
                a = lambda: plain.verify(res, x0, x1, intr)  # noqa: E731
                b = lambda: fine.verify(res, x0, x1, intr)   # noqa: E731
                pose = a()
                c = lambda: hook.refine(res, x0, x1, intr, pose)    # noqa: E731
                d = lambda: hook1.refine(res, x0, x1, intr, pose)   # noqa: E731
                out = c()
                torch.cuda.synchronize()
                cost = out.cost.cpu()
                rec = dict(base, part="polish", model="essential", K=k, P=pr, polish=n, noise_px=1.0, kept=int(out.kept.sum()),
                           inliers=[int(pose.num_inliers[0]), int(out.num_inliers[0])],
                           cost_px2=[round(float(cost[0, 0]), 3), round(float(cost[0, 1]), 3)])
                graphs = [graph_of(f, stream, CALLS) for f in (a, b, c, d)]
                times = [[], [], [], []]
                for _ in range(args.repeats):
                    for g, t in zip(graphs, times):
                        t.append(time_graph(g, stream, CALLS))
                med = [statistics.median(t) for t in times]
                rec.update(verify_us=spread(times[0]), verify_polish_us=spread(times[1]), hook_us=spread(times[2]),
                           hook_one_round_us=spread(times[3]), added_us=round(med[1] - med[0], 2),
                           per_round_us=round((med[2] - med[3]) / max(n - 1, 1), 2))
            emit(rec)
            del graphs


def absolute_part(args, dev, stream, base, emit):
    """AbsolutePoseRansac.localize on absolute_scene's correspondences: the whole call, the call without refits, the
    P3P solve alone (lg_ransac_solve3 on the call's own samples) and lg_link_landmarks on a full pair."""
    from lightglue_amd import AbsolutePoseRansac, absolute_scene, link_landmarks, ransac_samples3

    full, bare = AbsolutePoseRansac(THR, H, R, SEED), AbsolutePoseRansac(THR, H, 0, SEED)
    for k in (256, 1024, 2048):
        pts, kp, gt, kk, _, _ = absolute_scene(k, k, 0.25, 0.25)
        samples = ransac_samples3(SEED, H, k).to(dev)
        for pr in (1, 16):
            x, px = pts.to(dev)[None].repeat(pr, 1, 1).contiguous(), kp.to(dev)[None].repeat(pr, 1, 1).contiguous()
            counts = torch.full((pr,), k, dtype=torch.int32, device=dev)
            intr = torch.tensor([kk[0, 0], kk[1, 1], kk[0, 2], kk[1, 2]], dtype=torch.float32, device=dev)[None].repeat(pr, 1).contiguous()
            cand = torch.empty((pr, H, 4, 12), dtype=torch.float32, device=dev)
            num = torch.empty((pr, H), dtype=torch.int32, device=dev)
            m = torch.arange(k, dtype=torch.int32, device=dev)[None, :, None].repeat(pr, 1, 2).contiguous()
            res = MatchResult(None, None, None, None, m, None, counts)
            ok = torch.ones((pr, k), dtype=torch.uint8, device=dev)

            def solve():
                call("lg_ransac_solve3", x.data_ptr(), px.data_ptr(), counts.data_ptr(), intr.data_ptr(), pr, k, samples.data_ptr(), H,
                     cand.data_ptr(), num.data_ptr(), torch.cuda.current_stream().cuda_stream)

            with torch.no_grad():
                ours = lambda: full.localize(x, px, counts, intr)                       # noqa: E731
                norefit = lambda: bare.localize(x, px, counts, intr)                    # noqa: E731
                link = lambda: link_landmarks(res, x, ok, res, px, side_a=1, num_shared=k)  # noqa: E731
                mine, marks = ours(), link()
                torch.cuda.synchronize()
                rec = dict(base, part="localize", model="absolute", K=k, P=pr,
                           ours_mask_is_gt=bool((mine.inliers.bool().cpu() == gt[None]).all()), linked=int(marks.counts[0]))
                graphs = [graph_of(f, stream, CALLS) for f in (ours, norefit, solve, link)]
                times = [[], [], [], []]
                for _ in range(args.repeats):
                    for g, t in zip(graphs, times):
                        t.append(time_graph(g, stream, CALLS))
                med = [statistics.median(t) for t in times]
                rec.update(localize_us=spread(times[0]), localize_no_refits_us=spread(times[1]), solve3_us=spread(times[2]),
                           link_us=spread(times[3]), refits_add_us=round(med[0] - med[1], 2),
                           localize_eager_us=round(time_eager(ours, 50), 2), candidates_per_hypothesis=round(float(num.float().mean()), 2))
            emit(rec)
            del graphs


if __name__ == "__main__":
    main()
