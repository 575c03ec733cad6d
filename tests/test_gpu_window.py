"""The sequence window on the MI355X (csrc/lightglue_window.hip) against the contract in lightglue_amd/geometry_contract.py.
The scenes, their preconditions and the figures behind the bounds are in window_scenes.py and test_window.py (CPU).

Tracks and landmarks are integers and copies: bitwise. The points' decisions (seen, ok, counts) are the reference's exactly:
test_window.py asserts that no decision lies near its threshold. The points themselves: the arithmetic is fp64 on fp32
inputs, so what is left is the fp32 rounding of the output, 2^-23 max |X|, plus the order of a track's sums, which the
float64 contract moves by at most ORDER = 3.2e-14 between two orders (measured on the CPU), times the project's factor 4:
POINT_BOUND. Against scipy's converged minimiser the fixed-round contract itself is off by CONVERGED = 3.56e-6 (its worst
entry over the cases, measured on the CPU), so the GPU may be off by four times that. The tests print their figures before
they assert."""
import numpy as np
import pytest
import torch

import window_scenes as ws
from gpu_common import GuardedOut, capture_on_side_stream, equal_results, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "the gpu tests need the MI355X"
    return torch.device("cuda:0")


def _outs(dev, specs):
    return [GuardedOut(s, d, dev, fill=torch.full(s, 77, dtype=d)) for s, d in specs]


def tracks_raw(dev, matches, counts, mask, kp_counts, lmax):
    """lg_window_tracks through raw pointers into guarded outputs -> (track_kp, kept, found) on the host."""
    from lightglue_amd._host import call

    m, c, k, n = (x.contiguous().to(dev) for x in (matches, counts, mask, kp_counts))
    bw, views = n.shape
    outs = _outs(dev, (((bw, views, lmax), torch.int32), ((bw,), torch.int32), ((bw,), torch.int32)))
    call("lg_window_tracks", m.data_ptr(), c.data_ptr(), k.data_ptr(), n.data_ptr(), bw, views, m.shape[2], lmax, *(o.ptr for o in outs),
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.check(w) for o, w in zip(outs, ("track_kp", "kept", "found"))]


def points_raw(dev, track_kp, kept, kpts, intr, r, t, posed):
    """lg_window_points the same way -> (obs, seen, counts, points, ok, seen_all) on the host."""
    from lightglue_amd._host import call

    args = [x.contiguous().to(dev) for x in (track_kp, kept, kpts, intr, r, t, posed)]
    bw, views, lmax = track_kp.shape
    outs = _outs(dev, (((bw, views, lmax, 2), torch.float32), ((bw, views, lmax), torch.uint8), ((bw,), torch.int32),
                       ((bw, lmax, 3), torch.float32), ((bw, lmax), torch.uint8), ((bw, views, lmax), torch.uint8)))
    call("lg_window_points", *(x.data_ptr() for x in args), bw, views, lmax, kpts.shape[2], ws.THRESHOLD, *(o.ptr for o in outs),
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return [o.check(w) for o, w in zip(outs, ("obs", "seen", "counts", "points", "ok", "seen_all"))]


@pytest.mark.parametrize("views,k,lmax", ws.TRACK_CASES)
def test_tracks_bitwise(dev, views, k, lmax):
    s = ws.scene(views, k)
    tk, kept, found = ws.tracks(views, k, lmax)
    got = tracks_raw(dev, s.matches[None], s.counts[None], s.mask[None], s.kp_counts[None], lmax)
    print(f"V {views} k {k} lmax {lmax}: kept {int(got[1][0])} found {int(got[2][0])}")
    assert int(got[1][0]) == kept and int(got[2][0]) == found
    assert same_bits(got[0][0], torch.from_numpy(tk))


@pytest.mark.parametrize("views,k", list(ws.POINT_CASES))
def test_points_against_the_contract(dev, views, k):
    s, ref, lmax = ws.scene(views, k), ws.points(views, k), ws.POINT_CASES[(views, k)][0]
    tk, kept, _ = ws.tracks(views, k, lmax)
    got = points_raw(dev, torch.from_numpy(tk)[None], torch.tensor([kept], dtype=torch.int32), s.kpts[None],
                     *(x[None] for x in ws.cameras(s)), ws.posed_of(views, k)[None])
    ok = ref[4].astype(bool)
    diff = float(np.abs(got[3][0].numpy().astype(np.float64) - ref[3]).max())
    bound = 2.0 ** -23 * float(np.abs(ref[3]).max()) + 4.0 * ws.ORDER
    conv = max(float(np.abs(got[3][0, l].numpy() - x).max()) for l, x in ws.converged(views, k).items())
    print(f"V {views} k {k}: {int(ok.sum())} of {kept} ok, points {diff:.3e} (bound {bound:.3e}), converged {conv:.3e} (bound {4 * ws.CONVERGED:.3e})")
    assert same_bits(got[0][0], torch.from_numpy(ref[0])) and int(got[2][0]) == ref[2]
    assert same_bits(got[1][0], torch.from_numpy(ref[1])) and same_bits(got[4][0], torch.from_numpy(ref[4]))
    assert same_bits(got[5][0], torch.from_numpy(ref[5])) and not got[3][0][~torch.from_numpy(ok)].any()
    assert diff <= bound and conv <= 4.0 * ws.CONVERGED


def test_ragged_dirty_batch(dev):
    """Counts 0, one row and full, a pose that is not finite, a focal length of 0, a view with no keypoints: the decisions
    are the reference's, and a window alone, the batch reversed and a second call agree bitwise."""
    from lightglue_amd import window_points_reference, window_tracks_reference

    wins, lmax = ws.dirty_windows(), 64
    stack = lambda ws_: [torch.stack([w[i] for w in ws_]) for i in range(9)]  # noqa: E731

    def run(ws_):
        b = stack(ws_)
        tk = tracks_raw(dev, b[0], b[1], b[2], b[3], lmax)
        return tk + points_raw(dev, tk[0], tk[1], *b[4:])

    got = run(wins)
    for i, w in enumerate(wins):
        tk, kept, found = window_tracks_reference(w[0], w[1], w[2], w[3], lmax)
        ref = window_points_reference(tk, kept, *w[4:], ws.THRESHOLD)
        print(f"window {i}: kept {int(got[1][i])} found {int(got[2][i])} ok {int(got[7][i].sum())} (reference {kept}, {found}, {int(ref[4].sum())})")
        assert same_bits(got[0][i], torch.from_numpy(tk)) and (int(got[1][i]), int(got[2][i]), int(got[5][i])) == (kept, found, kept), i
        assert same_bits(got[4][i], torch.from_numpy(ref[1])) and same_bits(got[7][i], torch.from_numpy(ref[4])), i
        assert same_bits(got[8][i], torch.from_numpy(ref[5])), i
    assert int(got[1][1]) == 0 and int(got[1][2]) <= 1 and int(got[7][0].sum()) > 0
    again, flipped, alone = run(wins), run(wins[::-1]), run([wins[3]])
    for a, b, c, d in zip(got, again, flipped, alone):
        assert same_bits(a, b) and same_bits(a, c.flip(0)) and same_bits(a[3:4], d)


@pytest.mark.parametrize("view", (0, 7, 3))
def test_landmarks_and_public_interface(dev, view):
    """SequenceWindow.build equals the raw calls, and window_landmarks a gather in numpy: the first view, the last, the
    one that is not posed."""
    from lightglue_amd import SequenceWindow, window_landmarks
    from lightglue_amd.matches import MatchResult

    views, k = 8, 257
    s, lmax = ws.scene(views, k), ws.POINT_CASES[(views, k)][0]
    intr, r, t = (x[None].to(dev) for x in ws.cameras(s))
    res = [MatchResult(None, None, None, None, s.matches[v][None].to(dev), None, s.counts[v:v + 1].to(dev)) for v in range(views - 1)]
    kpts = [s.kpts[v][None].to(dev) for v in range(views)]
    w = SequenceWindow(ws.THRESHOLD).build(res, [s.mask[v][None].to(dev) for v in range(views - 1)], kpts, intr, r, t,
                                           ws.posed_of(views, k)[None].to(dev), lmax=lmax)
    marks = window_landmarks(w, kpts[view], view)
    torch.cuda.synchronize()
    ref = ws.points(views, k)
    tk = ws.tracks(views, k, lmax)[0]
    assert same_bits(w.track_kp[0].cpu(), torch.from_numpy(tk)) and same_bits(w.ok[0].cpu(), torch.from_numpy(ref[4]))
    assert same_bits(w.seen[0].cpu(), torch.from_numpy(ref[1])) and int(w.counts[0]) == ref[2]
    rows = np.nonzero((ref[4] != 0) & (tk[view] >= 0))[0]
    n = len(rows)
    print(f"view {view}: {n} landmarks of {int(ref[4].sum())} ok tracks")
    assert n > 0 and int(marks.counts[0]) == n
    assert np.array_equal(marks.rows[0, :n].cpu().numpy(), rows) and (marks.rows[0, n:] == -1).all()
    assert same_bits(marks.points[0, :n].cpu(), w.points[0].cpu()[rows]) and not marks.points[0, n:].any()
    assert same_bits(marks.image[0, :n].cpu(), s.kpts[view][tk[view][rows]]) and not marks.image[0, n:].any()


def test_sequence_is_one_captured_piece(dev):
    """Five views of sequence_scene: views 0 to 2 by the existing chain (EssentialRansac(polish).verify -> triangulate ->
    link_landmarks -> localize_landmarks -> inliers_on_matches); views 3 and 4 each by build over the views posed so far ->
    window_landmarks -> localize_landmarks; then build over all five -> BundleAdjust.refine. The replay equals the eager run
    bitwise, views 3 and 4 get valid poses, and view 4's error against the truth after the refinement is at most
    SEQUENCE_RATIO of its error before it on the same run: the float64 chain's ratio half way to 1 (test_window.py)."""
    import absolute_scenes as ab
    from lightglue_amd import (AbsolutePoseRansac, BundleAdjust, EssentialRansac, SequenceWindow, inliers_on_matches, link_landmarks,
                               triangulate, window_landmarks)
    from lightglue_amd.matches import MatchResult

    s, k, views = ws.sequence(), ws.SEQ_K, ws.SEQ_VIEWS
    one = ab.intrinsics_of(s.K).to(dev)
    pair_intr, cam_intr = one[None, None].repeat(1, 2, 1).contiguous(), one[None].contiguous()
    res = [MatchResult(None, None, None, None, s.matches[v][None].contiguous().to(dev), None, s.counts[v:v + 1].to(dev)) for v in range(views - 1)]
    kpts = [s.kpts[v][None].contiguous().to(dev) for v in range(views)]
    ones = torch.ones((1, k), dtype=torch.uint8, device=dev)
    eye, zero = torch.eye(3, device=dev)[None], torch.zeros((1, 3), device=dev)
    ea = EssentialRansac(ab.THRESHOLD, ab.HYPOTHESES, ab.REFITS, ab.SEED, polish=ab.CHAIN_POLISH)
    er, ba, sw = AbsolutePoseRansac(ab.THRESHOLD, ab.HYPOTHESES, ab.REFITS, ab.SEED), BundleAdjust(ws.SEQ_ITERATIONS), SequenceWindow(ws.THRESHOLD)

    posed_for = {(n, p): torch.tensor([[1] * p + [0] * (n - p)], dtype=torch.uint8, device=dev) for n, p in ((4, 3), (5, 4), (5, 5))}

    def build(n, rs, ts, masks):
        posed = posed_for[(n, len(rs))]
        r = torch.stack(rs + [eye] * (n - len(rs)), 1)
        t = torch.stack(ts + [zero] * (n - len(ts)), 1)
        return sw.build(res[:n - 1], masks[:n - 1], kpts[:n], one[None, None].repeat(1, n, 1).contiguous(), r, t, posed, lmax=ws.SEQ_LMAX)

    def chain():
        pose = ea.verify(res[0], kpts[0], kpts[1], pair_intr)
        points, ok = triangulate(res[0], kpts[0], kpts[1], pair_intr, pose)
        marks = link_landmarks(res[0], points, ok, res[1], kpts[2], side_a=1, num_shared=k)
        got = er.localize_landmarks(marks, cam_intr)
        masks = [pose.inliers, inliers_on_matches(marks, got, k), ones, ones]
        rs, ts, poses = [eye, pose.R, got.R], [zero, pose.t, got.t], []
        for new in (3, 4):
            w = build(new + 1, rs, ts, masks)
            poses.append(er.localize_landmarks(window_landmarks(w, kpts[new], new), cam_intr))
            rs.append(poses[-1].R)
            ts.append(poses[-1].t)
        w = build(views, rs, ts, masks)
        return poses[0], poses[1], w, ba.refine(w.obs, w.seen, w.counts, one[None, None].repeat(1, views, 1).contiguous(), w.R, w.t, w.points)

    with torch.no_grad():
        eager = chain()
    torch.cuda.synchronize()
    graph, captured = capture_on_side_stream(chain)
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b, what in zip(eager, captured, ("view 3", "view 4", "the window", "the bundle adjustment")):
            equal_results(a, b, what)
    p3, p4, w, fine = eager
    before = ab.pose_errors(p4.R[0].cpu(), p4.t[0].cpu(), s.R[4], s.t[4])
    after = ab.pose_errors(fine.R[0, 4].cpu(), fine.t[0, 4].cpu(), s.R[4], s.t[4])
    e3 = ab.pose_errors(p3.R[0].cpu(), p3.t[0].cpu(), s.R[3], s.t[3])
    print(f"the sequence: view 3 {e3[0]:.3e} deg, {e3[1]:.3e} ({int(p3.num_inliers[0])} inliers); view 4 {before[0]:.3e} deg, {before[1]:.3e} "
          f"({int(p4.num_inliers[0])} inliers) -> {after[0]:.3e} deg, {after[1]:.3e} (ratios {after[0] / before[0]:.3f}, {after[1] / before[1]:.3f}); "
          f"{int(w.ok[0].sum())} of {int(w.counts[0])} tracks ok, {int(fine.num_obs[0])} observations, cost {fine.cost[0].tolist()}")
    assert int(p3.valid[0]) == 1 and int(p4.valid[0]) == 1 and int(fine.kept[0]) == 1
    assert after[0] <= ws.SEQUENCE_RATIO[0] * before[0] and after[1] <= ws.SEQUENCE_RATIO[1] * before[1]
