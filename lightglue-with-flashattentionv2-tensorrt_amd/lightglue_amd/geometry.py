"""Geometric verification: a fundamental matrix per image pair by RANSAC over the matcher's matches, on gfx950
kernels (include/lightglue_glue.h, "geometric verification"; csrc/lightglue_geometry.hip).

The reference's demo does not stop at matches: after LightGlueTRT::PostProcess it runs
``cv::findFundamentalMat(points0, points1, cv::FM_RANSAC, 3, 0.99, inliers)`` on the host and draws only the
inliers (demo/demo_mono.cpp:326-366). ``FundamentalRansac.verify`` is that step for the P pairs of a
``MatchResult`` in two launches, with nothing read back: ``verify_source_images`` is ``match_source_images``
followed by it, still one capturable piece.

``HomographyRansac.verify`` is the same scheme for the homography x1 ~ H x0 (planar scenes and rotating cameras,
where the epipolar constraint is degenerate): ``cv::findHomography(pts0, pts1, cv::RANSAC, 3)`` without its final
Levenberg-Marquardt polish.

``EssentialRansac.verify`` is the calibrated case (csrc/lightglue_essential.hip): five-point RANSAC for the essential
matrix and the relative pose (R, t) from it, given each image's (fx, fy, cx, cy).

``PosePolish.refine`` (csrc/lightglue_polish.hip; ``EssentialRansac(polish=N)`` appends it) minimises the squared
Sampson distance in pixels over the pose's inliers by N rounds of Levenberg-Marquardt on the 5 parameters of (R, t),
recomputes the mask and keeps the result where it loses no inlier; ``triangulate`` writes every inlier's 3D point.

``AbsolutePoseRansac.localize`` (csrc/lightglue_absolute.hip) is the absolute pose: P3P RANSAC for the pose of a camera
against 3D points, what cv::solvePnPRansac does on the host; ``link_landmarks`` carries the points ``triangulate`` wrote
for one pair onto the match rows of the next pair that shares an image with it, and ``inliers_on_matches`` brings the
result's mask back onto those rows: EssentialRansac(polish=N).verify -> triangulate -> link_landmarks ->
localize_landmarks gives the next frame a pose in the first pair's frame at the first pair's scale.

This module is the kernel side only. What each call computes is pinned in float64 in geometry_contract.py, and the
synthetic pairs of the tests are in geometry_scenes.py; both are re-exported here.
"""
from __future__ import annotations

import torch

from . import _lib
from ._host import call, carve, require_gpu, stream_of
from .geometry_contract import (  # noqa: F401  (the public names this module had before the contract was split off)
    _M32, AbsolutePoseResult, Landmarks, MAX_HYPOTHESES, MAX_REFITS, MIN_INLIERS, MIN_INLIERS_E, MIN_INLIERS_H, MIN_POLISH_ROWS, PIVOT_EPS, GeometryResult,
    HomographyResult, PolishResult, PoseResult, Solve4, Solve5, Solve7, _check_params, _rows, camera_coordinates, direction_angle_deg,
    elimination_pivots, epipolar_error, essential_constraints, essential_reference, essential_refit, essential_residuals,
    essential_to_fundamental, fundamental_refit, gather_correspondences, homography_reference, homography_refit,
    polish_pose_reference, polish_reference, pose_candidates, pose_from_essential_reference, ransac_reference, ransac_samples,
    ransac_samples3, ransac_samples5, reprojection_error, rotation_angle_deg, sampson_error, solve4_reference, solve5_reference, solve7_reference, transfer_error,
    triangulate_reference, absolute_pose_reference, absolute_refit_reference, link_landmarks_reference, solve3_reference, Solve3)
from .geometry_scenes import (ThreeViews, absolute_scene, calibrated_planar_scene, calibrated_scene, planar_scene,  # noqa: F401
                              three_view_scene, two_view_scene)
from .image import ImageInput, match_source_images
from .matches import MatchResult

_STAGE = "the geometric verification"
MAX_POINTS = 2048       # kmax: the plugin's N limit
MAX_POLISH = 16         # rounds of the pose polish

# A result field's shape after [P] (None: Kmax) and dtype on the device; every field not named here is [P] int32.
_FIELDS = {"F": ((3, 3), torch.float32), "H": ((3, 3), torch.float32), "E": ((3, 3), torch.float32),
           "R": ((3, 3), torch.float32), "t": ((3,), torch.float32), "cost": ((2,), torch.float32),
           "inliers": ((None,), torch.uint8), "points": ((None, 3), torch.float32), "image": ((None, 2), torch.float32),
           "rows": ((None,), torch.int32)}


def _empty(result, pr: int, kmax: int, dev):
    """The result tuple's tensors for P pairs, uninitialised on dev."""
    def one(name):
        shape, dtype = _FIELDS.get(name, ((), torch.int32))
        return torch.empty((pr,) + tuple(kmax if s is None else s for s in shape), dtype=dtype, device=dev)

    return result(*(one(name) for name in result._fields))


def _like_matches(name: str, t: torch.Tensor, shape, matches: torch.Tensor) -> None:
    if tuple(t.shape) != shape:
        raise ValueError(f"{name}: expected {list(shape)}, got {tuple(t.shape)}")
    if t.device != matches.device:
        raise ValueError(f"{name}: on {t.device}, the matches on {matches.device}")


def _intrinsics(intrinsics: torch.Tensor, pr: int, matches: torch.Tensor) -> torch.Tensor:
    """The check of intrinsics [P, 2, 4] fp32 next to the matches -> contiguous."""
    require_gpu("intrinsics", intrinsics, _STAGE, (torch.float32,), 3)
    _like_matches("intrinsics", intrinsics, (pr, 2, 4), matches)
    return intrinsics.contiguous()


# ---- the kernels --------------------------------------------------------------------------------------------------
class _Ransac:
    """What the estimators share: the parameters, the checks of verify's inputs and the call. _ENTRY: the C entry
    point; _WORKSPACE: the entry point of its workspace size; _RESULT: the NamedTuple of its outputs."""
    _ENTRY, _WORKSPACE, _RESULT = "", "lg_ransac_workspace", None

    def __init__(self, threshold: float = 3.0, hypotheses: int = 512, refits: int = 2, seed: int = 888) -> None:
        _check_params(threshold, hypotheses, refits)
        self.threshold, self.hypotheses, self.refits = float(threshold), int(hypotheses), int(refits)
        self.seed = int(seed) & _M32

    @staticmethod
    def _inputs(result: MatchResult, kpts0: torch.Tensor, kpts1: torch.Tensor):
        """verify's checks of its inputs -> (matches, counts, kpts0, kpts1) contiguous, P, Kmax."""
        matches, counts = result.matches, result.counts
        require_gpu("matches", matches, _STAGE, (torch.int32,), 3)
        require_gpu("counts", counts, _STAGE, (torch.int32,), 1)
        require_gpu("kpts0", kpts0, _STAGE, (torch.float32,), 3)
        require_gpu("kpts1", kpts1, _STAGE, (torch.float32,), 3)
        pr, kmax = int(matches.shape[0]), int(matches.shape[1])
        if matches.shape[2] != 2 or not 1 <= kmax <= MAX_POINTS:
            raise ValueError(f"matches: expected [P, Kmax, 2] with 1 <= Kmax <= {MAX_POINTS}, got {tuple(matches.shape)}")
        if tuple(counts.shape) != (pr,):
            raise ValueError(f"counts: expected [{pr}], got {tuple(counts.shape)}")
        for name, t in (("kpts0", kpts0), ("kpts1", kpts1)):
            if t.shape[0] != pr or t.shape[1] < 1 or t.shape[2] != 2:
                raise ValueError(f"{name}: expected [{pr}, K, 2] with K >= 1, got {tuple(t.shape)}")
            if t.device != matches.device:
                raise ValueError(f"{name}: on {t.device}, the matches on {matches.device}")
        return tuple(t.contiguous() for t in (matches, counts, kpts0, kpts1)), pr, kmax

    def _run(self, inputs, pr: int, kmax: int, *extra: torch.Tensor):
        """The call on _inputs' outputs; extra: the tensors whose pointers follow kpts1's (the intrinsics)."""
        matches, _, kpts0, kpts1 = inputs
        out = _empty(self._RESULT, pr, kmax, matches.device)
        if pr == 0:
            return out
        stream = stream_of(matches)
        nbytes = int(getattr(_lib.load(), self._WORKSPACE)(pr, kmax, self.hypotheses))
        ws, = carve(matches.device, stream, [nbytes])
        call(self._ENTRY, *(t.data_ptr() for t in inputs + extra), pr, kmax, int(kpts0.shape[1]), int(kpts1.shape[1]),
             self.threshold, self.hypotheses, self.refits, self._seed32(), ws.data_ptr(), nbytes, *(t.data_ptr() for t in out),
             stream)
        return out

    def verify(self, result: MatchResult, kpts0: torch.Tensor, kpts1: torch.Tensor):
        """result.matches [P, Kmax, 2] / result.counts [P] (int32) index kpts0 [P, K0, 2] and kpts1 [P, K1, 2]
        (fp32, (x, y) in pixels; ImageInput.keypoints' output is the intended one) -> the estimator's result. Two
        launches on the current stream, nothing read back; counts and indices are clamped, never trusted."""
        return self._run(*self._inputs(result, kpts0, kpts1))

    def _seed32(self) -> int:
        return self.seed - (1 << 32) if self.seed >= 1 << 31 else self.seed  # the same 32 bits as int32


class FundamentalRansac(_Ransac):
    """RANSAC for the fundamental matrix of every pair of a MatchResult. threshold: the inlier bound in pixels
    (the demo's 3); hypotheses: their fixed number per pair (no early termination: the launches do not depend
    on the data); refits: least-squares rounds over the inliers; seed: of the samples. verify -> GeometryResult."""
    _ENTRY, _RESULT = "lg_ransac_fundamental", GeometryResult


class HomographyRansac(_Ransac):
    """RANSAC for the homography x1 ~ H x0 of every pair of a MatchResult (planar scenes, a rotating camera; what
    cv::findHomography(pts0, pts1, cv::RANSAC, 3) does on the host, without its final Levenberg-Marquardt polish: on
    the planar scenes a float64 prototype of it lowered the transfer cost by 3e-6 to 8e-5 relative).
    The parameters are FundamentalRansac's; verify -> HomographyResult. A pair is valid from 4 inliers on, and a
    4-inlier winner is only its own sample: threshold num_inliers before trusting H."""
    _ENTRY, _RESULT = "lg_ransac_homography", HomographyResult


class EssentialRansac(_Ransac):
    """Five-point RANSAC for the essential matrix, and the relative pose from it, of every pair of a MatchResult
    whose cameras are known (what cv::findEssentialMat and cv::recoverPose do on the host). The parameters are
    FundamentalRansac's; the threshold is in pixels; polish: 0 (the RANSAC pose as it is: the last kept 8-point
    refit, or the five-point winner), or the rounds in [1, 16] of PosePolish's Levenberg-Marquardt over the inliers,
    appended as a third launch. verify -> PoseResult. A pair is valid from 5 inliers on, and a 5-inlier winner is
    only its own sample: threshold num_inliers before trusting the pose. On a planar scene two poses fit; which of
    them comes out is not specified."""
    _ENTRY, _WORKSPACE, _RESULT = "lg_ransac_essential", "lg_ransac_essential_workspace", PoseResult

    def __init__(self, threshold: float = 3.0, hypotheses: int = 512, refits: int = 2, seed: int = 888, polish: int = 0) -> None:
        super().__init__(threshold, hypotheses, refits, seed)
        if not 0 <= int(polish) <= MAX_POLISH:
            raise ValueError(f"polish must be in [0, {MAX_POLISH}] rounds, got {polish}")
        self.polish = int(polish)

    def verify(self, result: MatchResult, kpts0: torch.Tensor, kpts1: torch.Tensor, intrinsics: torch.Tensor) -> PoseResult:
        """_Ransac.verify's inputs and intrinsics [P, 2, 4] fp32 ((fx, fy, cx, cy) of image 0 then image 1, in the
        keypoints' pixel frame) -> PoseResult. Two launches on the current stream (three with polish > 0: the result
        is then the polished one, valid and best the RANSAC's), nothing read back; a pair with a non-finite intrinsic
        or a focal length <= 0 is invalid."""
        inputs, pr, kmax = self._inputs(result, kpts0, kpts1)
        intrinsics = _intrinsics(intrinsics, pr, inputs[0])
        out = self._run(inputs, pr, kmax, intrinsics)
        if not self.polish or pr == 0:
            return out
        fine = _polish_call(*inputs, intrinsics, out, self.threshold, self.polish, stream_of(inputs[0]))
        return PoseResult(fine.E, fine.R, fine.t, fine.inliers, fine.num_inliers, fine.num_front, out.valid, out.best)


def _calibrated_inputs(result: MatchResult, kpts0, kpts1, intrinsics, pose):
    """The checks PosePolish.refine and triangulate share -> (matches, counts, kpts0, kpts1, intrinsics, R, t, inliers)
    contiguous, P, Kmax."""
    inputs, pr, kmax = _Ransac._inputs(result, kpts0, kpts1)
    intrinsics = _intrinsics(intrinsics, pr, inputs[0])
    require_gpu("R", pose.R, _STAGE, (torch.float32,), 3)
    require_gpu("t", pose.t, _STAGE, (torch.float32,), 2)
    require_gpu("inliers", pose.inliers, _STAGE, (torch.uint8,), 2)
    for name, t, shape in (("R", pose.R, (pr, 3, 3)), ("t", pose.t, (pr, 3)), ("inliers", pose.inliers, (pr, kmax))):
        _like_matches(name, t, shape, inputs[0])
    return inputs + (intrinsics,) + tuple(t.contiguous() for t in (pose.R, pose.t, pose.inliers)), pr, kmax


def _polish_call(matches, counts, kpts0, kpts1, intrinsics, pose, threshold: float, iterations: int, stream) -> PolishResult:
    pr, kmax = int(matches.shape[0]), int(matches.shape[1])
    out = _empty(PolishResult, pr, kmax, matches.device)
    if pr:
        call("lg_pose_polish", matches.data_ptr(), counts.data_ptr(), kpts0.data_ptr(), kpts1.data_ptr(), intrinsics.data_ptr(),
             pr, kmax, int(kpts0.shape[1]), int(kpts1.shape[1]), pose.R.data_ptr(), pose.t.data_ptr(), pose.inliers.data_ptr(),
             pose.valid.data_ptr(), threshold, iterations, *(t.data_ptr() for t in out), stream)
    return out


class PosePolish:
    """The non-linear polish of a calibrated pose (csrc/lightglue_polish.hip; what cv::findEssentialMat's callers add
    by hand): `iterations` rounds in [1, 16] of Levenberg-Marquardt on the 5 parameters of (R, t) over the squared
    Sampson distance in pixels of the pose's inliers, then the mask recomputed at `threshold` pixels over all the
    pair's correspondences; the polished pose is kept where it has at least as many inliers as the given one.
    refine -> PolishResult. EssentialRansac(polish=N) appends it to the RANSAC."""

    def __init__(self, threshold: float = 3.0, iterations: int = 10) -> None:
        if not 0.0 < float(threshold) <= 1e6:
            raise ValueError(f"threshold must be in (0, 1e6] pixels, got {threshold}")
        if not 1 <= int(iterations) <= MAX_POLISH:
            raise ValueError(f"iterations must be in [1, {MAX_POLISH}], got {iterations}")
        self.threshold, self.iterations = float(threshold), int(iterations)

    def refine(self, result: MatchResult, kpts0: torch.Tensor, kpts1: torch.Tensor, intrinsics: torch.Tensor, pose) -> PolishResult:
        """EssentialRansac.verify's inputs and its PoseResult (or any tuple with R [P, 3, 3], t [P, 3] fp32, inliers
        [P, Kmax] uint8 and valid [P] int32 on the device) -> PolishResult. One launch on the current stream, nothing
        read back."""
        (matches, counts, kpts0, kpts1, intrinsics, r, t, inliers), pr, _ = _calibrated_inputs(result, kpts0, kpts1, intrinsics, pose)
        require_gpu("valid", pose.valid, _STAGE, (torch.int32,), 1)
        if tuple(pose.valid.shape) != (pr,) or pose.valid.device != matches.device:
            raise ValueError(f"valid: expected [{pr}] on {matches.device}, got {tuple(pose.valid.shape)} on {pose.valid.device}")
        given = PoseResult(None, r, t, inliers, None, None, pose.valid.contiguous(), None)
        return _polish_call(matches, counts, kpts0, kpts1, intrinsics, given, self.threshold, self.iterations, stream_of(matches))


def triangulate(result: MatchResult, kpts0: torch.Tensor, kpts1: torch.Tensor, intrinsics: torch.Tensor, pose):
    """The 3D point of every inlier of a pose (a PoseResult or a PolishResult: R, t, inliers): (points [P, Kmax, 3] fp32
    in camera 0's frame at the scale |t| = 1, ok [P, Kmax] uint8), by the midpoint method the cheirality count uses
    (triangulate_reference); ok = 1 where both depths are positive and the point is finite, every other entry zeros.
    One launch on the current stream, nothing read back."""
    (matches, counts, kpts0, kpts1, intrinsics, r, t, inliers), pr, kmax = _calibrated_inputs(result, kpts0, kpts1, intrinsics, pose)
    points = torch.empty((pr, kmax, 3), dtype=torch.float32, device=matches.device)
    ok = torch.empty((pr, kmax), dtype=torch.uint8, device=matches.device)
    if pr:
        call("lg_triangulate", matches.data_ptr(), counts.data_ptr(), kpts0.data_ptr(), kpts1.data_ptr(), intrinsics.data_ptr(), pr,
             kmax, int(kpts0.shape[1]), int(kpts1.shape[1]), r.data_ptr(), t.data_ptr(), inliers.data_ptr(), points.data_ptr(),
             ok.data_ptr(), stream_of(matches))
    return points, ok


# ---- the absolute pose ------------------------------------------------------------------------------------------------
def link_landmarks(result_a: MatchResult, points_a: torch.Tensor, ok_a: torch.Tensor, result_b: MatchResult,
                   kpts_b1: torch.Tensor, *, side_a: int = 1, num_shared: int) -> Landmarks:
    """The 3D points of pair A onto the match rows of pair B, where both pairs share an image: result_a (matches
    [P, Ka, 2], counts [P]) with triangulate's points_a [P, Ka, 3] fp32 and ok_a [P, Ka] uint8; side_a: the column of
    pair A's matches that indexes the shared image (1: the sequence's case, A = (i - 1, i) and B = (i, i + 1));
    result_b, whose column 0 indexes the shared image; kpts_b1 [P, K1, 2] fp32: the new image's keypoints in pixels;
    num_shared in [1, 2048]: the shared image's keypoints -> Landmarks. A row of B is linked iff a row of A with
    ok_a != 0 names its shared keypoint (the lowest such row owns it); the linked rows are compacted in ascending order.
    One launch on the current stream, nothing read back."""
    ma, ca, mb, cb = result_a.matches, result_a.counts, result_b.matches, result_b.counts
    for name, t, dt, nd in (("matches_a", ma, torch.int32, 3), ("counts_a", ca, torch.int32, 1), ("points_a", points_a, torch.float32, 3),
                            ("ok_a", ok_a, torch.uint8, 2), ("matches_b", mb, torch.int32, 3), ("counts_b", cb, torch.int32, 1),
                            ("kpts_b1", kpts_b1, torch.float32, 3)):
        require_gpu(name, t, _STAGE, (dt,), nd)
    if side_a not in (0, 1):
        raise ValueError(f"side_a is 0 or 1, got {side_a}")
    if not 1 <= int(num_shared) <= MAX_POINTS:
        raise ValueError(f"num_shared must be in [1, {MAX_POINTS}], got {num_shared}")
    pr, ka, kb = int(ma.shape[0]), int(ma.shape[1]), int(mb.shape[1])
    if ma.shape[2] != 2 or not 1 <= ka <= MAX_POINTS:
        raise ValueError(f"matches_a: expected [P, Ka, 2] with 1 <= Ka <= {MAX_POINTS}, got {tuple(ma.shape)}")
    if mb.shape[0] != pr or mb.shape[2] != 2 or not 1 <= kb <= MAX_POINTS:
        raise ValueError(f"matches_b: expected [{pr}, Kb, 2] with 1 <= Kb <= {MAX_POINTS}, got {tuple(mb.shape)}")
    if kpts_b1.shape[0] != pr or kpts_b1.shape[1] < 1 or kpts_b1.shape[2] != 2:
        raise ValueError(f"kpts_b1: expected [{pr}, K, 2] with K >= 1, got {tuple(kpts_b1.shape)}")
    for name, t, shape in (("counts_a", ca, (pr,)), ("points_a", points_a, (pr, ka, 3)), ("ok_a", ok_a, (pr, ka)),
                           ("matches_b", mb, (pr, kb, 2)), ("counts_b", cb, (pr,)), ("kpts_b1", kpts_b1, tuple(kpts_b1.shape))):
        _like_matches(name, t, shape, ma)
    ma, ca, points_a, ok_a, mb, cb, kpts_b1 = (t.contiguous() for t in (ma, ca, points_a, ok_a, mb, cb, kpts_b1))
    out = _empty(Landmarks, pr, kb, ma.device)
    if pr:
        call("lg_link_landmarks", ma.data_ptr(), ca.data_ptr(), points_a.data_ptr(), ok_a.data_ptr(), int(side_a), mb.data_ptr(),
             cb.data_ptr(), kpts_b1.data_ptr(), pr, ka, kb, int(num_shared), int(kpts_b1.shape[1]), *(t.data_ptr() for t in out),
             stream_of(ma))
    return out


class AbsolutePoseRansac(_Ransac):
    """P3P RANSAC for the pose of a camera from 2D-3D correspondences (what cv::solvePnPRansac does on the host), with
    Levenberg-Marquardt refits of the reprojection error over the inliers. The parameters are FundamentalRansac's; the
    threshold is the reprojection error in pixels. localize -> AbsolutePoseResult: X_c = R X + t at the scale of the
    points. A pair is valid from 4 inliers on, and a 4-inlier winner is little more than its own sample: threshold
    num_inliers before trusting the pose. Unlike the 8-point refit, P3P is not degenerate on planar points."""
    _ENTRY, _WORKSPACE, _RESULT = "lg_ransac_absolute", "lg_ransac_absolute_workspace", AbsolutePoseResult

    def localize(self, points: torch.Tensor, image: torch.Tensor, counts: torch.Tensor, intrinsics: torch.Tensor) -> AbsolutePoseResult:
        """points [P, Kmax, 3], image [P, Kmax, 2] (pixels) fp32, counts [P] int32 (row k < counts[p] pairs points[p, k]
        with image[p, k]), intrinsics [P, 4] fp32 (fx, fy, cx, cy) -> AbsolutePoseResult. Two launches on the current
        stream, nothing read back; counts are clamped, never trusted; a pair with a non-finite intrinsic or a focal
        length <= 0 is invalid."""
        require_gpu("points", points, _STAGE, (torch.float32,), 3)
        require_gpu("image", image, _STAGE, (torch.float32,), 3)
        require_gpu("counts", counts, _STAGE, (torch.int32,), 1)
        require_gpu("intrinsics", intrinsics, _STAGE, (torch.float32,), 2)
        pr, kmax = int(points.shape[0]), int(points.shape[1])
        if points.shape[2] != 3 or not 1 <= kmax <= MAX_POINTS:
            raise ValueError(f"points: expected [P, Kmax, 3] with 1 <= Kmax <= {MAX_POINTS}, got {tuple(points.shape)}")
        for name, t, shape in (("image", image, (pr, kmax, 2)), ("counts", counts, (pr,)), ("intrinsics", intrinsics, (pr, 4))):
            _like_matches(name, t, shape, points)
        points, image, counts, intrinsics = (t.contiguous() for t in (points, image, counts, intrinsics))
        out = _empty(AbsolutePoseResult, pr, kmax, points.device)
        if pr == 0:
            return out
        stream = stream_of(points)
        nbytes = int(_lib.load().lg_ransac_absolute_workspace(pr, kmax, self.hypotheses))
        ws, = carve(points.device, stream, [nbytes])
        call(self._ENTRY, points.data_ptr(), image.data_ptr(), counts.data_ptr(), intrinsics.data_ptr(), pr, kmax, self.threshold,
             self.hypotheses, self.refits, self._seed32(), ws.data_ptr(), nbytes, *(t.data_ptr() for t in out), stream)
        return out

    def localize_landmarks(self, landmarks: Landmarks, intrinsics: torch.Tensor) -> AbsolutePoseResult:
        """localize on link_landmarks' output; the mask is aligned with the landmarks' rows (inliers_on_matches brings
        it back onto pair B's match rows)."""
        return self.localize(landmarks.points, landmarks.image, landmarks.counts, intrinsics)

    def verify(self, *args, **kwargs):
        raise TypeError("AbsolutePoseRansac has no verify: its inputs are 2D-3D correspondences (localize, localize_landmarks)")


def inliers_on_matches(landmarks: Landmarks, result: AbsolutePoseResult, kmax_b: int) -> torch.Tensor:
    """The absolute pose's mask on the rows of pair B's matches: [P, kmax_b] uint8, 1 where the row was linked and its
    landmark is an inlier of `result`. Framework ops (a masked scatter), nothing read back."""
    pr, kb = landmarks.rows.shape
    if tuple(result.inliers.shape) != (pr, kb) or int(kmax_b) < kb:
        raise ValueError(f"inliers_on_matches: a mask of {[pr, kb]} and kmax_b >= {kb}, got {tuple(result.inliers.shape)} and {kmax_b}")
    live = landmarks.rows >= 0
    # the rows past the count go to a column of their own (every write there is a 0), which is then cut off
    out = torch.zeros((pr, int(kmax_b) + 1), dtype=torch.uint8, device=landmarks.rows.device)
    index = torch.where(live, landmarks.rows, torch.full_like(landmarks.rows, int(kmax_b))).long()
    out.scatter_(1, index, (result.inliers != 0).to(torch.uint8) * live.to(torch.uint8))
    return out[:, :int(kmax_b)].contiguous()


def verify_source_images(image_input: ImageInput, encoder, frontend, matcher,
                         ransac: "FundamentalRansac | HomographyRansac | EssentialRansac", images0, images1, *, intrinsics=None):
    """match_source_images followed by ransac.verify on its outputs: (MatchResult, kpts0_src, kpts1_src,
    GeometryResult, HomographyResult or PoseResult), the matrices in the source images' own pixels; ransac is a
    FundamentalRansac, a HomographyRansac or an EssentialRansac, which takes intrinsics [P, 2, 4] (of the source
    images; required with it, refused with the others). What replaces the demo's PostProcess +
    cv::findFundamentalMat (demo/demo_mono.cpp:326-366); nothing is read back, so it enqueues, or is captured, as
    one piece."""
    calibrated = isinstance(ransac, EssentialRansac)
    if calibrated != (intrinsics is not None):
        raise ValueError("verify_source_images: intrinsics go with an EssentialRansac, and only with it")
    result, kp0, kp1 = match_source_images(image_input, encoder, frontend, matcher, images0, images1)
    if calibrated:
        return result, kp0, kp1, ransac.verify(result, kp0, kp1, intrinsics)
    return result, kp0, kp1, ransac.verify(result, kp0, kp1)
