"""Keypoint front end: SuperPoint's two dense heads to the matcher's inputs on gfx950 kernels.

The reference turns the detector logits (``convPb``'s output) and the dense descriptors (``convDb``'s) into
``(kpts, desc, count)`` with ``simple_nms`` (lightglue_pytorch_no_plugin/superpoint.py:52-69),
``sample_descriptors`` (:72-87) and ``SuperPointMonoTRT::PostProcess`` (demo/superpoint_mono_trt.cpp:153-253):
five 9 x 9 max-pools, about a dozen framework ops, and a ``nonzero`` that makes the host wait for each image's
count. ``KeypointFrontend`` does the same in at most five launches for any number of images (include/
lightglue_glue.h, "keypoint front end"; csrc/lightglue_frontend.hip) and leaves the counts on the device, as
the int32 table ``LightGlueMatcher.match_batch`` takes under stream capture. The CNN in front of it is
``superpoint.SuperPointEncoder`` (ten launches on the lg_sp_* kernels), whose ``heads`` writes both inputs in
the layouts ``extract`` reads in place; the heads of a framework SuperPoint are taken just the same.

``frontend_reference`` and the ``*_reference`` stages are the same contract in framework ops (CPU or GPU):
our restatement of those three reference pieces with the one rule they leave open pinned — among equal
scores the lower row-major pixel index comes first (``torch.topk`` promises no order there).
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _lib
from ._host import DT, _workspace, call, carve, require_gpu, stream_of

_STAGE = "the keypoint front end"
_FLOATS = (torch.float16, torch.float32)
MAX_KEYPOINTS = 2048  # the assignment head's limit (lg_assign_matches: m, n <= 2048, n % 8 == 0)
MAX_RADIUS = 4


class Features(NamedTuple):
    """The keypoints of B images, K slots each; rows past counts[b] are zero (scores too).

    kpts_px [B, K, 2] int32 (x, y); kpts [B, K, 2] = (xy - (W/2, H/2)) / (max(W, H)/2) and desc [B, K, 256]
    (unit L2 norm) in the front end's dtype; scores [B, K] fp32, descending; counts [B] int32."""
    kpts_px: torch.Tensor
    kpts: torch.Tensor
    desc: torch.Tensor
    scores: torch.Tensor
    counts: torch.Tensor

    def rows(self, sl) -> "Features":
        """The same slice of the images of every field."""
        return Features(*(t[sl] for t in self))


def _check_k(k: int) -> int:
    k = int(k)
    if not 1 <= k <= MAX_KEYPOINTS or k % 8:
        raise ValueError(f"max_keypoints must be a multiple of 8 in [8, {MAX_KEYPOINTS}], got {k}")
    return k


# ---- the four stages, one C entry point each ----------------------------------------------------------
def heatmap(logits: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lg_kp_heatmap: logits [B, 65, Hc, Wc] (fp16 / fp32) -> scores [B, 8 Hc, 8 Wc] fp32."""
    require_gpu("logits", logits, _STAGE, _FLOATS, 4)
    if logits.shape[1] != 65:
        raise ValueError(f"logits: expected [B, 65, Hc, Wc], got {tuple(logits.shape)}")
    logits = logits.contiguous()
    b, _, hc, wc = logits.shape
    if out is None:
        out = torch.empty((b, hc * 8, wc * 8), dtype=torch.float32, device=logits.device)
    call("lg_kp_heatmap", DT[logits.dtype], logits.data_ptr(), hc, wc, b, out.data_ptr(), stream_of(logits))
    return out


def nms(scores: torch.Tensor, radius: int = 4, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lg_kp_nms: simple_nms on scores [B, H, W] fp32, bitwise the reference's result."""
    require_gpu("scores", scores, _STAGE, (torch.float32,), 3)
    scores = scores.contiguous()
    b, h, w = scores.shape
    if out is None:
        out = torch.empty_like(scores)
    call("lg_kp_nms", scores.data_ptr(), h, w, b, int(radius), out.data_ptr(), stream_of(scores))
    return out


def select(nms_map: torch.Tensor, k: int, threshold: float = 0.0005, border: int = 4,
           workspace: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """lg_kp_select on the NMS map [B, H, W]: (count [B] int32, pix [B, k] int32, score [B, k] fp32), the k
    best candidates in descending score, ties by ascending pixel index; -1 / 0 past the count."""
    require_gpu("nms_map", nms_map, _STAGE, (torch.float32,), 3)
    nms_map = nms_map.contiguous()
    b, h, w = nms_map.shape
    dev = nms_map.device
    count = torch.empty((b,), dtype=torch.int32, device=dev)
    pix = torch.empty((b, int(k)), dtype=torch.int32, device=dev)
    score = torch.empty((b, int(k)), dtype=torch.float32, device=dev)
    stream = stream_of(nms_map)
    if workspace is None:
        workspace = _workspace(dev, stream, _lib.load().lg_kp_select_workspace(h, w, b))
    call("lg_kp_select", nms_map.data_ptr(), h, w, b, int(border), float(threshold), int(k), count.data_ptr(),
         pix.data_ptr(), score.data_ptr(), workspace.data_ptr(), stream)
    return count, pix, score


def describe(dense: torch.Tensor, count: torch.Tensor, pix: torch.Tensor, dense_normalized: bool = False,
             dtype: torch.dtype = torch.float16) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """lg_kp_describe: dense [B, 256, Hc, Wc] (fp16 / fp32, any strides: NCHW and channels_last are read in
    place) sampled at the selected pixels -> (desc [B, K, 256], kpts_px [B, K, 2] int32, kpts [B, K, 2])."""
    require_gpu("dense", dense, _STAGE, _FLOATS, 4)
    if dense.shape[1] != 256:
        raise ValueError(f"dense: expected [B, 256, Hc, Wc], got {tuple(dense.shape)}")
    if dtype not in DT:
        raise ValueError(f"dtype must be torch.float16 or torch.float32, got {dtype}")
    b, _, hc, wc = dense.shape
    k = pix.shape[1]
    if tuple(count.shape) != (b,) or tuple(pix.shape) != (b, k) or count.dtype != torch.int32 or pix.dtype != torch.int32:
        raise ValueError("count / pix: expected int32 [B] and [B, K] as select() returns them")
    if any(s < 0 for s in dense.stride()):
        dense = dense.contiguous()
    dev = dense.device
    desc = torch.empty((b, k, 256), dtype=dtype, device=dev)
    kpx = torch.empty((b, k, 2), dtype=torch.int32, device=dev)
    kpts = torch.empty((b, k, 2), dtype=dtype, device=dev)
    sb, sc, sy, sx = dense.stride()
    call("lg_kp_describe", DT[dense.dtype], dense.data_ptr(), sb, sc, sy, sx, hc, wc, b, k, count.contiguous().data_ptr(),
         pix.contiguous().data_ptr(), int(bool(dense_normalized)), DT[dtype], desc.data_ptr(), kpx.data_ptr(),
         kpts.data_ptr(), stream_of(dense))
    return desc, kpx, kpts


class KeypointFrontend:
    """SuperPoint's post-processing with the reference's defaults (superpoint.py:99-105; PostProcess' border
    of 4). max_keypoints is K, the slots per image: a multiple of 8, at most 2048 (the matcher's limits)."""

    def __init__(self, nms_radius: int = 4, threshold: float = 0.0005, max_keypoints: int = 1024,
                 remove_borders: int = 4, dtype: torch.dtype = torch.float16) -> None:
        if not 0 <= int(nms_radius) <= MAX_RADIUS:
            raise ValueError(f"nms_radius must be in [0, {MAX_RADIUS}], got {nms_radius}")
        if not float(threshold) >= 0.0:
            raise ValueError(f"threshold must be >= 0, got {threshold}")
        if int(remove_borders) < 0:
            raise ValueError(f"remove_borders must be >= 0, got {remove_borders}")
        if dtype not in DT:
            raise ValueError(f"dtype must be torch.float16 or torch.float32, got {dtype}")
        self.nms_radius, self.threshold = int(nms_radius), float(threshold)
        self.max_keypoints, self.remove_borders, self.dtype = _check_k(max_keypoints), int(remove_borders), dtype

    def _buffers(self, like: torch.Tensor, b: int, h: int, w: int):
        """The two [B, H, W] fp32 maps and lg_kp_select's workspace, carved from the stream's workspace."""
        plane = b * h * w * 4
        m0, m1, sel = carve(like.device, stream_of(like), [plane, plane, _lib.load().lg_kp_select_workspace(h, w, b)])
        return m0.view(torch.float32).view(b, h, w), m1.view(torch.float32).view(b, h, w), sel

    def _finish(self, nms_map, ws, dense, dense_normalized) -> Features:
        count, pix, score = select(nms_map, self.max_keypoints, self.threshold, self.remove_borders, workspace=ws)
        desc, kpx, kpts = describe(dense, count, pix, dense_normalized, self.dtype)
        return Features(kpx, kpts, desc, score, count)

    def _check_dense(self, dense, b, hc, wc):
        if dense.dim() != 4 or tuple(dense.shape) != (b, 256, hc, wc):
            raise ValueError(f"dense: expected [{b}, 256, {hc}, {wc}], got {tuple(dense.shape)}")

    def extract(self, logits: torch.Tensor, dense: torch.Tensor, dense_normalized: bool = False) -> Features:
        """logits [B, 65, Hc, Wc] (convPb's output) and dense [B, 256, Hc, Wc] (convDb's output, or with
        dense_normalized=True the L2-normalised map SuperPoint.forward returns) -> Features. Five launches."""
        require_gpu("logits", logits, _STAGE, _FLOATS, 4)
        b, _, hc, wc = logits.shape
        self._check_dense(dense, b, hc, wc)
        heat, nmap, ws = self._buffers(logits, b, hc * 8, wc * 8)
        heatmap(logits, out=heat)
        nms(heat, self.nms_radius, out=nmap)
        return self._finish(nmap, ws, dense, dense_normalized)

    def from_scores(self, scores: torch.Tensor, dense: torch.Tensor, dense_normalized: bool = False,
                    nms_done: bool = False) -> Features:
        """The same from a heatmap [B, H, W] fp32 a caller's SuperPoint already produced (H, W multiples of
        8). nms_done=True: the map is already simple_nms' output (what the reference's SuperPoint.forward
        returns), and the NMS launch is skipped."""
        require_gpu("scores", scores, _STAGE, (torch.float32,), 3)
        b, h, w = scores.shape
        if h % 8 or w % 8:
            raise ValueError(f"scores: H and W must be multiples of 8, got {h} x {w}")
        self._check_dense(dense, b, h // 8, w // 8)
        _, nmap, ws = self._buffers(scores, b, h, w)
        if nms_done:
            nmap = scores.contiguous()
        else:
            nms(scores, self.nms_radius, out=nmap)
        return self._finish(nmap, ws, dense, dense_normalized)


# ---- the same contract in framework ops (the tests' oracle) ---------------------------------------------
def heatmap_reference(logits: torch.Tensor) -> torch.Tensor:
    """superpoint.py:160-165 in the logits' dtype (fp16 is computed in fp32)."""
    x = logits.float() if logits.dtype == torch.float16 else logits
    b, _, hc, wc = x.shape
    p = torch.softmax(x, 1)[:, :64]
    return p.reshape(b, 8, 8, hc, wc).permute(0, 3, 1, 4, 2).reshape(b, hc * 8, wc * 8)


def nms_reference(scores: torch.Tensor, radius: int = 4) -> torch.Tensor:
    """simple_nms (superpoint.py:52-69): the local maxima, then twice the local maxima of what their
    neighbourhoods leave; equality comparisons, -inf padding."""
    def pool(x):
        return F.max_pool2d(x[:, None], 2 * radius + 1, stride=1, padding=radius)[:, 0]

    keep = scores == pool(scores)
    for _ in range(2):
        near = pool(keep.to(scores.dtype)) > 0
        rest = scores.masked_fill(near, 0.0)
        keep = keep | ((rest == pool(rest)) & ~near)
    return torch.where(keep, scores, torch.zeros_like(scores))


def select_reference(nms_map: torch.Tensor, k: int, threshold: float = 0.0005, border: int = 4):
    """PostProcess:167-217 with the order pinned: descending score, ties by ascending pixel index."""
    b, h, w = nms_map.shape
    dev = nms_map.device
    ys = torch.arange(h, device=dev)[:, None]
    xs = torch.arange(w, device=dev)[None, :]
    inner = (ys >= border) & (ys < h - border) & (xs >= border) & (xs < w - border)
    count = torch.zeros((b,), dtype=torch.int32, device=dev)
    pix = torch.full((b, k), -1, dtype=torch.int32, device=dev)
    score = torch.zeros((b, k), dtype=nms_map.dtype, device=dev)
    for i in range(b):
        flat = nms_map[i].reshape(-1)
        idx = torch.nonzero((inner & (nms_map[i] > threshold)).reshape(-1))[:, 0]  # ascending pixel index
        order = torch.sort(flat[idx], descending=True, stable=True)[1][:k]       # stable: ties keep that order
        n = order.numel()
        count[i], pix[i, :n], score[i, :n] = n, idx[order].to(torch.int32), flat[idx[order]]
    return count, pix, score


def describe_reference(dense: torch.Tensor, count: torch.Tensor, pix: torch.Tensor, dense_normalized: bool = False,
                       dtype: Optional[torch.dtype] = None, compute: Optional[torch.dtype] = None):
    """sample_descriptors + PostProcess:219-245 computed in `compute` (default fp32; torch.float64 is the
    tests' exact restatement), results cast to `dtype` (default: compute)."""
    compute = compute or torch.float32
    dtype = dtype or compute
    b, c, hc, wc = dense.shape
    h, w = hc * 8, wc * 8
    k = pix.shape[1]
    d = dense.to(compute)
    if not dense_normalized:
        d = d / d.norm(dim=1, keepdim=True).clamp_min(1e-12)
    p = pix.clamp(0, h * w - 1).long()
    xy = torch.stack([p % w, p // w], -1)  # [B, K, 2] (x, y)
    valid = (torch.arange(k, device=pix.device)[None, :] < count.clamp(0, k)[:, None])
    size = torch.tensor([w, h], dtype=compute, device=dense.device)
    grid = (xy.to(compute) - 4 + 0.5) / (size - 4 - 0.5) * 2 - 1
    out = F.grid_sample(d, grid[:, None], mode="bilinear", padding_mode="zeros", align_corners=True)[:, :, 0]  # [B, C, K]
    out = (out / out.norm(dim=1, keepdim=True).clamp_min(1e-12)).transpose(1, 2)
    kn = (xy.to(compute) - size / 2) / (max(w, h) / 2)
    m = valid[..., None]
    zero = torch.zeros((), dtype=compute, device=dense.device)
    return (torch.where(m, out, zero).to(dtype), torch.where(m, xy, torch.zeros_like(xy)).to(torch.int32),
            torch.where(m, kn, zero).to(dtype))


def frontend_reference(logits: Optional[torch.Tensor], dense: torch.Tensor, dense_normalized: bool = False, *,
                       scores: Optional[torch.Tensor] = None, nms_radius: int = 4, threshold: float = 0.0005,
                       max_keypoints: int = 1024, remove_borders: int = 4, dtype: torch.dtype = torch.float16) -> Features:
    """KeypointFrontend(...).extract(logits, dense, dense_normalized) — or, with logits None, .from_scores(
    scores, ...) — in framework ops, on the tensors' device (CPU or GPU). fp32 arithmetic throughout; only
    the returned desc / kpts are cast to `dtype`."""
    k = _check_k(max_keypoints)
    heat = heatmap_reference(logits) if logits is not None else scores
    nmap = nms_reference(heat.float(), nms_radius)
    count, pix, score = select_reference(nmap, k, threshold, remove_borders)
    d = dense.float() if dense.dtype == torch.float16 else dense
    desc, kpx, kpts = describe_reference(d, count, pix, dense_normalized, dtype=dtype)
    return Features(kpx, kpts, desc, score, count)
