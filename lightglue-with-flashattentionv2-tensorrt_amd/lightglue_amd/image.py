"""Image input: uint8 images of any size, channel count and strides to the encoder's input, and the keypoints
back to each source image's own pixels, on gfx950 kernels.

The reference never hands its network an unprepared frame: demo/demo_mono.cpp:151-152, 232-233 resizes to
640 x 480 with INTER_LINEAR, converts to float and divides by 255; lightglue_pytorch_no_plugin/utils.py:30-76
resizes (default ``area``), converts 0.299 R + 0.587 G + 0.114 B and keeps the scale; utils.py:94-97 maps the
keypoints back with ``(kp + 0.5) / scale - 0.5``. ``ImageInput.prepare`` does the first two in one launch for a
whole batch (include/lightglue_glue.h, "image input"; csrc/lightglue_image.hip): the sources may each have
their own size, channels and strides (a device table of descriptors, ``ImageInput.table``), or be one
``[B, ...]`` tensor of equal-sized frames (no table). ``ImageInput.keypoints`` is the third, and
``match_source_images`` puts ``match_images`` between them; nothing on the way synchronises with the host.

The resampling is pinned here (``resample_matrix``): ``out = Wy · grey · Wxᵀ / 255``, per axis ``linear``
(INTER_LINEAR's and ``F.interpolate(bilinear, align_corners=False)``'s convention) or, where the source is
larger than the target and ``area`` is asked for, the overlap-weighted mean of INTER_AREA. ``image_reference``
is the same contract in framework ops (CPU or GPU), the tests' oracle.
"""
from __future__ import annotations

import ctypes
import functools
from typing import NamedTuple, Sequence, Tuple, Union

import torch

from . import _lib
from ._host import DT, PluginError, call, require_gpu, stream_of
from .frontend import Features, KeypointFrontend
from .superpoint import SuperPointEncoder, extract_pairs

_STAGE = "the image input"
_INTERP = {"linear": _lib.IMG_LINEAR, "area": _lib.IMG_AREA}
MAX_SIDE = 16384  # source and target sides: (2 o + 1) w stays in int32
GREY = (0.299, 0.587, 0.114)  # utils.py:72-76


def _check_interp(interp: str) -> str:
    if interp not in _INTERP:
        raise ValueError(f"interp must be 'linear' or 'area', got {interp!r}")
    return interp


def _check_target(size) -> Tuple[int, int]:
    if isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(s, int) for s in size):
        h, w = size
        if h % 8 or w % 8 or not 8 <= h <= MAX_SIDE or not 8 <= w <= MAX_SIDE:
            raise ValueError(f"target size: H and W must be multiples of 8 in [8, {MAX_SIDE}], got {h} x {w}")
        return h, w
    raise ValueError(f"target size: expected (H, W), got {size!r} (target_size(h, w, resize) makes one from an int)")


def target_size(h: int, w: int, resize) -> Tuple[int, int]:
    """The target of a source of h x w pixels. resize=(H, W): that, both multiples of 8. resize=int: the longer
    side becomes `resize` as utils.resize_image does with fn=max (scale = resize / max(h, w), round(h scale),
    round(w scale)), then each side goes to the nearest multiple of 8 (a tie upwards), at least 8."""
    if not isinstance(resize, int) or isinstance(resize, bool):
        return _check_target(resize)
    if h < 1 or w < 1 or resize < 1:
        raise ValueError(f"target_size: sides and resize must be positive, got {h} x {w}, resize {resize}")
    scale = resize / max(h, w)
    return _check_target(tuple(max(8, (int(round(s * scale)) + 4) // 8 * 8) for s in (h, w)))


# ---- the pinned resampling ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=64)
def _matrix(n_src: int, n_dst: int, interp: str) -> torch.Tensor:
    o = torch.arange(n_dst, dtype=torch.int64)
    if interp == "area" and n_src > n_dst:
        i = torch.arange(n_src, dtype=torch.int64)[None, :]
        lo, hi = (o * n_src)[:, None], ((o + 1) * n_src)[:, None]
        num = (torch.minimum((i + 1) * n_dst, hi) - torch.maximum(i * n_dst, lo)).clamp_(min=0)
        return num.double() / n_src
    d = 2 * n_dst
    p = (2 * o + 1) * n_src - n_dst
    i0 = torch.div(p, d, rounding_mode="floor")
    r = p - i0 * d
    m = torch.zeros((n_dst, n_src), dtype=torch.float64)
    m.index_put_((o, i0.clamp(0, n_src - 1)), (d - r).double() / d, accumulate=True)
    m.index_put_((o, (i0 + 1).clamp(0, n_src - 1)), r.double() / d, accumulate=True)
    return m


def resample_matrix(n_src: int, n_dst: int, interp: str = "linear") -> torch.Tensor:
    """W [n_dst, n_src] float64 (CPU): one axis of the resampling, rows summing to 1.

    linear: output o sits at source position ((2 o + 1) n_src - n_dst) / (2 n_dst) = i + f; weights 1 - f and f
    on i and i + 1, both clamped into [0, n_src - 1]. area, where n_src > n_dst: output o covers
    [o n_src / n_dst, (o + 1) n_src / n_dst) and source i weighs its overlap with that interval over
    n_src / n_dst; elsewhere area is linear. Positions and overlaps are integers, one division per weight."""
    n_src, n_dst = int(n_src), int(n_dst)
    if not 1 <= n_src <= MAX_SIDE or not 1 <= n_dst <= MAX_SIDE:
        raise ValueError(f"resample_matrix: sides must be in [1, {MAX_SIDE}], got {n_src} -> {n_dst}")
    return _matrix(n_src, n_dst, _check_interp(interp)).clone()


@functools.lru_cache(maxsize=64)
def _matrix_on(n_src: int, n_dst: int, interp: str, device: str, dtype: torch.dtype) -> torch.Tensor:
    return _matrix(n_src, n_dst, interp).to(device=device, dtype=dtype)


# ---- sources ----------------------------------------------------------------------------------------------------
def _describe(img: torch.Tensor, layout: str, what: str = "image") -> Tuple[int, int, int, int, int, int]:
    """One source image -> (h, w, channels, stride_y, stride_x, stride_c), strides in elements (= bytes).
    Type, dtype, shape and sides are checked here, the device by the caller."""
    if not isinstance(img, torch.Tensor):
        raise ValueError(f"{what}: expected a tensor, got {type(img).__name__}")
    if img.dtype != torch.uint8:
        raise ValueError(f"{what}: expected torch.uint8, got {img.dtype}")
    if img.dim() == 2:
        (h, w), c, (sy, sx), sc = img.shape, 1, img.stride(), 0
    elif img.dim() == 3 and layout == "hwc":
        (h, w, c), (sy, sx, sc) = img.shape, img.stride()
    elif img.dim() == 3 and layout == "chw":
        (c, h, w), (sc, sy, sx) = img.shape, img.stride()
    else:
        raise ValueError(f"{what}: expected [H, W], [H, W, C] (layout='hwc') or [C, H, W] (layout='chw'), got "
                         f"{tuple(img.shape)} with layout={layout!r}")
    if c not in (1, 3, 4):
        raise ValueError(f"{what}: 1, 3 or 4 channels, got {c}")
    if not 1 <= h <= MAX_SIDE or not 1 <= w <= MAX_SIDE:
        raise ValueError(f"{what}: sides must be in [1, {MAX_SIDE}], got {h} x {w}")
    return int(h), int(w), int(c), int(sy), int(sx), int(sc)


def _check_layout(layout: str) -> str:
    if layout not in ("hwc", "chw"):
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    return layout


class ImageBatch(NamedTuple):
    """B source images as lg_img_prepare reads them: table, the device array of B descriptors (uint8
    [B * lg_img_src_bytes()]); src_sizes [B, 2] int32 (h, w) on the device; sources, the tensors the
    descriptors point into, kept alive here."""
    table: torch.Tensor
    src_sizes: torch.Tensor
    sources: Tuple[torch.Tensor, ...]


class PreparedImages(NamedTuple):
    """image [B, Ht, Wt], grey in [0, 1], contiguous: the encoder's input; src_sizes [B, 2] int32 (h, w) of
    each source, on the device."""
    image: torch.Tensor
    src_sizes: torch.Tensor


class ImageInput:
    """uint8 images to the encoder's input of size (Ht, Wt), both multiples of 8, shared by all images.
    interp: 'linear' or 'area' (the demo's and utils.load_image's defaults); dtype: the output's, fp16 or fp32."""

    def __init__(self, size, interp: str = "linear", dtype: torch.dtype = torch.float16) -> None:
        self.size = _check_target(tuple(size) if isinstance(size, list) else size)
        self.interp = _check_interp(interp)
        if dtype not in DT:
            raise ValueError(f"dtype must be torch.float16 or torch.float32, got {dtype}")
        self.dtype = dtype
        self._sizes = {}  # (device, B, h, w) -> src_sizes of a [B, ...] tensor's frames

    def table(self, images: Sequence[torch.Tensor], layout: str = "hwc", bgr: bool = False) -> ImageBatch:
        """A list of uint8 CUDA tensors, each [H, W], [H, W, C] or [C, H, W] (C = 1, 3, 4; any sizes and strides:
        views are read in place) -> ImageBatch. Everything is validated here; the table is uploaded once from
        pinned memory without synchronising. It describes the tensors, not their contents: new pixels written
        into the same tensors need no new table (the form to use under stream capture)."""
        _check_layout(layout)
        images = tuple(images)
        n = len(images)
        if n == 0:
            raise ValueError("images: no images")
        desc = [_describe(img, layout, f"images[{i}]") for i, img in enumerate(images)]
        for i, img in enumerate(images):
            require_gpu(f"images[{i}]", img, _STAGE)
        dev = images[0].device
        if any(img.device != dev for img in images):
            raise ValueError("images: all sources must be on one device")
        rec = ctypes.sizeof(_lib.ImgSrc)
        if _lib.load().lg_img_src_bytes() != rec:
            raise PluginError(f"lg_img_src is {_lib.load().lg_img_src_bytes()} bytes in the library, {rec} here")
        arr = (_lib.ImgSrc * n)()
        sizes = (ctypes.c_int32 * (2 * n))()
        for i, (img, (h, w, c, sy, sx, sc)) in enumerate(zip(images, desc)):
            arr[i] = _lib.ImgSrc(img.data_ptr(), h, w, c, int(bool(bgr)), sy, sx, sc)
            sizes[2 * i], sizes[2 * i + 1] = h, w
        host = torch.empty((n * (rec + 8),), dtype=torch.uint8).pin_memory()
        host[:n * rec] = torch.frombuffer(arr, dtype=torch.uint8)
        host[n * rec:] = torch.frombuffer(sizes, dtype=torch.uint8)
        both = host.to(dev, non_blocking=True)  # (rec % 8 == 0: the sizes behind the table stay aligned)
        return ImageBatch(both[:n * rec], both[n * rec:].view(torch.int32).view(n, 2), images)

    def _frame_sizes(self, dev: torch.device, b: int, h: int, w: int) -> torch.Tensor:
        key = (dev, b, h, w)
        t = self._sizes.get(key)
        if t is None:  # fills, not a copy from the host: safe under stream capture
            t = torch.empty((b, 2), dtype=torch.int32, device=dev)
            t[:, 0], t[:, 1] = h, w
            self._sizes[key] = t
        return t

    def prepare(self, images: Union[ImageBatch, torch.Tensor, Sequence[torch.Tensor]], layout: str = "hwc",
                bgr: bool = False) -> PreparedImages:
        """An ImageBatch, a list of images (table(images, layout, bgr) first) or one uint8 CUDA tensor of B
        equal-sized frames ([B, H, W], [B, H, W, C] or [B, C, H, W], any strides; lg_img_prepare_batch, no
        table) -> PreparedImages. One launch."""
        ht, wt = self.size
        if isinstance(images, torch.Tensor):
            _check_layout(layout)
            if images.dim() not in (3, 4):
                raise ValueError(f"images: expected [B, H, W], [B, H, W, C] or [B, C, H, W], got {tuple(images.shape)}")
            if images.shape[0] == 0:
                raise ValueError("images: no images")
            h, w, c, sy, sx, sc = _describe(images[0], layout, "images")
            require_gpu("images", images, _STAGE)
            b, dev = images.shape[0], images.device
            out = torch.empty((b, ht, wt), dtype=self.dtype, device=dev)
            call("lg_img_prepare_batch", images.data_ptr(), b, h, w, c, int(bool(bgr)), images.stride(0), sy, sx, sc, ht, wt,
                 _INTERP[self.interp], DT[self.dtype], out.data_ptr(), stream_of(images))
            return PreparedImages(out, self._frame_sizes(dev, b, h, w))
        batch = images if isinstance(images, ImageBatch) else self.table(images, layout, bgr)
        b, dev = batch.src_sizes.shape[0], batch.table.device
        require_gpu("table", batch.table, _STAGE)
        if batch.table.dtype != torch.uint8 or batch.table.numel() != b * ctypes.sizeof(_lib.ImgSrc) or b < 1:
            raise ValueError(f"table: expected table()'s uint8 [{b} * {ctypes.sizeof(_lib.ImgSrc)}], got "
                             f"{tuple(batch.table.shape)} {batch.table.dtype}")
        out = torch.empty((b, ht, wt), dtype=self.dtype, device=dev)
        call("lg_img_prepare", batch.table.data_ptr(), b, ht, wt, _INTERP[self.interp], DT[self.dtype], out.data_ptr(),
             stream_of(out))
        return PreparedImages(out, batch.src_sizes)

    def keypoints(self, features: Features, prepared: PreparedImages) -> torch.Tensor:
        """features.kpts_px [B, K, 2] (pixels of the prepared images) -> [B, K, 2] fp32 (x, y) in each source
        image's own pixels: (2 px + 1) w / (2 Wt) - 1/2 (utils.py:94-97); rows past features.counts are zero."""
        kpx, counts, sizes = features.kpts_px, features.counts, prepared.src_sizes
        for name, t in (("kpts_px", kpx), ("counts", counts), ("src_sizes", sizes)):
            require_gpu(name, t, _STAGE, (torch.int32,))
        if kpx.dim() != 3 or kpx.shape[2] != 2 or kpx.shape[1] < 1:
            raise ValueError(f"kpts_px: expected [B, K, 2], got {tuple(kpx.shape)}")
        b, k, _ = kpx.shape
        if tuple(counts.shape) != (b,) or tuple(sizes.shape) != (b, 2):
            raise ValueError(f"counts / src_sizes: expected [{b}] and [{b}, 2], got {tuple(counts.shape)} and "
                             f"{tuple(sizes.shape)}")
        out = torch.empty((b, k, 2), dtype=torch.float32, device=kpx.device)
        if b:
            call("lg_kp_to_source", kpx.contiguous().data_ptr(), counts.contiguous().data_ptr(), sizes.contiguous().data_ptr(),
                 self.size[0], self.size[1], b, k, out.data_ptr(), stream_of(kpx))
        return out


def match_source_images(image_input: ImageInput, encoder: SuperPointEncoder, frontend: KeypointFrontend, matcher, images0,
                        images1):
    """The matches of P pairs of source images and the keypoints in each source's own pixels: (MatchResult,
    kpts0_src [P, K, 2], kpts1_src [P, K, 2]). images0 / images1: what ImageInput.prepare takes (the two sides
    may differ in every source size; the target is shared). prepare on each side, extract_pairs on the prepared
    tensors, matcher.match_features and keypoints on its two Features. Nothing is read back: with an ImageBatch
    or a tensor per side the whole enqueues, or is captured, as one piece."""
    p0, p1 = image_input.prepare(images0), image_input.prepare(images1)
    f0, f1 = extract_pairs(encoder, frontend, p0.image, p1.image)
    result = matcher.match_features(f0, f1)
    return result, image_input.keypoints(f0, p0), image_input.keypoints(f1, p1)


# ---- the same contract in framework ops (the tests' oracle, the A/B's other arm) ----------------------------
def _grey(img: torch.Tensor, layout: str, bgr: bool, compute: torch.dtype) -> torch.Tensor:
    """[..., H, W] (no channel axis), [..., H, W, C] or [..., C, H, W] uint8 -> 0.299 R + 0.587 G + 0.114 B in
    `compute`, contiguous; one channel as it is, a fourth ignored."""
    if img.dim() == 2:
        return img.to(compute).contiguous()
    ch = img.unbind(-1 if layout == "hwc" else -3)
    if len(ch) == 1:
        return ch[0].to(compute).contiguous()
    r, g, b = (ch[i].to(compute) for i in ((2, 1, 0) if bgr else (0, 1, 2)))
    return ((GREY[0] * r + GREY[1] * g) + GREY[2] * b).contiguous()


def image_reference(images, size, interp: str = "linear", dtype: torch.dtype = torch.float16,
                    compute: torch.dtype = torch.float64, layout: str = "hwc", bgr: bool = False) -> torch.Tensor:
    """ImageInput(size, interp, dtype).prepare(images, layout, bgr).image in framework ops, on the images'
    device (CPU or GPU): Wy · grey · Wxᵀ / 255 with resample_matrix's weights, computed in `compute` and cast
    to `dtype` (any float type: torch.float64 keeps the unrounded value). images: a list of [H, W], [H, W, C]
    or [C, H, W] uint8 tensors, or one [B, ...] tensor."""
    ht, wt = int(size[0]), int(size[1])
    _check_interp(interp), _check_layout(layout)

    def resample(frames: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
        """One frame (`like` itself) or a batch of frames that `like` is one of -> [..., Ht, Wt]."""
        h, w = _describe(like, layout)[:2]
        wy = _matrix_on(h, ht, interp, str(like.device), compute)
        wx = _matrix_on(w, wt, interp, str(like.device), compute)
        grey = frames.to(compute).contiguous() if like.dim() == 2 else _grey(frames, layout, bgr, compute)
        return (wy @ grey @ wx.t()) / 255.0

    if isinstance(images, torch.Tensor):
        if images.dim() not in (3, 4) or images.shape[0] == 0:
            raise ValueError(f"images: expected a non-empty [B, H, W], [B, H, W, C] or [B, C, H, W], got {tuple(images.shape)}")
        return resample(images, images[0]).to(dtype)
    return torch.stack([resample(img, img) for img in images]).to(dtype)
