"""SuperPoint's encoder and its two dense heads on gfx950 kernels: images to the keypoint front end's inputs.

The reference's forward (lightglue_pytorch_no_plugin/superpoint.py:143-172) is twelve convolutions: conv1a ..
conv4b with three 2 x 2 max-pools, then convPa -> convPb (the detector's 65 logits per 8 x 8 cell) and convDa ->
convDb (the 256-d dense descriptors). ``SuperPointEncoder.heads`` runs them in fp16 in ten launches (include/
lightglue_glue.h, "SuperPoint encoder"; csrc/lightglue_superpoint.hip): lg_sp_conv1, eight lg_sp_conv3x3 (pools
fused, convPa and convDa as one 512-channel layer that reads conv4b's output once) and lg_sp_heads, which writes
the logits as ``[B, 65, Hc, Wc]`` and the descriptors as ``[B, Hc, Wc, 256]`` — what ``KeypointFrontend.extract``
takes without a copy. With its five launches that is fifteen from an image batch to ``Features``, and
``match_images`` goes on to the matches; nothing on the way synchronises with the host.

The arithmetic model ("fp16 storage"): weights, biases and every layer's output are fp16 values; a layer
accumulates in fp32, adds the bias in fp32, applies ReLU and rounds once. ``superpoint_reference`` is the same
forward in framework ops — with ``storage=None`` the reference's own chain of conv2d / relu / max_pool2d, with
``storage=torch.float16`` that model — and the tests' oracle.
"""
from __future__ import annotations

import zlib
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import _lib, synth
from ._host import DT, call, carve, require_gpu, stream_of
from .frontend import Features, KeypointFrontend

_STAGE = "the SuperPoint encoder"
_HALF = (torch.float16,)

# name -> (cout, cin, kernel), in forward order (superpoint.py:115-130)
LAYERS = {
    "conv1a": (64, 1, 3), "conv1b": (64, 64, 3), "conv2a": (64, 64, 3), "conv2b": (64, 64, 3),
    "conv3a": (128, 64, 3), "conv3b": (128, 128, 3), "conv4a": (128, 128, 3), "conv4b": (128, 128, 3),
    "convPa": (256, 128, 3), "convPb": (65, 256, 1), "convDa": (256, 128, 3), "convDb": (256, 256, 1),
}
_POOLED = ("conv1b", "conv2b", "conv3b")  # the layers a 2 x 2 max-pool follows
CONV_CIN = (64, 128)                     # lg_sp_conv3x3's channel counts
CONV_COUT = (64, 128, 256, 512)
HEAD_ROWS = 96 + 256                     # lg_sp_heads' weight rows: convPb's 65 padded to 96, then convDb's


# ---- packed weights ---------------------------------------------------------------------------------------
def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """[cout, cin, kh, kw] (cout % 32 == 0, cin % 16 == 0) -> the kernels' fragment-major stream
    [cout / 32][kh kw][cin / 16][2][32][8] (include/lightglue_glue.h, "packed weights"), flat."""
    cout, cin, kh, kw = w.shape
    if cout % 32 or cin % 16:
        raise ValueError(f"pack_conv: cout % 32 and cin % 16 must be 0, got {tuple(w.shape)}")
    x = w.reshape(cout // 32, 32, cin // 16, 2, 8, kh * kw)  # (cb, r, ks, hi, j, t)
    return x.permute(0, 5, 2, 3, 1, 4).contiguous().reshape(-1)


def unpack_conv(p: torch.Tensor, cout: int, cin: int, kh: int, kw: int) -> torch.Tensor:
    """pack_conv's inverse permutation."""
    x = p.reshape(cout // 32, kh * kw, cin // 16, 2, 32, 8)  # (cb, t, ks, hi, r, j)
    return x.permute(0, 4, 2, 3, 5, 1).contiguous().reshape(cout, cin, kh, kw)


# ---- the four entry points ----------------------------------------------------------------------------------
def conv1(image: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, relu: bool = True,
          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lg_sp_conv1: image [B, H, W] (fp16 / fp32), weight [64, 1, 3, 3] and bias [64] fp16 -> [B, H, W, 64] fp16."""
    require_gpu("image", image, _STAGE, tuple(DT))
    require_gpu("weight", weight, _STAGE, _HALF), require_gpu("bias", bias, _STAGE, _HALF)
    if image.dim() != 3 or tuple(weight.shape) != (64, 1, 3, 3) or tuple(bias.shape) != (64,):
        raise ValueError(f"conv1: expected image [B, H, W], weight [64, 1, 3, 3], bias [64]; got {tuple(image.shape)}, "
                         f"{tuple(weight.shape)}, {tuple(bias.shape)}")
    image, weight, bias = image.contiguous(), weight.contiguous(), bias.contiguous()
    b, h, w = image.shape
    if out is None:
        out = torch.empty((b, h, w, 64), dtype=torch.float16, device=image.device)
    call("lg_sp_conv1", DT[image.dtype], image.data_ptr(), weight.data_ptr(), bias.data_ptr(), h, w, b,
         _lib.SP_RELU if relu else 0, out.data_ptr(), stream_of(image))
    return out


def conv3x3(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, relu: bool = True, pool: bool = False,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """lg_sp_conv3x3: x [B, H, W, cin] fp16 contiguous, w_packed = pack_conv(weight [cout, cin, 3, 3]), bias
    [cout] -> [B, H, W, cout], or [B, H / 2, W / 2, cout] with pool (ReLU, then the 2 x 2 maximum)."""
    for name, t in (("x", x), ("w_packed", w_packed), ("bias", bias)):
        require_gpu(name, t, _STAGE, _HALF)
    if x.dim() != 4 or bias.dim() != 1 or w_packed.dim() != 1:
        raise ValueError("conv3x3: expected x [B, H, W, cin], a flat w_packed and bias [cout]")
    x, w_packed, bias = x.contiguous(), w_packed.contiguous(), bias.contiguous()
    b, h, w, cin = x.shape
    cout = bias.shape[0]
    need = _lib.load().lg_sp_packed_bytes(9, cin, cout)
    if need == 0 or w_packed.numel() * 2 != need:
        raise ValueError(f"conv3x3: cin {cin} / cout {cout} unsupported, or w_packed has {w_packed.numel()} elements, "
                         f"not {need // 2}")
    if pool and (h % 2 or w % 2):
        raise ValueError(f"conv3x3: pooling needs even H and W, got {h} x {w}")
    oh, ow = (h // 2, w // 2) if pool else (h, w)
    if out is None:
        out = torch.empty((b, oh, ow, cout), dtype=torch.float16, device=x.device)
    flags = (_lib.SP_RELU if relu else 0) | (_lib.SP_POOL2 if pool else 0)
    call("lg_sp_conv3x3", x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), cin, cout, h, w, b, flags, out.data_ptr(),
         stream_of(x))
    return out


def pack_heads(wpb: torch.Tensor, bpb: torch.Tensor, wdb: torch.Tensor, bdb: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """convPb's [65, 256, 1, 1] / [65] and convDb's [256, 256, 1, 1] / [256] -> lg_sp_heads' (w_packed, bias
    [352]): convPb's rows padded with zeros to 96, then convDb's."""
    w = torch.zeros((HEAD_ROWS, 256, 1, 1), dtype=wpb.dtype, device=wpb.device)
    b = torch.zeros((HEAD_ROWS,), dtype=bpb.dtype, device=bpb.device)
    w[:65], w[96:] = wpb, wdb
    b[:65], b[96:] = bpb, bdb
    return pack_conv(w), b


def heads(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """lg_sp_heads: x [B, Hc, Wc, 512] (cPa | cDa) fp16 -> (logits [B, 65, Hc, Wc] contiguous, dense: a
    [B, 256, Hc, Wc] view of the [B, Hc, Wc, 256] tensor the kernel wrote)."""
    for name, t in (("x", x), ("w_packed", w_packed), ("bias", bias)):
        require_gpu(name, t, _STAGE, _HALF)
    if x.dim() != 4 or x.shape[3] != 512 or w_packed.numel() != HEAD_ROWS * 256 or tuple(bias.shape) != (HEAD_ROWS,):
        raise ValueError(f"heads: expected x [B, Hc, Wc, 512], pack_heads' weights and bias; got {tuple(x.shape)}")
    x, w_packed, bias = x.contiguous(), w_packed.contiguous(), bias.contiguous()
    b, hc, wc, _ = x.shape
    logits = torch.empty((b, 65, hc, wc), dtype=torch.float16, device=x.device)
    dense = torch.empty((b, hc, wc, 256), dtype=torch.float16, device=x.device)
    call("lg_sp_heads", x.data_ptr(), w_packed.data_ptr(), bias.data_ptr(), hc, wc, b, logits.data_ptr(), dense.data_ptr(),
         stream_of(x))
    return logits, dense.permute(0, 3, 1, 2)


# ---- the encoder --------------------------------------------------------------------------------------------
def _checked_state(state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    out = {}
    for name, (cout, cin, k) in LAYERS.items():
        for key, shape in ((f"{name}.weight", (cout, cin, k, k)), (f"{name}.bias", (cout,))):
            if key not in state_dict:
                raise KeyError(f"SuperPoint state dict: missing {key}")
            t = state_dict[key]
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
                raise ValueError(f"SuperPoint state dict: {key} must be a tensor of shape {shape}, got "
                                 f"{tuple(getattr(t, 'shape', ()))}")
            out[key] = t
    return out


class SuperPointEncoder:
    """The SuperPoint forward up to convPb's and convDb's outputs, fp16, on the lg_sp_* kernels.

    state_dict: the reference's keys (conv1a.weight ... convDb.bias; superpoint_v1.pth loads unchanged), on
    any device. The weights are rounded to fp16 and packed once per device, at the first call there."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], dtype: torch.dtype = torch.float16) -> None:
        if dtype != torch.float16:
            raise ValueError(f"SuperPointEncoder: only torch.float16 is implemented, got {dtype}")
        self.dtype = dtype
        self._state = {k: v.detach() for k, v in _checked_state(state_dict).items()}
        self._packed: Dict[torch.device, dict] = {}

    def _weights(self, dev: torch.device) -> dict:
        p = self._packed.get(dev)
        if p is None:
            s = {k: v.to(dev, torch.float16) for k, v in self._state.items()}
            p = {"conv1a": (s["conv1a.weight"].contiguous(), s["conv1a.bias"].contiguous())}
            for name in ("conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b"):
                p[name] = (pack_conv(s[f"{name}.weight"]), s[f"{name}.bias"].contiguous())
            p["convPDa"] = (pack_conv(torch.cat([s["convPa.weight"], s["convDa.weight"]])),
                            torch.cat([s["convPa.bias"], s["convDa.bias"]]).contiguous())
            p["heads"] = pack_heads(s["convPb.weight"], s["convPb.bias"], s["convDb.weight"], s["convDb.bias"])
            self._packed[dev] = p
        return p

    @staticmethod
    def _image(image: torch.Tensor) -> torch.Tensor:
        require_gpu("image", image, _STAGE)
        if image.dim() == 4 and image.shape[1] == 1:
            image = image[:, 0]
        if image.dim() != 3 or image.dtype not in DT:
            raise ValueError(f"image: expected [B, 1, H, W] or [B, H, W] in fp16 or fp32, got {tuple(image.shape)} {image.dtype}")
        if image.shape[1] % 8 or image.shape[2] % 8 or image.shape[1] == 0 or image.shape[2] == 0:
            raise ValueError(f"image: H and W must be positive multiples of 8, got {image.shape[1]} x {image.shape[2]}")
        return image.contiguous()

    def heads(self, image: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """image [B, 1, H, W] or [B, H, W] (fp16 / fp32; H, W multiples of 8) -> (logits [B, 65, H/8, W/8]
        contiguous, dense [B, 256, H/8, W/8] with channels-last strides), both fp16. Ten launches; the
        intermediates live in the stream's workspace, the two results are new tensors."""
        image = self._image(image)
        b, h, w = image.shape
        p = self._weights(image.device)
        # conv1a's output, the largest, and conv1b's pooled output, the largest of the others
        regions = carve(image.device, stream_of(image), [b * h * w * 64 * 2, b * h * w * 16 * 2])

        def buf(which: int, hh: int, ww: int, c: int) -> torch.Tensor:
            return regions[which][:b * hh * ww * c * 2].view(torch.float16).view(b, hh, ww, c)

        x = conv1(image, *p["conv1a"], out=buf(0, h, w, 64))
        which = 1
        for name in ("conv1b", "conv2a", "conv2b", "conv3a", "conv3b", "conv4a", "conv4b", "convPDa"):
            pool = name in _POOLED
            hh, ww = (x.shape[1] // 2, x.shape[2] // 2) if pool else (x.shape[1], x.shape[2])
            x = conv3x3(x, *p[name], relu=True, pool=pool, out=buf(which, hh, ww, p[name][1].shape[0]))
            which ^= 1
        return heads(x, *p["heads"])

    def extract(self, image: torch.Tensor, frontend: KeypointFrontend) -> Features:
        """frontend.extract(*self.heads(image)): fifteen launches from images to Features."""
        return frontend.extract(*self.heads(image))


def extract_pairs(encoder: SuperPointEncoder, frontend: KeypointFrontend, images0: torch.Tensor,
                  images1: torch.Tensor) -> Tuple[Features, Features]:
    """The Features of both sides of P image pairs (images0[p], images1[p]; both [P, 1, H, W] or [P, H, W], one
    size): one encoder pass and one extract over the 2 P images, then the two halves."""
    if images0.shape != images1.shape or images0.dtype != images1.dtype:
        raise ValueError(f"match_images: the two image batches must agree in shape and dtype, got {tuple(images0.shape)} "
                         f"{images0.dtype} and {tuple(images1.shape)} {images1.dtype}")
    pairs = images0.shape[0]
    f = encoder.extract(torch.cat([images0, images1]), frontend)
    return f.rows(slice(0, pairs)), f.rows(slice(pairs, None))


def match_images(encoder: SuperPointEncoder, frontend: KeypointFrontend, matcher, images0: torch.Tensor,
                 images1: torch.Tensor):
    """The matches of P image pairs: matcher.match_features on extract_pairs' two halves. Nothing is read
    back, so the whole enqueues, or is captured, as one piece."""
    return matcher.match_features(*extract_pairs(encoder, frontend, images0, images1))


# ---- the same forward in framework ops (the tests' oracle) ------------------------------------------------
def superpoint_reference(state_dict: Dict[str, torch.Tensor], image: torch.Tensor, storage: Optional[torch.dtype] = None,
                         compute: torch.dtype = torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """superpoint.py:143-172 up to convPb's and convDb's outputs: image [B, 1, H, W] or [B, H, W] -> (logits
    [B, 65, H/8, W/8], dense [B, 256, H/8, W/8]) in `compute`, on the image's device. storage=None: the
    reference's chain of ops as it stands. storage=torch.float16: weights, biases and every layer's output
    are rounded to fp16 (the kernels' model); the arithmetic between two roundings is done in `compute`."""
    s = _checked_state(state_dict)

    def rnd(t: torch.Tensor) -> torch.Tensor:
        return t if storage is None else t.to(storage).to(compute)

    def conv(x: torch.Tensor, name: str, relu: bool = True) -> torch.Tensor:
        wt = rnd(s[f"{name}.weight"].to(image.device, compute))
        bs = rnd(s[f"{name}.bias"].to(image.device, compute))
        y = F.conv2d(x, wt, bs, stride=1, padding=wt.shape[-1] // 2)
        return rnd(F.relu(y) if relu else y)

    x = image[:, None] if image.dim() == 3 else image
    x = x.to(compute)
    x = conv(conv(x, "conv1a"), "conv1b")
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = conv(conv(x, "conv2a"), "conv2b")
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = conv(conv(x, "conv3a"), "conv3b")
    x = F.max_pool2d(x, kernel_size=2, stride=2)
    x = conv(conv(x, "conv4a"), "conv4b")
    logits = conv(conv(x, "convPa"), "convPb", relu=False)
    dense = conv(conv(x, "convDa"), "convDb", relu=False)
    return logits, dense


def seeded_superpoint_state_dict(seed: int) -> Dict[str, torch.Tensor]:
    """He-normal weights (std sqrt(2 / fan_in)) and biases of std 0.1 from synth's generator: identical on every
    machine. With it the logits and descriptors of uniform [0, 1) images stay within +-6: nothing saturates."""
    out = {}
    for name, (cout, cin, k) in LAYERS.items():
        for key, shape, std in ((f"{name}.weight", (cout, cin, k, k), float(np.sqrt(2.0 / (cin * k * k)))),
                                (f"{name}.bias", (cout,), 0.1)):
            s = (seed * 1_000_003 + zlib.crc32(key.encode())) & 0x7FFFFFFF
            out[key] = torch.from_numpy(np.ascontiguousarray(synth.normal(s, shape, std), dtype=np.float32))
    return out
