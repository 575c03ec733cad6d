"""Derived weights of the hip path, cached on the module that owns their sources: the message projection
folded into the FFN's first layer, the one-launch FFN's packed weight streams, the stacked cross
projection and Wqkv in the fused kernel's row order."""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn


def _cached(module: nn.Module, name: str, params: Sequence[torch.Tensor], dtype: torch.dtype, build):
    """Derived weights cached on `module`, rebuilt when any source parameter changes (in-place
    updates bump ``_version``; load_state_dict does) or the dtype/device differs."""
    key = (dtype, params[0].device, tuple(p._version for p in params), tuple(p.data_ptr() for p in params))
    hit = module.__dict__.get(name)
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        val = tuple(t.to(dtype).contiguous() for t in build())
    module.__dict__[name] = (key, val)
    return val


def _ffn_in_fused(block: nn.Module, proj: nn.Linear, dtype: torch.dtype):
    """The block's message projection folded into the FFN's first layer (hip path):
    ffn0(cat(x, proj(m))) = cat(x, m) @ [W_x | W_m·W_p]ᵀ + (b + W_m·b_p), computed in fp32.
    (lightglue.py:104-106, 181-183: the projection feeds only the FFN.)"""
    lin = block.ffn[0]

    def build():
        d = proj.weight.shape[0]
        w = lin.weight.float()
        wx, wm = w[:, :d], w[:, d:]
        return (torch.cat((wx, wm @ proj.weight.float()), 1), lin.bias.float() + wm @ proj.bias.float())

    return _cached(block, "_ffn_in_fused", (lin.weight, lin.bias, proj.weight, proj.bias), dtype, build)


def ffn_pack(w1: torch.Tensor, w2: torch.Tensor, w3: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The one-launch FFN's weight streams (lg_ffn_pack, include/lightglue_glue.h) by tensor ops, the
    32-row kernel's layout then the 16-row kernel's. 32-row: for wave w of 8, W1 rows 64w.. as pieces
    (step j, block b), then W2 rows 32w.. as pieces (step j), then (lg_linear_cat_ffn_proj) W3 rows
    (n3/8)w.. as pieces (step j, block b); each piece's 16-B lane l = W[row0 + 32b + l % 32][16j +
    8(l // 32) : + 8]. 16-row: the same rows per wave in 16-row blocks and k32 steps, lane l =
    W[row0 + 16b + l % 16][32j + 8(l // 16) : + 8]."""
    def layout(rows, k):  # W [8 waves * blocks * rows, steps * k] -> (w, step, block, lane group, row, e)
        def f(w):
            nb = w.shape[0] // (8 * rows)
            g = k // 8
            return w.reshape(8, nb, rows, w.shape[1] // k, g, 8).permute(0, 3, 1, 4, 2, 5).reshape(8, -1)
        return f
    parts32 = [layout(32, 16)(w1), layout(32, 16)(w2)]
    parts16 = [layout(16, 32)(w1), layout(16, 32)(w2)]
    if w3 is not None:
        parts32.append(layout(32, 16)(w3))
        parts16.append(layout(16, 32)(w3))
    return torch.cat([torch.cat(parts32, 1).reshape(-1), torch.cat(parts16, 1).reshape(-1)]).contiguous()


def _ffn_packed(block: nn.Module, proj: nn.Linear, dtype: torch.dtype, w3=None):
    """ffn_pack of the block's folded FFN input weight and its output weight (cached like them), and
    with w3 = (tag, source parameters, builder of W3) the next projection's weight appended."""
    lin, out = block.ffn[0], block.ffn[3]
    tag, src, w3_build = w3 if w3 is not None else ("", (), None)

    def build():
        w, _ = _ffn_in_fused(block, proj, dtype)
        return (ffn_pack(w, out.weight.to(dtype), w3_build().to(dtype) if w3_build else None),)

    return _cached(block, "_ffn_packed" + tag, (lin.weight, lin.bias, proj.weight, proj.bias, out.weight) + tuple(src), dtype,
                   build)[0]


def _cross_qkv(ca: nn.Module, dtype: torch.dtype):
    """CrossBlock to_qk | to_v stacked (one projection; lightglue.py:158-166)."""
    return _cached(ca, "_qkv_stacked", (ca.to_qk.weight, ca.to_qk.bias, ca.to_v.weight, ca.to_v.bias), dtype,
                   lambda: (torch.cat((ca.to_qk.weight, ca.to_v.weight), 0), torch.cat((ca.to_qk.bias, ca.to_v.bias), 0)))


def _qkv_perm(block: nn.Module, dtype: torch.dtype):
    """Wqkv's rows and bias in [q|k|v][head][dim] order (lg_linear_qkv_rotary's layout): new row
    j*H*64 + h*64 + d = reference row (h*64 + d)*3 + j (lightglue.py:111-114)."""
    lin = block.Wqkv

    def build():
        hd = block.heads * block.head_dim
        new = torch.arange(3 * hd, device=lin.weight.device)
        j, hd_idx = new // hd, new % hd
        old = hd_idx * 3 + j
        return lin.weight[old], lin.bias[old]

    return _cached(block, "_qkv_perm", (lin.weight, lin.bias), dtype, build)
