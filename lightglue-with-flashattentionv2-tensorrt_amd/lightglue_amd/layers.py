"""The matcher's blocks (lightglue_pytorch_no_plugin/lightglue.py:32-233): the Fourier positional
encoding, SelfBlock, CrossBlock, TransformerLayer and MatchAssignment, each with the reference's math in
framework ops and its gfx950 forms. What differs from the reference, and why:
* attention runs on the gfx950 kernel through the grouped launcher: per layer ONE launch for the two
  self-attention calls and ONE for the two cross directions (the reference makes four plugin enqueues
  per layer, TransformerLayer :186-194);
* the projections and FFNs whose weights both images share run once on the two images' rows
  concatenated (half the launches, twice the GEMM height); q/k/v are produced head-major in one copy
  (the reference splits an interleaved [N, H, 64, 3] projection and transposes);
* the column log-softmax of the assignment runs on a contiguous transpose (the reference's strided
  ``log_softmax(sim, 1)``);
* on the hip path the layout / normalisation steps around the attention are gfx950 kernels (glue.py), and
  the fp16 layer is ``TransformerLayer.fused_step``, which every fast path launches."""
from __future__ import annotations

from typing import Callable, List, Sequence, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from .glue import _Hip
from .matches import MatchResult
from .plugin import PluginError
from .weights import _cached, _cross_qkv, _ffn_in_fused, _ffn_packed, _qkv_perm

AttnFn = Callable[[Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]], List[torch.Tensor]]


def _fused_ok(x: torch.Tensor, block: nn.Module) -> bool:
    """The fused-projection kernels: fp16, 4 x 64 heads (k = 256 / 512)."""
    return x.dtype == torch.float16 and block.heads * block.head_dim == 256 and x.shape[-1] == 256


def _ffn_tail(block: nn.Module, x: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
    """x + Linear(GELU(LayerNorm(h))) with LayerNorm+GELU as one gfx950 kernel."""
    return x + block.ffn[3](_Hip.layernorm_gelu(h, block.ffn[1]))


def _ffn_apply(ffn: nn.Sequential, h: torch.Tensor, hip: bool) -> torch.Tensor:
    """Linear -> LayerNorm -> GELU -> Linear (the LN+GELU pair is one gfx950 kernel on the hip path)."""
    if not hip:
        return ffn(h)
    return ffn[3](_Hip.layernorm_gelu(ffn[0](h), ffn[1]))


def _kernel_attention(calls):
    for q, _, _ in calls:
        if not q.is_cuda:
            raise PluginError("LightGlueMatcher: the attention op runs on the GPU only (no CPU fallback)")
    qs, ks, vs = (list(t) for t in zip(*calls))
    return torch.ops.lightglue_amd.mha_hd64_grouped(qs, ks, vs)  # ops.py: grouped launches


def _kernel_attention_lens(calls, q_lens, kv_lens):
    """_kernel_attention on a ragged batch: q_lens[i] / kv_lens[i] (int32 [P] on the device) are call
    i's real query rows and keys. Keys past the count are never read; query rows past it are written
    as NaN and kept out of the decisions a wave takes for its 32 rows together, so a real row's bits
    depend on no padded row."""
    qs, ks, vs = (list(t) for t in zip(*calls))
    return torch.ops.lightglue_amd.mha_hd64_grouped_qkv_lens(qs, ks, vs, list(q_lens), list(kv_lens))  # ops.py


def _lens_attention(lens) -> Tuple[AttnFn, AttnFn]:
    """(self, cross) attention of a ragged batch: image i's rows end at lens[i]; self attention reads
    the keys of its own image, cross attention the other's."""
    return (lambda calls: _kernel_attention_lens(calls, lens, (lens[0], lens[1])),
            lambda calls: _kernel_attention_lens(calls, lens, (lens[1], lens[0])))


class FourierPositionalEncoding(nn.Module):
    """lightglue.py:32-52: cos/sin of a learned projection of the keypoints, each repeated
    for the two members of a rotary pair. Returns (cos, sin), each [1, 1, N, head_dim]."""

    def __init__(self, m: int = 2, head_dim: int = 64) -> None:
        super().__init__()
        self.Wr = nn.Linear(m, head_dim // 2, bias=False)

    def forward(self, kpts: torch.Tensor):
        proj = self.Wr(kpts)                                   # [1, N, head_dim/2]
        cos = torch.cos(proj).repeat_interleave(2, dim=-1)     # (c0, c0, c1, c1, ...)
        sin = torch.sin(proj).repeat_interleave(2, dim=-1)
        return cos.unsqueeze(1), sin.unsqueeze(1)


def _rotary(t: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """t * cos + swap(t) * sin with swap((x0, x1)) = (-x1, x0) on consecutive pairs
    (lightglue.py:124-134)."""
    pairs = t.unflatten(-1, (-1, 2))
    swapped = torch.stack((-pairs[..., 1], pairs[..., 0]), dim=-1).flatten(-2)
    return t * cos + swapped * sin


def _ffn(d: int) -> nn.Sequential:
    return nn.Sequential(nn.Linear(2 * d, 2 * d), nn.LayerNorm(2 * d, elementwise_affine=True), nn.GELU(),
                         nn.Linear(2 * d, d))


class SelfBlock(nn.Module):
    """lightglue.py:88-134 (weights shared by both images of a pair)."""

    def __init__(self, d: int, heads: int) -> None:
        super().__init__()
        self.heads, self.head_dim = heads, d // heads
        self.Wqkv = nn.Linear(d, 3 * d)
        self.out_proj = nn.Linear(d, d)
        self.ffn = _ffn(d)

    def qkv(self, x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, splits: Sequence[int], hip: bool = False):
        """x [1, N0+N1, d] (both images' rows) -> per image (q, k, v), each [1, H, Ni, 64]."""
        n = x.shape[1]
        if hip:
            return _Hip.qkv_rotary_split(self.Wqkv(x), cos, sin, self.heads, splits)
        # Wqkv output channel (h*64 + d)*3 + j  ->  [3, H, N, 64] head-major
        t = self.Wqkv(x).view(n, self.heads, self.head_dim, 3).permute(3, 1, 0, 2)
        q = _rotary(t[0], cos, sin)
        k = _rotary(t[1], cos, sin)
        out, a = [], 0
        for ni in splits[:2]:
            out.append(tuple(u[:, a:a + ni].unsqueeze(0).contiguous() for u in (q, k, t[2])))
            a += ni
        return out

    def finish(self, x: torch.Tensor, contexts: Sequence[torch.Tensor], hip: bool = False) -> torch.Tensor:
        if hip:  # [x | heads merged] in one pass, out_proj folded into ffn[0]
            w, b = _ffn_in_fused(self, self.out_proj, x.dtype)
            return _ffn_tail(self, x, F.linear(_Hip.merge_heads_cat(x, *contexts), w, b))
        merged = torch.cat([c[0].transpose(0, 1).reshape(c.shape[2], -1) for c in contexts], 0)[None]
        return x + _ffn_apply(self.ffn, torch.cat((x, self.out_proj(merged)), -1), hip)


class CrossBlock(nn.Module):
    """lightglue.py:137-183: shared q/k projection, both directions."""

    def __init__(self, d: int, heads: int) -> None:
        super().__init__()
        self.heads, self.head_dim = heads, d // heads
        self.to_qk = nn.Linear(d, d)
        self.to_v = nn.Linear(d, d)
        self.to_out = nn.Linear(d, d)
        self.ffn = _ffn(d)

    def heads_of(self, t: torch.Tensor, splits: Sequence[int]) -> List[torch.Tensor]:
        """[1, N0+N1, d] -> per image [1, H, Ni, 64]."""
        h = t[0].view(t.shape[1], self.heads, self.head_dim).transpose(0, 1)
        out, a = [], 0
        for ni in splits[:2]:
            out.append(h[:, a:a + ni].unsqueeze(0).contiguous())
            a += ni
        return out

    def qk_v(self, x: torch.Tensor, splits: Sequence[int]):
        """hip path: to_qk and to_v as ONE GEMM on stacked weights, heads split from its halves."""
        w, b = _cross_qkv(self, x.dtype)
        return _Hip.split_heads2_ld(F.linear(x, w, b), self.heads, splits)

    def finish(self, x: torch.Tensor, ms: Sequence[torch.Tensor], hip: bool = False) -> torch.Tensor:
        if hip:  # [x | heads merged] in one pass, to_out folded into ffn[0]
            w, b = _ffn_in_fused(self, self.to_out, x.dtype)
            return _ffn_tail(self, x, F.linear(_Hip.merge_heads_cat(x, *ms), w, b))
        merged = torch.cat([m[0].transpose(0, 1).reshape(m.shape[2], -1) for m in ms], 0)[None]
        return x + _ffn_apply(self.ffn, torch.cat((x, self.to_out(merged)), -1), hip)


class TransformerLayer(nn.Module):
    def __init__(self, d: int, heads: int) -> None:
        super().__init__()
        self.self_attn = SelfBlock(d, heads)
        self.cross_attn = CrossBlock(d, heads)

    def forward(self, x, cos, sin, splits, attention: AttnFn, hip: bool = False):
        """x: both images' descriptors [1, N0+N1, d] (image 0 rows first)."""
        sa, ca = self.self_attn, self.cross_attn
        if hip and _fused_ok(x, sa):
            return self._forward_fused(x, cos, sin, splits, attention)
        x = sa.finish(x, attention(sa.qkv(x, cos, sin, splits, hip)), hip)   # one grouped launch (self0, self1)
        if hip:
            (qk0, qk1), (v0, v1) = ca.qk_v(x, splits)
        else:
            qk0, qk1 = ca.heads_of(ca.to_qk(x), splits)
            v0, v1 = ca.heads_of(ca.to_v(x), splits)
        return ca.finish(x, attention([(qk0, qk1, v1), (qk1, qk0, v0)]), hip)  # one grouped launch (cross)

    def _forward_fused(self, x, cos, sin, splits, attention: AttnFn):
        """The fp16 hip layer on its own (no chain): fused_step with nothing folded."""
        return self.fused_step(x, cos, sin, splits, None, attention, attention)[0]

    def fused_step(self, x, cos, sin, splits, qkv, attn_self: AttnFn, attn_cross: AttnFn, fold_cross: bool = False,
                   then=None):
        """The fp16 hip layer: self attention on `qkv` (None: this layer's Wqkv + rotary), the self block's
        FFN, cross attention, the cross block's FFN. Each FFN is one launch with its residual
        (lg_linear_cat_ffn with the packed weight stream; the message projection is folded into its
        first weight) and may also project its output for what follows (lg_linear_cat_ffn_proj): with
        fold_cross the self block's FFN carries to_qk | to_v (kind 1); the cross block's FFN carries, for
        `then` the next layer's SelfBlock, its Wqkv + rotary (kind 2), for `then` a MatchAssignment its
        [W_final / scale ; w_match] (kind 3). Folded and unfolded forms are bitwise equal.
        Returns (x, the next layer's qkv or None, the head's projected rows [1, M, 384] or None)."""
        sa, ca, dt = self.self_attn, self.cross_attn, x.dtype
        if qkv is None:
            wq, bq = _qkv_perm(sa, dt)
            qkv = _Hip.linear_qkv_rotary(x, wq, bq, cos, sin, sa.heads, splits)
        c0, c1 = attn_self(qkv)                                               # self0, self1: one launch
        w0, b0 = _ffn_in_fused(sa, sa.out_proj, dt)
        wc, bc = _cross_qkv(ca, dt)
        if fold_cross:
            pk = _ffn_packed(sa, sa.out_proj, dt, ("_x", (ca.to_qk.weight, ca.to_qk.bias, ca.to_v.weight, ca.to_v.bias),
                                                   lambda: _cross_qkv(ca, dt)[0]))
            x, ((qk0, qk1), (v0, v1)) = _Hip.ffn_proj(x, c0, c1, b0, sa.ffn[1], sa.ffn[3].bias, pk, 1, bc, splits)
        else:
            x = _Hip.ffn(x, c0, c1, w0, b0, sa.ffn[1], sa.ffn[3].weight, sa.ffn[3].bias, _ffn_packed(sa, sa.out_proj, dt))
            (qk0, qk1), (v0, v1) = _Hip.linear_split2(x, wc, bc, ca.heads, splits)
        m0, m1 = attn_cross([(qk0, qk1, v1), (qk1, qk0, v0)])              # cross: one launch
        w0, b0 = _ffn_in_fused(ca, ca.to_out, dt)
        if isinstance(then, SelfBlock):
            _, bq = _qkv_perm(then, dt)
            pk = _ffn_packed(ca, ca.to_out, dt, ("_q", (then.Wqkv.weight, then.Wqkv.bias), lambda: _qkv_perm(then, dt)[0]))
            x, qkv = _Hip.ffn_proj(x, m0, m1, b0, ca.ffn[1], ca.ffn[3].bias, pk, 2, bq, splits, cos, sin)
            return x, qkv, None
        if then is not None:
            _, b3 = then.aug_weights(dt, 512)
            hp = (then.final_proj.weight, then.final_proj.bias, then.matchability.weight, then.matchability.bias)
            pk = _ffn_packed(ca, ca.to_out, dt, ("_h", hp, lambda: then.aug_weights(dt, 512)[0]))
            x, v = _Hip.ffn_proj(x, m0, m1, b0, ca.ffn[1], ca.ffn[3].bias, pk, 3, b3, splits, n_store=384)
            return x, None, v
        x = _Hip.ffn(x, m0, m1, w0, b0, ca.ffn[1], ca.ffn[3].weight, ca.ffn[3].bias, _ffn_packed(ca, ca.to_out, dt))
        return x, None, None


def log_double_softmax(sim: torch.Tensor, z0: torch.Tensor, z1: torch.Tensor) -> torch.Tensor:
    """lightglue.py:197-205: log_softmax over both axes plus the matchability log-sigmoids
    (the column pass on a contiguous transpose)."""
    col = F.log_softmax(sim.transpose(1, 2).contiguous(), 2).transpose(1, 2)
    return F.log_softmax(sim, 2) + col + F.logsigmoid(z0) + F.logsigmoid(z1).transpose(1, 2)


class MatchAssignment(nn.Module):
    """lightglue.py:208-233."""

    def __init__(self, d: int) -> None:
        super().__init__()
        self.scale = d ** 0.25
        self.final_proj = nn.Linear(d, d)
        self.matchability = nn.Linear(d, 1)

    def hip16_ok(self, x: torch.Tensor, m: int, n: int) -> bool:
        return x.dtype == torch.float16 and x.is_cuda and x.shape[-1] == 256 and n % 8 == 0 and n <= 2048 and m <= 2048

    def aug_weights(self, dtype: torch.dtype, rows: int = 384):
        """[W_final / scale ; w_match ; 0] [rows, d] and its bias (the head's one projection, cached)."""
        fp, mt = self.final_proj, self.matchability
        d = fp.weight.shape[1]

        def build():
            w = torch.zeros((rows, d), dtype=torch.float32, device=fp.weight.device)
            b = torch.zeros((rows,), dtype=torch.float32, device=fp.weight.device)
            w[:d], b[:d] = fp.weight.float() / self.scale, fp.bias.float() / self.scale
            w[d], b[d] = mt.weight.float()[0], mt.bias.float()[0]
            return w, b

        return _cached(self, f"_assign_aug{rows}", (fp.weight, fp.bias, mt.weight, mt.bias), dtype, build)

    def project_rows(self, x: torch.Tensor, pr: int, m: int, n: int) -> torch.Tensor:
        """The head's ONE projection of both images' rows x [1, P*(m+n), d] with [W_final / scale ;
        w_match ; 0] -> v [P, m + n, 384]: the scaled descriptors at channels 0..d-1, the matchability
        logit at channel d."""
        w, b = self.aug_weights(x.dtype, 384)
        return _Hip.linear(x, w, b).view(pr, m + n, 384)

    def forward_rows(self, x: torch.Tensor, pr: int, m: int, n: int) -> torch.Tensor:
        """fp16 hip path on both images' rows x [1, P*(m+n), d] at once: project_rows, then
        lg_assign_scores: the similarity of its fp16 halves by MFMA with each row's and column's
        logsumexp, and the combine (two launches, no framework op; lightglue.py:208-233). d^0.25 = 4 for
        d = 256, a power of two: dividing W and b by it is exact unless a quotient falls below 2^-14
        (fp16 subnormals), where it loses up to 2 bits; so the output equals the reference's
        fp16(final_proj(d)) / scale except for weights, biases or outputs that small, which differ by at
        most that subnormal rounding."""
        return _Hip.assign_scores(self.project_rows(x, pr, m, n), m, x.shape[-1])

    def matches_rows(self, x: torch.Tensor, pr: int, m: int, n: int, threshold: float) -> MatchResult:
        """forward_rows' projection, then lg_assign_matches: the matches of all P pairs without the
        scores tensor (filter_matches_dense's semantics on the scores forward_rows would return)."""
        return _Hip.assign_matches(self.project_rows(x, pr, m, n), m, x.shape[-1], threshold)

    def forward(self, d0: torch.Tensor, d1: torch.Tensor, hip: bool = False) -> torch.Tensor:
        m0 = self.final_proj(d0) / self.scale
        m1 = self.final_proj(d1) / self.scale
        sim = (m0 @ m1.transpose(1, 2)).float()
        z0, z1 = self.matchability(d0).float(), self.matchability(d1).float()
        if hip:
            return _Hip.log_double_softmax(sim.contiguous(), z0.contiguous(), z1.contiguous())
        return log_double_softmax(sim, z0, z1)
