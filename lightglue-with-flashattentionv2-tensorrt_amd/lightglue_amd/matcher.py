"""LightGlue matcher built around the MI355X attention op.

A restatement of the reference model (lightglue_pytorch_no_plugin/lightglue.py): input
projection, Fourier positional encoding applied as a rotary embedding (:32-52, :124-134),
``n_layers`` x (SelfBlock on each image with shared weights, CrossBlock in both directions)
(:88-194), MatchAssignment with the dual log-softmax (:197-233) and ``filter_matches``
(:236-262). Parameter names equal the reference's state-dict keys, so a reference checkpoint
(or ``seeded_state_dict``) loads unchanged.

What is different, and why:
* attention runs on the gfx950 kernel through the grouped launcher: per layer ONE launch for the
  two self-attention calls and ONE for the two cross directions (the reference makes four plugin
  enqueues per layer, TransformerLayer :186-194);
* the projections and FFNs whose weights both images share run once on the two images'
  rows concatenated (half the launches, twice the GEMM height); q/k/v are produced head-major
  in one copy (the reference splits an interleaved [N, H, 64, 3] projection and transposes);
* the column log-softmax of the assignment runs on a contiguous transpose (the reference's
  strided ``log_softmax(sim, 1)``);
* ``glue="hip"`` (default) runs the layout/normalisation steps around the attention on gfx950
  kernels (include/lightglue_glue.h: q/k/v split + rotary + per-image head-major layout in one
  pass, head split/merge, LayerNorm+GELU, the dual log-softmax); ``glue="torch"`` is the same
  math in framework ops (the restatement the CPU tests pin to the reference);
* ``match_batch`` returns the matches of all pairs of a forward as one ``MatchResult`` (the dense
  outputs ``filter_matches`` keeps commented out, :241-252, and the compacted list): on the fp16 hip
  path from ``lg_assign_matches``, which never writes the scores tensor; elsewhere from
  ``filter_matches_dense``, the same semantics in framework ops;
* ``forward`` / ``match_batch`` take per-pair keypoint counts (``counts0``, ``counts1``) for padded
  batches of pairs of different sizes, and ``match_pairs`` pads a list of pairs itself: on the fp16 hip
  path the equal-size forward's launches, with the counts as the attention's key and query-row counts
  and the heads' lens forms (no valid row's result reads a padded row); elsewhere pair by pair;
* ``match_adaptive`` (opt-in: ``depth_confidence`` / ``width_confidence`` > 0) applies the published
  LightGlue rules the reference ships the pieces of and never uses: a per-layer token confidence stops
  the forward early, a per-layer matchability drops points; ``adaptive_reference`` is the same in
  framework ops (the tests' oracle);
* ``match_features`` takes two ``frontend.Features`` (``KeypointFrontend``: SuperPoint's dense heads to
  keypoints, descriptors and device counts on gfx950 kernels) and is ``match_batch`` with those counts,
  pairs with an empty side masked on the device;
* ``attention=`` lets tests substitute the oracle for the kernel on CPU; the default path
  requires GPU tensors and fails loudly otherwise (no CPU fallback).
"""
from __future__ import annotations

import ctypes
import os
import zlib
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, synth
from .plugin import PluginError, _check, _workspace

AttnFn = Callable[[Sequence[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]]], List[torch.Tensor]]


_DT = {torch.float16: _lib.DT_HALF, torch.float32: _lib.DT_FLOAT}


def _sp(splits):
    """(n0, n1[, pairs]) -> (n0, n1, pairs): rows are `pairs` image pairs stacked pair-major."""
    return (splits[0], splits[1], splits[2] if len(splits) > 2 else 1)


class _Hip:
    """Thin wrappers of the gfx950 glue kernels (current stream, fail loudly on error). Row-major
    tensors hold P image pairs stacked pair-major ([1, P*(n0+n1), C]); per-image head-major
    tensors are [P, heads, ni, 64] (include/lightglue_glue.h)."""

    @staticmethod
    def _stream(t):
        return torch.cuda.current_stream(t.device).cuda_stream

    @staticmethod
    def qkv_rotary_split(qkv, cos, sin, heads, splits):
        n0, n1, pr = _sp(splits)
        mk = lambda n: torch.empty((pr, heads, n, 64), dtype=qkv.dtype, device=qkv.device)  # noqa: E731
        out = [tuple(mk(n) for _ in range(3)) for n in (n0, n1)]
        st = _lib.load().lg_qkv_rotary_split(_DT[qkv.dtype], qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), heads,
                                             n0, n1, pr, *(t.data_ptr() for t in out[0]),
                                             *(t.data_ptr() for t in out[1]), _Hip._stream(qkv))
        _check(st, "lg_qkv_rotary_split")
        return out

    @staticmethod
    def split_heads2(a, b, heads, splits):
        n0, n1, pr = _sp(splits)
        mk = lambda n: torch.empty((pr, heads, n, 64), dtype=a.dtype, device=a.device)  # noqa: E731
        a0, a1, b0, b1 = mk(n0), mk(n1), mk(n0), mk(n1)
        st = _lib.load().lg_split_heads2(_DT[a.dtype], a.data_ptr(), b.data_ptr(), heads, n0, n1, pr, a0.data_ptr(),
                                         a1.data_ptr(), b0.data_ptr(), b1.data_ptr(), _Hip._stream(a))
        _check(st, "lg_split_heads2")
        return (a0, a1), (b0, b1)

    @staticmethod
    def split_heads2_ld(ab, heads, splits):
        """ab [1, P*(N0+N1), 2*heads*64] = [a | b] (one GEMM's output) -> per image (a_i, b_i) heads."""
        n0, n1, pr = _sp(splits)
        mk = lambda n: torch.empty((pr, heads, n, 64), dtype=ab.dtype, device=ab.device)  # noqa: E731
        a0, a1, b0, b1 = mk(n0), mk(n1), mk(n0), mk(n1)
        half = heads * 64
        st = _lib.load().lg_split_heads2_ld(_DT[ab.dtype], ab.data_ptr(), ab.data_ptr() + half * ab.element_size(),
                                            2 * half, heads, n0, n1, pr, a0.data_ptr(), a1.data_ptr(), b0.data_ptr(),
                                            b1.data_ptr(), _Hip._stream(ab))
        _check(st, "lg_split_heads2_ld")
        return (a0, a1), (b0, b1)

    @staticmethod
    def merge_heads_cat(x, x0, x1):
        """[x | merge_heads(x0, x1)] -> [1, P*(N0+N1), 2*heads*64] (the FFN input)."""
        pr, heads, n0, n1 = x0.shape[0], x0.shape[1], x0.shape[2], x1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), 2 * heads * 64), dtype=x.dtype, device=x.device)
        st = _lib.load().lg_merge_heads_cat(_DT[x.dtype], x.data_ptr(), x0.data_ptr(), x1.data_ptr(), heads, n0, n1,
                                            pr, out.data_ptr(), _Hip._stream(x))
        _check(st, "lg_merge_heads_cat")
        return out

    # ---- projections with their neighbours fused (fp16; csrc/lightglue_linear.hip, lightglue_ffn.hip) ----
    @staticmethod
    def linear(a, w, b, res=None):
        """a [1, M, K] -> a·wᵀ + b (+ res) [1, M, N]."""
        m, k = a.shape[1], a.shape[2]
        out = torch.empty((1, m, w.shape[0]), dtype=a.dtype, device=a.device)
        st = _lib.load().lg_linear(a.data_ptr(), w.data_ptr(), b.data_ptr(), res.data_ptr() if res is not None else None,
                                   m, w.shape[0], k, out.data_ptr(), _Hip._stream(a))
        _check(st, "lg_linear")
        return out

    @staticmethod
    def linear_cat(x, c0, c1, w, b):
        """[x | merge_heads(c0, c1)]·wᵀ + b."""
        pr, heads, n0, n1 = c0.shape[0], c0.shape[1], c0.shape[2], c1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), w.shape[0]), dtype=x.dtype, device=x.device)
        st = _lib.load().lg_linear_cat(x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr, w.data_ptr(),
                                       b.data_ptr(), w.shape[0], out.data_ptr(), _Hip._stream(x))
        _check(st, "lg_linear_cat")
        return out

    @staticmethod
    def ffn(x, c0, c1, w, b, ln: nn.LayerNorm, w2, b2, packed=None):
        """x + ffn([x | merge_heads(c0, c1)]) (lightglue.py:101-106 with the block's residual):
        with `packed` (ffn_pack(w, w2)) one launch (ffn_rows_kernel), else linear_cat_ln_gelu into
        the scratch h, then linear(h, w2, b2, res=x) (include/lightglue_glue.h, lg_linear_set_ffn_fused)."""
        pr, heads, n0, n1 = c0.shape[0], c0.shape[1], c0.shape[2], c1.shape[2]
        m = pr * (n0 + n1)
        h = torch.empty((1, m, w.shape[0]), dtype=x.dtype, device=x.device)
        out = torch.empty((1, m, w2.shape[0]), dtype=x.dtype, device=x.device)
        st = _lib.load().lg_linear_cat_ffn(x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr,
                                           w.data_ptr(), b.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(),
                                           float(ln.eps), w2.data_ptr(), b2.data_ptr(),
                                           packed.data_ptr() if packed is not None else None, h.data_ptr(),
                                           out.data_ptr(), _Hip._stream(x))
        _check(st, "lg_linear_cat_ffn")
        return out

    @staticmethod
    def ffn_proj(x, c0, c1, b, ln: nn.LayerNorm, b2, packed, kind, b3, splits, cos=None, sin=None, n_store=0):
        """lg_linear_cat_ffn_proj: (x' = x + ffn([x | merge_heads(c0, c1)]), the next projection of x')
        in one launch; kind 1 -> ((a0, a1), (b0, b1)) per-image heads (to_qk | to_v), kind 2 -> q/k/v
        per image with the rotary, kind 3 -> [1, M, n_store] rows."""
        n0, n1, pr = _sp(splits)
        heads = c0.shape[1]
        m = pr * (n0 + n1)
        out = torch.empty((1, m, 256), dtype=x.dtype, device=x.device)
        mk = lambda n: torch.empty((pr, heads, n, 64), dtype=x.dtype, device=x.device)  # noqa: E731
        if kind == 1:
            outs = [mk(n0), mk(n1), mk(n0), mk(n1)]
        elif kind == 2:
            outs = [mk(n0), mk(n0), mk(n0), mk(n1), mk(n1), mk(n1)]
        else:
            outs = [torch.empty((1, m, n_store), dtype=x.dtype, device=x.device)]
        ptrs = (ctypes.c_void_p * 6)(*([t.data_ptr() for t in outs] + [None] * (6 - len(outs))))
        st = _lib.load().lg_linear_cat_ffn_proj(x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr, b.data_ptr(),
                                                ln.weight.data_ptr(), ln.bias.data_ptr(), float(ln.eps), b2.data_ptr(),
                                                packed.data_ptr(), kind, b3.data_ptr(),
                                                cos.data_ptr() if cos is not None else None,
                                                sin.data_ptr() if sin is not None else None, n_store, ptrs, out.data_ptr(),
                                                _Hip._stream(x))
        _check(st, "lg_linear_cat_ffn_proj")
        if kind == 1:
            return out, ((outs[0], outs[1]), (outs[2], outs[3]))
        if kind == 2:
            return out, [tuple(outs[:3]), tuple(outs[3:])]
        return out, outs[0]

    @staticmethod
    def linear_cat_ln_gelu(x, c0, c1, w, b, ln: nn.LayerNorm):
        """GELU(LayerNorm([x | merge_heads(c0, c1)]·wᵀ + b)) in one launch (P pairs of equal sizes)."""
        pr, heads, n0, n1 = c0.shape[0], c0.shape[1], c0.shape[2], c1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), w.shape[0]), dtype=x.dtype, device=x.device)
        st = _lib.load().lg_linear_cat_ln_gelu(x.data_ptr(), c0.data_ptr(), c1.data_ptr(), heads, n0, n1, pr,
                                               w.data_ptr(), b.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(),
                                               float(ln.eps), out.data_ptr(), _Hip._stream(x))
        _check(st, "lg_linear_cat_ln_gelu")
        return out

    @staticmethod
    def linear_qkv_rotary(x, w_perm, b_perm, cos, sin, heads, splits):
        n0, n1, pr = _sp(splits)
        mk = lambda n: torch.empty((pr, heads, n, 64), dtype=x.dtype, device=x.device)  # noqa: E731
        out = [tuple(mk(n) for _ in range(3)) for n in (n0, n1)]
        st = _lib.load().lg_linear_qkv_rotary(x.data_ptr(), w_perm.data_ptr(), b_perm.data_ptr(), cos.data_ptr(),
                                              sin.data_ptr(), heads, n0, n1, pr, x.shape[2],
                                              *(t.data_ptr() for t in out[0]), *(t.data_ptr() for t in out[1]),
                                              _Hip._stream(x))
        _check(st, "lg_linear_qkv_rotary")
        return out

    @staticmethod
    def linear_split2(x, w, b, heads, splits):
        n0, n1, pr = _sp(splits)
        mk = lambda n: torch.empty((pr, heads, n, 64), dtype=x.dtype, device=x.device)  # noqa: E731
        a0, a1, b0, b1 = mk(n0), mk(n1), mk(n0), mk(n1)
        st = _lib.load().lg_linear_split2(x.data_ptr(), w.data_ptr(), b.data_ptr(), heads, n0, n1, pr, x.shape[2],
                                          a0.data_ptr(), a1.data_ptr(), b0.data_ptr(), b1.data_ptr(), _Hip._stream(x))
        _check(st, "lg_linear_split2")
        return (a0, a1), (b0, b1)

    @staticmethod
    def merge_heads(x0, x1):
        pr, heads, n0, n1 = x0.shape[0], x0.shape[1], x0.shape[2], x1.shape[2]
        out = torch.empty((1, pr * (n0 + n1), heads * 64), dtype=x0.dtype, device=x0.device)
        st = _lib.load().lg_merge_heads(_DT[x0.dtype], x0.data_ptr(), x1.data_ptr(), heads, n0, n1, pr, out.data_ptr(),
                                        _Hip._stream(x0))
        _check(st, "lg_merge_heads")
        return out

    @staticmethod
    def layernorm_gelu(x, ln: nn.LayerNorm):
        y = torch.empty_like(x)
        rows, dim = x.numel() // x.shape[-1], x.shape[-1]
        st = _lib.load().lg_layernorm_gelu(_DT[x.dtype], x.data_ptr(), ln.weight.data_ptr(), ln.bias.data_ptr(), rows,
                                           dim, float(ln.eps), y.data_ptr(), _Hip._stream(x))
        _check(st, "lg_layernorm_gelu")
        return y

    @staticmethod
    def log_double_softmax(sim, z0, z1):
        """sim [P, m, n], z0 [P, m, 1], z1 [P, n, 1] (P pairs, one launch)."""
        pr, m, n = sim.shape[0], sim.shape[1], sim.shape[2]
        lib = _lib.load()
        out = torch.empty_like(sim)
        stream = _Hip._stream(sim)
        ws = _workspace(sim.device, stream, lib.lg_log_double_softmax_workspace(m, n, pr))
        st = lib.lg_log_double_softmax(sim.data_ptr(), z0.data_ptr(), z1.data_ptr(), m, n, pr, out.data_ptr(),
                                       ws.data_ptr(), stream)
        _check(st, "lg_log_double_softmax")
        return out


    @staticmethod
    def log_double_softmax_f16(sim, v, m, zc):
        """sim [P, m, n] fp16 (contiguous); the matchability logits at channel zc of v [P, m + n, C]
        (the assignment projection's output): one fp32 scores tensor [P, m, n], two launches."""
        pr, n, ch = sim.shape[0], sim.shape[2], v.shape[2]
        lib = _lib.load()
        out = torch.empty(sim.shape, dtype=torch.float32, device=sim.device)
        stream = _Hip._stream(sim)
        ws = _workspace(sim.device, stream, lib.lg_log_double_softmax_f16_workspace(m, n, pr))
        base = v.data_ptr() + zc * v.element_size()
        st = lib.lg_log_double_softmax_f16(sim.data_ptr(), base, base + m * ch * v.element_size(), (m + n) * ch, ch,
                                           m, n, pr, out.data_ptr(), ws.data_ptr(), stream)
        _check(st, "lg_log_double_softmax_f16")
        return out

    _last_assign_ws = None  # (tests read the similarity copy the kernel leaves in its workspace)

    @staticmethod
    def assign_scores(v, m, zc, lens=None):
        """v [P, m + n, C] fp16: the assignment projection of both images' rows (scaled descriptors at
        channels 0..255, the matchability logit at zc) -> fp32 scores [P, m, n] (lg_assign_scores: the
        similarity and the dual log-softmax in two launches). lens = (m_len, n_len), int32 [P] on the
        device: the ragged form (lg_assign_scores_lens; -inf on padded rows and columns)."""
        pr, n, ch = v.shape[0], v.shape[1] - m, v.shape[2]
        lib = _lib.load()
        out = torch.empty((pr, m, n), dtype=torch.float32, device=v.device)
        stream = _Hip._stream(v)
        ws = _workspace(v.device, stream, lib.lg_assign_scores_workspace(m, n, pr))
        _Hip._last_assign_ws = ws
        if lens is not None:
            st = lib.lg_assign_scores_lens(v.data_ptr(), (m + n) * ch, ch, zc, m, n, pr, lens[0].data_ptr(),
                                           lens[1].data_ptr(), out.data_ptr(), ws.data_ptr(), stream)
            _check(st, "lg_assign_scores_lens")
            return out
        st = lib.lg_assign_scores(v.data_ptr(), (m + n) * ch, ch, zc, m, n, pr, out.data_ptr(), ws.data_ptr(), stream)
        _check(st, "lg_assign_scores")
        return out

    @staticmethod
    def assign_matches(v, m, zc, threshold, lens=None):
        """v as for assign_scores -> MatchResult for all P pairs (lg_assign_matches: at most three
        launches, no fp32 scores tensor, no framework op, no host synchronisation). lens as for
        assign_scores (lg_assign_matches_lens: -1 / 0 on padded rows and columns)."""
        pr, n, ch = v.shape[0], v.shape[1] - m, v.shape[2]
        k = min(m, n)
        lib = _lib.load()
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=v.device)    # noqa: E731
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=v.device)  # noqa: E731
        out = MatchResult(i32(pr, m), i32(pr, n), f32(pr, m), f32(pr, n), i32(pr, k, 2), f32(pr, k), i32(pr))
        stream = _Hip._stream(v)
        ws = _workspace(v.device, stream, lib.lg_assign_matches_workspace(m, n, pr))
        if lens is not None:
            st = lib.lg_assign_matches_lens(v.data_ptr(), (m + n) * ch, ch, zc, m, n, pr, lens[0].data_ptr(),
                                            lens[1].data_ptr(), float(threshold), out.matches0.data_ptr(),
                                            out.matches1.data_ptr(), out.scores0.data_ptr(), out.scores1.data_ptr(),
                                            out.matches.data_ptr(), out.match_scores.data_ptr(), out.counts.data_ptr(),
                                            ws.data_ptr(), stream)
            _check(st, "lg_assign_matches_lens")
            return out
        st = lib.lg_assign_matches(v.data_ptr(), (m + n) * ch, ch, zc, m, n, pr, float(threshold), out.matches0.data_ptr(),
                                   out.matches1.data_ptr(), out.scores0.data_ptr(), out.scores1.data_ptr(),
                                   out.matches.data_ptr(), out.match_scores.data_ptr(), out.counts.data_ptr(),
                                   ws.data_ptr(), stream)
        _check(st, "lg_assign_matches")
        return out

    # ---- adaptive depth / width (csrc/lightglue_adaptive.hip) ----
    @staticmethod
    def token_scores(x, m, n, pr, lens, w_tok, b_tok, w_match, b_match, t_conf, t_keep, flags):
        """lg_token_scores on x [1, P*(m+n), 256]: (conf, mtch fp32 [P, m+n], keep uint8 [P, m+n], stats
        int32 [P, 4] = (kept0, kept1, unconfident, valid))."""
        dev = x.device
        conf = torch.empty((pr, m + n), dtype=torch.float32, device=dev)
        mtch = torch.empty_like(conf)
        keep = torch.empty((pr, m + n), dtype=torch.uint8, device=dev)
        stats = torch.empty((pr, 4), dtype=torch.int32, device=dev)
        l0, l1 = (t.data_ptr() if t is not None else None for t in (lens if lens is not None else (None, None)))
        st = _lib.load().lg_token_scores(x.data_ptr(), m, n, pr, l0, l1, w_tok.data_ptr(), b_tok.data_ptr(),
                                         w_match.data_ptr(), b_match.data_ptr(), float(t_conf), float(t_keep), int(flags),
                                         conf.data_ptr(), mtch.data_ptr(), keep.data_ptr(), stats.data_ptr(), _Hip._stream(x))
        _check(st, "lg_token_scores")
        return conf, mtch, keep, stats

    @staticmethod
    def compact_rows(x, cos, sin, keep, ind, m, n, pr, lens, m_out, n_out, prune=None, layers=0):
        """lg_compact_rows: the kept rows of x / cos / sin and of the index maps ind = (ind0, ind1) (None:
        identity) in the layout (m_out, n_out): (x, cos, sin, (ind0, ind1), (len0, len1)). prune = (prune0
        [P, m_orig], prune1 [P, n_orig]): the dropped rows' entries are set to `layers`."""
        dev = x.device
        rows = pr * (m_out + n_out)
        xo = torch.empty((1, rows, x.shape[2]), dtype=x.dtype, device=dev)
        co = torch.empty((1, rows, cos.shape[2]), dtype=cos.dtype, device=dev)
        so = torch.empty_like(co)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)  # noqa: E731
        i0, i1, l0, l1 = i32(pr, m_out), i32(pr, n_out), i32(pr), i32(pr)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        lens = lens if lens is not None else (None, None)
        p0, p1 = prune if prune is not None else (None, None)
        st = _lib.load().lg_compact_rows(x.data_ptr(), cos.data_ptr(), sin.data_ptr(), keep.data_ptr(), ptr(ind[0]),
                                         ptr(ind[1]), m, n, pr, ptr(lens[0]), ptr(lens[1]), m_out, n_out, xo.data_ptr(),
                                         co.data_ptr(), so.data_ptr(), i0.data_ptr(), i1.data_ptr(), l0.data_ptr(),
                                         l1.data_ptr(), ptr(p0), ptr(p1), p0.shape[1] if p0 is not None else 0,
                                         p1.shape[1] if p1 is not None else 0, int(layers), _Hip._stream(x))
        _check(st, "lg_compact_rows")
        return xo, co, so, (i0, i1), (l0, l1)

    @staticmethod
    def matches_scatter(r, ind, lens, m, n, stop, prune=None):
        """lg_matches_scatter: the MatchResult r of the surviving rows (layout r.matches0.shape[1] x
        r.matches1.shape[1]) in the original layout m x n; prune's surviving entries are set to `stop`."""
        pr, mc, nc = r.matches0.shape[0], r.matches0.shape[1], r.matches1.shape[1]
        dev, k = r.matches0.device, min(m, n)
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)    # noqa: E731
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731
        out = MatchResult(i32(pr, m), i32(pr, n), f32(pr, m), f32(pr, n), i32(pr, k, 2), f32(pr, k), i32(pr))
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        ind = ind if ind is not None else (None, None)
        lens = lens if lens is not None else (None, None)
        p0, p1 = prune if prune is not None else (None, None)
        st = _lib.load().lg_matches_scatter(*(t.data_ptr() for t in r), ptr(ind[0]), ptr(ind[1]), ptr(lens[0]), ptr(lens[1]),
                                            mc, nc, m, n, pr, int(stop), *(t.data_ptr() for t in out), ptr(p0), ptr(p1),
                                            _Hip._stream(r.matches0))
        _check(st, "lg_matches_scatter")
        return out

    @staticmethod
    def pair_inputs(desc0, desc1, kpts0, kpts1, wr):
        """x [1, P*(m+n), 256] pair-major and the rotary tables cos, sin [1, P*(m+n), 64] in one launch."""
        pr, m, n, d = desc0.shape[0], desc0.shape[1], desc1.shape[1], desc0.shape[2]
        rows = pr * (m + n)
        x = torch.empty((1, rows, d), dtype=desc0.dtype, device=desc0.device)
        cos = torch.empty((1, rows, 64), dtype=desc0.dtype, device=desc0.device)
        sin = torch.empty_like(cos)
        t = [u.contiguous() for u in (desc0, desc1, kpts0, kpts1, wr)]
        st = _lib.load().lg_pair_inputs(*(u.data_ptr() for u in t), m, n, pr, d, x.data_ptr(), cos.data_ptr(),
                                        sin.data_ptr(), _Hip._stream(desc0))
        _check(st, "lg_pair_inputs")
        return x, cos, sin


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
        w, b = _cached(self, "_qkv_stacked", (self.to_qk.weight, self.to_qk.bias, self.to_v.weight, self.to_v.bias),
                       x.dtype, lambda: (torch.cat((self.to_qk.weight, self.to_v.weight), 0),
                                         torch.cat((self.to_qk.bias, self.to_v.bias), 0)))
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
        """fp16 hip path per block: projection (+rotary/head split), grouped attention, and the FFN
        with its residual in one launch (lg_linear_cat_ffn with the packed weight stream: the input
        projection gathering [x | heads], LayerNorm+GELU, the output projection + residual); the
        message projection is folded into the FFN's first weight."""
        sa, ca = self.self_attn, self.cross_attn
        wq, bq = _qkv_perm(sa, x.dtype)
        qkv = _Hip.linear_qkv_rotary(x, wq, bq, cos, sin, sa.heads, splits)
        c0, c1 = attention(qkv)                                          # self0, self1: one launch
        w0, b0 = _ffn_in_fused(sa, sa.out_proj, x.dtype)
        x = _Hip.ffn(x, c0, c1, w0, b0, sa.ffn[1], sa.ffn[3].weight, sa.ffn[3].bias, _ffn_packed(sa, sa.out_proj, x.dtype))
        wc, bc = _cross_qkv(ca, x.dtype)
        (qk0, qk1), (v0, v1) = _Hip.linear_split2(x, wc, bc, ca.heads, splits)
        m0, m1 = attention([(qk0, qk1, v1), (qk1, qk0, v0)])            # cross: one launch
        w0, b0 = _ffn_in_fused(ca, ca.to_out, x.dtype)
        return _Hip.ffn(x, m0, m1, w0, b0, ca.ffn[1], ca.ffn[3].weight, ca.ffn[3].bias, _ffn_packed(ca, ca.to_out, x.dtype))


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

    def forward_rows(self, x: torch.Tensor, pr: int, m: int, n: int) -> torch.Tensor:
        """fp16 hip path on both images' rows x [1, P*(m+n), d] at once: ONE projection with
        [W_final / scale ; w_match ; 0], then lg_assign_scores: the similarity of its fp16 halves by
        MFMA with each row's and column's logsumexp, and the combine (two launches, no framework op;
        lightglue.py:208-233). d^0.25 = 4 for d = 256, a power of two: dividing W and b by it is
        exact unless a quotient falls below 2^-14 (fp16 subnormals), where it loses up to 2 bits; so
        the output equals the reference's fp16(final_proj(d)) / scale except for weights, biases or
        outputs that small, which differ by at most that subnormal rounding."""
        d = x.shape[-1]
        w, b = self.aug_weights(x.dtype, 384)
        v = _Hip.linear(x, w, b).view(pr, m + n, 384)
        return _Hip.assign_scores(v, m, d)   # sim (fp16) and the dual log-softmax: two launches

    def matches_rows(self, x: torch.Tensor, pr: int, m: int, n: int, threshold: float) -> "MatchResult":
        """forward_rows' projection, then lg_assign_matches: the matches of all P pairs without the
        scores tensor (filter_matches_dense's semantics on the scores forward_rows would return)."""
        d = x.shape[-1]
        w, b = self.aug_weights(x.dtype, 384)
        v = _Hip.linear(x, w, b).view(pr, m + n, 384)
        return _Hip.assign_matches(v, m, d, threshold)

    def forward(self, d0: torch.Tensor, d1: torch.Tensor, hip: bool = False) -> torch.Tensor:
        m0 = self.final_proj(d0) / self.scale
        m1 = self.final_proj(d1) / self.scale
        sim = (m0 @ m1.transpose(1, 2)).float()
        z0, z1 = self.matchability(d0).float(), self.matchability(d1).float()
        if hip:
            return _Hip.log_double_softmax(sim.contiguous(), z0.contiguous(), z1.contiguous())
        return log_double_softmax(sim, z0, z1)


def filter_matches(scores: torch.Tensor, th: float):
    """lightglue.py:236-262: mutual nearest neighbours of the log assignment above `th`.
    Returns (matches [K, 2] int64, scores [K])."""
    v0, m0 = scores.max(2)          # best column per row
    _, m1 = scores.max(1)           # best row per column
    rows = torch.arange(m0.shape[1], device=scores.device)
    mutual = m1[0].gather(0, m0[0]) == rows
    ms = torch.where(mutual, v0[0].exp(), torch.zeros((), device=scores.device, dtype=v0.dtype))
    keep = ms > th
    idx0 = rows[keep]
    return torch.stack([idx0, m0[0][idx0]], -1), ms[idx0]


class MatchResult(NamedTuple):
    """Matches of P image pairs (filter_matches with the reference's commented-out dense outputs,
    lightglue.py:235-258). Indices are int32, as lg_assign_matches writes them (filter_matches returns
    int64); scores are fp32.

    matches0 [P, M]: the column matched to row i, or -1; matches1 [P, N]: the row matched to column j,
    or -1; scores0 [P, M] / scores1 [P, N]: exp(score) of the mutual nearest neighbour, else 0 (also
    below the threshold, where matches* is -1); matches [P, min(M, N), 2] / match_scores [P, min(M, N)]:
    the matched (i, j) in ascending i, rows past counts[p] holding -1 / 0; counts [P]."""
    matches0: torch.Tensor
    matches1: torch.Tensor
    scores0: torch.Tensor
    scores1: torch.Tensor
    matches: torch.Tensor
    match_scores: torch.Tensor
    counts: torch.Tensor


def _argmax_lowest(scores: torch.Tensor, dim: int):
    """(max, argmax) along dim with ties to the lowest index (numpy's rule; torch.max promises none on
    the GPU): the minimum over the indices that hold the maximum."""
    size = scores.shape[dim]
    mx = scores.amax(dim, keepdim=True)
    shape = [1] * scores.dim()
    shape[dim] = size
    idx = torch.arange(size, device=scores.device).view(shape)
    first = torch.where(scores == mx, idx, idx.new_full((), size)).amin(dim)
    return mx.squeeze(dim), first.clamp_(max=size - 1)  # (a row of NaNs holds its maximum nowhere)


def filter_matches_dense(scores: torch.Tensor, th: float) -> MatchResult:
    """filter_matches for all P pairs of a log assignment [P, M, N] at once, with the dense outputs
    (lightglue.py:235-258 with its commented-out lines): framework ops only, no loop over pairs and no
    host synchronisation. Ties go to the lowest index. th >= 0. The restatement lg_assign_matches is
    checked against; LightGlueMatcher.match_batch runs it for the shapes that kernel does not take."""
    if th < 0:
        raise ValueError("filter_matches_dense: th must be >= 0")
    pr, m, n = scores.shape
    k, dev = min(m, n), scores.device
    i32 = torch.int32
    if k == 0:
        z = lambda *s: torch.zeros(s, dtype=scores.dtype, device=dev)       # noqa: E731
        e = lambda *s: torch.full(s, -1, dtype=i32, device=dev)             # noqa: E731
        return MatchResult(e(pr, m), e(pr, n), z(pr, m), z(pr, n), e(pr, 0, 2), z(pr, 0),
                           torch.zeros((pr,), dtype=i32, device=dev))
    v0, j0 = _argmax_lowest(scores, 2)       # best column per row
    _, i1 = _argmax_lowest(scores, 1)        # best row per column
    rows = torch.arange(m, device=dev)[None]
    cols = torch.arange(n, device=dev)[None]
    zero = torch.zeros((), dtype=v0.dtype, device=dev)
    mutual0 = i1.gather(1, j0) == rows
    ms0 = torch.where(mutual0, v0.exp(), zero)
    valid0 = ms0 > th
    mutual1 = j0.gather(1, i1) == cols
    ms1 = torch.where(mutual1, ms0.gather(1, i1), zero)
    valid1 = mutual1 & valid0.gather(1, i1)
    counts = valid0.sum(1)
    # the valid rows first, in ascending i (stable); valid rows are mutual, so there are <= min(M, N)
    order = torch.argsort((~valid0).to(torch.uint8), dim=1, stable=True)[:, :k]
    keep = torch.arange(k, device=dev)[None] < counts[:, None]
    lst = torch.stack([order, j0.gather(1, order)], -1)
    return MatchResult(torch.where(valid0, j0, -1).to(i32), torch.where(valid1, i1, -1).to(i32), ms0, ms1,
                       torch.where(keep[..., None], lst, -1).to(i32), torch.where(keep, ms0.gather(1, order), zero),
                       counts.to(i32))


class TokenConfidence(nn.Module):
    """lightglue.py:54-66: a per-token confidence Linear(d, 1) + Sigmoid (state-dict keys token.0.*).
    The reference defines it and never calls it; match_adaptive does."""

    def __init__(self, d: int) -> None:
        super().__init__()
        self.token = nn.Sequential(nn.Linear(d, 1), nn.Sigmoid())


class AdaptiveResult(NamedTuple):
    """match_adaptive's result. result: the MatchResult in original index space (pruned and padded rows
    -1 / 0); stop: the number of layers run (the head is log_assignment[stop - 1]); prune0 [P, M] /
    prune1 [P, N] int32: the number of layers each original point took part in (stop for a point never
    pruned, 0 for padding). With both knobs off nothing is pruned and prune0 / prune1 are None."""
    result: MatchResult
    stop: int
    prune0: Optional[torch.Tensor]
    prune1: Optional[torch.Tensor]


# ---- the published adaptive rules (LightGlue, ICCV 2023, section 3.3; the reference holds only their
# pieces: lightglue.py:54-66, 230-232, 270-271, 304), shared by the kernel path and adaptive_reference ----
def adaptive_thresholds(n_layers: int) -> List[float]:
    """t_i = clip(0.8 + 0.1 exp(-4 i / L), 0, 1) per layer, in float64 (the kernel takes float32(t_i))."""
    return [float(np.clip(0.8 + 0.1 * np.exp(-4.0 * i / n_layers), 0.0, 1.0)) for i in range(n_layers)]


def _f32(v: float) -> float:
    return float(np.float32(v))


def exit_passes(unconfident: int, valid: int, depth_confidence: float) -> bool:
    """A pair passes when the confident share of its valid rows (both images) exceeds depth_confidence."""
    return 1.0 - unconfident / valid > depth_confidence


def keep_rule(conf: torch.Tensor, mtch: torch.Tensor, t: float, depth_confidence: float,
              width_confidence: float) -> torch.Tensor:
    """The keep flags of one pruned segment (fp32 conf / mtch of its valid rows): mtch > float32(1 -
    width_confidence), with depth on also conf <= float32(t); never empty (else the row of highest mtch,
    the lowest index on ties)."""
    keep = mtch > _f32(1.0 - width_confidence)
    if depth_confidence > 0:
        keep = keep | (conf <= _f32(t))
    if keep.numel() and not bool(keep.any()):
        keep = keep.clone()
        keep[int((mtch == mtch.max()).nonzero()[0])] = True
    return keep


def compact_dims(kept0: Sequence[int], kept1: Sequence[int]) -> Tuple[int, int]:
    """The layout after a compaction: (max kept0, max kept1 rounded up to 8: the head's n % 8 == 0)."""
    return max(kept0), (max(kept1) + 7) // 8 * 8


def scatter_matches_reference(r: MatchResult, ind0, ind1, len0, len1, m: int, n: int, stop: int = 0,
                              prune0=None, prune1=None) -> MatchResult:
    """lg_matches_scatter in framework ops: r (the surviving rows' MatchResult, ind0 [P, mc] / ind1 [P, nc]
    their original indices, len0 / len1 their counts per pair) in the original layout m x n."""
    pr, dev, k = r.matches0.shape[0], r.matches0.device, min(m, n)
    i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev)                # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)                 # noqa: E731
    out = MatchResult(i32(pr, m), i32(pr, n), f32(pr, m), f32(pr, n), i32(pr, k, 2), f32(pr, k),
                      torch.zeros((pr,), dtype=torch.int32, device=dev))
    for p in range(pr):
        a, b = int(len0[p]), int(len1[p])
        i0, i1 = ind0[p, :a].long(), ind1[p, :b].long()
        for own, other, mi, si, om, os in ((i0, i1, r.matches0[p, :a], r.scores0[p, :a], out.matches0, out.scores0),
                                           (i1, i0, r.matches1[p, :b], r.scores1[p, :b], out.matches1, out.scores1)):
            mi = mi.long()
            om[p, own] = torch.where(mi >= 0, other[mi.clamp(min=0)], mi).to(torch.int32)
            os[p, own] = si.float()
        c = int(r.counts[p])
        lst = r.matches[p, :c].long()
        out.matches[p, :c, 0], out.matches[p, :c, 1] = i0[lst[:, 0]].to(torch.int32), i1[lst[:, 1]].to(torch.int32)
        out.match_scores[p, :c] = r.match_scores[p, :c].float()
        out.counts[p] = c
        if prune0 is not None:
            prune0[p, i0], prune1[p, i1] = stop, stop
    return out


class LightGlueMatcher(nn.Module):
    """LightGlue(features=None) of the reference with the MI355X attention (lightglue.py:265-353).

    forward(kpts0 [P,M,2], kpts1 [P,N,2], desc0 [P,M,in], desc1 [P,N,in])
        -> (desc0 [P,M,d], desc1 [P,N,d], log-assignment scores [P,M,N] fp32)

    P image pairs of equal sizes go through one forward (the reference's pair loop,
    demo/demo_mono.cpp:194-418, batched): on the hip path every projection, glue kernel and the
    dual log-softmax runs once on all pairs' rows, and each layer's self / cross attention is one
    grouped launch of P-batch calls. glue='torch' runs the pairs one by one."""

    def __init__(self, n_layers: int = 9, descriptor_dim: int = 256, input_dim: int = 256, num_heads: int = 4,
                 filter_threshold: float = 0.1, attention: Optional[AttnFn] = None, glue: str = "hip",
                 depth_confidence: float = -1.0, width_confidence: float = -1.0, prune_min_keypoints: int = 0) -> None:
        super().__init__()
        d = descriptor_dim
        self.depth_confidence, self.width_confidence = float(depth_confidence), float(width_confidence)
        self.prune_min_keypoints = int(prune_min_keypoints)
        self.n_layers, self.filter_threshold = n_layers, filter_threshold
        self.input_proj = nn.Linear(input_dim, d) if input_dim != d else nn.Identity()
        self.posenc = FourierPositionalEncoding(2, d // num_heads)
        self.transformers = nn.ModuleList([TransformerLayer(d, num_heads) for _ in range(n_layers)])
        self.log_assignment = nn.ModuleList([MatchAssignment(d) for _ in range(n_layers)])
        if self.adaptive:  # (only then: the default model's state dict is the reference's, key for key)
            self.token_confidence = nn.ModuleList([TokenConfidence(d) for _ in range(n_layers - 1)])
        self.attention = attention or _kernel_attention
        if glue not in ("hip", "torch"):
            raise ValueError("glue must be 'hip' or 'torch'")
        self.glue = glue

    @property
    def adaptive(self) -> bool:
        """match_adaptive exits early or prunes (a knob > 0); else it is match_batch."""
        return self.depth_confidence > 0 or self.width_confidence > 0

    def pair_inputs_ok(self, kpts0, kpts1, desc0, desc1) -> bool:
        """lg_pair_inputs reads both descriptor sets, both keypoint sets and posenc.Wr as raw fp16
        [.., 256] / [.., 2] / [32, 2] rows: take it only when every one of them is exactly that (an
        fp32 model or mixed-dtype inputs take the framework path, which casts or raises)."""
        f16 = torch.float16
        return (isinstance(self.input_proj, nn.Identity) and all(t.dtype == f16 for t in (kpts0, kpts1, desc0, desc1))
                and self.posenc.Wr.weight.dtype == f16 and desc0.shape[-1] == 256 and desc1.shape[-1] == 256
                and kpts0.shape[-1] == 2 and kpts1.shape[-1] == 2 and tuple(self.posenc.Wr.weight.shape) == (32, 2))

    def forward(self, kpts0, kpts1, desc0, desc1, counts0=None, counts1=None):
        """counts0 / counts1 (ragged batches): pair p's leading counts0[p] rows of image 0 and counts1[p]
        of image 1 are real, the rest padding of any content (_ragged). Padded rows of the returned
        descriptors are unspecified on the fast path and zero elsewhere; scores are -inf on padded rows
        and columns."""
        if counts0 is None and counts1 is None:
            return self._forward(kpts0, kpts1, desc0, desc1)
        return self._ragged(kpts0, kpts1, desc0, desc1, counts0, counts1, None)

    @staticmethod
    def _counts(counts, pr: int, limit: int, name: str, device):
        """One image's counts -> (host list or None, int32 [P] on `device`). Python ints or a CPU integer
        tensor: validated here (length P, 1 <= c <= limit, else ValueError) and uploaded once from
        pinned memory without synchronising. An int32 tensor already on `device` is taken as it is,
        unvalidated (the kernels clamp into [1, limit]): the form to use under stream capture, where
        new counts are written into the same tensor between replays. None: every pair has `limit`."""
        if isinstance(counts, torch.Tensor) and counts.is_cuda:
            if counts.dtype != torch.int32 or tuple(counts.shape) != (pr,) or counts.device != device:
                raise ValueError(f"{name}: a device tensor of counts must be int32 [{pr}] on {device}")
            return None, counts.contiguous()
        if counts is None:
            host = [limit] * pr
        elif isinstance(counts, torch.Tensor):
            if counts.is_floating_point() or counts.dim() != 1:
                raise ValueError(f"{name}: expected a 1-d integer tensor")
            host = [int(c) for c in counts.tolist()]
        else:
            host = [int(c) for c in counts]
        if len(host) != pr:
            raise ValueError(f"{name}: {len(host)} counts for {pr} pairs")
        for c in host:
            if not 1 <= c <= limit:
                raise ValueError(f"{name}: count {c} outside [1, {limit}]")
        t = torch.tensor(host, dtype=torch.int32)
        if device.type == "cuda":
            t = t.pin_memory().to(device, non_blocking=True)
        return host, t

    def _lens_fast(self, desc0, m: int, n: int) -> bool:
        """The path that takes per-pair counts on the device: fp16, hip glue, the kernel attention and
        the chained layers (chain_ok)."""
        d = self.transformers[0].self_attn.Wqkv.in_features if self.n_layers else desc0.shape[-1]
        return (self.glue == "hip" and self.attention is _kernel_attention and desc0.is_cuda and
                desc0.dtype == torch.float16 and self.posenc.Wr.weight.dtype == torch.float16 and
                self.chain_ok(desc0.new_empty((1, 0, d)), m, n))  # (x after input_proj: [.., d] in desc0's dtype)

    def _ragged(self, kpts0, kpts1, desc0, desc1, counts0, counts1, threshold: Optional[float]):
        """forward (threshold None) or match_batch on a padded batch with per-pair counts. fp16 hip
        path with the kernel attention and the chained layers (chain_ok): the equal-size forward with
        the counts as the attention's key counts (self attention of image i: counts_i; cross i -> j:
        counts_j) and the heads' lens forms; the same launches as an equal-size batch, no loop over
        pairs, no host synchronisation. Row-wise kernels compute the padded rows too (wasted, harmless:
        no valid row reads a padded one). Every other case: the pairs one at a time on their valid
        slices through the equal-size code, the results padded (scores -inf, descriptors 0, matches
        -1, match scores 0)."""
        pr, m, n = desc0.shape[0], desc0.shape[1], desc1.shape[1]
        dev = desc0.device
        h0, c0 = self._counts(counts0, pr, m, "counts0", dev)
        h1, c1 = self._counts(counts1, pr, n, "counts1", dev)
        d = self.transformers[0].self_attn.Wqkv.in_features if self.n_layers else desc0.shape[-1]
        if self._lens_fast(desc0, m, n):
            out = self._forward(kpts0, kpts1, desc0, desc1, threshold, lens=(c0, c1))
            return out if threshold is None else out[2]
        h0 = h0 if h0 is not None else c0.tolist()  # (device counts off the fast path: one synchronisation)
        h1 = h1 if h1 is not None else c1.tolist()
        k = min(m, n)
        if threshold is None:
            o0, o1 = desc0.new_zeros((pr, m, d)), desc1.new_zeros((pr, n, d))
            sc = torch.full((pr, m, n), float("-inf"), dtype=torch.float32, device=dev)
        else:
            i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev)      # noqa: E731
            f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
            res = MatchResult(i32(pr, m), i32(pr, n), f32(pr, m), f32(pr, n), i32(pr, k, 2), f32(pr, k),
                              torch.zeros((pr,), dtype=torch.int32, device=dev))
        for p in range(pr):
            a, b = h0[p], h1[p]
            args = (kpts0[p:p + 1, :a], kpts1[p:p + 1, :b], desc0[p:p + 1, :a], desc1[p:p + 1, :b])
            if threshold is None:
                q0, q1, s = self._forward(*args)
                o0[p, :a], o1[p, :b], sc[p, :a, :b] = q0[0].to(o0.dtype), q1[0].to(o1.dtype), s[0].float()
            else:
                r = self.match_batch(*args)
                kk = min(a, b)
                res.matches0[p, :a], res.matches1[p, :b] = r.matches0[0], r.matches1[0]
                res.scores0[p, :a], res.scores1[p, :b] = r.scores0[0].float(), r.scores1[0].float()
                res.matches[p, :kk], res.match_scores[p, :kk] = r.matches[0], r.match_scores[0].float()
                res.counts[p] = r.counts[0]
        return (o0, o1, sc) if threshold is None else res

    def _forward(self, kpts0, kpts1, desc0, desc1, threshold: Optional[float] = None, lens=None):
        """forward; with `threshold` (match_batch) the fp16 hip head returns a MatchResult from
        lg_assign_matches in the scores' place. Every other path returns scores as ever. lens
        (_ragged's fast path only: the chained fp16 path): the per-pair counts (counts0, counts1) on
        the device."""
        pr, m, n = desc0.shape[0], desc0.shape[1], desc1.shape[1]
        hip = self.glue == "hip"
        rows_out = threshold is not None and self.attention is _kernel_attention
        if not hip and pr > 1:  # the framework-op restatement: one pair at a time
            outs = [self.forward(kpts0[i:i + 1], kpts1[i:i + 1], desc0[i:i + 1], desc1[i:i + 1]) for i in range(pr)]
            return tuple(torch.cat(t, 0) for t in zip(*outs))
        splits = (m, n, pr)
        rows = pr * (m + n)
        if hip and not desc0.is_cuda:
            raise PluginError("LightGlueMatcher(glue='hip') runs on the GPU only (no CPU fallback)")
        if hip and self.pair_inputs_ok(kpts0, kpts1, desc0, desc1):  # pair-major rows + posenc in one launch
            x, cos, sin = _Hip.pair_inputs(desc0, desc1, kpts0, kpts1, self.posenc.Wr.weight)
        else:
            x = self.input_proj(torch.cat((desc0, desc1), 1))          # [P, M+N, d], pair-major rows
            cos, sin = self.posenc(torch.cat((kpts0, kpts1), 1).to(x.dtype))
            x = x.reshape(1, rows, x.shape[-1])
            cos, sin = cos.reshape(1, rows, -1), sin.reshape(1, rows, -1)  # [1, P*(M+N), 64], broadcast over heads
            if hip:
                cos, sin = cos.contiguous(), sin.contiguous()
        head = self.log_assignment[self.n_layers - 1]
        if hip and self.chain_ok(x, m, n):
            x, scores = self._forward_chain(x, cos, sin, splits, rows=rows_out, lens=lens)
            if rows_out:  # the head's projected rows v: the matches without the scores tensor
                scores = _Hip.assign_matches(scores, m, x.shape[-1], threshold, lens)
        else:
            if lens is not None:
                raise PluginError("LightGlueMatcher: per-pair counts reached a path that cannot mask them")
            for layer in self.transformers:
                x = layer(x, cos, sin, splits, self.attention, hip)
            if hip and head.hip16_ok(x, m, n):
                scores = head.matches_rows(x, pr, m, n, threshold) if rows_out else head.forward_rows(x, pr, m, n)
            else:
                scores = None
        x = x.view(pr, m + n, x.shape[-1])
        d0, d1 = x[:, :m], x[:, m:]
        return d0, d1, scores if scores is not None else head(d0, d1, hip)

    # Which projections the chained path folds into the FFN launch before them (s: the cross block's
    # to_qk | to_v, q: the next layer's Wqkv, h: the head's projection). Measured
    # (profiles/r06/chain_kinds_forward_ab.jsonl, ms per forward, none / s / h / sh / sqh): P = 1 n = 1024
    # 0.496 / 0.481 / 0.494 / 0.480 / 0.492, P = 4 0.790 / 0.729 / 0.747 / 0.723 / 0.772, P = 16 2.165 /
    # 2.133 / 2.163 / 2.128 / 2.183: "sh" with the 32-row FFN kernel; folding Wqkv (768 channels, 384 KiB
    # more per workgroup's stream) cost the launch more than the separate projection took. With the
    # 16-row kernel (up to 4,096 rows: twice the workgroups) and the QKV epilogues' rotary factors read
    # from a conflict-free table (prefetched, in the 16-row kernel), "sqh" wins at every size
    # (profiles/r06/chain_kinds_rows16_ab.jsonl, chain_kinds_sqh_ab.jsonl; sh / sqh: P = 1 n = 512 0.372 /
    # 0.367, n = 1024 0.440 / 0.420, n = 2048 0.679 / 0.634, P = 2 0.560 / 0.513, P = 4 0.724 / 0.709,
    # P = 8 1.195 / 1.159, P = 16 2.140 / 2.124). Outputs bitwise equal in every form. LG_CHAIN (or this
    # attribute) overrides, for A/B.
    chain_kinds: Optional[str] = None

    def _chain_kinds(self, rows: int) -> str:
        if self.chain_kinds is not None:
            return self.chain_kinds
        return os.environ.get("LG_CHAIN", "sqh")

    def chain_ok(self, x: torch.Tensor, m: int, n: int) -> bool:
        """The chained fp16 path: every block fusable (4 x 64 heads, d = 256) and the fp16 head."""
        return (self.n_layers > 0 and all(_fused_ok(x, layer.self_attn) for layer in self.transformers) and
                self.log_assignment[self.n_layers - 1].hip16_ok(x, m, n))

    def _forward_chain(self, x, cos, sin, splits, rows: bool = False, lens=None):
        """fp16 hip path with the layers chained (round 6): FFN launches also project their output for
        the attention that follows (lg_linear_cat_ffn_proj) — by default the self block's FFN the cross
        block's to_qk | to_v, the cross block's FFN the next layer's Wqkv (+ rotary) and the last FFN
        the assignment head's [W_final / scale ; w_match] (chain_kinds) — so a layer is 4 launches (self
        attention, FFN + cross projection, cross attention, FFN + next projection) and a forward
        2 + 4 L + 2 (inputs, layer 0's Wqkv, the layers, the head's two; lightglue.py:328-353)."""
        dt = x.dtype
        m, n, pr = _sp(splits)
        kinds = self._chain_kinds(x.shape[1])
        layers = self.transformers
        head = self.log_assignment[len(layers) - 1]
        if lens is None:
            attn_self = attn_cross = self.attention
        else:  # ragged: image i's rows end at lens[i] (self attention: keys of its own image, cross: the other's)
            attn_self = lambda calls: _kernel_attention_lens(calls, lens, (lens[0], lens[1]))   # noqa: E731
            attn_cross = lambda calls: _kernel_attention_lens(calls, lens, (lens[1], lens[0]))  # noqa: E731
        qkv = None
        for li, layer in enumerate(layers):
            sa, ca = layer.self_attn, layer.cross_attn
            if qkv is None:
                wq, bq = _qkv_perm(sa, dt)
                qkv = _Hip.linear_qkv_rotary(x, wq, bq, cos, sin, sa.heads, splits)
            c0, c1 = attn_self(qkv)                                               # self0, self1: one launch
            _, b0 = _ffn_in_fused(sa, sa.out_proj, dt)
            wc, bc = _cross_qkv(ca, dt)
            if "s" in kinds:
                pk = _ffn_packed(sa, sa.out_proj, dt, ("_x", (ca.to_qk.weight, ca.to_qk.bias, ca.to_v.weight, ca.to_v.bias),
                                                       lambda ca=ca: _cross_qkv(ca, dt)[0]))
                x, ((qk0, qk1), (v0, v1)) = _Hip.ffn_proj(x, c0, c1, b0, sa.ffn[1], sa.ffn[3].bias, pk, 1, bc, splits)
            else:
                w0, _ = _ffn_in_fused(sa, sa.out_proj, dt)
                x = _Hip.ffn(x, c0, c1, w0, b0, sa.ffn[1], sa.ffn[3].weight, sa.ffn[3].bias, _ffn_packed(sa, sa.out_proj, dt))
                (qk0, qk1), (v0, v1) = _Hip.linear_split2(x, wc, bc, ca.heads, splits)
            m0, m1 = attn_cross([(qk0, qk1, v1), (qk1, qk0, v0)])              # cross: one launch
            w0, b0 = _ffn_in_fused(ca, ca.to_out, dt)
            qkv = v = None
            if li + 1 < len(layers) and "q" in kinds:
                nsa = layers[li + 1].self_attn
                _, bq = _qkv_perm(nsa, dt)
                pk = _ffn_packed(ca, ca.to_out, dt, ("_q", (nsa.Wqkv.weight, nsa.Wqkv.bias),
                                                     lambda nsa=nsa: _qkv_perm(nsa, dt)[0]))
                x, qkv = _Hip.ffn_proj(x, m0, m1, b0, ca.ffn[1], ca.ffn[3].bias, pk, 2, bq, splits, cos, sin)
            elif li + 1 == len(layers) and "h" in kinds:
                _, b3 = head.aug_weights(dt, 512)
                hp = (head.final_proj.weight, head.final_proj.bias, head.matchability.weight, head.matchability.bias)
                pk = _ffn_packed(ca, ca.to_out, dt, ("_h", hp, lambda head=head: head.aug_weights(dt, 512)[0]))
                x, v = _Hip.ffn_proj(x, m0, m1, b0, ca.ffn[1], ca.ffn[3].bias, pk, 3, b3, splits, n_store=384)
            else:
                x = _Hip.ffn(x, m0, m1, w0, b0, ca.ffn[1], ca.ffn[3].weight, ca.ffn[3].bias, _ffn_packed(ca, ca.to_out, dt))
        if v is None:
            w, b = head.aug_weights(dt, 384)
            v = _Hip.linear(x, w, b)
        v = v.view(pr, m + n, 384)
        if rows:  # (match_batch: the head's projected rows instead of the scores)
            return x, v
        return x, _Hip.assign_scores(v, m, x.shape[-1], lens)

    def match(self, kpts0, kpts1, desc0, desc1):
        """forward + filter_matches (the demo's post-processing); for P > 1 pairs a list of
        (matches, scores), one per pair."""
        _, _, scores = self.forward(kpts0, kpts1, desc0, desc1)
        if scores.shape[0] == 1:
            return filter_matches(scores, self.filter_threshold)
        return [filter_matches(scores[i:i + 1], self.filter_threshold) for i in range(scores.shape[0])]

    def match_batch(self, kpts0, kpts1, desc0, desc1, counts0=None, counts1=None) -> MatchResult:
        """The matches of all P pairs as one MatchResult (dense matches and scores of both images and
        the compacted list), without a loop over pairs or a host synchronisation. On the fp16 hip path
        the forward stops at the head's projection and lg_assign_matches takes its rows (the forward's
        launches through the last FFN, then at most three; the fp32 scores tensor is never written).
        Every other case (fp32 model, glue='torch', n % 8 != 0, more than 2048 keypoints, a substituted
        attention=) computes the scores as forward does and runs filter_matches_dense on them.
        counts0 / counts1: a ragged batch, as for forward (matches -1 and scores 0 on padded rows and
        columns; the list keeps min(M, N) rows per pair)."""
        if counts0 is not None or counts1 is not None:
            return self._ragged(kpts0, kpts1, desc0, desc1, counts0, counts1, self.filter_threshold)
        out = self._forward(kpts0, kpts1, desc0, desc1, threshold=self.filter_threshold)[2]
        return out if isinstance(out, MatchResult) else filter_matches_dense(out, self.filter_threshold)

    def match_features(self, f0, f1) -> MatchResult:
        """match_batch on two frontend.Features (image 0 and image 1 of P pairs) with their device counts:
        nothing is read back, so extract + match enqueue, or capture, as one piece. The kernels clamp
        counts into [1, limit], so a pair with no keypoint on either side is masked afterwards on the
        device: matches -1, scores 0, count 0."""
        r = self.match_batch(f0.kpts, f1.kpts, f0.desc, f1.desc, counts0=f0.counts, counts1=f1.counts)
        ok = (f0.counts > 0) & (f1.counts > 0)
        row, cell = ok[:, None], ok[:, None, None]
        return MatchResult(torch.where(row, r.matches0, -1), torch.where(row, r.matches1, -1),
                           torch.where(row, r.scores0, 0.0), torch.where(row, r.scores1, 0.0),
                           torch.where(cell, r.matches, -1), torch.where(row, r.match_scores, 0.0),
                           torch.where(ok, r.counts, 0))

    def match_pairs(self, pairs):
        """pairs: a sequence of (kpts0 [m_p, 2], kpts1 [n_p, 2], desc0 [m_p, D], desc1 [n_p, D]) of any
        sizes (one device and dtype). Zero-pads them to M = max m_p and N = max n_p rounded up to 8 and
        runs match_batch with the counts: (MatchResult of the padded batch, counts0, counts1), the
        counts as Python ints. Also how a single pair with n % 8 != 0 reaches the fp16 fast path."""
        pairs = list(pairs)
        if not pairs:
            raise ValueError("match_pairs: no pairs")
        c0, c1 = [int(p[0].shape[0]) for p in pairs], [int(p[1].shape[0]) for p in pairs]
        m, n = max(c0), (max(c1) + 7) // 8 * 8
        batch = []
        for j, size in enumerate((m, n, m, n)):
            ref = pairs[0][j]
            t = ref.new_zeros((len(pairs), size, ref.shape[-1]))
            for p, pair in enumerate(pairs):
                t[p, :pair[j].shape[0]] = pair[j]
            batch.append(t)
        return self.match_batch(*batch, counts0=c0, counts1=c1), c0, c1

    # ---- adaptive depth and width ----
    def _token_params(self, li: int, dtype: torch.dtype):
        """Layer li's (w_tok, b_tok, w_match, b_match) as lg_token_scores reads them (cached)."""
        tok, mat = self.token_confidence[li].token[0], self.log_assignment[li].matchability
        return _cached(self.token_confidence[li], "_token_params", (tok.weight, tok.bias, mat.weight, mat.bias), dtype,
                       lambda: (tok.weight.reshape(-1), tok.bias.reshape(-1), mat.weight.reshape(-1), mat.bias.reshape(-1)))

    def match_adaptive(self, kpts0, kpts1, desc0, desc1, counts0=None, counts1=None,
                       trace: Optional[list] = None) -> AdaptiveResult:
        """match_batch with adaptive depth and width (the published LightGlue rules). After each layer
        i < L - 1 every valid row gets conf = sigmoid(token_confidence[i](x)) and mtch =
        sigmoid(log_assignment[i].matchability(x)), and with t_i = adaptive_thresholds(L)[i]:
          depth_confidence > 0: a pair passes when 1 - #(conf < t_i) / #valid > depth_confidence (both
            images' valid rows); when every pair passes the forward stops and log_assignment[i] is the head;
          width_confidence > 0, per image whose row dimension exceeds prune_min_keypoints: a row is kept when
            mtch > float32(1 - width_confidence), with depth on also when conf <= t_i; a segment (one image
            of one pair) never empties (keep_rule); the kept rows go on, in their order.
        Returns AdaptiveResult: the matches of the last layer run on the surviving rows, in original index
        space. trace (a list): receives per checked layer a dict (layer, threshold, stats [P][4] = (kept0,
        kept1, unconfident, valid), stop, dims = the layout that goes on, kept0 / kept1 = per pair the
        original indices that go on), which adaptive_reference(decisions=) follows; it costs copies.

        The fp16 hip path (forward's ragged fast path) runs the chained layer launches with the counts on
        the device; at a checked layer boundary the next layer's Wqkv is not folded into the FFN launch
        (its rows may be compacted first). lg_token_scores' [P, 4] stats are copied to pinned memory and
        the host waits for that copy: ONE synchronisation per checked layer, so this method cannot be
        captured in a graph. Rows are then compacted (lg_compact_rows) into the layout compact_dims gives
        and the forward goes on at the smaller shape. Every other case (fp32, glue='torch', a substituted
        attention=, off-size shapes): adaptive_reference. With both knobs <= 0: match_batch's launches and
        bits, stop = n_layers, prune0 = prune1 = None."""
        if not self.adaptive:
            return AdaptiveResult(self.match_batch(kpts0, kpts1, desc0, desc1, counts0, counts1), self.n_layers, None, None)
        pr, m, n = desc0.shape[0], desc0.shape[1], desc1.shape[1]
        if not self._lens_fast(desc0, m, n):
            return adaptive_reference(self, kpts0, kpts1, desc0, desc1, counts0, counts1, trace=trace)
        dev, dt = desc0.device, desc0.dtype
        h0, c0 = self._counts(counts0, pr, m, "counts0", dev)
        h1, c1 = self._counts(counts1, pr, n, "counts1", dev)
        if self.pair_inputs_ok(kpts0, kpts1, desc0, desc1):
            x, cos, sin = _Hip.pair_inputs(desc0, desc1, kpts0, kpts1, self.posenc.Wr.weight)
        else:
            x = self.input_proj(torch.cat((desc0, desc1), 1))
            cos, sin = self.posenc(torch.cat((kpts0, kpts1), 1).to(x.dtype))
            x = x.reshape(1, pr * (m + n), x.shape[-1])
            cos, sin = cos.reshape(1, pr * (m + n), -1).contiguous(), sin.reshape(1, pr * (m + n), -1).contiguous()
        layers, nl = self.transformers, self.n_layers
        depth, width = self.depth_confidence > 0, self.width_confidence > 0
        thr = adaptive_thresholds(nl)
        t_keep = _f32(1.0 - self.width_confidence) if width else 0.0
        kinds = self._chain_kinds(x.shape[1])
        pinned = self.__dict__.get("_stats_pinned")
        if pinned is None or tuple(pinned.shape) != (max(nl - 1, 1), pr, 4):
            pinned = self.__dict__["_stats_pinned"] = torch.empty((max(nl - 1, 1), pr, 4), dtype=torch.int32).pin_memory()
        prune = tuple(torch.zeros((pr, k), dtype=torch.int32, device=dev) for k in (m, n))
        lens, ind, mc, nc = (c0, c1), (None, None), m, n
        host = [h0, h1]                     # (the counts on the host, where known: the trace's index maps)
        v, stop = None, nl
        for li, layer in enumerate(layers):
            sa, ca = layer.self_attn, layer.cross_attn
            splits = (mc, nc, pr)
            wq, bq = _qkv_perm(sa, dt)
            qkv = _Hip.linear_qkv_rotary(x, wq, bq, cos, sin, sa.heads, splits)
            a0, a1 = _kernel_attention_lens(qkv, lens, (lens[0], lens[1]))
            _, b0 = _ffn_in_fused(sa, sa.out_proj, dt)
            wc, bc = _cross_qkv(ca, dt)
            if "s" in kinds:
                pk = _ffn_packed(sa, sa.out_proj, dt, ("_x", (ca.to_qk.weight, ca.to_qk.bias, ca.to_v.weight, ca.to_v.bias),
                                                       lambda ca=ca: _cross_qkv(ca, dt)[0]))
                x, ((qk0, qk1), (v0, v1)) = _Hip.ffn_proj(x, a0, a1, b0, sa.ffn[1], sa.ffn[3].bias, pk, 1, bc, splits)
            else:
                w0, _ = _ffn_in_fused(sa, sa.out_proj, dt)
                x = _Hip.ffn(x, a0, a1, w0, b0, sa.ffn[1], sa.ffn[3].weight, sa.ffn[3].bias, _ffn_packed(sa, sa.out_proj, dt))
                (qk0, qk1), (v0, v1) = _Hip.linear_split2(x, wc, bc, ca.heads, splits)
            m0, m1 = _kernel_attention_lens([(qk0, qk1, v1), (qk1, qk0, v0)], lens, (lens[1], lens[0]))
            w0, b0 = _ffn_in_fused(ca, ca.to_out, dt)
            if li + 1 == nl and "h" in kinds:
                head = self.log_assignment[li]
                _, b3 = head.aug_weights(dt, 512)
                hp = (head.final_proj.weight, head.final_proj.bias, head.matchability.weight, head.matchability.bias)
                pk = _ffn_packed(ca, ca.to_out, dt, ("_h", hp, lambda head=head: head.aug_weights(dt, 512)[0]))
                x, v = _Hip.ffn_proj(x, m0, m1, b0, ca.ffn[1], ca.ffn[3].bias, pk, 3, b3, splits, n_store=384)
            else:  # (a checked boundary: the next Wqkv runs on the compacted rows)
                x = _Hip.ffn(x, m0, m1, w0, b0, ca.ffn[1], ca.ffn[3].weight, ca.ffn[3].bias, _ffn_packed(ca, ca.to_out, dt))
            if li + 1 == nl:
                break
            flags = ((_lib.ADAPT_DEPTH if depth else 0) | (_lib.ADAPT_WIDTH0 if width and mc > self.prune_min_keypoints else 0) |
                     (_lib.ADAPT_WIDTH1 if width and nc > self.prune_min_keypoints else 0))
            _, _, keep, stats = _Hip.token_scores(x, mc, nc, pr, lens, *self._token_params(li, dt), _f32(thr[li]), t_keep, flags)
            pinned[li].copy_(stats, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
            done.synchronize()               # the one host wait of this layer boundary
            st = pinned[li].tolist()
            halt = depth and all(exit_passes(s[2], s[3], self.depth_confidence) for s in st)
            if not halt and any(s[0] + s[1] < s[3] for s in st):
                mo, no = compact_dims([s[0] for s in st], [s[1] for s in st])
                x, cos, sin, ind, lens = _Hip.compact_rows(x, cos, sin, keep, ind, mc, nc, pr, lens, mo, no, prune, li + 1)
                mc, nc = mo, no
                host = [[s[0] for s in st], [s[1] for s in st]]
            if trace is not None:
                host = [h if h is not None else t.tolist() for h, t in zip(host, lens)]
                maps = [[(i[p, :c].cpu().long() if i is not None else torch.arange(c)) for p, c in enumerate(h)]
                        for i, h in zip(ind, host)]
                trace.append(dict(layer=li, threshold=thr[li], stats=st, stop=halt, dims=(mc, nc), kept0=maps[0], kept1=maps[1]))
            if halt:
                stop = li + 1
                break
        if v is None:
            w, b = self.log_assignment[stop - 1].aug_weights(dt, 384)
            v = _Hip.linear(x, w, b)
        r = _Hip.assign_matches(v.view(pr, mc + nc, 384), mc, x.shape[-1], self.filter_threshold, lens)
        return AdaptiveResult(_Hip.matches_scatter(r, ind, lens, m, n, stop, prune), stop, prune[0], prune[1])


# --------------------------------------------------------------------------------------------
# Deterministic synthetic weights and inputs (no checkpoints offline): every parameter is drawn
# from lightglue_amd.synth (bit-reproducible on any host) with a seed derived from its name.
# --------------------------------------------------------------------------------------------
def seeded_state_dict(seed: int, n_layers: int = 9, descriptor_dim: int = 256, input_dim: int = 256,
                      num_heads: int = 4) -> dict:
    ref = LightGlueMatcher(n_layers, descriptor_dim, input_dim, num_heads)
    out = {}
    for name, p in ref.state_dict().items():
        s = (seed * 1_000_003 + zlib.crc32(name.encode())) & 0x7FFFFFFF
        shape = tuple(p.shape)
        if name.endswith("posenc.Wr.weight"):
            arr = synth.normal(s, shape, 1.0)                     # reference init: std gamma^-2 = 1
        elif ".ffn.1." in name:                                   # LayerNorm affine
            arr = (1.0 if name.endswith("weight") else 0.0) + synth.normal(s, shape, 0.1)
        elif name.endswith("weight"):
            arr = synth.normal(s, shape, 1.0 / np.sqrt(shape[-1]))
        else:
            arr = synth.normal(s, shape, 0.02)
        out[name] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    return out


def synthetic_pair(seed: int, m: int, n: int, input_dim: int = 256, overlap: int = 0):
    """Keypoints in the normalised [-1, 1] frame and unit-norm descriptors, fp32, batch 1.

    overlap > 0: the first `overlap` keypoints of image 1 re-observe distinct keypoints of image 0
    (a seeded permutation; positions moved by ~0.01, descriptors perturbed by 0.2-std noise and
    renormalised), so the pair has real correspondences for the matcher to find."""
    k0 = synth.uniform24(seed * 4 + 0, m * 2).reshape(1, m, 2) * 2.0 - 1.0
    k1 = synth.uniform24(seed * 4 + 1, n * 2).reshape(1, n, 2) * 2.0 - 1.0
    d0 = synth.normal(seed * 4 + 2, (1, m, input_dim))
    d1 = synth.normal(seed * 4 + 3, (1, n, input_dim))
    d0 = d0 / np.linalg.norm(d0, axis=-1, keepdims=True)
    if overlap > 0:
        assert overlap <= min(m, n)
        src = np.argsort(synth.uniform24(seed * 4 + 5, m), kind="stable")[:overlap]
        k1[0, :overlap] = k0[0, src] + 0.01 * synth.normal(seed * 4 + 6, (overlap, 2))
        d1[0, :overlap] = d0[0, src] + 0.2 * synth.normal(seed * 4 + 7, (overlap, input_dim)) / np.sqrt(input_dim)
    d1 = d1 / np.linalg.norm(d1, axis=-1, keepdims=True)
    return tuple(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in (k0, k1, d0, d1))


def seeded_confidence_state_dict(seed: int, n_layers: int = 9, descriptor_dim: int = 256) -> dict:
    """The token_confidence.* entries of an adaptive model (n_layers - 1 weight / bias pairs), drawn as
    seeded_state_dict draws every other parameter: load {**seeded_state_dict(..), **this}."""
    out = {}
    for i in range(n_layers - 1):
        for kind, shape in (("weight", (1, descriptor_dim)), ("bias", (1,))):
            name = f"token_confidence.{i}.token.0.{kind}"
            s = (seed * 1_000_003 + zlib.crc32(name.encode())) & 0x7FFFFFFF
            arr = synth.normal(s, shape, 1.0 / np.sqrt(shape[-1]) if kind == "weight" else 0.02)
            out[name] = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))
    return out


def adaptive_reference(model: "LightGlueMatcher", kpts0, kpts1, desc0, desc1, counts0=None, counts1=None,
                       trace: Optional[list] = None, decisions: Optional[Sequence[dict]] = None) -> AdaptiveResult:
    """match_adaptive's semantics in framework ops, one pair at a time on its valid rows (the layers in
    lock-step over the pairs: the exit is a decision of the whole batch): the path of fp32 models,
    glue='torch', a substituted attention= and off-size shapes, and the tests' oracle. conf and mtch are
    computed in fp32 from the layer's output. A pair's row dimension (prune_min_keypoints) is its own
    count here, and a trace entry's dims are the largest surviving counts (nothing is padded). decisions
    (a trace of match_adaptive or of this function): follow the recorded stop layer and kept index maps
    instead of this run's own scores."""
    nl = model.n_layers
    if not model.adaptive:
        return AdaptiveResult(model.match_batch(kpts0, kpts1, desc0, desc1, counts0, counts1), nl, None, None)
    pr, m, n = desc0.shape[0], desc0.shape[1], desc1.shape[1]
    dev = desc0.device
    hosts = []
    for counts, limit, name in ((counts0, m, "counts0"), (counts1, n, "counts1")):
        h, t = model._counts(counts, pr, limit, name, dev)
        hosts.append(h if h is not None else t.tolist())
    hip = model.glue == "hip"
    depth, width = model.depth_confidence > 0, model.width_confidence > 0
    thr = adaptive_thresholds(nl)
    state = []                              # per pair: [x, cos, sin, ind0, ind1]
    for p, (a, b) in enumerate(zip(*hosts)):
        x = model.input_proj(torch.cat((desc0[p:p + 1, :a], desc1[p:p + 1, :b]), 1))
        cos, sin = model.posenc(torch.cat((kpts0[p:p + 1, :a], kpts1[p:p + 1, :b]), 1).to(x.dtype))
        state.append([x, cos.reshape(1, a + b, -1).contiguous(), sin.reshape(1, a + b, -1).contiguous(),
                      torch.arange(a, device=dev), torch.arange(b, device=dev)])
    prune0 = torch.zeros((pr, m), dtype=torch.int32, device=dev)
    prune1 = torch.zeros((pr, n), dtype=torch.int32, device=dev)
    stop = nl
    for li, layer in enumerate(model.transformers):
        for s in state:
            s[0] = layer(s[0], s[1], s[2], (len(s[3]), len(s[4])), model.attention, hip)
        if li + 1 == nl:
            break
        dec = decisions[li] if decisions is not None else None
        tok, mat = model.token_confidence[li].token[0], model.log_assignment[li].matchability
        st, keeps = [], []
        for p, s in enumerate(state):
            xf, mc = s[0][0].float(), len(s[3])
            conf = torch.sigmoid(F.linear(xf, tok.weight.float(), tok.bias.float()))[:, 0]
            mtch = torch.sigmoid(F.linear(xf, mat.weight.float(), mat.bias.float()))[:, 0]
            ks = []
            for cf, mt in ((conf[:mc], mtch[:mc]), (conf[mc:], mtch[mc:])):
                on = width and cf.numel() > model.prune_min_keypoints
                ks.append(keep_rule(cf, mt, thr[li], model.depth_confidence, model.width_confidence) if on
                          else torch.ones_like(cf, dtype=torch.bool))
            if dec is not None:
                ks = [torch.isin(own, kept[p].to(dev)) for own, kept in ((s[3], dec["kept0"]), (s[4], dec["kept1"]))]
            keeps.append(ks)
            st.append([int(ks[0].sum()), int(ks[1].sum()), int((conf < _f32(thr[li])).sum()), conf.numel()])
        halt = depth and all(exit_passes(s[2], s[3], model.depth_confidence) for s in st)
        if dec is not None:
            halt = bool(dec["stop"])
        if not halt:
            for p, (s, (k0, k1)) in enumerate(zip(state, keeps)):
                mc = len(s[3])
                prune0[p, s[3][~k0]], prune1[p, s[4][~k1]] = li + 1, li + 1
                rows = torch.cat((k0, k1))
                s[0], s[1], s[2] = (t[:, rows].contiguous() for t in s[:3])
                s[3], s[4] = s[3][k0], s[4][k1]
        if trace is not None:
            k0s, k1s = [len(s[3]) for s in state], [len(s[4]) for s in state]
            trace.append(dict(layer=li, threshold=thr[li], stats=st, stop=halt, dims=(max(k0s), max(k1s)),
                              kept0=[s[3].cpu() for s in state], kept1=[s[4].cpu() for s in state]))
        if halt:
            stop = li + 1
            break
    head = model.log_assignment[stop - 1]
    k = min(m, n)
    i32 = lambda *s: torch.full(s, -1, dtype=torch.int32, device=dev)      # noqa: E731
    f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)       # noqa: E731
    res = MatchResult(i32(pr, m), i32(pr, n), f32(pr, m), f32(pr, n), i32(pr, k, 2), f32(pr, k),
                      torch.zeros((pr,), dtype=torch.int32, device=dev))
    for p, s in enumerate(state):
        mc, nc = len(s[3]), len(s[4])
        scores = head(s[0][:, :mc], s[0][:, mc:], hip)
        r = filter_matches_dense(scores.float(), model.filter_threshold)
        one = scatter_matches_reference(r, s[3][None], s[4][None], [mc], [nc], m, n, stop, prune0[p:p + 1], prune1[p:p + 1])
        for dst, src in zip(res, one):
            dst[p] = src[0]
    return AdaptiveResult(res, stop, prune0, prune1)
