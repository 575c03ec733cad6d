"""LightGlue matcher built around the MI355X attention op.

A restatement of the reference model (lightglue_pytorch_no_plugin/lightglue.py): input
projection, Fourier positional encoding applied as a rotary embedding (:32-52, :124-134),
``n_layers`` x (SelfBlock on each image with shared weights, CrossBlock in both directions)
(:88-194), MatchAssignment with the dual log-softmax (:197-233) and ``filter_matches``
(:236-262). Parameter names equal the reference's state-dict keys, so a reference checkpoint
(or ``seeded_state_dict``) loads unchanged.

This module holds the model and is the package's façade for the rest: the blocks are in layers.py, the
kernel wrappers in glue.py, the derived weights in weights.py, ``MatchResult`` and the framework-op
restatements of the match head in matches.py, the adaptive rules and ``adaptive_reference`` in adaptive.py.

What the model adds to the reference's forward, and why:
* ``glue="hip"`` (default) runs everything around the attention on gfx950 kernels too, chained on the
  fp16 path (``_forward_chain``); ``glue="torch"`` is the same math in framework ops (the restatement the
  CPU tests pin to the reference);
* ``match_batch`` returns the matches of all pairs of a forward as one ``MatchResult``: on the fp16 hip
  path from ``lg_assign_matches``, which never writes the scores tensor; elsewhere from
  ``filter_matches_dense``;
* ``forward`` / ``match_batch`` take per-pair keypoint counts (``counts0``, ``counts1``) for padded
  batches of pairs of different sizes, ``match_pairs`` pads a list of pairs itself, and
  ``match_features`` takes two ``frontend.Features`` with their device counts;
* ``match_adaptive`` (opt-in: ``depth_confidence`` / ``width_confidence`` > 0) applies the published
  LightGlue rules the reference ships the pieces of and never uses: a per-layer token confidence stops
  the forward early, a per-layer matchability drops points;
* ``attention=`` lets tests substitute the oracle for the kernel on CPU; the default path
  requires GPU tensors and fails loudly otherwise (no CPU fallback).
"""
from __future__ import annotations

import os
import zlib
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import _lib, synth
# (the façade: tests and tools read every one of these names as matcher.<name>)
from .adaptive import (AdaptiveResult, TokenConfidence, _f32, adaptive_reference, adaptive_thresholds,  # noqa: F401
                       compact_dims, exit_passes, keep_rule, seeded_confidence_state_dict)
from .glue import _Hip, _sp
from .layers import (AttnFn, CrossBlock, FourierPositionalEncoding, MatchAssignment, SelfBlock,  # noqa: F401
                     TransformerLayer, _fused_ok, _kernel_attention, _lens_attention, log_double_softmax)
from .matches import MatchResult, filter_matches, filter_matches_dense, scatter_matches_reference  # noqa: F401
from .plugin import PluginError
from .weights import _cached, _ffn_in_fused, _qkv_perm, ffn_pack  # noqa: F401


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
        if threshold is None:
            o0, o1 = desc0.new_zeros((pr, m, d)), desc1.new_zeros((pr, n, d))
            sc = torch.full((pr, m, n), float("-inf"), dtype=torch.float32, device=dev)
        else:
            res = MatchResult.blank(pr, m, n, dev)
        for p in range(pr):
            a, b = h0[p], h1[p]
            args = (kpts0[p:p + 1, :a], kpts1[p:p + 1, :b], desc0[p:p + 1, :a], desc1[p:p + 1, :b])
            if threshold is None:
                q0, q1, s = self._forward(*args)
                o0[p, :a], o1[p, :b], sc[p, :a, :b] = q0[0].to(o0.dtype), q1[0].to(o1.dtype), s[0].float()
            else:
                res.put(p, self.match_batch(*args))
        return (o0, o1, sc) if threshold is None else res

    def _inputs(self, kpts0, kpts1, desc0, desc1, hip: bool):
        """The layers' inputs: x [1, P*(M+N), d] (pair-major rows) and the rotary tables cos, sin
        [1, P*(M+N), 64] (broadcast over heads); on the hip path one launch where lg_pair_inputs takes them."""
        if hip and self.pair_inputs_ok(kpts0, kpts1, desc0, desc1):
            return _Hip.pair_inputs(desc0, desc1, kpts0, kpts1, self.posenc.Wr.weight)
        x = self.input_proj(torch.cat((desc0, desc1), 1))          # [P, M+N, d]
        cos, sin = self.posenc(torch.cat((kpts0, kpts1), 1).to(x.dtype))
        rows = x.shape[0] * x.shape[1]
        x, cos, sin = x.reshape(1, rows, x.shape[-1]), cos.reshape(1, rows, -1), sin.reshape(1, rows, -1)
        return (x, cos.contiguous(), sin.contiguous()) if hip else (x, cos, sin)

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
        if hip and not desc0.is_cuda:
            raise PluginError("LightGlueMatcher(glue='hip') runs on the GPU only (no CPU fallback)")
        x, cos, sin = self._inputs(kpts0, kpts1, desc0, desc1, hip)
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

    def _chain_kinds(self) -> str:
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
        2 + 4 L + 2 (inputs, layer 0's Wqkv, the layers, the head's two; lightglue.py:328-353). Every
        layer is TransformerLayer.fused_step; what it folds is decided here."""
        m, n, pr = _sp(splits)
        kinds = self._chain_kinds()
        layers = self.transformers
        head = self.log_assignment[len(layers) - 1]
        attn_self, attn_cross = (self.attention, self.attention) if lens is None else _lens_attention(lens)
        qkv = None
        for li, layer in enumerate(layers):
            last = li + 1 == len(layers)
            then = (head if last else layers[li + 1].self_attn) if ("h" if last else "q") in kinds else None
            x, qkv, v = layer.fused_step(x, cos, sin, splits, qkv, attn_self, attn_cross, "s" in kinds, then)
        v = v.view(pr, m + n, 384) if v is not None else head.project_rows(x, pr, m, n)
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
        x, cos, sin = self._inputs(kpts0, kpts1, desc0, desc1, True)
        layers, nl = self.transformers, self.n_layers
        depth, width = self.depth_confidence > 0, self.width_confidence > 0
        thr = adaptive_thresholds(nl)
        t_keep = _f32(1.0 - self.width_confidence) if width else 0.0
        kinds = self._chain_kinds()
        pinned = self.__dict__.get("_stats_pinned")
        if pinned is None or tuple(pinned.shape) != (max(nl - 1, 1), pr, 4):
            pinned = self.__dict__["_stats_pinned"] = torch.empty((max(nl - 1, 1), pr, 4), dtype=torch.int32).pin_memory()
        prune = tuple(torch.zeros((pr, k), dtype=torch.int32, device=dev) for k in (m, n))
        lens, ind, mc, nc = (c0, c1), (None, None), m, n
        host = [h0, h1]                     # (the counts on the host, where known: the trace's index maps)
        v, stop = None, nl
        for li, layer in enumerate(layers):
            last = li + 1 == nl
            # (never the next Wqkv: at a checked boundary it runs on the rows a compaction may leave)
            x, _, v = layer.fused_step(x, cos, sin, (mc, nc, pr), None, *_lens_attention(lens), "s" in kinds,
                                       self.log_assignment[li] if last and "h" in kinds else None)
            if last:
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
        v = v.view(pr, mc + nc, 384) if v is not None else self.log_assignment[stop - 1].project_rows(x, pr, mc, nc)
        r = _Hip.assign_matches(v, mc, x.shape[-1], self.filter_threshold, lens)
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
