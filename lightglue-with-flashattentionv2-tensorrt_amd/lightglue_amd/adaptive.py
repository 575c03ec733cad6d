"""Adaptive depth and width: the published LightGlue rules (ICCV 2023, section 3.3; the reference holds
only their pieces: lightglue.py:54-66, 230-232, 270-271, 304), shared by LightGlueMatcher.match_adaptive's
kernel path and ``adaptive_reference``, the same in framework ops (the tests' oracle)."""
from __future__ import annotations

import zlib
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import synth
from .matches import MatchResult, filter_matches_dense, scatter_matches_reference


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


def adaptive_reference(model, kpts0, kpts1, desc0, desc1, counts0=None, counts1=None,
                       trace: Optional[list] = None, decisions: Optional[Sequence[dict]] = None) -> AdaptiveResult:
    """match_adaptive's semantics (model: a LightGlueMatcher) in framework ops, one pair at a time on its valid rows (the layers in
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
    res = MatchResult.blank(pr, m, n, dev)
    for p, s in enumerate(state):
        mc, nc = len(s[3]), len(s[4])
        scores = head(s[0][:, :mc], s[0][:, mc:], hip)
        r = filter_matches_dense(scores.float(), model.filter_threshold)
        res.put(p, scatter_matches_reference(r, s[3][None], s[4][None], [mc], [nc], m, n, stop, prune0[p:p + 1],
                                             prune1[p:p + 1]))
    return AdaptiveResult(res, stop, prune0, prune1)
