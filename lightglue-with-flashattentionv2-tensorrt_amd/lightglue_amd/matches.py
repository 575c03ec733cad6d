"""The matcher's results: ``MatchResult`` and the framework-op restatements of what produces one
(``filter_matches`` of the reference, lightglue.py:236-262; ``filter_matches_dense``, what lg_assign_matches
is checked against; ``scatter_matches_reference``, the same for lg_matches_scatter)."""
from __future__ import annotations

from typing import NamedTuple

import torch


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

    @classmethod
    def empty(cls, pr: int, m: int, n: int, device, dtype: torch.dtype = torch.float32) -> "MatchResult":
        """Uninitialised, for P pairs of M x N (a kernel writes every entry)."""
        k = min(m, n)
        i = lambda *s: torch.empty(s, dtype=torch.int32, device=device)  # noqa: E731
        f = lambda *s: torch.empty(s, dtype=dtype, device=device)        # noqa: E731
        return cls(i(pr, m), i(pr, n), f(pr, m), f(pr, n), i(pr, k, 2), f(pr, k), i(pr))

    @classmethod
    def blank(cls, pr: int, m: int, n: int, device, dtype: torch.dtype = torch.float32) -> "MatchResult":
        """No match anywhere: indices -1, scores 0, counts 0."""
        out = cls.empty(pr, m, n, device, dtype)
        for t, fill in zip(out, (-1, -1, 0, 0, -1, 0, 0)):
            t.fill_(fill)
        return out

    def put(self, p: int, one: "MatchResult") -> None:
        """Write the single-pair result `one` (of this result's sizes or smaller) into row p's leading entries."""
        for dst, src in zip(self, one):
            dst[p:p + 1][tuple(slice(s) for s in src.shape)] = src


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
        return MatchResult.blank(pr, m, n, dev, scores.dtype)
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


def scatter_matches_reference(r: MatchResult, ind0, ind1, len0, len1, m: int, n: int, stop: int = 0,
                              prune0=None, prune1=None) -> MatchResult:
    """lg_matches_scatter in framework ops: r (the surviving rows' MatchResult, ind0 [P, mc] / ind1 [P, nc]
    their original indices, len0 / len1 their counts per pair) in the original layout m x n."""
    pr = r.matches0.shape[0]
    out = MatchResult.blank(pr, m, n, r.matches0.device)
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
