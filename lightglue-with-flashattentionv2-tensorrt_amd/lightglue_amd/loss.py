"""The matcher's training loss on the assignment head's input (csrc/lightglue_assign_nll.hip, lg_assign_nll).

v [P, m + n, C] fp16 is what ``MatchAssignment.project_rows`` returns: the scaled descriptors m0 / m1 in channels
0..255 and the matchability logit z at channel zc. gt0 int32 [P, m]: j >= 0: row i matches column j; -1: unmatchable;
any other negative: ignored. gt1 int32 [P, n] is read for its -1 entries. A gt0 at or past the pair's n_len and every
row or column past the pair's counts (lens = (m_len, n_len)) is ignored. Per pair, with sim = fp16(m0 . m1^T) and
s = log_softmax(sim, 2) + log_softmax(sim, 1) + logsig(z0) + logsig(z1)^T over the valid block:

    loss = -0.5/Pn sum_pos s[i][gt0[i]] - 0.5/Nn (sum_{gt0 == -1} logsig(-z0[i]) + sum_{gt1 == -1} logsig(-z1[j]))

Pn = max(#pos, 1), Nn = max(#negatives, 1): the published LightGlue loss with balancing 0.5.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .glue import _Hip


class _AssignmentNLL(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, m, zc, gt0, gt1, lens):
        loss, dv = _Hip.assign_nll(v.contiguous(), m, zc, gt0.contiguous(), gt1.contiguous(), lens,
                                   need_grad=ctx.needs_input_grad[0])
        if dv is not None:
            ctx.save_for_backward(dv)
        ctx.v_dtype = v.dtype
        return loss

    @staticmethod
    def backward(ctx, grad):
        (dv,) = ctx.saved_tensors
        return (dv * grad[:, None, None]).to(ctx.v_dtype), None, None, None, None, None


def assignment_nll(v, m, zc, gt0, gt1, lens=None):
    """loss fp32 [P], differentiable in v: one lg_assign_nll call computes the loss and fp32 dloss/dv; the backward
    multiplies by the incoming per-pair gradient (a loss scale included) before it rounds to v's dtype."""
    return _AssignmentNLL.apply(v, m, zc, gt0, gt1, lens)


def assignment_nll_reference(v, m, zc, gt0, gt1, lens=None):
    """The same loss in float64 framework ops on the operands as given (the fp16 rounding of the similarity
    included, passed straight through in the gradient), differentiable by ordinary autograd: loss float64 [P]."""
    pr, n = v.shape[0], v.shape[1] - m
    v64 = v.double()
    out = []
    for p in range(pr):
        ml, nl = (m, n) if lens is None else (int(lens[0][p]), int(lens[1][p]))
        a, b = v64[p, :ml, :256], v64[p, m:m + nl, :256]
        z0, z1 = v64[p, :ml, zc], v64[p, m:m + nl, zc]
        dot = a @ b.T
        sim = dot + (dot.detach().half().double() - dot.detach())
        s = (torch.log_softmax(sim, 1) + torch.log_softmax(sim, 0) + F.logsigmoid(z0)[:, None] +
             F.logsigmoid(z1)[None, :])
        g0, g1 = gt0[p, :ml].long(), gt1[p, :nl].long()
        pos = (g0 >= 0) & (g0 < nl)
        rows = torch.nonzero(pos)[:, 0]
        neg = F.logsigmoid(-z0)[g0 == -1].sum() + F.logsigmoid(-z1)[g1 == -1].sum()
        nneg = int((g0 == -1).sum()) + int((g1 == -1).sum())
        out.append(-0.5 / max(len(rows), 1) * s[rows, g0[rows]].sum() - 0.5 / max(nneg, 1) * neg)
    return torch.stack(out)
