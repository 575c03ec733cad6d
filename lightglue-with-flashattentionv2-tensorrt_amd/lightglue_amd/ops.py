"""torch.library operators over the plugin C ABI ("the caller is its own
PyTorch-ROCm module via a torch.library op that invokes enqueue on torch.cuda.current_stream()").

* ``torch.ops.lightglue_amd.mha_hd64(q, k, v) -> o``: the plugin's ``enqueue`` (the TensorRT node
  ``CustomOp::MHAHeadDim64``, lightglue_pytorch_with_plugin/lightglue.py:16-46): [1, 4, N, 64],
  all fp16 (-> fp16) or all fp32 (-> fp32).
* ``torch.ops.lightglue_amd.mha_hd64_backward(q, k, v, o, do) -> [dq, dk, dv]``: its gradient
  (csrc/mha_hd64_backward.hip), registered as the autograd of ``mha_hd64``; [B, H, N, 64].
* ``torch.ops.lightglue_amd.mha_hd64_grouped(qs, ks, vs) -> os``: up to any number of independent
  calls in grouped launches (4 per launch), e.g. the self0/self1 or the two cross directions of a
  LightGlue layer.
* ``torch.ops.lightglue_amd.mha_hd64_grouped_lens(qs, ks, vs, lens) -> os`` and
  ``mha_hd64_grouped_qkv_lens(qs, ks, vs, q_lens, kv_lens)``: the same on ragged batches, with int32
  device tables of per-item key (and query-row) counts (fp16 only).
* ``torch.ops.lightglue_amd.mha_hd64_grouped_backward(qs, ks, vs, os, dos, q_lens, kv_lens) -> [dq_0, dk_0, dv_0, ...]``:
  the gradient of all three grouped ops in one set of launches (mha_hd64_backward_grouped_lens), registered as their
  autograd; padded rows get zero gradients.

* ``torch.ops.lightglue_amd.assign_nll(v, m, zc, gt0, gt1, m_len=None, n_len=None) -> [loss, dv]``: the matcher's
  training loss per pair and its gradient in v (csrc/lightglue_assign_nll.hip), differentiable in v.

* ``torch.ops.lightglue_amd.ffn(x, ctx0, ctx1, w1, b1, gamma, beta, eps, w2, b2) -> out``: the matcher's FFN block
  with its residual on unpacked (training) weights (lg_linear_cat_ffn), differentiable in everything but eps through
  ``ffn_backward(x, ctx0, ctx1, w1, b1, gamma, beta, eps, w2, dy)`` (csrc/lightglue_ffn_backward.hip).

* ``torch.ops.lightglue_amd.qkv_rotary(x, w_perm, b_perm, cos, sin, n0, n1, pairs) -> [q0, k0, v0, q1, k1, v1]``,
  ``split2(x, w, b, n0, n1, pairs) -> [a0, a1, b0, b1]`` and ``project(x, w, b) -> v``: the fused projections
  (lg_linear_qkv_rotary, lg_linear_split2, lg_linear), differentiable in x, w and b through
  ``proj_backward(kind, x, w, grads, n0, n1, pairs, ...)`` (csrc/lightglue_proj_backward.hip).

Only a CUDA (HIP) kernel is registered: a CPU tensor has no implementation to dispatch to and
raises (no CPU fallback). The fake (meta) implementations give shapes/dtypes for tracing.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import torch

from .plugin import mha_hd64 as _enqueue
from .plugin import mha_hd64_backward as _backward
from .plugin import mha_hd64_backward_grouped as _grouped_backward
from .plugin import mha_hd64_grouped as _grouped


@torch.library.custom_op("lightglue_amd::mha_hd64", mutates_args=(), device_types="cuda")
def mha_hd64_op(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
    return _enqueue(query.contiguous(), key.contiguous(), value.contiguous())


@mha_hd64_op.register_fake
def _(query, key, value):
    return torch.empty_like(query, memory_format=torch.contiguous_format)


@torch.library.custom_op("lightglue_amd::mha_hd64_backward", mutates_args=(), device_types="cuda")
def mha_hd64_backward_op(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, out: torch.Tensor,
                         dout: torch.Tensor) -> List[torch.Tensor]:
    """(dQ, dK, dV) of mha_hd64 from its inputs, its output and dO (mha_hd64_backward_fp16 / _fp32)."""
    return list(_backward(query.contiguous(), key.contiguous(), value.contiguous(), out.contiguous(), dout.contiguous()))


@mha_hd64_backward_op.register_fake
def _(query, key, value, out, dout):
    return [torch.empty_like(t, memory_format=torch.contiguous_format) for t in (query, key, value)]


def _mha_hd64_setup_context(ctx, inputs, output):
    ctx.save_for_backward(*inputs, output)


def _mha_hd64_backward(ctx, dout):
    dq, dk, dv = torch.ops.lightglue_amd.mha_hd64_backward(*ctx.saved_tensors, dout)
    need = ctx.needs_input_grad
    return dq if need[0] else None, dk if need[1] else None, dv if need[2] else None


mha_hd64_op.register_autograd(_mha_hd64_backward, setup_context=_mha_hd64_setup_context)


@torch.library.custom_op("lightglue_amd::mha_hd64_grouped", mutates_args=(), device_types="cuda")
def mha_hd64_grouped_op(queries: List[torch.Tensor], keys: List[torch.Tensor],
                        values: List[torch.Tensor]) -> List[torch.Tensor]:
    return _grouped([(q.contiguous(), k.contiguous(), v.contiguous()) for q, k, v in zip(queries, keys, values)])


@mha_hd64_grouped_op.register_fake
def _(queries, keys, values):
    return [torch.empty_like(q, memory_format=torch.contiguous_format) for q in queries]


@torch.library.custom_op("lightglue_amd::mha_hd64_grouped_lens", mutates_args=(), device_types="cuda")
def mha_hd64_grouped_lens_op(queries: List[torch.Tensor], keys: List[torch.Tensor], values: List[torch.Tensor],
                             lens: List[torch.Tensor]) -> List[torch.Tensor]:
    """Ragged batches: call i's item b attends to its first lens[i][b] keys (int32 [B] on the device,
    read there when the kernel runs; mha_hd64_launch_grouped_lens). fp16 only."""
    return _grouped([(q.contiguous(), k.contiguous(), v.contiguous()) for q, k, v in zip(queries, keys, values)],
                    kv_lens=list(lens))


@mha_hd64_grouped_lens_op.register_fake
def _(queries, keys, values, lens):
    return [torch.empty_like(q, memory_format=torch.contiguous_format) for q in queries]


@torch.library.custom_op("lightglue_amd::mha_hd64_grouped_qkv_lens", mutates_args=(), device_types="cuda")
def mha_hd64_grouped_qkv_lens_op(queries: List[torch.Tensor], keys: List[torch.Tensor], values: List[torch.Tensor],
                                 q_lens: List[torch.Tensor], kv_lens: List[torch.Tensor]) -> List[torch.Tensor]:
    """mha_hd64_grouped_lens with query-row counts as well (mha_hd64_launch_grouped_qkv_lens): rows at or
    past q_lens[i][b] are padding (written as NaN; no real row's bits depend on them). The matcher's
    ragged forward."""
    return _grouped([(q.contiguous(), k.contiguous(), v.contiguous()) for q, k, v in zip(queries, keys, values)],
                    kv_lens=list(kv_lens), q_lens=list(q_lens))


@mha_hd64_grouped_qkv_lens_op.register_fake
def _(queries, keys, values, q_lens, kv_lens):
    return [torch.empty_like(q, memory_format=torch.contiguous_format) for q in queries]


@torch.library.custom_op("lightglue_amd::mha_hd64_grouped_backward", mutates_args=(), device_types="cuda")
def mha_hd64_grouped_backward_op(queries: List[torch.Tensor], keys: List[torch.Tensor], values: List[torch.Tensor],
                                 outs: List[torch.Tensor], douts: List[torch.Tensor], q_lens: List[Optional[torch.Tensor]],
                                 kv_lens: List[Optional[torch.Tensor]]) -> List[torch.Tensor]:
    """[dq_0, dk_0, dv_0, dq_1, ...] of the grouped ops from their inputs, outputs and the outputs' gradients
    (mha_hd64_backward_grouped_lens); q_lens / kv_lens: per call the int32 [B] counts or None, an empty list for none
    at all. Gradients of padded rows are zeros. fp16 only."""
    cont = [[t.contiguous() for t in ts] for ts in (queries, keys, values, outs, douts)]
    grads = _grouped_backward(list(zip(*cont[:3])), cont[3], cont[4], kv_lens=list(kv_lens) or None,
                              q_lens=list(q_lens) or None)
    return [g for triple in grads for g in triple]


@mha_hd64_grouped_backward_op.register_fake
def _(queries, keys, values, outs, douts, q_lens, kv_lens):
    return [torch.empty_like(t, memory_format=torch.contiguous_format) for qkv in zip(queries, keys, values) for t in qkv]


def _grouped_autograd(op, n_lens):
    """Registers mha_hd64_grouped_backward as op's autograd: inputs (queries, keys, values) and n_lens lists of counts
    (one: the key counts; two: query rows, then keys)."""

    def setup(ctx, inputs, output):
        ctx.n = len(output)
        ctx.lens = [list(l) for l in inputs[3:]]  # (int32 tables: no gradient, kept as they are)
        ctx.save_for_backward(*inputs[0], *inputs[1], *inputs[2], *output)

    def backward(ctx, douts):
        n, saved = ctx.n, ctx.saved_tensors
        qs, ks, vs, os_ = (list(saved[i * n:(i + 1) * n]) for i in range(4))
        q_lens, kv_lens = ([], []) if n_lens == 0 else ([], ctx.lens[0]) if n_lens == 1 else ctx.lens
        got = torch.ops.lightglue_amd.mha_hd64_grouped_backward(qs, ks, vs, os_, list(douts), q_lens, kv_lens)
        need = ctx.needs_input_grad
        grads = tuple([got[3 * i + j] if need[j][i] else None for i in range(n)] for j in range(3))
        return grads + tuple([None] * n for _ in range(n_lens))  # (a list input's gradient is a list)

    op.register_autograd(backward, setup_context=setup)


_grouped_autograd(mha_hd64_grouped_op, 0)
_grouped_autograd(mha_hd64_grouped_lens_op, 1)
_grouped_autograd(mha_hd64_grouped_qkv_lens_op, 2)


@torch.library.custom_op("lightglue_amd::assign_nll", mutates_args=(), device_types="cuda")
def assign_nll_op(v: torch.Tensor, m: int, zc: int, gt0: torch.Tensor, gt1: torch.Tensor,
                  m_len: Optional[torch.Tensor] = None, n_len: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """(loss fp32 [P], dloss/dv fp32 [P, m + n, C]) of the assignment head's input v (lg_assign_nll: loss.py)."""
    from .glue import _Hip

    lens = None if m_len is None else (m_len, n_len)
    return list(_Hip.assign_nll(v.contiguous(), m, zc, gt0.contiguous(), gt1.contiguous(), lens))


@assign_nll_op.register_fake
def _(v, m, zc, gt0, gt1, m_len=None, n_len=None):
    return [v.new_empty((v.shape[0],), dtype=torch.float32), torch.empty_like(v, dtype=torch.float32,
                                                                              memory_format=torch.contiguous_format)]


def _assign_nll_setup_context(ctx, inputs, output):
    ctx.v_dtype = inputs[0].dtype
    ctx.save_for_backward(output[1])
    ctx.mark_non_differentiable(output[1])


def _assign_nll_backward(ctx, grads):
    (dv,) = ctx.saved_tensors
    return (dv * grads[0][:, None, None]).to(ctx.v_dtype), None, None, None, None, None, None


assign_nll_op.register_autograd(_assign_nll_backward, setup_context=_assign_nll_setup_context)


@torch.library.custom_op("lightglue_amd::ffn", mutates_args=(), device_types="cuda")
def ffn_op(x: torch.Tensor, ctx0: torch.Tensor, ctx1: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor, gamma: torch.Tensor,
           beta: torch.Tensor, eps: float, w2: torch.Tensor, b2: torch.Tensor) -> torch.Tensor:
    """x + ffn([x | merge_heads(ctx0, ctx1)]) [1, M, 256] fp16 with w1 the folded first weight (lg_linear_cat_ffn, no
    packed stream: training weights change every step)."""
    from .glue import _Hip

    ln = SimpleNamespace(weight=gamma.contiguous(), bias=beta.contiguous(), eps=eps)
    return _Hip.ffn(x.contiguous(), ctx0.contiguous(), ctx1.contiguous(), w1.contiguous(), b1.contiguous(), ln,
                    w2.contiguous(), b2.contiguous())


@ffn_op.register_fake
def _(x, ctx0, ctx1, w1, b1, gamma, beta, eps, w2, b2):
    return torch.empty_like(x, memory_format=torch.contiguous_format)


@torch.library.custom_op("lightglue_amd::ffn_backward", mutates_args=(), device_types="cuda")
def ffn_backward_op(x: torch.Tensor, ctx0: torch.Tensor, ctx1: torch.Tensor, w1: torch.Tensor, b1: torch.Tensor,
                    gamma: torch.Tensor, beta: torch.Tensor, eps: float, w2: torch.Tensor, dout: torch.Tensor,
                    need_params: bool = True) -> List[torch.Tensor]:
    """(dx, dctx0, dctx1 fp16; dw1, db1, dgamma, dbeta, dw2, db2 fp32) of ffn from its inputs and dout (lg_ffn_backward);
    without need_params the three data gradients alone (its data-only form: the same bits, no weight kernel)."""
    from .glue import _Hip

    ln = SimpleNamespace(weight=gamma.contiguous(), bias=beta.contiguous(), eps=eps)
    out = _Hip.ffn_backward(x.contiguous(), ctx0.contiguous(), ctx1.contiguous(), w1.contiguous(), b1.contiguous(), ln,
                            w2.contiguous(), dout.contiguous(), need_params)
    return list(out if need_params else out[:3])


@ffn_backward_op.register_fake
def _(x, ctx0, ctx1, w1, b1, gamma, beta, eps, w2, dout, need_params=True):
    data = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in (x, ctx0, ctx1)]
    if not need_params:
        return data
    f32 = [w1, b1, gamma, beta, w2, w2.new_empty((w2.shape[0],))]
    return data + [torch.empty_like(t, dtype=torch.float32, memory_format=torch.contiguous_format) for t in f32]


def _ffn_setup_context(ctx, inputs, output):
    x, ctx0, ctx1, w1, b1, gamma, beta, eps, w2, b2 = inputs
    ctx.eps = eps
    ctx.save_for_backward(x, ctx0, ctx1, w1, b1, gamma, beta, w2, b2)


def _ffn_backward(ctx, dout):
    x, ctx0, ctx1, w1, b1, gamma, beta, w2, b2 = ctx.saved_tensors
    need = ctx.needs_input_grad
    params = any(need[i] for i in (3, 4, 5, 6, 8, 9))  # (frozen FFN weights: the data-only call)
    got = torch.ops.lightglue_amd.ffn_backward(x, ctx0, ctx1, w1, b1, gamma, beta, ctx.eps, w2, dout, params)
    grads = list(got[:3]) + [None] * 7
    if params:
        dw1, db1, dg, dbe, dw2, db2 = got[3:]
        grads[3:] = [dw1.to(w1.dtype), db1.to(b1.dtype), dg.to(gamma.dtype), dbe.to(beta.dtype), None, dw2.to(w2.dtype),
                     db2.to(b2.dtype)]
    return tuple(g if g is not None and n else None for g, n in zip(grads, need))


ffn_op.register_autograd(_ffn_backward, setup_context=_ffn_setup_context)


# ---- the fused projections, differentiable (csrc/lightglue_proj_backward.hip) ----
# Their forwards are the inference kernels (lg_linear_qkv_rotary, lg_linear_split2, lg_linear); w and b may be of any
# floating dtype and are cast to x's here, so that a caller who derives them in fp32 gets fp32 gradients back.
def _as(t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    return t.to(like.dtype).contiguous()


@torch.library.custom_op("lightglue_amd::qkv_rotary", mutates_args=(), device_types="cuda")
def qkv_rotary_op(x: torch.Tensor, w_perm: torch.Tensor, b_perm: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor,
                  n0: int, n1: int, pairs: int) -> List[torch.Tensor]:
    """x [1, M, 256] -> [q0, k0, v0, q1, k1, v1] head-major [pairs, 4, ni, 64]: Wqkv (rows in _qkv_perm's order) + rotary."""
    from .glue import _Hip

    i0, i1 = _Hip.linear_qkv_rotary(x.contiguous(), _as(w_perm, x), _as(b_perm, x), cos.contiguous(), sin.contiguous(), 4,
                                    (n0, n1, pairs))
    return [*i0, *i1]


@qkv_rotary_op.register_fake
def _(x, w_perm, b_perm, cos, sin, n0, n1, pairs):
    return [x.new_empty((pairs, 4, n, 64)) for n in (n0, n0, n0, n1, n1, n1)]


@torch.library.custom_op("lightglue_amd::split2", mutates_args=(), device_types="cuda")
def split2_op(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, n0: int, n1: int, pairs: int) -> List[torch.Tensor]:
    """x [1, M, 256] -> [a0, a1, b0, b1] head-major: [to_qk ; to_v] as one GEMM."""
    from .glue import _Hip

    (a0, a1), (b0, b1) = _Hip.linear_split2(x.contiguous(), _as(w, x), _as(b, x), 4, (n0, n1, pairs))
    return [a0, a1, b0, b1]


@split2_op.register_fake
def _(x, w, b, n0, n1, pairs):
    return [x.new_empty((pairs, 4, n, 64)) for n in (n0, n1, n0, n1)]


@torch.library.custom_op("lightglue_amd::project", mutates_args=(), device_types="cuda")
def project_op(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """x [1, M, 256] -> x w^T + b [1, M, n], n a multiple of 64 up to 512 (the head's rows)."""
    from .glue import _Hip

    return _Hip.linear(x.contiguous(), _as(w, x), _as(b, x))


@project_op.register_fake
def _(x, w, b):
    return x.new_empty((1, x.shape[1], w.shape[0]))


@torch.library.custom_op("lightglue_amd::proj_backward", mutates_args=(), device_types="cuda")
def proj_backward_op(kind: int, x: torch.Tensor, w: torch.Tensor, grads: List[Optional[torch.Tensor]], n0: int, n1: int,
                     pairs: int, cos: Optional[torch.Tensor] = None, sin: Optional[torch.Tensor] = None,
                     dx_add: Optional[torch.Tensor] = None, need_params: bool = True) -> List[torch.Tensor]:
    """[dx fp16, dw fp32 [n, 256], db fp32 [n]] of the projection of kind 1 (split2), 2 (qkv_rotary) or 3 (project, n =
    w's rows) from the gradients of its outputs, None for an unused one (lg_proj_backward); without need_params [dx]
    alone (the data-only form: the same bits, no weight kernel)."""
    from .glue import _Hip

    cont = lambda t: None if t is None else t.contiguous()  # noqa: E731
    out = _Hip.proj_backward(kind, x.contiguous(), _as(w, x), [cont(g) for g in grads], (n0, n1, pairs), cont(cos), cont(sin),
                             w.shape[0], cont(dx_add), need_params)
    return list(out if need_params else out[:1])


@proj_backward_op.register_fake
def _(kind, x, w, grads, n0, n1, pairs, cos=None, sin=None, dx_add=None, need_params=True):
    dx = torch.empty_like(x, memory_format=torch.contiguous_format)
    f32 = dict(dtype=torch.float32)
    return [dx, w.new_empty(tuple(w.shape), **f32), w.new_empty((w.shape[0],), **f32)] if need_params else [dx]


def _proj_autograd(op, kind, nw, n_in):
    """Registers op's backward: inputs (x, w, b, ...) with the integers (n0, n1, pairs) last where the op has them."""

    def setup(ctx, inputs, output):
        x, w, b = inputs[:3]
        ctx.tail = inputs[3 + nw:]
        ctx.b_dtype = b.dtype
        ctx.set_materialize_grads(False)  # (an unused output's gradient stays None: a null pointer, not a zero tensor)
        ctx.save_for_backward(x, w, *inputs[3:3 + nw])

    def backward(ctx, grads):
        x, w, *cs = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = list(grads) if kind != 3 else [None if grads is None else grads.float()]
        n0, n1, pairs = ctx.tail if kind != 3 else (x.shape[1], 0, 1)
        got = torch.ops.lightglue_amd.proj_backward(kind, x, w, grads, n0, n1, pairs, *cs, need_params=need[1] or need[2])
        dw, db = (got[1].to(w.dtype), got[2].to(ctx.b_dtype)) if len(got) > 1 else (None, None)
        return (got[0] if need[0] else None, dw if need[1] else None, db if need[2] else None) + (None,) * (n_in - 3)

    op.register_autograd(backward, setup_context=setup)


_proj_autograd(qkv_rotary_op, 2, 2, 8)
_proj_autograd(split2_op, 1, 0, 6)
_proj_autograd(project_op, 3, 0, 3)
