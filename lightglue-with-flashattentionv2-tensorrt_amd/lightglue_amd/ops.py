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

* ``torch.ops.lightglue_amd.assign_nll(v, m, zc, gt0, gt1, m_len=None, n_len=None) -> [loss, dv]``: the matcher's
  training loss per pair and its gradient in v (csrc/lightglue_assign_nll.hip), differentiable in v.

* ``torch.ops.lightglue_amd.ffn(x, ctx0, ctx1, w1, b1, gamma, beta, eps, w2, b2) -> out``: the matcher's FFN block
  with its residual on unpacked (training) weights (lg_linear_cat_ffn), differentiable in everything but eps through
  ``ffn_backward(x, ctx0, ctx1, w1, b1, gamma, beta, eps, w2, dy)`` (csrc/lightglue_ffn_backward.hip).

Only a CUDA (HIP) kernel is registered: a CPU tensor has no implementation to dispatch to and
raises (no CPU fallback). The fake (meta) implementations give shapes/dtypes for tracing.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional

import torch

from .plugin import mha_hd64 as _enqueue
from .plugin import mha_hd64_backward as _backward
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
