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

Only a CUDA (HIP) kernel is registered: a CPU tensor has no implementation to dispatch to and
raises (no CPU fallback). The fake (meta) implementations give shapes/dtypes for tracing.
"""
from __future__ import annotations

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
