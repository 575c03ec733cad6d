"""torch.library operators over the plugin C ABI ("the caller is its own
PyTorch-ROCm module via a torch.library op that invokes enqueue on torch.cuda.current_stream()").

* ``torch.ops.lightglue_amd.mha_hd64(q, k, v) -> o``: the plugin's ``enqueue`` (the TensorRT node
  ``CustomOp::MHAHeadDim64``, lightglue_pytorch_with_plugin/lightglue.py:16-46): [1, 4, N, 64],
  all fp16 (-> fp16) or all fp32 (-> fp32).
* ``torch.ops.lightglue_amd.mha_hd64_grouped(qs, ks, vs) -> os``: up to any number of independent
  calls in grouped launches (4 per launch), e.g. the self0/self1 or the two cross directions of a
  LightGlue layer.
* ``torch.ops.lightglue_amd.mha_hd64_grouped_lens(qs, ks, vs, lens) -> os`` and
  ``mha_hd64_grouped_qkv_lens(qs, ks, vs, q_lens, kv_lens)``: the same on ragged batches, with int32
  device tables of per-item key (and query-row) counts (fp16 only).

Only a CUDA (HIP) kernel is registered: a CPU tensor has no implementation to dispatch to and
raises (no CPU fallback). The fake (meta) implementations give shapes/dtypes for tracing.
"""
from __future__ import annotations

from typing import List

import torch

from .plugin import mha_hd64 as _enqueue
from .plugin import mha_hd64_grouped as _grouped


@torch.library.custom_op("lightglue_amd::mha_hd64", mutates_args=(), device_types="cuda")
def mha_hd64_op(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor) -> torch.Tensor:
    return _enqueue(query.contiguous(), key.contiguous(), value.contiguous())


@mha_hd64_op.register_fake
def _(query, key, value):
    return torch.empty_like(query, memory_format=torch.contiguous_format)


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
