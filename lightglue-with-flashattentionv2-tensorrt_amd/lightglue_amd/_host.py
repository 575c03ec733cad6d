"""What every kernel wrapper of the package needs on the host: the error type, the status check, the
per-stream workspace and its carving, the dtype codes, the current stream and the argument checks."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib


class PluginError(RuntimeError):
    """A contract violation the reference would have turned into PLUGIN_ASSERT -> abort()."""


DT = {torch.float16: _lib.DT_HALF, torch.float32: _lib.DT_FLOAT}

# one workspace per (device, stream), as the TensorRT execution context would own
_workspaces: Dict[Tuple[int, int], torch.Tensor] = {}


def _check(status: int, what: str) -> None:
    if status != _lib.STATUS_SUCCESS:
        raise PluginError(f"{what} failed (status {status}): {_lib.last_error()}")


def call(name: str, *args) -> None:
    """The entry point `name` of the library; any status but success raises."""
    _check(getattr(_lib.load(), name)(*args), name)


def stream_of(t: torch.Tensor) -> int:
    """The handle of the current stream on t's device."""
    return torch.cuda.current_stream(t.device).cuda_stream


def _workspace(device: torch.device, stream: int, nbytes: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def carve_offsets(sizes: Sequence[int]) -> Tuple[List[int], int]:
    """Regions of `sizes` bytes laid out in order at 256-byte-aligned offsets -> (offsets, total bytes).
    Every region takes its size rounded up to 256, an empty one 256 too: no two share an address."""
    offsets, total = [], 0
    for n in sizes:
        offsets.append(total)
        total += (max(int(n), 1) + 255) // 256 * 256
    return offsets, total


def carve(device: torch.device, stream: int, nbytes_list: Sequence[int]) -> List[torch.Tensor]:
    """One request to the stream's workspace for all regions; the uint8 views of them, in the order given."""
    offsets, total = carve_offsets(nbytes_list)
    ws = _workspace(device, stream, total)
    return [ws[o:o + int(n)] for o, n in zip(offsets, nbytes_list)]


def require_gpu(name: str, t, stage: str, dtypes: Optional[Sequence[torch.dtype]] = None,
                dim: Optional[int] = None) -> None:
    """t must be a CUDA tensor (else PluginError: `stage` has no CPU fallback), of one of `dtypes` and of
    `dim` dimensions where those are given (else ValueError)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise PluginError(f"{name}: {stage} runs on the GPU only (no CPU fallback)")
    if (dtypes is not None and t.dtype not in dtypes) or (dim is not None and t.dim() != dim):
        want = " or ".join(str(d) for d in dtypes) if dtypes is not None else "any dtype"
        if dim is not None:
            want = f"a {dim}-d tensor of {want}"
        raise ValueError(f"{name}: expected {want}, got {tuple(t.shape)} {t.dtype}")
