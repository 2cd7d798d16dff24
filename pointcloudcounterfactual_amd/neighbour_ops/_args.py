# ---- argument checks and list helpers every op family shares ------------------------------------------------------------

from __future__ import annotations

import numbers
from typing import Any

import torch

from pointcloudcounterfactual_amd import _lib

_L = _lib.lib
F32, I32, I64 = torch.float32, torch.int32, torch.int64


def _same_device(name: str, t: torch.Tensor, dev: torch.device) -> None:
    """``t`` is on ``dev``, or the ``RuntimeError`` of ``_lib.ptr``."""
    if t.device != dev:
        if dev.type == 'cuda' and t.device.type != 'cuda':
            raise RuntimeError(f'{name} must be a CUDA tensor')
        raise RuntimeError(f'{name} is on {t.device}, expected {dev}')


def _float32(name: str, t: torch.Tensor) -> None:
    """``t`` is float32, or the ``RuntimeError`` of ``_lib.ptr``."""
    if t.dtype != F32:
        raise RuntimeError(f'{name} must be {F32}, found {t.dtype}')


def _cloud_arg(what: str, name: str, xyz: torch.Tensor, b: int | None = None, min_n: int = 1, axis: str = 'N') -> tuple[int, int]:
    """``xyz[B,N,3]`` with ``N >= min_n`` (and the given ``B``), or the ``ValueError`` of ``what``: ``(b, n)``.  ``name`` and
    ``axis`` are what the message calls the tensor and its point axis."""
    if xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.shape[1] < min_n or (b is not None and xyz.shape[0] != b):
        lay = f'{name}[B,{axis},3]' if b is None else f'{name}[B = {b},{axis},3]'
        raise ValueError(f'{what}: expected {lay}{f" with {axis} >= {min_n}" if min_n else ""}, got {tuple(xyz.shape)}')
    return xyz.shape[0], xyz.shape[1]


def _features_arg(what: str, features: torch.Tensor, name: str = 'features') -> tuple[int, int, int]:
    """``features[B,C,N]`` with ``C >= 1`` and ``N >= 1``, or the ``ValueError`` of ``what``: ``(b, c, n)``."""
    if features.dim() != 3 or features.shape[1] < 1 or features.shape[2] < 1:
        raise ValueError(f'{what}: expected {name}[B,C,N] with C >= 1 and N >= 1, got {tuple(features.shape)}')
    b, c, n = features.shape
    return b, c, n


def _list_arg(what: str, idx: torch.Tensor, b: int) -> tuple[int, int]:
    """The shape of an index list ``idx[B,M,k]`` with ``k >= 1`` and ``M * k < 2^31``, or the ``ValueError`` of ``what``:
    ``(m, k)``.  Its dtype and device are ``_list_on``'s: every caller checks other shapes in between."""
    if idx.dim() != 3 or idx.shape[0] != b or idx.shape[2] < 1:
        raise ValueError(f'{what}: expected idx[B = {b},M,k] with k >= 1, got {tuple(idx.shape)}')
    m, k = idx.shape[1], idx.shape[2]
    if m * k >= 1 << 31:
        raise ValueError(f'{what}: idx[B,M,k] with M * k >= 2^31, got {tuple(idx.shape)}')
    return m, k


def _list_on(idx: torch.Tensor, dev: torch.device) -> None:
    """``idx`` is int64 and on ``dev``, or the ``RuntimeError`` of ``_lib.ptr``."""
    if idx.dtype != I64:
        raise RuntimeError(f'idx must be {I64}, found {idx.dtype}')
    _same_device('idx', idx, dev)


def _k_arg(what: str, k: Any) -> None:
    """``k`` is an integer in ``[1, 128]`` (what ``knn`` and ``knn_cross`` search), or the ``ValueError`` of ``what``."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= 128:
        raise ValueError(f'{what}: k must be an integer in [1, 128], got {k!r}')


def _canonical_nan(t: torch.Tensor) -> torch.Tensor:
    """A NaN becomes the word 0x7fc00000."""
    return torch.where(torch.isnan(t), torch.full((), float('nan'), dtype=t.dtype, device=t.device), t)


def _zero(t: torch.Tensor) -> torch.Tensor:
    """The scalar 0 of ``t``'s dtype on its device."""
    return torch.zeros((), dtype=t.dtype, device=t.device)


def _valid_slots(idx: torch.Tensor, n: int) -> torch.Tensor:
    """Which slots of a list name one of ``n`` points: ``0 <= idx < n``."""
    return (idx >= 0) & (idx < n)


def _list_slots(idx: torch.Tensor, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(valid, safe)``: ``_valid_slots``, and the list with index 0 standing in for a slot that is no point, so that every
    slot can be gathered and the result masked."""
    valid = _valid_slots(idx, n)
    return valid, torch.where(valid, idx, torch.zeros_like(idx))


def _slot_values(x: torch.Tensor, safe: torch.Tensor, rel: torch.Tensor | None) -> torch.Tensor:
    """``v[B,C,M,k] = x[b,ch,safe] (+ rel)`` along the ``safe`` list of ``_list_slots``."""
    b, c, _ = x.shape
    m, k = safe.shape[1:]
    v = torch.gather(x, 2, safe.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)
    return v if rel is None else v + rel
