"""``pointnet2_ops.pointnet2_utils`` with the original's names and argument orders over ``neighbour_ops``: farthest point
sampling, the two gathers, the ball query, the three-nearest-neighbour search and interpolation of a PointNet++ layer.

Differences from the original that are deliberate: CPU tensors work (the CPU paths of the ops); inputs are
made contiguous, not asserted contiguous; index inputs may be int32 or int64 (index outputs are int32, as there); an index
outside ``[0, N)`` gives +0 and no gradient where the original reads out of bounds; ties go to the lowest index everywhere;
farthest point sampling does not skip points of squared norm <= 1e-3.  Every search, gather and interpolation runs in the
library's ops: on the accelerator a HIP kernel, never a torch composition.
"""

from __future__ import annotations

from typing import Any, Callable

import torch
from torch import nn

from pointcloudcounterfactual_amd import neighbour_ops as ops

I32, I64 = torch.int32, torch.int64


def _list64(name: str, idx: torch.Tensor) -> torch.Tensor:
    """An int32 or int64 index tensor as the int64 list the ops take."""
    if idx.dtype not in (I32, I64):
        raise TypeError(f'{name} must be int32 or int64, found {idx.dtype}')
    return idx if idx.dtype == I64 else idx.to(I64)


def furthest_point_sample(xyz: torch.Tensor, npoint: int) -> torch.Tensor:
    """``idx[B,npoint]`` int32: farthest point sampling of ``xyz[B,N,3]`` from point 0, squared distances, ties to the lowest
    index, non-finite points never chosen while another is left (``neighbour_ops.farthest_point_sample``).  ``npoint > N``
    is a ``ValueError``.  Not differentiable."""
    return ops.farthest_point_sample(xyz, npoint, start=0).to(I32)


def gather_operation(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``out[B,C,npoint] = features[B,C,N]`` along ``idx[B,npoint]``: ``group_points`` with one slot per row.
    Differentiable in ``features``; repeated indices sum, an index outside ``[0, N)`` gives +0 and no gradient."""
    if idx.dim() != 2:
        raise ValueError(f'gather_operation: expected idx[B,npoint], got {tuple(idx.shape)}')
    return ops.group_points(features, _list64('idx', idx)[:, :, None]).squeeze(3)


def ball_query(radius: float, nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor) -> torch.Tensor:
    """``idx[B,npoint,nsample]`` int32: for every centre of ``new_xyz[B,npoint,3]`` the first ``nsample`` points of
    ``xyz[B,N,3]`` in ascending index with d^2 < r^2; the remaining slots repeat the row's first hit, an empty ball is all 0
    (``neighbour_ops.ball_query`` with ``pad='first'``).  Not differentiable."""
    return ops.ball_query(xyz, new_xyz, radius, nsample, pad='first').to(I32)


def grouping_operation(features: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``out[B,C,npoint,nsample] = features[B,C,N]`` along ``idx[B,npoint,nsample]`` (``group_points``).  Differentiable
    in ``features``; a slot outside ``[0, N)`` gives +0 and no gradient."""
    return ops.group_points(features, _list64('idx', idx))


def _stable_three_nn(unknown: torch.Tensor, known: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """The CPU path of the search behind ``three_nn``: the distances of ``knn_cross``'s CPU path, clamped at 0, and a stable
    sort in place of its ``topk``, whose order among equal distances is not fixed: ties by ascending index, as on the
    accelerator."""
    d = ops.cross_square_distance(unknown.transpose(1, 2), known.transpose(1, 2)).clamp_min(0)
    d, idx = torch.sort(d, dim=-1, stable=True)
    return idx[..., :k], d[..., :k]


def three_nn(unknown: torch.Tensor, known: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """``(dist[B,n,3], idx[B,n,3] int32)``: for every point of ``unknown[B,n,3]`` its three nearest points of
    ``known[B,m,3]``, ascending distance, ties by ascending index (``knn_cross``); ``dist`` is the Euclidean distance, the
    root of the squared distance of the search.  For m < 3 the missing slots hold ``dist = +inf``, ``idx = 0``.  Not
    differentiable."""
    if unknown.dim() != 3 or known.dim() != 3 or unknown.shape[2] != 3 or known.shape[2] != 3 or unknown.shape[0] != known.shape[0] \
            or known.shape[1] < 1:
        raise ValueError(f'three_nn: expected unknown[B,n,3] and known[B,m,3] with m >= 1, got {tuple(unknown.shape)} and '
                         f'{tuple(known.shape)}')
    unknown, known = unknown.detach(), known.detach()
    b, n, _ = unknown.shape
    k = min(3, known.shape[1])
    if n == 0:
        idx, d2 = unknown.new_zeros((b, 0, k), dtype=I64), unknown.new_zeros((b, 0, k))
    elif unknown.device.type == 'cuda':
        idx, d2 = ops.knn_cross(unknown.transpose(1, 2), known.transpose(1, 2), k, return_distance=True)
    else:
        idx, d2 = _stable_three_nn(unknown, known, k)
    # The correctly rounded float32 root on either device: the accelerator's float32 sqrt may be one ulp off, the float64 root
    # rounded to float32 is not (a root of a 24-bit number is never that close to the middle between two float32 values).
    dist, idx = torch.sqrt(d2.double()).float(), idx.to(I32)
    if k < 3:
        dist = torch.cat((dist, dist.new_full((b, n, 3 - k), float('inf'))), 2)
        idx = torch.cat((idx, idx.new_zeros((b, n, 3 - k))), 2)
    return dist, idx


def three_interpolate(features: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """``out[B,c,n] = sum_j weight[B,n,j] * features[B,c,m]`` along ``idx[B,n,3]`` (``interpolate_points``).
    Differentiable in ``features`` and ``weight``; a slot outside ``[0, m)`` adds nothing and carries no gradient."""
    return ops.interpolate_points(features, _list64('idx', idx), weight)


class _FunctionStyle:
    """The original's ``torch.autograd.Function`` spelling of a util: ``Name.apply(...)`` is the function."""

    def __init__(self, fn: Callable[..., Any]) -> None:
        self.apply = fn
        self.__doc__ = fn.__doc__


FurthestPointSampling = _FunctionStyle(furthest_point_sample)
GatherOperation = _FunctionStyle(gather_operation)
ThreeNN = _FunctionStyle(three_nn)
ThreeInterpolate = _FunctionStyle(three_interpolate)
GroupingOperation = _FunctionStyle(grouping_operation)
BallQuery = _FunctionStyle(ball_query)


class QueryAndGroup(nn.Module):
    """``forward(xyz[B,N,3], new_xyz[B,npoint,3], features[B,C,N] or None) -> [B,3+C,npoint,nsample]``: the ball query around
    every centre, then channels 0-2 the grouped coordinates minus the centre and behind them the grouped features, filled by
    one grouping op (``neighbour_ops.query_and_group``: no ``cat`` on the accelerator).  ``use_xyz=False``: the features
    only; ``features=None``: the coordinates only."""

    def __init__(self, radius: float, nsample: int, use_xyz: bool = True) -> None:
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz: torch.Tensor, new_xyz: torch.Tensor, features: torch.Tensor | None = None) -> torch.Tensor:
        if features is None:
            assert self.use_xyz, 'Cannot have not features and not use xyz as a feature!'
        if not self.use_xyz:
            return ops.group_points(features, ops.ball_query(xyz, new_xyz, self.radius, self.nsample, pad='first'))
        return ops.query_and_group(xyz, new_xyz, features, self.radius, self.nsample, pad='first').grouped


class GroupAll(nn.Module):
    """``forward(xyz[B,N,3], new_xyz (ignored), features[B,C,N] or None) -> [B,3+C,1,N]``: the whole cloud as one group,
    coordinates not centred."""

    def __init__(self, use_xyz: bool = True) -> None:
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz: torch.Tensor, new_xyz: torch.Tensor | None, features: torch.Tensor | None = None) -> torch.Tensor:
        grouped_xyz = xyz.transpose(1, 2).unsqueeze(2)
        if features is None:
            assert self.use_xyz, 'Cannot have not features and not use xyz as a feature!'
            return grouped_xyz
        grouped_features = features.unsqueeze(2)
        return torch.cat((grouped_xyz, grouped_features), 1) if self.use_xyz else grouped_features
