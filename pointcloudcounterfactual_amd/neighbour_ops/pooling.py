# ---- grid pooling: one slot per occupied cell of the voxel grid (PTv2's partition-based pooling, KPConv's grid subsampling) ----

from __future__ import annotations

import numbers
from typing import Any, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import (F32, I32, I64, _L, _canonical_nan, _features_arg, _float32, _same_device,
                                                              _valid_slots, _zero)
from pointcloudcounterfactual_amd.neighbour_ops.grouping import group_points
from pointcloudcounterfactual_amd.neighbour_ops.voxel import VoxelIndex, _index_arg, _voxel_cloud_args

_REDUCE = {'mean': 0, 'sum': 1, 'max': 2}  # pcc_segment_pool's modes


class GridIndex(NamedTuple):
    """What ``grid_cluster`` returns: the partition of a cloud into the occupied cells of a grid, padded to ``m`` slots."""

    cluster: torch.Tensor  # [B,N] int32 slot of every point: the rank of its cell among the occupied ones, -1 if dropped or non-finite
    seg: torch.Tensor      # [B,m+1] int32: the points of slot r are order[seg[r] : seg[r + 1]]; a padded slot's run is empty
    count: torch.Tensor    # [B] int32 occupied cells of the cloud (count > m: cells were dropped)
    order: torch.Tensor    # [B,N] int32 the permutation of the VoxelIndex


class GridPooled(NamedTuple):
    """What ``grid_pool`` returns."""

    xyz: torch.Tensor              # [B,m,3] mean coordinate of every slot's points, NaN in a padded slot
    features: torch.Tensor | None  # [B,C,m] pooled features, +0 in a padded slot
    index: GridIndex
    count: torch.Tensor            # [B] int32, index.count


def _grid_pool_size_args(what: str, b: int, n: int) -> None:
    """The size limits of the three entry points (include/pcc_neighbour.h)."""
    if b > 65535 or b * (n + 1) >= 1 << 31:
        raise ValueError(f'{what}: too large (B <= 65535, B * (N + 1) < 2^31), got B = {b}, N = {n}')


def _capacity_arg(what: str, m: Any, n: int) -> None:
    if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= n:
        raise ValueError(f'{what}: m must be None or an integer in [1, N = {n}], got {m!r}')


def _reduce_arg(what: str, reduce: Any) -> int:
    if not isinstance(reduce, str) or reduce not in _REDUCE:
        raise ValueError(f"{what}: reduce must be 'mean', 'sum' or 'max', got {reduce!r}")
    return _REDUCE[reduce]


def _grid_index_args(gindex: Any, what: str, b: int, n: int, dev: torch.device) -> int:
    """``gindex`` is a ``GridIndex`` of ``b`` clouds of ``n`` points on ``dev``: its capacity ``m``."""
    if not isinstance(gindex, GridIndex):
        raise ValueError(f'{what}: expected a GridIndex, got {type(gindex).__name__}')
    cluster, seg, count, order = gindex
    if tuple(cluster.shape) != (b, n) or tuple(order.shape) != (b, n):
        raise ValueError(f'{what}: expected index.cluster and index.order [B,N] = {(b, n)}, got {tuple(cluster.shape)} and {tuple(order.shape)}')
    if seg.dim() != 2 or seg.shape[0] != b or not 2 <= seg.shape[1] <= n + 1:
        raise ValueError(f'{what}: expected index.seg[B = {b},m + 1] with 1 <= m <= N = {n}, got {tuple(seg.shape)}')
    if tuple(count.shape) != (b,):
        raise ValueError(f'{what}: expected index.count[B = {b}], got {tuple(count.shape)}')
    for name, t in (('index.cluster', cluster), ('index.seg', seg), ('index.count', count), ('index.order', order)):
        if t.dtype != I32:
            raise RuntimeError(f'{name} must be {I32}, found {t.dtype}')
        _same_device(name, t, dev)
    return seg.shape[1] - 1


def torch_grid_cluster(index: VoxelIndex, m: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The rule of ``pcc_grid_cluster`` in torch: ``(cluster[B,N], seg[B,m+1], count[B])`` int32.  Integers only, so every
    word is the kernel's."""
    b, n = index.cell.shape
    order = index.order.to(I64)
    sorted_cell = torch.gather(index.cell.to(I64), 1, order)
    valid = sorted_cell >= 0
    is_start = valid.clone()
    is_start[:, 1:] &= sorted_cell[:, 1:] != sorted_cell[:, :-1]
    rank = torch.cumsum(is_start.to(I64), 1) - 1  # of the cell of every sorted position
    count, finite = is_start.sum(1), valid.sum(1)
    cluster = torch.empty((b, n), dtype=I64)
    cluster.scatter_(1, order, torch.where(valid & (rank < m), rank, torch.full((), -1, dtype=I64)))
    # starts[r]: the first position of rank r, F behind the last rank; its first m + 1 entries are seg at capacity m
    pos = torch.arange(n)[None, :].expand(b, n)
    starts = finite[:, None].expand(b, n + 1).clone()
    starts.scatter_(1, torch.where(is_start, rank, torch.full((), n, dtype=I64)), torch.where(is_start, pos, finite[:, None].expand(b, n)))
    return cluster.to(I32), starts[:, :m + 1].to(I32).contiguous(), count.to(I32)


def torch_segment_pool(features: torch.Tensor, order: torch.Tensor, seg: torch.Tensor, mode: int) -> tuple[torch.Tensor, torch.Tensor | None]:
    """The rule of ``pcc_segment_pool`` in torch: ``(out[B,C,m], arg[B,C,m] int32 or None)``.  One pass per rank within the
    run -- a pass touches every slot at most once, so every slot chains its points in ascending position --, the slots
    ordered by the length of their runs so that a pass visits only those it still has a point for."""
    b, c, n = features.shape
    m = seg.shape[1] - 1
    features = features.detach()
    seg64, order64 = seg.to(I64), order.to(I64)
    start = seg64[:, :-1].clamp(0, n)
    length = (seg64[:, 1:].clamp(0, n) - start).clamp(min=0)  # [B,m]
    out = torch.zeros((b, c, m), dtype=features.dtype)
    arg = torch.full((b, c, m), -1, dtype=I64) if mode == 2 else None
    flat_len = length.reshape(-1)
    by_len = torch.argsort(flat_len, descending=True, stable=True)
    bi_all, ri_all = by_len // m, by_len % m
    longest = int(flat_len.max()) if flat_len.numel() else 0
    longer = flat_len.numel() - torch.cumsum(torch.bincount(flat_len, minlength=longest + 1), 0)  # [j]: slots with len > j
    for j, live in enumerate(longer[:longest].tolist()):
        bi, ri = bi_all[:live], ri_all[:live]
        p = order64[bi, start[bi, ri] + j]
        v = features[bi, :, p]  # [live, C]
        cur = out[bi, :, ri]
        if mode == 2:
            at = arg[bi, :, ri]
            take = (at < 0) | (~torch.isnan(cur) & (torch.isnan(v) | (v > cur)))
            out[bi, :, ri] = torch.where(take, v, cur)
            arg[bi, :, ri] = torch.where(take, p[:, None], at)
        else:
            out[bi, :, ri] = cur + v
    if mode == 0:
        some = (length > 0)[:, None, :]
        out = torch.where(some, out / torch.where(some, length[:, None, :], torch.ones((), dtype=I64)).to(features.dtype),
                          _zero(features))
    return (out, arg.to(I32)) if mode == 2 else (_canonical_nan(out), None)


def torch_segment_pool_bwd(grad: torch.Tensor, cluster: torch.Tensor, seg: torch.Tensor, arg: torch.Tensor | None, mode: int) -> torch.Tensor:
    """The rule of ``pcc_segment_pool_bwd`` in torch: a gather along ``cluster``, ``[B,C,N]``."""
    b, c, m = grad.shape
    n = cluster.shape[1]
    slot = cluster.to(I64)
    ok = _valid_slots(slot, m)
    at = torch.where(ok, slot, _zero(slot))[:, None, :].expand(b, c, n)
    g = torch.gather(grad, 2, at)
    if mode == 0:
        seg64 = seg.to(I64)
        length = torch.gather(seg64[:, 1:] - seg64[:, :-1], 1, at[:, 0])
        g = g / torch.where(ok, length, torch.ones((), dtype=I64)).to(grad.dtype)[:, None, :]
    elif mode == 2:
        g = torch.where(torch.gather(arg.to(I64), 2, at) == torch.arange(n)[None, None, :], g, _zero(grad))
    return torch.where(ok[:, None, :], g, _zero(grad))


def grid_cluster(index_or_xyz: Any, resolution: int | None = None, lo: float = -0.5, extent: float = 1.0, m: int | None = None) -> GridIndex:
    """The partition of every cloud into the occupied cells of the grid of ``voxel_index``:
    ``GridIndex(cluster[B,N], seg[B,m+1], count[B], order[B,N])``, all int32.  ``index_or_xyz`` is the ``VoxelIndex`` of the
    clouds (``resolution``, if given, must be its own) or the clouds ``xyz[B,N,3]``, indexed here.  The occupied cells of a
    cloud are its slots, in ascending cell; ``m`` is the number of slots every cloud is padded -- or cut -- to.  With
    ``m=None`` it is the largest ``count`` of the batch (at least 1), which is read from the device: ONE host
    synchronisation; a given ``m`` (``1 <= m <= N``) synchronises nothing, and ``count > m`` then tells that the cells of
    rank ``m`` and above were dropped (their points have ``cluster = -1``).  A non-finite point has ``cluster = -1``.  Every
    word is fixed by the cloud alone (``pcc_grid_cluster``, include/pcc_neighbour.h); CPU tensors take the same rule in torch
    and give the same integers.  Carries no gradient."""
    what = 'grid_cluster'
    index, _ = _index_arg(what, index_or_xyz, resolution, lo, extent, check_n=None if m is None else lambda n: _capacity_arg(what, m, n))
    b, n = index.cell.shape
    _grid_pool_size_args(what, b, n)
    dev = index.cell.device
    cap = n if m is None else int(m)
    if b == 0:
        return GridIndex(torch.zeros((0, n), dtype=I32, device=dev), torch.zeros((0, (1 if m is None else cap) + 1), dtype=I32, device=dev),
                         torch.zeros((0,), dtype=I32, device=dev), index.order)
    if dev.type == 'cuda':
        cell, order = index.cell.contiguous(), index.order.contiguous()
        cluster, seg = torch.empty((b, n), dtype=I32, device=dev), torch.empty((b, cap + 1), dtype=I32, device=dev)
        count = torch.empty((b,), dtype=I32, device=dev)
        call(_L.pcc_grid_cluster, what, dev, b, n, cap, ptr(cell, 'index.cell', I32, dev), ptr(order, 'index.order', I32, dev),
             ptr(cluster, 'cluster', I32, dev), ptr(seg, 'seg', I32, dev), ptr(count, 'count', I32, dev))
    else:
        order = index.order
        cluster, seg, count = torch_grid_cluster(index, cap)
    if m is None:  # (at capacity N nothing was dropped: the first count.max() + 1 entries are the index at that capacity)
        seg = seg[:, :max(1, int(count.max().item())) + 1].contiguous()
    return GridIndex(cluster, seg, count, order)


class SegmentPooled(Function):
    """``SegmentPooled.apply(features, cluster, seg, order, mode)``: ``pcc_segment_pool``; the backward is
    ``pcc_segment_pool_bwd`` on the saved ``cluster``, ``seg`` and (max) ``arg``, run only when the gradient of ``features``
    is asked for.  CPU tensors take ``torch_segment_pool`` / ``torch_segment_pool_bwd``.  The arguments have been checked."""

    @staticmethod
    def forward(ctx: Any, features: torch.Tensor, cluster: torch.Tensor, seg: torch.Tensor, order: torch.Tensor, mode: int) -> torch.Tensor:
        features, cluster, seg, order = features.contiguous(), cluster.contiguous(), seg.contiguous(), order.contiguous()
        b, c, n = features.shape
        m = seg.shape[1] - 1
        dev = features.device
        if dev.type == 'cuda':
            xp, op, sp = ptr(features, 'features', F32, dev), ptr(order, 'index.order', I32, dev), ptr(seg, 'index.seg', I32, dev)
            out = torch.empty((b, c, m), dtype=F32, device=dev)
            arg = torch.empty((b, c, m), dtype=I32, device=dev) if mode == 2 else None
            call(_L.pcc_segment_pool, 'segment_pool', dev, b, c, n, m, mode, xp, op, sp, ptr(out, 'out', F32, dev), ptr(arg, 'arg', I32, dev))
        else:
            out, arg = torch_segment_pool(features, order, seg, mode)
        ctx.save_for_backward(cluster, seg, arg)
        ctx.n, ctx.mode = n, mode
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, None, None, None, None]:
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        cluster, seg, arg = ctx.saved_tensors
        grad = grad.contiguous()
        b, c, m = grad.shape
        dev = grad.device
        if dev.type != 'cuda':
            return torch_segment_pool_bwd(grad, cluster, seg, arg, ctx.mode), None, None, None, None
        gx = torch.empty((b, c, ctx.n), dtype=F32, device=dev)
        call(_L.pcc_segment_pool_bwd, 'segment_pool_bwd', dev, b, c, ctx.n, m, ctx.mode, ptr(cluster, 'index.cluster', I32, dev),
             ptr(seg, 'index.seg', I32, dev), ptr(arg, 'arg', I32, dev), ptr(grad, 'grad', F32, dev), ptr(gx, 'grad_features', F32, dev))
        return gx, None, None, None, None


def segment_pool(features: torch.Tensor, gindex: GridIndex, reduce: str = 'mean') -> torch.Tensor:
    """``out[B,C,m]``: the features ``features[B,C,N]`` float32 of the points of every slot of ``gindex`` (``grid_cluster``)
    reduced to one value -- ``'mean'``: summed in ascending point index from +0.0 and divided once, word for word what
    ``voxelize`` writes into that cell; ``'sum'``: the same without the division; ``'max'``: ``torch.max`` over the slot's
    points in ascending point index (the first NaN wins, else the greatest value, the lowest index among equal ones).  A
    padded slot is +0.0.  Nothing is atomic, so every word is fixed (``pcc_segment_pool``, include/pcc_neighbour.h);
    differentiable in ``features`` by a gather: the points of a slot share its gradient (divided by their number for the
    mean), the max hands it to the point it took; a dropped or non-finite point gets +0.0.  The HIP kernels on the
    accelerator, the same rule as a torch composition for CPU tensors: outputs and gradients agree word for word."""
    what = 'segment_pool'
    b, c, n = _features_arg(what, features)
    _float32('features', features)
    m = _grid_index_args(gindex, what, b, n, features.device)
    mode = _reduce_arg(what, reduce)
    _grid_pool_size_args(what, b, n)
    if b == 0:
        return torch.zeros((0, c, m), dtype=F32, device=features.device)
    return SegmentPooled.apply(features, gindex.cluster, gindex.seg, gindex.order, mode)


def grid_pool(xyz: torch.Tensor, features: torch.Tensor | None, resolution: int, lo: float = -0.5, extent: float = 1.0,
              m: int | None = None, reduce: str = 'max') -> GridPooled:
    """Partition-based pooling (Point Transformer V2's ``GridPool``) in one call: the clouds ``xyz[B,N,3]`` are cut by the
    grid of ``voxel_index(xyz, resolution, lo, extent)`` and every occupied cell becomes one point --
    ``GridPooled(xyz[B,m,3], features[B,C,m] or None, index, count)``: the mean coordinate of the cell's points, their
    features ``features[B,C,N]`` reduced by ``reduce`` (``segment_pool``), the ``GridIndex`` for ``grid_unpool`` on the way
    back up, and the number of occupied cells per cloud.  ``m`` as in ``grid_cluster``: ``None`` costs one host
    synchronisation.  A padded slot (``>= count``) holds NaN coordinates (the word 0x7fc00000) and +0 features: such a
    point is nobody's neighbour in ``ball_query``, never enters a ``knn`` / ``knn_cross`` list, is skipped by
    ``farthest_point_sample`` and has cell -1 in ``voxel_index``, so the pooled cloud can be fed to every op unchanged.
    Differentiable in ``features`` and, through the centres, in ``xyz``, with the partition held constant."""
    what = 'grid_pool'
    b, n = _voxel_cloud_args(xyz, what)
    mode = _reduce_arg(what, reduce)
    if features is not None:
        _features_arg(what, features)
        if features.shape[0] != b or features.shape[2] != n:
            raise ValueError(f'{what}: expected features[B = {b},C,N = {n}], got {tuple(features.shape)}')
        _float32('features', features)
        _same_device('features', features, xyz.device)
    gindex = grid_cluster(xyz, resolution, lo, extent, m)
    cap = gindex.seg.shape[1] - 1
    dev = xyz.device
    if b == 0:
        centres = torch.zeros((0, cap, 3), dtype=F32, device=dev)
        pooled = None if features is None else torch.zeros((0, features.shape[1], cap), dtype=F32, device=dev)
        return GridPooled(centres, pooled, gindex, gindex.count)
    centres = SegmentPooled.apply(xyz.transpose(1, 2), gindex.cluster, gindex.seg, gindex.order, 0).transpose(1, 2)
    padded = torch.arange(cap, device=dev)[None, :] >= gindex.count[:, None]
    centres = torch.where(padded[:, :, None], torch.full((), float('nan'), dtype=F32, device=dev), centres)
    pooled = None if features is None else SegmentPooled.apply(features, gindex.cluster, gindex.seg, gindex.order, mode)
    return GridPooled(centres, pooled, gindex, gindex.count)


def grid_subsample(xyz: torch.Tensor, resolution: int, lo: float = -0.5, extent: float = 1.0, m: int | None = None) -> torch.Tensor:
    """KPConv's ``grid_subsampling``: the barycentre of the points of every occupied cell, ``[B,m,3]``, NaN in the slots
    behind a cloud's last occupied cell -- ``grid_pool(xyz, None, ...).xyz``."""
    return grid_pool(xyz, None, resolution, lo, extent, m).xyz


def grid_unpool(pooled: torch.Tensor, gindex: GridIndex) -> torch.Tensor:
    """PTv2's map unpooling: ``out[B,C,N]``, every point takes the value ``pooled[B,C,m]`` holds for its slot --
    ``group_points`` along ``gindex.cluster`` with k = 1.  A point of a dropped or non-finite cell gets +0 and carries no
    gradient.  Differentiable in ``pooled``."""
    what = 'grid_unpool'
    if not isinstance(gindex, GridIndex):
        raise ValueError(f'{what}: expected a GridIndex, got {type(gindex).__name__}')
    if gindex.cluster.dim() != 2 or gindex.cluster.shape[1] < 1:
        raise ValueError(f'{what}: expected index.cluster[B,N] with N >= 1, got {tuple(gindex.cluster.shape)}')
    b, n = gindex.cluster.shape
    m = _grid_index_args(gindex, what, b, n, pooled.device)
    if pooled.dim() != 3 or pooled.shape[0] != b or pooled.shape[1] < 1 or pooled.shape[2] != m:
        raise ValueError(f'{what}: expected pooled[B = {b},C,m = {m}] with C >= 1, got {tuple(pooled.shape)}')
    _float32('pooled', pooled)
    return group_points(pooled, gindex.cluster.to(I64)[:, :, None])[:, :, :, 0]
