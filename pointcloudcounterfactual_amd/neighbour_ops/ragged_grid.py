# ---- ragged grid pooling: the grid index of a packed batch, clouds of any size (PTv2 / PTv3's GridPool on scenes) ----------

from __future__ import annotations

import math
import numbers
from typing import Any, NamedTuple

import numpy as np
import torch

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import F32, I32, I64, _L, _float32, _same_device
from pointcloudcounterfactual_amd.neighbour_ops.pooling import GridIndex, SegmentPooled, _capacity_arg, _reduce_arg, grid_unpool
from pointcloudcounterfactual_amd.neighbour_ops.ragged import _i32, _packed_arg, _valid_offsets

MAX_AXIS_BITS = 16      # pcc_grid_cluster_ragged: cells per axis up to 2^16 (include/pcc_neighbour.h)
GRID_RAGGED_TILE = 2048  # PCC_GRID_RAGGED_TILE: the keys one workgroup of the sort ranks


class RaggedGrid(NamedTuple):
    """What ``grid_cluster_ragged`` returns: the partition of a packed batch into the occupied cells of every cloud's grid."""

    index: GridIndex        # cluster[1,n], seg[1,m+1], count[1], order[1,n] int32: what segment_pool and grid_unpool take (b = 1)
    coord: torch.Tensor     # [m,4] int32 (cloud, i, j, k) of every slot, -1 in a padded one
    offset: torch.Tensor    # [B] int32 cumulative ends of the clouds of the pooled level: the next stage's offset
    count: torch.Tensor     # [1] int32 occupied cells of the batch (count > m: cells were dropped), index.count


class RaggedGridPooled(NamedTuple):
    """What ``grid_pool_ragged`` returns."""

    xyz: torch.Tensor              # [m,3] barycentre of every slot's points, NaN in a padded slot
    features: torch.Tensor | None  # [m,C] pooled features, +0 in a padded slot
    offset: torch.Tensor           # [B] int32, grid.offset
    grid: RaggedGrid


def _cloud_bits(b: int) -> int:
    return int(b).bit_length()


def default_axis_bits(b: int) -> int:
    """The widest cell coordinate a 63-bit key leaves beside the cloud field of a batch of ``b`` clouds, 16 at the most."""
    return min(MAX_AXIS_BITS, (63 - _cloud_bits(b)) // 3)


def _grid_ragged_args(what: str, xyz: torch.Tensor, offset: torch.Tensor, size: Any, start: torch.Tensor | None, m: Any,
                      axis_bits: Any) -> tuple[int, int, float, int]:
    """The checks the ragged grid ops make before anything runs: ``(b, n, size as the float32 the library receives, axis_bits)``."""
    b, n = _packed_arg(what, 'xyz', xyz, 'offset', offset)
    if n < 1 or n + 1 >= 1 << 31:
        raise ValueError(f'{what}: expected xyz[n,3] with 1 <= n and n + 1 < 2^31, got {tuple(xyz.shape)}')
    if not 1 <= b <= 65535:
        raise ValueError(f'{what}: expected offset[B] with 1 <= B <= 65535, got {tuple(offset.shape)}')
    if isinstance(size, bool) or not isinstance(size, numbers.Real):
        raise ValueError(f'{what}: size must be a number, got {size!r}')
    with np.errstate(over='ignore'):
        s32 = float(np.float32(size))
    if not math.isfinite(s32) or not s32 > 0.0:
        raise ValueError(f'{what}: size must be finite and > 0 as a float32, got {size!r}')
    if axis_bits is None:
        axis_bits = default_axis_bits(b)
    elif isinstance(axis_bits, bool) or not isinstance(axis_bits, numbers.Integral) or not 1 <= axis_bits <= MAX_AXIS_BITS:
        raise ValueError(f'{what}: axis_bits must be None or an integer in [1, {MAX_AXIS_BITS}], got {axis_bits!r}')
    if _cloud_bits(b) + 3 * int(axis_bits) > 63:
        raise ValueError(f'{what}: the key is wider than 63 bits: {_cloud_bits(b)} bits for B = {b} clouds and 3 * axis_bits = {3 * int(axis_bits)}')
    if m is not None:
        _capacity_arg(what, m, n)
    if start is not None:
        if not isinstance(start, torch.Tensor) or tuple(start.shape) != (b, 3):
            raise ValueError(f'{what}: expected start[B = {b},3], got {tuple(start.shape) if isinstance(start, torch.Tensor) else type(start).__name__}')
        _float32('start', start)
        _same_device('start', start, xyz.device)
    return b, n, s32, int(axis_bits)


def ragged_grid_start(xyz: torch.Tensor, offset: torch.Tensor) -> torch.Tensor:
    """``start[B,3]`` float32: per cloud and axis the minimum of the finite coordinates, on ``xyz``'s device and without a
    synchronisation (a minimum: the order of a scatter cannot change it).  The row of a cloud without a finite coordinate on
    an axis is +inf there: every point of that cloud is dropped on it anyway.  For offsets that do not ascend the rows are
    dealt by the running maximum of the clipped offsets."""
    b, n = offset.shape[0], xyz.shape[0]
    x = xyz.detach()
    ends = torch.cummax(offset.detach().to(I64).clamp(0, n), 0).values
    cloud = torch.bucketize(torch.arange(n, dtype=I64, device=x.device), ends, right=True)  # (b: a row of no cloud)
    inf = torch.full((), float('inf'), dtype=F32, device=x.device)
    start = torch.full((b + 1, 3), float('inf'), dtype=F32, device=x.device)
    start.scatter_reduce_(0, cloud[:, None].expand(n, 3), torch.where(torch.isfinite(x), x, inf), 'amin')
    return start[:b].contiguous()


def torch_grid_cluster_ragged(xyz: torch.Tensor, offset: torch.Tensor, start: torch.Tensor, size: float, m: int,
                              axis_bits: int) -> tuple[torch.Tensor, ...]:
    """The rule of ``pcc_grid_cluster_ragged`` (include/pcc_neighbour.h) in torch; CPU path of ``grid_cluster_ragged``:
    ``(cluster[n], order[n], seg[m+1], coord[m,4], new_offset[B], n_cells[1])`` int32.  The cells come from the float32
    subtraction, division and floor (torch's are IEEE), the keys are int64 and the sort is stable, so every word is the
    kernel's.  The offsets are validated -- non-decreasing from 0 and ending at or before the number of rows; the rows behind
    the last one belong to no cloud --, not clipped."""
    what = 'grid_cluster_ragged'
    n, b = xyz.shape[0], offset.shape[0]
    ends = _valid_offsets(what, 'offset', offset)
    if ends[-1] > n:
        raise ValueError(f'{what}: offset must end at or before {n}, got {ends[1:]}')
    dev = xyz.device
    x = xyz.detach()
    pos = torch.arange(n, dtype=I64, device=dev)
    cloud = torch.bucketize(pos, torch.tensor(ends[1:], dtype=I64, device=dev), right=True)  # the ends <= i; b: no cloud
    in_cloud = cloud < b
    t = (x - start.detach()[cloud.clamp(max=b - 1)]) / torch.tensor(size, dtype=F32, device=dev)
    f = torch.floor(t)
    valid = in_cloud & ((t >= 0) & (f < float(1 << axis_bits))).all(1)
    q = torch.where(valid[:, None], f, torch.zeros((), dtype=F32, device=dev)).to(I64)
    dropped = b << (3 * axis_bits)
    key = (cloud << (3 * axis_bits)) | (q[:, 0] << (2 * axis_bits)) | (q[:, 1] << axis_bits) | q[:, 2]
    key = torch.where(valid, key, torch.full((), dropped, dtype=I64, device=dev))
    key, order = torch.sort(key, stable=True)
    kept = key < dropped
    head = kept.clone()
    head[1:] &= key[1:] != key[:-1]
    rank = torch.cumsum(head.to(I64), 0) - 1
    u, v = head.sum(), kept.sum()
    cluster = torch.empty((n,), dtype=I64, device=dev)
    cluster[order] = torch.where(kept & (rank < m), rank, torch.full((), -1, dtype=I64, device=dev))
    starts = v.expand(n + 1).clone()  # [r]: the first position of rank r, the valid points behind the last rank
    starts[rank[head]] = pos[head]
    hk, hr = key[head], rank[head]
    mask = (1 << axis_bits) - 1
    all_coord = torch.stack((hk >> (3 * axis_bits), (hk >> (2 * axis_bits)) & mask, (hk >> axis_bits) & mask, hk & mask), 1)
    coord = torch.full((m, 4), -1, dtype=I64, device=dev)
    coord[hr[hr < m]] = all_coord[hr < m]
    new_offset = torch.cumsum(torch.bincount(all_coord[:, 0], minlength=b)[:b], 0).clamp(max=m)
    return (cluster.to(I32), order.to(I32), starts[:m + 1].to(I32).contiguous(), coord.to(I32), new_offset.to(I32), u.reshape(1).to(I32))


def hip_grid_cluster_ragged(xyz: torch.Tensor, offset: torch.Tensor, start: torch.Tensor, size: float, m: int,
                            axis_bits: int) -> tuple[torch.Tensor, ...]:
    """``pcc_grid_cluster_ragged`` on checked arguments (``_grid_ragged_args``): the tuple of ``torch_grid_cluster_ragged``.
    Nothing is read on the host."""
    dev = xyz.device
    xyz, offset, start = xyz.detach().contiguous(), _i32(offset), start.detach().contiguous()
    b, n = offset.shape[0], xyz.shape[0]
    # (checked before anything is allocated on the device)
    xp, op, sp = ptr(xyz, 'xyz', F32, dev), ptr(offset, 'offset', I32, dev), ptr(start, 'start', F32, dev)
    cluster, order = torch.empty((n,), dtype=I32, device=dev), torch.empty((n,), dtype=I32, device=dev)
    seg, coord = torch.empty((m + 1,), dtype=I32, device=dev), torch.empty((m, 4), dtype=I32, device=dev)
    new_offset, n_cells = torch.empty((b,), dtype=I32, device=dev), torch.empty((1,), dtype=I32, device=dev)
    call(_L.pcc_grid_cluster_ragged, 'grid_cluster_ragged', dev, b, n, m, axis_bits, xp, op, sp, size, ptr(cluster, 'cluster', I32, dev),
         ptr(order, 'order', I32, dev), ptr(seg, 'seg', I32, dev), ptr(coord, 'coord', I32, dev), ptr(new_offset, 'new_offset', I32, dev),
         ptr(n_cells, 'n_cells', I32, dev))
    return cluster, order, seg, coord, new_offset, n_cells


def grid_cluster_ragged(xyz: torch.Tensor, offset: torch.Tensor, size: float, start: torch.Tensor | None = None, m: int | None = None,
                        axis_bits: int | None = None) -> RaggedGrid:
    """The partition of a packed batch -- ``xyz[n,3]`` float32 with the cumulative ends ``offset[B]`` (int32 or int64) of its
    clouds -- into the occupied cells of a grid of edge ``size`` per cloud: ``RaggedGrid(index, coord[m,4], offset[B], count)``.
    Clouds of any size, up to ``2^axis_bits`` cells per axis.  A point of cloud ``c`` lies in the cell
    ``floor((xyz - start[c]) / size)`` per axis, float32 with a correctly rounded division; below ``start``, at or beyond
    ``2^axis_bits`` cells, non-finite or behind the last offset it is dropped (``cluster = -1``, last in ``order``).  The slots
    are the occupied cells ascending by (cloud, i, j, k); ``index`` is a ``GridIndex`` with ``b = 1`` that ``segment_pool`` and
    ``grid_unpool`` take unchanged, ``coord`` the integer coordinates sparse-convolution libraries take, ``offset`` the cumulative
    ends of the pooled level.  The full contract is ``pcc_grid_cluster_ragged``'s (include/pcc_neighbour.h).

    ``start[B,3]``: the origin of every cloud's grid; ``None``: per cloud the minimum of its finite coordinates
    (``ragged_grid_start``, on the device, no synchronisation).  ``axis_bits=None``: ``min(16, (63 - bits of B) // 3)``.
    ``m``: the capacity.  ``None`` reads the number of occupied cells from the device -- ONE host synchronisation -- and cuts
    the outputs to exactly that many slots, at least one, with no padding; a given ``m`` (``1 <= m <= n``) synchronises
    nothing, pads with empty runs and -1 coordinates, and ``count > m`` tells that the cells of rank ``m`` and above were
    dropped.  On the accelerator the HIP kernels (offsets clipped on the device, never trusted); for CPU tensors
    ``torch_grid_cluster_ragged`` (offsets validated): the same integers.  Carries no gradient."""
    what = 'grid_cluster_ragged'
    b, n, s32, bits = _grid_ragged_args(what, xyz, offset, size, start, m, axis_bits)
    if start is None:
        start = ragged_grid_start(xyz, offset)
    cap = n if m is None else int(m)
    run = hip_grid_cluster_ragged if xyz.device.type == 'cuda' else torch_grid_cluster_ragged
    cluster, order, seg, coord, new_offset, n_cells = run(xyz, offset, start, s32, cap, bits)
    if m is None:  # (at capacity n nothing was dropped: the first U + 1 entries are the index at capacity U)
        u = max(1, int(n_cells.item()))
        seg, coord = seg[:u + 1].contiguous(), coord[:u].contiguous()
    return RaggedGrid(GridIndex(cluster[None], seg[None], n_cells, order[None]), coord, new_offset, n_cells)


def _ragged_grid_arg(what: str, grid: Any) -> None:
    if not isinstance(grid, RaggedGrid) or not isinstance(grid.index, GridIndex):
        raise ValueError(f'{what}: expected a RaggedGrid, got {type(grid).__name__}')


def grid_pool_ragged(xyz: torch.Tensor, features: torch.Tensor | None, offset: torch.Tensor, size: float, reduce: str = 'mean',
                     start: torch.Tensor | None = None, m: int | None = None, axis_bits: int | None = None) -> RaggedGridPooled:
    """Partition-based pooling of a packed batch in one call (Point Transformer V2's ``GridPool``): every occupied cell of
    ``grid_cluster_ragged(xyz, offset, size, start, m, axis_bits)`` becomes one point --
    ``RaggedGridPooled(xyz[m,3], features[m,C] or None, offset[B], grid)``: the barycentre of the cell's points, their features
    ``features[n,C]`` reduced by ``reduce`` (``'mean'``, ``'sum'``, ``'max'``), the cumulative ends of the pooled clouds and the
    ``RaggedGrid`` for ``grid_unpool_ragged`` on the way back up.  Both go through ``segment_pool``'s autograd function with
    ``b = 1``, so a slot's mean is word for word ``segment_pool``'s; the point-major inputs are transposed to its channels-major
    ``[1,C,n]`` and the results back (two copies each way: plumbing, no arithmetic).  A padded slot holds NaN centres (the word
    0x7fc00000) and +0 features; ``knn_ragged`` / ``ball_query_ragged`` with ``offset`` treat such rows as rows of no cloud.
    Differentiable in ``features`` and, through the barycentres, in ``xyz``, with the partition held constant."""
    what = 'grid_pool_ragged'
    _, n, _, _ = _grid_ragged_args(what, xyz, offset, size, start, m, axis_bits)
    mode = _reduce_arg(what, reduce)
    if features is not None:
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != n or features.shape[1] < 1:
            raise ValueError(f'{what}: expected features[n = {n},C] with C >= 1, got '
                             f'{tuple(features.shape) if isinstance(features, torch.Tensor) else type(features).__name__}')
        _float32('features', features)
        _same_device('features', features, xyz.device)
    grid = grid_cluster_ragged(xyz, offset, size, start, m, axis_bits)
    cluster, seg, count, order = grid.index
    cap = seg.shape[1] - 1
    dev = xyz.device
    centres = SegmentPooled.apply(xyz.t()[None], cluster, seg, order, 0)[0].t()
    padded = torch.arange(cap, device=dev) >= count
    centres = torch.where(padded[:, None], torch.full((), float('nan'), dtype=F32, device=dev), centres)
    pooled = None if features is None else SegmentPooled.apply(features.t()[None], cluster, seg, order, mode)[0].t()
    return RaggedGridPooled(centres, pooled, grid.offset, grid)


def grid_unpool_ragged(pooled: torch.Tensor, grid: RaggedGrid) -> torch.Tensor:
    """PTv2's map unpooling on a packed batch: ``out[n,C]``, every point takes the row ``pooled[m,C]`` holds for its slot
    (``grid_unpool`` along ``grid.index``, transposed in and out).  A dropped point gets +0 and carries no gradient.
    Differentiable in ``pooled``."""
    what = 'grid_unpool_ragged'
    _ragged_grid_arg(what, grid)
    m = grid.index.seg.shape[-1] - 1
    if not isinstance(pooled, torch.Tensor) or pooled.dim() != 2 or pooled.shape[0] != m or pooled.shape[1] < 1:
        raise ValueError(f'{what}: expected pooled[m = {m},C] with C >= 1, got {tuple(pooled.shape) if isinstance(pooled, torch.Tensor) else type(pooled).__name__}')
    return grid_unpool(pooled.t()[None], grid.index)[0].t()
