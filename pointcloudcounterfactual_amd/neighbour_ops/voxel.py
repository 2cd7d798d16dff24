# ---- the point-voxel branch: features averaged into a dense grid, a grid read back at the points --------------------------

from __future__ import annotations

from typing import Any, Callable, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import (F32, I32, I64, _L, _canonical_nan, _cloud_arg, _features_arg, _float32,
                                                              _same_device, _zero)
from pointcloudcounterfactual_amd.set_metrics import _grid_args

MAX_VOXEL_POINTS = 16384  # pcc_voxel_index sorts a cloud in one workgroup's LDS


class VoxelIndex(NamedTuple):
    """What ``voxel_index`` returns: everything ``voxelize`` needs to know about where the points of a cloud fall."""

    cell: torch.Tensor    # [B,N] int32 flat cell (i * R + j) * R + k of every point, -1 for a non-finite point
    order: torch.Tensor   # [B,N] int32 permutation: the finite points by (cell, point index), then the non-finite ones
    counts: torch.Tensor  # [B,R,R,R] int32 points per cell


def _voxel_cloud_args(xyz: torch.Tensor, what: str, b: int | None = None, n: int | None = None) -> tuple[int, int]:
    """``xyz[B,N,3]`` float32 with ``1 <= N <= MAX_VOXEL_POINTS`` (and the given ``B``, ``N``): ``(b, n)``."""
    if xyz.dim() != 3 or xyz.shape[2] != 3 or not 1 <= xyz.shape[1] <= MAX_VOXEL_POINTS:
        raise ValueError(f'{what}: expected xyz[B,N,3] with 1 <= N <= {MAX_VOXEL_POINTS}, got {tuple(xyz.shape)}')
    if (b is not None and xyz.shape[0] != b) or (n is not None and xyz.shape[1] != n):
        raise ValueError(f'{what}: expected xyz[B = {b},N = {n},3], got {tuple(xyz.shape)}')
    _float32('xyz', xyz)
    return xyz.shape[0], xyz.shape[1]


def _voxel_size_args(what: str, b: int, n: int, res: int) -> None:
    """The size limits of the five entry points (include/pcc_neighbour.h)."""
    if b > 65535 or b * n >= 1 << 31 or b * res ** 3 >= 1 << 31:
        raise ValueError(f'{what}: too large (B <= 65535, B * N < 2^31, B * R^3 < 2^31), got B = {b}, N = {n}, R = {res}')


def torch_voxel_index(xyz: torch.Tensor, res: int, lo32: torch.Tensor, inv: torch.Tensor) -> VoxelIndex:
    """The rule of ``pcc_voxel_index`` in torch: the float32 operations of ``set_metrics._occupancy_host``, a stable sort by
    cell and a ``bincount``.  Integers only behind the cell rule, so every word is the kernel's."""
    b, n = xyz.shape[:2]
    bins = res ** 3
    finite = torch.isfinite(xyz).all(2)
    safe = torch.where(finite[:, :, None], xyz, _zero(xyz))
    ijk = torch.floor((safe - lo32) * inv + 0.5).clamp(0.0, float(res - 1)).to(I64)
    flat = (ijk[:, :, 0] * res + ijk[:, :, 1]) * res + ijk[:, :, 2]
    cell = torch.where(finite, flat, torch.full((), -1, dtype=I64))
    order = torch.argsort(torch.where(finite, flat, torch.full((), bins, dtype=I64)), dim=1, stable=True)
    rows = torch.arange(b)[:, None].expand(b, n)
    counts = torch.bincount((rows * bins + flat)[finite], minlength=b * bins).view(b, res, res, res)
    return VoxelIndex(cell.to(I32), order.to(I32), counts.to(I32))


def torch_voxelize(features: torch.Tensor, index: VoxelIndex) -> torch.Tensor:
    """The rule of ``pcc_voxelize`` as a torch composition, differentiable through autograd: the points in ``index.order``,
    then one pass per rank within the cell -- a pass adds at most one point to any cell, so every cell sums its points in
    ascending point index without an ``index_add_`` --, one division, +0.0 in the empty cells, a NaN as the word 0x7fc00000."""
    b, c, n = features.shape
    res = index.counts.shape[-1]
    bins = res ** 3
    order = index.order.to(I64)
    sorted_cell = torch.gather(index.cell.to(I64), 1, order)
    pos = torch.arange(n)[None, :].expand(b, n)
    is_start = torch.ones((b, n), dtype=torch.bool)
    is_start[:, 1:] = sorted_cell[:, 1:] != sorted_cell[:, :-1]
    rank = pos - torch.cummax(torch.where(is_start, pos, _zero(pos)), 1).values
    valid = sorted_cell >= 0
    acc = torch.zeros((b, c, bins), dtype=features.dtype)
    channels = torch.arange(c)[None, :]
    for r in range(int(rank[valid].max().item()) + 1 if valid.any() else 0):
        bi, si = (valid & (rank == r)).nonzero(as_tuple=True)
        at = (bi[:, None], channels, sorted_cell[bi, si][:, None])
        acc = acc.index_put(at, acc[at] + features[bi[:, None], channels, order[bi, si][:, None]])
    counts = index.counts.reshape(b, 1, bins)
    grid = torch.where(counts > 0, acc / torch.where(counts > 0, counts, torch.ones((), dtype=I32)).to(features.dtype),
                       _zero(features))
    return _canonical_nan(grid).view(b, c, res, res, res)


def _trilinear(xyz: torch.Tensor, res: int, lo32: torch.Tensor, inv: torch.Tensor) -> tuple[torch.Tensor, list[torch.Tensor], list[torch.Tensor]]:
    """``pcc_devoxelize``'s corners of the points ``xyz[B,N,3]`` (constants of the graph): ``finite[B,N]``, and for the
    corners 000, 001, 010, ... 111 the flat cells ``[B,N]`` int64 and the weights ``(wx * wy) * wz`` ``[B,N]``."""
    xyz = xyz.detach()
    finite = torch.isfinite(xyz).all(2)
    safe = torch.where(finite[:, :, None], xyz, _zero(xyz))
    t = ((safe - lo32.to(xyz.device)) * inv.to(xyz.device)).clamp(0.0, float(res - 1))
    base = torch.floor(t).clamp(max=float(res - 2))
    w1 = t - base
    w = (1.0 - w1, w1)
    i0 = base.to(I64)
    offs, weights = [], []
    for e in range(8):
        di, dj, dk = e >> 2, (e >> 1) & 1, e & 1
        offs.append(((i0[:, :, 0] + di) * res + i0[:, :, 1] + dj) * res + i0[:, :, 2] + dk)
        weights.append((w[di][:, :, 0] * w[dj][:, :, 1]) * w[dk][:, :, 2])
    return finite, offs, weights


def torch_devoxelize(grid: torch.Tensor, xyz: torch.Tensor, lo32: torch.Tensor, inv: torch.Tensor) -> torch.Tensor:
    """The rule of ``pcc_devoxelize`` as a torch composition, differentiable in ``grid`` through autograd: per corner, in the
    contract's order, a gather, a multiplication and an addition."""
    b, c, res = grid.shape[0], grid.shape[1], grid.shape[-1]
    n = xyz.shape[1]
    finite, offs, weights = _trilinear(xyz, res, lo32, inv)
    rows = grid.reshape(b, c, res ** 3)
    out = torch.zeros((b, c, n), dtype=grid.dtype, device=grid.device)
    for off, w in zip(offs, weights):
        out = out + w[:, None, :] * torch.gather(rows, 2, off[:, None, :].expand(b, c, n))
    out = torch.where(finite[:, None, :], out, _zero(grid))
    return _canonical_nan(out)


def voxel_index(xyz: torch.Tensor, resolution: int, lo: float = -0.5, extent: float = 1.0) -> VoxelIndex:
    """Where the points ``xyz[B,N,3]`` float32 fall on the grid of ``resolution`` points per axis over ``[lo, lo + extent]^3``
    (the grid and the cell rule of ``set_metrics.occupancy_grid``): ``VoxelIndex(cell[B,N], order[B,N], counts[B,R,R,R])``,
    all int32.  A point outside the cube lands in a border cell; a point with a NaN or infinite coordinate has cell -1, is
    counted nowhere and comes last in ``order``.  ``N <= 16384``.  Every word is fixed by the cloud alone
    (``pcc_voxel_index``, include/pcc_neighbour.h); CPU tensors take the same rule in torch and give the same integers.
    Carries no gradient."""
    what = 'voxel_index'
    b, n = _voxel_cloud_args(xyz, what)
    lo32, inv, _ = _grid_args(resolution, False, lo, extent)
    res = resolution
    _voxel_size_args(what, b, n, res)
    xyz = xyz.detach()
    dev = xyz.device
    if b == 0:
        return VoxelIndex(torch.zeros((0, n), dtype=I32, device=dev), torch.zeros((0, n), dtype=I32, device=dev),
                          torch.zeros((0, res, res, res), dtype=I32, device=dev))
    if dev.type != 'cuda':
        return torch_voxel_index(xyz, res, lo32, inv)
    xyz = xyz.contiguous()
    xp = ptr(xyz, 'xyz', F32, dev)
    cell, order = torch.empty((b, n), dtype=I32, device=dev), torch.empty((b, n), dtype=I32, device=dev)
    counts = torch.empty((b, res, res, res), dtype=I32, device=dev)
    call(_L.pcc_voxel_index, what, dev, b, n, xp, res, float(lo), float(extent), ptr(cell, 'cell', I32, dev),
         ptr(order, 'order', I32, dev), ptr(counts, 'counts', I32, dev))
    return VoxelIndex(cell, order, counts)


def _voxel_index_args(index: VoxelIndex, what: str, b: int, n: int, dev: torch.device) -> int:
    """``index`` is a ``VoxelIndex`` of ``b`` clouds of ``n`` points on ``dev``: its resolution."""
    cell, order, counts = index
    if tuple(cell.shape) != (b, n) or tuple(order.shape) != (b, n):
        raise ValueError(f'{what}: expected index.cell and index.order [B,N] = {(b, n)}, got {tuple(cell.shape)} and {tuple(order.shape)}')
    if counts.dim() != 4 or counts.shape[0] != b or not (2 <= counts.shape[1] == counts.shape[2] == counts.shape[3] <= 128):
        raise ValueError(f'{what}: expected index.counts[B = {b},R,R,R] with 2 <= R <= 128, got {tuple(counts.shape)}')
    for name, t in (('index.cell', cell), ('index.order', order), ('index.counts', counts)):
        if t.dtype != I32:
            raise RuntimeError(f'{name} must be {I32}, found {t.dtype}')
        _same_device(name, t, dev)
    return counts.shape[1]


def _index_arg(what: str, index_or_xyz: Any, resolution: Any, lo: float, extent: float, b: int | None = None, n: int | None = None,
               dev: torch.device | None = None, check_n: Callable[[int], None] | None = None) -> tuple[VoxelIndex, int]:
    """The ``index_or_xyz`` of ``voxelize`` and ``grid_cluster``: ``(index, its resolution)``.  A ``VoxelIndex`` is checked
    (against ``b``, ``n`` and ``dev``, or with none given against its own ``cell``) and ``resolution``, if given, must be its
    own; a cloud ``xyz[B,N,3]`` is checked likewise and indexed with ``voxel_index(xyz, resolution, lo, extent)``.
    ``check_n(N)`` is the caller's check of an argument against the point count: it runs last but before the indexing."""
    if isinstance(index_or_xyz, VoxelIndex):
        index = index_or_xyz
        if b is None:
            if index.cell.dim() != 2 or not 1 <= index.cell.shape[1] <= MAX_VOXEL_POINTS:
                raise ValueError(f'{what}: expected index.cell[B,N] with 1 <= N <= {MAX_VOXEL_POINTS}, got {tuple(index.cell.shape)}')
            (b, n), dev = index.cell.shape, index.cell.device
        res = _voxel_index_args(index, what, b, n, dev)
        if resolution is not None and resolution != res:
            raise ValueError(f'{what}: resolution {resolution!r} is not the index\'s ({res})')
        if check_n is not None:
            check_n(n)
        return index, res
    if isinstance(index_or_xyz, torch.Tensor):
        _, n = _voxel_cloud_args(index_or_xyz, what, b, n)
        if dev is not None:
            _same_device('xyz', index_or_xyz, dev)
        if resolution is None:
            raise ValueError(f'{what}: resolution is needed with a cloud')
        if check_n is not None:
            check_n(n)
        return voxel_index(index_or_xyz, resolution, lo, extent), resolution
    raise ValueError(f'{what}: expected a VoxelIndex or xyz[B,N,3], got {type(index_or_xyz).__name__}')


class Voxelized(Function):
    """``Voxelized.apply(features, cell, order, counts)``: ``pcc_voxelize``; the backward is ``pcc_voxelize_bwd`` on the saved
    ``cell`` and ``counts``, run only when the gradient of ``features`` is asked for.  The arguments have been checked."""

    @staticmethod
    def forward(ctx: Any, features: torch.Tensor, cell: torch.Tensor, order: torch.Tensor, counts: torch.Tensor) -> torch.Tensor:
        features, cell, order, counts = features.contiguous(), cell.contiguous(), order.contiguous(), counts.contiguous()
        b, c, n = features.shape
        res = counts.shape[1]
        dev = features.device
        xp, cp, op, np_ = ptr(features, 'features', F32, dev), ptr(cell, 'index.cell', I32, dev), ptr(order, 'index.order', I32, dev), \
            ptr(counts, 'index.counts', I32, dev)
        grid = torch.empty((b, c, res, res, res), dtype=F32, device=dev)
        call(_L.pcc_voxelize, 'voxelize', dev, b, c, n, res, xp, cp, op, np_, ptr(grid, 'grid', F32, dev))
        ctx.save_for_backward(cell, counts)
        ctx.n = n
        return grid

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, None, None, None]:
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        cell, counts = ctx.saved_tensors
        grad = grad.contiguous()
        b, c, res = grad.shape[:3]
        dev = grad.device
        gx = torch.empty((b, c, ctx.n), dtype=F32, device=dev)
        call(_L.pcc_voxelize_bwd, 'voxelize_bwd', dev, b, c, ctx.n, res, ptr(cell, 'index.cell', I32, dev),
             ptr(counts, 'index.counts', I32, dev), ptr(grad, 'grad', F32, dev), ptr(gx, 'grad_features', F32, dev))
        return gx, None, None, None


class Devoxelized(Function):
    """``Devoxelized.apply(grid, xyz, lo, extent)``: ``pcc_devoxelize``, differentiable in ``grid`` (``pcc_devoxelize_bwd``, run
    only when asked for).  The arguments have been checked."""

    @staticmethod
    def forward(ctx: Any, grid: torch.Tensor, xyz: torch.Tensor, lo: float, extent: float) -> torch.Tensor:
        grid, xyz = grid.contiguous(), xyz.contiguous()
        b, c, res = grid.shape[:3]
        n = xyz.shape[1]
        dev = grid.device
        gp, xp = ptr(grid, 'grid', F32, dev), ptr(xyz, 'xyz', F32, dev)
        out = torch.empty((b, c, n), dtype=F32, device=dev)
        call(_L.pcc_devoxelize, 'devoxelize', dev, b, c, n, res, lo, extent, gp, xp, ptr(out, 'out', F32, dev))
        ctx.save_for_backward(xyz)
        ctx.grid_args = (res, lo, extent)
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, None, None, None]:
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        xyz, = ctx.saved_tensors
        res, lo, extent = ctx.grid_args
        grad = grad.contiguous()
        b, c, n = grad.shape
        dev = grad.device
        gg = torch.empty((b, c, res, res, res), dtype=F32, device=dev)
        call(_L.pcc_devoxelize_bwd, 'devoxelize_bwd', dev, b, c, n, res, lo, extent, ptr(xyz, 'xyz', F32, dev),
             ptr(grad, 'grad', F32, dev), ptr(gg, 'grad_grid', F32, dev))
        return gg, None, None, None


def voxelize(features: torch.Tensor, index_or_xyz: Any, resolution: int | None = None, lo: float = -0.5, extent: float = 1.0) -> torch.Tensor:
    """``grid[B,C,R,R,R]``: the mean of the features ``features[B,C,N]`` float32 of the points in every cell, +0.0 in an empty
    cell.  ``index_or_xyz`` is the ``VoxelIndex`` of the cloud (``resolution``, if given, must be its own) or the cloud
    ``xyz[B,N,3]`` itself, indexed here with ``voxel_index(xyz, resolution, lo, extent)``.  A cell sums its points in
    ascending point index from +0.0 and divides once, so every word is fixed (``pcc_voxelize``, include/pcc_neighbour.h: the
    dense grid is written once, without atomics); differentiable in ``features``, the points of a cell sharing its gradient
    divided by their number.  The HIP kernels on the accelerator, the same rule as a torch composition for CPU tensors: the
    forwards agree word for word."""
    what = 'voxelize'
    b, c, n = _features_arg(what, features)
    _float32('features', features)
    dev = features.device
    index, res = _index_arg(what, index_or_xyz, resolution, lo, extent, b, n, dev)
    _voxel_size_args(what, b, n, res)
    if b == 0:
        return torch.zeros((0, c, res, res, res), dtype=F32, device=dev)
    if dev.type == 'cuda':
        return Voxelized.apply(features, index.cell, index.order, index.counts)
    return torch_voxelize(features, index)


def devoxelize(grid: torch.Tensor, xyz: torch.Tensor, lo: float = -0.5, extent: float = 1.0) -> torch.Tensor:
    """``out[B,C,N]``: the grid ``grid[B,C,R,R,R]`` float32 over ``[lo, lo + extent]^3`` read at the points ``xyz[B,N,3]`` by
    trilinear interpolation.  A point outside the cube reads the border; a point with a NaN or infinite coordinate gives
    +0.0 and carries no gradient.  The eight corners are added in a fixed order, a rounded product and a rounded sum each, so
    every word is fixed (``pcc_devoxelize``, include/pcc_neighbour.h).  Differentiable in ``grid`` (float atomics: the
    summation order of that gradient is not fixed); ``xyz`` carries no gradient and may hold any number of points, not only
    those the grid was voxelised from.  The HIP kernels on the accelerator, the
    same rule as a torch composition for CPU tensors: the forwards agree word for word."""
    what = 'devoxelize'
    if grid.dim() != 5 or grid.shape[1] < 1 or not (grid.shape[2] == grid.shape[3] == grid.shape[4]):
        raise ValueError(f'{what}: expected grid[B,C,R,R,R] with C >= 1, got {tuple(grid.shape)}')
    b, c, res = grid.shape[:3]
    lo32, inv, _ = _grid_args(res, False, lo, extent)
    _float32('grid', grid)
    _, n = _cloud_arg(what, 'xyz', xyz, b)  # (any N: only the index sort limits it)
    _float32('xyz', xyz)
    _same_device('xyz', xyz, grid.device)
    _voxel_size_args(what, b, n, res)
    xyz = xyz.detach()
    if b == 0:
        return torch.zeros((0, c, n), dtype=F32, device=grid.device)
    if grid.device.type == 'cuda':
        return Devoxelized.apply(grid, xyz, float(lo), float(extent))
    return torch_devoxelize(grid, xyz, lo32, inv)


def point_voxel(features: torch.Tensor, xyz: torch.Tensor, resolution: int, voxel_net: Callable[[torch.Tensor], torch.Tensor],
                lo: float = -0.5, extent: float = 1.0) -> torch.Tensor:
    """The voxel branch of a point-voxel convolution (PVCNN) in one call: one ``voxel_index`` of ``xyz[B,N,3]``,
    ``voxelize(features[B,C,N])``, ``voxel_net`` on the grid ``[B,C,R,R,R]`` (a ``Conv3d`` stack that keeps R) and
    ``devoxelize`` of its result at the same points: ``[B,C2,N]``.  Gradients reach ``features`` and the parameters of
    ``voxel_net``; ``xyz`` is a constant of the graph.  The arguments are checked before anything runs."""
    what = 'point_voxel'
    b, _, n = _features_arg(what, features)
    _voxel_cloud_args(xyz, what, b, n)
    _float32('features', features)
    _same_device('xyz', xyz, features.device)
    if not callable(voxel_net):
        raise ValueError(f'{what}: voxel_net must be callable, got {type(voxel_net).__name__}')
    index = voxel_index(xyz, resolution, lo, extent)
    grid = voxel_net(voxelize(features, index))
    if not isinstance(grid, torch.Tensor) or grid.dim() != 5 or grid.shape[0] != b or tuple(grid.shape[2:]) != (resolution,) * 3:
        got = tuple(grid.shape) if isinstance(grid, torch.Tensor) else type(grid).__name__
        raise ValueError(f'{what}: voxel_net must return [B = {b},C2,R,R,R] with R = {resolution}, got {got}')
    return devoxelize(grid, xyz, lo, extent)
