# ---- submanifold sparse convolution on a ragged grid level: the kernel map over grid_cluster_ragged's coord (scenes) --------

from __future__ import annotations

from typing import Any

import torch

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import I32, I64, _L, _same_device
from pointcloudcounterfactual_amd.neighbour_ops.ragged_grid import RaggedGrid, _ragged_grid_arg
from pointcloudcounterfactual_amd.neighbour_ops.sparse import SparseConvMap, _kernel_args, sparse_conv

AXIS_CELLS = 1 << 16  # pcc_cell_neighbours_ragged: every field of the key (cloud, i, j, k) holds [0, 65536)


def torch_cell_neighbours_ragged(coord: torch.Tensor, count: torch.Tensor, kernel_size: int, dilation: int) -> torch.Tensor:
    """The rule of ``pcc_cell_neighbours_ragged`` (include/pcc_neighbour.h) in torch; CPU path of ``cell_neighbours_ragged``:
    ``nbr[m,K^3]`` int64 from ``coord[m,4]`` and ``count[1]``.  The offsets are added to the decomposed coordinates and the
    range test comes before the packing into an int64 key (the cloud field biased by -32768 so that the signed keys ascend
    like the rows), one ``torch.searchsorted`` over the keys of the real slots finds the ranks.  Integers only, so every
    word is the kernel's."""
    m = coord.shape[0]
    taps = kernel_size ** 3
    nbr = torch.full((m, taps), -1, dtype=I64, device=coord.device)
    kept = min(max(int(count.reshape(-1)[0]), 0), m)
    if kept == 0:
        return nbr
    rows = coord[:kept].to(I64)
    inside_src = ((rows >= 0) & (rows < AXIS_CELLS)).all(1)

    def pack(c: torch.Tensor, i: torch.Tensor, j: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
        return ((c - (AXIS_CELLS >> 1)) << 48) + (i << 32) + (j << 16) + k

    masked = rows & (AXIS_CELLS - 1)
    keys = pack(masked[:, 0], masked[:, 1], masked[:, 2], masked[:, 3])
    h = (kernel_size - 1) // 2
    d = torch.arange(-h, h + 1, dtype=I64, device=coord.device) * min(dilation, AXIS_CELLS)  # (beyond 65536 nothing but the centre is inside)
    di, dj, dk = (t.reshape(-1) for t in torch.meshgrid(d, d, d, indexing='ij'))
    ti, tj, tk = rows[:, 1, None] + di, rows[:, 2, None] + dj, rows[:, 3, None] + dk
    inside = inside_src[:, None] & (ti >= 0) & (ti < AXIS_CELLS) & (tj >= 0) & (tj < AXIS_CELLS) & (tk >= 0) & (tk < AXIS_CELLS)
    lowest = torch.full((), -(1 << 63), dtype=I64, device=coord.device)
    want = torch.where(inside, pack(rows[:, 0, None].expand_as(ti), ti, tj, tk), lowest)
    pos = torch.searchsorted(keys, want.reshape(-1)).clamp(max=kept - 1)
    hit = inside & (keys[pos] == want.reshape(-1)).view(want.shape)
    nbr[:kept] = torch.where(hit, pos.view(want.shape), torch.full((), -1, dtype=I64, device=coord.device))
    return nbr


def hip_cell_neighbours_ragged(coord: torch.Tensor, count: torch.Tensor, kernel_size: int, dilation: int) -> torch.Tensor:
    """``pcc_cell_neighbours_ragged`` on checked arguments: ``nbr[m,K^3]`` int64.  Nothing is read on the host."""
    dev = coord.device
    coord, count = coord.contiguous(), count.contiguous()
    m = coord.shape[0]
    cp, np_ = ptr(coord, 'grid.coord', I32, dev), ptr(count, 'grid.count', I32, dev)  # (checked before anything is allocated)
    nbr = torch.empty((m, kernel_size ** 3), dtype=I64, device=dev)
    call(_L.pcc_cell_neighbours_ragged, 'cell_neighbours_ragged', dev, m, kernel_size, min(dilation, 1 << 20), cp, np_, ptr(nbr, 'nbr', I64, dev))
    return nbr


def cell_neighbours_ragged(grid: RaggedGrid, kernel_size: int = 3, dilation: int = 1) -> SparseConvMap:
    """The kernel map of a submanifold sparse convolution over the occupied cells of a packed batch -- the ``RaggedGrid`` of
    ``grid_cluster_ragged`` or ``grid_pool_ragged(...).grid``, padded (``m`` given) or not: ``SparseConvMap(nbr[1,m,K^3] int64,
    count = grid.count, kernel_size, dilation)`` with ``m = grid.coord.shape[0]``.  Clouds of any size, up to 2^16 cells per
    axis.  ``nbr[0,r,t]`` is the slot of the same cloud whose cell lies at offset ``(di, dj, dk) * dilation`` from slot ``r``'s,
    ``t = ((di + h) * K + (dj + h)) * K + (dk + h)`` with ``h = (K - 1) / 2``, or -1 where that cell is outside ``[0, 65536)^3``
    (nothing wraps around, and no tap crosses into another cloud), empty or dropped (rank >= ``m``); every tap of a padded
    slot is -1.  The centre tap of a real slot is the slot itself and the map is symmetric, so it is an ordinary
    ``SparseConvMap`` with ``B = 1``: ``sparse_conv`` / ``SubmanifoldConv3d`` (on ``features.t()[None]``, or
    ``sparse_conv_ragged`` on the point-major features), ``group_points``, ``aggregate_points`` and ``local_geometry`` take
    it unchanged.  Integers only, fixed by ``grid.coord`` alone (``pcc_cell_neighbours_ragged``, include/pcc_neighbour.h);
    CPU tensors take the same rule in torch and give the same words.  No host synchronisation on the accelerator; carries
    no gradient."""
    what = 'cell_neighbours_ragged'
    _ragged_grid_arg(what, grid)
    _kernel_args(what, kernel_size, dilation)
    coord, count = grid.coord, grid.count
    if not isinstance(coord, torch.Tensor) or coord.dim() != 2 or coord.shape[1] != 4 or coord.shape[0] < 1:
        raise ValueError(f'{what}: expected grid.coord[m,4] with m >= 1, got {tuple(coord.shape) if isinstance(coord, torch.Tensor) else type(coord).__name__}')
    if not isinstance(count, torch.Tensor) or count.numel() != 1:
        raise ValueError(f'{what}: expected grid.count[1], got {tuple(count.shape) if isinstance(count, torch.Tensor) else type(count).__name__}')
    m, taps = coord.shape[0], int(kernel_size) ** 3
    if m * taps >= 1 << 31:
        raise ValueError(f'{what}: too large (m * K^3 < 2^31), got m = {m}, K = {kernel_size}')
    for name, t in (('grid.coord', coord), ('grid.count', count)):
        if t.dtype != I32:
            raise RuntimeError(f'{name} must be {I32}, found {t.dtype}')
    _same_device('grid.count', count, coord.device)
    run = hip_cell_neighbours_ragged if coord.device.type == 'cuda' else torch_cell_neighbours_ragged
    nbr = run(coord.detach(), count.detach().reshape(1), int(kernel_size), int(dilation))
    return SparseConvMap(nbr[None], count, int(kernel_size), int(dilation))


def sparse_conv_ragged(features: torch.Tensor, cmap: SparseConvMap, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """``sparse_conv`` in the point-major layout of a packed batch (what Pointcept and spconv users hold): ``out[m,O]`` from
    ``features[m,C]``, the map of ``cell_neighbours_ragged``, ``weight[K^3,C,O]`` and ``bias[O]``.  It is ``sparse_conv`` on
    ``features.t()[None]``, transposed back: plumbing, no arithmetic, and differentiable exactly as ``sparse_conv`` is."""
    what = 'sparse_conv_ragged'
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] < 1 or features.shape[1] < 1:
        raise ValueError(f'{what}: expected features[m,C] with m, C >= 1, got {tuple(features.shape) if isinstance(features, torch.Tensor) else type(features).__name__}')
    if not isinstance(cmap, SparseConvMap) or cmap.nbr.dim() != 3 or cmap.nbr.shape[0] != 1:
        raise ValueError(f'{what}: expected the SparseConvMap of cell_neighbours_ragged (nbr[1,m,K^3])')
    return sparse_conv(features.t()[None], cmap, weight, bias)[0].t()
