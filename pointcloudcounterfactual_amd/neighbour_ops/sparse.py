# ---- submanifold sparse convolution on the slots of grid_cluster (MinkUNet, SparseUNet, PTv3's position encoding) ---------

from __future__ import annotations

import numbers
from typing import Any, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import (F32, I32, I64, _L, _features_arg, _float32, _list_slots, _same_device,
                                                              _valid_slots, _zero)
from pointcloudcounterfactual_amd.neighbour_ops.pooling import GridIndex, _grid_index_args
from pointcloudcounterfactual_amd.neighbour_ops.voxel import MAX_VOXEL_POINTS, VoxelIndex, _voxel_index_args

KERNEL_SIZES = (3, 5)  # pcc_cell_neighbours' kernel sizes


class SparseConvMap(NamedTuple):
    """What ``cell_neighbours`` returns: the kernel map of a submanifold convolution over the slots of a ``GridIndex``."""

    nbr: torch.Tensor    # [B,m,K^3] int64: the slot at every offset of every slot, -1 where there is none
    count: torch.Tensor  # [B] int32 occupied cells of the cloud, GridIndex.count
    kernel_size: int     # K: tap ((di + h) * K + (dj + h)) * K + (dk + h), h = (K - 1) / 2, is the cell at +(di, dj, dk) * dilation
    dilation: int


def _kernel_args(what: str, kernel_size: Any, dilation: Any) -> None:
    if isinstance(kernel_size, bool) or not isinstance(kernel_size, numbers.Integral) or kernel_size not in KERNEL_SIZES:
        raise ValueError(f'{what}: kernel_size must be 3 or 5, got {kernel_size!r}')
    if isinstance(dilation, bool) or not isinstance(dilation, numbers.Integral) or dilation < 1:
        raise ValueError(f'{what}: dilation must be an integer >= 1, got {dilation!r}')


def torch_cell_neighbours(index: VoxelIndex, gindex: GridIndex, kernel_size: int, dilation: int) -> torch.Tensor:
    """The rule of ``pcc_cell_neighbours`` in torch: ``nbr[B,m,K^3]`` int64.  The cell of every slot is decomposed into its
    triple before the offsets are added, and a batched ``searchsorted`` over the cloud's ascending kept cells finds the
    rank.  Integers only, so every word is the kernel's."""
    b, n = index.cell.shape
    res = index.counts.shape[1]
    m = gindex.seg.shape[1] - 1
    sorted_cell = torch.gather(index.cell.to(I64), 1, gindex.order.to(I64))
    real = torch.arange(m)[None, :] < gindex.count.to(I64).clamp(0, m)[:, None]
    start = gindex.seg[:, :m].to(I64).clamp(0, n - 1)
    cells = torch.where(real, torch.gather(sorted_cell, 1, start), torch.full((), res ** 3, dtype=I64))  # ascending: the padding is behind every cell
    h = (kernel_size - 1) // 2
    d = torch.arange(-h, h + 1) * min(dilation, res)  # (beyond res nothing but the centre is inside)
    di, dj, dk = (t.reshape(-1) for t in torch.meshgrid(d, d, d, indexing='ij'))
    ti, tj, tk = (cells // (res * res))[:, :, None] + di, (cells // res % res)[:, :, None] + dj, (cells % res)[:, :, None] + dk
    inside = real[:, :, None] & (ti >= 0) & (ti < res) & (tj >= 0) & (tj < res) & (tk >= 0) & (tk < res)
    want = torch.where(inside, (ti * res + tj) * res + tk, torch.full((), -1, dtype=I64))
    pos = torch.searchsorted(cells, want.reshape(b, -1)).clamp(max=m - 1)
    hit = inside & (torch.gather(cells, 1, pos) == want.reshape(b, -1)).view(want.shape)
    return torch.where(hit, pos.view(want.shape), torch.full((), -1, dtype=I64))


def cell_neighbours(index: VoxelIndex, gindex: GridIndex, kernel_size: int = 3, dilation: int = 1) -> SparseConvMap:
    """The kernel map of a submanifold sparse convolution over the occupied cells of a grid:
    ``SparseConvMap(nbr[B,m,K^3] int64, count[B], kernel_size, dilation)``.  ``index`` is the ``VoxelIndex`` of the clouds and
    ``gindex`` their ``GridIndex`` at some capacity ``m`` (``grid_cluster(index, m=...)``, or ``grid_pool(...).index`` with
    ``voxel_index`` of the same cloud and grid); the resolution is read from ``index.counts``.  ``nbr[b,r,t]`` is the slot of
    the cell at offset ``(di, dj, dk) * dilation`` from slot ``r``'s cell, ``t = ((di + h) * K + (dj + h)) * K + (dk + h)``
    with ``h = (K - 1) / 2``, or -1 where that cell is outside the grid (nothing wraps around), empty or dropped (rank >=
    m); every tap of a padded slot is -1.  The centre tap of a real slot is the slot itself, and the map is symmetric:
    ``nbr[r,t] = s`` exactly when ``nbr[s,K^3 - 1 - t] = r``.  It is an ordinary list: ``group_points``, ``aggregate_points``
    and ``local_geometry`` take ``nbr`` unchanged.  Integers only, fixed by the cloud alone (``pcc_cell_neighbours``,
    include/pcc_neighbour.h); CPU tensors take the same rule in torch and give the same words.  No host synchronisation;
    carries no gradient."""
    what = 'cell_neighbours'
    if not isinstance(index, VoxelIndex):
        raise ValueError(f'{what}: expected a VoxelIndex, got {type(index).__name__}')
    _kernel_args(what, kernel_size, dilation)
    if index.cell.dim() != 2 or not 1 <= index.cell.shape[1] <= MAX_VOXEL_POINTS:
        raise ValueError(f'{what}: expected index.cell[B,N] with 1 <= N <= {MAX_VOXEL_POINTS}, got {tuple(index.cell.shape)}')
    b, n = index.cell.shape
    dev = index.cell.device
    res = _voxel_index_args(index, what, b, n, dev)
    m = _grid_index_args(gindex, what, b, n, dev)
    taps = int(kernel_size) ** 3
    if b > 65535 or b * m * taps >= 1 << 31:
        raise ValueError(f'{what}: too large (B <= 65535, B * m * K^3 < 2^31), got B = {b}, m = {m}, K = {kernel_size}')
    if b == 0:
        return SparseConvMap(torch.zeros((0, m, taps), dtype=I64, device=dev), gindex.count, int(kernel_size), int(dilation))
    if dev.type == 'cuda':
        cell, order, seg, count = index.cell.contiguous(), gindex.order.contiguous(), gindex.seg.contiguous(), gindex.count.contiguous()
        nbr = torch.empty((b, m, taps), dtype=I64, device=dev)
        call(_L.pcc_cell_neighbours, what, dev, b, n, m, res, int(kernel_size), min(int(dilation), 1 << 20), ptr(cell, 'index.cell', I32, dev),
             ptr(order, 'index.order', I32, dev), ptr(seg, 'index.seg', I32, dev), ptr(count, 'index.count', I32, dev), ptr(nbr, 'nbr', I64, dev))
    else:
        nbr = torch_cell_neighbours(index, gindex, int(kernel_size), int(dilation))
    return SparseConvMap(nbr, gindex.count, int(kernel_size), int(dilation))


def torch_sparse_conv(features: torch.Tensor, nbr: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """The rule of ``pcc_sparse_conv`` as a torch composition, differentiable through autograd: tap by tap, the features
    gathered along ``nbr[:, :, t]`` (+0 where the tap is empty) times ``weight[t]``; a row with no tap at all is +0 without
    the bias.  Nothing ``K^3`` times the features is held."""
    b, c, n = features.shape
    m, taps = nbr.shape[1:]
    valid, safe = _list_slots(nbr, n)
    out = torch.zeros((b, weight.shape[2], m), dtype=features.dtype, device=features.device)
    zero = _zero(features)
    for t in range(taps):
        if not bool(valid[:, :, t].any()):
            continue
        got = torch.where(valid[:, None, :, t], torch.gather(features, 2, safe[:, None, :, t].expand(-1, c, -1)), zero)
        out = out + torch.einsum('bcm,co->bom', got, weight[t])
    if bias is not None:
        out = out + bias[None, :, None]
    return torch.where(valid.any(2)[:, None, :], out, zero)


def _mirrored(weight: torch.Tensor) -> torch.Tensor:
    """``weight'[t, oc, ch] = weight[T - 1 - t, ch, oc]``: the weights under which the convolution along a symmetric map is
    the transpose of the convolution under ``weight``."""
    return weight.flip(0).transpose(1, 2).contiguous()


class SparseConvolved(Function):
    """``SparseConvolved.apply(features, nbr, weight, bias)``: ``pcc_sparse_conv`` along a map of ``cell_neighbours``.  The
    gradient of ``features`` is the same kernel on the mirrored weights (the map is symmetric), without atomics; the
    gradients of ``weight`` and ``bias`` are torch compositions -- per tap ``group_points`` of ``features`` along
    ``nbr[:, :, t:t+1]`` and one matmul with the incoming gradient, the sum over the real slots for the bias: the part that
    is not fused yet.  Only the gradients asked for are computed.  The arguments have been checked."""

    @staticmethod
    def forward(ctx: Any, features: torch.Tensor, nbr: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None) -> torch.Tensor:
        features, nbr, weight = features.contiguous(), nbr.contiguous(), weight.contiguous()
        bias = None if bias is None else bias.contiguous()
        b, c, n = features.shape
        m, taps = nbr.shape[1:]
        o = weight.shape[2]
        dev = features.device
        out = torch.empty((b, o, m), dtype=F32, device=dev)
        call(_L.pcc_sparse_conv, 'sparse_conv', dev, b, c, o, n, m, taps, ptr(features, 'features', F32, dev), ptr(nbr, 'cmap.nbr', I64, dev),
             ptr(weight, 'weight', F32, dev), ptr(bias, 'bias', F32, dev), ptr(out, 'out', F32, dev))
        ctx.save_for_backward(features, nbr, weight)
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, None, Any, Any]:
        features, nbr, weight = ctx.saved_tensors
        grad = grad.contiguous()
        b, o, m = grad.shape
        c, taps = features.shape[1], nbr.shape[2]
        dev = grad.device
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = torch.empty((b, c, m), dtype=F32, device=dev)
            call(_L.pcc_sparse_conv, 'sparse_conv', dev, b, o, c, m, m, taps, ptr(grad, 'grad', F32, dev), ptr(nbr, 'cmap.nbr', I64, dev),
                 ptr(_mirrored(weight), 'weight', F32, dev), None, ptr(gx, 'grad_features', F32, dev))
        if ctx.needs_input_grad[2]:
            gw = torch.empty((taps, c, o), dtype=F32, device=dev)
            lists = nbr.permute(2, 0, 1).contiguous()  # [T,B,m]: the list of one tap is contiguous, k = 1
            got = torch.empty((b, c, m, 1), dtype=F32, device=dev)  # the features at one tap, +0 where it is empty
            xp, gp, grad_t = ptr(features, 'features', F32, dev), ptr(got, 'grouped', F32, dev), grad.transpose(1, 2)
            for t in range(taps):
                call(_L.pcc_group_points, 'group_points', dev, b, c, m, m, 1, 0, xp, ptr(lists[t], 'cmap.nbr', I64, dev), None, gp, c, 0)
                torch.sum(torch.bmm(got[:, :, :, 0], grad_t), 0, out=gw[t])
        if ctx.needs_input_grad[3]:
            real = _valid_slots(nbr, m).any(2)
            gb = torch.where(real[:, None, :], grad, _zero(grad)).sum((0, 2))
        return gx, None, gw, gb


def _sparse_conv_args(what: str, features: torch.Tensor, cmap: Any, weight: torch.Tensor, bias: torch.Tensor | None) -> tuple[int, int, int, int]:
    """The checks of ``sparse_conv``: ``(b, c, o, m)``."""
    if not isinstance(cmap, SparseConvMap):
        raise ValueError(f'{what}: expected a SparseConvMap (cell_neighbours), got {type(cmap).__name__}')
    b, c, m = _features_arg(what, features)
    _kernel_args(what, cmap.kernel_size, cmap.dilation)
    taps = cmap.kernel_size ** 3
    if tuple(cmap.nbr.shape) != (b, m, taps):
        raise ValueError(f'{what}: expected cmap.nbr[B,m,K^3] = {(b, m, taps)} for features[B,C,m], got {tuple(cmap.nbr.shape)}')
    if weight.dim() != 3 or weight.shape[0] != taps or weight.shape[1] != c or weight.shape[2] < 1:
        raise ValueError(f'{what}: expected weight[K^3 = {taps},C = {c},O] with O >= 1, got {tuple(weight.shape)}')
    o = weight.shape[2]
    if bias is not None and tuple(bias.shape) != (o,):
        raise ValueError(f'{what}: expected bias[O = {o}], got {tuple(bias.shape)}')
    if b > 65535 or m * taps >= 1 << 31 or taps * c * o >= 1 << 31:
        raise ValueError(f'{what}: too large (B <= 65535, m * K^3 < 2^31, K^3 * C * O < 2^31), got B = {b}, m = {m}, C = {c}, O = {o}')
    _float32('features', features)
    _float32('weight', weight)
    _same_device('weight', weight, features.device)
    if bias is not None:
        _float32('bias', bias)
        _same_device('bias', bias, features.device)
    if cmap.nbr.dtype != I64:
        raise RuntimeError(f'cmap.nbr must be {I64}, found {cmap.nbr.dtype}')
    _same_device('cmap.nbr', cmap.nbr, features.device)
    return b, c, o, m


def sparse_conv(features: torch.Tensor, cmap: SparseConvMap, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """Submanifold sparse convolution: ``out[B,O,m]`` from the features ``features[B,C,m]`` of the slots of a grid level
    (``grid_pool(...).features``), the map ``cmap`` of ``cell_neighbours`` for those slots, ``weight[K^3,C,O]`` and
    ``bias[O]`` -- ``out[b,oc,r] = bias[oc] + sum over the taps t with a neighbour and over ch of weight[t,ch,oc] *
    features[b,ch,cmap.nbr[b,r,t]]``.  A padded slot gives +0 (no bias), so the output is a level like its input.  One fused
    gather-GEMM kernel that never writes the ``[B,C,m,K^3]`` tensor of gathered features (``pcc_sparse_conv``,
    include/pcc_neighbour.h: the numerical contract is a bound against exact arithmetic, and a row's result does not depend
    on the batch around it); no float atomics.  Differentiable in ``features`` (the same kernel on mirrored weights: this is
    why only a map of ``cell_neighbours``, which is symmetric, is accepted), ``weight`` and ``bias`` (torch compositions per
    tap).  ``weight.view(K,K,K,C,O).permute(4,3,0,1,2)`` is the weight of a ``torch.nn.Conv3d`` with padding ``h *
    dilation`` on the dense grid ``[B,C,R,R,R]``.  CPU tensors take ``torch_sparse_conv``."""
    what = 'sparse_conv'
    b, c, o, m = _sparse_conv_args(what, features, cmap, weight, bias)
    if b == 0:
        return torch.zeros((0, o, m), dtype=F32, device=features.device)
    if features.device.type == 'cuda':
        return SparseConvolved.apply(features, cmap.nbr.detach(), weight, bias)
    return torch_sparse_conv(features, cmap.nbr.detach(), weight, bias)


class SubmanifoldConv3d(torch.nn.Module):
    """``torch.nn.Conv3d(in_channels, out_channels, kernel_size, padding=h * dilation, dilation=dilation)`` restricted to the
    occupied cells of a sparse grid level: ``forward(features[B,C,m], cmap) -> [B,O,m]`` with ``cmap =
    cell_neighbours(index, gindex, kernel_size, dilation)``.  ``weight[K^3,C,O]``: ``weight.view(K,K,K,C,O).permute(4,3,0,1,2)``
    is Conv3d's weight, and the initialisation is Conv3d's (Kaiming uniform with a = sqrt(5) over fan_in = C * K^3, the bias
    uniform in +-1 / sqrt(fan_in)).  One level of a voxel backbone::

        pooled = grid_pool(xyz, features, R)                   # points -> occupied cells
        cmap = cell_neighbours(voxel_index(xyz, R), pooled.index)
        y = conv(pooled.features, cmap)                        # SubmanifoldConv3d(C, O)
        back = grid_unpool(y, pooled.index)                    # cells -> points
    """

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, dilation: int = 1, bias: bool = True) -> None:
        super().__init__()
        _kernel_args('SubmanifoldConv3d', kernel_size, dilation)
        for name, v in (('in_channels', in_channels), ('out_channels', out_channels)):
            if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
                raise ValueError(f'SubmanifoldConv3d: {name} must be an integer >= 1, got {v!r}')
        self.in_channels, self.out_channels, self.kernel_size, self.dilation = int(in_channels), int(out_channels), int(kernel_size), int(dilation)
        taps = self.kernel_size ** 3
        fan_in = self.in_channels * taps
        bound = 1.0 / fan_in ** 0.5  # kaiming_uniform_(a = sqrt(5)): gain sqrt(2 / 6), bound gain * sqrt(3 / fan_in) = 1 / sqrt(fan_in)
        self.weight = torch.nn.Parameter(torch.empty(taps, self.in_channels, self.out_channels).uniform_(-bound, bound))
        self.bias = torch.nn.Parameter(torch.empty(self.out_channels).uniform_(-bound, bound)) if bias else None

    def forward(self, features: torch.Tensor, cmap: SparseConvMap) -> torch.Tensor:
        if not isinstance(cmap, SparseConvMap) or (cmap.kernel_size, cmap.dilation) != (self.kernel_size, self.dilation):
            raise ValueError(f'SubmanifoldConv3d: expected a SparseConvMap with kernel_size {self.kernel_size} and dilation {self.dilation}')
        return sparse_conv(features, cmap, self.weight, self.bias)
