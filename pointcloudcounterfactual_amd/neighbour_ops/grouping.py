# ---- grouping along a list of another point set ------------------------------------------------------------------------

from __future__ import annotations

from typing import Any, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import F32, I64, _L, _float32, _list_arg, _list_on, _list_slots, _same_device, _zero
from pointcloudcounterfactual_amd.neighbour_ops.sampling import _ball_args, _fps_args, ball_query, farthest_point_sample


def _group_args(x: torch.Tensor, idx: torch.Tensor, centres: torch.Tensor | None, point_major: Any,
                what: str = 'group_points') -> tuple[int, int, int, int, int]:
    """The checks ``group_points`` makes before anything runs: ``(b, c, n, m, k)``."""
    if not isinstance(point_major, bool):
        raise ValueError(f'{what}: point_major must be a bool, got {point_major!r}')
    lay, clay = ('x[B,N,C]', 'centres[B,M,C]') if point_major else ('x[B,C,N]', 'centres[B,C,M]')
    if x.dim() != 3 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError(f'{what}: expected {lay} with C >= 1 and N >= 1, got {tuple(x.shape)}')
    b = x.shape[0]
    n, c = (x.shape[1], x.shape[2]) if point_major else (x.shape[2], x.shape[1])
    m, k = _list_arg(what, idx, b)
    if centres is not None and tuple(centres.shape) != ((b, m, c) if point_major else (b, c, m)):
        raise ValueError(f'{what}: expected {clay} = {(b, m, c) if point_major else (b, c, m)}, got {tuple(centres.shape)}')
    _float32('x', x)
    _list_on(idx, x.device)
    if centres is not None:
        _float32('centres', centres)
        _same_device('centres', centres, x.device)
    return b, c, n, m, k


def torch_group_points(x: torch.Tensor, idx: torch.Tensor, centres: torch.Tensor | None = None,
                       point_major: bool = False) -> torch.Tensor:
    """The rule of ``pcc_group_points`` (include/pcc_neighbour.h) as a torch composition -- gather, subtract, mask; CPU path
    of ``group_points``, differentiable through autograd.  A slot outside ``[0, N)`` is +0 and carries no gradient."""
    xc = x.transpose(1, 2) if point_major else x  # [B,C,N]
    b, c, n = xc.shape
    m, k = idx.shape[1:]
    valid, safe = _list_slots(idx, n)
    out = torch.gather(xc, 2, safe.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)
    if centres is not None:
        out = out - (centres.transpose(1, 2) if point_major else centres)[:, :, :, None]
    return torch.where(valid[:, None], out, _zero(out))


class Grouped(Function):
    """``Grouped.apply(idx, x0, centres0, point_major0, x1, centres1, point_major1, ...)``: every part ``(x, centres or
    None, point_major)`` grouped along the one list ``idx[B,M,k]`` into its channel slice of ONE ``[B, sum C, M, k]``
    tensor (``pcc_group_points`` with ``out_c`` / ``out_c0``: no ``cat``); the backward hands every part its slice of the
    incoming gradient in place (``pcc_group_points_bwd``).  Differentiable in every ``x`` and ``centres``.  The arguments
    have passed ``_group_args``."""

    @staticmethod
    def forward(ctx: Any, idx: torch.Tensor, *parts: Any) -> torch.Tensor:
        idx = idx.contiguous()
        b, m, k = idx.shape
        dev = idx.device
        todo = []
        for x, centres, pm in zip(parts[0::3], parts[1::3], parts[2::3]):
            x = x.contiguous()
            centres = None if centres is None else centres.contiguous()
            n, c = (x.shape[1], x.shape[2]) if pm else (x.shape[2], x.shape[1])
            # (checked before anything is allocated on the device)
            todo.append((c, n, int(pm), ptr(x, 'x', F32, dev), ptr(centres, 'centres', F32, dev)))
        ip = ptr(idx, 'idx', I64, dev)
        out_c = sum(t[0] for t in todo)
        out = torch.empty((b, out_c, m, k), dtype=F32, device=dev)
        c0 = 0
        for c, n, pm, xp, cp in todo:
            call(_L.pcc_group_points, 'group_points', dev, b, c, n, m, k, pm, xp, ip, cp, ptr(out, 'out', F32, dev), out_c, c0)
            c0 += c
        ctx.save_for_backward(idx)
        ctx.parts = [(c, n, pm, cp is not None) for c, n, pm, _, cp in todo]
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, ...]:
        (idx,) = ctx.saved_tensors
        b, m, k = idx.shape
        grad = grad.contiguous()
        dev = grad.device
        out_c = grad.shape[1]
        grads: list[Any] = [None]
        c0 = 0
        for p, (c, n, pm, has_centre) in enumerate(ctx.parts):
            gx = gc = None
            if ctx.needs_input_grad[1 + 3 * p]:
                gx = torch.empty((b, n, c) if pm else (b, c, n), dtype=F32, device=dev)
            if has_centre and ctx.needs_input_grad[2 + 3 * p]:
                gc = torch.empty((b, m, c) if pm else (b, c, m), dtype=F32, device=dev)
            if gx is not None or gc is not None:
                call(_L.pcc_group_points_bwd, 'group_points_bwd', dev, b, c, n, m, k, pm, ptr(idx, 'idx', I64, dev),
                     ptr(grad, 'grad', F32, dev), out_c, c0, ptr(gx, 'grad_x', F32, dev), ptr(gc, 'grad_centres', F32, dev))
            grads += [gx, gc, None]
            c0 += c
        return tuple(grads)


def group_points(x: torch.Tensor, idx: torch.Tensor, centres: torch.Tensor | None = None, point_major: bool = False) -> torch.Tensor:
    """``out[B,C,M,k]``: ``x`` gathered along ``idx[B,M,k]`` int64, a list into the N points of ``x`` that belongs to another
    point set (M != N allowed): the rows of ``ball_query`` around ``farthest_point_sample`` centres, or of ``knn_cross``.
    ``point_major=False``: ``x[B,C,N]``, ``centres[B,C,M]`` (the feature layout); ``True``: ``x[B,N,C]``, ``centres[B,M,C]``
    (the xyz layout).  ``out[b,ch,i,j] = x[b,ch,idx[b,i,j]]``, bit for bit; with ``centres`` the value relative to the row's
    centre, ``x[b,ch,idx[b,i,j]] - centres[b,ch,i]``.  A slot whose index is outside ``[0, N)`` (the -1 of ``pad='none'``) is
    +0 and carries no gradient.  Both tensors float32; differentiable in ``x`` and ``centres`` (``idx`` carries no gradient).
    The full contract is ``pcc_group_points``'s (include/pcc_neighbour.h).  The HIP kernels on the accelerator, the same rule
    as a torch composition for CPU tensors: the forwards agree word for word."""
    _group_args(x, idx, centres, point_major)
    if x.device.type == 'cuda':
        return Grouped.apply(idx.detach(), x, centres, point_major)
    return torch_group_points(x, idx.detach(), centres, point_major)


def _group_relative(xyz: torch.Tensor, features: torch.Tensor | None, idx: torch.Tensor, centres: torch.Tensor,
                    point_major: bool) -> torch.Tensor:
    """``group_points_relative`` on checked arguments: one grouping op fills ``[B,3+C,M,k]`` on the accelerator (``out_c`` /
    ``out_c0``: no ``cat``), the torch composition for CPU tensors."""
    if xyz.device.type == 'cuda':
        return Grouped.apply(idx, xyz, centres, True, *(() if features is None else (features, None, point_major)))
    grouped = torch_group_points(xyz, idx, centres, True)
    if features is not None:
        grouped = torch.cat((grouped, torch_group_points(features, idx, None, point_major)), 1)
    return grouped


def group_points_relative(xyz: torch.Tensor, features: torch.Tensor | None, idx: torch.Tensor, centres: torch.Tensor,
                          point_major: bool = False) -> torch.Tensor:
    """``grouped[B,3+C,M,k]`` along one list ``idx[B,M,k]`` int64 into the N points: channels 0-2 the coordinates
    ``xyz[B,N,3]`` of the listed points relative to their row's centre ``centres[B,M,3]``, behind them ``features`` gathered
    along the same list -- ``[B,C,N]``, or ``[B,N,C]`` with ``point_major`` -- (absent for ``features=None``).  The grouping
    half of ``query_and_group`` for a list the caller has, in either feature layout.  A slot outside ``[0, N)`` is +0 in
    every channel and carries no gradient; differentiable in ``xyz``, ``centres`` and ``features``.  The arguments are those
    of ``group_points``, checked before anything runs."""
    what = 'group_points_relative'
    _group_args(xyz, idx, centres, True, what)
    if features is not None:
        _group_args(features, idx, None, point_major, what)
        if (features.shape[1] if point_major else features.shape[2]) != xyz.shape[1]:
            raise ValueError(f'{what}: xyz and features name different numbers of points: {tuple(xyz.shape)} and {tuple(features.shape)}')
        _same_device('features', features, xyz.device)
    return _group_relative(xyz, features, idx.detach(), centres, point_major)


class QueryGrouped(NamedTuple):
    """What ``query_and_group`` returns."""

    grouped: torch.Tensor     # [B,3+C,M,nsample] relative coordinates, then the gathered features
    idx: torch.Tensor         # [B,M,nsample] int64 into the cloud (ball_query, or the list that was given)
    cnt: torch.Tensor | None  # [B,M] int32 points inside each ball, capped at nsample; None for a given list


def query_and_group(xyz: torch.Tensor, centres: torch.Tensor, features: torch.Tensor | None, radius: float, nsample: int,
                    pad: str = 'first', idx: torch.Tensor | None = None) -> QueryGrouped:
    """The grouping half of a set-abstraction layer around centres the caller has: ``ball_query(xyz, centres, radius,
    nsample, pad)`` lists the neighbours of ``centres[B,M,3]`` in ``xyz[B,N,3]`` and one grouping op fills
    ``grouped[B,3+C,M,nsample]``: channels 0-2 the neighbours' coordinates relative to their centre, the rest
    ``features[B,C,N]`` gathered along the same list (absent for ``features=None``).  A list ``idx[B,M,nsample]`` int64 that
    is given (a recorded one, or one of ``knn_cross``) is used in place of the ball query; ``cnt`` is then ``None``.
    Gradients reach ``features``, ``xyz`` and ``centres``; ``idx`` and ``cnt`` are constants of the graph.  The arguments
    are those of ``ball_query`` and ``group_points``, checked before anything runs."""
    what = 'query_and_group'
    _ball_args(xyz, centres, radius, nsample, pad)
    b = xyz.shape[0]
    if features is not None:
        if features.dim() != 3 or features.shape[0] != b or features.shape[2] != xyz.shape[1] or features.shape[1] < 1:
            raise ValueError(f'{what}: expected features[B = {b},C,N = {xyz.shape[1]}] with C >= 1, got {tuple(features.shape)}')
        _float32('features', features)
        _same_device('features', features, xyz.device)
    cnt = None
    if idx is None:
        idx, cnt = ball_query(xyz, centres, radius, nsample, pad=pad, return_count=True)
    else:
        if tuple(idx.shape) != (b, centres.shape[1], nsample):
            raise ValueError(f'{what}: expected idx[B,M,nsample] = {(b, centres.shape[1], nsample)}, got {tuple(idx.shape)}')
        _list_arg(what, idx, b)
        _list_on(idx, xyz.device)
        idx = idx.detach()
    return QueryGrouped(_group_relative(xyz, features, idx, centres, False), idx, cnt)


class SampleAndGroup(NamedTuple):
    """What ``sample_and_group`` returns."""

    centres: torch.Tensor  # [B,M,3] the sampled points (differentiable in xyz)
    grouped: torch.Tensor  # [B,3+C,M,nsample] relative coordinates, then the gathered features
    idx: torch.Tensor      # [B,M,nsample] int64 into the cloud (ball_query)
    cnt: torch.Tensor      # [B,M] int32 points inside each ball, capped at nsample
    sel: torch.Tensor      # [B,M] int64 the sampled indices (farthest_point_sample)


def sample_and_group(xyz: torch.Tensor, features: torch.Tensor | None, m: int, radius: float, nsample: int, start: Any = None,
                     pad: str = 'first') -> SampleAndGroup:
    """The sampling and grouping front end of a set-abstraction layer in one call: ``farthest_point_sample(xyz, m, start)``
    picks ``sel[B,M]``, ``centres = xyz[sel]``, ``ball_query(xyz, centres, radius, nsample, pad)`` lists the neighbours, and
    one grouping op fills ``grouped[B,3+C,M,nsample]``: channels 0-2 the neighbours' coordinates relative to their centre,
    the rest ``features[B,C,N]`` gathered along the same list (absent for ``features=None``).  Gradients reach ``features``,
    and ``xyz`` both as neighbour and as centre (through the gather on ``sel``); ``idx``, ``cnt`` and ``sel`` are constants of
    the graph.  The arguments are those of the three functions, checked before anything runs."""
    _fps_args(xyz, m, start)
    if features is not None:
        if features.dim() != 3 or features.shape[0] != xyz.shape[0] or features.shape[2] != xyz.shape[1] or features.shape[1] < 1:
            raise ValueError(f'sample_and_group: expected features[B = {xyz.shape[0]},C,N = {xyz.shape[1]}] with C >= 1, '
                             f'got {tuple(features.shape)}')
        _float32('features', features)
        _same_device('features', features, xyz.device)
    b = xyz.shape[0]
    _ball_args(xyz, xyz.new_zeros((b, 0, 3)), radius, nsample, pad)  # (radius, nsample and pad, before the sampling runs)
    sel = farthest_point_sample(xyz, m, start)
    centres = torch.gather(xyz, 1, sel[:, :, None].expand(-1, -1, 3))
    grouped, idx, cnt = query_and_group(xyz, centres, features, radius, nsample, pad)
    return SampleAndGroup(centres, grouped, idx, cnt, sel)
