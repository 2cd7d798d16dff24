# ---- feature propagation: weighted interpolation along a list of another point set ----------------------------------------

from __future__ import annotations

from typing import Any, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import (F32, I64, _L, _canonical_nan, _cloud_arg, _features_arg, _float32, _k_arg,
                                                              _list_arg, _list_on, _list_slots, _same_device, _zero)
from pointcloudcounterfactual_amd.neighbour_ops.search import knn_cross


def interpolation_weights(dist: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """Inverse-distance weights ``w[B,M,k]`` of the squared distances ``dist[B,M,k]`` that ``knn_cross(...,
    return_distance=True)`` returns: ``r = 1 / (dist + eps)``, ``r = 0`` where ``dist`` is NaN (the padded slot of a list that
    ran short), ``w = r / sum_k r``, and all zeros where that sum is 0 (a row of padded slots only).  Plain torch on either
    device, differentiable in ``dist``."""
    if dist.dim() != 3 or not dist.is_floating_point():
        raise ValueError(f'interpolation_weights: expected floating-point dist[B,M,k], got {tuple(dist.shape)} {dist.dtype}')
    pad = torch.isnan(dist)
    zero = _zero(dist)
    r = torch.where(pad, zero, 1 / (torch.where(pad, zero + 1, dist) + eps))  # (no 1 / NaN behind the mask: its gradient is NaN)
    s = r.sum(-1, keepdim=True)
    return torch.where(s == 0, zero, r / torch.where(s == 0, zero + 1, s))


def _interp_args(x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, what: str = 'interpolate_points') -> tuple[int, int, int, int, int]:
    """The checks ``interpolate_points`` makes before anything runs: ``(b, c, n, m, k)``."""
    b, c, n = _features_arg(what, x, 'x')
    m, k = _list_arg(what, idx, b)
    if tuple(weights.shape) != (b, m, k):
        raise ValueError(f'{what}: expected weights[B,M,k] = {(b, m, k)}, got {tuple(weights.shape)}')
    _float32('x', x)
    _list_on(idx, x.device)
    _float32('weights', weights)
    _same_device('weights', weights, x.device)
    return b, c, n, m, k


def torch_interpolate_points(x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """The rule of ``pcc_interpolate`` (include/pcc_neighbour.h) as a torch composition -- per slot of the list a gather, a
    mask, a multiplication and an addition, in slot order; CPU path of ``interpolate_points``, differentiable through
    autograd.  A slot outside ``[0, N)`` adds nothing and carries no gradient; a NaN result is the word 0x7fc00000."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    out = torch.zeros((b, c, m), dtype=x.dtype, device=x.device)
    for j in range(k):
        valid, safe = _list_slots(idx[:, :, j], n)
        wj = torch.where(valid, weights[:, :, j], _zero(weights))
        term = wj[:, None] * torch.gather(x, 2, safe[:, None, :].expand(-1, c, -1))  # (a masked NaN weight would reach x.grad as 0 * NaN)
        out = torch.where(valid[:, None], out + term, out)
    return _canonical_nan(out)


class Interpolated(Function):
    """``Interpolated.apply(x, idx, weights, skip or None)``: ``x[B,C,N]`` interpolated along ``idx[B,M,k]`` with
    ``weights[B,M,k]`` into channels 0 .. C-1 of ONE ``[B, C + C2, M]`` tensor (``pcc_interpolate`` with ``out_c`` /
    ``out_c0``: no ``cat`` of the interpolated half), ``skip[B,C2,M]`` copied behind them; the backward reads its slice of
    the incoming gradient in place (``pcc_interpolate_bwd``) and computes the gradients that are asked for only.
    Differentiable in ``x``, ``weights`` and ``skip``.  The arguments have passed ``_interp_args``."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, skip: torch.Tensor | None) -> torch.Tensor:
        x, idx, weights = x.contiguous(), idx.contiguous(), weights.contiguous()
        b, c, n = x.shape
        m, k = idx.shape[1:]
        dev = x.device
        c2 = 0 if skip is None else skip.shape[1]
        # (checked before anything is allocated on the device)
        xp, ip, wp = ptr(x, 'x', F32, dev), ptr(idx, 'idx', I64, dev), ptr(weights, 'weights', F32, dev)
        if skip is not None:
            _float32('skip', skip)
            _same_device('skip', skip, dev)
        out = torch.empty((b, c + c2, m), dtype=F32, device=dev)
        call(_L.pcc_interpolate, 'interpolate', dev, b, c, n, m, k, xp, ip, wp, ptr(out, 'out', F32, dev), c + c2, 0)
        if skip is not None:
            out[:, c:].copy_(skip)
        ctx.save_for_backward(x, idx, weights)
        ctx.c2 = c2
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, ...]:
        x, idx, weights = ctx.saved_tensors
        b, c, n = x.shape
        m, k = idx.shape[1:]
        grad = grad.contiguous()
        dev = grad.device
        gx = torch.empty((b, c, n), dtype=F32, device=dev) if ctx.needs_input_grad[0] else None
        gw = torch.empty((b, m, k), dtype=F32, device=dev) if ctx.needs_input_grad[2] else None
        if gx is not None or gw is not None:
            call(_L.pcc_interpolate_bwd, 'interpolate_bwd', dev, b, c, n, m, k, ptr(x, 'x', F32, dev), ptr(idx, 'idx', I64, dev),
                 ptr(weights, 'weights', F32, dev), ptr(grad, 'grad', F32, dev), c + ctx.c2, 0, ptr(gx, 'grad_x', F32, dev),
                 ptr(gw, 'grad_weights', F32, dev))
        gskip = grad[:, c:] if ctx.c2 and ctx.needs_input_grad[3] else None
        return gx, None, gw, gskip


def interpolate_points(x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """``out[B,C,M]``: the features ``x[B,C,N]`` of a sparse cloud interpolated onto M dense points along ``idx[B,M,k]`` int64
    (the list of ``knn_cross`` with the dense points as queries) with ``weights[B,M,k]`` (``interpolation_weights`` of the
    list's distances, or any others): ``out[b,ch,i] = sum_j weights[b,i,j] * x[b,ch,idx[b,i,j]]``, in float32 slot by slot:
    one rounded product and one rounded sum each.  A slot whose index is outside ``[0, N)`` adds nothing, whatever its
    weight, and carries no gradient.  Both tensors float32; differentiable in ``x`` and ``weights`` (``idx`` carries no
    gradient).  The full contract is ``pcc_interpolate``'s (include/pcc_neighbour.h).  The HIP kernels on the accelerator, the
    same rule as a torch composition for CPU tensors: the forwards agree word for word."""
    _interp_args(x, idx, weights)
    if x.device.type == 'cuda':
        return Interpolated.apply(x, idx.detach(), weights, None)
    return torch_interpolate_points(x, idx.detach(), weights)


class FeaturePropagation(NamedTuple):
    """What ``feature_propagation`` returns."""

    out: torch.Tensor      # [B,C+C2,M] the interpolated features, then the skip features
    idx: torch.Tensor      # [B,M,min(k,N)] int64 into the sparse cloud (knn_cross)
    weights: torch.Tensor  # [B,M,min(k,N)] float32 inverse-distance weights (interpolation_weights)


def feature_propagation(xyz_dense: torch.Tensor, xyz_sparse: torch.Tensor, features: torch.Tensor, skip: torch.Tensor | None = None,
                        k: int = 3, eps: float = 1e-8) -> FeaturePropagation:
    """The interpolation step of a feature-propagation layer in one call: ``knn_cross`` finds for every point of
    ``xyz_dense[B,M,3]`` its ``min(k, N)`` nearest points of ``xyz_sparse[B,N,3]``, ``interpolation_weights(dist, eps)`` turns
    their squared distances into weights, and one op fills ``out[B,C+C2,M]``: channels 0 .. C-1 ``features[B,C,N]``
    interpolated along that list, the rest ``skip[B,C2,M]`` (absent for ``skip=None``).  Gradients reach ``features`` and
    ``skip``; ``idx`` and ``weights`` are constants of the graph, because ``knn_cross`` detaches its inputs: for gradients
    through the weights call ``knn_cross``, ``interpolation_weights`` and ``interpolate_points`` separately.  For CPU tensors
    the torch formulas of the three functions (the search's expanded-form distances clamped at 0).  The arguments are
    checked before anything runs."""
    what = 'feature_propagation'
    b, m = _cloud_arg(what, 'xyz_dense', xyz_dense, min_n=0, axis='M')
    _, n = _cloud_arg(what, 'xyz_sparse', xyz_sparse, b)
    if features.dim() != 3 or features.shape[0] != b or features.shape[2] != n or features.shape[1] < 1:
        raise ValueError(f'{what}: expected features[B = {b},C,N = {n}] with C >= 1, got {tuple(features.shape)}')
    if skip is not None and (skip.dim() != 3 or skip.shape[0] != b or skip.shape[2] != m):
        raise ValueError(f'{what}: expected skip[B = {b},C2,M = {m}], got {tuple(skip.shape)}')
    _k_arg(what, k)
    dev = xyz_dense.device
    for name, t in (('xyz_dense', xyz_dense), ('xyz_sparse', xyz_sparse), ('features', features), ('skip', skip)):
        if t is not None:
            _float32(name, t)
            _same_device(name, t, dev)
    idx, dist = knn_cross(xyz_dense.detach().transpose(1, 2), xyz_sparse.detach().transpose(1, 2), min(int(k), n), return_distance=True)
    if dev.type != 'cuda':
        dist = dist.clamp_min(0)  # (the expanded form of the torch search can round below 0; the kernel's difference form cannot)
    weights = interpolation_weights(dist, eps)
    if dev.type == 'cuda':
        out = Interpolated.apply(features, idx, weights, skip)
    else:
        out = torch_interpolate_points(features, idx, weights)
        if skip is not None:
            out = torch.cat((out, skip), 1)
    return FeaturePropagation(out, idx, weights)
