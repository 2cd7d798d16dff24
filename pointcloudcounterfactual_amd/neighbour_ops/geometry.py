# ---- local surface geometry along a list: mean, scatter matrix, its eigen-decomposition, surface variation ----------------

from __future__ import annotations

from typing import Any, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import (F32, I64, _L, _canonical_nan, _cloud_arg, _float32, _k_arg, _list_arg, _list_on,
                                                              _list_slots, _same_device, _zero)
from pointcloudcounterfactual_amd.neighbour_ops.search import knn


def _geometry_args(xyz: torch.Tensor, idx: torch.Tensor, what: str) -> tuple[int, int, int, int]:
    """The checks ``local_covariance`` / ``local_geometry`` make before anything runs: ``(b, n, m, k)``."""
    b, n = _cloud_arg(what, 'xyz', xyz)
    m, k = _list_arg(what, idx, b)
    _float32('xyz', xyz)
    _list_on(idx, xyz.device)
    return b, n, m, k


def torch_local_covariance(xyz: torch.Tensor, idx: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The rule of ``pcc_local_geometry`` (include/pcc_neighbour.h) for ``(cov[B,M,3,3], mean[B,M,3])`` as a torch
    composition over the slots of the list, in slot order: CPU path of ``local_covariance``, differentiable through
    autograd.  A slot outside ``[0, N)`` is skipped; a NaN result is the word 0x7fc00000."""
    b, n, _ = xyz.shape
    m, k = idx.shape[1:]
    valid, safe = _list_slots(idx, n)
    pts = [torch.gather(xyz, 1, safe[:, :, j, None].expand(-1, -1, 3)) for j in range(k)]
    acc = torch.zeros((b, m, 3), dtype=xyz.dtype, device=xyz.device)
    for j in range(k):
        acc = torch.where(valid[:, :, j, None], acc + pts[j], acc)
    cnt = valid.sum(-1)[:, :, None]
    mean = torch.where(cnt > 0, acc / cnt.clamp(min=1).to(xyz.dtype), _zero(xyz))
    cov = torch.zeros((b, m, 3, 3), dtype=xyz.dtype, device=xyz.device)
    for j in range(k):
        d = pts[j] - mean
        cov = torch.where(valid[:, :, j, None, None], cov + d[:, :, :, None] * d[:, :, None, :], cov)
    return _canonical_nan(cov), _canonical_nan(mean)


def _hip_local_geometry(xyz: torch.Tensor, idx: torch.Tensor, want: tuple[bool, bool, bool, bool, bool]) -> list[Any]:
    """``pcc_local_geometry`` on checked, contiguous, detached arguments: ``[mean, cov, eval, evec, curv]``, ``None`` where
    ``want`` does not ask."""
    b, n, _ = xyz.shape
    m, k = idx.shape[1:]
    dev = xyz.device
    xp, ip = ptr(xyz, 'xyz', F32, dev), ptr(idx, 'idx', I64, dev)  # (checked before anything is allocated on the device)
    shapes = ((b, m, 3), (b, m, 3, 3), (b, m, 3), (b, m, 3, 3), (b, m))
    outs = [torch.empty(s, dtype=F32, device=dev) if w else None for s, w in zip(shapes, want)]
    call(_L.pcc_local_geometry, 'local_geometry', dev, b, n, m, k, xp, ip,
         *(ptr(t, name, F32, dev) for t, name in zip(outs, ('mean', 'cov', 'eval', 'evec', 'curv'))))
    return outs


class LocalCovariance(Function):
    """``cov, mean[, eigenvalues, eigenvectors, curvature] = LocalCovariance.apply(xyz, idx, with_eigen)`` over
    ``pcc_local_geometry`` / ``pcc_local_covariance_bwd``: ``cov`` and ``mean`` differentiable in ``xyz``, the eigen outputs
    marked as carrying no gradient.  Only the gradients that arrive are handed to the library.  The arguments have passed
    ``_geometry_args``."""

    @staticmethod
    def forward(ctx: Any, xyz: torch.Tensor, idx: torch.Tensor, with_eigen: bool) -> tuple[torch.Tensor, ...]:
        xyz, idx = xyz.contiguous(), idx.contiguous()
        mean, cov, *eigen = _hip_local_geometry(xyz, idx, (True, True) + (with_eigen,) * 3)
        ctx.save_for_backward(xyz, idx, mean)
        ctx.set_materialize_grads(False)
        if with_eigen:
            ctx.mark_non_differentiable(*eigen)
            return (cov, mean, *eigen)
        return cov, mean

    @staticmethod
    def backward(ctx: Any, grad_cov: torch.Tensor | None, grad_mean: torch.Tensor | None, *eigen_grads: Any) -> tuple[Any, None, None]:
        xyz, idx, mean = ctx.saved_tensors
        b, n, _ = xyz.shape
        m, k = idx.shape[1:]
        dev = xyz.device
        if not ctx.needs_input_grad[0] or (grad_cov is None and grad_mean is None):
            return None, None, None
        if grad_cov is None:  # (only the mean was used)
            grad_cov = torch.zeros((b, m, 3, 3), dtype=F32, device=dev)
        grad_cov = grad_cov.contiguous()
        grad_mean = None if grad_mean is None else grad_mean.contiguous()
        gx = torch.empty((b, n, 3), dtype=F32, device=dev)
        call(_L.pcc_local_covariance_bwd, 'local_covariance_bwd', dev, b, n, m, k, ptr(xyz, 'xyz', F32, dev), ptr(idx, 'idx', I64, dev),
             ptr(mean, 'mean', F32, dev), ptr(grad_cov, 'grad_cov', F32, dev), ptr(grad_mean, 'grad_mean', F32, dev),
             ptr(gx, 'grad_xyz', F32, dev))
        return gx, None, None


def local_covariance(xyz: torch.Tensor, idx: torch.Tensor, return_mean: bool = False) -> Any:
    """``cov[B,M,3,3]``: the scatter matrix of the points of ``xyz[B,N,3]`` that each row of ``idx[B,M,k]`` int64 names (the
    list of ``knn``, ``knn_cross`` or ``ball_query``; M != N allowed), about their mean and NOT divided by their number (the
    convention of ``get_local_covariance``); with ``return_mean`` also ``mean[B,M,3]``.  A slot whose index is outside
    ``[0, N)`` (the -1 of ``pad='none'``) is skipped; a repeated index counts as often as it occurs, so ``pad='none'`` is the
    unbiased choice for ball-query lists.  Float32 in slot order, the rule of ``pcc_local_geometry``
    (include/pcc_neighbour.h): one fused HIP kernel on the accelerator, the same rule as a torch composition for CPU
    tensors, and the two agree word for word.  Differentiable in ``xyz`` (``idx`` carries no gradient)."""
    _geometry_args(xyz, idx, 'local_covariance')
    if xyz.device.type == 'cuda':
        cov, mean = LocalCovariance.apply(xyz, idx.detach(), False)
    else:
        cov, mean = torch_local_covariance(xyz, idx.detach())
    return (cov, mean) if return_mean else cov


class LocalGeometry(NamedTuple):
    """What ``local_geometry`` returns."""

    mean: torch.Tensor          # [B,M,3] the mean of each row's points (differentiable in xyz)
    cov: torch.Tensor           # [B,M,3,3] their scatter matrix (differentiable in xyz)
    eigenvalues: torch.Tensor   # [B,M,3] ascending (no gradient)
    eigenvectors: torch.Tensor  # [B,M,3,3] row r is the unit eigenvector of eigenvalue r; row 0 is the normal (no gradient)
    curvature: torch.Tensor     # [B,M] the surface variation max(l0, 0) / (l0 + l1 + l2) (no gradient)


def torch_scatter_eigen(cov: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``(eigenvalues, eigenvectors, curvature)`` of float32 scatter matrices ``cov[...,3,3]`` by ``torch.linalg.eigh`` in
    float64, then the contract of ``pcc_local_geometry`` applied to its result: ascending order, a decoupled axis (both
    off-diagonal entries of its row exactly 0) returned as an exact unit vector with the diagonal entry as its eigenvalue,
    the identity for a zero matrix, the sign rule, and NaN for a matrix with a non-finite entry.  CPU path of
    ``local_geometry``."""
    shape = cov.shape[:-2]
    s = cov.detach().reshape(-1, 3, 3).double()
    rows = s.shape[0]
    finite = torch.isfinite(s).all(-1).all(-1)
    s = torch.where(finite[:, None, None], s, _zero(s))
    s = torch.triu(s) + torch.triu(s, 1).transpose(1, 2)  # (the upper triangle is the matrix)
    val, vec = torch.linalg.eigh(s)
    vec = vec.transpose(1, 2).contiguous()  # rows are eigenvectors
    eye = torch.eye(3, dtype=s.dtype)
    diag = torch.diagonal(s, dim1=1, dim2=2)
    o01, o02, o12 = s[:, 0, 1] == 0, s[:, 0, 2] == 0, s[:, 1, 2] == 0
    alone = (o01 & o02, o01 & o12, o02 & o12)  # axis a is decoupled
    for a, (p, q) in enumerate(((1, 2), (0, 2), (0, 1))):
        pick = (alone[a] & ~(o01 & o02 & o12)).nonzero()[:, 0]
        if pick.numel():  # the 2x2 block of the other two axes; then the three pairs in ascending order
            bval, bvec = torch.linalg.eigh(s[pick][:, [p, q]][:, :, [p, q]])
            vals = torch.cat((diag[pick, a, None], bval), 1)
            vecs = torch.zeros((pick.numel(), 3, 3), dtype=s.dtype)
            vecs[:, 0, a] = 1
            vecs[:, 1:, p], vecs[:, 1:, q] = bvec[:, 0, :], bvec[:, 1, :]
            order = torch.sort(vals, dim=1, stable=True)[1]
            val[pick] = torch.gather(vals, 1, order)
            vec[pick] = torch.gather(vecs, 1, order[:, :, None].expand(-1, -1, 3))
    pick = (o01 & o02 & o12).nonzero()[:, 0]
    if pick.numel():  # a diagonal matrix: its axes, equal values in axis order
        dval, order = torch.sort(diag[pick], dim=1, stable=True)
        val[pick], vec[pick] = dval, eye[order]
    trace = (val[:, 0] + val[:, 1]) + val[:, 2]
    curv = torch.where(trace > 0, val[:, 0].clamp(min=0) / torch.where(trace > 0, trace, torch.ones_like(trace)), torch.zeros_like(trace))
    val, vec, curv = val.to(cov.dtype), vec.to(cov.dtype), curv.to(cov.dtype)
    lead = torch.gather(vec, 2, vec.abs().argmax(2, keepdim=True))  # (argmax returns the first of equal maxima)
    vec = torch.where(lead < 0, -vec, vec) + 0.0  # (no -0.0 is left behind)
    nan = torch.full((), float('nan'), dtype=cov.dtype)
    val, vec, curv = torch.where(finite[:, None], val, nan), torch.where(finite[:, None, None], vec, nan), torch.where(finite, curv, nan)
    return val.reshape(shape + (3,)), vec.reshape(shape + (3, 3)), curv.reshape(shape)


def local_geometry(xyz: torch.Tensor, idx: torch.Tensor) -> LocalGeometry:
    """The per-neighbourhood geometry of ``xyz[B,N,3]`` along ``idx[B,M,k]`` int64 in one call: ``mean`` and ``cov`` as
    ``local_covariance`` returns them, the eigenvalues of ``cov`` in ascending order, its unit eigenvectors as the rows of
    ``eigenvectors[B,M,3,3]`` (row 0 is the surface normal; the component of largest magnitude of each row is non-negative)
    and ``curvature[B,M]``, the surface variation ``max(l0, 0) / (l0 + l1 + l2)``.  A zero matrix (fewer than two valid
    slots) returns eigenvalues 0 and the axes; a non-finite one NaN.  The full contract is ``pcc_local_geometry``'s
    (include/pcc_neighbour.h): one fused HIP kernel on the accelerator (a float32 Jacobi iteration in registers); for CPU
    tensors ``torch.linalg.eigh`` in float64 on the float32 ``cov`` with the contract's ordering, sign rule and degenerate
    cases applied afterwards.  ``mean`` and ``cov`` are differentiable in ``xyz``; the eigen outputs carry NO gradient: call
    ``torch.linalg.eigh`` on the differentiable ``cov`` where one is needed."""
    _geometry_args(xyz, idx, 'local_geometry')
    idx = idx.detach()
    if xyz.device.type != 'cuda':
        cov, mean = torch_local_covariance(xyz, idx)
        return LocalGeometry(mean, cov, *torch_scatter_eigen(cov))
    cov, mean, val, vec, curv = LocalCovariance.apply(xyz, idx, True)
    return LocalGeometry(mean, cov, val, vec, curv)


def estimate_normals(xyz: torch.Tensor, k: int = 16, idx: torch.Tensor | None = None, viewpoint: torch.Tensor | None = None,
                     return_curvature: bool = False) -> Any:
    """Unit normals ``[B,N,3]`` of the cloud ``xyz[B,N,3]`` (``[B,M,3]`` along a given ``idx[B,M,k']``): the eigenvector of
    the smallest eigenvalue of each neighbourhood's scatter matrix (``local_geometry``), the neighbourhoods being the
    ``min(k, N)`` nearest neighbours (``knn``, the point itself included) when no list is given.  The sign is the
    contract's (largest component non-negative) unless a ``viewpoint`` of shape ``[3]`` or ``[B,3]`` is given: every normal
    is then flipped to face it, ``n . (viewpoint - mean) >= 0`` with ``mean`` the neighbourhood's mean.  With
    ``return_curvature`` also the surface variation ``[B,N]``.  The inputs are detached: the outputs are constants of the
    graph."""
    what = 'estimate_normals'
    b, n = _cloud_arg(what, 'xyz', xyz)
    xyz = xyz.detach()
    if idx is None:
        _k_arg(what, k)
        _float32('xyz', xyz)
        idx = knn(xyz.transpose(1, 2).contiguous(), min(int(k), n))
    if viewpoint is not None:
        if tuple(viewpoint.shape) not in ((3,), (b, 3)):
            raise ValueError(f'{what}: expected viewpoint[3] or viewpoint[B = {b},3], got {tuple(viewpoint.shape)}')
        _same_device('viewpoint', viewpoint, xyz.device)
    geo = local_geometry(xyz, idx)
    normals = geo.eigenvectors[:, :, 0, :]
    if viewpoint is not None:
        towards = viewpoint.detach().to(normals.dtype).reshape(-1, 1, 3) - geo.mean
        normals = torch.where((normals * towards).sum(-1, keepdim=True) < 0, -normals, normals) + 0.0  # (no -0.0)
    return (normals, geo.curvature) if return_curvature else normals
