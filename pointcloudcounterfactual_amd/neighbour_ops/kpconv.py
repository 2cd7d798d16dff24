# ---- kernel point convolution: influences of kernel points on the neighbours, a weighted sum per kernel point ---------------

from __future__ import annotations

import numbers
from typing import Any

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._float32 import sqrt32
from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import (F32, I64, _L, _canonical_nan, _cloud_arg, _features_arg, _float32, _list_arg,
                                                              _list_on, _list_slots, _same_device, _slot_values, _zero)
from pointcloudcounterfactual_amd.neighbour_ops.attention import MAX_LIST_K

MAX_KERNEL_POINTS = 32  # pcc_kpconv_aggregate's limit


def kernel_point_layout(kp: int, radius: float = 1.0) -> torch.Tensor:
    """A deterministic default disposition ``[kp,3]`` float32 of ``kp`` kernel points: point 0 at the origin, the others on
    the sphere of ``radius`` along a Fibonacci spiral -- point ``t >= 1`` is ``radius * (r cos a, r sin a, z)`` with
    ``i = t - 1``, ``z = 1 - (2 i + 1) / (kp - 1)``, ``r = sqrt(1 - z^2)`` and ``a = i * pi * (3 - sqrt(5))``, computed in
    float64 and rounded to float32.  It is NOT the paper's energy-optimised disposition: every function here accepts any
    ``[kp,3]`` tensor, the published dispositions included."""
    if isinstance(kp, bool) or not isinstance(kp, numbers.Integral) or not 1 <= kp <= MAX_KERNEL_POINTS:
        raise ValueError(f'kernel_point_layout: kp must be an integer in [1, {MAX_KERNEL_POINTS}], got {kp!r}')
    pts = torch.zeros((kp, 3), dtype=torch.float64)
    if kp > 1:
        i = torch.arange(kp - 1, dtype=torch.float64)
        z = 1.0 - (2.0 * i + 1.0) / (kp - 1)
        r = torch.sqrt(1.0 - z * z)
        a = i * (torch.pi * (3.0 - 5.0 ** 0.5))
        pts[1:] = torch.stack((r * torch.cos(a), r * torch.sin(a), z), 1) * float(radius)
    return pts.to(F32)


def _kpconv_args(what: str, x: torch.Tensor | None, xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor,
                 kernel_points: torch.Tensor, sigma: Any) -> tuple[int, int, int, int, int]:
    """The checks of the kernel point ops before anything runs: ``(b, n, m, k, kp)``.  ``x`` is None where there are no
    features (``kernel_point_influence``)."""
    if x is not None:
        b, _, n = _features_arg(what, x, 'x')
        _cloud_arg(what, 'xyz', xyz, b)
        if xyz.shape[1] != n:
            raise ValueError(f'{what}: expected xyz[B = {b},N = {n},3], got {tuple(xyz.shape)}')
    else:
        b, n = _cloud_arg(what, 'xyz', xyz)
    m, k = _list_arg(what, idx, b)
    if tuple(centres.shape) != (b, m, 3):
        raise ValueError(f'{what}: expected centres[B = {b},M = {m},3], got {tuple(centres.shape)}')
    if kernel_points.dim() != 2 or kernel_points.shape[1] != 3 or not 1 <= kernel_points.shape[0] <= MAX_KERNEL_POINTS:
        raise ValueError(f'{what}: expected kernel_points[K,3] with 1 <= K <= {MAX_KERNEL_POINTS}, got {tuple(kernel_points.shape)}')
    if k > MAX_LIST_K:
        raise ValueError(f'{what}: k must be <= {MAX_LIST_K}, got {k}')
    if isinstance(sigma, bool) or not isinstance(sigma, numbers.Real) or not 0.0 < float(sigma) < float('inf'):
        raise ValueError(f'{what}: sigma must be a finite number > 0, got {sigma!r}')
    first = xyz if x is None else x
    for name, t in (('x', x), ('xyz', xyz), ('centres', centres), ('kernel_points', kernel_points)):
        if t is not None:
            _float32(name, t)
            _same_device(name, t, first.device)
    _list_on(idx, first.device)
    return b, n, m, k, kernel_points.shape[0]


def _influence(xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor, kernel_points: torch.Tensor, sigma: float) -> torch.Tensor:
    """``pcc_kpconv_aggregate``'s influences in float32 torch operations, each rounded: ``h[B,M,k,K]``, +0.0 on a slot that
    is no point."""
    b, n = xyz.shape[:2]
    m, k = idx.shape[1:]
    valid, safe = _list_slots(idx, n)
    nb = torch.gather(xyz, 1, safe.reshape(b, m * k, 1).expand(-1, -1, 3)).view(b, m, k, 3)
    e = (nb - centres[:, :, None, :])[:, :, :, None, :] - kernel_points  # [B,M,k,K,3]
    ex, ey, ez = e.unbind(-1)
    d2 = (ex * ex + ey * ey) + ez * ez
    inv = torch.ones((), dtype=F32, device=xyz.device) / torch.tensor(sigma, dtype=F32, device=xyz.device)
    v = 1.0 - sqrt32(d2) * inv
    return torch.where((v > 0) & valid[..., None], v, _zero(v))


def kernel_point_influence(xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor, kernel_points: torch.Tensor,
                           sigma: float) -> torch.Tensor:
    """``h[B,M,k,K]`` float32: KPConv's linear influence ``max(0, 1 - |x_j - c_i - q_t| / sigma)`` of kernel point
    ``kernel_points[t]`` on the neighbour ``xyz[b, idx[b,i,j]]`` of the centre ``centres[b,i]``, in the words of
    ``pcc_kpconv_aggregate``'s contract (include/pcc_neighbour.h): +0.0 on a slot whose index is outside ``[0, N)`` and
    for a NaN or infinite distance.  Torch operations on either device and no gradient: what a variant of the convolution
    (another normalisation, another aggregation) starts from."""
    _kpconv_args('kernel_point_influence', None, xyz, centres, idx, kernel_points, sigma)
    with torch.no_grad():
        return _influence(xyz, centres, idx, kernel_points, float(sigma))


def torch_kpconv_aggregate(x: torch.Tensor, xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor,
                           kernel_points: torch.Tensor, sigma: float) -> torch.Tensor:
    """The rule of ``pcc_kpconv_aggregate`` in float32 torch operations (no autograd): per slot a gather, a rounded product
    and a rounded addition where the influence is positive, in slot order."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    kp = kernel_points.shape[0]
    h = _influence(xyz, centres, idx, kernel_points, sigma).permute(0, 3, 1, 2)  # [B,K,M,k]
    v = _slot_values(x, _list_slots(idx, n)[1], None)
    out = torch.zeros((b, kp, c, m), dtype=x.dtype, device=x.device)
    for j in range(k):
        hj = h[:, :, None, :, j]
        out = torch.where(hj > 0, out + hj * v[:, None, :, :, j], out)
    return _canonical_nan(out).view(b, kp * c, m)


def torch_kpconv_aggregate_bwd(xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor, kernel_points: torch.Tensor,
                               sigma: float, grad_out: torch.Tensor, n: int) -> torch.Tensor:
    """The rule of ``pcc_kpconv_aggregate_bwd``: per slot the sum over the kernel points in ascending order, then a
    ``scatter_add_`` over the slots."""
    b, m, k = idx.shape
    kp = kernel_points.shape[0]
    c = grad_out.shape[1] // kp
    h = _influence(xyz, centres, idx, kernel_points, sigma)  # [B,M,k,K]
    go = grad_out.view(b, kp, c, m)
    p = torch.zeros((b, c, m, k), dtype=grad_out.dtype, device=grad_out.device)
    for t in range(kp):
        ht = h[:, None, :, :, t]
        p = torch.where(ht > 0, p + ht * go[:, t, :, :, None], p)
    valid, safe = _list_slots(idx, n)
    return torch.zeros((b, c, n), dtype=p.dtype, device=p.device).scatter_add_(2, safe.reshape(b, 1, m * k).expand(-1, c, -1),
                                                                               p.reshape(b, c, m * k))


def hip_kpconv_aggregate(x: torch.Tensor, xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor,
                         kernel_points: torch.Tensor, sigma: float) -> torch.Tensor:
    """``pcc_kpconv_aggregate`` on contiguous device tensors (no autograd): ``[B, K * C, M]``."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    kp = kernel_points.shape[0]
    dev = x.device
    # (checked before anything is allocated on the device)
    ptrs = (ptr(xyz, 'xyz', F32, dev), ptr(centres, 'centres', F32, dev), ptr(idx, 'idx', I64, dev), ptr(x, 'x', F32, dev),
            ptr(kernel_points, 'kernel_points', F32, dev))
    out = torch.empty((b, kp * c, m), dtype=F32, device=dev)
    call(_L.pcc_kpconv_aggregate, 'kpconv_aggregate', dev, b, c, n, m, k, kp, *ptrs, sigma, ptr(out, 'out', F32, dev))
    return out


class KernelPointAggregated(Function):
    """``KernelPointAggregated.apply(x, xyz, centres, idx, kernel_points, sigma)``: ``pcc_kpconv_aggregate`` and
    ``pcc_kpconv_aggregate_bwd``; for CPU tensors the same rules in torch.  Differentiable in ``x`` alone.  The arguments
    have passed ``_kpconv_args``."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor, kernel_points: torch.Tensor,
                sigma: float) -> torch.Tensor:
        x, xyz, centres, idx, kernel_points = (t.contiguous() for t in (x, xyz, centres, idx, kernel_points))
        if x.device.type == 'cuda':
            out = hip_kpconv_aggregate(x, xyz, centres, idx, kernel_points, sigma)
        else:
            out = torch_kpconv_aggregate(x, xyz, centres, idx, kernel_points, sigma)
        ctx.save_for_backward(xyz, centres, idx, kernel_points)
        ctx.sigma, ctx.cn = sigma, x.shape[1:]
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, ...]:
        xyz, centres, idx, kernel_points = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 6
        c, n = ctx.cn
        b, m, k = idx.shape
        kp = kernel_points.shape[0]
        grad = grad.contiguous()
        dev = grad.device
        if dev.type != 'cuda':
            return (torch_kpconv_aggregate_bwd(xyz, centres, idx, kernel_points, ctx.sigma, grad, n),) + (None,) * 5
        gx = torch.empty((b, c, n), dtype=F32, device=dev)
        call(_L.pcc_kpconv_aggregate_bwd, 'kpconv_aggregate_bwd', dev, b, c, n, m, k, kp, ptr(xyz, 'xyz', F32, dev),
             ptr(centres, 'centres', F32, dev), ptr(idx, 'idx', I64, dev), ptr(kernel_points, 'kernel_points', F32, dev), ctx.sigma,
             ptr(grad, 'grad', F32, dev), ptr(gx, 'grad_x', F32, dev))
        return (gx,) + (None,) * 5


def kpconv_aggregate(x: torch.Tensor, xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor, kernel_points: torch.Tensor,
                     sigma: float) -> torch.Tensor:
    """``out[B, K * C, M]``: ``out[b, t * C + ch, i] = sum_j h[b,i,j,t] * x[b,ch,idx[b,i,j]]`` with ``h`` the linear influence
    of ``kernel_point_influence`` -- the aggregation of rigid KPConv along ``idx[B,M,k]`` int64, a list of the centres
    ``centres[B,M,3]`` into the points ``xyz[B,N,3]`` with the features ``x[B,C,N]``; ``kernel_points[K,3]`` (K <= 32) are
    shared by the batch and ``sigma`` is the extent of a kernel point's influence (KPConv's ``KP_extent``).  In float32 slot
    by slot: a rounded product and a rounded addition where the influence is positive; a pair whose influence is 0 and a
    slot whose index is outside ``[0, N)`` (the -1 of ``ball_query(pad='none')``, KPConv's shadow index N) add nothing and
    carry no gradient.  The convolution is then one matrix product over the result: ``kernel_point_conv``.  Differentiable
    in ``x`` only (coordinates and kernel points are constants; nothing is computed when ``x`` needs no gradient).  The full
    contract is ``pcc_kpconv_aggregate``'s (include/pcc_neighbour.h).  The HIP kernels on the accelerator, the same rule in
    torch for CPU tensors: the forwards agree word for word."""
    _kpconv_args('kpconv_aggregate', x, xyz, centres, idx, kernel_points, sigma)
    return KernelPointAggregated.apply(x, xyz.detach(), centres.detach(), idx.detach(), kernel_points.detach(), float(sigma))


def _kpconv_weight_args(what: str, c: int, kp: int, weight: torch.Tensor, bias: torch.Tensor | None) -> None:
    if weight.dim() != 3 or tuple(weight.shape[:2]) != (kp, c) or weight.shape[2] < 1:
        raise ValueError(f'{what}: expected weight[K = {kp},C = {c},O] with O >= 1, got {tuple(weight.shape)}')
    if bias is not None and tuple(bias.shape) != (weight.shape[2],):
        raise ValueError(f'{what}: expected bias[O = {weight.shape[2]}], got {tuple(bias.shape)}')


def kernel_point_conv(x: torch.Tensor, xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor, kernel_points: torch.Tensor,
                      sigma: float, weight: torch.Tensor, bias: torch.Tensor | None = None) -> torch.Tensor:
    """Rigid KPConv: ``out[B,O,M] = sum_t weight[t]^T @ (sum_j h[b,i,j,t] x_j)`` (+ ``bias[O]``) with ``weight[K,C,O]`` (the
    ``weights[K, in, out]`` of the published implementation) -- ``kpconv_aggregate`` followed by one batched matrix product
    ``weight.view(K * C, O)^T @ [B, K * C, M]``.  Not divided by the neighbour count.  Differentiable in ``x``, ``weight``
    and ``bias``."""
    _kpconv_args('kernel_point_conv', x, xyz, centres, idx, kernel_points, sigma)
    kp, c = kernel_points.shape[0], x.shape[1]
    _kpconv_weight_args('kernel_point_conv', c, kp, weight, bias)
    agg = KernelPointAggregated.apply(x, xyz.detach(), centres.detach(), idx.detach(), kernel_points.detach(), float(sigma))
    out = torch.matmul(weight.reshape(kp * c, -1).t(), agg)
    return out if bias is None else out + bias[None, :, None]


class KernelPointConv(torch.nn.Module):
    """A rigid KPConv layer: ``forward(x[B,C,N], xyz[B,N,3], centres[B,M,3], idx[B,M,k]) -> [B,O,M]`` through
    ``kernel_point_conv``.  ``weight[K,C,O]`` is drawn Kaiming-uniform over the fan-in ``K * C`` (``U(-1/sqrt(K C),
    1/sqrt(K C))``, torch's default for a linear layer of that fan-in), ``bias[O]`` is optional and starts at zero, and the
    kernel points are a buffer: ``kernel_points[K,3]`` if given, ``kernel_point_layout(num_kernel_points, radius)``
    otherwise.  ``sigma`` is the extent of a kernel point's influence (KPConv's ``KP_extent``)."""

    def __init__(self, in_channels: int, out_channels: int, sigma: float, radius: float = 1.0, num_kernel_points: int = 15,
                 bias: bool = False, kernel_points: torch.Tensor | None = None) -> None:
        super().__init__()
        pts = kernel_point_layout(num_kernel_points, radius) if kernel_points is None else kernel_points.detach().to(F32).clone()
        if pts.dim() != 2 or pts.shape[1] != 3 or not 1 <= pts.shape[0] <= MAX_KERNEL_POINTS:
            raise ValueError(f'KernelPointConv: expected kernel_points[K,3] with 1 <= K <= {MAX_KERNEL_POINTS}, got {tuple(pts.shape)}')
        if in_channels < 1 or out_channels < 1:
            raise ValueError(f'KernelPointConv: channels must be >= 1, got {in_channels} and {out_channels}')
        self.sigma = float(sigma)
        self.register_buffer('kernel_points', pts)
        self.weight = torch.nn.Parameter(torch.empty(pts.shape[0], in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.zeros(out_channels)) if bias else None
        bound = (pts.shape[0] * in_channels) ** -0.5
        torch.nn.init.uniform_(self.weight, -bound, bound)

    def forward(self, x: torch.Tensor, xyz: torch.Tensor, centres: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        return kernel_point_conv(x, xyz, centres, idx, self.kernel_points, self.sigma, self.weight, self.bias)
