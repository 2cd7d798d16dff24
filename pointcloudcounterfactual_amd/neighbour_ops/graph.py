# ---- gather / edge features / max over k -------------------------------------------------------------------------

from __future__ import annotations

from typing import Any, Callable, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import F32, I32, I64, _L
from pointcloudcounterfactual_amd.neighbour_ops.search import knn


class IndexedOp(NamedTuple):
    """One op of ``include/pcc_neighbour.h`` that reads ``x[B,C,N]`` along ``indices[B,N,k]`` and has a backward."""

    what: str  # the C pair is pcc_<what> / pcc_<what>_bwd; also the prefix of their error messages
    out_shape: Callable[[int, int, int, int], tuple[int, ...]]  # of (b, c, n, k)
    argmax: bool = False  # an int32 argmax [B,C,N] is produced, saved and handed to the backward
    names: tuple[str, str] = ('x', 'indices')  # what the pointer checks call the two inputs


GATHER = IndexedOp('gather_neighbours', lambda b, c, n, k: (b, c, n, k))
GRAPH_FEATURES = IndexedOp('graph_features', lambda b, c, n, k: (b, 2 * c, n, k))
GRAPH_MAX_POOL = IndexedOp('graph_max_pool', lambda b, c, n, k: (b, c, n), argmax=True)


class Indexed(Function):
    """``op`` of ``x`` along ``indices`` on the accelerator, differentiable in ``x``: ``Indexed.apply(op, x, indices)``."""

    @staticmethod
    def forward(ctx: Any, op: IndexedOp, x: torch.Tensor, indices: torch.Tensor) -> torch.Tensor:
        x = x.contiguous()
        indices = indices.contiguous()
        b, c, n = x.shape
        k = indices.shape[2]
        dev = x.device
        out = torch.empty(op.out_shape(b, c, n, k), dtype=torch.float32, device=dev)
        arg = (torch.empty((b, c, n), dtype=torch.int32, device=dev),) if op.argmax else ()
        call(getattr(_L, 'pcc_' + op.what), op.what, dev, b, c, n, k, ptr(x, op.names[0], F32, dev),
             ptr(indices, op.names[1], I64, dev), ptr(out, 'out', F32, dev), *(ptr(a, 'arg', I32, dev) for a in arg))
        ctx.save_for_backward(indices, *arg)
        ctx.op, ctx.shape = op, (b, c, n, k)
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[None, torch.Tensor, None]:
        indices, *arg = ctx.saved_tensors
        op, (b, c, n, k) = ctx.op, ctx.shape
        grad = grad.contiguous()
        dev = grad.device
        gx = torch.empty((b, c, n), dtype=torch.float32, device=dev)
        call(getattr(_L, f'pcc_{op.what}_bwd'), op.what + '_bwd', dev, b, c, n, k, ptr(indices, op.names[1], I64, dev),
             *(ptr(a, 'arg', I32, dev) for a in arg), ptr(grad, 'grad', F32, dev), ptr(gx, 'grad_' + op.names[0], F32, dev))
        return None, gx, None


class _GlobalMaxPool(Function):
    @staticmethod
    def forward(ctx: Any, x: torch.Tensor) -> torch.Tensor:
        x = x.contiguous()
        b, c, n = x.shape
        dev = x.device
        out = torch.empty((b, c), dtype=torch.float32, device=dev)
        arg = torch.empty((b, c), dtype=torch.int32, device=dev)
        call(_L.pcc_global_pool, 'global_pool', dev, b, c, n, ptr(x, 'x', F32, dev), ptr(out, 'out', F32, dev),
             ptr(arg, 'arg', I32, dev), None)
        ctx.save_for_backward(arg)
        ctx.n = n
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> torch.Tensor:
        (arg,) = ctx.saved_tensors
        gx = torch.zeros(grad.shape + (ctx.n,), dtype=grad.dtype, device=grad.device)
        gx.scatter_(2, arg.long().unsqueeze(2), grad.unsqueeze(2))
        return gx


def _on_gpu(x: torch.Tensor) -> bool:
    return x.device.type == 'cuda'


def get_neighbours(x: torch.Tensor, indices: torch.Tensor, k: int) -> tuple[torch.Tensor, torch.Tensor]:
    """``(indices, neighbours[B,C,N,k])`` (reference ``neighbour_ops.py:85-94``)."""
    batch, n_feat, n_points = x.size()
    if not indices.numel():
        indices = knn(x, k)
    if _on_gpu(x):
        return indices, Indexed.apply(GATHER, x, indices.to(x.device))
    indices_expanded = indices.contiguous().view(batch, 1, k * n_points).expand(-1, n_feat, -1)
    neighbours = torch.gather(x, 2, indices_expanded).view(batch, n_feat, n_points, k)
    return indices, neighbours


def get_local_covariance(x: torch.Tensor, indices: torch.Tensor, k: int = 16) -> torch.Tensor:
    """Reference ``neighbour_ops.py:97-103``: ``cat([x, scatter matrices])`` for any channel count, as the reference
    writes it (gather, subtract the mean, ``matmul``).  For coordinates the fused form is ``local_covariance`` (one HIP
    kernel along any list, M != N and padded rows included), and ``local_geometry`` adds the eigen-decomposition."""
    neighbours = get_neighbours(x, indices, k)[1]
    neighbours = neighbours - neighbours.mean(3, keepdim=True)
    covariances = torch.matmul(neighbours.transpose(1, 2), neighbours.permute(0, 2, 3, 1))
    return torch.cat([x, covariances.flatten(start_dim=2).transpose(1, 2)], dim=1).contiguous()


def graph_max_pooling(x: torch.Tensor, indices: torch.Tensor, k: int = 16) -> torch.Tensor:
    """``max_j x[:, :, indices[:, n, j]]`` (reference ``neighbour_ops.py:106-110``)."""
    if _on_gpu(x):
        if not indices.numel():
            indices = knn(x, k)
        return Indexed.apply(GRAPH_MAX_POOL, x, indices.to(x.device))
    neighbours = get_neighbours(x, indices, k)[1]
    return torch.max(neighbours, dim=-1)[0]


def get_graph_features(x: torch.Tensor, indices: torch.Tensor, k: int = 20) -> tuple[torch.Tensor, torch.Tensor]:
    """``(indices, cat([neighbours - x, x])[B,2C,N,k])`` (reference ``neighbour_ops.py:113-119``)."""
    if _on_gpu(x):
        if not indices.numel():
            indices = knn(x, k)
        return indices, Indexed.apply(GRAPH_FEATURES, x, indices.to(x.device))
    indices_out, neighbours = get_neighbours(x, indices, k)
    xe = x.unsqueeze(3).expand(-1, -1, -1, k)
    return indices_out, torch.cat([neighbours - xe, xe], dim=1).contiguous()


def graph_filtering(x: torch.Tensor, k: int = 4) -> torch.Tensor:
    """Laplacian-like smoothing of the decoder output (reference ``neighbour_ops.py:122-133``)."""
    neighbours = get_neighbours(x, k=k, indices=torch.empty(0))[1]
    neighbours = neighbours[..., 1:]  # the closest neighbour is the point itself
    diff = x.unsqueeze(-1).expand(-1, -1, -1, k - 1) - neighbours
    dist = torch.sqrt(abs((diff**2).sum(1)))
    sigma = torch.clamp(dist[..., 0:1].mean(1, keepdim=True), min=0.005)
    weights = torch.exp(-(dist / sigma))
    x_weight = weights.sum(2).unsqueeze(1).expand(-1, 3, -1)
    weighted_neighbours = weights.unsqueeze(1).expand(-1, 3, -1, -1) * neighbours
    return (1 + x_weight) * x - weighted_neighbours.sum(-1)


def global_max_pool(x: torch.Tensor) -> torch.Tensor:
    """``x[B,C,N].max(dim=2)[0]`` of the encoders / classifier (``encoders.py:58,90``; ``classifier.py:63``)."""
    if _on_gpu(x):
        return _GlobalMaxPool.apply(x)
    return x.max(dim=2, keepdim=False)[0]


def global_max_mean_pool(x: torch.Tensor) -> torch.Tensor:
    """``cat(max_n, mean_n)`` of the classifier head (``classifier.py:63-65``) in one read (inference only)."""
    if _on_gpu(x) and not x.requires_grad:
        x = x.contiguous()
        b, c, n = x.shape
        dev = x.device
        both = torch.empty((2, b, c), dtype=torch.float32, device=dev)  # max | mean: each the [B,C] block the kernel writes
        call(_L.pcc_global_pool, 'global_pool', dev, b, c, n, ptr(x, 'x', F32, dev), ptr(both[0], 'max', F32, dev), None,
             ptr(both[1], 'mean', F32, dev))
        return both.transpose(0, 1).reshape(b, 2 * c)
    return torch.cat((global_max_pool(x), x.mean(dim=2)), 1)
