"""Host-side mirror of the reference's ``structural_losses.structural_losses_backend`` pybind module
(``external/pytorch_structural_losses/src/structural_loss.cpp:24-135``): the same five functions, the
same argument meaning, output shapes/dtypes, ownership (fresh ``torch.empty`` outputs) and error
behaviour (``RuntimeError`` when an input is not a contiguous accelerator tensor), enqueuing on the
current stream without synchronising.  The arithmetic is the C-ABI library's HIP kernels; PyTorch is
only used for device memory and the stream handle.
"""

from __future__ import annotations

import ctypes

import torch

from pointcloudcounterfactual_amd import _lib
from pointcloudcounterfactual_amd._lib import call, ptr

_L = _lib.lib
F32, I32 = torch.float32, torch.int32


def _sizes(set_d: torch.Tensor, set_q: torch.Tensor) -> tuple[int, int, int]:
    return set_d.size(0), set_d.size(1), set_q.size(1)


def ApproxMatch(set_d: torch.Tensor, set_q: torch.Tensor) -> list[torch.Tensor]:
    """-> [match[B,M,N], temp[B,2(N+M)]]   (structural_loss.cpp:24-38)."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    match = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    temp = torch.empty((b, (n + m) * 2), dtype=torch.float32, device=dev)
    call(_L.pcc_approxmatch, 'ApproxMatch', dev, b, n, m, ptr(set_d, 'set_d', F32, dev), ptr(set_q, 'set_q', F32, dev),
         ptr(match, 'match', F32, dev), ptr(temp, 'temp', F32, dev))
    return [match, temp]


def ApproxMatchCost(set_d: torch.Tensor, set_q: torch.Tensor) -> list[torch.Tensor]:
    """ApproxMatch + MatchCost in one pass over ``match`` -> [match, temp, cost[B]] (extension)."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    match = torch.empty((b, m, n), dtype=torch.float32, device=dev)
    temp = torch.empty((b, (n + m) * 2), dtype=torch.float32, device=dev)
    cost = torch.empty((b,), dtype=torch.float32, device=dev)
    call(_L.pcc_approxmatch_cost, 'ApproxMatchCost', dev, b, n, m, ptr(set_d, 'set_d', F32, dev),
         ptr(set_q, 'set_q', F32, dev), ptr(match, 'match', F32, dev), ptr(temp, 'temp', F32, dev),
         ptr(cost, 'cost', F32, dev))
    return [match, temp, cost]


def MatchCostImplicit(set_d: torch.Tensor, set_q: torch.Tensor, with_grad: bool) -> list[torch.Tensor]:
    """``match_cost`` without the match tensor (extension, ``pcc_match_cost``): -> [cost[B]] or, ``with_grad``,
    [cost[B], grad1[B,N,3], grad2[B,M,3]] where the gradients are those of ``MatchCostGrad`` (upstream gradient 1).
    Every match element is evaluated in registers and consumed on the spot; nothing of size B*M*N touches HBM."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    cost = torch.empty((b,), dtype=torch.float32, device=dev)
    out = [cost]
    g1 = g2 = None
    if with_grad:
        g1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
        g2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
        out += [g1, g2]
    call(_L.pcc_match_cost, 'MatchCostImplicit', dev, b, n, m, ptr(set_d, 'set_d', F32, dev),
         ptr(set_q, 'set_q', F32, dev), None, ptr(cost, 'cost', F32, dev), ptr(g1, 'grad1', F32, dev),
         ptr(g2, 'grad2', F32, dev))
    return out


def MatchCost(set_d: torch.Tensor, set_q: torch.Tensor, match: torch.Tensor) -> torch.Tensor:
    """-> cost[B]   (structural_loss.cpp:40-53)."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    out = torch.empty((b,), dtype=torch.float32, device=dev)
    if match.numel() != b * n * m:
        raise RuntimeError(f'match has {match.numel()} elements, expected {b}x{m}x{n}')
    call(_L.pcc_matchcost, 'MatchCost', dev, b, n, m, ptr(set_d, 'set_d', F32, dev), ptr(set_q, 'set_q', F32, dev),
         ptr(match, 'match', F32, dev), ptr(out, 'cost', F32, dev))
    return out


def MatchCostGrad(set_d: torch.Tensor, set_q: torch.Tensor, match: torch.Tensor) -> list[torch.Tensor]:
    """-> [grad1[B,N,3], grad2[B,M,3]]   (structural_loss.cpp:55-70)."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
    if match.numel() != b * n * m:
        raise RuntimeError(f'match has {match.numel()} elements, expected {b}x{m}x{n}')
    call(_L.pcc_matchcostgrad, 'MatchCostGrad', dev, b, n, m, ptr(set_d, 'set_d', F32, dev),
         ptr(set_q, 'set_q', F32, dev), ptr(match, 'match', F32, dev), ptr(grad1, 'grad1', F32, dev),
         ptr(grad2, 'grad2', F32, dev))
    return [grad1, grad2]


def MatchCostGradScaled(set_d: torch.Tensor, set_q: torch.Tensor, match: torch.Tensor,
                        grad_cost: torch.Tensor) -> list[torch.Tensor]:
    """MatchCostGrad with the upstream gradient ``grad_cost[B]`` folded into the reduction (extension): equals
    ``grad * grad_cost[:, None, None]`` of the reference wrapper (match_cost.py:41-42) without the two extra passes."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
    if match.numel() != b * n * m or grad_cost.numel() != b:
        raise RuntimeError('MatchCostGradScaled: match / grad_cost shapes do not match the clouds')
    call(_L.pcc_matchcostgrad_scaled, 'MatchCostGradScaled', dev, b, n, m, ptr(set_d, 'set_d', F32, dev),
         ptr(set_q, 'set_q', F32, dev), ptr(match, 'match', F32, dev), ptr(grad_cost, 'grad_cost', F32, dev),
         ptr(grad1, 'grad1', F32, dev), ptr(grad2, 'grad2', F32, dev))
    return [grad1, grad2]


def NNDistance(set_d: torch.Tensor, set_q: torch.Tensor) -> list[torch.Tensor]:
    """-> [dist1[B,N] f32, idx1[B,N] i32, dist2[B,M] f32, idx2[B,M] i32]   (structural_loss.cpp:81-100)."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    dist1 = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=dev)
    dist2 = torch.empty((b, m), dtype=torch.float32, device=dev)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=dev)
    call(_L.pcc_nndistance, 'NNDistance', dev, b, n, ptr(set_d, 'set_d', F32, dev), m, ptr(set_q, 'set_q', F32, dev),
         ptr(dist1, 'dist1', F32, dev), ptr(idx1, 'idx1', I32, dev), ptr(dist2, 'dist2', F32, dev),
         ptr(idx2, 'idx2', I32, dev))
    return [dist1, idx1, dist2, idx2]


def ChamferLoss(set_d: torch.Tensor, set_q: torch.Tensor, mean: bool) -> list[torch.Tensor]:
    """NNDistance + the loss reduction in one call (extension, ``pcc_chamfer_loss``):
    -> [loss[B], dist1, idx1, dist2, idx2] with loss = mean_j dist1 + mean_k dist2 (``mean``) or the sums."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    loss = torch.empty((b,), dtype=torch.float32, device=dev)
    dist1 = torch.empty((b, n), dtype=torch.float32, device=dev)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=dev)
    dist2 = torch.empty((b, m), dtype=torch.float32, device=dev)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=dev)
    call(_L.pcc_chamfer_loss, 'ChamferLoss', dev, b, n, ptr(set_d, 'set_d', F32, dev), m, ptr(set_q, 'set_q', F32, dev),
         int(mean), ptr(loss, 'loss', F32, dev), ptr(dist1, 'dist1', F32, dev), ptr(idx1, 'idx1', I32, dev),
         ptr(dist2, 'dist2', F32, dev), ptr(idx2, 'idx2', I32, dev))
    return [loss, dist1, idx1, dist2, idx2]


def ChamferLossGrad(set_d: torch.Tensor, set_q: torch.Tensor, idx1: torch.Tensor, idx2: torch.Tensor,
                    grad_loss: torch.Tensor, mean: bool) -> list[torch.Tensor]:
    """NNDistanceGrad with ``grad_dist1[b,:] = grad_loss[b] (/N)``, ``grad_dist2[b,:] = grad_loss[b] (/M)`` formed
    inside the kernel (extension, ``pcc_chamfer_loss_grad``) -> [grad1[B,N,3], grad2[B,M,3]]."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
    if idx1.numel() != b * n or idx2.numel() != b * m or grad_loss.numel() != b:
        raise RuntimeError('ChamferLossGrad: idx / grad_loss shapes do not match the clouds')
    grad_loss, stride = _batch_stride(grad_loss, b)
    call(_L.pcc_chamfer_loss_grad, 'ChamferLossGrad', dev, b, n, ptr(set_d, 'set_d', F32, dev), m,
         ptr(set_q, 'set_q', F32, dev), ptr(idx1, 'idx1', I32, dev), ptr(idx2, 'idx2', I32, dev),
         ptr(grad_loss, 'grad_loss', F32, dev), stride, int(mean), ptr(grad1, 'grad1', F32, dev),
         ptr(grad2, 'grad2', F32, dev))
    return [grad1, grad2]


def ChamferEMD(set_d: torch.Tensor, set_q: torch.Tensor, mean: bool, with_grad: bool,
               return_dist: bool = False) -> list[torch.Tensor]:
    """``ChamferLoss`` and ``MatchCostImplicit`` on the same pair of clouds in ONE call (extension, ``pcc_chamfer_emd``;
    the reference's ChamferEMD loss, metrics_and_losses.py:70-79) -> [chamfer[B], idx1, idx2, emd[B]] (+ [emd_grad1,
    emd_grad2] ``with_grad``) (+ [dist1, dist2] ``return_dist``).  Same bits as the two calls; the nearest-neighbour
    search runs on the clouds the approximate EMD has just Hilbert-sorted, with box culling instead of the exhaustive
    scan."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    loss = torch.empty((b,), dtype=torch.float32, device=dev)
    idx1 = torch.empty((b, n), dtype=torch.int32, device=dev)
    idx2 = torch.empty((b, m), dtype=torch.int32, device=dev)
    cost = torch.empty((b,), dtype=torch.float32, device=dev)
    out = [loss, idx1, idx2, cost]
    g1 = g2 = None
    if with_grad:
        g1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
        g2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
        out += [g1, g2]
    d1 = torch.empty((b, n), dtype=torch.float32, device=dev)  # per-point distances: scratch of the reduction
    d2 = torch.empty((b, m), dtype=torch.float32, device=dev)
    call(_L.pcc_chamfer_emd, 'ChamferEMD', dev, b, n, ptr(set_d, 'set_d', F32, dev), m, ptr(set_q, 'set_q', F32, dev),
         int(mean), ptr(loss, 'loss', F32, dev), ptr(d1, 'dist1', F32, dev), ptr(idx1, 'idx1', I32, dev),
         ptr(d2, 'dist2', F32, dev), ptr(idx2, 'idx2', I32, dev), ptr(cost, 'cost', F32, dev),
         ptr(g1, 'emd_grad1', F32, dev), ptr(g2, 'emd_grad2', F32, dev))
    if return_dist:
        out += [d1, d2]
    return out


def _batch_stride(g: torch.Tensor, b: int) -> tuple[torch.Tensor, int]:
    """An upstream gradient [B] as (tensor, stride): one scalar expanded over the batch (what ``loss.sum().backward()``
    hands down) is read in place through stride 0 as its first element, no copy kernel."""
    stride = g.stride(0) if g.dim() == 1 and b > 1 else 1
    if stride == 0:
        return g[:1], 0
    if stride != 1:
        return g.contiguous(), 1
    return g, 1


def ChamferEMDGrad(set_d: torch.Tensor, set_q: torch.Tensor, idx1: torch.Tensor, idx2: torch.Tensor,
                   grad_chamfer: torch.Tensor, mean: bool, emd_grad1: torch.Tensor, emd_grad2: torch.Tensor,
                   grad_emd: torch.Tensor) -> list[torch.Tensor]:
    """Backward of Chamfer + match_cost on the same clouds in ONE launch (extension, ``pcc_chamfer_emd_grad``):
    ``ChamferLossGrad(grad_chamfer) + emd_grad * grad_emd[:, None, None]`` -> [grad1[B,N,3], grad2[B,M,3]]."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
    if (idx1.numel() != b * n or idx2.numel() != b * m or grad_chamfer.numel() != b or grad_emd.numel() != b
            or emd_grad1.numel() != b * n * 3 or emd_grad2.numel() != b * m * 3):
        raise RuntimeError('ChamferEMDGrad: shapes do not match the clouds')
    grad_chamfer, sc = _batch_stride(grad_chamfer, b)
    grad_emd, se = _batch_stride(grad_emd, b)
    call(_L.pcc_chamfer_emd_grad, 'ChamferEMDGrad', dev, b, n, ptr(set_d, 'set_d', F32, dev), m,
         ptr(set_q, 'set_q', F32, dev), ptr(idx1, 'idx1', I32, dev), ptr(idx2, 'idx2', I32, dev),
         ptr(grad_chamfer, 'grad_chamfer', F32, dev), sc, int(mean), ptr(emd_grad1, 'emd_grad1', F32, dev),
         ptr(emd_grad2, 'emd_grad2', F32, dev), ptr(grad_emd, 'grad_emd', F32, dev), se, ptr(grad1, 'grad1', F32, dev),
         ptr(grad2, 'grad2', F32, dev))
    return [grad1, grad2]


def NNDistanceGrad(set_d: torch.Tensor, set_q: torch.Tensor, idx1: torch.Tensor, idx2: torch.Tensor,
                   grad_dist1: torch.Tensor, grad_dist2: torch.Tensor) -> list[torch.Tensor]:
    """-> [grad1[B,N,3], grad2[B,M,3]]   (structural_loss.cpp:102-125)."""
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    grad1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev)
    grad2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev)
    if idx1.numel() != b * n or grad_dist1.numel() != b * n or idx2.numel() != b * m or grad_dist2.numel() != b * m:
        raise RuntimeError('NNDistanceGrad: idx/grad_dist shapes do not match the clouds')
    call(_L.pcc_nndistancegrad, 'NNDistanceGrad', dev, b, n, ptr(set_d, 'set_d', F32, dev), m,
         ptr(set_q, 'set_q', F32, dev), ptr(grad_dist1, 'grad_dist1', F32, dev), ptr(idx1, 'idx1', I32, dev),
         ptr(grad_dist2, 'grad_dist2', F32, dev), ptr(idx2, 'idx2', I32, dev), ptr(grad1, 'grad1', F32, dev),
         ptr(grad2, 'grad2', F32, dev))
    return [grad1, grad2]


def SlicedWasserstein(set_d: torch.Tensor, set_q: torch.Tensor, theta: torch.Tensor, grad1: bool = False, grad2: bool = False,
                      per_direction: bool = False) -> list[torch.Tensor | None]:
    """Sliced Wasserstein distance between paired clouds of equal size along ``theta[P,3]`` (extension,
    ``pcc_sliced_wasserstein``) -> [cost[B], cost_p[B,P] or None, grad1[B,N,3] or None, grad2[B,N,3] or None]: the
    gradients of ``cost`` (upstream gradient 1), each computed only when asked for."""
    if set_d.dim() != 3 or set_d.size(2) != 3 or set_q.shape != set_d.shape:
        raise ValueError(f'SlicedWasserstein: clouds must be [B,N,3] of one shape, got {tuple(set_d.shape)} and {tuple(set_q.shape)}')
    if theta.dim() != 2 or theta.size(1) != 3:
        raise ValueError(f'SlicedWasserstein: directions must be [P,3], got {tuple(theta.shape)}')
    b, n, p = set_d.size(0), set_d.size(1), theta.size(0)
    dev = set_d.device
    cost = torch.empty((b,), dtype=torch.float32, device=dev)
    cost_p = torch.empty((b, p), dtype=torch.float32, device=dev) if per_direction else None
    g1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if grad1 else None
    g2 = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if grad2 else None
    call(_L.pcc_sliced_wasserstein, 'SlicedWasserstein', dev, b, n, p, ptr(set_d, 'set_d', F32, dev), ptr(set_q, 'set_q', F32, dev),
         ptr(theta, 'directions', F32, dev), ptr(cost, 'cost', F32, dev), ptr(cost_p, 'cost_p', F32, dev),
         ptr(g1, 'grad1', F32, dev), ptr(g2, 'grad2', F32, dev))
    return [cost, cost_p, g1, g2]


def Sinkhorn(set_d: torch.Tensor, set_q: torch.Tensor, eps: list[float], debias: bool = True, grad1: bool = False,
             grad2: bool = False, potentials: bool = False) -> list[torch.Tensor | None]:
    """Sinkhorn divergence between paired clouds ``set_d[B,N,3]``, ``set_q[B,M,3]`` along the temperature schedule ``eps``
    (extension, ``pcc_sinkhorn``) -> [cost[B], pot1[B,N] or None, pot2[B,M] or None, grad1[B,N,3] or None, grad2[B,M,3] or
    None]: the gradients of ``cost`` (upstream gradient 1), each computed only when asked for."""
    if set_d.dim() != 3 or set_q.dim() != 3 or set_d.size(2) != 3 or set_q.size(2) != 3 or set_d.size(0) != set_q.size(0):
        raise ValueError(f'Sinkhorn: clouds must be [B,N,3] and [B,M,3], got {tuple(set_d.shape)} and {tuple(set_q.shape)}')
    b, n, m = _sizes(set_d, set_q)
    dev = set_d.device
    sched = (ctypes.c_float * len(eps))(*eps)  # read by the library before the call returns
    cost = torch.empty((b,), dtype=torch.float32, device=dev)
    p1 = torch.empty((b, n), dtype=torch.float32, device=dev) if potentials else None
    p2 = torch.empty((b, m), dtype=torch.float32, device=dev) if potentials else None
    g1 = torch.empty((b, n, 3), dtype=torch.float32, device=dev) if grad1 else None
    g2 = torch.empty((b, m, 3), dtype=torch.float32, device=dev) if grad2 else None
    call(_L.pcc_sinkhorn, 'Sinkhorn', dev, b, n, m, ptr(set_d, 'set_d', F32, dev), ptr(set_q, 'set_q', F32, dev), len(eps),
         ctypes.cast(sched, ctypes.c_void_p), int(bool(debias)), ptr(cost, 'cost', F32, dev), ptr(p1, 'pot1', F32, dev),
         ptr(p2, 'pot2', F32, dev), ptr(g1, 'grad1', F32, dev), ptr(g2, 'grad2', F32, dev))
    return [cost, p1, p2, g1, g2]
