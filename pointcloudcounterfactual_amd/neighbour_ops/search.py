# ---- squared distances (reference neighbour_ops.py:16-50) -----------------------------------------------------------------

from __future__ import annotations

from typing import Any

import torch

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import F32, I64, _L


def index_k_neighbours(pcs: list[Any], k: int) -> Any:
    """Host-side kNN precompute of the dataset readers (reference ``neighbour_ops.py:16-24``; ``modelnet.py:18``):
    a KD-tree per cloud, ``[len(pcs), N, k]``.  Dataset preparation, not on the device path."""
    import numpy as np
    from sklearn.neighbors import KDTree

    indices_list = []
    for pc in pcs:
        indices = KDTree(pc).query(pc, k, return_distance=False)
        indices_list.append(indices.reshape(-1, k))
    return np.stack(indices_list)


def pykeops_square_distance(t1: torch.Tensor, t2: torch.Tensor) -> Any:
    """Lazy ``D[b,i,j] = |t1[b,i] - t2[b,j]|^2`` (reference ``neighbour_ops.py:35-40``) over this package's
    ``LazyTensor`` (``keops_shim``): its reductions -- ``argmin`` / ``min`` over either axis, ``argKmin``, ``sum`` --
    run the HIP kernels; the matrix never exists.  Imported by ``metrics_and_losses.py:18`` and ``quantize.py:6``."""
    from pointcloudcounterfactual_amd.keops_shim import LazyTensor

    t1_lazy = LazyTensor(t1[:, :, None, :])
    t2_lazy = LazyTensor(t2[:, None, :, :])
    return ((t1_lazy - t2_lazy) ** 2).sum(-1)


def torch_square_distance(t1: torch.Tensor, t2: torch.Tensor) -> torch.Tensor:
    """Dense expanded-form ``[B,N,M]`` squared distances (reference ``neighbour_ops.py:43-50``): the reference's CPU
    path (``torch_chamfer``, ``metrics_and_losses.py:44-47``)."""
    from pointcloudcounterfactual_amd.losses import torch_square_distance as impl

    return impl(t1, t2)


def square_distance(t1: torch.Tensor, t2: torch.Tensor) -> Any:
    """Device dispatch of the reference (``neighbour_ops.py:27-32``): lazy on the accelerator, dense on the CPU."""
    if t1.device.type == 'cuda':
        return pykeops_square_distance(t1, t2)
    return torch_square_distance(t1, t2)


# ---- kNN ------------------------------------------------------------------------------------------------------


def self_square_distance(t1: torch.Tensor) -> torch.Tensor:
    """Expanded-form self distances (reference ``neighbour_ops.py:53-60``); CPU path of ``knn``."""
    t2 = t1.transpose(-1, -2)
    square_component = torch.sum(t1**2, -2, keepdim=True)
    dist = torch.tensor(-2) * torch.matmul(t2, t1)
    dist += square_component
    dist += square_component.transpose(-1, -2)
    return dist


def torch_knn(x: torch.Tensor, k: int) -> torch.Tensor:
    """Reference CPU kNN (``neighbour_ops.py:71-74``)."""
    return self_square_distance(x).topk(k=k, largest=False)[1]


def hip_knn(x: torch.Tensor, k: int) -> torch.Tensor:
    """``x[B,C,N] -> indices[B,N,k]`` int64, ascending distance, ties by ascending index (replaces ``pykeops_knn``).
    Any channel count C >= 1 and ``1 <= k <= min(N, 128)``."""
    x = x.contiguous()
    b, c, n = x.shape
    dev = x.device
    out = torch.empty((b, n, k), dtype=torch.int64, device=dev)
    call(_L.pcc_knn, 'knn', dev, b, c, n, k, ptr(x, 'x', F32, dev), ptr(out, 'indices', I64, dev))
    return out


def pykeops_knn(x: torch.Tensor, k: int) -> torch.Tensor:
    """The reference's accelerator kNN (``neighbour_ops.py:77-82``: ``argKmin`` of the lazy self distance), here the
    HIP search."""
    return hip_knn(x.detach(), k)


def knn(x: torch.Tensor, k: int) -> torch.Tensor:
    """Device dispatch of the reference (``neighbour_ops.py:63-68``)."""
    if x.device.type == 'cuda':
        return hip_knn(x.detach(), k)
    return torch_knn(x, k)


# ---- kNN between two clouds -------------------------------------------------------------------------------------


def cross_square_distance(q: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """Expanded-form distances ``[B,Nq,N]`` of the queries ``q[B,C,Nq]`` to the candidates ``x[B,C,N]``:
    ``self_square_distance`` written for two clouds; CPU path of ``knn_cross``."""
    dist = torch.tensor(-2) * torch.matmul(q.transpose(-1, -2), x)
    dist += torch.sum(x**2, -2, keepdim=True)
    dist += torch.sum(q**2, -2, keepdim=True).transpose(-1, -2)
    return dist


def torch_knn_cross(q: torch.Tensor, x: torch.Tensor, k: int, return_distance: bool = False) -> Any:
    """``torch_knn`` for two clouds: ``topk`` of the expanded-form distances."""
    dist, idx = cross_square_distance(q, x).topk(k=k, largest=False)
    return (idx, dist) if return_distance else idx


def hip_knn_cross(q: torch.Tensor, x: torch.Tensor, k: int, return_distance: bool = False) -> Any:
    """For every query of ``q[B,C,Nq]`` its ``k`` nearest candidates of ``x[B,C,N]``: ``indices[B,Nq,k]`` int64 into
    ``x``, ascending distance, ties by ascending index; with ``return_distance`` also their squared distances
    ``[B,Nq,k]`` float32 (``pcc_knn_cross``, include/pcc_neighbour.h).  Any channel count C >= 1, ``1 <= k <= min(N, 128)``;
    ``hip_knn_cross(x, x, k)`` is ``hip_knn(x, k)``.  The inputs are detached; the outputs are constants of the graph."""
    if q.dim() != 3 or x.dim() != 3 or q.shape[:2] != x.shape[:2]:
        raise ValueError(f'knn_cross: expected q[B,C,Nq] and x[B,C,N], got {tuple(q.shape)} and {tuple(x.shape)}')
    q, x = q.detach().contiguous(), x.detach().contiguous()
    b, c, nq = q.shape
    n = x.shape[2]
    dev = q.device
    qp, xp = ptr(q, 'q', F32, dev), ptr(x, 'x', F32, dev)  # (checked before anything is allocated on the device)
    out = torch.empty((b, nq, k), dtype=torch.int64, device=dev)
    dist = torch.empty((b, nq, k), dtype=torch.float32, device=dev) if return_distance else None
    call(_L.pcc_knn_cross, 'knn_cross', dev, b, c, nq, n, k, qp, xp, ptr(out, 'indices', I64, dev), ptr(dist, 'dist', F32, dev))
    return (out, dist) if return_distance else out


def knn_cross(q: torch.Tensor, x: torch.Tensor, k: int, return_distance: bool = False) -> Any:
    """k nearest candidates of ``x[B,C,N]`` for every query of ``q[B,C,Nq]`` (``knn`` for two clouds, same device
    dispatch): the HIP search on the accelerator, the torch formula for CPU tensors."""
    if q.device.type == 'cuda' or x.device.type == 'cuda':
        return hip_knn_cross(q, x, k, return_distance)
    return torch_knn_cross(q, x, k, return_distance)
