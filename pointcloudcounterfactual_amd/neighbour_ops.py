"""kNN-graph operations with the reference's Python API (``src/utils/neighbour_ops.py:63-133``).

On the accelerator every function runs hand-written HIP kernels through the C ABI
(``include/pcc_neighbour.h``); the reference uses PyKeOps there, which has no ROCm backend.  For CPU tensors the
functions follow the reference's own device dispatch (``neighbour_ops.py:29,65``) and evaluate its torch
formulas -- that is the reference's CPU path, not a fallback of the GPU path: an accelerator tensor never
leaves the device, and a missing HIP library is an ``ImportError``.

Layouts are the reference's: ``x[B,C,N]`` float32, ``indices[B,N,k]`` int64 (an empty ``indices`` tensor means
"compute the kNN now", ``:88-91``).
"""

from __future__ import annotations

import numbers
from typing import Any, Callable, NamedTuple

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd import _lib
from pointcloudcounterfactual_amd._float32 import fma32, sqrt32
from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.set_metrics import _grid_args

_L = _lib.lib
F32, I32, I64 = torch.float32, torch.int32, torch.int64


def _same_device(name: str, t: torch.Tensor, dev: torch.device) -> None:
    """``t`` is on ``dev``, or the ``RuntimeError`` of ``_lib.ptr``."""
    if t.device != dev:
        if dev.type == 'cuda' and t.device.type != 'cuda':
            raise RuntimeError(f'{name} must be a CUDA tensor')
        raise RuntimeError(f'{name} is on {t.device}, expected {dev}')


def _float32(name: str, t: torch.Tensor) -> None:
    """``t`` is float32, or the ``RuntimeError`` of ``_lib.ptr``."""
    if t.dtype != F32:
        raise RuntimeError(f'{name} must be {F32}, found {t.dtype}')


def _cloud_arg(what: str, name: str, xyz: torch.Tensor, b: int | None = None, min_n: int = 1, axis: str = 'N') -> tuple[int, int]:
    """``xyz[B,N,3]`` with ``N >= min_n`` (and the given ``B``), or the ``ValueError`` of ``what``: ``(b, n)``.  ``name`` and
    ``axis`` are what the message calls the tensor and its point axis."""
    if xyz.dim() != 3 or xyz.shape[2] != 3 or xyz.shape[1] < min_n or (b is not None and xyz.shape[0] != b):
        lay = f'{name}[B,{axis},3]' if b is None else f'{name}[B = {b},{axis},3]'
        raise ValueError(f'{what}: expected {lay}{f" with {axis} >= {min_n}" if min_n else ""}, got {tuple(xyz.shape)}')
    return xyz.shape[0], xyz.shape[1]


def _features_arg(what: str, features: torch.Tensor, name: str = 'features') -> tuple[int, int, int]:
    """``features[B,C,N]`` with ``C >= 1`` and ``N >= 1``, or the ``ValueError`` of ``what``: ``(b, c, n)``."""
    if features.dim() != 3 or features.shape[1] < 1 or features.shape[2] < 1:
        raise ValueError(f'{what}: expected {name}[B,C,N] with C >= 1 and N >= 1, got {tuple(features.shape)}')
    b, c, n = features.shape
    return b, c, n


def _list_arg(what: str, idx: torch.Tensor, b: int) -> tuple[int, int]:
    """The shape of an index list ``idx[B,M,k]`` with ``k >= 1`` and ``M * k < 2^31``, or the ``ValueError`` of ``what``:
    ``(m, k)``.  Its dtype and device are ``_list_on``'s: every caller checks other shapes in between."""
    if idx.dim() != 3 or idx.shape[0] != b or idx.shape[2] < 1:
        raise ValueError(f'{what}: expected idx[B = {b},M,k] with k >= 1, got {tuple(idx.shape)}')
    m, k = idx.shape[1], idx.shape[2]
    if m * k >= 1 << 31:
        raise ValueError(f'{what}: idx[B,M,k] with M * k >= 2^31, got {tuple(idx.shape)}')
    return m, k


def _list_on(idx: torch.Tensor, dev: torch.device) -> None:
    """``idx`` is int64 and on ``dev``, or the ``RuntimeError`` of ``_lib.ptr``."""
    if idx.dtype != I64:
        raise RuntimeError(f'idx must be {I64}, found {idx.dtype}')
    _same_device('idx', idx, dev)


def _k_arg(what: str, k: Any) -> None:
    """``k`` is an integer in ``[1, 128]`` (what ``knn`` and ``knn_cross`` search), or the ``ValueError`` of ``what``."""
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= 128:
        raise ValueError(f'{what}: k must be an integer in [1, 128], got {k!r}')


def _canonical_nan(t: torch.Tensor) -> torch.Tensor:
    """A NaN becomes the word 0x7fc00000."""
    return torch.where(torch.isnan(t), torch.full((), float('nan'), dtype=t.dtype, device=t.device), t)


# ---- squared distances (reference neighbour_ops.py:16-50) -----------------------------------------------------------------


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


# ---- farthest point sampling ---------------------------------------------------------------------------------------


def _fps_args(xyz: torch.Tensor, m: int, start: Any) -> tuple[torch.Tensor, int, torch.Tensor | None]:
    """The checks ``farthest_point_sample`` makes before anything runs: ``(xyz detached, m, start as a tensor or None)``."""
    b, n = _cloud_arg('farthest_point_sample', 'xyz', xyz, min_n=0)
    _float32('xyz', xyz)
    if isinstance(m, bool) or not isinstance(m, int) or m < 1 or m > n:
        raise ValueError(f'farthest_point_sample: m must be an int in [1, N = {n}], got {m!r}')
    if start is None or isinstance(start, torch.Tensor):
        if start is not None:
            if start.dim() != 1 or start.shape[0] != b or start.dtype not in (I32, I64, torch.int16, torch.int8, torch.uint8):
                raise ValueError(f'farthest_point_sample: start must be an int tensor [B = {b}], got {tuple(start.shape)} {start.dtype}')
            _same_device('start', start, xyz.device)
    elif isinstance(start, int) and not isinstance(start, bool):
        start = torch.full((b,), min(max(start, 0), n - 1), dtype=I32, device=xyz.device) if b else None
    else:
        raise ValueError(f'farthest_point_sample: start must be None, an int or an int tensor [B], got {type(start).__name__}')
    return xyz.detach(), m, start


def torch_farthest_point_sample(xyz: torch.Tensor, m: int, start: torch.Tensor | None, return_distance: bool = False) -> Any:
    """The rule of ``pcc_fps`` (include/pcc_neighbour.h) as a torch loop; CPU path of ``farthest_point_sample``."""
    b, n, _ = xyz.shape
    rows = torch.arange(b, device=xyz.device)
    # mind of an excluded point is -1: below every real minimum, and no distance is below it
    mind = torch.full((b, n), float('inf'), dtype=F32, device=xyz.device).masked_fill_(~torch.isfinite(xyz).all(-1), -1.0)
    idx = torch.zeros((b, m), dtype=I64, device=xyz.device)
    dist = torch.zeros((b, m), dtype=F32, device=xyz.device)
    sel = torch.zeros(b, dtype=I64, device=xyz.device) if start is None else start.to(I64).clamp(0, n - 1)
    for t in range(m):
        if t:
            sel = mind.argmax(1)  # (the first of equal maxima)
        idx[:, t] = sel
        at = mind[rows, sel]
        dist[:, t] = torch.where(at < 0, torch.full_like(at, float('nan')), at)
        df = xyz - xyz[rows, sel][:, None, :]
        d = df[..., 0] * df[..., 0]
        d = d + df[..., 1] * df[..., 1]
        d = d + df[..., 2] * df[..., 2]
        mind = torch.where(d < mind, d, mind)
    return (idx, dist) if return_distance else idx


def hip_farthest_point_sample(xyz: torch.Tensor, m: int, start: torch.Tensor | None, return_distance: bool = False) -> Any:
    """``pcc_fps`` on checked arguments (``_fps_args``)."""
    dev = xyz.device
    xyz = xyz.contiguous()
    b, n, _ = xyz.shape
    xp = ptr(xyz, 'xyz', F32, dev)  # (checked before anything is allocated on the device)
    if start is not None and start.dtype != I32:
        start = start.clamp(0, n - 1).to(I32)
    sp = ptr(None if start is None else start.contiguous(), 'start', I32, dev)
    idx = torch.empty((b, m), dtype=I64, device=dev)
    dist = torch.empty((b, m), dtype=F32, device=dev) if return_distance else None
    call(_L.pcc_fps, 'fps', dev, b, n, m, xp, sp, ptr(idx, 'idx', I64, dev), ptr(dist, 'dist', F32, dev))
    return (idx, dist) if return_distance else idx


def farthest_point_sample(xyz: torch.Tensor, m: int, start: Any = None, return_distance: bool = False) -> Any:
    """Farthest point sampling of ``xyz[B,N,3]`` float32: ``idx[B,m]`` int64, each entry the point farthest (squared
    distance, lowest index among equals) from the ones before it, starting from ``start`` (``None``: point 0; an int; an int
    tensor ``[B]``; clamped into ``[0, N-1]``).  With ``return_distance`` also ``dist[B,m]`` float32: the squared distance
    of each selected point to the ones selected before it (``dist[:,0] = inf``), i.e. the squared coverage radius after
    ``t`` picks.  Points with a non-finite coordinate are never selected while another point is left.  The full contract is
    ``pcc_fps``'s (include/pcc_neighbour.h); ``1 <= m <= N``.  The HIP kernel on the accelerator (one workgroup per
    cloud), the same rule as a torch loop for CPU tensors.  The inputs are detached; the outputs are constants of the graph."""
    xyz, m, start = _fps_args(xyz, m, start)
    if xyz.device.type == 'cuda':
        return hip_farthest_point_sample(xyz, m, start, return_distance)
    return torch_farthest_point_sample(xyz, m, start, return_distance)


# ---- ball query -------------------------------------------------------------------------------------------------------

BALL_PAD = {'first': 0, 'none': 1}  # PCC_BALL_PAD_FIRST / PCC_BALL_PAD_NONE (include/pcc_neighbour.h)


def _ball_args(xyz: torch.Tensor, centres: torch.Tensor, radius: Any, nsample: int, pad: str) -> tuple[torch.Tensor, torch.Tensor, float, int]:
    """The checks ``ball_query`` makes before anything runs: ``(xyz detached, centres detached, radius as the float32 the
    library receives, pad as the C constant)``."""
    b, _ = _cloud_arg('ball_query', 'xyz', xyz)
    _cloud_arg('ball_query', 'centres', centres, b, min_n=0, axis='M')
    _float32('xyz', xyz)
    _float32('centres', centres)
    _same_device('centres', centres, xyz.device)
    if isinstance(nsample, bool) or not isinstance(nsample, int) or nsample < 1:
        raise ValueError(f'ball_query: nsample must be an int >= 1, got {nsample!r}')
    if isinstance(radius, bool) or not isinstance(radius, numbers.Real):
        raise ValueError(f'ball_query: radius must be a real number > 0, got {radius!r}')
    r32 = torch.tensor(float(radius), dtype=F32).item()  # (what the C ABI's float parameter receives)
    if not r32 > 0:
        raise ValueError(f'ball_query: radius must be > 0 (as a float32), got {radius!r}')
    if not isinstance(pad, str) or pad not in BALL_PAD:
        raise ValueError(f"ball_query: pad must be 'first' or 'none', got {pad!r}")
    return xyz.detach(), centres.detach(), r32, BALL_PAD[pad]


def torch_ball_query(xyz: torch.Tensor, centres: torch.Tensor, radius: float, nsample: int, pad: int = 0,
                     return_count: bool = False) -> Any:
    """The rule of ``pcc_ball_query`` (include/pcc_neighbour.h) in torch, roundings included (``fma32`` is the kernel's
    ``fmaf``); CPU path of ``ball_query``.  ``pad`` is the C constant."""
    b, n, _ = xyz.shape
    m = centres.shape[1]
    dev = xyz.device
    r32 = torch.tensor(radius, dtype=F32, device=dev)
    r2 = r32 * r32  # one float32 multiplication
    idx = torch.zeros((b, m, nsample), dtype=I64, device=dev)
    cnt = torch.zeros((b, m), dtype=I32, device=dev)
    step = max(1, (1 << 21) // max(1, b * n))  # queries per block: about 2M distances at a time
    for m0 in range(0, m, step):
        df = xyz[:, None, :, :] - centres[:, m0:m0 + step, None, :]
        d = df[..., 0] * df[..., 0]
        d = fma32(df[..., 1], df[..., 1], d)
        d = fma32(df[..., 2], df[..., 2], d)
        inside = d < r2  # (false for a NaN distance)
        rank = inside.cumsum(-1)
        bb, ii, jj = (inside & (rank <= nsample)).nonzero(as_tuple=True)
        idx[bb, m0 + ii, rank[bb, ii, jj] - 1] = jj  # (ascending j along a row)
        cnt[:, m0:m0 + step] = rank[..., -1].clamp(max=nsample).to(I32)
    fill = idx[..., :1] if pad == BALL_PAD['first'] else torch.full((b, m, 1), -1, dtype=I64, device=dev)
    idx = torch.where(torch.arange(nsample, device=dev) < cnt[..., None], idx, fill)
    return (idx, cnt) if return_count else idx


def hip_ball_query(xyz: torch.Tensor, centres: torch.Tensor, radius: float, nsample: int, pad: int = 0,
                   return_count: bool = False) -> Any:
    """``pcc_ball_query`` on checked arguments (``_ball_args``)."""
    dev = xyz.device
    xyz, centres = xyz.contiguous(), centres.contiguous()
    b, n, _ = xyz.shape
    m = centres.shape[1]
    xp, cp = ptr(xyz, 'xyz', F32, dev), ptr(centres, 'centres', F32, dev)  # (checked before anything is allocated on the device)
    idx = torch.empty((b, m, nsample), dtype=I64, device=dev)
    cnt = torch.empty((b, m), dtype=I32, device=dev) if return_count else None
    call(_L.pcc_ball_query, 'ball_query', dev, b, n, m, nsample, radius, pad, xp, cp, ptr(idx, 'idx', I64, dev),
         ptr(cnt, 'cnt', I32, dev))
    return (idx, cnt) if return_count else idx


def ball_query(xyz: torch.Tensor, centres: torch.Tensor, radius: float, nsample: int, pad: str = 'first',
               return_count: bool = False) -> Any:
    """For every centre of ``centres[B,M,3]`` the first ``nsample`` points (ascending index) of ``xyz[B,N,3]`` strictly
    inside the ball of ``radius`` around it: ``idx[B,M,nsample]`` int64 into ``xyz`` and, with ``return_count``,
    ``cnt[B,M]`` int32 = min(points inside, nsample).  Slots past ``cnt`` repeat the row's first index (``pad='first'``;
    index 0 for an empty ball: every slot can be gathered without a mask) or hold -1 (``pad='none'``).  Both tensors are
    float32; ``centres`` may be ``xyz``.  The full contract is ``pcc_ball_query``'s (include/pcc_neighbour.h).  The HIP
    kernel on the accelerator (one wave per centre, stops as soon as the row is full), the same float32 rule in torch for
    CPU tensors: the two agree word for word.  The inputs are detached; the outputs are constants of the graph."""
    xyz, centres, radius, pad_c = _ball_args(xyz, centres, radius, nsample, pad)
    if xyz.device.type == 'cuda':
        return hip_ball_query(xyz, centres, radius, nsample, pad_c, return_count)
    return torch_ball_query(xyz, centres, radius, nsample, pad_c, return_count)


# ---- grouping along a list of another point set ------------------------------------------------------------------------


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
    valid = (idx >= 0) & (idx < n)
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    out = torch.gather(xc, 2, safe.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)
    if centres is not None:
        out = out - (centres.transpose(1, 2) if point_major else centres)[:, :, :, None]
    return torch.where(valid[:, None], out, torch.zeros((), dtype=out.dtype, device=out.device))


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
    idx, cnt = ball_query(xyz, centres, radius, nsample, pad=pad, return_count=True)
    if xyz.device.type == 'cuda':
        parts = (xyz, centres, True) + (() if features is None else (features, None, False))
        grouped = Grouped.apply(idx, *parts)
    else:
        grouped = torch_group_points(xyz, idx, centres, True)
        if features is not None:
            grouped = torch.cat((grouped, torch_group_points(features, idx)), 1)
    return SampleAndGroup(centres, grouped, idx, cnt, sel)


# ---- feature propagation: weighted interpolation along a list of another point set ----------------------------------------


def interpolation_weights(dist: torch.Tensor, eps: float = 1e-8) -> torch.Tensor:
    """Inverse-distance weights ``w[B,M,k]`` of the squared distances ``dist[B,M,k]`` that ``knn_cross(...,
    return_distance=True)`` returns: ``r = 1 / (dist + eps)``, ``r = 0`` where ``dist`` is NaN (the padded slot of a list that
    ran short), ``w = r / sum_k r``, and all zeros where that sum is 0 (a row of padded slots only).  Plain torch on either
    device, differentiable in ``dist``."""
    if dist.dim() != 3 or not dist.is_floating_point():
        raise ValueError(f'interpolation_weights: expected floating-point dist[B,M,k], got {tuple(dist.shape)} {dist.dtype}')
    pad = torch.isnan(dist)
    zero = torch.zeros((), dtype=dist.dtype, device=dist.device)
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
        col = idx[:, :, j]
        valid = (col >= 0) & (col < n)
        safe = torch.where(valid, col, torch.zeros_like(col))
        wj = torch.where(valid, weights[:, :, j], torch.zeros((), dtype=weights.dtype, device=weights.device))
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


# ---- vector attention: a softmax over the valid slots of a list, a grouped weighted sum of gathered values ------------------

MAX_LIST_K = 128  # the longest row the searches return


def _attn_args(what: str, x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, rel: torch.Tensor | None,
               wname: str = 'weights') -> tuple[int, int, int, int, int, int]:
    """The checks ``aggregate_points`` / ``attention_aggregate`` make before anything runs: ``(b, c, g, n, m, k)``."""
    b, c, n = _features_arg(what, x, 'x')
    m, k = _list_arg(what, idx, b)
    if weights.dim() != 4 or weights.shape[1] < 1 or tuple(weights.shape) != (b, weights.shape[1], m, k):
        raise ValueError(f'{what}: expected {wname}[B = {b},G,M = {m},k = {k}] with G >= 1, got {tuple(weights.shape)}')
    g = weights.shape[1]
    if c % g:
        raise ValueError(f'{what}: the G = {g} groups of {wname} do not divide the C = {c} channels of x')
    if rel is not None and tuple(rel.shape) != (b, c, m, k):
        raise ValueError(f'{what}: expected rel[B,C,M,k] = {(b, c, m, k)}, got {tuple(rel.shape)}')
    if k > MAX_LIST_K:
        raise ValueError(f'{what}: k must be <= {MAX_LIST_K}, got {k}')
    _float32('x', x)
    _list_on(idx, x.device)
    _float32(wname, weights)
    _same_device(wname, weights, x.device)
    if rel is not None:
        _float32('rel', rel)
        _same_device('rel', rel, x.device)
    return b, c, g, n, m, k


def _softmax_args(logits: torch.Tensor, idx: torch.Tensor, n: Any, what: str = 'neighbour_softmax') -> tuple[int, int, int, int]:
    """The checks ``neighbour_softmax`` makes before anything runs: ``(b, g, m, k)``."""
    if logits.dim() != 4 or logits.shape[1] < 1:
        raise ValueError(f'{what}: expected logits[B,G,M,k] with G >= 1, got {tuple(logits.shape)}')
    b, g = logits.shape[:2]
    m, k = _list_arg(what, idx, b)
    if tuple(logits.shape) != (b, g, m, k):
        raise ValueError(f'{what}: expected logits[B,G,M,k] = {(b, g, m, k)}, got {tuple(logits.shape)}')
    if k > MAX_LIST_K:
        raise ValueError(f'{what}: k must be <= {MAX_LIST_K}, got {k}')
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f'{what}: n must be an integer >= 1, got {n!r}')
    _float32('logits', logits)
    _list_on(idx, logits.device)
    return b, g, m, k


def _zero(t: torch.Tensor) -> torch.Tensor:
    return torch.zeros((), dtype=t.dtype, device=t.device)


def _slot_values(x: torch.Tensor, idx: torch.Tensor, valid: torch.Tensor, rel: torch.Tensor | None) -> torch.Tensor:
    """``v[B,C,M,k] = x[b,ch,idx] (+ rel)``, index 0 standing in for a slot that is no point."""
    b, c, _ = x.shape
    m, k = idx.shape[1:]
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    v = torch.gather(x, 2, safe.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)
    return v if rel is None else v + rel


def torch_neighbour_softmax(logits: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    """The rule of ``pcc_neighbour_softmax`` in float32 torch operations (no autograd): the maximum over the valid slots,
    ``exp`` of the rounded difference, the sum over the valid slots in slot order, one division."""
    valid = ((idx >= 0) & (idx < n))[:, None]  # [B,1,M,k]
    mx = torch.where(valid, logits, torch.full((), float('-inf'), dtype=logits.dtype, device=logits.device)).amax(-1, keepdim=True)
    e = torch.where(valid, torch.exp(logits - mx), _zero(logits))
    s = torch.zeros_like(e[..., 0])
    for j in range(idx.shape[2]):
        s = torch.where(valid[..., j], s + e[..., j], s)
    return torch.where(valid, _canonical_nan(e / s[..., None]), _zero(logits))


def torch_neighbour_softmax_bwd(attn: torch.Tensor, idx: torch.Tensor, n: int, grad_attn: torch.Tensor) -> torch.Tensor:
    """The rule of ``pcc_neighbour_softmax_bwd``: ``d`` summed over the valid slots in slot order, ``attn * (ga - d)``."""
    valid = ((idx >= 0) & (idx < n))[:, None]
    d = torch.zeros_like(attn[..., 0])
    for j in range(idx.shape[2]):
        d = torch.where(valid[..., j], d + attn[..., j] * grad_attn[..., j], d)
    return torch.where(valid, _canonical_nan(attn * (grad_attn - d[..., None])), _zero(attn))


def torch_aggregate_points(x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, rel: torch.Tensor | None = None) -> torch.Tensor:
    """The rule of ``pcc_aggregate_points`` in float32 torch operations (no autograd): per slot a gather, the sum with
    ``rel``, a product and an addition, in slot order."""
    b, c, n = x.shape
    s = c // weights.shape[1]
    valid = (idx >= 0) & (idx < n)
    v = _slot_values(x, idx, valid, rel)
    out = torch.zeros((b, c, idx.shape[1]), dtype=x.dtype, device=x.device)
    for j in range(idx.shape[2]):
        term = weights[..., j].repeat_interleave(s, dim=1) * v[..., j]
        out = torch.where(valid[:, None, :, j], out + term, out)
    return _canonical_nan(out)


def torch_aggregate_points_bwd(x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, rel: torch.Tensor | None,
                               grad_out: torch.Tensor, want: tuple[bool, bool, bool]) -> tuple[Any, Any, Any]:
    """The rule of ``pcc_aggregate_points_bwd``: ``(grad_x, grad_w, grad_rel)``, None where ``want`` is false."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    g = weights.shape[1]
    s = c // g
    valid = (idx >= 0) & (idx < n)
    gx = gw = gr = None
    if want[0] or want[2]:
        prod = torch.where(valid[:, None], weights.repeat_interleave(s, dim=1) * grad_out[..., None], _zero(x))
        if want[2]:
            gr = _canonical_nan(prod)
        if want[0]:
            safe = torch.where(valid, idx, torch.zeros_like(idx))
            gx = torch.zeros_like(x).scatter_add_(2, safe.reshape(b, 1, m * k).expand(-1, c, -1), prod.reshape(b, c, m * k))
    if want[1]:
        v = _slot_values(x, idx, valid, rel).view(b, g, s, m, k)
        go = grad_out.view(b, g, s, m)
        acc = torch.zeros((b, g, m, k), dtype=x.dtype, device=x.device)
        for ch in range(s):
            acc = acc + go[:, :, ch, :, None] * v[:, :, ch]
        gw = torch.where(valid[:, None], _canonical_nan(acc), _zero(x))
    return gx, gw, gr


class NeighbourSoftmax(Function):
    """``NeighbourSoftmax.apply(logits, idx, n)``: ``pcc_neighbour_softmax`` and, on the saved ``attn``,
    ``pcc_neighbour_softmax_bwd``; for CPU tensors the same rules in torch.  The arguments have passed ``_softmax_args``."""

    @staticmethod
    def forward(ctx: Any, logits: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
        logits, idx = logits.contiguous(), idx.contiguous()
        b, g, m, k = logits.shape
        dev = logits.device
        if dev.type == 'cuda':
            lp, ip = ptr(logits, 'logits', F32, dev), ptr(idx, 'idx', I64, dev)  # (checked before anything is allocated)
            attn = torch.empty_like(logits)
            call(_L.pcc_neighbour_softmax, 'neighbour_softmax', dev, b, g, n, m, k, ip, lp, ptr(attn, 'attn', F32, dev))
        else:
            attn = torch_neighbour_softmax(logits, idx, n)
        ctx.save_for_backward(idx, attn)
        ctx.n = n
        return attn

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, ...]:
        idx, attn = ctx.saved_tensors
        b, g, m, k = attn.shape
        grad = grad.contiguous()
        dev = grad.device
        if dev.type != 'cuda':
            return torch_neighbour_softmax_bwd(attn, idx, ctx.n, grad), None, None
        gl = torch.empty_like(attn)
        call(_L.pcc_neighbour_softmax_bwd, 'neighbour_softmax_bwd', dev, b, g, ctx.n, m, k, ptr(idx, 'idx', I64, dev),
             ptr(attn, 'attn', F32, dev), ptr(grad, 'grad', F32, dev), ptr(gl, 'grad_logits', F32, dev))
        return gl, None, None


class AggregatedPoints(Function):
    """``AggregatedPoints.apply(x, idx, weights, rel or None)``: ``pcc_aggregate_points`` and ``pcc_aggregate_points_bwd``,
    which computes the gradients that are asked for only; for CPU tensors the same rules in torch.  Differentiable in ``x``,
    ``weights`` and ``rel``.  The arguments have passed ``_attn_args``."""

    @staticmethod
    def forward(ctx: Any, x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, rel: torch.Tensor | None) -> torch.Tensor:
        x, idx, weights = x.contiguous(), idx.contiguous(), weights.contiguous()
        rel = None if rel is None else rel.contiguous()
        b, c, n = x.shape
        g, m, k = weights.shape[1:]
        dev = x.device
        if dev.type == 'cuda':
            # (checked before anything is allocated on the device)
            xp, ip, wp, rp = ptr(x, 'x', F32, dev), ptr(idx, 'idx', I64, dev), ptr(weights, 'weights', F32, dev), ptr(rel, 'rel', F32, dev)
            out = torch.empty((b, c, m), dtype=F32, device=dev)
            call(_L.pcc_aggregate_points, 'aggregate_points', dev, b, c, g, n, m, k, xp, ip, wp, rp, ptr(out, 'out', F32, dev))
        else:
            out = torch_aggregate_points(x, idx, weights, rel)
        ctx.save_for_backward(x, idx, weights, *(() if rel is None else (rel,)))
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, ...]:
        x, idx, weights, *rest = ctx.saved_tensors
        rel = rest[0] if rest else None
        b, c, n = x.shape
        g, m, k = weights.shape[1:]
        grad = grad.contiguous()
        dev = grad.device
        want = (ctx.needs_input_grad[0], ctx.needs_input_grad[2], rel is not None and ctx.needs_input_grad[3])
        if dev.type != 'cuda':
            gx, gw, gr = torch_aggregate_points_bwd(x, idx, weights, rel, grad, want)
            return gx, None, gw, gr
        gx = torch.empty((b, c, n), dtype=F32, device=dev) if want[0] else None
        gw = torch.empty((b, g, m, k), dtype=F32, device=dev) if want[1] else None
        gr = torch.empty((b, c, m, k), dtype=F32, device=dev) if want[2] else None
        if any(want):
            call(_L.pcc_aggregate_points_bwd, 'aggregate_points_bwd', dev, b, c, g, n, m, k, ptr(x, 'x', F32, dev),
                 ptr(idx, 'idx', I64, dev), ptr(weights, 'weights', F32, dev), ptr(rel, 'rel', F32, dev), ptr(grad, 'grad', F32, dev),
                 ptr(gx, 'grad_x', F32, dev), ptr(gw, 'grad_weights', F32, dev), ptr(gr, 'grad_rel', F32, dev))
        return gx, None, gw, gr


def neighbour_softmax(logits: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    """``attn[B,G,M,k]``: the softmax of ``logits[B,G,M,k]`` float32 over the k slots of every row, restricted to the slots of
    ``idx[B,M,k]`` int64 that name one of the ``n`` points: a slot outside ``[0, n)`` (the -1 of ``ball_query(pad='none')``)
    takes no part, carries no gradient and is +0; a row without a valid slot is all +0.  Non-finite logits behave as
    ``torch.softmax`` over the valid slots.  The sum runs over the slots in order, so the words do not depend on the batch;
    differentiable in ``logits``.  The full contract is ``pcc_neighbour_softmax``'s (include/pcc_neighbour.h).  The HIP kernels
    on the accelerator, the same rule in torch for CPU tensors."""
    _softmax_args(logits, idx, n)
    return NeighbourSoftmax.apply(logits, idx.detach(), int(n))


def aggregate_points(x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, rel: torch.Tensor | None = None) -> torch.Tensor:
    """``out[B,C,M]``: ``out[b,ch,i] = sum_j weights[b,ch // S,i,j] * (x[b,ch,idx[b,i,j]] + rel[b,ch,i,j])`` with ``x[B,C,N]``,
    ``idx[B,M,k]`` int64, ``weights[B,G,M,k]`` (G divides C, ``S = C // G`` consecutive channels share a weight) and the
    optional position encoding ``rel[B,C,M,k]`` (the layout of ``group_points``): the grouped vector attention of Point
    Transformer, the values gathered inside the kernel.  In float32 slot by slot: a rounded sum with ``rel``, a rounded
    product, a rounded addition.  A slot whose index is outside ``[0, N)`` adds nothing and carries no gradient.  All
    float32; differentiable in ``x``, ``weights`` and ``rel``, and only the gradients that are required are computed.  The
    full contract is ``pcc_aggregate_points``'s (include/pcc_neighbour.h).  The HIP kernels on the accelerator, the same rule
    in torch for CPU tensors: the forwards, ``grad_weights`` and ``grad_rel`` agree word for word."""
    _attn_args('aggregate_points', x, idx, weights, rel)
    return AggregatedPoints.apply(x, idx.detach(), weights, rel)


def attention_aggregate(x: torch.Tensor, idx: torch.Tensor, logits: torch.Tensor, rel: torch.Tensor | None = None,
                        return_attention: bool = False) -> Any:
    """``aggregate_points(x, idx, neighbour_softmax(logits, idx, N), rel)``: one attention read-out, ``out[B,C,M]`` (and
    ``attn[B,G,M,k]`` with ``return_attention``).  Differentiable in ``x``, ``logits`` and ``rel``; ``attn`` is the one
    ``[B,G,M,k]`` tensor kept for the backward (beside the inputs), and only the gradients that are required are computed."""
    _attn_args('attention_aggregate', x, idx, logits, rel, 'logits')
    idx = idx.detach()
    attn = NeighbourSoftmax.apply(logits, idx, x.shape[2])
    out = AggregatedPoints.apply(x, idx, attn, rel)
    return (out, attn) if return_attention else out


def vector_attention(xyz_q: torch.Tensor, xyz: torch.Tensor, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                     idx: torch.Tensor, pos_net: Callable[[torch.Tensor], torch.Tensor],
                     attn_net: Callable[[torch.Tensor], torch.Tensor]) -> torch.Tensor:
    """The data flow of one vector-attention layer (Point Transformer) along ``idx[B,M,k]``, a list of the M query points
    ``xyz_q[B,M,3]`` into the N points ``xyz[B,N,3]``: ``delta = pos_net(relative coordinates [B,3,M,k])`` gives the position
    encoding ``[B,C,M,k]``; ``logits = attn_net(delta - (key_j - query_i))`` gives ``[B,G,M,k]`` from ``key[B,C',N]`` and
    ``query[B,C',M]``; the result is ``attention_aggregate(value[B,C,N], idx, logits, rel=delta)``: ``[B,C,M]``.  ``pos_net``
    and ``attn_net`` are the caller's modules (1x1 ``Conv2d`` stacks read this layout); G divides C."""
    p = group_points(xyz, idx, centres=xyz_q, point_major=True)
    delta = pos_net(p)
    t = delta - group_points(key, idx, centres=query)
    return attention_aggregate(value, idx, attn_net(t), rel=delta)


# ---- kernel point convolution: influences of kernel points on the neighbours, a weighted sum per kernel point ---------------

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
    valid = (idx >= 0) & (idx < n)
    safe = torch.where(valid, idx, torch.zeros_like(idx))
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
    v = _slot_values(x, idx, (idx >= 0) & (idx < n), None)
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
    valid = (idx >= 0) & (idx < n)
    safe = torch.where(valid, idx, torch.zeros_like(idx))
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


# ---- the point-voxel branch: features averaged into a dense grid, a grid read back at the points --------------------------

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
    safe = torch.where(finite[:, :, None], xyz, torch.zeros((), dtype=xyz.dtype))
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
    rank = pos - torch.cummax(torch.where(is_start, pos, torch.zeros((), dtype=I64)), 1).values
    valid = sorted_cell >= 0
    acc = torch.zeros((b, c, bins), dtype=features.dtype)
    channels = torch.arange(c)[None, :]
    for r in range(int(rank[valid].max().item()) + 1 if valid.any() else 0):
        bi, si = (valid & (rank == r)).nonzero(as_tuple=True)
        at = (bi[:, None], channels, sorted_cell[bi, si][:, None])
        acc = acc.index_put(at, acc[at] + features[bi[:, None], channels, order[bi, si][:, None]])
    counts = index.counts.reshape(b, 1, bins)
    grid = torch.where(counts > 0, acc / torch.where(counts > 0, counts, torch.ones((), dtype=I32)).to(features.dtype),
                       torch.zeros((), dtype=features.dtype))
    return _canonical_nan(grid).view(b, c, res, res, res)


def _trilinear(xyz: torch.Tensor, res: int, lo32: torch.Tensor, inv: torch.Tensor) -> tuple[torch.Tensor, list[torch.Tensor], list[torch.Tensor]]:
    """``pcc_devoxelize``'s corners of the points ``xyz[B,N,3]`` (constants of the graph): ``finite[B,N]``, and for the
    corners 000, 001, 010, ... 111 the flat cells ``[B,N]`` int64 and the weights ``(wx * wy) * wz`` ``[B,N]``."""
    xyz = xyz.detach()
    finite = torch.isfinite(xyz).all(2)
    safe = torch.where(finite[:, :, None], xyz, torch.zeros((), dtype=xyz.dtype, device=xyz.device))
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
    out = torch.where(finite[:, None, :], out, torch.zeros((), dtype=grid.dtype, device=grid.device))
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
    if isinstance(index_or_xyz, VoxelIndex):
        index = index_or_xyz
        res = _voxel_index_args(index, what, b, n, dev)
        if resolution is not None and resolution != res:
            raise ValueError(f'{what}: resolution {resolution!r} is not the index\'s ({res})')
    elif isinstance(index_or_xyz, torch.Tensor):
        _voxel_cloud_args(index_or_xyz, what, b, n)
        _same_device('xyz', index_or_xyz, dev)
        if resolution is None:
            raise ValueError(f'{what}: resolution is needed with a cloud')
        index = voxel_index(index_or_xyz, resolution, lo, extent)
        res = resolution
    else:
        raise ValueError(f'{what}: expected a VoxelIndex or xyz[B,N,3], got {type(index_or_xyz).__name__}')
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


# ---- grid pooling: one slot per occupied cell of the voxel grid (PTv2's partition-based pooling, KPConv's grid subsampling) ----

_REDUCE = {'mean': 0, 'sum': 1, 'max': 2}  # pcc_segment_pool's modes


class GridIndex(NamedTuple):
    """What ``grid_cluster`` returns: the partition of a cloud into the occupied cells of a grid, padded to ``m`` slots."""

    cluster: torch.Tensor  # [B,N] int32 slot of every point: the rank of its cell among the occupied ones, -1 if dropped or non-finite
    seg: torch.Tensor      # [B,m+1] int32: the points of slot r are order[seg[r] : seg[r + 1]]; a padded slot's run is empty
    count: torch.Tensor    # [B] int32 occupied cells of the cloud (count > m: cells were dropped)
    order: torch.Tensor    # [B,N] int32 the permutation of the VoxelIndex


class GridPooled(NamedTuple):
    """What ``grid_pool`` returns."""

    xyz: torch.Tensor              # [B,m,3] mean coordinate of every slot's points, NaN in a padded slot
    features: torch.Tensor | None  # [B,C,m] pooled features, +0 in a padded slot
    index: GridIndex
    count: torch.Tensor            # [B] int32, index.count


def _grid_pool_size_args(what: str, b: int, n: int) -> None:
    """The size limits of the three entry points (include/pcc_neighbour.h)."""
    if b > 65535 or b * (n + 1) >= 1 << 31:
        raise ValueError(f'{what}: too large (B <= 65535, B * (N + 1) < 2^31), got B = {b}, N = {n}')


def _capacity_arg(what: str, m: Any, n: int) -> None:
    if isinstance(m, bool) or not isinstance(m, numbers.Integral) or not 1 <= m <= n:
        raise ValueError(f'{what}: m must be None or an integer in [1, N = {n}], got {m!r}')


def _reduce_arg(what: str, reduce: Any) -> int:
    if not isinstance(reduce, str) or reduce not in _REDUCE:
        raise ValueError(f"{what}: reduce must be 'mean', 'sum' or 'max', got {reduce!r}")
    return _REDUCE[reduce]


def _grid_index_args(gindex: Any, what: str, b: int, n: int, dev: torch.device) -> int:
    """``gindex`` is a ``GridIndex`` of ``b`` clouds of ``n`` points on ``dev``: its capacity ``m``."""
    if not isinstance(gindex, GridIndex):
        raise ValueError(f'{what}: expected a GridIndex, got {type(gindex).__name__}')
    cluster, seg, count, order = gindex
    if tuple(cluster.shape) != (b, n) or tuple(order.shape) != (b, n):
        raise ValueError(f'{what}: expected index.cluster and index.order [B,N] = {(b, n)}, got {tuple(cluster.shape)} and {tuple(order.shape)}')
    if seg.dim() != 2 or seg.shape[0] != b or not 2 <= seg.shape[1] <= n + 1:
        raise ValueError(f'{what}: expected index.seg[B = {b},m + 1] with 1 <= m <= N = {n}, got {tuple(seg.shape)}')
    if tuple(count.shape) != (b,):
        raise ValueError(f'{what}: expected index.count[B = {b}], got {tuple(count.shape)}')
    for name, t in (('index.cluster', cluster), ('index.seg', seg), ('index.count', count), ('index.order', order)):
        if t.dtype != I32:
            raise RuntimeError(f'{name} must be {I32}, found {t.dtype}')
        _same_device(name, t, dev)
    return seg.shape[1] - 1


def torch_grid_cluster(index: VoxelIndex, m: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The rule of ``pcc_grid_cluster`` in torch: ``(cluster[B,N], seg[B,m+1], count[B])`` int32.  Integers only, so every
    word is the kernel's."""
    b, n = index.cell.shape
    order = index.order.to(I64)
    sorted_cell = torch.gather(index.cell.to(I64), 1, order)
    valid = sorted_cell >= 0
    is_start = valid.clone()
    is_start[:, 1:] &= sorted_cell[:, 1:] != sorted_cell[:, :-1]
    rank = torch.cumsum(is_start.to(I64), 1) - 1  # of the cell of every sorted position
    count, finite = is_start.sum(1), valid.sum(1)
    cluster = torch.empty((b, n), dtype=I64)
    cluster.scatter_(1, order, torch.where(valid & (rank < m), rank, torch.full((), -1, dtype=I64)))
    # starts[r]: the first position of rank r, F behind the last rank; its first m + 1 entries are seg at capacity m
    pos = torch.arange(n)[None, :].expand(b, n)
    starts = finite[:, None].expand(b, n + 1).clone()
    starts.scatter_(1, torch.where(is_start, rank, torch.full((), n, dtype=I64)), torch.where(is_start, pos, finite[:, None].expand(b, n)))
    return cluster.to(I32), starts[:, :m + 1].to(I32).contiguous(), count.to(I32)


def torch_segment_pool(features: torch.Tensor, order: torch.Tensor, seg: torch.Tensor, mode: int) -> tuple[torch.Tensor, torch.Tensor | None]:
    """The rule of ``pcc_segment_pool`` in torch: ``(out[B,C,m], arg[B,C,m] int32 or None)``.  One pass per rank within the
    run -- a pass touches every slot at most once, so every slot chains its points in ascending position --, the slots
    ordered by the length of their runs so that a pass visits only those it still has a point for."""
    b, c, n = features.shape
    m = seg.shape[1] - 1
    features = features.detach()
    seg64, order64 = seg.to(I64), order.to(I64)
    start = seg64[:, :-1].clamp(0, n)
    length = (seg64[:, 1:].clamp(0, n) - start).clamp(min=0)  # [B,m]
    out = torch.zeros((b, c, m), dtype=features.dtype)
    arg = torch.full((b, c, m), -1, dtype=I64) if mode == 2 else None
    flat_len = length.reshape(-1)
    by_len = torch.argsort(flat_len, descending=True, stable=True)
    bi_all, ri_all = by_len // m, by_len % m
    longest = int(flat_len.max()) if flat_len.numel() else 0
    longer = flat_len.numel() - torch.cumsum(torch.bincount(flat_len, minlength=longest + 1), 0)  # [j]: slots with len > j
    for j, live in enumerate(longer[:longest].tolist()):
        bi, ri = bi_all[:live], ri_all[:live]
        p = order64[bi, start[bi, ri] + j]
        v = features[bi, :, p]  # [live, C]
        cur = out[bi, :, ri]
        if mode == 2:
            at = arg[bi, :, ri]
            take = (at < 0) | (~torch.isnan(cur) & (torch.isnan(v) | (v > cur)))
            out[bi, :, ri] = torch.where(take, v, cur)
            arg[bi, :, ri] = torch.where(take, p[:, None], at)
        else:
            out[bi, :, ri] = cur + v
    if mode == 0:
        some = (length > 0)[:, None, :]
        out = torch.where(some, out / torch.where(some, length[:, None, :], torch.ones((), dtype=I64)).to(features.dtype),
                          torch.zeros((), dtype=features.dtype))
    return (out, arg.to(I32)) if mode == 2 else (_canonical_nan(out), None)


def torch_segment_pool_bwd(grad: torch.Tensor, cluster: torch.Tensor, seg: torch.Tensor, arg: torch.Tensor | None, mode: int) -> torch.Tensor:
    """The rule of ``pcc_segment_pool_bwd`` in torch: a gather along ``cluster``, ``[B,C,N]``."""
    b, c, m = grad.shape
    n = cluster.shape[1]
    slot = cluster.to(I64)
    ok = (slot >= 0) & (slot < m)
    at = torch.where(ok, slot, torch.zeros((), dtype=I64))[:, None, :].expand(b, c, n)
    g = torch.gather(grad, 2, at)
    if mode == 0:
        seg64 = seg.to(I64)
        length = torch.gather(seg64[:, 1:] - seg64[:, :-1], 1, at[:, 0])
        g = g / torch.where(ok, length, torch.ones((), dtype=I64)).to(grad.dtype)[:, None, :]
    elif mode == 2:
        g = torch.where(torch.gather(arg.to(I64), 2, at) == torch.arange(n)[None, None, :], g, torch.zeros((), dtype=grad.dtype))
    return torch.where(ok[:, None, :], g, torch.zeros((), dtype=grad.dtype))


def grid_cluster(index_or_xyz: Any, resolution: int | None = None, lo: float = -0.5, extent: float = 1.0, m: int | None = None) -> GridIndex:
    """The partition of every cloud into the occupied cells of the grid of ``voxel_index``:
    ``GridIndex(cluster[B,N], seg[B,m+1], count[B], order[B,N])``, all int32.  ``index_or_xyz`` is the ``VoxelIndex`` of the
    clouds (``resolution``, if given, must be its own) or the clouds ``xyz[B,N,3]``, indexed here.  The occupied cells of a
    cloud are its slots, in ascending cell; ``m`` is the number of slots every cloud is padded -- or cut -- to.  With
    ``m=None`` it is the largest ``count`` of the batch (at least 1), which is read from the device: ONE host
    synchronisation; a given ``m`` (``1 <= m <= N``) synchronises nothing, and ``count > m`` then tells that the cells of
    rank ``m`` and above were dropped (their points have ``cluster = -1``).  A non-finite point has ``cluster = -1``.  Every
    word is fixed by the cloud alone (``pcc_grid_cluster``, include/pcc_neighbour.h); CPU tensors take the same rule in torch
    and give the same integers.  Carries no gradient."""
    what = 'grid_cluster'
    if isinstance(index_or_xyz, VoxelIndex):
        index = index_or_xyz
        if index.cell.dim() != 2 or not 1 <= index.cell.shape[1] <= MAX_VOXEL_POINTS:
            raise ValueError(f'{what}: expected index.cell[B,N] with 1 <= N <= {MAX_VOXEL_POINTS}, got {tuple(index.cell.shape)}')
        b, n = index.cell.shape
        res = _voxel_index_args(index, what, b, n, index.cell.device)
        if resolution is not None and resolution != res:
            raise ValueError(f'{what}: resolution {resolution!r} is not the index\'s ({res})')
        if m is not None:
            _capacity_arg(what, m, n)
    elif isinstance(index_or_xyz, torch.Tensor):
        b, n = _voxel_cloud_args(index_or_xyz, what)
        if resolution is None:
            raise ValueError(f'{what}: resolution is needed with a cloud')
        if m is not None:
            _capacity_arg(what, m, n)
        index = voxel_index(index_or_xyz, resolution, lo, extent)
    else:
        raise ValueError(f'{what}: expected a VoxelIndex or xyz[B,N,3], got {type(index_or_xyz).__name__}')
    _grid_pool_size_args(what, b, n)
    dev = index.cell.device
    cap = n if m is None else int(m)
    if b == 0:
        return GridIndex(torch.zeros((0, n), dtype=I32, device=dev), torch.zeros((0, (1 if m is None else cap) + 1), dtype=I32, device=dev),
                         torch.zeros((0,), dtype=I32, device=dev), index.order)
    if dev.type == 'cuda':
        cell, order = index.cell.contiguous(), index.order.contiguous()
        cluster, seg = torch.empty((b, n), dtype=I32, device=dev), torch.empty((b, cap + 1), dtype=I32, device=dev)
        count = torch.empty((b,), dtype=I32, device=dev)
        call(_L.pcc_grid_cluster, what, dev, b, n, cap, ptr(cell, 'index.cell', I32, dev), ptr(order, 'index.order', I32, dev),
             ptr(cluster, 'cluster', I32, dev), ptr(seg, 'seg', I32, dev), ptr(count, 'count', I32, dev))
    else:
        order = index.order
        cluster, seg, count = torch_grid_cluster(index, cap)
    if m is None:  # (at capacity N nothing was dropped: the first count.max() + 1 entries are the index at that capacity)
        seg = seg[:, :max(1, int(count.max().item())) + 1].contiguous()
    return GridIndex(cluster, seg, count, order)


class SegmentPooled(Function):
    """``SegmentPooled.apply(features, cluster, seg, order, mode)``: ``pcc_segment_pool``; the backward is
    ``pcc_segment_pool_bwd`` on the saved ``cluster``, ``seg`` and (max) ``arg``, run only when the gradient of ``features``
    is asked for.  CPU tensors take ``torch_segment_pool`` / ``torch_segment_pool_bwd``.  The arguments have been checked."""

    @staticmethod
    def forward(ctx: Any, features: torch.Tensor, cluster: torch.Tensor, seg: torch.Tensor, order: torch.Tensor, mode: int) -> torch.Tensor:
        features, cluster, seg, order = features.contiguous(), cluster.contiguous(), seg.contiguous(), order.contiguous()
        b, c, n = features.shape
        m = seg.shape[1] - 1
        dev = features.device
        if dev.type == 'cuda':
            xp, op, sp = ptr(features, 'features', F32, dev), ptr(order, 'index.order', I32, dev), ptr(seg, 'index.seg', I32, dev)
            out = torch.empty((b, c, m), dtype=F32, device=dev)
            arg = torch.empty((b, c, m), dtype=I32, device=dev) if mode == 2 else None
            call(_L.pcc_segment_pool, 'segment_pool', dev, b, c, n, m, mode, xp, op, sp, ptr(out, 'out', F32, dev), ptr(arg, 'arg', I32, dev))
        else:
            out, arg = torch_segment_pool(features, order, seg, mode)
        ctx.save_for_backward(cluster, seg, arg)
        ctx.n, ctx.mode = n, mode
        return out

    @staticmethod
    def backward(ctx: Any, grad: torch.Tensor) -> tuple[Any, None, None, None, None]:
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        cluster, seg, arg = ctx.saved_tensors
        grad = grad.contiguous()
        b, c, m = grad.shape
        dev = grad.device
        if dev.type != 'cuda':
            return torch_segment_pool_bwd(grad, cluster, seg, arg, ctx.mode), None, None, None, None
        gx = torch.empty((b, c, ctx.n), dtype=F32, device=dev)
        call(_L.pcc_segment_pool_bwd, 'segment_pool_bwd', dev, b, c, ctx.n, m, ctx.mode, ptr(cluster, 'index.cluster', I32, dev),
             ptr(seg, 'index.seg', I32, dev), ptr(arg, 'arg', I32, dev), ptr(grad, 'grad', F32, dev), ptr(gx, 'grad_features', F32, dev))
        return gx, None, None, None, None


def segment_pool(features: torch.Tensor, gindex: GridIndex, reduce: str = 'mean') -> torch.Tensor:
    """``out[B,C,m]``: the features ``features[B,C,N]`` float32 of the points of every slot of ``gindex`` (``grid_cluster``)
    reduced to one value -- ``'mean'``: summed in ascending point index from +0.0 and divided once, word for word what
    ``voxelize`` writes into that cell; ``'sum'``: the same without the division; ``'max'``: ``torch.max`` over the slot's
    points in ascending point index (the first NaN wins, else the greatest value, the lowest index among equal ones).  A
    padded slot is +0.0.  Nothing is atomic, so every word is fixed (``pcc_segment_pool``, include/pcc_neighbour.h);
    differentiable in ``features`` by a gather: the points of a slot share its gradient (divided by their number for the
    mean), the max hands it to the point it took; a dropped or non-finite point gets +0.0.  The HIP kernels on the
    accelerator, the same rule as a torch composition for CPU tensors: outputs and gradients agree word for word."""
    what = 'segment_pool'
    b, c, n = _features_arg(what, features)
    _float32('features', features)
    m = _grid_index_args(gindex, what, b, n, features.device)
    mode = _reduce_arg(what, reduce)
    _grid_pool_size_args(what, b, n)
    if b == 0:
        return torch.zeros((0, c, m), dtype=F32, device=features.device)
    return SegmentPooled.apply(features, gindex.cluster, gindex.seg, gindex.order, mode)


def grid_pool(xyz: torch.Tensor, features: torch.Tensor | None, resolution: int, lo: float = -0.5, extent: float = 1.0,
              m: int | None = None, reduce: str = 'max') -> GridPooled:
    """Partition-based pooling (Point Transformer V2's ``GridPool``) in one call: the clouds ``xyz[B,N,3]`` are cut by the
    grid of ``voxel_index(xyz, resolution, lo, extent)`` and every occupied cell becomes one point --
    ``GridPooled(xyz[B,m,3], features[B,C,m] or None, index, count)``: the mean coordinate of the cell's points, their
    features ``features[B,C,N]`` reduced by ``reduce`` (``segment_pool``), the ``GridIndex`` for ``grid_unpool`` on the way
    back up, and the number of occupied cells per cloud.  ``m`` as in ``grid_cluster``: ``None`` costs one host
    synchronisation.  A padded slot (``>= count``) holds NaN coordinates (the word 0x7fc00000) and +0 features: such a
    point is nobody's neighbour in ``ball_query``, never enters a ``knn`` / ``knn_cross`` list, is skipped by
    ``farthest_point_sample`` and has cell -1 in ``voxel_index``, so the pooled cloud can be fed to every op unchanged.
    Differentiable in ``features`` and, through the centres, in ``xyz``, with the partition held constant."""
    what = 'grid_pool'
    b, n = _voxel_cloud_args(xyz, what)
    mode = _reduce_arg(what, reduce)
    if features is not None:
        _features_arg(what, features)
        if features.shape[0] != b or features.shape[2] != n:
            raise ValueError(f'{what}: expected features[B = {b},C,N = {n}], got {tuple(features.shape)}')
        _float32('features', features)
        _same_device('features', features, xyz.device)
    gindex = grid_cluster(xyz, resolution, lo, extent, m)
    cap = gindex.seg.shape[1] - 1
    dev = xyz.device
    if b == 0:
        centres = torch.zeros((0, cap, 3), dtype=F32, device=dev)
        pooled = None if features is None else torch.zeros((0, features.shape[1], cap), dtype=F32, device=dev)
        return GridPooled(centres, pooled, gindex, gindex.count)
    centres = SegmentPooled.apply(xyz.transpose(1, 2), gindex.cluster, gindex.seg, gindex.order, 0).transpose(1, 2)
    padded = torch.arange(cap, device=dev)[None, :] >= gindex.count[:, None]
    centres = torch.where(padded[:, :, None], torch.full((), float('nan'), dtype=F32, device=dev), centres)
    pooled = None if features is None else SegmentPooled.apply(features, gindex.cluster, gindex.seg, gindex.order, mode)
    return GridPooled(centres, pooled, gindex, gindex.count)


def grid_subsample(xyz: torch.Tensor, resolution: int, lo: float = -0.5, extent: float = 1.0, m: int | None = None) -> torch.Tensor:
    """KPConv's ``grid_subsampling``: the barycentre of the points of every occupied cell, ``[B,m,3]``, NaN in the slots
    behind a cloud's last occupied cell -- ``grid_pool(xyz, None, ...).xyz``."""
    return grid_pool(xyz, None, resolution, lo, extent, m).xyz


def grid_unpool(pooled: torch.Tensor, gindex: GridIndex) -> torch.Tensor:
    """PTv2's map unpooling: ``out[B,C,N]``, every point takes the value ``pooled[B,C,m]`` holds for its slot --
    ``group_points`` along ``gindex.cluster`` with k = 1.  A point of a dropped or non-finite cell gets +0 and carries no
    gradient.  Differentiable in ``pooled``."""
    what = 'grid_unpool'
    if not isinstance(gindex, GridIndex):
        raise ValueError(f'{what}: expected a GridIndex, got {type(gindex).__name__}')
    if gindex.cluster.dim() != 2 or gindex.cluster.shape[1] < 1:
        raise ValueError(f'{what}: expected index.cluster[B,N] with N >= 1, got {tuple(gindex.cluster.shape)}')
    b, n = gindex.cluster.shape
    m = _grid_index_args(gindex, what, b, n, pooled.device)
    if pooled.dim() != 3 or pooled.shape[0] != b or pooled.shape[1] < 1 or pooled.shape[2] != m:
        raise ValueError(f'{what}: expected pooled[B = {b},C,m = {m}] with C >= 1, got {tuple(pooled.shape)}')
    _float32('pooled', pooled)
    return group_points(pooled, gindex.cluster.to(I64)[:, :, None])[:, :, :, 0]


# ---- submanifold sparse convolution on the slots of grid_cluster (MinkUNet, SparseUNet, PTv3's position encoding) ---------

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
    valid = (nbr >= 0) & (nbr < n)
    safe = torch.where(valid, nbr, torch.zeros_like(nbr))
    out = torch.zeros((b, weight.shape[2], m), dtype=features.dtype, device=features.device)
    zero = torch.zeros((), dtype=features.dtype, device=features.device)
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
            real = ((nbr >= 0) & (nbr < m)).any(2)
            gb = torch.where(real[:, None, :], grad, torch.zeros((), dtype=F32, device=dev)).sum((0, 2))
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


# ---- local surface geometry along a list: mean, scatter matrix, its eigen-decomposition, surface variation ----------------


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
    valid = (idx >= 0) & (idx < n)
    safe = torch.where(valid, idx, torch.zeros_like(idx))
    pts = [torch.gather(xyz, 1, safe[:, :, j, None].expand(-1, -1, 3)) for j in range(k)]
    acc = torch.zeros((b, m, 3), dtype=xyz.dtype, device=xyz.device)
    for j in range(k):
        acc = torch.where(valid[:, :, j, None], acc + pts[j], acc)
    cnt = valid.sum(-1)[:, :, None]
    mean = torch.where(cnt > 0, acc / cnt.clamp(min=1).to(xyz.dtype), torch.zeros((), dtype=xyz.dtype, device=xyz.device))
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
    s = torch.where(finite[:, None, None], s, torch.zeros((), dtype=s.dtype))
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


# ---- gather / edge features / max over k -------------------------------------------------------------------------


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
