# ---- farthest point sampling ---------------------------------------------------------------------------------------

from __future__ import annotations

import numbers
from typing import Any

import torch

from pointcloudcounterfactual_amd._float32 import fma32
from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import F32, I32, I64, _L, _cloud_arg, _float32, _same_device


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
