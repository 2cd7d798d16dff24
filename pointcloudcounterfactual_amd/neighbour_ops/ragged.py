# ---- ragged batches: searches and sampling over packed clouds -------------------------------------------------------------

from __future__ import annotations

import numbers
from typing import Any

import torch

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import F32, I32, I64, _L, _float32, _same_device
from pointcloudcounterfactual_amd.neighbour_ops.sampling import _ball_args, farthest_point_sample, torch_ball_query

MAX_RAGGED_K = 32  # pcc_knn_ragged's list slots (include/pcc_neighbour.h)


# ---- offsets: integers only, any device ------------------------------------------------------------------------------------

def _offset_arg(what: str, name: str, offset: torch.Tensor) -> None:
    """``offset[B]`` is a one-dimensional int32 or int64 tensor, or the ``ValueError`` of ``what``."""
    if not isinstance(offset, torch.Tensor) or offset.dim() != 1 or offset.dtype not in (I32, I64):
        got = f'{tuple(offset.shape)} {offset.dtype}' if isinstance(offset, torch.Tensor) else type(offset).__name__
        raise ValueError(f'{what}: expected {name}[B] int32 or int64, got {got}')


def offset2bincount(offset: torch.Tensor) -> torch.Tensor:
    """``count[B]`` int64, the number of rows of every cloud of a packed batch: the differences of ``offset[B]``, the
    cumulative ends of the clouds."""
    _offset_arg('offset2bincount', 'offset', offset)
    offset = offset.to(I64)
    return torch.diff(offset, prepend=offset.new_zeros(1))


def offset2batch(offset: torch.Tensor) -> torch.Tensor:
    """``batch[n]`` int64, the cloud of every row of a packed batch with the cumulative ends ``offset[B]``.  (The length of
    the result is a value of ``offset``: on the accelerator ``repeat_interleave`` reads it, one synchronisation.)"""
    count = offset2bincount(offset)
    return torch.arange(count.shape[0], dtype=I64, device=offset.device).repeat_interleave(count)


def batch2offset(batch: torch.Tensor) -> torch.Tensor:
    """``offset[B]`` int64, the cumulative ends of the clouds of a packed batch whose rows carry the ascending cloud numbers
    ``batch[n]``; ``B = batch.max() + 1``, and a number that does not occur is a cloud without rows."""
    _offset_arg('batch2offset', 'batch', batch)
    return torch.cumsum(torch.bincount(batch.to(I64)), 0)


def _packed_arg(what: str, name: str, xyz: torch.Tensor, oname: str, offset: torch.Tensor, dev: torch.device | None = None) -> tuple[int, int]:
    """A packed cloud ``xyz[n,3]`` float32 (on ``dev``, where one is given) with ``offset[B]`` on its device, or the errors of
    the other ops: ``(b, n)``."""
    if not isinstance(xyz, torch.Tensor) or xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f'{what}: expected {name}[n,3], got {tuple(xyz.shape) if isinstance(xyz, torch.Tensor) else type(xyz).__name__}')
    _offset_arg(what, oname, offset)
    _float32(name, xyz)
    if dev is not None:
        _same_device(name, xyz, dev)
    _same_device(oname, offset, xyz.device)
    return offset.shape[0], xyz.shape[0]


def _valid_offsets(what: str, name: str, offset: torch.Tensor, total: int | None = None) -> list[int]:
    """The CPU paths trust nothing either, but they refuse where the kernels clip: ``offset`` must not decrease from 0 and,
    where ``total`` is given, must end at it, or ``ValueError``.  -> the offsets as a list with a leading 0."""
    ends = [0] + [int(v) for v in offset.tolist()]
    if any(hi < lo for lo, hi in zip(ends[:-1], ends[1:])) or (total is not None and ends[-1] != total):
        raise ValueError(f'{what}: {name} must be non-decreasing from 0{"" if total is None else f" and end at {total}"}, got {ends[1:]}')
    return ends


def _i32(offset: torch.Tensor) -> torch.Tensor:
    return offset.detach().to(I32).contiguous()


# ---- k-NN -------------------------------------------------------------------------------------------------------------------

def _knn_ragged_args(xyz: torch.Tensor, offset: torch.Tensor, k: Any, query: torch.Tensor | None,
                     query_offset: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """The checks ``knn_ragged`` makes before anything runs: ``(xyz, offset, query, query_offset)``, detached, the self
    search spelled out."""
    what = 'knn_ragged'
    b, _ = _packed_arg(what, 'xyz', xyz, 'offset', offset)
    if (query is None) != (query_offset is None):
        raise ValueError(f'{what}: query and query_offset come together')
    if query is not None:
        if _packed_arg(what, 'query', query, 'query_offset', query_offset, xyz.device)[0] != b:
            raise ValueError(f'{what}: expected query_offset[B = {b}], got {tuple(query_offset.shape)}')
    if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= k <= MAX_RAGGED_K:
        raise ValueError(f'{what}: k must be an integer in [1, {MAX_RAGGED_K}], got {k!r}')
    xyz = xyz.detach()
    return (xyz, offset, xyz, offset) if query is None else (xyz, offset, query.detach(), query_offset)


def torch_knn_ragged(xyz: torch.Tensor, offset: torch.Tensor, k: int, query: torch.Tensor, query_offset: torch.Tensor,
                     return_distance: bool = False) -> Any:
    """The rule of ``pcc_knn_ragged`` (include/pcc_neighbour.h) in torch, cloud by cloud; CPU path of ``knn_ragged``.  The
    distances are the difference form in float32, ``(df0 * df0 + df1 * df1) + df2 * df2`` with every product rounded: torch
    has no fma, so they are the kernel's words where the products are exact (lattice coordinates) and within a few ulp of
    them elsewhere, where a near tie may come out in the other order.  A stable sort gives the (distance, index) order; a
    NaN distance is never listed; a row that runs short ends in ``(-1, +inf)``.  The offsets are validated (non-decreasing,
    ending at the number of rows), not clipped."""
    n, m = xyz.shape[0], query.shape[0]
    ends = _valid_offsets('knn_ragged', 'offset', offset, n)
    qends = _valid_offsets('knn_ragged', 'query_offset', query_offset, m)
    idx = torch.full((m, k), -1, dtype=I64, device=xyz.device)
    dist = torch.full((m, k), float('inf'), dtype=F32, device=xyz.device)
    for c in range(len(ends) - 1):
        lo, hi, qlo, qhi = ends[c], ends[c + 1], qends[c], qends[c + 1]
        if hi == lo or qhi == qlo:
            continue
        kk = min(k, hi - lo)
        step = max(1, (1 << 21) // (hi - lo))  # queries per block: about 2M distances at a time
        for q0 in range(qlo, qhi, step):
            q1 = min(q0 + step, qhi)
            df = xyz[None, lo:hi, :] - query[q0:q1, None, :]
            d = df[..., 0] * df[..., 0]
            d = d + df[..., 1] * df[..., 1]
            d = d + df[..., 2] * df[..., 2]
            d, order = torch.sort(d, dim=1, stable=True)  # (NaN behind +inf, equal distances in index order)
            d, order = d[:, :kk], order[:, :kk]
            listed = ~torch.isnan(d)
            idx[q0:q1, :kk] = torch.where(listed, order + lo, torch.full_like(order, -1))
            dist[q0:q1, :kk] = torch.where(listed, d, torch.full_like(d, float('inf')))
    return (idx, dist) if return_distance else idx


def hip_knn_ragged(xyz: torch.Tensor, offset: torch.Tensor, k: int, query: torch.Tensor, query_offset: torch.Tensor,
                   return_distance: bool = False) -> Any:
    """``pcc_knn_ragged`` on checked arguments (``_knn_ragged_args``).  Nothing is read on the host."""
    dev = xyz.device
    same = query is xyz and query_offset is offset
    xyz, offset = xyz.contiguous(), _i32(offset)
    query, query_offset = (xyz, offset) if same else (query.contiguous(), _i32(query_offset))
    b, n, m = offset.shape[0], xyz.shape[0], query.shape[0]
    # (checked before anything is allocated on the device)
    xp, op = ptr(xyz, 'xyz', F32, dev), ptr(offset, 'offset', I32, dev)
    qp, qop = ptr(query, 'query', F32, dev), ptr(query_offset, 'query_offset', I32, dev)
    idx = torch.empty((m, k), dtype=I64, device=dev)
    dist = torch.empty((m, k), dtype=F32, device=dev) if return_distance else None
    if b == 0:  # (no cloud holds a row: the call enqueues nothing)
        idx.fill_(-1)
        if dist is not None:
            dist.fill_(float('inf'))
    call(_L.pcc_knn_ragged, 'knn_ragged', dev, b, n, m, k, xp, op, qp, qop, ptr(idx, 'idx', I64, dev), ptr(dist, 'dist', F32, dev))
    return (idx, dist) if return_distance else idx


def knn_ragged(xyz: torch.Tensor, offset: torch.Tensor, k: int, query: torch.Tensor | None = None,
               query_offset: torch.Tensor | None = None, return_distance: bool = False) -> Any:
    """k-NN over a packed batch: ``xyz[n,3]`` float32 holds the clouds end to end and ``offset[B]`` (int32 or int64) their
    cumulative ends; ``query[m,3]`` with ``query_offset[B]`` is packed the same way, and without them the search is the
    self search.  ``idx[m,k]`` int64 are GLOBAL indices into ``xyz``, for every query the ``k`` nearest points of its own
    cloud, ascending by (squared distance, index); with ``return_distance`` also ``dist[m,k]`` float32, squared.  A row
    that runs short -- a cloud of fewer than ``k`` points, NaN distances, a row of no cloud -- ends in ``idx = -1``,
    ``dist = +inf``: every op along a list (``group_points``, ``interpolate_points``, ``aggregate_points``, ``local_geometry``,
    ``kpconv_aggregate``) skips a -1 slot, so with ``b = 1`` they take the list as it is.  ``1 <= k <= 32``.  The full
    contract is ``pcc_knn_ragged``'s (include/pcc_neighbour.h).  On the accelerator the HIP kernel: the offsets stay on the
    device, are clipped and never trusted, and nothing synchronises.  For CPU tensors ``torch_knn_ragged``, which validates
    the offsets.  The inputs are detached; the outputs are constants of the graph."""
    xyz, offset, query, query_offset = _knn_ragged_args(xyz, offset, k, query, query_offset)
    if xyz.device.type == 'cuda':
        return hip_knn_ragged(xyz, offset, int(k), query, query_offset, return_distance)
    return torch_knn_ragged(xyz, offset, int(k), query, query_offset, return_distance)


# ---- ball query -------------------------------------------------------------------------------------------------------------

def _ball_ragged_args(xyz: torch.Tensor, offset: torch.Tensor, centres: torch.Tensor, centre_offset: torch.Tensor, radius: Any,
                      nsample: int, pad: str) -> tuple[torch.Tensor, torch.Tensor, float, int]:
    """The checks ``ball_query_ragged`` makes before anything runs (``radius``, ``nsample`` and ``pad`` through
    ``ball_query``'s own): ``(xyz detached, centres detached, radius as the float32 the library receives, pad as the C
    constant)``."""
    what = 'ball_query_ragged'
    b, n = _packed_arg(what, 'xyz', xyz, 'offset', offset)
    if n < 1:
        raise ValueError(f'{what}: expected xyz[n,3] with n >= 1, got {tuple(xyz.shape)}')
    if _packed_arg(what, 'centres', centres, 'centre_offset', centre_offset, xyz.device)[0] != b:
        raise ValueError(f'{what}: expected centre_offset[B = {b}], got {tuple(centre_offset.shape)}')
    _, _, r32, pad_c = _ball_args(xyz[None], centres[None], radius, nsample, pad)
    return xyz.detach(), centres.detach(), r32, pad_c


def torch_ball_query_ragged(xyz: torch.Tensor, offset: torch.Tensor, centres: torch.Tensor, centre_offset: torch.Tensor, radius: float,
                            nsample: int, pad: int = 0, return_count: bool = False) -> Any:
    """The rule of ``pcc_ball_query_ragged`` (include/pcc_neighbour.h) as a loop over the clouds through
    ``torch_ball_query``, so the words are the kernel's; CPU path of ``ball_query_ragged``.  ``pad`` is the C constant.  The
    offsets are validated (non-decreasing, ending at the number of rows), not clipped."""
    n, m = xyz.shape[0], centres.shape[0]
    ends = _valid_offsets('ball_query_ragged', 'offset', offset, n)
    qends = _valid_offsets('ball_query_ragged', 'centre_offset', centre_offset, m)
    idx = torch.full((m, nsample), -1, dtype=I64, device=xyz.device)
    cnt = torch.zeros((m,), dtype=I32, device=xyz.device)
    for c in range(len(ends) - 1):
        lo, hi, qlo, qhi = ends[c], ends[c + 1], qends[c], qends[c + 1]
        if hi == lo or qhi == qlo:
            continue  # (a cloud without points: cnt = 0 and -1 throughout, whatever pad is)
        one, one_cnt = torch_ball_query(xyz[None, lo:hi], centres[None, qlo:qhi], radius, nsample, pad, True)
        idx[qlo:qhi] = torch.where(one[0] >= 0, one[0] + lo, one[0])
        cnt[qlo:qhi] = one_cnt[0]
    return (idx, cnt) if return_count else idx


def hip_ball_query_ragged(xyz: torch.Tensor, offset: torch.Tensor, centres: torch.Tensor, centre_offset: torch.Tensor, radius: float,
                          nsample: int, pad: int = 0, return_count: bool = False) -> Any:
    """``pcc_ball_query_ragged`` on checked arguments (``_ball_ragged_args``).  Nothing is read on the host."""
    dev = xyz.device
    xyz, centres, offset, centre_offset = xyz.contiguous(), centres.contiguous(), _i32(offset), _i32(centre_offset)
    b, n, m = offset.shape[0], xyz.shape[0], centres.shape[0]
    # (checked before anything is allocated on the device)
    xp, op = ptr(xyz, 'xyz', F32, dev), ptr(offset, 'offset', I32, dev)
    cp, cop = ptr(centres, 'centres', F32, dev), ptr(centre_offset, 'centre_offset', I32, dev)
    idx = torch.empty((m, nsample), dtype=I64, device=dev)
    cnt = torch.empty((m,), dtype=I32, device=dev) if return_count else None
    if b == 0:  # (no cloud holds a row: the call enqueues nothing)
        idx.fill_(-1)
        if cnt is not None:
            cnt.zero_()
    call(_L.pcc_ball_query_ragged, 'ball_query_ragged', dev, b, n, m, nsample, radius, pad, xp, op, cp, cop, ptr(idx, 'idx', I64, dev),
         ptr(cnt, 'cnt', I32, dev))
    return (idx, cnt) if return_count else idx


def ball_query_ragged(xyz: torch.Tensor, offset: torch.Tensor, centres: torch.Tensor, centre_offset: torch.Tensor, radius: float,
                      nsample: int, pad: str = 'first', return_count: bool = False) -> Any:
    """Ball query over a packed batch (the layout of ``knn_ragged``): for every centre of ``centres[m,3]`` the first
    ``nsample`` points (ascending index) of ITS cloud of ``xyz[n,3]`` strictly inside the ball of ``radius``:
    ``idx[m,nsample]`` int64 GLOBAL indices into ``xyz`` and, with ``return_count``, ``cnt[m]`` int32.  Per cloud this is
    ``ball_query``'s rule word for word.  Slots past ``cnt`` repeat the row's first index (``pad='first'``; the cloud's first
    point for an empty ball) or hold -1 (``pad='none'``); a row of no cloud or of a cloud without points is -1 throughout
    with ``cnt = 0``.  The full contract is ``pcc_ball_query_ragged``'s (include/pcc_neighbour.h).  The HIP kernel on the
    accelerator (offsets clipped on the device, no synchronisation), ``torch_ball_query_ragged`` for CPU tensors (offsets
    validated): the two agree word for word.  The inputs are detached; the outputs are constants of the graph."""
    xyz, centres, radius, pad_c = _ball_ragged_args(xyz, offset, centres, centre_offset, radius, nsample, pad)
    if xyz.device.type == 'cuda':
        return hip_ball_query_ragged(xyz, offset, centres, centre_offset, radius, nsample, pad_c, return_count)
    return torch_ball_query_ragged(xyz, offset, centres, centre_offset, radius, nsample, pad_c, return_count)


# ---- farthest point sampling ------------------------------------------------------------------------------------------------

def farthest_point_sample_ragged(xyz: torch.Tensor, offset: torch.Tensor, new_offset: torch.Tensor) -> torch.Tensor:
    """Farthest point sampling of every cloud of a packed batch ``xyz[n,3]`` / ``offset[B]``: cloud ``c`` gives
    ``m_c = new_offset[c] - new_offset[c-1]`` picks, and ``idx[m]`` int64 holds them packed, as GLOBAL indices into ``xyz``.
    Per cloud the picks are word for word ``farthest_point_sample`` of that cloud alone from its first point.  No kernel of
    its own: the clouds are padded with NaN rows to ``[B,Nmax,3]``, ``farthest_point_sample`` takes ``max m_c`` picks of each
    -- it never picks a non-finite point while a finite one is left, and its picks are a greedy prefix -- and the first
    ``m_c`` of each cloud are kept.  Both offset vectors are read on the host: ONE synchronisation (the models that sample
    this way compute ``new_offset`` on the host anyway).  Requires valid offsets (non-decreasing, ``offset`` ending at
    ``n``) and ``m_c <= n_c``, otherwise ``ValueError``.  Either device; not differentiable."""
    what = 'farthest_point_sample_ragged'
    b, n = _packed_arg(what, 'xyz', xyz, 'offset', offset)
    _offset_arg(what, 'new_offset', new_offset)
    if new_offset.shape[0] != b:
        raise ValueError(f'{what}: expected new_offset[B = {b}], got {tuple(new_offset.shape)}')
    dev = xyz.device
    host = torch.stack((offset.detach().to(I64), new_offset.detach().to(device=dev, dtype=I64))).cpu() if b else torch.zeros((2, 0), dtype=I64)
    ends = _valid_offsets(what, 'offset', host[0], n)
    new_ends = _valid_offsets(what, 'new_offset', host[1])
    count = [hi - lo for lo, hi in zip(ends[:-1], ends[1:])]
    new_count = [hi - lo for lo, hi in zip(new_ends[:-1], new_ends[1:])]
    if any(mc > nc for mc, nc in zip(new_count, count)):
        raise ValueError(f'{what}: a cloud cannot give more picks than it has points: counts {count}, picks {new_count}')
    m = new_ends[-1]
    if m == 0:
        return torch.zeros((0,), dtype=I64, device=dev)
    lo = torch.tensor(ends[:-1], dtype=I64, device=dev)
    new_lo = torch.tensor(new_ends[:-1], dtype=I64, device=dev)
    batch = torch.arange(b, dtype=I64, device=dev).repeat_interleave(torch.tensor(count, dtype=I64, device=dev), output_size=n)
    new_batch = torch.arange(b, dtype=I64, device=dev).repeat_interleave(torch.tensor(new_count, dtype=I64, device=dev), output_size=m)
    padded = torch.full((b, max(count), 3), float('nan'), dtype=F32, device=dev)
    padded[batch, torch.arange(n, dtype=I64, device=dev) - lo[batch]] = xyz.detach()
    sel = farthest_point_sample(padded, max(new_count), start=0)  # [B, max m_c]
    return sel[new_batch, torch.arange(m, dtype=I64, device=dev) - new_lo[new_batch]] + lo[new_batch]
