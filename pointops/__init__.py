"""``pointops`` with the names and argument orders of the op package the Point Transformer family and Pointcept ship (a
CUDA-only extension), on this library's HIP kernels.  Everything is point-major over PACKED batches: ``xyz[n,3]`` /
``feat[n,c]`` hold the clouds end to end and ``offset[B]`` their cumulative ends; a list is ``idx[m,nsample]`` int32 of
GLOBAL indices into the packed array, -1 for a slot that names no point.

The searches run in ``neighbour_ops.knn_ragged`` / ``ball_query_ragged`` (one launch for the whole batch, the offsets stay
on the device), the sampling in ``farthest_point_sample_ragged``, the gathers and the interpolation in ``group_points`` and
``interpolate_points`` with a batch of one: on the accelerator a HIP kernel, never a torch composition.

Differences from the original that are deliberate: ``min_radius != 0`` raises ``NotImplementedError``;
``nsample > 32`` in ``knn_query`` raises ``ValueError``; a padded k-NN slot is ``(-1, +inf)`` where the original has a
distance of 1e10; ties go to the lowest index; ``ball_query`` lists ascending indices with the strict ``d^2 < r^2`` and pads
with the first; CPU tensors work; inputs are made contiguous, not asserted contiguous.  ``random_ball_query``,
``subtraction``, ``aggregation`` and the ``attention_*_step`` ops are not covered (``neighbour_ops.aggregate_points`` is the
aggregation)."""

from __future__ import annotations

import torch

from pointcloudcounterfactual_amd import neighbour_ops as ops
from pointcloudcounterfactual_amd.neighbour_ops import batch2offset, offset2batch, offset2bincount  # noqa: F401

I32, I64 = torch.int32, torch.int64

__all__ = ['offset2batch', 'batch2offset', 'offset2bincount', 'farthest_point_sampling', 'knn_query', 'ball_query', 'grouping',
           'knn_query_and_group', 'ball_query_and_group', 'query_and_group', 'interpolation']


def _list64(idx: torch.Tensor) -> torch.Tensor:
    """An int32 or int64 list ``idx[m,nsample]`` as the int64 list ``[1,m,nsample]`` the ops take."""
    if idx.dim() != 2 or idx.dtype not in (I32, I64):
        raise ValueError(f'pointops: expected idx[m,nsample] int32 or int64, got {tuple(idx.shape)} {idx.dtype}')
    return idx.detach().to(I64)[None]


def _root(d2: torch.Tensor) -> torch.Tensor:
    """The correctly rounded float32 root of a squared distance on either device (``pointnet2_utils.three_nn`` has why)."""
    return torch.sqrt(d2.double()).float()


def farthest_point_sampling(xyz: torch.Tensor, offset: torch.Tensor, new_offset: torch.Tensor) -> torch.Tensor:
    """``idx[m]`` int32, global: farthest point sampling of every cloud of ``xyz[n,3]`` / ``offset[B]`` from its first point,
    cloud ``c`` giving ``new_offset[c] - new_offset[c-1]`` picks (``neighbour_ops.farthest_point_sample_ragged``: the two
    offset vectors are read on the host).  More picks than points in a cloud is a ``ValueError``.  Not differentiable."""
    return ops.farthest_point_sample_ragged(xyz, offset, new_offset).to(I32)


def knn_query(nsample: int, xyz: torch.Tensor, offset: torch.Tensor, new_xyz: torch.Tensor | None = None,
              new_offset: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``(idx[m,nsample] int32, dist[m,nsample])``: for every point of ``new_xyz[m,3]`` / ``new_offset[B]`` (default: the
    points themselves) the ``nsample`` nearest points of its own cloud of ``xyz[n,3]`` / ``offset[B]``, ascending Euclidean
    distance, ties by ascending index (``neighbour_ops.knn_ragged``).  A cloud of fewer than ``nsample`` points fills the
    rest of its rows with ``(-1, +inf)``.  ``nsample > 32`` is a ``ValueError``.  Not differentiable."""
    if new_xyz is None:
        new_offset = None  # (the original searches the points themselves with their own offsets)
    elif new_offset is None:
        raise ValueError('knn_query: new_xyz comes with new_offset')
    idx, d2 = ops.knn_ragged(xyz, offset, nsample, new_xyz, new_offset, return_distance=True)
    return idx.to(I32), _root(d2)


def ball_query(nsample: int, max_radius: float, min_radius: float, xyz: torch.Tensor, offset: torch.Tensor,
               new_xyz: torch.Tensor | None = None, new_offset: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """``(idx[m,nsample] int32, dist[m,nsample])``: for every centre of ``new_xyz[m,3]`` / ``new_offset[B]`` (default: the
    points themselves) the first ``nsample`` points of its own cloud in ascending index with ``d^2 < max_radius^2``; the
    remaining slots repeat the row's first hit, an empty ball names the cloud's first point, a cloud without points gives
    -1 (``neighbour_ops.ball_query_ragged`` with ``pad='first'``).  ``dist`` is the Euclidean distance of every slot's point
    to the centre (float64, rounded once), ``+inf`` for a -1 slot.  ``min_radius`` other than 0 is a
    ``NotImplementedError``.  Not differentiable."""
    if min_radius != 0:
        raise NotImplementedError('ball_query: min_radius != 0 is not supported (the inner shell is not searched)')
    if new_xyz is None:
        new_xyz, new_offset = xyz, offset
    elif new_offset is None:
        raise ValueError('ball_query: new_xyz comes with new_offset')
    idx = ops.ball_query_ragged(xyz, offset, new_xyz, new_offset, max_radius, nsample, pad='first')
    real = idx >= 0
    df = xyz.detach().double()[torch.where(real, idx, torch.zeros_like(idx))] - new_xyz.detach().double()[:, None, :]
    d2 = (df * df).sum(-1)
    dist = torch.where(real, torch.sqrt(d2), torch.full_like(d2, float('inf'))).float()
    return idx.to(I32), dist


def grouping(idx: torch.Tensor, feat: torch.Tensor, xyz: torch.Tensor, new_xyz: torch.Tensor | None = None,
             with_xyz: bool = False) -> torch.Tensor:
    """``out[m,nsample,c]``: ``feat[n,c]`` gathered along ``idx[m,nsample]``; with ``with_xyz`` ``out[m,nsample,3+c]``, in
    front the coordinates ``xyz[n,3]`` of the same points relative to ``new_xyz[m,3]`` (default ``xyz``).  A -1 slot is a
    zero row, relative coordinates included, and carries no gradient (the original appends a zero row and masks).  One
    grouping op (``neighbour_ops.group_points``, point-major, a batch of one); differentiable in ``feat``, ``xyz`` and
    ``new_xyz``."""
    if new_xyz is None:
        new_xyz = xyz
    lst = _list64(idx)
    if feat.dim() != 2 or xyz.dim() != 2 or new_xyz.dim() != 2:
        raise ValueError(f'grouping: expected feat[n,c], xyz[n,3] and new_xyz[m,3], got {tuple(feat.shape)}, {tuple(xyz.shape)} and '
                         f'{tuple(new_xyz.shape)}')
    if with_xyz:
        out = ops.group_points_relative(xyz[None], feat[None], lst, new_xyz[None], point_major=True)  # (one tensor, no cat)
    else:
        out = ops.group_points(feat[None], lst, point_major=True)
    return out[0].permute(1, 2, 0).contiguous()


def knn_query_and_group(feat: torch.Tensor, xyz: torch.Tensor, offset: torch.Tensor | None = None, new_xyz: torch.Tensor | None = None,
                        new_offset: torch.Tensor | None = None, idx: torch.Tensor | None = None, nsample: int | None = None,
                        with_xyz: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """``(grouping(idx, feat, xyz, new_xyz, with_xyz), idx)`` with ``idx`` from ``knn_query`` unless it is given."""
    if idx is None:
        if nsample is None or offset is None:
            raise ValueError('knn_query_and_group: without idx, nsample and offset are needed')
        idx, _ = knn_query(nsample, xyz, offset, new_xyz, new_offset)
    return grouping(idx, feat, xyz, new_xyz, with_xyz), idx


def ball_query_and_group(feat: torch.Tensor, xyz: torch.Tensor, offset: torch.Tensor | None = None, new_xyz: torch.Tensor | None = None,
                         new_offset: torch.Tensor | None = None, idx: torch.Tensor | None = None, max_radio: float | None = None,
                         min_radio: float | None = None, nsample: int | None = None, with_xyz: bool = False) -> tuple[torch.Tensor, torch.Tensor]:
    """``(grouping(idx, feat, xyz, new_xyz, with_xyz), idx)`` with ``idx`` from ``ball_query`` unless it is given (the
    original's spelling of the two radii)."""
    if idx is None:
        if nsample is None or offset is None or max_radio is None or min_radio is None:
            raise ValueError('ball_query_and_group: without idx, nsample, offset, max_radio and min_radio are needed')
        idx, _ = ball_query(nsample, max_radio, min_radio, xyz, offset, new_xyz, new_offset)
    return grouping(idx, feat, xyz, new_xyz, with_xyz), idx


def query_and_group(nsample: int, xyz: torch.Tensor, new_xyz: torch.Tensor | None, feat: torch.Tensor, idx: torch.Tensor | None,
                    offset: torch.Tensor, new_offset: torch.Tensor | None, dilation: int = 0, with_feat: bool = True,
                    with_xyz: bool = True) -> tuple[torch.Tensor, torch.Tensor]:
    """The older spelling: ``(new_feat[m,nsample,3+c], idx)``, the k-NN list (unless ``idx`` is given) and the grouping with
    the relative coordinates in front; ``with_xyz=False``: the features only, ``with_feat=False``: the coordinates only.  A
    ``dilation`` other than 0 (a random subset of a longer list) is a ``NotImplementedError``."""
    if dilation != 0:
        raise NotImplementedError('query_and_group: dilation != 0 is not supported')
    if not with_feat and not with_xyz:
        raise ValueError('query_and_group: with_feat or with_xyz')
    if idx is None:
        idx, _ = knn_query(nsample, xyz, offset, new_xyz, new_offset)
    if not with_feat:
        centres = xyz if new_xyz is None else new_xyz
        return ops.group_points_relative(xyz[None], None, _list64(idx), centres[None])[0].permute(1, 2, 0).contiguous(), idx
    return grouping(idx, feat, xyz, new_xyz, with_xyz), idx


def interpolation(xyz: torch.Tensor, new_xyz: torch.Tensor, feat: torch.Tensor, offset: torch.Tensor, new_offset: torch.Tensor,
                  k: int = 3) -> torch.Tensor:
    """``new_feat[m,c]``: ``feat[n,c]`` of the points ``xyz[n,3]`` / ``offset[B]`` interpolated onto ``new_xyz[m,3]`` /
    ``new_offset[B]`` from the ``k`` nearest points of the same cloud with the weights ``(1 / (dist + 1e-8))`` normalised
    over the row, ``dist`` Euclidean (``knn_query``, then ``neighbour_ops.interpolate_points`` with a batch of one).  A
    padded slot (a cloud of fewer than ``k`` points) has weight 0 and adds nothing; a row without any real slot is 0.
    Differentiable in ``feat``."""
    if feat.dim() != 2 or feat.shape[0] != xyz.shape[0]:
        raise ValueError(f'interpolation: expected feat[n = {xyz.shape[0]},c], got {tuple(feat.shape)}')
    idx, dist = knn_query(k, xyz, offset, new_xyz, new_offset)
    recip = 1.0 / (dist + 1e-8)
    norm = recip[:, :1]
    for j in range(1, recip.shape[1]):  # (in slot order: the same words on either device)
        norm = norm + recip[:, j:j + 1]
    weight = torch.where(norm > 0, recip / torch.where(norm > 0, norm, torch.ones_like(norm)), torch.zeros_like(recip))
    return ops.interpolate_points(feat.t()[None], idx.to(I64)[None], weight[None])[0].t().contiguous()
