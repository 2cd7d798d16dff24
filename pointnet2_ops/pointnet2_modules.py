"""``pointnet2_ops.pointnet2_modules``: the set-abstraction and feature-propagation modules of PointNet++ with the original's
constructor arguments and ``state_dict`` layout (a checkpoint trained with the original loads with ``strict=True``).  The
dense layers are plain torch; every search, gather and interpolation goes through ``pointnet2_utils``."""

from __future__ import annotations

from typing import Sequence

import torch
from torch import nn

from pointnet2_ops import pointnet2_utils


def build_shared_mlp(mlp_spec: Sequence[int], bn: bool = True) -> nn.Sequential:
    """A flat ``Sequential`` of ``Conv2d(a, b, 1, bias=not bn)``, ``BatchNorm2d(b)`` (with ``bn``) and ``ReLU(True)`` per
    consecutive pair ``(a, b)`` of ``mlp_spec``."""
    layers: list[nn.Module] = []
    for a, b in zip(mlp_spec[:-1], mlp_spec[1:]):
        layers.append(nn.Conv2d(a, b, kernel_size=1, bias=not bn))
        if bn:
            layers.append(nn.BatchNorm2d(b))
        layers.append(nn.ReLU(True))
    return nn.Sequential(*layers)


class _PointnetSAModuleBase(nn.Module):
    def __init__(self) -> None:
        super().__init__()
        self.npoint: int | None = None
        self.groupers: nn.ModuleList | None = None
        self.mlps: nn.ModuleList | None = None

    def forward(self, xyz: torch.Tensor, features: torch.Tensor | None) -> tuple[torch.Tensor | None, torch.Tensor]:
        """``xyz[B,N,3]``, ``features[B,C,N]`` or None -> ``(new_xyz[B,npoint,3] or None, new_features[B, sum of the last
        widths, npoint])``: one farthest point sampling, the centres gathered from ``xyz``, and per scale grouper -> MLP ->
        max over the group."""
        new_xyz = None
        if self.npoint is not None:
            sel = pointnet2_utils.furthest_point_sample(xyz, self.npoint)
            new_xyz = pointnet2_utils.gather_operation(xyz.transpose(1, 2), sel).transpose(1, 2).contiguous()
        pooled = []
        for grouper, mlp in zip(self.groupers, self.mlps):
            new_features = mlp(grouper(xyz, new_xyz, features))  # [B,C',npoint,nsample]
            pooled.append(torch.max(new_features, 3)[0])
        return new_xyz, torch.cat(pooled, 1)


class PointnetSAModuleMSG(_PointnetSAModuleBase):
    """Set abstraction with multi-scale grouping: ``npoint`` centres, one ``QueryAndGroup(radii[i], nsamples[i])`` and one
    shared MLP ``mlps[i]`` per scale (its first width raised by 3 with ``use_xyz``); ``npoint=None`` groups the whole
    cloud (``GroupAll``)."""

    def __init__(self, npoint: int | None, radii: Sequence[float], nsamples: Sequence[int], mlps: Sequence[Sequence[int]],
                 bn: bool = True, use_xyz: bool = True) -> None:
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        self.npoint = npoint
        self.groupers = nn.ModuleList()
        self.mlps = nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            spec = list(spec)
            if use_xyz:
                spec[0] += 3
            self.mlps.append(build_shared_mlp(spec, bn))


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction at a single scale."""

    def __init__(self, mlp: Sequence[int], npoint: int | None = None, radius: float | None = None, nsample: int | None = None,
                 bn: bool = True, use_xyz: bool = True) -> None:
        super().__init__(npoint=npoint, radii=[radius], nsamples=[nsample], mlps=[mlp], bn=bn, use_xyz=use_xyz)


class PointnetFPModule(nn.Module):
    """Feature propagation: the features of ``known`` interpolated onto ``unknown`` with inverse-distance weights of the
    three nearest neighbours, concatenated with the skip features, then a shared MLP."""

    def __init__(self, mlp: Sequence[int], bn: bool = True) -> None:
        super().__init__()
        self.mlp = build_shared_mlp(mlp, bn=bn)

    def forward(self, unknown: torch.Tensor, known: torch.Tensor | None, unknow_feats: torch.Tensor | None,
                known_feats: torch.Tensor) -> torch.Tensor:
        """``unknown[B,n,3]``, ``known[B,m,3]`` or None, ``unknow_feats[B,C1,n]`` or None, ``known_feats[B,C2,m]`` ->
        ``[B,mlp[-1],n]``."""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            dist_recip = 1.0 / (dist + 1e-8)
            weight = dist_recip / torch.sum(dist_recip, dim=2, keepdim=True)
            interpolated = pointnet2_utils.three_interpolate(known_feats, idx, weight)
        else:
            interpolated = known_feats.expand(*(tuple(known_feats.shape[:2]) + (unknown.shape[1],)))
        new_features = interpolated if unknow_feats is None else torch.cat((interpolated, unknow_feats), 1)
        return self.mlp(new_features.unsqueeze(-1)).squeeze(-1)
