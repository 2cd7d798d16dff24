"""Fused EdgeConv front-end.

The reference's EdgeConv block (``src/module/encoders.py:50-53`` with ``EdgeConvLayer``, ``src/module/layers.py:159-203``)

    feat = cat([x[idx] - x, x])            # [B, 2C, N, k]   up to 1.68 GB per layer at B=32, N=2048, k=25, C=128
    y = max_j act(BatchNorm2d(Conv2d_1x1(feat)))                        # act = LeakyReLU(0.2) or identity

never needs the ``[B,2C,N,k]`` tensor.  The 1x1 convolution is linear, so with ``W = [Wa | Wb]``

    z[b,:,n,j] = Wa (x_j - x_n) + Wb x_n = y1[b,:,idx[n,j]] + y2[b,:,n],     y1 = Wa x,  y2 = (Wb - Wa) x      ([B,C',N])

and, because BatchNorm is a per-channel affine map and the activation is increasing,

    max_j act(bn(z_j)) = act(bn(max_j z_j))  if the BatchNorm scale of the channel is >= 0, act(bn(min_j z_j)) otherwise,
    max_j z_j = max_j y1[idx[n,j]] + y2[n]   (y2 does not depend on j).

In float32 the products must not carry what ``x_j`` and ``x_n`` share: a cloud that sits at distance D from the origin
would round ``Wa x_j`` and ``Wa x_n`` at ``u D |Wa|`` each before the difference is formed, where the unfused block rounds
``x_j - x_n`` at ``u |x_j - x_n|``.  For ANY constant ``mu`` (per sample and channel)

    z[b,:,n,j] = Wa (xc_j - xc_n) + Wb (xc_n + mu) = y1[b,:,idx[n,j]] + y2[b,:,n] + c0[b,:],
    xc = x - mu,   y1 = Wa xc,   y2 = (Wb - Wa) xc,   c0 = Wb mu

is the same function of ``x``, so ``mu`` is a detached number: the sample's own mean over n with non-finite entries
counted as 0 (per sample: eval mode must not couple the samples of a batch; finite: one NaN or inf point must not reach
the other points through ``mu``).  The gradients are those of the unfused block whatever ``mu`` is.  ``c0`` is the only
large term left and BatchNorm takes most of it away again, so it never enters a float32 sum: ``c0 - mean`` is formed in
double, and the output is ``act((y1[t] + y2[n] + (c0 - mean)) scale + beta)``.

Training-mode BatchNorm statistics over (b,n,j) are exact sums of ``[B,C',N]`` quantities, taken in double:

    sum z          = sum_t deg[t] y1[t] + k sum_n (y2[n] + c0)
    sum (z - m)^2  = sum_t deg[t] y1[t]^2 + k sum_n y2m[n]^2 + 2 sum_n y2m[n] S1[n],
                     y2m = y2 + c0 - m,   m = sum z / (B N k),   S1[n] = sum_j y1[idx[n,j]]

The variance is centred, not ``E[z^2] - m^2``: in the backward of the latter the edge terms ``2 (y2[n] + c0) / M`` reach the
float32 neighbour-sum scatter before ``2 m deg[t] / M`` cancels them, which cost the input gradient a factor 5 off the
origin (tests/edgeconv_reference.py holds every output, gradient and statistic to float64; DESIGN.md 4n has the table).

(``deg[t]`` = in-degree of t in the kNN graph).  Everything is differentiable PyTorch on ``[B,C',N]`` tensors plus three
small HIP kernels (neighbour sum and its scatter backward, min/max neighbour selection), so autograd gives the exact
gradients of the unfused block, including the statistics' dependence on every edge.  The parameters are the
reference's (``Conv2d(2C, C', 1, bias=False)`` + ``BatchNorm2d(C')``), so state dicts are interchangeable.
"""

from __future__ import annotations

import torch
from torch import nn

from pointcloudcounterfactual_amd import _lib
from pointcloudcounterfactual_amd import neighbour_ops as ops
from pointcloudcounterfactual_amd._lib import call, ptr

_L = _lib.lib
F32, I64 = torch.float32, torch.int64


# ``S[b,c,n] = sum_j y[b,c,idx[b,n,j]]``; backward scatters ``g[b,c,n]`` along every edge
NEIGHBOUR_SUM = ops.IndexedOp('neighbour_sum', lambda b, c, n, k: (b, c, n), names=('y', 'idx'))


def neighbour_sum(y: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    if y.device.type == 'cuda':
        return ops.Indexed.apply(NEIGHBOUR_SUM, y, idx.contiguous())
    return ops.get_neighbours(y, idx, idx.shape[2])[1].sum(-1)


def neighbour_minmax_target(y: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``tsel[B,2,C,N]`` int64: per (channel, point) the neighbour with the largest / smallest ``y`` (no gradient)."""
    y = y.detach().contiguous()
    b, c, n = y.shape
    if y.device.type == 'cuda':
        dev = y.device
        tsel = torch.empty((b, 2, c, n), dtype=torch.int64, device=dev)
        call(_L.pcc_neighbour_minmax_target, 'neighbour_minmax_target', dev, b, c, n, idx.shape[2], ptr(y, 'y', F32, dev),
             ptr(idx.contiguous(), 'idx', I64, dev), ptr(tsel, 'tsel', I64, dev))
        return tsel
    nb = ops.get_neighbours(y, idx, idx.shape[2])[1]                      # [B,C,N,k]
    ie = idx[:, None, :, :].expand(-1, c, -1, -1)
    return torch.stack([torch.gather(ie, 3, nb.argmax(3, keepdim=True))[..., 0],
                        torch.gather(ie, 3, nb.argmin(3, keepdim=True))[..., 0]], dim=1)


class FusedEdgeConv(nn.Module):
    """Drop-in for ``get_graph_features -> EdgeConvLayer -> max(dim=3)`` of the reference's DGCNN blocks."""

    def __init__(self, in_dim: int, out_dim: int, act: bool = True, momentum: float = 0.1, eps: float = 1e-5) -> None:
        super().__init__()
        self.conv = nn.Conv2d(2 * in_dim, out_dim, 1, bias=False)         # same parameters as the unfused block
        self.bn = nn.BatchNorm2d(out_dim, momentum=momentum, eps=eps)
        self.act = nn.LeakyReLU(0.2) if act else nn.Identity()
        self.in_dim = in_dim

    def forward(self, x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
        """``x[B,C,N]``, ``idx[B,N,k]`` -> ``[B,C',N]``."""
        b, c, n = x.shape
        k = idx.shape[2]
        w = self.conv.weight[:, :, 0, 0]
        wa, wb = w[:, :c], w[:, c:]
        # a constant per (sample, channel) near the cloud's centre (module docstring); non-finite points count as 0, so one
        # of them cannot poison its sample, and no other sample enters, so eval does not couple the samples of a batch
        mu = torch.nan_to_num(x.detach(), nan=0.0, posinf=0.0, neginf=0.0).mean(dim=2, keepdim=True)
        xc = x - mu
        y1 = torch.matmul(wa, xc)                                         # [B,C',N]
        y2 = torch.matmul(wb - wa, xc)
        c0 = torch.matmul(wb, mu).double()                                # [B,C',1]: z = y1[t] + y2[n] + c0
        if self.training or not self.bn.track_running_stats:
            m = float(b * n * k)
            deg = torch.zeros((b, n), dtype=torch.float32, device=x.device)
            deg.scatter_add_(1, idx.reshape(b, -1), torch.ones((b, n * k), dtype=torch.float32, device=x.device))
            s1 = neighbour_sum(y1, idx)
            y1d, y2d, s1d, degd = y1.double(), y2.double() + c0, s1.double(), deg.double()[:, None, :]
            mean = ((degd * y1d).sum((0, 2)) + k * y2d.sum((0, 2))) / m
            y2m = y2d - mean[None, :, None]
            sum_d2 = (degd * y1d * y1d).sum((0, 2)) + k * (y2m * y2m).sum((0, 2)) + 2.0 * (y2m * s1d).sum((0, 2))
            var = (sum_d2 / m).clamp_min(0.0)                              # biased, as BatchNorm normalises with
            if self.training and self.bn.track_running_stats:
                with torch.no_grad():
                    mom = self.bn.momentum
                    self.bn.running_mean.mul_(1 - mom).add_(mom * mean.float())
                    self.bn.running_var.mul_(1 - mom).add_(mom * (var * m / max(m - 1.0, 1.0)).float())
                    self.bn.num_batches_tracked += 1
            var = var.float()
        else:
            mean, var = self.bn.running_mean.double(), self.bn.running_var
        scale = self.bn.weight * torch.rsqrt(var + self.bn.eps)
        off = (c0 - mean[None, :, None]).float()                          # [B,C',1]
        tsel = neighbour_minmax_target(y1, idx)                           # [B,2,C',N]
        pick = torch.where((scale >= 0)[None, :, None], tsel[:, 0], tsel[:, 1])
        z = torch.gather(y1, 2, pick) + y2 + off                          # the edge that survives max over k, minus the mean
        return self.act(z * scale[None, :, None] + self.bn.bias[None, :, None])


def reference_edgeconv(x: torch.Tensor, idx: torch.Tensor, conv: nn.Conv2d, bn: nn.BatchNorm2d, act: nn.Module) -> torch.Tensor:
    """The unfused block exactly as the reference composes it (used by the parity tests)."""
    _i, feat = ops.get_graph_features(x, idx, idx.shape[2])
    return act(bn(conv(feat))).max(dim=3)[0]
