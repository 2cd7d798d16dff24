"""Float32 arithmetic of the HIP kernels restated exactly in torch, for the CPU paths that promise the kernels' bits
(``set_metrics.occupancy_grid``, ``neighbour_ops.ball_query``, ``neighbour_ops.kernel_point_influence``)."""

from __future__ import annotations

import torch


def fma32(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """``fmaf(a, b, c)`` of float32 tensors with ``a b >= 0`` and ``c >= 0``, exactly.  The product is exact in float64; the
    float64 sum is rounded TO ODD (its rounding error comes from the two-sum), after which the rounding to float32 is the
    one rounding of the fused operation -- a plain float64 sum would round twice."""
    p, c = a.double() * b.double(), c.double()
    s = p + c
    t = s - p
    err = (p - (s - t)) + (c - t)  # the exact sum is s + err
    bits = s.view(torch.int64)
    odd = (torch.where(err < 0, bits - 1, bits) | 1).view(torch.float64)  # truncate towards 0 (s > 0 here), then the sticky bit
    return torch.where(torch.isfinite(s) & (err != 0), odd, s).float()


def sqrt32(a: torch.Tensor) -> torch.Tensor:
    """``sqrtf(a)`` of a float32 tensor, correctly rounded.  Torch hands the float32 square root on the CPU to a vector-math
    library that may be an ulp off; the float64 root rounded to float32 is the correctly rounded one (53 >= 2 * 24 + 2 bits:
    the second rounding cannot move it)."""
    return torch.sqrt(a.double()).float()
