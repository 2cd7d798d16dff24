"""Autograd surface of the structural losses.

``nn_distance`` / ``match_cost`` keep the reference's signatures and autograd behaviour
(``external/pytorch_structural_losses/structural_losses/nn_distance.py:9-43``,
``.../match_cost.py:11-50``); ``chamfer`` is the Chamfer loss the reference's GPU training path
computes with PyKeOps (``src/train/metrics_and_losses.py:21-41``), expressed through ``nn_distance``
(SURVEY.md section 8 row A7); ``torch_chamfer`` is the reference's CPU Chamfer (``:44-47``).
"""

from __future__ import annotations

import math
from typing import Any

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd import backend


class NNDistanceFunction(Function):
    """``(set1[B,N,3], set2[B,M,3]) -> (dist1[B,N], dist2[B,M])`` squared nearest-neighbour distances."""

    @staticmethod
    def forward(ctx: Any, *args: Any, **kwargs: Any) -> Any:
        set1, set2, *_ = args
        ctx.save_for_backward(set1, set2)
        dist1, idx1, dist2, idx2 = backend.NNDistance(set1, set2)
        ctx.idx1 = idx1  # indices are constants of the backward pass (nn_distance.py:22-24)
        ctx.idx2 = idx2
        return dist1, dist2

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> Any:
        set1, set2 = ctx.saved_tensors
        grad1, grad2 = backend.NNDistanceGrad(
            set1, set2, ctx.idx1, ctx.idx2, grad_outputs[0].contiguous(), grad_outputs[1].contiguous()
        )
        return grad1, grad2


class MatchCostFunction(Function):
    """``(set1[B,N,3], set2[B,M,3]) -> cost[B]`` approximate earth mover's distance.

    ``mode`` selects how the reference's ApproxMatch -> MatchCost / MatchCostGrad sequence (match_cost.py:25-27,
    39-42) is carried out; the three give the same cost and gradients up to float summation order:

    * ``'implicit'`` (default): ``match`` never exists.  One pass evaluates every match element in registers and
      accumulates the cost and -- when an input requires grad -- both gradients (they depend on the inputs only:
      the reference treats ``match`` as a constant); backward multiplies by ``grad_output``.  Saves the 4*B*M*N-byte
      tensor the reference keeps alive on ``ctx`` (512 MiB at B=32, N=2048) and two full passes over it.
    * ``'fused'``: ``match`` is materialised once (cost accumulated by the same pass) and read once in backward.
    * ``'reference'``: the reference's three backend calls, one after the other.
    """

    mode = 'implicit'

    @staticmethod
    def forward(ctx: Any, *args: torch.Tensor, **kwargs: Any) -> torch.Tensor:
        set1, set2, *_ = args
        mode = MatchCostFunction.mode
        ctx.mode = mode
        if mode == 'implicit':
            with_grad = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
            out = backend.MatchCostImplicit(set1, set2, with_grad)
            if with_grad:
                ctx.save_for_backward(out[1], out[2])
            return out[0]
        ctx.save_for_backward(set1, set2)
        if mode == 'fused':
            match, _temp, cost = backend.ApproxMatchCost(set1, set2)
        elif mode == 'reference':
            match, _temp = backend.ApproxMatch(set1, set2)
            cost = backend.MatchCost(set1, set2, match)
        else:
            raise ValueError(f'unknown MatchCostFunction.mode {mode!r}')
        ctx.match = match  # kept alive until backward, as the reference does (match_cost.py:26)
        return cost

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> tuple[torch.Tensor, torch.Tensor]:
        grad_output = grad_outputs[0]
        if ctx.mode == 'implicit':
            grad1, grad2 = ctx.saved_tensors
            scale = grad_output.unsqueeze(1).unsqueeze(2)
            return (grad1 * scale if ctx.needs_input_grad[0] else None,
                    grad2 * scale if ctx.needs_input_grad[1] else None)
        set1, set2 = ctx.saved_tensors
        if ctx.mode == 'fused':  # upstream gradient folded into the reduction of the gradient kernel
            grad1, grad2 = backend.MatchCostGradScaled(set1, set2, ctx.match, grad_output.contiguous().float())
            return grad1, grad2
        grad1, grad2 = backend.MatchCostGrad(set1, set2, ctx.match)
        scale = grad_output.unsqueeze(1).unsqueeze(2)
        return grad1 * scale, grad2 * scale

    @classmethod
    def apply(cls, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:  # type: ignore[override]
        return super().apply(x, y)  # type: ignore[return-value]


nn_distance = NNDistanceFunction.apply
match_cost = MatchCostFunction.apply


class ChamferFunction(Function):
    """``(t1[B,N,3], t2[B,M,3], mean) -> loss[B]``: nearest-neighbour search, loss reduction and -- in backward --
    the spreading of ``grad_loss[b]`` over the points, all inside the library (two launches forward, one backward)
    instead of six small elementwise / reduction launches around ``nn_distance``."""

    @staticmethod
    def forward(ctx: Any, *args: Any, **kwargs: Any) -> torch.Tensor:
        t1, t2, mean = args
        loss, _d1, idx1, _d2, idx2 = backend.ChamferLoss(t1, t2, bool(mean))
        ctx.save_for_backward(t1, t2, idx1, idx2)  # indices are constants of the backward pass
        ctx.mean = bool(mean)
        return loss

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> Any:
        t1, t2, idx1, idx2 = ctx.saved_tensors
        g = grad_outputs[0]
        grad1, grad2 = backend.ChamferLossGrad(t1, t2, idx1, idx2, g if g.dtype == torch.float32 else g.float(), ctx.mean)
        return grad1, grad2, None


def chamfer(t1: torch.Tensor, t2: torch.Tensor, reduction: str = 'mean') -> torch.Tensor:
    """Chamfer loss ``[B]`` on the accelerator.

    ``reduction='mean'`` reproduces ``pykeops_chamfer`` (metrics_and_losses.py:21-41):
    ``dist2.mean(1) + dist1.mean(1)``; ``'sum'`` reproduces the scale of ``torch_chamfer`` (:44-47).
    Gradients flow through the gathered nearest neighbours only (indices are constants), as in both.
    Equal to the same expression written with ``nn_distance`` (tests/test_gpu_structural.py) up to the order of
    the float sums.
    """
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    return ChamferFunction.apply(t1, t2, reduction == 'mean')


class ChamferEMDFunction(Function):
    """``(t1[B,N,3], t2[B,M,3], mean) -> (chamfer[B], emd[B])``: the two terms of the reference's ``ChamferEMD``
    reconstruction loss (``src/train/metrics_and_losses.py:70-79``: Chamfer and ``match_cost`` on the SAME pair of
    clouds) as one autograd node.  Same kernels and the same bits as ``chamfer(t1, t2)`` and ``match_cost(t1, t2)``;
    what the fusion buys is scheduling:

    * forward: the two losses do not depend on each other, and the approximate EMD is a chain of 19 dependent
      launches whose late passes are latency-bound and leave most of the chip idle.  One library call
      (``pcc_chamfer_emd``) enqueues the nearest-neighbour search (VALU-bound, one big launch) on an internal stream
      that starts when the chain reaches those passes, and joins it before returning.
    * backward: one launch (``pcc_chamfer_emd_grad``) writes the total gradient -- Chamfer's scatter term plus the
      saved ``match_cost`` gradients times their upstream scalar -- instead of three launches and two accumulations.
    """

    @staticmethod
    def forward(ctx: Any, *args: Any, **kwargs: Any) -> Any:
        t1, t2, mean = args
        with_grad = bool(ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        out = backend.ChamferEMD(t1, t2, bool(mean), with_grad)
        if with_grad:
            ctx.save_for_backward(t1, t2, out[1], out[2], out[4], out[5])
        ctx.mean = bool(mean)
        return out[0], out[3]

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> Any:
        t1, t2, idx1, idx2, e1, e2 = ctx.saved_tensors
        gc, ge = grad_outputs
        gc = gc if gc.dtype == torch.float32 else gc.float()
        ge = ge if ge.dtype == torch.float32 else ge.float()
        grad1, grad2 = backend.ChamferEMDGrad(t1, t2, idx1, idx2, gc, ctx.mean, e1, e2, ge)
        return (grad1 if ctx.needs_input_grad[0] else None, grad2 if ctx.needs_input_grad[1] else None, None)


def chamfer_emd(t1: torch.Tensor, t2: torch.Tensor, reduction: str = 'mean') -> tuple[torch.Tensor, torch.Tensor]:
    """``(chamfer(t1, t2, reduction), match_cost(t1, t2))`` as one autograd node (see ``ChamferEMDFunction``): the
    reference's ``ChamferEMD`` reconstruction loss is their sum (``metrics_and_losses.py:70-79``)."""
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    return ChamferEMDFunction.apply(t1, t2, reduction == 'mean')


def torch_square_distance(t1: torch.Tensor, t2: torch.Tensor) -> torch.Tensor:
    """Expanded-form squared distances ``[B,N,M]`` (reference ``src/utils/neighbour_ops.py:43-50``)."""
    t2 = t2.transpose(-1, -2)
    dist = -2 * torch.matmul(t1, t2)
    dist += torch.sum(t1**2, -1, keepdim=True)
    dist += torch.sum(t2**2, -2, keepdim=True)
    return dist


def torch_chamfer(t1: torch.Tensor, t2: torch.Tensor) -> torch.Tensor:
    """The reference's CPU Chamfer (sum over points; ``metrics_and_losses.py:44-47``).  This is the
    reference's own host path for ``user.cpu`` runs (BASELINE config 1), not a fallback of ``chamfer``."""
    dist = torch_square_distance(t1, t2)
    return torch.min(dist, dim=-1)[0].sum(1) + torch.min(dist, dim=-2)[0].sum(1)


def random_directions(p: int, device: torch.device | str, generator: torch.Generator | None = None) -> torch.Tensor:
    """``[p,3]`` float32 directions on ``device``: Gaussian rows, normalised (uniform on the sphere).  Drawn on the
    generator's device when one is given."""
    device = torch.device(device)
    raw = torch.randn(p, 3, generator=generator, device=device if generator is None else generator.device)
    return torch.nn.functional.normalize(raw, dim=1).to(device)


def _sw_forward(t1: torch.Tensor, t2: torch.Tensor, theta: torch.Tensor) -> tuple[torch.Tensor, ...]:
    """The contract of ``pcc_sliced_wasserstein`` (include/pcc_structural.h) in torch operations, none of which fuses a
    product with a sum: -> (cost[B], cost_p[B,P], d[B,P,N], perm1[B,P,N], perm2[B,P,N], inv)."""
    n, p = t1.size(1), theta.size(0)

    def sorted_projection(t: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        v, th = t[:, None, :, :], theta[None, :, None, :]
        proj = (v[..., 0] * th[..., 0] + v[..., 1] * th[..., 1]) + v[..., 2] * th[..., 2]
        proj = torch.where(proj == 0, torch.zeros_like(proj), proj)  # -0 counts as +0
        return torch.sort(proj, dim=2, stable=True)  # NaN sorts above +inf, equal values by ascending index

    (a, perm1), (b, perm2) = sorted_projection(t1), sorted_projection(t2)
    d = a - b
    size = 1 << max(n - 1, 0).bit_length()
    e = torch.zeros(d.shape[:2] + (size,), dtype=d.dtype)
    e[..., :n] = d * d
    while size > 1:  # the halving tree
        size //= 2
        e = e[..., :size] + e[..., size:2 * size]
    cost_p = e[..., 0]
    total = cost_p[:, 0]
    for k in range(1, p):
        total = total + cost_p[:, k]
    inv = torch.tensor(1.0 / (float(n) * float(p)), dtype=torch.float64).to(torch.float32)
    return total * inv, cost_p, d, perm1, perm2, inv


class TorchSlicedWassersteinFunction(Function):
    """The CPU path of ``sliced_wasserstein`` as one autograd node: ``(t1, t2, directions) -> cost[B]``; the backward
    holds the permutations constant, as the library does."""

    @staticmethod
    def forward(ctx: Any, *args: Any, **kwargs: Any) -> torch.Tensor:
        t1, t2, theta = args
        cost, _cost_p, d, perm1, perm2, inv = _sw_forward(t1, t2, theta)
        ctx.save_for_backward(d, perm1, perm2, theta, inv)
        return cost

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> Any:
        d, perm1, perm2, theta, inv = ctx.saved_tensors
        g = grad_outputs[0]
        scale = ((g if g.dtype == torch.float32 else g.float()) * (2 * inv))[:, None, None]

        def grad(perm: torch.Tensor, diff: torch.Tensor) -> torch.Tensor:
            by_point = torch.empty_like(diff).scatter_(2, perm, diff)  # [B,P,N]: rank -> point, a permutation
            return torch.einsum('bpn,pc->bnc', by_point, theta) * scale

        return (grad(perm1, d) if ctx.needs_input_grad[0] else None, grad(perm2, -d) if ctx.needs_input_grad[1] else None, None)


def torch_sliced_wasserstein(t1: torch.Tensor, t2: torch.Tensor, directions: torch.Tensor,
                             return_per_direction: bool = False) -> Any:
    """Sliced Wasserstein distance ``[B]`` of CPU clouds ``t1[B,N,3]``, ``t2[B,N,3]`` along ``directions[P,3]``: the
    contract of ``pcc_sliced_wasserstein`` in torch; ``cost`` and, with ``return_per_direction``, ``cost_p[B,P]`` (no
    gradient) equal the library's word for word."""
    for name, t in (('t1', t1), ('t2', t2), ('directions', directions)):
        if t.dtype != torch.float32:
            raise RuntimeError(f'{name} must be torch.float32, found {t.dtype}')
    if t1.dim() != 3 or t1.size(2) != 3 or t2.shape != t1.shape or t1.size(1) < 1:
        raise ValueError(f'clouds must be [B,N,3] of one shape with N >= 1, got {tuple(t1.shape)} and {tuple(t2.shape)}')
    if directions.dim() != 2 or directions.size(1) != 3 or directions.size(0) < 1:
        raise ValueError(f'directions must be [P,3] with P >= 1, got {tuple(directions.shape)}')
    cost = TorchSlicedWassersteinFunction.apply(t1, t2, directions)
    if return_per_direction:
        with torch.no_grad():
            return cost, _sw_forward(t1, t2, directions)[1]
    return cost


class SlicedWassersteinFunction(Function):
    """``(t1[B,N,3], t2[B,N,3], directions[P,3]) -> cost[B]`` on the accelerator, one autograd node: the forward call
    (``pcc_sliced_wasserstein``) also computes the unscaled gradient of every input that asks for one -- they come out of
    the sort the cost needs -- and the backward multiplies by the upstream ``g[b]``."""

    @staticmethod
    def forward(ctx: Any, *args: Any, **kwargs: Any) -> torch.Tensor:
        t1, t2, theta = args
        need1, need2 = bool(ctx.needs_input_grad[0]), bool(ctx.needs_input_grad[1])
        cost, _cost_p, g1, g2 = backend.SlicedWasserstein(t1, t2, theta, need1, need2)
        ctx.save_for_backward(*(g for g in (g1, g2) if g is not None))
        ctx.needs = (need1, need2)
        return cost

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> Any:
        saved = list(ctx.saved_tensors)
        g = grad_outputs[0]
        scale = (g if g.dtype == torch.float32 else g.float())[:, None, None]
        grad1 = saved.pop(0) * scale if ctx.needs[0] else None
        grad2 = saved.pop(0) * scale if ctx.needs[1] else None
        return grad1, grad2, None


def sliced_wasserstein(t1: torch.Tensor, t2: torch.Tensor, n_projections: int = 128, directions: torch.Tensor | None = None,
                       generator: torch.Generator | None = None) -> torch.Tensor:
    """Sliced Wasserstein loss ``[B]`` between clouds of equal size ``t1[B,N,3]`` and ``t2[B,N,3]``: the mean over the
    directions and the points of the squared difference of the two clouds' sorted projections -- the squared
    2-Wasserstein distance of the projected clouds, a transport distance whose cost is a sort.  ``directions[P,3]`` is used
    as given (not normalised); without it ``random_directions(n_projections, t1.device, generator)`` is drawn per call.
    Gradients flow to the clouds with the sorted order held constant; the directions get none.  CPU tensors take
    ``torch_sliced_wasserstein``, the same contract in torch (N <= 8192 on the accelerator)."""
    if directions is None:
        directions = random_directions(n_projections, t1.device, generator)
    if t1.device.type == 'cpu':
        return torch_sliced_wasserstein(t1, t2, directions)
    return SlicedWassersteinFunction.apply(t1, t2, directions)


def sinkhorn_schedule(blur: float, scaling: float, diameter: float) -> list[float]:
    """GeomLoss's epsilon-scaling for the cost ``|u - v|^2 / 2``: the temperatures ``[diameter^2]``, then ``exp(v)`` for ``v`` in
    ``arange(2 log diameter, 2 log blur, 2 log scaling)``, then ``[blur^2]``.  (0.05, 0.5, 2.0) gives 4, 4, 1, 0.25, 0.0625,
    0.015625, 0.00390625, 0.0025: 8 steps, 10 all-pairs rounds."""
    if not (blur > 0 and diameter > 0 and 0 < scaling < 1) or not all(math.isfinite(v) for v in (blur, scaling, diameter)):
        raise ValueError(f'sinkhorn_schedule: need blur > 0, diameter > 0 and 0 < scaling < 1, got {blur}, {scaling}, {diameter}')
    start, stop, step = 2 * math.log(diameter), 2 * math.log(blur), 2 * math.log(scaling)
    count = max(0, math.ceil((stop - start) / step))  # (numpy's arange)
    return [diameter**2] + [math.exp(start + i * step) for i in range(count)] + [blur**2]


def _halving_tree(e: torch.Tensor) -> torch.Tensor:
    """The contract's tree over the last axis: pad with +0 to a power of two, then ``e_i += e_{i+h}`` for h = L/2 .. 1."""
    n = e.size(-1)
    size = 1 << max(n - 1, 0).bit_length()
    pad = torch.zeros(e.shape[:-1] + (size,), dtype=e.dtype, device=e.device)
    pad[..., :n] = e
    while size > 1:
        size //= 2
        pad = pad[..., :size] + pad[..., size:2 * size]
    return pad[..., 0]


def _sk_forward(t1: torch.Tensor, t2: torch.Tensor, eps: list[float], debias: bool) -> tuple[torch.Tensor, ...]:
    """The contract of ``pcc_sinkhorn`` (include/pcc_structural.h) in float32 torch, dense: -> (cost[B], pot1[B,N], pot2[B,M],
    grad1[B,N,3], grad2[B,M,3]), the gradients for an upstream gradient of 1."""
    n, m = t1.size(1), t2.size(1)

    def pairs(u: torch.Tensor, v: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        diff = u[:, :, None, :] - v[:, None, :, :]  # coordinate differences, never the expanded form
        return diff, 0.5 * (diff * diff).sum(-1)

    def softmin(e: float, cost: torch.Tensor, h: torch.Tensor | None) -> torch.Tensor:
        arg = -cost / e if h is None else (h[:, None, :] - cost) / e
        return -e * torch.logsumexp(arg - math.log(cost.size(2)), dim=2)  # (subtracts the largest term)

    (dxy, cxy), (dyx, cyx) = pairs(t1, t2), pairs(t2, t1)  # (each its own tensor: the four scans are one function of their arguments)
    f, g = softmin(eps[0], cxy, None), softmin(eps[0], cyx, None)
    if debias:
        dxx, cxx = pairs(t1, t1)
        dyy, cyy = pairs(t2, t2)
        p, q = softmin(eps[0], cxx, None), softmin(eps[0], cyy, None)
    for e in eps:
        f, g = 0.5 * (f + softmin(e, cxy, g)), 0.5 * (g + softmin(e, cyx, f))
        if debias:
            p, q = 0.5 * (p + softmin(e, cxx, p)), 0.5 * (q + softmin(e, cyy, q))
    e = eps[-1]

    def plan_grad(cost: torch.Tensor, diff: torch.Tensor, h: torch.Tensor) -> torch.Tensor:
        return torch.einsum('bij,bijc->bic', torch.softmax((h[:, None, :] - cost) / e, dim=2), diff)

    pot1, pot2 = softmin(e, cxy, g), softmin(e, cyx, f)
    grad1, grad2 = plan_grad(cxy, dxy, g), plan_grad(cyx, dyx, f)
    if debias:
        pot1, pot2 = pot1 - softmin(e, cxx, p), pot2 - softmin(e, cyy, q)
        grad1, grad2 = grad1 - plan_grad(cxx, dxx, p), grad2 - plan_grad(cyy, dyy, q)
    inv_n = torch.tensor(1.0 / n, dtype=torch.float64).to(torch.float32)
    inv_m = torch.tensor(1.0 / m, dtype=torch.float64).to(torch.float32)
    cost = inv_n * _halving_tree(pot1) + inv_m * _halving_tree(pot2)
    return cost, pot1, pot2, inv_n * grad1, inv_m * grad2


def _sk_check(t1: torch.Tensor, t2: torch.Tensor, eps: list[float] | None) -> None:
    for name, t in (('t1', t1), ('t2', t2)):
        if t.dtype != torch.float32:
            raise RuntimeError(f'{name} must be torch.float32, found {t.dtype}')
    if t1.dim() != 3 or t2.dim() != 3 or t1.size(2) != 3 or t2.size(2) != 3 or t1.size(0) != t2.size(0) or t1.size(1) < 1 or t2.size(1) < 1:
        raise ValueError(f'clouds must be [B,N,3] and [B,M,3] with N, M >= 1, got {tuple(t1.shape)} and {tuple(t2.shape)}')
    if eps is not None and (not 1 <= len(eps) <= 256 or not all(math.isfinite(e) and e > 0 for e in eps)):
        raise ValueError('eps must hold 1 to 256 finite temperatures > 0')


class _SinkhornBase(Function):
    """``(t1[B,N,3], t2[B,M,3], eps, debias, potentials, grad_mode) -> (cost[B], pot1, pot2)``, one autograd node: the forward
    call also computes the unscaled gradient of every input that asks for one (the closed form needs the final round's
    softmax rows, no stored plan), and the backward multiplies by the upstream ``g[b]``.  ``grad_mode`` is the caller's
    ``torch.is_grad_enabled()``: inside ``forward`` it always reads False, and ``needs_input_grad`` stays True under
    ``no_grad``, where no gradient will ever be asked for.  The potentials carry no gradient."""

    @staticmethod
    def run(t1: torch.Tensor, t2: torch.Tensor, eps: list[float], debias: bool, need1: bool, need2: bool, potentials: bool) -> Any:
        raise NotImplementedError

    @classmethod
    def forward(cls, ctx: Any, *args: Any, **kwargs: Any) -> Any:
        t1, t2, eps, debias, potentials, grad_mode = args
        need1, need2 = bool(grad_mode and ctx.needs_input_grad[0]), bool(grad_mode and ctx.needs_input_grad[1])
        cost, p1, p2, g1, g2 = cls.run(t1, t2, eps, debias, need1, need2, potentials)
        ctx.save_for_backward(*(g for g in (g1, g2) if g is not None))
        ctx.needs = (need1, need2)
        if potentials:
            ctx.mark_non_differentiable(p1, p2)
        return cost, p1, p2

    @staticmethod
    def backward(ctx: Any, *grad_outputs: Any) -> Any:
        saved = list(ctx.saved_tensors)
        g = grad_outputs[0]
        scale = (g if g.dtype == torch.float32 else g.float())[:, None, None]
        grad1 = saved.pop(0) * scale if ctx.needs[0] else None
        grad2 = saved.pop(0) * scale if ctx.needs[1] else None
        return grad1, grad2, None, None, None, None


class TorchSinkhornFunction(_SinkhornBase):
    """The CPU path of ``sinkhorn_divergence``: the same contract and the same gradient convention in dense float32 torch."""

    @staticmethod
    def run(t1: torch.Tensor, t2: torch.Tensor, eps: list[float], debias: bool, need1: bool, need2: bool, potentials: bool) -> Any:
        cost, p1, p2, g1, g2 = _sk_forward(t1, t2, eps, debias)
        return cost, p1 if potentials else None, p2 if potentials else None, g1 if need1 else None, g2 if need2 else None


class SinkhornFunction(_SinkhornBase):
    """``sinkhorn_divergence`` on the accelerator (``pcc_sinkhorn``)."""

    @staticmethod
    def run(t1: torch.Tensor, t2: torch.Tensor, eps: list[float], debias: bool, need1: bool, need2: bool, potentials: bool) -> Any:
        return backend.Sinkhorn(t1, t2, eps, debias, need1, need2, potentials)


def torch_sinkhorn(t1: torch.Tensor, t2: torch.Tensor, eps: list[float], debias: bool = True, return_potentials: bool = False) -> Any:
    """Sinkhorn divergence ``[B]`` of CPU clouds ``t1[B,N,3]``, ``t2[B,M,3]`` along the temperatures ``eps``: the contract of
    ``pcc_sinkhorn`` in dense float32 torch (``torch.logsumexp``; four ``[B,N,M]``-sized tensors), with the library's
    gradient convention as an explicit autograd node.  With ``return_potentials``: ``(cost, pot1[B,N], pot2[B,M])``."""
    eps = [float(e) for e in eps]
    _sk_check(t1, t2, eps)
    cost, p1, p2 = TorchSinkhornFunction.apply(t1, t2, eps, bool(debias), bool(return_potentials), torch.is_grad_enabled())
    return (cost, p1, p2) if return_potentials else cost


def sinkhorn_divergence(t1: torch.Tensor, t2: torch.Tensor, blur: float = 0.05, scaling: float = 0.5, diameter: float | None = None,
                        eps: list[float] | None = None, debias: bool = True, return_potentials: bool = False) -> Any:
    """Debiased Sinkhorn divergence ``[B]`` between clouds ``t1[B,N,3]`` and ``t2[B,M,3]`` (N and M independent) with uniform
    weights and the cost ``|u - v|^2 / 2``: GeomLoss's ``SamplesLoss("sinkhorn", p=2, blur, scaling)``.  ``blur`` is a length:
    the resolution below which the loss stops telling points apart; ``scaling`` is the ratio between successive
    temperatures' lengths (closer to 1: more rounds, closer to the converged value).  The loss is exactly 0 between a cloud
    and itself.  ``eps``, when given, is the list of temperatures (squared lengths) and is used as is; otherwise it is
    ``sinkhorn_schedule(blur, scaling, diameter)``.  ``diameter=None`` takes the largest per-axis extent over both clouds
    and the whole batch, which costs ONE HOST SYNCHRONISATION per call: pass a constant (the data's known extent) when
    training.  ``debias=False`` returns the plain entropic cost OT_eps.  One autograd node: the gradients hold the other
    cloud and the pre-final potentials constant (GeomLoss's convention) and come out of the forward call.  With
    ``return_potentials``: ``(cost, pot1[B,N], pot2[B,M])``, ``cost[b] = mean(pot1[b]) + mean(pot2[b])``; the potentials carry no
    gradient.  CPU tensors take ``torch_sinkhorn``, the same contract in dense torch."""
    _sk_check(t1, t2, None)
    if eps is None:
        if diameter is None:
            both = torch.cat((t1.detach().reshape(-1, t1.size(-1)), t2.detach().reshape(-1, t2.size(-1))))
            diameter = float((both.max(0).values.double() - both.min(0).values.double()).max())  # (the host synchronisation)
            if not diameter > 0:
                diameter = float(blur)  # (all points equal: one temperature, blur^2, twice)
        eps = sinkhorn_schedule(float(blur), float(scaling), float(diameter))
    eps = [float(e) for e in eps]
    _sk_check(t1, t2, eps)
    fn = TorchSinkhornFunction if t1.device.type == 'cpu' else SinkhornFunction
    cost, p1, p2 = fn.apply(t1, t2, eps, bool(debias), bool(return_potentials), torch.is_grad_enabled())
    return (cost, p1, p2) if return_potentials else cost
