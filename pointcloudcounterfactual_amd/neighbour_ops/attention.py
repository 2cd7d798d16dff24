# ---- vector attention: a softmax over the valid slots of a list, a grouped weighted sum of gathered values ------------------

from __future__ import annotations

import numbers
from typing import Any, Callable

import torch
from torch.autograd import Function

from pointcloudcounterfactual_amd._lib import call, ptr
from pointcloudcounterfactual_amd.neighbour_ops._args import (F32, I64, _L, _canonical_nan, _features_arg, _float32, _list_arg, _list_on,
                                                              _list_slots, _same_device, _slot_values, _valid_slots, _zero)
from pointcloudcounterfactual_amd.neighbour_ops.grouping import group_points

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


def torch_neighbour_softmax(logits: torch.Tensor, idx: torch.Tensor, n: int) -> torch.Tensor:
    """The rule of ``pcc_neighbour_softmax`` in float32 torch operations (no autograd): the maximum over the valid slots,
    ``exp`` of the rounded difference, the sum over the valid slots in slot order, one division."""
    valid = _valid_slots(idx, n)[:, None]  # [B,1,M,k]
    mx = torch.where(valid, logits, torch.full((), float('-inf'), dtype=logits.dtype, device=logits.device)).amax(-1, keepdim=True)
    e = torch.where(valid, torch.exp(logits - mx), _zero(logits))
    s = torch.zeros_like(e[..., 0])
    for j in range(idx.shape[2]):
        s = torch.where(valid[..., j], s + e[..., j], s)
    return torch.where(valid, _canonical_nan(e / s[..., None]), _zero(logits))


def torch_neighbour_softmax_bwd(attn: torch.Tensor, idx: torch.Tensor, n: int, grad_attn: torch.Tensor) -> torch.Tensor:
    """The rule of ``pcc_neighbour_softmax_bwd``: ``d`` summed over the valid slots in slot order, ``attn * (ga - d)``."""
    valid = _valid_slots(idx, n)[:, None]
    d = torch.zeros_like(attn[..., 0])
    for j in range(idx.shape[2]):
        d = torch.where(valid[..., j], d + attn[..., j] * grad_attn[..., j], d)
    return torch.where(valid, _canonical_nan(attn * (grad_attn - d[..., None])), _zero(attn))


def torch_aggregate_points(x: torch.Tensor, idx: torch.Tensor, weights: torch.Tensor, rel: torch.Tensor | None = None) -> torch.Tensor:
    """The rule of ``pcc_aggregate_points`` in float32 torch operations (no autograd): per slot a gather, the sum with
    ``rel``, a product and an addition, in slot order."""
    b, c, n = x.shape
    s = c // weights.shape[1]
    valid, safe = _list_slots(idx, n)
    v = _slot_values(x, safe, rel)
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
    valid, safe = _list_slots(idx, n)
    gx = gw = gr = None
    if want[0] or want[2]:
        prod = torch.where(valid[:, None], weights.repeat_interleave(s, dim=1) * grad_out[..., None], _zero(x))
        if want[2]:
            gr = _canonical_nan(prod)
        if want[0]:
            gx = torch.zeros_like(x).scatter_add_(2, safe.reshape(b, 1, m * k).expand(-1, c, -1), prod.reshape(b, c, m * k))
    if want[1]:
        v = _slot_values(x, safe, rel).view(b, g, s, m, k)
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
