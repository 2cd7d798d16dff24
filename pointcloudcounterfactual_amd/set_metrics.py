"""Scoring a generated SET of clouds against a reference set: all-pairs Chamfer / approximate-EMD matrices and the
three set metrics built on them -- minimum matching distance (MMD), coverage (COV) and leave-one-out 1-nearest-neighbour
accuracy (1-NNA).

The losses in ``losses`` are paired (sample ``b`` against sample ``b``); these metrics need the distance between EVERY
generated cloud and EVERY reference cloud.  ``pairwise_chamfer`` computes that ``[S,R]`` matrix with one kernel
(``pcc_chamfer_matrix``: each point-pair distance evaluated once for both directions); ``pairwise_emd`` drives the
existing cost-only ``pcc_match_cost`` over large index-selected pair batches.  The matrices are constants of the graph
(inputs are detached, there is no backward).  ``mmd_cov``, ``one_nn_accuracy`` are plain torch on the matrices and run
on any device; ties in their argmins go to the LOWEST index, explicitly -- duplicate clouds in a bank give bit-identical
columns, so ties are real, and ``torch.min`` on the GPU does not promise which index it returns.
"""

from __future__ import annotations

import torch

from pointcloudcounterfactual_amd import _lib, backend
from pointcloudcounterfactual_amd._lib import call, ptr

_L = _lib.lib
F32 = torch.float32

# pcc_match_cost numbers the samples of a call in the 12 bits its failure report has for them, and launches its finish
# kernel with the batch on grid.y: pair batches stay at or below 4095.
MAX_PAIRS_PER_CALL = 4095
# one cost-only call takes T(B) ~ 161 us + 8.3 us * B at N = 2048; at 512 pairs the fixed part is 4 % of
# the call (at 32 it is 38 %), and the two staged pair batches take 2 * 512 * 24 KB = 24 MB.
DEFAULT_PAIRS_PER_CALL = 512


def _check_bank(t: torch.Tensor, name: str) -> None:
    if t.dim() != 3 or t.size(2) != 3:
        raise ValueError(f'{name} must be [clouds, points, 3], got {tuple(t.shape)}')
    if t.size(1) < 1:
        raise ValueError(f'{name} must hold at least one point per cloud')


def _chamfer_host(a: torch.Tensor, b: torch.Tensor, mean: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """Dense float64 difference form, a bounded block of the [R,N,M] distances at a time; float64 results."""
    s, n, r, m = a.size(0), a.size(1), b.size(0), b.size(1)
    a64, b64 = a.double(), b.double()
    d_ab = torch.empty((s, r), dtype=torch.float64)
    d_ba = torch.empty((s, r), dtype=torch.float64)
    step = max(1, (1 << 22) // (n * m))  # bank clouds per block
    for i in range(s):
        for j0 in range(0, r, step):
            diff = a64[i, None, :, None, :] - b64[j0:j0 + step, None, :, :]  # [r', n, m, 3]
            d2 = (diff * diff).sum(-1)
            ab, ba = d2.min(2).values.sum(1), d2.min(1).values.sum(1)
            d_ab[i, j0:j0 + step] = ab / n if mean else ab
            d_ba[i, j0:j0 + step] = ba / m if mean else ba
    return d_ab, d_ba


def pairwise_chamfer(a: torch.Tensor, b: torch.Tensor | None = None, reduction: str = 'mean',
                     directional: bool = False) -> torch.Tensor | tuple[torch.Tensor, torch.Tensor]:
    """All-pairs Chamfer distances between the clouds ``a[S,N,3]`` and ``b[R,M,3]`` -> ``cd[S,R]`` float32,
    ``cd[i,j] = chamfer(a_i, b_j)``; ``directional=True`` returns its two terms ``(d_ab, d_ba)``:
    ``d_ab[i,j] = mean_p min_q |a_i,p - b_j,q|^2`` and ``d_ba[i,j] = mean_q min_p`` (``reduction='sum'``: plain sums).

    ``b=None`` scores ``a`` against itself: only ``i <= j`` is evaluated (clouds of more than 2048 points: every
    pair, one direction each), the matrix is bit-symmetric with an exactly zero diagonal and equals
    ``pairwise_chamfer(a, a.clone())`` bit for bit.

    GPU tensors run ``pcc_chamfer_matrix``: an entry is a fixed-order float32 sum of minima that are bit-equal to
    ``nn_distance``'s, independent of where the two clouds sit in their banks.  CPU tensors evaluate the dense float64
    difference form and round once.  A cloud with a NaN or infinite coordinate gives NaN in every entry it takes part
    in (GPU).  The result does not require grad."""
    if reduction not in ('mean', 'sum'):
        raise ValueError(f"reduction must be 'mean' or 'sum', got {reduction!r}")
    mean = reduction == 'mean'
    _check_bank(a, 'a')
    a = a.detach()
    if b is not None:
        _check_bank(b, 'b')
        b = b.detach()
    if a.device.type != 'cuda' and (b is None or b.device.type != 'cuda'):
        d_ab, d_ba = _chamfer_host(a, a if b is None else b, mean)
        if directional:
            return d_ab.float(), d_ba.float()
        return (d_ab + d_ba).float()
    d_ab, d_ba = _chamfer_matrix(a, b, mean)
    return (d_ab, d_ba) if directional else d_ab + d_ba


def _chamfer_matrix(a: torch.Tensor, b: torch.Tensor | None, mean: bool, want_ab: bool = True,
                    want_ba: bool = True) -> tuple[torch.Tensor | None, torch.Tensor | None]:
    """``pcc_chamfer_matrix`` on GPU banks (``b=None``: ``a`` against itself) -> ``(d_ab, d_ba)``; an output that is
    not wanted is passed as NULL and returned as ``None``."""
    dev = a.device
    a = a.contiguous()
    other = a if b is None else b.contiguous()
    s, n, r, m = a.size(0), a.size(1), other.size(0), other.size(1)
    d_ab = torch.empty((s, r), dtype=F32, device=dev) if want_ab else None
    d_ba = torch.empty((s, r), dtype=F32, device=dev) if want_ba else None
    call(_L.pcc_chamfer_matrix, 'pairwise_chamfer', dev, s, n, ptr(a, 'a', F32, dev), r, m, ptr(other, 'b', F32, dev),
         int(mean), ptr(d_ab, 'd_ab', F32, dev), ptr(d_ba, 'd_ba', F32, dev))
    return d_ab, d_ba


def pairwise_emd(a: torch.Tensor, b: torch.Tensor | None = None, normalize: bool = True,
                 pairs_per_call: int = DEFAULT_PAIRS_PER_CALL) -> torch.Tensor:
    """All-pairs approximate earth mover's distances -> ``emd[S,R]`` float32, ``emd[i,j] = match_cost(a_i, b_j)``
    (divided by ``N`` when ``normalize``), through the cost-only ``pcc_match_cost`` on index-selected batches of
    ``pairs_per_call`` pairs (at most ``MAX_PAIRS_PER_CALL``): the fixed latency of its launch chain is paid once per
    batch, not once per pair.  The approximate EMD is not symmetric, so ``b=None`` (``a`` against itself) still
    computes the full matrix.  GPU only, like ``match_cost``; the result does not require grad."""
    _check_bank(a, 'a')
    a = a.detach()
    if b is None:
        b = a
    else:
        _check_bank(b, 'b')
        b = b.detach()
    pairs_per_call = int(pairs_per_call)
    if not 1 <= pairs_per_call <= MAX_PAIRS_PER_CALL:
        raise ValueError(f'pairs_per_call must be in 1..{MAX_PAIRS_PER_CALL}, got {pairs_per_call}')
    dev = a.device
    a, b = a.contiguous(), b.contiguous()
    ptr(a, 'a', F32, dev)  # 'a must be a CUDA tensor', as match_cost raises it, before anything is staged
    ptr(b, 'b', F32, dev)
    s, n, r = a.size(0), a.size(1), b.size(0)
    out = torch.empty((s * r,), dtype=F32, device=dev)
    pair_index = torch.arange(s * r, device=dev)  # pair p is (p // r, p % r): the row-major order of the matrix
    rows, cols = torch.div(pair_index, r, rounding_mode='floor'), pair_index % r
    for p0 in range(0, s * r, pairs_per_call):
        batch = slice(p0, p0 + pairs_per_call)
        out[batch] = backend.MatchCostImplicit(a.index_select(0, rows[batch]), b.index_select(0, cols[batch]), False)[0]
    out = out.view(s, r)
    return out / n if normalize else out


def _argmin_lowest(d: torch.Tensor, dim: int) -> torch.Tensor:
    """Index of the minimum along ``dim``, the LOWEST index among equal minima (a NaN counts as the smallest value,
    as in ``torch.argmin``)."""
    key = torch.where(d != d, torch.full_like(d, float('-inf')), d)
    best = key.min(dim, keepdim=True).values
    shape = [1] * d.dim()
    shape[dim] = d.size(dim)
    index = torch.arange(d.size(dim), device=d.device).view(shape)
    return torch.where(key == best, index, d.size(dim)).min(dim).values


def mmd_cov(d: torch.Tensor) -> dict[str, torch.Tensor]:
    """``d[S,R]``: distances from ``S`` generated clouds (rows) to ``R`` reference clouds (columns) ->
    ``mmd`` = mean over references of the distance to their nearest generated cloud, ``mmd_smp`` = the same with the
    roles swapped, ``cov`` = the share of references that are the nearest reference (lowest index on ties) of at
    least one generated cloud."""
    if d.dim() != 2 or d.size(0) < 1 or d.size(1) < 1:
        raise ValueError(f'd must be a non-empty [S,R] matrix, got {tuple(d.shape)}')
    nearest_ref = _argmin_lowest(d, 1)
    covered = torch.zeros(d.size(1), dtype=torch.bool, device=d.device)
    covered[nearest_ref] = True
    return {'mmd': d.min(0).values.mean(), 'mmd_smp': d.min(1).values.mean(),
            'cov': covered.sum().to(d.dtype) / d.size(1)}


def one_nn_accuracy(d_ss: torch.Tensor, d_sr: torch.Tensor, d_rr: torch.Tensor) -> dict[str, torch.Tensor]:
    """Leave-one-out 1-nearest-neighbour classifier on the union of ``S`` generated and ``R`` reference clouds, items
    ordered generated first: distances ``[[d_ss, d_sr], [d_sr^T, d_rr]]`` with an infinite diagonal; every item takes
    the label of its nearest OTHER item (lowest index on ties).  -> ``acc`` and the confusion counts, 'positive' being
    generated: ``tp`` generated items labelled generated, ``fn`` generated labelled reference, ``fp`` reference
    labelled generated, ``tn`` reference labelled reference.  0.5 is the score of a generator whose clouds cannot be
    told from the references."""
    s, r = d_sr.shape if d_sr.dim() == 2 else (-1, -1)
    if d_ss.shape != (s, s) or d_rr.shape != (r, r) or s < 1 or r < 1:
        raise ValueError(f'expected d_ss[S,S], d_sr[S,R], d_rr[R,R], got {tuple(d_ss.shape)}, {tuple(d_sr.shape)}, '
                         f'{tuple(d_rr.shape)}')
    full = torch.cat([torch.cat([d_ss, d_sr], 1), torch.cat([d_sr.t(), d_rr], 1)], 0).clone()
    full.fill_diagonal_(float('inf'))
    labelled_generated = _argmin_lowest(full, 1) < s
    tp = labelled_generated[:s].sum()
    fp = labelled_generated[s:].sum()
    fn, tn = s - tp, r - fp
    return {'acc': (tp + tn).to(full.dtype) / (s + r), 'tp': tp, 'fp': fp, 'fn': fn, 'tn': tn}


def compute_all_metrics(sample: torch.Tensor, ref: torch.Tensor,
                        pairs_per_call: int = DEFAULT_PAIRS_PER_CALL) -> dict[str, torch.Tensor]:
    """``sample[S,N,3]`` generated clouds, ``ref[R,M,3]`` reference clouds (GPU) -> ``MMD-CD``, ``COV-CD``,
    ``1-NNA-CD``, ``MMD-EMD``, ``COV-EMD``, ``1-NNA-EMD`` from the six distance matrices (the two Chamfer self matrices
    through the self mode of ``pairwise_chamfer``)."""
    def emd(x: torch.Tensor, y: torch.Tensor | None = None) -> torch.Tensor:
        return pairwise_emd(x, y, pairs_per_call=pairs_per_call)

    out = {}
    for tag, pairwise in (('CD', pairwise_chamfer), ('EMD', emd)):
        d_sr = pairwise(sample, ref)
        scores = mmd_cov(d_sr)
        out[f'MMD-{tag}'] = scores['mmd']
        out[f'COV-{tag}'] = scores['cov']
        out[f'1-NNA-{tag}'] = one_nn_accuracy(pairwise(sample), d_sr, pairwise(ref))['acc']
    return out
