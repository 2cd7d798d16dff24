"""Scoring a generated SET of clouds against a reference set: all-pairs Chamfer / approximate-EMD matrices and the
three set metrics built on them -- minimum matching distance (MMD), coverage (COV) and leave-one-out 1-nearest-neighbour
accuracy (1-NNA) -- and the one set metric that needs no distance matrix: the Jensen-Shannon divergence (JSD) between the
voxel-occupancy distributions of the two sets (``occupancy_grid``, ``jsd_between_sets``).

The losses in ``losses`` are paired (sample ``b`` against sample ``b``); these metrics need the distance between EVERY
generated cloud and EVERY reference cloud.  ``pairwise_chamfer`` computes that ``[S,R]`` matrix with one kernel
(``pcc_chamfer_matrix``: each point-pair distance evaluated once for both directions); ``pairwise_emd`` drives the
existing cost-only ``pcc_match_cost`` over large index-selected pair batches.  The matrices are constants of the graph
(inputs are detached, there is no backward).  ``mmd_cov``, ``one_nn_accuracy`` are plain torch on the matrices and run
on any device; ties in their argmins go to the LOWEST index, explicitly -- duplicate clouds in a bank give bit-identical
columns, so ties are real, and ``torch.min`` on the GPU does not promise which index it returns.
"""

from __future__ import annotations

import math

import torch

from pointcloudcounterfactual_amd import _lib, backend
from pointcloudcounterfactual_amd._float32 import fma32 as _fma32
from pointcloudcounterfactual_amd._lib import call, ptr

_L = _lib.lib
F32 = torch.float32
I32 = torch.int32
I64 = torch.int64

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


# ---- voxel occupancy and the Jensen-Shannon divergence between two sets ---------------------------------------------

MAX_RESOLUTION = 128  # pcc_occupancy_grid's range


def _grid_args(resolution: int, in_sphere: bool, lo: float, extent: float) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The checks ``pcc_occupancy_grid`` makes on the grid, before anything is enqueued -> the float32 scalars of the
    rule ``(lo, inv, step)``, rounded as the library rounds them."""
    if isinstance(resolution, bool) or not isinstance(resolution, int) or not 2 <= resolution <= MAX_RESOLUTION:
        raise ValueError(f'resolution must be an int in [2, {MAX_RESOLUTION}], got {resolution!r}')
    if in_sphere and resolution < 3:
        raise ValueError('in_sphere needs resolution >= 3: at resolution 2 no grid point lies inside the sphere')
    lo32, extent32 = torch.tensor(float(lo), dtype=F32), torch.tensor(float(extent), dtype=F32)
    top = torch.tensor(float(resolution - 1), dtype=F32)
    inv, step = top / extent32, extent32 / top
    if not (math.isfinite(extent32.item()) and extent32.item() > 0 and math.isfinite(inv.item()) and inv.item() > 0 and step.item() > 0):
        raise ValueError(f'extent must be finite and > 0, got {extent!r}')
    if not math.isfinite(lo32.item()):
        raise ValueError(f'lo must be finite, got {lo!r}')
    return lo32, inv, step


def _in_sphere_columns(res: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The columns ``(i, j)`` that hold an in-sphere grid point, in flat order -> ``(i, j, klo)``; the interval of a
    column is ``[klo, res - 1 - klo]``.  Integers only."""
    r1 = res - 1
    a = 2 * torch.arange(res, dtype=I64) - r1
    rem = r1 * r1 - a[:, None] ** 2 - a[None, :] ** 2  # (2k - r1)^2 <= rem
    m = rem.clamp(min=0).double().sqrt().floor().to(I64)
    m = m - (m * m > rem).to(I64)
    m = m + ((m + 1) * (m + 1) <= rem).to(I64)  # floor(sqrt(rem)), settled in integers
    klo = (res - m) >> 1  # ceil((r1 - m) / 2)
    ci, cj = ((rem >= 0) & (klo <= r1 - klo)).nonzero(as_tuple=True)
    return ci, cj, klo[ci, cj]


def _nearest_in_sphere(points: torch.Tensor, ks: torch.Tensor, res: int, lo32: torch.Tensor, step: torch.Tensor) -> torch.Tensor:
    """The column rule of ``pcc_occupancy_grid`` for ``points[P,3]`` with separable ``k`` index ``ks[P]`` -> flat cells."""
    ci, cj, klo = _in_sphere_columns(res)
    grid = torch.arange(res, dtype=F32) * step + lo32  # g = (float)index * step + lo: two roundings
    out = torch.empty(points.size(0), dtype=I64)
    for p0 in range(0, points.size(0), 2048):
        p = points[p0:p0 + 2048]
        k = torch.minimum(torch.maximum(ks[p0:p0 + 2048, None], klo[None, :]), (res - 1 - klo)[None, :])
        dx, dy, dz = p[:, 0:1] - grid[ci][None, :], p[:, 1:2] - grid[cj][None, :], p[:, 2:3] - grid[k]
        d = _fma32(dz, dz, _fma32(dx, dx, dy * dy))  # pcc::sq3
        flat = ((ci * res + cj) * res)[None, :] + k
        nearest = d == d.min(1, keepdim=True).values
        out[p0:p0 + 2048] = torch.where(nearest, flat, res ** 3).min(1).values  # lowest index among equal distances
    return out


def _occupancy_host(clouds: torch.Tensor, res: int, in_sphere: bool, per_cloud: bool, lo32: torch.Tensor, inv: torch.Tensor,
                    step: torch.Tensor) -> torch.Tensor:
    """The rule of ``pcc_occupancy_grid`` in torch: the same float32 operations in the same order, then ``bincount``."""
    s, n = clouds.shape[:2]
    bins = res ** 3
    points = clouds.reshape(-1, 3)
    finite = torch.isfinite(points).all(1)
    cloud = torch.arange(s).repeat_interleave(n)[finite]
    points = points[finite]
    ijk = torch.floor((points - lo32) * inv + 0.5).clamp(0.0, float(res - 1)).to(I64)
    flat = (ijk[:, 0] * res + ijk[:, 1]) * res + ijk[:, 2]
    if in_sphere:
        outside = ((2 * ijk - (res - 1)) ** 2).sum(1) > (res - 1) ** 2
        flat[outside] = _nearest_in_sphere(points[outside], ijk[outside, 2], res, lo32, step)
    if per_cloud:
        return torch.bincount(cloud * bins + flat, minlength=s * bins).view(s, res, res, res)
    return torch.bincount(flat, minlength=bins).view(res, res, res)


def occupancy_grid(clouds: torch.Tensor, resolution: int = 28, in_sphere: bool = False, per_cloud: bool = False,
                   lo: float = -0.5, extent: float = 1.0) -> torch.Tensor:
    """Voxel occupancy counts of the clouds ``clouds[S,N,3]`` float32 on the grid of ``resolution`` points per axis over
    ``[lo, lo + extent]^3`` (the defaults: PointFlow's 28^3 grid on the unit cube) -> int64 ``[res,res,res]``, the number
    of points of the whole bank nearest to each grid point, or with ``per_cloud`` ``[S,res,res,res]``, one histogram per
    cloud.  ``in_sphere``: only the grid points inside the inscribed sphere count and every point goes to the nearest of
    those.  A point outside the cube lands in a border cell; a point with a NaN or infinite coordinate is counted nowhere,
    so the counts sum to the number of finite points.

    The rule, rounding by rounding, is ``pcc_occupancy_grid``'s (include/pcc_structural.h).  GPU tensors run that
    kernel; CPU tensors the same float32 operations in torch, so both give the same integers.  Integer adds only: the
    result does not depend on the schedule or on the order of clouds and points."""
    _check_bank(clouds, 'clouds')
    lo32, inv, step = _grid_args(resolution, in_sphere, lo, extent)
    if clouds.dtype != F32:
        raise RuntimeError(f'clouds must be {F32}, found {clouds.dtype}')
    clouds = clouds.detach()
    s, n, res = clouds.size(0), clouds.size(1), resolution
    shape = (s, res, res, res) if per_cloud else (res, res, res)
    if s == 0:
        return torch.zeros(shape, dtype=I64, device=clouds.device)
    if clouds.device.type != 'cuda':
        return _occupancy_host(clouds, res, bool(in_sphere), bool(per_cloud), lo32, inv, step)
    dev = clouds.device
    clouds = clouds.contiguous()
    xp = ptr(clouds, 'clouds', F32, dev)
    counts = torch.empty(shape, dtype=I32, device=dev)
    call(_L.pcc_occupancy_grid, 'occupancy_grid', dev, s, n, xp, res, float(lo), float(extent), int(bool(in_sphere)),
         int(bool(per_cloud)), ptr(counts, 'counts', I32, dev))
    return counts.to(I64)


def _entropy_bits(p: torch.Tensor) -> torch.Tensor:
    positive = p > 0
    return -torch.where(positive, p * torch.log2(torch.where(positive, p, torch.ones_like(p))), torch.zeros_like(p)).sum()


def jsd_from_counts(p_counts: torch.Tensor, q_counts: torch.Tensor) -> torch.Tensor:
    """Jensen-Shannon divergence, base 2, between the distributions ``P``, ``Q`` two count tensors of one shape stand for:
    ``H(M) - (H(P) + H(Q)) / 2`` with ``M = (P + Q) / 2`` and ``0 log 0 = 0``, in float64 on the counts' device, in
    ``[0, 1]``.  ``ValueError`` for counts that sum to 0."""
    if p_counts.shape != q_counts.shape:
        raise ValueError(f'the count tensors differ in shape: {tuple(p_counts.shape)} and {tuple(q_counts.shape)}')
    totals = p_counts.sum().item(), q_counts.sum().item()
    if min(totals) <= 0:
        raise ValueError('a set without a finite point has no occupancy distribution')
    p, q = p_counts.reshape(-1).double() / totals[0], q_counts.reshape(-1).double() / totals[1]
    jsd = _entropy_bits((p + q) / 2) - (_entropy_bits(p) + _entropy_bits(q)) / 2
    return jsd.clamp(0.0, 1.0)


def jsd_between_sets(sample: torch.Tensor, ref: torch.Tensor, resolution: int = 28, in_sphere: bool = True) -> torch.Tensor:
    """Jensen-Shannon divergence between the voxel-occupancy distributions of the generated clouds ``sample[S,N,3]`` and
    the reference clouds ``ref[R,M,3]`` on the unit-cube grid of ``occupancy_grid`` (Achlioptas et al. / PointFlow:
    28^3 grid points, those inside the inscribed sphere) -> a float64 scalar tensor in ``[0, 1]``: 0 for equal
    distributions, 1 for sets that share no cell.  One pass over the points; no distance matrix.  Symmetric, and
    invariant to the order of clouds and points, bit for bit.  ``ValueError`` if a set has no finite point."""
    return jsd_from_counts(occupancy_grid(sample, resolution, in_sphere), occupancy_grid(ref, resolution, in_sphere))


def compute_all_metrics(sample: torch.Tensor, ref: torch.Tensor, pairs_per_call: int = DEFAULT_PAIRS_PER_CALL,
                        with_jsd: bool = False) -> dict[str, torch.Tensor]:
    """``sample[S,N,3]`` generated clouds, ``ref[R,M,3]`` reference clouds (GPU) -> ``MMD-CD``, ``COV-CD``,
    ``1-NNA-CD``, ``MMD-EMD``, ``COV-EMD``, ``1-NNA-EMD`` from the six distance matrices (the two Chamfer self matrices
    through the self mode of ``pairwise_chamfer``); ``with_jsd`` adds ``JSD`` = ``jsd_between_sets(sample, ref)``."""
    def emd(x: torch.Tensor, y: torch.Tensor | None = None) -> torch.Tensor:
        return pairwise_emd(x, y, pairs_per_call=pairs_per_call)

    out = {}
    for tag, pairwise in (('CD', pairwise_chamfer), ('EMD', emd)):
        d_sr = pairwise(sample, ref)
        scores = mmd_cov(d_sr)
        out[f'MMD-{tag}'] = scores['mmd']
        out[f'COV-{tag}'] = scores['cov']
        out[f'1-NNA-{tag}'] = one_nn_accuracy(pairwise(sample), d_sr, pairwise(ref))['acc']
    if with_jsd:
        out['JSD'] = jsd_between_sets(sample, ref)
    return out
