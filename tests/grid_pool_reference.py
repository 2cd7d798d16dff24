"""Numpy reference of grid pooling (``pcc_grid_cluster``, ``pcc_segment_pool`` / ``_bwd``, include/pcc_neighbour.h): loops that
follow the contract operation by operation (every float operation is on float32 operands, so each is rounded once, as the
contract writes it), and the clouds and feature words the CPU and GPU tests share.  The index a partition starts from is
``tests/voxel_reference.py``'s."""

import numpy as np

from tests import voxel_reference as vref

F32 = np.float32
MEAN, SUM, MAX = 0, 1, 2
MODES = {'mean': MEAN, 'sum': SUM, 'max': MAX}
# The dispatch of csrc/grid_pool.hip, for the tests that walk its boundaries: CB channels per thread; a run of more than
# LONG_RUN points goes to the kernel with the channels across the 64 lanes of a wave; SCAN_THREADS threads scan a cloud.
# Rows of up to LDS_MAX_N floats are staged in LDS, CB of them per workgroup up to LDS_ROWS_N[CB] points; longer rows are
# gathered from global memory.
# The backward stages rows of m gradients (and m indices, for max) the same way, up to LDS_MAX_BWD_M slots.
CB, LONG_RUN, SCAN_THREADS, LDS_MAX_N, LDS_MAX_BWD_M = 8, 64, 1024, 40000, 20000
LDS_ROWS_N = {8: 2048, 4: 4096, 2: 8192}


def _rows(words):
    """Rows of ``words`` floats a workgroup stages: 8, 4 or 2 while they fit 64 KB (LDS_ROWS_N), one above."""
    return next((cb for cb in (8, 4, 2) if words <= LDS_ROWS_N[cb]), 1)


def pool_kernels(n):
    """The exact launch-profile names of ``pcc_segment_pool`` on clouds of n points: the LDS kernel in its rows-per-workgroup
    instantiation up to LDS_MAX_N, the gathering kernel above; the long-run kernel is launched wherever a run can be longer
    than LONG_RUN (n > LONG_RUN)."""
    names = {f'seg_pool_lds_kernel<{_rows(n)}>' if n <= LDS_MAX_N else 'seg_pool_kernel'}
    return names | ({'seg_long_kernel'} if n > LONG_RUN else set())


def pool_bwd_kernel(m, mode):
    """... of ``pcc_segment_pool_bwd`` with m slots: rows of m gradients (and m indices, for max)."""
    return f'seg_pool_bwd_lds_kernel<{_rows(m * (2 if mode == MAX else 1))}>' if m <= LDS_MAX_BWD_M else 'seg_pool_bwd_kernel'


def grid_cluster(cell, order, m):
    """``(cluster[b,n], seg[b,m+1], count[b])`` int32 from ``pcc_voxel_index``'s ``cell`` and ``order``."""
    b, n = cell.shape
    cluster = np.full((b, n), -1, dtype=np.int32)
    seg = np.zeros((b, m + 1), dtype=np.int32)
    count = np.zeros(b, dtype=np.int32)
    for s in range(b):
        rank, last, finite, end = -1, None, 0, None
        for pos in range(n):
            p = order[s, pos]
            v = cell[s, p]
            if v < 0:
                continue
            finite += 1
            if v != last:
                rank, last = rank + 1, v
                if rank < m:
                    seg[s, rank] = pos
                elif rank == m:
                    end = pos  # the end of the last kept run
            if rank < m:
                cluster[s, p] = rank
        count[s] = rank + 1
        seg[s, min(rank + 1, m):] = finite if end is None else end
    return cluster, seg, count


def segment_pool(x, order, seg, mode):
    """``(out[b,c,m] float32, arg[b,c,m] int32)``; ``arg`` is all -1 unless ``mode`` is MAX."""
    b, c, _ = x.shape
    m = seg.shape[1] - 1
    out = np.zeros((b, c, m), dtype=F32)
    arg = np.full((b, c, m), -1, dtype=np.int32)
    with np.errstate(all='ignore'):
        for s in range(b):
            for r in range(m):
                run = order[s, seg[s, r]:seg[s, r + 1]]
                if len(run) == 0:
                    continue
                if mode == MAX:  # (the c channels side by side: each its own chain)
                    best, at = x[s, :, run[0]].copy(), np.full(c, run[0], dtype=np.int32)
                    for p in run[1:]:
                        v = x[s, :, p]
                        take = ~np.isnan(best) & (np.isnan(v) | (v > best))
                        best, at = np.where(take, v, best), np.where(take, p, at).astype(np.int32)
                    arg[s, :, r] = at
                    out[s, :, r].view(np.uint32)[:] = x[s].view(np.uint32)[np.arange(c), at]  # the word, a NaN's payload included
                    continue
                acc = np.zeros(c, dtype=F32)
                for p in run:
                    acc = acc + x[s, :, p]
                out[s, :, r] = vref.canonical(acc / F32(len(run)) if mode == MEAN else acc)
    return out, arg


def segment_pool_bwd(g, cluster, seg, arg, mode):
    """``grad_x[b,c,n]`` from ``g[b,c,m]``: a gather."""
    b, n = cluster.shape
    c = g.shape[1]
    out = np.zeros((b, c, n), dtype=F32)
    with np.errstate(all='ignore'):
        for s in range(b):
            for p in range(n):
                r = cluster[s, p]
                if r < 0:
                    continue
                if mode == MEAN:
                    out[s, :, p] = g[s, :, r] / F32(seg[s, r + 1] - seg[s, r])
                elif mode == SUM:
                    out[s, :, p] = g[s, :, r]
                else:
                    out[s, :, p] = np.where(arg[s, :, r] == p, g[s, :, r], F32(0))
    return out


def run_cloud(seed, b, res, lengths):
    """``xyz[b,n,3]`` whose occupied cells hold exactly ``lengths[j]`` points each (n = sum(lengths), len(lengths) <= res^3), at the
    nodes of the grid ``lo = 0, extent = res - 1``, the points shuffled."""
    rng = np.random.default_rng(seed)
    n = int(sum(lengths))
    xyz = np.zeros((b, n, 3), dtype=F32)
    for s in range(b):
        cells = np.repeat(rng.permutation(res ** 3)[:len(lengths)], lengths)
        cells = cells[rng.permutation(n)]
        xyz[s] = np.stack((cells // (res * res), cells // res % res, cells % res), -1)
    return xyz


def tie_features(seed, b, c, n):
    """``voxel_reference.features`` made of few distinct values, so that every run of a few points holds ties for the
    maximum (+0 against -0 among them), several NaNs and infinities of both signs."""
    rng = np.random.default_rng(seed)
    vals = np.array([0.0, -0.0, 1.0, 1.0, -2.0, 1e-40, -3e-42, np.inf, -np.inf, np.nan, 0.5, 0.5], dtype=F32)
    weights = np.array([3, 3, 3, 3, 3, 2, 2, 0.6, 1, 0.4, 3, 3])
    x = rng.choice(vals, size=(b, c, n), p=weights / weights.sum())
    nans = np.isnan(x)
    x.view(np.uint32)[nans] = rng.choice(np.array([0x7fc00000, 0xffc00001, 0x7fc12345], dtype=np.uint32), size=int(nans.sum()))
    return x


def random_runs(seed, b, n, tail=5, pad=3, slots=None):
    """A partition made by hand, for clouds larger than ``pcc_voxel_index`` sorts: ``(order[b,n], seg[b,m+1], cluster[b,n])`` with
    runs of 1 to 200 points (64 and 65 among them) over a random permutation, the last ``tail`` positions in no run (the
    non-finite points) and ``pad`` empty slots at the end; every cloud is cut alike.  With ``slots``: exactly that many
    slots, runs of one point but for one of 64, one of 65 and one that takes the rest."""
    rng = np.random.default_rng(seed)
    lengths = []
    if slots is not None:
        lengths = [1] * (slots - pad)
        lengths[1], lengths[3] = LONG_RUN, LONG_RUN + 1
        lengths[5] += n - tail - sum(lengths)
        assert lengths[5] >= 1
    while sum(lengths) < n - tail:
        lengths.append(int(rng.choice([1, 1, 2, 3, 5, 17, LONG_RUN, LONG_RUN + 1, 200])))
    lengths[-1] -= sum(lengths) - (n - tail)
    ends = np.concatenate(([0], np.cumsum(lengths), [n - tail] * pad)).astype(np.int32)
    m = len(ends) - 1
    order = np.stack([rng.permutation(n) for _ in range(b)]).astype(np.int32)
    cluster = np.full((b, n), -1, dtype=np.int32)
    for s in range(b):
        for r in range(m):
            order[s, ends[r]:ends[r + 1]].sort()  # (a run is in ascending point index)
            cluster[s, order[s, ends[r]:ends[r + 1]]] = r
    return order, np.tile(ends, (b, 1)), cluster
