"""Numpy reference of the submanifold sparse convolution (``pcc_cell_neighbours``, ``pcc_sparse_conv``,
include/pcc_neighbour.h): the kernel map by a dictionary from cell to rank, with the triple decomposed before the offset is
added, the convolution as float64 loops that also return the D and S of the contract's bound per output, and the clouds the CPU
and GPU tests share.  The index and the partition a map starts from are tests/voxel_reference.py's and
tests/grid_pool_reference.py's."""

import numpy as np

from tests import grid_pool_reference as gref
from tests import voxel_reference as vref

F32 = np.float32
# The dispatch of csrc/sparse_conv.hip, for the tests that walk its boundaries.  c >= MFMA_MIN_C and o >= MFMA_MIN_O: the MFMA
# kernel -- tiles of MFMA_TILE slots (the granularity at which an empty tap is skipped), MFMA_WAVE_ROWS slots per wave and
# MFMA_ROWS per workgroup, 16, 32 or 64 output channels per wave.  Otherwise the VALU kernel: a wave owns ROW_TILE slots, a lane
# OB output channels, OB the smallest of OB_SIZES that holds them all (the largest above).  MAP_SLOTS slots per workgroup of the
# map kernel.
ROW_TILE, MAP_SLOTS, OB_SIZES = 64, 256, (8, 16, 32, 64)
MFMA_MIN_C, MFMA_MIN_O, MFMA_TILE, MFMA_WAVE_ROWS, MFMA_ROWS, MFMA_SIZES = 8, 16, 16, 32, 128, (16, 32, 64)
KERNELS = [f'sparse_conv_kernel<{ob}>' for ob in OB_SIZES] + [f'sparse_conv_mfma_kernel<{ob}>' for ob in MFMA_SIZES]


def kernel_of(c, o):
    """The profile name of the kernel ``pcc_sparse_conv`` launches for ``c`` input and ``o`` output channels."""
    if c >= MFMA_MIN_C and o >= MFMA_MIN_O:
        return f'sparse_conv_mfma_kernel<{next((ob for ob in MFMA_SIZES if o <= ob), MFMA_SIZES[-1])}>'
    return f'sparse_conv_kernel<{next((ob for ob in OB_SIZES if o <= ob), OB_SIZES[-1])}>'


def offsets(ksize, dilation):
    """``[(di, dj, dk)]`` in tap order, already multiplied by the dilation."""
    h = (ksize - 1) // 2
    return [(dilation * di, dilation * dj, dilation * dk) for di in range(-h, h + 1) for dj in range(-h, h + 1) for dk in range(-h, h + 1)]


def cell_neighbours(cell, order, seg, count, res, ksize, dilation):
    """``nbr[b,m,ksize^3]`` int64 from the arrays of ``voxel_reference.voxel_index`` and ``grid_pool_reference.grid_cluster``."""
    b = cell.shape[0]
    m = seg.shape[1] - 1
    offs = offsets(ksize, dilation)
    nbr = np.full((b, m, len(offs)), -1, dtype=np.int64)
    for s in range(b):
        kept = min(int(count[s]), m)
        cells = [int(cell[s, order[s, seg[s, r]]]) for r in range(kept)]
        rank = {v: r for r, v in enumerate(cells)}
        assert len(rank) == kept
        for r, v in enumerate(cells):
            i, j, k = v // (res * res), v // res % res, v % res  # the triple first: nothing wraps around
            for t, (di, dj, dk) in enumerate(offs):
                ti, tj, tk = i + di, j + dj, k + dk
                if 0 <= ti < res and 0 <= tj < res and 0 <= tk < res:
                    nbr[s, r, t] = rank.get((ti * res + tj) * res + tk, -1)
    return nbr


def build(xyz, res, lo, extent, m=None, ksize=3, dilation=1):
    """``(cell, order, counts), (cluster, seg, count), nbr`` of the clouds ``xyz`` at capacity ``m`` (None: n)."""
    vi = vref.voxel_index(xyz, res, lo, extent)
    gi = gref.grid_cluster(vi[0], vi[1], xyz.shape[1] if m is None else m)
    return vi, gi, cell_neighbours(vi[0], vi[1], gi[1], gi[2], res, ksize, dilation)


def is_symmetric(nbr):
    b, m, taps = nbr.shape
    s, r, t = np.nonzero(nbr >= 0)
    return bool((nbr[s, nbr[s, r, t], taps - 1 - t] == r).all())


def cut(nbr, m):
    """The map at capacity ``m`` from the map at a larger capacity: the rows cut, the ranks >= m turned into -1."""
    return np.where(nbr[:, :m] < m, nbr[:, :m], -1)


def sparse_conv(x, nbr, weight, bias=None):
    """``(out[b,o,m] float64, D[b,m], S[b,o,m])``: the exact sum over the valid taps (a row without one: 0, no bias), and the
    D = (valid taps) * c + 1 and S = |bias| + sum |w| * |x| of the contract's bound."""
    b, c, n = x.shape
    m, taps = nbr.shape[1:]
    o = weight.shape[2]
    x64, w64 = x.astype(np.float64), weight.astype(np.float64)
    out, big_s, d = np.zeros((b, o, m)), np.zeros((b, o, m)), np.ones((b, m))
    valid = (nbr >= 0) & (nbr < n)
    with np.errstate(all='ignore'):
        for s in range(b):
            for t in range(taps):
                rows = np.nonzero(valid[s, :, t])[0]
                if len(rows) == 0:
                    continue
                got = x64[s][:, nbr[s, rows, t]]  # [c, rows]
                out[s][:, rows] += w64[t].T @ got
                big_s[s][:, rows] += np.abs(w64[t]).T @ np.abs(got)
                d[s, rows] += c
        if bias is not None:
            some = valid.any(2)[:, None, :]
            out += np.where(some, bias.astype(np.float64)[None, :, None], 0.0)
            big_s += np.where(some, np.abs(bias.astype(np.float64))[None, :, None], 0.0)
    return out, d, big_s


def bar(d, big_s):
    """The contract's bound ``D u / (1 - D u) S + D 2^-126`` with u = 2^-24, ``[b,o,m]``."""
    u = d[:, None, :] * 2.0 ** -24
    return u / (1 - u) * big_s + d[:, None, :] * 2.0 ** -126


def share(got, want, d, big_s):
    """The largest |got - want| as a share of the bar (0 where both the error and the bar are 0)."""
    err, lim = np.abs(got.astype(np.float64) - want), bar(d, big_s)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(lim, 1e-300))))


def grad_x_scatter(g, nbr, weight, n):
    """``grad_x[b,c,n]`` float64 by the scatter definition: every output hands ``weight[t] @ g`` to the slot it read."""
    b, o, m = g.shape
    c = weight.shape[1]
    out = np.zeros((b, c, n))
    g64, w64 = g.astype(np.float64), weight.astype(np.float64)
    for s in range(b):
        for r in range(m):
            for t in range(nbr.shape[2]):
                p = nbr[s, r, t]
                if 0 <= p < n:
                    out[s, :, p] += w64[t] @ g64[s, :, r]
    return out


def grad_weight_bias(x, g, nbr):
    """``(grad_weight[t,c,o], grad_bias[o])`` float64."""
    b, c, n = x.shape
    o = g.shape[1]
    taps = nbr.shape[2]
    gw = np.zeros((taps, c, o))
    valid = (nbr >= 0) & (nbr < n)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    for s in range(b):
        for t in range(taps):
            rows = np.nonzero(valid[s, :, t])[0]
            gw[t] += x64[s][:, nbr[s, rows, t]] @ g64[s][:, rows].T
    return gw, (g64 * valid.any(2)[:, None, :]).sum((0, 2))


def lattice_cloud(res, b=1):
    """Every cell of the res^3 grid ``lo = 0, extent = res - 1`` holds one point, in shuffled order."""
    rng = np.random.default_rng(res)
    cells = np.stack([rng.permutation(res ** 3) for _ in range(b)])
    return np.stack((cells // (res * res), cells // res % res, cells % res), -1).astype(F32)


def cells_cloud(cells, res, repeat=1):
    """One cloud with ``repeat`` points in each of the listed flat cells of the grid ``lo = 0, extent = res - 1``."""
    v = np.repeat(np.asarray(cells, dtype=np.int64), repeat)
    return np.stack((v // (res * res), v // res % res, v % res), -1).astype(F32)[None]


def lattice_inputs(seed, b, c, o, n, taps):
    """Small integer features and dyadic weights and bias: every partial sum of a row stays far below 2^24 in units of the
    smallest term, so float32 arithmetic in any order is exact."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-4, 5, size=(b, c, n)).astype(F32)
    w = (rng.integers(-8, 9, size=(taps, c, o)) / 8.0).astype(F32)
    bias = (rng.integers(-8, 9, size=o) / 4.0).astype(F32)
    return x, w, bias


def gaussian_inputs(seed, b, c, o, n, taps):
    """Gaussian features and weights pushed away from zero (|v| >= 2^-6), clear of denormal products and sums."""
    rng = np.random.default_rng(seed)

    def draw(shape):
        v = rng.standard_normal(shape)
        return (np.sign(v) * np.maximum(np.abs(v), 2.0 ** -6)).astype(F32)

    return draw((b, c, n)), draw((taps, c, o)), draw(o)
