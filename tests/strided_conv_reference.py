"""Numpy reference of the strided and transposed sparse convolution between two voxel levels (``neighbour_ops.coarsen_level``,
``stride_map``, ``sparse_conv_wgrad``): the coarse level and the map by loops over the slots; the weight gradient as float64 loops that also return, per tap, the number D of valid pairs and the sum S of |x| * |g|
over them; the dense grids a ``torch.nn.Conv3d(stride=2)`` reads.  The fine level a map starts from is
tests/voxel_reference.py's and tests/grid_pool_reference.py's, the convolution along a list tests/sparse_conv_reference.py's."""

import numpy as np

from tests import grid_pool_reference as gref
from tests import voxel_reference as vref

F32 = np.float32
TAPS = 8


def coarsen_cells(cell, order, seg, count, res):
    """``(cell_c[b,m], order_c[b,m], counts_c[b,rc^3], tap[b,m])`` int32 from the arrays of a fine level at capacity m."""
    b = cell.shape[0]
    m = seg.shape[1] - 1
    rc = (res + 1) // 2
    cell_c, tap = np.full((b, m), -1, dtype=np.int32), np.full((b, m), -1, dtype=np.int32)
    order_c, counts_c = np.zeros((b, m), dtype=np.int32), np.zeros((b, rc ** 3), dtype=np.int32)
    for s in range(b):
        for r in range(min(int(count[s]), m)):
            v = int(cell[s, order[s, seg[s, r]]])
            i, j, k = v // (res * res), v // res % res, v % res
            cell_c[s, r] = ((i >> 1) * rc + (j >> 1)) * rc + (k >> 1)
            tap[s, r] = ((i & 1) * 2 + (j & 1)) * 2 + (k & 1)
            counts_c[s, cell_c[s, r]] += 1
        order_c[s] = sorted(range(m), key=lambda r: (cell_c[s, r] if cell_c[s, r] >= 0 else rc ** 3, r))
    return cell_c, order_c, counts_c, tap


def stride_map(tap, cluster_c, count_c, m_c):
    """``(down[b,m_c,8], up[b,m_f,8])`` int64."""
    b, m_f = tap.shape
    down, up = np.full((b, m_c, TAPS), -1, dtype=np.int64), np.full((b, m_f, TAPS), -1, dtype=np.int64)
    for s in range(b):
        for f in range(m_f):
            r, t = int(cluster_c[s, f]), int(tap[s, f])
            if t >= 0 and 0 <= r < min(int(count_c[s]), m_c):
                assert down[s, r, t] == -1  # two fine cells never share a parent and a position
                down[s, r, t], up[s, f, t] = f, r
    return down, up


def build(xyz, res, lo, extent, m_f=None, m_c=None):
    """Both levels of the clouds ``xyz``: a dictionary with the fine index ``vi`` and partition ``gi`` at capacity ``m_f``
    (None: n), the coarse ``cvi = (cell_c, order_c, counts_c)``, ``tap``, the coarse partition ``cgi`` at capacity ``m_c`` (None:
    m_f), and ``down`` and ``up``."""
    vi = vref.voxel_index(xyz, res, lo, extent)
    gi = gref.grid_cluster(vi[0], vi[1], xyz.shape[1] if m_f is None else m_f)
    return coarsen(vi, gi, res, m_c)


def coarsen(vi, gi, res, m_c=None):
    """``build`` from a level's index and partition (the points of ``vi`` may themselves be the slots of a finer level)."""
    cell_c, order_c, counts_c, tap = coarsen_cells(vi[0], vi[1], gi[1], gi[2], res)
    cgi = gref.grid_cluster(cell_c, order_c, cell_c.shape[1] if m_c is None else m_c)
    down, up = stride_map(tap, cgi[0], cgi[2], cgi[1].shape[1] - 1)
    return dict(res=res, rc=(res + 1) // 2, vi=vi, gi=gi, cvi=(cell_c, order_c, counts_c), tap=tap, cgi=cgi, down=down, up=up)


def slot_cells(vi, gi):
    """``[b][r]``: the flat cell of every kept slot of a level."""
    cell, order = vi[:2]
    _, seg, count = gi
    m = seg.shape[1] - 1
    return [[int(cell[s, order[s, seg[s, r]]]) for r in range(min(int(count[s]), m))] for s in range(cell.shape[0])]


def dense(x, cells, res, size):
    """``[b,c,size,size,size]`` float64: the features ``x[b,c,m]`` of the slots scattered into the cells ``cells[b][r]`` of the
    grid of ``res``, padded with zeros to ``size`` per axis."""
    b, c = x.shape[:2]
    grid = np.zeros((b, c, size, size, size))
    for s in range(b):
        for r, v in enumerate(cells[s]):
            grid[s, :, v // (res * res), v // res % res, v % res] = x[s, :, r]
    return grid


def wgrad(x, nbr, g):
    """``(gw[t,c,o] float64, D[t], S[t,c,o])``: the exact sum over the valid pairs, their number per tap and the sum of |x| * |g|
    over them."""
    b, c, n = x.shape
    o = g.shape[1]
    taps = nbr.shape[2]
    gw, big_s, d = np.zeros((taps, c, o)), np.zeros((taps, c, o)), np.zeros(taps)
    valid = (nbr >= 0) & (nbr < n)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    with np.errstate(all='ignore'):
        for s in range(b):
            for t in range(taps):
                rows = np.nonzero(valid[s, :, t])[0]
                if len(rows) == 0:
                    continue
                got = x64[s][:, nbr[s, rows, t]]  # [c, rows]
                gw[t] += got @ g64[s][:, rows].T
                big_s[t] += np.abs(got) @ np.abs(g64[s][:, rows]).T
                d[t] += len(rows)
    return gw, d, big_s


def wgrad_bar(d, big_s):
    """The bound of a float32 sum of D rounded products in any order, ``D u / (1 - D u) S + D 2^-126`` with u = 2^-24, ``[t,c,o]``."""
    u = d[:, None, None] * 2.0 ** -24
    return u / (1 - u) * big_s + d[:, None, None] * 2.0 ** -126


def wgrad_share(got, want, d, big_s):
    """The largest |got - want| as a share of the bar (0 where both the error and the bar are 0)."""
    err, lim = np.abs(got.astype(np.float64) - want), wgrad_bar(d, big_s)
    return float(np.max(np.where(err == 0, 0.0, err / np.maximum(lim, 1e-300))))
