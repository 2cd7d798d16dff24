"""Reference of the ragged grid index (``pcc_grid_cluster_ragged``, include/pcc_neighbour.h) in numpy, and the inputs of
tests/test_grid_ragged_host.py and tests/test_gpu_grid_ragged.py.  Nothing here calls the code under test, and nothing imports torch.

The rule slot by slot: the cloud of a row from the (valid) offsets, the cell per axis in float32 numpy arithmetic --
``floor((x - start) / size)``, numpy's float32 subtraction and division are IEEE --, the key as an unsigned 64-bit integer, a
stable argsort, and a dictionary from every distinct valid key to its rank.  Offsets are valid here (non-decreasing from 0, ending
at or before n; the rows behind the last belong to no cloud): what the kernel does with other offsets is only bounded by the tests.

The key is ``cloud_bits + 3 * axis_bits`` wide with ``axis_bits >= 1`` and ``cloud_bits >= 1``, so the narrowest key has 4 bits:
WIDTHS lists (B, axis_bits) for 4, 8, 9, 16, 17, 33 and 63 bits, one to eight passes of 8-bit digits."""

import numpy as np

from tests import ragged_reference as R

TILE = 2048  # PCC_GRID_RAGGED_TILE: the keys one workgroup of the sort ranks


def cloud_bits(b):
    return int(b).bit_length()


def default_axis_bits(b):
    return min(16, (63 - cloud_bits(b)) // 3)


def starts(xyz, offset):
    """``start[B,3]``: per cloud and axis the minimum of the finite coordinates, +inf where there is none."""
    out = np.full((len(offset), 3), np.inf, np.float32)
    for c, (lo, hi) in enumerate(R.ranges(offset)):
        for a in range(3):
            col = xyz[lo:hi, a]
            col = col[np.isfinite(col)]
            if len(col):
                out[c, a] = col.min()
    return out


def cells(xyz, offset, start, size, axis_bits):
    """``(cloud[n], q[n,3], valid[n])``: the cell rule.  ``cloud`` is -1 for a row of no cloud."""
    xyz, start = np.asarray(xyz, np.float32), np.asarray(start, np.float32)
    n = len(xyz)
    cloud = np.full(n, -1, np.int64)
    assert len(offset) == 0 or int(offset[-1]) <= n
    for c, (lo, hi) in enumerate(R.ranges(offset)):
        cloud[lo:hi] = c
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        diff = xyz - start[np.maximum(cloud, 0)]
        t = diff / np.float32(size)
        assert diff.dtype == np.float32 and t.dtype == np.float32
        f = np.floor(t)
        valid = (cloud >= 0) & ((t >= 0) & (f < np.float32(2 ** axis_bits))).all(1)
    q = np.where(valid[:, None], f, 0).astype(np.int64)
    return cloud, q, valid


def grid_cluster(xyz, offset, start, size, m, axis_bits):
    """The six outputs of the contract as a dict of int32 arrays (``n_cells`` of shape [1])."""
    b, n = len(offset), len(xyz)
    assert 1 <= m <= n and 1 <= axis_bits <= 16 and cloud_bits(b) + 3 * axis_bits <= 63
    cloud, q, valid = cells(xyz, offset, start, size, axis_bits)
    s = np.uint64(axis_bits)
    dropped = np.uint64(b) << (np.uint64(3) * s)
    qq = q.astype(np.uint64)
    key = (np.maximum(cloud, 0).astype(np.uint64) << (np.uint64(3) * s)) | (qq[:, 0] << (np.uint64(2) * s)) | (qq[:, 1] << s) | qq[:, 2]
    key = np.where(valid, key, dropped)
    order = np.argsort(key, kind='stable')
    skey = key[order]
    distinct = np.unique(key[valid])  # ascending
    rank_of = {int(k): r for r, k in enumerate(distinct)}
    u, v = len(distinct), int(valid.sum())
    if n <= 200000:
        cluster = np.array([rank_of.get(int(k), -1) for k in key], np.int64)
    else:  # (the same lookup, vectorised)
        cluster = np.where(valid, np.searchsorted(distinct, key), -1)
    cluster[cluster >= m] = -1
    first = np.searchsorted(skey, distinct, side='left')  # the first sorted position of every run
    seg = np.full(m + 1, first[m] if u > m else v, np.int64)
    seg[:min(u, m)] = first[:min(u, m)]
    mask = (1 << axis_bits) - 1
    coord = np.full((m, 4), -1, np.int64)
    for r, k in enumerate(distinct[:m]):
        k = int(k)
        coord[r] = (k >> (3 * axis_bits), (k >> (2 * axis_bits)) & mask, (k >> axis_bits) & mask, k & mask)
    per_cloud = np.bincount((distinct >> (np.uint64(3) * s)).astype(np.int64), minlength=b)[:b]
    new_offset = np.minimum(np.cumsum(per_cloud), m)
    return {'cluster': cluster.astype(np.int32), 'order': order.astype(np.int32), 'seg': seg.astype(np.int32), 'coord': coord.astype(np.int32),
            'new_offset': new_offset.astype(np.int32), 'n_cells': np.array([u], np.int32)}


NAMES = ('cluster', 'order', 'seg', 'coord', 'new_offset', 'n_cells')


def cut(full, m):
    """The outputs at capacity ``m`` from those at capacity n (the contract's restriction rule)."""
    cluster = np.where(full['cluster'] < m, full['cluster'], -1)
    return {'cluster': cluster.astype(np.int32), 'order': full['order'], 'seg': full['seg'][:m + 1], 'coord': full['coord'][:m],
            'new_offset': np.minimum(full['new_offset'], m).astype(np.int32), 'n_cells': full['n_cells']}


def check_structure(out, n, m):
    """What holds for every input: ``order`` a permutation, runs ascending in point index (stability), ``seg`` non-decreasing,
    ``cluster`` the slot whose run holds the point."""
    order, seg, cluster = out['order'].astype(np.int64), out['seg'].astype(np.int64), out['cluster']
    assert np.array_equal(np.sort(order), np.arange(n))
    assert (np.diff(seg) >= 0).all() and seg[0] == 0 and seg[-1] <= n
    u = int(out['n_cells'][0])
    for r in range(min(u, m)):
        run = order[seg[r]:seg[r + 1]]
        assert len(run) >= 1 and (np.diff(run) > 0).all() and (cluster[run] == r).all()
    assert (np.diff(order[seg[min(u, m)]:]) > 0).all() or u > m  # the dropped points: in index order
    assert (cluster >= -1).all() and (cluster < min(u, m)).all()


# ---- inputs -------------------------------------------------------------------------------------------------------------------

WIDTHS = {4: (1, 1), 8: (2, 2), 9: (4, 2), 16: (1, 5), 17: (2, 5), 33: (4, 10), 63: (16384, 16)}
SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
# more than one block of the scan of the sort's table (256 words per tile, 1024 per block: above 4 tiles) and of the run heads
# (1024 positions per block); LOOP: more than 256 block sums, so the one workgroup that scans them takes a second round
MULTI_BLOCK_N = 40 * TILE + 77
LOOP_N = 1025 * TILE + 5
NONDYADIC = (0.05, 0.02, 1.0 / 3.0)


def _case(xyz, offset, start, size, axis_bits=None):
    offset = np.asarray(offset, np.int64)
    return {'xyz': np.ascontiguousarray(xyz, np.float32), 'offset': offset, 'start': np.ascontiguousarray(start, np.float32),
            'size': float(np.float32(size)), 'axis_bits': default_axis_bits(len(offset)) if axis_bits is None else axis_bits}


def sized(n):
    """Two Gaussian clouds (the first a third of the rows) on a grid of 0.25."""
    xyz, offset = R.batch(500 + n, [n // 3, n - n // 3], 'gauss')
    return _case(xyz, offset, starts(xyz, offset), 0.25)


def uniform(n, seed=3):
    """One cloud uniform in [0, 8)^3 on a grid of 0.25 from the origin: 32^3 cells, axis_bits = 5, two passes."""
    xyz = (np.random.default_rng(seed).random((n, 3)) * 8).astype(np.float32)
    return _case(xyz, [n], np.zeros((1, 3)), 0.25, 5)


def width(bits, n=300):
    """Integer cells on a unit grid at the extremes of every field, in the clouds 0, B // 2 and B - 1 (the same points in each):
    keys that differ in the top digit only (cloud 0 against B - 1; q0 = 0 against 2^axis_bits - 1) and in the lowest only
    (q2 = 0 against 1), and dropped points (a coordinate at 2^axis_bits, one below the start)."""
    b, ab = WIDTHS[bits]
    rng = np.random.default_rng(bits)
    top = (1 << ab) - 1
    pool = np.array(sorted({0, 1, top, max(top - 1, 0)}))
    q = rng.choice(pool, (n, 3))
    q[: n // 4] = rng.integers(0, top + 1, (n // 4, 3))
    xyz = q + 0.5
    xyz[5, 0] = top + 1.0   # at 2^axis_bits cells: dropped
    xyz[6, 2] = -0.25       # below the start: dropped
    used = sorted({0, b // 2, b - 1})
    sizes = np.zeros(b, np.int64)
    sizes[used] = n
    return _case(np.concatenate([xyz] * len(used), 0), np.cumsum(sizes), np.zeros((b, 3)), 1.0, ab)


def shapes():
    sizes = [0, 0, 1, 2, 63, 0, 0, 64, 65, 300, 2049, 0]
    xyz, offset = R.batch(77, sizes, 'gauss', extra=5)  # five rows behind the last offset
    return _case(xyz, offset, starts(xyz[:offset[-1]], offset), 0.3)


def many(b):
    sizes = np.random.default_rng(b).integers(0, 50, b)
    sizes[0] = max(sizes[0], 1)
    xyz, offset = R.batch(90 + b, list(sizes), 'gauss')
    return _case(xyz, offset, starts(xyz, offset), 0.5)


def one_cell(n=3000):
    xyz = (np.random.default_rng(4).random((n, 3)) * 0.1 + 2).astype(np.float32)
    return _case(xyz, [n], np.zeros((1, 3)), 4.0)


def lattice(side=12, shuffle=True):
    """Every point of the integer lattice of ``side`` in its own cell of a unit grid."""
    g = np.stack(np.meshgrid(*(np.arange(side),) * 3, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    if shuffle:
        g = g[np.random.default_rng(5).permutation(len(g))]
    return _case(g, [len(g)], np.zeros((1, 3)), 1.0)


def duplicates(n=500):
    rng = np.random.default_rng(6)
    base = rng.standard_normal((20, 3)).astype(np.float32)
    xyz = base[rng.integers(0, 20, n)]
    offset = [n // 2, n]
    return _case(xyz, offset, starts(xyz, offset), 0.1)


def non_finite():
    """NaN and +-inf points at the front and the back of a cloud, a coordinate below the start, at and beyond the last cell
    (axis_bits = 4 at size 0.5: 8.0 is the first coordinate outside), and a cloud whose start row is NaN."""
    rng = np.random.default_rng(8)
    sizes = [100, 70, 130, 50]
    xyz = (rng.random((sum(sizes), 3)) * 7.5).astype(np.float32)
    offset = np.cumsum(sizes)
    xyz[0, 0], xyz[1, 1], xyz[2, 2] = np.nan, np.inf, -np.inf                        # the front of cloud 0
    xyz[99, 2], xyz[98, 0] = np.nan, np.inf                                          # its back
    xyz[100, 1], xyz[169, 0] = -np.inf, np.nan                                       # cloud 1: first and last row
    xyz[110, 0], xyz[111, 1], xyz[112, 2] = -0.001, 8.0, 8.5                         # below, at, beyond
    xyz[113] = (7.9999995, 0.0, 7.9999995)                                           # the last cell, kept
    start = np.zeros((4, 3), np.float32)
    start[3, 1] = np.nan                                                             # every point of cloud 3 is dropped
    return _case(xyz, offset, start, 0.5, 4)


def gauss(kind):
    scale = 100.0 if kind.endswith('x100') else 1e-3 if kind.endswith('x1e-3') else 1.0
    xyz, offset = R.batch(31, [700, 0, 1300, 41], kind)
    return _case(xyz, offset, starts(xyz, offset), 0.25 * scale)


def boundaries(size, count=400):
    """Coordinates at the float32 nearest to ``q * size`` and one ulp either side, start 0: on these the quotient lies within
    an ulp of the integer q, so a reciprocal multiply, or a division that is not correctly rounded, lands in another cell."""
    rng = np.random.default_rng(int(size * 1000))
    s32 = np.float32(size)
    qs = rng.integers(1, 3000, count)
    x = (qs.astype(np.float64) * np.float64(s32)).astype(np.float32)
    col = np.concatenate([np.nextafter(x, np.float32(0)), x, np.nextafter(x, np.float32(np.inf))])
    xyz = np.zeros((len(col), 3), np.float32)
    xyz[:, 0], xyz[:, 1], xyz[:, 2] = col, np.roll(col, 1), np.roll(col, 7)
    return _case(xyz, [len(xyz) // 2, len(xyz)], np.zeros((2, 3)), s32, 12)


CASES = {f'n{n}': (lambda n=n: sized(n)) for n in SIZES}
CASES.update({f'bits{bits}': (lambda bits=bits: width(bits)) for bits in WIDTHS})
CASES.update({f'B{b}': (lambda b=b: many(b)) for b in (1, 2, 3, 37)})
CASES.update({kind: (lambda kind=kind: gauss(kind)) for kind in ('gauss', 'gauss_x100', 'gauss_x1e-3', 'gauss_+50')})
CASES.update({f'boundary{i}': (lambda s=s: boundaries(s)) for i, s in enumerate(NONDYADIC)})
CASES.update({'shapes': shapes, 'one_cell': one_cell, 'own_cell': lattice, 'duplicates': duplicates, 'non_finite': non_finite,
              'multi_block': lambda: uniform(MULTI_BLOCK_N)})

_BUILT = {}


def case(name):
    """The inputs of a case and its reference outputs at capacity n, computed once and never changed."""
    if name not in _BUILT:
        i = CASES[name]()
        _BUILT[name] = (i, grid_cluster(i['xyz'], i['offset'], i['start'], i['size'], len(i['xyz']), i['axis_bits']))
    return _BUILT[name]


def capacities(u, n):
    return sorted({m for m in (1, u - 1, u, u + 1, n) if 1 <= m <= n})
