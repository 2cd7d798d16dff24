"""Reference of the ragged kernel map (``pcc_cell_neighbours_ragged``, include/pcc_neighbour.h) in numpy, and the inputs of
tests/test_cell_ragged_host.py and tests/test_gpu_cell_ragged.py.  Nothing here calls the code under test.

The rule slot by slot: a dictionary from the row ``(c, i, j, k)`` of every real slot to its rank, and plain loops over the slots
and the taps in Python integers (nothing can wrap; the dilation is taken as given, not clamped).  The inputs are rows of ``coord``
directly -- distinct, ascending by (c, i, j, k), which is what ``pcc_grid_cluster_ragged`` writes --, so that a cell can sit at 65535
on an axis without a cloud that spans 65536 cells.  ``dense_conv_reference`` is the float64 side of the end-to-end tests: the dense
``torch.nn.functional.conv3d`` of the level, its gradients, and the quantities of ``pcc_sparse_conv``'s bound."""

import itertools

import numpy as np

TOP = 65535           # the last cell of an axis
SLOTS = 256           # threads of the kernel's workgroup, each a (slot, di, dj) row of taps: a workgroup holds fewer slots than this
SLOT_COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513, 40 * SLOTS + 77)  # either side of 64 and of 256; hundreds of workgroups
DILATIONS = (1, 2, 3, 7, 65535, 65536, 2 ** 20)


def cell_map(coord, n_cells, ksize, dilation):
    """``nbr[m, ksize^3]`` int64 of ``coord[m, 4]`` with ``n_cells`` occupied cells."""
    coord = np.asarray(coord)
    m = len(coord)
    kept = min(max(int(n_cells), 0), m)
    h = (ksize - 1) // 2
    rows = [tuple(int(v) for v in coord[r]) for r in range(kept)]
    rank = {row: r for r, row in enumerate(rows)}
    assert len(rank) == kept
    offsets = list(itertools.product(range(-h, h + 1), repeat=3))  # tap t = ((di + h) * K + (dj + h)) * K + (dk + h), in this order
    nbr = np.full((m, ksize ** 3), -1, np.int64)
    for r, (c, i, j, k) in enumerate(rows):
        for t, (di, dj, dk) in enumerate(offsets):
            ti, tj, tk = i + dilation * di, j + dilation * dj, k + dilation * dk
            if 0 <= ti <= TOP and 0 <= tj <= TOP and 0 <= tk <= TOP:
                nbr[r, t] = rank.get((c, ti, tj, tk), -1)
    return nbr


def cut(full, m):
    """The map at capacity ``m`` from the map at a capacity >= the number of cells (the contract's restriction rule); rows behind
    the full map are padded slots."""
    out = np.full((m, full.shape[1]), -1, np.int64)
    rows = min(m, len(full))
    out[:rows] = np.where(full[:rows] < m, full[:rows], -1)
    return out


def padded(rows, m):
    """``(coord[m, 4] int32, n_cells)`` at capacity ``m``: the first ``m`` rows, -1 in a padded slot."""
    coord = np.full((m, 4), -1, np.int32)
    coord[:min(m, len(rows))] = rows[:m]
    return coord, len(rows)


def capacities(u, n):
    return sorted({m for m in (1, u - 1, u, u + 1, n) if 1 <= m <= n})


def check_properties(nbr, kept, ksize):
    """The centre tap of a real slot is the slot, the map is symmetric, a padded slot is empty, every word is in [-1, kept)."""
    taps = ksize ** 3
    assert ((nbr >= -1) & (nbr < max(kept, 1))).all() and (nbr[kept:] == -1).all()
    assert np.array_equal(nbr[:kept, taps // 2], np.arange(kept))
    r, t = np.nonzero(nbr >= 0)
    assert np.array_equal(nbr[nbr[r, t], taps - 1 - t], r)


# ---- inputs -------------------------------------------------------------------------------------------------------------------

def sort_rows(rows):
    rows = np.unique(np.asarray(rows, np.int64).reshape(-1, 4), axis=0)  # ascending by (c, i, j, k), distinct
    return rows.astype(np.int32)


def scene(u, seed=None, clouds=2):
    """A random sparse scene of exactly ``u`` cells in ``clouds`` clouds, about a third of a box at the origin occupied."""
    if u == 0:
        return np.zeros((0, 4), np.int32)
    rng = np.random.default_rng(1000 + u if seed is None else seed)
    side = max(2, int(np.ceil((3 * u / clouds) ** (1 / 3))))
    flat = rng.choice(clouds * side ** 3, u, replace=False)
    return sort_rows(np.stack([flat // side ** 3, flat // side ** 2 % side, flat // side % side, flat % side], 1))


def cube(side=6, cloud=0, origin=(0, 0, 0)):
    g = np.stack(np.meshgrid(*(np.arange(side),) * 3, indexing='ij'), -1).reshape(-1, 3) + np.asarray(origin)
    return sort_rows(np.concatenate([np.full((len(g), 1), cloud), g], 1))


def lines(length=70):
    """A line along each axis, each in a cloud of its own, crossing nothing."""
    rows = []
    for axis in range(3):
        for s in range(length):
            p = [3, 3, 3]
            p[axis] = s
            rows.append([axis] + p)
    return sort_rows(rows)


def traps():
    """The no-wrap traps: cells a carry out of k, out of j or out of the cloud field would join, coordinates 0 under a negative
    offset, and the corners of the grid, which are neighbours at dilation 65535 and at no other."""
    rows = [[0, 0, 0, TOP], [0, 0, 1, 0],            # (0, 0, 65535) + dk is not (0, 1, 0)
            [0, 0, TOP, 5], [0, 1, 0, 5],            # (0, 65535, 5) + dj is not (1, 0, 5)
            [0, TOP, TOP, TOP], [1, 0, 0, 0],        # cloud 0's last cell + dk is not cloud 1's first
            [0, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 2], [0, 0, 1, 1], [0, 1, 0, 0], [0, 1, 1, 1],  # coordinates 0 under negative offsets
            [1, 0, 0, 1], [1, TOP, TOP, TOP], [1, TOP, TOP, TOP - 1], [1, TOP, TOP - 2, TOP],
            [2, 0, 0, 0]]
    rows += [[3, a, b, c] for a in (0, TOP) for b in (0, TOP) for c in (0, TOP)]   # the corners: dilation 65535
    rows += [[3, 7, 7, c] for c in (0, 7, 14, 21, TOP - 7, TOP)]                  # dilation 7 along k
    return sort_rows(rows)


def batch37():
    """37 clouds, some of them empty, every other with a few cells; the last id holds the corners too."""
    rng = np.random.default_rng(37)
    rows = []
    for c in range(37):
        if c in (3, 4, 20):
            continue
        count = int(rng.integers(1, 30))
        rows += [[c, *rng.integers(0, 4, 3)] for _ in range(count)]
    rows += [[36, TOP, TOP, TOP], [36, 0, 0, 0], [36, TOP, TOP, TOP - 1]]
    return sort_rows(rows)


def high_clouds():
    """Cloud ids either side of 2^15 and the largest (B <= 65535): the top bit of the key's cloud field."""
    base = scene(40, seed=5, clouds=1)
    out = []
    for c in (0, 32767, 32768, 65534):
        part = base.copy()
        part[:, 0] = c
        out.append(part)
    return sort_rows(np.concatenate(out))


def one_cell_clouds():
    return sort_rows([[c, 5, 5, 5] for c in range(9)] + [[11, 5, 5, 6]])


def empties():
    """Empty clouds first (0, 1), adjacent in the middle (4, 5) and last (8, 9 of a batch of 10)."""
    a, b, c = scene(90, seed=11, clouds=1), scene(130, seed=12, clouds=1), scene(20, seed=13, clouds=1)
    a[:, 0], b[:, 0], c[:, 0] = 2, 3, 7
    return sort_rows(np.concatenate([a, b, c]))


def placed(where):
    """One cloud of 300 cells alone (None) or at position ``where`` among four others: ``(rows, its cloud id)``."""
    x = scene(300, seed=21, clouds=1)
    if where is None:
        return x, 0
    others = [scene(u, seed=22 + s, clouds=1) for s, u in enumerate((65, 700, 1, 31))]
    parts = others[:where] + [x] + others[where:]
    for c, part in enumerate(parts):
        part[:, 0] = c
    return sort_rows(np.concatenate(parts)), where


CASES = {f'u{u}': (lambda u=u: scene(u)) for u in SLOT_COUNTS}
CASES.update({'cube': cube, 'lines': lines, 'traps': traps, 'batch37': batch37, 'high_clouds': high_clouds, 'one_cell_clouds': one_cell_clouds,
              'empties': empties})
BIG = f'u{SLOT_COUNTS[-1]}'
# (case, ksize, dilation) of every comparison of the accelerator tests: every case at both kernel sizes, the small ones that reach
# far at every dilation
GRID = [(name, k, 1) for name in CASES for k in (3, 5)]
GRID += [(name, k, d) for name in ('traps', 'u257', 'cube', 'batch37') for k in (3, 5) for d in DILATIONS[1:]]

_ROWS, _MAPS = {}, {}


def rows_of(name):
    if name not in _ROWS:
        _ROWS[name] = CASES[name]()
        assert np.array_equal(_ROWS[name], sort_rows(_ROWS[name]))
    return _ROWS[name]


def case(name, ksize, dilation):
    """``(rows[U, 4], the reference map at capacity max(U, 1))``, computed once and never changed."""
    key = (name, ksize, dilation)
    if key not in _MAPS:
        rows = rows_of(name)
        coord, u = padded(rows, max(len(rows), 1))
        _MAPS[key] = cell_map(coord, u, ksize, dilation)
        _MAPS[key].setflags(write=False)
    return rows_of(name), _MAPS[key]


# ---- the end-to-end level: two clouds of unequal size on 16^3 grids -------------------------------------------------------------

E2E = dict(sizes=(700, 1500), axis_bits=4, size=1.0, c=4, o=5)   # about 1900 occupied cells: eight workgroups of the map


def e2e_inputs(seed=3):
    """``xyz[n, 3]`` in [0, 16)^3, ``offset``, features ``[n, c]``, and an integer gradient ``[n, o]`` (so that the sums of
    grid_unpool_ragged's backward are exact in float32)."""
    rng = np.random.default_rng(seed)
    n = sum(E2E['sizes'])
    xyz = (rng.random((n, 3)) * 16).astype(np.float32)
    return {'xyz': xyz, 'offset': np.cumsum(E2E['sizes']).astype(np.int64), 'start': np.zeros((2, 3), np.float32),
            'features': rng.standard_normal((n, E2E['c'])).astype(np.float32), 'grad': rng.integers(-3, 4, (n, E2E['o'])).astype(np.float32)}


def bar(d, s):
    """``pcc_sparse_conv``'s bound: D * 2^-24 / (1 - D * 2^-24) * S + D * 2^-126."""
    u = d * 2.0 ** -24
    return u / (1 - u) * s + d * 2.0 ** -126


def dense_conv_reference(coord, x, grad_y, weight, bias, nbr, ksize, dilation):
    """The float64 side: ``coord[m, 4]`` (every slot real, two clouds, cells inside 16^3), ``x[m, c]`` the float32 input of the
    convolution, ``grad_y[m, o]`` the gradient arriving at its output, ``weight[K^3, c, o]``, ``bias[o]`` and the reference
    map ``nbr[m, K^3]``.  Returns ``{name: (value, bound)}`` for ``out[m, o]``, ``grad_x[m, c]``, ``grad_weight`` and
    ``grad_bias``: the values from ``torch.nn.functional.conv3d`` on the dense grids and its autograd, the bounds from the
    contract's formula with S from the same graph on magnitudes and D from the map -- valid taps * c + 1 for a row of the
    output, valid taps * o + 1 for a row of grad_x (the same kernel on mirrored weights along the symmetric map), the rows
    that have tap t, + 1, for grad_weight[t] and the real slots + 1 for grad_bias (sums of that many terms in any order)."""
    import torch

    res = 1 << E2E['axis_bits']
    m, c = x.shape
    o = weight.shape[2]
    h = (ksize - 1) // 2
    cc, ii, jj, kk = (torch.from_numpy(coord[:, a].astype(np.int64)) for a in range(4))

    def run(x_, w_, b_, g_):
        xs, ws, bs = (torch.from_numpy(np.asarray(a, np.float64)).requires_grad_(True) for a in (x_, w_, b_))
        dense = torch.zeros((2, c, res, res, res), dtype=torch.float64)
        dense[cc, :, ii, jj, kk] = xs
        w5 = ws.view(ksize, ksize, ksize, c, o).permute(4, 3, 0, 1, 2)
        y = torch.nn.functional.conv3d(dense, w5, bs, padding=h * dilation, dilation=dilation)[cc, :, ii, jj, kk]
        (y * torch.from_numpy(np.asarray(g_, np.float64))).sum().backward()
        return y.detach().numpy(), xs.grad.numpy(), ws.grad.numpy(), bs.grad.numpy()

    value = run(x, weight, bias, grad_y)
    mag = run(np.abs(x), np.abs(weight), np.abs(bias), np.abs(grad_y))
    valid = nbr >= 0
    taps = valid.sum(1).astype(np.float64)
    d = (taps[:, None] * c + 1, taps[:, None] * o + 1, valid.sum(0).astype(np.float64)[:, None, None] + 1, float(m) + 1)
    names = ('out', 'grad_x', 'grad_weight', 'grad_bias')
    return {name: (value[i], bar(d[i], mag[i])) for i, name in enumerate(names)}
