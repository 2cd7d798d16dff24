"""Numpy reference of the point-voxel ops (``pcc_voxel_index``, ``pcc_voxelize`` / ``_bwd``, ``pcc_devoxelize`` / ``_bwd``,
include/pcc_neighbour.h): loops that follow the contract operation by operation in float32 (every numpy operation below
is on float32 operands, so each is rounded once, as the contract writes it), float64 evaluations for the gradients whose
summation order is not fixed, and the clouds the CPU and GPU tests share."""

import numpy as np

F32 = np.float32
NAN_WORD = 0x7fc00000

# The dispatch of csrc/voxelize.hip, for the tests that walk its boundaries: the register sort up to WAVE_SORT points, the
# LDS network padded to the next power of two above, MAX_POINTS at the most; CB channels per thread; a run of more than
# LONG_RUN points of one cell goes to the kernel with the channels across lanes; LDS bins up to res = LDS_RES.
WAVE_SORT, MAX_POINTS, CB, LONG_RUN, LDS_RES = 256, 16384, 8, 64, 32
SORT_THREADS = 1024  # threads of the LDS sort at the most: 2 keys per thread up to 2048 keys, then 4, 8, 16


# ---- which kernels a call runs, as exact launch-profile names (restated from DESIGN.md and the comments above) ----
def index_kernel(n):
    """``pcc_voxel_index``: the register sort of one wave up to WAVE_SORT points, the LDS sort above, instantiated by its keys
    per thread: the points padded to a power of two (512 at the least) over at most SORT_THREADS threads."""
    if n <= WAVE_SORT:
        return 'vox_index_wave_kernel'
    npad = 2 * WAVE_SORT
    while npad < n:
        npad *= 2
    return f'vox_index_lds_kernel<{max(2, npad // SORT_THREADS)}>'


def voxelize_kernels(n, res, aligned=True):
    """``pcc_voxelize``: the cell starts, the forward four cells per thread where res^3 is a multiple of 4 and counts and
    grid are 16-byte aligned (one otherwise), and the long-run kernel wherever a cell can hold more than LONG_RUN points."""
    wide = res ** 3 % 4 == 0 and aligned
    return {'vox_start_kernel', 'vox_fwd_kernel<4>' if wide else 'vox_fwd_kernel<1>'} | ({'vox_long_kernel'} if n > LONG_RUN else set())


def devox_bwd_kernel(res):
    """``pcc_devoxelize_bwd``: LDS bins up to LDS_RES -- rows of res^3 floats, 8 per workgroup while they fit 128 KB (res <=
    16), 4 to 20, 2 to 25, 1 above -- and global atomics beyond."""
    if res > LDS_RES:
        return 'devox_bwd_global_kernel'
    return 'devox_bwd_lds_kernel<%d>' % next((cb for cb in (8, 4, 2) if cb * res ** 3 * 4 <= 128 * 1024), 1)
GRIDS = ((-0.5, 1.0), None)  # (lo, extent); None: lo = 0, extent = res - 1, so that inv = 1 and grid coordinates are exact


def gamma(t):
    u = t * 2.0 ** -24
    return u / (1 - u)


def grid_of(res, which):
    return GRIDS[0] if which == 0 else (0.0, float(res - 1))


def scalars(res, lo, extent):
    """``(lo, inv, top)`` as the library rounds them."""
    top = F32(res - 1)
    return F32(lo), top / F32(extent), top


def canonical(a):
    a = np.array(a, dtype=F32)
    a.view(np.uint32)[np.isnan(a)] = NAN_WORD
    return a


# ---- pcc_voxel_index --------------------------------------------------------------------------------------------------

def voxel_index(xyz, res, lo, extent):
    """``(cell[b,n], order[b,n], counts[b,res^3])`` int32."""
    lo32, inv, top = scalars(res, lo, extent)
    b, n = xyz.shape[:2]
    cell = np.full((b, n), -1, dtype=np.int32)
    order = np.zeros((b, n), dtype=np.int32)
    counts = np.zeros((b, res ** 3), dtype=np.int32)
    finite = np.isfinite(xyz).all(2)
    with np.errstate(all='ignore'):
        t = (np.where(finite[:, :, None], xyz, F32(0)).astype(F32) - lo32) * inv  # two roundings
        ijk = np.minimum(np.maximum(np.floor(t + F32(0.5)), F32(0)), top).astype(np.int64)  # clamped as a float
    assert t.dtype == F32
    flat = (ijk[:, :, 0] * res + ijk[:, :, 1]) * res + ijk[:, :, 2]
    for s in range(b):
        for p in range(n):
            if finite[s, p]:
                cell[s, p] = flat[s, p]
                counts[s, flat[s, p]] += 1
        order[s] = sorted(range(n), key=lambda p: (cell[s, p] if cell[s, p] >= 0 else res ** 3, p))
    return cell, order, counts


# ---- pcc_voxelize / pcc_voxelize_bwd --------------------------------------------------------------------------------------

def voxelize(x, cell, counts):
    """``grid[b,c,res^3]``: the points of a cell added in ascending point index from +0.0, one division."""
    b, c, n = x.shape
    bins = counts.shape[1]
    acc = np.zeros((b, c, bins), dtype=F32)
    with np.errstate(all='ignore'):
        for s in range(b):
            for p in range(n):
                v = cell[s, p]
                if v >= 0:
                    acc[s, :, v] = acc[s, :, v] + x[s, :, p]
        cnt = counts[:, None, :]
        grid = np.where(cnt > 0, acc / np.maximum(cnt, 1).astype(F32), F32(0))
    return canonical(grid)


def voxelize_bwd(g, cell, counts):
    """``grad_x[b,c,n]`` from ``g[b,c,res^3]``: one division, +0.0 for cell -1."""
    b, n = cell.shape
    out = np.zeros((b, g.shape[1], n), dtype=F32)
    with np.errstate(all='ignore'):
        for s in range(b):
            for p in range(n):
                v = cell[s, p]
                if v >= 0:
                    out[s, :, p] = g[s, :, v] / F32(counts[s, v])
    return out


def voxelize_bwd_f64(g, cell, counts):
    safe = np.maximum(cell, 0)
    out = np.take_along_axis(g.astype(np.float64), safe[:, None, :].astype(np.int64), 2) / np.maximum(np.take_along_axis(counts, safe, 1), 1)[:, None, :]
    return np.where(cell[:, None, :] >= 0, out, 0.0)


# ---- pcc_devoxelize / pcc_devoxelize_bwd ------------------------------------------------------------------------------------

def corners(xyz, res, lo, extent):
    """``(finite[b,n], t[b,n,3] float32, off[8][b,n], w[8][b,n] float32, w64[8][b,n])``: the clamped grid coordinate, the
    flat cell and the float32 weight ``(wx * wy) * wz`` of every corner in the contract's order, and the same weights
    evaluated without rounding from the float32 ``t``."""
    lo32, inv, top = scalars(res, lo, extent)
    finite = np.isfinite(xyz).all(2)
    safe = np.where(finite[:, :, None], xyz, F32(0)).astype(F32)
    with np.errstate(all='ignore'):
        t = np.minimum(np.maximum((safe - lo32) * inv, F32(0)), top)
    i0 = np.minimum(np.floor(t).astype(np.int64), res - 2)
    f = t - i0.astype(F32)
    assert f.dtype == F32 and (f >= 0).all() and (f <= 1).all()
    w = (F32(1) - f, f)
    w64 = (1.0 - f.astype(np.float64), f.astype(np.float64))
    offs, ws, ws64 = [], [], []
    for e in range(8):
        di, dj, dk = e >> 2, (e >> 1) & 1, e & 1
        offs.append(((i0[:, :, 0] + di) * res + i0[:, :, 1] + dj) * res + i0[:, :, 2] + dk)
        ws.append((w[di][:, :, 0] * w[dj][:, :, 1]) * w[dk][:, :, 2])
        ws64.append(w64[di][:, :, 0] * w64[dj][:, :, 1] * w64[dk][:, :, 2])
    return finite, t, offs, ws, ws64


def devoxelize(grid, xyz, res, lo, extent):
    """``out[b,c,n]`` from ``grid[b,c,res^3]``: per corner a rounded product and a rounded sum, from +0.0."""
    finite, _, offs, ws, _ = corners(xyz, res, lo, extent)
    b, c = grid.shape[:2]
    acc = np.zeros((b, c, xyz.shape[1]), dtype=F32)
    with np.errstate(all='ignore'):
        for off, w in zip(offs, ws):
            acc = acc + w[:, None, :] * np.take_along_axis(grid, off[:, None, :], 2)
    return canonical(np.where(finite[:, None, :], acc, F32(0)))


def devoxelize_f64(grid, xyz, res, lo, extent):
    """``(value, sum |w g|)`` in float64 with exact weights from the float32 ``t``."""
    finite, _, offs, _, ws64 = corners(xyz, res, lo, extent)
    val, mag = 0.0, 0.0
    for off, w in zip(offs, ws64):
        term = w[:, None, :] * np.take_along_axis(grid.astype(np.float64), off[:, None, :], 2)
        val, mag = val + term, mag + np.abs(term)
    return np.where(finite[:, None, :], val, 0.0), np.where(finite[:, None, :], mag, 0.0)


class GradGrid:
    """``grad_grid[b,c,res^3]`` of ``g[b,c,n]`` in float64 with exact weights from the kernel's float32 ``t``, the sum of the
    magnitudes and the number of contributions to every element."""

    def __init__(self, xyz, g, res, lo, extent):
        finite, _, offs, _, ws64 = corners(xyz, res, lo, extent)
        b, c, n = g.shape
        bins = res ** 3
        self.want, self.mag = np.zeros((b, c, bins)), np.zeros((b, c, bins))
        self.deg = np.zeros((b, bins), dtype=np.int64)
        rows = np.arange(b)[:, None].repeat(n, 1)
        for off, w in zip(offs, ws64):
            term = np.where(finite[:, None, :], w[:, None, :] * g.astype(np.float64), 0.0)
            for ch in range(c):
                np.add.at(self.want[:, ch], (rows, off), term[:, ch])
                np.add.at(self.mag[:, ch], (rows, off), np.abs(term[:, ch]))
            np.add.at(self.deg, (rows[finite], off[finite]), 1)

    def check_exact(self, got):
        """Integer gradients, dyadic coordinates: every product and partial sum is representable."""
        got = got.reshape(self.want.shape)
        assert got.dtype == F32 and np.array_equal(got.astype(np.float64), self.want)
        assert not np.signbit(got[self.want == 0]).any()  # +0.0 where nothing points

    def check_bound(self, got):
        """Every element within gamma(t + 3) * sum |w g|: t - 1 additions, the product, and the three roundings of w."""
        got = got.reshape(self.want.shape)
        assert got.dtype == F32 and np.isfinite(got).all()
        bound = gamma(self.deg + 3)[:, None, :] * self.mag
        assert (np.abs(got.astype(np.float64) - self.want) <= bound).all()
        untouched = np.broadcast_to((self.deg == 0)[:, None, :], got.shape)
        assert (got[untouched].view(np.uint32) == 0).all()


# ---- the clouds -------------------------------------------------------------------------------------------------------

def cloud(seed, b, n, res, lo, extent, kind='mixed'):
    """``xyz[b,n,3]`` float32.  'mixed': Gaussian points around the cube (a fifth of them outside it), points on exact cell
    midpoints and on grid nodes (exact where the grid's inv is 1), and in every row a NaN point first, a +inf point last and a
    -inf and a NaN point inside (positions 0, n - 1, n // 2, n // 3).  'one_cell': every point in one cell.  'own_cell': point p at the node of cell p (n <= res^3)."""
    rng = np.random.default_rng(seed)
    step = extent / (res - 1)
    if kind == 'one_cell':
        u = np.tile(rng.integers(0, res, size=(b, 1, 3)).astype(np.float64), (1, n, 1)) + rng.uniform(-0.4, 0.4, size=(b, n, 3))
    elif kind == 'own_cell':
        assert n <= res ** 3
        p = np.stack([rng.permutation(res ** 3)[:n] for _ in range(b)])
        u = np.stack((p // (res * res), p // res % res, p % res), -1).astype(np.float64)
    else:
        u = rng.normal((res - 1) / 2, (res - 1) * 0.4, size=(b, n, 3))
        mid = rng.random((b, n)) < 0.25  # a midpoint on every axis, or a node
        u[mid] = rng.integers(-1, res + 1, size=(int(mid.sum()), 3)) + rng.choice([0.0, 0.5], size=(int(mid.sum()), 1))
    xyz = (lo + u * step).astype(F32)
    if kind == 'mixed':
        bad = [0, n - 1, n // 2, n // 3]
        vals = [np.nan, np.inf, -np.inf, np.nan]
        for s in range(b):  # (every row holds all four; where n is small and positions coincide the later value stands)
            for j, (p, v) in enumerate(zip(bad, vals)):
                xyz[s, p, (s + j) % 3] = v
    return xyz


def features(seed, b, c, n):
    """Gaussian ``x[b,c,n]`` float32 with +-0, denormals, +-inf and NaN sprinkled in."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((b, c, n)).astype(F32)
    special = np.array([0.0, -0.0, 1e-40, -3e-42, np.inf, -np.inf, np.nan], dtype=F32)
    hit = rng.random((b, c, n)) < 0.08
    x[hit] = rng.choice(special, size=int(hit.sum()))
    return x


def dyadic_cloud(seed, b, n, res):
    """Points whose grid coordinates are multiples of 1/4 on the grid ``lo = 0, extent = res - 1`` (inv = 1), some of them
    outside the cube, on nodes and on the top faces; one NaN point."""
    rng = np.random.default_rng(seed)
    xyz = (rng.integers(-4, 4 * res + 1, size=(b, n, 3)) / 4.0).astype(F32)
    xyz[:, n // 2, 1] = np.nan
    xyz[:, 0] = F32(res - 1)
    return xyz
