"""numpy references for the voxel occupancy counts (``pcc_occupancy_grid`` / ``set_metrics.occupancy_grid``) and the
Jensen-Shannon divergence built on them.  Nothing here imports the library.

``cell_rule`` restates the float32 rule of include/pcc_structural.h; ``nearest_grid64`` is what the rule approximates: the
nearest grid point by a float64 brute force over every (in-sphere) grid point, with the points whose two nearest grid
points are too close to call marked ``ambiguous``.  A histogram treats every point on its own, so a test removes the
ambiguous points from the INPUT and compares the rest exactly.

``lattice_points``: for ``res`` in ``LATTICE_RES`` and power-of-two ``lo`` / ``extent`` the step ``extent / (res - 1)`` is a
power of two, and points at multiples of ``step / 2`` make every float32 operation of the rule exact (differences are
multiples of ``step / 2``, their squares and sums fit 24 bits): the float32 rule and float64 agree to the bit, exact cell
midpoints and ties between in-sphere grid points included."""

import functools

import numpy as np

LATTICE_RES = (3, 5, 9, 17, 33)
GENERIC_KINDS = ('uniform', 'gauss', 'sphere', 'shell', 'cell')
AMBIGUOUS_GAP = 1e-5  # relative gap between the two smallest distances below which a point is not compared
AMBIGUOUS_CAP = 0.01  # the share of points a test may remove


def sphere_mask(res):
    """[res,res,res] bool: the grid points inside the inscribed sphere, in integers."""
    a = 2 * np.arange(res, dtype=np.int64) - (res - 1)
    return a[:, None, None] ** 2 + a[None, :, None] ** 2 + a[None, None, :] ** 2 <= (res - 1) ** 2


def cell_rule(points, res, lo=-0.5, extent=1.0, in_sphere=False):
    """Flat cell of every point of ``points[..., 3]`` by the rule of include/pcc_structural.h, -1 for a point with a
    non-finite coordinate.  float32 for the separable cell and the grid coordinates; the distances of the in-sphere
    column scan in float64."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    lo32, top = np.float32(lo), np.float32(res - 1)
    inv, step = top / np.float32(extent), np.float32(extent) / top
    out = np.full(len(p), -1, np.int64)
    finite = np.isfinite(p).all(1)
    q = p[finite]
    with np.errstate(over='ignore'):
        t = (q - lo32) * inv
        assert t.dtype == np.float32
        ijk = np.minimum(np.maximum(np.floor(t + np.float32(0.5)), np.float32(0)), top).astype(np.int64)
    flat = (ijk[:, 0] * res + ijk[:, 1]) * res + ijk[:, 2]
    if in_sphere:
        mask = sphere_mask(res)
        ci, cj = np.nonzero(mask.any(2))  # the columns, in flat order
        klo = mask.argmax(2)[ci, cj]
        khi = res - 1 - mask[:, :, ::-1].argmax(2)[ci, cj]
        grid = (np.arange(res, dtype=np.float32) * step + lo32).astype(np.float64)
        assert (np.arange(res, dtype=np.float32) * step).dtype == np.float32
        for r in np.nonzero(~mask[ijk[:, 0], ijk[:, 1], ijk[:, 2]])[0]:
            k = np.clip(ijk[r, 2], klo, khi)
            x, y, z = q[r].astype(np.float64)
            with np.errstate(over='ignore'):
                d = (x - grid[ci]) ** 2 + (y - grid[cj]) ** 2 + (z - grid[k]) ** 2
            cand = (ci * res + cj) * res + k
            flat[r] = cand[d == d.min()].min()
    out[finite] = flat
    return out


def nearest_grid64(points, res, lo=-0.5, extent=1.0, in_sphere=False):
    """float64 brute force over all grid points (all in-sphere grid points) -> ``(flat[P], ambiguous[P])``: the nearest
    grid point of every point (lowest flat index among equal distances) and whether the gap between its two smallest
    (Euclidean) distances is at most ``AMBIGUOUS_GAP`` of the larger.  Finite points only."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    axis = lo + np.arange(res, dtype=np.float64) * (extent / (res - 1))
    cells = np.nonzero(sphere_mask(res).reshape(-1))[0] if in_sphere else np.arange(res ** 3)
    gi, gj, gk = cells // (res * res), cells // res % res, cells % res
    flat = np.empty(len(p), np.int64)
    ambiguous = np.empty(len(p), bool)
    for p0 in range(0, len(p), 128):
        c = p[p0:p0 + 128]
        d = np.sqrt((c[:, 0:1] - axis[gi]) ** 2 + (c[:, 1:2] - axis[gj]) ** 2 + (c[:, 2:3] - axis[gk]) ** 2)
        flat[p0:p0 + 128] = cells[d.argmin(1)]  # (the first minimum: the lowest flat index)
        two = np.partition(d, 1, axis=1)[:, :2]
        ambiguous[p0:p0 + 128] = two[:, 1] - two[:, 0] <= AMBIGUOUS_GAP * two[:, 1]
    return flat, ambiguous


def counts_of(flat, res, clouds=None, per_cloud=False):
    """Histogram of flat cells (-1 = counted nowhere) -> ``[res,res,res]``, or ``[clouds,res,res,res]`` for ``flat`` of
    ``clouds`` equal runs."""
    flat = np.asarray(flat).reshape(-1)
    bins = res ** 3
    if per_cloud:
        cloud = np.repeat(np.arange(clouds), len(flat) // clouds)
        keep = flat >= 0
        return np.bincount(cloud[keep] * bins + flat[keep], minlength=clouds * bins).reshape(clouds, res, res, res)
    return np.bincount(flat[flat >= 0], minlength=bins).reshape(res, res, res)


def jsd64(p_counts, q_counts):
    """``H(M) - (H(P) + H(Q)) / 2``, base 2, ``0 log 0 = 0``, of the two count arrays' distributions, in float64."""
    def entropy(x):
        x = x[x > 0]
        return -(x * np.log2(x)).sum()

    p = np.asarray(p_counts, np.float64).reshape(-1)
    q = np.asarray(q_counts, np.float64).reshape(-1)
    p, q = p / p.sum(), q / q.sum()
    return entropy((p + q) / 2) - (entropy(p) + entropy(q)) / 2


def lattice_points(res, seed, clouds, n, lo=-0.5, extent=1.0):
    """``[clouds, n, 3]`` float32 at multiples of ``step / 2`` from three steps below the cube to three steps above it: on
    grid points, on exact cell midpoints, and outside."""
    assert res in LATTICE_RES
    step = extent / (res - 1)
    m = np.random.default_rng(seed).integers(-6, 2 * (res - 1) + 7, size=(clouds, n, 3))
    x = (lo + m * (step / 2)).astype(np.float32)
    assert np.array_equal(x.astype(np.float64), lo + m * (step / 2))  # (representable: the premise of exactness)
    return x


def generic_points(kind, seed, clouds, n):
    """``[clouds, n, 3]`` float32 around PointFlow's unit cube [-0.5, 0.5]^3: ``uniform`` in [-0.7, 0.7]^3 (a good half
    outside the inscribed sphere), ``gauss`` sigma 0.2, ``sphere`` on the unit sphere (radius 1: every point outside
    the cube), ``shell`` on the inscribed sphere (radius 0.5: along the in-sphere border), ``cell``: every cloud inside one
    cell of the 28^3 grid."""
    rng = np.random.default_rng(seed)
    if kind == 'uniform':
        x = rng.uniform(-0.7, 0.7, size=(clouds, n, 3))
    elif kind == 'gauss':
        x = rng.normal(0.0, 0.2, size=(clouds, n, 3))
    elif kind in ('sphere', 'shell'):
        v = rng.normal(size=(clouds, n, 3))
        x = v / np.linalg.norm(v, axis=2, keepdims=True) * (1.0 if kind == 'sphere' else 0.5)
    elif kind == 'cell':
        centre = -0.5 + rng.integers(8, 20, size=(clouds, 1, 3)) / 27.0
        x = centre + rng.uniform(-0.4, 0.4, size=(clouds, n, 3)) / 27.0
    else:
        raise ValueError(kind)
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def generic_case(kind, seed, clouds, n, res, in_sphere):
    """One generic bank with its ambiguous points removed from every cloud (and every cloud cut to the shortest, so the
    bank stays rectangular) -> ``(points[clouds, n', 3], expected counts [clouds,res,res,res], removed share)``.
    Computed once per case and shared; callers do not write to it."""
    x = generic_points(kind, seed, clouds, n)
    flat, ambiguous = nearest_grid64(x, res, in_sphere=in_sphere)
    flat, ambiguous = flat.reshape(clouds, n), ambiguous.reshape(clouds, n)
    keep = n - ambiguous.sum(1).max()
    rows = [np.nonzero(~ambiguous[c])[0][:keep] for c in range(clouds)]
    points = np.stack([x[c, r] for c, r in enumerate(rows)])
    expected = counts_of(np.stack([flat[c, r] for c, r in enumerate(rows)]), res, clouds, per_cloud=True)
    for a in (points, expected):
        a.setflags(write=False)
    return points, expected, 1.0 - keep / n


# ---- which kernels a call runs (include/pcc_structural.h; include/pcc_test_hooks.h, occupancy_path), exact profile names ----
LDS_MAX_RES = 32  # res^3 int32 counters fit the LDS histogram's 128 KB up to here


def kernels_of(res, in_sphere, per_cloud, forced=0):
    """The LDS-histogram kernel (per cloud / whole set) wherever res^3 counters fit a workgroup's LDS, the global-atomic
    kernel otherwise; occupancy_path = 1 forces the global path, 2 the LDS path -- ignored where the counters do not fit
    (res > 32).  With in_sphere the deferred points take one more pass, the fallback kernel."""
    if res <= LDS_MAX_RES and forced != 1:
        names = {'occ_lds_kernel(per cloud)' if per_cloud else 'occ_lds_kernel(set)'}
    else:
        names = {'occ_global_kernel'}
    return names | ({'occ_fallback_kernel'} if in_sphere else set())
