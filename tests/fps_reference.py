"""Float64 reference of farthest point sampling for tests/test_gpu_fps.py and tests/test_fps_host.py: the rule of
``pcc_fps`` (include/pcc_neighbour.h) as a numpy greedy loop over a batch, the clouds the tests use, and the validity
check that follows a selection sequence it is given.  Nothing here calls the code under test."""

import numpy as np

INF = np.float64(np.inf)


def _clamped_start(start, b, n):
    if start is None:
        return np.zeros(b, np.int64)
    return np.clip(np.broadcast_to(np.asarray(start, np.int64), (b,)), 0, n - 1)


def _sqdist(x, sel):
    """``[b,n]`` squared distances of every point to point ``sel[b]`` of its cloud, coordinate order 0, 1, 2."""
    with np.errstate(invalid='ignore', over='ignore'):
        df = x - x[np.arange(x.shape[0]), sel][:, None, :]
        return df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1] + df[..., 2] * df[..., 2]


def fps_reference(xyz, m, start=None):
    """``(idx[b,m] int64, dist[b,m] float64)`` of the greedy rule in float64: running minima from +inf, lowered only by
    ``d < mind`` (a NaN lowers nothing), argmax with the lowest index among equal maxima; a point with a non-finite
    coordinate is excluded (never selected while another is left; NaN ``dist`` when it is selected, as a start too).
    The selection for ``m`` is a prefix of the selection for any larger ``m``."""
    x = np.asarray(xyz, np.float64)
    b, n, _ = x.shape
    rows = np.arange(b)
    mind = np.where(np.isfinite(x).all(-1), INF, -1.0)  # -1: excluded, below every minimum, never lowered
    idx = np.zeros((b, m), np.int64)
    dist = np.zeros((b, m), np.float64)
    sel = _clamped_start(start, b, n)
    for t in range(m):
        if t:
            sel = mind.argmax(1)  # numpy returns the first of equal maxima
        idx[:, t] = sel
        at = mind[rows, sel]
        dist[:, t] = np.where(at < 0, np.nan, at)
        d = _sqdist(x, sel)
        mind = np.where(d < mind, d, mind)
    return idx, dist


def check_validity(xyz, idx, dist=None):
    """Follow the selection ``idx[b,m]`` over finite clouds in float64 and require, at every step ``t >= 1``,
    ``mind64[idx[t]] >= max_j mind64[j] * (1 - 2**-20)``; ``dist`` (float32) within relative 2**-21 of the float64 value and
    non-increasing; no index twice.

    The bounds: a float32 distance carries five roundings on non-negative terms (three differences squared -- difference and
    square --, two additions; relative error at most 5u, u = 2**-24), so two candidates the float32 code compares can be
    misordered only when they differ by less than 10u relative: 2**-20 = 16u is the margin.  ``dist`` itself is one such
    distance: 5u, checked at 2**-21 = 8u."""
    x = np.asarray(xyz, np.float64)
    idx = np.asarray(idx)
    b, m = idx.shape
    assert np.isfinite(x).all()
    rows = np.arange(b)
    assert idx.min() >= 0 and idx.max() < x.shape[1]
    assert all(len(np.unique(idx[i])) == m for i in range(b)), 'an index repeats'
    mind = np.full(x.shape[:2], INF)
    for t in range(m):
        at = mind[rows, idx[:, t]]
        if t:
            top = mind.max(1)
            assert (at >= top * (1 - 2.0 ** -20)).all(), (t, at, top)
        if dist is not None:
            got = np.asarray(dist[:, t], np.float64)
            if t == 0:
                assert np.isposinf(got).all()
            else:
                assert (np.abs(got - at) <= 2.0 ** -21 * at).all(), (t, got, at)
        mind = np.minimum(mind, _sqdist(x, idx[:, t]))
    if dist is not None:
        assert (np.diff(np.asarray(dist, np.float64), axis=1) <= 0).all()


def lattice_cloud(seed, b, n, levels):
    """``[b,n,3]`` float32 points drawn (with repetition) from the lattice of ``levels``^3 points with coordinates ``k/16``,
    ``k`` a multiple of ``16 / levels`` in ``[0, 15]``: every difference, square and sum of squares is exact in float32, so
    the float32 and float64 greedy selections and distances are identical."""
    assert 16 % levels == 0
    k = np.random.default_rng(seed).integers(0, levels, (b, n, 3)) * (16 // levels)
    return (k / 16.0).astype(np.float32)


def generic_cloud(seed, b, n, kind):
    """Clouds of distinct points: uniform, Gaussian, those scaled by 100 and by 1e-3, and translated by +50."""
    rng = np.random.default_rng(seed)
    base = rng.random((b, n, 3)) if kind.startswith('uniform') else rng.standard_normal((b, n, 3))
    if kind.endswith('x100'):
        base = base * 100.0
    elif kind.endswith('x1e-3'):
        base = base * 1e-3
    elif kind.endswith('+50'):
        base = base + 50.0
    x = base.astype(np.float32)
    assert all(len(np.unique(x[i], axis=0)) == n for i in range(b))
    return x


GENERIC_KINDS = ('uniform', 'gauss', 'uniform_x100', 'gauss_x100', 'uniform_x1e-3', 'gauss_x1e-3', 'uniform_+50', 'gauss_+50')


# The kernel variants of pcc_fps (include/pcc_test_hooks.h, fps_path): value -> (exact launch-profile
# name, points the variant holds).  Six register variants (block, P) of capacity block * P, smallest first, then the
# memory path for any n.
VARIANTS = {1: ('fps_reg_kernel<64,4>', 256), 2: ('fps_reg_kernel<256,4>', 1024), 3: ('fps_reg_kernel<256,8>', 2048),
            4: ('fps_reg_kernel<512,8>', 4096), 5: ('fps_reg_kernel<1024,8>', 8192), 6: ('fps_reg_kernel<1024,16>', 16384),
            7: ('fps_mem_kernel', None)}


def kernel_of(n, forced=0):
    """The kernel a cloud of ``n`` points runs: the product takes the first variant that holds the cloud; a forced
    variant that cannot hold it is ignored."""
    if forced and (VARIANTS[forced][1] is None or VARIANTS[forced][1] >= n):
        return VARIANTS[forced][0]
    return next(name for name, cap in VARIANTS.values() if cap is None or cap >= n)
