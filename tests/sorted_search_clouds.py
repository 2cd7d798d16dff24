"""Deterministic stress clouds for the sorted searches (numpy only, no GPU).

The Hilbert sort (``am_sort_kernel``) and the box bound of the two searches that run on its output (``knn_sorted_kernel``,
``nn_sorted_kernel``) are exact by construction: nothing that could win, or tie with a lower ORIGINAL index, may be
skipped.  The clouds here are the shapes where that construction is under load: axes without extent (the quantisation
scale ``hi > lo ? 1023 / (hi - lo) : 0``), boxes of zero size, exact distance ties between points that the sort puts
into different 16-point boxes, coordinates whose differences cancel almost all of their bits, and extents that differ
by 2^26 between the axes.

Also here: the float64 brute-force neighbours the host test holds the CPU oracle against, and the counter of exact ties
that proves the tie clouds have them.
"""

from __future__ import annotations

import numpy as np

from tests.util import ref_cloud

KINDS = ('line', 'plane', 'point', 'lattice', 'clusters', 'offset', 'aniso', 'surface')

# axes on which every point of a sample has the same coordinate
ZERO_EXTENT_AXES = {'line': (1, 2), 'plane': (2,), 'point': (0, 1, 2), 'lattice': (), 'clusters': (), 'offset': (),
                    'aniso': (), 'surface': ()}

# kinds whose squared distances are computed without any rounding in float32, whatever the order of the operations
# (small integers; all differences zero): an exact float64 tie is an exact float32 tie there
EXACT_KINDS = ('lattice', 'point')

PLANE_Z = np.float32(0.25)
CLUSTER_GAP = np.float32(1000.0)
CLUSTER_SIGMA = 0.01
OFFSET = np.float32(1024.0)


def stress_cloud(kind: str, seed: int, b: int, n: int) -> np.ndarray:
    """``float32 [b, n, 3]``, a function of its arguments only.

    * ``line``: x uniform in [0, 1), y = z = 0.
    * ``plane``: x, y uniform in [0, 1), z = 0.25.
    * ``point``: every point of a sample is the same point.
    * ``lattice``: integer coordinates in [0, 6)^3 drawn independently, so every one of the 216 positions is held by
      about n / 216 points spread over the whole index range.
    * ``clusters``: two Gaussian blobs of sigma 0.01, centres 1000 apart on x, membership drawn per point.
    * ``offset``: uniform [0, 1)^3 + 1024: every coordinate is a multiple of 2^-13, every squared distance an exactly
      representable sum of multiples of 2^-26 before its roundings.
    * ``aniso``: uniform [0, 1)^3 with x * 2^13 and z * 2^-13.
    * ``surface``: ``tests.util.ref_cloud``, the cloud every other test uses.
    """
    rng = np.random.default_rng([seed, KINDS.index(kind)])
    if kind == 'surface':
        return ref_cloud(rng, b, n)
    u = rng.random((b, n, 3), dtype=np.float32)
    if kind == 'line':
        u[:, :, 1:] = 0.0
    elif kind == 'plane':
        u[:, :, 2] = PLANE_Z
    elif kind == 'point':
        u[:] = u[:, :1]
    elif kind == 'lattice':
        u = rng.integers(0, 6, (b, n, 3)).astype(np.float32)
    elif kind == 'clusters':
        u = rng.normal(0.0, CLUSTER_SIGMA, (b, n, 3)).astype(np.float32)
        u[:, :, 0] += rng.integers(0, 2, (b, n)).astype(np.float32) * CLUSTER_GAP
    elif kind == 'offset':
        u = u + OFFSET
    elif kind == 'aniso':
        u[:, :, 0] *= np.float32(2.0 ** 13)
        u[:, :, 2] *= np.float32(2.0 ** -13)
    else:
        raise ValueError(f'unknown kind {kind!r}')
    return np.ascontiguousarray(u, dtype=np.float32)


def channels_major(cloud: np.ndarray, channels=(0, 1, 2)) -> np.ndarray:
    """``[b, n, 3] -> [b, len(channels), n]`` contiguous: the layout of the k-NN graph's input."""
    return np.ascontiguousarray(cloud.transpose(0, 2, 1)[:, list(channels)])


def sqdist_f64(q: np.ndarray, c: np.ndarray) -> np.ndarray:
    """``q[n, ch], c[m, ch] -> [n, m]`` squared distances in float64 (differences of float32 values are exact in
    float64 whenever their exponents are less than 29 apart, which holds for every kind here)."""
    d = q[:, None, :].astype(np.float64) - c[None, :, :].astype(np.float64)
    return (d * d).sum(-1)


def knn_f64(x: np.ndarray, k: int) -> tuple[np.ndarray, np.ndarray]:
    """Brute-force k-NN of one channels-major cloud ``x[ch, n]`` in float64, ties by ascending index (the reference's
    rule): -> (idx[n, k + 1], dist[n, k + 1]); the extra column is what a test needs to see whether the k-th entry is
    separated from the first one left out (clipped to n columns)."""
    p = x.T
    d = sqdist_f64(p, p)
    order = np.argsort(d, axis=1, kind='stable')[:, : k + 1]
    return order, np.take_along_axis(d, order, axis=1)


def nn_f64(q: np.ndarray, c: np.ndarray) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Brute-force nearest neighbour in float64, lowest index on ties -> (idx[n], dist[n], runner_up_dist[n]) (the
    runner-up: the smallest distance of any OTHER candidate; +inf for a single candidate)."""
    d = sqdist_f64(q, c)
    idx = d.argmin(axis=1)  # (first occurrence)
    best = d[np.arange(len(q)), idx]
    d[np.arange(len(q)), idx] = np.inf
    return idx, best, d.min(axis=1)


def exact_sqdist_f32(q: np.ndarray, c: np.ndarray) -> np.ndarray:
    """The float32 squared distances ``fmaf(dz, dz, fmaf(dx, dx, dy * dy))`` of ``pcc_nndistance`` for the kinds where
    this float64 emulation is exact: ``lattice`` (nothing rounds) and ``offset`` (differences are multiples of 2^-13
    below 1, so every product and partial sum is a multiple of 2^-26 below 4 -- 28 bits, exact in float64 -- and the
    single rounding to float32 of each step is the fused operation's)."""
    d = q[:, None, :].astype(np.float64) - c[None, :, :].astype(np.float64)
    t = (d[..., 1] * d[..., 1]).astype(np.float32).astype(np.float64)
    t = (d[..., 0] * d[..., 0] + t).astype(np.float32).astype(np.float64)
    return (d[..., 2] * d[..., 2] + t).astype(np.float32)


def far_tie_counts(q: np.ndarray, c: np.ndarray, gap: int = 16) -> tuple[int, int]:
    """Exact ties of the float32 distances (``exact_sqdist_f32``: ``lattice`` and ``offset`` only) between candidates
    more than ``gap`` original indices apart -- further apart than any box of 16 consecutive points, so that the sort
    is free to put them into different boxes.  -> (queries whose MINIMUM is such a tie: the lowest-index rule decides
    their neighbour; queries with such a tie anywhere among their distances)."""
    d = exact_sqdist_f32(q, c)
    n, m = d.shape
    at_min = d == d.min(axis=1, keepdims=True)
    first = at_min.argmax(axis=1)
    last = m - 1 - at_min[:, ::-1].argmax(axis=1)
    decisive = int((last - first > gap).sum())
    order = np.argsort(d, axis=1, kind='stable')
    ds = np.take_along_axis(d, order, axis=1)
    # runs of equal values: a run's indices ascend (stable sort), so its spread is last - first
    run_start = np.ones((n, m), bool)
    run_start[:, 1:] = ds[:, 1:] != ds[:, :-1]
    run_id = run_start.cumsum(axis=1) - 1
    anywhere = 0
    for r in range(n):
        lo = np.full(run_id[r, -1] + 1, m, np.int64)
        hi = np.full(run_id[r, -1] + 1, -1, np.int64)
        np.minimum.at(lo, run_id[r], order[r])
        np.maximum.at(hi, run_id[r], order[r])
        anywhere += bool((hi - lo > gap).any())
    return decisive, anywhere
