"""Deterministic feature clouds for the k-NN kernels off the unit Gaussian (numpy only, no GPU).

The c >= 4 searches compute the expanded form ``(-2 x_i.x_j + |x_j|^2) + |x_i|^2`` and select on its VALUE: the role-split
kernel screens candidates against a bound derived from the k-th distance and the query's norm, the 128-query kernel lowers
its buffering threshold to "the next float above t", the wide path orders by an integer key of the float's bits.  The kinds
here put that machinery under load: norms far larger than the distances (``offset*``, ``const_channel``), distances that
round BELOW zero (``twins``), exact ties between distant indices (``lattice``), subnormal distances, every candidate
displacing an entry (``ray_rev``), and norms that overflow to +inf (``overflow``).

Also here: the lists the contract of ``include/pcc_neighbour.h`` prescribes for a given distance matrix
(``expected_lists``), float64 distances (``f64_sqdist``), the bound inside which a float32 list may differ from the
float64 one (``near_tie_bound``) and the check built on the three (``f64_list_check``).
"""

from __future__ import annotations

import numpy as np

KINDS = ('gauss', 'offset8', 'offset64', 'const_channel', 'relu', 'lattice', 'twins', 'aniso', 'scale_up', 'scale_down',
         'subnormal', 'ray', 'ray_rev', 'overflow', 'clones')

EPS32 = float(np.finfo(np.float32).eps)

# ``overflow``: the value of a big point's one non-zero channel.  Its square is above FLT_MAX, so |x_j|^2 = +inf.
OVERFLOW_BIG = np.float32(2e19)
# ``overflow`` for the difference form (c <= 3): big points are the Gaussian ones times this; (2e19 g)^2 overflows for
# |g| > 0.93, so a row mixes finite and +inf distances.  Differences of finite numbers are finite: no inf - inf, no NaN.
OVERFLOW_DIFF_MUL = np.float32(2e19)


def _gauss(seed: int, b: int, c: int, n: int) -> np.ndarray:
    return np.random.default_rng([seed, 0]).standard_normal((b, c, n), dtype=np.float32)


def overflow_big_points(c: int, n: int, first: int = 5, step: int = 3) -> np.ndarray:
    """The indices of the big points of ``overflow``: ``first::step``, at most 2 c of them (see ``feature_cloud``)."""
    return np.arange(first, n, step)[: 2 * c]


def overflow_cloud(seed: int, b: int, c: int, n: int, first: int = 5, step: int = 3) -> np.ndarray:
    """``gauss`` with the points ``overflow_big_points`` replaced by one-hot points of value +-2e19: the m-th big point has
    (-1)^m * 2e19 on channel (m // 2) % c and zeros elsewhere.  |x_j|^2 = +inf for a big point.  Two big points have the
    inner product 0 (different channels) or -inf (same channel: opposite signs by construction), never +inf, so the
    distance between them is +inf and not ``-inf + inf``: the only NaN of the distance matrix is a big point's distance to
    itself.  That caps the big points at 2 c.  (Gaussian points times 1e19 fail this: their mutual inner products overflow
    with either sign.)"""
    x = _gauss(seed, b, c, n)
    for m, j in enumerate(overflow_big_points(c, n, first, step)):
        x[:, :, j] = 0.0
        x[:, (m // 2) % c, j] = OVERFLOW_BIG if m % 2 == 0 else -OVERFLOW_BIG
    return np.ascontiguousarray(x)


def overflow_diff_cloud(seed: int, b: int, c: int, n: int) -> np.ndarray:
    """c <= 3, difference form: ``gauss`` with the points ``5::3`` multiplied by 2e19, so ``df * df`` overflows."""
    x = _gauss(seed, b, c, n)
    x[:, :, 5::3] *= OVERFLOW_DIFF_MUL
    return np.ascontiguousarray(x)


def feature_cloud(kind: str, seed: int, b: int, c: int, n: int) -> np.ndarray:
    """``float32 [b, c, n]``, a function of its arguments only.

    * ``gauss``: standard normal.
    * ``offset8``, ``offset64``: normal + 8 / + 64.
    * ``const_channel``: normal, channel 0 = 1000 for every point.
    * ``relu``: max(normal, 0).
    * ``lattice``: integers in {0, 1, 2}.
    * ``twins``: normal + 64 for ceil(n / 2) points; the other floor(n / 2) are copies of the first ones with about half
      of the coordinates moved one ulp up; then a fixed permutation of the points.
    * ``aniso``: normal, channel 0 * 2^13, the others * 2^-13.
    * ``scale_up``, ``scale_down``, ``subnormal``: ``gauss`` of the same seed * 2^40 / 2^-40 / 2^-70 (exact scalings).
    * ``ray``, ``ray_rev``: the points 64 + t_i v for one Gaussian direction v per sample, t = i / n ascending /
      descending along the index.
    * ``overflow``: ``overflow_cloud`` (one-hot big points at ``5::3``, at most 2 c of them).
    * ``clones``: ``twins`` with eight near-copies of every point instead of two: a row has eight distances around zero,
      so the 4th distance -- the K-th of the smallest list instantiation, and what the two half-wave lists of
      ``knn_mfma_kernel`` lower their threshold to -- is itself negative in many rows (with twins only the first two are).
    """
    if kind not in KINDS:
        raise ValueError(f'unknown kind {kind!r}')
    rng = np.random.default_rng([seed, 1 + KINDS.index(kind)])
    g = _gauss(seed, b, c, n)
    if kind == 'gauss':
        x = g
    elif kind in ('offset8', 'offset64'):
        x = rng.standard_normal((b, c, n), dtype=np.float32) + np.float32(8 if kind == 'offset8' else 64)
    elif kind == 'const_channel':
        x = rng.standard_normal((b, c, n), dtype=np.float32)
        x[:, 0, :] = 1000.0
    elif kind == 'relu':
        x = np.maximum(rng.standard_normal((b, c, n), dtype=np.float32), 0)
    elif kind == 'lattice':
        x = rng.integers(0, 3, (b, c, n)).astype(np.float32)
    elif kind == 'twins':
        h = n - n // 2
        base = rng.standard_normal((b, c, h), dtype=np.float32) + np.float32(64)
        copy = base[:, :, : n // 2].copy()
        up = rng.random(copy.shape) < 0.5
        copy[up] = np.nextafter(copy[up], np.float32(np.inf))
        x = np.concatenate([base, copy], axis=2)[:, :, rng.permutation(n)]
    elif kind == 'aniso':
        x = rng.standard_normal((b, c, n), dtype=np.float32) * np.float32(2.0 ** -13)
        x[:, 0, :] *= np.float32(2.0 ** 26)
    elif kind == 'scale_up':
        x = g * np.float32(2.0 ** 40)
    elif kind == 'scale_down':
        x = g * np.float32(2.0 ** -40)
    elif kind == 'subnormal':
        x = g * np.float32(2.0 ** -70)
    elif kind in ('ray', 'ray_rev'):
        t = (np.arange(n, dtype=np.float32) / np.float32(n))
        t = t if kind == 'ray' else t[::-1]
        v = rng.standard_normal((b, c, 1), dtype=np.float32)
        x = np.float32(64) + t[None, None, :] * v
    elif kind == 'clones':
        base = rng.standard_normal((b, c, -(-n // 8)), dtype=np.float32) + np.float32(64)
        x = np.tile(base, (1, 1, 8))[:, :, :n]
        up = rng.random(x.shape) < 0.5
        x[up] = np.nextafter(x[up], np.float32(np.inf))
        x = x[:, :, rng.permutation(n)]
    else:
        x = overflow_cloud(seed, b, c, n)
    return np.ascontiguousarray(x, dtype=np.float32)


def expected_lists(dist: np.ndarray, k: int) -> np.ndarray:
    """The lists of the header's contract for the distance rows ``dist[..., nq, n]``: per row the candidates whose
    distance is not NaN, ascending by (distance with -0 = +0, index), padded with ``n - 1`` -> int64 ``[..., nq, k]``.
    (A +inf distance is a distance; only NaN is left out.)"""
    dist = np.asarray(dist, np.float32)
    n = dist.shape[-1]
    order = np.argsort(dist + np.float32(0), axis=-1, kind='stable')[..., :k]  # (NaN sorts behind +inf; stable: by index)
    valid = (~np.isnan(dist)).sum(-1)[..., None]
    return np.where(np.arange(k) < valid, order, n - 1).astype(np.int64)


def f64_sqdist(q: np.ndarray, x: np.ndarray) -> np.ndarray:
    """``q[c, nq], x[c, n] -> [nq, n]`` squared distances in float64, difference form, channel by channel."""
    d = np.zeros((q.shape[1], x.shape[1]), np.float64)
    for ch in range(q.shape[0]):
        df = q[ch, :, None].astype(np.float64) - x[ch, None, :].astype(np.float64)
        d += df * df
    return d


def near_tie_bound(c: int, qn, xn):
    """How far apart in float64 two candidates may be and still change places in a float32 list of the expanded form:
    ``4 (c + 2) eps32 (|q|^2 + |x|^2)``."""
    return 4 * (c + 2) * EPS32 * (qn + xn)


def f64_list_check(q: np.ndarray, x: np.ndarray, idx: np.ndarray) -> tuple[float, int]:
    """``idx[nq, k]`` (a k-NN list of the queries ``q[c, nq]`` among ``x[c, n]``) against the float64 list.  Asserts
    that every entry that differs from the float64 list is a certified near tie,
    ``|d64[got] - d64[expected]| <= near_tie_bound`` (with the smaller of the two candidates' norms), and that the
    float64 distance of the k-th returned entry is at most the true k-th distance plus the bound.
    -> (the worst ratio of either difference to its bound, the number of differing entries)."""
    c, k = q.shape[0], idx.shape[1]
    d64 = f64_sqdist(q, x)
    qn = (q.astype(np.float64) ** 2).sum(0)[:, None]
    xn = (x.astype(np.float64) ** 2).sum(0)
    exp = np.argsort(d64, axis=1, kind='stable')[:, :k]
    dg, de = np.take_along_axis(d64, idx, 1), np.take_along_axis(d64, exp, 1)
    bound = near_tie_bound(c, qn, np.minimum(xn[idx], xn[exp]))
    differ = idx != exp
    # (a bound of 0 -- the zero vectors of ``relu`` -- admits no difference and has no ratio)
    ratio = np.divide(np.abs(dg - de), bound, out=np.zeros_like(bound), where=bound > 0)
    worst = float(ratio[differ].max()) if differ.any() else 0.0
    assert (np.abs(dg - de) <= bound)[differ].all(), worst
    kth_bound = near_tie_bound(c, qn[:, 0], xn[idx[:, -1]])
    over = dg[:, -1] - de[:, -1]
    over_ratio = np.divide(over, kth_bound, out=np.zeros_like(kth_bound), where=kth_bound > 0)
    assert (over <= kth_bound).all(), float(over_ratio.max())
    return max(worst, float(over_ratio.max())), int(differ.sum())
