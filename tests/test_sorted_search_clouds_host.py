"""The stress clouds of tests/sorted_search_clouds.py are what they claim, and the CPU oracle the GPU tests compare
against is right on them (no GPU needed).

The GPU tests (tests/test_gpu_sorted_search.py) are bit-exact comparisons with ``oracle_mod.knn_diff`` and
``oracle_mod.nndistance``.  Those are float32 restatements of the reference's loops; here they are held against a float64
brute force with the reference's tie rule (lowest index), on every kind of cloud, wherever float64 can decide: an entry
is compared when the float64 distances on both sides of it are separated by more than the float32 chain can move them,
and -- on the kinds whose float32 arithmetic is exact -- also through exact ties.
"""

import numpy as np
import pytest

from tests.sorted_search_clouds import (EXACT_KINDS, KINDS, ZERO_EXTENT_AXES, channels_major, far_tie_counts, knn_f64,
                                        nn_f64, stress_cloud)

# Relative error of a float32 squared distance against the exact one: each difference is rounded once (2^-24, doubled by
# the square), each of the three products / fused sums once more; the terms are non-negative, so the relative errors do
# not amplify: (2 + 3) * 2^-24 < 2^-21 per distance.  Two distances further apart than 4x that, relative to the larger,
# keep their order in float32.
SEPARATED = 2.0 ** -19


@pytest.mark.parametrize('kind', KINDS)
def test_kinds_are_what_they_claim(kind):
    x = stress_cloud(kind, 3, 2, 500)
    assert x.shape == (2, 500, 3) and x.dtype == np.float32 and x.flags['C_CONTIGUOUS'] and np.isfinite(x).all()
    assert np.array_equal(x, stress_cloud(kind, 3, 2, 500))           # deterministic
    assert not np.array_equal(x, stress_cloud(kind, 4, 2, 500))       # and seeded
    assert not np.array_equal(x[0], x[1])                             # samples differ
    extent = x.max(axis=1) - x.min(axis=1)                            # [b, 3]
    for axis in range(3):
        if axis in ZERO_EXTENT_AXES[kind]:
            assert (extent[:, axis] == 0).all(), (kind, axis)
        else:
            assert (extent[:, axis] > 0).all(), (kind, axis)
    cm = channels_major(x)
    assert cm.shape == (2, 3, 500) and cm.flags['C_CONTIGUOUS'] and np.array_equal(cm[1, 2], x[1, :, 2])
    assert np.array_equal(channels_major(x, (0, 1))[0, 1], x[0, :, 1])
    if kind == 'line':
        assert (x[:, :, 1:] == 0).all()
    if kind == 'plane':
        assert (x[:, :, 2] == np.float32(0.25)).all()
    if kind == 'point':
        assert (x == x[:, :1]).all()
    if kind == 'lattice':
        assert np.array_equal(x, np.round(x)) and x.min() == 0 and x.max() == 5
        # every position is taken, by about n / 216 points each
        _pos, cnt = np.unique(stress_cloud(kind, 3, 1, 2100)[0], axis=0, return_counts=True)
        assert len(cnt) == 216 and cnt.min() >= 2
    if kind == 'clusters':
        far = x[:, :, 0] > 500
        assert 0.3 < far.mean() < 0.7                                          # both blobs are populated
        assert np.abs(x[:, :, 0] - np.where(far, 1000.0, 0.0)).max() < 0.06    # sigma 0.01 (6 sigma)
        assert np.abs(x[:, :, 1:]).max() < 0.06
        assert (far[:, :-1] != far[:, 1:]).mean() > 0.3                         # membership is drawn per point
    if kind == 'offset':
        assert x.min() >= 1024 and x.max() <= 1025
        assert np.array_equal(x * 8192, np.round(x * 8192))                    # multiples of 2^-13
    if kind == 'aniso':
        assert extent[:, 0].min() > 0.9 * 8192 and extent[:, 2].max() < 1 / 8192 and 0.9 < extent[:, 1].min() <= 1


def test_tie_kinds_have_exact_ties_between_far_indices():
    """What ``lattice`` and ``offset`` are for: exact ties of the float32 distance between candidates more than 16
    original indices apart, so that the tied candidates sit in different boxes of the sort and the searches must carry
    the lowest ORIGINAL index across blocks they visit in another order.

    ``lattice`` (2100 queries, 2049 candidates): a query's minimum, 0, is attained by every candidate at its position;
    their number is Binomial(2049, 1/216) (mean 9.5), spread over the index range.  A query is NOT decided by the tie
    rule only if at most one candidate shares its position -- probability e^-9.5 (1 + 9.5) < 0.001, and then the 6
    positions at distance 1 tie instead -- or if all sharers lie within 16 indices (below 1e-6).  Bar: 95 % of the
    queries.  Inside one cloud (the k-NN graph) it is the same count with the query itself among the sharers.

    ``offset``: the differences are multiples of 2^-13 below 1, the squared distances multiples of 2^-26 below 3
    rounded to 24 bits: at most 2^23 values per binade, and about three binades ([1/8, 1)) hold nearly all of a
    query's 2049 distances.  2049^2 / 2 pairs of distances over at most 3 * 2^23 values: about 0.08 expected exact ties
    per query, hence about 8 % of the queries with one, nearly all of them between far indices.  Bar: 2 %, a
    quarter of that.  Ties AT the minimum are rare on this kind (the minimum sits in a binade with far more values
    than candidates): it loads the box bound, whose gaps are differences of coordinates that agree in their
    leading 10 bits, not the tie rule."""
    a, c = stress_cloud('lattice', 11, 1, 2100)[0], stress_cloud('lattice', 12, 1, 2049)[0]
    decisive, anywhere = far_tie_counts(a, c)
    assert decisive >= 0.95 * 2100 and anywhere >= decisive, (decisive, anywhere)
    decisive, _ = far_tie_counts(a, a)
    assert decisive >= 0.95 * 2100, decisive
    a, c = stress_cloud('offset', 11, 1, 2100)[0], stress_cloud('offset', 12, 1, 2049)[0]
    decisive, anywhere = far_tie_counts(a, c)
    assert anywhere >= 0.02 * 2100, (decisive, anywhere)


def _compared(dist_sorted, exact):
    """Which entries of float64-sorted lists ``dist_sorted[n, k + 1]`` float64 decides: both neighbours in the list (the
    first one left out included) are separated, or -- ``exact`` kinds -- anything."""
    if exact:
        return np.ones(dist_sorted[:, :-1].shape, bool)
    gap_ok = dist_sorted[:, 1:] - dist_sorted[:, :-1] > SEPARATED * dist_sorted[:, 1:]   # [n, k]: entry o vs o + 1
    ok = gap_ok.copy()
    ok[:, 1:] &= gap_ok[:, :-1]
    return ok


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('b,c,n,k', [(2, 3, 300, 20), (1, 3, 257, 32), (2, 2, 100, 7), (1, 1, 64, 5)])
def test_knn_oracle_equals_float64_brute_force(oracle_mod, kind, b, c, n, k):
    x = channels_major(stress_cloud(kind, 20 + n, b, n), range(c))
    got = oracle_mod.knn_diff(x, k)
    compared = 0
    for s in range(b):
        idx, dist = knn_f64(x[s], k)
        if dist.shape[1] == k:  # (k == n: nothing is left out)
            dist = np.concatenate([dist, np.full((n, 1), np.inf)], axis=1)
        ok = _compared(dist, kind in EXACT_KINDS)
        assert np.array_equal(got[s][ok], idx[:, :k][ok]), (kind, s)
        compared += int(ok.sum())
    # float64 decides nearly everything except on the clouds made of near-ties
    floor = {'offset': 0.5, 'clusters': 0.5}.get(kind, 0.9)
    assert compared >= floor * b * n * k, (kind, compared, b * n * k)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('b,n,m', [(2, 300, 257), (1, 257, 130), (1, 100, 17), (2, 5, 300)])
def test_nndistance_oracle_equals_float64_brute_force(oracle_mod, kind, b, n, m):
    a, c = stress_cloud(kind, 40 + n, b, n), stress_cloud(kind, 41 + n, b, m)
    d1, i1, d2, i2 = oracle_mod.nndistance(a, c)
    compared = 0
    for s in range(b):
        for q, cand, gd, gi in ((a[s], c[s], d1[s], i1[s]), (c[s], a[s], d2[s], i2[s])):
            idx, best, second = nn_f64(q, cand)
            ok = np.ones(len(q), bool) if kind in EXACT_KINDS else second - best > SEPARATED * second
            assert np.array_equal(gi[ok], idx[ok]), (kind, s)
            # the float32 distance is the float64 one to the chain's rounding (exactly, where nothing rounds)
            assert np.all(np.abs(gd.astype(np.float64) - best) <= (0.0 if kind == 'lattice' else 2.0 ** -21) * best)
            compared += int(ok.sum())
    assert compared >= 0.9 * b * (n + m), (kind, compared)
    if kind == 'lattice':  # a cloud against its copy: every point is its own nearest neighbour, the lowest copy wins
        d1, i1, d2, i2 = oracle_mod.nndistance(a, a)
        _pos, first = np.unique(a[0], axis=0, return_index=True)
        assert (d1 == 0).all() and set(i1[0].tolist()) == set(first.tolist()) and np.array_equal(i1, i2)
