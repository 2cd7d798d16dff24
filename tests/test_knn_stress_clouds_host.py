"""CPU tests of tests/knn_stress_clouds.py: the clouds do what their table claims (so the GPU tests that use them cannot
pass vacuously), ``expected_lists`` is the oracle's order, and the oracle itself is within the float64 bound the GPU
lists are held to."""

import numpy as np
import pytest

from tests import knn_stress_clouds as sc

CS = (4, 17, 64, 128)
N, K = 260, 8


def _oracle(oracle_mod, x, k=K):
    return oracle_mod.knn_expanded(x, k, return_dist=True)


@pytest.mark.parametrize('c', CS)
def test_twins_have_negative_distances_and_displaced_selves(oracle_mod, c):
    x = sc.feature_cloud('twins', 3, 2, c, N)
    idx, dm = _oracle(oracle_mod, x)
    d = np.take_along_axis(dm, idx, axis=2)
    negative = (d < 0).mean()
    not_self_first = (idx[:, :, 0] != np.arange(N)).mean()
    print(f'twins c={c}: {100 * negative:.2f} % negative entries, {100 * not_self_first:.1f} % rows not self-first')
    assert negative > 0.01
    assert not_self_first > 0.25
    # A negative value is the k-th entry of a row for k = 1 only.  (A row of twins has ONE negative entry at most: the
    # distance of a point to itself is (-2 s + s) + s = +0 exactly, s being one fma chain, and a point has one twin.  The
    # k-th entry of a longer list can be negative only with more copies: that is what ``clones`` is for, below.)
    assert (d[:, :, 0] < 0).any()
    assert ((d[:, :, 1:] >= 0) & ~np.signbit(d[:, :, 1:])).all()


@pytest.mark.parametrize('c', CS)
def test_clones_have_a_negative_kth_distance(oracle_mod, c):
    """The 4th distance (the K-th of the smallest list instantiation, and the rank the 128-query kernel's shared threshold
    reads in both half lists at K = 8) is negative in more than 10 % of the rows; measured 20-28 %."""
    x = sc.feature_cloud('clones', 3, 2, c, N)
    idx, dm = _oracle(oracle_mod, x)
    d = np.take_along_axis(dm, idx, axis=2)
    share = (d[:, :, 3] < 0).mean()
    print(f'clones c={c}: 4th distance negative in {100 * share:.1f} % of the rows, {100 * (d < 0).mean():.1f} % of all entries')
    assert share > 0.10
    assert (d[:, :, :4] < 0).all(axis=2).any()


@pytest.mark.parametrize('c', CS)
def test_lattice_ties_at_the_kth_distance_between_distant_indices(oracle_mod, c):
    x = sc.feature_cloud('lattice', 3, 2, c, N)
    idx, dm = _oracle(oracle_mod, x)
    kth = np.take_along_axis(dm, idx[:, :, K - 1 :], axis=2)  # [b,n,1]
    tied = dm == kth
    lo = tied.argmax(axis=2)
    hi = N - 1 - tied[:, :, ::-1].argmax(axis=2)
    assert (hi - lo > 64).any()
    # nothing rounds: the float32 distances are the float64 ones
    for s in range(2):
        assert np.array_equal(dm[s].astype(np.float64), sc.f64_sqdist(x[s], x[s]))


@pytest.mark.parametrize('c', CS + (8, 200))
@pytest.mark.parametrize('n,first,step', [(N, 5, 3), (40, 5, 1), (130, 6, 1)])
def test_overflow_rows(oracle_mod, c, n, first, step):
    """Rows of small queries hold +inf and no NaN; rows of big queries hold exactly their own NaN (and are +inf elsewhere)."""
    x = sc.overflow_cloud(3, 2, c, n, first, step)
    assert np.isfinite(x).all()
    big = np.zeros(n, bool)
    big[sc.overflow_big_points(c, n, first, step)] = True
    assert big.sum() == min(2 * c, len(range(first, n, step)))
    _, dm = _oracle(oracle_mod, x)
    assert np.isinf(dm[:, ~big][:, :, big]).all() and (dm[:, ~big][:, :, big] > 0).all()
    assert np.isfinite(dm[:, ~big][:, :, ~big]).all()
    nan = np.isnan(dm)
    assert np.array_equal(nan, np.broadcast_to(np.diag(big), nan.shape))
    assert (dm[:, big][~nan[:, big]] == np.inf).all()


def test_overflow_default_is_the_table_construction():
    assert np.array_equal(sc.feature_cloud('overflow', 9, 1, 64, N), sc.overflow_cloud(9, 1, 64, N))
    assert np.array_equal(sc.overflow_big_points(64, N), np.arange(5, N, 3))


@pytest.mark.parametrize('c', (1, 2, 3))
def test_overflow_diff_form_has_inf_and_no_nan(c):
    x = sc.overflow_diff_cloud(3, 2, c, 300)
    assert np.isfinite(x).all()
    with np.errstate(over='ignore'):
        d = np.zeros((2, 300, 300), np.float32)
        for ch in range(c):
            df = x[:, ch, None, :] - x[:, ch, :, None]
            assert np.isfinite(df).all()  # no inf - inf anywhere: the sum of squares cannot be NaN
            d += df * df
    assert not np.isnan(d).any()
    finite_per_row = np.isfinite(d).sum(-1)
    assert (finite_per_row < 25).any() and np.isinf(d).any()  # rows whose 25- and 32-lists reach +inf


@pytest.mark.parametrize('c', CS)
@pytest.mark.parametrize('kind', sc.KINDS)
def test_expected_lists_is_the_oracles_order(oracle_mod, kind, c):
    x = sc.feature_cloud(kind, 5, 2, c, N)
    idx, dm = _oracle(oracle_mod, x, 32)
    clean = ~np.isnan(dm).any(-1)
    assert clean.any()
    assert np.array_equal(sc.expected_lists(dm, 32)[clean], idx[clean])
    if kind != 'overflow':
        assert clean.all()


def test_expected_lists_on_nan_inf_and_signed_zero():
    inf, nan = np.inf, np.nan
    row = np.array([[3.0, nan, inf, -0.0, 0.0, -1.0, inf, nan]], np.float32)
    assert sc.expected_lists(row, 8).tolist() == [[5, 3, 4, 0, 2, 6, 7, 7]]
    assert sc.expected_lists(row, 3).tolist() == [[5, 3, 4]]
    assert sc.expected_lists(np.full((1, 4), nan, np.float32), 2).tolist() == [[3, 3]]


@pytest.mark.parametrize('kind', ('scale_up', 'scale_down'))
def test_scaled_clouds_have_the_lists_of_gauss(oracle_mod, kind):
    for c in CS:
        g, s = sc.feature_cloud('gauss', 7, 1, c, N), sc.feature_cloud(kind, 7, 1, c, N)
        assert np.array_equal(oracle_mod.knn_expanded(g, 32), oracle_mod.knn_expanded(s, 32))


@pytest.mark.parametrize('c', CS)
@pytest.mark.parametrize('kind', [k for k in sc.KINDS if k not in ('subnormal', 'overflow')])
def test_oracle_lists_against_float64(oracle_mod, kind, c):
    """The oracle's float32 lists differ from the float64 ones only inside ``near_tie_bound``; no cap on how many do
    off-centre (the expanded form loses the bits the offset takes), 0.1 % on the unit Gaussian."""
    x = sc.feature_cloud(kind, 5, 2, c, N)
    idx = oracle_mod.knn_expanded(x, K)
    worst, differ = 0.0, 0
    for s in range(2):
        w, d = sc.f64_list_check(x[s], x[s], idx[s])
        worst, differ = max(worst, w), differ + d
    print(f'{kind} c={c}: worst ratio {worst:.4f}, {differ} of {idx.size} entries differ')
    if kind == 'gauss':
        assert differ <= 0.001 * idx.size


def test_subnormal_distances_are_subnormal(oracle_mod):
    tiny = np.finfo(np.float32).tiny
    for c in CS:
        x = sc.feature_cloud('subnormal', 5, 1, c, N)
        _, dm = _oracle(oracle_mod, x)
        assert (np.abs(dm) < tiny).all() and (dm != 0).any() and ((x * x) < tiny).all()
