"""GPU tests of the k-NN kernels on the clouds of tests/knn_stress_clouds.py: offset, scaled, tied, negative-distance,
subnormal and overflowing feature clouds through every c >= 4 kernel (``knn_mfma_kernel``, ``knn_mfma_split_kernel``,
``knn_wide_dist_kernel`` + ``knn_wide_select_kernel``), ``pcc_knn_cross``, and the c <= 3 kernels on overflowing clouds.

The expectation is the header's contract applied to the oracle's distance matrix (``expected_lists``): candidates
ascending by (distance, index), a +inf distance listed like any other, only NaN left out, short lists padded with n - 1.
Which kernel ran is read from the library's launch profile."""

import contextlib
import functools

import numpy as np
import pytest
import torch

from tests import knn_reference as kr
from tests import knn_stress_clouds as sc
from tests.which_ran import assert_only
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

CS = (4, 17, 64, 128)
KS = (8, 25, 32)
# (tuning switch, the kernel that must run, the kernels that must not)
SWITCHES = {
    'mfma': (('knn_nosplit', 1), 'knn_mfma_kernel', ('knn_mfma_split_kernel', 'knn_wide_select_kernel')),
    'split': (('knn_nosplit', 2), 'knn_mfma_split_kernel', ('knn_mfma_kernel', 'knn_wide_select_kernel')),
    'wide': (('knn_wide', 1), 'knn_wide_select_kernel', ('knn_mfma_kernel', 'knn_mfma_split_kernel')),
    # the product's own dispatch: two samples of a few hundred points do not fill the chip
    'auto': (None, 'knn_mfma_kernel', ('knn_mfma_split_kernel', 'knn_wide_select_kernel')),
}
FORCED = ('mfma', 'split', 'wide')
# the list lengths at which the k-th distance itself is negative (see the host test)
EXTRA_KS = {'clones': (4,), 'twins': (1, 2)}


def _t(a):
    return torch.from_numpy(np.array(a))  # (a writable copy: the shared cases are read-only)


def _ns(kind):
    return (700,) if kind in ('ray', 'ray_rev') else (130, 300)


@functools.lru_cache(maxsize=None)
def _case(kind, c, n, seed=11):
    """(x[2,c,n], the oracle's distance matrix [2,n,n]), computed once and read-only."""
    import oracle

    x = sc.feature_cloud(kind, seed, 2, c, n)
    _, dm = oracle.knn_expanded(x, 1, return_dist=True)
    x.setflags(write=False)
    dm.setflags(write=False)
    return x, dm


@contextlib.contextmanager
def _launches():
    """Counts of the launches inside the body, by kernel-name prefix: ``counts(name)`` after the body; ``counts.exact``:
    the exact launch record."""
    from pointcloudcounterfactual_amd import _lib

    got = {}

    def counts(name):
        return got[name]

    with _lib.profile() as read:
        yield counts
        torch.cuda.synchronize()
        for name in ('knn_mfma_kernel', 'knn_mfma_split_kernel', 'knn_wide_select_kernel', 'knn_sorted_kernel', 'knn_small_kernel'):
            got[name] = read(name)[1]
        counts.exact = read.exact()


def _knn(xd, k, switch):
    """``ops.knn`` under one entry of SWITCHES; asserts that the intended kernel ran and the others did not."""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    tune, ran, idle = SWITCHES[switch]
    with _launches() as counts:
        with _lib.tuning(*tune) if tune else contextlib.nullcontext():
            idx = ops.knn(xd, k)
    assert counts(ran) >= 1, (switch, ran)
    assert all(counts(name) == 0 for name in idle), (switch, idle)
    # ... and the instantiation: the list width and the padded channel count of this call
    b, c, n = xd.shape
    forced = {tune[0]: tune[1]} if tune else {}
    exact = kr.kernel_of(b, c, n, k, torch.cuda.get_device_properties(xd.device).multi_processor_count,
                         nosplit=forced.get('knn_nosplit', 0), wide=forced.get('knn_wide', 0))
    assert exact.startswith(ran), (exact, ran)
    assert_only(counts.exact, exact, 'knn_sorted_kernel', 'knn_small_kernel', 'knn_mfma_kernel', 'knn_mfma_split_kernel',
                'knn_wide_select_kernel')  # (the self search never slices: no merge launch either)
    return idx


def _assert_lists(got, exp, tag):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    if not np.array_equal(got, exp):
        s, r = np.argwhere((got != exp).any(-1))[0]
        bad = int((got != exp).any(-1).sum())
        print(f'{tag}: {bad} of {got.shape[0] * got.shape[1]} rows differ; sample {s} row {r}:\n  got      {got[s, r].tolist()}\n'
              f'  expected {exp[s, r].tolist()}')
    assert np.array_equal(got, exp), tag


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)  # (-0 and +0 are one distance)


def _expected_dist(dm, exp_idx):
    """The distances of the expected lists; NaN in the padded slots (the rows' valid entries come first)."""
    d = np.take_along_axis(dm, exp_idx, axis=-1)
    valid = (~np.isnan(dm)).sum(-1)[..., None]
    return np.where(np.arange(exp_idx.shape[-1]) < valid, d, np.float32(np.nan))


@pytest.mark.parametrize('c', CS)
@pytest.mark.parametrize('kind', sc.KINDS)
def test_knn_stress_every_kernel_matches_the_oracle(cuda, oracle_mod, kind, c):
    for n in _ns(kind):
        x, dm = _case(kind, c, n)
        exp = sc.expected_lists(dm, 32)
        xd = _t(x).to(cuda)
        for switch in SWITCHES:
            for k in KS + EXTRA_KS.get(kind, ()):
                _assert_lists(_knn(xd, k, switch), exp[:, :, :k], f'{kind} c={c} n={n} k={k} {switch}')


@pytest.mark.parametrize('c', (4, 9, 17, 33, 65))
def test_knn_every_instantiation_matches_the_oracle(cuda, oracle_mod, c):
    """Every (list width, padded channel count) instantiation of the two MFMA kernels -- k at the top of every slot class
    and one above the class below, c one above every padded count -- forced through knn_nosplit, proven by the launch
    record (``_knn``) and held to the oracle's lists."""
    for kind, n in (('gauss', 300), ('twins', 130)):
        x, dm = _case(kind, c, n)
        exp = sc.expected_lists(dm, 32)
        xd = _t(x).to(cuda)
        for k in (1, 4, 5, 8, 9, 16, 17, 20, 21, 25, 26, 32):
            for switch in ('mfma', 'split'):
                _assert_lists(_knn(xd, k, switch), exp[:, :, :k], f'{kind} c={c} n={n} k={k} {switch}')


@pytest.mark.parametrize('c,n,first', [(4, 14, 6), (17, 40, 6), (64, 130, 6), (128, 130, 6), (128, 262, 6)])
def test_knn_stress_lists_that_end_in_inf(cuda, oracle_mod, c, n, first):
    """Every point from ``first`` on is big (as many as the construction allows, 2 c): a small query has fewer finite
    distances than k, so its list ends with +inf entries in index order; a big query's list holds +inf alone."""
    x = sc.overflow_cloud(13, 2, c, n, first, 1)
    _, dm = oracle_mod.knn_expanded(x, 1, return_dist=True)
    assert ((np.isfinite(dm).sum(-1) < 8) & ~np.isnan(dm).any(-1)).any()
    xd = _t(x).to(cuda)
    for k in (k for k in KS if k <= n):
        exp = sc.expected_lists(dm, k)
        for switch in SWITCHES:
            _assert_lists(_knn(xd, k, switch), exp, f'dense overflow c={c} n={n} k={k} {switch}')


@pytest.mark.parametrize('kind', ('offset64', 'twins', 'lattice', 'overflow'))
def test_knn_stress_streamed_channels(cuda, oracle_mod, kind):
    """c = 200: the channels stream through LDS in chunks; k > 32 on the wide path."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for n in (130, 300):
        x, dm = _case(kind, 200, n)
        exp = sc.expected_lists(dm, 128)
        xd = _t(x).to(cuda)
        for k in (40, 128):
            with _launches() as counts:
                idx = ops.knn(xd, k)
            assert counts('knn_wide_select_kernel') >= 1 and counts('knn_mfma_kernel') == 0
            _assert_lists(idx, exp[:, :, :k], f'{kind} c=200 n={n} k={k}')


@pytest.mark.parametrize('c', CS)
@pytest.mark.parametrize('kind', sc.KINDS)
def test_knn_stress_cross_of_a_cloud_with_itself(cuda, oracle_mod, kind, c):
    """``pcc_knn_cross(x, x)``: the indices of ``pcc_knn`` whichever kernel that runs, and the oracle's distances bit for
    bit (negative ones and +inf included); NaN only in padded slots."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for n in _ns(kind):
        x, dm = _case(kind, c, n)
        xd = _t(x).to(cuda)
        for k in KS:
            exp = sc.expected_lists(dm, k)
            idx, dist = ops.hip_knn_cross(xd, xd, k, return_distance=True)
            _assert_lists(idx, exp, f'cross {kind} c={c} n={n} k={k}')
            for switch in FORCED:
                assert torch.equal(idx, _knn(xd, k, switch)), (kind, c, n, k, switch)
            dist, want = dist.cpu().numpy(), _expected_dist(dm, exp)
            assert np.array_equal(np.isnan(dist), np.isnan(want))
            ok = ~np.isnan(want)
            assert np.array_equal(_bits(dist)[ok], _bits(want)[ok]), (kind, c, n, k)
            assert not (np.signbit(dist) & (dist == 0)).any()


@pytest.mark.parametrize('c', CS)
@pytest.mark.parametrize('kind', ('offset64', 'twins', 'lattice', 'overflow'))
def test_knn_stress_cross_of_two_clouds(cuda, oracle_mod, kind, c):
    """Queries from a different cloud of the same kind (nq = 45): the oracle searches cat([x, q]); its rows n.. against
    the columns ..n are the queries against the candidates in the library's own rounding."""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    nq = 45
    for n in (130, 300):
        x = _case(kind, c, n)[0]
        q = sc.feature_cloud(kind, 12, 2, c, nq)
        z = np.ascontiguousarray(np.concatenate([x, q], axis=2))
        _, dz = oracle_mod.knn_expanded(z, 1, return_dist=True)
        dm = np.ascontiguousarray(dz[:, n:, :n])
        xd, qd = _t(x).to(cuda), _t(q).to(cuda)
        for k in KS + (40, 128):
            exp = sc.expected_lists(dm, k)
            want = _expected_dist(dm, exp)
            ok = ~np.isnan(want)
            for split in (0, 1, 2, 7) if kind in ('twins', 'overflow') else (0,):
                with _lib.tuning('knn_cross_split', split), _launches() as counts:
                    idx, dist = ops.hip_knn_cross(qd, xd, k, return_distance=True)
                # one launch over the 2 x 45 queries; unforced, n <= 300 < 2048 candidates never slices
                sliced = kr.cross_slices(2 * nq, n, torch.cuda.get_device_properties(cuda).multi_processor_count, split) > 1
                assert_only(counts.exact, {kr.wide_select(c, k, sliced)} | ({kr.wide_merge(k)} if sliced else set()), 'knn_wide_select_kernel')
                _assert_lists(idx, exp, f'cross {kind} c={c} n={n} k={k} split={split}')
                dist = dist.cpu().numpy()
                assert np.array_equal(np.isnan(dist), ~ok), (kind, c, n, k, split)
                assert np.array_equal(_bits(dist)[ok], _bits(want)[ok]), (kind, c, n, k, split)


@pytest.mark.parametrize('kind', [k for k in sc.KINDS if k not in ('subnormal', 'overflow')])
def test_knn_stress_lists_against_float64(cuda, kind):
    """What oracle equality implies, asserted on the GPU lists directly so that a change of the formula is caught against
    float64 and not only against the oracle: every entry that differs from the float64 list is inside ``near_tie_bound``,
    and the k-th returned entry is at most the bound beyond the true k-th distance.  (``subnormal`` is outside any
    relative bound -- the spacing of subnormals is absolute -- and is held to the oracle only.)"""
    worst, differ, total = 0.0, 0, 0
    n = _ns(kind)[-1]
    for c in CS:
        x = _case(kind, c, n)[0]
        xd = _t(x).to(cuda)
        for switch in FORCED:
            idx = _knn(xd, 32, switch).cpu().numpy()
            for s in range(2):
                w, d = sc.f64_list_check(x[s], x[s], idx[s])
                worst, differ, total = max(worst, w), differ + d, total + idx[s].size
    print(f'{kind}: worst ratio to the bound {worst:.4f}; {differ} of {total} entries differ from the float64 list')
    if kind == 'gauss':
        assert differ <= 0.001 * total


@pytest.mark.parametrize('c', CS)
def test_knn_stress_exact_scaling(cuda, c):
    """Scaling by a power of two scales every product, sum and distance exactly: the lists are those of ``gauss``."""
    for n in (130, 300):
        ref = {s: _knn(_t(_case('gauss', c, n)[0]).to(cuda), 32, s) for s in FORCED}
        for kind in ('scale_up', 'scale_down'):
            xd = _t(_case(kind, c, n)[0]).to(cuda)
            for s in FORCED:
                assert torch.equal(_knn(xd, 32, s), ref[s]), (kind, c, n, s)


@pytest.mark.parametrize('c', CS)
def test_knn_stress_batch_independence(cuda, c):
    """An overflowing sample between two Gaussian ones leaves their rows as they are computed alone."""
    n = 300
    g0, ov, g1 = _case('gauss', c, n)[0][:1], _case('overflow', c, n)[0][:1], _case('gauss', c, n)[0][1:]
    batch = _t(np.ascontiguousarray(np.concatenate([g0, ov, g1], axis=0))).to(cuda)
    for switch in FORCED:
        got = _knn(batch, 32, switch)
        for pos, alone in ((0, g0), (1, ov), (2, g1)):
            ref = _knn(_t(np.ascontiguousarray(alone)).to(cuda), 32, switch)
            assert torch.equal(got[pos], ref[0]), (c, switch, pos)


@pytest.mark.parametrize('c,n,stride,kernel', [(3, 300, 1, 'knn_sorted_kernel'), (3, 2100, 1, 'knn_sorted_kernel'),
                                                (1, 300, 1, 'knn_sorted_kernel'), (2, 300, 1, 'knn_sorted_kernel'),
                                                (3, 17000, 97, 'knn_small_kernel')])
def test_knn_stress_difference_form_overflow(cuda, oracle_mod, c, n, stride, kernel):
    """c <= 3: the squares of the differences overflow, so rows mix finite and +inf distances and hold no NaN (asserted on
    the construction by the host test).  The k <= 32 kernel of the size, the wide path and ``pcc_knn_cross``."""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b = 1 if n > 3000 else 2
    x = sc.overflow_diff_cloud(17, b, c, n)
    xd = _t(x).to(cuda)
    exp = oracle_mod.knn_diff(x, 32, stride)
    for k in KS:
        with _launches() as counts:
            idx = ops.knn(xd, k)
        assert counts(kernel) >= 1 and counts('knn_wide_select_kernel') == 0
        assert kr.kernel_of(b, c, n, k).startswith(kernel + '<')
        assert_only(counts.exact, kr.kernel_of(b, c, n, k), *kr.FAMILIES)
        _assert_lists(idx[:, ::stride], exp[:, ::stride, :k], f'diff overflow c={c} n={n} k={k} {kernel}')
        with _launches() as counts, _lib.tuning('knn_wide', 1):
            idx = ops.knn(xd, k)
        assert counts('knn_wide_select_kernel') >= 1 and counts(kernel) == 0
        assert_only(counts.exact, kr.wide_select(c, k), *kr.FAMILIES)  # (c <= 3: no distance kernel)
        _assert_lists(idx[:, ::stride], exp[:, ::stride, :k], f'diff overflow c={c} n={n} k={k} wide')
        if n <= 3000:
            idx, dist = ops.hip_knn_cross(xd, xd, k, return_distance=True)
            _assert_lists(idx, exp[:, :, :k], f'diff overflow c={c} n={n} k={k} cross')
            assert not torch.isnan(dist).any() and (dist[:, :, 1:] >= dist[:, :, :-1]).all()
