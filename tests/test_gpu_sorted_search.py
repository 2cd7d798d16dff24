"""The Hilbert sort (``am_sort_kernel<SLOTS>``) and the two searches on its output -- the c <= 3 k-NN graph
(``knn_sorted_kernel``) and the nearest-neighbour half of ``pcc_chamfer_emd`` (``nn_sorted_kernel``) -- at every size
class of the sort and on the clouds of tests/sorted_search_clouds.py; and ``ChamferEMD`` on non-finite points.

Everything is bit-exact: the k-NN lists against ``oracle_mod.knn_diff``, ``NNDistance`` against
``oracle_mod.nndistance``, ``ChamferEMD``'s neighbours, distances and loss against ``NNDistance`` / ``ChamferLoss``.
Which kernel and which instantiation of the sort a case ran is read from the library's profiler and asserted, so a case
cannot drift onto another path unnoticed.

Size classes of the sort (512 threads x SLOTS keys): 4 -> 2048 points, 8 -> 4096, 16 -> 8192, 32 -> 16384,
64 -> 32768; larger clouds keep their order.  The k-NN graph uses the sorted search up to 16384 points.
"""

import contextlib
import ctypes

import numpy as np
import pytest
import torch

from tests import knn_reference as kr
from tests.sorted_search_clouds import KINDS, channels_major, stress_cloud
from tests.util import pair
from tests.which_ran import assert_only
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu


def _dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _launches(prefix):
    """Launches recorded by the library's profiler whose kernel name starts with ``prefix``."""
    from pointcloudcounterfactual_amd import _lib

    count = ctypes.c_int(0)
    _lib.lib.pcc_profile_read(prefix.encode(), None, ctypes.byref(count))
    return count.value


@contextlib.contextmanager
def _profiled():
    """``launches(prefix)`` over the body's launches; ``launches.exact()``: the exact launch record."""
    from pointcloudcounterfactual_amd import _lib

    with _lib.profile() as read:  # (cleared and enabled on entry, disabled behind the body)
        def launches(prefix):
            return _launches(prefix)

        launches.exact = read.exact
        yield launches


def _sort_slots(*sizes):
    """The instantiation that sorts clouds of these sizes in one launch (the largest decides; a cloud of more than
    32768 points is not sorted and does not count)."""
    slots = 4
    for n in sizes:
        if n <= 32768:
            while 512 * slots < n:
                slots *= 2
    return slots


def _ran_only(launches, family, name):
    """Every launch of the kernels whose names start with ``family`` was one of ``name``, and there was one."""
    return launches(name) >= 1 and launches(family) == launches(name)


# ---- k-NN graph ------------------------------------------------------------------------------------------------------

_KNN_ORACLE = {}
KMAX = 32


def _knn_oracle(oracle_mod, x, key, stride):
    """Oracle lists of length 32 for the queries q % stride == 0 and for the last query, computed once per cloud: a
    shorter list is a prefix (the lists are sorted by (distance, index)).  -> (rows[b, nq], lists[b, nq, k])"""
    if key not in _KNN_ORACLE:
        n = x.shape[2]
        k = min(KMAX, n)
        rows = np.arange(0, n, stride)
        lists = oracle_mod.knn_diff(x, k, stride)[:, rows]
        if rows[-1] != n - 1:  # stride n - 1 computes the queries 0 and n - 1
            last = oracle_mod.knn_diff(x, k, n - 1)[:, n - 1:]
            rows, lists = np.append(rows, n - 1), np.concatenate([lists, last], axis=1)
        lists.setflags(write=False)
        _KNN_ORACLE[key] = rows, lists
    return _KNN_ORACLE[key]


def _check_knn(cuda, oracle_mod, x, k, key, stride, kernel=None):
    """``knn(x, k)`` equals the oracle on the sampled queries; -> the index tensor (host)."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    n = x.shape[2]
    with _profiled() as launches:
        idx = ops.knn(_dev(x, cuda), k).cpu().numpy()
        if kernel is not None:
            other = 'knn_small_kernel' if kernel == 'knn_sorted_kernel' else 'knn_sorted_kernel'
            assert launches(kernel) >= 1 and launches(other) == 0, (kernel, n)
            exact = kr.kernel_of(x.shape[0], x.shape[1], n, k)  # ... in the instantiation of this list width
            assert exact.startswith(kernel + '<'), (exact, kernel)
            assert_only(launches.exact(), exact, *kr.FAMILIES)
            if kernel == 'knn_sorted_kernel':
                assert _ran_only(launches, 'am_sort_kernel', f'am_sort_kernel<{_sort_slots(n)}>'), n
            else:
                assert launches('am_sort_kernel') == 0, n
    assert idx.shape == (x.shape[0], n, k) and idx.min() >= 0 and idx.max() < n
    rows, lists = _knn_oracle(oracle_mod, x, key, stride)
    assert np.array_equal(idx[:, rows], lists[:, :, :k]), key
    return idx


@pytest.mark.parametrize('k', [1, 20, 32])
@pytest.mark.parametrize('kind', ['surface', 'lattice'])
@pytest.mark.parametrize('n', [8191, 8192, 8193, 12001, 16383, 16384, 16385])
def test_knn_sorted_search_size_classes(cuda, oracle_mod, n, kind, k):
    """The sorted k-NN search between 8191 and 16384 points -- four to eight windows of 128 blocks, 16-bit merge indices
    above 8191, am_sort_kernel<16> up to 8192 points and <32> behind it -- and the exhaustive kernel from 16385.  Every
    37th query (odd: every position inside a box of 16 is sampled) and the last one against the oracle.  (The lattice at
    16385 points is also the regression test of the exhaustive kernel's merge: its four waves take a quarter of every
    2048-candidate chunk each, and a tie between two waves used to go to the earlier wave instead of the lower index.)"""
    x = channels_major(stress_cloud(kind, 100 + n, 1, n))
    _check_knn(cuda, oracle_mod, x, k, ('size', kind, n), 37,
               kernel='knn_sorted_kernel' if n <= 16384 else 'knn_small_kernel')


@pytest.mark.parametrize('k', [4, 5, 8, 9, 16, 17, 21, 26])
def test_knn_exhaustive_kernel_every_list_width(cuda, oracle_mod, k):
    """The exhaustive kernel (16385 points) in every list-width instantiation, at both ends of the slot classes (k = 1, 20
    and 32 are in the size classes above); the launch record names the instantiation."""
    n = 16385
    x = channels_major(stress_cloud('surface', 100 + n, 1, n))
    _check_knn(cuda, oracle_mod, x, k, ('size', 'surface', n), 37, kernel='knn_small_kernel')


def test_knn_sorted_search_two_channels_two_samples(cuda, oracle_mod):
    """b = 2, c = 2, n = 9000: the third coordinate of the sort reads as 0, am_sort_kernel<32>."""
    x = channels_major(stress_cloud('surface', 9000, 2, 9000), (0, 1))
    _check_knn(cuda, oracle_mod, x, 20, ('c2', 9000), 37, kernel='knn_sorted_kernel')


KNN_GEOMETRY = [(2, 3, 2100, 20), (1, 3, 257, 32), (2, 3, 4100, 7)]


@pytest.mark.parametrize('b,c,n,k', KNN_GEOMETRY)
@pytest.mark.parametrize('kind', KINDS)
def test_knn_on_stress_clouds(cuda, oracle_mod, kind, b, c, n, k):
    cloud = stress_cloud(kind, 200 + n, b, n)
    stride = 5 if n == 4100 else 1
    _check_knn(cuda, oracle_mod, channels_major(cloud), k, ('geo', kind, b, n), stride, kernel='knn_sorted_kernel')
    # the flat kinds once more on their non-degenerate channels alone
    sub = {'line': [(0,)], 'plane': [(0,), (0, 1)]}.get(kind, [])
    for ch in sub:
        _check_knn(cuda, oracle_mod, channels_major(cloud, ch), k, ('geo', kind, b, n, ch), stride,
                   kernel='knn_sorted_kernel')


@pytest.mark.parametrize('kind', ['surface', 'clusters'])
def test_knn_is_invariant_under_power_of_two_scaling(cuda, oracle_mod, kind):
    """``knn(x * 2^s)`` for s = -40, +40 lists exactly the indices of ``knn(x)``: the scaling commutes with every float32
    operation of the sort and of the search (differences, products, fused sums, ``1023 / extent``; the squared
    distances stay far inside the normal range), and each result equals the oracle on its own input."""
    x = channels_major(stress_cloud(kind, 77, 1, 2100))
    base = _check_knn(cuda, oracle_mod, x, 20, ('scale', kind, 0), 1)
    for s in (-40, 40):
        xs = x * np.float32(2.0 ** s)
        assert np.array_equal(xs * np.float32(2.0 ** -s), x)  # (the scaling itself is exact)
        got = _check_knn(cuda, oracle_mod, xs, 20, ('scale', kind, s), 1)
        assert np.array_equal(got, base), s


def test_knn_nan_candidates_in_two_windows(cuda, oracle_mod):
    """n = 2100 (two windows of 128 blocks), NaN points at the original indices 5 and 2070: no finite query ever lists
    them, the other lists are the oracle's on the cloud without the two (re-indexed), every index lies in the cloud."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    n, k, bad = 2100, 20, (5, 2070)
    x = channels_major(stress_cloud('surface', 31, 1, n))
    x[0, 1, bad[0]] = np.nan
    x[0, :, bad[1]] = np.nan
    idx = ops.knn(_dev(x, cuda), k).cpu().numpy()
    assert idx.min() >= 0 and idx.max() < n
    ok = np.ones(n, bool)
    ok[list(bad)] = False
    assert not np.isin(idx[0, ok], bad).any()
    ref = oracle_mod.knn_diff(np.ascontiguousarray(x[:, :, ok]), k)[0]
    ref = ref + (ref >= bad[0])    # indices of the cloud without the two points -> original numbering
    ref = ref + (ref >= bad[1])
    assert np.array_equal(idx[0, ok], ref)


# ---- nearest neighbours: NNDistance against the oracle, ChamferEMD against NNDistance -----------------------------------


def _check_chamfer_emd_neighbours(cuda, a, c, slots=None):
    """The assertions of test_chamfer_emd_neighbours_are_the_exhaustive_ones (tests/test_gpu_structural.py) on indices,
    distances and the loss; -> (NNDistance's outputs on the host, ChamferEMD's index tensors)."""
    from pointcloudcounterfactual_amd import backend

    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    d1, i1, d2, i2 = backend.NNDistance(t1, t2)
    with _profiled() as launches:
        loss, j1, j2, _cost, e1, e2 = backend.ChamferEMD(t1, t2, True, False, return_dist=True)
        torch.cuda.synchronize()
        assert launches('nn_sorted_kernel') >= 1
        if slots is not None:
            assert _ran_only(launches, 'am_sort_kernel', f'am_sort_kernel<{slots}>'), slots
    assert torch.equal(j1, i1) and torch.equal(j2, i2)
    assert torch.equal(e1, d1) and torch.equal(e2, d2)
    ref_loss = backend.ChamferLoss(t1, t2, True)[0]
    assert torch.equal(loss, ref_loss)
    return [t.cpu().numpy() for t in (d1, i1, d2, i2)]


@pytest.mark.parametrize('kind', ['surface', 'lattice'])
@pytest.mark.parametrize('b,n,m', [(1, 8193, 300), (1, 300, 16384), (1, 16385, 64), (1, 32768, 40), (1, 40, 32769)])
def test_chamfer_emd_neighbours_size_classes(cuda, kind, b, n, m):
    """am_sort_kernel<32> (8193 and 16384 points), <64> (16385 and 32768, the last sorted size) and the first size
    that keeps its order (32769: only the 40-point cloud is sorted, by <4>), each as the query cloud and as the
    candidate cloud of one direction."""
    a, c = stress_cloud(kind, 300 + n, b, n), stress_cloud(kind, 301 + m, b, m)
    _check_chamfer_emd_neighbours(cuda, a, c, slots=_sort_slots(n, m))


NN_GEOMETRY = [(2, 2100, 2049), (1, 257, 130), (1, 4100, 17)]


@pytest.mark.parametrize('b,n,m', NN_GEOMETRY)
@pytest.mark.parametrize('kind', KINDS)
def test_nearest_neighbours_on_stress_clouds(cuda, oracle_mod, kind, b, n, m):
    """Two clouds of one kind (different seeds): the exhaustive ``NNDistance`` equals the oracle, the sorted search of
    ``ChamferEMD`` equals ``NNDistance``."""
    a, c = stress_cloud(kind, 400 + n, b, n), stress_cloud(kind, 401 + n, b, m)
    d1, i1, d2, i2 = _check_chamfer_emd_neighbours(cuda, a, c, slots=_sort_slots(n, m))
    od1, oi1, od2, oi2 = oracle_mod.nndistance(a, c)
    assert np.array_equal(i1, oi1) and np.array_equal(i2, oi2)
    assert np.array_equal(d1, od1) and np.array_equal(d2, od2)


@pytest.mark.parametrize('b,n', [(2, 2100), (1, 257), (1, 4100)])
def test_nearest_neighbours_of_a_lattice_in_its_copy(cuda, oracle_mod, b, n):
    """``lattice`` against a copy of itself: every point finds its own position at distance 0 -- about n / 216 candidates
    tie there, in boxes all over the sorted order, and the lowest original index among them (the first point of that
    position, the point itself only if it is that one) must win in both directions."""
    a = stress_cloud('lattice', 500 + n, b, n)
    d1, i1, d2, i2 = _check_chamfer_emd_neighbours(cuda, a, a.copy(), slots=_sort_slots(n))
    od1, oi1, od2, oi2 = oracle_mod.nndistance(a, a)
    assert np.array_equal(i1, oi1) and np.array_equal(i2, oi2) and np.array_equal(d1, od1) and np.array_equal(d2, od2)
    assert (d1 == 0).all() and (d2 == 0).all() and np.array_equal(i1, i2)
    for s in range(b):
        _pos, first, inverse = np.unique(a[s], axis=0, return_index=True, return_inverse=True)
        assert np.array_equal(i1[s], first[inverse.reshape(-1)])
        assert (i1[s] <= np.arange(n)).all() and (i1[s] < np.arange(n)).any()


# ---- ChamferEMD on non-finite points ---------------------------------------------------------------------------------

NF_B, NF_N, NF_M = 3, 600, 513


def _poison(case, a, c):
    """Changes sample 1 only.  -> (rows of cloud 1 / cloud 2 of sample 1 that hold a NaN, every query of sample 1 sees
    NaN candidates only)"""
    if case == 'nan_coordinate_cloud1':
        a[1, 100, 1] = np.nan
        return [100], [], False
    if case == 'nan_coordinate_cloud2':
        c[1, 100, 1] = np.nan
        return [], [100], False
    if case == 'nan_point_at_index_0_of_cloud2':
        c[1, 0, :] = np.nan
        return [], [0], False
    if case == 'inf_coordinate_cloud1':
        a[1, 100, 1] = np.inf
        return [], [], False
    assert case == 'cloud2_all_nan'
    c[1] = np.nan
    return [], list(range(NF_M)), True


NF_CASES = ['nan_coordinate_cloud1', 'nan_coordinate_cloud2', 'nan_point_at_index_0_of_cloud2', 'inf_coordinate_cloud1',
            'cloud2_all_nan']


def _in_range(idx, size):
    """Host copy of an index tensor, asserted to lie inside a cloud of ``size`` points BEFORE anything gathers through it."""
    host = idx.detach().cpu().numpy()
    assert host.min() >= 0 and host.max() < size, (int(host.min()), int(host.max()), size)
    return host


@pytest.fixture(scope='module')
def nf_clean(cuda):
    """The clean batch, run once: forward outputs and the gradients of ``(chamfer + emd).sum()``."""
    from pointcloudcounterfactual_amd import backend, losses

    a, c = pair(8100, NF_B, NF_N, NF_M, 'recon')
    fwd = [t.cpu().numpy() for t in backend.ChamferEMD(_dev(a, cuda), _dev(c, cuda), True, False, return_dist=True)]
    t1, t2 = _dev(a, cuda).requires_grad_(True), _dev(c, cuda).requires_grad_(True)
    cham, emd = losses.chamfer_emd(t1, t2)
    (cham + emd).sum().backward()
    grads = t1.grad.cpu().numpy(), t2.grad.cpu().numpy()
    assert all(np.isfinite(x).all() for x in fwd) and all(np.isfinite(g).all() for g in grads)
    for x in (a, c, *fwd, *grads):
        x.setflags(write=False)
    return a, c, fwd, grads


@pytest.mark.parametrize('case', NF_CASES)
def test_chamfer_emd_non_finite_points_stay_inside_the_clouds(cuda, nf_clean, case):
    """A NaN or infinite coordinate in one sample of a ``ChamferEMD`` batch: every index written lies inside the other
    cloud (the backward gathers through them), a NaN query gets distance NaN / index 0 as in ``pcc_nndistance``, the
    sample's Chamfer loss is NaN whenever one of its distances is, and the other samples carry the bits of the clean
    batch -- forward and backward.  No index reaches a backward call before it has been checked on the host."""
    from pointcloudcounterfactual_amd import backend, losses

    ca, cc, clean, clean_grads = nf_clean
    a, c = ca.copy(), cc.copy()
    nan1, nan2, all_nan = _poison(case, a, c)
    loss, j1, j2, cost, e1, e2 = backend.ChamferEMD(_dev(a, cuda), _dev(c, cuda), True, False, return_dist=True)
    i1, i2 = _in_range(j1, NF_M), _in_range(j2, NF_N)
    loss, cost, e1, e2 = (t.cpu().numpy() for t in (loss, cost, e1, e2))
    for rows, dist, idx in ((nan1, e1, i1), (nan2, e2, i2)):
        assert np.isnan(dist[1, rows]).all() and (idx[1, rows] == 0).all(), case
    if all_nan:  # every candidate distance of every query of cloud 1 is NaN
        assert np.isnan(e1[1]).all() and (i1[1] == 0).all()
    if np.isnan(e1[1]).any() or np.isnan(e2[1]).any():
        assert np.isnan(loss[1]), case
    assert bool(nan1 or nan2) == bool(np.isnan(e1[1]).any() or np.isnan(e2[1]).any())
    keep = [0, 2]
    for got, want in zip((loss, i1, i2, cost, e1, e2), clean):
        assert np.array_equal(got[keep], want[keep]), case

    t1, t2 = _dev(a, cuda).requires_grad_(True), _dev(c, cuda).requires_grad_(True)
    cham, emd = losses.chamfer_emd(t1, t2)
    saved = cham.grad_fn.saved_tensors  # (t1, t2, idx1, idx2, emd_grad1, emd_grad2): what the backward will gather through
    assert saved[2].dtype == torch.int32 and saved[2].shape == (NF_B, NF_N) and saved[3].shape == (NF_B, NF_M)
    _in_range(saved[2], NF_M)
    _in_range(saved[3], NF_N)
    (cham + emd).sum().backward()
    g1, g2 = t1.grad.cpu().numpy(), t2.grad.cpu().numpy()
    assert np.array_equal(g1[keep], clean_grads[0][keep]) and np.array_equal(g2[keep], clean_grads[1][keep]), case
    assert np.isnan(g1[1]).any() and np.isnan(g2[1]).any(), case
