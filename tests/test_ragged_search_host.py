"""The searches over packed (ragged) batches without a device: the reference of tests/ragged_reference.py against closed forms,
the CPU paths of ``knn_ragged`` / ``ball_query_ragged`` / ``farthest_point_sample_ragged`` against the reference, the offset
helpers, the argument errors, and every refusal of the two C entry points (they come back before anything is enqueued)."""

import ctypes

import numpy as np
import pytest
import torch

from pointcloudcounterfactual_amd import neighbour_ops as ops
from tests import ragged_reference as R
from tests.ball_query_reference import between_lattice
from tests import unaligned_views_ragged  # noqa: F401  (registers the two entry points' cases before the registry suites read it)
from tests.unaligned_views import same_words

SIZES = [1, 0, 2, 31, 63, 300, 0, 129, 65]
QUERIES = [1, 1, 1, 63, 65, 130, 64, 0, 64]


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ---- the reference against closed forms ---------------------------------------------------------------------------------------

def test_reference_two_identical_clouds_give_the_same_local_lists(oracle_mod):
    x = R.cloud(1, 50, 'gauss')
    xyz, offset = R.pack([x, x])
    idx = R.knn(oracle_mod, xyz, offset, k=8)
    assert np.array_equal(idx[:50], idx[50:] - 50) and (idx[:50] < 50).all() and (idx[:, 0] == np.arange(100)).all()
    q = R.cloud(2, 7, 'gauss')
    query, qoff = R.pack([q, q])
    idx = R.knn(oracle_mod, xyz, offset, query, qoff, k=8)
    assert np.array_equal(idx[:7], idx[7:] - 50)
    d = ((x[None].astype(np.float64) - q[:, None].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(idx[:7], np.argsort(d, 1, kind='stable')[:, :8])  # (no near ties among 50 Gaussian points)


def test_reference_short_clouds_nan_and_rows_of_no_cloud(oracle_mod):
    one, three = np.array([[1, 2, 3]], np.float32), R.cloud(3, 3, 'lattice4')
    xyz, offset = R.pack([one, three])
    idx = R.knn(oracle_mod, xyz, offset, k=5)
    assert np.array_equal(idx[0], [0, -1, -1, -1, -1])  # a cloud of one point
    assert (np.sort(idx[1:, :3], 1) == [1, 2, 3]).all() and (idx[1:, 3:] == -1).all()  # k above the cloud: n_b real slots
    # a NaN point is never listed; a NaN query gives a padded row; +inf is listed behind the finite distances
    x = R.cloud(4, 20, 'gauss')
    x[5, 1], x[9, 0] = np.nan, np.inf
    q = R.cloud(5, 4, 'gauss')
    q[2, 2] = np.nan
    idx = R.knn(oracle_mod, x, np.array([20]), q, np.array([4]), k=20)
    assert not (idx == 5).any() and (idx[2] == -1).all()
    for i in (0, 1, 3):
        assert idx[i, 18] == 9 and idx[i, 19] == -1 and sorted(idx[i, :19]) == [j for j in range(20) if j != 5]
    self_idx = R.knn(oracle_mod, x, np.array([20]), k=20)
    assert (self_idx[5] == -1).all() and np.array_equal(self_idx[9, :18], [j for j in range(20) if j not in (5, 9)]) and (self_idx[9, 18:] == -1).all()
    # queries behind the last offset, points behind the last offset
    idx = R.knn(oracle_mod, np.concatenate([x, x]), np.array([20]), np.concatenate([q, q]), np.array([4]), k=3)
    assert (idx[4:] == -1).all() and (idx[:4] < 20).all()
    R.check_knn_dist(x, q, idx[:4], np.where(idx[:4] >= 0, ((x[np.maximum(idx[:4], 0)] - q[:, None]) ** 2).sum(-1), np.inf).astype(np.float32))


def test_reference_ball_rows_of_no_cloud_and_empty_clouds():
    x, off = R.batch(6, [4, 0, 9], 'lattice4', extra=2)
    c, coff = R.batch(7, [2, 3, 1], 'lattice4', extra=1)
    ref = R.RaggedBall(x, off, c, coff)
    for pad in ('first', 'none'):
        idx, cnt = ref.query(10.0, 5, pad)
        assert (idx[2:5] == -1).all() and (cnt[2:5] == 0).all() and (idx[6] == -1).all() and cnt[6] == 0
        assert np.array_equal(idx[0], [0, 1, 2, 3, 0 if pad == 'first' else -1]) and np.array_equal(idx[5], [4, 5, 6, 7, 8]) and cnt[5] == 5
    idx, cnt = ref.query(1e-4, 3, 'first')  # (a ball this small holds coincident points only; FIRST names the cloud's first point otherwise)
    assert ((idx[:2] >= 0) & (idx[:2] < 4)).all() and (idx[5] >= 4).all() and (idx[5] < 13).all()


# ---- the CPU paths against the reference ---------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['lattice4', 'lattice16'])
def test_cpu_knn_word_for_word_on_lattices(oracle_mod, kind):
    """Lattice coordinates: every product and sum is exact, so the CPU path's float32 distances are the oracle's, ties
    (coincident points included) go to the lowest index, and the distances are the float64 values."""
    xyz, offset = R.batch(10, SIZES, kind, extra=0)
    query, qoff = R.batch(20, QUERIES, kind, extra=0)
    want, want_self = R.knn(oracle_mod, xyz, offset, query, qoff), R.knn(oracle_mod, xyz, offset)
    for k in (1, 3, 4, 5, 16, 20, 25, 32):
        idx, dist = ops.knn_ragged(_t(xyz), _t(offset), k, _t(query), _t(qoff), return_distance=True)
        assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.shape == dist.shape == (len(query), k)
        assert np.array_equal(idx.numpy(), want[:, :k]), k
        R.check_knn_dist(xyz, query, idx.numpy(), dist.numpy())
        real = want[:, :k] >= 0
        d64 = ((xyz[np.maximum(want[:, :k], 0)].astype(np.float64) - query[:, None].astype(np.float64)) ** 2).sum(-1)
        assert same_words(dist.numpy(), np.where(real, d64, np.inf).astype(np.float32))
        assert np.array_equal(ops.knn_ragged(_t(xyz), _t(offset).int(), k).numpy(), want_self[:, :k]), k


@pytest.mark.parametrize('kind', ['gauss', 'gauss_x100', 'gauss_x1e-3', 'gauss_+50'])
def test_cpu_knn_bounded_on_generic_clouds(kind):
    """No fma on the CPU path, so a near tie may come out in the other order: the returned distances are within 5 ulp of
    float64 for the returned indices, rows ascend, and the k-th distance is at most (1 + 2^-20) times the true k-th."""
    xyz, offset = R.batch(30, SIZES, kind)
    query, qoff = R.batch(40, QUERIES, kind)
    k = 16
    idx, dist = ops.knn_ragged(_t(xyz), _t(offset), k, _t(query), _t(qoff), return_distance=True)
    idx, dist = idx.numpy(), dist.numpy()
    R.check_knn_dist(xyz, query, idx, dist)
    for (lo, hi), (qlo, qhi) in zip(R.ranges(offset), R.ranges(qoff)):
        real = min(k, hi - lo)
        assert (idx[qlo:qhi, :real] >= lo).all() and (idx[qlo:qhi, :real] < hi).all() and (idx[qlo:qhi, real:] == -1).all()
        if real and qhi > qlo:
            d64 = np.sort(((xyz[None, lo:hi].astype(np.float64) - query[qlo:qhi, None].astype(np.float64)) ** 2).sum(-1), 1)
            assert (dist[qlo:qhi, real - 1].astype(np.float64) <= (1 + 2.0 ** -20) * d64[:, real - 1]).all()
            assert all(len(set(row[:real])) == real for row in idx[qlo:qhi])


def test_cpu_knn_non_finite_values(oracle_mod):
    xyz, offset = R.batch(50, [40, 30], 'lattice16')
    xyz[7, 0], xyz[45, 2] = np.nan, np.inf
    query, qoff = R.batch(60, [9, 5], 'lattice16')
    query[3, 1] = np.nan
    want = R.knn(oracle_mod, xyz, offset, query, qoff)
    idx, dist = ops.knn_ragged(_t(xyz), _t(offset), 32, _t(query), _t(qoff), return_distance=True)
    assert np.array_equal(idx.numpy(), want)
    R.check_knn_dist(xyz, query, idx.numpy(), dist.numpy())
    assert (want[3] == -1).all() and not (want == 7).any() and (want[9:, 29] == 45).all() and (want[9:, 30:] == -1).all()
    assert np.array_equal(ops.knn_ragged(_t(xyz), _t(offset), 32).numpy(), R.knn(oracle_mod, xyz, offset))


def test_cpu_ball_query_word_for_word():
    xyz, offset = R.batch(70, SIZES, 'lattice16')
    centres, coff = R.pack([between_lattice(80 + b, 1, m)[0] for b, m in enumerate(QUERIES)])
    ref = R.RaggedBall(xyz, offset, centres, coff)
    for radius in (1e-4, 0.125, 0.25, 10.0, float('inf')):
        for nsample in (1, 16, 200):
            for pad in ('first', 'none'):
                idx, cnt = ops.ball_query_ragged(_t(xyz), _t(offset), _t(centres), _t(coff), radius, nsample, pad=pad, return_count=True)
                assert cnt.dtype == torch.int32 and cnt.shape == (len(centres),) and idx.shape == (len(centres), nsample)
                ref.check_exact(radius, nsample, pad, idx.numpy(), cnt.numpy())
    idx = ops.ball_query_ragged(_t(xyz), _t(offset), _t(centres), _t(coff), 1e-4, 4)
    for (lo, hi), (qlo, qhi) in zip(R.ranges(offset), R.ranges(coff)):
        assert (idx[qlo:qhi].numpy() == (lo if hi > lo else -1)).all()  # empty balls: the cloud's first point


def test_cpu_fps_equals_the_per_cloud_sampling():
    xyz, offset = R.batch(90, [1, 0, 2, 31, 300, 65], 'gauss')
    picks = [1, 0, 2, 7, 64, 65]
    new_offset = np.cumsum(picks)
    got = ops.farthest_point_sample_ragged(_t(xyz), _t(offset), _t(new_offset))
    assert got.dtype == torch.int64 and got.shape == (sum(picks),)
    for (lo, hi), (qlo, qhi) in zip(R.ranges(offset), R.ranges(new_offset)):
        if qhi > qlo:
            alone = ops.farthest_point_sample(_t(xyz[None, lo:hi]), qhi - qlo, start=0)[0]
            assert torch.equal(got[qlo:qhi], alone + lo)
    with pytest.raises(ValueError, match='more picks than it has points'):
        ops.farthest_point_sample_ragged(_t(xyz), _t(offset), _t(np.cumsum([1, 1, 2, 7, 64, 65])))
    with pytest.raises(ValueError, match='offset must be non-decreasing'):
        ops.farthest_point_sample_ragged(_t(xyz), _t(offset[:-1].tolist() + [5]), _t(new_offset))
    assert ops.farthest_point_sample_ragged(_t(xyz), _t(offset), _t(np.zeros(6, np.int64))).shape == (0,)


# ---- offsets -------------------------------------------------------------------------------------------------------------------

def test_offset_helpers_round_trip():
    offset = torch.tensor([3, 3, 10, 11])
    batch = ops.offset2batch(offset)
    assert batch.dtype == torch.int64 and batch.tolist() == [0] * 3 + [2] * 7 + [3]
    assert torch.equal(ops.batch2offset(batch), offset) and ops.batch2offset(batch).dtype == torch.int64
    assert ops.offset2bincount(offset).tolist() == [3, 0, 7, 1]
    assert torch.equal(ops.batch2offset(ops.offset2batch(offset.int())), offset)
    assert ops.offset2batch(torch.zeros(0, dtype=torch.int64)).shape == (0,)
    with pytest.raises(ValueError, match='int32 or int64'):
        ops.offset2batch(torch.tensor([1.0, 2.0]))
    import pointcloudcounterfactual_amd as pkg
    for name in ('offset2batch', 'batch2offset', 'offset2bincount', 'knn_ragged', 'ball_query_ragged', 'farthest_point_sample_ragged'):
        assert getattr(pkg, name) is getattr(ops, name) and name in pkg.__all__


def test_offset_validation_and_argument_errors():
    xyz, q = torch.zeros(10, 3), torch.zeros(4, 3)
    good, qgood = torch.tensor([4, 10]), torch.tensor([1, 4])
    for bad in ([4, 9], [4, 11], [11, 10], [-1, 10]):
        with pytest.raises(ValueError, match='offset must be non-decreasing'):
            ops.knn_ragged(xyz, torch.tensor(bad), 2, q, qgood)
        with pytest.raises(ValueError, match='offset must be non-decreasing'):
            ops.ball_query_ragged(xyz, torch.tensor(bad), q, qgood, 1.0, 2)
    with pytest.raises(ValueError, match='query_offset must be non-decreasing'):
        ops.knn_ragged(xyz, good, 2, q, torch.tensor([3, 2]))
    with pytest.raises(ValueError, match='centre_offset must be non-decreasing'):
        ops.ball_query_ragged(xyz, good, q, torch.tensor([1, 5]), 1.0, 2)
    for k in (0, 33, 2.0, True):
        with pytest.raises(ValueError, match=r'k must be an integer in \[1, 32\]'):
            ops.knn_ragged(xyz, good, k)
    with pytest.raises(ValueError, match='come together'):
        ops.knn_ragged(xyz, good, 2, q)
    with pytest.raises(ValueError, match=r'expected xyz\[n,3\]'):
        ops.knn_ragged(torch.zeros(1, 10, 3), good, 2)
    with pytest.raises(ValueError, match=r'query_offset\[B = 2\]'):
        ops.knn_ragged(xyz, good, 2, q, torch.tensor([4]))
    with pytest.raises(RuntimeError, match='xyz must be torch.float32'):
        ops.knn_ragged(xyz.double(), good, 2)
    with pytest.raises(ValueError, match='radius must be > 0'):
        ops.ball_query_ragged(xyz, good, q, qgood, 0.0, 2)
    with pytest.raises(ValueError, match="pad must be 'first' or 'none'"):
        ops.ball_query_ragged(xyz, good, q, qgood, 1.0, 2, pad='zero')
    with pytest.raises(ValueError, match='nsample must be an int >= 1'):
        ops.ball_query_ragged(xyz, good, q, qgood, 1.0, 0)
    # the outputs are constants of the graph
    idx, dist = ops.knn_ragged(xyz.clone().requires_grad_(True), good, 2, return_distance=True)
    assert not idx.requires_grad and not dist.requires_grad


# ---- the C entry points without a device ---------------------------------------------------------------------------------------

def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched), and so does PCC_OK of a
    call with nothing to do."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    knn = lambda b, n, m, k, *ptrs: L.pcc_knn_ragged(b, n, m, k, *ptrs, None, None)  # noqa: E731  (dist and stream NULL)
    assert knn(0, 8, 4, 2, None, None, None, None, None) == 0  # b = 0: nothing to do
    assert knn(3, 8, 0, 2, None, None, None, None, None) == 0  # m = 0
    for args, word in [((1, 8, 4, 0, p, p, p, p, p), 'bad size'), ((1, 8, 4, 33, p, p, p, p, p), 'k > 32 is not supported'),
                       ((-1, 8, 4, 2, p, p, p, p, p), 'bad size'), ((1, -1, 4, 2, p, p, p, p, p), 'bad size'),
                       ((1, 8, -1, 2, p, p, p, p, p), 'bad size'), ((65536, 8, 4, 2, p, p, p, p, p), 'batch too large'),
                       ((1, 8, 4, 2, None, p, p, p, p), 'null pointer'), ((1, 8, 4, 2, p, None, p, p, p), 'null pointer'),
                       ((1, 8, 4, 2, p, p, None, p, p), 'null pointer'), ((1, 8, 4, 2, p, p, p, None, p), 'null pointer'),
                       ((1, 8, 4, 2, p, p, p, p, None), 'null pointer'), ((0, 8, 4, 33, p, p, p, p, p), 'k > 32')]:
        assert knn(*args) != 0, args
        assert L.pcc_last_error().decode() == 'knn_ragged: ' + word or word in L.pcc_last_error().decode(), (args, L.pcc_last_error())
        assert L.pcc_last_error().decode().startswith('knn_ragged:')
    ball = lambda b, n, m, ns, r, pad, *ptrs: L.pcc_ball_query_ragged(b, n, m, ns, r, pad, *ptrs, None, None)  # noqa: E731
    assert ball(0, 8, 4, 2, 1.0, 0, None, None, None, None, None) == 0
    assert ball(3, 8, 0, 2, 1.0, 1, None, None, None, None, None) == 0
    bad = [(1, 0, 4, 2, 1.0, 0, p, p, p, p, p), (1, 8, 4, 0, 1.0, 0, p, p, p, p, p), (1, 8, 4, 2, 0.0, 0, p, p, p, p, p),
           (1, 8, 4, 2, -1.0, 0, p, p, p, p, p), (1, 8, 4, 2, float('nan'), 0, p, p, p, p, p), (1, 8, 4, 2, 1.0, 2, p, p, p, p, p),
           (1, 8, 4, 2, 1.0, -1, p, p, p, p, p), (65536, 8, 4, 2, 1.0, 0, p, p, p, p, p), (-1, 8, 4, 2, 1.0, 0, p, p, p, p, p),
           (1, 8, -1, 2, 1.0, 0, p, p, p, p, p), (1, 8, 4, 2, 1.0, 0, None, p, p, p, p), (1, 8, 4, 2, 1.0, 0, p, None, p, p, p),
           (1, 8, 4, 2, 1.0, 0, p, p, None, p, p), (1, 8, 4, 2, 1.0, 0, p, p, p, None, p), (1, 8, 4, 2, 1.0, 0, p, p, p, p, None),
           (0, 8, 4, 2, 0.0, 0, p, p, p, p, p), (1, 8, 0, 0, 1.0, 0, p, p, p, p, p)]  # (an empty call is still checked)
    for args in bad:
        assert ball(*args) != 0, args
        assert L.pcc_last_error().decode().startswith('ball_query_ragged:')


def test_the_registry_of_unaligned_views_holds_both_entry_points():
    """tests/unaligned_views_ragged.py has appended one case per entry point, once, whatever imported it first."""
    from tests import unaligned_views as U

    names = [case.name for case in U.CASES]
    assert all(names.count(name) == 1 for name in unaligned_views_ragged.NAMES)
    assert {'pcc_knn_ragged', 'pcc_ball_query_ragged'} <= U.covered()
    for case in U.CASES:
        if case.name in unaligned_views_ragged.NAMES:
            assert case.dims['b'] == 2 and max(case.dims.values()) <= 512 and case.anchor is not None and case.cpu
