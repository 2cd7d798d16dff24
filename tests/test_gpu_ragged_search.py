"""GPU tests of the searches over packed (ragged) batches (``pcc_knn_ragged``, ``pcc_ball_query_ragged`` through
``neighbour_ops``) against tests/ragged_reference.py, against the rectangular ops on every cloud alone, and against the CPU paths.

The kernels give a workgroup 64 (k-NN) or 16 (ball query) consecutive query rows and stage candidates in LDS chunks of 2048 /
tiles of 4096, so the cloud sizes lie either side of a wave, a query tile, a chunk and a tile, and the query counts are arranged
so that a 64-query tile lies inside one cloud (batch B, cloud 0), ends exactly on a cloud boundary (B: rows 64 and 128), spans
four clouds of sizes 1, 0, 2, 31 (A: rows 0-63), a cloud has points but no queries (B: cloud 2), a cloud has queries but no
points (A: clouds 1 and 6), and rows lie behind the last offset on either side (A).  A cloud one below, at and above a chunk or
a tile is scanned by queries of its own: 2047 (B), 2048 (B, S), 2049 (A, S), 4095 / 4096 / 4097 (C)."""

import functools

import numpy as np
import pytest
import torch

from tests import ragged_reference as R
from tests import unaligned_views as U
from tests import unaligned_views_ragged  # noqa: F401  (registers the two entry points' cases before the registry suites read it)
from tests.ball_query_reference import GENERIC_KINDS, GENERIC_SHAPES, between_lattice, generic_cloud
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

KS = (1, 3, 4, 5, 16, 20, 25, 32)  # every kSlots instantiation and one below each
NSAMPLES = (1, 16, 32, 64, 200)
BATCHES = {
    #     cloud sizes                                   queries per cloud                      rows of no cloud (points, queries)
    'A': ([1, 0, 2, 31, 63, 300, 0, 2049, 129], [1, 1, 1, 63, 65, 130, 64, 64, 700], (3, 5)),
    'B': ([2048, 65, 127, 2047, 4100], [64, 64, 0, 130, 700], (0, 0)),
    'C': ([4095, 4096, 4097], [1, 65, 130], (0, 0)),
    'S': ([64, 128, 1, 0, 2, 31, 65, 2048, 2049], None, (0, 0)),  # the self search
}


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@functools.lru_cache(maxsize=None)
def _inputs(name, kind):
    """``(xyz, offset, query, query_offset)`` numpy; query is None for the self search."""
    sizes, queries, (px, pq) = BATCHES[name]
    xyz, offset = R.batch(1000 + 7 * len(name + kind), sizes, kind, extra=px)
    if queries is None:
        return xyz, offset, None, None
    query, qoff = R.batch(2000 + 11 * len(name + kind), queries, kind, extra=pq)
    return xyz, offset, query, qoff


_WANT = {}


def _want(oracle_mod, name, kind):
    """The reference lists for k = 32 of a batch, computed once."""
    if (name, kind) not in _WANT:
        xyz, offset, query, qoff = _inputs(name, kind)
        _WANT[name, kind] = R.knn(oracle_mod, xyz, offset, query, qoff)
    return _WANT[name, kind]


def _knn(cuda, xyz, offset, k, query=None, qoff=None):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    args = (_dev(xyz, cuda), _dev(offset, cuda), k) + (() if query is None else (_dev(query, cuda), _dev(qoff, cuda)))
    idx, dist = ops.knn_ragged(*args, return_distance=True)
    m = len(xyz if query is None else query)
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.shape == dist.shape == (m, k)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check_against_knn_cross(cuda, xyz, offset, query, qoff, k, idx, dist):
    """``idx - lo_b`` and ``dist`` bit for bit ``hip_knn_cross`` of every cloud alone (clouds of at least k points, no NaN)."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for (lo, hi), (qlo, qhi) in zip(R.ranges(offset), R.ranges(qoff)):
        if hi - lo >= k and qhi > qlo and not np.isnan(xyz[lo:hi]).any() and not np.isnan(query[qlo:qhi]).any():
            q1, x1 = _dev(query[qlo:qhi].T, cuda)[None], _dev(xyz[lo:hi].T, cuda)[None]
            one_idx, one_dist = ops.hip_knn_cross(q1, x1, k, return_distance=True)
            assert np.array_equal(idx[qlo:qhi] - lo, one_idx[0].cpu().numpy()), (lo, hi, k)
            assert U.same_words(dist[qlo:qhi], one_dist[0].cpu().numpy()), (lo, hi, k)


CROSS = [('A', kind) for kind in R.KINDS] + [('B', 'lattice4'), ('B', 'gauss')]


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('name,kind', CROSS)
def test_knn_cross_search(cuda, oracle_mod, name, kind, k):
    """Indices word for word against the oracle (lattices: exact ties and coincident points, lowest index first), distances
    inside the bound, and both bit for bit ``pcc_knn_cross`` of each cloud alone."""
    xyz, offset, query, qoff = _inputs(name, kind)
    idx, dist = _knn(cuda, xyz, offset, k, query, qoff)
    assert np.array_equal(idx, _want(oracle_mod, name, kind)[:, :k])
    R.check_knn_dist(xyz, query, idx, dist)
    _check_against_knn_cross(cuda, xyz, offset, query, qoff, k, idx, dist)


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('kind', ['lattice4', 'gauss'])
def test_knn_self_search(cuda, oracle_mod, kind, k):
    """Without ``query`` the pointers alias; a copy of the points as queries gives the same words."""
    xyz, offset, _, _ = _inputs('S', kind)
    idx, dist = _knn(cuda, xyz, offset, k)
    assert np.array_equal(idx, _want(oracle_mod, 'S', kind)[:, :k])
    R.check_knn_dist(xyz, xyz, idx, dist)
    idx2, dist2 = _knn(cuda, xyz, offset, k, xyz.copy(), offset)
    assert np.array_equal(idx, idx2) and U.same_words(dist, dist2)
    _check_against_knn_cross(cuda, xyz, offset, xyz, offset, k, idx, dist)


@pytest.mark.parametrize('k', [4, 32])
def test_knn_non_finite_values(cuda, oracle_mod, k):
    xyz, offset, query, qoff = (a.copy() for a in _inputs('A', 'gauss'))
    xyz[97 + 17, 1] = np.nan        # a point of cloud 5 (rows 97 .. 396)
    xyz[2446 + 3, 0] = np.inf       # a point of cloud 8 (rows 2446 .. 2574)
    query[131 + 9, 2] = np.nan      # a query of cloud 5 (rows 131 .. 260)
    query[400, 0] = np.inf          # a query of cloud 8 (rows 389 .. 1088)
    want = R.knn(oracle_mod, xyz, offset, query, qoff, k)
    idx, dist = _knn(cuda, xyz, offset, k, query, qoff)
    assert np.array_equal(idx, want)
    R.check_knn_dist(xyz, query, idx, dist)
    assert (idx[140] == -1).all() and not (idx == 114).any() and not np.isnan(dist).any()
    assert (idx[400] >= 0).all() and np.isposinf(dist[400]).all() and not (idx[400] == 2449).any()  # inf - inf is NaN
    # k above the number of finite distances: the +inf point is listed last, then the padding
    small, soff = np.array([[0, 0, 0], [np.inf, 0, 0], [1, 0, 0], [np.nan, 0, 0]], np.float32), np.array([4])
    idx, dist = _knn(cuda, small, soff, 4, np.array([[0.25, 0, 0]], np.float32), np.array([1]))
    assert np.array_equal(idx, [[0, 2, 1, -1]]) and U.same_words(dist, np.array([[0.0625, 0.5625, np.inf, np.inf]], np.float32))


# ---- ball query -----------------------------------------------------------------------------------------------------------------

def _ball(cuda, xyz, offset, centres, coff, radius, nsample, pad):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    idx, cnt = ops.ball_query_ragged(_dev(xyz, cuda), _dev(offset, cuda), _dev(centres, cuda), _dev(coff, cuda), radius, nsample, pad=pad,
                                     return_count=True)
    assert idx.dtype == torch.int64 and cnt.dtype == torch.int32 and idx.shape == (len(centres), nsample) and cnt.shape == (len(centres),)
    return idx.cpu().numpy(), cnt.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ball_inputs(name, between):
    sizes, queries, (px, pq) = BATCHES[name]
    xyz, offset = R.batch(3000 + len(name), sizes, 'lattice16' if between else 'lattice4', extra=px)
    if between:
        centres, coff = R.pack([between_lattice(3100 + b, 1, m)[0] for b, m in enumerate(queries)])
        centres = np.concatenate([centres, between_lattice(3200, 1, pq)[0]], 0)
    else:
        centres, coff = R.batch(3300 + len(name), queries, 'lattice4', extra=pq)
    return xyz, offset, centres, coff, R.RaggedBall(xyz, offset, centres, coff)


@pytest.mark.parametrize('nsample', NSAMPLES)
@pytest.mark.parametrize('between', [False, True])
@pytest.mark.parametrize('name', ['A', 'B', 'C'])
def test_ball_query_exact_on_lattices(cuda, name, between, nsample):
    """Exact mode: word for word against the float64 reference, against ``hip_ball_query`` of every cloud alone and against
    the CPU path, both pads; radius 1e-4 leaves the balls between lattice points empty (FIRST: the cloud's first point)."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    xyz, offset, centres, coff, ref = _ball_inputs(name, between)
    for radius in (1e-4, 0.125, 0.2, float('inf')):
        for pad in ('first', 'none'):
            idx, cnt = _ball(cuda, xyz, offset, centres, coff, radius, nsample, pad)
            ref.check_exact(radius, nsample, pad, idx, cnt)
            if radius == 0.2 or nsample == 16:
                for (lo, hi), (qlo, qhi) in zip(R.ranges(offset), R.ranges(coff)):
                    if hi > lo and qhi > qlo:
                        one = ops.ball_query(_dev(xyz[None, lo:hi], cuda), _dev(centres[None, qlo:qhi], cuda), radius, nsample, pad=pad, return_count=True)
                        assert np.array_equal(np.where(idx[qlo:qhi] >= 0, idx[qlo:qhi] - lo, -1), one[0][0].cpu().numpy())
                        assert np.array_equal(cnt[qlo:qhi], one[1][0].cpu().numpy())
            if radius == 0.125 and name != 'C':
                cpu = ops.ball_query_ragged(*(torch.from_numpy(a) for a in (xyz[:offset[-1]], offset, centres[:coff[-1]], coff)), radius, nsample, pad=pad,
                                            return_count=True)
                assert np.array_equal(idx[:coff[-1]], cpu[0].numpy()) and np.array_equal(cnt[:coff[-1]], cpu[1].numpy())
    if between:
        idx, cnt = _ball(cuda, xyz, offset, centres, coff, 1e-4, nsample, 'first')
        assert (cnt == 0).all()
        for (lo, hi), (qlo, qhi) in zip(R.ranges(offset), R.ranges(coff)):
            assert (idx[qlo:qhi] == (lo if hi > lo else -1)).all()
        assert (idx[coff[-1]:] == -1).all()


@pytest.mark.parametrize('kind', GENERIC_KINDS)
def test_ball_query_margin_mode_on_cut_generic_clouds(cuda, kind):
    """The generic clouds, radii and seed of tests/test_gpu_ball_query.py, every cloud cut into four of unequal size; the centres
    are the first M points as there, each in the piece that holds it, so cutting only removes candidate pairs."""
    for b, n, m, r in GENERIC_SHAPES:
        x, scale = generic_cloud(11, b, n, kind)
        cuts = [0, n // 10, n // 10 + n // 20, (6 * n) // 10, n]
        xyz = np.ascontiguousarray(x.reshape(-1, 3))
        offset = np.array([s * n + c for s in range(b) for c in cuts[1:]])
        centres = np.ascontiguousarray(x[:, :m].reshape(-1, 3))
        coff = np.array([s * m + min(c, m) for s in range(b) for c in cuts[1:]])
        ref = R.RaggedBall(xyz, offset, centres, coff)
        for k, nsample in enumerate((16, 64)):
            pad = ('first', 'none')[k]
            idx, cnt = _ball(cuda, xyz, offset, centres, coff, r * scale, nsample, pad)
            ref.check_margin(r * scale, nsample, pad, idx, cnt)


# ---- independence, clipping, sampling ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['lattice4', 'gauss'])
def test_a_cloud_gives_the_same_words_wherever_it_lies(cuda, kind):
    """The same cloud first, last, in the middle of the packed array and alone: equal ``idx - lo_b``, ``dist`` and ``cnt`` words;
    and the call twice gives the same words."""
    x, q = R.cloud(71, 333, kind), R.cloud(72, 150, kind)
    others = [(R.cloud(73 + i, s, kind), R.cloud(83 + i, t, kind)) for i, (s, t) in enumerate(((65, 1), (2500, 70), (0, 9), (31, 64)))]
    base = None
    for place in (None, 0, 2, 4):
        parts = list(others) if place is not None else []
        parts.insert(place or 0, (x, q))
        xyz, offset = R.pack([p[0] for p in parts])
        query, qoff = R.pack([p[1] for p in parts])
        at = place or 0
        (lo, hi), (qlo, qhi) = R.ranges(offset)[at], R.ranges(qoff)[at]
        got = []
        for k in (5, 32):
            idx, dist = _knn(cuda, xyz, offset, k, query, qoff)
            again = _knn(cuda, xyz, offset, k, query, qoff)
            assert np.array_equal(idx, again[0]) and U.same_words(dist, again[1])
            got += [idx[qlo:qhi] - lo, U.words(dist[qlo:qhi])]
        for pad in ('first', 'none'):
            idx, cnt = _ball(cuda, xyz, offset, query, qoff, 0.3 if kind == 'lattice4' else 0.8, 20, pad)
            again = _ball(cuda, xyz, offset, query, qoff, 0.3 if kind == 'lattice4' else 0.8, 20, pad)
            assert np.array_equal(idx, again[0]) and np.array_equal(cnt, again[1])
            got += [np.where(idx[qlo:qhi] >= 0, idx[qlo:qhi] - lo, -1), cnt[qlo:qhi]]
        if base is None:
            base = got
        assert all(np.array_equal(a, b) for a, b in zip(got, base)), place


GARBAGE = [([50, 20, 10], [40, 10, 5]), ([-5, -1, 30], [-3, 0, 200]), ([10, 10 ** 9, 2 * 10 ** 9], [7, 2 ** 31 - 1, -2 ** 31]),
           ([10 ** 9, 3, -2], [0, 0, 0]), ([0, 0, 0], [10, 20, 90]), ([30, 60, 100], [90, 30, 60])]


@pytest.mark.parametrize('offset,qoff', GARBAGE)
def test_garbage_offsets_are_clipped(cuda, offset, qoff):
    """Decreasing, negative and too large offsets: every index is -1 or a row of ``xyz[0:n]``, every output word is written and
    none outside the outputs (guarded buffers).  The points sit inside a larger buffer whose other rows are copies of the
    queries' position: a row read outside ``xyz[0:n]`` would be the nearest neighbour and inside every ball, and would show as an
    index outside ``[0, n)``."""
    from pointcloudcounterfactual_amd import _lib

    n, m, k, pad_rows = 100, 90, 8, 4096
    big = torch.zeros((n + 2 * pad_rows, 3), dtype=torch.float32, device=cuda)
    big[pad_rows:pad_rows + n] = _dev(R.cloud(5, n, 'gauss') + 10.0, cuda)
    xyz = big[pad_rows:pad_rows + n]
    query = torch.zeros((m, 3), dtype=torch.float32, device=cuda)
    off, qo = torch.tensor(offset, dtype=torch.int32, device=cuda), torch.tensor(qoff, dtype=torch.int32, device=cuda)
    idx, dist = U.guarded((m, k), U.I64, cuda), U.guarded((m, k), U.F32, cuda)
    _lib.call(_lib.lib.pcc_knn_ragged, 'knn_ragged', cuda, 3, n, m, k, xyz.data_ptr(), off.data_ptr(), query.data_ptr(), qo.data_ptr(), idx.ptr(), dist.ptr())
    torch.cuda.synchronize()
    i, d = idx.numpy(), dist.numpy()
    assert ((i >= -1) & (i < n)).all() and np.isposinf(d[i < 0]).all() and (d[i >= 0] > 100).all()
    bidx, cnt = U.guarded((m, k), U.I64, cuda), U.guarded((m,), U.I32, cuda)
    for pad in (0, 1):
        _lib.call(_lib.lib.pcc_ball_query_ragged, 'ball_query_ragged', cuda, 3, n, m, k, 1e6, pad, xyz.data_ptr(), off.data_ptr(), query.data_ptr(),
                  qo.data_ptr(), bidx.ptr(), cnt.ptr())
        torch.cuda.synchronize()
        i, c = bidx.numpy(), cnt.numpy()
        assert ((i >= -1) & (i < n)).all() and ((c >= 0) & (c <= k)).all()
        assert all((row[:cc] >= 0).all() and (np.diff(row[:cc]) > 0).all() for row, cc in zip(i, c))


def test_fps_ragged_equals_the_per_cloud_sampling(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    sizes, picks = [1, 0, 2, 31, 300, 2049, 65], [1, 0, 2, 7, 64, 130, 65]
    xyz, offset = R.batch(91, sizes, 'gauss')
    new_offset = np.cumsum(picks)
    got = ops.farthest_point_sample_ragged(_dev(xyz, cuda), _dev(offset, cuda), _dev(new_offset, cuda))
    assert got.dtype == torch.int64 and got.shape == (sum(picks),) and got.device == cuda
    for (lo, hi), (qlo, qhi) in zip(R.ranges(offset), R.ranges(new_offset)):
        if qhi > qlo:
            alone = ops.hip_farthest_point_sample(_dev(xyz[None, lo:hi], cuda), qhi - qlo, None)[0]
            assert torch.equal(got[qlo:qhi], alone + lo)
    cpu = ops.farthest_point_sample_ragged(torch.from_numpy(xyz), torch.from_numpy(offset), torch.from_numpy(new_offset))
    assert cpu.shape == got.shape  # (the CPU loop has no fma: its picks are tied to the kernel's on lattices only)
    lat, loff = R.batch(92, sizes, 'lattice16')
    got = ops.farthest_point_sample_ragged(_dev(lat, cuda), _dev(loff, cuda), _dev(new_offset, cuda))
    assert torch.equal(got.cpu(), ops.farthest_point_sample_ragged(torch.from_numpy(lat), torch.from_numpy(loff), torch.from_numpy(new_offset)))


def test_binding_checks(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    xyz, offset = _dev(R.cloud(1, 50, 'gauss'), cuda), torch.tensor([20, 50], device=cuda)
    with pytest.raises(RuntimeError, match='offset must be a CUDA tensor'):
        ops.knn_ragged(xyz, offset.cpu(), 4)
    with pytest.raises(RuntimeError, match='query must be a CUDA tensor'):
        ops.knn_ragged(xyz, offset, 4, xyz.cpu(), offset)
    with pytest.raises(RuntimeError, match='centres must be a CUDA tensor'):
        ops.ball_query_ragged(xyz, offset, xyz.cpu(), offset, 1.0, 4)
    idx, dist = ops.knn_ragged(xyz, offset, 4, xyz[:0], torch.zeros(2, dtype=torch.int64, device=cuda), return_distance=True)
    assert idx.shape == dist.shape == (0, 4)
    idx = ops.knn_ragged(xyz[:0], torch.zeros(2, dtype=torch.int32, device=cuda), 4, xyz, offset)  # n = 0: every row is padding
    assert (idx == -1).all() and idx.shape == (50, 4)
    none = ops.knn_ragged(xyz, offset[:0], 3, return_distance=True)  # no cloud at all
    assert (none[0] == -1).all() and torch.isposinf(none[1]).all()
    # non-contiguous inputs give the result of their contiguous copies; int32 and int64 offsets alike
    xt = xyz.t().contiguous().t()
    assert not xt.is_contiguous() and torch.equal(ops.knn_ragged(xt, offset.int(), 4), ops.knn_ragged(xyz, offset, 4))
