"""CPU tests of grid pooling (``neighbour_ops.grid_cluster`` / ``segment_pool`` / ``grid_pool`` / ``grid_subsample`` /
``grid_unpool``): the numpy reference (tests/grid_pool_reference.py) against closed forms, the torch path of CPU tensors
against that reference word for word, the mean against ``voxelize``, CPU autograd against float64, and the argument checks of
the C ABI and of Python that need no device."""

import ctypes

import numpy as np
import pytest
import torch

from tests import grid_pool_reference as ref
from tests import voxel_reference as vref

EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
CASES = [(2, 2, 37, 5, 0), (3, 3, 70, 3, 1), (5, 1, 300, 9, 1), (32, 2, 513, 2, 0), (4, 2, 200, 8, 1)]  # (res, b, n, c, grid)


def _words(a):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def clouds():
    out = {}
    for res, b, n, c, which in CASES:
        lo, extent = vref.grid_of(res, which)
        xyz = vref.cloud(res * 1000 + n, b, n, res, lo, extent)
        out[res] = (xyz, lo, extent, vref.voxel_index(xyz, res, lo, extent))
    return out


def test_reference_each_point_in_its_own_cell():
    b, n, res, c = 2, 20, 3, 4
    xyz = vref.cloud(1, b, n, res, -0.5, 1.0, 'own_cell')
    cell, order, counts = vref.voxel_index(xyz, res, -0.5, 1.0)
    cluster, seg, count = ref.grid_cluster(cell, order, n)
    assert (count == n).all() and np.array_equal(seg, np.tile(np.arange(n + 1, dtype=np.int32), (b, 1)))
    x = vref.features(2, b, c, n)
    in_cell_order = np.take_along_axis(x, order[:, None, :].astype(np.int64).repeat(c, 1), 2)
    mean, _ = ref.segment_pool(x, order, seg, ref.MEAN)
    mx, arg = ref.segment_pool(x, order, seg, ref.MAX)
    assert np.array_equal(_words(mx), _words(in_cell_order)) and np.array_equal(arg, order[:, None, :].repeat(c, 1))
    # the mean is +0.0 + x: the feature itself, but for -0.0 and the payload of a NaN
    assert np.array_equal(_words(mean), _words(vref.canonical(F0 + in_cell_order)))
    for s in range(b):
        assert np.array_equal(cluster[s, order[s]], np.arange(n))


F0 = np.float32(0)


def test_reference_all_points_in_one_cell():
    b, n, res, c = 2, 150, 4, 3
    xyz = vref.cloud(5, b, n, res, -0.5, 1.0, 'one_cell')
    cell, order, counts = vref.voxel_index(xyz, res, -0.5, 1.0)
    for m in (1, 7, n):
        cluster, seg, count = ref.grid_cluster(cell, order, m)
        assert (count == 1).all() and (cluster == 0).all() and (seg[:, 0] == 0).all() and (seg[:, 1:] == n).all()
        x = np.random.default_rng(m).standard_normal((b, c, n)).astype(np.float32)
        acc = np.zeros((b, c), dtype=np.float32)
        for p in range(n):
            acc = acc + x[:, :, p]
        total, _ = ref.segment_pool(x, order, seg, ref.SUM)
        mx, arg = ref.segment_pool(x, order, seg, ref.MAX)
        assert np.array_equal(total[:, :, 0], acc) and (_words(total[:, :, 1:]) == 0).all()
        assert np.array_equal(mx[:, :, 0], x.max(2)) and np.array_equal(arg[:, :, 0], x.argmax(2)) and (arg[:, :, 1:] == -1).all()


def test_reference_count_unpool_and_truncation(clouds):
    for res, b, n, c, _ in CASES:
        _, _, _, (cell, order, counts) = clouds[res]
        full = ref.grid_cluster(cell, order, n)
        assert np.array_equal(full[2], (counts > 0).sum(1))  # count: the non-zeros of VoxelIndex.counts
        u = int(full[2].max())
        for m in sorted({1, max(u - 1, 1), u, min(u + 1, n), n}):
            cluster, seg, count = ref.grid_cluster(cell, order, m)
            # capacity m: capacity n restricted to its first m (+ 1) entries, apart from the -1 of the dropped ranks
            assert np.array_equal(count, full[2]) and np.array_equal(seg, full[1][:, :m + 1])
            assert np.array_equal(cluster, np.where(full[0] < m, full[0], -1))
            for s in range(b):
                kept = min(int(count[s]), m)
                assert (np.diff(seg[s, :kept + 1]) > 0).all() and (seg[s, kept:] == seg[s, kept]).all()
                assert seg[s, m] == ((cell[s] >= 0).sum() if count[s] <= m else full[1][s, m])
        # a feature that is constant on every cell comes back from pool and unpool
        cluster, seg, count = full
        x = np.where(cell >= 0, (cell % 17).astype(np.float32) - 3.5, 0)[:, None, :].repeat(c, 1).astype(np.float32)
        for mode in (ref.MEAN, ref.MAX):
            pooled, _ = ref.segment_pool(x, order, seg, mode)
            back = np.where(cluster[:, None, :] >= 0, np.take_along_axis(pooled, np.maximum(cluster, 0)[:, None, :].astype(np.int64).repeat(c, 1), 2), 0)
            assert np.array_equal(back, x)


def _capacities(u, n):
    return sorted({1, max(u - 1, 1), u, min(u + 1, n), n})


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'res{c[0]}')
def test_cpu_paths_word_for_word(clouds, case):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    res, b, n, c, _ = case
    xyz, lo, extent, (cell, order, counts) = clouds[res]
    txyz = torch.from_numpy(xyz)
    vindex = ops.voxel_index(txyz, res, lo, extent)
    u = int((counts > 0).sum(1).max())
    auto = ops.grid_cluster(vindex)
    assert auto._fields == ('cluster', 'seg', 'count', 'order') and all(t.dtype == torch.int32 for t in auto)
    assert auto.seg.shape == (b, u + 1) and auto.order is vindex.order
    x, g_all = ref.tie_features(res, b, c, n), vref.features(res + 1, b, c, n)
    for m in _capacities(u, n):
        want = ref.grid_cluster(cell, order, m)
        gi = ops.grid_cluster(vindex, m=m)
        from_cloud = ops.grid_cluster(txyz, res, lo, extent, m=m)
        for got in (gi, from_cloud):
            assert np.array_equal(got.cluster.numpy(), want[0]) and np.array_equal(got.seg.numpy(), want[1])
            assert np.array_equal(got.count.numpy(), want[2]) and np.array_equal(got.order.numpy(), order)
        if m == u:
            assert all(torch.equal(a, w) for a, w in zip(auto, gi))
        g = np.ascontiguousarray(g_all[:, :, :m])
        for name, mode in ref.MODES.items():
            want_out, want_arg = ref.segment_pool(x, order, want[1], mode)
            out, arg = ops.torch_segment_pool(torch.from_numpy(x), gi.order, gi.seg, mode)
            assert np.array_equal(_words(out), _words(want_out))
            assert arg is None if mode != ref.MAX else np.array_equal(arg.numpy(), want_arg)
            tx = torch.from_numpy(x).requires_grad_(True)
            pooled = ops.segment_pool(tx, gi, name)
            assert pooled.shape == (b, c, m) and pooled.dtype == torch.float32 and np.array_equal(_words(pooled), _words(want_out))
            pooled.backward(torch.from_numpy(g))
            assert np.array_equal(_words(tx.grad), _words(ref.segment_pool_bwd(g, want[0], want[1], want_arg, mode)))
            # unpool: the gather of the backward, on values
            back = ops.grid_unpool(torch.from_numpy(g), gi)
            assert back.shape == (b, c, n) and np.array_equal(_words(back), _words(ref.segment_pool_bwd(g, want[0], want[1], want_arg, ref.SUM)))


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'res{c[0]}')
def test_mean_is_voxelize_at_the_occupied_cells_and_grid_pool(clouds, case):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    res, b, n, c, _ = case
    xyz, lo, extent, (cell, order, counts) = clouds[res]
    txyz = torch.from_numpy(xyz)
    vindex = ops.voxel_index(txyz, res, lo, extent)
    x = vref.features(res + 2, b, c, n)
    grid = _words(ops.torch_voxelize(torch.from_numpy(x), vindex)).reshape(b, c, -1)
    pooled = ops.grid_pool(txyz, torch.from_numpy(x), res, lo, extent, reduce='mean')
    assert pooled._fields == ('xyz', 'features', 'index', 'count') and pooled.count is pooled.index.count
    m = pooled.features.shape[2]
    assert m == int((counts > 0).sum(1).max()) and pooled.xyz.shape == (b, m, 3)
    for s in range(b):
        occupied = np.flatnonzero(counts[s])
        assert np.array_equal(_words(pooled.features)[s, :, :len(occupied)], grid[s][:, occupied])
        assert (_words(pooled.features)[s, :, len(occupied):] == 0).all()  # +0 features and
        assert (_words(pooled.xyz)[s, len(occupied):] == vref.NAN_WORD).all()  # NaN centres in the padded slots
    cluster, seg, count = ref.grid_cluster(cell, order, m)
    safe = np.where(np.isfinite(xyz).all(2)[:, :, None], xyz, 0).astype(np.float32)  # (a non-finite point is in no run)
    centres, _ = ref.segment_pool(np.ascontiguousarray(safe.transpose(0, 2, 1)), order, seg, ref.MEAN)
    kept = np.arange(m)[None, :] < count[:, None]
    assert np.array_equal(_words(pooled.xyz)[kept], _words(np.ascontiguousarray(centres.transpose(0, 2, 1)))[kept])
    assert np.isfinite(pooled.xyz.numpy()[kept]).all()
    sub = ops.grid_subsample(txyz, res, lo, extent)
    assert np.array_equal(_words(sub), _words(pooled.xyz))
    mx = ops.grid_pool(txyz, torch.from_numpy(x), res, lo, extent, m=n)
    want, _ = ref.segment_pool(x, order, ref.grid_cluster(cell, order, n)[1], ref.MAX)
    assert np.array_equal(_words(mx.features), _words(want)) and mx.xyz.shape == (b, n, 3)
    assert ops.grid_pool(txyz, None, res, lo, extent, m=3).features is None


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'res{c[0]}')
def test_cpu_autograd_against_float64(clouds, case):
    """A gather, and for the mean one rounded division per element: gamma(1), taken as gamma(2).  The centres: the same for
    the points of the kept cells, nothing for a non-finite point; the partition is a constant."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    res, b, n, c, _ = case
    xyz, lo, extent, (cell, order, counts) = clouds[res]
    u = int((counts > 0).sum(1).max())
    rng = np.random.default_rng(res)
    for m in (u, max(u - 1, 1)):
        cluster, seg, count = ref.grid_cluster(cell, order, m)
        safe = np.maximum(cluster, 0).astype(np.int64)
        length = np.maximum(np.take_along_axis(np.diff(seg, axis=1), safe, 1), 1)
        live = cluster >= 0
        x = rng.standard_normal((b, c, n)).astype(np.float32)
        g = rng.standard_normal((b, c, m)).astype(np.float32)
        gathered = np.take_along_axis(g.astype(np.float64), safe[:, None, :].repeat(c, 1), 2)
        gi = ops.grid_cluster(torch.from_numpy(xyz), res, lo, extent, m=m)
        for name in ref.MODES:
            tx = torch.from_numpy(x).requires_grad_(True)
            ops.segment_pool(tx, gi, name).backward(torch.from_numpy(g))
            if name == 'max':
                _, arg = ref.segment_pool(x, order, seg, ref.MAX)
                hit = np.take_along_axis(arg, safe[:, None, :].repeat(c, 1), 2) == np.arange(n)[None, None, :]
                want = np.where(hit, gathered, 0.0)
            else:
                want = gathered / (length[:, None, :] if name == 'mean' else 1)
            want = np.where(live[:, None, :], want, 0.0)
            assert (np.abs(tx.grad.numpy() - want) <= vref.gamma(2) * np.abs(want)).all(), name
            assert (_words(tx.grad)[np.broadcast_to(~live[:, None, :], want.shape)] == 0).all()
        txyz = torch.from_numpy(xyz).requires_grad_(True)
        gc = rng.standard_normal((b, m, 3)).astype(np.float32)
        pooled = ops.grid_pool(txyz, None, res, lo, extent, m=m)
        pooled.xyz.backward(torch.from_numpy(gc))
        want = np.take_along_axis(gc.astype(np.float64), safe[:, :, None].repeat(3, 2), 1) / length[:, :, None]
        want = np.where(live[:, :, None], want, 0.0)
        assert (np.abs(txyz.grad.numpy() - want) <= vref.gamma(2) * np.abs(want)).all()
        assert (_words(txyz.grad)[~live] == 0).all()


def test_exports_views_and_the_empty_batch():
    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for name in ('GridIndex', 'GridPooled', 'grid_cluster', 'segment_pool', 'grid_pool', 'grid_subsample', 'grid_unpool'):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(ops, name)
    b, c, n, res = 2, 3, 40, 3
    xyz = torch.from_numpy(vref.cloud(1, b, n, res, -0.5, 1.0))
    gi = ops.grid_cluster(xyz, res)
    xv = torch.randn(b, 2 * c, 2 * n)[:, ::2, ::2]
    assert torch.equal(ops.segment_pool(xv, gi, 'max'), ops.segment_pool(xv.contiguous(), gi, 'max'))
    empty = ops.grid_cluster(xyz[:0], res)
    assert empty.cluster.shape == (0, n) and empty.seg.shape == (0, 2) and empty.count.shape == (0,)
    assert ops.grid_cluster(xyz[:0], res, m=5).seg.shape == (0, 6)
    assert ops.segment_pool(torch.zeros(0, c, n), empty).shape == (0, c, 1)
    pooled = ops.grid_pool(xyz[:0], torch.zeros(0, c, n), res, m=4)
    assert pooled.xyz.shape == (0, 4, 3) and pooled.features.shape == (0, c, 4)
    # a cloud without a finite point: no cell, one padded slot
    none = ops.grid_pool(torch.full((1, 5, 3), float('nan')), torch.ones(1, 2, 5), res)
    assert none.count.tolist() == [0] and none.xyz.shape == (1, 1, 3) and torch.isnan(none.xyz).all()
    assert (_words(none.features) == 0).all() and (none.index.cluster == -1).all() and none.index.seg.tolist() == [[0, 0]]


def test_argument_errors():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    xyz, x = torch.rand(2, 10, 3) - 0.5, torch.zeros(2, 4, 10)
    vindex = ops.voxel_index(xyz, 5)
    gi = ops.grid_cluster(vindex, m=6)
    for bad in (xyz[0], xyz[:, :, :2], xyz[:, :0], torch.zeros(1, ops.MAX_VOXEL_POINTS + 1, 3)):
        with pytest.raises(ValueError, match='grid_cluster: expected xyz'):
            ops.grid_cluster(bad, 5)
        with pytest.raises(ValueError, match='grid_pool: expected xyz'):
            ops.grid_pool(bad, None, 5)
    with pytest.raises(ValueError, match='resolution is needed'):
        ops.grid_cluster(xyz)
    with pytest.raises(ValueError, match="not the index's"):
        ops.grid_cluster(vindex, 6)
    for res in (1, 129, 2.0, True):
        with pytest.raises(ValueError, match='resolution'):
            ops.grid_cluster(xyz, res)
    for m in (0, 11, -1, 2.0, True, 'all'):
        with pytest.raises(ValueError, match='grid_cluster: m must be'):
            ops.grid_cluster(vindex, m=m)
        with pytest.raises(ValueError, match='grid_cluster: m must be'):
            ops.grid_pool(xyz, x, 5, m=m)
    for bad in (None, (vindex.cell, vindex.order, vindex.counts), 5):
        with pytest.raises(ValueError, match='grid_cluster: expected a VoxelIndex or xyz'):
            ops.grid_cluster(bad, 5)
    with pytest.raises(ValueError, match='grid_cluster: expected index.cell and index.order'):
        ops.grid_cluster(ops.VoxelIndex(vindex.cell, vindex.order[:, :9], vindex.counts))
    with pytest.raises(RuntimeError, match='index.cell must be torch'):
        ops.grid_cluster(ops.VoxelIndex(vindex.cell.long(), vindex.order, vindex.counts))
    with pytest.raises(RuntimeError, match='xyz must be torch'):
        ops.grid_cluster(xyz.double(), 5)
    with pytest.raises(ValueError, match='too large'):
        ops.grid_cluster(torch.zeros(65536, 1, 3), 2, m=1)
    for reduce in ('min', None, 0, 'MAX'):
        with pytest.raises(ValueError, match='reduce must be'):
            ops.segment_pool(x, gi, reduce)
        with pytest.raises(ValueError, match='reduce must be'):
            ops.grid_pool(xyz, x, 5, reduce=reduce)
    for bx, bi in ((x[0], gi), (x[:, :0], gi), (x[:, :, :9], gi), (x[:1], gi), (x, vindex), (x, tuple(gi)), (x, None),
                   (x, ops.GridIndex(gi.cluster, gi.seg[:, :1], gi.count, gi.order)),
                   (x, ops.GridIndex(gi.cluster, gi.seg.reshape(-1), gi.count, gi.order)),
                   (x, ops.GridIndex(gi.cluster, torch.zeros(2, 12, dtype=torch.int32), gi.count, gi.order)),
                   (x, ops.GridIndex(gi.cluster, gi.seg, gi.count[:1], gi.order)),
                   (x, ops.GridIndex(gi.cluster, gi.seg, gi.count, gi.order[:, :9]))):
        with pytest.raises(ValueError, match='segment_pool:'):
            ops.segment_pool(bx, bi)
    for bx, bi, name in ((x.double(), gi, 'features'), (x, ops.GridIndex(gi.cluster.long(), gi.seg, gi.count, gi.order), 'index.cluster'),
                         (x, ops.GridIndex(gi.cluster, gi.seg.long(), gi.count, gi.order), 'index.seg'),
                         (x, ops.GridIndex(gi.cluster, gi.seg, gi.count.long(), gi.order), 'index.count'),
                         (x, ops.GridIndex(gi.cluster, gi.seg, gi.count, gi.order.long()), 'index.order')):
        with pytest.raises(RuntimeError, match=f'{name} must be torch'):
            ops.segment_pool(bx, bi)
    with pytest.raises(RuntimeError, match='expected cpu'):
        ops.segment_pool(x, ops.GridIndex(gi.cluster.to('meta'), gi.seg, gi.count, gi.order))
    for bf in (x[0], x[:1], x[:, :, :9], x[:, :0]):
        with pytest.raises(ValueError, match='grid_pool: expected features'):
            ops.grid_pool(xyz, bf, 5)
    with pytest.raises(RuntimeError, match='features must be torch'):
        ops.grid_pool(xyz, x.double(), 5)
    pooled = torch.zeros(2, 4, 6)
    for bp, bi in ((pooled[0], gi), (pooled[:1], gi), (pooled[:, :0], gi), (pooled[:, :, :5], gi), (pooled, vindex), (pooled, None)):
        with pytest.raises(ValueError, match='grid_unpool:'):
            ops.grid_unpool(bp, bi)
    with pytest.raises(RuntimeError, match='pooled must be torch'):
        ops.grid_unpool(pooled.double(), gi)
    with pytest.raises(RuntimeError, match='expected cpu'):
        ops.grid_unpool(pooled, ops.GridIndex(gi.cluster, gi.seg.to('meta'), gi.count, gi.order))


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched: the guard stays)."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)(*([0x5a] * 64))
    p = ctypes.addressof(buf)
    fns = {
        'grid_cluster': lambda b, c, n, m, mode, q=p: L.pcc_grid_cluster(b, n, m, q, q, q, q, q, None),
        'segment_pool': lambda b, c, n, m, mode, q=p: L.pcc_segment_pool(b, c, n, m, mode, q, q, q, q, q, None),
        'segment_pool_bwd': lambda b, c, n, m, mode, q=p: L.pcc_segment_pool_bwd(b, c, n, m, mode, q, q, q, q, q, None),
    }
    # (b, c, n, m, mode): sizes every entry point refuses, the empty batch included
    sizes = [(-1, 3, 8, 4, 0), (65536, 3, 8, 4, 0), (1, 3, 0, 1, 0), (1, 3, 8, 0, 0), (1, 3, 8, 9, 0), (1, 3, 8, -1, 0),
             (65535, 3, 1 << 15, 4, 0), (32768, 3, (1 << 16) - 1, 4, 0), (0, 3, 0, 4, 0), (0, 3, 8, 9, 0)]
    for name, fn in fns.items():
        for args in sizes:
            assert fn(*args) == EINVAL, (name, args)
            assert L.pcc_last_error().decode().startswith(name + ':'), (name, args)
        if name != 'grid_cluster':
            for c in (0, -1):
                assert fn(1, c, 8, 4, 0) == EINVAL and L.pcc_last_error().decode().startswith(name + ': c must be')
            for mode in (-1, 3):
                assert fn(1, 3, 8, 4, mode) == EINVAL and L.pcc_last_error().decode().startswith(name + ': mode must be')
        assert fn(1, 3, 8, 4, 0, None) == EINVAL
        assert L.pcc_last_error().decode().startswith(name + ': null pointer')
        # an empty batch enqueues nothing, whatever the pointers
        for mode in (0, 1, 2):
            assert fn(0, 3, 8, 4, mode, None) == 0 and L.pcc_last_status() == 0
    # every pointer on its own (arg may be null in the forward, and in the backward unless the mode is max: a call with
    # such a null and nothing else wrong would be enqueued, so it is not made here)
    for i in range(5):
        q = [p] * 5
        q[i] = None
        assert L.pcc_grid_cluster(1, 8, 4, *q, None) == EINVAL
        for mode in (0, 1, 2):
            if i < 4:
                assert L.pcc_segment_pool(1, 3, 8, 4, mode, *q, None) == EINVAL, (i, mode)
            if i != 2 or mode == 2:
                assert L.pcc_segment_pool_bwd(1, 3, 8, 4, mode, *q, None) == EINVAL, (i, mode)
    # the largest cloud one workgroup scans is named in the message; the pooling itself has no such limit
    assert L.pcc_grid_cluster(1, vref.MAX_POINTS + 1, 4, p, p, p, p, p, None) == EINVAL
    assert L.pcc_last_error().decode() == f'grid_cluster: n must be <= {vref.MAX_POINTS}'
    assert bytes(buf) == b'\x5a' * 64


def test_the_abi_is_bound_and_the_tuning_table_is_untouched():
    from pointcloudcounterfactual_amd import _lib

    assert [len(_lib.ABI[f][1]) for f in ('pcc_grid_cluster', 'pcc_segment_pool', 'pcc_segment_pool_bwd')] == [9, 11, 11]
    assert len(_lib.TUNING) == 16 and max(_lib.TUNING.values()) == 15
