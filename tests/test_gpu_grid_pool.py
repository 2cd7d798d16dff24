"""GPU tests of grid pooling (``pcc_grid_cluster``, ``pcc_segment_pool`` / ``_bwd`` through the C ABI on guarded, prefilled
buffers, and ``neighbour_ops.grid_cluster`` / ``segment_pool`` / ``grid_pool`` / ``grid_unpool``) against the numpy loops of
tests/grid_pool_reference.py and the CPU path: every output word for word, the gradients included (they are gathers), so
nothing here has a tolerance; independence of the batch and of the run; one level of an encoder end to end."""

import numpy as np
import pytest
import torch

from tests import grid_pool_reference as ref
from tests import voxel_reference as vref
from tests.which_ran import ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 32        # words of sentinel around every output
INT_FILL = -7777  # what an int32 output holds before the call


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _words(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


class _Out:
    """An output of ``shape`` inside a flat buffer with GUARD sentinel words on either side.  Floats start as NaN with a
    payload no kernel produces, integers as INT_FILL: every element must be written, and nothing around it."""

    FLOAT_FILL = 0x7fdead00

    def __init__(self, shape, dtype, cuda):
        self.is_float = dtype == torch.float32
        numel = int(np.prod(shape))
        self.flat = torch.full((numel + 2 * GUARD,), self.FLOAT_FILL if self.is_float else INT_FILL, dtype=torch.int32, device=cuda)
        self.lo, self.hi = GUARD, GUARD + numel
        self.view = self.flat[self.lo:self.hi].view(shape)

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self, untouched=False):
        flat = self.flat.cpu().numpy()
        fill = np.int32(self.FLOAT_FILL) if self.is_float else INT_FILL
        assert (np.concatenate((flat[:self.lo], flat[self.hi:])) == fill).all()
        body = flat[self.lo:self.hi].reshape(self.view.shape)
        assert (body == fill).all() if untouched else not (body == fill).any()
        return body.view(np.float32) if self.is_float else body


def _call(name, dev, *args):
    from pointcloudcounterfactual_amd import _lib

    _lib.call(getattr(_lib.lib, 'pcc_' + name), name, dev, *args)


def _index(xyz, res, lo, extent):
    """``pcc_voxel_index`` of the device cloud ``xyz``: ``(cell, order)`` on the device."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    index = ops.voxel_index(xyz, res, lo, extent)
    return index.cell, index.order


def _cluster(cell, order, m):
    b, n = cell.shape
    dev = cell.device
    cluster, seg, count = _Out((b, n), torch.int32, dev), _Out((b, m + 1), torch.int32, dev), _Out((b,), torch.int32, dev)
    _call('grid_cluster', dev, b, n, m, cell.data_ptr(), order.data_ptr(), cluster.ptr(), seg.ptr(), count.ptr())
    return (cluster, seg, count), (cluster.numpy(), seg.numpy(), count.numpy())


def _pool(x, order, seg, mode, with_arg=True):
    """``(out, arg)`` as numpy; ``arg`` is checked to stay untouched outside mode max."""
    b, c, n = x.shape
    m = seg.shape[1] - 1
    out, arg = _Out((b, c, m), torch.float32, x.device), _Out((b, c, m), torch.int32, x.device)
    _, names = ran(lambda: _call('segment_pool', x.device, b, c, n, m, mode, x.data_ptr(), order.data_ptr(), seg.data_ptr(), out.ptr(),
                                 arg.ptr() if with_arg else None))
    assert set(names) == (ref.pool_kernels(n) if b else set()), (n, names)  # (the variant the size predicts, no sibling)
    written = mode == ref.MAX and with_arg
    return out.numpy(), arg.numpy(untouched=not written)


def _pool_bwd(g, cluster, seg, arg, mode, n):
    b, c, m = g.shape
    gx = _Out((b, c, n), torch.float32, g.device)
    _, names = ran(lambda: _call('segment_pool_bwd', g.device, b, c, n, m, mode, cluster.data_ptr(), seg.data_ptr(),
                                 None if arg is None else arg.data_ptr(), g.data_ptr(), gx.ptr()))
    assert set(names) == ({ref.pool_bwd_kernel(m, mode)} if b else set()), (m, mode, names)
    return gx.numpy()


def _check_all(cuda, xyz, res, lo, extent, x, g, capacities, cpu=True):
    """Every output of the three entry points on the clouds ``xyz`` with features ``x[b,c,n]`` and gradients ``g[b,c,>=m]``
    at every capacity, against the numpy loops and (``cpu``) the CPU path.  Returns the numpy reference at the last
    capacity."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, n = xyz.shape[:2]
    cell, order, counts = vref.voxel_index(xyz, res, lo, extent)
    dcell, dorder = _index(_dev(xyz, cuda), res, lo, extent)
    assert np.array_equal(dcell.cpu().numpy(), cell) and np.array_equal(dorder.cpu().numpy(), order)
    dx = _dev(x, cuda)
    vindex_cpu = ops.VoxelIndex(torch.from_numpy(cell), torch.from_numpy(order), torch.from_numpy(counts).view(b, res, res, res))
    for m in capacities:
        want = ref.grid_cluster(cell, order, m)
        outs, got = _cluster(dcell, dorder, m)
        for gt, w, name in zip(got, want, ('cluster', 'seg', 'count')):
            assert np.array_equal(gt, w), (res, m, name)
        gi_cpu = ops.grid_cluster(vindex_cpu, m=m) if cpu else None
        if cpu:
            assert all(np.array_equal(t.numpy(), w) for t, w in zip(gi_cpu[:3], want))
        dseg, dcluster = outs[1].view, outs[0].view
        gm = np.ascontiguousarray(g[:, :, :m])
        dg = _dev(gm, cuda)
        for name, mode in ref.MODES.items():
            want_out, want_arg = ref.segment_pool(x, order, want[1], mode)
            out, arg = _pool(dx, dorder, dseg, mode)
            assert np.array_equal(_words(out), _words(want_out)), (res, m, name)
            if mode == ref.MAX:
                assert np.array_equal(arg, want_arg), (res, m)
            want_gx = ref.segment_pool_bwd(gm, want[0], want[1], want_arg, mode)
            gx = _pool_bwd(dg, dcluster, dseg, _dev(want_arg, cuda) if mode == ref.MAX else None, mode, n)
            assert np.array_equal(_words(gx), _words(want_gx)), (res, m, name)
            if cpu:
                tx = torch.from_numpy(x).requires_grad_(True)
                pooled = ops.segment_pool(tx, gi_cpu, name)
                pooled.backward(torch.from_numpy(gm))
                assert np.array_equal(_words(pooled), _words(out)) and np.array_equal(_words(tx.grad), _words(gx)), (res, m, name)
    return (cell, order, counts), want


def _three_clouds(n, res, lo, extent):
    """Rows 0 and 2: one mixed cloud (outside the cube, midpoints, nodes, a NaN point first, a +inf point last, a -inf and a
    NaN point inside) at two batch positions; row 1, with another number of occupied cells: every point in its own cell
    where the grid has that many, all in one cell where not."""
    mixed = vref.cloud(7 * n + res, 1, n, res, lo, extent)
    return np.concatenate((mixed, vref.cloud(n + res, 1, n, res, lo, extent, 'own_cell' if n <= res ** 3 else 'one_cell'), mixed))


# a wave, a wave and a point; the scan's 1024 threads with one position each, then two; 16 positions per thread
SIZES = (1, 63, 64, 65, 256, 257, ref.SCAN_THREADS, ref.SCAN_THREADS + 1, 4097, vref.MAX_POINTS)


@pytest.mark.parametrize('n', SIZES)
def test_sizes_word_for_word(cuda, n):
    """B = 3 with a different number of occupied cells per cloud, at the capacity of the fullest cloud (the others are
    padded) and, for the integers, at capacity n; the words of a cloud at every batch position, alone and twice."""
    c = ref.CB + 1
    for res, which in ((2, 0), (3, 1), (32, 1), (128, 0)):
        lo, extent = vref.grid_of(res, which)
        xyz = _three_clouds(n, res, lo, extent)
        x = ref.tie_features(n + res, 2, c, n)[[0, 1, 0]]
        cell, order, counts = vref.voxel_index(xyz, res, lo, extent)
        u = (counts > 0).sum(1)
        m = max(1, int(u.max()))
        assert n < 4 or u[0] != u[1]
        g = vref.features(n + res + 1, 3, c, m)
        _check_all(cuda, xyz, res, lo, extent, x, g, (m,), cpu=n <= 4097)
        # the integers at capacity n; a cloud's words at every batch position, alone, and in a second run
        dcell, dorder = _index(_dev(xyz, cuda), res, lo, extent)
        _, full = _cluster(dcell, dorder, n)
        for gt, w in zip(full, ref.grid_cluster(cell, order, n)):
            assert np.array_equal(gt, w)
        outs, got = _cluster(dcell, dorder, m)
        _, alone = _cluster(dcell[:1].contiguous(), dorder[:1].contiguous(), m)
        _, again = _cluster(dcell, dorder, m)
        for gt, a, r in zip(got, alone, again):
            assert np.array_equal(gt[0], gt[2]) and np.array_equal(a[0], gt[0]) and np.array_equal(r, gt)
        dx = _dev(x, cuda)
        for mode in ref.MODES.values():
            out, arg = _pool(dx, dorder, outs[1].view, mode)
            one, one_arg = _pool(dx[:1].contiguous(), dorder[:1].contiguous(), outs[1].view[:1].contiguous(), mode)
            twice, twice_arg = _pool(dx, dorder, outs[1].view, mode)
            assert np.array_equal(_words(out[0]), _words(out[2])) and np.array_equal(_words(one[0]), _words(out[0]))
            assert np.array_equal(_words(twice), _words(out)) and np.array_equal(twice_arg, arg) and np.array_equal(one_arg[0], arg[0])


@pytest.mark.parametrize('c', (1, 3, ref.CB - 1, ref.CB, ref.CB + 1, 64, 65))
def test_channels_and_capacities(cuda, c):
    """The channel block of a thread and the 64 lanes of a long run, on a cloud with short and long runs, at the capacities
    1, U - 1, U, U + 1 and n (U: the fullest cloud's cells; the other clouds are padded or cut elsewhere)."""
    n, res = 600, 3
    lo, extent = vref.grid_of(res, 0)
    xyz = _three_clouds(n, res, lo, extent)
    _, _, counts = vref.voxel_index(xyz, res, lo, extent)
    u = int((counts > 0).sum(1).max())
    assert counts.max() > ref.LONG_RUN and u > 2
    x = ref.tie_features(c, 3, c, n) if c % 2 else vref.features(c, 3, c, n)
    _check_all(cuda, xyz, res, lo, extent, x, vref.features(c + 1, 3, c, n), (1, u - 1, u, u + 1, n))


def test_runs_of_exactly_64_and_65_points(cuda):
    """Either side of the cut between a thread's chain and a wave's: runs of 1, 63, 64, 65, 66, 128 and 129 points in one cloud."""
    lengths = (64, 1, 65, 63, 129, 64, 66, 128, 65)
    res, c = 3, 11
    xyz = ref.run_cloud(3, 2, res, lengths)
    n = xyz.shape[1]
    (_, _, counts), want = _check_all(cuda, xyz, res, 0.0, float(res - 1), ref.tie_features(1, 2, c, n), vref.features(2, 2, c, n), (len(lengths), 5))
    assert sorted(counts[0][counts[0] > 0]) == sorted(lengths)


def test_all_points_in_one_cell_and_each_in_its_own(cuda):
    """The sequential chain of a run is part of the contract; a cell holding the whole cloud stays bounded (the channels go
    across the lanes of a wave).  And n runs of one point."""
    b, c, n, res = 2, 64, 2048, 32
    xyz = vref.cloud(3, b, n, res, -0.5, 1.0, 'one_cell')
    x = vref.features(9, b, c, n)
    x[np.isinf(x) | np.isnan(x)] = 1.0  # (one NaN would be the whole cell: keep the sum a test of its order)
    (_, _, counts), _ = _check_all(cuda, xyz, res, -0.5, 1.0, x, vref.features(10, b, c, n), (1, 2))
    assert (counts.max(1) == n).all()
    xyz = vref.cloud(4, b, n, res, -0.5, 1.0, 'own_cell')
    (_, _, counts), (_, _, count) = _check_all(cuda, xyz, res, -0.5, 1.0, ref.tie_features(11, b, 5, n), vref.features(12, b, 5, n), (n - 1, n))
    assert counts.max() == 1 and (count == n).all()


@pytest.mark.parametrize('n, slots', ((ref.LDS_ROWS_N[8] + 1, None), (ref.LDS_MAX_N, None), (ref.LDS_MAX_N + 1, None),
                                      (ref.LDS_MAX_BWD_M + 400, ref.LDS_MAX_BWD_M), (ref.LDS_MAX_BWD_M + 400, ref.LDS_MAX_BWD_M + 1)))
def test_rows_in_lds_and_rows_too_long_for_it(cuda, n, slots):
    """The two entry points on a partition made by hand: the first size with fewer than 8 rows of x per workgroup; the longest
    row of x a workgroup stages in LDS and the first it gathers from global memory instead (longer than ``pcc_voxel_index``
    sorts); the same cut for the rows of the backward, whose length is the number of slots."""
    b, c = 2, ref.CB + 1
    order, seg, cluster = ref.random_runs(n, b, n, slots=slots)
    m = seg.shape[1] - 1
    assert slots is None or m == slots
    x, g = ref.tie_features(n, b, c, n), vref.features(n + 1, b, c, m)
    dx, dg, dorder, dseg, dcluster = (_dev(a, cuda) for a in (x, g, order, seg, cluster))
    for mode in ref.MODES.values():
        want_out, want_arg = ref.segment_pool(x, order, seg, mode)
        out, arg = _pool(dx, dorder, dseg, mode)
        assert np.array_equal(_words(out), _words(want_out)) and (mode != ref.MAX or np.array_equal(arg, want_arg)), mode
        gx = _pool_bwd(dg, dcluster, dseg, _dev(want_arg, cuda) if mode == ref.MAX else None, mode, n)
        assert np.array_equal(_words(gx), _words(ref.segment_pool_bwd(g, cluster, seg, want_arg, mode))), mode


def test_mean_is_voxelize_at_the_occupied_cells(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, n, res = 3, 9, 700, 4
    xyz = _three_clouds(n, res, -0.5, 1.0)
    x = vref.features(5, b, c, n)
    dxyz, dx = _dev(xyz, cuda), _dev(x, cuda)
    vindex = ops.voxel_index(dxyz, res)
    grid = _words(ops.voxelize(dx, vindex)).reshape(b, c, -1)
    pooled = ops.grid_pool(dxyz, dx, res, reduce='mean')
    counts = vindex.counts.cpu().numpy().reshape(b, -1)
    assert pooled.count.cpu().tolist() == (counts > 0).sum(1).tolist() and counts.max() > ref.LONG_RUN
    for s in range(b):
        occupied = np.flatnonzero(counts[s])
        assert np.array_equal(_words(pooled.features)[s, :, :len(occupied)], grid[s][:, occupied])
        assert (_words(pooled.features)[s, :, len(occupied):] == 0).all()
        assert (_words(pooled.xyz)[s, len(occupied):] == vref.NAN_WORD).all()


def test_more_channel_blocks_than_a_launch_has_rows(cuda):
    """c > 65535 * CB: more blocks of channels than a launch has rows.  Rows this short are staged in LDS, whose kernels deal
    the blocks of channels as the workgroups of a one-dimensional launch; the kernels that gather from global memory would
    stride over the blocks beyond gridDim.y, but only at sizes (n > 40000 with this c: 84 GB) no test can hold."""
    c, n, b, res = 65535 * ref.CB + ref.CB + 1, 3, 1, 2
    xyz = vref.cloud(res, b, 8, res, -0.5, 1.0)[:, 1:1 + n]  # (two finite points around a NaN one)
    cell, order, _ = vref.voxel_index(xyz, res, -0.5, 1.0)
    cluster, seg, count = ref.grid_cluster(cell, order, 2)
    assert (cell[0] >= 0).sum() == 2
    rng = np.random.default_rng(res)
    x, g = rng.standard_normal((b, c, n)).astype(np.float32), rng.standard_normal((b, c, 2)).astype(np.float32)
    dx, dg, dorder, dseg, dcluster = (_dev(a, cuda) for a in (x, g, order, seg, cluster))
    for mode in ref.MODES.values():
        want_out, want_arg = ref.segment_pool(x, order, seg, mode)
        out, arg = _pool(dx, dorder, dseg, mode)
        assert np.array_equal(_words(out), _words(want_out)) and (mode != ref.MAX or np.array_equal(arg, want_arg))
        gx = _pool_bwd(dg, dcluster, dseg, _dev(want_arg, cuda) if mode == ref.MAX else None, mode, n)
        assert np.array_equal(_words(gx), _words(ref.segment_pool_bwd(g, cluster, seg, want_arg, mode)))
    out, _ = _pool(dx, dorder, dseg, ref.MAX, with_arg=False)  # (arg may be null)
    assert np.array_equal(_words(out), _words(want_out))


def test_autograd_against_the_cpu_path(cuda):
    """``segment_pool``, ``grid_pool`` (features and centres) and ``grid_unpool`` on both devices: outputs and gradients word
    for word; nothing is computed for a gradient nobody asked for."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, n, res = 3, 5, 400, 4
    xyz = _three_clouds(n, res, -0.5, 1.0)
    rng = np.random.default_rng(4)
    x = rng.standard_normal((b, c, n)).astype(np.float32)
    for m in (None, 7):
        for reduce in ref.MODES:
            got = []
            for dev in (torch.device('cpu'), cuda):
                tx, txyz = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(xyz).to(dev).requires_grad_(True)
                pooled = ops.grid_pool(txyz, tx, res, m=m, reduce=reduce)
                cap = pooled.features.shape[2]
                gen = np.random.default_rng(cap)
                gf, gc = (torch.from_numpy(gen.standard_normal(s).astype(np.float32)).to(dev) for s in ((b, c, cap), (b, cap, 3)))
                torch.autograd.backward((pooled.features, pooled.xyz), (gf, gc))
                # unpooling sums the gradients of a slot's points in an order of its own (group_points): small integers,
                # whose sums are exact in any order
                leaf = pooled.features.detach().requires_grad_(True)
                back = ops.grid_unpool(leaf, pooled.index)
                back.backward(torch.from_numpy(gen.integers(-8, 9, size=(b, c, n)).astype(np.float32)).to(dev))
                got.append([t.detach().cpu() for t in (pooled.features, pooled.xyz, back, leaf.grad, tx.grad, txyz.grad, *pooled.index)])
            for a, d in zip(*got):
                assert a.shape == d.shape and np.array_equal(_words(a), _words(d)), (m, reduce)
    gi = ops.grid_cluster(torch.from_numpy(xyz).to(cuda), res)
    assert not ops.segment_pool(torch.from_numpy(x).to(cuda), gi).requires_grad


def test_one_level_end_to_end(cuda):
    """``grid_pool`` -> ``knn_cross(k = 3)`` from the dense cloud into the pooled one -> ``interpolate_points``, on both
    devices: no list names a padded slot whenever the cloud has at least 3 occupied cells, and the result is finite."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, n, res = 3, 6, 500, 6
    xyz = np.concatenate((vref.cloud(1, 1, n, res, -0.5, 1.0), vref.cloud(2, 1, n, 3, -0.5, 1.0),
                          ref.run_cloud(3, 1, res, (100, 150, 250)) / np.float32(res - 1) - np.float32(0.5)))
    finite = np.isfinite(xyz).all(2)
    xyz[~finite] = 0.25  # (a non-finite dense point has no neighbours to propagate from: not this test's subject)
    x = np.random.default_rng(6).standard_normal((b, c, n)).astype(np.float32)
    results = []
    for dev in (torch.device('cpu'), cuda):
        txyz, tx = torch.from_numpy(xyz).to(dev), torch.from_numpy(x).to(dev).requires_grad_(True)
        pooled = ops.grid_pool(txyz, tx, res)
        counts = pooled.count.cpu().numpy()
        m = pooled.xyz.shape[1]
        assert m == counts.max() and counts.min() == 3 and (counts < m).any()  # (padded slots exist, and a cloud of 3 cells)
        idx, dist = ops.knn_cross(txyz.transpose(1, 2), pooled.xyz.detach().transpose(1, 2), 3, return_distance=True)
        assert (idx.cpu().numpy() < counts[:, None, None]).all() and (idx >= 0).all() and torch.isfinite(dist).all()
        up = ops.interpolate_points(pooled.features, idx, ops.interpolation_weights(dist.clamp(min=0)))  # (the CPU formula can round below 0)
        assert up.shape == (b, c, n) and torch.isfinite(up).all()
        up.sum().backward()
        assert torch.isfinite(tx.grad).all()
        results.append((pooled.xyz.detach().cpu(), pooled.features.detach().cpu()))
    for a, d in zip(*results):  # (the pooled level word for word; the lists may break ties of distance differently)
        assert np.array_equal(_words(a), _words(d))
