"""CPU tests of the point-voxel ops (``neighbour_ops.voxel_index`` / ``voxelize`` / ``devoxelize`` / ``point_voxel``): the numpy
reference (tests/voxel_reference.py) against closed forms, the torch path of CPU tensors against that reference word for
word, CPU autograd against the float64 gradients, and the argument checks of the C ABI and of Python that need no device."""

import ctypes

import numpy as np
import pytest
import torch

from tests import voxel_reference as ref

EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
CASES = [(2, 2, 37, 5, 0), (3, 3, 70, 3, 1), (5, 1, 300, 9, 1), (32, 2, 513, 2, 0), (33, 1, 64, 4, 1)]  # (res, b, n, c, grid)


def _words(a):
    a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope='module')
def clouds():
    out = {}
    for res, b, n, c, which in CASES:
        lo, extent = ref.grid_of(res, which)
        xyz = ref.cloud(res * 1000 + n, b, n, res, lo, extent)
        out[res] = (xyz, lo, extent, ref.voxel_index(xyz, res, lo, extent))
    return out


def test_non_finite_points_first_last_and_inside():
    """What the clouds of these tests and of the GPU tests promise: a NaN first, a +inf last, a -inf and a NaN inside, in every mixed row."""
    for n in (63, 257, ref.MAX_POINTS):
        xyz = ref.cloud(n, 2, n, 32, -0.5, 1.0)
        for row in xyz:
            assert np.isnan(row[0]).any() and np.isposinf(row[n - 1]).any() and np.isneginf(row[n // 2]).any() and np.isnan(row[n // 3]).any()
            assert (~np.isfinite(row).all(1)).sum() == 4


def test_reference_counts_are_the_occupancy_grid(clouds):
    from pointcloudcounterfactual_amd import set_metrics

    for res, b, n, _, _ in CASES:
        xyz, lo, extent, (cell, order, counts) = clouds[res]
        lo32, inv, step = set_metrics._grid_args(res, False, lo, extent)
        want = set_metrics._occupancy_host(torch.from_numpy(xyz), res, False, True, lo32, inv, step).numpy()
        assert np.array_equal(counts.reshape(want.shape), want)
        assert counts.sum() == np.isfinite(xyz).all(2).sum() and (cell >= 0).sum() == counts.sum()
        for s in range(b):  # a permutation: the finite points by (cell, index), the others behind them in index order
            assert sorted(order[s]) == list(range(n))
            key = [(cell[s, p] if cell[s, p] >= 0 else res ** 3, p) for p in order[s]]
            assert key == sorted(key)
        assert (cell[~np.isfinite(xyz).all(2)] == -1).all()


def test_reference_voxelize_of_a_constant_is_the_constant(clouds):
    for res, b, n, c, _ in CASES:
        _, _, _, (cell, _, counts) = clouds[res]
        grid = ref.voxelize(np.full((b, c, n), 0.75, dtype=np.float32), cell, counts)
        occupied = np.broadcast_to(counts[:, None, :] > 0, grid.shape)
        assert (grid[occupied] == np.float32(0.75)).all() and (_words(grid)[~occupied] == 0).all()


def test_reference_devoxelize_reproduces_an_affine_grid_and_the_nodes():
    """Integer coefficients: the grid is exact in float32 and its trilinear interpolant is the affine function itself.  The
    bound is gamma(11) * sum |w g|: 8 products, 2 weight roundings and 1 for w0."""
    for res, which in ((2, 0), (3, 1), (9, 0), (33, 1)):
        lo, extent = ref.grid_of(res, which)
        b, n = 2, 200
        xyz = ref.cloud(res + 7, b, n, res, lo, extent)
        i, j, k = np.meshgrid(np.arange(res), np.arange(res), np.arange(res), indexing='ij')
        grid = np.tile((3 + 2 * i - 5 * j + 7 * k).astype(np.float32).reshape(1, 1, -1), (b, 1, 1))
        got = ref.devoxelize(grid, xyz, res, lo, extent)
        finite, t, _, _, _ = ref.corners(xyz, res, lo, extent)
        t = t.astype(np.float64)
        want = np.where(finite, 3 + 2 * t[:, :, 0] - 5 * t[:, :, 1] + 7 * t[:, :, 2], 0.0)
        _, mag = ref.devoxelize_f64(grid, xyz, res, lo, extent)
        assert (np.abs(got[:, 0].astype(np.float64) - want) <= ref.gamma(11) * mag[:, 0]).all()
        assert (_words(got[:, 0])[~finite] == 0).all()
    # a point on a grid node returns that node's word (inv = 1: the nodes are exact), whatever the other corners hold
    res = 5
    rng = np.random.default_rng(3)
    grid = ref.features(11, 1, 2, res ** 3)
    grid[np.isnan(grid) | np.isinf(grid)] = 1.0  # (0 * inf of a neighbouring corner would be NaN: IEEE, and the contract's)
    nodes = rng.integers(0, res, size=(1, 50, 3))
    got = ref.devoxelize(grid, nodes.astype(np.float32), res, 0.0, float(res - 1))
    flat = (nodes[:, :, 0] * res + nodes[:, :, 1]) * res + nodes[:, :, 2]
    want = np.take_along_axis(grid, flat[:, None, :].repeat(2, 1), 2)
    assert np.array_equal(got, want)  # (values: a -0.0 node reads as +0.0 + -0.0 = +0.0)
    assert np.array_equal(_words(got)[want != 0], _words(want)[want != 0])


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'res{c[0]}')
def test_cpu_paths_word_for_word(clouds, case):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    res, b, n, c, _ = case
    xyz, lo, extent, (cell, order, counts) = clouds[res]
    txyz = torch.from_numpy(xyz)
    index = ops.voxel_index(txyz, res, lo, extent)
    assert index._fields == ('cell', 'order', 'counts') and all(t.dtype == torch.int32 for t in index)
    assert np.array_equal(index.cell.numpy(), cell) and np.array_equal(index.order.numpy(), order)
    assert index.counts.shape == (b, res, res, res) and np.array_equal(index.counts.numpy().reshape(b, -1), counts)
    x = ref.features(res, b, c, n)
    grid = ops.voxelize(torch.from_numpy(x), index)
    assert grid.shape == (b, c, res, res, res) and grid.dtype == torch.float32
    assert np.array_equal(_words(grid).reshape(b, c, -1), _words(ref.voxelize(x, cell, counts)))
    assert torch.equal(ops.voxelize(torch.from_numpy(x), txyz, res, lo, extent).view(torch.int32), grid.view(torch.int32))
    rows = ref.features(res + 1, b, c, res ** 3)
    out = ops.devoxelize(torch.from_numpy(rows).view(b, c, res, res, res), txyz, lo, extent)
    assert out.shape == (b, c, n) and out.dtype == torch.float32
    assert np.array_equal(_words(out), _words(ref.devoxelize(rows, xyz, res, lo, extent)))


def test_cpu_path_all_in_one_cell_and_each_in_its_own():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for kind, res, n in (('one_cell', 4, 150), ('own_cell', 5, 125), ('own_cell', 3, 20)):
        xyz = ref.cloud(5, 2, n, res, -0.5, 1.0, kind)
        cell, order, counts = ref.voxel_index(xyz, res, -0.5, 1.0)
        assert counts.max() == (n if kind == 'one_cell' else 1)
        index = ops.voxel_index(torch.from_numpy(xyz), res)
        assert np.array_equal(index.cell.numpy(), cell) and np.array_equal(index.order.numpy(), order)
        x = ref.features(n, 2, 3, n)
        assert np.array_equal(_words(ops.voxelize(torch.from_numpy(x), index)).reshape(2, 3, -1), _words(ref.voxelize(x, cell, counts)))


@pytest.mark.parametrize('case', CASES, ids=lambda c: f'res{c[0]}')
def test_cpu_autograd_against_float64(clouds, case):
    """voxelize: one rounded division per element (gamma(1), taken as gamma(2)).  devoxelize: autograd adds the products in
    an order of its own: gamma(t + 3) * sum |w g| with t contributions, the bound of the kernel."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    res, b, n, c, _ = case
    xyz, lo, extent, (cell, _, counts) = clouds[res]
    rng = np.random.default_rng(res)
    x = torch.from_numpy(rng.standard_normal((b, c, n)).astype(np.float32)).requires_grad_(True)
    txyz = torch.from_numpy(xyz).requires_grad_(True)
    g = rng.standard_normal((b, c, res ** 3)).astype(np.float32)
    ops.voxelize(x, txyz, res, lo, extent).backward(torch.from_numpy(g).view(b, c, res, res, res))
    want = ref.voxelize_bwd_f64(g, cell, counts)
    assert (np.abs(x.grad.numpy() - want) <= ref.gamma(2) * np.abs(want)).all()
    assert (x.grad.numpy()[np.broadcast_to(cell[:, None, :] < 0, want.shape)] == 0).all()
    assert np.array_equal(_words(x.grad), _words(ref.voxelize_bwd(g, cell, counts)))
    grid = torch.from_numpy(rng.standard_normal((b, c, res, res, res)).astype(np.float32)).requires_grad_(True)
    go = rng.standard_normal((b, c, n)).astype(np.float32)
    ops.devoxelize(grid, txyz, lo, extent).backward(torch.from_numpy(go))
    ref.GradGrid(xyz, go, res, lo, extent).check_bound(grid.grad.numpy())
    assert txyz.grad is None  # coordinates carry no gradient


def test_point_voxel_on_the_cpu():
    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for name in ('VoxelIndex', 'voxel_index', 'voxelize', 'devoxelize', 'point_voxel'):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(ops, name)
    res, b, n, c = 6, 2, 90, 3
    xyz = torch.from_numpy(ref.cloud(1, b, n, res, -0.5, 1.0))
    torch.manual_seed(0)
    net = torch.nn.Conv3d(c, 4, 3, padding=1)
    x = torch.randn(b, c, n, requires_grad=True)
    out = ops.point_voxel(x, xyz, res, net)
    want = ops.devoxelize(net(ops.voxelize(x, ops.voxel_index(xyz, res))), xyz)
    assert out.shape == (b, 4, n) and torch.equal(out.view(torch.int32), want.view(torch.int32))
    out.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all() and net.weight.grad is not None
    with pytest.raises(ValueError, match='voxel_net must return'):
        ops.point_voxel(x, xyz, res, lambda g: g[:, :, 1:])
    with pytest.raises(ValueError, match='callable'):
        ops.point_voxel(x, xyz, res, None)
    # views and the empty batch
    xv = torch.randn(b, 2 * c, 2 * n)[:, ::2, ::2]
    assert torch.equal(ops.voxelize(xv, xyz, res), ops.voxelize(xv.contiguous(), xyz, res))
    empty = ops.voxel_index(xyz[:0], res)
    assert empty.cell.shape == (0, n) and empty.counts.shape == (0, res, res, res)
    assert ops.voxelize(x[:0], xyz[:0], res).shape == (0, c, res, res, res)
    assert ops.devoxelize(torch.zeros(0, c, res, res, res), xyz[:0]).shape == (0, c, n)


def test_argument_errors():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    xyz, x, grid = torch.rand(2, 10, 3), torch.zeros(2, 4, 10), torch.zeros(2, 4, 5, 5, 5)
    index = ops.voxel_index(xyz, 5)
    for bad in (xyz[0], xyz[:, :, :2], xyz[:, :0], torch.zeros(1, ops.MAX_VOXEL_POINTS + 1, 3)):
        with pytest.raises(ValueError, match='voxel_index: expected xyz'):
            ops.voxel_index(bad, 5)
    for res in (1, 129, 2.0, True, None):
        with pytest.raises(ValueError, match='resolution'):
            ops.voxel_index(xyz, res)
    for lo, extent in ((0.0, 0.0), (0.0, -1.0), (0.0, float('inf')), (float('nan'), 1.0), (0.0, float('nan')), (0.0, 1e-40)):
        with pytest.raises(ValueError):
            ops.voxel_index(xyz, 5, lo, extent)
        with pytest.raises(ValueError):
            ops.devoxelize(grid, xyz, lo, extent)
    with pytest.raises(RuntimeError, match='xyz must be torch'):
        ops.voxel_index(xyz.double(), 5)
    with pytest.raises(ValueError, match='too large'):
        ops.voxel_index(torch.zeros(1025, 1, 3), 128)
    for bx, bi, kw in ((x[0], index, {}), (x[:, :0], index, {}), (x[:, :, :9], index, {}), (x[:1], index, {}), (x, index, {'resolution': 6}),
                       (x, xyz, {}), (x, xyz[:, :9], {'resolution': 5}), (x, None, {}), (x, (index.cell, index.order, index.counts), {}),
                       (x, ops.VoxelIndex(index.cell, index.order[:, :9], index.counts), {}),
                       (x, ops.VoxelIndex(index.cell, index.order, index.counts[:, :, :, :4]), {}),
                       (x, ops.VoxelIndex(index.cell, index.order, index.counts.reshape(2, -1)), {})):
        with pytest.raises(ValueError, match='voxelize:'):
            ops.voxelize(bx, bi, **kw)
    for bx, bi, name in ((x.double(), index, 'features'), (x, ops.VoxelIndex(index.cell.long(), index.order, index.counts), 'index.cell'),
                         (x, ops.VoxelIndex(index.cell, index.order, index.counts.long()), 'index.counts')):
        with pytest.raises(RuntimeError, match=f'{name} must be torch'):
            ops.voxelize(bx, bi)
    with pytest.raises(RuntimeError, match='expected cpu'):
        ops.voxelize(x, ops.VoxelIndex(index.cell.to('meta'), index.order, index.counts))
    assert ops.devoxelize(grid, torch.rand(2, ops.MAX_VOXEL_POINTS + 1, 3)).shape == (2, 4, ops.MAX_VOXEL_POINTS + 1)  # (no limit here)
    for bg, bx in ((grid[0], xyz), (grid[:, :0], xyz), (grid[:, :, :4], xyz), (grid, xyz[:1]), (grid, xyz[0]), (grid[:, :, :1, :1, :1], xyz)):
        with pytest.raises(ValueError):
            ops.devoxelize(bg, bx)
    for bg, bx, name in ((grid.double(), xyz, 'grid'), (grid, xyz.half(), 'xyz')):
        with pytest.raises(RuntimeError, match=f'{name} must be torch'):
            ops.devoxelize(bg, bx)
    with pytest.raises(RuntimeError, match='expected cpu'):
        ops.devoxelize(grid, xyz.to('meta'))
    for args in ((x[0], xyz, 5), (x, xyz[:, :9], 5), (x, xyz, 1), (x, xyz[:1], 5)):
        with pytest.raises(ValueError):
            ops.point_voxel(*args, torch.nn.Identity())


def test_messages_word_for_word():
    """The refusals of ``voxelize``, ``devoxelize`` and ``point_voxel`` whose checks other ops share, in their words and in
    the order in which a call with several bad arguments reports them."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import raised

    xyz, x, grid = torch.rand(2, 10, 3), torch.zeros(2, 4, 10), torch.zeros(2, 4, 5, 5, 5)
    index = ops.voxel_index(xyz, 5)
    for bad, shown in ((x[0], '(4, 10)'), (x[:, :0], '(2, 0, 10)'), (x[:, :, :0], '(2, 4, 0)')):
        text = f'expected features[B,C,N] with C >= 1 and N >= 1, got {shown}'
        assert raised(ValueError, ops.voxelize, bad.double(), index) == 'voxelize: ' + text  # (the shape before the dtype)
        assert raised(ValueError, ops.point_voxel, bad.double(), xyz[:1], 5, None) == 'point_voxel: ' + text
    assert raised(RuntimeError, ops.voxelize, x.double(), None) == 'features must be torch.float32, found torch.float64'
    assert raised(ValueError, ops.point_voxel, x.double(), xyz[:1], 5, None) == 'point_voxel: expected xyz[B = 2,N = 10,3], got (1, 10, 3)'
    for bad, shown in ((xyz[:1], '(1, 10, 3)'), (xyz[0], '(10, 3)'), (xyz[:, :, :2], '(2, 10, 2)'), (xyz[:, :0], '(2, 0, 3)')):
        assert raised(ValueError, ops.devoxelize, grid, bad.double()) == f'devoxelize: expected xyz[B = 2,N,3] with N >= 1, got {shown}'
    assert raised(RuntimeError, ops.devoxelize, grid.double(), xyz[:1]) == 'grid must be torch.float32, found torch.float64'
    assert raised(RuntimeError, ops.devoxelize, grid, xyz.double().to('meta')) == 'xyz must be torch.float32, found torch.float64'
    assert raised(RuntimeError, ops.devoxelize, grid, xyz.to('meta')) == 'xyz is on meta, expected cpu'
    assert raised(ValueError, ops.devoxelize, grid, xyz[:1], 0.0, 0.0) == 'extent must be finite and > 0, got 0.0'  # (the grid first)


def _entry_points(L, p):
    """name -> call(b, c, n, res, lo, extent, q): the five functions with every pointer ``q``."""
    return {
        'voxel_index': lambda b, c, n, res, lo, extent, q=p: L.pcc_voxel_index(b, n, q, res, lo, extent, q, q, q, None),
        'voxelize': lambda b, c, n, res, lo, extent, q=p: L.pcc_voxelize(b, c, n, res, q, q, q, q, q, None),
        'voxelize_bwd': lambda b, c, n, res, lo, extent, q=p: L.pcc_voxelize_bwd(b, c, n, res, q, q, q, q, None),
        'devoxelize': lambda b, c, n, res, lo, extent, q=p: L.pcc_devoxelize(b, c, n, res, lo, extent, q, q, q, None),
        'devoxelize_bwd': lambda b, c, n, res, lo, extent, q=p: L.pcc_devoxelize_bwd(b, c, n, res, lo, extent, q, q, q, None),
    }


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched: the guard stays)."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)(*([0x5a] * 64))
    p = ctypes.addressof(buf)
    inf, nan = float('inf'), float('nan')
    # (b, c, n, res, lo, extent); the last six need lo and extent: the entry points that take them
    sizes = [(-1, 3, 8, 4, 0.0, 1.0), (65536, 3, 8, 4, 0.0, 1.0), (1, 3, 0, 4, 0.0, 1.0), (1, 3, 8, 1, 0.0, 1.0), (1, 3, 8, 129, 0.0, 1.0),
             (65535, 3, 1 << 16, 4, 0.0, 1.0), (1024, 3, 8, 128, 0.0, 1.0), (0, 3, 8, 1, 0.0, 1.0), (0, 3, 0, 4, 0.0, 1.0)]
    scalars = [(1, 3, 8, 4, 0.0, 0.0), (1, 3, 8, 4, 0.0, -1.0), (1, 3, 8, 4, 0.0, inf), (1, 3, 8, 4, 0.0, nan), (1, 3, 8, 4, nan, 1.0),
               (1, 3, 8, 4, -inf, 1.0), (1, 3, 8, 4, 0.0, 1e-40), (0, 3, 8, 4, 0.0, 0.0)]
    fns = _entry_points(L, p)
    for name, fn in fns.items():
        takes_scalars = name in ('voxel_index', 'devoxelize', 'devoxelize_bwd')
        for args in sizes + (scalars if takes_scalars else []):
            assert fn(*args) == EINVAL, (name, args)
            assert L.pcc_last_error().decode().startswith(name + ':'), (name, args)
        if name != 'voxel_index':
            for c in (0, -1):
                assert fn(1, c, 8, 4, 0.0, 1.0) == EINVAL and L.pcc_last_error().decode().startswith(name + ': c must be')
        assert fn(1, 3, 8, 4, 0.0, 1.0, None) == EINVAL
        assert L.pcc_last_error().decode().startswith(name + ': null pointer')
        # an empty batch enqueues nothing, whatever the pointers
        assert fn(0, 3, 8, 4, 0.0, 1.0, None) == 0 and L.pcc_last_status() == 0
    # every pointer on its own
    for i in range(4):
        q = [p] * 4
        q[i] = None
        assert L.pcc_voxel_index(1, 8, q[0], 4, 0.0, 1.0, q[1], q[2], q[3], None) == EINVAL
        assert L.pcc_voxelize_bwd(1, 3, 8, 4, q[0], q[1], q[2], q[3], None) == EINVAL
    for i in range(5):
        q = [p] * 5
        q[i] = None
        assert L.pcc_voxelize(1, 3, 8, 4, q[0], q[1], q[2], q[3], q[4], None) == EINVAL
    for i in range(3):
        q = [p] * 3
        q[i] = None
        assert L.pcc_devoxelize(1, 3, 8, 4, 0.0, 1.0, q[0], q[1], q[2], None) == EINVAL
        assert L.pcc_devoxelize_bwd(1, 3, 8, 4, 0.0, 1.0, q[0], q[1], q[2], None) == EINVAL
    # the largest cloud the index sorts is named in the message
    assert L.pcc_voxel_index(1, ref.MAX_POINTS + 1, p, 4, 0.0, 1.0, p, p, p, None) == EINVAL
    assert L.pcc_last_error().decode() == f'voxel_index: n must be <= {ref.MAX_POINTS}'
    assert bytes(buf) == b'\x5a' * 64


def test_the_abi_is_bound_and_the_tuning_table_is_untouched():
    from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops

    assert [len(_lib.ABI[f][1]) for f in ('pcc_voxel_index', 'pcc_voxelize', 'pcc_voxelize_bwd', 'pcc_devoxelize', 'pcc_devoxelize_bwd')] == \
        [10, 10, 9, 10, 10]
    assert len(_lib.TUNING) == 16 and max(_lib.TUNING.values()) == 15
    assert ops.MAX_VOXEL_POINTS == ref.MAX_POINTS
