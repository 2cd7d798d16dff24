"""GPU tests of the point-voxel ops (``pcc_voxel_index``, ``pcc_voxelize`` / ``_bwd``, ``pcc_devoxelize`` / ``_bwd`` through the C
ABI on guarded, prefilled buffers, and ``neighbour_ops.voxelize`` / ``devoxelize`` / ``point_voxel``) against the numpy
reference of tests/voxel_reference.py: the index, the grid, its gradient and the interpolation word for word on either side
of every boundary of the dispatch; the one gradient whose summation order is not fixed exactly on integer gradients with
dyadic coordinates and inside the float32 summation bound on Gaussian ones; independence of the batch and of the run."""

import numpy as np
import pytest
import torch

from tests import voxel_reference as ref
from tests.which_ran import ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 32        # words of sentinel around every output (128 bytes: the output itself stays 16-byte aligned)
INT_FILL = -7777  # what an int32 output holds before the call


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class _Out:
    """An output of ``shape`` inside a flat buffer: GUARD (+ ``shift``: off the 16-byte alignment) sentinel words before it
    and GUARD behind.  Floats start as NaN, integers as INT_FILL: every element must be written, and nothing around it."""

    def __init__(self, shape, dtype, cuda, shift=0):
        self.fill = float('nan') if dtype == torch.float32 else INT_FILL
        numel = int(np.prod(shape))
        self.flat = torch.full((numel + 2 * GUARD + shift,), self.fill, dtype=dtype, device=cuda)
        self.lo, self.hi = GUARD + shift, GUARD + shift + numel
        self.view = self.flat[self.lo:self.hi].view(shape)

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        flat = self.flat.cpu().numpy()
        guard = np.concatenate((flat[:self.lo], flat[self.hi:]))
        assert np.isnan(guard).all() if flat.dtype == np.float32 else (guard == INT_FILL).all()
        return flat[self.lo:self.hi].reshape(self.view.shape)


def _call(name, dev, *args):
    from pointcloudcounterfactual_amd import _lib

    _lib.call(getattr(_lib.lib, 'pcc_' + name), name, dev, *args)


def _index(xyz, res, lo, extent):
    """``pcc_voxel_index`` on the device cloud ``xyz``: the three outputs as device views (their guards checked)."""
    b, n = xyz.shape[:2]
    dev = xyz.device
    cell, order, counts = _Out((b, n), torch.int32, dev), _Out((b, n), torch.int32, dev), _Out((b, res ** 3), torch.int32, dev)
    _, names = ran(lambda: _call('voxel_index', dev, b, n, xyz.data_ptr(), res, lo, extent, cell.ptr(), order.ptr(), counts.ptr()))
    assert names == ({ref.index_kernel(n): 1} if b else {}), (n, names)  # (the sort the size predicts, no sibling)
    return (cell, order, counts), (cell.numpy(), order.numpy(), counts.numpy())


def _vox(x, index, res, shift=0):
    b, c, n = x.shape
    grid = _Out((b, c, res ** 3), torch.float32, x.device, shift)
    _, names = ran(lambda: _call('voxelize', x.device, b, c, n, res, x.data_ptr(), index[0].ptr(), index[1].ptr(), index[2].ptr(),
                                 grid.ptr()))
    aligned = (index[2].ptr() | grid.ptr()) % 16 == 0
    assert set(names) == (ref.voxelize_kernels(n, res, aligned) if b else set()), (n, res, aligned, names)
    return grid.numpy()


def _vox_bwd(g, index, n, res):
    b, c = g.shape[:2]
    gx = _Out((b, c, n), torch.float32, g.device)
    _call('voxelize_bwd', g.device, b, c, n, res, index[0].ptr(), index[2].ptr(), g.data_ptr(), gx.ptr())
    return gx.numpy()


def _devox(grid, xyz, res, lo, extent):
    b, c = grid.shape[:2]
    n = xyz.shape[1]
    out = _Out((b, c, n), torch.float32, xyz.device)
    _call('devoxelize', xyz.device, b, c, n, res, lo, extent, grid.data_ptr(), xyz.data_ptr(), out.ptr())
    return out.numpy()


def _devox_bwd(xyz, go, res, lo, extent, shift=0):
    b, c, n = go.shape
    gg = _Out((b, c, res ** 3), torch.float32, xyz.device, shift)
    _, names = ran(lambda: _call('devoxelize_bwd', xyz.device, b, c, n, res, lo, extent, xyz.data_ptr(), go.data_ptr(), gg.ptr()))
    assert names == ({ref.devox_bwd_kernel(res): 1} if b else {}), (res, names)  # (the rows per workgroup the resolution predicts)
    return gg.numpy()


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _three_clouds(n, res, lo, extent):
    """Rows 0 and 2: one mixed cloud (outside the cube, midpoints, nodes, NaN and +-inf at the first, last and interior
    positions) at two batch positions; row 1: every point in its own cell where the grid has that many, in one cell where
    not."""
    mixed = ref.cloud(7 * n + res, 1, n, res, lo, extent)
    other = ref.cloud(n + res, 1, n, res, lo, extent, 'own_cell' if n <= res ** 3 else 'one_cell')
    return np.concatenate((mixed, other, mixed))


# every register / LDS boundary of the sort: one wave up to 256 points, then an LDS network over 512, 1024, ... 16384 keys
INDEX_N = (1, 63, 64, 65, ref.WAVE_SORT - 1, ref.WAVE_SORT, ref.WAVE_SORT + 1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097,
           8191, 8192, 8193, ref.MAX_POINTS - 1, ref.MAX_POINTS)


@pytest.mark.parametrize('n', INDEX_N)
def test_voxel_index_word_for_word(cuda, n):
    from pointcloudcounterfactual_amd import _lib

    for res, which in ((2, 0), (3, 1), (32, 1), (128, 0)):
        lo, extent = ref.grid_of(res, which)
        xyz = _three_clouds(n, res, lo, extent)
        want = ref.voxel_index(xyz, res, lo, extent)
        assert want[2][1].max() == (1 if n <= res ** 3 else n)  # (row 1 is what it is meant to be)
        xd = _dev(xyz, cuda)
        _, got = _index(xd, res, lo, extent)
        for g, w, name in zip(got, want, ('cell', 'order', 'counts')):
            assert np.array_equal(g, w), (res, name)
        # the counts of pcc_occupancy_grid(per_cloud = 1), word for word
        occ = torch.full((3, res ** 3), INT_FILL, dtype=torch.int32, device=cuda)
        _lib.call(_lib.lib.pcc_occupancy_grid, 'occupancy_grid', cuda, 3, n, xd.data_ptr(), res, lo, extent, 0, 1, occ.data_ptr())
        assert np.array_equal(got[2], occ.cpu().numpy())
        # a cloud's words at every batch position, alone, and in a second run
        for g in got:
            assert np.array_equal(g[0], g[2])
        _, alone = _index(xd[:1].contiguous(), res, lo, extent)
        _, again = _index(xd, res, lo, extent)
        for g, a, r in zip(got, alone, again):
            assert np.array_equal(a[0], g[0]) and np.array_equal(r, g)


# (n, res, grid): a cell of exactly LONG_RUN points and of one more; odd and even res (16-byte stores or not); LDS sort
VOX_SHAPES = ((ref.LONG_RUN, 2, 1), (ref.LONG_RUN + 1, 3, 0), (130, 32, 1), (300, 3, 1), (600, 4, 0))
VOX_C = (1, 3, ref.CB - 1, ref.CB, ref.CB + 1, 63, 64, 65)  # the channel block of a thread; the 64 lanes of a long run


@pytest.mark.parametrize('shape', VOX_SHAPES, ids=lambda s: f'n{s[0]}-res{s[1]}')
def test_voxelize_forward_and_backward_word_for_word(cuda, shape):
    n, res, which = shape
    lo, extent = ref.grid_of(res, which)
    xyz = np.concatenate((_three_clouds(n, res, lo, extent), ref.cloud(n, 1, n, res, lo, extent, 'one_cell')))
    b = xyz.shape[0]
    cell, order, counts = ref.voxel_index(xyz, res, lo, extent)
    assert counts.max() == n
    index, got = _index(_dev(xyz, cuda), res, lo, extent)
    assert np.array_equal(got[0], cell) and np.array_equal(got[1], order) and np.array_equal(got[2], counts)
    x_all = ref.features(n + res, b, max(VOX_C), n)
    g_all = ref.features(n + res + 1, b, max(VOX_C), res ** 3)
    for j, c in enumerate(VOX_C):
        x, g = np.ascontiguousarray(x_all[:, :c]), np.ascontiguousarray(g_all[:, :c])
        want = _words(ref.voxelize(x, cell, counts))
        for shift in (0, 1) if j % 2 == 0 else (0,):  # (shift 1: the grid off the 16-byte alignment, scalar stores)
            assert np.array_equal(_words(_vox(_dev(x, cuda), index, res, shift)), want), (c, shift)
        assert np.array_equal(_words(_vox_bwd(_dev(g, cuda), index, n, res)), _words(ref.voxelize_bwd(g, cell, counts))), c


@pytest.mark.parametrize('res', (2, 3))
def test_more_channel_blocks_than_a_launch_has_rows(cuda, res):
    """c > 65535 * CB: the kernels stride over the channel blocks beyond gridDim.y (res 2: 16-byte stores, 3: scalar)."""
    c, n, b = 65535 * ref.CB + ref.CB + 1, 3, 1
    xyz = ref.cloud(res, b, 8, res, -0.5, 1.0)[:, 1:1 + n]  # (two finite points around a NaN one)
    cell, order, counts = ref.voxel_index(xyz, res, -0.5, 1.0)
    index, _ = _index(_dev(xyz, cuda), res, -0.5, 1.0)
    rng = np.random.default_rng(res)
    x, g = rng.standard_normal((b, c, n)).astype(np.float32), rng.standard_normal((b, c, res ** 3)).astype(np.float32)
    assert np.array_equal(_words(_vox(_dev(x, cuda), index, res)), _words(ref.voxelize(x, cell, counts)))
    assert np.array_equal(_words(_vox_bwd(_dev(g, cuda), index, n, res)), _words(ref.voxelize_bwd(g, cell, counts)))
    assert np.array_equal(_words(_devox(_dev(g, cuda), _dev(xyz, cuda), res, -0.5, 1.0)), _words(ref.devoxelize(g, xyz, res, -0.5, 1.0)))


def test_voxelize_all_points_in_one_cell(cuda):
    """The sequential chain of a cell is part of the contract; a cell holding the whole cloud stays bounded (the channels go
    across the lanes of a wave)."""
    b, c, n, res = 2, 64, 2048, 32
    xyz = ref.cloud(3, b, n, res, -0.5, 1.0, 'one_cell')
    cell, order, counts = ref.voxel_index(xyz, res, -0.5, 1.0)
    assert (counts.max(1) == n).all()
    index, got = _index(_dev(xyz, cuda), res, -0.5, 1.0)
    assert np.array_equal(got[1], order)
    x = ref.features(9, b, c, n)
    x[np.isinf(x) | np.isnan(x)] = 1.0  # (one NaN would be the whole cell: keep the sum a test of its order)
    assert np.array_equal(_words(_vox(_dev(x, cuda), index, res)), _words(ref.voxelize(x, cell, counts)))


@pytest.mark.parametrize('res', (2, 3, 32, 33))
def test_devoxelize_word_for_word(cuda, res):
    """Mixed clouds on both grids and points at multiples of 1/4 of a cell (nodes, the top faces t = res - 1, outside the
    cube, a NaN point); grids with +-0, denormals, inf and NaN."""
    n, b = 333, 2
    for which in (0, 1):
        lo, extent = ref.grid_of(res, which)
        xyz = ref.cloud(res + which, b, n, res, lo, extent) if which == 0 else ref.dyadic_cloud(res, b, n, res)
        finite, t, _, _, _ = ref.corners(xyz, res, lo, extent)
        if which == 1:
            assert (t[finite] == res - 1).any() and (t[finite] == np.floor(t[finite])).any()
        for c in (1, ref.CB, ref.CB + 1):
            for seed, clean in ((1, False), (2, True)):
                grid = ref.features(seed + c, b, c, res ** 3)
                if clean:
                    grid[np.isinf(grid) | np.isnan(grid)] = -2.5
                got = _devox(_dev(grid, cuda), _dev(xyz, cuda), res, lo, extent)
                assert np.array_equal(_words(got), _words(ref.devoxelize(grid, xyz, res, lo, extent))), (which, c, clean)
                assert (_words(got)[np.broadcast_to(~finite[:, None, :], got.shape)] == 0).all()


@pytest.mark.parametrize('res', (2, 16, 17, 20, 21, 25, 26, ref.LDS_RES, ref.LDS_RES + 1))
def test_devoxelize_bwd_exact_and_in_bound(cuda, res):
    """LDS bins (res <= 32: 8 channels per workgroup up to res = 16, 4 to 20, 2 to 25, 1 above) and global atomics (33).  Integer gradients at dyadic coordinates: every partial sum is
    representable, so the sum is exact in any order.  Gaussian gradients: every element within gamma(t + 3) * sum |w g| of
    the float64 sum with the kernel's own float32 t, t the number of contributions; no element excluded; +0.0 where nothing
    points."""
    n, b = 700, 2
    rng = np.random.default_rng(res)
    for c in (1, ref.CB + 1) if res > 2 else (1, ref.CB - 1, ref.CB, ref.CB + 1):
        lo, extent = ref.grid_of(res, 1)
        xyz = ref.dyadic_cloud(res + c, b, n, res)
        g = rng.integers(-8, 9, size=(b, c, n)).astype(np.float32)
        for shift in (0, 1):
            ref.GradGrid(xyz, g, res, lo, extent).check_exact(_devox_bwd(_dev(xyz, cuda), _dev(g, cuda), res, lo, extent, shift))
        for which in (0, 1):
            lo, extent = ref.grid_of(res, which)
            xyz = ref.cloud(res + c + which, b, n, res, lo, extent)
            g = rng.standard_normal((b, c, n)).astype(np.float32)
            ref.GradGrid(xyz, g, res, lo, extent).check_bound(_devox_bwd(_dev(xyz, cuda), _dev(g, cuda), res, lo, extent))


def test_autograd_voxelize_and_devoxelize_against_the_cpu_path(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, n, res = 2, 5, 400, 6
    xyz = ref.cloud(4, b, n, res, -0.5, 1.0)
    rng = np.random.default_rng(4)
    x, g = rng.standard_normal((b, c, n)).astype(np.float32), rng.standard_normal((b, c, res, res, res)).astype(np.float32)
    grads, outs = [], []
    for dev in (torch.device('cpu'), cuda):
        tx, txyz = torch.from_numpy(x).to(dev).requires_grad_(True), torch.from_numpy(xyz).to(dev).requires_grad_(True)
        index = ops.voxel_index(txyz, res)
        out = ops.voxelize(tx, index)
        out.backward(torch.from_numpy(g).to(dev))
        assert txyz.grad is None
        outs.append(out.detach().cpu())
        grads.append(tx.grad.cpu())
    # the forward and this gradient are fixed word for word
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and torch.equal(grads[0].view(torch.int32), grads[1].view(torch.int32))
    go = rng.standard_normal((b, c, n)).astype(np.float32)
    want = ref.GradGrid(xyz, go, res, -0.5, 1.0)
    outs = []
    for dev in (torch.device('cpu'), cuda):
        tg, txyz = torch.from_numpy(g).to(dev).requires_grad_(True), torch.from_numpy(xyz).to(dev).requires_grad_(True)
        out = ops.devoxelize(tg, txyz)
        out.backward(torch.from_numpy(go).to(dev))
        assert txyz.grad is None
        outs.append(out.detach().cpu())
        want.check_bound(tg.grad.cpu().numpy())  # both paths inside the bound of the float64 sum
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    # nothing is computed for a gradient nobody asked for
    assert not ops.voxelize(torch.from_numpy(x).to(cuda), index).requires_grad


def test_point_voxel_with_a_small_conv3d(cuda):
    """``point_voxel`` with a 1x1x1 Conv3d on the GPU against the float64 composition, output and gradients.  Every quantity
    is a sum of products of the inputs; its float32 evaluation, in any order, stays within gamma(K) times the same sum taken
    over magnitudes, K the roundings along the longest path: the cell's sum and division (m + 1 for m points in the fullest
    cell), the convolution (c + 2), the eight corners (12); the gradients add the reduction they end in (8 n corner terms
    per cloud for a feature, every cell of every cloud for a weight)."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, c2, n, res = 2, 4, 3, 200, 5
    xyz = ref.cloud(8, b, n, res, -0.5, 1.0)
    cell, _, counts = ref.voxel_index(xyz, res, -0.5, 1.0)
    finite, _, offs, _, ws64 = ref.corners(xyz, res, -0.5, 1.0)
    rng = np.random.default_rng(8)
    x, go = rng.standard_normal((b, c, n)).astype(np.float32), rng.standard_normal((b, c2, n)).astype(np.float32)
    torch.manual_seed(8)
    net = torch.nn.Conv3d(c, c2, 1)

    def chain64(x64, w64, bias64):
        safe = torch.from_numpy(np.maximum(cell, 0).astype(np.int64))[:, None, :].expand(b, c, n)
        live = torch.from_numpy(cell >= 0)[:, None, :]
        acc = torch.zeros(b, c, res ** 3, dtype=torch.float64).scatter_add(2, safe, torch.where(live, x64, torch.zeros((), dtype=torch.float64)))
        grid = acc / torch.from_numpy(np.maximum(counts, 1))[:, None, :]
        y = torch.einsum('oc,bcv->bov', w64, grid) + bias64[None, :, None]
        out = 0
        for off, w in zip(offs, ws64):
            out = out + torch.from_numpy(w)[:, None, :] * torch.gather(y, 2, torch.from_numpy(off)[:, None, :].expand(b, c2, n))
        return torch.where(torch.from_numpy(finite)[:, None, :], out, torch.zeros((), dtype=torch.float64))

    def leaves(absolute):
        ts = [torch.from_numpy(x).double(), net.weight.detach().double().view(c2, c), net.bias.detach().double()]
        return [(t.abs() if absolute else t).requires_grad_(True) for t in ts]

    want, mag = leaves(False), leaves(True)
    want_out, mag_out = chain64(*want), chain64(*mag)
    want_out.backward(torch.from_numpy(go).double())
    mag_out.backward(torch.from_numpy(go).double().abs())

    net = net.to(cuda)
    tx = torch.from_numpy(x).to(cuda).requires_grad_(True)
    out = ops.point_voxel(tx, torch.from_numpy(xyz).to(cuda), res, net)
    out.backward(torch.from_numpy(go).to(cuda))
    k_out = int(counts.max()) + 1 + c + 2 + 12
    assert out.shape == (b, c2, n) and out.dtype == torch.float32

    def inside(got, ref64, mag64, k):
        return (np.abs(got.detach().cpu().double().numpy() - ref64.detach().numpy()) <= ref.gamma(k) * mag64.detach().numpy()).all()

    assert inside(out, want_out, mag_out, k_out)
    assert inside(tx.grad, want[0].grad, mag[0].grad, k_out + 8 * n)
    assert inside(net.weight.grad.view(c2, c), want[1].grad, mag[1].grad, k_out + 8 * n + b * res ** 3)
    assert inside(net.bias.grad, want[2].grad, mag[2].grad, k_out + 8 * n + b * res ** 3)
