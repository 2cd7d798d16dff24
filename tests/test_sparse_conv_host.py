"""CPU tests of the submanifold sparse convolution (``neighbour_ops.cell_neighbours`` / ``sparse_conv`` /
``SubmanifoldConv3d``): the numpy reference (tests/sparse_conv_reference.py) against closed forms and against
``torch.nn.functional.conv3d`` on the dense grid, the torch paths of CPU tensors against that reference (the map word for word,
the convolution inside the contract's bar), CPU autograd against float64, and the argument checks of the C ABI and of Python
that need no device."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

from tests import sparse_conv_reference as ref
from tests import voxel_reference as vref

EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
# (res, b, n, grid, ksize, dilation)
CASES = [(2, 2, 37, 0, 3, 1), (3, 3, 70, 1, 3, 2), (5, 1, 300, 1, 5, 1), (8, 2, 200, 0, 3, 1), (8, 2, 150, 1, 5, 2), (32, 2, 513, 0, 3, 3)]


def _ids(case):
    return 'res{}k{}d{}'.format(case[0], case[4], case[5])


def _ops_index(xyz, res, lo, extent, m):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    vindex = ops.voxel_index(torch.from_numpy(xyz), res, lo, extent)
    return ops, vindex, ops.grid_cluster(vindex, m=m)


@pytest.fixture(scope='module')
def maps():
    """Per case: the cloud, its grid and the reference at capacity n -- computed once, never modified."""
    out = {}
    for case in CASES:
        res, b, n, which, ksize, dil = case
        lo, extent = vref.grid_of(res, which)
        xyz = vref.cloud(res * 100 + n, b, n, res, lo, extent)
        out[case] = (xyz, lo, extent) + ref.build(xyz, res, lo, extent, None, ksize, dil)
    return out


def test_reference_full_lattice_has_the_border_pattern():
    res = 4
    xyz = ref.lattice_cloud(res)
    _, (_, _, count), nbr = ref.build(xyz, res, 0.0, res - 1.0)
    assert count[0] == res ** 3 and ref.is_symmetric(nbr)
    for r in range(res ** 3):  # (every cell is occupied, so the rank of a cell is the cell)
        i, j, k = r // 16, r // 4 % 4, r % 4
        for t, (di, dj, dk) in enumerate(ref.offsets(3, 1)):
            inside = all(0 <= v < res for v in (i + di, j + dj, k + dk))
            assert nbr[0, r, t] == (((i + di) * res + j + dj) * res + k + dk if inside else -1)
    interior = [(i * 4 + j) * 4 + k for i in (1, 2) for j in (1, 2) for k in (1, 2)]
    assert (nbr[0, interior] >= 0).all() and ((nbr[0] >= 0).sum(1) == 27).sum() == 8
    assert sorted(set((nbr[0] >= 0).sum(1))) == [8, 12, 18, 27]  # corner, edge, face, interior


def test_reference_single_cell_and_wrap_around():
    res = 5
    _, _, nbr = ref.build(ref.cells_cloud([62], res, repeat=3), res, 0.0, res - 1.0)
    assert nbr.shape == (1, 3, 27) and nbr[0, 0, 13] == 0 and (np.delete(nbr[0, 0], 13) == -1).all() and (nbr[0, 1:] == -1).all()
    # (i, j, res - 1) and (i, j + 1, 0) are adjacent flat cells, and no neighbours
    a, b_ = (2 * res + 1) * res + res - 1, (2 * res + 2) * res
    assert b_ == a + 1
    for ksize, dil in ((3, 1), (5, 1), (3, 2)):
        _, _, nbr = ref.build(ref.cells_cloud([a, b_], res), res, 0.0, res - 1.0, None, ksize, dil)
        centre = ksize ** 3 // 2
        assert (nbr[0, :, centre] == [0, 1]).all() and (np.delete(nbr[0], centre, 1) == -1).all()


def test_reference_dilation_two_on_a_checkerboard():
    res = 6
    even = [(i * res + j) * res + k for i in range(res) for j in range(res) for k in range(res) if (i + j + k) % 2 == 0]
    xyz = ref.cells_cloud(even, res)
    _, _, one = ref.build(xyz, res, 0.0, res - 1.0, None, 3, 1)
    _, _, two = ref.build(xyz, res, 0.0, res - 1.0, None, 3, 2)
    rank = {v: r for r, v in enumerate(even)}
    odd_tap = np.array([(di + dj + dk) % 2 != 0 for di, dj, dk in ref.offsets(3, 1)])
    assert (one[0][:, odd_tap] == -1).all()  # an offset of odd parity leaves the colour
    for r, v in enumerate(even):  # at dilation 2 every offset keeps the colour: a tap is empty only outside the grid
        i, j, k = v // 36, v // 6 % 6, v % 6
        for t, (di, dj, dk) in enumerate(ref.offsets(3, 2)):
            inside = all(0 <= u < res for u in (i + di, j + dj, k + dk))
            assert two[0, r, t] == (rank[((i + di) * res + j + dj) * res + k + dk] if inside else -1)
    assert ref.is_symmetric(one) and ref.is_symmetric(two)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_cpu_map_word_for_word_at_every_capacity(maps, case):
    res, b, n, _, ksize, dil = case
    xyz, lo, extent, (cell, order, counts), (_, _, count), full = maps[case]
    assert ref.is_symmetric(full) and full.dtype == np.int64
    u = int(count.max())
    for m in sorted({1, max(u - 1, 1), u, min(u + 1, n), n}):
        _, (_, seg, cnt), want = ref.build(xyz, res, lo, extent, m, ksize, dil)
        assert np.array_equal(want, ref.cut(full, m)) and ref.is_symmetric(want)
        for s in range(b):
            kept = min(int(cnt[s]), m)
            assert (want[s, :kept, ksize ** 3 // 2] == np.arange(kept)).all() and (want[s, kept:] == -1).all()
        ops, vindex, gindex = _ops_index(xyz, res, lo, extent, m)
        cmap = ops.cell_neighbours(vindex, gindex, ksize, dil)
        assert cmap._fields == ('nbr', 'count', 'kernel_size', 'dilation') and (cmap.kernel_size, cmap.dilation) == (ksize, dil)
        assert cmap.nbr.dtype == torch.int64 and cmap.count is gindex.count
        assert np.array_equal(cmap.nbr.numpy(), want), (case, m)


@pytest.mark.parametrize('case', CASES, ids=_ids)
def test_cpu_conv_inside_the_bar_and_other_list_ops_take_the_map(maps, case):
    res, b, n, _, ksize, dil = case
    xyz, lo, extent, _, (_, _, count), _ = maps[case]
    m = min(int(count.max()) + 2, n)
    _, _, nbr = ref.build(xyz, res, lo, extent, m, ksize, dil)
    ops, vindex, gindex = _ops_index(xyz, res, lo, extent, m)
    cmap = ops.cell_neighbours(vindex, gindex, ksize, dil)
    for c, o, with_bias in ((3, 5, True), (7, 2, False)):
        x, w, bias = ref.gaussian_inputs(res + c, b, c, o, m, ksize ** 3)
        want, d, big_s = ref.sparse_conv(x, nbr, w, bias if with_bias else None)
        got = ops.sparse_conv(torch.from_numpy(x), cmap, torch.from_numpy(w), torch.from_numpy(bias) if with_bias else None).numpy()
        assert ref.share(got, want, d, big_s) <= 1.0
        padded = ~(nbr >= 0).any(2)
        assert padded.any() and (got.transpose(0, 2, 1)[padded].view(np.uint32) == 0).all()  # +0, no bias
    grouped = ops.group_points(torch.from_numpy(x), cmap.nbr)
    assert grouped.shape == (b, c, m, ksize ** 3) and (grouped.numpy()[:, 0][nbr < 0].view(np.uint32) == 0).all()
    assert ops.aggregate_points(torch.from_numpy(x), cmap.nbr, torch.ones(b, 1, m, ksize ** 3)).shape == (b, c, m)


@pytest.mark.parametrize('res,ksize,dil', [(4, 3, 1), (8, 3, 2), (8, 5, 1), (6, 5, 2)])
def test_reference_equals_dense_conv3d_at_the_occupied_cells(res, ksize, dil):
    b, n, c, o = 2, 3 * res * res, 3, 4
    xyz = vref.cloud(res + ksize, b, n, res, 0.0, res - 1.0)
    (cell, order, _), (_, seg, count), nbr = ref.build(xyz, res, 0.0, res - 1.0, None, ksize, dil)
    x, w, bias = ref.gaussian_inputs(res, b, c, o, n, ksize ** 3)
    want, _, _ = ref.sparse_conv(x, nbr, w, bias)
    dense = torch.zeros(b, c, res ** 3, dtype=torch.float64)
    slots = [[int(cell[s, order[s, seg[s, r]]]) for r in range(int(count[s]))] for s in range(b)]
    for s in range(b):
        dense[s][:, slots[s]] = torch.from_numpy(x[s][:, :len(slots[s])]).double()
    conv_w = torch.from_numpy(w).double().view(ksize, ksize, ksize, c, o).permute(4, 3, 0, 1, 2)
    h = (ksize - 1) // 2
    y = torch.nn.functional.conv3d(dense.view(b, c, res, res, res), conv_w, torch.from_numpy(bias).double(), padding=h * dil, dilation=dil)
    for s in range(b):
        np.testing.assert_allclose(y[s].view(o, -1)[:, slots[s]].numpy(), want[s][:, :len(slots[s])], rtol=1e-12, atol=1e-12)
        assert (want[s][:, len(slots[s]):] == 0).all()


def test_cpu_autograd_against_float64(maps):
    case = CASES[3]
    res, b, n, _, ksize, dil = case
    xyz, lo, extent, _, (_, _, count), _ = maps[case]
    m = int(count.max()) + 1
    _, _, nbr = ref.build(xyz, res, lo, extent, m, ksize, dil)
    ops, vindex, gindex = _ops_index(xyz, res, lo, extent, m)
    cmap = ops.cell_neighbours(vindex, gindex, ksize, dil)
    c, o = 4, 3
    x, w, bias = ref.gaussian_inputs(9, b, c, o, m, 27)
    g = ref.gaussian_inputs(10, b, o, 1, m, 1)[0]
    tx, tw, tb = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, bias))
    ops.sparse_conv(tx, cmap, tw, tb).backward(torch.from_numpy(g))
    gx = ref.grad_x_scatter(g, nbr, w, m)
    gw, gb = ref.grad_weight_bias(x, g, nbr)
    # the mirrored forward is the scatter definition: the map is symmetric
    mirrored, d, big_s = ref.sparse_conv(g, nbr, np.ascontiguousarray(w[::-1].transpose(0, 2, 1)))
    np.testing.assert_allclose(mirrored, gx, rtol=1e-12, atol=1e-12)
    assert ref.share(tx.grad.numpy(), gx, d, big_s) <= 1.0
    np.testing.assert_allclose(tw.grad.numpy(), gw, rtol=1e-4, atol=1e-4 * np.abs(gw).max())
    np.testing.assert_allclose(tb.grad.numpy(), gb, rtol=1e-4, atol=1e-4 * np.abs(gb).max())


def test_module_matches_conv3d_and_initialises_like_it():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    torch.manual_seed(3)
    res, b, n, c, o = 8, 2, 300, 5, 6
    xyz = torch.rand(b, n, 3) - 0.5
    feats = torch.randn(b, c, n)
    pooled = ops.grid_pool(xyz, feats, res, reduce='mean')
    vindex = ops.voxel_index(xyz, res)
    for ksize, dil in ((3, 1), (5, 2)):
        conv = ops.SubmanifoldConv3d(c, o, ksize, dil)
        dense_conv = torch.nn.Conv3d(c, o, ksize, padding=(ksize - 1) // 2 * dil, dilation=dil)
        assert conv.weight.shape == (ksize ** 3, c, o) and conv.bias.shape == (o,)
        bound = 1 / (c * ksize ** 3) ** 0.5  # Conv3d's: both tensors uniform inside +-1 / sqrt(fan_in)
        assert float(conv.weight.detach().abs().max()) <= bound and float(conv.bias.detach().abs().max()) <= bound
        assert abs(float(conv.weight.detach().std()) / float(dense_conv.weight.detach().std()) - 1) < 0.1
        with torch.no_grad():
            dense_conv.weight.copy_(conv.weight.view(ksize, ksize, ksize, c, o).permute(4, 3, 0, 1, 2))
            dense_conv.bias.copy_(conv.bias)
        cmap = ops.cell_neighbours(vindex, pooled.index, ksize, dil)
        y = conv(pooled.features, cmap)
        back = ops.grid_unpool(y, pooled.index)  # the level end to end
        assert back.shape == (b, o, n)
        dense = dense_conv(ops.voxelize(feats, vindex))  # voxelize is the mean per cell: the same level, dense
        at = vindex.cell.long()[:, None, :].expand(b, o, n)
        torch.testing.assert_close(back, torch.gather(dense.view(b, o, -1), 2, at), rtol=1e-4, atol=1e-5)
        y.sum().backward()
        assert conv.weight.grad is not None and conv.bias.grad is not None
    assert ops.SubmanifoldConv3d(c, o, bias=False).bias is None
    with pytest.raises(ValueError, match='expected a SparseConvMap with kernel_size 3'):
        ops.SubmanifoldConv3d(c, o)(pooled.features, cmap)


def test_python_argument_checks():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    xyz = torch.rand(2, 10, 3) - 0.5
    vindex = ops.voxel_index(xyz, 5)
    gi = ops.grid_cluster(vindex, m=6)
    cmap = ops.cell_neighbours(vindex, gi)
    for k in (1, 2, 4, 7, 3.0, True, None):
        with pytest.raises(ValueError, match='kernel_size must be 3 or 5'):
            ops.cell_neighbours(vindex, gi, k)
    for d in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match='dilation must be'):
            ops.cell_neighbours(vindex, gi, 3, d)
    for bad in (None, tuple(vindex), xyz):
        with pytest.raises(ValueError, match='cell_neighbours: expected a VoxelIndex'):
            ops.cell_neighbours(bad, gi)
    for bad in (None, tuple(gi), vindex, ops.GridIndex(gi.cluster[:, :9], gi.seg, gi.count, gi.order), ops.GridIndex(gi.cluster, gi.seg, gi.count[:1], gi.order),
                ops.GridIndex(gi.cluster, gi.seg[:, :1], gi.count, gi.order)):
        with pytest.raises(ValueError, match='cell_neighbours:'):
            ops.cell_neighbours(vindex, bad)
    with pytest.raises(RuntimeError, match='index.seg must be torch'):
        ops.cell_neighbours(vindex, ops.GridIndex(gi.cluster, gi.seg.long(), gi.count, gi.order))
    with pytest.raises(RuntimeError, match='index.cell must be torch'):
        ops.cell_neighbours(ops.VoxelIndex(vindex.cell.long(), vindex.order, vindex.counts), gi)
    with pytest.raises(RuntimeError, match='expected cpu'):
        ops.cell_neighbours(vindex, ops.GridIndex(gi.cluster, gi.seg.to('meta'), gi.count, gi.order))
    assert ops.cell_neighbours(vindex, gi, 3, 10 ** 12).nbr.shape == (2, 6, 27)  # any dilation: only the centre is left
    x, w, bias = torch.zeros(2, 4, 6), torch.zeros(27, 4, 3), torch.zeros(3)
    assert ops.sparse_conv(x, cmap, w, bias).shape == (2, 3, 6)
    for bx, bm, bw, bb in ((x, cmap.nbr, w, bias), (x, tuple(cmap), w, bias), (x[0], cmap, w, bias), (x[:, :, :5], cmap, w, bias), (x[:1], cmap, w, bias),
                           (x, cmap, w[:26], bias), (x, cmap, w[:, :3], bias), (x, cmap, w[:, :, :0], bias), (x, cmap, w[0], bias),
                           (x, cmap, w, bias[:2]), (x, cmap, w, bias[None]), (x, cmap._replace(kernel_size=5), w, bias),
                           (x, cmap._replace(dilation=0), w, bias), (x, cmap._replace(nbr=cmap.nbr[:, :, :26]), w, bias)):
        with pytest.raises(ValueError, match='sparse_conv:'):
            ops.sparse_conv(bx, bm, bw, bb)
    for bx, bm, bw, bb, name in ((x.double(), cmap, w, bias, 'features'), (x, cmap, w.double(), bias, 'weight'), (x, cmap, w, bias.double(), 'bias'),
                                 (x, cmap._replace(nbr=cmap.nbr.int()), w, bias, 'cmap.nbr')):
        with pytest.raises(RuntimeError, match=f'{name} must be torch'):
            ops.sparse_conv(bx, bm, bw, bb)
    with pytest.raises(RuntimeError, match='expected cpu'):
        ops.sparse_conv(x, cmap, w.to('meta'), bias)
    empty = ops.cell_neighbours(ops.voxel_index(xyz[:0], 5), ops.grid_cluster(ops.voxel_index(xyz[:0], 5), m=6))
    assert empty.nbr.shape == (0, 6, 27) and ops.sparse_conv(x[:0], empty, w, bias).shape == (0, 3, 6)
    for args in ((0, 3), (4, 0), (4, 3, 4), (4, 3, 3, 0), (True, 3)):
        with pytest.raises(ValueError, match='SubmanifoldConv3d:'):
            ops.SubmanifoldConv3d(*args)


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched: the guard stays)."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)(*([0x5a] * 64))
    p = ctypes.addressof(buf)

    def nbrs(b=1, n=8, m=4, res=4, ksize=3, dil=1, q=(p,) * 5):
        return L.pcc_cell_neighbours(b, n, m, res, ksize, dil, *q, None)

    def conv(b=1, c=3, o=2, n=8, m=4, t=27, q=(p,) * 5):
        return L.pcc_sparse_conv(b, c, o, n, m, t, *q, None)

    bad_map = [dict(b=-1), dict(b=65536), dict(n=0), dict(n=vref.MAX_POINTS + 1, m=4), dict(m=0), dict(m=9), dict(m=-1), dict(res=1), dict(res=129),
               dict(ksize=1), dict(ksize=4), dict(ksize=7), dict(ksize=-3), dict(dil=0), dict(dil=-2), dict(b=65535, n=16384, m=16384, ksize=5),
               dict(b=5000, n=16384, m=16384), dict(b=0, m=9), dict(b=0, ksize=2)]
    for kw in bad_map:
        assert nbrs(**kw) == EINVAL and L.pcc_last_error().decode().startswith('cell_neighbours:'), kw
    bad_conv = [dict(b=-1), dict(b=65536), dict(c=0), dict(o=0), dict(n=0), dict(m=0), dict(m=-1), dict(t=0), dict(m=1 << 28, t=27),
                dict(c=1 << 12, o=1 << 12, t=128), dict(b=0, c=0), dict(b=0, t=0)]
    for kw in bad_conv:
        assert conv(**kw) == EINVAL and L.pcc_last_error().decode().startswith('sparse_conv:'), kw
    for i in range(5):  # every pointer on its own; the bias may be null, and a call with nothing else wrong would be enqueued
        q = [p] * 5
        q[i] = None
        assert nbrs(q=q) == EINVAL and L.pcc_last_error().decode() == 'cell_neighbours: null pointer'
        if i != 3:
            assert conv(q=q) == EINVAL and L.pcc_last_error().decode() == 'sparse_conv: null pointer'
    for ksize, dil in itertools.product((3, 5), (1, 1000)):  # an empty batch enqueues nothing, whatever the pointers
        assert nbrs(b=0, ksize=ksize, dil=dil, q=(None,) * 5) == 0 and L.pcc_last_status() == 0
    assert conv(b=0, q=(None,) * 5) == 0 and L.pcc_last_status() == 0
    assert bytes(buf) == b'\x5a' * 64


def test_the_abi_is_bound_and_the_tuning_table_is_untouched():
    from pointcloudcounterfactual_amd import _lib

    assert [len(_lib.ABI[f][1]) for f in ('pcc_cell_neighbours', 'pcc_sparse_conv')] == [12, 12]
    assert len(_lib.TUNING) == 16 and max(_lib.TUNING.values()) == 15
