"""CPU tests of the strided and transposed sparse convolution between two voxel levels: the numpy reference
(tests/strided_conv_reference.py) against ``torch.nn.functional.conv3d(stride=2)`` and ``conv_transpose3d(stride=2)`` on dense
grids in float64, the torch rules of ``coarsen_level`` and ``stride_map`` word for word against the reference, the properties
of the map, a second coarsening with the existing ops on it, and the CPU path of the two ops against float64 autograd."""

import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import grid_pool_reference as gref
from tests import sparse_conv_reference as sref
from tests import strided_conv_reference as ref
from tests import voxel_reference as vref


def _clouds(seed, n, res, lo, extent):
    """B = 3: mixed (a NaN point first, an infinite point last), all points in one cell, mixed again."""
    return np.concatenate([vref.cloud(seed + i, 1, n, res, lo, extent, kind) for i, kind in enumerate(('mixed', 'one_cell', 'mixed'))])


def _levels(res, cut):
    """The two levels of three clouds at resolution ``res``; ``cut``: both capacities below the fullest cloud's counts."""
    n = 40 if res <= 4 else 300
    lo, extent = vref.grid_of(res, res % 2)
    xyz = _clouds(res, n, res, lo, extent)
    assert np.isnan(xyz[0]).any()
    lv = ref.build(xyz, res, lo, extent)
    u_f, u_c = int(lv['gi'][2].max()), int(lv['cgi'][2].max())
    assert int(lv['gi'][2].min()) == 1  # the cloud in one cell
    if cut and u_c > 1:
        lv = ref.build(xyz, res, lo, extent, u_f - 1, u_c - 1)
        assert int(lv['cgi'][2].max()) >= u_c - 1
    else:
        lv = ref.build(xyz, res, lo, extent, u_f, u_c)
    return xyz, lv


def _ops_level(lv, level='fine'):
    """The ``VoxelIndex`` and ``GridIndex`` of a reference level as CPU tensors."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    vi, gi, res = (lv['vi'], lv['gi'], lv['res']) if level == 'fine' else (lv['cvi'], lv['cgi'], lv['rc'])
    b = vi[0].shape[0]
    vindex = ops.VoxelIndex(torch.from_numpy(vi[0]), torch.from_numpy(vi[1]), torch.from_numpy(vi[2]).view(b, res, res, res))
    return vindex, ops.GridIndex(torch.from_numpy(gi[0]), torch.from_numpy(gi[1]), torch.from_numpy(gi[2]), vindex.order)


@pytest.mark.parametrize('cut', [False, True], ids=['full', 'cut'])
@pytest.mark.parametrize('res', [3, 4, 9, 32])
def test_reference_map_and_both_convolutions_are_the_dense_ones(res, cut):
    _, lv = _levels(res, cut)
    b, rc = 3, lv['rc']
    m_f, m_c = lv['up'].shape[1], lv['down'].shape[1]
    c, o = 3, 4
    rng = np.random.default_rng(res)
    fine_cells, coarse_cells = ref.slot_cells(lv['vi'], lv['gi']), ref.slot_cells(lv['cvi'], lv['cgi'])
    even = 2 * rc  # the dense fine grid padded to an even size
    # the way down
    x, w, bias = rng.standard_normal((b, c, m_f)), rng.standard_normal((8, c, o)), rng.standard_normal(o)
    for s in range(b):
        x[s, :, len(fine_cells[s]):] = 0  # padded slots hold +0
    got, _, _ = sref.sparse_conv(x, lv['down'], w, bias)
    want = F.conv3d(torch.from_numpy(ref.dense(x, fine_cells, lv['res'], even)), torch.from_numpy(w).view(2, 2, 2, c, o).permute(4, 3, 0, 1, 2),
                    torch.from_numpy(bias), stride=2).numpy()
    assert want.shape[2:] == (rc, rc, rc)
    for s in range(b):
        at = np.array(coarse_cells[s])
        np.testing.assert_allclose(got[s][:, :len(at)], want[s].reshape(o, -1)[:, at], rtol=1e-12, atol=1e-12)
        assert (got[s][:, len(at):] == 0).all()
        assert (lv['down'][s, :len(at)] >= 0).any(1).all()  # every real coarse slot has a child
    # the way up: the dense transposed convolution read at the occupied fine cells
    y, v = rng.standard_normal((b, c, m_c)), rng.standard_normal((8, c, o))
    for s in range(b):
        y[s, :, len(coarse_cells[s]):] = 0
    got, _, _ = sref.sparse_conv(y, lv['up'], v, bias)
    want = F.conv_transpose3d(torch.from_numpy(ref.dense(y, coarse_cells, rc, rc)), torch.from_numpy(v).view(2, 2, 2, c, o).permute(3, 4, 0, 1, 2),
                              torch.from_numpy(bias), stride=2).numpy()
    assert want.shape[2:] == (even, even, even)
    for s in range(b):
        cells = np.array(fine_cells[s])
        at = (cells // lv['res'] ** 2 * even + cells // lv['res'] % lv['res']) * even + cells % lv['res']
        has = (lv['up'][s, :len(at)] >= 0).any(1)  # (a fine slot whose parent was dropped stays +0, without the bias)
        assert cut or has.all()
        np.testing.assert_allclose(got[s][:, :len(at)][:, has], want[s].reshape(o, -1)[:, at[has]], rtol=1e-12, atol=1e-12)
        assert (got[s][:, :len(at)][:, ~has] == 0).all() and (got[s][:, len(at):] == 0).all()


@pytest.mark.parametrize('cut', [False, True], ids=['full', 'cut'])
@pytest.mark.parametrize('res', [3, 4, 9, 32])
def test_cpu_paths_word_for_word_and_map_properties(res, cut):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    _, lv = _levels(res, cut)
    vindex, gindex = _ops_level(lv)
    m_c = lv['down'].shape[1]
    coarse, cgindex, tap = ops.coarsen_level(vindex, gindex, m=m_c)
    cell_c, order_c, counts_c = lv['cvi']
    assert np.array_equal(coarse.cell.numpy(), cell_c) and np.array_equal(coarse.order.numpy(), order_c)
    assert np.array_equal(coarse.counts.numpy().reshape(3, -1), counts_c) and np.array_equal(tap.numpy(), lv['tap'])
    assert all(t.dtype == torch.int32 for t in (*coarse, tap))
    for got, want in zip(cgindex[:3], lv['cgi']):
        assert np.array_equal(got.numpy(), want)
    smap = ops.stride_map(tap, cgindex)
    down, up = smap.down.numpy(), smap.up.numpy()
    assert np.array_equal(down, lv['down']) and np.array_equal(up, lv['up']) and smap.down.dtype == smap.up.dtype == torch.int64
    assert np.array_equal(smap.count_fine.numpy(), np.minimum(lv['gi'][2], up.shape[1])) and np.array_equal(smap.count_coarse.numpy(), lv['cgi'][2])
    # up and down are transposes of each other
    s, r, t = np.nonzero(down >= 0)
    assert (up[s, down[s, r, t], t] == r).all()
    s, f, t = np.nonzero(up >= 0)
    assert (down[s, up[s, f, t], t] == f).all() and (down >= 0).sum() == (up >= 0).sum()
    for s in range(3):
        kept_c, kept_f = min(int(lv['cgi'][2][s]), m_c), min(int(lv['gi'][2][s]), up.shape[1])
        children = (down[s] >= 0).sum(1)
        assert (children[:kept_c] >= 1).all() and (children[kept_c:] == 0).all() and int(counts_c[s].max()) <= 8
        taps = (up[s] >= 0).sum(1)
        dropped = lv['cgi'][0][s] < 0  # the parent's rank is >= m_c (or the slot is padded)
        assert (taps[:kept_f][~dropped[:kept_f]] == 1).all() and (taps[dropped] == 0).all() and (taps[kept_f:] == 0).all()
    # m=None: the fullest cloud's count
    assert ops.coarsen_level(vindex, gindex)[1].seg.shape[1] - 1 == int(lv['cgi'][2].max())


def test_coarsening_nests_and_the_existing_ops_take_the_second_level():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    res, n = 32, 400
    xyz = _clouds(5, n, res, -0.5, 1.0)
    first = ref.build(xyz, res, -0.5, 1.0, int(vref.voxel_index(xyz, res, -0.5, 1.0)[2].astype(bool).sum(1).max()))
    second = ref.coarsen(first['cvi'], first['cgi'], first['rc'])
    assert (first['rc'], second['rc']) == (16, 8)
    vindex, gindex = _ops_level(first)
    c1, g1, tap1 = ops.coarsen_level(vindex, gindex, m=first['down'].shape[1])
    c2, g2, tap2 = ops.coarsen_level(c1, g1, m=second['down'].shape[1])
    assert c2.counts.shape[1:] == (8, 8, 8) and np.array_equal(tap2.numpy(), second['tap'])
    for got, want in zip((*c2[:2], *g2[:3]), (*second['cvi'][:2], *second['cgi'])):
        assert np.array_equal(got.numpy(), want)
    smap = ops.stride_map(tap2, g2)
    assert np.array_equal(smap.down.numpy(), second['down']) and np.array_equal(smap.up.numpy(), second['up'])
    # the second level is an ordinary level: its submanifold map from the cells, pooling from the first level and back
    cells = ref.slot_cells(second['cvi'], second['cgi'])
    assert all(len(set(row)) == len(row) and row == sorted(row) for row in cells)
    nbr = ops.cell_neighbours(c2, g2).nbr.numpy()
    want = sref.cell_neighbours(second['cvi'][0], second['cvi'][1], second['cgi'][1], second['cgi'][2], 8, 3, 1)
    assert np.array_equal(nbr, want) and sref.is_symmetric(nbr)
    for s in range(3):
        assert (nbr[s, :len(cells[s]), 13] == np.arange(len(cells[s]))).all()  # the centre tap is the slot
    m1 = first['down'].shape[1]
    feats = np.random.default_rng(0).standard_normal((3, 5, m1)).astype(np.float32)
    for mode in ('max', 'mean'):
        pooled = ops.segment_pool(torch.from_numpy(feats), g2, mode).numpy()
        want, _ = gref.segment_pool(feats, second['cvi'][1], second['cgi'][1], gref.MODES[mode])
        assert np.array_equal(pooled, want)
    back = ops.grid_unpool(torch.from_numpy(pooled), g2).numpy()
    slot = second['cgi'][0]
    for s in range(3):
        assert np.array_equal(back[s][:, slot[s] >= 0], pooled[s][:, slot[s][slot[s] >= 0]]) and (back[s][:, slot[s] < 0] == 0).all()


@pytest.mark.parametrize('way', ['down', 'up'])
def test_cpu_node_every_subset_of_gradients_against_float64_autograd(way):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    _, lv = _levels(9, True)
    smap = ops.StrideMap(torch.from_numpy(lv['down']), torch.from_numpy(lv['up']), torch.from_numpy(lv['gi'][2]), torch.from_numpy(lv['cgi'][2]))
    op, lst = (ops.strided_sparse_conv, smap.down) if way == 'down' else (ops.sparse_conv_transpose, smap.up)
    n, m = (smap.up.shape[1], smap.down.shape[1]) if way == 'down' else (smap.down.shape[1], smap.up.shape[1])
    c, o = 5, 6
    x, w, bias = sref.gaussian_inputs(3, 3, c, o, n, 8)
    g = sref.gaussian_inputs(4, 3, o, 1, m, 1)[0]
    # float64 autograd of the composition: gather per tap, matmul, mask
    x64, w64, b64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, bias))
    want = ops.torch_sparse_conv(x64, lst, w64, b64)
    want.backward(torch.from_numpy(g).double())
    ref_out, d, big_s = sref.sparse_conv(x, lst.numpy(), w, bias)
    np.testing.assert_allclose(want.detach().numpy(), ref_out, rtol=1e-12, atol=1e-12)
    gw64, dw, sw = ref.wgrad(x, lst.numpy(), g)
    np.testing.assert_allclose(w64.grad.numpy(), gw64, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(x64.grad.numpy(), sref.grad_x_scatter(g, lst.numpy(), w, n), rtol=1e-12, atol=1e-12)
    gamma = (3 * m + 1) * 2.0 ** -24  # sums of at most B * m terms in an order torch chooses
    for needs in itertools.product((False, True), repeat=3):
        tx, tw, tb = (torch.from_numpy(a).requires_grad_(need) for a, need in zip((x, w, bias), needs))
        out = op(tx, smap, tw, tb)
        assert out.shape == (3, o, m) and sref.share(out.detach().numpy(), ref_out, d, big_s) <= 1.0
        if any(needs):
            out.backward(torch.from_numpy(g))
        assert [t.grad is not None for t in (tx, tw, tb)] == list(needs)
        if needs[0]:
            assert (np.abs(tx.grad.numpy() - x64.grad.numpy()) <= 9 * o * 2.0 ** -24 * sref.grad_x_scatter(np.abs(g), lst.numpy(), np.abs(w), n)).all()
        if needs[1]:
            assert (np.abs(tw.grad.numpy() - gw64) <= gamma * sw + 1e-300).all()
        if needs[2]:
            assert (np.abs(tb.grad.numpy() - b64.grad.numpy()) <= gamma * np.abs(g).sum((0, 2))).all()
    gw = ops.sparse_conv_wgrad(torch.from_numpy(x), lst, torch.from_numpy(g)).numpy()
    assert ref.wgrad_share(gw, gw64, np.maximum(dw, 3 * m), sw) <= 1.0  # (torch's einsum: at most B * m terms per word)


def test_argument_checks_and_modules():
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    import pointcloudcounterfactual_amd as pkg

    for name in ('StrideMap', 'coarsen_level', 'stride_map', 'strided_sparse_conv', 'sparse_conv_transpose', 'sparse_conv_wgrad', 'SparseConv3d',
                 'SparseConvTranspose3d'):
        assert getattr(pkg, name) is getattr(ops, name) and name in pkg.__all__
    _, lv = _levels(4, False)
    vindex, gindex = _ops_level(lv)
    coarse, cgindex, tap = ops.coarsen_level(vindex, gindex)
    smap = ops.stride_map(tap, cgindex)
    m_f, m_c = smap.up.shape[1], smap.down.shape[1]
    with pytest.raises(ValueError, match='coarsen_level: the resolution must be >= 3'):
        ops.coarsen_level(*_ops_level(lv, 'coarse'))  # (R = 4 -> 2: no third level)
    with pytest.raises(ValueError, match='coarsen_level: m must be'):
        ops.coarsen_level(vindex, gindex, m=m_f + 1)
    with pytest.raises(ValueError, match='strided_sparse_conv: expected a StrideMap'):
        ops.strided_sparse_conv(torch.zeros(3, 2, m_f), smap.down, torch.zeros(8, 2, 2))
    with pytest.raises(ValueError, match='strided_sparse_conv: expected features'):
        ops.strided_sparse_conv(torch.zeros(3, 2, m_f + 1), smap, torch.zeros(8, 2, 2))
    with pytest.raises(ValueError, match='sparse_conv_transpose: expected weight'):
        ops.sparse_conv_transpose(torch.zeros(3, 2, m_c), smap, torch.zeros(27, 2, 2))
    with pytest.raises(RuntimeError, match='tap must be torch.int32'):
        ops.stride_map(tap.long(), cgindex)
    with pytest.raises(ValueError, match='sparse_conv_wgrad: expected grad'):
        ops.sparse_conv_wgrad(torch.zeros(3, 2, m_f), smap.down, torch.zeros(3, 2, m_c + 1))
    torch.manual_seed(0)
    down, up = ops.SparseConv3d(3, 5), ops.SparseConvTranspose3d(5, 3, bias=False)
    assert down.weight.shape == (8, 3, 5) and up.weight.shape == (8, 5, 3) and up.bias is None
    assert float(down.weight.detach().abs().max()) <= 24 ** -0.5 and float(down.bias.detach().abs().max()) <= 24 ** -0.5  # Conv3d: fan_in = 8 C
    assert float(up.weight.detach().abs().max()) <= 24 ** -0.5  # ConvTranspose3d: fan_in = 8 O
    y = down(torch.randn(3, 3, m_f), smap)
    assert y.shape == (3, 5, m_c) and up(y, smap).shape == (3, 3, m_f)
    # a coarse slot without a child stays +0 without the bias
    assert (y[1, :, 1:] == 0).all() and (y[1, :, 0] != 0).any()
