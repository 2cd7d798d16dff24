"""GPU tests of the submanifold sparse convolution (``pcc_cell_neighbours`` and ``pcc_sparse_conv`` through the C ABI on guarded,
prefilled buffers, and ``neighbour_ops.cell_neighbours`` / ``sparse_conv`` / ``SubmanifoldConv3d``).  The map is integers: word
for word against the numpy loops of tests/sparse_conv_reference.py and the CPU path.  The convolution's contract is a bound:
exact equality with float64 on lattice inputs (which separates indexing errors from rounding), the contract's bar on Gaussian
inputs, float equality between runs and batch positions."""

import itertools

import numpy as np
import pytest
import torch

from tests import sparse_conv_reference as ref
from tests import voxel_reference as vref
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

GUARD = 32        # words of sentinel around every output
INT_FILL = -7777  # what an integer output holds before the call
KD = list(itertools.product((3, 5), (1, 2, 3)))  # (kernel size, dilation)


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


class _Out:
    """An output of ``shape`` inside a flat buffer with GUARD sentinel words on either side.  Floats start as NaN with a
    payload no kernel produces, integers as INT_FILL: every element must be written, and nothing around it."""

    FLOAT_FILL = 0x7fdead00

    def __init__(self, shape, dtype, cuda):
        self.is_float = dtype == torch.float32
        numel = int(np.prod(shape))
        self.flat = torch.full((numel + 2 * GUARD,), self.FLOAT_FILL if self.is_float else INT_FILL, dtype=torch.int32 if self.is_float else dtype,
                               device=cuda)
        self.lo, self.hi = GUARD, GUARD + numel
        self.view = self.flat[self.lo:self.hi].view(shape)

    def ptr(self):
        return self.view.data_ptr()

    def numpy(self):
        flat = self.flat.cpu().numpy()
        fill = self.FLOAT_FILL if self.is_float else INT_FILL
        assert (np.concatenate((flat[:self.lo], flat[self.hi:])) == fill).all()
        body = flat[self.lo:self.hi].reshape(self.view.shape)
        assert not (body == fill).any()
        return body.view(np.float32) if self.is_float else body


def _call(name, dev, *args):
    from pointcloudcounterfactual_amd import _lib

    _lib.call(getattr(_lib.lib, 'pcc_' + name), name, dev, *args)


def _map(cuda, vi, gi, res, ksize, dil):
    """``pcc_cell_neighbours`` on the numpy index ``vi`` and partition ``gi``, as numpy."""
    cell, order, _ = vi
    _, seg, count = gi
    b, n = cell.shape
    m = seg.shape[1] - 1
    dcell, dorder, dseg, dcount = (_dev(a, cuda) for a in (cell, order, seg, count))
    nbr = _Out((b, m, ksize ** 3), torch.int64, cuda)
    _call('cell_neighbours', cuda, b, n, m, res, ksize, dil, dcell.data_ptr(), dorder.data_ptr(), dseg.data_ptr(), dcount.data_ptr(), nbr.ptr())
    return nbr.numpy()


def _conv(cuda, x, nbr, w, bias):
    """``pcc_sparse_conv`` on numpy inputs, as numpy."""
    b, c, n = x.shape
    m, taps = nbr.shape[1:]
    o = w.shape[2]
    dx, dn, dw = _dev(x, cuda), _dev(nbr, cuda), _dev(w, cuda)
    db = None if bias is None else _dev(bias, cuda)
    out = _Out((b, o, m), torch.float32, cuda)
    _call('sparse_conv', cuda, b, c, o, n, m, taps, dx.data_ptr(), dn.data_ptr(), dw.data_ptr(), None if db is None else db.data_ptr(), out.ptr())
    return out.numpy()


def _three_clouds(seed, n, res, lo, extent):
    """B = 3 with a different number of occupied cells per cloud: mixed (a NaN point first, an infinite point last), all
    points in one cell, each point in its own cell (where the grid has that many cells; mixed otherwise)."""
    kinds = ('mixed', 'one_cell', 'own_cell' if n <= res ** 3 else 'mixed')
    return np.concatenate([vref.cloud(seed + i, 1, n, res, lo, extent, kind) for i, kind in enumerate(kinds)])


def _check_map(cuda, xyz, res, lo, extent, m, ksize, dil, cpu=True):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    vi, gi, want = ref.build(xyz, res, lo, extent, m, ksize, dil)
    got = _map(cuda, vi, gi, res, ksize, dil)
    assert np.array_equal(got, want), (xyz.shape, res, m, ksize, dil)
    if cpu:
        b = xyz.shape[0]
        vindex = ops.VoxelIndex(*(torch.from_numpy(a) for a in vi[:2]), torch.from_numpy(vi[2]).view(b, res, res, res))
        gindex = ops.GridIndex(torch.from_numpy(gi[0]), torch.from_numpy(gi[1]), torch.from_numpy(gi[2]), vindex.order)
        assert np.array_equal(ops.cell_neighbours(vindex, gindex, ksize, dil).nbr.numpy(), want)
    return want


@pytest.mark.parametrize('res', [2, 3, 32, 128])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 1024, 1025, 16384])
def test_map_word_for_word_at_every_size(cuda, n, res):
    lo, extent = vref.grid_of(res, n % 2)
    xyz = _three_clouds(n + res, n, res, lo, extent)
    _check_map(cuda, xyz, res, lo, extent, n, 3, 1)
    if n <= 1025:  # (the numpy loops over 125 taps of 16384 slots take too long: the large clouds keep to 27 taps)
        ksize, dil = KD[1:][(n + res) % 5]
        _check_map(cuda, xyz, res, lo, extent, n, ksize, dil)
    else:
        _check_map(cuda, xyz, res, lo, extent, n, 3, 2 + res % 2, cpu=False)


@pytest.mark.parametrize('ksize,dil', KD)
def test_map_kernels_dilations_capacities_and_batch_positions(cuda, ksize, dil):
    res, n = 8, 300
    lo, extent = vref.grid_of(res, dil % 2)
    xyz = _three_clouds(ksize * 10 + dil, n, res, lo, extent)
    xyz[2, 200:] = xyz[2, 0]  # (200 occupied cells, so that U + 1 is a capacity)
    full = _check_map(cuda, xyz, res, lo, extent, n, ksize, dil)
    assert ref.is_symmetric(full)
    occupied = (full[:, :, ksize ** 3 // 2] >= 0).sum(1)
    u = int(occupied.max())
    assert len(set(occupied.tolist())) == 3 and 1 < u < n  # a different U per cloud
    for m in sorted({1, u - 1, u, u + 1, n}):
        assert np.array_equal(_check_map(cuda, xyz, res, lo, extent, m, ksize, dil), ref.cut(full, m))
    m = u - 1
    want = ref.cut(full, m)
    for shift in (1, 2):  # every cloud at every batch position ...
        got = _check_map(cuda, np.roll(xyz, shift, 0), res, lo, extent, m, ksize, dil, cpu=False)
        assert np.array_equal(np.roll(got, -shift, 0), want)
    for s in range(3):  # ... and alone
        assert np.array_equal(_check_map(cuda, xyz[s:s + 1], res, lo, extent, m, ksize, dil, cpu=False)[0], want[s])


def _random_list(seed, b, m, n, taps, empty=0.5):
    rng = np.random.default_rng(seed)
    nbr = rng.integers(0, n, size=(b, m, taps)).astype(np.int64)
    nbr[rng.random((b, m, taps)) < empty] = -1
    return nbr


def _exact(cuda, x, nbr, w, bias):
    want, _, _ = ref.sparse_conv(x, nbr, w, bias)
    got = _conv(cuda, x, nbr, w, bias)
    assert np.array_equal(got.astype(np.float64), want), (x.shape, w.shape, nbr.shape)
    return got


SIZES = (1, 3, 4, 5, 31, 32, 33, 64, 65, 130)


@pytest.mark.parametrize('c', SIZES)
def test_conv_every_channel_count_exact_and_inside_the_bar(cuda, c):
    b, m, n, taps = 2, ref.ROW_TILE + 1, 50, 27  # (a partial tile of either kernel)
    worst = 0.0
    for o in SIZES:
        nbr = _random_list(c * 1000 + o, b, m, n, taps)
        nbr[0, 3] = -1  # a padded slot
        x, w, bias = ref.lattice_inputs(c + o, b, c, o, n, taps)
        got = _exact(cuda, x, nbr, w, bias if o % 2 else None)
        assert (got[0, :, 3].view(np.uint32) == 0).all()  # +0, without the bias
        x, w, bias = ref.gaussian_inputs(c + o, b, c, o, n, taps)
        want, d, big_s = ref.sparse_conv(x, nbr, w, bias)
        worst = max(worst, ref.share(_conv(cuda, x, nbr, w, bias), want, d, big_s))
    print(f'c = {c}: largest share of the bar {worst:.3f}')
    assert worst <= 1.0


# the row tiles of the two kernels: a tile of the MFMA kernel, a wave of it, a wave of the VALU kernel, a workgroup of the MFMA kernel
TILES = (ref.MFMA_TILE, ref.MFMA_WAVE_ROWS, ref.ROW_TILE, ref.MFMA_ROWS)


@pytest.mark.parametrize('c,o', [(5, 9), (9, 20)], ids=['valu', 'mfma'])
@pytest.mark.parametrize('taps', [27, 125])
def test_conv_row_tile_boundaries_bias_and_padding(cuda, taps, c, o):
    assert ref.kernel_of(5, 9).startswith('sparse_conv_kernel') and ref.kernel_of(9, 20).startswith('sparse_conv_mfma_kernel')
    b, n = 2, 40
    for m in sorted({1, 3 * ref.ROW_TILE + 7} | {tile + d for tile in TILES for d in (-1, 0, 1)}):
        nbr = _random_list(m + taps, b, m, n, taps, empty=0.7)
        nbr[1, m - 1] = -1  # a padded slot
        nbr[1, 0] = -1
        nbr[1, 0, taps // 2] = 7  # a row with only the centre tap
        x, w, bias = ref.lattice_inputs(m, b, c, o, n, taps)
        for with_bias in (True, False):
            got = _exact(cuda, x, nbr, w, bias if with_bias else None)
            assert m == 1 or (got[1, :, m - 1].view(np.uint32) == 0).all()
            assert np.array_equal(got[1, :, 0], w[taps // 2].T @ x[1, :, 7] + (bias if with_bias else 0))


@pytest.mark.parametrize('tile,c,o', [(ref.ROW_TILE, 6, 7), (ref.MFMA_TILE, 12, 18), (ref.MFMA_TILE, 16, 64)], ids=['valu', 'mfma', 'mfma64'])
def test_conv_tap_empty_for_a_whole_tile_next_to_a_tile_where_one_row_has_it(cuda, tile, c, o):
    assert ref.kernel_of(c, o).startswith('sparse_conv_kernel' if tile == ref.ROW_TILE else 'sparse_conv_mfma_kernel')
    b, taps = 1, 27
    m = n = 4 * tile
    nbr = np.random.default_rng(0).integers(0, n, size=(b, m, taps)).astype(np.int64)
    nbr[0, :tile, 3] = -1       # the first tile skips tap 3 ...
    nbr[0, tile + 6, 3] = -1    # ... the second computes it, with a +0 feature in one row
    nbr[0, tile:2 * tile, 5] = -1
    nbr[0, tile + 9, 5] = 2     # (and the reverse: one row of a tile has a tap the rest lacks)
    nbr[0, 2 * tile:, 7] = -1   # two tiles side by side skip tap 7 (a whole wave of the MFMA kernel)
    x, w, bias = ref.lattice_inputs(1, b, c, o, n, taps)
    _exact(cuda, x, nbr, w, bias)
    x, w, bias = ref.gaussian_inputs(1, b, c, o, n, taps)
    x[0, :, 0] = np.nan  # IEEE: the rows that read slot 0 are NaN, nobody else
    want, d, big_s = ref.sparse_conv(x, nbr, w, bias)
    got = _conv(cuda, x, nbr, w, bias)
    reads = (nbr[0] == 0).any(1)
    assert reads.any() and not reads.all()
    assert np.isnan(got[0][:, reads]).all() and not np.isnan(got[0][:, ~reads]).any()
    assert ref.share(got[0][:, ~reads][None], want[0][:, ~reads][None], d[:, ~reads], big_s[0][:, ~reads][None]) <= 1.0


def test_conv_kernel_variant_at_each_boundary_of_the_dispatch(cuda):
    from pointcloudcounterfactual_amd import _lib

    b, m, n, taps = 1, 10, 10, 27
    nbr = _random_list(5, b, m, n, taps)
    for c, o in itertools.product((3, ref.MFMA_MIN_C - 1, ref.MFMA_MIN_C), (1, 8, 9, 15, 16, 17, 32, 33, 64, 65, 130)):
        x, w, bias = ref.lattice_inputs(o, b, c, o, n, taps)
        with _lib.profile() as read:
            _exact(cuda, x, nbr, w, bias)
            torch.cuda.synchronize()
            ran = {name: read(name)[1] for name in ref.KERNELS}
        assert ran == {name: int(name == ref.kernel_of(c, o)) for name in ref.KERNELS}, (c, o, ran)
    with _lib.profile() as read:
        xyz = ref.lattice_cloud(3)
        _check_map(cuda, xyz, 3, 0.0, 2.0, 27, 3, 1)
        torch.cuda.synchronize()
        assert read('cell_nbr_kernel')[1] == 1


@pytest.fixture(scope='module', params=[(6, 5), (16, 24)], ids=['valu', 'mfma'])
def level(request):
    """One grid level shared by the tests below: three clouds, their numpy index, partition and map, Gaussian inputs; with
    channel counts that take the VALU kernel forwards and backwards, and the MFMA kernel."""
    res, n, ksize, dil = 8, 400, 3, 1
    c, o = request.param
    assert ref.kernel_of(c, o).startswith('sparse_conv_mfma') == ref.kernel_of(o, c).startswith('sparse_conv_mfma') == (c > 8)
    xyz = _three_clouds(77, n, res, -0.5, 1.0)
    vi, gi, nbr = ref.build(xyz, res, -0.5, 1.0, None, ksize, dil)
    m = min(int(gi[2].max()) + 3, n)
    vi, gi, nbr = ref.build(xyz, res, -0.5, 1.0, m, ksize, dil)
    x, w, bias = ref.gaussian_inputs(5, 3, c, o, m, ksize ** 3)
    g = ref.gaussian_inputs(6, 3, o, 1, m, 1)[0]
    return dict(res=res, xyz=xyz, m=m, nbr=nbr, x=x, w=w, bias=bias, g=g)


def _gpu_map(cuda, level, rows=slice(None)):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    vindex = ops.voxel_index(_dev(level['xyz'][rows], cuda), level['res'])
    cmap = ops.cell_neighbours(vindex, ops.grid_cluster(vindex, m=level['m']))
    assert np.array_equal(cmap.nbr.cpu().numpy(), level['nbr'][rows])
    return cmap


def _run(cuda, level, cmap, rows=slice(None), needs=(True, True, True), with_bias=True):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x, w, bias = (_dev(a, cuda).requires_grad_(need) for a, need in zip((level['x'][rows], level['w'], level['bias']), needs))
    out = ops.sparse_conv(x, cmap, w, bias if with_bias else None)
    if any(needs[:2]) or (needs[2] and with_bias):
        out.backward(_dev(level['g'][rows], cuda))
    return [None if t is None else t.detach().cpu().numpy() for t in (out, x.grad, w.grad, bias.grad)]


def test_stability_alone_in_a_batch_and_twice(cuda, level):
    cmap = _gpu_map(cuda, level)
    out, gx, _, _ = _run(cuda, level, cmap)
    again = _run(cuda, level, cmap)
    assert np.array_equal(out, again[0], equal_nan=True) and np.array_equal(gx, again[1], equal_nan=True)  # (float equality: -0 == +0)
    for s in range(3):
        alone = _run(cuda, level, _gpu_map(cuda, level, slice(s, s + 1)), slice(s, s + 1))
        assert np.array_equal(alone[0][0], out[s]) and np.array_equal(alone[1][0], gx[s])
    for shift in (1, 2):
        rolled = {k: (np.roll(v, shift, 0) if k in ('xyz', 'nbr', 'x', 'g') else v) for k, v in level.items()}
        got = _run(cuda, rolled, _gpu_map(cuda, rolled))
        assert np.array_equal(np.roll(got[0], -shift, 0), out) and np.array_equal(np.roll(got[1], -shift, 0), gx)


def test_grad_x_through_the_mirrored_call_is_the_scatter_definition(cuda):
    res, ksize, dil, c, o = 6, 3, 2, 33, 9
    xyz = _three_clouds(3, 150, res, 0.0, res - 1.0)
    _, gi, nbr = ref.build(xyz, res, 0.0, res - 1.0, None, ksize, dil)
    m = int(gi[2].max())
    nbr = ref.cut(nbr, m)
    g, w, _ = ref.lattice_inputs(2, 3, o, c, m, ksize ** 3)  # (g[b,o,m]; w[t,o,c] read as the transpose below)
    w = np.ascontiguousarray(w.transpose(0, 2, 1))  # weight[t,c,o]
    want = ref.grad_x_scatter(g, nbr, w, m)
    got = _conv(cuda, g, nbr, np.ascontiguousarray(w[::-1].transpose(0, 2, 1)), None)
    assert np.array_equal(got.astype(np.float64), want)


def _gamma(d):
    return d * 2.0 ** -24 / (1 - d * 2.0 ** -24)


def test_every_subset_of_gradients_against_float64_and_the_cpu_path(cuda, level):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    nbr, x, w, bias, g, m = (level[k] for k in ('nbr', 'x', 'w', 'bias', 'g', 'm'))
    cmap = _gpu_map(cuda, level)
    want_out, d, big_s = ref.sparse_conv(x, nbr, w, bias)
    want_gx, dx, sx = ref.sparse_conv(g, nbr, np.ascontiguousarray(w[::-1].transpose(0, 2, 1)))
    np.testing.assert_allclose(want_gx, ref.grad_x_scatter(g, nbr, w, m), rtol=1e-12, atol=1e-12)
    want_gw, want_gb = ref.grad_weight_bias(x, g, nbr)
    sw, sb = ref.grad_weight_bias(np.abs(x), np.abs(g), nbr)
    # grad_weight and grad_bias are sums of at most B * m rounded products / terms in an order torch chooses
    bar_w, bar_b = _gamma(3 * m + 1) * sw, _gamma(3 * m + 1) * sb
    cpu_map = ops.SparseConvMap(torch.from_numpy(nbr), torch.zeros(3, dtype=torch.int32), 3, 1)
    tx, tw, tb = (torch.from_numpy(a).requires_grad_(True) for a in (x, w, bias))
    cpu_out = ops.sparse_conv(tx, cpu_map, tw, tb)
    cpu_out.backward(torch.from_numpy(g))
    assert ref.share(cpu_out.detach().numpy(), want_out, d, big_s) <= 1.0 and ref.share(tx.grad.numpy(), want_gx, dx, sx) <= 1.0
    assert (np.abs(tw.grad.numpy() - want_gw) <= bar_w).all() and (np.abs(tb.grad.numpy() - want_gb) <= bar_b).all()
    for needs in itertools.product((False, True), repeat=3):
        out, gx, gw, gb = _run(cuda, level, cmap, needs=needs)
        assert [t is not None for t in (gx, gw, gb)] == list(needs)
        print(f'{needs}: out at {ref.share(out, want_out, d, big_s):.3f} of the bar')
        assert ref.share(out, want_out, d, big_s) <= 1.0
        if needs[0]:
            print(f'  grad_x at {ref.share(gx, want_gx, dx, sx):.3f} of the bar')
            assert ref.share(gx, want_gx, dx, sx) <= 1.0
        if needs[1]:
            assert (np.abs(gw - want_gw) <= bar_w).all()
        if needs[2]:
            assert (np.abs(gb - want_gb) <= bar_b).all()
    assert _run(cuda, level, cmap, needs=(True, True, True), with_bias=False)[3] is None


def test_one_level_end_to_end_on_both_devices_and_against_conv3d(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    torch.manual_seed(11)
    res, b, n = 8, 2, 500
    xyz = torch.rand(b, n, 3) - 0.5
    for ksize, dil, c, o in ((3, 1, 7, 9), (5, 2, 16, 32)):  # (the VALU kernel, the MFMA kernel)
        feats = torch.randn(b, c, n)
        conv = ops.SubmanifoldConv3d(c, o, ksize, dil)
        outs = []
        for dev in (torch.device('cpu'), cuda):
            net, p, f = conv.to(dev), xyz.to(dev), feats.to(dev)
            pooled = ops.grid_pool(p, f, res, reduce='mean')
            cmap = ops.cell_neighbours(ops.voxel_index(p, res), pooled.index, ksize, dil)
            y = net(pooled.features, cmap)
            outs.append((pooled, cmap, y.detach().cpu(), ops.grid_unpool(y, pooled.index).detach().cpu()))
        (pooled, cmap, y_cpu, back_cpu), (gpooled, gmap, y_gpu, back_gpu) = outs
        assert torch.equal(cmap.nbr, gmap.nbr.cpu()) and torch.equal(pooled.features, gpooled.features.cpu())
        conv = conv.to('cpu')
        want, d, big_s = ref.sparse_conv(pooled.features.numpy(), cmap.nbr.numpy(), conv.weight.detach().numpy(), conv.bias.detach().numpy())
        assert ref.share(y_cpu.numpy(), want, d, big_s) <= 1.0 and ref.share(y_gpu.numpy(), want, d, big_s) <= 1.0
        # torch.nn.Conv3d holding the permuted weight, in float64 on the dense grid of cell means, read back at the points
        dense_conv = torch.nn.Conv3d(c, o, ksize, padding=(ksize - 1) // 2 * dil, dilation=dil).double()
        with torch.no_grad():
            dense_conv.weight.copy_(conv.weight.view(ksize, ksize, ksize, c, o).permute(4, 3, 0, 1, 2))
            dense_conv.bias.copy_(conv.bias)
            vindex = ops.voxel_index(xyz, res)
            dense = dense_conv(ops.voxelize(feats, vindex).double()).view(b, o, -1)
            at_points = torch.gather(dense, 2, vindex.cell.long()[:, None, :].expand(b, o, n))
        slot = pooled.index.cluster.long()
        for back in (back_cpu, back_gpu):
            for s in range(b):  # every point reads its slot: the slot's bar is the point's
                err = (back[s].double() - at_points[s]).abs().numpy()
                assert (err <= ref.bar(d, big_s)[s][:, slot[s].numpy()] + 1e-12 * np.abs(at_points[s].numpy())).all()
