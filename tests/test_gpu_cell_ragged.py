"""GPU tests of the ragged kernel map (``pcc_cell_neighbours_ragged``) and of the sparse convolution of a packed batch on top of it.

The C entry point is called with ``nbr`` in a guarded buffer prefilled with a sentinel (tests/unaligned_views.guarded: every word
written, none outside), and the map is compared word for word with tests/cell_ragged_reference.py and with the CPU path.  A thread
owns one (slot, di, dj) row of taps and a workgroup 256 consecutive rows -- 28.4 slots at K = 3, 10.24 at K = 5, so workgroup and
wave boundaries fall inside slots --, and the top 8 levels of the bisection come from a 255-node tree over [0, kept): the slot counts
lie either side of 64 and of 256 (the tree full and not) and reach 363 and 1008 workgroups.

The library's launch profile has no census entry for the two names of this kernel (tests/kernel_census.py lists ``..._kernel...``
names only), so every comparing test asserts itself, with tests/which_ran.ran_only, that ``cell_map_ragged<K>`` for its K, and not its
sibling, launched inside that very test.

Garbage ``coord`` runs in guarded buffers inside a larger allocation and asserts only in-range or -1 outputs: the input is legal under
the contract, its result is defined, and nothing here is built to fault."""

import numpy as np
import pytest
import torch

from tests import cell_ragged_reference as C
from tests import unaligned_views as U
from tests import unaligned_views_cell_ragged as V  # (registers the entry point's case before the registry suites read it)
from tests.test_cell_ragged_host import check_level, run_level
from tests.which_ran import ran_only

pytestmark = pytest.mark.gpu


def _ops():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    return ops


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _name(ksize):
    return f'cell_map_ragged<{ksize}>'


def _call(cuda, coord, n_cells, m, ksize, dilation):
    """``pcc_cell_neighbours_ragged`` on device tensors, ``nbr`` in a guarded buffer: ``nbr[m, K^3]`` as numpy.  Asserts that the
    kernel of this ``ksize`` and no sibling launched."""
    from pointcloudcounterfactual_amd import _lib

    out = U.guarded((m, ksize ** 3), U.I64, cuda)

    def run():
        _lib.call(_lib.lib.pcc_cell_neighbours_ragged, 'cell_neighbours_ragged', cuda, m, ksize, dilation, coord.data_ptr(), n_cells.data_ptr(), out.ptr())
        torch.cuda.synchronize()

    ran_only(run, _name(ksize), 'cell_map_ragged')
    return out.numpy()


def _gpu(cuda, rows, m, ksize, dilation, n_cells=None):
    coord, u = C.padded(rows, m)
    return _call(cuda, _dev(coord, cuda), _dev(np.array([u if n_cells is None else n_cells], np.int32), cuda), m, ksize, dilation)


def _cpu(rows, m, ksize, dilation, n_cells=None):
    coord, u = C.padded(rows, m)
    count = torch.tensor([u if n_cells is None else n_cells], dtype=torch.int32)
    return _ops().torch_cell_neighbours_ragged(torch.from_numpy(coord), count, ksize, dilation).numpy()


@pytest.mark.parametrize('name,ksize,dilation', C.GRID, ids=[f'{n}-K{k}-d{d}' for n, k, d in C.GRID])
def test_the_map_word_for_word(cuda, name, ksize, dilation):
    """Against the reference and the CPU path; the call twice gives the same words."""
    rows, want = C.case(name, ksize, dilation)
    m = max(len(rows), 1)
    got = _gpu(cuda, rows, m, ksize, dilation)
    assert got.dtype == np.int64 and U.same_words(got, want)
    assert U.same_words(got, _cpu(rows, m, ksize, dilation))
    assert U.same_words(_gpu(cuda, rows, m, ksize, dilation), got)
    C.check_properties(got, len(rows), ksize)


@pytest.mark.parametrize('name', ['u257', 'u513', 'traps', 'batch37', 'empties'])
@pytest.mark.parametrize('ksize,dilation', [(3, 1), (5, 2)])
def test_capacities(cuda, name, ksize, dilation):
    rows, full = C.case(name, ksize, dilation)
    u, n = len(rows), len(rows) + 300
    for m in C.capacities(u, n):
        got = _gpu(cuda, rows, m, ksize, dilation)
        assert U.same_words(got, C.cut(full, m)), m
        assert U.same_words(got, _cpu(rows, m, ksize, dilation)), m


@pytest.mark.parametrize('n_cells', [-5, -2 ** 31, 0, 300, 2 ** 31 - 1])
@pytest.mark.parametrize('ksize', [3, 5])
def test_garbage_count_is_clipped(cuda, n_cells, ksize):
    """``n_cells`` negative and above ``m``: kept = min(max(n_cells, 0), m), and the rows at or after it are never read."""
    rows = C.rows_of('u257')
    kept = min(max(n_cells, 0), 257)
    coord, _ = C.padded(rows, 257)
    got = _gpu(cuda, rows, 257, ksize, 1, n_cells)
    assert U.same_words(got, C.cell_map(coord, kept, ksize, 1)) and U.same_words(got, _cpu(rows, 257, ksize, 1, n_cells))


def test_traps_do_not_wrap(cuda):
    """The pairs a carry would join are in the input next to each other, and the kernel joins none of them."""
    rows = C.rows_of('traps')
    rank = {tuple(int(v) for v in row): r for r, row in enumerate(rows)}
    T = C.TOP
    for ksize in (3, 5):
        got = _gpu(cuda, rows, len(rows), ksize, 1)
        assert U.same_words(got, C.case('traps', ksize, 1)[1])
        for a, b in [((0, 0, 0, T), (0, 0, 1, 0)), ((0, 0, T, 5), (0, 1, 0, 5)), ((0, T, T, T), (1, 0, 0, 0)), ((2, 0, 0, 0), (1, T, T, T))]:
            assert rank[b] not in got[rank[a]] and rank[a] not in got[rank[b]]
        h = ksize // 2
        origin = got[rank[(0, 0, 0, 0)]]
        assert all(origin[t] == -1 for t in range(ksize ** 3) if min(t // ksize ** 2, t // ksize % ksize, t % ksize) < h)
    batch = C.rows_of('batch37')
    got = _gpu(cuda, batch, len(batch), 3, 1)
    last = np.nonzero(batch[:, 0] == 36)[0]
    assert U.same_words(got, C.case('batch37', 3, 1)[1]) and (got[last][got[last] >= 0] >= last[0]).all()


def test_a_cloud_gives_the_same_relative_rows_wherever_it_lies(cuda):
    base = {}
    for where in (None, 0, 2, 4):
        rows, c = C.placed(where)
        for ksize, dilation in ((3, 1), (5, 2)):
            got = _gpu(cuda, rows, len(rows), ksize, dilation)
            assert U.same_words(got, C.cell_map(rows, len(rows), ksize, dilation))
            mine = np.nonzero(rows[:, 0] == c)[0]
            assert len(mine) == 300 and np.array_equal(mine, np.arange(mine[0], mine[0] + 300))
            rel = np.where(got[mine] >= 0, got[mine] - mine[0], -1)
            if where is None:
                base[ksize] = rel
            assert np.array_equal(rel, base[ksize]), where


@pytest.mark.parametrize('ksize,dilation', [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_against_the_rectangular_map(cuda, ksize, dilation):
    """A rectangular batch through ``voxel_index -> grid_cluster -> cell_neighbours``, its slots packed into ``coord``: the ragged
    map is ``pcc_cell_neighbours``' ranks plus the cloud's first packed rank, word for word."""
    ops = _ops()
    b, n, res = 3, 1500, 16
    xyz = torch.from_numpy(np.random.default_rng(9).random((b, n, 3)).astype(np.float32) - 0.5).to(cuda)
    index = ops.voxel_index(xyz, res)
    gindex = ops.grid_cluster(index, m=n)
    rect = ops.cell_neighbours(index, gindex, ksize, dilation).nbr.cpu().numpy()
    cell, order, seg, count = (t.cpu().numpy().astype(np.int64) for t in (index.cell, gindex.order, gindex.seg, gindex.count))
    rows, want = [], []
    first = 0
    for s in range(b):
        u = int(count[s])
        assert 600 < u < n
        flat = cell[s, order[s, seg[s, :u]]]
        rows.append(np.stack([np.full(u, s), flat // (res * res), flat // res % res, flat % res], 1))
        want.append(np.where(rect[s, :u] >= 0, rect[s, :u] + first, -1))
        first += u
    rows = np.concatenate(rows).astype(np.int32)
    assert np.array_equal(rows, C.sort_rows(rows))
    got = _gpu(cuda, rows, len(rows), ksize, dilation)
    assert U.same_words(got, np.concatenate(want))


@pytest.mark.parametrize('kind', ['int32', 'small', 'fields'])
@pytest.mark.parametrize('ksize', [3, 5])
def test_garbage_coord_gives_words_in_range(cuda, kind, ksize):
    """Random rows -- any int32, a few values with many repeats, components inside their fields --, unsorted: every word of
    ``nbr`` is written, none outside (guarded buffer), and every word is in [-1, kept).  The rows sit inside a larger
    zero-filled allocation, so a row read outside ``coord[0:m]`` would be device memory of this test."""
    m, pad_rows = 1000, 4096
    rng = np.random.default_rng(ksize)
    rows = {'int32': lambda: rng.integers(-2 ** 31, 2 ** 31, (m, 4)), 'small': lambda: rng.integers(-1, 3, (m, 4)),
            'fields': lambda: rng.integers(0, 65536, (m, 4))}[kind]().astype(np.int32)
    big = torch.zeros((m + 2 * pad_rows, 4), dtype=torch.int32, device=cuda)
    big[pad_rows:pad_rows + m] = _dev(rows, cuda)
    for n_cells, dilation in ((m, 1), (m - 7, 3), (2 ** 31 - 1, 65536)):
        kept = min(n_cells, m)
        count = torch.tensor([n_cells], dtype=torch.int32, device=cuda)
        got = _call(cuda, big[pad_rows:pad_rows + m], count, m, ksize, dilation)
        assert ((got >= -1) & (got < kept)).all() and (got[kept:] == -1).all()
        assert U.same_words(_call(cuda, big[pad_rows:pad_rows + m], count, m, ksize, dilation), got)


def test_python_op_on_the_device(cuda):
    ops = _ops()
    rows = C.rows_of('u513')
    coord, count = _dev(rows, cuda), torch.tensor([513], dtype=torch.int32, device=cuda)
    cmap = ran_only(lambda: ops.cell_neighbours_ragged(V._grid(coord, count), 5, 2), _name(5), 'cell_map_ragged')
    assert cmap.nbr.device == cuda and cmap.nbr.dtype == torch.int64 and cmap.count is count and (cmap.kernel_size, cmap.dilation) == (5, 2)
    assert U.same_words(cmap.nbr[0], C.cell_map(rows, 513, 5, 2))
    with pytest.raises(RuntimeError, match='grid.count must be a CUDA tensor'):
        ops.cell_neighbours_ragged(V._grid(coord, count.cpu()))
    # the other consumers of a list take it unchanged
    nbr = ran_only(lambda: ops.cell_neighbours_ragged(V._grid(coord, count)), _name(3), 'cell_map_ragged').nbr
    feats = torch.randn(1, 3, 513, device=cuda)
    grouped = ops.group_points(feats, nbr)
    assert grouped.shape == (1, 3, 513, 27)
    want = torch.where(nbr[:, None] >= 0, feats[0][:, nbr[0].clamp(min=0)][None], torch.zeros((), device=cuda))
    assert torch.equal(grouped, want)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ksize,dilation', [(3, 1), (5, 1), (3, 2)])
def test_one_level_on_the_device_against_the_dense_float64_conv3d(cuda, ksize, dilation):
    """``grid_pool_ragged -> cell_neighbours_ragged -> SubmanifoldConv3d -> grid_unpool_ragged`` on two clouds of unequal size whose
    level spans several workgroups of the map, inside the bars of ``pcc_sparse_conv``'s contract."""
    got = ran_only(lambda: run_level(cuda, ksize, dilation), _name(ksize), 'cell_map_ragged')
    assert len(got['coord']) > 4 * C.SLOTS
    check_level(got, ksize, dilation)


def test_sparse_conv_ragged_device_against_cpu(cuda):
    """Point-major in and out, forward and the three gradients: both sides lie inside the bar against exact arithmetic, so they
    differ by twice the bar at the most."""
    ops = _ops()
    ksize, dilation = 3, 1
    level = run_level('cpu', ksize, dilation, seed=5)
    ref = check_level(level, ksize, dilation)
    res = {}
    for dev in ('cpu', cuda):
        def run(dev=dev):
            to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
            coord = to(level['coord'])
            cmap = ops.cell_neighbours_ragged(V._grid(coord, torch.tensor([len(coord)], dtype=torch.int32, device=dev)), ksize, dilation)
            x, w, b = (to(level[k]).requires_grad_(True) for k in ('x', 'weight', 'bias'))
            out = ops.sparse_conv_ragged(x, cmap, w, b)
            assert out.shape == (len(coord), C.E2E['o']) and out.device == torch.device(dev)
            out.backward(to(level['grad_y']))
            return {'out': out.detach().cpu().numpy(), 'grad_x': x.grad.cpu().numpy(), 'grad_weight': w.grad.cpu().numpy(), 'grad_bias': b.grad.cpu().numpy()}
        res[dev] = ran_only(run, _name(ksize), 'cell_map_ragged') if dev == cuda else run()
    for name, (value, bound) in ref.items():
        a, b = res['cpu'][name].astype(np.float64), res[cuda][name].astype(np.float64)
        worst = float(np.max(np.abs(a - b) / bound))
        print(f'{name}: worst |device - cpu| / bar = {worst:.3f}; device against float64 {float(np.max(np.abs(b - value) / bound)):.3f}')
        assert worst <= 2.0, name
