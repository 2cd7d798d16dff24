"""The ragged kernel map without a device: tests/cell_ragged_reference.py against closed forms, the CPU path
(``torch_cell_neighbours_ragged`` through ``neighbour_ops.cell_neighbours_ragged``) word for word against that reference on every
input the accelerator tests use, the properties of the contract (centre tap, symmetry, the capacity rule), every refusal of the C
entry point and of the Python layer, and one level of a scene backbone end to end on CPU tensors against the dense float64
``conv3d``."""

import ctypes

import numpy as np
import pytest
import torch

from tests import cell_ragged_reference as C
from tests import unaligned_views as U
from tests import unaligned_views_cell_ragged as V  # (registers the entry point's case before the registry suites read it)


def _ops():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    return ops


@pytest.fixture(autouse=True)
def the_op_exists():
    """Every test of this file is about ``cell_neighbours_ragged``, the reference's own included: without the op none of them passes."""
    assert callable(_ops().cell_neighbours_ragged) and callable(_ops().sparse_conv_ragged)


def _cpu(rows, m, ksize, dilation, n_cells=None):
    """The CPU path's map of the first ``m`` rows at capacity ``m``, as numpy ``[m, K^3]``."""
    coord, u = C.padded(rows, m)
    count = torch.tensor([u if n_cells is None else n_cells], dtype=torch.int32)
    cmap = _ops().cell_neighbours_ragged(V._grid(torch.from_numpy(coord), count), ksize, dilation)
    assert cmap.nbr.shape == (1, m, ksize ** 3) and cmap.nbr.dtype == torch.int64 and cmap.count is count
    assert (cmap.kernel_size, cmap.dilation) == (ksize, dilation)
    return cmap.nbr[0].numpy()


# ---- the reference against closed forms ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ksize,dilation', [(3, 1), (5, 1), (3, 2)])
def test_reference_full_cube_is_the_analytic_rank_inside_and_empty_outside(ksize, dilation):
    side, h = 6, (ksize - 1) // 2
    rows, nbr = C.case('cube', ksize, dilation)
    assert len(rows) == side ** 3 and np.array_equal(rows[:, 1:], np.stack(np.unravel_index(np.arange(side ** 3), (side,) * 3), 1))
    for r in range(side ** 3):
        i, j, k = rows[r, 1:]
        for t in range(ksize ** 3):
            ti, tj, tk = i + dilation * (t // ksize ** 2 - h), j + dilation * (t // ksize % ksize - h), k + dilation * (t % ksize - h)
            inside = 0 <= ti < side and 0 <= tj < side and 0 <= tk < side
            assert nbr[r, t] == ((ti * side + tj) * side + tk if inside else -1)


def test_reference_a_line_along_each_axis():
    rows, nbr = C.case('lines', 3, 1)
    length = len(rows) // 3
    for axis in range(3):  # cloud `axis` holds the line along that axis: rank = axis * length + position
        step = 3 ** (2 - axis)
        for s in range(length):
            want = np.full(27, -1)
            want[13] = axis * length + s
            if s > 0:
                want[13 - step] = axis * length + s - 1
            if s < length - 1:
                want[13 + step] = axis * length + s + 1
            assert np.array_equal(nbr[axis * length + s], want)


def test_reference_no_tap_crosses_between_identical_clouds():
    one = C.scene(150, seed=2, clouds=1)
    two = one.copy()
    two[:, 0] = 1
    alone = C.cell_map(one, len(one), 5, 1)
    both = C.cell_map(np.concatenate([one, two]), 2 * len(one), 5, 1)
    assert np.array_equal(both[:150], alone) and np.array_equal(both[150:], np.where(alone >= 0, alone + 150, -1))


def test_reference_traps_do_not_wrap():
    rows, nbr = C.case('traps', 3, 1)
    rank = {tuple(int(v) for v in row): r for r, row in enumerate(rows)}
    T = C.TOP
    for a, b in [((0, 0, 0, T), (0, 0, 1, 0)), ((0, 0, T, 5), (0, 1, 0, 5)), ((0, T, T, T), (1, 0, 0, 0)), ((2, 0, 0, 0), (1, T, T, T))]:
        assert rank[b] not in nbr[rank[a]] and rank[a] not in nbr[rank[b]]
    origin = nbr[rank[(0, 0, 0, 0)]]  # every tap with a negative offset is outside; (0, 0, 1) and (0, 1, 1) are there
    assert all(origin[t] == -1 for t in range(27) if min(t // 9, t // 3 % 3, t % 3) == 0)
    assert origin[14] == rank[(0, 0, 0, 1)] and origin[17] == rank[(0, 0, 1, 1)] and origin[22] == rank[(0, 1, 0, 0)]
    far = C.case('traps', 3, 65535)[1]
    assert far[rank[(3, 0, 0, 0)], 26] == rank[(3, T, T, T)] and far[rank[(3, T, T, T)], 0] == rank[(3, 0, 0, 0)]
    for d in (65536, 2 ** 20):  # nothing but the centre
        only = C.case('traps', 3, d)[1]
        assert np.array_equal(only[:, 13], np.arange(len(rows))) and (np.delete(only, 13, 1) == -1).all()


# ---- the CPU path against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name,ksize,dilation', C.GRID, ids=[f'{n}-K{k}-d{d}' for n, k, d in C.GRID])
def test_cpu_path_word_for_word(name, ksize, dilation):
    rows, want = C.case(name, ksize, dilation)
    got = _cpu(rows, max(len(rows), 1), ksize, dilation)
    assert U.same_words(got, want)
    C.check_properties(got, len(rows), ksize)


@pytest.mark.parametrize('name', ['u257', 'traps', 'batch37', 'empties'])
@pytest.mark.parametrize('ksize,dilation', [(3, 1), (5, 2)])
def test_capacities_are_the_cut_full_map(name, ksize, dilation):
    rows, full = C.case(name, ksize, dilation)
    u, n = len(rows), len(rows) + 40
    for m in C.capacities(u, n):
        want = C.cut(full, m)
        coord, _ = C.padded(rows, m)
        assert np.array_equal(C.cell_map(coord, u, ksize, dilation), want)
        got = _cpu(rows, m, ksize, dilation)
        assert U.same_words(got, want)
        C.check_properties(got, min(u, m), ksize)


@pytest.mark.parametrize('n_cells', [-5, -2 ** 31, 0, 300, 2 ** 31 - 1])
def test_garbage_count_is_clipped(n_cells):
    rows = C.rows_of('u257')
    kept = min(max(n_cells, 0), 257)
    coord, _ = C.padded(rows, 257)
    assert U.same_words(_cpu(rows, 257, 3, 1, n_cells), C.cell_map(coord, kept, 3, 1))


def test_unpadded_and_padded_grids_of_the_pipeline():
    """``m=None`` and a padded level of ``grid_cluster_ragged`` give the same map up to the padding, the reference's."""
    ops = _ops()
    i = C.e2e_inputs()
    args = (torch.from_numpy(i['xyz']), torch.from_numpy(i['offset']), C.E2E['size'], torch.from_numpy(i['start']))
    tight = ops.grid_cluster_ragged(*args, axis_bits=C.E2E['axis_bits'])
    loose = ops.grid_cluster_ragged(*args, m=len(i['xyz']), axis_bits=C.E2E['axis_bits'])
    u = int(tight.count)
    want = C.cell_map(tight.coord.numpy(), u, 3, 1)
    a, b = ops.cell_neighbours_ragged(tight), ops.cell_neighbours_ragged(loose, 3, 1)
    assert a.nbr.shape == (1, u, 27) and b.nbr.shape == (1, len(i['xyz']), 27) and a.count is tight.count
    assert U.same_words(a.nbr[0], want) and U.same_words(b.nbr[0], C.cut(want, len(i['xyz'])))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_c_abi_refusals():
    """PCC_EINVAL under the entry point's name before anything is enqueued: no stream, no device memory is touched."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)

    def run(m=4, ksize=3, dilation=1, null=None):
        q = [p, p, p]  # coord n_cells | nbr
        if null is not None:
            q[null] = None
        return L.pcc_cell_neighbours_ragged(m, ksize, dilation, *q, None)

    bad = [dict(m=0), dict(m=-1), dict(ksize=1), dict(ksize=4), dict(ksize=7), dict(ksize=-3), dict(dilation=0), dict(dilation=-1),
           dict(m=(2 ** 31 + 26) // 27), dict(m=(2 ** 31 + 124) // 125, ksize=5), dict(m=2 ** 31 - 1)]
    bad += [dict(null=k) for k in range(3)]
    for kw in bad:
        assert run(**kw) == -22, kw
        assert L.pcc_last_error().decode().startswith('cell_neighbours_ragged:') and L.pcc_last_status() == -22, kw
    assert run(m=(2 ** 31 + 26) // 27) == -22 and '2^31' in L.pcc_last_error().decode()
    assert run(null=1) == -22 and 'null pointer' in L.pcc_last_error().decode()


def test_python_refusals():
    ops = _ops()
    coord, count = torch.zeros((6, 4), dtype=torch.int32), torch.tensor([1], dtype=torch.int32)
    grid = V._grid(coord, count)
    for what, args in [('not a grid', (coord,)), ('a grid index', (grid.index,)), ('kernel 4', (grid, 4)), ('kernel bool', (grid, True)),
                       ('kernel float', (grid, 3.0)), ('dilation 0', (grid, 3, 0)), ('dilation float', (grid, 3, 1.5)), ('dilation bool', (grid, 3, True)),
                       ('coord shape', (V._grid(torch.zeros((6, 3), dtype=torch.int32), count),)),
                       ('no slot', (V._grid(torch.zeros((0, 4), dtype=torch.int32), count),)),
                       ('count shape', (V._grid(coord, torch.zeros(2, dtype=torch.int32)),))]:
        with pytest.raises(ValueError, match='cell_neighbours_ragged'):
            ops.cell_neighbours_ragged(*args)
    for what, args in [('coord dtype', (V._grid(coord.long(), count),)), ('count dtype', (V._grid(coord, count.long()),))]:
        with pytest.raises(RuntimeError, match='must be torch.int32'):
            ops.cell_neighbours_ragged(*args)
    huge = torch.zeros(1, dtype=torch.int32).expand((2 ** 31 + 124) // 125, 4)  # (no memory behind it)
    with pytest.raises(ValueError, match='too large'):
        ops.cell_neighbours_ragged(V._grid(huge, count), 5)
    cmap = ops.cell_neighbours_ragged(grid)
    w = torch.zeros(27, 2, 3)
    for feats, m in ((torch.zeros(1, 2, 6), cmap), (torch.zeros(6), cmap), (torch.zeros(6, 2), cmap.nbr),
                     (torch.zeros(6, 2), cmap._replace(nbr=cmap.nbr[0])), (torch.zeros(5, 2), cmap), (torch.zeros(6, 3), cmap)):
        with pytest.raises(ValueError, match='sparse_conv'):
            ops.sparse_conv_ragged(feats, m, w)


def test_the_registry_of_unaligned_views_holds_the_entry_point():
    names = [case.name for case in U.CASES]
    assert names.count('cell_neighbours_ragged') == 1 and 'pcc_cell_neighbours_ragged' in U.covered()
    case = U.CASES[names.index('cell_neighbours_ragged')]
    assert case.dims['b'] == 2 and max(case.dims.values()) <= 512 and case.anchor is not None and case.cpu


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------

def run_level(dev, ksize, dilation, seed=3):
    """One level of a scene backbone on ``dev``: ``grid_pool_ragged -> cell_neighbours_ragged -> SubmanifoldConv3d ->
    grid_unpool_ragged`` on two clouds of unequal size.  The pooled features are the leaf the convolution's gradient is taken
    at.  Returns what the comparison needs, as numpy."""
    ops = _ops()
    i = C.e2e_inputs(seed)
    to = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    torch.manual_seed(seed)
    conv = ops.SubmanifoldConv3d(C.E2E['c'], C.E2E['o'], ksize, dilation)
    with torch.no_grad():  # (make the bias count against the products)
        conv.bias.mul_(8.0)
    conv = conv.to(dev)
    pooled = ops.grid_pool_ragged(to(i['xyz']), to(i['features']), to(i['offset']), C.E2E['size'], 'mean', start=to(i['start']),
                                  axis_bits=C.E2E['axis_bits'])
    x = pooled.features.detach().clone().requires_grad_(True)
    cmap = ops.cell_neighbours_ragged(pooled.grid, ksize, dilation)
    y = conv(x.t()[None], cmap)
    back = ops.grid_unpool_ragged(y[0].t(), pooled.grid)
    (back * to(i['grad'])).sum().backward()
    cluster = pooled.grid.index.cluster[0].long().cpu().numpy()
    assert (cluster >= 0).all() and back.shape == (len(cluster), C.E2E['o'])
    grad_y = np.zeros((x.shape[0], C.E2E['o']), np.float64)
    np.add.at(grad_y, cluster, i['grad'].astype(np.float64))  # small integers: exact in float32 too
    return {'coord': pooled.grid.coord.cpu().numpy(), 'x': x.detach().cpu().numpy(), 'nbr': cmap.nbr[0].cpu().numpy(), 'cluster': cluster,
            'weight': conv.weight.detach().cpu().numpy(), 'bias': conv.bias.detach().cpu().numpy(), 'grad_y': grad_y.astype(np.float32),
            'back': back.detach().cpu().numpy(), 'grad_x': x.grad.cpu().numpy(), 'grad_weight': conv.weight.grad.cpu().numpy(),
            'grad_bias': conv.bias.grad.cpu().numpy()}


def check_level(got, ksize, dilation, scale=1.0):
    """``run_level``'s result against the dense float64 reference inside ``scale`` times the contract's bars: the figures are printed
    before they are asserted."""
    want_nbr = C.cell_map(got['coord'], len(got['coord']), ksize, dilation)
    assert U.same_words(got['nbr'], want_nbr)
    ref = C.dense_conv_reference(got['coord'], got['x'], got['grad_y'], got['weight'], got['bias'], want_nbr, ksize, dilation)
    worst = {}
    for name in ('out', 'grad_x', 'grad_weight', 'grad_bias'):
        value, bound = ref[name]
        mine = got['back'] if name == 'out' else got[name]
        if name == 'out':  # the unpooling is a gather: every point holds its slot's row
            value, bound = value[got['cluster']], bound[got['cluster']]
        worst[name] = float(np.max(np.abs(mine.astype(np.float64) - value) / bound))
        print(f'K={ksize} dilation={dilation} {name}: worst error / bar = {worst[name]:.3f}')
    assert all(v <= scale for v in worst.values()), worst
    return ref


@pytest.mark.parametrize('ksize,dilation', [(3, 1), (5, 1), (3, 2)])
def test_one_level_on_cpu_tensors_against_the_dense_float64_conv3d(ksize, dilation):
    got = run_level('cpu', ksize, dilation)
    assert len(got['coord']) > 4 * C.SLOTS and (np.bincount(got['coord'][:, 0]) > 0).all()
    check_level(got, ksize, dilation)


def test_sparse_conv_ragged_is_sparse_conv_transposed():
    ops = _ops()
    rows = C.rows_of('u513')
    cmap = ops.cell_neighbours_ragged(V._grid(torch.from_numpy(rows), torch.tensor([513], dtype=torch.int32)))
    g = torch.Generator().manual_seed(4)
    x, w, b = (torch.randn(s, generator=g).requires_grad_(True) for s in ((513, 3), (27, 3, 2), (2,)))
    out = ops.sparse_conv_ragged(x, cmap, w, b)
    out.backward(torch.ones_like(out))
    x2, w2, b2 = (t.detach().clone().requires_grad_(True) for t in (x, w, b))
    want = ops.sparse_conv(x2.t()[None], cmap, w2, b2)
    want.backward(torch.ones_like(want))
    assert out.shape == (513, 2) and U.same_words(out.detach().contiguous(), want[0].t().detach().contiguous())
    assert U.same_words(x.grad, x2.grad) and U.same_words(w.grad, w2.grad) and U.same_words(b.grad, b2.grad)
