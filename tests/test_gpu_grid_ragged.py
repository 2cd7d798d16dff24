"""GPU tests of the ragged grid index (``pcc_grid_cluster_ragged``) and of ``grid_pool_ragged`` / ``grid_unpool_ragged`` on top of it.

The C entry point is called on guarded buffers prefilled with a sentinel (tests/unaligned_views.guarded: every word written, none
outside), and all six outputs are compared word for word with tests/grid_ragged_reference.py and with the CPU path.  The sort ranks
T = PCC_GRID_RAGGED_TILE = 2048 keys per workgroup, so n lies either side of a wave, of T and of two tiles; its table of 256 words
per tile and the run heads are scanned in blocks of 1024 words (more than one block from 5 tiles / 1025 points: ``multi_block``), and
the ONE workgroup that scans the block sums takes 256 of them per round: ``LOOP_N`` = 1025 tiles + 5 gives 257 and a second round.
The key is ``cloud_bits + 3 * axis_bits`` wide with both at least 1, so its narrowest form has 4 bits (the reference's WIDTHS): one
to eight passes at 4, 8, 9, 16, 17, 33 and 63 bits.

Garbage offsets run in guarded buffers inside a larger allocation and assert only in-range or -1 outputs: the kernel clips them,
and nothing here is built to fault."""

import numpy as np
import pytest
import torch

from tests import grid_ragged_reference as G
from tests import ragged_reference as R
from tests import unaligned_views as U
from tests import unaligned_views_grid_ragged  # noqa: F401  (registers the entry point's case before the registry suites read it)
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu


def _ops():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    return ops


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _call(cuda, xyz, offset, start, size, m, axis_bits):
    """``pcc_grid_cluster_ragged`` on device tensors, every output in a guarded buffer: the six outputs as numpy."""
    from pointcloudcounterfactual_amd import _lib

    n, b = xyz.shape[0], offset.shape[0]
    shapes = {'cluster': (n,), 'order': (n,), 'seg': (m + 1,), 'coord': (m, 4), 'new_offset': (b,), 'n_cells': (1,)}
    outs = {name: U.guarded(shapes[name], U.I32, cuda) for name in G.NAMES}
    _lib.call(_lib.lib.pcc_grid_cluster_ragged, 'grid_cluster_ragged', cuda, b, n, m, axis_bits, xyz.data_ptr(), offset.data_ptr(), start.data_ptr(),
              size, *(outs[name].ptr() for name in G.NAMES))
    torch.cuda.synchronize()
    return {name: g.numpy() for name, g in outs.items()}


def _gpu(cuda, i, m=None):
    n = len(i['xyz'])
    return _call(cuda, _dev(i['xyz'], cuda), _dev(i['offset'].astype(np.int32), cuda), _dev(i['start'], cuda), i['size'], n if m is None else m,
                 i['axis_bits'])


def _cpu(i, m=None):
    n = len(i['xyz'])
    got = _ops().torch_grid_cluster_ragged(torch.from_numpy(i['xyz']), torch.from_numpy(i['offset']), torch.from_numpy(i['start']), i['size'],
                                           n if m is None else m, i['axis_bits'])
    return dict(zip(G.NAMES, (t.numpy() for t in got)))


def _same(got, want):
    for name in G.NAMES:
        assert got[name].dtype == np.int32 and U.same_words(got[name], want[name]), name


def test_the_tile_is_the_documented_one():
    assert _ops().GRID_RAGGED_TILE == G.TILE == 2048


@pytest.mark.parametrize('name', list(G.CASES))
def test_every_output_word_for_word(cuda, name):
    """Against the reference and the CPU path; the call twice gives the same words; inside every run ``order`` ascends."""
    i, want = G.case(name)
    got = _gpu(cuda, i)
    _same(got, want)
    _same(got, _cpu(i))
    _same(_gpu(cuda, i), got)
    G.check_structure(got, len(i['xyz']), len(i['xyz']))


def test_block_sums_beyond_one_round_of_their_scan(cuda):
    i = G.uniform(G.LOOP_N)
    n = G.LOOP_N
    tiles = -(-n // G.TILE)
    assert -(-256 * tiles // 1024) > 256  # the table's scan has more block sums than the one workgroup takes per round
    want = G.grid_cluster(i['xyz'], i['offset'], i['start'], i['size'], n, i['axis_bits'])
    assert want['n_cells'][0] == 32 ** 3
    _same(_gpu(cuda, i), want)


@pytest.mark.parametrize('name', ['shapes', 'B37', 'bits9', 'bits63', 'non_finite', 'n4097'])
def test_capacities(cuda, name):
    i, full = G.case(name)
    n, u = len(i['xyz']), int(full['n_cells'][0])
    for m in G.capacities(u, n):
        got = _gpu(cuda, i, m)
        _same(got, G.cut(full, m))
        _same(got, _cpu(i, m))


def test_dropped_key_sorts_last_at_every_width(cuda):
    for bits in G.WIDTHS:
        i, want = G.case(f'bits{bits}')
        got = _gpu(cuda, i)
        dropped = np.nonzero(want['cluster'] < 0)[0]
        assert len(dropped) >= 2 and np.array_equal(got['order'][-len(dropped):], dropped)
        b = len(i['offset'])
        assert set(got['coord'][:int(got['n_cells'][0]), 0]) == {0, b // 2, b - 1}


def test_a_cloud_gives_the_same_relative_words_wherever_it_lies(cuda):
    x = R.cloud(71, 333, 'gauss')
    x[7, 1] = np.nan
    others = [R.cloud(73 + k, s, 'gauss') for k, s in enumerate((65, 2500, 0, 31))]
    base = None
    for place in (None, 0, 2, 4):
        parts = list(others) if place is not None else []
        at = place or 0
        parts.insert(at, x)
        xyz, offset = R.pack(parts)
        i = G._case(xyz, offset, G.starts(xyz, offset), 0.2, 9)
        got = _gpu(cuda, i)
        lo = int(offset[at - 1]) if at else 0
        r0 = int(got['new_offset'][at - 1]) if at else 0
        r1 = int(got['new_offset'][at])
        cluster = got['cluster'][lo:lo + len(x)]
        rel = [got['coord'][r0:r1, 1:], np.where(cluster >= 0, cluster - r0, -1), np.diff(got['seg'][r0:r1 + 1]),
               got['order'][got['seg'][r0]:got['seg'][r1]] - lo]
        assert (got['coord'][r0:r1, 0] == at).all()
        if base is None:
            base = rel
        assert all(np.array_equal(a, b) for a, b in zip(rel, base)), place


GARBAGE = [[50, 20, 10], [-5, -1, 30], [10, 10 ** 9, 2 * 10 ** 9], [10 ** 9, 3, -2], [0, 0, 0], [30, 60, 100], [2 ** 31 - 1, -2 ** 31, 5]]


@pytest.mark.parametrize('offset', GARBAGE)
def test_garbage_offsets_are_clipped(cuda, offset):
    """Decreasing, negative and too large offsets: every output word is written, none outside (guarded buffers), and every word is
    in range or -1.  The points sit inside a larger zero-filled allocation, so a row read outside ``xyz[0:n]`` is device memory
    of this test."""
    n, m, pad_rows = 100, 100, 4096
    big = torch.zeros((n + 2 * pad_rows, 3), dtype=torch.float32, device=cuda)
    big[pad_rows:pad_rows + n] = _dev(R.cloud(5, n, 'gauss') + 10.0, cuda)
    off = torch.zeros(3 + 2 * 1024, dtype=torch.int32, device=cuda)
    off[1024:1027] = torch.tensor(offset, dtype=torch.int64).to(torch.int32).to(cuda)
    start = torch.zeros((3 + 2 * 1024, 3), dtype=torch.float32, device=cuda)
    got = _call(cuda, big[pad_rows:pad_rows + n], off[1024:1027], start[1024:1027], 0.5, m, 8)
    u = int(got['n_cells'][0])
    assert 0 <= u <= n and np.array_equal(np.sort(got['order']), np.arange(n))
    assert ((got['cluster'] >= -1) & (got['cluster'] < max(u, 1))).all() and ((got['seg'] >= 0) & (got['seg'] <= n)).all()
    assert (np.diff(got['seg']) >= 0).all() and (np.diff(got['new_offset']) >= 0).all() and got['new_offset'][-1] == u
    assert ((got['coord'][:u, 0] >= 0) & (got['coord'][:u, 0] < 3)).all() and (got['coord'][:u, 1:] >= 0).all() and (got['coord'][u:] == -1).all()


def test_python_op_defaults_device_against_cpu(cuda):
    ops = _ops()
    i, _ = G.case('shapes')
    xyz, offset = i['xyz'][:i['offset'][-1]], i['offset']
    want = ops.grid_cluster_ragged(torch.from_numpy(xyz), torch.from_numpy(offset), 0.3)
    got = ops.grid_cluster_ragged(_dev(xyz, cuda), _dev(offset, cuda), 0.3)
    for a, b in zip(list(got.index) + list(got[1:]), list(want.index) + list(want[1:])):
        assert a.device == cuda and a.dtype == torch.int32 and torch.equal(a.cpu(), b)
    assert U.same_words(ops.ragged_grid_start(_dev(xyz, cuda), _dev(offset, cuda)), G.starts(xyz, offset))
    with pytest.raises(RuntimeError, match='offset must be a CUDA tensor'):
        ops.grid_cluster_ragged(_dev(xyz, cuda), torch.from_numpy(offset), 0.3)
    with pytest.raises(RuntimeError, match='start must be a CUDA tensor'):
        ops.grid_cluster_ragged(_dev(xyz, cuda), _dev(offset, cuda), 0.3, start=torch.zeros(len(offset), 3))


def _pool_case(kind):
    if kind == 'one_cell':  # a run of n: segment_pool's long-run kernel downstream
        i, _ = G.case('one_cell')
        return i, len(i['xyz'])
    n, m = kind  # either side of segment_pool's LDS limits
    rng = np.random.default_rng(n)
    xyz = (rng.random((n, 3)) * 8).astype(np.float32)
    return G._case(xyz, [n // 3, n], np.zeros((2, 3)), 0.25, 5), m


@pytest.mark.parametrize('kind', ['one_cell', (40000, 20000), (40001, 20001)], ids=['one_cell', 'lds', 'global'])
def test_grid_pool_ragged_device_against_cpu(cuda, kind):
    """Index words, pooled mean / sum / max and the gradients of the features and of ``xyz``, word for word: the sums run in
    ascending point index on both sides, and ``pcc_segment_pool_bwd`` is a gather.  The launch record of the device side
    proves the side of ``segment_pool``'s LDS limits the case names: rows of n points staged in LDS up to 40000 and gathered
    above, rows of m slots for the backward up to 20000 (tests/grid_pool_reference.py)."""
    from pointcloudcounterfactual_amd import _lib
    from tests import grid_pool_reference as pref
    from tests.which_ran import family

    ops = _ops()
    i, m = _pool_case(kind)
    n, c = len(i['xyz']), 3
    rng = np.random.default_rng(5)
    feats, w, v = rng.standard_normal((n, c)).astype(np.float32), rng.standard_normal((m, c)).astype(np.float32), rng.standard_normal((m, 3)).astype(np.float32)
    for reduce in ('mean', 'sum', 'max'):
        res = []
        for dev in ('cpu', cuda):
            to = (lambda a: torch.from_numpy(a)) if dev == 'cpu' else (lambda a: _dev(a, cuda))
            xyz, f = to(i['xyz']).requires_grad_(True), to(feats).requires_grad_(True)
            with _lib.profile() as read:  # (the CPU side records nothing)
                out = ops.grid_pool_ragged(xyz, f, to(i['offset']), i['size'], reduce, start=to(i['start']), m=m, axis_bits=i['axis_bits'])
                u = int(out.grid.count)
                assert kind == 'one_cell' or u >= m
                keep = min(u, m)
                ((out.features * to(w)).sum() + (out.xyz[:keep] * to(v)[:keep]).sum()).backward()
                pools = set(family(read.exact(), 'seg_')) if dev == cuda else None
            res.append([*out.grid.index, out.grid.coord, out.offset, out.xyz.detach(), out.features.detach(), f.grad, xyz.grad,
                        ops.grid_unpool_ragged(out.features.detach(), out.grid)])
        mode = pref.MODES[reduce]
        assert pools == pref.pool_kernels(n) | {pref.pool_bwd_kernel(m, pref.MEAN), pref.pool_bwd_kernel(m, mode)}, (kind, reduce, pools)
        for a, b in zip(*res):
            assert b.device == cuda and U.same_words(a, b), reduce
