"""The ragged grid index without a device: tests/grid_ragged_reference.py against closed forms, the CPU path
(``torch_grid_cluster_ragged`` through ``neighbour_ops.grid_cluster_ragged``) word for word against that reference on every input the
accelerator tests use (all but the two-million-point one, which only sizes the kernel's scan), ``grid_pool_ragged`` /
``grid_unpool_ragged`` against a float64 loop per slot and against ``segment_pool``, the composition with ``knn_ragged``, and every
refusal of the C entry point and of the Python layer."""

import ctypes

import numpy as np
import pytest
import torch

from tests import grid_ragged_reference as G
from tests import ragged_reference as R
from tests import unaligned_views as U
from tests import unaligned_views_grid_ragged  # noqa: F401  (registers the entry point's case before the registry suites read it)


def _ops():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    return ops


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _cpu(i, m=None):
    """The six outputs of the CPU path as numpy, at capacity ``m`` (None: n)."""
    n = len(i['xyz'])
    grid = _ops().grid_cluster_ragged(_t(i['xyz']), _t(i['offset']), i['size'], _t(i['start']), n if m is None else m, i['axis_bits'])
    idx = grid.index
    assert idx.cluster.shape == idx.order.shape == (1, n) and idx.count is grid.count and all(t.dtype == torch.int32 for t in idx)
    return {'cluster': idx.cluster[0].numpy(), 'order': idx.order[0].numpy(), 'seg': idx.seg[0].numpy(), 'coord': grid.coord.numpy(),
            'new_offset': grid.offset.numpy(), 'n_cells': grid.count.numpy()}


def _same(got, want):
    for name in G.NAMES:
        assert got[name].dtype == np.int32 and U.same_words(got[name], want[name]), name


# ---- the reference against closed forms ---------------------------------------------------------------------------------------------

def test_reference_full_lattice_gives_one_slot_per_point_in_lexicographic_order():
    side = 5
    i = G.lattice(side, shuffle=False)
    out = G.grid_cluster(i['xyz'], i['offset'], i['start'], 1.0, side ** 3, 3)
    n = side ** 3
    assert out['n_cells'][0] == n and np.array_equal(out['cluster'], np.arange(n)) and np.array_equal(out['order'], np.arange(n))
    assert np.array_equal(out['seg'], np.arange(n + 1)) and np.array_equal(out['new_offset'], [n])
    assert np.array_equal(out['coord'][:, 1:], i['xyz'].astype(np.int32)) and (out['coord'][:, 0] == 0).all()
    shuffled, _ = G.case('own_cell')
    full = G.case('own_cell')[1]
    assert np.array_equal(shuffled['xyz'][full['order']].astype(np.int32), full['coord'][:, 1:])  # sorted back into lexicographic order


def test_reference_all_points_in_one_cell():
    i, out = G.case('one_cell')
    n = len(i['xyz'])
    assert out['n_cells'][0] == 1 and (out['cluster'] == 0).all() and np.array_equal(out['order'], np.arange(n))
    assert out['seg'][0] == 0 and (out['seg'][1:] == n).all() and np.array_equal(out['coord'][0], [0, 0, 0, 0]) and (out['coord'][1:] == -1).all()


def test_reference_identical_clouds_give_identical_relative_outputs():
    x = R.cloud(3, 200, 'gauss')
    xyz, offset = R.pack([x, x])
    start = G.starts(xyz, offset)
    out = G.grid_cluster(xyz, offset, start, 0.3, 400, 8)
    u = int(out['new_offset'][0])
    assert out['n_cells'][0] == 2 * u and np.array_equal(out['coord'][:u, 1:], out['coord'][u:2 * u, 1:])
    assert np.array_equal(out['cluster'][:200], out['cluster'][200:] - u)
    assert np.array_equal(np.diff(out['seg'][:u + 1]), np.diff(out['seg'][u:2 * u + 1]))
    assert np.array_equal(out['order'][:out['seg'][u]] + 200, out['order'][out['seg'][u]:out['seg'][2 * u]])


def test_reference_dyadic_boundary_lands_in_q_and_one_ulp_below_in_q_minus_one():
    size, start = np.float32(0.125), np.float32(1.5)
    qs = np.arange(1, 60)
    at = (start + qs * size).astype(np.float32)
    below = np.nextafter(at, np.float32(-np.inf))
    xyz = np.zeros((2 * len(qs), 3), np.float32) + start
    xyz[:, 0] = np.concatenate([at, below])
    _, q, valid = G.cells(xyz, [len(xyz)], np.full((1, 3), start), size, 8)
    assert valid.all() and np.array_equal(q[:len(qs), 0], qs) and np.array_equal(q[len(qs):, 0], qs - 1)


# ---- the CPU path against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(G.CASES))
def test_cpu_path_word_for_word(name):
    i, want = G.case(name)
    G.check_structure(want, len(i['xyz']), len(i['xyz']))
    _same(_cpu(i), want)


def test_non_finite_case_drops_what_the_contract_says():
    i, want = G.case('non_finite')
    dropped = [0, 1, 2, 98, 99, 100, 169, 110, 111, 112] + list(range(300, 350))
    assert (want['cluster'][dropped] == -1).all() and want['cluster'][113] >= 0 and (want['cluster'] == -1).sum() == len(dropped)
    assert np.array_equal(want['order'][-len(dropped):], sorted(dropped))
    assert want['new_offset'][3] == want['new_offset'][2] == want['n_cells'][0]


def test_boundary_cases_tell_a_reciprocal_multiply_from_the_division():
    """The probes do probe: on each non-dyadic size a reciprocal multiply puts some point in another cell."""
    for k in range(len(G.NONDYADIC)):
        i, _ = G.case(f'boundary{k}')
        s32 = np.float32(i['size'])
        x = i['xyz'][:, 0]
        assert (np.floor(x / s32) != np.floor(x * (np.float32(1) / s32))).any()


@pytest.mark.parametrize('name', ['shapes', 'B37', 'bits9', 'non_finite'])
def test_capacities_are_the_cut_capacity_n_result(name):
    i, full = G.case(name)
    n, u = len(i['xyz']), int(full['n_cells'][0])
    for m in G.capacities(u, n):
        want = G.cut(full, m)
        _same(G.grid_cluster(i['xyz'], i['offset'], i['start'], i['size'], m, i['axis_bits']), want)
        _same(_cpu(i, m), want)
        G.check_structure(want, n, m)


def test_defaults_start_axis_bits_and_the_unpadded_form():
    ops = _ops()
    i, _ = G.case('shapes')
    xyz, offset = i['xyz'][:i['offset'][-1]], i['offset']
    start = ops.ragged_grid_start(_t(xyz), _t(offset))
    want_start = G.starts(xyz, offset)
    assert U.same_words(start, want_start)
    assert [ops.default_axis_bits(b) for b in (1, 2, 37, 16383, 16384, 32767, 32768, 65535)] == [16, 16, 16, 16, 16, 16, 15, 15]
    grid = ops.grid_cluster_ragged(_t(xyz), _t(offset), 0.3)
    want = G.grid_cluster(xyz, offset, want_start, 0.3, len(xyz), 16)
    u = int(want['n_cells'][0])
    assert grid.index.seg.shape == (1, u + 1) and grid.coord.shape == (u, 4) and (grid.coord.numpy() >= 0).all()
    _same({'cluster': grid.index.cluster[0].numpy(), 'order': grid.index.order[0].numpy(), 'seg': grid.index.seg[0].numpy(),
           'coord': grid.coord.numpy(), 'new_offset': grid.offset.numpy(), 'n_cells': grid.count.numpy()}, G.cut(want, u))


# ---- pooling ------------------------------------------------------------------------------------------------------------------------------

def _pool_inputs():
    i, _ = G.case('shapes')
    rng = np.random.default_rng(12)
    return i, rng.standard_normal((len(i['xyz']), 5)).astype(np.float32)


@pytest.mark.parametrize('m', [None, 40, 2500])
@pytest.mark.parametrize('reduce', ['mean', 'sum', 'max'])
def test_grid_pool_ragged_against_a_float64_loop_and_segment_pool(reduce, m):
    ops = _ops()
    i, feats = _pool_inputs()
    xyz, f = _t(i['xyz']).requires_grad_(True), _t(feats).requires_grad_(True)
    out = ops.grid_pool_ragged(xyz, f, _t(i['offset']), i['size'], reduce, start=_t(i['start']), m=m, axis_bits=i['axis_bits'])
    n = len(feats)
    want = G.grid_cluster(i['xyz'], i['offset'], i['start'], i['size'], n, i['axis_bits'])
    u = int(want['n_cells'][0])
    cap = u if m is None else m
    want = G.cut(want, cap)
    assert out.xyz.shape == (cap, 3) and out.features.shape == (cap, 5) and out.offset is out.grid.offset
    _same({'cluster': out.grid.index.cluster[0].numpy(), 'order': out.grid.index.order[0].numpy(), 'seg': out.grid.index.seg[0].numpy(),
           'coord': out.grid.coord.numpy(), 'new_offset': out.offset.numpy(), 'n_cells': out.grid.count.numpy()}, want)
    # word for word segment_pool on the same index (channels-major, b = 1)
    direct = ops.segment_pool(_t(feats).t()[None].contiguous(), out.grid.index, reduce)
    assert U.same_words(out.features.detach(), direct[0].t().contiguous())
    centres = ops.segment_pool(_t(i['xyz']).t()[None].contiguous(), out.grid.index, 'mean')[0].t()
    kept = min(u, cap)
    assert U.same_words(out.xyz.detach()[:kept], centres[:kept].contiguous())
    assert (U.words(out.xyz.detach()[kept:]) == 0x7fc00000).all() and not U.words(out.features.detach()[kept:]).any()
    # the float64 loop: forward, and the gradients of sum(w * features) + sum(v * centres)
    rng = np.random.default_rng(13)
    w, v = rng.standard_normal((cap, 5)), rng.standard_normal((cap, 3))
    (out.features * _t(w)).sum().add((out.xyz[:kept] * _t(v[:kept])).sum()).backward()
    order, seg = want['order'].astype(np.int64), want['seg'].astype(np.int64)
    gf, gx = np.zeros((n, 5)), np.zeros((n, 3))
    f64, x64 = feats.astype(np.float64), i['xyz'].astype(np.float64)
    for r in range(kept):
        run = order[seg[r]:seg[r + 1]]
        red = {'mean': f64[run].mean(0), 'sum': f64[run].sum(0), 'max': f64[run].max(0)}[reduce]
        # float32 sums of up to len(run) terms: (len(run) + 1) roundings of 2^-24 relative to the sum of magnitudes
        bound = (len(run) + 1) * 2.0 ** -24 * np.abs(f64[run]).sum(0) + 1e-45
        assert (np.abs(out.features.detach().numpy()[r] - red) <= (0 if reduce == 'max' else bound)).all()
        assert (np.abs(out.xyz.detach().numpy()[r] - x64[run].mean(0)) <= (len(run) + 1) * 2.0 ** -24 * np.abs(x64[run]).sum(0) / len(run)).all()
        gx[run] = v[r] / len(run)
        if reduce == 'max':
            gf[run[f64[run].argmax(0)], np.arange(5)] = w[r]
        else:
            gf[run] = w[r] / (len(run) if reduce == 'mean' else 1)
    np.testing.assert_allclose(f.grad.numpy(), gf, rtol=2 ** -22, atol=0)   # one float32 division and the float32 weights
    np.testing.assert_allclose(xyz.grad.numpy(), gx, rtol=2 ** -22, atol=0)


def test_grid_unpool_ragged():
    ops = _ops()
    i, _ = G.case('non_finite')
    grid = ops.grid_cluster_ragged(_t(i['xyz']), _t(i['offset']), i['size'], _t(i['start']), 60, i['axis_bits'])
    pooled = torch.randn(60, 3, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    out = ops.grid_unpool_ragged(pooled, grid)
    cluster = grid.index.cluster[0].long()
    assert out.shape == (len(i['xyz']), 3) and (cluster < 0).any()
    assert torch.equal(out[cluster >= 0], pooled[cluster[cluster >= 0]]) and not U.words(out[cluster < 0]).any()
    out.sum().backward()
    assert torch.equal(pooled.grad[:, 0], torch.bincount(cluster[cluster >= 0], minlength=60).float())


def test_knn_ragged_on_the_pooled_level_padded_and_unpadded():
    """``new_offset`` is the next stage's offset.  The CPU search validates where the kernel clips, so it takes the padded level
    cut at ``new_offset[-1]``: the rows behind it are the NaN rows of no cloud.  Both give the lists of the unpadded level."""
    ops = _ops()
    i, _ = G.case('gauss')
    args = (_t(i['xyz']), None, _t(i['offset']), i['size'])
    tight = ops.grid_pool_ragged(*args, start=_t(i['start']))
    padded = ops.grid_pool_ragged(*args, start=_t(i['start']), m=len(i['xyz']))
    u = int(tight.grid.count)
    assert tight.features is None and tight.xyz.shape == (u, 3) and int(padded.offset[-1]) == u and torch.isnan(padded.xyz[u:]).all()
    assert U.same_words(tight.xyz, padded.xyz[:u].contiguous()) and torch.equal(tight.offset, padded.offset)
    a = ops.knn_ragged(tight.xyz, tight.offset, 4)
    b = ops.knn_ragged(padded.xyz[:u], padded.offset, 4)
    assert torch.equal(a, b) and (a[:, 0] == torch.arange(u)).all()
    for (lo, hi) in R.ranges(tight.offset.numpy()):
        assert ((a[lo:hi] >= lo) & (a[lo:hi] < hi) | (a[lo:hi] == -1)).all()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------

def test_c_abi_refusals():
    """PCC_EINVAL under the entry point's name before anything is enqueued: no stream, no device memory is touched."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    ptrs = [p] * 9  # xyz offset start | cluster order seg coord new_offset n_cells

    def run(b=2, n=8, m=4, ab=4, size=0.5, null=None):
        q = list(ptrs)
        if null is not None:
            q[null] = None
        return L.pcc_grid_cluster_ragged(b, n, m, ab, q[0], q[1], q[2], size, *q[3:], None)

    bad = [dict(n=0), dict(n=-1), dict(m=0), dict(m=9), dict(b=0), dict(b=-1), dict(b=65536), dict(n=2 ** 31 - 1, m=1), dict(ab=0), dict(ab=17),
           dict(b=32768, ab=16), dict(b=65535, ab=16), dict(size=0.0), dict(size=-1.0), dict(size=float('inf')), dict(size=float('nan'))]
    bad += [dict(null=k) for k in range(9)]
    for kw in bad:
        assert run(**kw) == -22, kw
        assert L.pcc_last_error().decode().startswith('grid_cluster_ragged:') and L.pcc_last_status() == -22, kw
    assert run(b=32768, ab=16) == -22 and 'wider than 63 bits' in L.pcc_last_error().decode()
    assert run(n=2 ** 31 - 1, m=1) == -22 and '2^31' in L.pcc_last_error().decode()


def test_python_refusals():
    ops = _ops()
    xyz, offset = torch.zeros(10, 3), torch.tensor([4, 10])
    ok = dict(size=0.5)
    for name, kw, exc in [
        ('xyz shape', dict(xyz=torch.zeros(10, 2)), ValueError), ('xyz dtype', dict(xyz=torch.zeros(10, 3, dtype=torch.float64)), RuntimeError),
        ('n = 0', dict(xyz=torch.zeros(0, 3)), ValueError), ('offset dtype', dict(offset=torch.tensor([4.0, 10.0])), ValueError),
        ('no cloud', dict(offset=torch.zeros(0, dtype=torch.int64)), ValueError), ('too many clouds', dict(offset=torch.zeros(65536, dtype=torch.int64)), ValueError),
        ('size 0', dict(size=0.0), ValueError), ('size nan', dict(size=float('nan')), ValueError), ('size inf', dict(size=float('inf')), ValueError),
        ('size str', dict(size='1'), ValueError), ('size underflows', dict(size=1e-60), ValueError), ('m 0', dict(m=0), ValueError),
        ('m > n', dict(m=11), ValueError), ('m float', dict(m=2.0), ValueError), ('axis_bits 0', dict(axis_bits=0), ValueError),
        ('axis_bits 17', dict(axis_bits=17), ValueError), ('axis_bits bool', dict(axis_bits=True), ValueError),
        ('start shape', dict(start=torch.zeros(3, 3)), ValueError), ('start dtype', dict(start=torch.zeros(2, 3, dtype=torch.float64)), RuntimeError),
        ('descending', dict(offset=torch.tensor([6, 4])), ValueError), ('negative', dict(offset=torch.tensor([-1, 4])), ValueError),
        ('beyond n', dict(offset=torch.tensor([4, 11])), ValueError),
    ]:
        args = dict(xyz=xyz, offset=offset, **ok)
        args.update(kw)
        with pytest.raises(exc, match='grid_cluster_ragged|must be'):
            ops.grid_cluster_ragged(**args)
    with pytest.raises(ValueError, match='wider than 63 bits'):
        ops.grid_cluster_ragged(torch.zeros(10, 3), torch.full((40000,), 10), 0.5, axis_bits=16)
    for kw in (dict(features=torch.zeros(9, 2)), dict(features=torch.zeros(10, 0)), dict(features=torch.zeros(10, 2, dtype=torch.float64)),
               dict(features=torch.zeros(10, 2), reduce='min'), dict(features=torch.zeros(1, 2, 10))):
        with pytest.raises((ValueError, RuntimeError), match='grid_pool_ragged|must be'):
            ops.grid_pool_ragged(xyz, kw.pop('features'), offset, 0.5, **kw)
    grid = ops.grid_cluster_ragged(xyz, offset, 0.5, m=3)
    for pooled, g in ((torch.zeros(4, 2), grid), (torch.zeros(3), grid), (torch.zeros(3, 2), grid.index)):
        with pytest.raises(ValueError, match='grid_unpool_ragged'):
            ops.grid_unpool_ragged(pooled, g)


def test_the_registry_of_unaligned_views_holds_the_entry_point():
    names = [case.name for case in U.CASES]
    assert names.count('grid_cluster_ragged') == 1 and 'pcc_grid_cluster_ragged' in U.covered()
    case = U.CASES[names.index('grid_cluster_ragged')]
    assert case.dims['b'] == 2 and max(case.dims.values()) <= 512 and case.anchor is not None and case.cpu
