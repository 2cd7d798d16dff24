"""CPU tests of ``set_metrics.occupancy_grid`` / ``jsd_between_sets``: the torch path of CPU tensors against the numpy
references of tests/occupancy_reference.py (exactly: the counts are integers), the Jensen-Shannon divergence against its
float64 formula, and every argument check of ``pcc_occupancy_grid`` through the C ABI, which needs no device."""

import ctypes
import inspect

import numpy as np
import pytest
import torch

from pointcloudcounterfactual_amd import jsd_between_sets, occupancy_grid, set_metrics
from tests.occupancy_reference import (AMBIGUOUS_CAP, GENERIC_KINDS, LATTICE_RES, cell_rule, counts_of, generic_case,
                                       generic_points, jsd64, lattice_points, nearest_grid64, sphere_mask)

PCC_OK, PCC_EINVAL = 0, -22


def _grid(x, *args, **kwargs):
    out = occupancy_grid(torch.from_numpy(np.array(x, dtype=np.float32)), *args, **kwargs)
    assert out.dtype == torch.int64
    return out.numpy()


def test_package_exports():
    assert occupancy_grid is set_metrics.occupancy_grid and jsd_between_sets is set_metrics.jsd_between_sets


@pytest.mark.parametrize('in_sphere', [False, True])
@pytest.mark.parametrize('res', LATTICE_RES)
def test_cpu_path_equals_the_rule_on_lattices(res, in_sphere):
    """Power-of-two steps and points at multiples of step / 2: every float32 operation is exact, so the counts equal the
    restated rule AND the float64 nearest grid point wherever that is unique."""
    for lo, extent in ((-0.5, 1.0), (-2.0, 4.0), (0.25, 0.5)):
        x = lattice_points(res, 10 * res + in_sphere, 3, 600, lo, extent)
        flat = cell_rule(x, res, lo, extent, in_sphere)
        per_cloud = _grid(x, res, in_sphere, True, lo, extent)
        assert per_cloud.shape == (3, res, res, res)
        assert np.array_equal(per_cloud, counts_of(flat, res, 3, per_cloud=True)), (lo, extent)
        whole = _grid(x, res, in_sphere, False, lo, extent)
        assert whole.shape == (res, res, res) and np.array_equal(whole, counts_of(flat, res)) and whole.sum() == 3 * 600
        if in_sphere:
            assert whole[~sphere_mask(res)].sum() == 0
        near, ambiguous = nearest_grid64(x, res, lo, extent, in_sphere)
        assert np.array_equal(flat[~ambiguous], near[~ambiguous])


def test_midpoints_go_up_and_outside_points_land_in_border_cells():
    res, step = 5, 0.25
    mid = np.array([[[-0.5 + (i + 0.5) * step, -0.5 + (j + 0.5) * step, 0.0] for i in range(4) for j in range(4)]], np.float32)
    got = _grid(mid, res)
    want = np.zeros((res, res, res), np.int64)
    want[1:, 1:, 2] = 1  # floorf(t + 0.5f): the midpoint between i and i + 1 belongs to i + 1
    assert np.array_equal(got, want)
    far = np.array([[[-3e38, 3e38, 0.0], [9.0, -9.0, 0.51], [-0.5 - step / 2, 0.5 + step / 2, -0.5]]], np.float32)
    got = _grid(far, res)
    assert got[0, 4, 2] == 1 and got[4, 0, 4] == 1 and got[0, 4, 0] == 1 and got.sum() == 3


def test_in_sphere_ties_go_to_the_lowest_flat_index():
    """res 3: the in-sphere grid points are the centre and the six face centres.  A cube corner is equally far from three
    face centres; the one with the lowest flat index takes it.  +-3e38 overflows every distance to inf: all seven tie."""
    res = 3
    assert sphere_mask(res).sum() == 7
    corner = np.array([[[0.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, -0.5, -0.5], [3e38, 3e38, 3e38], [0.5, 0.5, 0.0]]], np.float32)
    got = _grid(corner, res, in_sphere=True, per_cloud=True)[0]
    want = np.zeros((res, res, res), np.int64)
    for cell in ((1, 1, 2), (0, 1, 1), (1, 0, 1), (0, 1, 1), (1, 2, 1)):
        want[cell] += 1
    assert np.array_equal(got, want)
    assert np.array_equal(got, counts_of(cell_rule(corner, res, in_sphere=True), res))


@pytest.mark.parametrize('in_sphere', [False, True])
@pytest.mark.parametrize('kind', GENERIC_KINDS)
def test_cpu_path_equals_the_float64_nearest_grid_point_on_generic_clouds(kind, in_sphere):
    for res, n in ((5, 1024), (28, 512)):
        points, expected, removed = generic_case(kind, 3, 2, n, res, in_sphere)
        print(f'{kind} res={res} in_sphere={in_sphere}: removed share {removed:.4f} (cap {AMBIGUOUS_CAP})')
        assert removed <= AMBIGUOUS_CAP
        assert np.array_equal(_grid(points, res, in_sphere, True), expected)
        assert np.array_equal(_grid(points, res, in_sphere), expected.sum(0))


def test_uniform_points_mostly_take_the_in_sphere_fallback():
    """The case the rule was checked on: uniform in [-0.7, 0.7]^3 at res 28, where most points leave their separable cell."""
    points, expected, removed = generic_case('uniform', 5, 1, 2048, 28, True)
    assert removed <= AMBIGUOUS_CAP
    separable = counts_of(cell_rule(points, 28), 28)
    assert separable[~sphere_mask(28)].sum() > 0.5 * points.shape[1]
    assert np.array_equal(_grid(points, 28, True), expected[0])


def test_non_finite_points_are_counted_nowhere():
    x = generic_points('gauss', 11, 3, 200)
    clean = _grid(x, 9, per_cloud=True)
    bad = [0, 7, 63, 64, 199]
    x[0, bad] = [[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.1, -np.inf], [np.nan] * 3, [np.inf, -np.inf, 0]]
    x[1] = np.nan
    for in_sphere in (False, True):
        got = _grid(x, 9, in_sphere, per_cloud=True)
        assert got.sum(axis=(1, 2, 3)).tolist() == [200 - len(bad), 0, 200]
        assert np.array_equal(got.sum(0), _grid(x, 9, in_sphere))
        assert np.array_equal(got, counts_of(cell_rule(x, 9, in_sphere=in_sphere), 9, 3, per_cloud=True))
    assert np.array_equal(_grid(x, 9, per_cloud=True)[2], clean[2])
    assert np.array_equal(_grid(np.delete(x[:1], bad, axis=1), 9), _grid(x[:1], 9))


def test_argument_errors():
    x = torch.zeros(2, 10, 3)
    for resolution in (1, 0, -3, 129, 28.0, True, None):
        with pytest.raises(ValueError, match='resolution'):
            occupancy_grid(x, resolution)
    with pytest.raises(ValueError, match='in_sphere'):
        occupancy_grid(x, 2, in_sphere=True)
    assert occupancy_grid(x, 2).sum() == 20 and occupancy_grid(x, 3, in_sphere=True)[1, 1, 1] == 20
    for extent in (0.0, -1.0, float('inf'), float('nan'), 1e-44, 1e39):
        with pytest.raises(ValueError, match='extent'):
            occupancy_grid(x, 5, extent=extent)
    for lo in (float('inf'), float('nan'), -1e39):
        with pytest.raises(ValueError, match='lo'):
            occupancy_grid(x, 5, lo=lo)
    for bad in (torch.zeros(2, 3, 10), torch.zeros(10, 3), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError):
            occupancy_grid(bad)
    with pytest.raises(RuntimeError, match='float32'):
        occupancy_grid(x.double())
    assert occupancy_grid(x[:0], 4).shape == (4, 4, 4) and occupancy_grid(x[:0], 4).sum() == 0
    assert occupancy_grid(x[:0], 4, per_cloud=True).shape == (0, 4, 4, 4)
    view = torch.from_numpy(generic_points('gauss', 2, 2, 64))[:, ::2, :]
    assert not view.is_contiguous() and torch.equal(occupancy_grid(view), occupancy_grid(view.contiguous()))
    assert not occupancy_grid(x.clone().requires_grad_(True)).requires_grad


def test_jsd_against_the_float64_formula():
    a = torch.from_numpy(generic_points('gauss', 21, 6, 500))
    b = torch.from_numpy(generic_points('uniform', 22, 4, 300))
    for resolution, in_sphere in ((28, True), (28, False), (5, True)):
        got = jsd_between_sets(a, b, resolution, in_sphere)
        assert got.dtype == torch.float64 and got.dim() == 0
        want = jsd64(occupancy_grid(a, resolution, in_sphere).numpy(), occupancy_grid(b, resolution, in_sphere).numpy())
        assert 0.0 < got.item() < 1.0
        # entropies of at most log2(28^3) < 15 bits, each a float64 sum of < 22000 terms in another order than numpy's
        assert abs(got.item() - want) <= 1e-12
        assert torch.equal(got, jsd_between_sets(b, a, resolution, in_sphere))  # symmetric, bit for bit
    # the defaults are PointFlow's: 28^3, in the sphere
    assert torch.equal(jsd_between_sets(a, b), jsd_between_sets(a, b, 28, True))
    # invariant to the order of clouds and of points: the counts are
    shuffled = a[torch.randperm(6, generator=torch.Generator().manual_seed(1))][:, torch.randperm(500, generator=torch.Generator().manual_seed(2))]
    assert torch.equal(jsd_between_sets(shuffled, b), jsd_between_sets(a, b))
    assert torch.equal(jsd_between_sets(a.reshape(12, 250, 3), b), jsd_between_sets(a, b))


def test_jsd_is_exactly_0_for_equal_and_exactly_1_for_disjoint_distributions():
    a = torch.from_numpy(generic_points('gauss', 23, 3, 400))
    assert jsd_between_sets(a, a).item() == 0.0
    assert jsd_between_sets(a, a.flip(0).flip(1)).item() == 0.0
    assert jsd_between_sets(a, torch.cat([a, a], 0)).item() == 0.0  # twice the counts: the same distribution, exactly
    # two sets in disjoint cells: M is half of P on P's cells and half of Q on Q's
    left = torch.from_numpy(generic_points('cell', 24, 1, 64))
    right = left + torch.tensor([5 / 27, 0.0, 0.0])
    assert (occupancy_grid(left, in_sphere=True) * occupancy_grid(right, in_sphere=True)).sum() == 0
    assert jsd_between_sets(left, right).item() == 1.0
    p, q = np.zeros((4, 4, 4)), np.zeros((4, 4, 4))
    p[0, 0, :2], q[3, 3, :] = (3, 3), (1, 2, 2, 3)
    assert set_metrics.jsd_from_counts(torch.from_numpy(p), torch.from_numpy(q)).item() == pytest.approx(1.0, abs=1e-15)
    assert jsd64(p, q) == pytest.approx(1.0, abs=1e-15) and jsd64(p, p) == 0.0
    with pytest.raises(ValueError, match='finite'):
        jsd_between_sets(a, torch.full((2, 5, 3), float('nan')))
    with pytest.raises(ValueError, match='finite'):
        jsd_between_sets(torch.full((1, 5, 3), float('inf')), a)


def test_compute_all_metrics_has_with_jsd_and_it_defaults_to_off():
    parameter = inspect.signature(set_metrics.compute_all_metrics).parameters['with_jsd']
    assert parameter.default is False
    assert list(inspect.signature(set_metrics.compute_all_metrics).parameters) == ['sample', 'ref', 'pairs_per_call', 'with_jsd']


def test_c_abi_checks_every_argument_before_any_launch():
    """Each refusal of ``pcc_occupancy_grid`` with its own message, ahead of the first HIP call: the pointers are dummies
    that are never dereferenced, and there is no device here."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    dummy = 0x1000
    inf, nan = float('inf'), float('nan')

    def status_and_error(s, n, xyz, res, lo, extent, in_sphere, per_cloud, counts):
        rc = L.pcc_occupancy_grid(s, n, xyz, res, lo, extent, in_sphere, per_cloud, counts, None)
        return rc, L.pcc_last_error().decode()

    def refused(what, s=1, n=8, xyz=dummy, res=28, lo=-0.5, extent=1.0, in_sphere=0, per_cloud=0, counts=dummy):
        assert status_and_error(s, n, xyz, res, lo, extent, in_sphere, per_cloud, counts) == (PCC_EINVAL, 'occupancy_grid: ' + what)

    refused('s must be >= 0', s=-1)
    refused('n must be >= 1', n=0)
    refused('n must be >= 1', s=0, n=-1)
    for res in (1, 0, -1, 129):
        refused('res must be in [2, 128]', res=res)
    refused('in_sphere needs res >= 3', res=2, in_sphere=1)
    for extent in (0.0, -1.0, inf, nan, 1e-44):
        refused('extent must be finite and > 0', extent=extent)
    for lo in (inf, -inf, nan):
        refused('lo must be finite', lo=lo)
    refused('too many points (s * n > INT_MAX)', s=65536, n=32768)
    refused('per-cloud output too large (s * res^3 > INT_MAX)', s=2 ** 31 // 28 ** 3 + 1, n=1, per_cloud=1)
    refused('per-cloud output too large (s * res^3 > INT_MAX)', s=1024, n=1, res=128, per_cloud=1)
    refused('null pointer', xyz=None)
    refused('null pointer', counts=None)
    refused('null pointer', xyz=None, counts=None, in_sphere=1, per_cloud=1)
    # s == 0 is a no-op, whatever the pointers; the other sizes are still checked
    for in_sphere, per_cloud in ((0, 0), (1, 1)):
        assert status_and_error(0, 8, None, 28, -0.5, 1.0, in_sphere, per_cloud, None) == (PCC_OK, '')
        assert status_and_error(0, 8, dummy, 28, -0.5, 1.0, in_sphere, per_cloud, dummy) == (PCC_OK, '')
    assert _lib.TUNING['occupancy_path'] == 12
    assert L.pcc_occupancy_grid.argtypes[4] is ctypes.c_float and L.pcc_occupancy_grid.argtypes[5] is ctypes.c_float
