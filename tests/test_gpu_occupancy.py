"""GPU tests of the voxel occupancy counts (``pcc_occupancy_grid`` through ``set_metrics.occupancy_grid``) and of the
Jensen-Shannon divergence on them.  The counts are integers: every comparison is exact -- against the CPU function (the
same float32 rule in torch), against the restated rule on lattices where float32 is exact, and against the float64
nearest grid point on generic clouds with the ambiguous points removed from the input (tests/occupancy_reference.py).
Every shape runs both ``in_sphere`` values, both ``per_cloud`` values and the three values of the ``occupancy_path``
switch (0 the product's choice, 1 the global-atomic path, 2 the LDS histogram where it fits)."""

import functools

import numpy as np
import pytest
import torch

from tests.occupancy_reference import (AMBIGUOUS_CAP, GENERIC_KINDS, LATTICE_RES, cell_rule, counts_of, generic_case,
                                       generic_points, kernels_of, lattice_points)
from tests.which_ran import ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

# (S, N, res): the smallest legal call; odd sizes; the workload's grid; the global path by size (step exactly 1/32); many
# slabs per workgroup; the largest grid of the LDS path
SHAPES = [(1, 1, 3), (3, 257, 5), (2, 1000, 28), (4, 2048, 33), (1, 70000, 9), (5, 64, 32)]
PATHS = (0, 1, 2)


def _sm():
    from pointcloudcounterfactual_amd import set_metrics

    return set_metrics


def _gpu(x, cuda, *args, path=0, **kwargs):
    from pointcloudcounterfactual_amd import _lib

    x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x, dtype=np.float32))
    xd = x.to(cuda)
    with _lib.tuning('occupancy_path', path):
        out, names = ran(lambda: _sm().occupancy_grid(xd, *args, **kwargs))
    # the forced path's kernel ran and no sibling (path 2 is ignored where res > 32: the global kernel, the product's choice)
    res, in_sphere, per_cloud = (lambda resolution=28, in_sphere=False, per_cloud=False, *_, **__: (resolution, in_sphere, per_cloud))(*args, **kwargs)
    if xd.numel():
        assert set(names) == kernels_of(res, in_sphere, per_cloud, path), (res, in_sphere, per_cloud, path, names)
    assert out.dtype == torch.int64 and out.device.type == 'cuda'
    return out.cpu()


@functools.lru_cache(maxsize=None)
def _bank(s, n, res, in_sphere):
    """A uniform bank in [-0.7, 0.7]^3 (with in_sphere most points take the fallback) and the CPU function's per-cloud
    counts for it, computed once."""
    x = torch.from_numpy(generic_points('uniform', 100 * s + res, s, n))
    return x, _sm().occupancy_grid(x, res, in_sphere, per_cloud=True)


@pytest.mark.parametrize('in_sphere', [False, True])
@pytest.mark.parametrize('s,n,res', SHAPES)
def test_counts_equal_the_cpu_function_on_every_path(cuda, s, n, res, in_sphere):
    x, cpu = _bank(s, n, res, in_sphere)
    assert cpu.sum() == s * n
    for path in PATHS:
        per_cloud = _gpu(x, cuda, res, in_sphere, True, path=path)
        assert torch.equal(per_cloud, cpu), path
        whole = _gpu(x, cuda, res, in_sphere, False, path=path)
        assert torch.equal(whole, cpu.sum(0)), path
        assert torch.equal(per_cloud.sum(0), whole)
        i = s // 2  # cloud i of the batch gives the row of the cloud alone
        assert torch.equal(_gpu(x[i:i + 1], cuda, res, in_sphere, True, path=path)[0], per_cloud[i]), path


@pytest.mark.parametrize('in_sphere', [False, True])
@pytest.mark.parametrize('res', LATTICE_RES)
def test_exact_on_lattices(cuda, res, in_sphere):
    """Power-of-two steps, points at multiples of step / 2 (cell midpoints, ties between in-sphere grid points and points
    outside the cube among them), also on grids that are not the unit cube."""
    for lo, extent in ((-0.5, 1.0), (-2.0, 4.0), (0.25, 0.5)):
        x = lattice_points(res, 10 * res + in_sphere, 3, 600, lo, extent)
        want = torch.from_numpy(counts_of(cell_rule(x, res, lo, extent, in_sphere), res, 3, per_cloud=True))
        for path in PATHS:
            assert torch.equal(_gpu(x, cuda, res, in_sphere, True, lo, extent, path=path), want), (lo, extent, path)
            assert torch.equal(_gpu(x, cuda, res, in_sphere, False, lo, extent, path=path), want.sum(0)), (lo, extent, path)


@pytest.mark.parametrize('in_sphere', [False, True])
@pytest.mark.parametrize('kind', GENERIC_KINDS)
def test_nearest_grid_point_on_generic_clouds(cuda, kind, in_sphere):
    for res, n in ((5, 1024), (28, 512)):
        points, expected, removed = generic_case(kind, 3, 2, n, res, in_sphere)
        print(f'{kind} res={res} in_sphere={in_sphere}: removed share {removed:.4f} (cap {AMBIGUOUS_CAP})')
        assert removed <= AMBIGUOUS_CAP
        for path in PATHS:
            assert torch.equal(_gpu(points, cuda, res, in_sphere, True, path=path), torch.from_numpy(np.array(expected))), (res, path)


def test_non_finite_points_are_counted_nowhere(cuda):
    x = generic_points('gauss', 11, 3, 200)
    healthy = x[2].copy()
    bad = [0, 7, 63, 64, 199]
    x[0, bad] = [[np.nan, 0, 0], [0, np.inf, 0], [0.1, 0.1, -np.inf], [np.nan] * 3, [np.inf, -np.inf, 0]]
    x[1] = np.nan
    for in_sphere in (False, True):
        want = torch.from_numpy(counts_of(cell_rule(x, 9, in_sphere=in_sphere), 9, 3, per_cloud=True))
        for path in PATHS:
            got = _gpu(x, cuda, 9, in_sphere, True, path=path)
            assert got.sum(dim=(1, 2, 3)).tolist() == [200 - len(bad), 0, 200]  # a whole cloud of NaN: a zero row
            assert torch.equal(got, want)
            assert torch.equal(_gpu(x, cuda, 9, in_sphere, path=path), want.sum(0))
            assert torch.equal(_gpu(healthy[None], cuda, 9, in_sphere, path=path), got[2])
            assert torch.equal(_gpu(np.delete(x[:1], bad, axis=1), cuda, 9, in_sphere, path=path), got[0])


def test_huge_coordinates_are_clamped_to_border_cells(cuda):
    big = 3e38
    x = np.array([[[big, big, big], [-big, -big, -big], [big, -big, 0.0], [0.0, 0.0, -big], [-big, 0.2, big], [0.1, big, -0.3]]],
                 np.float32)
    for res in (5, 28, 33):
        for in_sphere in (False, True):
            want = _sm().occupancy_grid(torch.from_numpy(x), res, in_sphere)
            assert want.sum() == 6
            if not in_sphere:
                assert want[res - 1, res - 1, res - 1] == 1 and want[0, 0, 0] == 1 and want[res - 1, 0, (res - 1) // 2 + (res % 2 == 0)] == 1
            for path in PATHS:
                assert torch.equal(_gpu(x, cuda, res, in_sphere, path=path), want), (res, in_sphere, path)


def test_side_stream(cuda):
    x, cpu = _bank(3, 257, 5, True)
    xd = x.to(cuda)
    side = torch.cuda.Stream(device=cuda)
    side.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(side):
        per_cloud = _sm().occupancy_grid(xd, 5, True, True)
        whole = _sm().occupancy_grid(xd, 5, True)
    side.synchronize()
    assert torch.equal(per_cloud.cpu(), cpu) and torch.equal(whole.cpu(), cpu.sum(0))


def test_a_dirty_counts_buffer_is_overwritten(cuda):
    """Through the C ABI: the caller's buffer holds garbage, the call zeroes what it must itself."""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd._lib import call, ptr

    for s, n, res in ((3, 257, 5), (2, 1000, 28), (2, 300, 33)):
        for in_sphere in (0, 1):
            x, cpu = _bank(s, n, res, bool(in_sphere))
            xd = x.to(cuda).contiguous()
            for per_cloud in (0, 1):
                for path in PATHS:
                    counts = torch.full((s if per_cloud else 1, res ** 3), 12345, dtype=torch.int32, device=cuda)
                    with _lib.tuning('occupancy_path', path):
                        for _ in range(2):  # (the second call finds the first one's counts)
                            _, names = ran(lambda: call(_lib.lib.pcc_occupancy_grid, 'occupancy_grid', cuda, s, n,
                                                        ptr(xd, 'xyz', torch.float32, cuda), res, -0.5, 1.0, in_sphere, per_cloud,
                                                        ptr(counts, 'counts', torch.int32, cuda)))
                            assert set(names) == kernels_of(res, in_sphere, per_cloud, path), (res, in_sphere, per_cloud, path, names)
                    want = cpu if per_cloud else cpu.sum(0, keepdim=True)
                    assert torch.equal(counts.cpu().to(torch.int64), want.reshape(-1, res ** 3)), (s, n, res, in_sphere, per_cloud, path)


def test_argument_errors_raise_before_any_launch(cuda):
    sm = _sm()
    x = torch.zeros(2, 10, 3, device=cuda)
    for resolution in (1, 129, 28.0, True):
        with pytest.raises(ValueError, match='resolution'):
            sm.occupancy_grid(x, resolution)
    with pytest.raises(ValueError, match='in_sphere'):
        sm.occupancy_grid(x, 2, in_sphere=True)
    for extent in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='extent'):
            sm.occupancy_grid(x, 5, extent=extent)
    with pytest.raises(ValueError, match='lo'):
        sm.occupancy_grid(x, 5, lo=float('nan'))
    with pytest.raises(ValueError):
        sm.occupancy_grid(x.transpose(1, 2).contiguous())
    with pytest.raises(RuntimeError, match='float32'):
        sm.occupancy_grid(x.double())
    empty = sm.occupancy_grid(x[:0], 4)
    assert empty.shape == (4, 4, 4) and empty.sum() == 0 and empty.device == x.device
    assert sm.occupancy_grid(x[:0], 4, per_cloud=True).shape == (0, 4, 4, 4)
    view = torch.from_numpy(generic_points('gauss', 2, 2, 64)).to(cuda)[:, ::2, :]
    assert not view.is_contiguous() and torch.equal(sm.occupancy_grid(view), sm.occupancy_grid(view.contiguous()))
    with pytest.raises(ValueError, match='finite'):
        sm.jsd_between_sets(x, torch.full((2, 5, 3), float('nan'), device=cuda))


def test_jsd_on_the_gpu_equals_the_cpu_value(cuda):
    """The same integer counts (checked exactly) and the same float64 formula on both devices.  The values are not the same
    bits: torch's float64 ``log2`` and the order of its sums differ between the CPU and the GPU (measured on an MI355X at
    res 28 in_sphere: 0.8668139036702218 on the CPU, 0.8668139036702254 on the GPU, 3.6e-15 apart), so the comparison
    falls back to 1e-12 absolute.  What is exact on the GPU stays exact: symmetry, 0 for equal sets, 1 for disjoint ones."""
    sm = _sm()
    a = torch.from_numpy(generic_points('gauss', 21, 6, 500))
    b = torch.from_numpy(generic_points('uniform', 22, 4, 300))
    for resolution, in_sphere in ((28, True), (28, False), (5, True)):
        cpu = sm.jsd_between_sets(a, b, resolution, in_sphere)
        gpu = sm.jsd_between_sets(a.to(cuda), b.to(cuda), resolution, in_sphere)
        assert gpu.dtype == torch.float64 and gpu.device.type == 'cuda' and gpu.dim() == 0
        print(f'res={resolution} in_sphere={in_sphere}: JSD cpu {cpu.item()!r} gpu {gpu.item()!r} difference {gpu.item() - cpu.item():.3e}')
        assert torch.equal(sm.occupancy_grid(a.to(cuda), resolution, in_sphere).cpu(), sm.occupancy_grid(a, resolution, in_sphere))
        assert torch.equal(sm.occupancy_grid(b.to(cuda), resolution, in_sphere).cpu(), sm.occupancy_grid(b, resolution, in_sphere))
        assert abs(gpu.item() - cpu.item()) <= 1e-12
        assert torch.equal(gpu, sm.jsd_between_sets(b.to(cuda), a.to(cuda), resolution, in_sphere))
    ad = a.to(cuda)
    assert sm.jsd_between_sets(ad, ad).item() == 0.0
    left = torch.from_numpy(generic_points('cell', 24, 1, 64)).to(cuda)
    assert sm.jsd_between_sets(left, left + torch.tensor([5 / 27, 0.0, 0.0], device=cuda)).item() == 1.0


def test_compute_all_metrics_with_jsd(cuda):
    sm = _sm()
    sample = torch.from_numpy(generic_points('gauss', 31, 3, 64)).to(cuda)
    ref = torch.from_numpy(generic_points('gauss', 32, 4, 64)).to(cuda)
    plain, full = sm.compute_all_metrics(sample, ref), sm.compute_all_metrics(sample, ref, with_jsd=True)
    assert 'JSD' not in plain and set(full) == set(plain) | {'JSD'}
    assert torch.equal(full['JSD'], sm.jsd_between_sets(sample, ref))
    for key in plain:
        assert torch.equal(plain[key], full[key]), key
