"""CPU tests of ``neighbour_ops.farthest_point_sample``: the torch loop of CPU tensors against the float64 greedy
reference (tests/fps_reference.py) and the argument checks that need no device."""

import numpy as np
import pytest
import torch

from tests.fps_reference import GENERIC_KINDS, check_validity, fps_reference, generic_cloud, lattice_cloud


def _fps(x, m, start=None):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    idx, dist = ops.farthest_point_sample(torch.from_numpy(x), m, start=start, return_distance=True)
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.shape == dist.shape == (x.shape[0], m)
    return idx.numpy(), dist.numpy()


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize('levels', [4, 16])
def test_cpu_path_exact_on_lattices(n, levels):
    x = lattice_cloud(100 + n, 3, n, levels)
    given = torch.tensor([n - 1, n // 2, 0])
    for start in (None, given):
        ref_idx, ref_dist = fps_reference(x, n, None if start is None else start.numpy())
        for m in sorted({1, min(2, n), max(1, n // 3), n}):
            idx, dist = _fps(x, m, start)
            assert np.array_equal(idx, ref_idx[:, :m]), (m, start)
            assert np.array_equal(dist.astype(np.float64), ref_dist[:, :m]), (m, start)  # (inf at t = 0 included)
            assert np.isposinf(dist[:, 0]).all()


@pytest.mark.parametrize('kind', GENERIC_KINDS)
def test_cpu_path_valid_on_generic_clouds(kind):
    for b, n, m in ((2, 300, 300), (2, 1025, 256)):
        x = generic_cloud(7, b, n, kind)
        idx, dist = _fps(x, m)
        check_validity(x, idx, dist)


def test_start_forms_agree_and_are_clamped():
    from pointcloudcounterfactual_amd import farthest_point_sample, neighbour_ops as ops

    assert farthest_point_sample is ops.farthest_point_sample
    x = torch.from_numpy(generic_cloud(3, 4, 200, 'gauss'))
    base = ops.farthest_point_sample(x, 50)
    assert torch.equal(base, ops.farthest_point_sample(x, 50, start=0))
    assert torch.equal(base, ops.farthest_point_sample(x, 50, start=torch.zeros(4, dtype=torch.int64)))
    assert torch.equal(base, ops.farthest_point_sample(x, 50, start=torch.zeros(4, dtype=torch.int32)))
    seven = ops.farthest_point_sample(x, 50, start=7)
    assert (seven[:, 0] == 7).all() and torch.equal(seven, ops.farthest_point_sample(x, 50, start=torch.full((4,), 7)))
    assert torch.equal(ops.farthest_point_sample(x, 50, start=-1), base)
    assert torch.equal(ops.farthest_point_sample(x, 50, start=200), ops.farthest_point_sample(x, 50, start=199))
    assert torch.equal(ops.farthest_point_sample(x, 50, start=torch.tensor([-1, 200, 10 ** 12, -10 ** 12])),
                       ops.farthest_point_sample(x, 50, start=torch.tensor([0, 199, 199, 0])))
    # the inputs are detached: no graph reaches the outputs
    idx, dist = ops.farthest_point_sample(x.clone().requires_grad_(True), 5, return_distance=True)
    assert not idx.requires_grad and not dist.requires_grad


def test_non_finite_points_are_excluded_on_the_cpu_path():
    x = lattice_cloud(5, 2, 100, 16)  # (exact in float32: the float64 reference gives the same bits)
    x[0, [0, 17, 99]] = [[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf]]
    x[1] = np.nan
    idx, dist = _fps(x, 40, torch.tensor([17, 3]))
    ref_idx, ref_dist = fps_reference(x, 40, [17, 3])
    assert np.array_equal(idx, ref_idx) and np.array_equal(dist.astype(np.float64), ref_dist, equal_nan=True)
    assert idx[0, 0] == 17 and not np.isin(idx[0, 1:], [0, 17, 99]).any() and np.isnan(dist[0, 0]) and np.isposinf(dist[0, 1])
    assert idx[1].tolist() == [3] + [0] * 39 and np.isnan(dist[1]).all()


def test_argument_errors():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x = torch.zeros(2, 10, 3)
    for m in (0, 11, -1, 2.0, True):
        with pytest.raises(ValueError):
            ops.farthest_point_sample(x, m)
    with pytest.raises(ValueError):
        ops.farthest_point_sample(torch.zeros(2, 3, 10), 2)  # channels-major
    with pytest.raises(ValueError):
        ops.farthest_point_sample(torch.zeros(10, 3), 2)
    with pytest.raises(RuntimeError):
        ops.farthest_point_sample(x.double(), 2)
    for start in (torch.zeros(3, dtype=torch.int64), torch.zeros(2), torch.zeros(2, 1, dtype=torch.int64), 1.5, 'first'):
        with pytest.raises(ValueError):
            ops.farthest_point_sample(x, 2, start=start)
    empty = ops.farthest_point_sample(torch.zeros(0, 10, 3), 4, return_distance=True)
    assert empty[0].shape == (0, 4) and empty[0].dtype == torch.int64 and empty[1].shape == (0, 4)
    # a view that is not contiguous gives the result of its contiguous copy
    big = torch.from_numpy(generic_cloud(9, 2, 128, 'gauss'))
    view = big[:, ::2, :]
    assert not view.is_contiguous()
    assert torch.equal(ops.farthest_point_sample(view, 20), ops.farthest_point_sample(view.contiguous(), 20))


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched)."""
    import ctypes

    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    assert L.pcc_fps(0, 8, 4, None, None, None, None, None) == 0  # b = 0: nothing to do
    for b, n, m, xyz, idx in ((1, 0, 1, p, p), (1, 8, 0, p, p), (1, 8, 9, p, p), (65536, 8, 4, p, p), (-1, 8, 4, p, p),
                              (1, 8, 4, None, p), (1, 8, 4, p, None)):
        assert L.pcc_fps(b, n, m, xyz, None, idx, None, None) != 0, (b, n, m)
        assert L.pcc_last_error().decode().startswith('fps:')


def test_cloud_shape_message_word_for_word():
    """The shape refusal of ``farthest_point_sample``, in its words and ahead of the dtype."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import raised

    xyz = torch.zeros(2, 10, 3)
    for bad, shown in ((xyz[0], '(10, 3)'), (xyz[:, :, :2], '(2, 10, 2)'), (xyz.transpose(1, 2), '(2, 3, 10)')):
        assert raised(ValueError, ops.farthest_point_sample, bad.double(), 2) == f'farthest_point_sample: expected xyz[B,N,3], got {shown}'
    assert raised(ValueError, ops.farthest_point_sample, xyz[:, :0], 1) == 'farthest_point_sample: m must be an int in [1, N = 0], got 1'
    assert raised(RuntimeError, ops.farthest_point_sample, xyz[:, :0].double(), 1) == 'xyz must be torch.float32, found torch.float64'
