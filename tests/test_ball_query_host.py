"""CPU tests of ``neighbour_ops.ball_query``: the torch path of CPU tensors against the float64 reference
(tests/ball_query_reference.py) -- word for word on lattices and, because the path evaluates the kernel's float32 rule
exactly, on generic clouds too wherever the reference is unambiguous -- and the argument checks that need no device."""

import ctypes

import numpy as np
import pytest
import torch

from tests.ball_query_reference import GENERIC_KINDS, GENERIC_SHAPES, BallReference, between_lattice, generic_cloud
from tests.fps_reference import lattice_cloud

RADII = (0.0625, 0.125, 0.25, 0.2, 10.0, float('inf'))
NSAMPLES = (1, 2, 31, 64, 65, 200)


def _ball(x, c, radius, nsample, pad):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    idx, cnt = ops.ball_query(torch.from_numpy(x), torch.from_numpy(c), radius, nsample, pad=pad, return_count=True)
    assert idx.dtype == torch.int64 and cnt.dtype == torch.int32
    assert idx.shape == (x.shape[0], c.shape[1], nsample) and cnt.shape == (x.shape[0], c.shape[1])
    return idx.numpy(), cnt.numpy()


def lattice_centres(seed, x, m, between):
    """``m`` centres per cloud: points of the cloud itself (cycled when m > n), or points between lattice points."""
    if between:
        return between_lattice(seed, x.shape[0], m)
    return np.ascontiguousarray(x[:, np.arange(m) % x.shape[1]])


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 129, 1025, 2049])
def test_cpu_path_exact_on_lattices(n):
    for levels in (4, 16):
        x = lattice_cloud(500 * levels + n, 3, n, levels)
        for m, between in ((1, False), (3, True), (65, False), (65, True)):
            c = lattice_centres(n + m, x, m, between)
            ref = BallReference(x, c)
            for radius in RADII:
                for k, nsample in enumerate(NSAMPLES):
                    pad = ('first', 'none')[(k + m) % 2]  # (both pads at every radius; the GPU test takes the full product)
                    idx, cnt = _ball(x, c, radius, nsample, pad)
                    ref.check_exact(radius, nsample, pad, idx, cnt)


@pytest.mark.parametrize('kind', GENERIC_KINDS)
def test_cpu_path_on_generic_clouds(kind):
    for b, n, m, r in GENERIC_SHAPES:
        x, scale = generic_cloud(11, b, n, kind)
        c = np.ascontiguousarray(x[:, :m])
        ref = BallReference(x, c)
        for radius in (r, 0.5) if n == 2048 else (r,):
            for nsample, pad in ((16, 'first'), (64, 'none')):
                idx, cnt = _ball(x, c, radius * scale, nsample, pad)
                ref.check_margin(radius * scale, nsample, pad, idx, cnt)


def test_non_finite_input_on_the_cpu_path():
    x = lattice_cloud(3, 3, 100, 4)
    x[0, [0, 17, 99]] = [[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf]]
    x[1] = np.nan
    c = np.ascontiguousarray(x[:, :40])
    c[2, 5] = [0.5, np.nan, 0.5]
    for radius in (0.3, float('inf')):
        for pad, fill in (('first', 0), ('none', -1)):
            idx, cnt = _ball(x, c, radius, 20, pad)
            BallReference(x, c).check_exact(radius, 20, pad, idx, cnt)
            for qi in range(40):
                assert not np.isin(idx[0, qi, :cnt[0, qi]], [0, 17, 99]).any()  # a non-finite candidate is never returned
            assert (cnt[1] == 0).all() and (idx[1] == fill).all()  # the all-NaN cloud
            assert cnt[0, 0] == 0 and cnt[0, 17] == 0 and cnt[2, 5] == 0 and (idx[2, 5] == fill).all()  # non-finite centres
            assert cnt[2, 0] > 0


def test_outputs_are_constants_and_the_package_exports_the_function():
    from pointcloudcounterfactual_amd import ball_query, neighbour_ops as ops

    assert ball_query is ops.ball_query
    x = torch.from_numpy(generic_cloud(5, 2, 200, 'gauss')[0])
    idx, cnt = ops.ball_query(x.clone().requires_grad_(True), x[:, :10].clone().requires_grad_(True), 0.3, 8, return_count=True)
    assert not idx.requires_grad and not cnt.requires_grad
    assert torch.equal(idx, ops.ball_query(x, x[:, :10], 0.3, 8))  # (a centres view that is not contiguous; no count)
    assert torch.equal(idx, ops.ball_query(x, x[:, :10], np.float32(0.3), 8))
    big = torch.from_numpy(generic_cloud(6, 2, 256, 'gauss')[0])
    view = big[:, ::2, :]
    assert not view.is_contiguous()
    assert torch.equal(ops.ball_query(view, view, 0.4, 8), ops.ball_query(view.contiguous(), view.contiguous(), 0.4, 8))


def test_argument_errors():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x, c = torch.zeros(2, 10, 3), torch.zeros(2, 4, 3)
    for radius in (0, 0.0, -1.0, float('nan'), None, '1', True, torch.tensor(1.0)):
        with pytest.raises(ValueError):
            ops.ball_query(x, c, radius, 4)
    with pytest.raises(ValueError):
        ops.ball_query(x, c, 1e-60, 4)  # 0 once it is the float32 the library receives
    for nsample in (0, -1, 2.0, True, None):
        with pytest.raises(ValueError):
            ops.ball_query(x, c, 1.0, nsample)
    for pad in ('zero', 0, None, 'FIRST'):
        with pytest.raises(ValueError):
            ops.ball_query(x, c, 1.0, 4, pad=pad)
    for bad_x, bad_c in ((torch.zeros(2, 3, 10), c), (torch.zeros(10, 3), c), (x, torch.zeros(2, 3, 4)), (x, torch.zeros(3, 4, 3)),
                         (x, torch.zeros(4, 3)), (torch.zeros(2, 0, 3), c)):
        with pytest.raises(ValueError):
            ops.ball_query(bad_x, bad_c, 1.0, 4)
    for bad_x, bad_c in ((x.double(), c), (x, c.double()), (x, c.to(torch.int32))):
        with pytest.raises(RuntimeError):
            ops.ball_query(bad_x, bad_c, 1.0, 4)
    with pytest.raises(RuntimeError):
        ops.ball_query(x, c.to('meta'), 1.0, 4)
    for ex, ec, shape in ((x[:0], c[:0], (0, 4, 5)), (x, c[:, :0], (2, 0, 5))):
        idx, cnt = ops.ball_query(ex, ec, 1.0, 5, return_count=True)
        assert idx.shape == shape and idx.dtype == torch.int64 and cnt.shape == shape[:2] and cnt.dtype == torch.int32
    # nsample may exceed n; a huge radius squares to +inf and holds every point
    idx, cnt = ops.ball_query(x, c, 1e30, 15, return_count=True)
    assert (cnt == 10).all() and torch.equal(idx[0, 0], torch.tensor(list(range(10)) + [0] * 5))


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched)."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    assert L.pcc_ball_query(0, 8, 4, 2, 1.0, 0, None, None, None, None, None) == 0  # b = 0: nothing to do
    assert L.pcc_ball_query(3, 8, 0, 2, 1.0, 1, None, None, None, None, None) == 0  # m = 0
    bad = [(1, 0, 4, 2, 1.0, 0, p, p, p), (1, 8, 4, 0, 1.0, 0, p, p, p), (1, 8, 4, 2, 0.0, 0, p, p, p),
           (1, 8, 4, 2, -1.0, 0, p, p, p), (1, 8, 4, 2, float('nan'), 0, p, p, p), (1, 8, 4, 2, 1.0, 2, p, p, p),
           (1, 8, 4, 2, 1.0, -1, p, p, p), (65536, 8, 4, 2, 1.0, 0, p, p, p), (-1, 8, 4, 2, 1.0, 0, p, p, p),
           (1, 8, -1, 2, 1.0, 0, p, p, p), (65535, 8, 65535, 2, 1.0, 0, p, p, p), (1, 8, 4, 2, 1.0, 0, None, p, p),
           (1, 8, 4, 2, 1.0, 0, p, None, p), (1, 8, 4, 2, 1.0, 0, p, p, None),
           (0, 8, 4, 2, 0.0, 0, p, p, p), (1, 8, 0, 0, 1.0, 0, p, p, p)]  # (an empty call is still checked)
    for b, n, m, nsample, radius, pad, xyz, centres, idx in bad:
        assert L.pcc_ball_query(b, n, m, nsample, radius, pad, xyz, centres, idx, None, None) != 0, (b, n, m, nsample, radius, pad)
        assert L.pcc_last_error().decode().startswith('ball_query:')


def test_the_switch_of_the_variants_is_bound():
    import os
    import re

    from pointcloudcounterfactual_amd import _lib

    hooks = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pcc_test_hooks.h')).read()
    assert re.search(r'PCC_TUNE_BALL_PATH = %d\b' % _lib.TUNING['ball_path'], hooks) and _lib.TUNING['ball_path'] == 13


def test_cloud_shape_messages_word_for_word():
    """The shape refusals of ``ball_query``, in their words, xyz before centres and both ahead of the dtypes."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import raised

    xyz, centres = torch.zeros(2, 10, 3), torch.zeros(2, 4, 3)
    for bad, shown in ((xyz[0], '(10, 3)'), (xyz[:, :, :2], '(2, 10, 2)'), (xyz[:, :0], '(2, 0, 3)')):
        assert raised(ValueError, ops.ball_query, bad.double(), centres[:1], 1.0, 4) == f'ball_query: expected xyz[B,N,3] with N >= 1, got {shown}'
    for bad, shown in ((centres[0], '(4, 3)'), (centres[:, :, :2], '(2, 4, 2)'), (centres[:1], '(1, 4, 3)')):
        assert raised(ValueError, ops.ball_query, xyz.double(), bad, 1.0, 4) == f'ball_query: expected centres[B = 2,M,3], got {shown}'
    assert ops.ball_query(xyz, centres[:, :0], 1.0, 4).shape == (2, 0, 4)  # (no centre is no error)
