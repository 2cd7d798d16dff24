"""CPU tests of ``neighbour_ops.interpolation_weights`` / ``interpolate_points`` / ``feature_propagation``: the torch path of
CPU tensors against the numpy reference (tests/interpolate_reference.py) -- the forward word for word, grad_x against
float64 by the summation bound derived there, grad_w inside the bound of its channel sum --, out-of-range slots, the weights
of degenerate rows, the argument checks that need no device, and the pins of the ABI and of the variant switch."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import interpolate_reference as ref


def _words(t):
    return t.detach().numpy().view(np.uint32)


@pytest.mark.parametrize('n', ref.N_GRID)
def test_cpu_path_forward_word_for_word_and_gradients_in_bound(n):
    """grad_x by gamma(deg + 1) * sum |w g|; grad_w (autograd sums the channels in an order of its own) by
    gamma(c + 1) * sum_ch |g x|, the same bound for its sum of c rounded products."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x_all = ref.cloud(n, n)
    rng = np.random.default_rng(1000 + n)
    for m, k, c, b, _, j in ref.grid():
        idx = ref.random_list(31 * m + k + n, ref.B_MAX, n, m, k)[:b]
        w = ref.gaussian_weights(j, b, m, k)
        x = np.ascontiguousarray(x_all[:b, :c])
        tx = torch.from_numpy(x).requires_grad_(True)
        tw = torch.from_numpy(w).requires_grad_(True)
        out = ops.interpolate_points(tx, torch.from_numpy(idx), tw)
        assert out.shape == (b, c, m) and out.dtype == torch.float32
        assert np.array_equal(_words(out), ref.forward(x, idx, w).view(np.uint32)), (m, k, c, b)
        g = rng.standard_normal((b, c, m)).astype(np.float32)
        out.backward(torch.from_numpy(g))
        ref.GradX(idx, w, g, n).check_bound(tx.grad.numpy())
        valid, xg = ref._gathered(x.astype(np.float64), idx)
        prod = g.astype(np.float64)[:, :, :, None] * xg
        want, bound = np.where(valid, prod.sum(1), 0.0), ref.gamma(c + 1) * np.abs(prod).sum(1)
        assert (np.abs(tw.grad.numpy() - want) <= bound).all()
        assert (tw.grad.numpy()[~valid] == 0).all()


def test_out_of_range_slots_add_nothing_and_carry_no_gradient():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    nan, inf = float('nan'), float('inf')
    x = torch.tensor([[[1.0, 2.0, 4.0]]], requires_grad=True)  # [1,1,3]
    idx = torch.tensor([[[0, -1, 3, 1], [1 << 40, 2, -7, 1]]])
    w = torch.tensor([[[1.0, nan, inf, 0.5], [nan, 2.0, -inf, 1.0]]], requires_grad=True)
    out = ops.interpolate_points(x, idx, w)
    assert out.shape == (1, 1, 2)
    assert np.array_equal(_words(out).reshape(-1), np.array([2.0, 10.0], dtype=np.float32).view(np.uint32))
    out.backward(torch.tensor([[[1.0, 10.0]]]))
    assert torch.equal(x.grad, torch.tensor([[[1.0, 10.5, 20.0]]]))
    assert torch.equal(w.grad, torch.tensor([[[1.0, 0.0, 0.0, 2.0], [0.0, 40.0, 0.0, 20.0]]]))
    # IEEE elsewhere: 0 * inf is NaN, a NaN weight of an in-range slot propagates; the NaN is the word 0x7fc00000
    x2 = torch.tensor([[[inf, 1.0, -0.0]]])
    got = ops.interpolate_points(x2, torch.tensor([[[0, 1], [1, 2], [2, 2], [0, 0]]]),
                                 torch.tensor([[[0.0, 1.0], [nan, 1.0], [1.0, 1.0], [1.0, -1.0]]]))
    assert np.array_equal(_words(got).reshape(-1), np.array([0x7fc00000, 0x7fc00000, 0, 0x7fc00000], dtype=np.uint32))


def test_interpolation_weights():
    from pointcloudcounterfactual_amd import interpolation_weights, neighbour_ops as ops

    assert interpolation_weights is ops.interpolation_weights
    nan = float('nan')
    dist = torch.tensor([[[0.0, 0.0, 1.0], [1.0, 3.0, nan], [nan, nan, nan], [0.25, 0.25, 0.25], [0.0, 4.0, 9.0]]])
    w = ops.interpolation_weights(dist)
    assert w.shape == dist.shape and w.dtype == torch.float32
    r = 1 / (dist.double() + 1e-8)
    r[torch.isnan(dist)] = 0
    want = r / r.sum(-1, keepdim=True).clamp_min(1e-300)
    assert torch.allclose(w.double(), want, rtol=1e-6, atol=0)
    assert torch.equal(w[0, 2], torch.zeros(3)) and w[0, 1, 2] == 0        # an all-NaN row, a padded slot
    assert abs(w[0, 0, 0] - 0.5) < 1e-6 and w[0, 0, 2] < 1e-7               # coincident points take all the weight
    assert torch.allclose(w[0, :2].sum(-1), torch.ones(2)) and torch.allclose(w[0, 3:].sum(-1), torch.ones(2))
    assert abs(w[0, 4, 0] - 1) < 1e-6
    # another eps; differentiable in dist, and no NaN gradient from behind the mask
    assert torch.allclose(ops.interpolation_weights(torch.tensor([[[1.0, 3.0]]]), eps=1.0), torch.tensor([[[2 / 3, 1 / 3]]]))
    d = dist.clone().requires_grad_(True)
    ops.interpolation_weights(d)[..., 0].sum().backward()
    assert torch.isfinite(d.grad).all() and (d.grad[0, 2] == 0).all() and d.grad[0, 1, 0] < 0 < d.grad[0, 1, 1]
    for bad in (dist[0], dist.long()):
        with pytest.raises(ValueError):
            ops.interpolation_weights(bad)


@pytest.mark.parametrize('with_skip', [True, False])
def test_feature_propagation_on_the_cpu(with_skip):
    from pointcloudcounterfactual_amd import feature_propagation, neighbour_ops as ops

    assert feature_propagation is ops.feature_propagation
    b, n, m, c, c2 = 3, 37, 300, 5, 4
    rng = np.random.default_rng(5)
    dense_np, sparse_np = rng.random((b, m, 3)).astype(np.float32), rng.random((b, n, 3)).astype(np.float32)
    feat_np, skip_np = rng.standard_normal((b, c, n)).astype(np.float32), rng.standard_normal((b, c2, m)).astype(np.float32)
    for k in (3, 1, 40):
        dense, sparse = torch.from_numpy(dense_np).requires_grad_(True), torch.from_numpy(sparse_np).requires_grad_(True)
        feat = torch.from_numpy(feat_np).requires_grad_(True)
        skip = torch.from_numpy(skip_np).requires_grad_(True) if with_skip else None
        res = ops.feature_propagation(dense, sparse, feat, skip, k=k)
        assert res._fields == ('out', 'idx', 'weights')
        kk = min(k, n)
        # the hand-written composition: the search, the weights, a gather of [B,C,M,k], a multiplication and the sums
        idx, dist = ops.knn_cross(dense.detach().transpose(1, 2), sparse.detach().transpose(1, 2), kk, return_distance=True)
        weights = ops.interpolation_weights(dist.clamp_min(0))
        assert res.idx.shape == (b, m, kk) and torch.equal(res.idx, idx) and torch.equal(res.weights, weights)
        assert not res.idx.requires_grad and not res.weights.requires_grad
        assert torch.allclose(res.weights.sum(-1), torch.ones(b, m), atol=1e-5)
        want = ref.hand_propagation(feat_np, skip_np if with_skip else None, idx.numpy(), weights.numpy())
        assert res.out.shape == (b, c + (c2 if with_skip else 0), m)
        assert np.array_equal(_words(res.out), want.view(np.uint32))
        g = rng.standard_normal(want.shape).astype(np.float32)
        res.out.backward(torch.from_numpy(g))
        ref.GradX(idx.numpy(), weights.numpy(), g[:, :c], n).check_bound(feat.grad.numpy())
        if with_skip:
            assert np.array_equal(skip.grad.numpy(), g[:, c:])
        assert dense.grad is None and sparse.grad is None  # (constants of the graph)


def test_views_constants_and_exports():
    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import interpolate_points, neighbour_ops as ops

    assert interpolate_points is ops.interpolate_points
    for name in ('interpolation_weights', 'interpolate_points', 'feature_propagation'):
        assert name in pkg.__all__
    x = torch.from_numpy(ref.cloud(3, 40, 2, 6))
    idx = torch.from_numpy(ref.random_list(4, 2, 20, 7, 6))
    w = torch.from_numpy(ref.gaussian_weights(5, 2, 7, 6))
    view, iview, wview = x[:, ::2, ::2], idx[:, :, ::2], w[:, :, ::2]
    assert not view.is_contiguous() and not iview.is_contiguous() and not wview.is_contiguous()
    assert torch.equal(ops.interpolate_points(view, iview, wview),
                       ops.interpolate_points(view.contiguous(), iview.contiguous(), wview.contiguous()))
    for shape in ((0, 7), (2, 0)):
        out = ops.interpolate_points(x[:shape[0]], idx[:shape[0], :shape[1]], w[:shape[0], :shape[1]])
        assert out.shape == (shape[0], 6, shape[1]) and out.dtype == torch.float32


def test_argument_errors():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x, idx, w = torch.zeros(2, 4, 10), torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 5, 3)
    ops.interpolate_points(x, idx, w)
    bad_shapes = [(x[0], idx, w), (x, idx[0], w), (x, idx[:1], w), (x, idx[:, :, :0], w[:, :, :0]), (x[:, :0], idx, w),
                  (x[:, :, :0], idx, w), (x, idx, w[:, :4]), (x, idx, w[:, :, :2]), (x, idx, w[:1]), (x, idx, w[0])]
    for bx, bi, bw in bad_shapes:
        with pytest.raises(ValueError):
            ops.interpolate_points(bx, bi, bw)
    for bx, bi, bw, name in ((x.double(), idx, w, 'x'), (x, idx.int(), w, 'idx'), (x, idx.float(), w, 'idx'),
                             (x, idx, w.double(), 'weights'), (x, idx, w.half(), 'weights')):
        with pytest.raises(RuntimeError, match=f'{name} must be torch'):
            ops.interpolate_points(bx, bi, bw)
    for bx, bi, bw in ((x, idx.to('meta'), w), (x, idx, w.to('meta'))):
        with pytest.raises(RuntimeError, match='expected cpu'):
            ops.interpolate_points(bx, bi, bw)
    dense, sparse, feat, skip = torch.rand(2, 7, 3), torch.rand(2, 10, 3), torch.zeros(2, 4, 10), torch.zeros(2, 3, 7)
    ops.feature_propagation(dense, sparse, feat, skip)
    bad = [(dense[0], sparse, feat, skip), (dense[:, :, :2], sparse, feat, skip), (dense, sparse[:1], feat, skip),
           (dense, sparse.transpose(1, 2), feat, skip), (dense, sparse[:, :0], feat[:, :, :0], skip), (dense, sparse, feat[:, :, :9], skip),
           (dense, sparse, feat[:, :0], skip), (dense, sparse, feat[:1], skip), (dense, sparse, feat, skip[:, :, :6]),
           (dense, sparse, feat, skip[:1]), (dense, sparse, feat, skip[0])]
    for args in bad:
        with pytest.raises(ValueError):
            ops.feature_propagation(*args)
    for k in (0, -1, 129, 2.0, True, None):
        with pytest.raises(ValueError):
            ops.feature_propagation(dense, sparse, feat, skip, k=k)
    for args in ((dense.double(), sparse, feat, skip), (dense, sparse.double(), feat, skip), (dense, sparse, feat.half(), skip),
                 (dense, sparse, feat, skip.double()), (dense, sparse.to('meta'), feat, skip), (dense, sparse, feat, skip.to('meta'))):
        with pytest.raises(RuntimeError):
            ops.feature_propagation(*args)


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched: the sentinel stays)."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)(*([0x5a] * 64))
    p = ctypes.addressof(buf)
    # (b, c, n, m, k, out_c, out_c0)
    good = (1, 3, 8, 4, 2, 3, 0)
    bad = [(-1, 3, 8, 4, 2, 3, 0), (65536, 3, 8, 4, 2, 3, 0), (1, 0, 8, 4, 2, 3, 0), (1, 3, 0, 4, 2, 3, 0), (1, 3, 8, -1, 2, 3, 0),
           (1, 3, 8, 4, 0, 3, 0), (1, 3, 8, 4, 2, 2, 0), (1, 3, 8, 4, 2, 3, 1), (1, 3, 8, 4, 2, 3, -1), (1, 3, 8, 1 << 16, 1 << 15, 3, 0),
           (0, 3, 8, 4, 0, 3, 0), (1, 3, 8, 0, 2, 2, 0)]  # (an empty call is still checked)
    for b, c, n, m, k, out_c, out_c0 in bad:
        assert L.pcc_interpolate(b, c, n, m, k, p, p, p, p, out_c, out_c0, None) != 0, (b, c, n, m, k, out_c, out_c0)
        assert L.pcc_last_error().decode().startswith('interpolate:')
        assert L.pcc_interpolate_bwd(b, c, n, m, k, p, p, p, p, out_c, out_c0, p, p, None) != 0
        assert L.pcc_last_error().decode().startswith('interpolate_bwd:')
    b, c, n, m, k, out_c, out_c0 = good
    for x, idx, w, out in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.pcc_interpolate(b, c, n, m, k, x, idx, w, out, out_c, out_c0, None) != 0
        assert L.pcc_last_error().decode().startswith('interpolate: null pointer')
    for x, idx, w, g, gx, gw in ((p, None, p, p, p, p), (p, p, None, p, p, p), (p, p, p, None, p, p), (None, p, p, p, p, p),
                                 (None, p, p, p, None, p)):
        assert L.pcc_interpolate_bwd(b, c, n, m, k, x, idx, w, g, out_c, out_c0, gx, gw, None) != 0
        assert L.pcc_last_error().decode().startswith('interpolate_bwd: null pointer')
    # nothing to do: an empty batch, an empty list forward, no gradient asked for
    assert L.pcc_interpolate(0, c, n, m, k, None, None, None, None, out_c, out_c0, None) == 0
    assert L.pcc_interpolate(b, c, n, 0, k, None, None, None, None, out_c, out_c0, None) == 0
    assert L.pcc_interpolate_bwd(0, c, n, m, k, None, None, None, None, out_c, out_c0, None, None, None) == 0
    assert L.pcc_interpolate_bwd(b, c, n, m, k, None, None, None, None, out_c, out_c0, None, None, None) == 0
    assert L.pcc_last_status() == 0
    assert bytes(buf) == b'\x5a' * 64


def test_the_abi_and_the_switch_of_the_paths_are_bound():
    from pointcloudcounterfactual_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = open(os.path.join(root, 'include', 'pcc_test_hooks.h')).read()
    assert re.search(r'PCC_TUNE_INTERP_PATH = %d\b' % _lib.TUNING['interp_path'], hooks) and _lib.TUNING['interp_path'] == 15
    assert re.search(r'PCC_TUNE_KEYS = 16\b', hooks)
    assert len(_lib.ABI['pcc_interpolate'][1]) == 12 and len(_lib.ABI['pcc_interpolate_bwd'][1]) == 14


def test_messages_word_for_word():
    """Every refusal ``interpolate_points`` / ``feature_propagation`` and ``pcc_interpolate`` / ``_bwd`` share with the other
    list ops, in their words and in the order in which a call with several bad arguments reports them."""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import c_status, raised

    x, idx, w = torch.zeros(2, 4, 10), torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 5, 3)
    huge = torch.zeros(2, 1 << 16, 1 << 15, dtype=torch.int64, device='meta')
    val = [((x[0], idx, w), 'expected x[B,C,N] with C >= 1 and N >= 1, got (4, 10)'),
           ((x[:, :0], idx, w), 'expected x[B,C,N] with C >= 1 and N >= 1, got (2, 0, 10)'),
           ((x[:, :, :0], idx[:1], w), 'expected x[B,C,N] with C >= 1 and N >= 1, got (2, 4, 0)'),
           ((x, idx[0], w), 'expected idx[B = 2,M,k] with k >= 1, got (5, 3)'),
           ((x, idx[:1], w), 'expected idx[B = 2,M,k] with k >= 1, got (1, 5, 3)'),
           ((x, idx[:, :, :0], w), 'expected idx[B = 2,M,k] with k >= 1, got (2, 5, 0)'),
           ((x, huge, w), 'idx[B,M,k] with M * k >= 2^31, got (2, 65536, 32768)'),
           ((x.double(), idx.int(), w[:1]), 'expected weights[B,M,k] = (2, 5, 3), got (1, 5, 3)')]  # (shapes before dtypes)
    for args, text in val:
        assert raised(ValueError, ops.interpolate_points, *args) == 'interpolate_points: ' + text
    assert raised(RuntimeError, ops.interpolate_points, x, idx.int(), w) == 'idx must be torch.int64, found torch.int32'
    assert raised(RuntimeError, ops.interpolate_points, x.double(), idx.int(), w) == 'x must be torch.float32, found torch.float64'
    assert raised(RuntimeError, ops.interpolate_points, x, idx.int().to('meta'), w.double()) == 'idx must be torch.int64, found torch.int32'
    assert raised(RuntimeError, ops.interpolate_points, x, idx.to('meta'), w.double()) == 'idx is on meta, expected cpu'

    dense, sparse, feat, skip = torch.rand(2, 7, 3), torch.rand(2, 10, 3), torch.zeros(2, 4, 10), torch.zeros(2, 3, 7)
    val = [((dense[0], sparse, feat, skip), 'expected xyz_dense[B,M,3], got (7, 3)'),
           ((dense[:, :, :2], sparse[:1], feat, skip), 'expected xyz_dense[B,M,3], got (2, 7, 2)'),
           ((dense, sparse[:1], feat, skip), 'expected xyz_sparse[B = 2,N,3] with N >= 1, got (1, 10, 3)'),
           ((dense, sparse.transpose(1, 2), feat, skip), 'expected xyz_sparse[B = 2,N,3] with N >= 1, got (2, 3, 10)'),
           ((dense, sparse[:, :0], feat[:, :, :0], skip), 'expected xyz_sparse[B = 2,N,3] with N >= 1, got (2, 0, 3)'),
           ((dense, sparse, feat[:, :, :9], skip), 'expected features[B = 2,C,N = 10] with C >= 1, got (2, 4, 9)')]
    for args, text in val:
        assert raised(ValueError, ops.feature_propagation, *args) == 'feature_propagation: ' + text
    assert ops.feature_propagation(dense[:, :0], sparse, feat).out.shape == (2, 4, 0)  # (no dense point is no error)
    for k, shown in ((0, '0'), (129, '129'), (2.0, '2.0'), (True, 'True'), (None, 'None')):
        assert raised(ValueError, ops.feature_propagation, dense, sparse, feat, skip, k=k) == \
            f'feature_propagation: k must be an integer in [1, 128], got {shown}'
    assert raised(ValueError, ops.feature_propagation, dense, sparse, feat.double(), skip, k=0) == \
        'feature_propagation: k must be an integer in [1, 128], got 0'  # (k before the dtypes)

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
    # (b, c, n, m, k, out_c, out_c0): the first refusal in the order of the checks wins
    cases = [((-1, 3, 8, 4, 2, 3, 0), 'bad size'), ((1, 0, 8, 4, 2, 3, 0), 'bad size'), ((1, 3, 0, 4, 2, 3, 0), 'bad size'),
             ((1, 3, 8, -1, 2, 3, 0), 'bad size'), ((1, 3, 8, 4, 0, 3, 0), 'bad size'), ((65536, 0, 8, 4, 2, 3, 0), 'bad size'),
             ((65536, 3, 8, 4, 2, 3, 0), 'batch too large'), ((65536, 3, 8, 1 << 16, 1 << 15, 2, 0), 'batch too large'),
             ((1, 3, 8, 1 << 16, 1 << 15, 3, 0), 'list too long (m * k >= 2^31)'),
             ((1, 3, 8, 1 << 16, 1 << 15, 2, 0), 'list too long (m * k >= 2^31)'),
             ((1, 3, 8, 4, 2, 2, 0), 'channels out_c0 .. out_c0 + c - 1 are not inside out_c'),
             ((1, 3, 8, 4, 2, 3, 1), 'channels out_c0 .. out_c0 + c - 1 are not inside out_c'),
             ((0, 3, 8, 0, 2, 3, -1), 'channels out_c0 .. out_c0 + c - 1 are not inside out_c')]
    for (b, c, n, m, k, out_c, out_c0), text in cases:
        assert c_status(L, L.pcc_interpolate, b, c, n, m, k, p, p, p, p, out_c, out_c0, None) == (EINVAL, 'interpolate: ' + text)
        assert c_status(L, L.pcc_interpolate_bwd, b, c, n, m, k, p, p, p, p, out_c, out_c0, p, p, None) == \
            (EINVAL, 'interpolate_bwd: ' + text)
    assert c_status(L, L.pcc_interpolate, 1, 3, 8, 4, 2, None, p, p, p, 3, 0, None) == (EINVAL, 'interpolate: null pointer')
    assert c_status(L, L.pcc_interpolate, 0, 3, 8, 4, 2, None, None, None, None, 3, 0, None) == (0, '')  # (the error is cleared)
