"""CPU tests of ``neighbour_ops.group_points`` / ``sample_and_group``: the torch path of CPU tensors against the numpy
reference (tests/grouping_reference.py) -- the forward word for word, the gradients against float64 by the summation bound
derived there --, out-of-range slots, the argument checks that need no device, and the pin of the variant switch."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import grouping_reference as ref


def _words(t):
    return t.detach().numpy().view(np.uint32)


def _lists(seed, b, n, m, k):
    return {'random': ref.random_list(seed, b, n, m, k), 'first': ref.padded_list(seed + 1, b, n, m, k, 'first'),
            'none': ref.padded_list(seed + 2, b, n, m, k, 'none')}


@pytest.mark.parametrize('n', ref.N_GRID)
def test_cpu_path_forward_word_for_word_and_gradients_in_bound(n):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x_all = ref.cloud(n, n)
    rng = np.random.default_rng(1000 + n)
    lists = {}
    for m, k, c, point_major, relative, b, _, j in ref.grid():
        if (m, k) not in lists:
            lists[m, k] = _lists(31 * m + k + n, ref.B_MAX, n, m, k)
        kind = ('random', 'first', 'none')[j % 3]
        idx = lists[m, k][kind][:b]
        x = np.ascontiguousarray(x_all[:b, :c])
        centre = rng.standard_normal((b, c, m)).astype(np.float32) if relative else None
        tx = torch.from_numpy(ref.to_layout(x, point_major)).requires_grad_(True)
        tc = torch.from_numpy(ref.to_layout(centre, point_major)).requires_grad_(True) if relative else None
        out = ops.group_points(tx, torch.from_numpy(idx), tc, point_major=point_major)
        assert out.shape == (b, c, m, k) and out.dtype == torch.float32
        assert np.array_equal(_words(out), ref.forward(x, idx, centre).view(np.uint32)), (m, k, c, point_major, relative, kind)
        g = rng.standard_normal((b, c, m, k)).astype(np.float32)
        out.backward(torch.from_numpy(g))
        want = ref.Backward(idx, g, n)
        want.check_bound(gx=ref.to_layout(tx.grad.numpy(), point_major),
                         gc=ref.to_layout(tc.grad.numpy(), point_major) if relative else None)


def test_out_of_range_slots_are_zero_and_carry_no_gradient():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x = torch.tensor([[[1.0, 2.0, float('nan')]]], requires_grad=True)  # [1,1,3]
    c = torch.tensor([[[10.0, 20.0]]], requires_grad=True)              # [1,1,2]
    idx = torch.tensor([[[0, -1, 3, 1], [1 << 40, 2, -7, 1]]])
    out = ops.group_points(x, idx, c)
    assert out.shape == (1, 1, 2, 4)
    assert np.array_equal(_words(out)[0, 0, 0], np.array([-9.0, 0.0, 0.0, -8.0], dtype=np.float32).view(np.uint32))
    assert np.array_equal(_words(out)[0, 0, 1, [0, 2, 3]], np.array([0.0, 0.0, -18.0], dtype=np.float32).view(np.uint32))
    assert torch.isnan(out[0, 0, 1, 1])
    out.backward(torch.tensor([[[[1.0, 100.0, 100.0, 2.0], [100.0, 4.0, 100.0, 8.0]]]]))
    assert torch.equal(x.grad, torch.tensor([[[1.0, 10.0, 4.0]]]))
    assert torch.equal(c.grad, torch.tensor([[[-3.0, -12.0]]]))
    # the copy mode moves NaN payloads untouched
    payload = np.array([0x7fc12345, 0xffc00001, 0x7f800000, 0x80000000], dtype=np.uint32).view(np.float32).reshape(1, 1, 4)
    got = ops.group_points(torch.from_numpy(payload), torch.tensor([[[3, 0, 1, 2, 9]]]))
    assert np.array_equal(_words(got).reshape(-1), np.array([0x80000000, 0x7fc12345, 0xffc00001, 0x7f800000, 0], dtype=np.uint32))


@pytest.mark.parametrize('with_features', [True, False])
def test_sample_and_group_on_the_cpu(with_features):
    from pointcloudcounterfactual_amd import neighbour_ops as ops, sample_and_group

    assert sample_and_group is ops.sample_and_group
    b, n, m, nsample, c = 3, 300, 37, 16, 5
    rng = np.random.default_rng(5)
    xyz_np = rng.random((b, n, 3)).astype(np.float32)
    feat_np = rng.standard_normal((b, c, n)).astype(np.float32)
    for pad in ('first', 'none'):
        xyz = torch.from_numpy(xyz_np).requires_grad_(True)
        feat = torch.from_numpy(feat_np).requires_grad_(True) if with_features else None
        res = ops.sample_and_group(xyz, feat, m, 0.15, nsample, start=2, pad=pad)
        assert res._fields == ('centres', 'grouped', 'idx', 'cnt', 'sel')
        sel, idx = res.sel.numpy(), res.idx.numpy()
        assert torch.equal(res.sel, ops.farthest_point_sample(xyz, m, 2)) and not res.sel.requires_grad
        centres = np.take_along_axis(xyz_np, sel[:, :, None], axis=1)
        assert np.array_equal(res.centres.detach().numpy(), centres)
        want_idx, want_cnt = ops.ball_query(xyz, res.centres, 0.15, nsample, pad=pad, return_count=True)
        assert torch.equal(res.idx, want_idx) and torch.equal(res.cnt, want_cnt) and not res.idx.requires_grad
        assert (res.cnt.numpy() < nsample).any()  # (padding takes part)
        want = ref.forward(np.ascontiguousarray(xyz_np.transpose(0, 2, 1)), idx, np.ascontiguousarray(centres.transpose(0, 2, 1)))
        if with_features:
            want = np.concatenate([want, ref.forward(feat_np, idx)], axis=1)
        assert res.grouped.shape == (b, 3 + (c if with_features else 0), m, nsample)
        assert np.array_equal(_words(res.grouped), want.view(np.uint32))
        g = rng.standard_normal(want.shape).astype(np.float32)
        res.grouped.backward(torch.from_numpy(g))
        back = ref.Backward(idx, g[:, :3], n)
        # xyz as neighbour and as centre: one float32 sum of deg + nsample terms for a sampled point (any order)
        gxyz, gabs, deg = back.gx.copy(), back.gx_abs.copy(), back.deg.copy()
        for bi in range(b):
            np.add.at(gxyz[bi], (slice(None), sel[bi]), back.gc[bi])
            np.add.at(gabs[bi], (slice(None), sel[bi]), back.gc_abs[bi])
            np.add.at(deg[bi], sel[bi], nsample)
        got = xyz.grad.numpy().transpose(0, 2, 1)
        assert (np.abs(got - gxyz) <= ref.gamma(deg)[:, None, :] * gabs).all()
        if with_features:
            ref.Backward(idx, g[:, 3:], n).check_bound(gx=feat.grad.numpy())


def test_views_constants_and_exports():
    from pointcloudcounterfactual_amd import group_points, neighbour_ops as ops

    assert group_points is ops.group_points
    x = torch.from_numpy(ref.cloud(3, 40, 2, 6))
    idx = torch.from_numpy(ref.random_list(4, 2, 20, 7, 5))
    view, iview = x[:, ::2, ::2], idx[:, :, ::2]
    assert not view.is_contiguous() and not iview.is_contiguous()
    assert torch.equal(ops.group_points(view, iview), ops.group_points(view.contiguous(), iview.contiguous()))
    pm = x.transpose(1, 2)  # a point-major view of channels-major memory
    assert torch.equal(ops.group_points(pm, idx, point_major=True), ops.group_points(x, idx))
    for shape in ((0, 7, 5), (2, 0, 5)):
        out = ops.group_points(x[:shape[0]], idx[:shape[0], :shape[1]])
        assert out.shape == (shape[0], 6, shape[1], 5) and out.dtype == torch.float32


def test_argument_errors():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x, idx, c = torch.zeros(2, 4, 10), torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 4, 5)
    ops.group_points(x, idx, c)
    ops.group_points(x.transpose(1, 2), idx, c.transpose(1, 2), point_major=True)
    bad_shapes = [(x[0], idx, None), (x, idx[0], None), (x, idx[:1], None), (x, idx[:, :, :0], None), (x[:, :0], idx, None),
                  (x[:, :, :0], idx, None), (x, idx, c[:, :3]), (x, idx, c.transpose(1, 2)), (x, idx, c[:, :, :4]), (x, idx, c[:1])]
    for bx, bi, bc in bad_shapes:
        with pytest.raises(ValueError):
            ops.group_points(bx, bi, bc)
    with pytest.raises(ValueError):
        ops.group_points(x, idx, c, point_major=True)  # (the layouts of the other mode)
    for pm in (1, None, 'yes'):
        with pytest.raises(ValueError):
            ops.group_points(x, idx, point_major=pm)
    for bx, bi, bc, name in ((x.double(), idx, None, 'x'), (x, idx.int(), None, 'idx'), (x, idx.float(), None, 'idx'),
                             (x, idx, c.half(), 'centres')):
        with pytest.raises(RuntimeError, match=f'{name} must be torch'):
            ops.group_points(bx, bi, bc)
    for bx, bi, bc in ((x, idx.to('meta'), None), (x, idx, c.to('meta'))):
        with pytest.raises(RuntimeError, match='expected cpu'):
            ops.group_points(bx, bi, bc)
    xyz, feat = torch.rand(2, 10, 3), torch.zeros(2, 4, 10)
    for bad in (feat[:1], feat[:, :, :9], feat[0], feat[:, :0]):
        with pytest.raises(ValueError):
            ops.sample_and_group(xyz, bad, 4, 0.5, 3)
    with pytest.raises(RuntimeError):
        ops.sample_and_group(xyz, feat.double(), 4, 0.5, 3)
    with pytest.raises(RuntimeError):
        ops.sample_and_group(xyz, feat.to('meta'), 4, 0.5, 3)
    for m, radius, nsample, pad in ((0, 0.5, 3, 'first'), (11, 0.5, 3, 'first'), (4, 0.0, 3, 'first'), (4, 0.5, 0, 'first'),
                                    (4, 0.5, 3, 'zero')):
        with pytest.raises(ValueError):
            ops.sample_and_group(xyz, feat, m, radius, nsample, pad=pad)
    with pytest.raises(ValueError):
        ops.sample_and_group(xyz.transpose(1, 2), feat, 4, 0.5, 3)


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched)."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    # (b, c, n, m, k, point_major, out_c, out_c0)
    good = (1, 3, 8, 4, 2, 0, 3, 0)
    bad = [(-1, 3, 8, 4, 2, 0, 3, 0), (65536, 3, 8, 4, 2, 0, 3, 0), (1, 0, 8, 4, 2, 0, 3, 0), (1, 3, 0, 4, 2, 0, 3, 0),
           (1, 3, 8, -1, 2, 0, 3, 0), (1, 3, 8, 4, 0, 0, 3, 0), (1, 3, 8, 4, 2, 2, 3, 0), (1, 3, 8, 4, 2, -1, 3, 0),
           (1, 3, 8, 4, 2, 0, 2, 0), (1, 3, 8, 4, 2, 0, 3, 1), (1, 3, 8, 4, 2, 0, 3, -1), (1, 3, 8, 1 << 16, 1 << 15, 0, 3, 0),
           (0, 3, 8, 4, 0, 0, 3, 0), (1, 3, 8, 0, 2, 0, 2, 0)]  # (an empty call is still checked)
    for b, c, n, m, k, pm, out_c, out_c0 in bad:
        assert L.pcc_group_points(b, c, n, m, k, pm, p, p, p, p, out_c, out_c0, None) != 0, (b, c, n, m, k, pm, out_c, out_c0)
        assert L.pcc_last_error().decode().startswith('group_points:')
        assert L.pcc_group_points_bwd(b, c, n, m, k, pm, p, p, out_c, out_c0, p, p, None) != 0
        assert L.pcc_last_error().decode().startswith('group_points_bwd:')
    b, c, n, m, k, pm, out_c, out_c0 = good
    for x, idx, out in ((None, p, p), (p, None, p), (p, p, None)):
        assert L.pcc_group_points(b, c, n, m, k, pm, x, idx, None, out, out_c, out_c0, None) != 0
        assert L.pcc_last_error().decode().startswith('group_points: null pointer')
    for idx, g in ((None, p), (p, None)):
        assert L.pcc_group_points_bwd(b, c, n, m, k, pm, idx, g, out_c, out_c0, p, p, None) != 0
        assert L.pcc_last_error().decode().startswith('group_points_bwd: null pointer')
    # nothing to do: an empty batch, an empty list forward, no gradient asked for
    assert L.pcc_group_points(0, c, n, m, k, pm, None, None, None, None, out_c, out_c0, None) == 0
    assert L.pcc_group_points(b, c, n, 0, k, pm, None, None, None, None, out_c, out_c0, None) == 0
    assert L.pcc_group_points_bwd(0, c, n, m, k, pm, None, None, out_c, out_c0, None, None, None) == 0
    assert L.pcc_group_points_bwd(b, c, n, m, k, pm, None, None, out_c, out_c0, None, None, None) == 0
    assert L.pcc_last_status() == 0


def test_the_switch_of_the_paths_is_bound():
    from pointcloudcounterfactual_amd import _lib

    hooks = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'pcc_test_hooks.h')).read()
    assert re.search(r'PCC_TUNE_GROUP_PATH = %d\b' % _lib.TUNING['group_path'], hooks) and _lib.TUNING['group_path'] == 14


def test_messages_word_for_word():
    """Every refusal ``group_points`` and ``pcc_group_points`` / ``_bwd`` share with the other list ops, in their words and in
    the order in which a call with several bad arguments reports them."""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import c_status, raised

    x, idx = torch.zeros(2, 4, 10), torch.zeros(2, 5, 3, dtype=torch.int64)
    huge = torch.zeros(2, 1 << 16, 1 << 15, dtype=torch.int64, device='meta')
    val = [((x[0], idx), 'expected x[B,C,N] with C >= 1 and N >= 1, got (4, 10)'),
           ((x, idx[0]), 'expected idx[B = 2,M,k] with k >= 1, got (5, 3)'),
           ((x, idx[:1]), 'expected idx[B = 2,M,k] with k >= 1, got (1, 5, 3)'),
           ((x, idx[:, :, :0]), 'expected idx[B = 2,M,k] with k >= 1, got (2, 5, 0)'),
           ((x, huge), 'idx[B,M,k] with M * k >= 2^31, got (2, 65536, 32768)'),
           ((x.double(), idx.int()[:1]), 'expected idx[B = 2,M,k] with k >= 1, got (1, 5, 3)'),  # (shapes before dtypes)
           ((x, idx, torch.zeros(2, 4, 4)), 'expected centres[B,C,M] = (2, 4, 5), got (2, 4, 4)')]
    for args, text in val:
        assert raised(ValueError, ops.group_points, *args) == 'group_points: ' + text
    assert raised(RuntimeError, ops.group_points, x, idx.int()) == 'idx must be torch.int64, found torch.int32'
    assert raised(RuntimeError, ops.group_points, x.double(), idx.int()) == 'x must be torch.float32, found torch.float64'
    assert raised(RuntimeError, ops.group_points, x, idx.to('meta')) == 'idx is on meta, expected cpu'

    L = _lib.lib
    buf = (ctypes.c_char * 64)()
    p = ctypes.addressof(buf)
    EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
    # (b, c, n, m, k, point_major, out_c, out_c0): the first refusal in the order of the checks wins
    cases = [((-1, 3, 8, 4, 2, 0, 3, 0), 'bad size'), ((1, 0, 8, 4, 2, 0, 3, 0), 'bad size'), ((1, 3, 0, 4, 2, 0, 3, 0), 'bad size'),
             ((1, 3, 8, -1, 2, 0, 3, 0), 'bad size'), ((1, 3, 8, 4, 0, 0, 3, 0), 'bad size'), ((65536, 0, 8, 4, 2, 0, 3, 0), 'bad size'),
             ((65536, 3, 8, 4, 2, 0, 3, 0), 'batch too large'), ((65536, 3, 8, 1 << 16, 1 << 15, 0, 2, 0), 'batch too large'),
             ((1, 3, 8, 1 << 16, 1 << 15, 0, 3, 0), 'list too long (m * k >= 2^31)'),
             ((1, 3, 8, 1 << 16, 1 << 15, 2, 2, 0), 'list too long (m * k >= 2^31)'),
             ((1, 3, 8, 4, 2, 0, 2, 0), 'channels out_c0 .. out_c0 + c - 1 are not inside out_c'),
             ((1, 3, 8, 4, 2, 0, 3, 1), 'channels out_c0 .. out_c0 + c - 1 are not inside out_c'),
             ((1, 3, 8, 4, 2, 0, 3, -1), 'channels out_c0 .. out_c0 + c - 1 are not inside out_c'),
             ((1, 3, 8, 4, 2, 2, 3, 1), 'channels out_c0 .. out_c0 + c - 1 are not inside out_c'),
             ((1, 3, 8, 4, 2, 2, 3, 0), 'point_major must be 0 or 1'), ((0, 3, 8, 0, 2, -1, 3, 0), 'point_major must be 0 or 1')]
    for (b, c, n, m, k, pm, out_c, out_c0), text in cases:
        assert c_status(L, L.pcc_group_points, b, c, n, m, k, pm, p, p, p, p, out_c, out_c0, None) == (EINVAL, 'group_points: ' + text)
        assert c_status(L, L.pcc_group_points_bwd, b, c, n, m, k, pm, p, p, out_c, out_c0, p, p, None) == \
            (EINVAL, 'group_points_bwd: ' + text)
    assert c_status(L, L.pcc_group_points, 1, 3, 8, 4, 2, 0, None, p, p, p, 3, 0, None) == (EINVAL, 'group_points: null pointer')
    assert c_status(L, L.pcc_group_points, 0, 3, 8, 4, 2, 0, None, None, None, None, 3, 0, None) == (0, '')  # (the error is cleared)
