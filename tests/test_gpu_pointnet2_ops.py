"""The ``pointnet2_ops`` drop-in on the accelerator: every util against the numpy loops of
``tests/pointnet2_ops_reference.py`` and, word for word, against the CPU path of the same call, at the smallest shapes at
which an adapter can go wrong; every module's forward and parameter gradients between the device and the CPU."""

import copy

import numpy as np
import pytest
import torch

from pointnet2_ops import pointnet2_modules as pm
from pointnet2_ops import pointnet2_utils as pu
from tests import pointnet2_ops_reference as ref
from tests.pointnet2_ops_reference import RADIUS, T, index_lists, words

pytestmark = pytest.mark.gpu

SIZES = [1, 5, 64, 65, 300]


def same_words(dev_t, cpu_t, want=None):
    """The device result equals the CPU path's words (dtype included) and, where given, the reference."""
    assert dev_t.dtype == cpu_t.dtype and tuple(dev_t.shape) == tuple(cpu_t.shape)
    if dev_t.is_floating_point():
        assert np.array_equal(words(dev_t), words(cpu_t))
        if want is not None:
            assert np.array_equal(words(dev_t), words(want))
    else:
        assert torch.equal(dev_t.cpu(), cpu_t)
        if want is not None:
            assert np.array_equal(dev_t.cpu().numpy(), want)


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('b', [1, 3])
def test_sample_and_query(cuda, b, n):
    """``furthest_point_sample`` for npoint in {1, 17, N} and, around those centres plus one far outside the cloud (an empty
    ball), ``ball_query`` and ``QueryAndGroup`` for nsample in {1, 8, 33}."""
    xyz = ref.lattice_cloud(100 + n, b, n)
    feats = ref.integer_features(200 + n, b, 4, n)
    xyz_d, feats_d = T(xyz).to(cuda), T(feats).to(cuda)
    full = ref.furthest_point_sample(xyz, n)  # (a greedy loop: its first npoint picks are the answer for npoint)
    for npoint in sorted({1, min(17, n), n}):
        sel = pu.furthest_point_sample(xyz_d, npoint)
        assert not sel.requires_grad
        same_words(sel, pu.furthest_point_sample(T(xyz), npoint), full[:, :npoint])
        new_xyz = np.concatenate((np.take_along_axis(xyz, full[:, :npoint, None].astype(np.int64), 1),
                                  np.full((b, 1, 3), 5.0, np.float32)), 1)
        new_d = T(new_xyz).to(cuda)
        same_words(pu.gather_operation(xyz_d.transpose(1, 2), sel).transpose(1, 2), T(new_xyz[:, :-1]))
        for nsample in (1, 8, 33):
            idx = pu.ball_query(RADIUS, nsample, xyz_d, new_d)
            assert not idx.requires_grad
            same_words(idx, pu.ball_query(RADIUS, nsample, T(xyz), T(new_xyz)), ref.ball_query(RADIUS, nsample, xyz, new_xyz))
            assert (idx[:, -1] == 0).all()
            grouper = pu.QueryAndGroup(RADIUS, nsample)
            same_words(grouper(xyz_d, new_d, feats_d), grouper(T(xyz), T(new_xyz), T(feats)),
                       ref.query_and_group(RADIUS, nsample, xyz, new_xyz, feats))
        grouper = pu.QueryAndGroup(RADIUS, 8, use_xyz=False)
        same_words(grouper(xyz_d, new_d, feats_d), grouper(T(xyz), T(new_xyz), T(feats)),
                   ref.query_and_group(RADIUS, 8, xyz, new_xyz, feats, use_xyz=False))
        grouper = pu.QueryAndGroup(RADIUS, 8)
        same_words(grouper(xyz_d, new_d), grouper(T(xyz), T(new_xyz)), ref.query_and_group(RADIUS, 8, xyz, new_xyz, None))
    with pytest.raises(ValueError):
        pu.furthest_point_sample(xyz_d, n + 1)
    both = pu.GroupAll()(xyz_d, None, feats_d)
    assert tuple(both.shape) == (b, 7, 1, n)
    same_words(both, pu.GroupAll()(T(xyz), None, T(feats)), np.concatenate((xyz.transpose(0, 2, 1), feats), 1)[:, :, None])


@pytest.mark.parametrize('m', [1, 2, 3, 4, 100])
@pytest.mark.parametrize('b', [1, 3])
def test_three_nn(cuda, b, m):
    for n in (1, 65):
        unknown, known = ref.lattice_cloud(300 + n, b, n), ref.lattice_cloud(400 + m, b, m)
        dist, idx = pu.three_nn(T(unknown).to(cuda), T(known).to(cuda))
        cdist, cidx = pu.three_nn(T(unknown), T(known))
        rdist, ridx = ref.three_nn(unknown, known)
        assert not dist.requires_grad and not idx.requires_grad
        same_words(idx, cidx, ridx)
        same_words(dist, cdist)
        k = min(3, m)
        assert np.isposinf(dist.cpu().numpy()[..., k:]).all()
        got, want = dist.cpu().numpy()[..., :k].astype(np.float64), rdist[..., :k]
        assert (np.abs(got - want) <= np.spacing(want.astype(np.float32))).all()


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('b', [1, 3])
def test_gathers(cuda, b, n):
    """``gather_operation`` and ``grouping_operation`` along lists with repeated and out-of-range entries, int32 and int64:
    forward word for word, the gradient exact on integer gradients."""
    c, m, k = 5, 19, 6
    feats = ref.integer_features(500 + n, b, c, n)
    idx = index_lists(600 + n, b, n, m, k)
    grad = ref.integer_features(700 + n, b, c, m * k).reshape(b, c, m, k)
    for dtype in (torch.int32, torch.int64):
        for fn, lst, g, fwd, bwd in ((pu.grouping_operation, idx, grad, ref.grouping_operation, ref.grouping_operation_grad),
                                     (pu.gather_operation, idx[:, :, 0], grad[..., 0], ref.gather_operation, ref.gather_operation_grad)):
            x_d = T(feats).to(cuda).requires_grad_(True)
            x_c = T(feats).requires_grad_(True)
            out_d, out_c = fn(x_d, T(lst).to(dtype).to(cuda)), fn(x_c, T(lst).to(dtype))
            same_words(out_d, out_c, fwd(feats, lst))
            out_d.backward(T(g).to(cuda))
            out_c.backward(T(g))
            assert np.array_equal(x_d.grad.cpu().numpy().astype(np.float64), bwd(g, lst, n))
            assert torch.equal(x_d.grad.cpu(), x_c.grad)


@pytest.mark.parametrize('m', [1, 2, 3, 4, 100])
@pytest.mark.parametrize('b', [1, 3])
def test_three_interpolate(cuda, b, m):
    c, n = 5, 65
    feats = ref.integer_features(800 + m, b, c, m)
    idx = index_lists(900 + m, b, m, n, 3)
    weight = ref.dyadic_weights(1000 + m, b, n)
    grad = ref.integer_features(1100 + m, b, c, n)
    for dtype in (torch.int32, torch.int64):
        x_d, w_d = T(feats).to(cuda).requires_grad_(True), T(weight).to(cuda).requires_grad_(True)
        x_c, w_c = T(feats).requires_grad_(True), T(weight).requires_grad_(True)
        out_d = pu.three_interpolate(x_d, T(idx).to(dtype).to(cuda), w_d)
        out_c = pu.three_interpolate(x_c, T(idx).to(dtype), w_c)
        same_words(out_d, out_c, ref.three_interpolate(feats, idx, weight))
        out_d.backward(T(grad).to(cuda))
        out_c.backward(T(grad))
        assert np.array_equal(x_d.grad.cpu().numpy().astype(np.float64), ref.three_interpolate_grad(grad, idx, weight, m))
        assert torch.equal(x_d.grad.cpu(), x_c.grad) and torch.equal(w_d.grad.cpu(), w_c.grad)


def _compare_modules(cuda, module, inputs, grad_inputs):
    """Forward, input gradients and parameter gradients of ``module`` on the device against the same module on the CPU.
    The bound is the one of the conv + BatchNorm + ReLU block in ``tests/test_gpu_harness.py``
    (``test_points_conv_fused_tail_matches_torch``)."""
    with torch.no_grad():
        for mod in module.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.5, 0.5)
    on_dev = copy.deepcopy(module).to(cuda)
    ins_c = [None if t is None else t.clone().requires_grad_(i in grad_inputs) for i, t in enumerate(inputs)]
    ins_d = [None if t is None else t.to(cuda).clone().requires_grad_(i in grad_inputs) for i, t in enumerate(inputs)]
    out_c, out_d = module(*ins_c), on_dev(*ins_d)
    if isinstance(out_c, tuple):  # the SA modules return (new_xyz, new_features); the centres are fixed by the lattice
        assert (out_c[0] is None and out_d[0] is None) or np.array_equal(words(out_d[0]), words(out_c[0]))
        out_c, out_d = out_c[1], out_d[1]
    torch.testing.assert_close(out_d.cpu(), out_c, rtol=1e-4, atol=1e-5)
    w = torch.randn_like(out_c)
    (out_c * w).sum().backward()
    (out_d * w.to(cuda)).sum().backward()
    for i in grad_inputs:
        torch.testing.assert_close(ins_d[i].grad.cpu(), ins_c[i].grad, rtol=1e-3, atol=1e-4)
    for (name, p_d), (_, p_c) in zip(on_dev.named_parameters(), module.named_parameters()):
        scale = float(p_c.grad.abs().max()) + 1e-6
        torch.testing.assert_close(p_d.grad.cpu(), p_c.grad, rtol=1e-3, atol=1e-4 * scale, msg=name)


@pytest.mark.parametrize('which', ['sa', 'msg', 'group_all', 'fp', 'fp_two_known'])
def test_modules_device_against_cpu(cuda, which):
    """Same parameters on both devices; the inputs are on the lattice, so the recorded farthest point samples, ball-query
    lists and three_nn lists are the same words on both (asserted first) and the dense layers see the same groups."""
    torch.manual_seed(5)
    b, n, c = 3, 65, 4
    xyz, feats, known_feats = T(ref.lattice_cloud(1200, b, n)), torch.randn(b, c, n), torch.randn(b, 6, 17)
    sel = pu.furthest_point_sample(xyz, 17)
    assert torch.equal(pu.furthest_point_sample(xyz.to(cuda), 17).cpu(), sel)
    centres = pu.gather_operation(xyz.transpose(1, 2), sel).transpose(1, 2).contiguous()
    if which in ('sa', 'msg'):
        for radius, nsample in ((0.25, 8), (0.5, 33)):
            assert torch.equal(pu.ball_query(radius, nsample, xyz.to(cuda), centres.to(cuda)).cpu(),
                               pu.ball_query(radius, nsample, xyz, centres))
    if which == 'sa':
        _compare_modules(cuda, pm.PointnetSAModule([c, 8, 16], npoint=17, radius=0.25, nsample=8), (xyz, feats), (1,))
    elif which == 'msg':
        _compare_modules(cuda, pm.PointnetSAModuleMSG(17, [0.25, 0.5], [8, 33], [[c, 8], [c, 8, 12]]), (xyz, feats), (1,))
    elif which == 'group_all':
        _compare_modules(cuda, pm.PointnetSAModule([c, 8, 16]), (xyz, feats), (1,))
    else:
        m = 17 if which == 'fp' else 2  # two known points: the third slot is (+inf, 0) and weighs 0
        known, known_feats = centres[:, :m].contiguous(), known_feats[:, :, :m].contiguous()
        assert torch.equal(pu.three_nn(xyz.to(cuda), known.to(cuda))[1].cpu(), pu.three_nn(xyz, known)[1])
        if which == 'fp':
            _compare_modules(cuda, pm.PointnetFPModule([6 + c, 16, 8]), (xyz, known, feats, known_feats), (2, 3))
        else:
            _compare_modules(cuda, pm.PointnetFPModule([6, 8], bn=False), (xyz, known, None, known_feats), (3,))
