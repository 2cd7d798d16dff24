"""The ``pointnet2_ops`` drop-in on CPU tensors against the numpy loops of ``tests/pointnet2_ops_reference.py``: every util
(indices exactly, values word for word, gradients exact on integer gradients with dyadic weights), dtypes, the two index
dtypes, the groupers, the modules' shapes and ``state_dict`` layout, and a small SA -> SA -> FP -> FP stack."""

import numpy as np
import pytest
import torch

import pointnet2_ops
from pointcloudcounterfactual_amd import neighbour_ops as ops
from pointnet2_ops import pointnet2_modules as pm
from pointnet2_ops import pointnet2_utils as pu
from tests import pointnet2_ops_reference as ref
from tests.pointnet2_ops_reference import RADIUS, T, index_lists, words


def test_version_and_names():
    assert pointnet2_ops.__version__ == '3.0.0'
    for fn, cls in ((pu.furthest_point_sample, pu.FurthestPointSampling), (pu.gather_operation, pu.GatherOperation),
                    (pu.three_nn, pu.ThreeNN), (pu.three_interpolate, pu.ThreeInterpolate),
                    (pu.grouping_operation, pu.GroupingOperation), (pu.ball_query, pu.BallQuery)):
        assert cls.apply is fn


@pytest.mark.parametrize('b,n,npoint', [(1, 1, 1), (2, 5, 5), (3, 64, 17), (1, 65, 65)])
def test_furthest_point_sample(b, n, npoint):
    xyz = ref.lattice_cloud(n, b, n)
    idx = pu.furthest_point_sample(T(xyz), npoint)
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (b, npoint) and not idx.requires_grad
    assert np.array_equal(idx.numpy(), ref.furthest_point_sample(xyz, npoint))
    assert (idx[:, 0] == 0).all()


def test_furthest_point_sample_skips_non_finite_and_ignores_grad():
    xyz = ref.lattice_cloud(3, 2, 9)
    xyz[0, 4, 1] = np.nan
    xyz[1, 7, 0] = np.inf
    t = T(xyz).requires_grad_(True)
    idx = pu.furthest_point_sample(t, 8)
    assert not idx.requires_grad
    assert np.array_equal(idx.numpy(), ref.furthest_point_sample(xyz, 8))
    assert 4 not in idx[0].tolist() and 7 not in idx[1].tolist()


def test_furthest_point_sample_npoint_above_n_raises():
    with pytest.raises(ValueError):
        pu.furthest_point_sample(T(ref.lattice_cloud(0, 2, 5)), 6)


@pytest.mark.parametrize('b,n,m,nsample', [(1, 1, 1, 1), (2, 5, 3, 8), (3, 64, 17, 8), (1, 65, 9, 33), (2, 64, 5, 1)])
def test_ball_query(b, n, m, nsample):
    xyz = ref.lattice_cloud(10 + n, b, n)
    new_xyz = xyz[:, :m].copy()
    new_xyz[:, -1] = 5.0  # a centre far outside the cloud: an empty ball
    idx = pu.ball_query(RADIUS, nsample, T(xyz), T(new_xyz).requires_grad_(True))
    assert idx.dtype == torch.int32 and tuple(idx.shape) == (b, m, nsample) and not idx.requires_grad
    assert np.array_equal(idx.numpy(), ref.ball_query(RADIUS, nsample, xyz, new_xyz))
    assert (idx[:, -1] == 0).all()


@pytest.mark.parametrize('b,n,m', [(1, 1, 1), (2, 5, 2), (3, 17, 3), (2, 33, 4), (1, 20, 100)])
def test_three_nn(b, n, m):
    unknown, known = ref.lattice_cloud(20 + n, b, n), ref.lattice_cloud(30 + m, b, m)
    dist, idx = pu.three_nn(T(unknown).requires_grad_(True), T(known).requires_grad_(True))
    assert dist.dtype == torch.float32 and idx.dtype == torch.int32
    assert tuple(dist.shape) == tuple(idx.shape) == (b, n, 3) and not dist.requires_grad and not idx.requires_grad
    rdist, ridx = ref.three_nn(unknown, known)
    assert np.array_equal(idx.numpy(), ridx)
    k = min(3, m)
    assert np.isposinf(dist.numpy()[..., k:]).all() and (idx.numpy()[..., k:] == 0).all()
    got, want = dist.numpy()[..., :k].astype(np.float64), rdist[..., :k]
    assert (np.abs(got - want) <= np.spacing(want.astype(np.float32))).all()  # within one ulp of the float64 root


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_gather_operation(dtype):
    b, c, n, m = 3, 5, 17, 23
    feats = ref.integer_features(1, b, c, n)
    idx = index_lists(2, b, n, m, 1)[:, :, 0]
    x = T(feats).requires_grad_(True)
    out = pu.gather_operation(x, T(idx).to(dtype))
    assert tuple(out.shape) == (b, c, m) and out.dtype == torch.float32
    assert np.array_equal(words(out), words(ref.gather_operation(feats, idx)))
    grad = ref.integer_features(3, b, c, m)
    out.backward(T(grad))
    assert np.array_equal(x.grad.numpy().astype(np.float64), ref.gather_operation_grad(grad, idx, n))


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_grouping_operation(dtype):
    b, c, n, m, k = 2, 4, 17, 9, 6
    feats = ref.integer_features(4, b, c, n)
    idx = index_lists(5, b, n, m, k)
    x = T(feats).requires_grad_(True)
    out = pu.grouping_operation(x, T(idx).to(dtype))
    assert tuple(out.shape) == (b, c, m, k)
    assert np.array_equal(words(out), words(ref.grouping_operation(feats, idx)))
    grad = ref.integer_features(6, b, c, m * k).reshape(b, c, m, k)
    out.backward(T(grad))
    assert np.array_equal(x.grad.numpy().astype(np.float64), ref.grouping_operation_grad(grad, idx, n))


@pytest.mark.parametrize('dtype', [torch.int32, torch.int64])
def test_three_interpolate(dtype):
    b, c, m, n = 2, 5, 7, 19
    feats = ref.integer_features(7, b, c, m)
    idx = index_lists(8, b, m, n, 3)
    weight = ref.dyadic_weights(9, b, n)
    x = T(feats).requires_grad_(True)
    w = T(weight).requires_grad_(True)
    out = pu.three_interpolate(x, T(idx).to(dtype), w)
    assert tuple(out.shape) == (b, c, n)
    assert np.array_equal(words(out), words(ref.three_interpolate(feats, idx, weight)))
    grad = ref.integer_features(10, b, c, n)
    out.backward(T(grad))
    assert np.array_equal(x.grad.numpy().astype(np.float64), ref.three_interpolate_grad(grad, idx, weight, m))
    assert w.grad is not None and tuple(w.grad.shape) == (b, n, 3)


def test_index_dtype_is_checked():
    with pytest.raises(TypeError):
        pu.grouping_operation(torch.zeros(1, 2, 3), torch.zeros(1, 2, 2))


def test_non_contiguous_inputs():
    b, n, m = 2, 33, 7
    xyz = ref.lattice_cloud(40, b, n)
    feats = ref.integer_features(41, b, 4, n)
    xyz_t = T(np.ascontiguousarray(xyz.transpose(0, 2, 1))).transpose(1, 2)      # [B,N,3] view
    feats_t = T(np.ascontiguousarray(feats.transpose(0, 2, 1))).transpose(1, 2)  # [B,C,N] view
    assert not xyz_t.is_contiguous() and not feats_t.is_contiguous()
    sel = pu.furthest_point_sample(xyz_t, m)
    assert np.array_equal(sel.numpy(), ref.furthest_point_sample(xyz, m))
    centres = pu.gather_operation(xyz_t.transpose(1, 2), sel).transpose(1, 2)  # not contiguous either
    idx = pu.ball_query(RADIUS, 8, xyz_t, centres)
    assert np.array_equal(idx.numpy(), ref.ball_query(RADIUS, 8, xyz, centres.numpy()))
    assert np.array_equal(words(pu.grouping_operation(feats_t, idx)), words(ref.grouping_operation(feats, idx.numpy())))


@pytest.mark.parametrize('use_xyz,with_features', [(True, True), (False, True), (True, False)])
def test_query_and_group_module(use_xyz, with_features):
    b, n, m, nsample, c = 2, 64, 9, 8, 3
    xyz = ref.lattice_cloud(50, b, n)
    new_xyz = xyz[:, :m].copy()
    new_xyz[:, -1] = 5.0
    feats = ref.integer_features(51, b, c, n) if with_features else None
    out = pu.QueryAndGroup(RADIUS, nsample, use_xyz=use_xyz)(T(xyz), T(new_xyz), None if feats is None else T(feats))
    want = ref.query_and_group(RADIUS, nsample, xyz, new_xyz, feats, use_xyz)
    assert tuple(out.shape) == (b, (3 if use_xyz else 0) + (c if with_features else 0), m, nsample)
    assert np.array_equal(words(out), words(want))


def test_groupers_need_something_to_group():
    xyz = T(ref.lattice_cloud(52, 1, 8))
    with pytest.raises(AssertionError):
        pu.QueryAndGroup(RADIUS, 4, use_xyz=False)(xyz, xyz[:, :2])
    with pytest.raises(AssertionError):
        pu.GroupAll(use_xyz=False)(xyz, None)


@pytest.mark.parametrize('use_xyz,with_features', [(True, True), (False, True), (True, False)])
def test_group_all(use_xyz, with_features):
    b, n, c = 2, 11, 4
    xyz = ref.lattice_cloud(53, b, n)
    feats = ref.integer_features(54, b, c, n) if with_features else None
    out = pu.GroupAll(use_xyz)(T(xyz), None, None if feats is None else T(feats))
    parts = ([xyz.transpose(0, 2, 1)] if use_xyz else []) + ([feats] if with_features else [])
    want = np.concatenate(parts, 1)[:, :, None, :]
    assert tuple(out.shape) == want.shape and np.array_equal(words(out), words(want))


def test_query_and_group_is_sample_and_groups_second_half():
    b, n, m, nsample = 2, 64, 9, 8
    xyz, feats = T(ref.lattice_cloud(60, b, n)), T(ref.integer_features(61, b, 5, n))
    sg = ops.sample_and_group(xyz, feats, m, RADIUS, nsample)
    for pad in ('first', 'none'):
        sgp = ops.sample_and_group(xyz, feats, m, RADIUS, nsample, pad=pad)
        qg = ops.query_and_group(xyz, sgp.centres, feats, RADIUS, nsample, pad=pad)
        assert torch.equal(qg.idx, sgp.idx) and torch.equal(qg.cnt, sgp.cnt)
        assert np.array_equal(words(qg.grouped), words(sgp.grouped))
    given = ops.query_and_group(xyz, sg.centres, feats, RADIUS, nsample, idx=sg.idx)  # a recorded list
    assert given.cnt is None and np.array_equal(words(given.grouped), words(sg.grouped))
    with pytest.raises(ValueError):
        ops.query_and_group(xyz, sg.centres, feats, RADIUS, nsample, idx=sg.idx[:, :, :-1])
    with pytest.raises(RuntimeError):
        ops.query_and_group(xyz, sg.centres, feats, RADIUS, nsample, idx=sg.idx.to(torch.int32))


def test_module_output_shapes():
    b, n, c = 2, 64, 4
    xyz, feats = T(ref.lattice_cloud(70, b, n)), T(ref.integer_features(71, b, c, n))
    new_xyz, out = pm.PointnetSAModule([c, 8, 16], npoint=9, radius=0.4, nsample=8)(xyz, feats)
    assert tuple(new_xyz.shape) == (b, 9, 3) and tuple(out.shape) == (b, 16, 9)
    new_xyz, out = pm.PointnetSAModuleMSG(7, [0.2, 0.4, 0.8], [4, 8, 16], [[c, 8], [c, 8, 12], [c, 4]])(xyz, feats)
    assert tuple(new_xyz.shape) == (b, 7, 3) and tuple(out.shape) == (b, 8 + 12 + 4, 7)
    new_xyz, out = pm.PointnetSAModule([c, 8, 16])(xyz, feats)  # npoint=None: GroupAll
    assert new_xyz is None and tuple(out.shape) == (b, 16, 1)
    new_xyz, out = pm.PointnetSAModule([0, 8], npoint=5, radius=0.4, nsample=4)(xyz, None)
    assert tuple(new_xyz.shape) == (b, 5, 3) and tuple(out.shape) == (b, 8, 5)
    new_xyz, out = pm.PointnetSAModule([c, 8], npoint=5, radius=0.4, nsample=4, use_xyz=False, bn=False)(xyz, feats)
    assert tuple(out.shape) == (b, 8, 5)
    known, known_feats = xyz[:, :9].contiguous(), T(ref.integer_features(72, b, 6, 9))
    out = pm.PointnetFPModule([6 + c, 16, 8])(xyz, known, feats, known_feats)
    assert tuple(out.shape) == (b, 8, n)
    out = pm.PointnetFPModule([6, 8])(xyz, known, None, known_feats)
    assert tuple(out.shape) == (b, 8, n)
    out = pm.PointnetFPModule([6 + c, 8])(xyz, None, feats, known_feats[:, :, :1])  # known=None: expanded to n
    assert tuple(out.shape) == (b, 8, n)


def test_state_dict_layout():
    """Key names and shapes of the original's modules, written out."""
    def layout(module):
        return [(k, tuple(v.shape)) for k, v in module.state_dict().items()]

    assert layout(pm.PointnetSAModuleMSG(8, [0.1, 0.2], [4, 8], [[5, 16, 32], [5, 8]])) == [
        ('mlps.0.0.weight', (16, 8, 1, 1)),
        ('mlps.0.1.weight', (16,)), ('mlps.0.1.bias', (16,)), ('mlps.0.1.running_mean', (16,)), ('mlps.0.1.running_var', (16,)),
        ('mlps.0.1.num_batches_tracked', ()),
        ('mlps.0.3.weight', (32, 16, 1, 1)),
        ('mlps.0.4.weight', (32,)), ('mlps.0.4.bias', (32,)), ('mlps.0.4.running_mean', (32,)), ('mlps.0.4.running_var', (32,)),
        ('mlps.0.4.num_batches_tracked', ()),
        ('mlps.1.0.weight', (8, 8, 1, 1)),
        ('mlps.1.1.weight', (8,)), ('mlps.1.1.bias', (8,)), ('mlps.1.1.running_mean', (8,)), ('mlps.1.1.running_var', (8,)),
        ('mlps.1.1.num_batches_tracked', ())]
    assert layout(pm.PointnetSAModule([5, 16], npoint=8, radius=0.1, nsample=4, bn=False, use_xyz=False)) == [
        ('mlps.0.0.weight', (16, 5, 1, 1)), ('mlps.0.0.bias', (16,))]
    assert layout(pm.PointnetSAModule([5, 16], bn=False)) == [('mlps.0.0.weight', (16, 8, 1, 1)), ('mlps.0.0.bias', (16,))]
    assert layout(pm.PointnetFPModule([20, 16, 8])) == [
        ('mlp.0.weight', (16, 20, 1, 1)),
        ('mlp.1.weight', (16,)), ('mlp.1.bias', (16,)), ('mlp.1.running_mean', (16,)), ('mlp.1.running_var', (16,)),
        ('mlp.1.num_batches_tracked', ()),
        ('mlp.3.weight', (8, 16, 1, 1)),
        ('mlp.4.weight', (8,)), ('mlp.4.bias', (8,)), ('mlp.4.running_mean', (8,)), ('mlp.4.running_var', (8,)),
        ('mlp.4.num_batches_tracked', ())]
    assert layout(pm.PointnetFPModule([20, 16], bn=False)) == [('mlp.0.weight', (16, 20, 1, 1)), ('mlp.0.bias', (16,))]
    assert [k for k, _ in layout(pm.build_shared_mlp([3, 4, 5]))][:7] == [
        '0.weight', '1.weight', '1.bias', '1.running_mean', '1.running_var', '1.num_batches_tracked', '3.weight']
    sa = pm.PointnetSAModule([5, 16], npoint=8, radius=0.1, nsample=4)
    assert isinstance(sa.groupers, torch.nn.ModuleList) and isinstance(sa.mlps, torch.nn.ModuleList)
    assert isinstance(sa.groupers[0], pu.QueryAndGroup) and isinstance(pm.PointnetSAModule([5, 16]).groupers[0], pu.GroupAll)


def test_stack_backward_reaches_every_parameter_and_the_features():
    torch.manual_seed(0)
    b, n, c = 2, 64, 4
    xyz = T(ref.lattice_cloud(80, b, n))
    feats = torch.randn(b, c, n, requires_grad=True)
    sa1 = pm.PointnetSAModule([c, 8, 8], npoint=16, radius=0.4, nsample=8)
    sa2 = pm.PointnetSAModuleMSG(4, [0.5, 0.9], [4, 8], [[8, 16], [8, 16]])
    fp2 = pm.PointnetFPModule([32 + 8, 16])
    fp1 = pm.PointnetFPModule([16 + c, 8])
    xyz1, f1 = sa1(xyz, feats)
    xyz2, f2 = sa2(xyz1, f1)
    up1 = fp2(xyz1, xyz2, f1, f2)
    out = fp1(xyz, xyz1, feats, up1)
    assert tuple(out.shape) == (b, 8, n)
    (out * torch.randn_like(out)).sum().backward()
    assert torch.isfinite(feats.grad).all() and float(feats.grad.abs().sum()) > 0
    for module in (sa1, sa2, fp2, fp1):
        for name, p in module.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().sum()) > 0, name
