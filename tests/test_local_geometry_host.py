"""CPU tests of ``neighbour_ops.local_covariance`` / ``local_geometry`` / ``estimate_normals``: the torch path of CPU tensors
against the numpy reference (tests/local_geometry_reference.py) -- ``mean`` and ``cov`` word for word, the eigen outputs
inside the contract's bars, the gradient against float64 autograd of the plain composition --, the contract's special
cases, the reference's fixture, the argument checks that need no device, and the pin of the ABI."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import local_geometry_reference as ref


def _words(t):
    return t.detach().numpy().view(np.uint32)


def _geometry(xyz, idx):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    return ops.local_geometry(torch.from_numpy(xyz), torch.from_numpy(idx))


@pytest.mark.parametrize('n', ref.N_GRID)
def test_cpu_path_mean_and_cov_word_for_word(n):
    """The grid of the GPU test, about a tenth of the slots -1, n or 2^40; the eigen outputs of the same calls inside the
    bars and under the conventions."""
    xyz_all = ref.cloud(n, n)
    j = 0
    for m in ref.M_GRID:
        for k in ref.K_GRID:
            b = (1, 3)[j % 2]
            j += 1
            idx = ref.random_list(31 * m + k + n, ref.B_MAX, n, m, k)[:b]
            xyz = xyz_all[:b]
            got = _geometry(xyz, idx)
            assert got._fields == ('mean', 'cov', 'eigenvalues', 'eigenvectors', 'curvature')
            assert got.mean.shape == (b, m, 3) and got.cov.shape == (b, m, 3, 3) and got.curvature.shape == (b, m)
            mean, cov = ref.mean_cov(xyz, idx)
            assert np.array_equal(_words(got.mean), mean.view(np.uint32)), (m, k, b)
            assert np.array_equal(_words(got.cov), cov.view(np.uint32)), (m, k, b)
            val, vec, curv = (t.numpy() for t in got[2:])
            ref.EigenBars(cov).check(val, vec, curv)
            ref.check_conventions(cov, val, vec, curv)


def test_cpu_path_eigen_outputs_are_inside_the_bars():
    for name, (xyz, idx) in ref.accuracy_cases().items():
        got = _geometry(xyz, idx)
        cov = got.cov.numpy()
        assert np.array_equal(cov.view(np.uint32), ref.mean_cov(xyz, idx)[1].view(np.uint32)), name
        ref.EigenBars(cov).check(*(t.numpy() for t in got[2:]))
        ref.check_conventions(cov, *(t.numpy() for t in got[2:]))


@pytest.mark.parametrize('use_mean', [False, True])
def test_gradient_against_float64_autograd_of_the_plain_composition(use_mean):
    """The plain composition: gather, mean over the valid slots, differences, one einsum -- in float64.  The float32 path
    sums, per bin, deg terms that are each made of at most 2 k + 8 rounded operations (the slot sums of the mean and of the
    matrix, both passes of autograd) on quantities of size |Gs| (|x| + |mean|) and |grad_mean| / cnt: the bound is
    (deg + 2 k + 8) * U times the sum of those sizes over the slots that reach the bin."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    rng = np.random.default_rng(3)
    for n, m, k, b in ((65, 257, 5, 3), (300, 64, 16, 2), (3, 33, 33, 1), (1025, 65, 3, 2)):
        xyz, idx = ref.cloud(n, n, b, shift=0.5), ref.random_list(n + k, b, n, m, k)
        gc = rng.standard_normal((b, m, 3, 3)).astype(np.float32)
        gmean = rng.standard_normal((b, m, 3)).astype(np.float32)
        x32 = torch.from_numpy(xyz).requires_grad_(True)
        cov, mean = ops.local_covariance(x32, torch.from_numpy(idx), return_mean=True)
        assert cov.requires_grad and mean.requires_grad
        loss = (cov * torch.from_numpy(gc)).sum() + ((mean * torch.from_numpy(gmean)).sum() if use_mean else 0)
        loss.backward()
        # float64, written plainly
        x64 = torch.from_numpy(xyz).double().requires_grad_(True)
        valid = torch.from_numpy((idx >= 0) & (idx < n))
        safe = torch.from_numpy(np.where((idx >= 0) & (idx < n), idx, 0))
        pts = x64[torch.arange(b)[:, None, None], safe] * valid[..., None]
        cnt = valid.sum(-1).clamp(min=1)[..., None]
        mean64 = pts.sum(2) / cnt
        d = (pts - mean64[:, :, None, :]) * valid[..., None]
        cov64 = torch.einsum('bmja,bmjc->bmac', d, d)
        loss64 = (cov64 * torch.from_numpy(gc).double()).sum() + ((mean64 * torch.from_numpy(gmean).double()).sum() if use_mean else 0)
        loss64.backward()
        gs = np.abs(gc + gc.transpose(0, 1, 3, 2)).astype(np.float64)                                 # [B,M,a,c]
        size = np.abs(pts.detach().numpy()) + np.abs(mean64.detach().numpy())[:, :, None, :]       # [B,M,k,c]
        per_slot = np.einsum('bmac,bmjc->bmja', gs, size) + (np.abs(gmean)[:, :, None, :] / cnt.numpy()[:, :, None] if use_mean else 0)
        scale, deg = np.zeros((b, n, 3)), np.zeros((b, n))
        for bi in range(b):
            ok = valid[bi].numpy()
            np.add.at(scale[bi], idx[bi][ok], per_slot[bi][ok])
            np.add.at(deg[bi], idx[bi][ok], 1)
        err = np.abs(x32.grad.numpy() - x64.grad.numpy())
        assert (err <= (deg + 2 * k + 8)[:, :, None] * ref.U * scale).all(), (n, m, k)
        assert (x32.grad.numpy()[deg == 0] == 0).all()


def test_special_cases():
    """cnt = 0, cnt = 1, all slots equal, -1 / n / 2^40 indices, a NaN coordinate."""
    nan = float('nan')
    xyz = np.array([[[1.0, 2.0, 3.0], [4.0, 6.0, 8.0], [nan, 0.0, 0.0], [-1.0, 0.5, 0.25]]], dtype=np.float32)
    idx = np.array([[[-1, 4, 1 << 40, -7],       # cnt = 0
                     [1, -1, 4, 1 << 40],        # cnt = 1
                     [3, 3, 3, 3],               # all slots equal
                     [0, 1, -1, 4],              # two points: rank one
                     [0, 2, 1, 3],               # a NaN coordinate
                     [0, 1, 3, 4]]], dtype=np.int64)
    got = _geometry(xyz, idx)
    mean, cov, val, vec, curv = (t.numpy()[0] for t in got)
    eye = np.eye(3, dtype=np.float32)
    assert (mean[0].view(np.uint32) == 0).all() and np.array_equal(mean[1], xyz[0, 1]) and np.array_equal(mean[2], xyz[0, 3])
    for r in (0, 1, 2):
        assert (cov[r].view(np.uint32) == 0).all() and (val[r].view(np.uint32) == 0).all() and curv[r].view(np.uint32) == 0
        assert np.array_equal(vec[r].view(np.uint32), eye.view(np.uint32))
    assert np.array_equal(mean[3], np.array([2.5, 4.0, 5.5], dtype=np.float32))
    half = np.array([1.5, 2.0, 2.5])
    assert np.array_equal(cov[3], (2 * np.outer(half, half)).astype(np.float32))
    assert abs(val[3][2] - 2 * half @ half) < 1e-5 and np.abs(val[3][:2]).max() < 1e-5 and curv[3] < 1e-6
    assert np.allclose(vec[3][2], half / np.linalg.norm(half), atol=1e-6)
    assert mean[4].view(np.uint32)[0] == ref.NAN_WORD and np.array_equal(mean[4][1:], np.array([2.125, 2.8125], dtype=np.float32))
    assert (cov[4][0].view(np.uint32) == ref.NAN_WORD).all() and (cov[4][:, 0].view(np.uint32) == ref.NAN_WORD).all()
    assert np.isfinite(cov[4][1:, 1:]).all()
    for a in (val[4], vec[4], curv[4]):
        assert (a.view(np.uint32) == ref.NAN_WORD).all()
    assert np.isfinite(val[5]).all() and np.isfinite(vec[5]).all()
    want_mean, want_cov = ref.mean_cov(xyz, idx)
    assert np.array_equal(got.mean.numpy().view(np.uint32), want_mean.view(np.uint32))
    assert np.array_equal(got.cov.numpy().view(np.uint32), want_cov.view(np.uint32))
    ref.check_conventions(cov, val, vec, curv)


def test_a_plane_returns_its_normal_exactly():
    """The plane z = 0.25: the z axis is decoupled, so the normal is exactly (0, 0, 1), eval0 = +0.0 and curv = +0.0."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    rng = np.random.default_rng(9)
    xyz = rng.random((2, 200, 3)).astype(np.float32)
    xyz[:, :, 2] = 0.25
    t = torch.from_numpy(xyz)
    got = ops.local_geometry(t, ops.knn(t.transpose(1, 2).contiguous(), 16))
    normal = got.eigenvectors[:, :, 0].numpy()
    assert np.array_equal(normal.view(np.uint32), np.broadcast_to(np.array([0, 0, 1], dtype=np.float32), normal.shape).view(np.uint32))
    assert (got.eigenvalues[:, :, 0].numpy().view(np.uint32) == 0).all() and (got.curvature.numpy().view(np.uint32) == 0).all()
    assert (got.eigenvalues[:, :, 1] > 0).all()
    assert torch.equal(ops.estimate_normals(t, 16), got.eigenvectors[:, :, 0])


def test_estimate_normals_orients_towards_a_viewpoint():
    from pointcloudcounterfactual_amd import estimate_normals, neighbour_ops as ops

    assert estimate_normals is ops.estimate_normals
    p = torch.from_numpy(ref.sphere(4, 400))[None].repeat(2, 1, 1)
    outward, curv = ops.estimate_normals(p, 12, viewpoint=torch.tensor([[0.0, 0.0, 0.0], [0.0, 0.0, 9.0]]), return_curvature=True)
    assert outward.shape == (2, 400, 3) and curv.shape == (2, 400)
    assert ((outward[0] * p[0]).sum(-1) < -0.9).all()             # seen from the centre: inward
    towards = torch.tensor([0.0, 0.0, 9.0]) - p[1]
    assert ((outward[1] * towards).sum(-1) >= 0).all()
    assert ((outward * p).sum(-1).abs() > 0.9).all() and torch.allclose(outward.norm(dim=-1), torch.ones(2, 400), atol=1e-5)
    plain = ops.estimate_normals(p, 12)
    assert torch.equal(plain.abs(), outward.abs())
    one = ops.estimate_normals(p, 12, viewpoint=torch.tensor([0.0, 0.0, 9.0]))
    assert torch.equal(one[1], outward[1])
    idx = ops.knn(p.transpose(1, 2).contiguous(), 12)[:, :50]
    assert torch.equal(ops.estimate_normals(p, idx=idx), plain[:, :50])
    assert ops.estimate_normals(p[:, :5], 16).shape == (2, 5, 3)  # k > N: min(k, N) neighbours
    for bad in (torch.zeros(2), torch.zeros(3, 3), torch.zeros(1, 3)):
        with pytest.raises(ValueError):
            ops.estimate_normals(p, 12, viewpoint=bad)
    for k in (0, 129, 2.0, True):
        with pytest.raises(ValueError):
            ops.estimate_normals(p, k)


def test_local_covariance_reproduces_the_reference_fixture():
    """``cov_out[:, 3:]`` of tests/golden/ref_neighbour_ops.npz (the reference's get_local_covariance, k = 16, 2 x 150
    points) along the k-NN list, inside the bar of test_get_local_covariance_vs_reference_fixture."""
    from pointcloudcounterfactual_amd import local_covariance, neighbour_ops as ops

    assert local_covariance is ops.local_covariance
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_neighbour_ops.npz'))
    x, k = z['cov_x'], int(z['cov_k'])  # [2,3,150]
    xyz = np.ascontiguousarray(x.transpose(0, 2, 1))
    idx = np.stack([ref.brute_knn(c, k) for c in xyz])
    cov = ops.local_covariance(torch.from_numpy(xyz), torch.from_numpy(idx)).numpy()
    want = z['cov_out'][:, 3:].transpose(0, 2, 1).reshape(2, 150, 3, 3)
    np.testing.assert_allclose(cov, want, rtol=1e-4, atol=2e-5)


def test_views_exports_and_argument_errors():
    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for name in ('local_covariance', 'local_geometry', 'estimate_normals'):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(ops, name)
    xyz = torch.from_numpy(ref.cloud(3, 40, 2))
    idx = torch.from_numpy(ref.random_list(4, 2, 20, 7, 6))
    view, iview = xyz[:, ::2], idx[:, :, ::2]
    assert not view.is_contiguous() and not iview.is_contiguous()
    assert torch.equal(ops.local_covariance(view, iview), ops.local_covariance(view.contiguous(), iview.contiguous()))
    cov, mean = ops.local_covariance(xyz, idx, return_mean=True)
    assert cov.shape == (2, 7, 3, 3) and mean.shape == (2, 7, 3) and not cov.requires_grad
    geo = ops.local_geometry(xyz.clone().requires_grad_(True), idx)
    assert geo.cov.requires_grad and geo.mean.requires_grad
    assert not geo.eigenvalues.requires_grad and not geo.eigenvectors.requires_grad and not geo.curvature.requires_grad
    for eb, em in ((0, 7), (2, 0)):
        empty = ops.local_geometry(xyz[:eb], idx[:eb, :em])
        assert empty.cov.shape == (eb, em, 3, 3) and empty.eigenvectors.shape == (eb, em, 3, 3) and empty.curvature.shape == (eb, em)
    for fn in (ops.local_covariance, ops.local_geometry):
        for bx, bi in ((xyz[0], idx), (xyz[:, :, :2], idx), (xyz[:, :0], idx), (xyz, idx[0]), (xyz, idx[:1]), (xyz, idx[:, :, :0])):
            with pytest.raises(ValueError):
                fn(bx, bi)
        for bx, bi, name in ((xyz.double(), idx, 'xyz'), (xyz, idx.int(), 'idx'), (xyz, idx.float(), 'idx')):
            with pytest.raises(RuntimeError, match=f'{name} must be torch'):
                fn(bx, bi)
        with pytest.raises(RuntimeError, match='expected cpu'):
            fn(xyz, idx.to('meta'))


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued (no stream, no device memory is touched: the guard stays)."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    buf = (ctypes.c_char * 128)(*([0x5a] * 128))
    p = ctypes.addressof(buf)
    EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
    # (b, n, m, k)
    good = (1, 8, 4, 2)
    bad = [(-1, 8, 4, 2), (65536, 8, 4, 2), (1, 0, 4, 2), (1, -1, 4, 2), (1, 8, -1, 2), (1, 8, 4, 0), (1, 8, 1 << 16, 1 << 15),
           (0, 8, 4, 0), (1, 0, 0, 2)]  # (an empty call is still checked)
    for s in bad:
        assert L.pcc_local_geometry(*s, p, p, p, p, p, p, p, None) == EINVAL, s
        assert L.pcc_last_error().decode().startswith('local_geometry:') and L.pcc_last_status() == EINVAL
        assert L.pcc_local_covariance_bwd(*s, p, p, p, p, p, p, None) == EINVAL, s
        assert L.pcc_last_error().decode().startswith('local_covariance_bwd:')
    for xyz, idx in ((None, p), (p, None)):
        assert L.pcc_local_geometry(*good, xyz, idx, p, p, p, p, p, None) == EINVAL
        assert L.pcc_last_error().decode().startswith('local_geometry: null pointer')
        assert L.pcc_local_geometry(*good, xyz, idx, None, None, None, None, p, None) == EINVAL
    for xyz, idx, mean, gc in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert L.pcc_local_covariance_bwd(*good, xyz, idx, mean, gc, p, p, None) == EINVAL
        assert L.pcc_last_error().decode().startswith('local_covariance_bwd: null pointer')
        assert L.pcc_local_covariance_bwd(*good, xyz, idx, mean, gc, None, p, None) == EINVAL  # (grad_mean may be null, these may not)
    # nothing to do: an empty batch, an empty list, no output asked for
    b, n, m, k = good
    assert L.pcc_local_geometry(0, n, m, k, None, None, p, p, p, p, p, None) == 0
    assert L.pcc_local_geometry(b, n, 0, k, None, None, p, p, p, p, p, None) == 0
    assert L.pcc_local_geometry(b, n, m, k, p, p, None, None, None, None, None, None) == 0
    assert L.pcc_local_covariance_bwd(0, n, m, k, None, None, None, None, None, p, None) == 0
    assert L.pcc_local_covariance_bwd(b, n, m, k, p, p, p, p, p, None, None) == 0
    assert L.pcc_last_status() == 0
    assert bytes(buf) == b'\x5a' * 128


def test_the_abi_is_bound_and_no_tuning_key_was_added():
    from pointcloudcounterfactual_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'pcc_neighbour.h')).read()
    assert re.search(r'int pcc_local_geometry\(int b, int n, int m, int k, const float \*xyz, const int64_t \*idx, float \*mean, float \*cov,\s+'
                     r'float \*eval, float \*evec, float \*curv, pcc_stream_t stream\);', header)
    assert re.search(r'int pcc_local_covariance_bwd\(int b, int n, int m, int k, const float \*xyz, const int64_t \*idx, const float \*mean,\s+'
                     r'const float \*grad_cov, const float \*grad_mean, float \*grad_xyz, pcc_stream_t stream\);', header)
    assert len(_lib.ABI['pcc_local_geometry'][1]) == 12 and len(_lib.ABI['pcc_local_covariance_bwd'][1]) == 11
    assert re.search(r'PCC_TUNE_KEYS = 16\b', open(os.path.join(root, 'include', 'pcc_test_hooks.h')).read())
    assert max(_lib.TUNING.values()) == 15


def test_messages_word_for_word():
    """Every refusal ``local_covariance`` / ``local_geometry`` / ``estimate_normals`` and ``pcc_local_geometry`` /
    ``pcc_local_covariance_bwd`` share with the other list ops, in their words and in the order in which a call with several
    bad arguments reports them."""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import c_status, raised

    xyz, idx = torch.zeros(2, 20, 3), torch.zeros(2, 7, 6, dtype=torch.int64)
    huge = torch.zeros(2, 1 << 16, 1 << 15, dtype=torch.int64, device='meta')
    val = [((xyz[0], idx), 'expected xyz[B,N,3] with N >= 1, got (20, 3)'),
           ((xyz[:, :, :2], idx[:1]), 'expected xyz[B,N,3] with N >= 1, got (2, 20, 2)'),
           ((xyz[:, :0], idx), 'expected xyz[B,N,3] with N >= 1, got (2, 0, 3)'),
           ((xyz, idx[0]), 'expected idx[B = 2,M,k] with k >= 1, got (7, 6)'),
           ((xyz, idx[:1]), 'expected idx[B = 2,M,k] with k >= 1, got (1, 7, 6)'),
           ((xyz.double(), idx.int()[:, :, :0]), 'expected idx[B = 2,M,k] with k >= 1, got (2, 7, 0)'),  # (shapes before dtypes)
           ((xyz, huge), 'idx[B,M,k] with M * k >= 2^31, got (2, 65536, 32768)')]
    for what, fn in (('local_covariance', ops.local_covariance), ('local_geometry', ops.local_geometry)):
        for args, text in val:
            assert raised(ValueError, fn, *args) == f'{what}: {text}'
        assert raised(RuntimeError, fn, xyz, idx.int()) == 'idx must be torch.int64, found torch.int32'
        assert raised(RuntimeError, fn, xyz.double(), idx.int()) == 'xyz must be torch.float32, found torch.float64'
        assert raised(RuntimeError, fn, xyz, idx.int().to('meta')) == 'idx must be torch.int64, found torch.int32'
        assert raised(RuntimeError, fn, xyz, idx.to('meta')) == 'idx is on meta, expected cpu'
    for bad, shown in ((xyz[0], '(20, 3)'), (xyz[:, :, :2], '(2, 20, 2)'), (xyz[:, :0], '(2, 0, 3)')):
        assert raised(ValueError, ops.estimate_normals, bad, k='x') == f'estimate_normals: expected xyz[B,N,3] with N >= 1, got {shown}'
    for k, shown in ((0, '0'), (129, '129'), (2.0, '2.0'), (True, 'True'), (None, 'None')):
        assert raised(ValueError, ops.estimate_normals, xyz.double(), k=k) == \
            f'estimate_normals: k must be an integer in [1, 128], got {shown}'  # (k before the dtype)
    assert raised(RuntimeError, ops.estimate_normals, xyz.double()) == 'xyz must be torch.float32, found torch.float64'
    assert raised(ValueError, ops.estimate_normals, xyz, k=0, idx=idx[:1]) == \
        'local_geometry: expected idx[B = 2,M,k] with k >= 1, got (1, 7, 6)'  # (k is not looked at beside a list)

    L = _lib.lib
    buf = (ctypes.c_char * 128)()
    p = ctypes.addressof(buf)
    EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
    # (b, n, m, k): the first refusal in the order of the checks wins
    cases = [((-1, 8, 4, 2), 'bad size'), ((1, 0, 4, 2), 'bad size'), ((1, -1, 4, 2), 'bad size'), ((1, 8, -1, 2), 'bad size'),
             ((1, 8, 4, 0), 'bad size'), ((0, 8, 4, 0), 'bad size'), ((1, 0, 0, 2), 'bad size'), ((65536, 0, 4, 2), 'bad size'),
             ((65536, 8, 4, 2), 'batch too large'), ((65536, 8, 1 << 16, 1 << 15), 'batch too large'),
             ((1, 8, 1 << 16, 1 << 15), 'list too long (m * k >= 2^31)'), ((0, 8, 1 << 16, 1 << 15), 'list too long (m * k >= 2^31)')]
    for s, text in cases:
        assert c_status(L, L.pcc_local_geometry, *s, p, p, p, p, p, p, p, None) == (EINVAL, 'local_geometry: ' + text)
        assert c_status(L, L.pcc_local_covariance_bwd, *s, p, p, p, p, p, p, None) == (EINVAL, 'local_covariance_bwd: ' + text)
    assert c_status(L, L.pcc_local_geometry, 1, 8, 4, 2, None, p, p, p, p, p, p, None) == (EINVAL, 'local_geometry: null pointer')
    assert c_status(L, L.pcc_local_geometry, 0, 8, 4, 2, None, None, p, p, p, p, p, None) == (0, '')  # (the error is cleared)
