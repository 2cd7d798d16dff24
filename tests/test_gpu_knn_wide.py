"""GPU tests of the wide k-NN path (knn_wide.hip): k up to 128 and any channel count, bit-identical to the oracle's
difference-form (c <= 3) and expanded-form (c >= 4) lists, and the same lists as the existing kernels where both run."""

import numpy as np
import pytest
import torch

# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu


def _cloud(seed, b, c, n, kind='normal'):
    g = torch.Generator().manual_seed(seed)
    if kind == 'uniform':
        return torch.rand(b, c, n, generator=g).contiguous()
    x = torch.randn(b, c, n, generator=g)
    if kind == 'sphere':
        x = x / x.norm(dim=1, keepdim=True)
    return x.contiguous()


def _knn(x, k, cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    return ops.knn(x.to(cuda), k).cpu().numpy()


@pytest.mark.parametrize('b,c,n,stride', [(2, 3, 257, 1), (1, 3, 2048, 1), (2, 3, 2100, 1), (3, 1, 300, 1), (2, 2, 333, 1),
                                          (1, 3, 17000, 97)])
@pytest.mark.parametrize('k', [33, 40, 64, 100, 128])
def test_knn_wide_small_c(cuda, oracle_mod, b, c, n, stride, k):
    kind = ('normal', 'uniform', 'sphere')[(n + k) % 3] if c == 3 else ('normal', 'uniform')[(n + k) % 2]
    x = _cloud(n * 7 + k, b, c, n, kind)
    idx = _knn(x, k, cuda)
    exp = oracle_mod.knn_diff(x.numpy(), k, stride)
    assert np.array_equal(idx[:, ::stride], exp[:, ::stride])


@pytest.mark.parametrize('n,k', [(40, 40), (128, 128)])
def test_knn_wide_k_equals_n(cuda, oracle_mod, n, k):
    for c in (3, 8):
        x = _cloud(n + c, 2, c, n)
        exp = oracle_mod.knn_diff(x.numpy(), k) if c <= 3 else oracle_mod.knn_expanded(x.numpy(), k)
        assert np.array_equal(_knn(x, k, cuda), exp), c


@pytest.mark.parametrize('c', [4, 17, 64, 128])
@pytest.mark.parametrize('n', [200, 1000, 2050])
def test_knn_wide_expanded(cuda, oracle_mod, c, n):
    x = _cloud(c * 31 + n, 2, c, n)
    exp = oracle_mod.knn_expanded(x.numpy(), 128)  # (the first k of the sorted lists: every k at once)
    for k in (33, 40, 64, 128):
        assert np.array_equal(_knn(x, k, cuda), exp[:, :, :k]), k


@pytest.mark.parametrize('c,n', [(129, 300), (130, 1000), (200, 777), (256, 2048), (512, 1024)])
def test_knn_wide_many_channels(cuda, oracle_mod, c, n):
    """c > 128: the channels stream through LDS in chunks, one accumulator carried across them (odd c, c not a multiple
    of the chunk, several chunks)."""
    b = 1 if n >= 2048 or c >= 512 else 2
    x = _cloud(c + n, b, c, n, 'uniform' if c % 2 else 'normal')
    exp = oracle_mod.knn_expanded(x.numpy(), 128)
    for k in (4, 20, 25, 40, 128):
        assert np.array_equal(_knn(x, k, cuda), exp[:, :, :k]), k


def test_knn_wide_adversarial_orders(cuda, oracle_mod):
    """Distances descending along the index (every candidate displaces an entry), ascending, and ten-fold exact ties."""
    n = 700
    t = torch.linspace(0, 1, n)
    line5 = torch.stack([t, 2 * t, -t, 0.5 * t, t * t], 0)[None]
    line3 = line5[:, :3]
    for line, k, oracle in ((line5, 64, oracle_mod.knn_expanded), (line3, 48, oracle_mod.knn_diff)):
        c = line.shape[1]
        ties = torch.cat([_cloud(11 + c, 1, c, 70)] * 10, dim=2)
        for x in (line, line.flip(2), ties, torch.cat([line, line.flip(2), ties], 0)):
            x = x.contiguous()
            assert np.array_equal(_knn(x, k, cuda), oracle(x.numpy(), k)), (c, k)


def test_knn_wide_degenerate_clouds(cuda, oracle_mod):
    from pointcloudcounterfactual_amd import _lib

    for c in (3, 64):
        same = torch.full((2, c, 100), 0.25)
        assert (_knn(same, 40, cuda) == np.arange(40)[None, None, :]).all(), c
    one = torch.rand(3, 3, 1)
    from tests import knn_reference as kr
    from tests.which_ran import assert_only, ran

    with _lib.tuning('knn_wide', 1):  # (n = 1 launches too: the selection kernel, and the distance kernel where c > 3)
        got, names = ran(lambda: _knn(one, 1, cuda))
        assert_only(names, kr.wide_select(3, 1), *kr.FAMILIES)
        assert (got == 0).all()
        got, names = ran(lambda: _knn(torch.rand(2, 9, 1), 1, cuda))
        assert_only(names, {kr.wide_select(9, 1), 'knn_wide_dist_kernel'}, *kr.FAMILIES)
        assert (got == 0).all()
    for c, oracle in ((3, oracle_mod.knn_diff), (200, oracle_mod.knn_expanded)):
        x = _cloud(5 + c, 2, c, 200)
        x[0, 1, 17] = float('nan')
        x[1, 0, 3] = float('inf')
        idx = _knn(x, 40, cuda)
        assert idx.min() >= 0 and idx.max() < 200
        ok = np.ones(200, bool)
        ok[17] = False
        assert not (idx[0, ok] == 17).any()
        clean = torch.cat([x[0, :, :17], x[0, :, 18:]], dim=1)[None]
        ref = oracle(clean.numpy(), 40)[0]
        ref = ref + (ref >= 17)
        assert np.array_equal(idx[0, ok], ref), c


@pytest.mark.parametrize('b,c,n,k', [(2, 3, 1000, 4), (2, 3, 777, 20), (1, 3, 3000, 25), (32, 3, 2048, 32), (2, 64, 500, 25),
                                       (32, 64, 2048, 20), (2, 128, 300, 32), (1, 128, 2048, 4), (3, 1, 100, 8)])
def test_knn_wide_switch_matches_the_existing_kernels(cuda, b, c, n, k):
    """The test switch sends calls the existing kernels handle through the wide path: the same bits."""
    from pointcloudcounterfactual_amd import _lib

    from tests import knn_reference as kr
    from tests.which_ran import assert_only, ran

    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    x = _cloud(b * 13 + c + n + k, b, c, n)
    ref, names = ran(lambda: _knn(x, k, cuda))
    assert_only(names, kr.kernel_of(b, c, n, k, cus), *kr.FAMILIES)  # (the kernel of the size, none of the wide path)
    with _lib.tuning('knn_wide', 1):
        got, names = ran(lambda: _knn(x, k, cuda))
    assert_only(names, {kr.wide_select(c, k)} | ({'knn_wide_dist_kernel'} if c > 3 else set()), *kr.FAMILIES)
    assert np.array_equal(got, ref)


def test_knn_wide_graph_features_and_max_pool(cuda, oracle_mod):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x = _cloud(3, 2, 64, 300)
    idx, feat = ops.get_graph_features(x.to(cuda), torch.empty(0), k=40)
    idx = idx.cpu()
    assert np.array_equal(idx.numpy(), oracle_mod.knn_expanded(x.numpy(), 40))
    nb = torch.stack([x[s][:, idx[s]] for s in range(2)])  # [B,C,N,k]
    xe = x.unsqueeze(3).expand(-1, -1, -1, 40)
    assert torch.equal(feat.cpu(), torch.cat([nb - xe, xe], dim=1))

    y = _cloud(4, 2, 256, 400)
    pooled = ops.graph_max_pooling(y.to(cuda), torch.empty(0), k=40).cpu()
    ref_idx = torch.from_numpy(oracle_mod.knn_expanded(y.numpy(), 40))
    ref = torch.stack([y[s][:, ref_idx[s]] for s in range(2)]).max(dim=-1)[0]
    assert torch.equal(pooled, ref)


def test_knn_wide_argkmin_and_graph_filtering(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from pykeops.torch import LazyTensor  # (the shim package of this repository)

    x = _cloud(8, 2, 3, 500).to(cuda)
    pts = x.transpose(1, 2).contiguous()
    d = ((LazyTensor(pts[:, :, None, :]) - LazyTensor(pts[:, None, :, :])) ** 2).sum(-1)
    assert torch.equal(d.argKmin(40, dim=2), ops.hip_knn(x, 40))
    out = ops.graph_filtering(x, k=40)
    assert out.shape == x.shape and torch.isfinite(out).all()


def test_knn_wide_dgcnn_classifier_k40(cuda):
    from pointcloudcounterfactual_amd import harness

    torch.manual_seed(0)
    model = harness.DGCNNClassifier(k=40).to(cuda)
    cloud = torch.randn(4, 512, 3, device=cuda, requires_grad=True)  # [B,N,3], as the encoder takes it
    out = model(cloud)
    out.sum().backward()
    assert torch.isfinite(out).all()
    assert torch.isfinite(cloud.grad).all()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


def test_knn_wide_side_stream(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for c, k in ((3, 64), (200, 40)):
        x = _cloud(21 + c, 4, c, 1500).to(cuda)
        ref = ops.hip_knn(x, k)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = ops.hip_knn(x, k)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert torch.equal(got, ref), c
