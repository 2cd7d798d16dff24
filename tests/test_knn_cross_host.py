"""CPU tests of the k-NN between two clouds: the torch path of ``knn_cross`` against float64 brute force, and the
argument checks that run before anything reaches the accelerator."""

import numpy as np
import pytest
import torch

EPS32 = float(np.finfo(np.float32).eps)


def _certified(got, d64, k, c, qn, xn):
    """``got[B,Nq,k]`` equals the float64 list, or differs from it only in certified near ties: the float64 distances of
    the two entries differ by at most 4 (c + 2) eps32 (|q|^2 + |x|^2).  Returns the fraction of entries excused."""
    exp = d64.topk(k, largest=False)[1]
    dg, de = d64.gather(2, got), d64.gather(2, exp)
    bound = 4 * (c + 2) * EPS32 * (qn[:, :, None] + torch.minimum(xn.gather(1, got.flatten(1)).view_as(got),
                                                                  xn.gather(1, exp.flatten(1)).view_as(exp)))
    differ = got != exp
    assert ((dg - de).abs() <= bound)[differ].all()
    return differ.double().mean().item()


@pytest.mark.parametrize('b,c,nq,n,k', [(2, 3, 250, 80, 5), (1, 3, 60, 40, 40), (2, 16, 90, 33, 20), (1, 64, 40, 300, 128)])
def test_knn_cross_cpu_matches_float64(b, c, nq, n, k):
    """At most 0.1 % of a case's entries may be excused as certified near ties; every case has more than 2000 entries, so
    that this admits one swapped pair at all."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    g = torch.Generator().manual_seed(b + c + nq + n + k)
    q, x = torch.randn(b, c, nq, generator=g), torch.randn(b, c, n, generator=g)
    idx, dist = ops.knn_cross(q, x, k, return_distance=True)
    assert idx.shape == (b, nq, k) and idx.dtype == torch.int64 and dist.shape == (b, nq, k)
    assert torch.equal(ops.knn_cross(q, x, k), idx)
    q64, x64 = q.double(), x.double()
    d64 = ((q64[:, :, :, None] - x64[:, :, None, :]) ** 2).sum(1)
    qn, xn = (q64**2).sum(1), (x64**2).sum(1)
    assert _certified(idx, d64, k, c, qn, xn) <= 0.001
    bound = 4 * (c + 2) * EPS32 * (qn[:, :, None] + xn.gather(1, idx.flatten(1)).view_as(idx))
    assert ((dist.double() - d64.gather(2, idx)).abs() <= bound).all()
    # a cloud against itself is the one-cloud search
    assert torch.equal(ops.knn_cross(x, x, min(k, n)), ops.knn(x, min(k, n)))


def test_hip_knn_cross_refuses_host_tensors():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    q, x = torch.zeros(2, 3, 5), torch.zeros(2, 3, 9)
    with pytest.raises(RuntimeError, match='q must be a CUDA tensor'):
        ops.hip_knn_cross(q, x, 3)
    with pytest.raises(RuntimeError, match='q must be a CUDA tensor'):
        ops.hip_knn_cross(q, x, 3, return_distance=True)
    with pytest.raises(ValueError, match='knn_cross'):
        ops.hip_knn_cross(q, torch.zeros(2, 4, 9), 3)


def test_shim_two_cloud_reductions_need_the_accelerator():
    from pykeops.torch import LazyTensor

    t1, t2 = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    dist = ((LazyTensor(t1[:, :, None, :]) - LazyTensor(t2[:, None, :, :])) ** 2).sum(-1)
    for bad in (lambda: dist.argKmin(3, dim=2), lambda: dist.argKmin(3, axis=1), lambda: dist.Kmin(3, dim=2),
                lambda: dist.Kmin(3, axis=1)):
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            bad()
    with pytest.raises(NotImplementedError):
        dist.Kmin(3, axis=0)


def test_knn_cross_is_declared_bound_and_switchable():
    import os
    import re

    from pointcloudcounterfactual_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert 'pcc_knn_cross' in _lib.ABI and len(_lib.ABI['pcc_knn_cross'][1]) == 10
    assert re.search(r'int pcc_knn_cross\(int b, int c, int nq, int n, int k,', open(os.path.join(root, 'include', 'pcc_neighbour.h')).read())
    hooks = open(os.path.join(root, 'include', 'pcc_test_hooks.h')).read()
    assert re.search(r'PCC_TUNE_KNN_CROSS_SPLIT = %d\b' % _lib.TUNING['knn_cross_split'], hooks)
