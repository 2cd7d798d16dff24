"""The binding layer refuses a tensor the library must never see before anything is enqueued.

Every pointer the package hands to ``libpcc_structural.so`` passes ``_lib.ptr``: on exactly the launch device, of the
declared dtype, contiguous.  For each public entry point that takes more than one tensor, one bad argument (a CPU index
tensor, int32 indices where int64 is declared, float64 features, a non-contiguous tensor the wrapper does not copy, a
tensor on another GPU) must raise a ``RuntimeError`` that names it, with no library launch recorded by the profiler and
caller-provided outputs untouched.
"""

import ctypes
import re

import pytest
import torch

from pointcloudcounterfactual_amd import _lib, backend, edgeconv
from pointcloudcounterfactual_amd import neighbour_ops as ops
from pointcloudcounterfactual_amd.harness import _BNReLURes
from pointcloudcounterfactual_amd.keops_shim import LazyTensor

pytestmark = pytest.mark.gpu


def _refused(fn, name, *prefilled):
    """``fn()`` raises a RuntimeError starting with ``name``, launches no kernel and leaves ``prefilled`` as it was."""
    before = [t.clone() for t in prefilled]
    torch.cuda.synchronize()
    _lib.lib.pcc_profile_enable(1)  # (also clears what an earlier call recorded)
    try:
        with pytest.raises(RuntimeError, match=rf'^{re.escape(name)} '):
            fn()
        launches = ctypes.c_int(-1)
        _lib.lib.pcc_profile_read(b'', None, ctypes.byref(launches))
    finally:
        _lib.lib.pcc_profile_enable(0)
    assert launches.value == 0, f'{name}: {launches.value} library launches'
    torch.cuda.synchronize()
    for t, b in zip(prefilled, before):
        assert torch.equal(t, b), name


def _clouds(dev):
    g = torch.Generator().manual_seed(0)
    p, q = torch.rand(2, 64, 3, generator=g).to(dev), torch.rand(2, 48, 3, generator=g).to(dev)
    return p, q, q.transpose(1, 2).contiguous().transpose(1, 2)  # the last one: q as a non-contiguous view


def _structural_cases(dev):
    p, q, q_nc = _clouds(dev)
    i1, i2 = torch.zeros(2, 64, dtype=torch.int32, device=dev), torch.zeros(2, 48, dtype=torch.int32, device=dev)
    match = torch.rand(2, 48, 64, device=dev)
    gb = torch.ones(2, device=dev)
    e1, e2 = torch.zeros(2, 64, 3, device=dev), torch.zeros(2, 48, 3, device=dev)
    d1, d2 = torch.ones(2, 64, device=dev), torch.ones(2, 48, device=dev)
    return [
        ('set_q', lambda: backend.ApproxMatch(p, q.double())),
        ('set_q', lambda: backend.ApproxMatch(p, q_nc)),
        ('set_q', lambda: backend.ApproxMatchCost(p, q.double())),
        ('set_q', lambda: backend.MatchCostImplicit(p, q_nc, True)),
        ('match', lambda: backend.MatchCost(p, q, match.transpose(1, 2).contiguous().transpose(1, 2))),
        ('match', lambda: backend.MatchCostGrad(p, q, match.double())),
        ('grad_cost', lambda: backend.MatchCostGradScaled(p, q, match, gb.cpu())),
        ('set_q', lambda: backend.NNDistance(p, q_nc)),
        ('set_q', lambda: backend.ChamferLoss(p, q.double(), True)),
        ('idx1', lambda: backend.ChamferLossGrad(p, q, i1.cpu(), i2, gb, True)),
        ('idx2', lambda: backend.ChamferLossGrad(p, q, i1, i2.long(), gb, True)),
        ('grad_loss', lambda: backend.ChamferLossGrad(p, q, i1, i2, gb.double(), True)),
        ('set_q', lambda: backend.ChamferEMD(p, q.double(), True, True)),
        ('idx2', lambda: backend.ChamferEMDGrad(p, q, i1, i2.cpu(), gb, True, e1, e2, gb)),
        ('idx1', lambda: backend.ChamferEMDGrad(p, q, i1.long(), i2, gb, True, e1, e2, gb)),
        ('emd_grad2', lambda: backend.ChamferEMDGrad(p, q, i1, i2, gb, True, e1, e2.transpose(0, 1).contiguous()
                                                      .transpose(0, 1), gb)),
        ('grad_emd', lambda: backend.ChamferEMDGrad(p, q, i1, i2, gb, True, e1, e2, gb.double())),
        ('idx2', lambda: backend.NNDistanceGrad(p, q, i1, i2.long(), d1, d2)),
        ('grad_dist1', lambda: backend.NNDistanceGrad(p, q, i1, i2, d1.cpu(), d2)),
        ('grad_dist2', lambda: backend.NNDistanceGrad(p, q, i1, i2, d1, d2.t().contiguous().t())),
        ('set_q', lambda: ((LazyTensor(p[:, :, None, :]) - LazyTensor(q.double()[:, None, :, :])) ** 2).sum(-1).min(axis=2)),
        ('q', lambda: ((LazyTensor(p[:, :, None, :]) - LazyTensor(q.double()[:, None, :, :])) ** 2).sum(-1).sum(axis=2)),
    ]


def _graph_cases(dev):
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 5, 64, generator=g).to(dev)
    idx = torch.randint(0, 64, (2, 64, 4), generator=g).to(dev)
    cb = torch.rand(2, 16, 4, generator=g).to(dev)
    return [
        ('indices', lambda: ops.get_neighbours(x, idx.int(), 4)),
        ('x', lambda: ops.get_neighbours(x.double(), idx, 4)),
        ('indices', lambda: ops.graph_max_pooling(x, idx.int(), 4)),
        ('indices', lambda: ops.get_graph_features(x, idx.int(), 4)),
        ('idx', lambda: edgeconv.neighbour_sum(x, idx.cpu())),
        ('idx', lambda: edgeconv.neighbour_sum(x, idx.int())),
        ('y', lambda: edgeconv.neighbour_sum(x.double(), idx)),
        ('idx', lambda: edgeconv.neighbour_minmax_target(x, idx.cpu())),
        ('idx', lambda: edgeconv.neighbour_minmax_target(x, idx.int())),
        ('y', lambda: edgeconv.neighbour_minmax_target(x.double(), idx)),
        # the nearest code of quantize.py:22-26 (feature width 4: the general pair search)
        ('q', lambda: ((LazyTensor(cb[:, :1, None, :]) - LazyTensor(cb.double()[:, None, :, :])) ** 2).sum(-1).argmin(axis=2)),
    ]


def _bn_cases(dev):
    z = torch.rand(2, 8, 16, device=dev)
    gamma, beta, mean, var = (torch.ones(8, device=dev) for _ in range(4))

    def bn(gamma=gamma, beta=beta, res=None, mean=mean, var=var):
        return _BNReLURes.apply(z, gamma, beta, res, 1, mean, var, 1e-5, True)

    return [
        ('gamma', lambda: bn(gamma=torch.ones(16, device=dev)[::2])),
        ('beta', lambda: bn(beta=beta.double())),
        ('mean', lambda: bn(mean=mean.cpu())),
        ('var', lambda: bn(var=var.double())),
        ('res', lambda: bn(res=z.double())),
    ]


@pytest.mark.parametrize('group', ['structural', 'graph', 'bn'])
def test_bad_argument_is_refused_before_launch(cuda, group):
    cases = {'structural': _structural_cases, 'graph': _graph_cases, 'bn': _bn_cases}[group](cuda)
    for name, fn in cases:
        _refused(fn, name)


def test_emd_backend_refuses_and_leaves_outputs(cuda):
    from emd import emd_backend

    g = torch.Generator().manual_seed(2)
    x1, x2 = torch.rand(2, 1024, 3, generator=g).to(cuda), torch.rand(2, 1024, 3, generator=g).to(cuda)
    dist = torch.full((2, 1024), 7.0, device=cuda)
    ass = torch.full((2, 1024), 3, dtype=torch.int32, device=cuda)
    _refused(lambda: emd_backend.forward(x1, x2.cpu(), dist, ass), 'xyz2', dist, ass)
    _refused(lambda: emd_backend.forward(x1, x2, dist, ass.long()), 'assignment', dist, ass)
    dist_nc = torch.full((1024, 2), 7.0, device=cuda).t()
    _refused(lambda: emd_backend.forward(x1, x2, dist_nc, ass), 'dist', dist_nc, ass)
    gradxyz = torch.full((2, 1024, 3), 5.0, device=cuda)
    _refused(lambda: emd_backend.backward(x1, x2, gradxyz, dist.double(), ass), 'graddist', gradxyz)
    _refused(lambda: emd_backend.backward(x1, x2, gradxyz, dist, ass.cpu()), 'idx', gradxyz)
    gradxyz_nc = torch.full((3, 1024, 2), 5.0, device=cuda).permute(2, 1, 0)
    _refused(lambda: emd_backend.backward(x1, x2, gradxyz_nc, dist, ass), 'gradxyz', gradxyz_nc)


def test_tensors_on_two_gpus_are_refused(cuda):
    if torch.cuda.device_count() < 2:
        pytest.skip('needs two GPUs')
    from emd import emd_backend

    other = torch.device('cuda:1')
    p, q, _ = _clouds(cuda)
    _refused(lambda: backend.NNDistance(p, q.to(other)), 'set_q')
    _refused(lambda: backend.ChamferEMD(p.to(other), q, True, True), 'set_q')
    _refused(lambda: ((LazyTensor(p[:, :, None, :]) - LazyTensor(q.to(other)[:, None, :, :])) ** 2).sum(-1).sum(axis=2),
             'q')
    x = torch.rand(2, 5, 64, device=cuda)
    idx = torch.randint(0, 64, (2, 64, 4), device=cuda)
    _refused(lambda: edgeconv.neighbour_sum(x, idx.to(other)), 'idx')
    _refused(lambda: edgeconv.neighbour_minmax_target(x.to(other), idx), 'idx')
    x1, x2 = torch.rand(1, 1024, 3, device=cuda), torch.rand(1, 1024, 3, device=cuda)
    dist = torch.full((1, 1024), 7.0, device=other)
    ass = torch.full((1, 1024), 3, dtype=torch.int32, device=cuda)
    _refused(lambda: emd_backend.forward(x1, x2, dist, ass), 'dist', dist, ass)
    z = torch.rand(2, 8, 16, device=cuda)
    ones = torch.ones(8, device=cuda)
    _refused(lambda: _BNReLURes.apply(z, ones, ones, None, 1, ones.to(other), ones, 1e-5, True), 'mean')
