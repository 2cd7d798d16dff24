"""CPU tests of the fused EdgeConv block: the float64 reference (tests/edgeconv_reference.py) against closed forms, the
selection-mask budget of every committed case, and the CPU path of ``edgeconv.FusedEdgeConv`` -- the formulas the HIP path
shares -- held to the bar of the reference module, with the float32 CPU composition as yardstick."""

import pytest
import torch
import torch.nn.functional as F

from tests import edgeconv_reference as ref

IDS = [c.id for c in ref.ALL_CASES]


def _plain_inputs(seed, b, c, cout, n, k):
    gen = torch.Generator().manual_seed(seed)
    return {'x': torch.randn(b, c, n, generator=gen), 'w': torch.randn(cout, 2 * c, generator=gen) / (2 * c) ** 0.5,
            'gamma': torch.randn(cout, generator=gen), 'beta': torch.randn(cout, generator=gen),
            'running_mean': torch.randn(cout, generator=gen), 'running_var': torch.rand(cout, generator=gen) + 0.5,
            'num_batches_tracked': 5, 'cot': torch.randn(b, cout, n, generator=gen)}


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('act', [True, False])
def test_reference_self_loops_reduce_to_pointwise_conv_bn(training, act):
    """k = 1 with idx[n] = n: x_j - x_n = 0, so the block is act(BatchNorm1d(Wb x)) -- torch's own layers in float64:
    output, all four gradients (the Wa half of the weight gradient is 0), the running statistics and the counter."""
    b, c, cout, n = 3, 5, 7, 40
    d = _plain_inputs(11, b, c, cout, n, 1)
    d['idx'] = torch.arange(n).view(1, n, 1).expand(b, n, 1).contiguous()
    got = ref.reference(d, act, training, d['cot'])
    x = d['x'].double().requires_grad_(True)
    wb = d['w'][:, c:].double().requires_grad_(True)
    gamma, beta = d['gamma'].double().requires_grad_(True), d['beta'].double().requires_grad_(True)
    rm, rv = d['running_mean'].double().clone(), d['running_var'].double().clone()
    y = F.batch_norm(F.conv1d(x, wb.unsqueeze(2)), rm, rv, gamma, beta, training, ref.MOMENTUM, ref.EPS)
    out = F.leaky_relu(y, 0.2) if act else y
    out.backward(d['cot'].double())
    tol = {'rtol': 1e-11, 'atol': 1e-12}
    torch.testing.assert_close(got['out'], out.detach(), **tol)
    torch.testing.assert_close(got['grad_x'], x.grad, **tol)
    torch.testing.assert_close(got['grad_conv'][:, c:], wb.grad, **tol)
    assert not got['grad_conv'][:, :c].any()
    torch.testing.assert_close(got['grad_gamma'], gamma.grad, **tol)
    torch.testing.assert_close(got['grad_beta'], beta.grad, **tol)
    torch.testing.assert_close(got['running_mean'], rm, **tol)
    torch.testing.assert_close(got['running_var'], rv, **tol)
    assert got['num_batches_tracked'] == 5 + int(training)


@pytest.mark.parametrize('act', [True, False])
def test_reference_constant_cloud_gives_act_of_beta(act):
    """Every point equal: z is constant per channel, the batch variance 0 and z - mean 0, so out = act(beta) whatever the
    graph; the running mean moves towards Wb x, the running variance towards 0."""
    b, c, cout, n, k = 2, 4, 6, 30, 5
    d = _plain_inputs(12, b, c, cout, n, k)
    d['x'] = torch.tensor([2.0, -1.5, 0.25, 8.0]).view(1, c, 1).expand(b, c, n).contiguous()  # (dyadic: z is exact)
    d['w'] = (d['w'] * 64).round() / 64
    d['idx'] = ref.hub_graph(torch.Generator().manual_seed(1), b, n, k)
    got = ref.reference(d, act, True)
    beta = d['beta'].double()
    want = torch.where(beta < 0, 0.2 * beta, beta) if act else beta
    torch.testing.assert_close(got['out'], want.view(1, cout, 1).expand(b, cout, n), rtol=0, atol=1e-12)
    z = d['w'][:, c:].double() @ d['x'][0, :, 0].double()
    torch.testing.assert_close(got['running_mean'], (1 - ref.MOMENTUM) * d['running_mean'].double() + ref.MOMENTUM * z, rtol=1e-13, atol=0)
    torch.testing.assert_close(got['running_var'], (1 - ref.MOMENTUM) * d['running_var'].double(), rtol=1e-13, atol=0)


def test_case_table_is_what_the_bar_was_set_for():
    """Six shapes x two graphs at offset 0, the c = 3 / 16 / 64 shapes at offset 8, the c = 3 / 5 shapes at offset 64; the
    graphs are what they claim (k-NN lists start with the point itself; hub rows all list point 0)."""
    assert len(ref.CASES) == 2 * (6 + 3 + 2) and len(set(ref.ALL_CASES)) == len(ref.ALL_CASES)
    assert {(c.c, c.offset) for c in ref.CASES if c.offset} == {(3, 8.0), (16, 8.0), (64, 8.0), (3, 64.0), (5, 64.0)}
    for case in ref.ALL_CASES:
        d = ref.inputs(case)
        idx = d['idx']
        assert idx.shape == (case.b, case.n, case.k) and int(idx.min()) >= 0 and int(idx.max()) < case.n
        if case.graph == 'knn':
            assert torch.equal(idx[:, :, 0], torch.arange(case.n).expand(case.b, case.n))
            assert (idx.sort(dim=2).values.diff(dim=2) > 0).all()  # distinct targets
        else:
            assert not idx[:, :, 0].any() and int(torch.bincount(idx[0].reshape(-1))[0]) >= case.n
        assert float((d['x'].mean() - case.offset).abs()) < 0.05
        assert (d['gamma'] > 0).any() and (d['gamma'] < 0).any() or case.cout == 1
        assert (d['gamma'] == 0).sum() == (2 if case.special == 'zero-gamma' else 0)


@pytest.mark.parametrize('case', ref.GRAD_CASES, ids=[c.id for c in ref.GRAD_CASES])
def test_mask_budget(case):
    """At most 2 % of a case's output elements are masked; k = 1 masks nothing (one edge: no runner-up)."""
    share = ref.masked_cotangent(case)[1]
    print(f'edgeconv-mask | {case.id} | {share:.4%}')
    assert share <= ref.MASK_CAP
    if case.k == 1:
        assert share == 0.0


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('case', ref.ALL_CASES, ids=IDS)
def test_cpu_path_meets_the_bar(case, training):
    """FusedEdgeConv on CPU tensors against float64, every quantity within 16 x the float32 composition's own error."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from pointcloudcounterfactual_amd.edgeconv import FusedEdgeConv

    fused = ref.fused_float32(FusedEdgeConv, case, training)
    unfused = ref.unfused_float32(ops.get_graph_features, case, training)
    ref.check_bar(f'cpu {case.id} {"train" if training else "eval"}', fused, unfused, ref.case_reference(case, training))


@pytest.mark.parametrize('value', [float('nan'), float('inf')], ids=['nan', 'inf'])
def test_cpu_path_keeps_non_finite_values_where_the_reference_has_them(value):
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from pointcloudcounterfactual_amd.edgeconv import FusedEdgeConv

    ref.check_nonfinite(FusedEdgeConv, ops.get_graph_features, 'cpu', value)


def _kernel_rule(y, idx, nan_wins):
    """gather_lds_kernel<kMinMax>'s loop over j restated: `nan_wins` is the rule of the kernel, False the plain compares
    (v > acc, v < lo) it had before."""
    b, c, n = y.shape
    k = idx.shape[2]
    nb = torch.gather(y, 2, idx.reshape(b, 1, n * k).expand(-1, c, -1)).view(b, c, n, k)
    ie = idx.unsqueeze(1).expand(-1, c, -1, -1)
    acc, lo = nb[..., 0].clone(), nb[..., 0].clone()
    tb, tl = ie[..., 0].clone(), ie[..., 0].clone()
    for j in range(1, k):
        v, t = nb[..., j], ie[..., j]
        live = acc == acc  # (a NaN enters acc and lo at the same j: one test serves both)
        gt = ~(v <= acc) & live if nan_wins else v > acc
        lt = ~(v >= lo) & live if nan_wins else v < lo
        acc, tb = torch.where(gt, v, acc), torch.where(gt, t, tb)
        lo, tl = torch.where(lt, v, lo), torch.where(lt, t, tl)
    return torch.stack([tb, tl], dim=1)


def test_minmax_target_rule_on_special_values():
    """The min/max target on NaN and +-inf: the module's CPU path (argmax / argmin) and the kernel's compare rule restated
    both give the reference's targets (the first NaN wins both); the plain compares the kernel used to have do not."""
    from pointcloudcounterfactual_amd.edgeconv import neighbour_minmax_target

    y, idx = ref.minmax_special_inputs()
    want = ref.minmax_target_reference(y, idx)
    assert torch.equal(neighbour_minmax_target(y, idx), want)
    assert torch.equal(_kernel_rule(y, idx, True), want)
    plain = _kernel_rule(y, idx, False)
    assert (plain != want)[0].any() and torch.equal(plain[1], want[1])
