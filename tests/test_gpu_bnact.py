"""pcc_bn_stats, pcc_bn_relu_res_fwd and pcc_bn_relu_bwd (csrc/bnact.hip) through the C ABI against float64, at every
branch of their launchers and kernels.  The case table, the float64 references, the derivation of every bound and the
construction that keeps the ReLU mask unambiguous are in tests/bn_pair_reference.py; tests/test_bn_pair_bounds.py shows
without a GPU that the bounds can be met and that wrong kernels miss them.

Two value modes per case:
  * exact  -- z, grad_y, res integers in [-8, 8], channel 0 constant.  The sums are exact in double, so `mean` equals the
              float32 rounding of the float64 quotient bit for bit, the constant channel's `var` is exactly 0.0, and
              `grad_beta` equals the float64 sum bit for bit in every split geometry: a dropped, doubled or misrouted
              sample fails.  (The backward runs on given half-integer means, so that no pre-activation is near zero.)
  * random -- normal values, channel 1 ~ N(1000, 1): the derived bounds.

Non-finite values follow the PyTorch composition, observed on an MI355X with the native kernels and with MIOpen alike:
relu(NaN) = NaN; a channel that holds a NaN or an infinity has a NaN batch variance (and a NaN / infinite mean), so in
training mode its whole output and grad_z are NaN; PyTorch's ReLU backward (threshold_backward) zeroes only
`result <= 0`, so a NaN pre-activation *passes* the gradient: grad_beta of such a channel stays the finite sum of the
gradients that passed, and in eval mode grad_z at a NaN element is the finite gamma * invstd * grad_y, while grad_gamma
(a sum over xhat) is NaN or infinite.  The library follows that, not "NaN everywhere".
"""

import pytest
import torch

from tests import bn_pair_reference as R
from tests.unaligned_views import shifted
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENTINEL = -12345.0


def _L():
    from pointcloudcounterfactual_amd import _lib

    return _lib


def _stats(z):
    lib = _L()
    b, c, n = z.shape
    dev = z.device
    mean = torch.empty(c, device=dev)
    var = torch.empty(c, device=dev)
    lib.call(lib.lib.pcc_bn_stats, 'bn_stats', dev, b, c, n, lib.ptr(z, 'z', F32, dev), lib.ptr(mean, 'mean', F32, dev),
             lib.ptr(var, 'var', F32, dev))
    return mean, var


def _fwd(z, mean, var, gamma, beta, res, r, y=None, res_c=None):
    lib = _L()
    b, c, n = z.shape
    dev = z.device
    y = torch.empty_like(z) if y is None else y
    if res_c is None:
        res_c = res.shape[1] if res is not None else 0
    lib.call(lib.lib.pcc_bn_relu_res_fwd, 'bn_relu_res_fwd', dev, b, c, n, lib.ptr(z, 'z', F32, dev),
             lib.ptr(mean, 'mean', F32, dev), lib.ptr(var, 'var', F32, dev), R.EPS, lib.ptr(gamma, 'gamma', F32, dev),
             lib.ptr(beta, 'beta', F32, dev), lib.ptr(res, 'res', F32, dev), res_c, r, lib.ptr(y, 'y', F32, dev))
    return y


def _bwd(z, mean, var, gamma, beta, gy, training, dz=None):
    lib = _L()
    b, c, n = z.shape
    dev = z.device
    dz = torch.empty_like(z) if dz is None else dz
    dgamma = torch.empty(c, device=dev)
    dbeta = torch.empty(c, device=dev)
    lib.call(lib.lib.pcc_bn_relu_bwd, 'bn_relu_bwd', dev, b, c, n, lib.ptr(z, 'z', F32, dev), lib.ptr(mean, 'mean', F32, dev),
             lib.ptr(var, 'var', F32, dev), R.EPS, lib.ptr(gamma, 'gamma', F32, dev), lib.ptr(beta, 'beta', F32, dev),
             lib.ptr(gy, 'grad_y', F32, dev), int(training), lib.ptr(dz, 'grad_z', F32, dev),
             lib.ptr(dgamma, 'grad_gamma', F32, dev), lib.ptr(dbeta, 'grad_beta', F32, dev))
    return dz, dgamma, dbeta


def _to(inp, dev):
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in inp.items()}


def _check_stats(tag, z, exact):
    mean, var = _stats(z)
    m64, v64, bm, bv = R.bn_stats_ref(z)
    if exact:
        R.assert_bits(f'{tag} mean', mean, m64)
        assert float(var[R.CONST_CH]) == 0.0, f'{tag}: the constant channel has var = {float(var[R.CONST_CH])!r}'
    else:
        R.assert_close(f'{tag} mean', mean, m64, bm)
    R.assert_close(f'{tag} var', var, v64, bv)


def _check_fwd(tag, z, mean, var, inp):
    gamma, beta, res, r = inp['gamma'], inp['beta'], inp['res'], inp['r']
    y64, by, _, _ = R.bn_fwd_ref(z, mean, var, R.EPS, gamma, beta, res, r)
    R.assert_close(f'{tag} y', _fwd(z, mean, var, gamma, beta, res, r), y64, by)


def _check_bwd(tag, z, mean, var, inp, training, exact):
    gamma, beta, gy = inp['gamma'], inp['beta'], inp['gy']
    left = R.ambiguous(z, mean, var, R.EPS, gamma, beta)[0]
    assert not left.any(), f'{tag}: {int(left.sum())} reference pre-activations within the mask margin of zero'
    del left
    ref = R.bn_bwd_ref(z, mean, var, R.EPS, gamma, beta, gy, training)
    dz, dgamma, dbeta = _bwd(z, mean, var, gamma, beta, gy, training)
    if exact:
        R.assert_bits(f'{tag} grad_beta', dbeta, ref['grad_beta'][0])
    for name, got in (('grad_z', dz), ('grad_gamma', dgamma), ('grad_beta', dbeta)):
        R.assert_close(f'{tag} training={training} {name}', got, *ref[name])


@pytest.mark.parametrize('mode', ['exact', 'random'])
@pytest.mark.parametrize('name,b,c,n,residual', R.BN_CASES, ids=R.BN_CASE_IDS)
def test_bn_entries_at_every_branch(cuda, name, b, c, n, residual, mode):
    inp = _to(R.bn_inputs(b, c, n, residual, mode, seed=b * 1009 + c * 31 + n), cuda)
    exact = mode == 'exact'
    tag = f'{name} {mode}'
    _check_stats(tag, inp['z'], exact)
    if exact:  # given statistics; the `training` flag only selects the grad_z formula
        _check_bwd(tag, inp['z'], inp['mean'], inp['var'], inp, False, True)
        _check_bwd(tag, inp['z'], inp['mean'], inp['var'], inp, True, True)
        return
    z, mean, var = R.settle_mask(inp['z'], inp['gamma'], inp['beta'], R.EPS, inp['mean'], inp['var'])
    _check_bwd(f'{tag} eval', z, mean, var, inp, False, False)
    z, mean, var = R.settle_mask(inp['z'], inp['gamma'], inp['beta'], R.EPS)
    _check_stats(f'{tag} settled', z, False)
    _check_bwd(f'{tag} training', z, mean, var, inp, True, False)


@pytest.mark.parametrize('mode', ['exact', 'random'])
@pytest.mark.parametrize('name,b,c,n,residual', R.BN_CASES, ids=R.BN_CASE_IDS)
def test_bn_forward_at_every_branch(cuda, name, b, c, n, residual, mode):
    """pcc_bn_relu_res_fwd against float64 under the forward bound
        (DELTA + 2u) (|z sc| + |mean sc|) + u |beta| + u |y64|
    at the given (eval) statistics and at the batch statistics of the settled z.  The kernel's centred pre-activation
    fma(z - mean, sc, beta) meets it; the shifted form fma(z, sc, beta - mean sc) it replaced missed it at three
    random-mode cases (splits-21-uneven, splits-2-even, workload: 2, 1 and 80 elements, by up to 1.3e-08, where the
    residual cancels most of relu(pre) and beta was rounded twice)."""
    inp = _to(R.bn_inputs(b, c, n, residual, mode, seed=b * 1009 + c * 31 + n), cuda)
    tag = f'{name} {mode}'
    if mode == 'exact':
        _check_fwd(tag, inp['z'], inp['mean'], inp['var'], inp)
        return
    z, mean, var = R.settle_mask(inp['z'], inp['gamma'], inp['beta'], R.EPS, inp['mean'], inp['var'])
    _check_fwd(f'{tag} eval', z, mean, var, inp)
    z, mean, var = R.settle_mask(inp['z'], inp['gamma'], inp['beta'], R.EPS)
    _check_fwd(f'{tag} training', z, mean, var, inp)


def _offset_view(t):
    """A contiguous copy of t that starts one float past a 16-byte boundary."""
    return shifted(t)


@pytest.mark.parametrize('which', ['z', 'res', 'gy', 'y', 'grad_z'])
def test_offset_views_take_the_scalar_path(cuda, which):
    """n % 4 == 0, and one operand in turn is a contiguous view 4 bytes past a 16-byte boundary: the kernels must fall
    back to 4-byte accesses (every base a kernel vectorises is checked), with the same values."""
    b, c, n = 2, 8, 256
    inp = _to(R.bn_inputs(b, c, n, (1, 8), 'random', seed=77), cuda)
    z, mean, var = R.settle_mask(inp['z'], inp['gamma'], inp['beta'], R.EPS, inp['mean'], inp['var'])
    gamma, beta, res, gy = inp['gamma'], inp['beta'], inp['res'], inp['gy']
    if which == 'z':
        z = _offset_view(z)
    elif which == 'res':
        res = _offset_view(res)
    elif which == 'gy':
        gy = _offset_view(gy)
    y = _offset_view(torch.full_like(z, float('nan'))) if which == 'y' else None
    dz = _offset_view(torch.full_like(z, float('nan'))) if which == 'grad_z' else None
    y64, by, _, _ = R.bn_fwd_ref(z, mean, var, R.EPS, gamma, beta, res, 1)
    R.assert_close(f'offset {which}: y', _fwd(z, mean, var, gamma, beta, res, 1, y=y), y64, by)
    stat_m, stat_v = _stats(z)
    m64, v64, bm, bv = R.bn_stats_ref(z)
    R.assert_close(f'offset {which}: mean', stat_m, m64, bm)
    R.assert_close(f'offset {which}: var', stat_v, v64, bv)
    for training in (False, True):
        ref = R.bn_bwd_ref(z, mean, var, R.EPS, gamma, beta, gy, training)
        got = _bwd(z, mean, var, gamma, beta, gy, training, dz=dz)
        for name, t in zip(('grad_z', 'grad_gamma', 'grad_beta'), got):
            R.assert_close(f'offset {which}: training={training} {name}', t, *ref[name])


def test_refusals_leave_the_outputs_untouched(cuda):
    """b c = 65536 rows: refused by the two entries whose grid has one row per (sample, channel), accepted by
    pcc_bn_stats; a residual with too few channels and r < 1 are refused; nothing is written on a refusal."""
    lib = _L()
    b, c, n = 16, 4096, 4
    gen = torch.Generator().manual_seed(1)
    z = torch.randint(-8, 9, (b, c, n), generator=gen).float().to(cuda)
    gy = torch.ones_like(z)
    ones = torch.ones(c, device=cuda)
    y = torch.full_like(z, SENTINEL)
    with pytest.raises(RuntimeError, match=r'^bn_relu_res_fwd: bn_relu_res_fwd: more than 65535 \(sample, channel\) rows$'):
        _fwd(z, ones, ones, ones, ones, None, 1, y=y)
    dz = torch.full_like(z, SENTINEL)
    with pytest.raises(RuntimeError, match=r'^bn_relu_bwd: bn_relu_bwd: more than 65535 \(sample, channel\) rows$'):
        _bwd(z, ones, ones, ones, ones, gy, 1, dz=dz)
    torch.cuda.synchronize()
    assert (y == SENTINEL).all() and (dz == SENTINEL).all()
    mean, var = _stats(z)  # accepted: its grid is channels x splits
    m64, v64, _, bv = R.bn_stats_ref(z)
    R.assert_bits('stats at 65536 rows: mean', mean, m64)
    R.assert_close('stats at 65536 rows: var', var, v64, bv)

    b, c, n = 2, 7, 8
    z = torch.zeros(b, c, n, device=cuda)
    ones = torch.ones(c, device=cuda)
    y = torch.full_like(z, SENTINEL)
    few = r'^bn_relu_res_fwd: bn_relu_res_fwd: residual has too few channels$'
    with pytest.raises(RuntimeError, match=few):  # (c - 1) / r = 3 >= res_c = 3
        _fwd(z, ones, ones, ones, ones, torch.zeros(b, 3, n, device=cuda), 2, y=y)
    with pytest.raises(RuntimeError, match=few):  # r < 1
        _fwd(z, ones, ones, ones, ones, torch.zeros(b, 7, n, device=cuda), 0, y=y)
    with pytest.raises(RuntimeError, match=few):
        _fwd(z, ones, ones, ones, ones, torch.zeros(b, 7, n, device=cuda), -1, y=y)
    with pytest.raises(RuntimeError, match=r'^bn_relu_res_fwd: bn_relu_res_fwd: bad size$'):
        lib.call(lib.lib.pcc_bn_relu_res_fwd, 'bn_relu_res_fwd', cuda, -1, c, n, z.data_ptr(), ones.data_ptr(),
                 ones.data_ptr(), R.EPS, ones.data_ptr(), ones.data_ptr(), None, 0, 1, y.data_ptr())
    torch.cuda.synchronize()
    assert (y == SENTINEL).all()
    _fwd(z, torch.zeros_like(ones), ones, ones, ones, torch.zeros(b, 4, n, device=cuda), 2, y=y)  # 3 < res_c = 4: accepted
    assert (y == 1.0).all()  # fma(0, sc, beta - 0 * sc) + 0


@pytest.mark.parametrize('b,c,n', [(0, 4, 8), (3, 0, 8), (3, 4, 0)])
def test_empty_sizes(cuda, b, c, n):
    """b, c or n = 0: PCC_OK without a launch and without touching an output, except pcc_bn_stats with channels but no
    samples, which refuses (a mean over nothing)."""
    lib = _L()
    cc = max(c, 1)
    buf = torch.full((64,), SENTINEL, device=cuda)
    ones = torch.ones(cc, device=cuda)
    args = (b, c, n, buf.data_ptr(), ones.data_ptr(), ones.data_ptr(), R.EPS, ones.data_ptr(), ones.data_ptr())
    lib.lib.pcc_profile_enable(1)
    try:
        lib.call(lib.lib.pcc_bn_relu_res_fwd, 'bn_relu_res_fwd', cuda, *args, None, 0, 1, buf.data_ptr())
        lib.call(lib.lib.pcc_bn_relu_bwd, 'bn_relu_bwd', cuda, *args, buf.data_ptr(), 1, buf.data_ptr(), buf.data_ptr(),
                 buf.data_ptr())
        if c == 0:
            lib.call(lib.lib.pcc_bn_stats, 'bn_stats', cuda, b, c, n, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
        else:
            with pytest.raises(RuntimeError, match=r'^bn_stats: bn_stats: no samples$'):
                lib.call(lib.lib.pcc_bn_stats, 'bn_stats', cuda, b, c, n, buf.data_ptr(), buf.data_ptr(), buf.data_ptr())
        import ctypes

        count = ctypes.c_int(0)
        lib.lib.pcc_profile_read(b'', None, ctypes.byref(count))
        assert count.value == 0
    finally:
        lib.lib.pcc_profile_enable(0)
    torch.cuda.synchronize()
    assert (buf == SENTINEL).all()


# ---- non-finite values ---------------------------------------------------------------------------------------------------


def _torch_composition(z, gamma, beta, res, gy, training, mean, var):
    """batch_norm + relu + residual add and autograd through it, on z's device; momentum 1 so that the running
    statistics after a training call are the batch statistics."""
    import torch.nn.functional as F

    z = z.detach().clone().requires_grad_(True)
    gamma = gamma.detach().clone().requires_grad_(True)
    beta = beta.detach().clone().requires_grad_(True)
    rm, rv = (torch.zeros_like(mean), torch.ones_like(var)) if training else (mean.clone(), var.clone())
    y = torch.relu(F.batch_norm(z, rm, rv, gamma, beta, training, 1.0, R.EPS)) + res
    y.backward(gy)
    return {'mean': rm, 'var': rv, 'y': y.detach(), 'grad_z': z.grad, 'grad_gamma': gamma.grad, 'grad_beta': beta.grad}


def _same_nan_set(what, got, ref):
    assert torch.equal(got.isnan(), ref.isnan()), (f'{what}: NaN at {int(got.isnan().sum())} positions, the PyTorch '
                                                   f'composition at {int(ref.isnan().sum())}')


@pytest.mark.parametrize('training', [False, True], ids=['eval', 'training'])
@pytest.mark.parametrize('n', [pytest.param(256, id='vector'), pytest.param(259, id='scalar')])
def test_non_finite_values_follow_the_pytorch_composition(cuda, n, training):
    """One NaN, one +inf and one -inf in three channels of z: mean, var, y, grad_z, grad_gamma and grad_beta are NaN
    exactly where the PyTorch composition on the same GPU is, and every other position obeys the float64 bounds."""
    b, c = 3, 8
    inp = _to(R.bn_inputs(b, c, n, (1, c), 'random', seed=n), cuda)
    inp['gamma'] = inp['gamma'].abs()
    gamma, beta, res, gy = inp['gamma'], inp['beta'], inp['res'], inp['gy']
    if training:
        z, _, _ = R.settle_mask(inp['z'], gamma, beta, R.EPS)
    else:
        z, mean, var = R.settle_mask(inp['z'], gamma, beta, R.EPS, inp['mean'], inp['var'])
    z[1, 2, n // 2] = float('nan')
    z[0, 3, 5] = float('inf')
    z[2, 4, n - 1] = float('-inf')
    if training:
        mean, var = R.rounded_stats(z)  # the finite channels' statistics are those the mask was settled with
        assert var[2:5].isnan().all() and mean[3] == float('inf') and mean[4] == float('-inf')
    pt = _torch_composition(z, gamma, beta, res, gy, training, mean, var)

    if training:
        k_mean, k_var = _stats(z)
        _same_nan_set('mean', k_mean, pt['mean'])
        _same_nan_set('var', k_var, pt['var'])
        m64, v64, bm, bv = R.bn_stats_ref(z)
        R.assert_close('mean', k_mean, m64, bm)
        R.assert_close('var', k_var, v64, bv)
    y = _fwd(z, mean, var, gamma, beta, res, 1)
    _same_nan_set('y', y, pt['y'])
    y64, by, _, _ = R.bn_fwd_ref(z, mean, var, R.EPS, gamma, beta, res, 1)
    R.assert_close('y', y, y64, by)
    got = _bwd(z, mean, var, gamma, beta, gy, training)
    ref = R.bn_bwd_ref(z, mean, var, R.EPS, gamma, beta, gy, training)
    for name, t in zip(('grad_z', 'grad_gamma', 'grad_beta'), got):
        _same_nan_set(name, t, pt[name])
        assert torch.equal(t.isinf(), pt[name].isinf()), f'{name}: infinities differ from the PyTorch composition'
        R.assert_close(name, t, *ref[name])
    assert not got[2].isnan().any()  # PyTorch's rule: grad_beta stays finite


@pytest.mark.parametrize('training', [False, True], ids=['eval', 'training'])
def test_points_conv_with_nan_input_matches_the_composition(cuda, training):
    """Through the module: a NaN in x reaches every output channel at that point.  Fused tail against the PyTorch
    composition: the same NaN positions in y, the input gradient, running_mean and running_var."""
    import copy

    from pointcloudcounterfactual_amd import harness

    torch.manual_seed(5)
    fused = harness.PointsConv(16, 16, torch.nn.ReLU(inplace=True), residual=True).to(cuda)
    plain = copy.deepcopy(fused)
    plain._fused_tail = lambda z, x: None
    fused.train(training)
    plain.train(training)
    x1 = torch.randn(3, 16, 64, device=cuda)
    x1[1, 3, 7] = float('nan')
    x2 = x1.clone().requires_grad_(True)
    x1.requires_grad_(True)
    y1, y2 = fused(x1), plain(x2)
    assert y1.isnan().any()
    _same_nan_set('y', y1, y2)
    w = torch.randn_like(y1)
    (y1 * w).sum().backward()
    (y2 * w).sum().backward()
    _same_nan_set('grad_x', x1.grad, x2.grad)
    _same_nan_set('running_mean', fused.bn.running_mean, plain.bn.running_mean)
    _same_nan_set('running_var', fused.bn.running_var, plain.bn.running_var)
    assert bool(fused.bn.running_var.isnan().all()) == training
    fin = ~y2.isnan()
    torch.testing.assert_close(y1[fin], y2[fin], rtol=1e-4, atol=1e-5)
