"""The CPU half of tests/test_gpu_bnact.py and tests/test_gpu_pairwise.py: for every case's inputs, a float32
restatement of the kernels' formulas (tests/bn_pair_reference.py; fma emulated through float64, a correctly rounded
1/sqrt in place of v_rsq_f32) meets every bound, so the bounds are attainable by a correct float32 evaluation, and three
deliberately wrong variants miss them, so the bounds are not loose enough to hide a wrong kernel:
  * statistics that skip the last sample of one split range,
  * a float32-accumulated variance on the large-mean channel,
  * a pairwise argmin that keeps the last index on ties.
The restatement checks the slack of the bounds, not the kernels.  The mask-margin construction must terminate here
for every case (settle_mask raises if it does not)."""

import pytest
import torch

from tests import bn_pair_reference as R


def _settled(inp, training):
    if training:
        return R.settle_mask(inp['z'], inp['gamma'], inp['beta'], R.EPS)
    return R.settle_mask(inp['z'], inp['gamma'], inp['beta'], R.EPS, inp['mean'], inp['var'])


def _seed(b, c, n):
    return b * 1009 + c * 31 + n


@pytest.mark.parametrize('name,b,c,n,residual', R.BN_CASES, ids=R.BN_CASE_IDS)
def test_bn_statistics_bounds(name, b, c, n, residual):
    splits = R.pick_splits(b, c)
    for mode in ('exact', 'random'):
        z = R.bn_inputs(b, c, n, residual, mode, _seed(b, c, n))['z']
        m64, v64, bm, bv = R.bn_stats_ref(z)
        mean, var = R.bn_stats_f32(z)
        if mode == 'exact':
            R.assert_bits('mean', mean, m64)
            assert float(var[R.CONST_CH]) == 0.0
        R.assert_close('mean', mean, m64, bm)
        R.assert_close('var', var, v64, bv)
        if b > 1:  # wrong: one sample of the middle range is never added
            mean, var = R.bn_stats_f32(z, drop_last_of_range=splits // 2)
            with pytest.raises(AssertionError):
                if mode == 'exact':
                    R.assert_bits('mean', mean, m64)
                else:
                    R.assert_close('mean', mean, m64, bm)
            with pytest.raises(AssertionError):
                R.assert_close('var', var, v64, bv)
        if mode == 'random':  # wrong: float32 sums; E[z^2] - m^2 cancels seven digits on the N(1000, 1) channel
            _, var = R.bn_stats_f32(z, float32_sums=True)
            big = slice(R.BIG_CH, R.BIG_CH + 1)
            with pytest.raises(AssertionError):
                R.assert_close('var', var[big], v64[big], bv[big])


@pytest.mark.parametrize('name,b,c,n,residual', R.BN_CASES, ids=R.BN_CASE_IDS)
def test_bn_backward_bounds(name, b, c, n, residual):
    for mode in ('exact', 'random'):
        inp = R.bn_inputs(b, c, n, residual, mode, _seed(b, c, n))
        gamma, beta, gy = inp['gamma'], inp['beta'], inp['gy']
        for training in (False, True):
            if mode == 'exact':
                z, mean, var = inp['z'], inp['mean'], inp['var']
            else:
                z, mean, var = _settled(inp, training)  # raises unless it terminates
            assert not R.ambiguous(z, mean, var, R.EPS, gamma, beta)[0].any()
            ref = R.bn_bwd_ref(z, mean, var, R.EPS, gamma, beta, gy, training)
            dz, dgamma, dbeta = R.bn_bwd_f32(z, mean, var, R.EPS, gamma, beta, gy, training)
            if mode == 'exact':
                R.assert_bits('grad_beta', dbeta, ref['grad_beta'][0])
            R.assert_close('grad_z', dz, *ref['grad_z'])
            R.assert_close('grad_gamma', dgamma, *ref['grad_gamma'])
            R.assert_close('grad_beta', dbeta, *ref['grad_beta'])


@pytest.mark.parametrize('name,b,c,n,residual', R.BN_CASES, ids=R.BN_CASE_IDS)
def test_bn_forward_bound(name, b, c, n, residual):
    """The float32 restatement of the forward, fma(z - mean, sc, beta), meets the forward bound at the eval and at the
    batch statistics (the shifted form fma(z, sc, beta - mean sc) does not: it rounds beta twice)."""
    for mode in ('exact', 'random'):
        inp = R.bn_inputs(b, c, n, residual, mode, _seed(b, c, n))
        gamma, beta, res, r = inp['gamma'], inp['beta'], inp['res'], inp['r']
        for training in (False, True):
            if mode == 'exact':
                z, mean, var = inp['z'], inp['mean'], inp['var']
            else:
                z, mean, var = _settled(inp, training)
            y64, by, _, _ = R.bn_fwd_ref(z, mean, var, R.EPS, gamma, beta, res, r)
            R.assert_close(f'{mode} training={training} y', R.bn_fwd_f32(z, mean, var, R.EPS, gamma, beta, res, r), y64, by)


def test_a_flipped_mask_element_fails_the_backward_bound():
    """Why the mask is settled: one element on the other side of the ReLU moves grad_z by a whole grad_y."""
    inp = R.bn_inputs(3, 16, 256, None, 'random', 1)
    z, mean, var = _settled(inp, False)
    ref = R.bn_bwd_ref(z, mean, var, R.EPS, inp['gamma'], inp['beta'], inp['gy'], False)
    dz, _, _ = R.bn_bwd_f32(z, mean, var, R.EPS, inp['gamma'], inp['beta'], inp['gy'], False)
    at = tuple(dz.nonzero()[0].tolist())
    dz[at] = 0.0
    with pytest.raises(AssertionError):
        R.assert_close('grad_z', dz, *ref['grad_z'])


@pytest.mark.parametrize('b,n_p,n_q,d', R.PAIR_CASES)
def test_pair_bounds(b, n_p, n_q, d):
    for mode in ('exact', 'random'):
        p, q, go = R.pair_inputs(b, n_p, n_q, d, mode, n_p * 131 + n_q * 7 + d)
        ref = R.pair_ref(p, q, go)
        idx, dist, total, gp, gq = R.pair_f32(p, q, go)
        exact = mode == 'exact'
        R.pair_argmin_check(mode, idx, dist, ref['D'], d, exact)
        if exact:
            assert max(float(ref['sum'].max()), float(ref['grad_p_mag'].max()), float(ref['grad_q_mag'].max())) < 2 ** 24
            R.assert_bits('sum', total, ref['sum'])
            R.assert_bits('grad_p', gp, ref['grad_p'])
            R.assert_bits('grad_q', gq, ref['grad_q'])
            if n_q > 1:  # wrong: the last of the duplicated candidates
                idx, dist, *_ = R.pair_f32(p, q, go, last_on_ties=True)
                with pytest.raises(AssertionError):
                    R.pair_argmin_check(mode, idx, dist, ref['D'], d, True)
        else:
            bounds = R.pair_bounds(ref, n_p, n_q, d)
            R.assert_close('sum', total, ref['sum'], bounds['sum'])
            R.assert_close('grad_p', gp, ref['grad_p'], bounds['grad_p'])
            R.assert_close('grad_q', gq, ref['grad_q'], bounds['grad_q'])


def test_first_argmin_non_finite_rule():
    nan, inf = float('nan'), float('inf')
    dm = torch.tensor([[nan, 2.0, 1.0, 1.0], [nan, nan, nan, nan], [inf, inf, nan, inf], [nan, inf, 3.0, inf]], dtype=torch.float64)
    idx, best = R.first_argmin(dm)
    assert idx.tolist() == [2, 0, 0, 2] and best.tolist() == [1.0, inf, inf, 3.0]
