"""pcc_pair_argmin, pcc_pair_sqdist_sum and pcc_pair_sqdist_sum_bwd (csrc/pairwise.hip) through the C ABI against the
float64 distance matrix.  Cases, references and the derivation of the bounds: tests/bn_pair_reference.py.

  * exact  -- integer coordinates in [-8, 8] with many duplicated rows in q.  Every distance and sum is exact (all sums
              stay below 2^24, asserted), so idx is the first index of the float64 minimum and dist, the sum and both
              gradients equal float64 bit for bit.
  * random -- normal coordinates: the relative bounds g(d + 3), g(nq + d + 3), g(nq + 2), g(np + 3).
"""

import pytest
import torch

from tests import bn_pair_reference as R
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = torch.float32
I64 = torch.int64


def _L():
    from pointcloudcounterfactual_amd import _lib

    return _lib


def _argmin(p, q, want_dist=True):
    lib = _L()
    dev = p.device
    b, n_p, d = p.shape
    idx = torch.empty(b, n_p, dtype=I64, device=dev)
    dist = torch.empty(b, n_p, device=dev) if want_dist else None
    lib.call(lib.lib.pcc_pair_argmin, 'pair_argmin', dev, b, n_p, q.shape[1], d, lib.ptr(p, 'p', F32, dev),
             lib.ptr(q, 'q', F32, dev), lib.ptr(idx, 'idx', I64, dev), lib.ptr(dist, 'dist', F32, dev))
    return idx, dist


def _sum(p, q):
    lib = _L()
    dev = p.device
    b, n_p, d = p.shape
    out = torch.empty(b, n_p, device=dev)
    lib.call(lib.lib.pcc_pair_sqdist_sum, 'pair_sqdist_sum', dev, b, n_p, q.shape[1], d, lib.ptr(p, 'p', F32, dev),
             lib.ptr(q, 'q', F32, dev), lib.ptr(out, 'out', F32, dev))
    return out


def _sum_bwd(p, q, go, want_p=True, want_q=True):
    lib = _L()
    dev = p.device
    b, n_p, d = p.shape
    gp = torch.empty_like(p) if want_p else None
    gq = torch.empty_like(q) if want_q else None
    lib.call(lib.lib.pcc_pair_sqdist_sum_bwd, 'pair_sqdist_sum_bwd', dev, b, n_p, q.shape[1], d, lib.ptr(p, 'p', F32, dev),
             lib.ptr(q, 'q', F32, dev), lib.ptr(go, 'grad_out', F32, dev), lib.ptr(gp, 'grad_p', F32, dev),
             lib.ptr(gq, 'grad_q', F32, dev))
    return gp, gq


@pytest.mark.parametrize('mode', ['exact', 'random'])
@pytest.mark.parametrize('b,n_p,n_q,d', R.PAIR_CASES)
def test_pair_entries_against_float64(cuda, b, n_p, n_q, d, mode):
    p, q, go = (t.to(cuda) for t in R.pair_inputs(b, n_p, n_q, d, mode, seed=n_p * 131 + n_q * 7 + d))
    exact = mode == 'exact'
    tag = f'{mode} b={b} np={n_p} nq={n_q} d={d}'
    ref = R.pair_ref(p, q, go)
    idx, dist = _argmin(p, q)
    R.pair_argmin_check(tag, idx, dist, ref['D'], d, exact)
    idx_only, _ = _argmin(p, q, want_dist=False)  # dist = NULL leaves idx as it was
    assert torch.equal(idx_only, idx)
    total = _sum(p, q)
    gp, gq = _sum_bwd(p, q, go)
    gp_only, none_q = _sum_bwd(p, q, go, want_q=False)
    none_p, gq_only = _sum_bwd(p, q, go, want_p=False)
    assert none_q is None and none_p is None and torch.equal(gp_only, gp) and torch.equal(gq_only, gq)
    if exact:
        # float32 holds every integer below 2^24: partial sums of the non-negative distances stay below the total,
        # and the signed gradient sums below the sums of magnitudes
        assert max(float(ref['sum'].max()), float(ref['grad_p_mag'].max()), float(ref['grad_q_mag'].max())) < 2 ** 24
        R.assert_bits(f'{tag} sum', total, ref['sum'])
        R.assert_bits(f'{tag} grad_p', gp, ref['grad_p'])
        R.assert_bits(f'{tag} grad_q', gq, ref['grad_q'])
        return
    bounds = R.pair_bounds(ref, n_p, n_q, d)
    R.assert_close(f'{tag} sum', total, ref['sum'], bounds['sum'])
    R.assert_close(f'{tag} grad_p', gp, ref['grad_p'], bounds['grad_p'])
    R.assert_close(f'{tag} grad_q', gq, ref['grad_q'], bounds['grad_q'])


def test_nothing_to_reduce_over(cuda):
    """nq = 0: an argmin over nothing is refused (idx untouched); the sum over nothing is 0."""
    p = torch.randn(2, 5, 4, device=cuda)
    q = torch.empty(2, 0, 4, device=cuda)
    idx = torch.full((2, 5), -7, dtype=I64, device=cuda)
    lib = _L()
    with pytest.raises(RuntimeError, match=r'^pair_argmin: pair_argmin: nothing to reduce over$'):
        lib.call(lib.lib.pcc_pair_argmin, 'pair_argmin', cuda, 2, 5, 0, 4, p.data_ptr(), q.data_ptr(), idx.data_ptr(), None)
    torch.cuda.synchronize()
    assert (idx == -7).all()
    assert torch.equal(_sum(p, q), torch.zeros(2, 5, device=cuda))


def test_argmin_non_finite_rule(cuda):
    """The rule of include/pcc_neighbour.h: a NaN distance never wins; a row whose distances are all NaN returns index 0
    and dist = +inf; an infinite distance loses to any finite one, and among all-infinite distances index 0 is kept."""
    nan, inf = float('nan'), float('inf')
    gen = torch.Generator().manual_seed(9)
    p = torch.randint(-8, 9, (2, 6, 4), generator=gen).float()
    q = torch.randint(-8, 9, (2, 9, 4), generator=gen).float()
    q[0, 0] = p[0, 0]            # candidate 0 would win row 0 ...
    q[0, 0, 2] = nan             # ... but its distance is NaN
    q[0, 3, 1] = inf             # an infinite distance never beats a finite one
    p[0, 2, 0] = nan             # a NaN query row: every distance NaN
    p[1, 1, 3] = inf             # an infinite query coordinate: every distance +inf ...
    q[1, 4, 3] = inf             # ... except inf - inf = NaN against this candidate
    p, q = p.to(cuda), q.to(cuda)
    idx, dist = _argmin(p, q)
    dm = R.pair_ref(p, q, torch.zeros(2, 6, device=cuda))['D']
    assert dm[0, 2].isnan().all() and dm[0, :, 0].isnan().all() and dm[1, 1, 4].isnan() and dm[1, 1, :4].isinf().all()
    ref_idx, best = R.first_argmin(dm)  # NaN as +inf, first minimum, index 0 when nothing is finite
    assert torch.equal(idx, ref_idx)
    assert torch.equal(dist.double(), best)
    assert int(idx[0, 2]) == 0 and float(dist[0, 2]) == inf and int(idx[1, 1]) == 0 and float(dist[1, 1]) == inf
    # batch 0: candidate 0 (NaN) only where nothing is finite, candidate 3 (+inf) never
    assert (idx[0, [0, 1, 3, 4, 5]] != 0).all() and (idx[0] != 3).all()
