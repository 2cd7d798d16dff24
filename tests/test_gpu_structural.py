"""GPU parity tests: HIP path (through the C ABI) vs the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): nearest-neighbour indices and squared distances bit-exact;
float results of the EMD path within the tolerance written next to each assert.
"""

import numpy as np
import pytest
import torch

from tests.util import pair
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

NN_SHAPES = [(1, 1, 1), (2, 3, 5), (1, 7, 1), (2, 64, 64), (3, 257, 130), (2, 512, 513), (2, 1024, 1024),
             (1, 2049, 2047), (2, 100, 4100), (4, 1024, 1024)]


def _dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


@pytest.mark.parametrize('b,n,m', NN_SHAPES)
@pytest.mark.parametrize('kind', ['recon', 'uniform'])
def test_nndistance_bit_exact(cuda, oracle_mod, b, n, m, kind):
    from pointcloudcounterfactual_amd import backend

    a, c = pair(100 + n + m, b, n, m, kind)
    d1, i1, d2, i2 = backend.NNDistance(_dev(a, cuda), _dev(c, cuda))
    od1, oi1, od2, oi2 = oracle_mod.nndistance(a, c)
    assert np.array_equal(i1.cpu().numpy(), oi1)
    assert np.array_equal(i2.cpu().numpy(), oi2)
    assert np.array_equal(d1.cpu().numpy(), od1)  # bit-exact f32
    assert np.array_equal(d2.cpu().numpy(), od2)


def test_nndistance_ties_lowest_index(cuda, oracle_mod):
    """Duplicate candidates: the lowest index must win (nndistance.cu:26,36,116)."""
    from pointcloudcounterfactual_amd import backend

    rng = np.random.default_rng(5)
    base = rng.random((2, 40, 3), dtype=np.float32)
    c = np.concatenate([base] * 30, axis=1)  # 1200 candidates, every point repeated 30x, spans chunks/waves
    a = base[:, ::-1].copy()
    d1, i1, d2, i2 = backend.NNDistance(_dev(a, cuda), _dev(c, cuda))
    od1, oi1, od2, oi2 = oracle_mod.nndistance(a, c)
    assert np.array_equal(i1.cpu().numpy(), oi1) and np.array_equal(i2.cpu().numpy(), oi2)
    assert (i1.cpu().numpy() < 40).all()
    assert np.array_equal(d1.cpu().numpy(), od1) and np.array_equal(d2.cpu().numpy(), od2)


def test_nndistance_self(cuda):
    from pointcloudcounterfactual_amd import backend

    a, _ = pair(9, 2, 777, 777, 'uniform')
    t = _dev(a, cuda)
    d1, i1, d2, i2 = backend.NNDistance(t, t)
    assert (d1 == 0).all() and (d2 == 0).all()
    ar = torch.arange(777, device=cuda, dtype=torch.int32).expand(2, -1)
    assert torch.equal(i1, ar) and torch.equal(i2, ar)


@pytest.mark.parametrize('b,n,m', [(2, 3, 5), (3, 257, 130), (2, 1024, 1024), (1, 2049, 2047)])
def test_nndistancegrad(cuda, oracle_mod, b, n, m):
    from pointcloudcounterfactual_amd import backend

    a, c = pair(200 + n, b, n, m)
    rng = np.random.default_rng(1)
    g1 = rng.standard_normal((b, n)).astype(np.float32)
    g2 = rng.standard_normal((b, m)).astype(np.float32)
    _, oi1, _, oi2 = oracle_mod.nndistance(a, c)
    og1, og2 = oracle_mod.nndistancegrad(a, c, oi1, oi2, g1, g2)
    r1, r2 = backend.NNDistanceGrad(_dev(a, cuda), _dev(c, cuda), _dev(oi1, cuda), _dev(oi2, cuda), _dev(g1, cuda),
                                    _dev(g2, cuda))
    # scatter-add order differs (reference: unordered atomics) -> 1e-5 relative, small absolute floor
    np.testing.assert_allclose(r1.cpu().numpy(), og1, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r2.cpu().numpy(), og2, rtol=1e-5, atol=1e-6)


def test_nn_distance_autograd_matches_torch(cuda):
    """Autograd through nn_distance == autograd through a dense torch fp32 evaluation of the same loss."""
    from structural_losses import nn_distance

    a, c = pair(11, 2, 300, 200)
    t1 = _dev(a, cuda).requires_grad_(True)
    t2 = _dev(c, cuda).requires_grad_(True)
    d1, d2 = nn_distance(t1, t2)
    (d1.mean(1) + d2.mean(1)).sum().backward()
    u1 = _dev(a, cuda).requires_grad_(True)
    u2 = _dev(c, cuda).requires_grad_(True)
    D = ((u1[:, :, None, :] - u2[:, None, :, :]) ** 2).sum(-1)
    (D.min(2)[0].mean(1) + D.min(1)[0].mean(1)).sum().backward()
    np.testing.assert_allclose(t1.grad.cpu().numpy(), u1.grad.cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(t2.grad.cpu().numpy(), u2.grad.cpu().numpy(), rtol=1e-5, atol=1e-7)


AM_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 64, 64), (2, 257, 130), (2, 128, 256), (1, 513, 512), (2, 1024, 1024),
             (1, 2100, 2300), (1, 4099, 100), (2, 70, 2050),  # these three span several 2048-candidate chunks
             (1, 60, 16500),  # more than 512 words of live bits per sample (two per thread in the owner-compacted passes)
             (1, 9000, 40),   # rank / soa of am_sort_kernel<32> (8193 .. 16384 points)
             (1, 40, 33000)]  # more than 32768 points: the cloud keeps its order, nothing is culled


@pytest.mark.parametrize('b,n,m', AM_SHAPES)
@pytest.mark.parametrize('kind', ['recon', 'uniform'])
def test_approxmatch_vs_oracle(cuda, oracle_mod, b, n, m, kind):
    a, c = pair(300 + n + m, b, n, m, kind)
    _approxmatch_inside_the_oracle_bars(cuda, oracle_mod, a, c)


def _approxmatch_inside_the_oracle_bars(cuda, oracle_mod, a, c):
    """``backend.ApproxMatch`` + ``MatchCost`` of the clouds ``a``, ``c`` against the float64 recurrence; -> (match, cost)."""
    from pointcloudcounterfactual_amd import backend

    n, m = a.shape[1], c.shape[1]
    match, temp = backend.ApproxMatch(_dev(a, cuda), _dev(c, cuda))
    om64, ot64 = oracle_mod.approxmatch_f64(a, c)
    got = match.cpu().numpy()
    gtemp = temp.cpu().numpy()[:, : n + m]
    # Element-wise the f32 recurrence is ill-conditioned (remain* are clamped differences that feed ratios): LEGITIMATE
    # float32 evaluations of the reference's own formulas -- the oracle with exp taken as libm expf, as exp2 of the
    # exactly scaled argument, as CUDA's documented __expf argument path, and with ex2.approx's permitted 2 ulp
    # (oracle exp modes 0-3) -- sit up to 7e-4 from the float64 recurrence and from each other at N=2048.  Bars
    # (measured: tools/parity_report.py, gpurun_out/parity_report.jsonl): elements, per-point masses and remainders
    # within 3x that spread (floors 5e-5 / 1e-5 where the spread itself is at rounding level); total mass and
    # cost -- the well-conditioned quantities -- 1e-5 relative, flat (north_star).
    spread = mspread1 = mspread2 = rspread = 0.0
    try:
        for mode in (0, 1, 2, 3):
            oracle_mod.set_exp_mode(mode)
            om, ot = oracle_mod.approxmatch(a, c)
            spread = max(spread, np.abs(om - om64).max())
            mspread1 = max(mspread1, np.abs(om.sum(1) - om64.sum(1)).max())
            mspread2 = max(mspread2, np.abs(om.sum(2) - om64.sum(2)).max())
            rspread = max(rspread, np.abs(ot[:, : n + m] - ot64[:, : n + m]).max())
    finally:
        oracle_mod.set_exp_mode(0)
    err_ours = np.abs(got - om64).max()
    assert err_ours <= max(3 * spread, 5e-5), (err_ours, spread)
    assert np.abs(got.sum(1) - om64.sum(1)).max() <= max(3 * mspread1, 1e-5)
    assert np.abs(got.sum(2) - om64.sum(2)).max() <= max(3 * mspread2, 1e-5)
    np.testing.assert_allclose(got.sum((1, 2)), om64.sum((1, 2)), rtol=1e-5)
    assert np.abs(gtemp - ot64[:, : n + m]).max() <= max(3 * rspread, 1e-5), rspread  # remainL | remainR
    # cost: 1e-5 relative against the float64 recurrence's cost (north_star tolerance), no widening
    cost = backend.MatchCost(_dev(a, cuda), _dev(c, cuda), match).cpu().numpy()
    oc64 = oracle_mod.matchcost_f64(a, c, om64)
    np.testing.assert_allclose(cost, oc64, rtol=1e-5, atol=1e-7)
    return got, cost


# the 19 passes of one approximate EMD under their launch-profile names, on the kernels without skip logic
PLAIN_PASSES = ({'am_phase_kernel<A> L0 plain', 'am_phase_kernel<C> L8 plain'} | {f'am_phase_kernel<B> L{i} plain' for i in range(9)}
                | {f'am_phase_kernel<CA> L{i} plain' for i in range(8)})


@pytest.mark.parametrize('b,n,m', [(2, 64, 64), (2, 257, 130), (1, 513, 512), (2, 1024, 1024)])
@pytest.mark.parametrize('kind', ['recon', 'uniform'])
def test_plain_passes_vs_oracle(cuda, oracle_mod, b, n, m, kind, capsys):
    """The am_nocull switch (include/pcc_test_hooks.h) runs all 19 passes on the plain am_phase_kernel variants -- the
    arithmetic behind the no-skip roofline bench.py reports.  ApproxMatch + MatchCost, the implicit match_cost and
    chamfer_emd under it are held to the bars of the product path (test_approxmatch_vs_oracle, tests.util.check_match_cost),
    and the launch record proves what ran: each plain pass once, no fine-level, owner-compacted or list variant, no
    resident launch -- and, with the switch at 0, at least one of those, so the switch acts.  Printed, not asserted: the
    largest difference between the skipping and the no-skip result."""
    from pointcloudcounterfactual_amd import _lib, backend
    from tests.util import check_match_cost
    from tests.which_ran import family, ran

    def passes(names):
        return set(family(names, 'am_phase_kernel', 'am_fine'))

    a, c = pair(300 + n + m, b, n, m, kind)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    (match0, _), names = ran(lambda: backend.ApproxMatch(t1, t2))
    assert passes(names) - PLAIN_PASSES, names  # the product skips somewhere
    cost0, g0, h0 = backend.MatchCostImplicit(t1, t2, True)
    with _lib.tuning('am_nocull', 1):
        (match, _cost), names = ran(lambda: _approxmatch_inside_the_oracle_bars(cuda, oracle_mod, a, c))
        assert passes(names) == PLAIN_PASSES and all(names[p] == 1 for p in PLAIN_PASSES), names
        (cost, g1, g2), names = ran(lambda: backend.MatchCostImplicit(t1, t2, True))
        assert passes(names) == PLAIN_PASSES and all(names[p] == 1 for p in PLAIN_PASSES), names
        check_match_cost(oracle_mod, a, c, cost.cpu().numpy(), g1.cpu().numpy(), g2.cpu().numpy())
        (loss, j1, j2, emd, e1, e2, d1, d2), names = ran(lambda: backend.ChamferEMD(t1, t2, True, True, return_dist=True))
        assert passes(names) == PLAIN_PASSES and all(names[p] == 1 for p in PLAIN_PASSES), names
        check_match_cost(oracle_mod, a, c, emd.cpu().numpy(), e1.cpu().numpy(), e2.cpu().numpy())
    ref_loss, r1, i1, r2, i2 = backend.ChamferLoss(t1, t2, True)  # the Chamfer half: the bits of the exhaustive search
    assert torch.equal(loss, ref_loss) and torch.equal(j1, i1) and torch.equal(j2, i2) and torch.equal(d1, r1) and torch.equal(d2, r2)
    # ... which are the oracle's, bit for bit (as in test_nndistance_bit_exact): the sorted search of chamfer_emd held to it directly
    od1, oi1, od2, oi2 = oracle_mod.nndistance(a, c)
    assert np.array_equal(j1.cpu().numpy(), oi1) and np.array_equal(j2.cpu().numpy(), oi2)
    assert np.array_equal(d1.cpu().numpy(), od1) and np.array_equal(d2.cpu().numpy(), od2)
    with capsys.disabled():
        print(f'\n  no-skip against skipping, ({b}, {n}, {m}) {kind}: match {float((torch.from_numpy(match).to(cuda) - match0).abs().max()):.3e}'
              f' cost {float((cost - cost0).abs().max()):.3e} grad {max(float((g1 - g0).abs().max()), float((g2 - h0).abs().max())):.3e}')


@pytest.mark.parametrize('b,n,m', [(2, 3, 5), (2, 257, 130), (2, 1024, 1024), (1, 100, 2100)])
def test_matchcost_and_grad_given_match(cuda, oracle_mod, b, n, m):
    """MatchCost / MatchCostGrad on the ORACLE's match: isolates these kernels from the recurrence."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(400 + n, b, n, m)
    om, _ = oracle_mod.approxmatch(a, c)
    t1, t2, tm = _dev(a, cuda), _dev(c, cuda), _dev(om, cuda)
    cost = backend.MatchCost(t1, t2, tm).cpu().numpy()
    oc64 = oracle_mod.matchcost_f64(a, c, om.astype(np.float64))
    np.testing.assert_allclose(cost, oc64, rtol=1e-5)
    g1, g2 = backend.MatchCostGrad(t1, t2, tm)
    h1, h2 = oracle_mod.matchcostgrad_f64(a, c, om.astype(np.float64))
    scale = max(np.abs(h1).max(), np.abs(h2).max())
    np.testing.assert_allclose(g1.cpu().numpy(), h1, rtol=1e-5, atol=1e-5 * scale)
    np.testing.assert_allclose(g2.cpu().numpy(), h2, rtol=1e-5, atol=1e-5 * scale)


def test_match_cost_fused_equals_two_step(cuda):
    from pointcloudcounterfactual_amd import backend

    a, c = pair(17, 3, 500, 384)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    match, temp = backend.ApproxMatch(t1, t2)
    cost = backend.MatchCost(t1, t2, match)
    match2, temp2, cost2 = backend.ApproxMatchCost(t1, t2)
    assert torch.equal(match, match2) and torch.equal(temp, temp2)
    np.testing.assert_allclose(cost2.cpu().numpy(), cost.cpu().numpy(), rtol=1e-5)


def test_approxmatch_known_answers(cuda):
    """n=m=1 at distance r: match=1, cost=r, grad1=(p1-p2)/r."""
    from structural_losses import match_cost

    p = torch.tensor([[[0.0, 0.0, 0.0]]], device=cuda, requires_grad=True)
    q = torch.tensor([[[0.3, 0.4, 0.0]]], device=cuda, requires_grad=True)
    cost = match_cost(p, q)
    cost.sum().backward()
    np.testing.assert_allclose(cost.item(), 0.5, rtol=1e-6)
    np.testing.assert_allclose(p.grad.cpu().numpy(), [[[-0.6, -0.8, 0.0]]], rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(q.grad.cpu().numpy(), [[[0.6, 0.8, 0.0]]], rtol=1e-5, atol=1e-7)


def test_backend_input_checks(cuda):
    from pointcloudcounterfactual_amd import backend

    x = torch.zeros(1, 4, 3)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        backend.NNDistance(x, x)
    y = torch.zeros(1, 3, 4, device=cuda).transpose(1, 2)
    with pytest.raises(RuntimeError, match='must be contiguous'):
        backend.ApproxMatch(y, y)


@pytest.mark.parametrize('kind', ['recon', 'uniform'])
def test_full_size_properties(cuda, kind):
    """BASELINE config 2/3 sizes (B=32, N=2048): size-independent properties instead of the oracle."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(1234 + 2, 32, 2048, 2048, kind)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    d1, i1, d2, i2 = backend.NNDistance(t1, t2)
    # gather check: returned distance == distance to the returned index (exact), and no candidate is closer
    g = torch.gather(t2, 1, i1.long()[..., None].expand(-1, -1, 3))
    assert torch.equal(((g - t1) ** 2).sum(-1) >= 0, torch.ones_like(d1, dtype=torch.bool))
    D = torch.cdist(t1.double(), t2.double()) ** 2
    assert (D.min(2)[0] - d1.double()).abs().max() < 1e-6
    assert (D.min(1)[0] - d2.double()).abs().max() < 1e-6
    # permutation equivariance of the argmin
    perm = torch.randperm(2048, device=cuda)
    e1, j1, e2, j2 = backend.NNDistance(t1[:, perm].contiguous(), t2)
    assert torch.equal(e1, d1[:, perm]) and torch.equal(j1, i1[:, perm])
    assert torch.equal(e2, d2)
    # approximate EMD: mass conservation (row mass <= multiR=1, column mass <= multiL=1), total mass ~ N
    match, temp = backend.ApproxMatch(t1, t2)
    assert match.min() >= 0
    assert match.sum(1).max() <= 1 + 1e-5 and match.sum(2).max() <= 1 + 1e-5
    assert (match.sum((1, 2)) > 2048 * 0.98).all()
    cost = backend.MatchCost(t1, t2, match)
    # cost is bounded below by the nearest-neighbour transport and above by mass * diameter
    lower = 0.5 * (d1.sqrt().sum(1) + d2.sqrt().sum(1)) * 0.98
    assert (cost >= lower * 0.99).all() and (cost <= 2048 * 2.0).all()


@pytest.mark.parametrize('tag', list('abcde'))
def test_against_committed_golden_fixture(cuda, tag):
    """HIP path vs tests/golden/oracle_structural.npz (no oracle build needed for this one)."""
    import os

    from pointcloudcounterfactual_amd import backend

    z = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'oracle_structural.npz'), allow_pickle=False)
    s1, s2 = _dev(z[f'{tag}_set1'], cuda), _dev(z[f'{tag}_set2'], cuda)
    d1, i1, d2, i2 = backend.NNDistance(s1, s2)
    assert np.array_equal(d1.cpu().numpy(), z[f'{tag}_dist1']) and np.array_equal(i1.cpu().numpy(), z[f'{tag}_idx1'])
    assert np.array_equal(d2.cpu().numpy(), z[f'{tag}_dist2']) and np.array_equal(i2.cpu().numpy(), z[f'{tag}_idx2'])
    g1, g2 = backend.NNDistanceGrad(s1, s2, i1, i2, _dev(z[f'{tag}_gdist1'], cuda), _dev(z[f'{tag}_gdist2'], cuda))
    np.testing.assert_allclose(g1.cpu().numpy(), z[f'{tag}_nngrad1'], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g2.cpu().numpy(), z[f'{tag}_nngrad2'], rtol=1e-5, atol=1e-6)
    match, temp, cost = backend.ApproxMatchCost(s1, s2)
    np.testing.assert_allclose(cost.cpu().numpy(), z[f'{tag}_cost'], rtol=1e-5)
    gm1, gm2 = backend.MatchCostGrad(s1, s2, _dev(z[f'{tag}_match'], cuda))
    scale = max(np.abs(z[f'{tag}_mgrad1']).max(), np.abs(z[f'{tag}_mgrad2']).max())
    np.testing.assert_allclose(gm1.cpu().numpy(), z[f'{tag}_mgrad1'], rtol=1e-5, atol=1e-5 * scale)
    np.testing.assert_allclose(gm2.cpu().numpy(), z[f'{tag}_mgrad2'], rtol=1e-5, atol=1e-5 * scale)


def test_bit_reproducible_run_to_run(cuda):
    """No float atomics on the forward path and fixed-order two-stage reductions: two runs give the same bits
    (the reference's unordered atomics do not).  The Chamfer backward accumulates with LDS float atomics and is
    only reproducible to rounding when three or more neighbours share a target."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(31, 8, 2048, 2048)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    r1 = backend.ApproxMatchCost(t1, t2)
    n1 = backend.NNDistance(t1, t2)
    g1 = backend.MatchCostGrad(t1, t2, r1[0])
    for _ in range(3):
        r2 = backend.ApproxMatchCost(t1, t2)
        n2 = backend.NNDistance(t1, t2)
        g2 = backend.MatchCostGrad(t1, t2, r2[0])
        assert all(torch.equal(x, y) for x, y in zip(r1, r2))
        assert all(torch.equal(x, y) for x, y in zip(n1, n2))
        assert all(torch.equal(x, y) for x, y in zip(g1, g2))


def test_match_cost_autograd_modes_agree(cuda):
    """match_cost in its three modes -- 'implicit' (pcc_match_cost: no match tensor), 'fused' (pcc_approxmatch_cost,
    pcc_matchcostgrad_scaled) and 'reference' (the reference's call sequence ApproxMatch -> MatchCost ->
    MatchCostGrad -> grad * grad_output, match_cost.py:25-42) -- gives the same cost and gradients."""
    from pointcloudcounterfactual_amd.losses import MatchCostFunction, match_cost

    a, c = pair(23, 3, 700, 512)
    w = torch.tensor([0.5, -2.0, 3.0], device=cuda)
    res = {}
    try:
        for mode in ('reference', 'fused', 'implicit'):
            MatchCostFunction.mode = mode
            t1 = _dev(a, cuda).requires_grad_(True)
            t2 = _dev(c, cuda).requires_grad_(True)
            cost = match_cost(t1, t2)
            (cost * w).sum().backward()
            res[mode] = (cost.detach().cpu().numpy(), t1.grad.cpu().numpy(), t2.grad.cpu().numpy())
    finally:
        MatchCostFunction.mode = 'implicit'
    ref = res['reference']
    np.testing.assert_allclose(res['fused'][0], ref[0], rtol=1e-5)
    np.testing.assert_allclose(res['implicit'][0], ref[0], rtol=1e-5)
    scale = max(np.abs(ref[1]).max(), np.abs(ref[2]).max())
    for k in (1, 2):
        np.testing.assert_allclose(res['fused'][k], ref[k], rtol=1e-6, atol=1e-7)
        # same match elements bit for bit; only the order of the row / column sums differs
        np.testing.assert_allclose(res['implicit'][k], ref[k], rtol=1e-5, atol=1e-5 * scale)


IM_SHAPES = [(1, 1, 1), (2, 3, 5), (2, 64, 64), (2, 257, 130), (2, 128, 256), (1, 513, 512), (2, 1024, 1024),
             (1, 2100, 2300), (1, 4099, 100), (2, 70, 2050), (4, 2048, 2048)]


@pytest.mark.parametrize('b,n,m', IM_SHAPES)
@pytest.mark.parametrize('kind', ['recon', 'uniform'])
def test_implicit_match_cost_equals_materialised(cuda, b, n, m, kind):
    """pcc_match_cost (match never stored; sorted index space, exact-zero levels skipped per column box) against the
    materialised path of the same library: the match elements are the same bits, so cost and gradients agree to the
    rounding of the differently ordered sums (1e-5 of the largest gradient component)."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(900 + n + m, b, n, m, kind)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    match, _temp, cost = backend.ApproxMatchCost(t1, t2)
    g1, g2 = backend.MatchCostGrad(t1, t2, match)
    only_cost, = backend.MatchCostImplicit(t1, t2, False)
    cost_i, h1, h2 = backend.MatchCostImplicit(t1, t2, True)
    # the gradient variant takes sqrt(d2) as d2 * rsqrt(max(d2, 1e-20)) (one transcendental for cost and gradient)
    np.testing.assert_allclose(only_cost.cpu().numpy(), cost_i.cpu().numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(cost_i.cpu().numpy(), cost.cpu().numpy(), rtol=1e-5, atol=1e-7)
    scale = max(float(g1.abs().max()), float(g2.abs().max()), 1e-30)
    np.testing.assert_allclose(h1.cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-5 * scale)
    np.testing.assert_allclose(h2.cpu().numpy(), g2.cpu().numpy(), rtol=1e-5, atol=1e-5 * scale)


@pytest.mark.parametrize('b,n,m', [(2, 3, 5), (2, 257, 130), (2, 1024, 1024)])
def test_implicit_match_cost_vs_oracle(cuda, oracle_mod, b, n, m):
    """pcc_match_cost against the float64 recurrence of the oracle: cost to a flat 1e-5 (north_star), gradients within
    3x the spread of the oracle's own legitimate float32 evaluations (the match elements are ill-conditioned, see
    test_approxmatch_vs_oracle; floor 5e-5 of the largest component where that spread is at rounding level)."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(300 + n + m, b, n, m)
    cost, g1, g2 = backend.MatchCostImplicit(_dev(a, cuda), _dev(c, cuda), True)
    om64, _ = oracle_mod.approxmatch_f64(a, c)
    oc64 = oracle_mod.matchcost_f64(a, c, om64)
    np.testing.assert_allclose(cost.cpu().numpy(), oc64, rtol=1e-5, atol=1e-7)
    # the cost-only call (am_pair_kernel<cost>: no gradient sums, sqrt taken directly) against the same float64 cost, same bar
    only_cost, = backend.MatchCostImplicit(_dev(a, cuda), _dev(c, cuda), False)
    np.testing.assert_allclose(only_cost.cpu().numpy(), oc64, rtol=1e-5, atol=1e-7)
    h1, h2 = oracle_mod.matchcostgrad_f64(a, c, om64)
    scale = max(np.abs(h1).max(), np.abs(h2).max())
    spread = 0.0
    try:
        for mode in (0, 1, 2, 3):  # legitimate float32 evaluations of the reference's formulas (oracle exp modes)
            oracle_mod.set_exp_mode(mode)
            om, _ = oracle_mod.approxmatch(a, c)
            f1, f2 = oracle_mod.matchcostgrad(a, c, om)
            spread = max(spread, np.abs(f1 - h1).max(), np.abs(f2 - h2).max())
    finally:
        oracle_mod.set_exp_mode(0)
    assert np.abs(g1.cpu().numpy() - h1).max() <= max(3 * spread, 5e-5 * scale)
    assert np.abs(g2.cpu().numpy() - h2).max() <= max(3 * spread, 5e-5 * scale)


def test_implicit_match_cost_edge_cases(cuda):
    from pointcloudcounterfactual_amd import _lib, backend

    # far clouds: every exponential underflows -> no mass, cost 0, zero gradients
    a, c = pair(5, 2, 300, 300)
    t1, t2 = _dev(a, cuda), _dev(c + 40.0, cuda)
    cost, g1, g2 = backend.MatchCostImplicit(t1, t2, True)
    assert float(cost.abs().max()) == 0.0 and float(g1.abs().max()) == 0.0 and float(g2.abs().max()) == 0.0
    # identical clouds: all mass on the diagonal, d = 0 -> cost ~ 0 and finite gradients (rsqrt(max(d2, 1e-20)))
    t = _dev(a, cuda)
    cost, g1, g2 = backend.MatchCostImplicit(t, t, True)
    assert torch.isfinite(g1).all() and torch.isfinite(g2).all()
    ref_cost = backend.ApproxMatchCost(t, t)[2]
    np.testing.assert_allclose(cost.cpu().numpy(), ref_cost.cpu().numpy(), rtol=1e-5, atol=1e-6)
    # empty batch / empty clouds
    e = torch.empty(0, 5, 3, device=cuda)
    assert backend.MatchCostImplicit(e, e, True)[0].shape == (0,)
    z1, z2 = torch.zeros(2, 0, 3, device=cuda), torch.zeros(2, 4, 3, device=cuda)
    cost, g1, g2 = backend.MatchCostImplicit(z1, z2, True)
    assert float(cost.abs().sum()) == 0.0 and g1.shape == (2, 0, 3) and float(g2.abs().sum()) == 0.0
    # the other entry points zero-fill empty clouds too (C ABI, outputs pre-filled with NaN; temp is not written)
    lib, st = _lib.lib, torch.cuda.current_stream(cuda).cuda_stream

    def nan(*shape):
        return torch.full(shape, float('nan'), device=cuda)

    for n, m in ((0, 4), (4, 0)):
        x1, x2 = torch.zeros(2, n, 3, device=cuda), torch.zeros(2, m, 3, device=cuda)
        match, temp = torch.zeros(2, m, n, device=cuda), nan(2, 2 * (n + m))
        cost = nan(2)
        assert lib.pcc_approxmatch_cost(2, n, m, x1.data_ptr(), x2.data_ptr(), match.data_ptr(), temp.data_ptr(),
                                        cost.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(cost, torch.zeros_like(cost))
        cost = nan(2)
        assert lib.pcc_matchcost(2, n, m, x1.data_ptr(), x2.data_ptr(), match.data_ptr(), cost.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert torch.equal(cost, torch.zeros_like(cost))
        for scaled in (False, True):
            g1, g2, gc = nan(2, n, 3), nan(2, m, 3), torch.ones(2, device=cuda)
            if scaled:
                rc = lib.pcc_matchcostgrad_scaled(2, n, m, x1.data_ptr(), x2.data_ptr(), match.data_ptr(), gc.data_ptr(),
                                                  g1.data_ptr(), g2.data_ptr(), st)
            else:
                rc = lib.pcc_matchcostgrad(2, n, m, x1.data_ptr(), x2.data_ptr(), match.data_ptr(), g1.data_ptr(),
                                           g2.data_ptr(), st)
            torch.cuda.synchronize()
            assert rc == 0 and torch.equal(g1, torch.zeros_like(g1)) and torch.equal(g2, torch.zeros_like(g2))


def test_implicit_match_cost_bit_reproducible(cuda):
    from pointcloudcounterfactual_amd import backend

    a, c = pair(32, 8, 2048, 2048)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    r1 = backend.MatchCostImplicit(t1, t2, True)
    for _ in range(3):
        r2 = backend.MatchCostImplicit(t1, t2, True)
        assert all(torch.equal(x, y) for x, y in zip(r1, r2))


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('b,n,m', [(2, 3, 5), (3, 257, 130), (2, 2048, 2048)])
def test_chamfer_fused_equals_nn_distance_expression(cuda, b, n, m, reduction):
    """chamfer() (pcc_chamfer_loss / pcc_chamfer_loss_grad: reductions inside the library) == the same loss written
    with nn_distance and torch reductions (pykeops_chamfer / torch_chamfer shape, metrics_and_losses.py:21-47)."""
    from pointcloudcounterfactual_amd.losses import chamfer, nn_distance

    a, c = pair(55 + n, b, n, m)
    w = torch.linspace(-1.0, 2.0, b, device=cuda)
    t1 = _dev(a, cuda).requires_grad_(True)
    t2 = _dev(c, cuda).requires_grad_(True)
    loss = chamfer(t1, t2, reduction)
    (loss * w).sum().backward()
    u1 = _dev(a, cuda).requires_grad_(True)
    u2 = _dev(c, cuda).requires_grad_(True)
    d1, d2 = nn_distance(u1, u2)
    ref = d2.mean(1) + d1.mean(1) if reduction == 'mean' else d1.sum(1) + d2.sum(1)
    (ref * w).sum().backward()
    np.testing.assert_allclose(loss.detach().cpu().numpy(), ref.detach().cpu().numpy(), rtol=2e-6)
    np.testing.assert_allclose(t1.grad.cpu().numpy(), u1.grad.cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(t2.grad.cpu().numpy(), u2.grad.cpu().numpy(), rtol=1e-5, atol=1e-7)
    with pytest.raises(ValueError):
        chamfer(t1, t2, 'max')


def test_two_lane_schedule_equals_single_stream(cuda):
    """At the bench size (B=32, N=2048) the level passes run as two half-batch lanes on two streams.
    Per sample nothing changes, so the results carry the same bits as the single-stream schedule (measurement switch
    `am_nosplit`, include/pcc_test_hooks.h), run to run.  The launch record shows the schedule: every pass launched twice
    per call, once per lane, and once under the switch."""
    from pointcloudcounterfactual_amd import _lib, backend
    from tests.which_ran import family, ran

    def launches_per_pass(names):
        passes = family(names, 'am_phase_kernel')
        assert len(passes) == 19, names  # (the 19 passes; 65536 owners x tiles: no resident launch at this size)
        return set(passes.values())

    a, c = pair(91, 32, 2048, 2048)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    r1, names = ran(lambda: backend.MatchCostImplicit(t1, t2, True))
    assert launches_per_pass(names) == {2}
    r2 = backend.MatchCostImplicit(t1, t2, True)
    assert all(torch.equal(x, y) for x, y in zip(r1, r2))
    m1 = backend.ApproxMatchCost(t1, t2)
    rowmass1 = m1[0].sum(2)
    temp1, mc1 = m1[1].clone(), m1[2].clone()
    del m1
    with _lib.tuning('am_nosplit', 1):
        s1, names = ran(lambda: backend.MatchCostImplicit(t1, t2, True))
        assert launches_per_pass(names) == {1}
        sm = backend.ApproxMatchCost(t1, t2)
        torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(r1, s1))
    assert torch.equal(mc1, sm[2]) and torch.equal(temp1, sm[1]) and torch.equal(rowmass1, sm[0].sum(2))


def test_resident_fine_levels_equal_one_launch_per_pass(cuda):
    """Levels 0-2 (passes A0 B0 CA0 B1 CA1 B2 CA2) run as ONE resident launch with per-sample barriers
    (am_fine_persist_kernel) when both clouds fit its LDS (<= 2048 points) and the whole launch fits the device
    (batch x tiles <= compute units: b <= 8 at N = 2048); the measurement switch `am_noresident` runs them as one
    launch per pass (am_fine_kernel).  Same walk, same reduction order: every output carries the same bits -- cost,
    both gradients, the materialised path's cost, temp (remainL | remainR | ratioL | ratioR of the last level) and the
    row masses of match -- at the largest qualifying batch, at unequal clouds, at ragged sizes and at clouds smaller
    than one tile.  The launch record shows which ran: the resident launch and no fine-level pass of its own where the
    rule above admits it, the seven fine-level passes and no resident launch under the switch."""
    from pointcloudcounterfactual_amd import _lib, backend
    from tests.which_ran import family, ran

    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    fine = {'am_phase_kernel<A> L0 fine'} | {f'am_phase_kernel<{p}> L{i} fine' for p in ('B', 'CA') for i in range(3)}
    shapes = [(8, 2048, 2048, 'recon'), (3, 1000, 2048, 'recon'), (2, 2048, 700, 'uniform'), (5, 257, 130, 'recon'),
              (2, 40, 17, 'uniform'), (9, 1024, 1024, 'uniform'), (1, 1, 1, 'recon')]

    def run(k, b, n, m, kind):
        a, c = pair(300 + k, b, n, m, kind)
        t1, t2 = _dev(a, cuda), _dev(c, cuda)
        (cost, g1, g2), names = ran(lambda: backend.MatchCostImplicit(t1, t2, True))
        (mt, t, mc), more = ran(lambda: backend.ApproxMatchCost(t1, t2))
        for record in (names, more):
            assert set(family(record, 'am_fine_persist_kernel', *fine)) == expected, (b, n, m, record)
        return {'cost': cost, 'g1': g1, 'g2': g2, 'mc': mc, 'temp': t, 'rowmass': mt.sum(2)}

    for k, shape in enumerate(shapes):
        b, n, m, _ = shape
        assert max(n, m) <= 2048 and b * -(-max(n, m) // 64) <= cus  # (every shape qualifies for the resident launch)
        expected = {'am_fine_persist_kernel'}
        resident = run(k, *shape)
        with _lib.tuning('am_noresident', 1):
            expected = fine
            per_pass = run(k, *shape)
            torch.cuda.synchronize()
        for name in resident:
            assert np.array_equal(resident[name].cpu().numpy(), per_pass[name].cpu().numpy(), equal_nan=True), (name, shape)
        assert torch.isfinite(resident['cost']).all()


def test_resident_failure_is_reported_not_silent(cuda):
    """A resident launch of levels 0-2 whose sample barriers fail (here: injected through the test hook, which makes every
    sample fail at its first barrier) gives NaN for its samples on both paths -- cost and gradients of the implicit path,
    match / temp / cost of the materialising one -- AND surfaces as an error: the next call on the device raises
    instead of starting, and the call after it is finite again."""
    from pointcloudcounterfactual_amd import _lib, backend

    a, c = pair(61, 4, 2048, 2048, 'recon')
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    assert _lib.lib.pcc_test_inject_approxmatch_failure() == 1  # armed: tests/conftest.py sets PCC_TEST_HOOKS=1
    cost, g1, g2 = backend.MatchCostImplicit(t1, t2, True)
    torch.cuda.synchronize()
    assert torch.isnan(cost).all() and torch.isnan(g1).all() and torch.isnan(g2).all()
    with pytest.raises(RuntimeError, match='did not complete'):
        backend.MatchCostImplicit(t1, t2, True)
    cost, g1, g2 = backend.MatchCostImplicit(t1, t2, True)
    torch.cuda.synchronize()
    assert torch.isfinite(cost).all() and torch.isfinite(g1).all() and torch.isfinite(g2).all()

    assert _lib.lib.pcc_test_inject_approxmatch_failure() == 1
    match, temp, mc = backend.ApproxMatchCost(t1, t2)
    torch.cuda.synchronize()
    assert torch.isnan(match).all() and torch.isnan(temp).all() and torch.isnan(mc).all()
    with pytest.raises(RuntimeError, match='did not complete'):
        backend.ApproxMatchCost(t1, t2)
    match, temp, mc = backend.ApproxMatchCost(t1, t2)
    torch.cuda.synchronize()
    assert torch.isfinite(match).all() and torch.isfinite(temp).all() and torch.isfinite(mc).all()


def test_stale_workspace_does_not_leak_into_results(cuda):
    """The library's scratch comes from a stream-ordered pool and is not cleared; the suite runs with PCC_WS_POISON=1
    (conftest.py), which fills every workspace with NaN patterns first.  Results must not depend on it: a call repeated
    after other library calls have recycled the pool returns the same bits (sizes whose dense candidate lists end in a
    partial float4 group, the case that once multiplied a stale NaN coordinate by a zero weight)."""
    import os

    from pointcloudcounterfactual_amd import backend
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    assert os.environ.get('PCC_WS_POISON') == '1'
    for seed, b, n, m in ((3, 2, 1024, 1024), (4, 3, 777, 1530), (5, 9, 2048, 2048)):
        a, c = pair(seed, b, n, m, 'uniform')
        t1, t2 = _dev(a, cuda), _dev(c, cuda)
        first = [x.clone() for x in backend.MatchCostImplicit(t1, t2, True)]
        ops.hip_knn(t1.transpose(1, 2).contiguous(), 7)  # other users of the pool in between
        backend.NNDistance(t1, t2)
        again = backend.MatchCostImplicit(t1, t2, True)
        assert all(torch.isfinite(x).all() for x in first)
        assert all(torch.equal(x, y) for x, y in zip(first, again))


def test_non_finite_coordinates_follow_the_reference(cuda, oracle_mod):
    """NaN / infinite coordinates.  The reference has no guard: a NaN coordinate reaches the sums through the distances; an
    infinite one makes its point's pairs exp(-inf) = 0, which matchcost then multiplies by sqrt(inf) -- NaN cost
    (approxmatch.cu:207).  The implicit path skips exact zeros, so it flags such a sample and reports NaN cost and
    gradients for it; the other samples of the batch are untouched.  The NaN patterns of cost (and of grad1 for a NaN
    input) equal the oracle's."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(7, 3, 512, 512, 'recon')
    base = [x.cpu().numpy() for x in backend.MatchCostImplicit(_dev(a, cuda), _dev(c, cuda), True)]
    for which, smp, val in ((0, 0, np.nan), (1, 1, np.inf), (0, 2, -np.inf)):
        x, y = a.copy(), c.copy()
        (x if which == 0 else y)[smp, 100, 1] = val
        cost, g1, g2 = [t.cpu().numpy() for t in backend.MatchCostImplicit(_dev(x, cuda), _dev(y, cuda), True)]
        _m, _t, cost_m = backend.ApproxMatchCost(_dev(x, cuda), _dev(y, cuda))
        om, _ = oracle_mod.approxmatch(x, y)
        oc = oracle_mod.matchcost(x, y, om)
        og1, _og2 = oracle_mod.matchcostgrad(x, y, om)
        assert np.array_equal(np.isnan(cost), np.isnan(oc)) and np.isnan(cost[smp]), (which, smp, val, cost, oc)
        assert np.array_equal(np.isnan(cost_m.cpu().numpy()), np.isnan(oc))
        keep = [s for s in range(3) if s != smp]
        assert np.array_equal(cost[keep], base[0][keep])
        assert np.array_equal(g1[keep], base[1][keep]) and np.array_equal(g2[keep], base[2][keep])
        assert np.isnan(g1[smp]).any() and np.isnan(g2[smp]).any()
        if np.isnan(val):
            assert np.array_equal(np.isnan(g1).any(-1), np.isnan(og1).any(-1))
        else:  # every gradient of the other cloud involves the infinite point (reference: 0 * inf)
            assert np.isnan((g1 if which == 1 else g2)[smp]).all()


def test_calls_on_two_caller_streams_at_once(cuda):
    """Two caller streams enqueue library calls back to back without synchronising in between: both calls fork onto the one
    internal side stream of the device, draw their scratch from the one pool, and must still return what each returns
    alone (stream-ordered allocation, fork / join events per call)."""
    from pointcloudcounterfactual_amd import backend
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    a1, c1 = pair(31, 32, 2048, 2048, 'recon')
    a2, c2 = pair(32, 16, 1500, 2048, 'uniform')
    t = [_dev(v, cuda) for v in (a1, c1, a2, c2)]
    alone = [backend.ChamferEMD(t[0], t[1], True, True), backend.ChamferEMD(t[2], t[3], True, True),
             ops.hip_knn(t[2].transpose(1, 2).contiguous(), 20)]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    pts = t[2].transpose(1, 2).contiguous()
    outs = [[], [], []]
    for _ in range(4):
        with torch.cuda.stream(s1):
            outs[0].append(backend.ChamferEMD(t[0], t[1], True, True))
        with torch.cuda.stream(s2):
            outs[1].append(backend.ChamferEMD(t[2], t[3], True, True))
            outs[2].append(ops.hip_knn(pts, 20))
    torch.cuda.synchronize()
    for r in outs[0]:
        assert all(torch.equal(x, y) for x, y in zip(r, alone[0]) if torch.is_tensor(x))
    for r in outs[1]:
        assert all(torch.equal(x, y) for x, y in zip(r, alone[1]) if torch.is_tensor(x))
    for r in outs[2]:
        assert torch.equal(r, alone[2])


def test_two_host_threads_call_the_library_at_once(cuda):
    """ctypes releases the GIL: two Python threads are inside the library's host code at the same time, each on its own
    stream (the side stream, the pool, the profiling and error state are shared or per-thread).  Results equal the
    serial ones."""
    import threading

    from pointcloudcounterfactual_amd import backend
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    a1, c1 = pair(41, 32, 2048, 2048, 'recon')
    a2, c2 = pair(42, 9, 1000, 1300, 'uniform')
    t = [_dev(v, cuda) for v in (a1, c1, a2, c2)]
    pts = t[2].transpose(1, 2).contiguous()
    want = [backend.ChamferEMD(t[0], t[1], True, True), backend.MatchCostImplicit(t[2], t[3], True), ops.hip_knn(pts, 16)]
    torch.cuda.synchronize()
    got = [[], []]
    errs = []

    def work(which):
        try:
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                for _ in range(10):
                    if which == 0:
                        got[0].append(backend.ChamferEMD(t[0], t[1], True, True))
                    else:
                        got[1].append((backend.MatchCostImplicit(t[2], t[3], True), ops.hip_knn(pts, 16)))
            st.synchronize()
        except Exception as e:  # surfaced below: an exception in a thread would otherwise vanish
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    [x.start() for x in th]
    [x.join() for x in th]
    torch.cuda.synchronize()
    assert not errs, errs
    for r in got[0]:
        assert all(torch.equal(x, y) for x, y in zip(r, want[0]))
    for emd, knn in got[1]:
        assert all(torch.equal(x, y) for x, y in zip(emd, want[1])) and torch.equal(knn, want[2])


def test_package_import_before_torch(cuda):
    """The library must share torch's HIP runtime whatever the import order (``_lib`` imports torch before it loads
    the shared object): a fresh process that imports the package first, as ``__graft_entry__.build()`` followed by
    ``smoke()`` does, runs the kernels."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import pointcloudcounterfactual_amd, structural_losses, emd, pykeops\n"
        "import torch\n"
        "from structural_losses import nn_distance\n"
        "x = torch.rand(2, 64, 3, device='cuda')\n"
        "d1, d2 = nn_distance(x, x)\n"
        "assert float(d1.abs().max()) == 0.0\n"
        "print('ok')\n"
    ) % root
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'ok' in r.stdout, r.stderr[-2000:]


def test_random_shape_sweep(cuda, oracle_mod):
    """Seeded sweep over awkward shapes (sizes that are not multiples of 4 / 16 / 64, very unequal clouds, batches that
    do and do not split into lanes): Chamfer bit-exact vs the oracle; approximate EMD cost vs the float64 recurrence;
    implicit path vs materialised path."""
    from pointcloudcounterfactual_amd import backend

    rng = np.random.default_rng(2026)
    for trial in range(24):
        b = int(rng.choice([1, 2, 3, 5, 9]))
        n = int(rng.integers(1, 700))
        m = int(rng.integers(1, 700))
        if trial % 6 == 0:
            n, m = int(rng.integers(2000, 2300)), int(rng.integers(1, 40))
        kind = 'uniform' if trial % 2 else 'recon'
        a, c = pair(5000 + trial, b, n, m, kind)
        t1, t2 = _dev(a, cuda), _dev(c, cuda)
        d1, i1, d2, i2 = backend.NNDistance(t1, t2)
        od1, oi1, od2, oi2 = oracle_mod.nndistance(a, c)
        assert np.array_equal(i1.cpu().numpy(), oi1) and np.array_equal(i2.cpu().numpy(), oi2), (b, n, m)
        assert np.array_equal(d1.cpu().numpy(), od1) and np.array_equal(d2.cpu().numpy(), od2), (b, n, m)
        match, _temp, cost = backend.ApproxMatchCost(t1, t2)
        g1, g2 = backend.MatchCostGrad(t1, t2, match)
        cost_i, h1, h2 = backend.MatchCostImplicit(t1, t2, True)
        om64, _ = oracle_mod.approxmatch_f64(a, c)
        oc64 = oracle_mod.matchcost_f64(a, c, om64)
        np.testing.assert_allclose(cost.cpu().numpy(), oc64, rtol=1e-5, atol=1e-6, err_msg=str((b, n, m, kind)))
        np.testing.assert_allclose(cost_i.cpu().numpy(), cost.cpu().numpy(), rtol=1e-5, atol=1e-6, err_msg=str((b, n, m, kind)))
        scale = max(float(g1.abs().max()), float(g2.abs().max()), 1e-30)
        np.testing.assert_allclose(h1.cpu().numpy(), g1.cpu().numpy(), rtol=1e-5, atol=1e-5 * scale, err_msg=str((b, n, m)))
        np.testing.assert_allclose(h2.cpu().numpy(), g2.cpu().numpy(), rtol=1e-5, atol=1e-5 * scale, err_msg=str((b, n, m)))


def test_lanes_with_odd_batch_and_unequal_clouds(cuda):
    """A batch that splits into two unequal lanes (9 samples -> 4 + 5) with n != m: every sample's cost and gradients
    carry the bits of the same sample run on its own (one lane, one stream)."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(313, 9, 4099, 3000)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    cost, g1, g2 = backend.MatchCostImplicit(t1, t2, True)
    match, _temp, mcost = backend.ApproxMatchCost(t1, t2)
    for s in (0, 3, 4, 8):
        cs, h1, h2 = backend.MatchCostImplicit(t1[s:s + 1].contiguous(), t2[s:s + 1].contiguous(), True)
        assert torch.equal(cs, cost[s:s + 1]) and torch.equal(h1, g1[s:s + 1]) and torch.equal(h2, g2[s:s + 1]), s
        ms, _ts, mc = backend.ApproxMatchCost(t1[s:s + 1].contiguous(), t2[s:s + 1].contiguous())
        assert torch.equal(mc, mcost[s:s + 1]) and torch.equal(ms, match[s:s + 1]), s


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('b,n,m', [(2, 3, 5), (3, 257, 130), (8, 2048, 2048)])
def test_chamfer_emd_node_equals_separate_losses(cuda, b, n, m, reduction):
    """chamfer_emd() (one autograd node: nearest-neighbour search on a side stream in the shadow of the approximate-EMD
    launch chain, one backward launch for the total gradient) carries the bits of chamfer() and match_cost() called one
    after the other, forward and backward, with per-sample upstream weights and with the expanded scalar that
    ``loss.sum().backward()`` hands down."""
    from pointcloudcounterfactual_amd.losses import chamfer, chamfer_emd, match_cost

    a, c = pair(700 + n, b, n, m)
    for weights in (None, torch.linspace(-1.0, 2.0, b, device=cuda)):
        t1 = _dev(a, cuda).requires_grad_(True)
        t2 = _dev(c, cuda).requires_grad_(True)
        lc, le = chamfer_emd(t1, t2, reduction)
        total = lc + 0.5 * le
        (total.sum() if weights is None else (total * weights).sum()).backward()
        u1 = _dev(a, cuda).requires_grad_(True)
        u2 = _dev(c, cuda).requires_grad_(True)
        rc, re = chamfer(u1, u2, reduction), match_cost(u1, u2)
        ref = rc + 0.5 * re
        (ref.sum() if weights is None else (ref * weights).sum()).backward()
        assert torch.equal(lc, rc) and torch.equal(le, re)
        # same products, same sums; the Chamfer scatter term accumulates with LDS float atomics whose order is free when
        # three or more neighbours share a target (as in pcc_nndistancegrad itself): rounding-level differences only
        for got, exp in ((t1.grad, u1.grad), (t2.grad, u2.grad)):
            np.testing.assert_allclose(got.cpu().numpy(), exp.cpu().numpy(), rtol=1e-5, atol=1e-6 * float(exp.abs().max()))
    # only one input requires a gradient / none does
    t1 = _dev(a, cuda).requires_grad_(True)
    lc, le = chamfer_emd(t1, _dev(c, cuda), reduction)
    (lc + le).sum().backward()
    assert t1.grad is not None and torch.isfinite(t1.grad).all()
    with torch.no_grad():
        lc2, le2 = chamfer_emd(_dev(a, cuda), _dev(c, cuda), reduction)
    assert torch.equal(lc2, lc)
    # the cost-only kernel takes sqrt(d2) directly, the gradient variant as d2 * rsqrt(d2): 2e-6, as for match_cost
    np.testing.assert_allclose(le2.cpu().numpy(), le.detach().cpu().numpy(), rtol=2e-6, atol=1e-7)


CE_SHAPES = NN_SHAPES + [(2, 40, 1200), (1, 5000, 3000), (1, 17000, 300), (33, 2048, 2048)]


@pytest.mark.parametrize('b,n,m', CE_SHAPES)
@pytest.mark.parametrize('kind', ['recon', 'uniform'])
def test_chamfer_emd_neighbours_are_the_exhaustive_ones(cuda, b, n, m, kind):
    """pcc_chamfer_emd finds the nearest neighbours on the clouds the EMD has sorted, visiting only the candidate blocks
    that can hold one (nn_sorted_kernel): indices and distances carry the bits of the exhaustive pcc_nndistance -- also
    across candidate chunks (> 2048), for clouds of more than 16384 points (17000: am_sort_kernel<64>; the clouds too large
    for the sort, > 32768 points, are in tests/test_gpu_sorted_search.py) and for batches that run as two lanes."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(4000 + n + m, b, n, m, kind)
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    d1, i1, d2, i2 = backend.NNDistance(t1, t2)
    loss, j1, j2, cost, e1, e2 = backend.ChamferEMD(t1, t2, True, False, return_dist=True)
    assert torch.equal(j1, i1) and torch.equal(j2, i2)
    assert torch.equal(e1, d1) and torch.equal(e2, d2)
    ref_loss = backend.ChamferLoss(t1, t2, True)[0]
    assert torch.equal(loss, ref_loss)
    ref_cost, = backend.MatchCostImplicit(t1, t2, False)
    assert torch.equal(cost, ref_cost)


def test_chamfer_emd_neighbour_ties_lowest_original_index(cuda):
    """Duplicate candidates: the lowest ORIGINAL index must win although the search runs in the sorted order
    (nndistance.cu:26,36,116)."""
    from pointcloudcounterfactual_amd import backend

    rng = np.random.default_rng(5)
    base = rng.random((2, 40, 3), dtype=np.float32)
    c = np.concatenate([base] * 30, axis=1)  # 1200 candidates, every point repeated 30x
    a = base[:, ::-1].copy()
    t1, t2 = _dev(a, cuda), _dev(c, cuda)
    d1, i1, d2, i2 = backend.NNDistance(t1, t2)
    _loss, j1, j2, _cost, e1, e2 = backend.ChamferEMD(t1, t2, False, False, return_dist=True)
    assert torch.equal(j1, i1) and torch.equal(j2, i2) and torch.equal(e1, d1) and torch.equal(e2, d2)
    assert int(j1.max()) < 40
    # a cloud against itself: every point is its own nearest neighbour at distance 0
    s = _dev(rng.random((3, 777, 3), dtype=np.float32), cuda)
    _loss, j1, j2, _cost, e1, e2 = backend.ChamferEMD(s, s, True, False, return_dist=True)
    ar = torch.arange(777, device=cuda, dtype=torch.int32).expand(3, -1)
    assert torch.equal(j1, ar) and torch.equal(j2, ar) and float(e1.abs().max()) == 0.0


def test_nndistance_non_finite_inputs_follow_the_reference(cuda, oracle_mod):
    """nndistance.cu:26-28 takes candidate 0 unconditionally and then only strict improvements: a NaN query point gives
    dist = NaN / index 0, a NaN candidate 0 poisons every query, a NaN candidate elsewhere never wins.  The oracle is the
    line-by-line restatement of that loop; the HIP kernel must show the same NaN pattern and the same finite results."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(77, 2, 300, 257)
    a[0, 5] = np.nan            # a NaN query in sample 0
    c[0, 9, 1] = np.nan         # a NaN candidate (not the first) in sample 0
    c[1, 0, 2] = np.nan         # NaN candidate 0 in sample 1
    d1, i1, d2, i2 = backend.NNDistance(_dev(a, cuda), _dev(c, cuda))
    od1, oi1, od2, oi2 = oracle_mod.nndistance(a, c)
    for got, exp in ((d1, od1), (d2, od2)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(exp))
        assert np.array_equal(g[~np.isnan(exp)], exp[~np.isnan(exp)])
    assert np.array_equal(i1.cpu().numpy(), oi1) and np.array_equal(i2.cpu().numpy(), oi2)
    assert np.isnan(od1[0, 5]) and np.isnan(od1[1]).all() and not np.isnan(od1[0, :5]).any()


def test_nndistance_nan_chunk_head_hides_its_chunk_like_the_reference(cuda, oracle_mod):
    """The reference's `k == 0` (nndistance.cu:26) is local to its 512-candidate chunks: a NaN candidate at index 512*c
    (c >= 1) becomes the chunk's `best`, nothing compares below NaN, and the cross-chunk merge (`result > best`, :116)
    drops the whole chunk -- candidates 512c .. 512c+511 are hidden.  The oracle restates that loop; the HIP kernel must
    give the same indices and distances (a NaN candidate at 513 is merely skipped; a NaN query gives NaN / index 0)."""
    from pointcloudcounterfactual_amd import backend

    a, c = pair(78, 2, 1500, 1300)
    c[0, 512, 0] = np.nan       # hides candidates 512..1023 of sample 0 from every query of set 1
    c[1, 1024, 2] = np.nan      # hides 1024..1299 of sample 1
    c[1, 513, 1] = np.nan       # not a chunk head: skipped only
    a[0, 1024] = np.nan         # the other direction: hides 1024..1499 of set 1 from the queries of set 2
    d1, i1, d2, i2 = backend.NNDistance(_dev(a, cuda), _dev(c, cuda))
    od1, oi1, od2, oi2 = oracle_mod.nndistance(a, c)
    assert not ((oi1[0] >= 512) & (oi1[0] < 1024)).any() and not (oi1[1] >= 1024).any()  # the quirk is really there
    assert not (oi2[0] >= 1024).any()
    for got, exp in ((d1, od1), (d2, od2)):
        g = got.cpu().numpy()
        assert np.array_equal(np.isnan(g), np.isnan(exp))
        assert np.array_equal(g[~np.isnan(exp)], exp[~np.isnan(exp)])
    assert np.array_equal(i1.cpu().numpy(), oi1) and np.array_equal(i2.cpu().numpy(), oi2)
