"""GPU tests of the all-pairs Chamfer matrix (``pcc_chamfer_matrix`` through ``set_metrics.pairwise_chamfer``), of
``pairwise_emd`` and of ``compute_all_metrics``.

The directional entries are checked against the library's own pinned search: for every pair ``(i, j)`` the float32
minima of ``backend.NNDistance`` on the replicated pair, summed in float64.  The tolerance is derived: a float32 sum of
``n`` non-negative terms in any order has relative error at most ``(n - 1) 2^-24``; one more rounding for the division
and one for the add give ``rtol = (max(n, m) + 2) 2^-24``, computed from the shape."""

import numpy as np
import pytest
import torch

from tests.util import pair
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

POINTS = (1, 3, 64, 257, 513, 2048)


def _sm():
    from pointcloudcounterfactual_amd import set_metrics

    return set_metrics


def _banks(seed, s, n, r, m, kind, cuda):
    """Two unrelated banks of the given kind (tests/util.py): recon-like / surface-like clouds, or uniform ones."""
    a = pair(seed, s, n, kind=kind)[0]
    b = pair(seed + 1000, r, m, kind=kind)[1]
    return torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda)


def _pinned(a, b, mean):
    """float64 sums of NNDistance's float32 minima for every pair: (d_ab[S,R], d_ba[S,R]) as float64 numpy."""
    from pointcloudcounterfactual_amd import backend

    s, n, r, m = a.size(0), a.size(1), b.size(0), b.size(1)
    d1, _i1, d2, _i2 = backend.NNDistance(a.repeat_interleave(r, 0).contiguous(), b.repeat(s, 1, 1).contiguous())
    ab, ba = d1.double().sum(1).view(s, r), d2.double().sum(1).view(s, r)
    if mean:
        ab, ba = ab / n, ba / m
    return ab.cpu().numpy(), ba.cpu().numpy()


def _rtol(n, m):
    return (max(n, m) + 2) * 2.0 ** -24


def _check_directional(a, b, kind_tag, oracle_mod=None):
    sm = _sm()
    n, m = a.size(1), b.size(1)
    for mean in (True, False):
        e_ab, e_ba = _pinned(a, b, mean)
        if oracle_mod is not None and mean:  # the minima under the pinned sums are the oracle's, bit for bit (pair (0, 0))
            from pointcloudcounterfactual_amd import backend

            od1, _, od2, _ = oracle_mod.nndistance(a[:1].cpu().numpy(), b[:1].cpu().numpy())
            d1, _, d2, _ = backend.NNDistance(a[:1].contiguous(), b[:1].contiguous())
            assert np.array_equal(d1.cpu().numpy(), od1) and np.array_equal(d2.cpu().numpy(), od2)
        d_ab, d_ba = sm._chamfer_matrix(a, b, mean)
        err_ab = np.abs(d_ab.cpu().numpy() - e_ab) / e_ab.clip(min=np.finfo(np.float64).tiny)
        err_ba = np.abs(d_ba.cpu().numpy() - e_ba) / e_ba.clip(min=np.finfo(np.float64).tiny)
        print(f'{kind_tag} S={a.size(0)} R={b.size(0)} n={n} m={m} mean={mean}: max relative error d_ab {err_ab.max():.3e} '
              f'd_ba {err_ba.max():.3e}, bound {_rtol(n, m):.3e}')
        np.testing.assert_allclose(d_ab.cpu().numpy(), e_ab, rtol=_rtol(n, m), atol=0)
        np.testing.assert_allclose(d_ba.cpu().numpy(), e_ba, rtol=_rtol(n, m), atol=0)
        # either output NULL: the other one keeps its bits
        only_ab, none_ba = sm._chamfer_matrix(a, b, mean, want_ba=False)
        none_ab, only_ba = sm._chamfer_matrix(a, b, mean, want_ab=False)
        assert none_ab is None and none_ba is None
        assert torch.equal(only_ab, d_ab) and torch.equal(only_ba, d_ba)
        # the public surface: the sum of the two, and the two
        red = 'mean' if mean else 'sum'
        assert torch.equal(sm.pairwise_chamfer(a, b, red), d_ab + d_ba)
        pub = sm.pairwise_chamfer(a, b, red, directional=True)
        assert torch.equal(pub[0], d_ab) and torch.equal(pub[1], d_ba)


@pytest.mark.parametrize('s,r', [(1, 1), (5, 7), (33, 2)])
@pytest.mark.parametrize('n', POINTS)
@pytest.mark.parametrize('m', POINTS)
def test_directional_entries_against_the_pinned_search(cuda, oracle_mod, s, r, n, m):
    for kind in ('recon', 'uniform'):
        a, b = _banks(n * 7 + m + s, s, n, r, m, kind, cuda)
        _check_directional(a, b, kind, oracle_mod)


@pytest.mark.parametrize('s,r,n,m', [(3, 2, 2049, 100), (2, 3, 100, 4100), (2, 2, 2500, 2300), (1, 2, 4096, 4097)])
def test_clouds_larger_than_a_chunk(cuda, s, r, n, m):
    a, b = _banks(n + m, s, n, r, m, 'uniform', cuda)
    _check_directional(a, b, 'uniform')


def test_position_independence_and_repeatability(cuda):
    sm = _sm()
    for n, m in ((257, 513), (2048, 2048), (64, 2300), (2500, 2100)):
        x, y = _banks(n + m, 1, n, 1, m, 'recon', cuda)
        base = sm._chamfer_matrix(x, y, True)
        for s, r, i, j in ((1, 1, 0, 0), (5, 7, 3, 6), (33, 2, 32, 0), (40, 70, 17, 41)):
            a, b = _banks(s * r + n, s, n, r, m, 'uniform', cuda)
            a[i], b[j] = x[0], y[0]
            got = sm._chamfer_matrix(a, b, True)
            again = sm._chamfer_matrix(a, b, True)
            for k in (0, 1):
                assert torch.equal(got[k][i, j], base[k][0, 0]), (n, m, s, r, k)
                assert torch.equal(got[k], again[k]), (n, m, s, r, k)


@pytest.mark.parametrize('s,n', [(1, 64), (7, 257), (33, 513), (40, 2048), (5, 1), (3, 2100)])
def test_self_mode(cuda, s, n):
    sm = _sm()
    a = torch.from_numpy(pair(s + n, s, n)[0]).to(cuda)
    a[s - 1] = a[0]  # a duplicate cloud: bit-identical rows and columns (and an exact zero off the diagonal)
    for mean in (True, False):
        d_ab, d_ba = sm._chamfer_matrix(a, None, mean)
        g_ab, g_ba = sm._chamfer_matrix(a, a.clone(), mean)
        assert torch.equal(d_ab, g_ab) and torch.equal(d_ba, g_ba)
        assert torch.equal(d_ab, d_ba.t())
        assert (d_ab.diagonal() == 0).all() and (d_ba.diagonal() == 0).all()
        assert not torch.signbit(d_ab.diagonal()).any()
        assert torch.equal(d_ab[s - 1], d_ab[0]) and torch.equal(d_ab[:, s - 1], d_ab[:, 0])
        only_ab, _ = sm._chamfer_matrix(a, None, mean, want_ba=False)
        _, only_ba = sm._chamfer_matrix(a, None, mean, want_ab=False)
        assert torch.equal(only_ab, d_ab) and torch.equal(only_ba, d_ba)
    cd = sm.pairwise_chamfer(a)
    assert torch.equal(cd, cd.t()) and (cd.diagonal() == 0).all()
    assert torch.equal(cd, sm.pairwise_chamfer(a, a.clone()))
    if n <= 2048:
        e_ab, e_ba = _pinned(a, a, True)
        d_ab, d_ba = sm._chamfer_matrix(a, None, True)
        np.testing.assert_allclose(d_ab.cpu().numpy(), e_ab, rtol=_rtol(n, n), atol=0)
        np.testing.assert_allclose(d_ba.cpu().numpy(), e_ba, rtol=_rtol(n, n), atol=0)


@pytest.mark.parametrize('n,m', [(64, 257), (2048, 2048), (2100, 300), (2100, 2200)])
@pytest.mark.parametrize('value', [float('nan'), float('inf'), float('-inf')])
def test_non_finite_clouds_poison_their_row_or_column(cuda, n, m, value):
    sm = _sm()
    s, r = 6, 5
    a, b = _banks(n + m, s, n, r, m, 'recon', cuda)
    clean = sm._chamfer_matrix(a, b, True)
    a2, b2 = a.clone(), b.clone()
    a2[2, n - 1, 1] = value
    b2[4, m // 2, 2] = value
    got_a = sm._chamfer_matrix(a2, b, True)
    got_b = sm._chamfer_matrix(a, b2, True)
    rows = torch.arange(s, device=cuda) != 2
    cols = torch.arange(r, device=cuda) != 4
    for k in (0, 1):
        assert torch.isnan(got_a[k][2]).all() and torch.equal(got_a[k][rows], clean[k][rows])
        assert torch.isnan(got_b[k][:, 4]).all() and torch.equal(got_b[k][:, cols], clean[k][:, cols])
    if n == m:
        own = sm._chamfer_matrix(a2, None, True)
        ref = sm._chamfer_matrix(a, None, True)
        for k in (0, 1):
            assert torch.isnan(own[k][2]).all() and torch.isnan(own[k][:, 2]).all()
            assert torch.equal(own[k][rows][:, rows], ref[k][rows][:, rows])


def test_sizes_and_binding_checks(cuda):
    from pointcloudcounterfactual_amd import _lib

    sm = _sm()
    a, b = _banks(1, 3, 50, 4, 60, 'uniform', cuda)
    assert sm.pairwise_chamfer(a[:0], b).shape == (0, 4) and sm.pairwise_chamfer(a, b[:0]).shape == (3, 0)
    with pytest.raises(RuntimeError, match='b must be a CUDA tensor'):
        sm.pairwise_chamfer(a, b.cpu())
    with pytest.raises(RuntimeError, match='a must be a CUDA tensor'):
        sm.pairwise_chamfer(a.cpu(), b)
    with pytest.raises(RuntimeError, match='a must be torch.float32'):
        sm.pairwise_chamfer(a.double(), b)
    with pytest.raises(RuntimeError, match='b must be a CUDA tensor'):
        sm.pairwise_emd(a, b.cpu())
    out = torch.zeros(3, 4, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    fn = _lib.lib.pcc_chamfer_matrix
    assert fn(-1, 50, a.data_ptr(), 4, 60, b.data_ptr(), 1, out.data_ptr(), None, st) == -22
    assert fn(3, 0, a.data_ptr(), 4, 60, b.data_ptr(), 1, out.data_ptr(), None, st) == -22
    assert fn(3, 50, None, 4, 60, b.data_ptr(), 1, out.data_ptr(), None, st) == -22
    assert b'null pointer' in _lib.lib.pcc_last_error()
    assert fn(0, 50, None, 4, 60, None, 1, None, None, st) == 0
    assert fn(3, 50, a.data_ptr(), 4, 60, b.data_ptr(), 1, None, None, st) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()
    # non-contiguous inputs give the result of their contiguous copies; inputs are detached
    at = a.transpose(1, 2).contiguous().transpose(1, 2)
    assert not at.is_contiguous()
    ref = sm.pairwise_chamfer(a, b)
    assert torch.equal(sm.pairwise_chamfer(at, b), ref)
    got = sm.pairwise_chamfer(a.clone().requires_grad_(True), b)
    assert not got.requires_grad and torch.equal(got, ref)
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = sm.pairwise_chamfer(a, b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert torch.equal(got, ref)


@pytest.mark.parametrize('s,r,n,m,ppc', [(5, 7, 300, 257, 4), (3, 3, 64, 64, 512), (6, 5, 1024, 1024, 7), (2, 9, 2048, 2048, 5)])
def test_pairwise_emd_entries_are_match_cost_alone(cuda, s, r, n, m, ppc):
    """The library's cost does not depend on the batch around a sample: every schedule of the pass chain works sample
    by sample with the same walk and reduction order (test_gpu_structural.py pins the schedules against
    each other).  So the cost of a pair alone, in a batch of ``ppc`` and in one batch of all S R pairs must carry the
    same bits, and every entry is compared bit for bit; S R is not a multiple of ``ppc``."""
    from pointcloudcounterfactual_amd import match_cost

    sm = _sm()
    assert (s * r) % ppc != 0
    a, b = (torch.from_numpy(x).to(cuda) for x in pair(s * 11 + r, max(s, r), n, m))
    a, b = a[:s].contiguous(), b[:r].contiguous()
    b[0] = b[r - 1]  # duplicate reference clouds: bit-identical columns
    raw = sm.pairwise_emd(a, b, normalize=False, pairs_per_call=ppc)
    one_call = sm.pairwise_emd(a, b, normalize=False, pairs_per_call=sm.MAX_PAIRS_PER_CALL)
    alone = torch.stack([torch.cat([match_cost(a[i:i + 1], b[j:j + 1]) for j in range(r)]) for i in range(s)])
    print(f'S={s} R={r} n={n} m={m}: max |batched - alone| / alone = {((raw - alone).abs() / alone).max().item():.3e}')
    assert torch.equal(raw, alone) and torch.equal(one_call, alone)
    assert torch.equal(raw[:, 0], raw[:, r - 1])
    assert torch.equal(sm.pairwise_emd(a, b, pairs_per_call=ppc), alone / n)
    if n == m:
        assert torch.equal(sm.pairwise_emd(a, pairs_per_call=ppc), sm.pairwise_emd(a, a.clone(), pairs_per_call=ppc))
    assert not raw.requires_grad


def test_evaluation_sized_run(cuda):
    """S = R = 64 clouds of 2048 points: compute_all_metrics against the same metrics on matrices assembled pair by pair
    through ``chamfer()`` / ``match_cost()`` (a row of pairs per call).  The Chamfer entries differ from ``chamfer()``'s
    by the order of a float32 sum only, so MMD agrees within the derived bound; COV and 1-NNA are counts."""
    from pointcloudcounterfactual_amd import chamfer, match_cost

    sm = _sm()
    count, n = 64, 2048
    sample, ref = (torch.from_numpy(x).to(cuda) for x in pair(2024, count, n, kind='recon'))
    ref = ref[torch.randperm(count, generator=torch.Generator().manual_seed(1)).to(cuda)].contiguous()

    def by_pairs(fn, x, y):
        return torch.stack([fn(x[i:i + 1].expand(y.size(0), -1, -1).contiguous(), y) for i in range(x.size(0))])

    got = sm.compute_all_metrics(sample, ref)
    assert sorted(got) == ['1-NNA-CD', '1-NNA-EMD', 'COV-CD', 'COV-EMD', 'MMD-CD', 'MMD-EMD']
    for tag, fn in (('CD', chamfer), ('EMD', lambda x, y: match_cost(x, y) / n)):
        d_sr, d_ss, d_rr = by_pairs(fn, sample, ref), by_pairs(fn, sample, sample), by_pairs(fn, ref, ref)
        exp = sm.mmd_cov(d_sr)
        exp_acc = sm.one_nn_accuracy(d_ss, d_sr, d_rr)['acc']
        print(tag, {k: v.item() for k, v in got.items() if k.endswith(tag)}, 'by pairs', exp['mmd'].item(),
              exp['cov'].item(), exp_acc.item())
        # both entries are within _rtol of the exact sum of the same minima; then a float32 mean over `count` columns each
        rtol = 2 * _rtol(n, n) + 2 * count * 2.0 ** -24
        np.testing.assert_allclose(got[f'MMD-{tag}'].item(), exp['mmd'].item(), rtol=rtol, atol=0)
        # COV and 1-NNA are counts of argmins.  The EMD matrices are bit-equal, so those counts are equal; the Chamfer
        # matrices differ by the order of a float32 sum, which can move an argmin only where the two smallest entries
        # of a row are closer than the bound on that difference -- checked here, so the equality below is derived
        if tag == 'CD':
            full = torch.cat([torch.cat([d_ss, d_sr], 1), torch.cat([d_sr.t(), d_rr], 1)], 0).double()
            full.fill_diagonal_(float('inf'))
            for mat in (d_sr.double(), full):
                two = mat.topk(2, dim=1, largest=False).values
                assert ((two[:, 1] - two[:, 0]) > 4 * _rtol(n, n) * two[:, 1]).all()
        assert got[f'COV-{tag}'].item() == exp['cov'].item()
        assert got[f'1-NNA-{tag}'].item() == exp_acc.item()
    # the matrices themselves
    cd = sm.pairwise_chamfer(sample, ref)
    np.testing.assert_allclose(cd.cpu().numpy(), by_pairs(chamfer, sample, ref).cpu().numpy(), rtol=2 * _rtol(n, n), atol=0)
