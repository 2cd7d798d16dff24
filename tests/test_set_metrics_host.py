"""Host tests of ``set_metrics``: the three set metrics against plain float64 loops, the lowest-index tie rule, and the
CPU path of ``pairwise_chamfer`` against a float64 brute force."""

import numpy as np
import pytest
import torch

from tests.util import pair


def _sm():
    from pointcloudcounterfactual_amd import set_metrics

    return set_metrics


def _np_mmd_cov(d):
    d = np.asarray(d, np.float64)
    s, r = d.shape
    mmd = sum(min(d[i, j] for i in range(s)) for j in range(r)) / r
    mmd_smp = sum(min(d[i, j] for j in range(r)) for i in range(s)) / s
    hit = set()
    for i in range(s):
        best = 0
        for j in range(1, r):
            if d[i, j] < d[i, best]:  # strict: the lowest index keeps a tie
                best = j
        hit.add(best)
    return mmd, mmd_smp, len(hit) / r


def _np_one_nn(d_ss, d_sr, d_rr):
    s, r = d_sr.shape
    full = np.block([[d_ss, d_sr], [d_sr.T, d_rr]]).astype(np.float64)
    tp = fp = fn = tn = 0
    for x in range(s + r):
        best = None
        for y in range(s + r):
            if y != x and (best is None or full[x, y] < full[x, best]):
                best = y
        if x < s:
            tp, fn = tp + (best < s), fn + (best >= s)
        else:
            fp, tn = fp + (best < s), tn + (best >= s)
    return (tp + tn) / (s + r), tp, fp, fn, tn


@pytest.mark.parametrize('s,r', [(1, 1), (5, 7), (9, 4), (12, 12)])
def test_mmd_cov_matches_a_float64_loop(s, r):
    rng = np.random.default_rng(s * 31 + r)
    d = rng.random((s, r))
    got = _sm().mmd_cov(torch.from_numpy(d))
    mmd, mmd_smp, cov = _np_mmd_cov(d)
    assert abs(got['mmd'].item() - mmd) <= 1e-15 and abs(got['mmd_smp'].item() - mmd_smp) <= 1e-15
    assert got['cov'].item() == cov
    got32 = _sm().mmd_cov(torch.from_numpy(d.astype(np.float32)))
    assert got32['cov'].item() == np.float32(cov) and got32['mmd'].dtype == torch.float32


@pytest.mark.parametrize('s,r', [(1, 1), (2, 1), (5, 7), (9, 4), (8, 8)])
def test_one_nn_accuracy_matches_a_float64_loop(s, r):
    rng = np.random.default_rng(s * 17 + r)
    pts = rng.random((s + r, 4))
    full = ((pts[:, None] - pts[None]) ** 2).sum(-1)
    d_ss, d_sr, d_rr = full[:s, :s], full[:s, s:], full[s:, s:]
    got = _sm().one_nn_accuracy(*(torch.from_numpy(np.ascontiguousarray(x)) for x in (d_ss, d_sr, d_rr)))
    acc, tp, fp, fn, tn = _np_one_nn(d_ss, d_sr, d_rr)
    assert (got['tp'].item(), got['fp'].item(), got['fn'].item(), got['tn'].item()) == (tp, fp, fn, tn)
    assert got['acc'].item() == acc
    assert tp + fn == s and fp + tn == r


def test_ties_go_to_the_lowest_index():
    sm = _sm()
    # duplicated columns 1 == 3 and 0 == 4, duplicated rows 0 == 2: every row's minimum is an exact tie
    d = torch.tensor([[3., 1., 2., 1., 3.], [0.5, 4., 4., 4., 0.5], [3., 1., 2., 1., 3.]])
    assert sm._argmin_lowest(d, 1).tolist() == [1, 0, 1]
    assert sm._argmin_lowest(d, 0).tolist() == [1, 0, 0, 0, 1]
    got = sm.mmd_cov(d)
    assert got['cov'].item() == pytest.approx(2 / 5)  # columns 1 and 0 only: never 3 or 4
    assert got['mmd'].item() == pytest.approx((0.5 + 1 + 2 + 1 + 0.5) / 5)
    assert got['mmd_smp'].item() == pytest.approx((1 + 0.5 + 1) / 3)
    assert _np_mmd_cov(d.numpy())[2] == 2 / 5
    # a constant matrix: every argmin is index 0, one reference covered
    assert sm.mmd_cov(torch.ones(6, 4))['cov'].item() == 0.25
    # 1-NN: item 0 is equally near to item 1 (generated) and items 2, 3 (reference): generated, the lowest index, wins
    d_ss = torch.tensor([[0., 1.], [1., 0.]])
    d_sr = torch.tensor([[1., 1.], [5., 5.]])
    d_rr = torch.tensor([[0., 1.], [1., 0.]])
    got = sm.one_nn_accuracy(d_ss, d_sr, d_rr)
    # item 1 -> item 0 (generated); items 2, 3: tie between item 0 (distance 1) and each other (1): item 0, generated
    assert (got['tp'].item(), got['fn'].item(), got['fp'].item(), got['tn'].item()) == (2, 0, 2, 0)
    assert got['acc'].item() == 0.5
    assert _np_one_nn(d_ss.numpy(), d_sr.numpy(), d_rr.numpy()) == (0.5, 2, 2, 0, 0)


def test_identical_and_separated_sets():
    sm = _sm()
    rng = np.random.default_rng(5)
    pts = rng.random((6, 3))
    d = torch.from_numpy(((pts[:, None] - pts[None]) ** 2).sum(-1))
    # S == R, the generated set IS the reference set: every item's nearest other item is its zero-distance twin in the
    # OTHER set (item S + i for generated item i, item i for reference item S + i), so every label is wrong
    got = sm.one_nn_accuracy(d, d, d)
    assert got['acc'].item() == 0.0 and got['tp'].item() == 0 and got['tn'].item() == 0
    scores = sm.mmd_cov(d)
    assert scores['mmd'].item() == 0.0 and scores['mmd_smp'].item() == 0.0 and scores['cov'].item() == 1.0
    # two well-separated clusters of duplicates: every item's nearest other item has its own label
    d_ss, d_rr = torch.zeros(4, 4), torch.zeros(5, 5)
    d_sr = torch.full((4, 5), 9.0)
    got = sm.one_nn_accuracy(d_ss, d_sr, d_rr)
    assert got['acc'].item() == 1.0 and got['tp'].item() == 4 and got['tn'].item() == 5
    assert sm.mmd_cov(d_sr.double())['cov'].item() == 0.2  # every generated cloud picks reference 0


def _brute(a, b, mean):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d_ab = np.empty((a.shape[0], b.shape[0]))
    d_ba = np.empty_like(d_ab)
    for i in range(a.shape[0]):
        for j in range(b.shape[0]):
            d2 = ((a[i][:, None, :] - b[j][None, :, :]) ** 2).sum(-1)
            d_ab[i, j] = d2.min(1).mean() if mean else d2.min(1).sum()
            d_ba[i, j] = d2.min(0).mean() if mean else d2.min(0).sum()
    return d_ab, d_ba


RTOL = 2.0 ** -23  # one rounding to float32 (2^-24), doubled


@pytest.mark.parametrize('s,r,n,m', [(3, 4, 50, 50), (2, 5, 37, 64), (4, 2, 1, 9), (3, 3, 130, 1), (1, 1, 1, 1)])
@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_pairwise_chamfer_cpu_against_float64(s, r, n, m, reduction):
    sm = _sm()
    a = torch.from_numpy(pair(n + s, s, n, kind='uniform')[0])
    b = torch.from_numpy(pair(m + r, r, m)[1])
    e_ab, e_ba = _brute(a.numpy(), b.numpy(), reduction == 'mean')
    d_ab, d_ba = sm.pairwise_chamfer(a, b, reduction, directional=True)
    cd = sm.pairwise_chamfer(a, b, reduction)
    assert d_ab.dtype == d_ba.dtype == cd.dtype == torch.float32 and cd.shape == (s, r)
    np.testing.assert_allclose(d_ab.numpy(), e_ab, rtol=RTOL, atol=0)
    np.testing.assert_allclose(d_ba.numpy(), e_ba, rtol=RTOL, atol=0)
    np.testing.assert_allclose(cd.numpy(), e_ab + e_ba, rtol=RTOL, atol=0)


def test_pairwise_chamfer_cpu_self_mode():
    sm = _sm()
    a = torch.from_numpy(pair(3, 5, 40)[0])
    e_ab, e_ba = _brute(a.numpy(), a.numpy(), True)
    d_ab, d_ba = sm.pairwise_chamfer(a, directional=True)
    np.testing.assert_allclose(d_ab.numpy(), e_ab, rtol=RTOL, atol=0)
    np.testing.assert_allclose(d_ba.numpy(), e_ba, rtol=RTOL, atol=0)
    cd = sm.pairwise_chamfer(a)
    assert torch.equal(cd, cd.t()) and (cd.diagonal() == 0).all()
    assert torch.equal(cd, sm.pairwise_chamfer(a, a.clone()))
    assert torch.equal(d_ab, d_ba.t())
    # constants of the graph
    assert not sm.pairwise_chamfer(a.clone().requires_grad_(True)).requires_grad


def test_argument_errors():
    sm = _sm()
    good = torch.zeros(2, 5, 3)
    for bad in (torch.zeros(5, 3), torch.zeros(2, 5, 3, 1), torch.zeros(2, 5, 2), torch.zeros(2, 3, 5), torch.zeros(2, 0, 3)):
        with pytest.raises(ValueError, match='must '):
            sm.pairwise_chamfer(bad)
        with pytest.raises(ValueError, match='must '):
            sm.pairwise_chamfer(good, bad)
        with pytest.raises(ValueError, match='must '):
            sm.pairwise_emd(bad)
    with pytest.raises(ValueError, match='reduction'):
        sm.pairwise_chamfer(good, reduction='max')
    with pytest.raises(RuntimeError, match='a must be a CUDA tensor'):
        sm.pairwise_emd(good)
    with pytest.raises(RuntimeError, match='a must be a CUDA tensor'):
        sm.pairwise_emd(good, good)
    with pytest.raises(ValueError, match='pairs_per_call'):
        sm.pairwise_emd(good, pairs_per_call=0)
    with pytest.raises(ValueError, match='pairs_per_call'):
        sm.pairwise_emd(good, pairs_per_call=sm.MAX_PAIRS_PER_CALL + 1)
    with pytest.raises(ValueError, match='non-empty'):
        sm.mmd_cov(torch.zeros(0, 3))
    with pytest.raises(ValueError, match='expected d_ss'):
        sm.one_nn_accuracy(torch.zeros(2, 2), torch.zeros(3, 2), torch.zeros(2, 2))


def test_package_exports_the_module():
    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import _lib

    assert pkg.set_metrics is _sm() and 'set_metrics' in pkg.__all__
    assert 'pcc_chamfer_matrix' in _lib.ABI
