"""GPU tests of the k-NN between two clouds (``pcc_knn_cross`` through ``neighbour_ops.hip_knn_cross``).

The exact expectation comes from the one-cloud oracle without changing it: for ``q[b,c,nq]`` and ``x[b,c,n]`` the oracle
searches ``z = cat([x, q], 2)`` with ``K = n + nq``; row ``n + i`` is query ``i`` against all of ``z`` in the library's own
rounding, ordered by (distance, index), and dropping the entries ``>= n`` leaves the candidates of ``x`` in that order."""

import numpy as np
import pytest
import torch

# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

EPS32 = float(np.finfo(np.float32).eps)
KS = (1, 4, 20, 64, 128)


def _cloud(seed, b, c, n, kind='normal'):
    g = torch.Generator().manual_seed(seed)
    if kind == 'uniform':
        return torch.rand(b, c, n, generator=g).contiguous()
    x = torch.randn(b, c, n, generator=g)
    if kind == 'sphere':
        x = x / x.norm(dim=1, keepdim=True)
    return x.contiguous()


def _cross(q, x, k, cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    idx, dist = ops.hip_knn_cross(q.to(cuda), x.to(cuda), k, return_distance=True)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _expected(oracle_mod, q, x):
    """The full sorted candidate lists ``idx[b,nq,n]`` of the oracle and, for c >= 4, their distances (else None)."""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    b, c, nq = q.shape
    n = x.shape[2]
    z = np.ascontiguousarray(np.concatenate([x, q], axis=2))
    if c <= 3:
        full, dm = oracle_mod.knn_diff(z, n + nq), None
    else:
        full, dm = oracle_mod.knn_expanded(z, n + nq, return_dist=True)
    rows = full[:, n:, :]
    idx = rows[rows < n].reshape(b, nq, n)  # (every row holds each candidate of x exactly once)
    dist = None if dm is None else np.take_along_axis(dm[:, n:, :n], idx, axis=2)
    return idx, dist


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)  # (-0 and +0 are one distance)


def _check_diff_dist(q, x, idx, dist):
    """c <= 3 (numpy has no fma): dist within c + 2 float32 ulp of the float64 value and of the float32 distance
    recomputed for the returned index, and non-decreasing along k."""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    c = q.shape[1]
    xs = np.stack([np.take_along_axis(x[:, ch, None, :], idx, axis=2) for ch in range(c)], 1)  # [b,c,nq,k]
    d64 = ((xs.astype(np.float64) - q[:, :, :, None].astype(np.float64)) ** 2).sum(1)
    df = xs - q[:, :, :, None]
    d32 = np.zeros_like(df[:, 0])
    for ch in range(c):
        d32 = d32 + df[:, ch] * df[:, ch]
    ulp = np.spacing(np.maximum(d64, np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
    assert (np.abs(dist.astype(np.float64) - d64) <= (c + 2) * ulp).all()
    assert (np.abs(dist.astype(np.float64) - d32.astype(np.float64)) <= (c + 2) * ulp).all()
    assert (np.diff(dist, axis=2) >= 0).all()


def _check_against_oracle(oracle_mod, cuda, q, x, ks):
    exp_idx, exp_dist = _expected(oracle_mod, q.numpy(), x.numpy())
    n = x.shape[2]
    for k in ks:
        if k > n:
            continue
        idx, dist = _cross(q, x, k, cuda)
        assert np.array_equal(idx, exp_idx[:, :, :k]), k
        if exp_dist is not None:
            assert np.array_equal(_bits(dist), _bits(exp_dist[:, :, :k])), k
        else:
            _check_diff_dist(q.numpy(), x.numpy(), idx, dist)
        assert not (np.signbit(dist) & (dist == 0)).any()


SHAPES = [(3, 1, 200), (2, 7, 333), (2, 257, 129), (1, 1000, 2050), (1, 2050, 1000), (2, 33, 128), (3, 50, 20)]


@pytest.mark.parametrize('b,nq,n', SHAPES)
@pytest.mark.parametrize('c', [1, 2, 3, 4, 17, 64, 129, 300])
def test_knn_cross_matches_the_oracle(cuda, oracle_mod, c, b, nq, n):
    """nq < n, nq > n, nq = 1, k = n (n = 128 and n = 20), sizes off every tile edge; indices bit for bit, distances
    bit for bit where the oracle has them (c >= 4)."""
    kinds = ('normal', 'uniform', 'sphere') if c >= 2 else ('normal', 'uniform')
    kind = kinds[(c + nq + n) % len(kinds)]
    q = _cloud(c * 101 + nq, b, c, nq, kind)
    x = _cloud(c * 103 + n + 1, b, c, n, kind)
    _check_against_oracle(oracle_mod, cuda, q, x, KS + (n,) if n <= 128 else KS)


@pytest.mark.parametrize('b,c,n,k', [(2, 3, 1000, 4), (2, 3, 777, 20), (1, 3, 3000, 25), (32, 3, 2048, 32), (2, 64, 500, 25),
                                       (32, 64, 2048, 20), (2, 128, 300, 32), (1, 128, 2048, 4), (3, 1, 100, 8),
                                       (2, 3, 900, 64), (2, 200, 600, 40)])
def test_knn_cross_of_a_cloud_with_itself_is_knn(cuda, b, c, n, k):
    """Whichever kernel pcc_knn picks (sorted, MFMA, role-split, wide): the same indices, also with q and x one tensor."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x = _cloud(b * 13 + c + n + k, b, c, n).to(cuda)
    ref = ops.hip_knn(x, k)
    assert torch.equal(ops.hip_knn_cross(x, x, k), ref)
    assert torch.equal(ops.hip_knn_cross(x.clone(), x, k), ref)
    idx, dist = ops.knn_cross(x, x, k, return_distance=True)
    assert torch.equal(idx, ref) and dist.shape == ref.shape


def test_knn_cross_adversarial_orders_and_ties(cuda, oracle_mod):
    n = 700
    t = torch.linspace(0, 1, n)
    line5 = torch.stack([t, 2 * t, -t, 0.5 * t, t * t], 0)[None]
    for c, k in ((5, 64), (3, 48)):
        line = line5[:, :c].contiguous()
        q = (-0.01 * _cloud(c, 1, c, 37, 'uniform')).contiguous()  # before the start of the line: distance grows with the index
        for x in (line, line.flip(2).contiguous()):
            _check_against_oracle(oracle_mod, cuda, q, x, (k,))
        base = _cloud(11 + c, 1, c, 70)
        ties = torch.cat([base] * 10, dim=2).contiguous()  # exact ties: ascending index
        _check_against_oracle(oracle_mod, cuda, _cloud(12 + c, 1, c, 45), ties, (k,))
        # queries that coincide with candidates
        same = ties[:, :, 5:300:7].contiguous()
        _check_against_oracle(oracle_mod, cuda, same, ties, (k,))
        idx, dist = _cross(same, ties, 10, cuda)
        if c <= 3:
            assert (dist == 0).all() and not np.signbit(dist).any()
            assert np.array_equal(idx[0, :, 0], (np.arange(5, 300, 7) % 70))
    # a zero cloud: every product is a zero of either sign
    zq, zx = torch.zeros(1, 3, 9), -torch.zeros(1, 3, 150)
    idx, dist = _cross(zq, zx, 20, cuda)
    assert (idx == np.arange(20)).all() and (dist == 0).all() and not np.signbit(dist).any()


def test_knn_cross_non_finite_values(cuda, oracle_mod):
    for c in (3, 200):
        n, nq, k = 200, 90, 40
        x, q = _cloud(5 + c, 2, c, n), _cloud(6 + c, 2, c, nq)
        x[0, 1, 17] = float('nan')
        x[1, 0, 3] = float('inf')
        idx, dist = _cross(q, x, k, cuda)
        assert idx.min() >= 0 and idx.max() < n
        assert not (idx[0] == 17).any() and not np.isnan(dist[0]).any()
        clean = torch.cat([x[0, :, :17], x[0, :, 18:]], dim=1)[None].contiguous()
        ref, _ = _expected(oracle_mod, q[:1].numpy(), clean.numpy())
        ref = ref[:, :, :k]
        assert np.array_equal(idx[0], (ref + (ref >= 17))[0]), c
        # a NaN query: nothing enters its list
        q2 = _cloud(7 + c, 1, c, nq)
        q2[0, c - 1, 5] = float('nan')
        x2 = _cloud(8 + c, 1, c, n)
        idx, dist = _cross(q2, x2, k, cuda)
        assert (idx[0, 5] == n - 1).all() and np.isnan(dist[0, 5]).all()
        ok = np.arange(nq) != 5
        ref, _ = _expected(oracle_mod, q2[:, :, ok].numpy(), x2.numpy())
        assert np.array_equal(idx[0, ok], ref[0, :, :k]) and not np.isnan(dist[0, ok]).any()


@pytest.mark.parametrize('b,nq,n', [(1, 5, 20000), (2, 64, 3000)])
@pytest.mark.parametrize('c', [3, 64])
def test_knn_cross_split_is_invisible(cuda, b, nq, n, c):
    """... and the launch record shows that the switch acts: the selection kernel of (k, c) alone where the slices the rule
    of tests/knn_reference.py predicts are 1, its "sliced" launch and the merge launch where they are more.  (The record
    tells one slice from several, not how many: the count is an argument of the kernel, not an instantiation.)"""
    from pointcloudcounterfactual_amd import _lib
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests import knn_reference as kr
    from tests.which_ran import assert_only, ran

    def selection(k, forced):
        cus = torch.cuda.get_device_properties(cuda).multi_processor_count
        sliced = kr.cross_slices(b * nq, n, cus, forced) > 1  # (both shapes: one launch over all b * nq rows)
        return {kr.wide_select(c, k, sliced)} | ({kr.wide_merge(k)} if sliced else set())

    q, x = _cloud(nq + c, b, c, nq).to(cuda), _cloud(n + c, b, c, n).to(cuda)
    for k in (16, 128):
        auto, names = ran(lambda: ops.hip_knn_cross(q, x, k, return_distance=True))
        assert_only(names, selection(k, 0), 'knn_wide_select_kernel')
        for s in (1, 2, 7, 16):
            with _lib.tuning('knn_cross_split', s):
                (idx, dist), names = ran(lambda: ops.hip_knn_cross(q, x, k, return_distance=True))
            assert_only(names, selection(k, s), 'knn_wide_select_kernel')
            assert torch.equal(idx, auto[0]), (k, s)
            assert torch.equal(dist, auto[1]), (k, s)
        assert idx.min() >= 0 and idx.max() < n


@pytest.mark.parametrize('nq,n,c,k', [(64, 200000, 3, 20), (640, 120000, 8, 64), (128, 50000, 64, 128),
                                       (5, 20000, 3, 128)])  # (the last: the 128-slot selection on difference-form distances, sliced)
def test_knn_cross_large_shapes_against_float64(cuda, nq, n, c, k):
    """Too large for the oracle: float64 distances on the device.  An entry may differ from the float64 list only as a
    certified near tie, |d64[got] - d64[expected]| <= 4 (c + 2) eps32 (|q|^2 + |x|^2), and at most 0.1 % of the entries."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    q, x = _cloud(nq + c, 1, c, nq).to(cuda), _cloud(n + c, 1, c, n).to(cuda)
    idx, dist = ops.hip_knn_cross(q, x, k, return_distance=True)
    q64, x64 = q.double(), x.double()
    qn, xn = (q64**2).sum(1), (x64**2).sum(1)  # [1,nq], [1,n]
    d64 = torch.zeros(1, nq, n, dtype=torch.float64, device=cuda)
    for ch in range(c):  # the difference form, one channel at a time
        d64 += (q64[:, ch, :, None] - x64[:, ch, None, :]) ** 2
    exp = d64.topk(k, largest=False)[1]
    dg, de = d64.gather(2, idx), d64.gather(2, exp)
    xg, xe = xn.gather(1, idx.flatten(1)).view_as(idx), xn.gather(1, exp.flatten(1)).view_as(exp)
    bound = 4 * (c + 2) * EPS32 * (qn[:, :, None] + torch.minimum(xg, xe))
    differ = idx != exp
    excused = int(differ.sum())
    print(f'nq={nq} n={n} c={c} k={k}: {excused} of {idx.numel()} entries differ from the float64 list')
    assert ((dg - de).abs() <= bound)[differ].all()
    assert excused <= 0.001 * idx.numel()
    assert ((dist.double() - dg).abs() <= 4 * (c + 2) * EPS32 * (qn[:, :, None] + xg)).all()
    assert (dist[:, :, 1:] >= dist[:, :, :-1]).all()


@pytest.mark.parametrize('d', [3, 16])
def test_knn_cross_through_the_shim(cuda, d):
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from pykeops.torch import LazyTensor  # (the shim package of this repository)

    a = _cloud(d, 2, d, 300).to(cuda)  # [B,D,N]
    b = _cloud(d + 1, 2, d, 170).to(cuda)  # [B,D,M]
    pa, pb = a.transpose(1, 2).contiguous(), b.transpose(1, 2).contiguous()
    dm = ((LazyTensor(pa[:, :, None, :]) - LazyTensor(pb[:, None, :, :])) ** 2).sum(-1)
    for k in (1, 8, 40):
        i2, d2 = ops.hip_knn_cross(a, b, k, return_distance=True)  # neighbours of the rows among the columns
        i1, d1 = ops.hip_knn_cross(b, a, k, return_distance=True)
        assert torch.equal(dm.argKmin(k, dim=2), i2) and torch.equal(dm.argKmin(k, axis=1), i1)
        assert torch.equal(dm.Kmin(k, dim=2), d2) and torch.equal(dm.Kmin(k, axis=1), d1)
        assert dm.argKmin(k, dim=2).shape == (2, 300, k) and dm.argKmin(k, dim=1).shape == (2, 170, k)
    self_d = ((LazyTensor(pa[:, :, None, :]) - LazyTensor(pa[:, None, :, :])) ** 2).sum(-1)
    assert torch.equal(self_d.argKmin(40, dim=2), ops.hip_knn(a, 40))
    assert torch.equal(self_d.argKmin(40, dim=1), ops.hip_knn(a, 40))


def test_knn_cross_binding_checks(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    q, x = _cloud(1, 2, 3, 50).to(cuda), _cloud(2, 2, 3, 130).to(cuda)
    for fn in (ops.hip_knn_cross, ops.knn_cross):
        with pytest.raises(RuntimeError, match='q must be a CUDA tensor'):
            fn(q.cpu(), x, 4)
        with pytest.raises(RuntimeError, match='x must be a CUDA tensor'):
            fn(q, x.cpu(), 4)
    with pytest.raises(RuntimeError, match='q must be torch.float32'):
        ops.hip_knn_cross(q.double(), x, 4)
    with pytest.raises(RuntimeError, match='x must be torch.float32'):
        ops.hip_knn_cross(q, x.double(), 4)
    if torch.cuda.device_count() >= 2:
        with pytest.raises(RuntimeError, match='x is on cuda:1'):
            ops.hip_knn_cross(q, x.to('cuda:1'), 4)
    with pytest.raises(RuntimeError, match='knn_cross: bad size'):
        ops.hip_knn_cross(q, x, 0)
    with pytest.raises(RuntimeError, match='k exceeds the number of candidates'):
        ops.hip_knn_cross(x, q, 51)
    with pytest.raises(RuntimeError, match='k > 128 is not supported'):
        ops.hip_knn_cross(q, x, 129)
    idx, dist = ops.hip_knn_cross(q[:, :, :0], x, 4, return_distance=True)
    assert idx.shape == (2, 0, 4) and idx.dtype == torch.int64 and dist.shape == (2, 0, 4)
    # non-contiguous inputs give the result of their contiguous copies
    qt, xt = q.transpose(1, 2).contiguous().transpose(1, 2), x.transpose(1, 2).contiguous().transpose(1, 2)
    assert not qt.is_contiguous() and not xt.is_contiguous()
    ref = ops.hip_knn_cross(q, x, 9, return_distance=True)
    got = ops.hip_knn_cross(qt, xt, 9, return_distance=True)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    # inputs are detached; outputs are constants of the graph
    got = ops.hip_knn_cross(q.clone().requires_grad_(True), x, 9, return_distance=True)
    assert not got[0].requires_grad and not got[1].requires_grad and torch.equal(got[0], ref[0])


def test_knn_cross_side_stream(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for c, k, nq, n in ((3, 64, 1500, 900), (200, 40, 700, 1500), (3, 16, 8, 30000)):
        q, x = _cloud(21 + c, 4, c, nq).to(cuda), _cloud(22 + c, 4, c, n).to(cuda)
        ref = ops.hip_knn_cross(q, x, k, return_distance=True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            got = ops.hip_knn_cross(q, x, k, return_distance=True)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]), c
