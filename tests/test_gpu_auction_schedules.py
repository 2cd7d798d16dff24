"""The auction EMD (csrc/auction.hip) at every launch schedule, size class, cloud kind and edge of its C ABI, bit for bit
against the deterministic oracle (oracle.auction_forward_ext: oracle/auction_oracle.c without the reference's n % 1024
and b <= 512 limits, plus the iterations each sample used).

Schedules (pcc_auction_forward; `forced` is the measurement switch `auction_cluster`, include/pcc_test_hooks.h):
  * C = 1 when forced == 1 or n < 512; otherwise C = forced (2..16) or 8, halved while n / C < 128 or C > CUs.
  * C > 1 and 16 n + 12 njmax + 16 <= 160 KiB - 256 (njmax = ceil(n / C) + 1): `auction_cluster_kernel`, C workgroups per
    sample, CUs // C samples per launch.  The product's C: 4 for 512 <= n < 1024, 8 from 1024 on (fits up to n = 8192).
  * otherwise `auction_kernel`, one workgroup per sample, all samples in one launch: the bidder-side state and the highest
    increments in LDS while 40 n + 16 <= 160 KiB (n <= 4095), in global scratch from n = 4096 on (16 n + 16 bytes of LDS).
`_expected` restates that arithmetic and every run asserts, through the library's profiler, that the kernel it names ran
the number of launches it gives: a later change of a threshold cannot silently leave a branch untested.  Which of the two
state layouts `auction_kernel` uses follows from n alone (comments at the cases).

Every comparison with the oracle is exact (`dist` as uint32, `assignment`); the one tolerance is the theorem of
`test_converged_assignment_is_within_n_eps_of_the_optimum`, which does not use the oracle's result.
"""

import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.util import pair
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of float32
PCC_EINVAL = -22
LDS = 160 * 1024


def _lib():
    from pointcloudcounterfactual_amd import _lib

    return _lib


# ---- inputs ---------------------------------------------------------------------------------------------------------
KINDS = ('uniform', 'recon', 'dup_targets', 'dup_bidders', 'identical', 'lattice', 'one_target', 'clusters')


def _clouds(kind, seed, b, n):
    """(bidders xyz1, targets xyz2), float32 [b, n, 3]."""
    rng = np.random.default_rng(seed)
    if kind == 'uniform':
        return pair(seed, b, n, n, 'uniform')
    if kind == 'recon':  # coordinates in [-1, 1], as users pass them
        return pair(seed, b, n, n, 'recon')
    a, c = rng.random((b, n, 3), dtype=np.float32), rng.random((b, n, 3), dtype=np.float32)
    rep = np.arange(n) % ((n + 3) // 4)  # each distinct point four times (32 x 4 at n = 128)
    if kind == 'dup_targets':
        return a, np.ascontiguousarray(c[:, rep])
    if kind == 'dup_bidders':
        return np.ascontiguousarray(a[:, rep]), c
    if kind == 'identical':  # every bidder's best target is itself
        return a, a.copy()
    if kind == 'lattice':  # 5 levels per axis: many exactly equal distances, many exactly equal points
        return ((rng.integers(0, 5, (b, n, 3)) / 4).astype(np.float32), (rng.integers(0, 5, (b, n, 3)) / 4).astype(np.float32))
    if kind == 'one_target':
        return a, np.ascontiguousarray(np.broadcast_to(c[:, :1], (b, n, 3)))
    if kind == 'clusters':  # 8 clusters of radius ~1e-3: near-ties inside a cluster
        cen = rng.random((b, 8, 3), dtype=np.float32)
        pick = rng.integers(0, 8, (2, b, n))
        jit = rng.normal(0.0, 1e-3, (2, b, n, 3)).astype(np.float32)
        rows = np.arange(b)[:, None]
        return cen[rows, pick[0]] + jit[0], cen[rows, pick[1]] + jit[1]
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _oracle(kind, seed, b, n, eps, iters):
    """The extended oracle on `_clouds(kind, seed, b, n)`, computed once per case and shared (read-only arrays)."""
    import oracle

    oracle.set_threads(min(8, oracle.max_threads()))
    a, c = _clouds(kind, seed, b, n)
    out = (a, c) + tuple(oracle.auction_forward_ext(a, c, eps, iters))
    for x in out:
        x.setflags(write=False)
    return out  # a, c, dist, assignment, price, iters_used


# ---- running the library ------------------------------------------------------------------------------------------------
def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _expected(b, n, forced):
    """(kernel, launches) of pcc_auction_forward(b, n) under `auction_cluster = forced` (0: the product's choice)."""
    cus, C = _cus(), 1
    if forced != 1 and n >= 512:
        C = forced if forced > 1 else 8
        while C > 1 and n // C < 128:
            C //= 2
        while C > 1 and C > cus:
            C //= 2
    njmax = (n + C - 1) // C + 1
    if C > 1 and 16 * n + 12 * njmax + 16 <= LDS - 256:
        group = max(1, cus // C)
        return 'auction_cluster_kernel', (b + group - 1) // group
    return 'auction_kernel', 1


def _launches(prefix):
    count = ctypes.c_int(0)
    _lib().lib.pcc_profile_read(prefix.encode(), None, ctypes.byref(count))
    return count.value


@contextlib.contextmanager
def _profiled():
    lib = _lib().lib
    lib.pcc_profile_enable(1)  # (also clears what an earlier call recorded)
    try:
        yield
    finally:
        lib.pcc_profile_enable(0)


def _raw_forward(cuda, b, n, t1, t2, eps, iters, dist, ass):
    """pcc_auction_forward's return code (nothing raised)."""
    L = _lib()
    with torch.cuda.device(cuda):
        return L.lib.pcc_auction_forward(b, n, L.ptr(t1, 'xyz1', torch.float32, cuda), L.ptr(t2, 'xyz2', torch.float32, cuda),
                                         float(eps), int(iters), L.ptr(dist, 'dist', torch.float32, cuda),
                                         L.ptr(ass, 'assignment', torch.int32, cuda), torch.cuda.current_stream(cuda).cuda_stream)


def _run(cuda, a, c, eps, iters, forced=0):
    """dist, assignment (numpy) of the library under `auction_cluster = forced`, through emdModule where it takes the
    size and through the C ABI otherwise; asserts the schedule `_expected` names."""
    from emd import emdModule

    b, n, _ = a.shape
    t1, t2 = torch.tensor(a, device=cuda), torch.tensor(c, device=cuda)
    with _lib().tuning('auction_cluster', forced), _profiled():
        if n % 1024 == 0:
            dist, ass = emdModule()(t1, t2, eps, iters)
        else:
            dist, ass = torch.empty(b, n, device=cuda), torch.empty(b, n, device=cuda, dtype=torch.int32)  # (poisoned: conftest)
            assert _raw_forward(cuda, b, n, t1, t2, eps, iters, dist, ass) == 0, _lib().lib.pcc_last_error()
        torch.cuda.synchronize()
        ran = {k: _launches(k) for k in ('auction_cluster_kernel', 'auction_kernel')}
    kernel, launches = _expected(b, n, forced)
    assert ran == {'auction_cluster_kernel': 0, 'auction_kernel': 0, kernel: launches}, (ran, kernel, launches)
    return dist.cpu().numpy(), ass.cpu().numpy()


def _backward(cuda, a, c, g, ass):
    L = _lib()
    b, n, _ = a.shape
    t1, t2 = torch.tensor(a, device=cuda), torch.tensor(c, device=cuda)
    tg, ta = torch.tensor(g, device=cuda), torch.tensor(np.asarray(ass, dtype=np.int32), device=cuda)
    out = torch.empty(b, n, 3, device=cuda)
    L.call(L.lib.pcc_auction_backward, 'auction backward', cuda, b, n, L.ptr(t1, 'xyz1', torch.float32, cuda),
           L.ptr(t2, 'xyz2', torch.float32, cuda), L.ptr(tg, 'g', torch.float32, cuda), L.ptr(ta, 'idx', torch.int32, cuda),
           L.ptr(out, 'grad', torch.float32, cuda))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same(got, want, what):
    d, a = got
    od, oa = want
    assert np.array_equal(a, oa), f'{what}: {int((a != oa).sum())} assignments differ'
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32)), f'{what}: {int((d.view(np.uint32) != od.view(np.uint32)).sum())} dist words differ'


def _schedules(n):
    """The product's choice, one workgroup per sample, and every forced C in {2, 4, 16} that keeps 128 bidders per slice."""
    return [0, 1] + [C for C in (2, 4, 16) if n // C >= 128]


# ---- 1. schedule x size -----------------------------------------------------------------------------------------------
#          (n, b, iters)   eps = 0.005 throughout
SIZES = [
    # n < 512: auction_kernel, state in LDS; nu <= n bidders share 1024 threads, so the lanes-per-bidder ladder starts at
    # 64 (n = 1, 2, 3), 16 (n = 63, 64), 8 (n = 65), 4 (n = 127), 2 (n = 511: one round of 512) and climbs as bidders are
    # assigned
    (1, 3, 10), (2, 3, 10), (3, 2, 20), (63, 3, 30), (64, 2, 30), (65, 3, 30), (127, 2, 30), (511, 3, 30),
    # 512 <= n < 1024: product C = 4 (n / 8 < 128); slices of 128 | 128/129 | 250 | 255/256 bidders; forced 2 runs too
    (512, 2, 30), (513, 3, 30), (1000, 2, 20), (1023, 3, 20),
    # product C = 8 with even (1024) and uneven slices; forced 16 from 2048 on (2049: slices of 128 / 129)
    (1024, 3, 20), (1025, 2, 20), (2047, 2, 12), (2049, 3, 12), (3000, 2, 10),
    # auction_cluster = 1: 4095 is the last size with the state in LDS (40 n + 16 = 163816 <= 163840), 4096 (163856) the
    # first with it in global scratch, 8192 the LDS limit of that layout (16 n + 16 = 131088); b = 2 gives the second
    # sample its own block of scratch.  Forced 2 does not fit from 7435 on and falls back to auction_kernel.
    (4095, 2, 8), (4096, 2, 8), (5000, 1, 6), (8191, 1, 5), (8192, 2, 5),
]


@pytest.mark.parametrize('n,b,iters', SIZES, ids=[f'n{n}' for n, _, _ in SIZES])
def test_every_schedule_matches_the_oracle(cuda, n, b, iters):
    a, c, od, oa, _, _ = _oracle('uniform', 1000 + n, b, n, 0.005, iters)
    for forced in _schedules(n):
        _same(_run(cuda, a, c, 0.005, iters, forced), (od, oa), f'n={n} auction_cluster={forced}')


def test_n_above_8192_is_refused(cuda):
    n = 8193
    t = torch.zeros(1, n, 3, device=cuda)
    dist, ass = torch.full((1, n), 7.0, device=cuda), torch.full((1, n), 7, device=cuda, dtype=torch.int32)
    assert _raw_forward(cuda, 1, n, t, t, 0.005, 5, dist, ass) == PCC_EINVAL
    assert b'8192' in _lib().lib.pcc_last_error()
    torch.cuda.synchronize()
    assert bool((dist == 7.0).all()) and bool((ass == 7).all())


def test_forced_pair_either_side_of_its_lds_fit(cuda):
    """C = 2 needs 16 n + 12 (ceil(n / 2) + 1) + 16 <= 160 KiB - 256 = 163584 B: n = 7434 (163576) is the last size that
    runs as a cluster of two; n = 7435 (163604) falls back to auction_kernel with the state in global scratch.  Same bits."""
    fits = [n for n in range(7000, 8193) if 16 * n + 12 * ((n + 1) // 2 + 1) + 16 <= LDS - 256]
    assert fits[-1] == 7434
    for n, kernel in ((7434, 'auction_cluster_kernel'), (7435, 'auction_kernel')):
        assert _expected(1, n, 2)[0] == kernel
        a, c, od, oa, _, _ = _oracle('uniform', 1000 + n, 1, n, 0.005, 4)
        _same(_run(cuda, a, c, 0.005, 4, 2), (od, oa), f'n={n} auction_cluster=2')


def test_batch_beyond_one_cluster_launch(cuda):
    """b = 33 clusters of 8 workgroups on 256 CUs: two launches, of 32 samples and of 1 (asserted by `_run`)."""
    a, c, od, oa, _, _ = _oracle('uniform', 33, 33, 1024, 0.005, 5)
    if _cus() == 256:
        assert _expected(33, 1024, 0) == ('auction_cluster_kernel', 2)
    _same(_run(cuda, a, c, 0.005, 5), (od, oa), 'b=33')


def test_empty_batch_writes_nothing(cuda):
    t = torch.zeros(1, 64, 3, device=cuda)
    dist, ass = torch.full((1, 64), 7.0, device=cuda), torch.full((1, 64), 7, device=cuda, dtype=torch.int32)
    with _profiled():
        assert _raw_forward(cuda, 0, 64, t, t, 0.005, 5, dist, ass) == 0
        torch.cuda.synchronize()
        assert _launches('auction') == 0
    assert bool((dist == 7.0).all()) and bool((ass == 7).all())


# ---- 2. cloud kinds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [128, 513, 1024])
@pytest.mark.parametrize('kind', KINDS)
def test_cloud_kinds_match_the_oracle(cuda, kind, n):
    """Ties and near-ties: equal bid values across the lanes of a bidder (first maximum: `merge`), equal increments of
    several bidders for one target (the 1e-6 window, lowest bidder wins), zero increments (eps = 0: best == better for a
    duplicated target), and the forced last iteration on its own (iters = 1: every bidder takes its best target).
    n = 128: auction_kernel; 513: cluster of 4 (uneven slices) vs one workgroup; 1024: cluster of 8 vs one workgroup."""
    for iters in (30, 1):
        for eps in (0.005, 0.0):
            a, c, od, oa, _, _ = _oracle(kind, 2000 + n, 2, n, eps, iters)
            for forced in (0, 1):
                _same(_run(cuda, a, c, eps, iters, forced), (od, oa), f'{kind} n={n} iters={iters} eps={eps} auction_cluster={forced}')


# ---- 3. convergence and early exit ----------------------------------------------------------------------------------------
# (kind, n, eps, iters, schedules); iters is about twice the iteration count at which the oracle's assignment was
# measured to be complete.  "used" = iterations that started with an unassigned bidder, b = 2 samples, seed 3000 + n,
# as measured with the extended oracle:
CONVERGED = [
    ('uniform', 63, 0.02, 400, (0,)),             # used 103, 119
    ('uniform', 128, 0.02, 800, (0,)),            # used 311, 115
    ('uniform', 128, 0.05, 400, (0,)),            # used 250, 130
    ('dup_targets', 128, 0.02, 800, (0,)),        # used 273, 240
    ('lattice', 128, 0.02, 1600, (0,)),           # used 413, 344
    ('one_target', 128, 0.02, 400, (0,)),         # used 128, 128
    ('uniform', 513, 0.05, 1600, (0, 1, 2)),      # used 691, 509    cluster of 4, one workgroup, cluster of 2
    ('uniform', 1024, 0.05, 6400, (0, 1, 4)),     # used 906, 1451   cluster of 8, one workgroup, cluster of 4
]
_CONV_IDS = [f'{k}-n{n}-eps{e}' for k, n, e, _, _ in CONVERGED]


@pytest.mark.parametrize('kind,n,eps,iters,schedules', CONVERGED, ids=_CONV_IDS)
def test_converged_runs_take_the_early_exit(cuda, kind, n, eps, iters, schedules):
    """Every sample is completely assigned before `iters`: the kernels leave their iteration loop through `nu == 0`
    (auction_kernel) / through a zero bidder total of the sample (auction_cluster_kernel), and must give what the oracle
    gives when it stops there."""
    a, c, od, oa, _, used = _oracle(kind, 3000 + n, 2, n, eps, iters)
    print(f'{kind} n={n} eps={eps}: iterations used {used.tolist()} of {iters}')
    assert (used < iters).all() and (used > 1).all()
    assert all(len(np.unique(row)) == n for row in oa)  # complete
    for forced in schedules:
        _same(_run(cuda, a, c, eps, iters, forced), (od, oa), f'{kind} n={n} auction_cluster={forced}')


# ---- 4. bidders without a bid, non-finite inputs --------------------------------------------------------------------------
@pytest.mark.parametrize('n', [128, 1024])
def test_bidders_without_a_bid(cuda, n):
    """The contract of include/pcc_emd.h: a bidder with a NaN or infinite coordinate never bids -- assignment -1, dist NaN,
    zero gradient -- and costs nobody else anything: the rest of its sample is what the oracle (same rule) gives, the other
    samples are what a clean call gives, and nothing outside the call's own state was written (a clean call afterwards is
    still right; on the cluster path the parent code's `price[-1]` of bidder 0 / sample 0 was the word in front of the
    workspace).  A non-finite target is simply never chosen.  n = 128: auction_kernel; n = 1024: clusters of 8."""
    b, eps, iters = 4, 0.005, 20
    a, c, cd, ca, _, _ = _oracle('uniform', 4000 + n, b, n, eps, iters)
    nobid = {0: (0, n // 2, n - 1), 2: (1, n // 3, n - 2)}  # sample -> bidders with NaN, +inf, -inf in coordinate 0, 1, 2
    pa, pc = a.copy(), c.copy()
    for s, rows in nobid.items():
        for axis, (j, v) in enumerate(zip(rows, (np.nan, np.inf, -np.inf))):
            pa[s, j, axis] = v
    bad_target = n // 5
    pc[1, bad_target, 1] = np.nan

    import oracle

    od, oa, _, _ = oracle.auction_forward_ext(pa, pc, eps, iters)
    clean = _run(cuda, a, c, eps, iters)
    _same(clean, (cd, ca), 'clean, before')
    d, asg = _run(cuda, pa, pc, eps, iters)
    g = np.random.default_rng(n).standard_normal((b, n)).astype(np.float32)
    grad = _backward(cuda, pa, pc, g, asg)
    for s, rows in nobid.items():
        rows = list(rows)
        assert (asg[s, rows] == -1).all() and np.isnan(d[s, rows]).all()
        assert (grad[s, rows].view(np.uint32) << 1 == 0).all()  # +-0, never NaN
        rest = np.setdiff1d(np.arange(n), rows)
        assert (asg[s, rest] >= 0).all() and np.isfinite(d[s, rest]).all()
    assert bad_target not in asg[1] and (asg[1] >= 0).all() and np.isfinite(d[1]).all()
    _same((d, asg), (od, oa), 'poisoned')  # -1 and the NaN word included
    _same((d[3], asg[3]), (cd[3], ca[3]), 'untouched sample')
    _same(_run(cuda, a, c, eps, iters), (cd, ca), 'clean, after')


# ---- 5. backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,forced', [(128, 0), (1000, 0), (4096, 1)], ids=['one-workgroup', 'cluster', 'global-state'])
def test_backward_is_the_float32_expression(cuda, n, forced):
    """grad_xyz1 = (g * 2) * (xyz1 - xyz2[assignment]): the doubling is exact and the difference and the product are one
    rounding each, so numpy's float32 evaluation must match bit for bit.  Assignments outside [0, n) give zero rows."""
    a, c, _, oa, _, _ = _oracle('uniform', 5000 + n, 2, n, 0.005, 8)
    _, asg = _run(cuda, a, c, 0.005, 8, forced)
    assert np.array_equal(asg, oa)
    g = np.random.default_rng(n).standard_normal((2, n)).astype(np.float32)
    asg = asg.copy()
    out_of_range = {(0, 0): -1, (0, n - 1): n, (1, n // 2): n + 5, (1, 1): -7}
    for (s, j), v in out_of_range.items():
        asg[s, j] = v
    grad = _backward(cuda, a, c, g, asg)
    partner = np.take_along_axis(c, np.clip(asg, 0, n - 1)[..., None].astype(np.int64), 1)
    want = (g * np.float32(2))[..., None] * (a - partner)
    assert want.dtype == np.float32
    for s, j in out_of_range:
        want[s, j] = 0
    assert np.array_equal(grad.view(np.uint32), want.view(np.uint32))


# ---- 6. an oracle-independent check -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind,n,eps,iters,schedules', [p for p in CONVERGED if p[1] <= 513],
                         ids=[i for i, p in zip(_CONV_IDS, CONVERGED) if p[1] <= 513])
def test_converged_assignment_is_within_n_eps_of_the_optimum(cuda, kind, n, eps, iters, schedules):
    """The oracle was written to match the kernel, so a shared misreading of the algorithm passes every comparison above.
    This one uses the inputs, the library's outputs and the auction's own theorem only.

    Clouds in [0,1]^3, s_jk = |a_j - c_k| <= sqrt(3), exact bid value v_jk = 3 - s_jk - p_k.  While a bidder is
    unassigned some target has never been bid on and has price 0, so the best value is >= 3 - sqrt(3) and every price a
    bid sets is <= sqrt(3) + eps (<= 2 sqrt(3) + 2 eps for the bid on the last free target, which ends the auction): prices,
    increments and |v| stay below 4.
      * delta, the error of one computed bid value: the squared distance carries the rounding of the three differences
        (relative 2u on each square) and of the three operations of sq3 (3u), the correctly rounded square root halves that
        and adds u: s~ = s (1 + 3.5u), |s~ - s| <= 3.5 u sqrt(3) < 8u; `3.0 - s~ - p` is exact in double and rounded
        once to float (<= 4u).  delta = 12u.
      * rho, the rounding of the price update: `best - better + eps` is two float operations (2 * 4u), `price + inc` one
        (4u).  rho = 12u.
    When j bids for t the new price leaves it v_jt >= better~ - eps - delta - rho while every other target has
    v_jk <= better~ + delta; prices of other targets only rise afterwards and p_t is fixed while j holds t.  So a complete
    assignment satisfies (eps + 2 delta + rho)-complementary slackness and costs at most the optimum plus n times that
    (Bertsekas 1988, prop. 1): the bound below, with 2 delta + rho = 36u = 2.1e-6 against eps >= 0.02.  Nothing in it is fitted;
    the oracle sits at 0.05 to 0.15 of n eps on such inputs."""
    from scipy.optimize import linear_sum_assignment

    a, c = _clouds(kind, 3000 + n, 2, n)
    assert a.min() >= 0 and a.max() <= 1 and c.min() >= 0 and c.max() <= 1
    d, asg = _run(cuda, a, c, eps, iters, schedules[-1])
    a64, c64 = a.astype(np.float64), c.astype(np.float64)
    for s in range(2):
        assert np.array_equal(np.sort(asg[s]), np.arange(n)), 'not a permutation'
        d64 = ((a64[s] - c64[s][asg[s]]) ** 2).sum(-1)
        # dist = sq3 of float32 differences: each difference one rounding (2u on its square), sq3 three more: gamma_5
        assert (np.abs(d[s].astype(np.float64) - d64) <= 5 * U / (1 - 5 * U) * d64).all()
        cost = np.sqrt(((a64[s][:, None, :] - c64[s][None, :, :]) ** 2).sum(-1))
        r, col = linear_sum_assignment(cost)
        opt, got = cost[r, col].sum(), np.sqrt(d64).sum()
        print(f'{kind} n={n} eps={eps} sample {s}: cost - optimum = {got - opt:.6f} = {(got - opt) / (n * eps):.4f} n eps')
        assert got >= opt - 1e-9 * n
        assert got <= opt + n * (eps + 36 * U)


# ---- 7. eps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('eps', [-0.01, float('nan')])
@pytest.mark.parametrize('n', [128, 1024])
def test_negative_or_nan_eps_is_refused(cuda, eps, n):
    """The highest increment per target is an integer atomicMax on float bits, which orders increments >= 0 only."""
    t = torch.rand(2, n, 3, device=cuda)
    dist, ass = torch.full((2, n), 7.0, device=cuda), torch.full((2, n), 7, device=cuda, dtype=torch.int32)
    with _profiled():
        assert _raw_forward(cuda, 2, n, t, t, eps, 5, dist, ass) == PCC_EINVAL
        assert b'eps' in _lib().lib.pcc_last_error()
        torch.cuda.synchronize()
        assert _launches('auction') == 0
    assert bool((dist == 7.0).all()) and bool((ass == 7).all())
    if n % 1024 == 0:
        from emd import emdModule

        with pytest.raises(RuntimeError, match='eps'):
            emdModule()(t, t, eps, 5)
