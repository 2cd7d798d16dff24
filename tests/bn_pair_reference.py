"""Float64 references, derived error bounds and case tables for csrc/bnact.hip and csrc/pairwise.hip.

Shared by tests/test_gpu_bnact.py, tests/test_gpu_pairwise.py (the kernels, on a GPU) and tests/test_bn_pair_bounds.py
(no GPU: a float32 restatement of the kernels' formulas must meet every bound, three wrong variants must miss them).
Everything here is plain torch in float64 and runs on whatever device its inputs live on.

Notation: u = 2^-24 is the unit roundoff of float32; g(k) = k u / (1 - k u) bounds the relative error of a product of
k factors (1 + d_i), |d_i| <= u.

BatchNorm + ReLU (+ residual), csrc/bnact.hip
---------------------------------------------
Statistics.  The kernel adds z and z*z in double (each product exact in double), at most count/256 + 8 sequential
additions per partial, and rounds m = s/count and max(q/count - m*m, 0) to float32 once:
    |mean - mean64| <= u |mean64| + 2^-40 E|z|          |var - var64| <= u var64 + 2^-40 E[z^2]
The 2^-40 terms are ~30x the worst case of the double accumulation at count = 65536 (264 additions of relative error
2^-53 each) and seven orders below what a float32 accumulation would leave; on a channel z ~ N(1000, 1) the bound is
~1e-6 where a float32 E[z^2] - m^2 is off by ~0.1.  On integer inputs every sum is exact, so mean is the float32
rounding of the float64 quotient bit for bit and a constant channel has var == 0.0.

Forward.  The reference is float64 arithmetic on the same float32 mean, var, gamma, beta, eps the kernel receives.  The
kernel forms t = fl(var + eps), inv = v_rsq_f32(t), sc = fl(gamma inv), pre = fma(fl(z - mean), sc, beta),
y = fl(relu(pre) + res).  The relative error of inv is DINV = g(1) + R (the rounding of t, halved
by the square root but counted whole, and the instruction's own error R); of sc, DELTA = DINV + u.  Then
    |y - y64| <= (DELTA + 2u) (|z sc| + |mean sc|) + u |beta| + u |y64|
(the subtraction u and sc's DELTA on |(z - mean) sc| <= |z sc| + |mean sc|; the fma's rounding u relu(pre) <=
u (|(z - mean) sc| + |beta|); the final add u |y64|).  The shifted form fma(z, sc, fl(beta - fl(mean sc))) does not meet
this bound: it rounds beta twice, and loses ~u |mean sc| to cancellation on a large-mean channel.
v_rsq_f32's accuracy is not stated in the ISA text available to this project, so R was measured on an MI355X against
1/sqrt in float64, exhaustively over [1, 4) (all 2^24 mantissa / exponent-parity combinations; the relative error
repeats every two binades) and sampled over [2^-20, 2^20): the worst error is RSQ_MEASURED_ULP ulp, rounded up to
RSQ_ULPS whole ulp; one ulp is at most 2u relative.

Backward.  With mask = not (pre <= 0) (PyTorch's threshold_backward: a NaN pre-activation passes the gradient),
ga = g mask, xhat = (z - mean) inv, M = b n:
  grad_beta  = sum ga: four terms in float32 (3 additions), the running sum in double, one final rounding:
               Eb = (g(4) + 2^-40) sum|ga|; exact on integer g.
  grad_gamma = sum ga xhat: xhat carries DINV + 2u (the subtraction and the product), four fma steps in float32, the
               running sum in double, one final rounding: Eg = (DINV + g(7) + 2^-40) sum|ga xhat|.
  grad_z     = gsc (ga - a - xhat bq), a = fl(grad_beta fl(1/fl(b n))), bq likewise from grad_gamma:
               Ea = Eb / M + g(3) |a|, Ebq = Eg / M + g(3) |bq|, and with S = |ga| + |a| + |xhat bq|
               |grad_z - ref| <= |gsc| (Ea + Ebq |xhat| + (DINV + g(5)) S) + (DELTA + 2u) |ref|
               (eval mode: a = bq = 0 and the same expression).

The ReLU mask.  An element whose float64 pre-activation lies within the forward bound of zero may fall on either side
in float32, and one flipped element moves grad_z by a whole g.  `settle_mask` therefore moves every element with
|pre64| < MASK_MARGIN x its own forward bound to 2 x that margin away from zero, re-derives the statistics in
training mode and repeats until none is left; the tests assert that none is.

Pairwise reductions, csrc/pairwise.hip
--------------------------------------
D = sum_c (p_c - q_c)^2 in difference form: t = fl(p - q) carries u, t^2 carries 2u, the fma chain one rounding per
channel, and every term is non-negative, so the error is relative: |D - D64| <= g(d + 3) D64.  The returned index j*
then satisfies D64[j*] <= min_j D64 (1 + 2 g(d + 3)).  The sum over nq is a sequential float32 sum of non-negative
terms: g(nq + d + 3) sum64.  grad_p = 2 g sum_j (p - q_j): 2|g| g(nq + 2) sum_j |p - q_j|.  grad_q = -2 sum_i g_i (p_i - q):
2 g(np + 3) sum_i |g_i (p_i - q)|.  On integer coordinates in [-8, 8] with sums below 2^24 everything is exact.
Non-finite rule of pcc_pair_argmin (pinned, not PyKeOps-derived): a NaN distance never wins; a row whose distances
are all NaN (or all +inf) returns index 0 and dist = +inf.
"""

from __future__ import annotations

import math

import torch

U = 2.0 ** -24
D40 = 2.0 ** -40
RSQ_MEASURED_ULP = 0.8636  # at x = 1.34368575 (worst relative error 1.5767 u); sampled binades: 0.8345
RSQ_ULPS = 1
# v_sqrt_f32, measured the same way (used by tests/structural_grad_reference.py).  Both instructions, exhaustively over
# [1, 4) against float64: build tools/sqrt_probe.hip with the line in its header, then `timeout -k 10 120 tools/sqrt_probe`
# on an MI355X; the run prints 0.9236 ulp for v_sqrt_f32 and reproduces the 0.8636 ulp of v_rsq_f32 above.
SQRT_MEASURED_ULP = 0.9236  # at x = 3.49945736
SQRT_ULPS = 1
MASK_MARGIN = 16.0
EPS = 1e-5


def g(k: float) -> float:
    return k * U / (1.0 - k * U)


R_RSQ = RSQ_ULPS * 2.0 * U
R_SQRT = SQRT_ULPS * 2.0 * U
DINV = g(1) + R_RSQ
DELTA = DINV + U

# ---- BatchNorm cases ---------------------------------------------------------------------------------------------------
# pick_splits(b, c) = min(b, max(1, ceil(2048 / c))); sample range sp = [b sp / splits, b (sp + 1) / splits).
# The two apply kernels run ceil(n / 1024) workgroups per (sample, channel) row; all four streaming kernels take the
# 16-byte path when n % 4 == 0 and their bases are 16-byte aligned.
# residual variants: None | (r, res_c)
#   (id, b, c, n, residual)
BN_CASES = [
    # ceil(2048 / 16) = 128 > b: splits = b = 3, one sample per range; n % 4 == 0: 16-byte path; r = 1
    ('splits-b-vec', 3, 16, 256, (1, 16)),
    # ceil(2048 / 100) = 21 < b = 32: ranges of 1 and 2 samples (32 sp / 21); r = 3, c % 3 != 0, res_c = ceil(100 / 3)
    ('splits-21-uneven', 32, 100, 260, (3, 34)),
    # 2048 / 1024 = 2 ranges of 16 samples; r = 2, res_c = c / 2
    ('splits-2-even', 32, 1024, 64, (2, 512)),
    # c >= 2048: splits = 1 (one workgroup adds all 31 samples), b c = 63488
    ('splits-1', 31, 2048, 8, None),
    # b c = 65535: grid.y at its maximum; splits = 1
    ('row-limit', 5, 13107, 4, None),
    # n % 4 != 0: scalar path, 2 workgroups per row, the last thread's group of 4 is ragged (1027 = 4 * 256 + 3)
    ('scalar-n1027', 2, 5, 1027, (2, 4)),  # res_c = 4 > ceil(5 / 2) = 3: one spare residual channel
    # 3 workgroups per row, the third holds one element
    ('scalar-n2049', 2, 3, 2049, (1, 3)),
    # n < 4: the tail loop only
    ('n3', 4, 7, 3, (3, 3)),
    ('n1', 4, 7, 1, None),
    # 1 / 2 / 4 workgroups per row
    ('n1024', 2, 6, 1024, (1, 9)),  # three spare residual channels
    ('n1025', 2, 6, 1025, None),
    ('n4096', 2, 6, 4096, (2, 3)),
    # b = 1: ceil(2048 / 64) = 32 > b, clamped to splits = 1
    ('b1', 1, 64, 512, (1, 64)),
    # the PCGen decoder's 1024 -> 1024 layers at B = 32, N = 2048 (268 MB per tensor); splits = 2
    ('workload', 32, 1024, 2048, (2, 512)),
]
BN_CASE_IDS = [c[0] for c in BN_CASES]
# channel roles (every case has c >= 3): 0 constant, 1 large mean N(1000, 1), the others N(0, 1) / integers
CONST_CH, BIG_CH = 0, 1


def pick_splits(b: int, c: int) -> int:
    return min(b, max(1, -(-2048 // c)))


def bn_inputs(b, c, n, residual, mode, seed):
    """z, gamma, beta, res, grad_y and eval-mode statistics, float32 on the CPU.  exact: integers in [-8, 8], beta = 0
    and half-integer eval means, so that |z - mean| >= 0.5 and no pre-activation is near zero; random: normal values,
    gamma of both signs, the constant channel with |beta| = 0.4."""
    gen = torch.Generator().manual_seed(seed)
    if mode == 'exact':
        z = torch.randint(-8, 9, (b, c, n), generator=gen).float()
        gy = torch.randint(-8, 9, (b, c, n), generator=gen).float()
        z[:, CONST_CH] = 3.0
        gamma = torch.randint(1, 4, (c,), generator=gen).float() * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float()
        beta = torch.zeros(c)
        mean = torch.randint(-2, 3, (c,), generator=gen).float() + 0.5
        var = torch.tensor([0.25, 1.0, 4.0])[torch.randint(0, 3, (c,), generator=gen)]
    else:
        z = torch.randn(b, c, n, generator=gen)
        gy = torch.randn(b, c, n, generator=gen)
        z[:, CONST_CH] = 0.75
        z[:, BIG_CH] += 1000.0
        gamma = (torch.rand(c, generator=gen) + 0.5) * (torch.randint(0, 2, (c,), generator=gen) * 2 - 1).float()
        beta = torch.rand(c, generator=gen) - 0.5
        beta[CONST_CH] = 0.4
        mean = 0.1 * torch.randn(c, generator=gen)
        mean[CONST_CH] += 0.75
        mean[BIG_CH] += 1000.0
        var = torch.rand(c, generator=gen) + 0.5
    res = None
    if residual is not None:
        r, res_c = residual
        res = (torch.randint(-8, 9, (b, res_c, n), generator=gen).float() if mode == 'exact'
               else torch.randn(b, res_c, n, generator=gen))
    return {'z': z, 'gamma': gamma, 'beta': beta, 'res': res, 'r': residual[0] if residual else 1, 'gy': gy,
            'mean': mean, 'var': var}


def _close(what, got, ref, bound):
    """got within bound of ref wherever ref is finite; NaN where ref is NaN; the same infinity where ref is one."""
    got = got.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = torch.isfinite(ref)
    bad = torch.where(fin, ~((got - ref).abs() <= bound), ~((got == ref) | (got.isnan() & ref.isnan())))
    if bad.any():
        err = torch.where(fin & bad, (got - ref).abs() - bound, torch.zeros_like(ref))
        where = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound; worst excess '
                             f'{float(err.max()):.3e}; first at {where}: got {float(got[tuple(where)])!r}, '
                             f'reference {float(ref[tuple(where)])!r}, bound {float(torch.as_tensor(bound).expand_as(ref)[tuple(where)]):.3e}')


def assert_close(what, got, ref, bound):
    _close(what, got, ref, bound)


def assert_bits(what, got, ref64):
    """got (float32) equals the float32 rounding of the float64 reference bit for bit."""
    want = ref64.float()
    bad = ~((got == want) | (got.isnan() & want.isnan()))
    assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 reference'


def bn_stats_ref(z):
    """(mean64, var64, bound_mean, bound_var) per channel over (b, n); biased variance, centred in float64."""
    zd = z.double()
    mean = zd.mean((0, 2))
    var = ((zd - mean.view(1, -1, 1)) ** 2).mean((0, 2))
    e_abs = zd.abs().mean((0, 2))
    e_sq = (zd * zd).mean((0, 2))
    return mean, var, U * mean.abs() + D40 * e_abs, U * var + D40 * e_sq


def _chan(t):
    return t.double().view(1, -1, 1)


def _expand_res(res, c, r):
    if res is None:
        return None
    idx = torch.arange(c, device=res.device) // r
    return res.double().index_select(1, idx)


def bn_fwd_ref(z, mean, var, eps, gamma, beta, res, r):
    """(y64, bound, pre64, pre_bound): float64 on the float32 operands; pre_bound is the bound without the final add."""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    zd = z.double()
    sc = _chan(gamma) / torch.sqrt(_chan(var) + eps)
    pre = (zd - _chan(mean)) * sc + _chan(beta)
    act = torch.where(pre < 0, torch.zeros_like(pre), pre)  # torch.relu: NaN stays NaN
    rr = _expand_res(res, z.shape[1], r)
    y = act if rr is None else act + rr
    pre_bound = (DELTA + 2 * U) * ((zd * sc).abs() + (_chan(mean) * sc).abs()) + U * _chan(beta).abs()
    return y, pre_bound + U * y.abs(), pre, pre_bound + U * act.abs()


def bn_bwd_ref(z, mean, var, eps, gamma, beta, gy, training):
    """{'grad_z', 'grad_gamma', 'grad_beta'} -> (reference, bound)."""
    eps = float(torch.tensor(eps, dtype=torch.float32))
    b, _, n = z.shape
    m = float(b * n)
    zd = z.double()
    inv = 1.0 / torch.sqrt(_chan(var) + eps)
    gsc = _chan(gamma) * inv
    pre = (zd - _chan(mean)) * gsc + _chan(beta)
    ga = torch.where(pre <= 0, torch.zeros_like(pre), gy.double())  # a NaN pre-activation passes the gradient
    xhat = (zd - _chan(mean)) * inv
    gx = ga * xhat
    sum_g, sum_gx = ga.sum((0, 2)), gx.sum((0, 2))
    eb = (g(4) + D40) * ga.abs().sum((0, 2))
    eg = (DINV + g(7) + D40) * gx.abs().sum((0, 2))
    if training:
        a, bq = (sum_g / m).view(1, -1, 1), (sum_gx / m).view(1, -1, 1)
        ea = eb.view(1, -1, 1) / m + g(3) * a.abs()
        ebq = eg.view(1, -1, 1) / m + g(3) * bq.abs()
        ref = gsc * (ga - a - xhat * bq)
        s = ga.abs() + a.abs() + (xhat * bq).abs()
        bound = gsc.abs() * (ea + ebq * xhat.abs() + (DINV + g(5)) * s) + (DELTA + 2 * U) * ref.abs()
    else:
        ref = gsc * ga
        bound = gsc.abs() * (DINV + g(5)) * ga.abs() + (DELTA + 2 * U) * ref.abs()
    return {'grad_z': (ref, bound), 'grad_gamma': (sum_gx, eg), 'grad_beta': (sum_g, eb)}


def ambiguous(z, mean, var, eps, gamma, beta):
    """Elements whose float64 pre-activation is within MASK_MARGIN forward bounds of zero, and (pre, bound, sc)."""
    _, _, pre, pb = bn_fwd_ref(z, mean, var, eps, gamma, beta, None, 1)
    sc = _chan(gamma) / torch.sqrt(_chan(var) + float(torch.tensor(eps, dtype=torch.float32)))
    return pre.abs() < MASK_MARGIN * pb, pre, pb, sc


def rounded_stats(z):
    mean, var, _, _ = bn_stats_ref(z)
    return mean.float(), var.float()


def settle_mask(z, gamma, beta, eps, mean=None, var=None, rounds=6):
    """z with every ambiguous element moved to 2 x MASK_MARGIN bounds away from zero (on the side it was on), and the
    float32 statistics that go with it: the given ones (eval mode) or the rounded float64 statistics of the moved z
    (training mode, repeated until none is left).  Raises if an ambiguous element remains after `rounds`."""
    training = mean is None
    z = z.clone()
    for _ in range(rounds):
        if training:
            mean, var = rounded_stats(z)
        bad, pre, pb, sc = ambiguous(z, mean, var, eps, gamma, beta)
        if not bad.any():
            return z, mean, var
        side = torch.where(pre >= 0, torch.ones_like(pre), -torch.ones_like(pre))
        # pb grows with |z sc|; 2.5 x leaves room for that and for the float32 rounding of the moved z
        moved = z.double() + (side * 2.5 * MASK_MARGIN * pb - pre) / sc
        z = torch.where(bad, moved.float(), z)
    raise AssertionError(f'{int(bad.sum())} elements still within the mask margin after {rounds} rounds')


# ---- float32 restatements of the BatchNorm kernels (numpy has no fma: emulated through float64) -------------------------


def _fma32(a, b, c):
    """round32(a b + c) for float32 tensors: the product is exact in float64, the sum correct to 2^-53."""
    return (a.double() * b.double() + c.double()).float()


def bn_stats_f32(z, drop_last_of_range=None, float32_sums=False):
    """The statistics kernel restated: double sums over the sample ranges of pick_splits, combined in range order.
    drop_last_of_range = sp: a wrong variant that skips the last sample of range sp.
    float32_sums: a wrong variant that accumulates z and z*z in float32."""
    b, c, n = z.shape
    if float32_sums:
        s = z.sum((0, 2), dtype=torch.float32)
        q = (z * z).sum((0, 2), dtype=torch.float32)
        mean = s / float(b * n)
        return mean, torch.clamp(q / float(b * n) - mean * mean, min=0.0)
    splits = pick_splits(b, c)
    zd = z.double()
    per_s, per_q = zd.sum(2), (zd * zd).sum(2)  # [b, c]
    s = torch.zeros(c, dtype=torch.float64)
    q = torch.zeros(c, dtype=torch.float64)
    for sp in range(splits):
        s0, s1 = b * sp // splits, b * (sp + 1) // splits
        if drop_last_of_range == sp:
            s1 -= 1
        s += per_s[s0:s1].sum(0)
        q += per_q[s0:s1].sum(0)
    m = s / float(b * n)
    v = q / float(b * n) - m * m
    return m.float(), torch.where(v < 0, torch.zeros_like(v), v).float()


def _coeffs_f32(mean, var, eps, gamma, beta):
    t = var + torch.tensor(eps, dtype=torch.float32)
    inv = (1.0 / torch.sqrt(t.double())).float()  # a correctly rounded stand-in for v_rsq_f32
    sc = gamma * inv
    return inv.view(1, -1, 1), sc.view(1, -1, 1), beta.view(1, -1, 1)


def bn_fwd_f32(z, mean, var, eps, gamma, beta, res, r):
    _, sc, bt = _coeffs_f32(mean, var, eps, gamma, beta)
    pre = _fma32(z - mean.view(1, -1, 1), sc, bt)
    act = torch.where(pre < 0, torch.zeros_like(pre), pre)
    if res is None:
        return act
    return act + res.index_select(1, torch.arange(z.shape[1]) // r)


def bn_bwd_f32(z, mean, var, eps, gamma, beta, gy, training):
    b, _, n = z.shape
    inv, sc, bt = _coeffs_f32(mean, var, eps, gamma, beta)
    mu = mean.view(1, -1, 1)
    pre = _fma32(z - mu, sc, bt)
    ga = torch.where(pre <= 0, torch.zeros_like(pre), gy)
    xhat = (z - mu) * inv
    sum_g = ga.double().sum((0, 2)).float()
    sum_gx = (ga.double() * xhat.double()).sum((0, 2)).float()
    if not training:
        return sc * ga, sum_gx, sum_g
    inv_count = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(float(b)) * torch.tensor(float(n)))
    a, bq = (sum_g * inv_count).view(1, -1, 1), (sum_gx * inv_count).view(1, -1, 1)
    return sc * (ga - a - xhat * bq), sum_gx, sum_g


# ---- pairwise ---------------------------------------------------------------------------------------------------------------
#   (b, np, nq, d)
PAIR_CASES = [
    (3, 1, 7, 4),         # np = 1
    (3, 9, 1, 4),         # nq = 1: the only candidate
    (2, 40, 33, 1),       # d = 1
    (2, 50, 40, 3),       # d = 3 through the C ABI (the wrapper sends 3-D clouds to pcc_nndistance)
    (4, 8, 16, 4),
    (3, 5, 7, 11),
    (2, 30, 20, 64),
    (1, 255, 9, 4),       # b np = 255 / 256 / 257: one workgroup short of, exactly, and one row past a workgroup
    (1, 256, 9, 4),
    (1, 257, 9, 4),
    (8192, 1, 16, 4),     # the reference's vqvae.yaml: 32 x 256 queries, book 16, dim 4
    (2, 2048, 2048, 5),
]


def pair_inputs(b, n_p, n_q, d, mode, seed):
    gen = torch.Generator().manual_seed(seed)
    if mode == 'exact':
        p = torch.randint(-8, 9, (b, n_p, d), generator=gen).float()
        q = torch.randint(-8, 9, (b, n_q, d), generator=gen).float()
        go = torch.randint(-8, 9, (b, n_p), generator=gen).float()
        if n_q > 1:  # many duplicated rows: ties in every argmin
            src = torch.arange(n_q) % (n_q // 3 + 1)
            q = q[:, src].contiguous()
        if n_q > 2 and n_p > 1:
            p[:, 1] = q[:, 1]  # a distance of exactly 0, twice or more
    else:
        p = torch.randn(b, n_p, d, generator=gen)
        q = torch.randn(b, n_q, d, generator=gen)
        go = torch.randn(b, n_p, generator=gen)
    return p, q, go


def first_argmin(dm):
    """(first index of the minimum over the last axis, the minimum); NaN counts as +inf; all +inf -> index 0."""
    dm = torch.where(dm.isnan(), torch.full_like(dm, math.inf), dm)
    best = dm.min(dim=-1).values
    ar = torch.arange(dm.shape[-1], device=dm.device).expand_as(dm)
    idx = torch.where(dm == best.unsqueeze(-1), ar, torch.full_like(ar, dm.shape[-1])).min(dim=-1).values
    return idx, best


def pair_ref(p, q, go):
    """Float64 D[b,i,j], its sum over j, both gradients of the sum, and the magnitudes the gradient bounds need."""
    diff = p.double().unsqueeze(2) - q.double().unsqueeze(1)  # [b, np, nq, d]
    dm = (diff * diff).sum(-1)
    gd = go.double().view(*go.shape, 1, 1)
    return {'D': dm, 'sum': dm.sum(2),
            'grad_p': 2 * gd[:, :, 0] * diff.sum(2), 'grad_p_mag': 2 * gd[:, :, 0].abs() * diff.abs().sum(2),
            'grad_q': -2 * (gd * diff).sum(1), 'grad_q_mag': 2 * (gd * diff).abs().sum(1)}


def pair_argmin_check(what, idx, dist, dm, d, exact):
    n_q = dm.shape[-1]
    assert idx.dtype == torch.int64 and ((idx >= 0) & (idx < n_q)).all(), f'{what}: index outside [0, {n_q})'
    ref_idx, best = first_argmin(dm)
    at = dm.gather(2, idx.unsqueeze(-1)).squeeze(-1)
    if exact:
        assert torch.equal(idx, ref_idx), f'{what}: {int((idx != ref_idx).sum())} indices are not the first minimum'
        if dist is not None:
            assert_bits(f'{what} dist', dist, best)
        return
    assert (at <= best * (1 + 2 * g(d + 3))).all(), f'{what}: an index whose distance is not within 2 g(d+3) of the minimum'
    if dist is not None:
        assert_close(f'{what} dist', dist, at, g(d + 3) * at)


def pair_bounds(ref, n_p, n_q, d):
    return {'sum': g(n_q + d + 3) * ref['sum'], 'grad_p': g(n_q + 2) * ref['grad_p_mag'],
            'grad_q': g(n_p + 3) * ref['grad_q_mag']}


def pair_f32(p, q, go, last_on_ties=False):
    """The pairwise kernels restated in float32 (fma through float64), loops in the kernels' order.
    last_on_ties: a wrong variant whose argmin keeps the last of equal distances."""
    b, n_p, d = p.shape
    n_q = q.shape[1]
    best = torch.full((b, n_p), math.inf)
    best_j = torch.zeros(b, n_p, dtype=torch.int64)
    total = torch.zeros(b, n_p)
    acc_p = torch.zeros(b, n_p, d)
    for j in range(n_q):
        qj = q[:, j:j + 1]  # [b, 1, d]
        acc = torch.zeros(b, n_p)
        for ch in range(d):
            t = p[:, :, ch] - qj[:, :, ch]
            acc = _fma32(t, t, acc)
        lt = acc <= best if last_on_ties else acc < best
        best = torch.where(lt, acc, best)
        best_j = torch.where(lt, torch.full_like(best_j, j), best_j)
        total = total + acc
        acc_p = acc_p + (p - qj)
    grad_p = 2.0 * go.unsqueeze(-1) * acc_p
    acc_q = torch.zeros(b, n_q, d)
    for i in range(n_p):
        acc_q = acc_q + go[:, i].view(b, 1, 1) * (p[:, i:i + 1] - q)
    return best_j, best, total, grad_p, -2.0 * acc_q
