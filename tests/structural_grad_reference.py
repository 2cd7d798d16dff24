"""Float64 references, derived error bounds and case tables for the stored-index and stored-match gradient kernels:
nn_bwd_range_kernel (csrc/chamfer.hip: pcc_nndistancegrad, pcc_chamfer_loss_grad, pcc_chamfer_emd_grad) and
am_row_kernel / am_grad_fused_kernel (csrc/matchcost.hip: pcc_matchcost, pcc_matchcostgrad, pcc_matchcostgrad_scaled).

Shared by tests/test_gpu_structural_grads.py (the kernels, on a GPU) and tests/test_structural_grad_bounds.py (no GPU:
a float32 restatement of the kernels' formulas must meet every bound, eight wrong variants must miss them).  Plain
numpy in float64 on the float32 inputs; nothing here calls the CPU oracle.

Notation (tests/bn_pair_reference.py): u = 2^-24, g(k) = k u / (1 - k u) bounds the relative error of a product of k
factors (1 + d_i), |d_i| <= u.  The library is built with -ffp-contract=off: a product followed by a sum is two
roundings unless the source says fmaf.

Chamfer backward, nn_bwd_range_kernel
-------------------------------------
    grad1[j] = 2 g1[j] (p1_j - p2[idx1[j]]) - sum_{k: idx2[k] = j} 2 g2[k] (p2_k - p1_j)        (and symmetrically grad2)
Every term is fl(g' fl(a - b)) with g' = 2 g exact: two roundings.  The loss entries form g = fl(gloss / n) (mean) in
the kernel: one more.  The deg + 1 terms of an element (deg = the number of scattered terms) are summed in float32 in
whatever order the LDS atomics retire, so a term passes through at most deg additions:
    |got - ref64| <= g(deg + 3) sum|t|.
The ChamferEMD tail is out = fl(acc + fl(a s)): a rounded product (u |a s|), then a rounded sum (u |out|):
    |out - out64| <= (g(deg + 3) sum|t| + u |a s|) (1 + u) + u |out64|.
Exact mode: coordinates on the lattice Z / 16 in [-L / 16, L / 16], integer upstream gradients |c| <= cmax, and for
`mean` gloss[b] = c_b n m, so that gloss / n = c_b m exactly; every term is then a multiple of the quantum 2 / 16 and,
as long as sum|t| stays below 2^24 quanta, every partial sum in every order is exact: the float32 result is the float64
result word for word.  L and cmax shrink until that holds for the case's index lists (a hub of 2048 terms at the
workload's shape with `mean` leaves L = 1, cmax = 1); `assert_exact` checks it on the reference itself.

The destination ranges.  launch_bwd cuts a sample into P ranges, restated in `bwd_ranges`:
    P = max(1, ceil(512 / b));  P = min(P, max(1, min(n, m) / 64));  P = max(P, (n + m) 12 / (48 KiB) + 1)
and range p of a cloud of n points is [n p / P, n (p + 1) / P).

Match cost and gradients, am_row_kernel / am_grad_fused_kernel
--------------------------------------------------------------
    cost[b] = sum_{k,l} match[b,k,l] |p1_l - p2_k|
    grad1[b,l] = sum_k t[k,l],  grad2[b,k] = -sum_l t[k,l],  t = match (p1_l - p2_k) rsqrt(fmax(|p1_l - p2_k|^2, 1e-20f))
(fmax as the instruction takes it: a NaN squared distance gives 1e-20f, so a NaN coordinate leaves NaN in its own
component only; the reference does what the kernel does).
Squared distance: d = fl(a - b) carries u, d^2 carries 2u, fmaf(dz,dz, fmaf(dx,dx, fl(dy dy))) three more roundings on
non-negative terms: relative g(5); through a square root that is at most g(3).
Gradient term: f = fl(match v_rsq_f32(.)), t = fl(d f): E_T = (1 + g(6)) (1 + R_RSQ) - 1  (d: 1, the root's argument: 3,
two products: 2).  Depth of the sums, from the loops of am_grad_fused_kernel (kGradRT = 64 rows, kGradSlab = 1024):
  grad1: a lane adds the <= 16 rows of its wave one after the other, waves 1, 2, 3 are added to wave 0 in turn (3),
         reduce_splits_kernel adds the row tiles in index order (ceil(m / 64) - 1), and the upstream gradient is one
         more product:                         D1 = 16 + 3 + ceil(m / 64) - 1 (+ 1 scaled)
  grad2: a lane subtracts its 4 x 4 columns of the slab one after the other (16), the wave tree has 6 levels,
         reduce_splits_kernel adds the slabs (ceil(n / 1024) - 1), the upstream gradient one more product:
                                               D2 = 16 + 6 + ceil(n / 1024) - 1 (+ 1 scaled)
    |grad - grad64| <= ((1 + E_T) (1 + g(D)) - 1) sum|t|.
Cost term: fmaf(match, v_sqrt_f32(d2), csum): the product is not rounded; the root carries E_S = (1 + g(3)) (1 + R_SQRT) - 1.
Depth, from am_row_kernel (kRowRT = 32 rows, 8 per wave; chunks of 2048 columns) and reduce_rows_kernel: a lane's
chain runs over the chunks, its wave's 8 rows and its 4 ceil(cnt / 256) columns of each (LC steps), then the wave
tree (6), the four waves (3), a thread of reduce_rows_kernel adds ceil(tiles / 256) partials and the tree over 256
threads has 8 levels:                          DC = LC + 6 + 3 + ceil(ceil(m / 32) / 256) + 8
    |cost - cost64| <= ((1 + E_S) (1 + g(DC)) - 1) sum |match| d.
At n = 4100, m = 130 that is DC = 562: 3.4e-5 relative, where an any-order bound would be g(n m) = 3e-2.
v_rsq_f32: R_RSQ of tests/bn_pair_reference.py.  v_sqrt_f32 was measured the same way, exhaustively over [1, 4) against
the float64 square root, by tools/sqrt_probe.hip on an MI355X: the worst error is SQRT_MEASURED_ULP ulp, rounded up to
SQRT_ULPS whole ulp (both recorded beside RSQ_MEASURED_ULP in tests/bn_pair_reference.py, with the command); one ulp is
at most 2u relative.
"""

from __future__ import annotations

import numpy as np

from tests.bn_pair_reference import R_RSQ, R_SQRT, SQRT_MEASURED_ULP, SQRT_ULPS, U, g  # noqa: F401  (the measured constants live there)

TINY = float(np.float32(1e-20))  # the kernel's 1e-20f
E_T = (1 + g(6)) * (1 + R_RSQ) - 1
E_S = (1 + g(3)) * (1 + R_SQRT) - 1
QUANTA = 2.0 ** 24

K_ROW_RT, K_ROW_CH = 32, 2048        # am_row_kernel: rows per workgroup, columns per staged chunk
K_GRAD_RT, K_GRAD_SLAB = 64, 1024    # am_grad_fused_kernel: rows per workgroup, columns per slab
STEP = 1.0 / 16.0                    # exact mode: the coordinate lattice
QUANTUM = 2.0 * STEP                 # ... and what every term is a multiple of


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


# ---- checks -------------------------------------------------------------------------------------------------------------


def assert_close(what, got, ref, bound):
    """got within bound of ref wherever ref is finite; NaN where ref is NaN; the same infinity where ref is one.
    Returns the worst |got - ref| / bound over the finite elements (0 where both are exactly equal)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    fin = np.isfinite(ref)
    with np.errstate(invalid='ignore', divide='ignore'):
        err = np.abs(got - ref)
        bad = np.where(fin, ~(err <= bound), ~((got == ref) | (np.isnan(got) & np.isnan(ref))))
        ratio = np.where(fin & (err > 0), err / bound, 0.0)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} elements beyond the bound; first at {at}: got '
                             f'{got[at]!r}, reference {ref[at]!r}, bound {bound[at]:.3e}')
    return float(ratio.max()) if ratio.size else 0.0


def assert_words(what, got, want):
    """Two float32 arrays hold the same values word for word (NaN equals NaN; a zero of either sign is a zero)."""
    got = np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, want.dtype)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError(f'{what}: {int(bad.sum())} of {bad.size} words differ; first at {at}: {got[at]!r} != {want[at]!r}')


def assert_exact(what, ref, mag, quantum=QUANTUM):
    """The exact-mode premise, checked on the reference: sum|t| below 2^24 quanta and a float64 result that float32 holds."""
    assert float(np.max(mag, initial=0.0)) / quantum < QUANTA, f'{what}: sum|t| reaches 2^24 quanta, partial sums may round'
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), f'{what}: the reference does not fit float32'


# ---- Chamfer backward -----------------------------------------------------------------------------------------------------
#   (id, b, n, m); P from bwd_ranges
CHAMFER_CASES = [
    ('p1-single', 1, 1, 1),          # min(n, m) / 64 = 0 -> P = 1
    ('p1-small', 2, 3, 5),           # P = 1
    ('p1-n1', 1, 1, 300),            # min / 64 = 0 -> P = 1; every idx2 is 0: a natural hub of 300
    ('p2-uneven', 3, 257, 130),      # ceil(512 / 3) = 171, 130 / 64 = 2 -> P = 2: ranges 128 | 129 and 65 | 65
    ('p8-by-b', 64, 600, 515),       # ceil(512 / 64) = 8 = 515 / 64 -> P = 8: 75-point and 64 / 65-point ranges
    ('p1-by-b', 513, 70, 64),        # ceil(512 / 513) = 1 although min / 64 = 1
    ('p3-lds-n5', 1, 5, 8200),       # min / 64 = 0 -> 1, LDS floor 8205 * 12 / 49152 + 1 = 3: ranges of n hold 1, 2, 2 points
    ('p3-lds-m5', 1, 8200, 5),       # the same with the clouds exchanged
    ('p1-lds-full', 1, 4, 4091),     # 4095 * 12 = 49140 < 49152: the largest single range, 49164 bytes of LDS with the spare
    ('p32-workload', 2, 2048, 2048), # ceil(512 / 2) = 256, 2048 / 64 = 32 -> P = 32: the workload's own shape
]
CHAMFER_CASE_IDS = [c[0] for c in CHAMFER_CASES]
LIST_KINDS = ['nn', 'uniform', 'hub', 'border']


def bwd_ranges(b: int, n: int, m: int) -> int:
    """launch_bwd's P (csrc/chamfer.hip), restated."""
    p = max(1, ceil_div(512, b))
    p = min(p, max(1, min(n, m) // 64))
    return max(p, (n + m) * 12 // (48 * 1024) + 1)


def range_edges(n: int, p: int) -> list[int]:
    return [n * i // p for i in range(p + 1)]


def nn_lists_host(p1, p2):
    """First-minimum nearest neighbours in float64 (the tie rule of pcc_nndistance); the host stand-in for it."""
    b = p1.shape[0]
    i1 = np.empty(p1.shape[:2], np.int32)
    i2 = np.empty(p2.shape[:2], np.int32)
    for s in range(b):
        a, c = p1[s].astype(np.float64), p2[s].astype(np.float64)
        d = np.zeros((a.shape[0], c.shape[0]))
        for ax in range(3):
            d += (a[:, ax, None] - c[None, :, ax]) ** 2
        i1[s] = d.argmin(1)
        i2[s] = d.argmin(0)
    return i1, i2


def index_lists(kind, b, n, m, rng, p1=None, p2=None, nn_fn=nn_lists_host):
    """(idx1[b,n] into cloud 2, idx2[b,m] into cloud 1), int32, valid indices only (the entries do not check them).
    nn: nn_fn(p1, p2); uniform: any valid index; hub: one target per sample for a whole list; border: every index is
    the first, the last or the one-past-last element of one of the kernel's destination ranges."""
    if kind == 'nn':
        i1, i2 = nn_fn(p1, p2)
        return np.ascontiguousarray(i1, np.int32), np.ascontiguousarray(i2, np.int32)
    if kind == 'uniform':
        return rng.integers(0, m, (b, n)).astype(np.int32), rng.integers(0, n, (b, m)).astype(np.int32)
    if kind == 'hub':
        k = rng.integers(0, m, (b, 1))
        j = rng.integers(0, n, (b, 1))
        return np.broadcast_to(k, (b, n)).astype(np.int32), np.broadcast_to(j, (b, m)).astype(np.int32)
    assert kind == 'border', kind
    p = bwd_ranges(b, n, m)

    def pick(count, size, shape):
        e = range_edges(size, p)
        vals = sorted({v for i in range(p) for v in (e[i], e[i + 1] - 1, e[i + 1]) if 0 <= v < size})
        return np.asarray(vals)[rng.integers(0, len(vals), shape)].astype(np.int32)

    return pick(n, m, (b, n)), pick(m, n, (b, m))


def _degrees(idx, size):
    b = idx.shape[0]
    deg = np.zeros((b, size), np.int64)
    np.add.at(deg, (np.arange(b)[:, None], idx), 1)
    return deg


def chamfer_inputs(b, n, m, kind, mode, mean, seed, nn_fn=nn_lists_host):
    """One case's inputs, float32 / int32 numpy: p1, p2, idx1, idx2, per-point g1, g2 (pcc_nndistancegrad), per-sample
    gloss (the loss entries), emd1, emd2, gemd (the ChamferEMD tail).  mode 'exact': the lattice construction of the
    module docstring, budgeted for `mean` (gloss = c n m) or not (gloss = c); 'gauss': standard normal everything."""
    rng = np.random.default_rng(seed)
    if mode == 'gauss':
        p1 = rng.standard_normal((b, n, 3)).astype(np.float32)
        p2 = rng.standard_normal((b, m, 3)).astype(np.float32)
        idx1, idx2 = index_lists(kind, b, n, m, rng, p1, p2, nn_fn)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        return dict(p1=p1, p2=p2, idx1=idx1, idx2=idx2, g1=f(b, n), g2=f(b, m), gloss=f(b), emd1=f(b, n, 3),
                    emd2=f(b, m, 3), gemd=f(b))
    assert mode == 'exact', mode
    s1, s2 = (m, n) if mean else (1, 1)  # |gs1| = |c| m, |gs2| = |c| n with mean
    lim, cmax = 32, 3
    lists = None if kind == 'nn' else index_lists(kind, b, n, m, rng)
    for _ in range(8):
        p1 = (rng.integers(-lim, lim + 1, (b, n, 3)) * STEP).astype(np.float32)
        p2 = (rng.integers(-lim, lim + 1, (b, m, 3)) * STEP).astype(np.float32)
        idx1, idx2 = lists if lists is not None else index_lists('nn', b, n, m, rng, p1, p2, nn_fn)
        d1, d2 = int(_degrees(idx2, n).max()), int(_degrees(idx1, m).max())
        # quanta of 2 / 16 an element can reach: cmax 2 lim (direct + deg scattered), plus the tail's 8 * 3 eighths
        need = lambda lm, cm: cm * 2 * lm * max(s1 + d1 * s2, s2 + d2 * s1) + 64
        if need(lim, cmax) < QUANTA:
            break
        if need(1, cmax) >= QUANTA:
            cmax = 1
        lim = max(1, min(lim - 1, int((QUANTA - 65) // (cmax * 2 * max(s1 + d1 * s2, s2 + d2 * s1)))))
    else:
        raise AssertionError('no lattice fits 2^24 quanta for this case')
    ci = lambda *s: rng.integers(-cmax, cmax + 1, s).astype(np.float32)
    gloss = ci(b) * np.float32(n * m if mean else 1)
    assert np.array_equal(gloss.astype(np.float64), np.round(gloss.astype(np.float64)))
    emd = lambda *s: (rng.integers(-8, 9, s) / 8.0).astype(np.float32)
    return dict(p1=p1, p2=p2, idx1=idx1, idx2=idx2, g1=ci(b, n), g2=ci(b, m), gloss=gloss, emd1=emd(b, n, 3),
                emd2=emd(b, m, 3), gemd=rng.integers(-3, 4, b).astype(np.float32))


def chamfer_bwd_ref(p1, p2, idx1, idx2, g1, g2):
    """Float64 gradients of sum g1 dist1 + sum g2 dist2 for stored neighbour lists; g1[b,n], g2[b,m] float64.
    -> {'grad1', 'grad2'} (reference), {'mag1', 'mag2'} (sum|t| per element), {'deg1', 'deg2'} (scattered terms)."""
    p1d, p2d = p1.astype(np.float64), p2.astype(np.float64)
    b, n, m = p1.shape[0], p1.shape[1], p2.shape[1]
    bi = np.arange(b)[:, None]
    with np.errstate(invalid='ignore', over='ignore'):
        t1 = 2.0 * np.asarray(g1, np.float64)[..., None] * (p1d - p2d[bi, idx1])  # [b, n, 3]
        t2 = 2.0 * np.asarray(g2, np.float64)[..., None] * (p2d - p1d[bi, idx2])  # [b, m, 3]
        grad1, grad2, mag1, mag2 = t1.copy(), t2.copy(), np.abs(t1), np.abs(t2)
        np.add.at(grad1, (bi, idx2), -t2)
        np.add.at(grad2, (bi, idx1), -t1)
        np.add.at(mag1, (bi, idx2), np.abs(t2))
        np.add.at(mag2, (bi, idx1), np.abs(t1))
    return dict(grad1=grad1, grad2=grad2, mag1=mag1, mag2=mag2, deg1=_degrees(idx2, n), deg2=_degrees(idx1, m))


def loss_gradients(gloss, b, n, m, mean, stride=1):
    """The per-point upstream gradients the loss entries stand for, float64: gloss[b * stride] (/ n, / m with mean)."""
    gl = np.asarray(gloss, np.float64)[np.arange(b) * stride]
    return (np.repeat((gl / n if mean else gl)[:, None], n, 1), np.repeat((gl / m if mean else gl)[:, None], m, 1))


def chamfer_bound(ref, which):
    """g(deg + 3) sum|t| for grad1 (which = 1) or grad2 (2)."""
    return g(ref[f'deg{which}'] + 3.0)[..., None] * ref[f'mag{which}']


def emd_tail_ref(ref, which, emd, gemd, b, stride=1):
    """(out64, bound, magnitude) of grad + emd * gemd[b * stride]; gemd None = 1."""
    s = np.ones(b) if gemd is None else np.asarray(gemd, np.float64)[np.arange(b) * stride]
    with np.errstate(invalid='ignore', over='ignore'):
        add = emd.astype(np.float64) * s[:, None, None]
        out = ref[f'grad{which}'] + add
        return out, (chamfer_bound(ref, which) + U * np.abs(add)) * (1 + U) + U * np.abs(out), ref[f'mag{which}'] + np.abs(add)


def _f32(x):
    return np.asarray(x, np.float32)


def chamfer_bwd_f32(p1, p2, idx1, idx2, g1=None, g2=None, gloss=None, mean=False, stride=1, emd1=None, emd2=None,
                    gemd=None, gemd_stride=1, seed=0, wrong=None):
    """nn_bwd_range_kernel restated in float32: the same rounding points, the scattered terms added one at a time in a
    shuffled order (the LDS atomics).  wrong: 'drop-range-last' (the scattered term of an index equal to the last
    element of a destination range is lost), 'mean-n-for-m' (cloud 2's gradient divided by n), 'g1-for-g2' (the scattered
    term into grad1 takes cloud 1's upstream gradient), 'tail-unscaled' (the ChamferEMD tail added without its scale)."""
    b, n, m = p1.shape[0], p1.shape[1], p2.shape[1]
    rng = np.random.default_rng(seed)
    bi = np.arange(b)[:, None]
    if gloss is not None:
        gs = _f32(gloss)[np.arange(b) * stride]
        gs1 = gs / np.float32(n) if mean else gs
        gs2 = gs / np.float32(n if wrong == 'mean-n-for-m' else m) if mean else gs
        g1 = np.repeat(gs1[:, None], n, 1)
        g2 = np.repeat(gs2[:, None], m, 1)
    g1, g2 = _f32(g1), _f32(g2)
    with np.errstate(invalid='ignore', over='ignore'):
        t1 = (g1 * np.float32(2))[..., None] * (p1 - p2[bi, idx1])
        t2 = (g2 * np.float32(2))[..., None] * (p2 - p1[bi, idx2])
        s2 = t2
        if wrong == 'g1-for-g2':  # the destination's own upstream gradient instead of the source's
            s2 = (np.take_along_axis(g1, idx2.astype(np.int64), 1) * np.float32(2))[..., None] * (p2 - p1[bi, idx2])
        p = bwd_ranges(b, n, m)

        def scatter(acc, idx, terms, size):
            keep = np.ones(idx.shape, bool)
            if wrong == 'drop-range-last':
                keep = ~np.isin(idx, np.asarray(range_edges(size, p)[1:]) - 1)
            # every destination's terms in a random order: term r of each destination is added in round r
            flat = (np.arange(b)[:, None] * size + idx)[keep]
            src = np.flatnonzero(keep.ravel())
            order = np.lexsort((rng.random(flat.size), flat))
            flat, src = flat[order], src[order]
            rank = np.arange(flat.size) - np.searchsorted(flat, flat, 'left')
            by_rank = np.argsort(rank, kind='stable')
            flat, src, rank = flat[by_rank], src[by_rank], rank[by_rank]
            out, tr = acc.reshape(-1, 3), terms.reshape(-1, 3)
            for r in range(int(rank[-1]) + 1 if rank.size else 0):
                lo, hi = np.searchsorted(rank, [r, r + 1])
                out[flat[lo:hi]] = out[flat[lo:hi]] - tr[src[lo:hi]]
            return out.reshape(acc.shape)

        acc1 = scatter(t1.copy(), idx2, s2, n)
        acc2 = scatter(t2.copy(), idx1, t1, m)
        if emd1 is not None:
            sc = np.ones(b, np.float32) if gemd is None or wrong == 'tail-unscaled' else _f32(gemd)[np.arange(b) * gemd_stride]
            acc1 = acc1 + emd1 * sc[:, None, None]
            acc2 = acc2 + emd2 * sc[:, None, None]
    assert acc1.dtype == np.float32 and acc2.dtype == np.float32
    return acc1, acc2


# ---- match cost and gradients -------------------------------------------------------------------------------------------------
#   (id, b, n, m).  n against kGradSlab = 1024 (slabs) and CH = 2048 (chunks of the row kernel); m against kRowRT = 32
#   and kGradRT = 64 (row tiles).  The 16-byte path needs n % 4 == 0; the largest match tensor is 4100 * 130 * 4 = 2.1 MB.
MATCH_CASES = [
    ('n1-m1', 1, 1, 1),
    ('n3-m3', 3, 3, 3),
    ('n1-m130', 3, 1, 130),          # one column; row tiles 64 | 64 | 2 and 32 x 4 | 2
    ('n3-m65', 1, 3, 65),            # 65 = one row past a 64-row tile
    ('n1023-m31', 1, 1023, 31),      # one column short of a slab, one row short of a 32-row tile; scalar path
    ('n1023-m63', 3, 1023, 63),      # one row short of a 64-row tile
    ('n1024-m32', 3, 1024, 32),      # exactly one slab (the branch-free body), exactly one 32-row tile
    ('n1024-m1', 1, 1024, 1),        # one row: three waves of the gradient kernel have nothing to do
    ('n1025-m33', 1, 1025, 33),      # a second slab of one column: part2, the second reduce; scalar path
    ('n1025-m64', 3, 1025, 64),      # exactly one 64-row tile
    ('n2048-m63', 1, 2048, 63),      # two whole slabs, exactly one chunk
    ('n2048-m3', 1, 2048, 3),
    ('n2048-m130', 1, 2048, 130),
    ('n2049-m64', 3, 2049, 64),      # a third slab and a second chunk of one column
    ('n2049-m33', 1, 2049, 33),
    ('n2052-m65', 1, 2052, 65),      # the same on the 16-byte path (2052 = 4 * 513): a slab and a chunk of 4 columns
    ('n2052-m32', 1, 2052, 32),
    ('n4100-m130', 1, 4100, 130),    # 5 slabs, 3 chunks, 3 row tiles of 64, 5 of 32; 16-byte path
    ('n4100-m31', 1, 4100, 31),
    ('n4-m8200', 1, 4, 8200),        # 257 row tiles of 32: the strided loop of reduce_rows_kernel; 129 tiles of 64
]
MATCH_CASE_IDS = [c[0] for c in MATCH_CASES]
ORACLE_MATCH_CASES = ['n1025-m64', 'n2049-m33']  # the CPU oracle's approxmatch output as `match`


def match_inputs(b, n, m, kind, seed):
    """p1[b,n,3], p2[b,m,3], match[b,m,n], gc[b] float32.  kind 'dense': standard normal clouds, match uniform on [0, 1);
    'coincident': cloud 2 repeats the points of cloud 1 (p2_k = p1_{k mod n}: d = 0 wherever l = k mod n)."""
    rng = np.random.default_rng(seed)
    p1 = rng.standard_normal((b, n, 3)).astype(np.float32)
    p2 = rng.standard_normal((b, m, 3)).astype(np.float32)
    if kind == 'coincident':
        p2 = np.ascontiguousarray(p1[:, np.arange(m) % n])
    match = rng.random((b, m, n), dtype=np.float32)
    gc = (rng.standard_normal(b) + np.where(rng.random(b) < 0.5, -2.0, 2.0)).astype(np.float32)  # never near 1
    return p1, p2, match, gc


def corner_entries(n, m, max_bytes=2 << 20):
    """(samples, rows, cols): rows / cols are the corners (first and last element) of every row tile of either kernel
    and of every slab and chunk; samples = as many rotations of the pairing as fit max_bytes, at most len(cols)."""
    rows = sorted({v for t in (K_ROW_RT, K_GRAD_RT) for i in range(ceil_div(m, t)) for v in (i * t, min(m, (i + 1) * t) - 1)})
    cols = sorted({v for t in (K_GRAD_SLAB, K_ROW_CH) for i in range(ceil_div(n, t)) for v in (i * t, min(n, (i + 1) * t) - 1)})
    samples = max(1, min(len(cols), max_bytes // (4 * n * m)))
    return samples, rows, cols


def corner_match(n, m, seed):
    """(match[s,m,n], list of (sample, row, col)): single-entry matches.  EVERY sample holds an entry on every row corner
    and on every column corner: entry i of sample s sits at (rows[i % len(rows)], cols[(i + s) % len(cols)]) for
    i < max(len(rows), len(cols)), so the shorter list is cycled (a row, or a column, then holds several entries, each
    in another column, or row) and the samples rotate which row corner meets which column corner.  Everything else is 0."""
    rng = np.random.default_rng(seed)
    samples, rows, cols = corner_entries(n, m)
    match = np.zeros((samples, m, n), np.float32)
    where = []
    for s in range(samples):
        for i in range(max(len(rows), len(cols))):
            r, c = rows[i % len(rows)], cols[(i + s) % len(cols)]
            if match[s, r, c] == 0:
                match[s, r, c] = np.float32(0.5 + rng.random())
                where.append((s, r, c))
    return match, where


def match_depths(n, m, scaled):
    """(D1, D2, DC) of the module docstring."""
    d1 = 16 + 3 + ceil_div(m, K_GRAD_RT) - 1 + (1 if scaled else 0)
    d2 = 16 + 6 + ceil_div(n, K_GRAD_SLAB) - 1 + (1 if scaled else 0)
    lc = sum(8 * 4 * ceil_div(min(K_ROW_CH, n - q0), 256) for q0 in range(0, n, K_ROW_CH))
    dc = lc + 6 + 3 + ceil_div(ceil_div(m, K_ROW_RT), 256) + 8
    return d1, d2, dc


def match_ref(p1, p2, match, gc=None):
    """Float64 cost and gradients over a stored match (gc: the upstream gradient per sample, None = 1) and their
    bounds: {'cost', 'grad1', 'grad2'} -> (reference, bound)."""
    b, n, m = p1.shape[0], p1.shape[1], p2.shape[1]
    scale = np.ones(b) if gc is None else np.asarray(gc, np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        diff = p1.astype(np.float64)[:, None, :, :] - p2.astype(np.float64)[:, :, None, :]  # [b, m, n, 3]: p1_l - p2_k
        d2 = (diff * diff).sum(-1)
        md = match.astype(np.float64)
        dist = np.sqrt(d2)
        cost, cost_mag = (md * dist).sum((1, 2)), (np.abs(md) * dist).sum((1, 2))
        t = (md / np.sqrt(np.fmax(d2, TINY)))[..., None] * diff * scale[:, None, None, None]
        grad1, mag1 = t.sum(1), np.abs(t).sum(1)
        grad2, mag2 = -t.sum(2), np.abs(t).sum(2)
    d1, dd2, dc = match_depths(n, m, gc is not None)
    return {'cost': (cost, ((1 + E_S) * (1 + g(dc)) - 1) * cost_mag),
            'grad1': (grad1, ((1 + E_T) * (1 + g(d1)) - 1) * mag1),
            'grad2': (grad2, ((1 + E_T) * (1 + g(dd2)) - 1) * mag2)}


def _fma32(a, b, c):
    """round32(a b + c): the product of two float32 is exact in float64, the sum correct to 2^-53."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _sq3_f32(dx, dy, dz):
    return _fma32(dz, dz, _fma32(dx, dx, dy * dy))


def _pad(a, shape):
    out = np.zeros(shape, a.dtype)
    out[tuple(slice(0, s) for s in a.shape)] = a
    return out


def matchcost_f32(p1, p2, match, wrong=None):
    """am_row_kernel + reduce_rows_kernel restated in float32 for one batch: every lane's fma chain in the kernel's
    order, the wave tree, the four waves, the strided sum and the tree of the reduce.  A correctly rounded square root
    stands in for v_sqrt_f32.  wrong: 'first-coords' (chunks after the first read the first chunk's points),
    'skip-tile-last-row' (the last row of every full 32-row tile is skipped)."""
    b, n, m = p1.shape[0], p1.shape[1], p2.shape[1]
    tiles, chunks = ceil_div(m, K_ROW_RT), ceil_div(n, K_ROW_CH)
    out = np.empty(b, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(b):
            q1 = p1[s]
            if wrong == 'first-coords':
                q1 = q1[np.arange(n) % K_ROW_CH]
            d = p2[s][:, None, :] - q1[None, :, :]  # [m, n, 3]: p2_k - p1_l, as the kernel takes it
            root = np.sqrt(_sq3_f32(d[..., 0], d[..., 1], d[..., 2]).astype(np.float64)).astype(np.float32)
            mv = match[s].copy()
            if wrong == 'skip-tile-last-row':
                mv[K_ROW_RT - 1:: K_ROW_RT] = 0
            term = _pad(mv.astype(np.float64) * root.astype(np.float64), (tiles * K_ROW_RT, chunks * K_ROW_CH))
            # row = tile 32 + 4 i + w; column = chunk 2048 + 256 j + 4 lane + q
            term = term.reshape(tiles, 8, 4, chunks, 8, 64, 4)  # [tile, i, w, chunk, j, lane, q]
            csum = np.zeros((tiles, 4, 64), np.float32)
            for ch in range(chunks):
                for i in range(8):
                    for j in range(8):
                        for q in range(4):
                            csum = (term[:, i, :, ch, j, :, q] + csum.astype(np.float64)).astype(np.float32)
            for off in (32, 16, 8, 4, 2, 1):
                csum[..., :off] = csum[..., :off] + csum[..., off:2 * off]
            w = csum[..., 0]
            part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
            red = np.zeros(256, np.float32)
            for i0 in range(0, tiles, 256):
                blk = part[i0:i0 + 256]
                red[: blk.size] = red[: blk.size] + blk
            for off in (128, 64, 32, 16, 8, 4, 2, 1):
                red[:off] = red[:off] + red[off:2 * off]
            out[s] = red[0]
    return out


def matchgrad_f32(p1, p2, match, gc=None, wrong=None):
    """am_grad_fused_kernel + reduce_splits_kernel restated in float32: column sums over a wave's rows in order, the
    waves in turn, the row tiles in turn; row sums over a lane's 16 columns in order, the wave tree, the slabs in turn;
    the upstream gradient where the library applies it.  A correctly rounded 1 / sqrt stands in for v_rsq_f32.
    wrong: 'drop-slab-last' (the last column of a partial slab is dropped), 'first-coords' (slabs after the first read
    the first slab's points), 'grad2-unscaled' (grad2 is left unscaled when there is more than one slab),
    'skip-tile-last-row' (the last row of every full 64-row tile is skipped)."""
    b, n, m = p1.shape[0], p1.shape[1], p2.shape[1]
    slabs, row_tiles = ceil_div(n, K_GRAD_SLAB), ceil_div(m, K_GRAD_RT)
    npad = slabs * K_GRAD_SLAB
    grad1 = np.full((b, n, 3), np.nan, np.float32)
    grad2 = np.full((b, m, 3), np.nan, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(b):
            q1 = p1[s]
            if wrong == 'first-coords':
                q1 = q1[np.arange(n) % K_GRAD_SLAB]
            mv = _pad(match[s], (m, npad))
            if wrong == 'drop-slab-last' and n % K_GRAD_SLAB:
                mv[:, n - 1] = 0  # written, without its terms: the bound has to catch it, not an unwritten element
            d = _pad(q1, (npad, 3))[None, :, :] - p2[s][:, None, :]  # [m, npad, 3]: padded columns hold (0, 0, 0)
            d2 = _sq3_f32(d[..., 0], d[..., 1], d[..., 2])
            rs = (1.0 / np.sqrt(np.fmax(d2, np.float32(TINY)).astype(np.float64))).astype(np.float32)
            t = d * (mv * rs)[..., None]  # [m, npad, 3] float32
            live = np.ones(m, bool)
            if wrong == 'skip-tile-last-row':  # its terms are lost to grad1 and its grad2 row is written as 0
                live[K_GRAD_RT - 1:: K_GRAD_RT] = False
            # grad1: per row tile, wave w adds rows r_begin + w, + 4, ... in order; waves 1, 2, 3 join wave 0 in turn
            col = np.zeros((npad, 3), np.float32)
            for rt in range(row_tiles):
                r0, r1 = rt * K_GRAD_RT, min(m, (rt + 1) * K_GRAD_RT)
                waves = []
                for w in range(4):
                    acc = np.zeros((npad, 3), np.float32)
                    for r in range(r0 + w, r1, 4):
                        if live[r]:
                            acc = acc + t[r]
                    waves.append(acc)
                tile = ((waves[0] + waves[1]) + waves[2]) + waves[3]
                col = tile if rt == 0 else col + tile
            if gc is not None:
                col = col * np.float32(gc[s])
            grad1[s] = col[:n]
            # grad2: lane sums over (step, q) in order, tree over the 64 lanes, slabs in turn
            tl = t.reshape(m, slabs, 4, 64, 4, 3)  # [row, slab, step, lane, q, c]
            rx = np.zeros((m, slabs, 64, 3), np.float32)
            for st in range(4):
                for q in range(4):
                    rx = rx - tl[:, :, st, :, q]
            for off in (32, 16, 8, 4, 2, 1):
                rx[:, :, :off] = rx[:, :, :off] + rx[:, :, off:2 * off]
            part = rx[:, :, 0]  # [m, slabs, 3]
            if slabs == 1:
                row = part[:, 0] * np.float32(gc[s]) if gc is not None else part[:, 0]
            else:
                row = part[:, 0]
                for sl in range(1, slabs):
                    row = row + part[:, sl]
                if gc is not None and wrong != 'grad2-unscaled':
                    row = row * np.float32(gc[s])
            grad2[s] = np.where(live[:, None], row, np.float32(0))
    return grad1, grad2
