"""numpy reference of the sliced Wasserstein loss (``pcc_sliced_wasserstein``, include/pcc_structural.h) for
tests/test_sliced_wasserstein_host.py and tests/test_gpu_sliced_wasserstein.py.

The forward is the contract word for word in float32: the projection ``(v0 * t0 + v1 * t1) + v2 * t2`` (three rounded
products, two rounded sums), -0 taken as +0, a stable argsort (NaN above +inf, equal values by ascending index), the
halving tree over the squared rank differences padded to a power of two, the chain over the directions in ascending
order, and ``inv`` = the float32 nearest to 1 / (n p).  The gradient is float64 on the contract's float32 differences and
the reference's own permutations, together with the per-element ``sum_p |d theta_c|`` the summation bound needs."""

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32
CHUNK = 8       # PCC_SW_CHUNK: projections per workgroup
# how many points variant v = 1 .. 10 of the sw_path switch holds (include/pcc_test_hooks.h)
VARIANT_CAPACITY = (64, 128, 256, 512, 1024, 2048, 4096, 8192, 2048, 4096)
# ... and its (threads, elements per thread), which its exact launch-profile name carries
VARIANT_SHAPE = ((64, 1), (64, 2), (64, 4), (128, 4), (256, 4), (512, 4), (1024, 4), (1024, 8), (256, 8), (512, 8))
assert all(t * e == cap for (t, e), cap in zip(VARIANT_SHAPE, VARIANT_CAPACITY))


def kernel_of(n, forced=0):
    """The slice kernel a cloud of ``n`` points runs: the product takes the first variant that holds
    the cloud; a forced variant that cannot hold it is ignored."""
    v = forced - 1 if forced and VARIANT_CAPACITY[forced - 1] >= n else next(i for i, cap in enumerate(VARIANT_CAPACITY) if cap >= n)
    return 'sw_slice_kernel<%d,%d>' % VARIANT_SHAPE[v]


# The grid of the forward tests.  n: the sizes the issue names -- they hold both sides of every power of two from 64 to
# 2048, where the kernel changes its thread count or its elements per thread -- and 4097, 8191 for the last two changes
# (n = 8193 is refused).  p: the sizes the issue names and both sides of the chunk boundaries 8, 16 and 128.
N_GRID = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096,
          4097, 5000, 8191, 8192)
P_GRID = (1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129)
# the reduced grids of the host tests (the same code path for every size: torch, not the kernel)
N_HOST = (1, 2, 3, 63, 64, 65, 257, 1000)
P_HOST = (1, 2, 7, 8, 9, 17)


def gamma(d):
    """The bound of a float32 sum of d terms in any order: |computed - exact| <= gamma(d) * sum |terms|."""
    d = np.asarray(d, dtype=np.float64)
    return d * U / (1.0 - d * U)


def inv_of(n, p):
    return np.float32(1.0 / (float(n) * float(p)))


def clouds(seed, b, n, scale=1.0, shift=0.0):
    """Two Gaussian clouds ``[b,n,3]`` float32, the second one shifted and scaled a little differently."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((b, n, 3)) * scale + shift).astype(np.float32)
    y = (rng.standard_normal((b, n, 3)) * (0.8 * scale) + (shift + 0.1 * scale)).astype(np.float32)
    return x, y


def unit_directions(seed, p):
    t = np.random.default_rng(seed).standard_normal((p, 3))
    return (t / np.linalg.norm(t, axis=1, keepdims=True)).astype(np.float32)


def dyadic_directions(seed, p):
    """Components from {0, +-1/2, +-1}; row 0 is all zeros, row 1 (if any) has two zero components."""
    t = np.random.default_rng(seed).choice(np.array([0, .5, -.5, 1, -1], dtype=np.float32), size=(p, 3))
    t[0] = 0
    if p > 1:
        t[1] = (0, 1, 0)
    return t


def lattice_clouds(seed, b, n, reach=64):
    """Integer coordinates with |v| <= reach, about a third of the points duplicates of others, zeros of both signs."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        c = rng.integers(-reach, reach + 1, size=(b, n, 3)).astype(np.float32)
        src = rng.integers(0, n, size=(b, n))
        dup = rng.random((b, n)) < 1 / 3
        c = np.where(dup[..., None], np.take_along_axis(c, src[..., None].repeat(3, 2), 1), c)
        c[rng.random((b, n, 3)) < 0.1] = -0.0
        c[rng.random((b, n, 3)) < 0.1] = 0.0
        out.append(c)
    return out


def project(v, theta):
    """``t[b,p,n]`` float32 of ``v[b,n,3]`` on ``theta[p,3]``; -0 comes out as +0."""
    v, th = v[:, None, :, :], theta[None, :, None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        t = ((v[..., 0] * th[..., 0]).astype(np.float32) + (v[..., 1] * th[..., 1]).astype(np.float32)).astype(np.float32)
        t = (t + (v[..., 2] * th[..., 2]).astype(np.float32)).astype(np.float32)
    return np.where(t == 0, np.float32(0), t)


class Forward:
    """``cost[b]``, ``cost_p[b,p]`` float32 and what the gradient needs: ``d[b,p,n]`` float32 and the permutations
    ``perm_x``, ``perm_y`` ``[b,p,n]`` (rank -> point).  Compare words through ``.view(np.uint32)``."""

    def __init__(self, x, y, theta):
        b, n, _ = x.shape
        p = theta.shape[0]
        tx, ty = project(x, theta), project(y, theta)
        self.perm_x, self.perm_y = np.argsort(tx, axis=2, kind='stable'), np.argsort(ty, axis=2, kind='stable')
        with np.errstate(invalid='ignore', over='ignore'):
            self.d = (np.take_along_axis(tx, self.perm_x, 2) - np.take_along_axis(ty, self.perm_y, 2)).astype(np.float32)
            size = 1
            while size < n:
                size *= 2
            e = np.zeros((b, p, size), dtype=np.float32)
            e[..., :n] = (self.d * self.d).astype(np.float32)
            while size > 1:
                size //= 2
                e = (e[..., :size] + e[..., size:2 * size]).astype(np.float32)
            self.cost_p = e[..., 0].copy()
            total = self.cost_p[:, 0].copy()
            for k in range(1, p):
                total = (total + self.cost_p[:, k]).astype(np.float32)
            self.inv = inv_of(n, p)
            self.cost = (total * self.inv).astype(np.float32)


class Grad:
    """Float64 gradients of ``cost`` for the permutations of ``fwd``: ``gx``, ``gy`` ``[b,n,3]`` and the per-element sums
    of the absolute terms ``gx_abs``, ``gy_abs`` (without the factor 2 inv)."""

    def __init__(self, fwd, theta):
        d = fwd.d.astype(np.float64)
        th = theta.astype(np.float64)
        self.two_inv = 2.0 * float(fwd.inv)
        self.p = theta.shape[0]

        def by_point(perm, diff):
            out = np.empty_like(diff)
            np.put_along_axis(out, perm, diff, 2)
            return out

        dx, dy = by_point(fwd.perm_x, d), by_point(fwd.perm_y, -d)
        self.gx = 0.0 + np.einsum('bpn,pc->bnc', dx, th) * self.two_inv
        self.gy = 0.0 + np.einsum('bpn,pc->bnc', dy, th) * self.two_inv
        self.gx_abs = np.einsum('bpn,pc->bnc', np.abs(dx), np.abs(th))
        self.gy_abs = np.einsum('bpn,pc->bnc', np.abs(dy), np.abs(th))

    def ratio(self, got_x, got_y):
        """The largest |got - ref64| over its bound gamma(p + 2) * 2 inv * sum_p |d theta_c| (one rounding per product, p
        sums in any order, the final scale); elements whose bound is 0 must be met exactly."""
        worst = 0.0
        for got, ref, mag in ((got_x, self.gx, self.gx_abs), (got_y, self.gy, self.gy_abs)):
            if got is None:
                continue
            assert np.isfinite(got).all()
            err, bound = np.abs(got - ref), gamma(self.p + 2) * self.two_inv * mag
            assert (err[bound == 0] == 0).all()
            if (bound > 0).any():
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        return worst

    def check_bound(self, got_x, got_y):
        assert self.ratio(got_x, got_y) <= 1.0

    def check_exact(self, got_x, got_y):
        """Inputs whose products and partial sums are exact: the words are those of the float64 result (a zero is +0: the
        sums start from +0)."""
        for got, ref in ((got_x, self.gx), (got_y, self.gy)):
            if got is not None:
                assert np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))
