"""numpy reference of the kernel point convolution (``pcc_kpconv_aggregate`` / ``pcc_kpconv_aggregate_bwd``,
include/pcc_neighbour.h) for tests/test_kpconv_host.py and tests/test_gpu_kpconv.py.

The contract fixes the words of the influences, of the forward and of the per-slot words ``p`` of the backward, so the
reference is its float32 loop: numpy's float32 subtraction, multiplication, addition and square root, one rounding each
(``np.sqrt`` of a float32 is the correctly rounded square root), a pair with ``h = +0.0`` left out, a NaN result the word
0x7fc00000.  The float64 versions of the same are what the closed forms and the autograd composition are held against.
``grad_x`` is the float64 sum of the float32 words ``p`` per bin, with the bin's in-degree and the sum of ``|p|`` for the
bound of a float32 sum in any order."""

import numpy as np

from tests.attention_reference import canonical, gaussian, same_words, valid_slots  # noqa: F401
from tests.interpolate_reference import NAN_WORD, U, cloud, gamma, random_list  # noqa: F401

# the grids of the forward and backward tests
N_GRID = (1, 3, 63, 64, 65, 1025)
M_GRID = (1, 3, 65, 257)
K_GRID = (1, 3, 4, 16, 17, 64, 128)
K_GRID_HOST = (1, 3, 16, 17)
CKP_GRID = ((1, 1), (3, 2), (8, 15), (9, 15), (5, 32))  # one block of kernel points and two, channel blocks whole and not
B_MAX, C_MAX = 3, 9
# n on both sides of every boundary of the backward's dispatch: the channel block 8 -> 4 -> 2 -> 1 (64 KB of bins), and LDS ->
# direct where the bins of a single channel no longer fit (160 KB).  The forward has one path: it runs at the same n.
BOUNDARIES = (2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 40960, 40961)
# the random-geometry inputs: clouds uniform in [0,1)^3, kernel_point_layout(kp, RADIUS), SIGMA
RADIUS, SIGMA = 0.5, 0.6


def grid():
    """(m, k, c, kp, b, j): every (m, k) with every (c, kp); b in {1, 3} rotates with the running number j."""
    j = 0
    for m in M_GRID:
        for k in K_GRID:
            for c, kp in CKP_GRID:
                yield m, k, c, kp, (1, 3)[j % 2], j
                j += 1


def layout(kp, radius=1.0):
    """``kernel_point_layout`` written independently: the origin, then a Fibonacci spiral on the sphere, float64 -> float32."""
    pts = np.zeros((kp, 3))
    for t in range(1, kp):
        i = t - 1
        z = 1.0 - (2.0 * i + 1.0) / (kp - 1)
        r = np.sqrt(1.0 - z * z)
        a = i * np.pi * (3.0 - np.sqrt(5.0))
        pts[t] = radius * np.array([r * np.cos(a), r * np.sin(a), z])
    return pts.astype(np.float32)


def uniform_geometry(seed, b, n, m):
    """``(xyz[b,n,3], centres[b,m,3])`` float32, uniform in [0,1)^3."""
    rng = np.random.default_rng(seed)
    return rng.random((b, n, 3), dtype=np.float32), rng.random((b, m, 3), dtype=np.float32)


def lattice_geometry(seed, b, n, m, kp):
    """``(xyz, centres, kernel_points)`` on the lattice Z x 2Z x 2Z, for ``sigma = 2``: a difference of lattice points has the
    length |a| of its first coordinate, or a length >= 2, so every influence is 1, 0.5 or 0 exactly -- and with integer
    gradients every word ``p`` and every sum of them is exact in any order.  Kernel point 0 is the origin."""
    rng = np.random.default_rng(seed)

    def pts(count, lo, hi, off):
        """x an integer in [lo, hi); y and z from {-2, 0, 2}, off 0 with probability ``off`` each."""
        yz = 2 * rng.integers(-1, 2, size=(count, 2)) * (rng.random((count, 2)) < off)
        return np.concatenate((rng.integers(lo, hi, size=(count, 1)), yz), -1).astype(np.float32)

    kpts = pts(kp, -2, 3, 0.5)
    kpts[0] = 0
    return pts(b * n, 0, 4, 0.3).reshape(b, n, 3), pts(b * m, 0, 4, 0.3).reshape(b, m, 3), kpts


def _relative(xyz, centres, idx, dtype):
    """``(valid[B,M,k], r[B,M,k,3])``: the neighbours relative to their centres, index 0 standing in for a slot that is no point."""
    b, n = xyz.shape[:2]
    m, k = idx.shape[1:]
    valid = valid_slots(idx, n)
    safe = np.where(valid, idx, 0).reshape(b, m * k, 1)
    nb = np.take_along_axis(xyz.astype(dtype), np.broadcast_to(safe, (b, m * k, 3)), axis=1).reshape(b, m, k, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        return valid, nb - centres.astype(dtype)[:, :, None, :]


def influence(xyz, centres, idx, kpts, sigma, dtype=np.float32):
    """``h[B,M,k,K]`` in ``dtype``: the contract's operations in its order, each rounded to ``dtype``; +0.0 on a slot that is
    no point and for a NaN or infinite distance."""
    valid, r = _relative(xyz, centres, idx, dtype)
    one = dtype(1.0)
    inv = one / dtype(np.float32(sigma))
    with np.errstate(invalid='ignore', over='ignore'):
        e = r[:, :, :, None, :] - kpts.astype(dtype)
        ex, ey, ez = e[..., 0], e[..., 1], e[..., 2]
        d2 = (ex * ex + ey * ey) + ez * ez
        v = one - np.sqrt(d2) * inv
        h = np.where((v > 0) & valid[..., None], v, dtype(0))
    assert h.dtype == dtype
    return h


def positive_share(h, idx, n):
    """The share of the (slot, kernel point) pairs of the valid slots with ``h > 0``."""
    valid = valid_slots(idx, n)
    return float((h[valid] > 0).mean()) if valid.any() else 0.0


def _gathered(x, idx):
    b, c, n = x.shape
    m, k = idx.shape[1:]
    safe = np.where(valid_slots(idx, n), idx, 0).reshape(b, 1, m * k)
    return np.take_along_axis(x, np.broadcast_to(safe, (b, c, m * k)), axis=2).reshape(b, c, m, k)


def forward(x, h):
    """``out[B, K * C, M]`` in the dtype of ``h``: ``acc = acc + (h * x[b,ch,idx])`` over the slots in order for the pairs with
    ``h > 0``; ``x`` here is the gathered ``[B,C,M,k]`` (``_gathered``).  float32: a NaN is the word 0x7fc00000."""
    b, c, m, k = x.shape
    kp = h.shape[3]
    acc = np.zeros((b, kp, c, m), dtype=h.dtype)
    xg = x.astype(h.dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(k):
            hj = np.moveaxis(h[:, :, j, :], 2, 1)[:, :, None, :]  # [B,K,1,M]
            acc = np.where(hj > 0, acc + hj * xg[:, None, :, :, j], acc)
    assert acc.dtype == h.dtype
    out = acc.reshape(b, kp * c, m)
    return canonical(out) if h.dtype == np.float32 else out


def kpconv(x, xyz, centres, idx, kpts, sigma, dtype=np.float32):
    """The whole forward: ``(out[B, K * C, M], h[B,M,k,K])``."""
    h = influence(xyz, centres, idx, kpts, sigma, dtype)
    return forward(_gathered(x, idx), h), h


def slot_words(h, go, c):
    """``p[B,C,M,k]`` in the dtype of ``h``: ``p = p + (h * grad_out[b, t * c + ch, i])`` over t ascending for the pairs with
    ``h > 0``; +0.0 on a slot that is no point (all its ``h`` are +0.0)."""
    b, m, k, kp = h.shape
    g = go.astype(h.dtype).reshape(b, kp, c, m)
    p = np.zeros((b, c, m, k), dtype=h.dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        for t in range(kp):
            ht = h[:, None, :, :, t]
            p = np.where(ht > 0, p + ht * g[:, t, :, :, None], p)
    assert p.dtype == h.dtype
    return p


class GradX:
    """``grad_x`` as the float64 sum per bin of the words ``p[B,C,M,k]`` along ``idx``: ``gx[B,C,N]``, the in-degree ``deg[B,N]``
    and the absolute sum ``gx_abs`` of the words that reach a bin."""

    def __init__(self, idx, p, n):
        b, c, m, k = p.shape
        valid = valid_slots(idx, n)
        self.gx, self.gx_abs = np.zeros((b, c, n)), np.zeros((b, c, n))
        self.deg = np.zeros((b, n), dtype=np.int64)
        for bi in range(b):
            ok = valid[bi].reshape(-1)
            t = idx[bi].reshape(-1)[ok]
            words = p[bi].astype(np.float64).reshape(c, m * k)[:, ok]
            np.add.at(self.gx[bi], (slice(None), t), words)
            np.add.at(self.gx_abs[bi], (slice(None), t), np.abs(words))
            np.add.at(self.deg[bi], t, 1)

    def free(self, gx):
        return np.broadcast_to((self.deg == 0)[:, None, :], gx.shape)

    def check_exact(self, gx):
        """Lattice geometry and integer gradients: every word and partial sum is exact, so the words are those of the float64
        sums; a point nothing refers to is +0.0."""
        assert gx.dtype == np.float32 and np.array_equal(gx, self.gx.astype(np.float32))
        assert (gx.view(np.uint32)[self.free(gx)] == 0).all()

    def ratio(self, gx):
        """The largest ``|got - sum64 p|`` over its bound ``gamma(deg) * sum |p|`` -- a float32 sum of deg exact words in any
        order; where the bound is 0 the error must be.  A point nothing refers to is the word 0."""
        assert gx.dtype == np.float32 and np.isfinite(gx).all()
        assert (gx.view(np.uint32)[self.free(gx)] == 0).all()
        err, bound = np.abs(gx - self.gx), gamma(self.deg)[:, None, :] * self.gx_abs
        assert (err[bound == 0] == 0).all()
        return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
