"""numpy reference of the interpolation op (``pcc_interpolate`` / ``pcc_interpolate_bwd``, include/pcc_neighbour.h) for
tests/test_interpolate_host.py and tests/test_gpu_interpolate.py.

The forward is the contract's float32 loop over the k slots: ``acc = acc + (w * x)``, numpy's float32 multiplication and
addition (two roundings per slot, what the kernel does); a slot whose index is outside [0, n) is skipped, and a NaN result
is the word 0x7fc00000.  ``grad_w`` is the same kind of loop over the channels.  ``grad_x`` is float64, together with what
the summation bound needs per bin: its in-degree and the sum of the absolute products that reach it."""

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32

# the grid of the forward and backward tests
N_GRID = (1, 3, 63, 64, 65, 1025)
M_GRID = (1, 3, 65, 257)
K_GRID = (1, 3, 4, 5)
C_GRID = (1, 3, 8, 9)
B_MAX, C_MAX = 3, 9
# n on both sides of every boundary of the dispatch: the channel block 8 -> 4 -> 2 -> 1 (64 KB of rows), one row of 160 KB
BOUNDARIES = (2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 40960, 40961)
NAN_WORD = np.uint32(0x7fc00000)


def grid():
    """(m, k, c, b, out_c0, j): the full product of the first three; b in {1, 3} and out_c0 in {0, 1, 3} rotate with the
    running number j, so that every value of either meets every m, k and c."""
    j = 0
    for m in M_GRID:
        for k in K_GRID:
            for c in C_GRID:
                yield m, k, c, (1, 3)[j % 2], (0, 1, 3)[j % 3], j
                j += 1


def gamma(d):
    """The bound of a float32 sum of d terms in any order: |computed - exact| <= gamma(d) * sum |terms|."""
    d = np.asarray(d, dtype=np.float64)
    return d * U / (1.0 - d * U)


def cloud(seed, n, b=B_MAX, c=C_MAX):
    """Gaussian values ``x[b,c,n]`` float32; the first three channels double as coordinates."""
    return np.random.default_rng(seed).standard_normal((b, c, n)).astype(np.float32)


def random_list(seed, b, n, m, k, bad=True):
    """Uniform indices; with ``bad`` about a tenth of the slots hold -1, n or 2^40 (at least one of each when b*m*k >= 3)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, size=(b, m, k), dtype=np.int64)
    if bad:
        flat = idx.reshape(-1)
        pos = rng.permutation(flat.size)[:max(3, flat.size // 10)]
        flat[pos] = np.resize(np.array([-1, n, 1 << 40], dtype=np.int64), pos.size)
    return idx


def gaussian_weights(seed, b, m, k):
    return np.random.default_rng(seed).standard_normal((b, m, k)).astype(np.float32)


def dyadic_weights(seed, b, m, k):
    """Weights from {0, +-1/2, +-1, +-2}: their products with small integers and every sum of those are exact."""
    return np.random.default_rng(seed).choice(np.array([0, .5, -.5, 1, -1, 2, -2], dtype=np.float32), size=(b, m, k))


def _gathered(x, idx):
    """``(valid[B,M,k], x[b, :, idx] as [B,C,M,k])`` with index 0 in place of an out-of-range one."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    valid = (idx >= 0) & (idx < n)
    safe = np.where(valid, idx, 0).reshape(b, 1, m * k)
    return valid, np.take_along_axis(x, np.broadcast_to(safe, (b, c, m * k)), axis=2).reshape(b, c, m, k)


def forward(x, idx, w):
    """``out[B,C,M]`` float32 of ``x[B,C,N]`` float32 along ``idx[B,M,k]`` with ``w[B,M,k]``; compare through
    ``.view(np.uint32)``."""
    valid, xg = _gathered(x, idx)
    acc = np.zeros(xg.shape[:3], dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(idx.shape[2]):
            term = (w[:, None, :, j] * xg[:, :, :, j]).astype(np.float32)
            acc = np.where(valid[:, None, :, j], (acc + term).astype(np.float32), acc)
    words = acc.view(np.uint32).copy()
    words[np.isnan(acc)] = NAN_WORD
    return words.view(np.float32)


def grad_w(x, idx, g):
    """``grad_w[B,M,k]`` float32: ``acc = acc + (g[b,ch,i] * x[b,ch,idx])`` for ch ascending; +0.0 for an out-of-range slot."""
    valid, xg = _gathered(x, idx)
    acc = np.zeros(idx.shape, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for ch in range(x.shape[1]):
            term = (g[:, ch, :, None] * xg[:, ch]).astype(np.float32)
            acc = (acc + term).astype(np.float32)
    return np.where(valid, acc, np.float32(0))


class GradX:
    """Float64 ``grad_x`` of ``g[B,C,M]`` along ``idx`` with ``w``: ``gx[B,C,N]`` and, per bin, the in-degree (``deg[B,N]``)
    and the absolute sum ``gx_abs`` of the products that reach it."""

    def __init__(self, idx, w, g, n):
        b, c, m = g.shape
        k = idx.shape[2]
        valid = (idx >= 0) & (idx < n)
        self.gx, self.gx_abs = np.zeros((b, c, n)), np.zeros((b, c, n))
        self.deg = np.zeros((b, n), dtype=np.int64)
        for bi in range(b):
            ok = valid[bi].reshape(-1)
            t = idx[bi].reshape(-1)[ok]
            prod = (w[bi].astype(np.float64)[None] * g[bi].astype(np.float64)[:, :, None]).reshape(c, m * k)[:, ok]
            np.add.at(self.gx[bi], (slice(None), t), prod)
            np.add.at(self.gx_abs[bi], (slice(None), t), np.abs(prod))
            np.add.at(self.deg[bi], t, 1)

    def check_exact(self, gx):
        """Integer gradients and dyadic weights: every product and partial sum is exact, so the words are those of the
        float64 sums; a point nothing refers to is +0.0."""
        assert np.array_equal(gx, self.gx.astype(np.float32))
        free = np.broadcast_to((self.deg == 0)[:, None, :], gx.shape)
        assert (gx.view(np.uint32)[free] == 0).all()

    def ratio(self, gx):
        """The largest |got - ref64| over its bound gamma(deg + 1) * sum |w g| (one rounding per product and a sum of deg
        terms in any order); 0 where the bound is 0 and met."""
        assert np.isfinite(gx).all()
        err, bound = np.abs(gx - self.gx), gamma(self.deg + 1)[:, None, :] * self.gx_abs
        assert (err[bound == 0] == 0).all()
        return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0

    def check_bound(self, gx):
        """|got - ref64| <= gamma(deg + 1) * sum |w g| per bin."""
        assert self.ratio(gx) <= 1.0


def hand_propagation(features, skip, idx, weights):
    """What ``feature_propagation`` computes on the list ``idx`` with ``weights``, written by hand: [B,C+C2,M] float32."""
    out = forward(features, idx, weights)
    return out if skip is None else np.concatenate([out, skip], axis=1)
