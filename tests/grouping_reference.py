"""numpy reference of the grouping op (``pcc_group_points`` / ``pcc_group_points_bwd``, include/pcc_neighbour.h) for
tests/test_grouping_host.py and tests/test_gpu_grouping.py.

The forward works on float32 bit patterns: a gather of uint32 words, and numpy's float32 subtraction in the relative mode
(one IEEE subtraction, what the kernel does); a slot whose index is outside [0, n) is the word 0.  The backward is float64,
together with what the summation bound needs per bin: its in-degree and the sum of the absolute values that reach it.

Everything here takes and returns the channels-major layout ``x[B,C,N]``, ``centre[B,C,M]``; ``to_layout`` turns an array
into what a ``point_major`` call takes and back."""

import numpy as np

U = 2.0 ** -24  # unit roundoff of float32

# the grid of the forward and backward tests
N_GRID = (1, 63, 64, 65, 1025)
M_GRID = (1, 3, 65)
K_GRID = (1, 3, 4, 5, 32, 33)  # m * k % 4 == 0 (the 16-byte stores) and every remainder
C_GRID = (1, 3, 8, 9)
B_MAX, C_MAX = 3, 9
# n on both sides of every boundary of the dispatch: the channel block 8 -> 4 -> 2 -> 1 (64 KB of rows), one row of 160 KB
BOUNDARIES = (2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 40960, 40961)


def grid():
    """(m, k, c, point_major, relative, b, out_c0, j): the full product of the first five; b in {1, 3} and out_c0 in
    {0, 1, 3} rotate with the running number j, so that every value of either meets every m, k, c and mode."""
    j = 0
    for m in M_GRID:
        for k in K_GRID:
            for c in C_GRID:
                for point_major in (False, True):
                    for relative in (False, True):
                        yield m, k, c, point_major, relative, (1, 3)[j % 2], (0, 1, 3)[j % 3], j
                        j += 1


def gamma(d):
    """The bound of a float32 sum of d terms in any order: |computed - exact| <= gamma(d) * sum |terms|."""
    d = np.asarray(d, dtype=np.float64)
    return d * U / (1.0 - d * U)


def to_layout(a, point_major):
    """[B,C,X] <-> [B,X,C] (contiguous) when ``point_major``; the array itself otherwise."""
    return np.ascontiguousarray(a.transpose(0, 2, 1)) if point_major else a


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


def padded_list(seed, b, n, m, k, pad):
    """Rows shaped like ``ball_query``'s: cnt ascending indices, then the first one repeated (``pad='first'``) or -1."""
    rng = np.random.default_rng(seed)
    idx = np.empty((b, m, k), dtype=np.int64)
    for bi in range(b):
        for i in range(m):
            cnt = int(rng.integers(0 if pad == 'none' else 1, min(n, k) + 1))
            row = np.sort(rng.choice(n, size=cnt, replace=False))
            idx[bi, i] = np.concatenate([row, np.full(k - cnt, row[0] if pad == 'first' else -1)])
    return idx


def forward(x, idx, centre=None):
    """``out[B,C,M,k]`` float32 of ``x[B,C,N]`` float32 along ``idx[B,M,k]``; compare through ``.view(np.uint32)``."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    valid = (idx >= 0) & (idx < n)
    safe = np.where(valid, idx, 0).reshape(b, 1, m * k)
    words = np.take_along_axis(x.view(np.uint32), np.broadcast_to(safe, (b, c, m * k)), axis=2).reshape(b, c, m, k)
    if centre is not None:
        with np.errstate(invalid='ignore'):
            words = (words.view(np.float32) - centre[:, :, :, None]).astype(np.float32).view(np.uint32)
    return np.where(valid[:, None], words, np.uint32(0)).astype(np.uint32).view(np.float32)


class Backward:
    """Float64 gradients of ``g[B,C,M,k]`` along ``idx``: ``gx[B,C,N]``, ``gc[B,C,M]`` and, per bin, the in-degree
    (``deg[B,N]``) and the absolute sums ``gx_abs``, ``gc_abs``."""

    def __init__(self, idx, g, n):
        b, c, m, k = g.shape
        g = g.astype(np.float64)
        valid = (idx >= 0) & (idx < n)
        self.valid = valid
        self.gx, self.gx_abs = np.zeros((b, c, n)), np.zeros((b, c, n))
        self.deg = np.zeros((b, n), dtype=np.int64)
        for bi in range(b):
            ok = valid[bi].reshape(-1)
            t = idx[bi].reshape(-1)[ok]
            gb = g[bi].reshape(c, m * k)[:, ok]
            np.add.at(self.gx[bi], (slice(None), t), gb)
            np.add.at(self.gx_abs[bi], (slice(None), t), np.abs(gb))
            np.add.at(self.deg[bi], t, 1)
        masked = np.where(valid[:, None], g, 0.0)
        self.gc, self.gc_abs = -masked.sum(-1), np.abs(masked).sum(-1)
        self.k = k

    def check_exact(self, gx=None, gc=None):
        """Integer-valued gradients: every partial sum is exact, so the words are those of the float64 sums; a point
        nothing refers to is +0.0."""
        if gx is not None:
            assert np.array_equal(gx, self.gx.astype(np.float32))
            free = np.broadcast_to((self.deg == 0)[:, None, :], gx.shape)
            assert (gx.view(np.uint32)[free] == 0).all()
        if gc is not None:
            assert np.array_equal(gc, self.gc.astype(np.float32))

    def check_bound(self, gx=None, gc=None):
        """|got - ref64| <= gamma(deg) * sum |g_e| per bin (gamma(k) for a centre)."""
        if gx is not None:
            assert np.isfinite(gx).all()
            assert (np.abs(gx - self.gx) <= gamma(self.deg)[:, None, :] * self.gx_abs).all()
        if gc is not None:
            assert np.isfinite(gc).all()
            assert (np.abs(gc - self.gc) <= gamma(self.k) * self.gc_abs).all()
