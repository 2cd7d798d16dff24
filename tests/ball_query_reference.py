"""Float64 reference of the ball query for tests/test_gpu_ball_query.py and tests/test_ball_query_host.py: the rule of
``pcc_ball_query`` (include/pcc_neighbour.h) in numpy -- float64 distances of the float32 inputs, ``r2`` the float32 product
``radius * radius``, the first ``nsample`` inside points in index order, count and padding -- and the two ways a result is
compared with it.  Nothing here calls the code under test.

Exact mode (lattice clouds, coordinates k/16 or k/32): every difference, square and sum is exact in float32, so the float64
answer is the float32 answer and ``idx`` / ``cnt`` must match word for word, points exactly on the sphere (outside) included.

Margin mode (generic clouds): a (query, candidate) pair is *ambiguous* when ``|d64 - r2| <= r2 * 2**-20``.  The float32
distance carries at most five roundings on non-negative terms (three differences, each squared, two additions: relative
error at most 5 * 2**-24 < 2**-20, the bound of ``fps_reference.check_validity``), so the float32 code can disagree with
float64 about membership for an ambiguous pair only.  A query without an ambiguous pair must match word for word; one with
an ambiguous pair is checked for validity; more than 1 % ambiguous queries fail the case as mis-specified."""

import numpy as np

MARGIN = 2.0 ** -20
MAX_AMBIGUOUS_SHARE = 0.01

GENERIC_KINDS = ('uniform', 'gauss', 'gauss_x100', 'uniform_x1e-3', 'gauss_+50')
GENERIC_SHAPES = ((2, 300, 300, 0.3), (3, 2048, 512, 0.2), (2, 4100, 1000, 0.1))  # (B, N, M, radius at unit scale)


def generic_cloud(seed, b, n, kind):
    """``(xyz[b,n,3] float32, scale)``: uniform in [-1,1]^3 or N(0, 0.5^2), scaled by 100 or 1e-3 (``scale``: what a radius
    meant for the unit-scale cloud is multiplied by) or translated by +50."""
    rng = np.random.default_rng(seed)
    base = rng.random((b, n, 3)) * 2.0 - 1.0 if kind.startswith('uniform') else rng.standard_normal((b, n, 3)) * 0.5
    scale = 1.0
    if kind.endswith('x100'):
        scale = 100.0
    elif kind.endswith('x1e-3'):
        scale = 1e-3
    base = base * scale
    if kind.endswith('+50'):
        base = base + 50.0
    return base.astype(np.float32), scale


def between_lattice(seed, b, m):
    """``[b,m,3]`` float32 centres between the points of the k/16 lattice: odd multiples of 1/32 in (0, 1).  Differences to
    lattice points are multiples of 1/32, so the distances stay exact in float32."""
    k = np.random.default_rng(seed).integers(0, 16, (b, m, 3)) * 2 + 1
    return (k / 32.0).astype(np.float32)


class BallReference:
    """The float64 distances of ``centres[b,m,3]`` to ``xyz[b,n,3]`` (float32 inputs), computed once; ``query`` applies the
    selection rule for one (radius, nsample, pad)."""

    def __init__(self, xyz, centres):
        x, c = np.asarray(xyz), np.asarray(centres)
        assert x.dtype == np.float32 and c.dtype == np.float32 and x.shape[0] == c.shape[0]
        self.b, self.n, self.m = x.shape[0], x.shape[1], c.shape[1]
        with np.errstate(invalid='ignore', over='ignore'):
            self.d = np.zeros((self.b, self.m, self.n))
            for k in range(3):  # coordinate order 0, 1, 2
                df = x[:, None, :, k].astype(np.float64) - c[:, :, None, k].astype(np.float64)
                self.d += df * df
        self._radius = None

    def _membership(self, radius):
        if self._radius is None or self._radius != radius:
            with np.errstate(over='ignore', invalid='ignore'):
                r2 = np.float64(np.float32(radius) * np.float32(radius))
                self.inside = self.d < r2  # (false for a NaN distance)
                self.ambiguous = (np.abs(self.d - r2) <= r2 * MARGIN) if np.isfinite(r2) else np.zeros_like(self.inside)
            self.rank = self.inside.cumsum(-1, dtype=np.int64)
            self._radius = radius

    def query(self, radius, nsample, pad):
        """``(idx[b,m,nsample] int64, cnt[b,m] int32)`` of the header's rule; ``pad`` is 'first' or 'none'."""
        self._membership(radius)
        idx = np.zeros((self.b, self.m, nsample), np.int64)
        bb, ii, jj = np.nonzero(self.inside & (self.rank <= nsample))
        idx[bb, ii, self.rank[bb, ii, jj] - 1] = jj
        cnt = np.minimum(self.rank[..., -1], nsample).astype(np.int32)
        fill = idx[..., :1] if pad == 'first' else np.int64(-1)  # (idx[..., 0] is 0 for an empty ball)
        return np.where(np.arange(nsample) < cnt[..., None], idx, fill), cnt

    def check_exact(self, radius, nsample, pad, idx, cnt, rows=slice(None)):
        """Word for word; ``rows`` selects the clouds of the reference that ``idx`` / ``cnt`` were computed for."""
        ref_idx, ref_cnt = self.query(radius, nsample, pad)
        idx, cnt = np.asarray(idx), np.asarray(cnt)
        assert idx.dtype == np.int64 and cnt.dtype == np.int32
        assert np.array_equal(cnt, ref_cnt[rows]), ('cnt', radius, nsample, pad)
        assert np.array_equal(idx, ref_idx[rows]), ('idx', radius, nsample, pad)

    def ambiguous_share(self, radius):
        self._membership(radius)
        return self.ambiguous.any(-1).mean()

    def check_margin(self, radius, nsample, pad, idx, cnt):
        """Margin mode.  Returns the number of ambiguous queries (each checked for validity only)."""
        ref_idx, ref_cnt = self.query(radius, nsample, pad)
        idx, cnt = np.asarray(idx), np.asarray(cnt)
        assert idx.dtype == np.int64 and cnt.dtype == np.int32
        assert idx.shape == ref_idx.shape and cnt.shape == ref_cnt.shape
        amb_rows = self.ambiguous.any(-1)
        assert amb_rows.mean() <= MAX_AMBIGUOUS_SHARE, f'mis-specified case: {amb_rows.mean():.3%} of the queries are ambiguous'
        clear = ~amb_rows
        assert np.array_equal(cnt[clear], ref_cnt[clear]), ('cnt', radius, nsample, pad)
        assert np.array_equal(idx[clear], ref_idx[clear]), ('idx', radius, nsample, pad)
        for bi, qi in zip(*np.nonzero(amb_rows)):
            c = int(cnt[bi, qi])
            assert 0 <= c <= nsample
            got = idx[bi, qi, :c]
            assert (got >= 0).all() and (got < self.n).all() and (np.diff(got) > 0).all(), (bi, qi, got)
            assert (self.inside[bi, qi, got] | self.ambiguous[bi, qi, got]).all(), (bi, qi, 'a returned point is clearly outside')
            sure = np.nonzero(self.inside[bi, qi] & ~self.ambiguous[bi, qi])[0]
            if c < nsample:  # the list is not full: the whole cloud was scanned
                assert np.isin(sure, got).all(), (bi, qi, 'a clearly inside point is missing')
            else:
                assert np.isin(sure[sure < got[-1]], got).all(), (bi, qi, 'a clearly inside point below the last one is missing')
            fill = (got[0] if c else 0) if pad == 'first' else -1
            assert (idx[bi, qi, c:] == fill).all(), (bi, qi, 'padding')
        return int(amb_rows.sum())


# The kernel variants of pcc_ball_query (include/pcc_test_hooks.h, ball_path): value -> exact
# launch-profile name.  1, 2: candidates from global memory, 4 / 16 queries (one wave each) per workgroup; 3, 4: candidates
# staged through LDS, 4 queries x tiles of 1024 / 16 queries x tiles of 4096.  Every size takes PRODUCT.
VARIANTS = {1: 'ball_direct_kernel<4>', 2: 'ball_direct_kernel<16>', 3: 'ball_lds_kernel<4,1024>', 4: 'ball_lds_kernel<16,4096>'}
PRODUCT = 4


def kernel_of(forced=0):
    return VARIANTS[forced or PRODUCT]
