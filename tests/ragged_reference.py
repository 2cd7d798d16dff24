"""References of the searches over packed (ragged) batches and of the ``pointops`` drop-in, for tests/test_ragged_search_host.py,
tests/test_gpu_ragged_search.py, tests/test_pointops_host.py and tests/test_gpu_pointops.py.  Nothing here calls the code under
test.

A packed batch is ``xyz[n,3]`` with ``offset[B]``, the cumulative ends of its clouds; the queries are packed the same way.  Rows
behind the last offset belong to no cloud.

k-NN indices come, cloud by cloud, from the one-cloud C oracle exactly as tests/test_gpu_knn_cross.py::_expected takes them: the
oracle searches ``z = cat([x_b, q_b])``, row ``n_b + i`` is query ``i`` against all of ``z`` in the library's own rounding (a real
``fmaf``) ordered by (distance, index), the entries ``>= n_b`` are dropped, the first ``k`` taken, ``lo_b`` added and -1 put
behind.  So indices are compared word for word on every input.  (The oracle is asked for ``k + m_b`` entries per row, not
``n_b + m_b``: at most ``m_b`` entries of a row are queries, so the first ``k`` candidates are among them.)  The oracle's ``qsort``
has no place for a NaN, so what the contract says about them is applied around it: a point with a NaN coordinate is taken out
of the cloud before the oracle runs (a NaN distance is never listed), and the row of a query with a non-finite coordinate --
every distance +inf or NaN -- is written down directly: the candidates at +inf in index order.

Distances: a padded slot is +inf exactly; a real slot is within ``c + 2 = 5`` float32 ulp of the float64 value (the bound of
``_check_diff_dist`` there) and rows do not decrease.

Ball query: tests/ball_query_reference.BallReference per cloud, its exact mode on lattice clouds and its margin mode, with its own
1 % cap of ambiguous queries taken over the packed batch, on generic ones.

Drop-in: numpy loops of ``grouping`` and ``interpolation`` on packed arrays."""

import numpy as np

from tests.ball_query_reference import MAX_AMBIGUOUS_SHARE, BallReference

KMAX = 32


def pack(clouds):
    """``(xyz[n,3] float32, offset[B] int64)`` of a list of ``[n_b,3]`` arrays."""
    xyz = np.concatenate([np.asarray(c, np.float32).reshape(-1, 3) for c in clouds], 0) if clouds else np.zeros((0, 3), np.float32)
    return np.ascontiguousarray(xyz), np.cumsum([len(c) for c in clouds]).astype(np.int64)


KINDS = ('lattice4', 'lattice16', 'gauss', 'gauss_x100', 'gauss_x1e-3', 'gauss_+50')


def cloud(seed, n, kind):
    """``[n,3]`` float32: points drawn with repetition from the 4^3 or 16^3 lattice of coordinates k/16 (exact distances,
    exact ties, coincident points), or N(0, 1), scaled by 100 or 1e-3 or translated by +50."""
    rng = np.random.default_rng(seed)
    if kind.startswith('lattice'):
        levels = int(kind[7:])
        return (rng.integers(0, levels, (n, 3)) * (16 // levels) / 16.0).astype(np.float32)
    base = rng.standard_normal((n, 3))
    scale = 100.0 if kind.endswith('x100') else 1e-3 if kind.endswith('x1e-3') else 1.0
    return (base * scale + (50.0 if kind.endswith('+50') else 0.0)).astype(np.float32)


def batch(seed, sizes, kind, extra=0):
    """``pack`` of ``cloud(seed + b, sizes[b], kind)``, with ``extra`` more rows behind the last offset (of no cloud)."""
    xyz, offset = pack([cloud(seed + b, s, kind) for b, s in enumerate(sizes)])
    return np.ascontiguousarray(np.concatenate([xyz, cloud(seed + len(sizes), extra, kind)], 0)), offset


def ranges(offset):
    """``[(lo_b, hi_b)]`` of valid offsets."""
    ends = [0] + [int(v) for v in offset]
    assert all(hi >= lo for lo, hi in zip(ends[:-1], ends[1:]))
    return list(zip(ends[:-1], ends[1:]))


def _cloud_knn(oracle, x, q, k, self_search):
    """Local ``idx[m_b,k]`` (-1 behind) of the queries ``q[m_b,3]`` in the cloud ``x[n_b,3]``."""
    n, m = len(x), len(q)
    out = np.full((m, k), -1, np.int64)
    keep = np.nonzero(~np.isnan(x).any(1))[0]  # a NaN point is never listed
    xc = x[keep]
    finite_q = np.isfinite(q).all(1)
    with np.errstate(invalid='ignore', over='ignore'):
        for i in np.nonzero(~finite_q)[0]:  # every distance +inf or NaN, whatever the rounding
            df = xc - q[i]
            inf = np.nonzero(np.isposinf((df * df).sum(1)))[0][:k]
            out[i, :len(inf)] = keep[inf]
    rows = np.nonzero(finite_q)[0]
    if len(xc) == 0 or len(rows) == 0:
        return out
    kk = min(k, len(xc))
    if self_search and len(keep) == n and finite_q.all():
        got = oracle.knn_diff(np.ascontiguousarray(x.T)[None], kk)[0]  # pcc_knn_cross(x, x) is pcc_knn(x): the oracle's own rows
    else:
        z = np.ascontiguousarray(np.concatenate([xc, q[rows]], 0).T)[None]
        full = oracle.knn_diff(z, min(len(xc) + len(rows), kk + len(rows)))[0, len(xc):]
        got = np.stack([r[r < len(xc)][:kk] for r in full])
    out[rows, :kk] = keep[got]
    return out


def knn(oracle, xyz, offset, query=None, query_offset=None, k=KMAX):
    """Global ``idx[m,k]`` int64 of the contract; ``idx[:, :k']`` is the answer for every ``k' <= k``."""
    self_search = query is None
    if self_search:
        query, query_offset = xyz, offset
    out = np.full((len(query), k), -1, np.int64)
    for (lo, hi), (qlo, qhi) in zip(ranges(offset), ranges(query_offset)):
        if hi > lo and qhi > qlo:
            local = _cloud_knn(oracle, xyz[lo:hi], query[qlo:qhi], k, self_search)
            out[qlo:qhi] = np.where(local >= 0, local + lo, -1)
    return out


def check_knn_dist(xyz, query, idx, dist):
    """``dist[m,k]`` of the returned ``idx[m,k]``: +inf exactly in a padded slot, within 5 float32 ulp of the float64 distance
    in a real one, rows non-decreasing, no negative zero."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    assert dist.dtype == np.float32 and idx.shape == dist.shape
    real = idx >= 0
    assert np.isposinf(dist[~real]).all()
    with np.errstate(invalid='ignore', over='ignore'):
        df = xyz[np.where(real, idx, 0)].astype(np.float64) - query[:, None, :].astype(np.float64)
        d64 = (df * df).sum(-1)
        ulp = np.spacing(np.maximum(np.minimum(d64, np.finfo(np.float32).max), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)
        fin = real & np.isfinite(d64) & (d64 <= np.finfo(np.float32).max)
        assert (np.abs(dist.astype(np.float64) - d64)[fin] <= 5 * ulp[fin]).all()
        assert np.isposinf(dist[real & ~fin]).all()  # (a real slot is never NaN: +inf is listed, NaN is not)
        assert (dist[:, 1:] >= dist[:, :-1]).all()
    assert not (np.signbit(dist) & (dist == 0)).any()


class RaggedBall:
    """``BallReference`` of every cloud of a packed batch that has points and centres."""

    def __init__(self, xyz, offset, centres, centre_offset):
        self.n, self.m = len(xyz), len(centres)
        self.parts = []
        for (lo, hi), (qlo, qhi) in zip(ranges(offset), ranges(centre_offset)):
            if hi > lo and qhi > qlo:
                self.parts.append((lo, qlo, qhi, BallReference(xyz[None, lo:hi], centres[None, qlo:qhi])))

    def query(self, radius, nsample, pad):
        """``(idx[m,nsample] int64 global, cnt[m] int32)``: a row of no cloud or of a cloud without points is -1 / 0."""
        idx, cnt = np.full((self.m, nsample), -1, np.int64), np.zeros(self.m, np.int32)
        for lo, qlo, qhi, ref in self.parts:
            i, c = ref.query(radius, nsample, pad)
            idx[qlo:qhi], cnt[qlo:qhi] = np.where(i[0] >= 0, i[0] + lo, -1), c[0]
        return idx, cnt

    def check_exact(self, radius, nsample, pad, idx, cnt):
        ref_idx, ref_cnt = self.query(radius, nsample, pad)
        idx, cnt = np.asarray(idx), np.asarray(cnt)
        assert idx.dtype == np.int64 and cnt.dtype == np.int32
        assert np.array_equal(cnt, ref_cnt), ('cnt', radius, nsample, pad)
        assert np.array_equal(idx, ref_idx), ('idx', radius, nsample, pad)

    def check_margin(self, radius, nsample, pad, idx, cnt):
        """``BallReference.check_margin`` over the packed batch: rows without an ambiguous pair word for word, the others for
        validity; the cap of ambiguous rows is taken over all rows.  -> the number of ambiguous rows."""
        ref_idx, ref_cnt = self.query(radius, nsample, pad)
        idx, cnt = np.asarray(idx), np.asarray(cnt)
        assert idx.dtype == np.int64 and cnt.dtype == np.int32 and idx.shape == ref_idx.shape and cnt.shape == ref_cnt.shape
        amb = np.zeros(self.m, bool)
        for lo, qlo, qhi, ref in self.parts:
            ref._membership(radius)
            amb[qlo:qhi] = ref.ambiguous[0].any(-1)
            for qi in np.nonzero(amb[qlo:qhi])[0]:
                c = int(cnt[qlo + qi])
                assert 0 <= c <= nsample
                got = idx[qlo + qi, :c] - lo
                assert (got >= 0).all() and (got < ref.n).all() and (np.diff(got) > 0).all(), (qlo + qi, got)
                assert (ref.inside[0, qi, got] | ref.ambiguous[0, qi, got]).all(), (qlo + qi, 'a returned point is clearly outside')
                sure = np.nonzero(ref.inside[0, qi] & ~ref.ambiguous[0, qi])[0]
                assert np.isin(sure if c < nsample else sure[sure < got[-1]], got).all(), (qlo + qi, 'a clearly inside point is missing')
                fill = (got[0] if c else 0) + lo if pad == 'first' else -1
                assert (idx[qlo + qi, c:] == fill).all(), (qlo + qi, 'padding')
        assert amb.mean() <= MAX_AMBIGUOUS_SHARE, f'mis-specified case: {amb.mean():.3%} of the queries are ambiguous'
        assert np.array_equal(cnt[~amb], ref_cnt[~amb]), ('cnt', radius, nsample, pad)
        assert np.array_equal(idx[~amb], ref_idx[~amb]), ('idx', radius, nsample, pad)
        return int(amb.sum())


# ---- the drop-in ------------------------------------------------------------------------------------------------------------

def grouping(idx, feat, xyz, new_xyz=None, with_xyz=False):
    """``out[m,nsample,(3+)c]`` float32 of the published rule as loops: a -1 slot is a zero row, relative coordinates included;
    the relative coordinates are one float32 subtraction."""
    new_xyz = xyz if new_xyz is None else new_xyz
    m, ns = idx.shape
    c = feat.shape[1]
    out = np.zeros((m, ns, (3 if with_xyz else 0) + c), np.float32)
    for i in range(m):
        for j in range(ns):
            t = int(idx[i, j])
            if t < 0:
                continue
            if with_xyz:
                out[i, j, :3] = xyz[t] - new_xyz[i]
            out[i, j, -c:] = feat[t]
    return out


def grouping_grad(idx, grad, n, with_xyz=False):
    """``grad_feat[n,c]`` float64 of ``grouping`` for the incoming ``grad[m,nsample,(3+)c]``: exact on integer gradients."""
    c = grad.shape[2] - (3 if with_xyz else 0)
    out = np.zeros((n, c))
    for i in range(idx.shape[0]):
        for j in range(idx.shape[1]):
            if idx[i, j] >= 0:
                out[int(idx[i, j])] += grad[i, j, -c:].astype(np.float64)
    return out


def interpolation_weights(idx, xyz, new_xyz):
    """``w[m,k]`` float64: ``1 / (dist + 1e-8)`` over its row sum, ``dist`` the Euclidean distance (float64 of the float32
    inputs), 0 for a -1 slot and for a row of -1 slots.  Exact in float32 where the real slots of a row are equidistant and
    their number is a power of two."""
    m, k = idx.shape
    w = np.zeros((m, k))
    for i in range(m):
        real = idx[i] >= 0
        if real.any():
            d = np.sqrt(((xyz[idx[i, real]].astype(np.float64) - new_xyz[i].astype(np.float64)) ** 2).sum(-1))
            r = 1.0 / (d.astype(np.float32).astype(np.float64) + np.float64(np.float32(1e-8)))
            w[i, real] = r / r.sum()
    return w


def interpolation(idx, w, feat):
    """``new_feat[m,c]`` float64: the weighted sum over the real slots, in slot order."""
    out = np.zeros((idx.shape[0], feat.shape[1]))
    for i in range(idx.shape[0]):
        for j in range(idx.shape[1]):
            if idx[i, j] >= 0:
                out[i] += w[i, j] * feat[int(idx[i, j])].astype(np.float64)
    return out


def interpolation_grad(idx, w, grad, n):
    """``grad_feat[n,c]`` float64 for the incoming ``grad[m,c]``."""
    out = np.zeros((n, grad.shape[1]))
    for i in range(idx.shape[0]):
        for j in range(idx.shape[1]):
            if idx[i, j] >= 0:
                out[int(idx[i, j])] += w[i, j] * grad[i].astype(np.float64)
    return out


def dropin_batch(seed=400, c=5):
    """Lattice clouds of 40, 3 and 17 points with 9, 4 and 6 query points and integer features ``feat[n,c]``: every distance is
    exact, the cloud of 3 runs short of any ``nsample > 3``."""
    xyz, offset = batch(seed, [40, 3, 17], 'lattice4')
    new_xyz, new_offset = batch(seed + 50, [9, 4, 6], 'lattice4')
    feat = np.random.default_rng(seed + 99).integers(-4, 5, (len(xyz), c)).astype(np.float32)
    return xyz, offset, new_xyz, new_offset, feat


def dyadic_interpolation_batch(seed=500, c=6):
    """Geometry on which the interpolation weights are dyadic for ``k <= 2`` (and for ``k = 3`` in the last two clouds, whose
    third slot is padding): cloud 0 is the 8 corners of a cube of side 1/2, queried at its 12 edge midpoints, its 6 face centres
    and its centre -- the two nearest corners (ties: the lowest indices) are equidistant; cloud 1 is two points queried on their
    bisecting plane; cloud 2 is one point.  Integer features."""
    corners = np.array([[x, y, z] for x in (0, .5) for y in (0, .5) for z in (0, .5)], np.float32)
    mids = [(corners[a] + corners[b]) / 2 for a in range(8) for b in range(a + 1, 8) if np.abs(corners[a] - corners[b]).sum() == .5]
    faces = [[.25, .25, 0], [.25, .25, .5], [.25, 0, .25], [.25, .5, .25], [0, .25, .25], [.5, .25, .25]]
    q0 = np.array(mids + faces + [[.25, .25, .25]], np.float32)
    two, q1 = np.array([[0, 0, 0], [.5, 0, 0]], np.float32), np.array([[.25, 0, 0], [.25, .5, .25], [.25, -1, 2]], np.float32)
    one, q2 = np.array([[1, 1, 1]], np.float32), np.array([[1, 1, 1], [0, .5, 2]], np.float32)
    xyz, offset = pack([corners, two, one])
    new_xyz, new_offset = pack([q0, q1, q2])
    feat = np.random.default_rng(seed).integers(-4, 5, (len(xyz), c)).astype(np.float32)
    return xyz, offset, new_xyz, new_offset, feat
