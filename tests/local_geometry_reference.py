"""numpy reference of the local-geometry op (``pcc_local_geometry`` / ``pcc_local_covariance_bwd``,
include/pcc_neighbour.h) for tests/test_local_geometry_host.py and tests/test_gpu_local_geometry.py.

``mean`` and ``cov`` are the contract's float32 loops over the slots (numpy's float32 addition, subtraction, multiplication
and division: one rounding each, what the kernel does), compared through ``.view(np.uint32)``.  The eigen outputs are not
pinned to a formula: they are bounded against float64 ``numpy.linalg.eigh`` of that same float32 ``cov`` (``EigenBars``).
``GradXyz`` is the float64 gradient with, per bin, its in-degree and the absolute sum of its terms for the summation bound
``gamma(deg + 4) * sum |terms|``."""

import numpy as np

from tests.interpolate_reference import gamma, random_list  # noqa: F401  (the bound and the lists of the interpolation op)

U = 2.0 ** -24  # unit roundoff of float32
NAN_WORD = np.uint32(0x7fc00000)

# the grid of the forward and backward tests
M_GRID = (1, 3, 63, 64, 65, 257)
K_GRID = (1, 2, 3, 16, 17, 33)   # 33: a row longer than the 32 slots of a row the kernels hold in LDS at a time
N_GRID = (1, 3, 64, 1025)
B_MAX = 3
# n on both sides of the one boundary the dispatch has in n: the backward's LDS bins hold 8192 points
BOUNDARIES = (8192, 8193)
LDS_MAX_N = 8192  # 12 n bytes of bins in the backward's 96 KB of LDS


def bwd_kernel(n):
    """The exact launch-profile name of pcc_local_covariance_bwd's kernel: LDS bins while a sample's fit, global atomics above."""
    return 'local_covariance_bwd_kernel<lds>' if n <= LDS_MAX_N else 'local_covariance_bwd_kernel<direct>'


def cloud(seed, n, b=B_MAX, scale=1.0, shift=0.0):
    """Gaussian points ``xyz[b,n,3]`` float32."""
    return (np.random.default_rng(seed).standard_normal((b, n, 3)) * scale + shift).astype(np.float32)


def _gathered(xyz, idx):
    """``(valid[B,M,k], xyz[b, idx] as [B,M,k,3])`` with index 0 in place of an out-of-range one."""
    b, n, _ = xyz.shape
    valid = (idx >= 0) & (idx < n)
    safe = np.where(valid, idx, 0)
    return valid, xyz[np.arange(b)[:, None, None], safe]


def canonical(a):
    words = a.view(np.uint32).copy()
    words[np.isnan(a)] = NAN_WORD
    return words.view(np.float32)


def mean_cov(xyz, idx):
    """``(mean[B,M,3], cov[B,M,3,3])`` float32 of ``xyz[B,N,3]`` float32 along ``idx[B,M,k]``; compare through
    ``.view(np.uint32)``."""
    valid, pts = _gathered(xyz, idx)
    b, m, k = idx.shape
    acc = np.zeros((b, m, 3), dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for j in range(k):
            acc = np.where(valid[:, :, j, None], (acc + pts[:, :, j]).astype(np.float32), acc)
        cnt = valid.sum(-1)
        mean = np.where(cnt[:, :, None] > 0, (acc / np.maximum(cnt, 1).astype(np.float32)[:, :, None]).astype(np.float32), np.float32(0))
        cov = np.zeros((b, m, 3, 3), dtype=np.float32)
        for j in range(k):
            d = (pts[:, :, j] - mean).astype(np.float32)
            prod = (d[:, :, :, None] * d[:, :, None, :]).astype(np.float32)
            cov = np.where(valid[:, :, j, None, None], (cov + prod).astype(np.float32), cov)
    return canonical(mean), canonical(cov)


class EigenBars:
    """float64 ``eigh`` of float32 scatter matrices ``cov[...,3,3]`` (rows with a non-finite entry excluded) and the bars of
    the contract on ``(eval, evec, curv)``: ``measure`` returns the four maxima in units of U (the first two relative to
    ``|S|_F``), ``check`` asserts them."""

    BARS = {'residual': 64.0, 'eigenvalue': 64.0, 'orthogonality': 64.0, 'curvature': 16.0}

    def __init__(self, cov):
        self.s = cov.reshape(-1, 3, 3).astype(np.float64)
        self.finite = np.isfinite(self.s).all((1, 2))
        self.lam = np.zeros((self.s.shape[0], 3))
        self.lam[self.finite] = np.linalg.eigvalsh(self.s[self.finite])
        self.fro = np.sqrt((np.where(self.finite[:, None, None], self.s, 0.0) ** 2).sum((1, 2)))

    def measure(self, val, vec, curv):
        ok = self.finite
        val, vec, curv = (a.astype(np.float64) for a in (val.reshape(-1, 3)[ok], vec.reshape(-1, 3, 3)[ok], curv.reshape(-1)[ok]))
        assert np.isfinite(val).all() and np.isfinite(vec).all() and np.isfinite(curv).all()
        s, lam, fro = self.s[ok], self.lam[ok], self.fro[ok]
        res = np.linalg.norm(np.einsum('rab,rib->ria', s, vec) - val[:, :, None] * vec, axis=2).max(1)
        err = np.abs(val - lam).max(1)
        assert (res[fro == 0] == 0).all() and (err[fro == 0] == 0).all()
        pos = fro > 0
        trace = lam.sum(1)
        want_curv = np.where(trace > 0, np.maximum(lam[:, 0], 0) / np.where(trace > 0, trace, 1), 0.0)
        return {'residual': float((res[pos] / fro[pos]).max(initial=0.0)) / U,
                'eigenvalue': float((err[pos] / fro[pos]).max(initial=0.0)) / U,
                'orthogonality': float(np.abs(np.einsum('ria,rja->rij', vec, vec) - np.eye(3)).max(initial=0.0)) / U,
                'curvature': float(np.abs(curv - want_curv).max(initial=0.0)) / U}

    def check(self, val, vec, curv):
        got = self.measure(val, vec, curv)
        for name, bar in self.BARS.items():
            assert got[name] <= bar, (name, got[name], bar)
        return got


def check_conventions(cov, val, vec, curv):
    """What the contract says of the eigen outputs beyond accuracy, on float32 arrays: ascending eigenvalues; the component
    of largest magnitude of every eigenvector non-negative (the lowest axis deciding a tie) and no -0.0; a decoupled axis
    returned as its exact unit vector with the diagonal entry as its eigenvalue; the identity and +0.0 for a zero matrix;
    the word 0x7fc00000 everywhere for a matrix with a non-finite entry."""
    s, val, vec, curv = cov.reshape(-1, 3, 3), val.reshape(-1, 3), vec.reshape(-1, 3, 3), curv.reshape(-1)
    finite = np.isfinite(s).all((1, 2))
    for a in (val[~finite], vec[~finite], curv[~finite]):
        assert (a.view(np.uint32) == NAN_WORD).all()
    s, val, vec, curv = s[finite], val[finite], vec[finite], curv[finite]
    assert (np.diff(val, axis=1) >= 0).all()
    lead = np.take_along_axis(vec, np.abs(vec).argmax(2)[:, :, None], 2)  # (argmax: the first of equal maxima)
    assert (lead > 0).all()
    assert not ((vec == 0) & np.signbit(vec)).any()
    assert ((curv >= 0) & (curv <= np.float32(1 / 3) * (1 + 16 * U))).all()
    zero = (s == 0).all((1, 2))
    assert (val[zero].view(np.uint32) == 0).all() and (curv[zero].view(np.uint32) == 0).all()
    assert (vec[zero].view(np.uint32) == np.eye(3, dtype=np.float32).view(np.uint32)).all()
    for a, (p, q) in enumerate(((1, 2), (0, 2), (0, 1))):
        alone = (s[:, a, p] == 0) & (s[:, a, q] == 0) & ~zero
        unit = np.eye(3, dtype=np.float32)[a]
        hit = (vec[alone] == unit).all(2)  # [rows, 3]: which eigenvector is the axis
        assert (hit.sum(1) >= 1).all()
        r = hit.argmax(1)
        assert np.array_equal(val[alone][np.arange(len(r)), r], s[alone][:, a, a])


class GradXyz:
    """Float64 ``grad_xyz[B,N,3]`` of ``grad_cov[B,M,3,3]`` and ``grad_mean[B,M,3]`` (or None) along ``idx`` on the cloud
    ``xyz`` with the saved float32 ``mean``, on the contract's float32 ``Gs``, ``gm`` and ``d`` (each one rounded operation,
    so they are determined): what is left to the kernel is, per slot, three rounded products and three rounded sums, and
    the float32 sum of a bin's ``deg`` terms in any order.  ``gx_abs`` is the sum of |Gs_a0 d_0| + |Gs_a1 d_1| + |Gs_a2 d_2|
    + |gm_a| over the slots that reach a bin, ``deg[B,N]`` their number."""

    def __init__(self, xyz, idx, mean, grad_cov, grad_mean):
        b, n, _ = xyz.shape
        valid, pts = _gathered(xyz, idx)
        with np.errstate(invalid='ignore', divide='ignore'):
            d = (pts - mean[:, :, None, :]).astype(np.float32).astype(np.float64)               # [B,M,k,3]
            gs = (grad_cov + grad_cov.transpose(0, 1, 3, 2)).astype(np.float32).astype(np.float64)  # [B,M,3,3]
            cnt = valid.sum(-1).astype(np.float32)
            gm = np.zeros(mean.shape) if grad_mean is None else (grad_mean / cnt[:, :, None]).astype(np.float32).astype(np.float64)
        prod = gs[:, :, None, :, :] * d[:, :, :, None, :]                                         # [B,M,k,a,c]
        term = prod.sum(-1) + gm[:, :, None, :]
        mag = np.abs(prod).sum(-1) + np.abs(gm)[:, :, None, :]
        self.gx, self.gx_abs = np.zeros((b, n, 3)), np.zeros((b, n, 3))
        self.deg = np.zeros((b, n), dtype=np.int64)
        for bi in range(b):
            ok = valid[bi]
            t = idx[bi][ok]
            np.add.at(self.gx[bi], t, term[bi][ok])
            np.add.at(self.gx_abs[bi], t, mag[bi][ok])
            np.add.at(self.deg[bi], t, 1)

    def check_exact(self, gx):
        """Integer inputs: every intermediate is exact, so the words are those of the float64 sums; a point nothing refers
        to is +0.0."""
        assert np.array_equal(gx, self.gx.astype(np.float32))
        free = np.broadcast_to((self.deg == 0)[:, :, None], gx.shape)
        assert (gx.view(np.uint32)[free] == 0).all()

    def ratio(self, gx):
        """The largest |got - ref64| over its bound gamma(deg + 4) * sum |terms|; 0 where the bound is 0 and met."""
        assert np.isfinite(gx).all()
        err, bound = np.abs(gx - self.gx), gamma(self.deg + 4)[:, :, None] * self.gx_abs
        assert (err[bound == 0] == 0).all()
        return float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0

    def check_bound(self, gx):
        assert self.ratio(gx) <= 1.0


def exact_backward_inputs(seed, b, n, m, k):
    """Inputs on which every intermediate of the backward is exact in float32: integer coordinates in [-8, 8], rows with
    1, 2, 4 or 8 valid slots (at most k; the other slots -1, n or 2^40), integer ``grad_cov`` in [-4, 4] and ``grad_mean``
    an integer multiple of the row's ``cnt``.  ``(xyz, idx, mean, grad_cov, grad_mean)``; the mean is a multiple of 1/8."""
    rng = np.random.default_rng(seed)
    xyz = rng.integers(-8, 9, size=(b, n, 3)).astype(np.float32)
    idx = rng.integers(0, n, size=(b, m, k), dtype=np.int64)
    choices = np.array([c for c in (1, 2, 4, 8) if c <= k])
    cnt = rng.choice(choices, size=(b, m))
    order = np.argsort(rng.random((b, m, k)), axis=2)  # which slots of a row stay valid: the first cnt of a permutation
    keep = np.zeros((b, m, k), dtype=bool)
    np.put_along_axis(keep, order, np.arange(k)[None, None, :] < cnt[:, :, None], axis=2)
    bad = np.resize(np.array([-1, n, 1 << 40], dtype=np.int64), idx.shape)
    idx = np.where(keep, idx, bad)
    mean, _ = mean_cov(xyz, idx)
    grad_cov = rng.integers(-4, 5, size=(b, m, 3, 3)).astype(np.float32)
    grad_mean = (rng.integers(-4, 5, size=(b, m, 3)) * cnt[:, :, None]).astype(np.float32)
    return xyz, idx, mean, grad_cov, grad_mean


def sphere(seed, n):
    """n points on the unit sphere, float32 ``[n,3]``."""
    p = np.random.default_rng(seed).standard_normal((n, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


def brute_knn(xyz, k):
    """float64 brute-force k nearest neighbours of every point of ``xyz[n,3]`` (itself included): ``[n,k]`` int64."""
    p = xyz.astype(np.float64)
    d = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    return np.argsort(d, axis=1, kind='stable')[:, :k].astype(np.int64)


def accuracy_cases(seed=0):
    """The constructions on which the eigen stage's accuracy is bounded, ``{name: (xyz[1,n,3], idx[1,m,k])}`` with
    n <= 4097: k-NN patches of a sphere (k = 16; also scaled by 1e-3 and shifted by 5), Gaussian random lists with
    k in {2, 3, 4, 5, 17, 33}, a rotated plane, and near-isotropic octahedra."""
    rng = np.random.default_rng(seed)
    cases = {}
    p = sphere(seed + 1, 2049)
    nn = brute_knn(p, 16)[None]
    cases['sphere'] = (p[None], nn)
    cases['sphere * 1e-3'] = ((p * np.float32(1e-3))[None], nn)
    cases['sphere + 5'] = ((p + np.float32(5))[None], nn)
    g = rng.standard_normal((1, 4097, 3)).astype(np.float32)
    for k in (2, 3, 4, 5, 17, 33):
        cases[f'gaussian k={k}'] = (g, rng.integers(0, 4097, size=(1, 1500, k), dtype=np.int64))
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    flat = np.concatenate([rng.standard_normal((2048, 2)), np.zeros((2048, 1))], 1) @ q.T
    cases['rotated plane'] = (flat.astype(np.float32)[None], rng.integers(0, 2048, size=(1, 1500, 16), dtype=np.int64))
    octa = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
    pts = (octa[None] + 1e-4 * rng.standard_normal((600, 6, 3))).reshape(-1, 3).astype(np.float32)
    cases['octahedra'] = (pts[None], np.arange(3600, dtype=np.int64).reshape(1, 600, 6))
    return cases
