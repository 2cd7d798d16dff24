"""numpy reference of the vector-attention ops (``pcc_neighbour_softmax`` / ``_bwd``, ``pcc_aggregate_points`` / ``_bwd``,
include/pcc_neighbour.h) for tests/test_attention_host.py and tests/test_gpu_attention.py.

Where the contract fixes the words the reference is its float32 loop: numpy's float32 multiplication and addition, one
rounding each, over the slots (the forward, ``d`` of the softmax backward) or over the channels of a group (``grad_w``); a
slot whose index is outside [0, n) is skipped, and a NaN result is the word 0x7fc00000.  The softmax itself is float64 with
the bar the tests hold the float32 results to, and ``grad_x`` is float64 with every bin's in-degree and the sum of the
absolute products that reach it (the ``GradX`` of tests/interpolate_reference.py)."""

import numpy as np

from tests.interpolate_reference import NAN_WORD, U, GradX, cloud, gamma, random_list  # noqa: F401

# the grids of the forward and backward tests
N_GRID = (1, 3, 63, 64, 65, 1025)
M_GRID = (1, 3, 65, 257)
K_GRID = (1, 3, 4, 5, 16, 17, 64, 128)
CG_GRID = ((1, 1), (3, 3), (8, 1), (8, 2), (9, 3), (16, 2), (18, 2), (24, 3))  # S < 8, S = 8, S > 8, blocks astride a group
B_MAX, C_MAX = 3, 24
# n on both sides of every boundary of the dispatch (the channel block 8 -> 4 -> 2 -> 1, one row of 160 KB)
BOUNDARIES = (2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 40960, 40961)
TINY = 2.0 ** -126


def grid():
    """(m, k, c, g, b, j): every (m, k) with every (c, g); b in {1, 3} rotates with the running number j."""
    j = 0
    for m in M_GRID:
        for k in K_GRID:
            for c, g in CG_GRID:
                yield m, k, c, g, (1, 3)[j % 2], j
                j += 1


def canonical(a):
    """float32 ``a`` with every NaN as the word 0x7fc00000."""
    a = np.asarray(a, dtype=np.float32)
    words = a.view(np.uint32).copy()
    words[np.isnan(a)] = NAN_WORD
    return words.view(np.float32)


def same_words(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32),
                                                 np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def valid_slots(idx, n):
    return (idx >= 0) & (idx < n)


def gaussian(seed, shape, scale=1.0):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def dyadic(seed, shape):
    """Weights from {0, +-1/2, +-1, +-2}: their products with small integers and every sum of those are exact."""
    return np.random.default_rng(seed).choice(np.array([0, .5, -.5, 1, -1, 2, -2], dtype=np.float32), size=shape)


def slot_values(x, idx, rel=None):
    """``(valid[B,M,k], v[B,C,M,k])`` with ``v = x[b,ch,idx] (+ rel)``, one rounded sum; index 0 stands in for a slot that is
    no point."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    valid = valid_slots(idx, n)
    safe = np.where(valid, idx, 0).reshape(b, 1, m * k)
    v = np.take_along_axis(x, np.broadcast_to(safe, (b, c, m * k)), axis=2).reshape(b, c, m, k)
    if rel is not None:
        with np.errstate(invalid='ignore', over='ignore'):
            v = (v + rel).astype(np.float32)
    return valid, v


def per_channel(w, c):
    """``w[B,G,M,k]`` as ``[B,C,M,k]``: channel ch reads group ch // S, S = C // G."""
    return np.repeat(w, c // w.shape[1], axis=1)


# ---- the softmax ---------------------------------------------------------------------------------------------------------


def softmax64(logits, idx, n):
    """float64 softmax over the valid slots: ``(ref[B,G,M,k], dist[B,G,M,k])`` with ``dist = |l - mx|`` (0 where invalid)."""
    valid = np.broadcast_to(valid_slots(idx, n)[:, None], logits.shape)
    l64 = np.where(valid, logits.astype(np.float64), -np.inf)
    mx = l64.max(-1, keepdims=True)
    with np.errstate(invalid='ignore'):
        d = np.where(valid, l64 - mx, -np.inf)
        e = np.where(valid, np.exp(d), 0.0)
    s = e.sum(-1, keepdims=True)
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = np.where(valid, e / s, 0.0)
        dist = np.where(valid & np.isfinite(d), -d, 0.0)
    return ref, dist


def softmax_ratio(got, logits, idx, n):
    """The largest ``|got - ref| / (((k + 8 + 4 |l - mx|) 2^-24) ref + 2^-126)`` over the valid slots of the rows whose valid
    logits hold a finite maximum and no NaN or +inf; the slots that are no point must be the word 0."""
    k = idx.shape[2]
    valid = np.broadcast_to(valid_slots(idx, n)[:, None], logits.shape)
    assert (got.view(np.uint32)[~valid] == 0).all()
    ref, dist = softmax64(logits, idx, n)
    rows_ok = np.isfinite(ref).all(-1, keepdims=True) & valid.any(-1, keepdims=True)
    use = valid & rows_ok
    assert np.isfinite(got[use]).all()
    bar = (k + 8 + 4 * dist) * U * ref + TINY
    return float((np.abs(got.astype(np.float64) - ref)[use] / bar[use]).max()) if use.any() else 0.0


def softmax32(logits, idx, n):
    """The contract in numpy float32 (numpy's exp): what the bar is checked against on the CPU."""
    valid = np.broadcast_to(valid_slots(idx, n)[:, None], logits.shape)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        mx = np.where(valid, logits, -np.inf).max(-1, keepdims=True).astype(np.float32)
        e = np.where(valid, np.exp((logits - mx).astype(np.float32)), np.float32(0)).astype(np.float32)
        s = np.zeros(logits.shape[:3], dtype=np.float32)
        for j in range(idx.shape[2]):
            s = np.where(valid[..., j], (s + e[..., j]).astype(np.float32), s)
        return np.where(valid, canonical((e / s[..., None]).astype(np.float32)), np.float32(0))


def softmax_bwd(attn, idx, n, ga):
    """``grad_logits[B,G,M,k]`` float32: ``d = d + (attn * ga)`` over the valid slots in order, then ``attn * (ga - d)``."""
    valid = np.broadcast_to(valid_slots(idx, n)[:, None], attn.shape)
    d = np.zeros(attn.shape[:3], dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(idx.shape[2]):
            p = (attn[..., j] * ga[..., j]).astype(np.float32)
            d = np.where(valid[..., j], (d + p).astype(np.float32), d)
        diff = (ga - d[..., None]).astype(np.float32)
        return np.where(valid, canonical((attn * diff).astype(np.float32)), np.float32(0))


# ---- the aggregation -----------------------------------------------------------------------------------------------------


def forward(x, idx, w, rel=None):
    """``out[B,C,M]`` float32: ``acc = acc + (w[b,ch // S,i,j] * v)`` over the valid slots in order."""
    valid, v = slot_values(x, idx, rel)
    wc = per_channel(w, x.shape[1])
    acc = np.zeros(v.shape[:3], dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for j in range(idx.shape[2]):
            term = (wc[..., j] * v[..., j]).astype(np.float32)
            acc = np.where(valid[:, None, :, j], (acc + term).astype(np.float32), acc)
    return canonical(acc)


def grad_rel(idx, w, g, n):
    """``grad_rel[B,C,M,k]`` float32: ``w * g[b,ch,i]``, one rounded product; +0.0 at a slot that is no point."""
    valid = valid_slots(idx, n)
    with np.errstate(invalid='ignore', over='ignore'):
        prod = (per_channel(w, g.shape[1]) * g[..., None]).astype(np.float32)
    return np.where(valid[:, None], canonical(prod), np.float32(0))


def grad_w(x, idx, g, groups, rel=None):
    """``grad_w[B,G,M,k]`` float32: ``acc = acc + (g[b,ch,i] * v)`` over the channels of the group in ascending order."""
    valid, v = slot_values(x, idx, rel)
    b, c = x.shape[:2]
    m, k = idx.shape[1:]
    s = c // groups
    v, gg = v.reshape(b, groups, s, m, k), g.reshape(b, groups, s, m)
    acc = np.zeros((b, groups, m, k), dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        for ch in range(s):
            term = (gg[:, :, ch, :, None] * v[:, :, ch]).astype(np.float32)
            acc = (acc + term).astype(np.float32)
    return np.where(valid[:, None], canonical(acc), np.float32(0))


class GroupedGradX:
    """Float64 ``grad_x`` of ``g[B,C,M]`` along ``idx`` with ``w[B,G,M,k]``: one ``GradX`` (tests/interpolate_reference.py) per
    group over the group's channels -- ``gx``, the absolute sums and the in-degree, with its exact check and its bound
    ``gamma(deg + 1) * sum |w g|`` per bin."""

    def __init__(self, idx, w, g, n):
        b, c, _ = g.shape
        self.s = c // w.shape[1]
        self.parts = [GradX(idx, np.ascontiguousarray(w[:, gi]), np.ascontiguousarray(g[:, gi * self.s:(gi + 1) * self.s]), n)
                      for gi in range(w.shape[1])]
        self.gx = np.concatenate([p.gx for p in self.parts], axis=1)
        self.deg = self.parts[0].deg

    def _slices(self, gx):
        return [(p, np.ascontiguousarray(gx[:, gi * self.s:(gi + 1) * self.s])) for gi, p in enumerate(self.parts)]

    def check_exact(self, gx):
        for p, part in self._slices(gx):
            p.check_exact(part)

    def ratio(self, gx):
        return max(p.ratio(part) for p, part in self._slices(gx))

    def check_bound(self, gx):
        assert self.ratio(gx) <= 1.0


# ---- which kernels a call runs (include/pcc_test_hooks.h, interp_path), as exact launch-profile names ----
TILE_WORDS = 1024 + 512  # words of LDS per channel the forward stages its tile of list rows in, beside the rows of x


def fwd_kernel(b, c, n, forced=0):
    from tests.list_plan_reference import kernel_of

    return kernel_of('agg_fwd_kernel', b, c, n, forced, tile_words=TILE_WORDS)


def bwd_kernels(b, c, n, want, cus, forced=0):
    """The kernels of ``pcc_aggregate_points_bwd`` for ``want = (grad_x, grad_w, grad_rel)`` on a device of ``cus`` compute
    units.  grad_x: the plan of the list ops, its channel block halved while the LDS bins leave compute units idle; grad_rel
    rides along unless those bins tie the launch to fewer workgroups than compute units -- it then, and where grad_x is not
    asked for, takes a launch of the direct kernel of its own."""
    from tests.list_plan_reference import kernel_of, plan

    names = set()
    if want[0]:
        path, cb = plan(b, c, n, forced, spread_cus=cus)
        names.add(kernel_of('agg_bwd_kernel', b, c, n, forced, spread_cus=cus))
        if want[2] and path == 'lds' and b * -(-c // cb) < cus:
            names.add('agg_bwd_kernel<direct>')
    elif want[2]:
        names.add('agg_bwd_kernel<direct>')
    if want[1]:
        names.add('agg_bwd_w_kernel')
    return names
