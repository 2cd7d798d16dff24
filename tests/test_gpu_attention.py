"""GPU tests of the vector-attention ops (``pcc_neighbour_softmax`` / ``_bwd`` and ``pcc_aggregate_points`` / ``_bwd`` through
the C ABI, and ``neighbour_ops.neighbour_softmax`` / ``aggregate_points`` / ``attention_aggregate`` / ``vector_attention``)
against the numpy reference of tests/attention_reference.py: the softmax inside its bar against float64 and independent of
the batch, the forward, grad_rel, grad_w and the softmax backward word for word, grad_x word for word on integer gradients
with dyadic weights and inside the float32 summation bound on Gaussian ones, both paths on either side of every boundary
of the dispatch, every subset of the gradients, non-finite input, autograd and the argument checks."""

import itertools

import numpy as np
import pytest
import torch

from tests import attention_reference as ref
from tests.which_ran import ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ('random', 'knn_cross', 'ball_none', 'ball_first')


_PATH = [0]  # the interp_path value in force: every aggregate call below asserts the kernels the plan predicts under it


def _forced(path, fn):
    """``fn()`` under interp_path = ``path``.  ``_fwd`` and ``_bwd`` assert from their launch records that the forced
    variant ran and its sibling did not; a forced LDS path that cannot hold a row (and, forward, its tile) is ignored
    (include/pcc_test_hooks.h): the plan then predicts the direct kernel, the product's choice."""
    from pointcloudcounterfactual_amd import _lib

    with _lib.tuning('interp_path', path):
        _PATH[0] = path
        try:
            return fn()
        finally:
            _PATH[0] = 0


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _nan(shape, dev):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=dev)


def _softmax(idx, logits, n):
    """``pcc_neighbour_softmax`` on device tensors, as numpy; ``attn`` starts as NaN: every element must be written."""
    from pointcloudcounterfactual_amd import _lib

    b, g, m, k = logits.shape
    attn = _nan((b, g, m, k), logits.device)
    _lib.call(_lib.lib.pcc_neighbour_softmax, 'neighbour_softmax', logits.device, b, g, n, m, k, _p(idx), _p(logits), _p(attn))
    return attn.cpu().numpy()


def _softmax_bwd(idx, attn, ga, n):
    from pointcloudcounterfactual_amd import _lib

    b, g, m, k = attn.shape
    gl = _nan((b, g, m, k), attn.device)
    _lib.call(_lib.lib.pcc_neighbour_softmax_bwd, 'neighbour_softmax_bwd', attn.device, b, g, n, m, k, _p(idx), _p(attn), _p(ga), _p(gl))
    return gl.cpu().numpy()


def _fwd(x, idx, w, rel=None):
    from pointcloudcounterfactual_amd import _lib

    b, c, n = x.shape
    g, m, k = w.shape[1:]
    out = _nan((b, c, m), x.device)
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_aggregate_points, 'aggregate_points', x.device, b, c, g, n, m, k, _p(x), _p(idx),
                                     _p(w), _p(rel), _p(out)))
    assert names == ({ref.fwd_kernel(b, c, n, _PATH[0]): 1} if b and m else {}), (n, _PATH[0], names)
    return out.cpu().numpy()


def _bwd(x, idx, w, rel, go, n, want=(True, True, True)):
    """``pcc_aggregate_points_bwd``: ``(grad_x, grad_w, grad_rel)`` as numpy arrays, None where not asked for.  The outputs
    start as NaN: every element must be written."""
    from pointcloudcounterfactual_amd import _lib

    b, c, m = go.shape
    g, k = w.shape[1], w.shape[3]
    dev = go.device
    gx = _nan((b, c, n), dev) if want[0] else None
    gw = _nan((b, g, m, k), dev) if want[1] else None
    gr = _nan((b, c, m, k), dev) if want[2] else None
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_aggregate_points_bwd, 'aggregate_points_bwd', dev, b, c, g, n, m, k, _p(x), _p(idx),
                                     _p(w), _p(rel), _p(go), _p(gx), _p(gw), _p(gr)))
    if b and m:
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        assert set(names) == ref.bwd_kernels(b, c, n, want, cus, _PATH[0]), (n, want, _PATH[0], names)
    return tuple(None if t is None else t.cpu().numpy() for t in (gx, gw, gr))


_LISTS = {}


def _lists(cuda, seed, n, m, k):
    """``{origin: idx[B_MAX,m,k]}`` (made once per key): a random list with -1, n and 2^40 in it, a ``knn_cross`` list from m
    points into a Gaussian cloud of n (where k <= n), and the ``ball_query`` lists around them with ``pad='none'`` and
    ``pad='first'``."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    if (seed, n, m, k) not in _LISTS:
        rng = np.random.default_rng(seed)
        lists = {'random': ref.random_list(seed, ref.B_MAX, n, m, k)}
        xyz = _dev(rng.standard_normal((ref.B_MAX, n, 3)).astype(np.float32), cuda)
        q = _dev(rng.standard_normal((ref.B_MAX, m, 3)).astype(np.float32), cuda)
        if k <= n:
            lists['knn_cross'] = ops.knn_cross(q.transpose(1, 2).contiguous(), xyz.transpose(1, 2).contiguous(), k).cpu().numpy()
        for pad in ('none', 'first'):
            lists['ball_' + pad] = ops.ball_query(xyz, q, 1.2, k, pad=pad).cpu().numpy()
        _LISTS[seed, n, m, k] = lists
    return _LISTS[seed, n, m, k]


def _pick(lists, j):
    """The origin of the list rotates with the running number of the grid, one step further at every (m, k)."""
    kinds = [kind for kind in KINDS if kind in lists]
    kind = kinds[(j + j // len(ref.CG_GRID)) % len(kinds)]
    return kind, lists[kind]


# ---- 1, 2: the softmax -----------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('scale', (1.0, 3.0, 30.0))
def test_softmax_against_float64(cuda, scale):
    """Gaussian logits at the given scale, rows with -inf slots among them, over the grid of m, k and g (n and the origin of
    the list rotate): the slots that are no point and the rows without one are the word 0, and every valid slot is inside
    ``((k + 8 + 4 |l - mx|) 2^-24) ref + 2^-126`` of the float64 softmax."""
    worst = 0.0
    for m, k, c, g, b, j in ref.grid():
        n = ref.N_GRID[(j // len(ref.CG_GRID)) % len(ref.N_GRID)]
        kind, idx = _pick(_lists(cuda, 17 * m + k + n, n, m, k), j)
        idx = idx[:b]
        logits = ref.gaussian(1000 + j, (b, g, m, k), scale)
        logits[:, :, ::3, ::2] = -np.inf  # (k = 1: whole rows of -inf, which are NaN)
        got = _softmax(_dev(idx, cuda), _dev(logits, cuda), n)
        valid = np.broadcast_to(ref.valid_slots(idx, n)[:, None], got.shape)
        dead = valid & np.isneginf(logits) & np.isneginf(np.where(valid, logits, -np.inf).max(-1, keepdims=True))
        assert (got.view(np.uint32)[dead] == ref.NAN_WORD).all(), (m, k, g, kind)
        worst = max(worst, ref.softmax_ratio(got, logits, idx, n))
        assert worst <= 1.0, (m, k, g, n, kind)
    print(f'softmax at scale {scale:g}: the largest error is {worst:.3f} of the bar')


def test_softmax_words_do_not_depend_on_the_batch(cuda):
    """A batch against its samples one by one and against a permuted batch; a prefix of m against the slice of the full m;
    forward and backward."""
    b, g, n, m, k = 5, 3, 40, 300, 17
    idx, logits = ref.random_list(1, b, n, m, k), ref.gaussian(2, (b, g, m, k), 3.0)
    ga = ref.gaussian(3, (b, g, m, k))
    idxd, ld, gad = (_dev(a, cuda) for a in (idx, logits, ga))
    attn = _softmax(idxd, ld, n)
    ad = _dev(attn, cuda)
    gl = _softmax_bwd(idxd, ad, gad, n)
    assert ref.same_words(gl, ref.softmax_bwd(attn, idx, n, ga))
    for i in (0, 2, 4):
        assert ref.same_words(_softmax(idxd[i:i + 1], ld[i:i + 1], n)[0], attn[i])
        assert ref.same_words(_softmax_bwd(idxd[i:i + 1], ad[i:i + 1], gad[i:i + 1], n)[0], gl[i])
    order = [2, 4, 0, 3, 1]
    assert ref.same_words(_softmax(idxd[order].contiguous(), ld[order].contiguous(), n), attn[order])
    for pre in (1, 43, 128):
        cut = lambda t: t[..., :pre, :].contiguous()  # noqa: E731
        assert ref.same_words(_softmax(cut(idxd), cut(ld), n), attn[:, :, :pre])
        assert ref.same_words(_softmax_bwd(cut(idxd), cut(ad), cut(gad), n), gl[:, :, :pre])


# ---- 3, 4: the words the contract fixes --------------------------------------------------------------------------------------


@pytest.mark.parametrize('n', ref.N_GRID)
def test_forward_and_fixed_gradients_word_for_word(cuda, n):
    """Every m, k and (c, g) of the grid, b and the origin of the list rotating: the forward with and without rel, grad_rel
    and grad_w against the float32 loops, the softmax backward on the kernel's own attn; with g = 1 and no rel the forward
    is ``pcc_interpolate``'s words."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    x_all = ref.cloud(n, n, ref.B_MAX, ref.C_MAX)
    for m, k, c, g, b, j in ref.grid():
        kind, idx = _pick(_lists(cuda, 17 * m + k + n, n, m, k), j)
        idx = idx[:b]
        tag = (m, k, c, g, b, kind)
        x = np.ascontiguousarray(x_all[:b, :c])
        w, rel = ref.gaussian(j, (b, g, m, k)), ref.gaussian(j + 1, (b, c, m, k))
        go = ref.gaussian(j + 2, (b, c, m))
        xd, idxd, wd, reld, god = (_dev(a, cuda) for a in (x, idx, w, rel, go))
        plain = _fwd(xd, idxd, wd)
        assert ref.same_words(plain, ref.forward(x, idx, w)), tag
        assert ref.same_words(_fwd(xd, idxd, wd, reld), ref.forward(x, idx, w, rel)), tag
        if g == 1:
            assert ref.same_words(ops.interpolate_points(xd, idxd, wd[:, 0].contiguous()).cpu().numpy(), plain), tag
        with_rel = j % 2 == 0
        _, gw, gr = _bwd(xd, idxd, wd, reld if with_rel else None, god, n, (False, True, True))
        assert ref.same_words(gr, ref.grad_rel(idx, w, go, n)), tag
        assert ref.same_words(gw, ref.grad_w(x, idx, go, g, rel if with_rel else None)), tag
        attn = _softmax(idxd, wd, n)
        assert ref.same_words(_softmax_bwd(idxd, _dev(attn, cuda), _dev(gw, cuda), n), ref.softmax_bwd(attn, idx, n, gw)), tag


def test_long_lists_and_many_blocks(cuda):
    """Units of several passes, lists split over several workgroups and more units than one sample's, on both paths."""
    rng = np.random.default_rng(21)
    for b, c, g, n, m, k in ((2, 16, 2, 300, 5003, 16), (4, 64, 8, 64, 2048, 5), (1, 9, 3, 16385, 4100, 128)):
        x = ref.cloud(22, n, b, c)
        idx, w, wq = ref.random_list(23, b, n, m, k), ref.gaussian(24, (b, g, m, k)), ref.dyadic(25, (b, g, m, k))
        rel = ref.gaussian(26, (b, c, m, k))
        go = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
        want, want_w, want_r = ref.forward(x, idx, w, rel), ref.grad_w(x, idx, go, g, rel), ref.grad_rel(idx, wq, go, n)
        back = ref.GroupedGradX(idx, wq, go, n)
        xd, idxd, wd, wqd, reld, god = (_dev(a, cuda) for a in (x, idx, w, wq, rel, go))
        for path in (1, 2):
            assert ref.same_words(_forced(path, lambda: _fwd(xd, idxd, wd, reld)), want), (n, path)
            gx, gw, gr = _forced(path, lambda: _bwd(xd, idxd, wqd, reld, god, n))
            back.check_exact(gx)
            assert ref.same_words(gw, want_w) and ref.same_words(gr, want_r), (n, path)


# ---- 5: grad_x -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('n', ref.N_GRID)
def test_grad_x_word_for_word(cuda, n):
    """Integer gradients in [-8, 8] and weights from {0, +-1/2, +-1, +-2}: every product and partial sum is exact in any
    order.  The grid of the forward test on both paths; points nothing refers to get the word 0."""
    rng = np.random.default_rng(70 + n)
    for m, k, c, g, b, j in ref.grid():
        kind, idx = _pick(_lists(cuda, 17 * m + k + n, n, m, k), j)
        idx = idx[:b]
        w = ref.dyadic(j, (b, g, m, k))
        go = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
        back = ref.GroupedGradX(idx, w, go, n)
        idxd, wd, god = _dev(idx, cuda), _dev(w, cuda), _dev(go, cuda)
        for path in (1, 2):
            gx, _, _ = _forced(path, lambda: _bwd(None, idxd, wd, None, god, n, (True, False, False)))  # (x may be null)
            back.check_exact(gx)


def test_grad_x_on_generic_gradients_is_inside_the_summation_bound(cuda):
    """Gaussian gradients and weights: |got - ref64| <= gamma(deg + 1) * sum |w g| per bin -- one rounding per product and a
    float32 sum of deg terms in any order (the merged runs are such an order): derived, not tuned."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for n, m, k, c, g, b in ((65, 257, 5, 9, 3, 3), (1025, 257, 16, 8, 2, 2), (300, 300, 3, 3, 3, 2), (2049, 65, 64, 16, 2, 2), (3, 257, 17, 18, 2, 3)):
        lists = {'random': ref.random_list(n, b, n, m, k), 'hub': np.full((b, m, k), n - 1, dtype=np.int64)}
        for kind, idx in lists.items():
            w = ref.gaussian(n + 1, (b, g, m, k))
            go = rng.standard_normal((b, c, m)).astype(np.float32)
            back = ref.GroupedGradX(idx, w, go, n)
            idxd, wd, god = _dev(idx, cuda), _dev(w, cuda), _dev(go, cuda)
            for path in (1, 2):
                gx, _, _ = _forced(path, lambda: _bwd(None, idxd, wd, None, god, n, (True, False, False)))
                worst = max(worst, back.ratio(gx))
                back.check_bound(gx)
                free = np.broadcast_to((back.deg == 0)[:, None, :], gx.shape)
                assert (gx.view(np.uint32)[free] == 0).all()
    print(f'grad_x: the largest error is {worst:.2f} of the bound')


# ---- 6: both paths -----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('n', ref.BOUNDARIES)
def test_every_variant_gives_the_same_words(cuda, n):
    """The LDS path (1) and the direct path (2) forced against the product's choice, and that against the reference, on
    both sides of every step of the channel block and of the LDS -> direct switch; forward and (integer gradients, dyadic
    weights) backward.  Where a row no longer fits beside the forward's tile the forced LDS path is ignored."""
    m, k, b = 65, 3, 2
    x_all = ref.cloud(n, n, b, 18)
    rng = np.random.default_rng(n)
    idx = ref.random_list(n, b, n, m, k)
    idxd = _dev(idx, cuda)
    for c, g in ((9, 3), (3, 3), (8, 2), (18, 2)):
        x = np.ascontiguousarray(x_all[:, :c])
        w, wq, rel = ref.gaussian(n + c, (b, g, m, k)), ref.dyadic(n + c, (b, g, m, k)), ref.gaussian(n + c + 1, (b, c, m, k))
        go = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
        xd, wd, wqd, reld, god = (_dev(a, cuda) for a in (x, w, wq, rel, go))
        want = ref.forward(x, idx, w, rel)
        back, want_w, want_r = ref.GroupedGradX(idx, wq, go, n), ref.grad_w(x, idx, go, g, rel), ref.grad_rel(idx, wq, go, n)
        for path in (0, 1, 2):
            assert ref.same_words(_forced(path, lambda: _fwd(xd, idxd, wd, reld)), want), (c, path)
            gx, gw, gr = _forced(path, lambda: _bwd(xd, idxd, wqd, reld, god, n))
            back.check_exact(gx)
            assert ref.same_words(gw, want_w) and ref.same_words(gr, want_r), (c, path)


# ---- 7: only what is asked for -----------------------------------------------------------------------------------------------


def test_every_subset_of_the_gradients(cuda):
    """Each subset of (grad_x, grad_w, grad_rel) returns what the full call returns, every element written over its NaN; a
    single cloud (grad_rel gets a launch of its own) and batches wide enough for grad_rel to ride in the grad_x launch at
    8, 4 and 2 channels per workgroup (b * c / 8 >= 256 compute units, then halved twice), with rel and without."""
    rng = np.random.default_rng(8)
    for b, c, g, n, m, k in ((1, 9, 3, 500, 300, 5), (40, 64, 8, 33, 70, 4), (24, 64, 2, 33, 20, 3), (10, 64, 64, 33, 20, 3)):
        x = ref.cloud(9, n, b, c)
        idx, wq, rel = ref.random_list(10, b, n, m, k), ref.dyadic(11, (b, g, m, k)), ref.gaussian(12, (b, c, m, k))
        go = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
        xd, idxd, wqd, reld, god = (_dev(a, cuda) for a in (x, idx, wq, rel, go))
        for r, rd in ((rel, reld), (None, None)):
            full = _bwd(xd, idxd, wqd, rd, god, n)
            ref.GroupedGradX(idx, wq, go, n).check_exact(full[0])
            assert ref.same_words(full[1], ref.grad_w(x, idx, go, g, r)) and ref.same_words(full[2], ref.grad_rel(idx, wq, go, n))
            for want in itertools.product((False, True), repeat=3):
                part = _bwd(xd if want[1] else None, idxd, wqd, rd if want[1] else None, god, n, want)  # (x, rel: for grad_w only)
                for asked, got, whole in zip(want, part, full):
                    assert (got is None) == (not asked)
                    assert got is None or ref.same_words(got, whole), want


# ---- 8: non-finite input -----------------------------------------------------------------------------------------------------


def test_non_finite_input(cuda):
    """NaN and +-inf in the logits, the values, the weights and rel: the softmax follows ``torch.softmax`` restricted to the
    valid slots, the aggregation is the reference's words (a NaN result is the word 0x7fc00000), and what sits on a slot
    that is no point changes nothing."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    nan, inf = float('nan'), float('inf')
    idx = torch.tensor([[[0, 1, 2, -1], [0, 1, 2, -1], [0, 1, 2, -1], [0, 1, -1, 7], [-1, 9, -1, 7], [0, 1, 2, -1]]], device=cuda)
    logits = torch.tensor([[[[0.0, nan, 1.0, 5.0], [0.0, inf, 1.0, 5.0], [-inf, -inf, -inf, 0.0], [-inf, 2.0, nan, inf],
                             [1.0, 2.0, 3.0, 4.0], [1.0, -inf, 1.0, nan]]]], device=cuda)
    got = ops.neighbour_softmax(logits, idx, 3).cpu().numpy().view(np.uint32)[0, 0]
    NAN, HALF, ONE = 0x7fc00000, 0x3f000000, 0x3f800000
    assert got.tolist() == [[NAN, NAN, NAN, 0], [NAN, NAN, NAN, 0], [NAN, NAN, NAN, 0], [0, ONE, 0, 0], [0, 0, 0, 0], [HALF, 0, HALF, 0]]
    assert ref.same_words(got.view(np.float32), ops.neighbour_softmax(logits.cpu(), idx.cpu(), 3).numpy()[0, 0])

    n, m, k, c, g, b = 300, 128, 4, 6, 3, 3
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    x = ref.cloud(11, n, b, c)
    x[0, :5, ::7] = special[:, None]
    x[1] = np.nan
    idx, w, rel = ref.random_list(12, b, n, m, k), ref.gaussian(13, (b, g, m, k)), ref.gaussian(14, (b, c, m, k))
    w[0, :, ::5, 1] = special[np.arange(len(range(0, m, 5))) % 4]
    rel[2, :, ::3, 2] = special[np.arange(len(range(0, m, 3))) % 5]
    go = ref.gaussian(15, (b, c, m))
    go[2, 1, ::9] = np.inf
    xd, idxd, god = _dev(x, cuda), _dev(idx, cuda), _dev(go, cuda)
    bad = ~ref.valid_slots(idx, n)
    dirty_w, dirty_rel = w.copy(), rel.copy()
    dirty_w[np.broadcast_to(bad[:, None], w.shape)] = np.nan  # NaN on the slots that are no point
    dirty_rel[np.broadcast_to(bad[:, None], rel.shape)] = np.inf
    want = ref.forward(x, idx, w, rel)
    assert np.isnan(want[1]).mean() > 0.9 and np.isfinite(want[2]).any() and np.isnan(want[0]).any()
    for ww, rr in ((w, rel), (dirty_w, dirty_rel)):
        wd, reld = _dev(ww, cuda), _dev(rr, cuda)
        for path in (1, 2):
            assert ref.same_words(_forced(path, lambda: _fwd(xd, idxd, wd, reld)), want)
            _, gw, gr = _forced(path, lambda: _bwd(xd, idxd, wd, reld, god, n, (False, True, True)))
            assert ref.same_words(gw, ref.grad_w(x, idx, go, g, rel)) and ref.same_words(gr, ref.grad_rel(idx, w, go, n))
        cpu = ops.aggregate_points(torch.from_numpy(x), torch.from_numpy(idx), torch.from_numpy(ww), torch.from_numpy(rr)).numpy()
        assert ref.same_words(cpu, want)
    # a healthy cloud beside the all-NaN one is unaffected, gradients included
    gx, _, _ = _bwd(None, idxd, _dev(dirty_w, cuda), None, _dev(ref.gaussian(16, (b, c, m)), cuda), n, (True, False, False))
    assert np.isfinite(gx[1]).all() and np.isfinite(gx[2]).all()


# ---- 9: autograd -------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('need', ((True, True, True), (True, False, False), (False, True, False), (False, False, True), (False, True, None)))
def test_attention_aggregate_under_autograd(cuda, need):
    """The three gradients of ``attention_aggregate`` are, word for word, what the reference loops compute from the kernel's
    own attn (grad_x inside its bound); only the required ones exist.  ``need[2] is None``: no rel."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, g, n, m, k = 2, 18, 2, 70, 130, 16
    x = ref.cloud(30, n, b, c)
    idx, logits, gout = ref.random_list(31, b, n, m, k), ref.gaussian(32, (b, g, m, k), 3.0), ref.gaussian(34, (b, c, m))
    rel = None if need[2] is None else ref.gaussian(33, (b, c, m, k))
    tx, tl = _dev(x, cuda).requires_grad_(need[0]), _dev(logits, cuda).requires_grad_(need[1])
    tr = None if rel is None else _dev(rel, cuda).requires_grad_(need[2])
    out, attn = ops.attention_aggregate(tx, _dev(idx, cuda), tl, tr, return_attention=True)
    a = attn.detach().cpu().numpy()
    assert ref.softmax_ratio(a, logits, idx, n) <= 1.0
    assert ref.same_words(out.detach().cpu().numpy(), ref.forward(x, idx, a, rel))
    out.backward(_dev(gout, cuda))
    assert [t is not None and t.grad is not None for t in (tx, tl, tr)] == [bool(v) for v in need]
    if need[0]:
        ref.GroupedGradX(idx, a, gout, n).check_bound(tx.grad.cpu().numpy())
    if need[1]:
        assert ref.same_words(tl.grad.cpu().numpy(), ref.softmax_bwd(a, idx, n, ref.grad_w(x, idx, gout, g, rel)))
    if need[2]:
        assert ref.same_words(tr.grad.cpu().numpy(), ref.grad_rel(idx, a, gout, n))


def test_vector_attention_is_its_hand_written_composition(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    torch.manual_seed(0)
    b, c, g, n, m, k = 2, 16, 4, 200, 90, 8
    xyz, xyz_q = torch.rand(b, n, 3, device=cuda), torch.rand(b, m, 3, device=cuda)
    query, key = torch.randn(b, c, m, device=cuda), torch.randn(b, c, n, device=cuda)
    value = torch.randn(b, c, n, device=cuda, requires_grad=True)
    pos_net, attn_net = torch.nn.Conv2d(3, c, 1).to(cuda), torch.nn.Conv2d(c, g, 1).to(cuda)
    idx = ops.ball_query(xyz, xyz_q, 0.25, k, pad='none')
    got = ops.vector_attention(xyz_q, xyz, query, key, value, idx, pos_net, attn_net)
    delta = pos_net(ops.group_points(xyz, idx, centres=xyz_q, point_major=True))
    logits = attn_net(delta - ops.group_points(key, idx, centres=query))
    want = ops.aggregate_points(value, idx, ops.neighbour_softmax(logits, idx, n), delta)
    assert got.shape == (b, c, m) and torch.equal(got, want)
    (g1,) = torch.autograd.grad(got.sum(), value, retain_graph=True)
    assert torch.isfinite(g1).all() and pos_net.weight.grad is None
    got.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for net in (pos_net, attn_net) for p in net.parameters())


# ---- 10: the argument checks through the binding -------------------------------------------------------------------------------


def test_einval_messages_and_empty_calls(cuda):
    from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops
    from tests.util import raised

    L = _lib.lib
    b, c, g, n, m, k = 2, 6, 3, 50, 20, 4
    x, idx = _dev(ref.cloud(1, n, b, c), cuda), _dev(ref.random_list(2, b, n, m, k), cuda)
    w, rel = _dev(ref.gaussian(3, (b, g, m, k)), cuda), _dev(ref.gaussian(4, (b, c, m, k)), cuda)
    SENT = -1234.5
    out, gx = torch.full((b, c, m), SENT, device=cuda), torch.full((b, c, n), SENT, device=cuda)
    gw, gr = torch.full((b, g, m, k), SENT, device=cuda), torch.full((b, c, m, k), SENT, device=cuda)
    ptrs = {'x': x, 'idx': idx, 'w': w, 'rel': rel, 'out': out, 'gx': gx, 'gw': gw, 'gr': gr}
    P = {name: t.data_ptr() for name, t in ptrs.items()}

    def entries(b, c, g, n, m, k):
        return (('neighbour_softmax', L.pcc_neighbour_softmax, (b, g, n, m, k, P['idx'], P['w'], P['gw'])),
                ('neighbour_softmax_bwd', L.pcc_neighbour_softmax_bwd, (b, g, n, m, k, P['idx'], P['w'], P['w'], P['gw'])),
                ('aggregate_points', L.pcc_aggregate_points, (b, c, g, n, m, k, P['x'], P['idx'], P['w'], P['rel'], P['out'])),
                ('aggregate_points_bwd', L.pcc_aggregate_points_bwd,
                 (b, c, g, n, m, k, P['x'], P['idx'], P['w'], P['rel'], P['out'], P['gx'], P['gw'], P['gr'])))

    cases = [((-1, c, g, n, m, k), 'bad size'), ((b, c, g, 0, m, k), 'bad size'), ((b, c, g, n, m, 0), 'bad size'),
             ((65536, c, g, n, m, k), 'batch too large'), ((b, c, g, n, 1 << 16, 1 << 15), 'list too long (m * k >= 2^31)'),
             ((b, c, g, n, m, 129), 'k > 128')]
    for sizes, text in cases:
        for name, fn, args in entries(*sizes):
            assert raised(RuntimeError, _lib.call, fn, name, cuda, *args) == f'{name}: {name}: {text}'
    for name, fn, args in entries(b, c, 4, n, m, k)[2:]:
        assert raised(RuntimeError, _lib.call, fn, name, cuda, *args) == f'{name}: {name}: g must be >= 1 and divide c'
    for name, fn, args in entries(0, c, g, n, m, k) + entries(b, c, g, n, 0, k)[:3]:
        _lib.call(fn, name, cuda, *args)  # an empty batch; an empty list forward
    _lib.call(L.pcc_aggregate_points_bwd, 'aggregate_points_bwd', cuda, b, c, g, n, m, k, P['x'], P['idx'], P['w'], None, P['out'],
              None, None, None)  # no gradient asked for
    torch.cuda.synchronize()
    for t in (out, gx, gw, gr):
        assert (t == SENT).all()  # nothing ran
    _lib.call(L.pcc_aggregate_points_bwd, 'aggregate_points_bwd', cuda, b, c, g, n, 0, k, None, None, None, None, None, P['gx'],
              P['gw'], P['gr'])  # m = 0: grad_x zero-filled
    torch.cuda.synchronize()
    assert (gx.cpu().numpy().view(np.uint32) == 0).all() and (gw == SENT).all() and (gr == SENT).all()
    # the Python layer: refusals before anything is allocated, empty calls
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.aggregate_points(x, idx.cpu(), w, rel)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.attention_aggregate(x, idx, w, rel.cpu())
    with pytest.raises(ValueError, match='do not divide'):
        ops.aggregate_points(x, idx, w[:, :1].expand(-1, 4, -1, -1), rel)
    for bb, mm in ((0, m), (b, 0)):
        t = ops.attention_aggregate(x[:bb].clone().requires_grad_(True), idx[:bb, :mm], w[:bb, :, :mm], rel[:bb, :, :mm])
        assert t.shape == (bb, c, mm)
        t.sum().backward()
    assert ref.same_words(ops.aggregate_points(x, idx, w, rel).cpu().numpy(),
                          ref.forward(*(t.cpu().numpy() for t in (x, idx, w, rel))))  # the library still answers
