"""GPU tests of the interpolation op (``pcc_interpolate`` / ``pcc_interpolate_bwd`` through the C ABI and through
``neighbour_ops.interpolate_points`` / ``feature_propagation``) against the numpy reference of tests/interpolate_reference.py:
the forward and grad_w word for word, grad_x word for word on integer gradients with dyadic weights (every product and
partial sum is exact in any order) and inside the float32 summation bound on Gaussian ones, both paths against the
product's choice on either side of every boundary of the dispatch, independence of the batch and of m, non-finite input,
the argument checks, and the composite."""

import numpy as np
import pytest
import torch

from tests import interpolate_reference as ref
from tests.list_plan_reference import kernel_of
from tests.which_ran import assert_only, ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5  # what the channels outside a call's slice must keep


_PATH = [0]  # the interp_path value in force: every call below asserts the kernel the plan predicts under it


def _forced(path, fn):
    """``fn()`` under interp_path = ``path``.  ``_fwd`` and ``_bwd`` assert from their launch records that the forced
    variant ran and its sibling did not; a forced LDS path that cannot hold a row is ignored (include/pcc_test_hooks.h):
    the plan then predicts the direct kernel, the product's choice."""
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


def _fwd(x, idx, w, out_c=None, out_c0=0):
    """``pcc_interpolate`` on device tensors: the slice ``[b,c,m]`` as numpy; the channels outside it must still hold the
    sentinel."""
    from pointcloudcounterfactual_amd import _lib

    b, c, n = x.shape
    m, k = idx.shape[1:]
    out_c = c if out_c is None else out_c
    out = torch.full((b, out_c, m), SENTINEL, dtype=torch.float32, device=x.device)
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_interpolate, 'interpolate', x.device, b, c, n, m, k, _p(x), _p(idx), _p(w), _p(out),
                                     out_c, out_c0))
    assert names == ({kernel_of('interp_fwd_kernel', b, c, n, _PATH[0]): 1} if b and m else {}), (n, _PATH[0], names)
    out = out.cpu().numpy()
    rest = np.delete(out, np.s_[out_c0:out_c0 + c], axis=1)
    assert (rest == np.float32(SENTINEL)).all()
    return out[:, out_c0:out_c0 + c]


def _bwd(x, idx, w, g, c, n, out_c0=0, want_x=True, want_w=True):
    """``pcc_interpolate_bwd`` on the slice ``out_c0 .. out_c0 + c - 1`` of ``g[b,out_c,m]``: ``(grad_x, grad_w)`` as numpy
    arrays (None where not asked for).  The outputs start as NaN: every element must be written."""
    from pointcloudcounterfactual_amd import _lib

    b, out_c, m = g.shape
    k = idx.shape[2]
    gx = torch.full((b, c, n), float('nan'), device=g.device) if want_x else None
    gw = torch.full((b, m, k), float('nan'), device=g.device) if want_w else None
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_interpolate_bwd, 'interpolate_bwd', g.device, b, c, n, m, k, _p(x), _p(idx), _p(w),
                                     _p(g), out_c, out_c0, _p(gx), _p(gw)))
    if b and m:
        assert_only(names, [kernel_of('interp_bwd_x_kernel', b, c, n, _PATH[0])] if want_x else [], 'interp_bwd_x_kernel')
        assert ('interp_bwd_w_kernel' in names) == want_w, names
    back = lambda t: None if t is None else t.cpu().numpy()  # noqa: E731
    return back(gx), back(gw)


def _sliced_gradient(g, out_c0):
    """``g[b,c,m]`` inside ``[b, out_c0 + c + 1, m]``, NaN around it (the backward must not read it)."""
    b, c, m = g.shape
    full = np.full((b, out_c0 + c + 1, m), np.nan, dtype=np.float32)
    full[:, out_c0:out_c0 + c] = g
    return full


def _lists(cuda, seed, x_all, n, m, k):
    """``{origin: (idx[B_MAX,m,k], w[B_MAX,m,k])}``: a random list with -1, n and 2^40 in it under Gaussian signed weights,
    a ``knn_cross`` list from m other points (where k <= n) under ``interpolation_weights`` of its distances, and a
    ``ball_query(pad='none')`` list around m other points under Gaussian weights."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    rng = np.random.default_rng(seed)
    lists = {'random': (ref.random_list(seed, ref.B_MAX, n, m, k), ref.gaussian_weights(seed + 1, ref.B_MAX, m, k))}
    xyz = _dev(x_all[:, :3].transpose(0, 2, 1), cuda)  # [B,n,3]: the first channels of the cloud as coordinates
    q = rng.standard_normal((ref.B_MAX, m, 3)).astype(np.float32)
    if k <= n:
        idx, dist = ops.knn_cross(_dev(q.transpose(0, 2, 1), cuda), xyz.transpose(1, 2).contiguous(), k, return_distance=True)
        lists['knn_cross'] = (idx.cpu().numpy(), ops.interpolation_weights(dist).cpu().numpy())
    lists['ball_none'] = (ops.ball_query(xyz, _dev(q, cuda), 1.2, k, pad='none').cpu().numpy(), ref.gaussian_weights(seed + 2, ref.B_MAX, m, k))
    return lists


@pytest.mark.parametrize('n', ref.N_GRID)
def test_forward_and_grad_w_word_for_word(cuda, n):
    """Every m, k, c of the grid with every origin of the list; b and out_c0 rotate (out_c = out_c0 + c + 2: the channels
    around the slice keep their sentinel).  grad_w against the float32 channel loop, the origin of the list rotating."""
    x_all = ref.cloud(n, n)
    rng = np.random.default_rng(50 + n)
    lists = {}
    for m, k, c, b, out_c0, j in ref.grid():
        if (m, k) not in lists:
            lists[m, k] = _lists(cuda, 17 * m + k + n, x_all, n, m, k)
        x = np.ascontiguousarray(x_all[:b, :c])
        xd = _dev(x, cuda)
        for kind, (idx, w) in lists[m, k].items():
            got = _fwd(xd, _dev(idx[:b], cuda), _dev(w[:b], cuda), out_c0 + c + 2, out_c0)
            assert np.array_equal(got.view(np.uint32), ref.forward(x, idx[:b], w[:b]).view(np.uint32)), (m, k, c, b, out_c0, kind)
        kinds = sorted(lists[m, k])
        idx, w = lists[m, k][kinds[j % len(kinds)]]
        g = rng.standard_normal((b, c, m)).astype(np.float32)
        _, gw = _bwd(xd, _dev(idx[:b], cuda), _dev(w[:b], cuda), _dev(_sliced_gradient(g, out_c0), cuda), c, n, out_c0, want_x=False)
        assert np.array_equal(gw.view(np.uint32), ref.grad_w(x, idx[:b], g).view(np.uint32)), (m, k, c, b, out_c0)


@pytest.mark.parametrize('n', ref.BOUNDARIES)
def test_every_variant_gives_the_same_words(cuda, n):
    """The LDS path (1) and the direct path (2) forced against the product's choice, and that against the reference, on
    both sides of every step of the channel block and of the LDS -> direct switch; forward and (integer gradients, dyadic
    weights) backward.  At 40961 the forced LDS path cannot hold a row and is ignored."""
    m, k, b = 65, 3, 2
    x_all = ref.cloud(n, n, b)
    rng = np.random.default_rng(n)
    idx = ref.random_list(n, b, n, m, k)
    idxd = _dev(idx, cuda)
    for c, out_c0 in ((9, 1), (3, 0), (8, 3), (5, 0)):
        x = np.ascontiguousarray(x_all[:, :c])
        xd = _dev(x, cuda)
        w, wq = ref.gaussian_weights(n + c, b, m, k), ref.dyadic_weights(n + c, b, m, k)
        wd, wqd = _dev(w, cuda), _dev(wq, cuda)
        g = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
        gd = _dev(_sliced_gradient(g, out_c0), cuda)
        want = ref.forward(x, idx, w).view(np.uint32)
        back, want_w = ref.GradX(idx, wq, g, n), ref.grad_w(x, idx, g).view(np.uint32)
        for path in (0, 1, 2):
            got = _forced(path, lambda: _fwd(xd, idxd, wd, out_c0 + c + 1, out_c0))
            assert np.array_equal(got.view(np.uint32), want), (c, path)
            gx, gw = _forced(path, lambda: _bwd(xd, idxd, wqd, gd, c, n, out_c0))
            back.check_exact(gx)
            assert np.array_equal(gw.view(np.uint32), want_w)


@pytest.mark.parametrize('n', ref.N_GRID)
def test_grad_x_word_for_word(cuda, n):
    """Integer gradients in [-8, 8] and weights from {0, +-1/2, +-1, +-2}: every product and partial sum is exact in any
    order.  The grid of the forward test, the origin of the list rotating, on both paths; points nothing refers to get
    +0.0."""
    x_all = ref.cloud(n, n)
    rng = np.random.default_rng(70 + n)
    lists = {}
    for m, k, c, b, out_c0, j in ref.grid():
        if (m, k) not in lists:
            lists[m, k] = _lists(cuda, 17 * m + k + n, x_all, n, m, k)
        kinds = sorted(lists[m, k])
        idx = lists[m, k][kinds[j % len(kinds)]][0][:b]
        w = ref.dyadic_weights(j, b, m, k)
        g = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
        back = ref.GradX(idx, w, g, n)
        idxd, wd, gd = _dev(idx, cuda), _dev(w, cuda), _dev(_sliced_gradient(g, out_c0), cuda)
        for path in (1, 2):
            gx, _ = _forced(path, lambda: _bwd(None, idxd, wd, gd, c, n, out_c0, want_w=False))  # (x may be null without grad_w)
            back.check_exact(gx)


def test_grad_x_on_a_hub(cuda):
    """Every slot pointing at one point (m = 300, k = 3), on both paths."""
    rng = np.random.default_rng(3)
    n, m, k, b, c = 500, 300, 3, 2, 9
    hub = np.full((b, m, k), 77, dtype=np.int64)
    hub[1] = 499
    w = ref.dyadic_weights(4, b, m, k)
    g = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
    back = ref.GradX(hub, w, g, n)
    idxd, wd, gd = _dev(hub, cuda), _dev(w, cuda), _dev(_sliced_gradient(g, 2), cuda)
    for path in (1, 2):
        gx, _ = _forced(path, lambda: _bwd(None, idxd, wd, gd, c, n, 2, want_w=False))
        back.check_exact(gx)


def test_grad_x_on_generic_gradients_is_inside_the_summation_bound(cuda):
    """Gaussian gradients and weights: |got - ref64| <= gamma(deg + 1) * sum |w g| per bin, one rounding per product and a
    float32 sum of deg terms in any order (tests/interpolate_reference.py): derived, not tuned."""
    rng = np.random.default_rng(4)
    worst = 0.0
    for n, m, k, c, b in ((65, 257, 5, 9, 3), (1025, 257, 4, 8, 2), (300, 300, 3, 3, 2), (2049, 65, 3, 5, 2), (3, 257, 3, 9, 3)):
        lists = {'random': ref.random_list(n, b, n, m, k), 'hub': np.full((b, m, k), n - 1, dtype=np.int64)}
        for kind, idx in lists.items():
            w = ref.gaussian_weights(n + 1, b, m, k)
            g = rng.standard_normal((b, c, m)).astype(np.float32)
            back = ref.GradX(idx, w, g, n)
            idxd, wd, gd = _dev(idx, cuda), _dev(w, cuda), _dev(g, cuda)
            for path in (1, 2):
                gx, _ = _forced(path, lambda: _bwd(None, idxd, wd, gd, c, n, want_w=False))
                worst = max(worst, back.ratio(gx))
                back.check_bound(gx)
    print(f'grad_x: the largest error is {worst:.2f} of the bound')


def test_long_lists_and_many_blocks(cuda):
    """Units longer than one pass of a workgroup (every size of workgroup up to the full 1024 threads, the strided loops of
    the forward with scalar and with 16-byte stores and of the backward) and a list split over several workgroups, on both
    paths: (b, c, n, m) = (8, 64, 64, 8195) is 64 channel blocks of CB = 8, (4, 128, 16385, 8192) 512 of CB = 1."""
    rng = np.random.default_rng(21)
    k = 3
    for b, c, n, m in ((8, 64, 64, 8195), (4, 128, 16385, 8192)):
        x = ref.cloud(22, n, b, c)
        idx, w, wq = ref.random_list(23, b, n, m, k), ref.gaussian_weights(24, b, m, k), ref.dyadic_weights(25, b, m, k)
        g = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
        want, want_w, back = ref.forward(x, idx, w).view(np.uint32), ref.grad_w(x, idx, g).view(np.uint32), ref.GradX(idx, wq, g, n)
        xd, idxd, wd, wqd, gd = (_dev(a, cuda) for a in (x, idx, w, wq, g))
        for path in (1, 2):
            got = _forced(path, lambda: _fwd(xd, idxd, wd))
            assert np.array_equal(got.view(np.uint32), want), (n, path)
            gx, gw = _forced(path, lambda: _bwd(xd, idxd, wqd, gd, c, n))
            back.check_exact(gx)
            assert np.array_equal(gw.view(np.uint32), want_w)


def test_independence(cuda):
    """A batch against its clouds one by one and against a permuted batch; a prefix of m equals the slice of the full m;
    either gradient alone equals the pair."""
    n, m, k, c, b = 1025, 300, 3, 9, 5
    rng = np.random.default_rng(6)
    x = ref.cloud(7, n, b, c)
    idx, w = ref.random_list(8, b, n, m, k), ref.gaussian_weights(9, b, m, k)
    wq = ref.dyadic_weights(10, b, m, k)
    g = rng.integers(-8, 9, size=(b, c, m)).astype(np.float32)
    xd, idxd, wd, wqd, gd = (_dev(a, cuda) for a in (x, idx, w, wq, g))
    order = [2, 4, 0, 3, 1]
    for path in (0, 1, 2):
        out = _forced(path, lambda: _fwd(xd, idxd, wd))
        assert np.array_equal(out.view(np.uint32), ref.forward(x, idx, w).view(np.uint32))
        gx, gw = _forced(path, lambda: _bwd(xd, idxd, wqd, gd, c, n))
        for i in (0, 2, 4):
            alone = _forced(path, lambda: _fwd(xd[i:i + 1], idxd[i:i + 1], wd[i:i + 1]))
            assert np.array_equal(alone[0].view(np.uint32), out[i].view(np.uint32))
            ax, aw = _forced(path, lambda: _bwd(xd[i:i + 1], idxd[i:i + 1], wqd[i:i + 1], gd[i:i + 1], c, n))
            assert np.array_equal(ax[0], gx[i]) and np.array_equal(aw[0].view(np.uint32), gw[i].view(np.uint32))
        moved = _forced(path, lambda: _fwd(xd[order].contiguous(), idxd[order].contiguous(), wd[order].contiguous()))
        assert np.array_equal(moved.view(np.uint32), out[order].view(np.uint32))
        for pre in (43, 128):  # (another m: other alignment, the other store width)
            fewer = _forced(path, lambda: _fwd(xd, idxd[:, :pre].contiguous(), wd[:, :pre].contiguous()))
            assert np.array_equal(fewer.view(np.uint32), out[:, :, :pre].view(np.uint32))
        only_x = _forced(path, lambda: _bwd(None, idxd, wqd, gd, c, n, want_w=False))
        only_w = _forced(path, lambda: _bwd(xd, idxd, wqd, gd, c, n, want_x=False))
        assert only_x[1] is None and only_w[0] is None
        assert np.array_equal(only_x[0], gx) and np.array_equal(only_w[1].view(np.uint32), gw.view(np.uint32))


def test_non_finite_input(cuda):
    """NaN and +-inf in x and in w: the same words as the CPU path and as the reference (a NaN result is the word
    0x7fc00000); an out-of-range slot with a NaN weight changes nothing; a healthy cloud beside an all-NaN one is
    unaffected."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    n, m, k, c, b = 300, 128, 4, 5, 3
    x = ref.cloud(11, n, b, c)
    x[0, :, ::7] = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)[:, None]
    x[1] = np.nan
    idx, w = ref.random_list(12, b, n, m, k), ref.gaussian_weights(13, b, m, k)
    w[0, ::5, 1] = np.array([np.nan, np.inf, 0.0, -np.inf], dtype=np.float32)[np.arange(len(range(0, m, 5))) % 4]
    plain = w.copy()
    bad = (idx < 0) | (idx >= n)
    w[bad & (np.arange(m)[None, :, None] % 2 == 0)] = np.nan  # NaN weights on slots that are no point
    want = ref.forward(x, idx, w)
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any() and np.isfinite(want[2]).all()
    assert np.array_equal(want.view(np.uint32), ref.forward(x, idx, plain).view(np.uint32))
    cpu = ops.interpolate_points(torch.from_numpy(x), torch.from_numpy(idx), torch.from_numpy(w)).numpy()
    assert np.array_equal(cpu.view(np.uint32), want.view(np.uint32))
    xd, idxd, wd = _dev(x, cuda), _dev(idx, cuda), _dev(w, cuda)
    for path in (0, 1, 2):
        for mm in (m, m - 1):  # (16-byte stores, scalar stores)
            got = _forced(path, lambda: _fwd(xd, idxd[:, :mm].contiguous(), wd[:, :mm].contiguous()))
            assert np.array_equal(got.view(np.uint32), cpu[:, :, :mm].view(np.uint32)), (path, mm)
        alone = _forced(path, lambda: _fwd(xd[2:], idxd[2:], wd[2:]))
        assert np.array_equal(alone[0].view(np.uint32), want[2].view(np.uint32))


def test_arguments(cuda):
    from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops

    L = _lib.lib
    b, c, n, m, k = 2, 3, 300, 20, 3
    x = _dev(ref.cloud(13, n, b, c), cuda)
    idx, w = _dev(ref.random_list(14, b, n, m, k), cuda), _dev(ref.gaussian_weights(15, b, m, k), cuda)
    good = ops.interpolate_points(x, idx, w)
    out = torch.full((b, c, m), SENTINEL, device=cuda)
    gx, gw = torch.full((b, c, n), SENTINEL, device=cuda), torch.full((b, m, k), SENTINEL, device=cuda)
    xp, ip, wp, op, gxp, gwp = (t.data_ptr() for t in (x, idx, w, out, gx, gw))
    stream = torch.cuda.current_stream(cuda).cuda_stream
    # (b, c, n, m, k, out_c, out_c0)
    sizes = (b, c, n, m, k, c, 0)
    bad_sizes = [(-1, c, n, m, k, c, 0), (65536, c, n, m, k, c, 0), (b, 0, n, m, k, c, 0), (b, c, 0, m, k, c, 0), (b, c, n, -1, k, c, 0),
                 (b, c, n, m, 0, c, 0), (b, c, n, m, k, c - 1, 0), (b, c, n, m, k, c, 1), (b, c, n, m, k, c, -1),
                 (b, c, n, 1 << 16, 1 << 15, c, 0)]
    for s in bad_sizes:
        assert L.pcc_interpolate(*s[:5], xp, ip, wp, op, *s[5:], stream) != 0, s
        assert L.pcc_last_error().decode().startswith('interpolate:')
        assert L.pcc_interpolate_bwd(*s[:5], xp, ip, wp, op, *s[5:], gxp, gwp, stream) != 0, s
        assert L.pcc_last_error().decode().startswith('interpolate_bwd:')
    for ptrs in ((None, ip, wp, op), (xp, None, wp, op), (xp, ip, None, op), (xp, ip, wp, None)):
        assert L.pcc_interpolate(*sizes[:5], *ptrs, *sizes[5:], stream) != 0
        assert L.pcc_last_error().decode().startswith('interpolate:')
    for ptrs in ((xp, None, wp, op), (xp, ip, None, op), (xp, ip, wp, None), (None, ip, wp, op)):
        assert L.pcc_interpolate_bwd(*sizes[:5], *ptrs, *sizes[5:], gxp, gwp, stream) != 0
        assert L.pcc_last_error().decode().startswith('interpolate_bwd:')
    assert L.pcc_interpolate_bwd(*sizes[:5], xp, ip, wp, op, *sizes[5:], None, None, stream) == 0  # no gradient asked for
    assert L.pcc_interpolate(0, *sizes[1:5], xp, ip, wp, op, *sizes[5:], stream) == 0              # b = 0
    assert L.pcc_interpolate_bwd(0, *sizes[1:5], xp, ip, wp, op, *sizes[5:], gxp, gwp, stream) == 0
    assert L.pcc_interpolate(b, c, n, 0, k, xp, None, None, None, c, 0, stream) == 0               # m = 0 forward
    torch.cuda.synchronize()
    for t in (out, gx, gw):
        assert (t == SENTINEL).all()  # nothing ran
    assert L.pcc_interpolate_bwd(b, c, n, 0, k, None, None, None, None, c, 0, gxp, gwp, stream) == 0  # m = 0: grad_x zero-filled
    torch.cuda.synchronize()
    assert (gx.cpu().numpy().view(np.uint32) == 0).all() and (gw == SENTINEL).all()
    # the Python layer: refusals before anything is allocated, empty calls, views
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.interpolate_points(x, idx.cpu(), w)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.interpolate_points(x, idx, w.cpu())
    with pytest.raises(RuntimeError):
        ops.interpolate_points(x.cpu(), idx, w)
    with pytest.raises(RuntimeError):
        ops.interpolate_points(x.double(), idx, w)
    with pytest.raises(RuntimeError):
        ops.interpolate_points(x, idx.int(), w)
    with pytest.raises(ValueError):
        ops.interpolate_points(x, idx, w[:, :, :2])
    with pytest.raises(ValueError):
        ops.interpolate_points(x, idx[:1], w[:1])
    for eb, em in ((0, m), (b, 0)):
        xe = x[:eb].clone().requires_grad_(True)
        we = w[:eb, :em].clone().requires_grad_(True)
        empty = ops.interpolate_points(xe, idx[:eb, :em], we)
        assert empty.shape == (eb, c, em) and empty.dtype == torch.float32 and empty.device == x.device
        empty.sum().backward()
        assert xe.grad.shape == xe.shape and (xe.grad == 0).all() and we.grad.shape == we.shape
    big = _dev(ref.cloud(15, 2 * n, b, 2 * c), cuda)
    view, iview, wview = big[:, ::2, ::2], torch.cat((idx, idx), 2)[:, :, ::2], torch.cat((w, w), 2)[:, :, ::2]
    assert not view.is_contiguous() and not iview.is_contiguous() and not wview.is_contiguous()
    assert torch.equal(ops.interpolate_points(view, iview, wview),
                       ops.interpolate_points(view.contiguous(), iview.contiguous(), wview.contiguous()))
    assert torch.equal(ops.interpolate_points(x, idx, w), good)  # the library still answers


@pytest.mark.parametrize('x_grad,w_grad', [(True, True), (True, False), (False, True), (False, False)])
def test_interpolate_points_under_autograd_agrees_with_the_cpu_path(cuda, x_grad, w_grad):
    """``interpolate_points`` on the device against its CPU path on the GPU's own list and weights (a ``knn_cross`` list
    with ``interpolation_weights``): forward word for word, grad_x inside the summation bound, grad_w word for word against
    the channel loop and inside gamma(c + 1) * sum |g x| of the CPU path's; a gradient that is not asked for is None."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    n, m, k, c, b = 37, 300, 3, 5, 3
    rng = np.random.default_rng(16)
    x = ref.cloud(17, n, b, c)
    q = _dev(rng.standard_normal((b, 3, m)).astype(np.float32), cuda)
    idxd, dist = ops.knn_cross(q, _dev(x[:, :3], cuda), k, return_distance=True)
    wdev = ops.interpolation_weights(dist)
    idx, w = idxd.cpu().numpy(), wdev.cpu().numpy()
    g = rng.standard_normal((b, c, m)).astype(np.float32)
    res = {}
    for dev in (cuda, torch.device('cpu')):
        tx = _dev(x, dev).requires_grad_(x_grad)
        tw = _dev(w, dev).requires_grad_(w_grad)
        out = ops.interpolate_points(tx, _dev(idx, dev), tw)
        assert out.requires_grad == (x_grad or w_grad)
        if out.requires_grad:
            out.backward(_dev(g, dev))
        res[dev.type] = (out.detach().cpu().numpy(), tx.grad, tw.grad)
    assert np.array_equal(res['cuda'][0].view(np.uint32), res['cpu'][0].view(np.uint32))
    assert np.array_equal(res['cuda'][0].view(np.uint32), ref.forward(x, idx, w).view(np.uint32))
    for kind in ('cuda', 'cpu'):
        assert (res[kind][1] is not None) == x_grad and (res[kind][2] is not None) == w_grad
    if x_grad:
        back = ref.GradX(idx, w, g, n)
        back.check_bound(res['cuda'][1].cpu().numpy())
        back.check_bound(res['cpu'][1].numpy())
    if w_grad:
        assert np.array_equal(res['cuda'][2].cpu().numpy().view(np.uint32), ref.grad_w(x, idx, g).view(np.uint32))
        _, xg = ref._gathered(x.astype(np.float64), idx)
        prod = g.astype(np.float64)[:, :, :, None] * xg
        assert (np.abs(res['cpu'][2].numpy() - prod.sum(1)) <= ref.gamma(c + 1) * np.abs(prod).sum(1)).all()


@pytest.mark.parametrize('n,with_skip', [(37, True), (37, False), (2, True)])
def test_feature_propagation(cuda, n, with_skip):
    """Every output against the hand-written composition on the same list (knn_cross, interpolation_weights, gather +
    multiply + sum, cat); N = 2 < k: the list has min(k, N) columns.  The gradients of the features against float64 by the
    bound, those of skip bit for bit; the CPU path on the GPU's list against the kernel word for word."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, m, c, c2, k = 3, 300, 5, 4, 3
    rng = np.random.default_rng(19)
    dense_np, sparse_np = rng.random((b, m, 3)).astype(np.float32), rng.random((b, n, 3)).astype(np.float32)
    feat_np, skip_np = rng.standard_normal((b, c, n)).astype(np.float32), rng.standard_normal((b, c2, m)).astype(np.float32)
    dense, sparse = _dev(dense_np, cuda).requires_grad_(True), _dev(sparse_np, cuda).requires_grad_(True)
    feat = _dev(feat_np, cuda).requires_grad_(True)
    skip = _dev(skip_np, cuda).requires_grad_(True) if with_skip else None
    res = ops.feature_propagation(dense, sparse, feat, skip, k=k)
    kk = min(k, n)
    idx, dist = ops.knn_cross(dense.detach().transpose(1, 2), sparse.detach().transpose(1, 2), kk, return_distance=True)
    weights = ops.interpolation_weights(dist)
    assert res.idx.shape == (b, m, kk) and torch.equal(res.idx, idx) and torch.equal(res.weights, weights)
    assert not res.idx.requires_grad and not res.weights.requires_grad
    gathered = feat.detach().gather(2, idx.reshape(b, 1, m * kk).expand(-1, c, -1)).view(b, c, m, kk)
    hand = torch.zeros(b, c, m, device=cuda)
    for j in range(kk):
        hand = hand + weights[:, None, :, j] * gathered[:, :, :, j]
    if with_skip:
        hand = torch.cat((hand, skip.detach()), 1)
    assert res.out.shape == hand.shape == (b, c + (c2 if with_skip else 0), m)
    assert np.array_equal(res.out.detach().cpu().numpy().view(np.uint32), hand.cpu().numpy().view(np.uint32))
    idx_np, w_np = idx.cpu().numpy(), weights.cpu().numpy()
    want = ref.hand_propagation(feat_np, skip_np if with_skip else None, idx_np, w_np)
    assert np.array_equal(res.out.detach().cpu().numpy().view(np.uint32), want.view(np.uint32))
    cpu = ops.interpolate_points(torch.from_numpy(feat_np), torch.from_numpy(idx_np), torch.from_numpy(w_np))
    assert np.array_equal(cpu.numpy().view(np.uint32), want[:, :c].view(np.uint32))
    g = rng.standard_normal(want.shape).astype(np.float32)
    res.out.backward(_dev(g, cuda))
    ref.GradX(idx_np, w_np, g[:, :c], n).check_bound(feat.grad.cpu().numpy())
    if with_skip:
        assert np.array_equal(skip.grad.cpu().numpy(), g[:, c:])
    assert dense.grad is None and sparse.grad is None
