"""GPU tests of the grouping op (``pcc_group_points`` / ``pcc_group_points_bwd`` through the C ABI and through
``neighbour_ops.group_points`` / ``sample_and_group``) against the numpy reference of tests/grouping_reference.py: the
forward word for word, the backward word for word on integer-valued gradients (every partial sum is exact in any order)
and inside the float32 summation bound on Gaussian ones, both paths against the product's choice on either side of every
boundary of the dispatch, independence of the batch, non-finite input, the argument checks, and the composite."""

import numpy as np
import pytest
import torch

from tests import grouping_reference as ref
from tests.list_plan_reference import kernel_of
from tests.which_ran import assert_only, ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5  # what the channels outside a call's slice must keep


_PATH = [0]  # the group_path value in force: every call below asserts the kernel the plan predicts under it


def _forced(path, fn):
    """``fn()`` under group_path = ``path``.  ``_fwd`` and ``_bwd`` assert from their launch records that the forced
    variant ran and its sibling did not; a forced LDS path that cannot hold a row is ignored (include/pcc_test_hooks.h):
    the plan then predicts the direct kernel, the product's choice."""
    from pointcloudcounterfactual_amd import _lib

    with _lib.tuning('group_path', path):
        _PATH[0] = path
        try:
            return fn()
        finally:
            _PATH[0] = 0


def _p(t):
    return None if t is None else t.data_ptr()


def _fwd(x, idx, centre, point_major, out_c=None, out_c0=0):
    """``pcc_group_points`` on device tensors (``x`` and ``centre`` in the layout of ``point_major``): the slice
    ``[b,c,m,k]`` as numpy; the channels outside it must still hold the sentinel."""
    from pointcloudcounterfactual_amd import _lib

    b = x.shape[0]
    n, c = (x.shape[1], x.shape[2]) if point_major else (x.shape[2], x.shape[1])
    m, k = idx.shape[1:]
    out_c = c if out_c is None else out_c
    out = torch.full((b, out_c, m, k), SENTINEL, dtype=torch.float32, device=x.device)
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_group_points, 'group_points', x.device, b, c, n, m, k, int(point_major), _p(x),
                                     _p(idx), _p(centre), _p(out), out_c, out_c0))
    assert names == ({kernel_of('group_fwd_kernel', b, c, n, _PATH[0]): 1} if b and m else {}), (n, _PATH[0], names)
    out = out.cpu().numpy()
    rest = np.delete(out, np.s_[out_c0:out_c0 + c], axis=1)
    assert (rest == np.float32(SENTINEL)).all()
    return out[:, out_c0:out_c0 + c]


def _bwd(idx, g, n, c, point_major, out_c0=0, want_x=True, want_c=True):
    """``pcc_group_points_bwd`` on the slice ``out_c0 .. out_c0 + c - 1`` of ``g[b,out_c,m,k]``: ``(grad_x, grad_centre)``
    as channels-major numpy arrays (None where not asked for).  The outputs start as NaN: every element must be written."""
    from pointcloudcounterfactual_amd import _lib

    b, out_c, m, k = g.shape
    gx = torch.full((b, n, c) if point_major else (b, c, n), float('nan'), device=g.device) if want_x else None
    gc = torch.full((b, m, c) if point_major else (b, c, m), float('nan'), device=g.device) if want_c else None
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_group_points_bwd, 'group_points_bwd', g.device, b, c, n, m, k, int(point_major),
                                     _p(idx), _p(g), out_c, out_c0, _p(gx), _p(gc)))
    if b and m:
        assert_only(names, [kernel_of('group_bwd_kernel', b, c, n, _PATH[0])] if want_x else [], 'group_bwd_kernel')
        assert ('group_centre_bwd_kernel' in names) == want_c, names
    back = lambda t: None if t is None else ref.to_layout(t.cpu().numpy(), point_major)  # noqa: E731
    return back(gx), back(gc)


def _dev(a, cuda, point_major=False):
    return None if a is None else torch.from_numpy(ref.to_layout(a, point_major)).to(cuda)


def _lists(cuda, seed, x_all, n, m, k):
    """Index lists ``[B_MAX,m,k]`` of every origin: ``ball_query`` (either pad) around m of the cloud's points, ``knn_cross``
    from m other points (where k <= n), a random list with -1, n and 2^40 in it."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    rng = np.random.default_rng(seed)
    xyz = torch.from_numpy(np.ascontiguousarray(x_all[:, :3].transpose(0, 2, 1))).to(cuda)  # [B,n,3]
    centres = xyz[:, torch.from_numpy(rng.integers(0, n, size=m)).to(cuda)].contiguous()
    lists = {'random': ref.random_list(seed, ref.B_MAX, n, m, k)}
    for pad in ('first', 'none'):
        lists['ball_' + pad] = ops.ball_query(xyz, centres, 0.9, k, pad=pad).cpu().numpy()
    if k <= min(n, 128):
        q = torch.from_numpy(rng.standard_normal((ref.B_MAX, 3, m)).astype(np.float32)).to(cuda)
        lists['knn_cross'] = ops.knn_cross(q, xyz.transpose(1, 2).contiguous(), k).cpu().numpy()
    return lists


@pytest.mark.parametrize('n', ref.N_GRID)
def test_forward_word_for_word(cuda, n):
    """Both layouts, with and without centres, every m, k, c of the grid with every origin of the list; b and out_c0 rotate
    (out_c = out_c0 + c + 2: the channels around the slice keep their sentinel)."""
    x_all = ref.cloud(n, n)
    rng = np.random.default_rng(50 + n)
    lists = {}
    for m, k, c, point_major, relative, b, out_c0, _ in ref.grid():
        if (m, k) not in lists:
            lists[m, k] = _lists(cuda, 17 * m + k + n, x_all, n, m, k)
        x = np.ascontiguousarray(x_all[:b, :c])
        centre = rng.standard_normal((b, c, m)).astype(np.float32) if relative else None
        xd, cd = _dev(x, cuda, point_major), _dev(centre, cuda, point_major)
        for kind, idx in lists[m, k].items():
            got = _fwd(xd, torch.from_numpy(idx[:b]).to(cuda), cd, point_major, out_c0 + c + 2, out_c0)
            want = ref.forward(x, idx[:b], centre)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (m, k, c, point_major, relative, b, out_c0, kind)


@pytest.mark.parametrize('n', ref.BOUNDARIES)
def test_every_variant_gives_the_same_words(cuda, n):
    """The LDS path (1) and the direct path (2) forced against the product's choice, and that against the reference, on
    both sides of every step of the channel block and of the LDS -> direct switch; forward and (integer gradients)
    backward.  At 40961 the forced LDS path cannot hold a row and is ignored."""
    m, k, b = 65, 5, 2
    x_all = ref.cloud(n, n, b)
    rng = np.random.default_rng(n)
    lists = {'random': ref.random_list(n, b, n, m, k), 'first': ref.padded_list(n + 1, b, n, m, k, 'first')}
    for c, point_major, relative, out_c0 in ((9, False, False, 1), (3, True, True, 0), (8, False, True, 3), (5, True, False, 0)):
        x = np.ascontiguousarray(x_all[:, :c])
        centre = rng.standard_normal((b, c, m)).astype(np.float32) if relative else None
        xd, cd = _dev(x, cuda, point_major), _dev(centre, cuda, point_major)
        g = np.full((b, out_c0 + c + 1, m, k), np.nan, dtype=np.float32)
        g[:, out_c0:out_c0 + c] = rng.integers(-8, 9, size=(b, c, m, k))
        gd = torch.from_numpy(g).to(cuda)
        for kind, idx in lists.items():
            idxd = torch.from_numpy(idx).to(cuda)
            want = ref.forward(x, idx, centre).view(np.uint32)
            back = ref.Backward(idx, g[:, out_c0:out_c0 + c], n)
            for path in (0, 1, 2):
                got = _forced(path, lambda: _fwd(xd, idxd, cd, point_major, out_c0 + c + 1, out_c0))
                assert np.array_equal(got.view(np.uint32), want), (c, point_major, relative, kind, path)
                gx, gc = _forced(path, lambda: _bwd(idxd, gd, n, c, point_major, out_c0))
                back.check_exact(gx, gc)


def _integer_gradient(rng, b, c, m, k, out_c0):
    """``g[b, out_c0 + c + 1, m, k]``: integers in [-8, 8] inside the slice, NaN around it (the backward must not read it)."""
    g = np.full((b, out_c0 + c + 1, m, k), np.nan, dtype=np.float32)
    g[:, out_c0:out_c0 + c] = rng.integers(-8, 9, size=(b, c, m, k))
    return g


@pytest.mark.parametrize('n', ref.N_GRID)
def test_backward_word_for_word(cuda, n):
    """Integer-valued gradients in [-8, 8]: every partial sum is an integer below 2^24, exact in any order.  The grid of the
    forward test, the origin of the list rotating, on both paths; points nothing refers to get +0.0."""
    x_all = ref.cloud(n, n)
    rng = np.random.default_rng(70 + n)
    lists = {}
    for m, k, c, point_major, _, b, out_c0, j in ref.grid():
        if (m, k) not in lists:
            lists[m, k] = _lists(cuda, 17 * m + k + n, x_all, n, m, k)
        kinds = sorted(lists[m, k])
        idx = lists[m, k][kinds[j % len(kinds)]][:b]
        g = _integer_gradient(rng, b, c, m, k, out_c0)
        back = ref.Backward(idx, g[:, out_c0:out_c0 + c], n)
        idxd, gd = torch.from_numpy(idx).to(cuda), torch.from_numpy(g).to(cuda)
        for path in (1, 2):
            gx, gc = _forced(path, lambda: _bwd(idxd, gd, n, c, point_major, out_c0))
            back.check_exact(gx, gc)


def test_backward_on_hubs_and_repeated_rows(cuda):
    """Every slot pointing at one point (m = 300, k = 64), and rows that are one index repeated (the pad-only rows of a
    ball query with one point inside): the runs a wave sums before it adds."""
    rng = np.random.default_rng(3)
    n, m, k, b, c = 500, 300, 64, 2, 9
    hub = np.full((b, m, k), 77, dtype=np.int64)
    hub[1] = 499
    rows = np.broadcast_to(rng.integers(0, n, size=(b, m, 1)), (b, m, k)).copy()
    mixed = rows.copy()
    mixed[:, ::3, :5] = np.sort(rng.integers(0, n, size=(b, len(range(0, m, 3)), 5)), axis=-1)  # ascending, then the pad
    mixed[:, 1::7, 40:] = -1
    for idx in (hub, rows, mixed):
        for point_major in (False, True):
            g = _integer_gradient(rng, b, c, m, k, 2)
            back = ref.Backward(idx, g[:, 2:2 + c], n)
            idxd, gd = torch.from_numpy(idx).to(cuda), torch.from_numpy(g).to(cuda)
            for path in (1, 2):
                gx, gc = _forced(path, lambda: _bwd(idxd, gd, n, c, point_major, 2))
                back.check_exact(gx, gc)


def test_backward_on_generic_gradients_is_inside_the_summation_bound(cuda):
    """Gaussian gradients: |got - ref64| <= gamma(deg) * sum |g_e| per bin of grad_x and gamma(k) per centre, the bound of
    a float32 sum in any order (tests/grouping_reference.py): derived, not tuned."""
    rng = np.random.default_rng(4)
    for n, m, k, c, b in ((65, 65, 33, 9, 3), (1025, 65, 32, 8, 2), (300, 300, 64, 3, 2), (2049, 65, 5, 5, 2)):
        lists = {'random': ref.random_list(n, b, n, m, k), 'first': ref.padded_list(n, b, n, m, k, 'first'),
                 'hub': np.full((b, m, k), n - 1, dtype=np.int64)}
        for kind, idx in lists.items():
            for point_major in (False, True):
                g = rng.standard_normal((b, c, m, k)).astype(np.float32)
                back = ref.Backward(idx, g, n)
                idxd, gd = torch.from_numpy(idx).to(cuda), torch.from_numpy(g).to(cuda)
                for path in (1, 2):
                    gx, gc = _forced(path, lambda: _bwd(idxd, gd, n, c, point_major))
                    back.check_bound(gx, gc)


def test_independence(cuda):
    """A batch against its clouds one by one and against a permuted batch; fewer centres equal the slice; either gradient
    alone; x aliasing centre (M = N, point-major)."""
    n, m, k, c, b = 1025, 300, 24, 9, 5
    rng = np.random.default_rng(6)
    x = ref.cloud(7, n, b, c)
    centre = rng.standard_normal((b, c, m)).astype(np.float32)
    idx = ref.padded_list(8, b, n, m, k, 'none')
    g = rng.integers(-8, 9, size=(b, c, m, k)).astype(np.float32)
    idxd, gd = torch.from_numpy(idx).to(cuda), torch.from_numpy(g).to(cuda)
    order = [2, 4, 0, 3, 1]
    for path in (0, 1, 2):
        for point_major in (False, True):
            xd, cd = _dev(x, cuda, point_major), _dev(centre, cuda, point_major)
            out = _forced(path, lambda: _fwd(xd, idxd, cd, point_major))
            assert np.array_equal(out.view(np.uint32), ref.forward(x, idx, centre).view(np.uint32))
            gx, gc = _forced(path, lambda: _bwd(idxd, gd, n, c, point_major))
            for i in (0, 2, 4):
                alone = _forced(path, lambda: _fwd(xd[i:i + 1], idxd[i:i + 1], cd[i:i + 1], point_major))
                assert np.array_equal(alone[0].view(np.uint32), out[i].view(np.uint32))
                ax, ac = _forced(path, lambda: _bwd(idxd[i:i + 1], gd[i:i + 1], n, c, point_major))
                assert np.array_equal(ax[0], gx[i]) and np.array_equal(ac[0], gc[i])
            moved = _forced(path, lambda: _fwd(xd[order].contiguous(), idxd[order].contiguous(), cd[order].contiguous(), point_major))
            assert np.array_equal(moved.view(np.uint32), out[order].view(np.uint32))
            sub = slice(7, 50)  # (another m: other slots, other alignment)
            csub = (cd[:, sub] if point_major else cd[:, :, sub]).contiguous()
            fewer = _forced(path, lambda: _fwd(xd, idxd[:, sub].contiguous(), csub, point_major))
            assert np.array_equal(fewer.view(np.uint32), out[:, :, sub].view(np.uint32))
            only_x = _forced(path, lambda: _bwd(idxd, gd, n, c, point_major, want_c=False))
            only_c = _forced(path, lambda: _bwd(idxd, gd, n, c, point_major, want_x=False))
            assert only_x[1] is None and only_c[0] is None
            assert np.array_equal(only_x[0], gx) and np.array_equal(only_c[1], gc)
        # the cloud as its own centres, the same memory: every row relative to its own point
        xyz = _dev(x[:, :3], cuda, True)
        self_idx = torch.from_numpy(ref.random_list(9, b, n, n, 4, bad=False)).to(cuda)
        aliased = _forced(path, lambda: _fwd(xyz, self_idx, xyz, True))
        copied = _forced(path, lambda: _fwd(xyz, self_idx, xyz.clone(), True))
        assert np.array_equal(aliased.view(np.uint32), copied.view(np.uint32))
        assert np.array_equal(aliased.view(np.uint32), ref.forward(x[:, :3], self_idx.cpu().numpy(), x[:, :3]).view(np.uint32))


def test_non_finite_input(cuda):
    """NaN (payloads included) and +-inf are copied bit for bit; the relative mode agrees up to the NaN's payload; a healthy
    cloud beside an all-NaN one is unaffected."""
    n, m, k, c, b = 300, 65, 8, 4, 3
    rng = np.random.default_rng(10)
    x = ref.cloud(11, n, b, c)
    words = x.view(np.uint32)
    words[0, :, ::7] = np.array([0x7fc12345, 0xffc00001, 0x7f800000, 0xff800000], dtype=np.uint32)[:, None]
    words[0, 1, 5] = 0x7f800001  # a signalling NaN
    x[1] = np.nan
    centre = rng.standard_normal((b, c, m)).astype(np.float32)
    centre[2, 0, 3] = np.inf
    idx = ref.random_list(12, b, n, m, k)
    idxd = torch.from_numpy(idx).to(cuda)
    for path in (0, 1, 2):
        for point_major in (False, True):
            xd, cd = _dev(x, cuda, point_major), _dev(centre, cuda, point_major)
            copy = _forced(path, lambda: _fwd(xd, idxd, None, point_major))
            assert np.array_equal(copy.view(np.uint32), ref.forward(x, idx).view(np.uint32))
            rel = _forced(path, lambda: _fwd(xd, idxd, cd, point_major))
            want = ref.forward(x, idx, centre)
            assert np.array_equal(rel, want, equal_nan=True) and np.array_equal(np.isnan(rel), np.isnan(want))
            assert np.array_equal(rel[2].view(np.uint32)[np.isfinite(want[2])], want[2].view(np.uint32)[np.isfinite(want[2])])
            alone = _forced(path, lambda: _fwd(xd[2:], idxd[2:], cd[2:], point_major))
            assert np.array_equal(alone[0], rel[2], equal_nan=True)


def test_arguments(cuda):
    from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops

    L = _lib.lib
    b, c, n, m, k = 2, 3, 300, 20, 8
    x = torch.from_numpy(ref.cloud(13, n, b, c)).to(cuda)
    centre = torch.randn(b, c, m, device=cuda)
    idx = torch.from_numpy(ref.random_list(14, b, n, m, k)).to(cuda)
    good = ops.group_points(x, idx, centre)
    out = torch.full((b, c, m, k), SENTINEL, device=cuda)
    gx, gc = torch.full((b, c, n), SENTINEL, device=cuda), torch.full((b, c, m), SENTINEL, device=cuda)
    xp, ip, cp, op, gxp, gcp = (t.data_ptr() for t in (x, idx, centre, out, gx, gc))
    stream = torch.cuda.current_stream(cuda).cuda_stream
    # (b, c, n, m, k, point_major, out_c, out_c0)
    sizes = (b, c, n, m, k, 0, c, 0)
    bad_sizes = [(-1, c, n, m, k, 0, c, 0), (65536, c, n, m, k, 0, c, 0), (b, 0, n, m, k, 0, c, 0), (b, c, 0, m, k, 0, c, 0),
                 (b, c, n, -1, k, 0, c, 0), (b, c, n, m, 0, 0, c, 0), (b, c, n, m, k, 2, c, 0), (b, c, n, m, k, 0, c - 1, 0),
                 (b, c, n, m, k, 0, c, 1), (b, c, n, m, k, 0, c, -1), (b, c, n, 1 << 16, 1 << 15, 0, c, 0)]
    for s in bad_sizes:
        assert L.pcc_group_points(*s[:6], xp, ip, cp, op, *s[6:], stream) != 0, s
        assert L.pcc_last_error().decode().startswith('group_points:')
        assert L.pcc_group_points_bwd(*s[:6], ip, op, *s[6:], gxp, gcp, stream) != 0, s
        assert L.pcc_last_error().decode().startswith('group_points_bwd:')
    for ptrs in ((None, ip, cp, op), (xp, None, cp, op), (xp, ip, cp, None)):
        assert L.pcc_group_points(*sizes[:6], *ptrs, *sizes[6:], stream) != 0
        assert L.pcc_last_error().decode().startswith('group_points:')
    for ptrs in ((None, op), (ip, None)):
        assert L.pcc_group_points_bwd(*sizes[:6], *ptrs, *sizes[6:], gxp, gcp, stream) != 0
        assert L.pcc_last_error().decode().startswith('group_points_bwd:')
    assert L.pcc_group_points_bwd(*sizes[:6], ip, op, *sizes[6:], None, None, stream) == 0  # no gradient asked for
    assert L.pcc_group_points(0, *sizes[1:6], xp, ip, cp, op, *sizes[6:], stream) == 0       # b = 0
    assert L.pcc_group_points_bwd(0, *sizes[1:6], ip, op, *sizes[6:], gxp, gcp, stream) == 0
    assert L.pcc_group_points(b, c, n, 0, k, 0, xp, None, None, None, c, 0, stream) == 0     # m = 0 forward
    torch.cuda.synchronize()
    for t in (out, gx, gc):
        assert (t == SENTINEL).all()  # nothing ran
    assert L.pcc_group_points_bwd(b, c, n, 0, k, 0, None, None, c, 0, gxp, None, stream) == 0  # m = 0: grad_x zero-filled
    torch.cuda.synchronize()
    assert (gx.cpu().numpy().view(np.uint32) == 0).all()
    # the Python layer: refusals before anything is allocated, empty calls, views
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.group_points(x, idx.cpu())
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.group_points(x, idx, centre.cpu())
    with pytest.raises(RuntimeError):
        ops.group_points(x.cpu(), idx)
    with pytest.raises(RuntimeError):
        ops.group_points(x.double(), idx)
    with pytest.raises(RuntimeError):
        ops.group_points(x, idx.int())
    with pytest.raises(ValueError):
        ops.group_points(x, idx, centre[:, :, :5])
    with pytest.raises(ValueError):
        ops.group_points(x, idx[:1])
    for eb, em in ((0, m), (b, 0)):
        xe = x[:eb].clone().requires_grad_(True)
        empty = ops.group_points(xe, idx[:eb, :em], centre[:eb, :, :em])
        assert empty.shape == (eb, c, em, k) and empty.dtype == torch.float32 and empty.device == x.device
        empty.sum().backward()
        assert xe.grad.shape == xe.shape and (xe.grad == 0).all()
    big = torch.from_numpy(ref.cloud(15, 2 * n, b, 2 * c)).to(cuda)
    view, iview = big[:, ::2, ::2], torch.cat((idx, idx), 2)[:, :, ::2]
    assert not view.is_contiguous() and not iview.is_contiguous()
    assert torch.equal(ops.group_points(view, iview), ops.group_points(view.contiguous(), iview.contiguous()))
    pm = x.transpose(1, 2)  # a point-major view of channels-major memory
    assert torch.equal(ops.group_points(pm, idx, centre.transpose(1, 2), point_major=True), good)
    assert torch.equal(ops.group_points(x, idx, centre), good)  # the library still answers


def test_group_points_is_differentiable_and_agrees_with_the_cpu_path(cuda):
    """``group_points`` through autograd on the device against its CPU path: forward word for word, the gradients of x and
    centres inside the summation bound; idx carries no gradient."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    n, m, k, c, b = 300, 37, 16, 5, 3
    rng = np.random.default_rng(16)
    x, centre = ref.cloud(17, n, b, c), rng.standard_normal((b, c, m)).astype(np.float32)
    idx = ref.padded_list(18, b, n, m, k, 'none')
    g = rng.standard_normal((b, c, m, k)).astype(np.float32)
    back = ref.Backward(idx, g, n)
    for point_major in (False, True):
        outs = []
        for dev in (cuda, torch.device('cpu')):
            tx = _dev(x, dev, point_major).requires_grad_(True)
            tc = _dev(centre, dev, point_major).requires_grad_(True)
            out = ops.group_points(tx, torch.from_numpy(idx).to(dev), tc, point_major=point_major)
            out.backward(torch.from_numpy(g).to(dev))
            back.check_bound(ref.to_layout(tx.grad.cpu().numpy(), point_major), ref.to_layout(tc.grad.cpu().numpy(), point_major))
            outs.append(out.detach().cpu().numpy().view(np.uint32))
        assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], ref.forward(x, idx, centre).view(np.uint32))
        only = _dev(x, cuda, point_major).requires_grad_(True)  # (x alone requires a gradient; no centres at all)
        ops.group_points(only, torch.from_numpy(idx).to(cuda), _dev(centre, cuda, point_major), point_major=point_major).backward(
            torch.from_numpy(g).to(cuda))
        back.check_bound(ref.to_layout(only.grad.cpu().numpy(), point_major))


@pytest.mark.parametrize('with_features', [True, False])
def test_sample_and_group(cuda, with_features):
    """Every output against the hand-written composition (farthest_point_sample, gather, ball_query, expand + gather +
    subtract + cat): word for word forward; the gradients of xyz (as neighbour and as centre: one float32 sum of
    deg + nsample terms for a sampled point) and of the features against float64 by the bound; the CPU path against the
    kernel word for word."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, n, m, nsample, c = 3, 300, 37, 16, 5
    rng = np.random.default_rng(19)
    xyz_np = rng.random((b, n, 3)).astype(np.float32)
    feat_np = rng.standard_normal((b, c, n)).astype(np.float32)
    for pad in ('first', 'none'):
        xyz = torch.from_numpy(xyz_np).to(cuda).requires_grad_(True)
        feat = torch.from_numpy(feat_np).to(cuda).requires_grad_(True) if with_features else None
        res = ops.sample_and_group(xyz, feat, m, 0.15, nsample, pad=pad)
        sel = ops.farthest_point_sample(xyz, m)
        centres = torch.gather(xyz.detach(), 1, sel[:, :, None].expand(-1, -1, 3))
        idx, cnt = ops.ball_query(xyz, centres, 0.15, nsample, pad=pad, return_count=True)
        assert torch.equal(res.sel, sel) and torch.equal(res.idx, idx) and torch.equal(res.cnt, cnt)
        assert torch.equal(res.centres.detach(), centres) and res.centres.requires_grad
        assert not (res.sel.requires_grad or res.idx.requires_grad or res.cnt.requires_grad)
        assert (cnt < nsample).any()
        safe = idx.clamp(min=0)  # (pad = 'none': the composition masks what the op zeroes)
        hand = (xyz.detach().gather(1, safe.reshape(b, m * nsample, 1).expand(-1, -1, 3)).view(b, m, nsample, 3)
                - centres[:, :, None, :]).permute(0, 3, 1, 2)
        if with_features:
            hand = torch.cat((hand, feat.detach().gather(2, safe.reshape(b, 1, m * nsample).expand(-1, c, -1)).view(b, c, m, nsample)), 1)
        hand = torch.where((idx >= 0)[:, None], hand, torch.zeros((), device=cuda))
        assert res.grouped.shape == hand.shape
        assert np.array_equal(res.grouped.detach().cpu().numpy().view(np.uint32), hand.cpu().numpy().view(np.uint32))
        cpu = ops.sample_and_group(torch.from_numpy(xyz_np), torch.from_numpy(feat_np) if with_features else None, m, 0.15, nsample, pad=pad)
        assert torch.equal(cpu.sel, sel.cpu()) and torch.equal(cpu.idx, idx.cpu()) and torch.equal(cpu.cnt, cnt.cpu())
        assert np.array_equal(cpu.grouped.numpy().view(np.uint32), res.grouped.detach().cpu().numpy().view(np.uint32))
        g = rng.standard_normal(tuple(hand.shape)).astype(np.float32)
        res.grouped.backward(torch.from_numpy(g).to(cuda))
        idx_np, sel_np = idx.cpu().numpy(), sel.cpu().numpy()
        back = ref.Backward(idx_np, g[:, :3], n)
        gxyz, gabs, deg = back.gx.copy(), back.gx_abs.copy(), back.deg.copy()
        for bi in range(b):
            np.add.at(gxyz[bi], (slice(None), sel_np[bi]), back.gc[bi])
            np.add.at(gabs[bi], (slice(None), sel_np[bi]), back.gc_abs[bi])
            np.add.at(deg[bi], sel_np[bi], nsample)
        got = xyz.grad.cpu().numpy().transpose(0, 2, 1)
        assert np.isfinite(got).all() and (np.abs(got - gxyz) <= ref.gamma(deg)[:, None, :] * gabs).all()
        if with_features:
            ref.Backward(idx_np, g[:, 3:], n).check_bound(gx=feat.grad.cpu().numpy())
