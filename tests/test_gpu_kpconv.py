"""GPU tests of the kernel point convolution (``pcc_kpconv_aggregate`` / ``pcc_kpconv_aggregate_bwd`` through the C ABI, and
``neighbour_ops.kpconv_aggregate`` / ``kernel_point_conv`` / ``KernelPointConv``) against the numpy reference of
tests/kpconv_reference.py: the forward word for word, grad_x word for word on the lattice geometry (influences of 0, 0.5
and 1) with integer gradients and inside the float32 summation bound on random inputs, both paths of the backward on either side
of every boundary of its dispatch, independence of the batch, non-finite input, autograd and the argument checks.  Every output
buffer starts as NaN: every element must be written.

The random-geometry inputs are clouds uniform in [0,1)^3, ``kernel_point_layout(kp, 0.5)`` and ``sigma = 0.6``.  A zero-skip
is exercised only if both kinds of pair occur, so each test on them asserts, on the reference's h over its cases with
random lists, that between 0.2 and 0.8 of the (valid slot, kernel point) pairs have h > 0.  (A searched list holds the
points nearest the centre: its share is whatever the search makes it.)"""

import numpy as np
import pytest
import torch

from tests import kpconv_reference as ref
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

KINDS = ('random', 'knn_cross', 'ball_none', 'ball_first')


def _forced(path, fn):
    from pointcloudcounterfactual_amd import _lib

    with _lib.tuning('interp_path', path):
        return fn()


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _nan(shape, dev):
    return torch.full(shape, float('nan'), dtype=torch.float32, device=dev)


def _fwd(x, xyz, centres, idx, kpts, sigma):
    """``pcc_kpconv_aggregate`` on device tensors, as numpy; ``out`` starts as NaN."""
    from pointcloudcounterfactual_amd import _lib

    b, c, n = x.shape
    m, k = idx.shape[1:]
    kp = kpts.shape[0]
    out = _nan((b, kp * c, m), x.device)
    _lib.call(_lib.lib.pcc_kpconv_aggregate, 'kpconv_aggregate', x.device, b, c, n, m, k, kp, _p(xyz), _p(centres), _p(idx), _p(x),
              _p(kpts), sigma, _p(out))
    return out.cpu().numpy()


def _bwd(xyz, centres, idx, kpts, sigma, go, c):
    """``pcc_kpconv_aggregate_bwd``: ``grad_x`` as numpy; it starts as NaN."""
    from pointcloudcounterfactual_amd import _lib

    b, n = xyz.shape[:2]
    m, k = idx.shape[1:]
    kp = kpts.shape[0]
    gx = _nan((b, c, n), go.device)
    _lib.call(_lib.lib.pcc_kpconv_aggregate_bwd, 'kpconv_aggregate_bwd', go.device, b, c, n, m, k, kp, _p(xyz), _p(centres), _p(idx),
              _p(kpts), sigma, _p(go), _p(gx))
    return gx.cpu().numpy()


def _expected_cb(b, c, n, cus):
    """The channel block of the backward's LDS path by the rule of its plan (``make_list_plan`` and
    ``ListPlan::spread_bins`` of chan_block.hpp): the largest of 8, 4, 2, 1 whose bins of n floats fit 64 KB (1 if none does), halved while there
    are fewer workgroups, ``b * ceil(c / cb)``, than compute units; None where one channel's bins exceed 160 KB (direct)."""
    cb = 8
    while cb > 1 and cb * n * 4 > 64 * 1024:
        cb //= 2
    if cb * n * 4 > 160 * 1024:
        return None
    while cb > 1 and b * -(-c // cb) < cus:
        cb //= 2
    return cb


def _bwd_variant(*args):
    """``_bwd(*args)`` and the variant that ran, from the library's launch profile: 'cb=1' ... 'cb=8' or 'direct'."""
    from pointcloudcounterfactual_amd import _lib

    with _lib.profile() as read:
        gx = _bwd(*args)
        ran = []
        for tag, name in [(f'cb={cb}', f'kp_bwd_kernel<lds> cb={cb}') for cb in (1, 2, 4, 8)] + [('direct', 'kp_bwd_kernel<direct>')]:
            ran += [tag] * read(name)[1]
    assert len(ran) == 1, ran
    return gx, ran[0]


_GEOMETRY = {}


def _geometry(cuda, lattice, seed, n, m, k):
    """``(xyz, centres, {origin: idx[B_MAX,m,k]})`` (made once per key): clouds uniform in [0,1)^3, or on the lattice; a random
    list with -1, n and 2^40 in it, the ``knn_cross`` list of the centres into the cloud (where k <= n), and the
    ``ball_query`` lists around them with ``pad='none'`` and ``pad='first'``."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    key = (lattice, seed, n, m, k)
    if key not in _GEOMETRY:
        if lattice:
            xyz, centres, _ = ref.lattice_geometry(seed, ref.B_MAX, n, m, 1)
        else:
            xyz, centres = ref.uniform_geometry(seed, ref.B_MAX, n, m)
        lists = {'random': ref.random_list(seed, ref.B_MAX, n, m, k)}
        xd, qd = _dev(xyz, cuda), _dev(centres, cuda)
        if k <= n:
            lists['knn_cross'] = ops.knn_cross(qd.transpose(1, 2).contiguous(), xd.transpose(1, 2).contiguous(), k).cpu().numpy()
        for pad in ('none', 'first'):
            lists['ball_' + pad] = ops.ball_query(xd, qd, 2.5 if lattice else 0.4, k, pad=pad).cpu().numpy()
        _GEOMETRY[key] = xyz, centres, lists
    return _GEOMETRY[key]


def _pick(lists, j):
    """The origin of the list rotates with the running number of the grid, one step further at every (m, k)."""
    kinds = [kind for kind in KINDS if kind in lists]
    kind = kinds[(j + j // len(ref.CKP_GRID)) % len(kinds)]
    return kind, lists[kind]


class _Share:
    """The share of positive pairs over the cases of a test that are added."""

    def __init__(self):
        self.pos = self.tot = 0

    def add(self, h, idx, n):
        valid = ref.valid_slots(idx, n)
        self.pos += int((h[valid] > 0).sum())
        self.tot += int(valid.sum()) * h.shape[3]

    def check(self, lo=0.2, hi=0.8):
        assert self.tot and lo <= self.pos / self.tot <= hi, (self.pos, self.tot)


# ---- the words the contract fixes ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('n', ref.N_GRID)
def test_forward_word_for_word(cuda, n):
    """Every m, k and (c, kp) of the grid, b and the origin of the list rotating, on the random-geometry inputs."""
    x_all = ref.cloud(n, n, ref.B_MAX, ref.C_MAX)
    share = _Share()
    for m, k, c, kp, b, j in ref.grid():
        xyz, centres, lists = _geometry(cuda, False, 17 * m + k + n, n, m, k)
        kind, idx = _pick(lists, j)
        xyz, centres, idx, x = xyz[:b], centres[:b], idx[:b], np.ascontiguousarray(x_all[:b, :c])
        kpts = ref.layout(kp, ref.RADIUS)
        want, h = ref.kpconv(x, xyz, centres, idx, kpts, ref.SIGMA)
        if kind == 'random':
            share.add(h, idx, n)
        got = _fwd(*(_dev(a, cuda) for a in (x, xyz, centres, idx, kpts)), ref.SIGMA)
        assert ref.same_words(got, want), (m, k, c, kp, b, kind)
    share.check()


@pytest.mark.parametrize('n', ref.N_GRID)
def test_grad_x_word_for_word_on_the_lattice(cuda, n):
    """The lattice geometry (every influence 0, 0.5 or 1) with integer gradients in [-8, 8]: every word p and every partial
    sum is exact in any order.  The grid of the forward test on both paths; points nothing refers to get the word 0."""
    rng = np.random.default_rng(70 + n)
    seen = set()
    for m, k, c, kp, b, j in ref.grid():
        xyz, centres, lists = _geometry(cuda, True, 17 * m + k + n, n, m, k)
        kind, idx = _pick(lists, j)
        xyz, centres, idx = xyz[:b], centres[:b], idx[:b]
        kpts = ref.lattice_geometry(j, 1, 1, 1, kp)[2]
        go = rng.integers(-8, 9, size=(b, kp * c, m)).astype(np.float32)
        h = ref.influence(xyz, centres, idx, kpts, 2.0)
        seen.update(np.unique(h).tolist())
        back = ref.GradX(idx, ref.slot_words(h, go, c), n)
        args = tuple(_dev(a, cuda) for a in (xyz, centres, idx, kpts))
        god = _dev(go, cuda)
        for path in (1, 2):
            back.check_exact(_forced(path, lambda: _bwd(*args, 2.0, god, c)))
    assert seen == {0.0, 0.5, 1.0}


def test_grad_x_on_random_inputs_is_inside_the_summation_bound(cuda):
    """Gaussian gradients on the random-geometry inputs: |got - sum64 p| <= gamma(deg) * sum |p| per bin with p the
    reference's float32 words -- the bound of a float32 sum of deg terms in any order (the merged runs are such an order):
    derived, not tuned.  A list that names one point throughout ('hub') is one long run."""
    rng = np.random.default_rng(4)
    worst = 0.0
    share = _Share()
    for n, m, k, c, kp, b in ((65, 257, 5, 9, 15, 3), (1025, 257, 16, 8, 15, 2), (300, 300, 3, 3, 2, 2), (2049, 65, 64, 5, 32, 2),
                              (3, 257, 17, 1, 1, 3)):
        xyz, centres = ref.uniform_geometry(n, b, n, m)
        kpts = ref.layout(kp, ref.RADIUS)
        for kind, idx in (('random', ref.random_list(n, b, n, m, k)), ('hub', np.full((b, m, k), n - 1, dtype=np.int64))):
            go = rng.standard_normal((b, kp * c, m)).astype(np.float32)
            h = ref.influence(xyz, centres, idx, kpts, ref.SIGMA)
            if kind == 'random':
                share.add(h, idx, n)
            back = ref.GradX(idx, ref.slot_words(h, go, c), n)
            args = tuple(_dev(a, cuda) for a in (xyz, centres, idx, kpts))
            god = _dev(go, cuda)
            for path in (1, 2):
                ratio = back.ratio(_forced(path, lambda: _bwd(*args, ref.SIGMA, god, c)))
                worst = max(worst, ratio)
                assert ratio <= 1.0, (n, kind, path)
    share.check()
    print(f'grad_x: the largest error is {worst:.3f} of the bound')


@pytest.mark.parametrize('sigma,lo,hi', ((0.3, 0.02, 0.2), (1.0, 0.7, 0.98)))
def test_a_small_and_a_large_extent(cuda, sigma, lo, hi):
    """sigma = 0.3: few pairs are positive and most rows of the output are empty; sigma = 1.0: most pairs are.  Either way
    there are pairs to sum and pairs to skip."""
    b, c, n, m, k, kp = 2, 9, 500, 300, 16, 15
    xyz, centres = ref.uniform_geometry(5, b, n, m)
    x, idx, kpts = ref.cloud(6, n, b, c), ref.random_list(7, b, n, m, k), ref.layout(kp, ref.RADIUS)
    want, h = ref.kpconv(x, xyz, centres, idx, kpts, sigma)
    share = _Share()
    share.add(h, idx, n)
    share.check(lo, hi)
    go = ref.gaussian(8, (b, kp * c, m))
    back = ref.GradX(idx, ref.slot_words(h, go, c), n)
    xd, *args = (_dev(a, cuda) for a in (x, xyz, centres, idx, kpts))
    for path in (1, 2):
        assert ref.same_words(_forced(path, lambda: _fwd(xd, *args, sigma)), want)
        assert back.ratio(_forced(path, lambda: _bwd(*args, sigma, _dev(go, cuda), c))) <= 1.0


def test_long_lists_and_many_blocks(cuda):
    """Units of several passes, lists split over several workgroups and more units than one sample's, on both paths."""
    rng = np.random.default_rng(21)
    share = _Share()
    for b, c, n, m, k, kp in ((2, 16, 300, 5003, 16, 15), (4, 64, 64, 2048, 5, 2), (1, 9, 16385, 2100, 128, 32)):
        x, idx = ref.cloud(22, n, b, c), ref.random_list(23, b, n, m, k)
        xyz, centres = ref.uniform_geometry(24, b, n, m)
        want, h = ref.kpconv(x, xyz, centres, idx, ref.layout(kp, ref.RADIUS), ref.SIGMA)
        share.add(h, idx, n)
        lxyz, lcentres, lkpts = ref.lattice_geometry(25, b, n, m, kp)
        go = rng.integers(-8, 9, size=(b, kp * c, m)).astype(np.float32)
        back = ref.GradX(idx, ref.slot_words(ref.influence(lxyz, lcentres, idx, lkpts, 2.0), go, c), n)
        xd, idxd, god = _dev(x, cuda), _dev(idx, cuda), _dev(go, cuda)
        fwd_args = (_dev(xyz, cuda), _dev(centres, cuda), idxd, _dev(ref.layout(kp, ref.RADIUS), cuda))
        bwd_args = (_dev(lxyz, cuda), _dev(lcentres, cuda), idxd, _dev(lkpts, cuda))
        for path in (1, 2):
            assert ref.same_words(_forced(path, lambda: _fwd(xd, *fwd_args, ref.SIGMA)), want), (n, path)
            back.check_exact(_forced(path, lambda: _bwd(*bwd_args, 2.0, god, c)))
    share.check()


# ---- both paths ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('n', ref.BOUNDARIES)
def test_every_variant_gives_the_same_words(cuda, n):
    """The backward's LDS path (1) and direct path (2) forced against the product's choice, and that against the reference,
    on the lattice with integer gradients; the forward, which has one path and ignores the switch, on the random-geometry
    inputs at the same n.  At this narrow batch the plan halves every channel block down to one channel, so among these n
    only 40960 / 40961 changes the variant (a row of bins no longer fits: the forced LDS path is ignored); the channel
    blocks of 8, 4 and 2 are ``test_backward_with_bins_of_several_channels``'s."""
    m, k, b = 65, 3, 2
    x_all = ref.cloud(n, n, b, 9)
    rng = np.random.default_rng(n)
    idx = ref.random_list(n, b, n, m, k)
    xyz, centres = ref.uniform_geometry(n + 1, b, n, m)
    share = _Share()
    idxd, xyzd, centresd = (_dev(a, cuda) for a in (idx, xyz, centres))
    for c, kp in ((9, 15), (3, 2), (8, 32)):
        x = np.ascontiguousarray(x_all[:, :c])
        kpts = ref.layout(kp, ref.RADIUS)
        want, h = ref.kpconv(x, xyz, centres, idx, kpts, ref.SIGMA)
        share.add(h, idx, n)
        lxyz, lcentres, lkpts = ref.lattice_geometry(n + c, b, n, m, kp)
        go = rng.integers(-8, 9, size=(b, kp * c, m)).astype(np.float32)
        back = ref.GradX(idx, ref.slot_words(ref.influence(lxyz, lcentres, idx, lkpts, 2.0), go, c), n)
        xd, kd, god = _dev(x, cuda), _dev(kpts, cuda), _dev(go, cuda)
        bwd_args = (_dev(lxyz, cuda), _dev(lcentres, cuda), idxd, _dev(lkpts, cuda))
        for path in (0, 1, 2):
            assert ref.same_words(_forced(path, lambda: _fwd(xd, xyzd, centresd, idxd, kd, ref.SIGMA)), want), (c, path)
            gx, ran = _forced(path, lambda: _bwd_variant(*bwd_args, 2.0, god, c))
            assert ran == ('direct' if path == 2 or n > 40960 else 'cb=1'), (c, path, ran)
            back.check_exact(gx)
    share.check()


def _lattice_backward(cuda, seed, b, c, n, m, k, kp):
    """Lattice inputs with integer gradients for the backward alone: the exact reference and the device arguments."""
    xyz, centres, kpts = ref.lattice_geometry(seed, b, n, m, kp)
    idx = ref.random_list(seed + 1, b, n, m, k)
    go = np.random.default_rng(seed + 2).integers(-8, 9, size=(b, kp * c, m)).astype(np.float32)
    h = ref.influence(xyz, centres, idx, kpts, 2.0)
    assert (h == 0.5).any() and (h == 1.0).any()
    back = ref.GradX(idx, ref.slot_words(h, go, c), n)
    return back, tuple(_dev(a, cuda) for a in (xyz, centres, idx, kpts)), _dev(go, cuda)


@pytest.mark.parametrize('n', (2048, 2049, 4096, 4097, 8192, 8193))
def test_backward_with_bins_of_several_channels(cuda, n):
    """A batch wide enough for the channel blocks of 8, 4 and 2 to survive the halving (32 clouds of 65 channels: 288, 544
    and 1056 workgroups), with a last block of one channel: ``grad_x`` exact on the lattice on either side of every n where
    the block steps down.  The block that ran is read from the library's launch profile and must be the plan's."""
    b, c, m, k, kp = 32, 65, 17, 3, 15
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    want_cb = _expected_cb(b, c, n, cus)
    if cus <= 288:  # (every MI355X: the blocks this test is about)
        assert want_cb == {2048: 8, 2049: 4, 4096: 4, 4097: 2, 8192: 2, 8193: 1}[n]
    back, args, god = _lattice_backward(cuda, n, b, c, n, m, k, kp)
    for path, want in ((0, f'cb={want_cb}'), (1, f'cb={want_cb}'), (2, 'direct')):
        gx, ran = _forced(path, lambda: _bwd_variant(*args, 2.0, god, c))
        assert ran == want, (path, ran, want)
        back.check_exact(gx)


def test_backward_either_side_of_the_halving(cuda):
    """The plan halves the channel block while there are fewer workgroups than compute units: the smallest batch that
    keeps 8 channels of 63 per workgroup at n = 2048, the batch one cloud short of it, and a batch that halves down to one
    channel; a last block of 7, 3 and 1 channels."""
    c, n, m, k, kp = 63, 2048, 33, 5, 15
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    keep = -(-cus // 8)  # b * ceil(63 / 8) >= cus
    seen = []
    for b in (keep, keep - 1, 2):
        want_cb = _expected_cb(b, c, n, cus)
        seen.append(want_cb)
        back, args, god = _lattice_backward(cuda, 7 * b, b, c, n, m, k, kp)
        gx, ran = _bwd_variant(*args, 2.0, god, c)
        assert ran == f'cb={want_cb}', (b, ran, want_cb)
        back.check_exact(gx)
    assert seen[0] == 8 and seen[1] in (2, 4) and seen[2] == 1, seen


# ---- independence of the batch -------------------------------------------------------------------------------------------------


def test_words_do_not_depend_on_the_batch(cuda):
    """A batch against its samples one by one and against a permuted batch; a prefix of m against the slice of the full m;
    the forward on the random-geometry inputs, grad_x on the lattice."""
    b, c, n, m, k, kp = 5, 9, 40, 300, 17, 15
    x, idx = ref.cloud(1, n, b, c), ref.random_list(2, b, n, m, k)
    xyz, centres = ref.uniform_geometry(3, b, n, m)
    kpts = ref.layout(kp, ref.RADIUS)
    want, h = ref.kpconv(x, xyz, centres, idx, kpts, ref.SIGMA)
    share = _Share()
    share.add(h, idx, n)
    share.check()
    lxyz, lcentres, lkpts = ref.lattice_geometry(4, b, n, m, kp)
    go = np.random.default_rng(5).integers(-8, 9, size=(b, kp * c, m)).astype(np.float32)
    xd, xyzd, centresd, idxd, kd = (_dev(a, cuda) for a in (x, xyz, centres, idx, kpts))
    lxd, lcd, lkd, god = (_dev(a, cuda) for a in (lxyz, lcentres, lkpts, go))
    out = _fwd(xd, xyzd, centresd, idxd, kd, ref.SIGMA)
    assert ref.same_words(out, want)
    gx = _bwd(lxd, lcd, idxd, lkd, 2.0, god, c)
    ref.GradX(idx, ref.slot_words(ref.influence(lxyz, lcentres, idx, lkpts, 2.0), go, c), n).check_exact(gx)
    for i in (0, 2, 4):
        s = slice(i, i + 1)
        assert ref.same_words(_fwd(xd[s], xyzd[s], centresd[s], idxd[s], kd, ref.SIGMA)[0], out[i])
        assert ref.same_words(_bwd(lxd[s], lcd[s], idxd[s], lkd, 2.0, god[s], c)[0], gx[i])
    order = [2, 4, 0, 3, 1]
    perm = lambda t: t[order].contiguous()  # noqa: E731
    assert ref.same_words(_fwd(perm(xd), perm(xyzd), perm(centresd), perm(idxd), kd, ref.SIGMA), out[order])
    assert ref.same_words(_bwd(perm(lxd), perm(lcd), perm(idxd), lkd, 2.0, perm(god), c), gx[order])
    for pre in (1, 43, 128):
        cut = lambda t: t[:, :pre].contiguous()  # noqa: E731
        assert ref.same_words(_fwd(xd, xyzd, cut(centresd), cut(idxd), kd, ref.SIGMA), out[:, :, :pre])
        part = ref.GradX(idx[:, :pre], ref.slot_words(ref.influence(lxyz, lcentres[:, :pre], idx[:, :pre], lkpts, 2.0), go[:, :, :pre], c), n)
        part.check_exact(_bwd(lxd, cut(lcd), cut(idxd), lkd, 2.0, god[:, :, :pre].contiguous(), c))


# ---- non-finite input ----------------------------------------------------------------------------------------------------------


def test_non_finite_input(cuda):
    """NaN and +-inf among the coordinates, the centres, the features and the gradients: a NaN or infinite distance gives
    h = 0, a feature word under h = 0 does not spread, elsewhere IEEE holds and a NaN result is the word 0x7fc00000; a
    healthy cloud beside an all-NaN one is unaffected."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    n, m, k, c, kp, b = 300, 128, 4, 6, 15, 3
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0], dtype=np.float32)
    x = ref.cloud(11, n, b, c)
    x[0, :5, ::7] = special[:, None]
    x[1] = np.nan
    xyz, centres = ref.uniform_geometry(12, b, n, m)
    xyz[0, ::11, 0] = special[np.arange(len(range(0, n, 11))) % 3]
    xyz[2, 5::13, 2] = np.inf
    centres[0, ::9, 1] = special[np.arange(len(range(0, m, 9))) % 3]
    idx, kpts = ref.random_list(13, b, n, m, k), ref.layout(kp, ref.RADIUS)
    want, h = ref.kpconv(x, xyz, centres, idx, kpts, ref.SIGMA)
    assert np.isfinite(h).all() and (h[0, ::9] == 0).all()
    share = _Share()
    share.add(h, idx, n)
    share.check()
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any() and np.isfinite(want[2]).all()
    empty = ~(h[1] > 0).any(1).T  # [kp, m]: the rows of the all-NaN cloud no pair reaches
    assert ((want[1].reshape(kp, c, m).view(np.uint32) == 0) == empty[:, None, :]).all()
    go = ref.gaussian(15, (b, kp * c, m))
    go[2, 1, ::9] = np.inf
    go[0, 3] = np.nan
    p = ref.slot_words(h, go, c)
    assert not np.isfinite(p).all()
    xd, *args = (_dev(a, cuda) for a in (x, xyz, centres, idx, kpts))
    # a bin a non-finite word reaches is not finite; every other bin is inside the bound of its float32 sum
    dirty = ref.GradX(idx, (~np.isfinite(p)).astype(np.float32), n).gx > 0
    back = ref.GradX(idx, np.where(np.isfinite(p), p, np.float32(0)), n)
    bound = ref.gamma(back.deg)[:, None, :] * back.gx_abs
    assert dirty.any() and not dirty.all()
    for path in (1, 2):
        assert ref.same_words(_forced(path, lambda: _fwd(xd, *args, ref.SIGMA)), want)
        gx = _forced(path, lambda: _bwd(*args, ref.SIGMA, _dev(go, cuda), c))
        assert not np.isfinite(gx[dirty]).any() and np.isfinite(gx[~dirty]).all()
        assert (np.abs(gx - back.gx)[~dirty] <= bound[~dirty]).all()
    cpu = ops.kpconv_aggregate(*(torch.from_numpy(a) for a in (x, xyz, centres, idx, kpts)), ref.SIGMA).numpy()
    assert ref.same_words(cpu, want)


# ---- autograd and composition ----------------------------------------------------------------------------------------------------


def test_autograd_and_composition(cuda):
    """``kpconv_aggregate`` with and without a gradient, ``kernel_point_conv`` against ``torch.einsum`` over the op's own
    output, one forward and backward of ``KernelPointConv`` behind FPS and ``ball_query(pad='none')``."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, n, m, k, kp, o = 2, 18, 700, 130, 16, 15, 7
    x, (xyz, _) = ref.cloud(30, n, b, c), ref.uniform_geometry(31, b, n, m)
    xd, xyzd = _dev(x, cuda), _dev(xyz, cuda)
    centresd = torch.gather(xyzd, 1, ops.farthest_point_sample(xyzd, m)[:, :, None].expand(-1, -1, 3))
    idxd = ops.ball_query(xyzd, centresd, 0.25, k, pad='none')
    kd = ops.kernel_point_layout(kp, 0.25).to(cuda)
    sigma = 0.25 / 2.5
    idx, centres, kpts = idxd.cpu().numpy(), centresd.cpu().numpy(), kd.cpu().numpy()
    assert (idx == -1).any()
    want, h = ref.kpconv(x, xyz, centres, idx, kpts, sigma)
    tx = xd.clone().requires_grad_(True)
    out = ops.kpconv_aggregate(tx, xyzd, centresd, idxd, kd, sigma)
    assert out.requires_grad and ref.same_words(out.detach().cpu().numpy(), want)
    go = ref.gaussian(32, (b, kp * c, m))
    out.backward(_dev(go, cuda))
    assert ref.GradX(idx, ref.slot_words(h, go, c), n).ratio(tx.grad.cpu().numpy()) <= 1.0
    plain = ops.kpconv_aggregate(xd, xyzd, centresd, idxd, kd, sigma)
    assert not plain.requires_grad and torch.equal(plain, out.detach())
    assert torch.equal(ops.hip_kpconv_aggregate(xd, xyzd, centresd, idxd, kd, sigma), plain)

    torch.manual_seed(0)
    weight, bias = torch.randn(kp, c, o, device=cuda, requires_grad=True), torch.randn(o, device=cuda, requires_grad=True)
    got = ops.kernel_point_conv(tx, xyzd, centresd, idxd, kd, sigma, weight, bias)
    agg = plain.view(b, kp, c, m).double()
    ref64 = torch.einsum('btcm,tco->bom', agg, weight.double()) + bias.double()[None, :, None]
    mag = torch.einsum('btcm,tco->bom', agg.abs(), weight.double().abs()) + bias.double().abs()[None, :, None]
    # a float32 dot product of kp * c terms in any order, and the bias
    assert got.shape == (b, o, m) and ((got.double() - ref64).abs() <= ref.gamma(kp * c + 1) * mag).all()
    tx.grad = None
    got.sum().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in (tx, weight, bias))

    layer = ops.KernelPointConv(c, o, sigma=sigma, radius=0.25, bias=True).to(cuda)
    assert layer.kernel_points.device.type == 'cuda' and torch.equal(layer.kernel_points, kd)
    y = layer(tx, xyzd, centresd, idxd)
    assert torch.equal(y, ops.kernel_point_conv(tx, xyzd, centresd, idxd, kd, sigma, layer.weight, layer.bias))
    y.square().sum().backward()
    assert layer.weight.grad.abs().sum() > 0 and layer.bias.grad.abs().sum() > 0 and torch.isfinite(layer.weight.grad).all()


# ---- the argument checks through the binding -----------------------------------------------------------------------------------


def test_einval_messages_and_empty_calls(cuda):
    from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops
    from tests.util import raised

    L = _lib.lib
    b, c, n, m, k, kp = 2, 6, 50, 20, 4, 5
    x, idx = _dev(ref.cloud(1, n, b, c), cuda), _dev(ref.random_list(2, b, n, m, k), cuda)
    xyz, centres = (_dev(a, cuda) for a in ref.uniform_geometry(3, b, n, m))
    kpts = _dev(ref.layout(kp, ref.RADIUS), cuda)
    SENT = -1234.5
    out, gx = torch.full((b, kp * c, m), SENT, device=cuda), torch.full((b, c, n), SENT, device=cuda)
    P = {name: t.data_ptr() for name, t in {'x': x, 'idx': idx, 'xyz': xyz, 'centres': centres, 'kpts': kpts, 'out': out, 'gx': gx}.items()}

    def entries(b, c, n, m, k, kp, sigma):
        return (('kpconv_aggregate', L.pcc_kpconv_aggregate,
                 (b, c, n, m, k, kp, P['xyz'], P['centres'], P['idx'], P['x'], P['kpts'], sigma, P['out'])),
                ('kpconv_aggregate_bwd', L.pcc_kpconv_aggregate_bwd,
                 (b, c, n, m, k, kp, P['xyz'], P['centres'], P['idx'], P['kpts'], sigma, P['out'], P['gx'])))

    cases = [((-1, c, n, m, k, kp, 1.0), 'bad size'), ((b, c, 0, m, k, kp, 1.0), 'bad size'), ((b, c, n, m, 0, kp, 1.0), 'bad size'),
             ((65536, c, n, m, k, kp, 1.0), 'batch too large'), ((b, c, n, 1 << 16, 1 << 15, kp, 1.0), 'list too long (m * k >= 2^31)'),
             ((b, c, n, m, 129, 0, 0.0), 'kernel points must be 1..32'), ((b, c, n, m, k, 33, 1.0), 'kernel points must be 1..32'),
             ((b, c, n, m, 129, kp, 0.0), 'k > 128'), ((b, c, n, m, k, kp, 0.0), 'sigma must be finite and > 0'),
             ((b, c, n, m, k, kp, float('inf')), 'sigma must be finite and > 0'), ((b, c, n, m, k, kp, float('nan')), 'sigma must be finite and > 0')]
    for sizes, text in cases:
        for name, fn, args in entries(*sizes):
            assert raised(RuntimeError, _lib.call, fn, name, cuda, *args) == f'{name}: {name}: {text}'
    for name, fn, args in entries(0, c, n, m, k, kp, 1.0) + entries(b, c, n, 0, k, kp, 1.0)[:1]:
        _lib.call(fn, name, cuda, *args)  # an empty batch; an empty list forward
    torch.cuda.synchronize()
    assert (out == SENT).all() and (gx == SENT).all()  # nothing ran
    name, fn, args = entries(b, c, n, 0, k, kp, 1.0)[1]
    _lib.call(fn, name, cuda, *args)  # m = 0: grad_x zero-filled
    torch.cuda.synchronize()
    assert (gx.cpu().numpy().view(np.uint32) == 0).all() and (out == SENT).all()
    # the Python layer: refusals before anything is allocated, empty calls
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.kpconv_aggregate(x, xyz, centres, idx.cpu(), kpts, 1.0)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.kpconv_aggregate(x, xyz, centres, idx, kpts.cpu(), 1.0)
    with pytest.raises(ValueError, match='sigma must be a finite number > 0'):
        ops.kpconv_aggregate(x, xyz, centres, idx, kpts, 0.0)
    weight = torch.randn(kp, c, 3, device=cuda)
    for bb, mm in ((0, m), (b, 0)):
        t = ops.kernel_point_conv(x[:bb].clone().requires_grad_(True), xyz[:bb], centres[:bb, :mm], idx[:bb, :mm], kpts, 1.0, weight)
        assert t.shape == (bb, 3, mm)
        t.sum().backward()
    got = ops.kpconv_aggregate(x, xyz, centres, idx, kpts, ref.SIGMA).cpu().numpy()
    assert ref.same_words(got, ref.kpconv(*(t.cpu().numpy() for t in (x, xyz, centres, idx, kpts)), ref.SIGMA)[0])  # the library still answers
