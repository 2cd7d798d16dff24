"""CPU tests of the kernel point convolution (``neighbour_ops.kernel_point_layout`` / ``kernel_point_influence`` /
``kpconv_aggregate`` / ``kernel_point_conv`` / ``KernelPointConv``): the numpy reference (tests/kpconv_reference.py) against
closed forms, against the interpolation reference and against a float64 autograd composition; the torch path of CPU
tensors against that reference, word for word; the rules for zero influences and non-finite input; every argument error;
the ABI and the header."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import interpolate_reference as iref
from tests import kpconv_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pcc_kpconv_aggregate', 'pcc_kpconv_aggregate_bwd')


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _random_case(seed, b, c, n, m, k, kp):
    """The random-geometry inputs: clouds uniform in [0,1)^3, a random list with -1, n and 2^40 in it, the default layout."""
    xyz, centres = ref.uniform_geometry(seed, b, n, m)
    return ref.cloud(seed + 1, n, b, c), xyz, centres, ref.random_list(seed + 2, b, n, m, k), ref.layout(kp, ref.RADIUS)


# ---- the reference against closed forms ------------------------------------------------------------------------------------


def test_reference_a_neighbour_on_a_kernel_point_passes_its_features_through():
    """The neighbour of centre i sits exactly on kernel point t = i: h = 1 there, and out[t * c + ch, i] = x[ch, idx]."""
    kp, c, n = 5, 3, 7
    kpts = np.array([[0, 0, 0], [.5, 0, 0], [0, -.25, 0], [0, 0, 1.5], [1, 1, -1]], dtype=np.float32)
    centres = np.random.default_rng(0).integers(-4, 5, size=(1, kp, 3)).astype(np.float32)
    idx = np.array([[[3], [0], [6], [2], [5]]], dtype=np.int64)
    xyz = np.full((1, n, 3), 100.0, dtype=np.float32)
    xyz[0, idx[0, :, 0]] = centres[0] + kpts  # (exact: quarters of small integers)
    x = ref.cloud(1, n, 1, c)
    for dtype in (np.float32, np.float64):
        out, h = ref.kpconv(x, xyz, centres, idx, kpts, 0.75, dtype)
        for t in range(kp):
            assert h[0, t, 0, t] == 1.0
            assert np.array_equal(out[0, t * c:(t + 1) * c, t], x[0, :, idx[0, t, 0]].astype(dtype))


def test_reference_influences_on_the_lattice_are_one_a_half_or_zero():
    """Integer coordinates and sigma = 2: an offset of length 0, 1 or >= 2 from a kernel point gives exactly 1, 0.5 or 0."""
    b, n, m, k, kp = 2, 40, 30, 6, 9
    xyz, centres, kpts = ref.lattice_geometry(3, b, n, m, kp)
    idx = ref.random_list(4, b, n, m, k)
    h = ref.influence(xyz, centres, idx, kpts, 2.0)
    valid = ref.valid_slots(idx, n)
    e = (xyz[np.arange(b)[:, None, None], np.where(valid, idx, 0)] - centres[:, :, None])[:, :, :, None] - kpts  # [B,M,k,K,3]
    length2 = (e.astype(np.int64) ** 2).sum(-1)
    want = np.select([length2 == 0, length2 == 1], [1.0, 0.5], 0.0) * valid[..., None]
    assert np.array_equal(h, want.astype(np.float32)) and not np.signbit(h).any()
    assert all((h == v).any() for v in (0.0, 0.5, 1.0))
    assert set(np.unique(length2)) >= {0, 1, 4} and 2 not in length2 and 3 not in length2
    assert np.array_equal(ref.influence(xyz, centres, idx, kpts, 2.0, np.float64), want)


def test_reference_one_kernel_point_with_positive_influences_is_the_interpolation():
    """kp = 1 at the origin and an extent beyond the cube's diagonal: every h > 0, and the forward is, word for word,
    ``pcc_interpolate``'s with the weights h."""
    for seed, (b, c, n, m, k) in enumerate(((3, 9, 65, 33, 5), (2, 8, 7, 65, 16), (1, 1, 1, 3, 1))):
        x, xyz, centres, idx, _ = _random_case(seed, b, c, n, m, k, 1)
        out, h = ref.kpconv(x, xyz, centres, idx, np.zeros((1, 3), dtype=np.float32), 4.0)
        assert (h[ref.valid_slots(idx, n)] > 0).all()
        assert ref.same_words(out, iref.forward(x, idx, h[..., 0]))


def test_reference_gradient_against_float64_autograd():
    """``grad_x`` of the float32 words against torch's float64 autograd of the composition ``sum_j h x_j``.  The bar, per
    bin: h is off by at most 32 * 2^-24 in absolute terms on the unit cube (a rounding in each of r, e, the three products,
    the two sums, the root, the product and the difference, at magnitudes below 2.3, times 1 / sigma = 1.67), and the
    float32 sum over the kernel points adds (kp + 2) roundings relative to the absolute sum."""
    b, c, n, m, k, kp = 2, 6, 40, 17, 5, 15
    x, xyz, centres, idx, kpts = _random_case(20, b, c, n, m, k, kp)
    go = ref.gaussian(24, (b, kp * c, m))
    h64 = ref.influence(xyz, centres, idx, kpts, ref.SIGMA, np.float64)
    valid = _t(ref.valid_slots(idx, n))
    safe = torch.where(valid, _t(idx), torch.zeros((), dtype=torch.int64))
    tx = _t(x).double().requires_grad_(True)
    v = torch.gather(tx, 2, safe.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)
    out = torch.einsum('bmjt,bcmj->btcm', _t(h64), v).reshape(b, kp * c, m)
    out64, _ = ref.kpconv(x, xyz, centres, idx, kpts, ref.SIGMA, np.float64)
    assert np.abs(out.detach().numpy() - out64).max() <= 1e-12
    out.backward(_t(go).double())
    h32 = ref.influence(xyz, centres, idx, kpts, ref.SIGMA)
    assert np.abs(h32 - h64).max() <= 32 * ref.U
    back = ref.GradX(idx, ref.slot_words(h32, go, c), n)
    abs64 = ref.GradX(idx, ref.slot_words(h64, np.abs(go), c), n).gx
    reach = ref.GradX(idx, ref.slot_words(np.ones_like(h64), np.abs(go), c), n).gx
    assert (np.abs(back.gx - tx.grad.numpy()) <= (kp + 2) * ref.U * abs64 + 32 * ref.U * reach).all()
    out32, _ = ref.kpconv(x, xyz, centres, idx, kpts, ref.SIGMA)
    assert np.abs(out32 - out64).max() <= (k + 34) * ref.U * np.abs(x).max() * k


# ---- the CPU path ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('c,kp', ref.CKP_GRID)
def test_cpu_path_word_for_word(c, kp):
    """The influences and the forward word for word, grad_x inside the bound of a float32 sum in any order, over the k of
    the grid on the random-geometry inputs; between 0.2 and 0.8 of the pairs of valid slots have h > 0 (so both kinds of
    pair are exercised), taken over the cases of the test."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    pos = tot = 0
    for seed, k in enumerate(ref.K_GRID_HOST):
        b, n, m = ((3, 65, 33), (1, 3, 65), (2, 1025, 9), (2, 64, 20))[seed]
        x, xyz, centres, idx, kpts = _random_case(seed + 10 * c, b, c, n, m, k, kp)
        want, h = ref.kpconv(x, xyz, centres, idx, kpts, ref.SIGMA)
        nv = int(ref.valid_slots(idx, n).sum()) * kp
        pos, tot = pos + ref.positive_share(h, idx, n) * nv, tot + nv
        tx = _t(x).requires_grad_(True)
        args = (_t(xyz), _t(centres), _t(idx), _t(kpts), ref.SIGMA)
        assert ref.same_words(ops.kernel_point_influence(*args).numpy(), h)
        out = ops.kpconv_aggregate(tx, *args)
        assert ref.same_words(out.detach().numpy(), want)
        assert torch.equal(ops.torch_kpconv_aggregate(_t(x), *args), out)
        go = ref.gaussian(seed + 51, (b, kp * c, m))
        out.backward(_t(go))
        assert ref.GradX(idx, ref.slot_words(h, go, c), n).ratio(tx.grad.numpy()) <= 1.0
    assert 0.2 <= pos / tot <= 0.8, pos / tot


@pytest.mark.parametrize('sigma,lo,hi', ((0.3, 0.02, 0.2), (1.0, 0.7, 0.98)))
def test_cpu_path_at_a_small_and_a_large_extent(sigma, lo, hi):
    """sigma = 0.3: few pairs are positive and most rows of the output are empty; sigma = 1.0: most pairs are."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, n, m, k, kp = 2, 8, 200, 50, 16, 15
    x, xyz, centres, idx, kpts = _random_case(7, b, c, n, m, k, kp)
    want, h = ref.kpconv(x, xyz, centres, idx, kpts, sigma)
    assert lo <= ref.positive_share(h, idx, n) <= hi
    if sigma < 0.5:
        assert (want.view(np.uint32) == 0).mean() > 0.5
    tx = _t(x).requires_grad_(True)
    out = ops.kpconv_aggregate(tx, _t(xyz), _t(centres), _t(idx), _t(kpts), sigma)
    assert ref.same_words(out.detach().numpy(), want)
    go = ref.gaussian(8, (b, kp * c, m))
    out.backward(_t(go))
    assert ref.GradX(idx, ref.slot_words(h, go, c), n).ratio(tx.grad.numpy()) <= 1.0


def test_cpu_path_exact_grad_x_on_the_lattice():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, n, m, k, kp = 2, 9, 30, 40, 4, 15
    xyz, centres, kpts = ref.lattice_geometry(60, b, n, m, kp)
    idx = ref.random_list(61, b, n, m, k)
    go = np.random.default_rng(62).integers(-8, 9, size=(b, kp * c, m)).astype(np.float32)
    h = ref.influence(xyz, centres, idx, kpts, 2.0)
    assert 0.05 <= ref.positive_share(h, idx, n) <= 0.8
    tx = _t(ref.cloud(63, n, b, c)).requires_grad_(True)
    ops.kpconv_aggregate(tx, _t(xyz), _t(centres), _t(idx), _t(kpts), 2.0).backward(_t(go))
    ref.GradX(idx, ref.slot_words(h, go, c), n).check_exact(tx.grad.numpy())


def test_zero_influences_and_non_finite_input():
    """A NaN feature under h = 0 does not spread; NaN and infinite coordinates give h = 0; a row without a valid slot is
    all +0.0; elsewhere IEEE holds and a NaN result is the word 0x7fc00000."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    nan, inf = float('nan'), float('inf')
    kpts = np.array([[0, 0, 0], [1, 0, 0]], dtype=np.float32)
    #             on point 0   on point 1   far away     NaN          inf           -inf
    xyz = np.array([[[0, 0, 0], [1, 0, 0], [9, 9, 9], [nan, 0, 0], [0, inf, 0], [-inf, 0, 0]]], dtype=np.float32)
    centres = np.zeros((1, 6, 3), dtype=np.float32)
    centres[0, 5] = (inf, 0, 0)
    idx = np.array([[[0, 1], [1, 2], [2, -1], [3, 4], [5, 6], [0, 1]]], dtype=np.int64)
    x = np.array([[[1.0, nan, 3.0, 4.0, 5.0, 6.0], [inf, 2.0, nan, 1.0, 1.0, 1.0]]], dtype=np.float32)
    h = ops.kernel_point_influence(_t(xyz), _t(centres), _t(idx), _t(kpts), 1.0).numpy()
    assert ref.same_words(h, ref.influence(xyz, centres, idx, kpts, 1.0))
    want_h = np.zeros((1, 6, 2, 2), dtype=np.float32)
    want_h[0, 0, 0, 0] = want_h[0, 0, 1, 1] = want_h[0, 1, 0, 1] = 1.0
    assert ref.same_words(h, want_h)  # rows 3, 4, 5: NaN and infinite distances; row 2: too far, and no point
    out = ops.kpconv_aggregate(_t(x), _t(xyz), _t(centres), _t(idx), _t(kpts), 1.0).numpy()
    assert ref.same_words(out, ref.kpconv(x, xyz, centres, idx, kpts, 1.0)[0])
    NAN, words = 0x7fc00000, out.view(np.uint32)
    one, two = np.float32(1).view(np.uint32), np.float32(2).view(np.uint32)
    # out[0, t * 2 + ch, i]: centre 0 reads x[:, 0] under kernel point 0 (the NaN of x[0, 1] has h = 0 there) and x[:, 1] under 1
    assert words[0, :, 0].tolist() == [one, np.float32(inf).view(np.uint32), NAN, two]
    assert words[0, :, 1].tolist() == [0, 0, NAN, two]
    assert (words[0, :, 2:] == 0).all()


def test_kernel_point_conv_and_the_module():
    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for name in ('kernel_point_layout', 'kernel_point_influence', 'kpconv_aggregate', 'kernel_point_conv', 'KernelPointConv'):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(ops, name)
    b, c, n, m, k, kp, o = 2, 6, 50, 21, 8, 15, 5
    x, xyz, centres, idx, kpts = (_t(a) for a in _random_case(70, b, c, n, m, k, kp))
    torch.manual_seed(0)
    weight, bias = torch.randn(kp, c, o, requires_grad=True), torch.randn(o, requires_grad=True)
    x.requires_grad_(True)
    agg = ops.kpconv_aggregate(x, xyz, centres, idx, kpts, ref.SIGMA)
    got = ops.kernel_point_conv(x, xyz, centres, idx, kpts, ref.SIGMA, weight, bias)
    want = torch.einsum('btcm,tco->bom', agg.view(b, kp, c, m).double(), weight.double()) + bias.double()[None, :, None]
    mag = torch.einsum('btcm,tco->bom', agg.view(b, kp, c, m).double().abs(), weight.double().abs())
    # a float32 dot product of kp * c terms in any order, and the bias
    assert got.shape == (b, o, m) and ((got.double() - want).abs() <= ref.gamma(kp * c + 1) * (mag + bias.abs()[None, :, None])).all()
    got.sum().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in (x, weight, bias))
    # nothing is recorded when x needs no gradient
    assert not ops.kpconv_aggregate(x.detach(), xyz, centres, idx, kpts, ref.SIGMA).requires_grad

    layer = ops.KernelPointConv(c, o, sigma=ref.SIGMA, radius=ref.RADIUS, bias=True)
    assert layer.weight.shape == (15, c, o) and layer.bias.shape == (o,) and 'kernel_points' in dict(layer.named_buffers())
    assert torch.equal(layer.kernel_points, ops.kernel_point_layout(15, ref.RADIUS))
    assert layer.weight.abs().max() <= (15 * c) ** -0.5 and layer.weight.abs().max() > 0.5 * (15 * c) ** -0.5
    y = layer(x, xyz, centres, idx)
    assert torch.equal(y, ops.kernel_point_conv(x, xyz, centres, idx, kpts, ref.SIGMA, layer.weight, layer.bias))
    y.square().sum().backward()
    assert layer.weight.grad.abs().sum() > 0 and layer.bias.grad.abs().sum() > 0
    own = ops.KernelPointConv(c, o, sigma=1.0, kernel_points=torch.eye(3))
    assert own.bias is None and own.weight.shape == (3, c, o) and own(x, xyz, centres, idx).shape == (b, o, m)
    # views, and empty shapes
    vx, vi, vc = x.detach()[:, :, ::2], idx[:, ::2], centres[:, ::2]
    vxyz = xyz[:, ::2]
    assert not vx.is_contiguous() and not vi.is_contiguous()
    assert torch.equal(ops.kpconv_aggregate(vx, vxyz, vc, vi, kpts, ref.SIGMA),
                       ops.kpconv_aggregate(vx.contiguous(), vxyz.contiguous(), vc.contiguous(), vi.contiguous(), kpts, ref.SIGMA))
    for bb, mm in ((0, m), (b, 0)):
        out = ops.kernel_point_conv(x[:bb], xyz[:bb], centres[:bb, :mm], idx[:bb, :mm], kpts, ref.SIGMA, weight)
        assert out.shape == (bb, o, mm) and out.dtype == torch.float32
        out.sum().backward()


def test_kernel_point_layout():
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import raised

    for kp in (1, 2, 15, 32):
        for radius in (1.0, 0.5, 0.06):
            pts = ops.kernel_point_layout(kp, radius)
            assert pts.shape == (kp, 3) and pts.dtype == torch.float32 and (pts[0] == 0).all()
            assert (np.abs(np.linalg.norm(pts[1:].double().numpy() / radius, axis=1) - 1.0) <= 1e-6).all()
            assert torch.equal(pts, ops.kernel_point_layout(kp, radius))
            assert np.abs(pts.numpy() - ref.layout(kp, radius)).max() <= 1e-7 * radius
    pts = ops.kernel_point_layout(15).double()
    assert torch.cdist(pts, pts).add(torch.eye(15)).min() > 0.5  # (spread out: no two points close together)
    assert "NOT the paper's energy-optimised disposition" in ops.kernel_point_layout.__doc__
    for bad in (0, 33, 2.0, True):
        assert raised(ValueError, ops.kernel_point_layout, bad) == f'kernel_point_layout: kp must be an integer in [1, 32], got {bad!r}'


# ---- argument errors -------------------------------------------------------------------------------------------------------


def test_argument_errors_word_for_word():
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import raised

    x, xyz, centres = torch.zeros(2, 6, 10), torch.zeros(2, 10, 3), torch.zeros(2, 5, 3)
    idx, kpts = torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(4, 3)
    weight = torch.zeros(4, 6, 7)
    ops.kpconv_aggregate(x, xyz, centres, idx, kpts, 1.0)
    ops.kernel_point_conv(x, xyz, centres, idx, kpts, 1, weight)
    long_idx = torch.zeros(2, 5, 129, dtype=torch.int64)
    huge = torch.zeros(2, 1 << 16, 1 << 15, dtype=torch.int64, device='meta')
    val = [((x[0], xyz, centres, idx, kpts, 1.0), 'expected x[B,C,N] with C >= 1 and N >= 1, got (6, 10)'),
           ((x, xyz[:, :9], centres, idx, kpts, 1.0), 'expected xyz[B = 2,N = 10,3], got (2, 9, 3)'),
           ((x, xyz[:1], centres, idx, kpts, 1.0), 'expected xyz[B = 2,N,3] with N >= 1, got (1, 10, 3)'),
           ((x, xyz, centres, idx[:1], kpts, 1.0), 'expected idx[B = 2,M,k] with k >= 1, got (1, 5, 3)'),
           ((x, xyz, centres, huge, kpts, 1.0), 'idx[B,M,k] with M * k >= 2^31, got (2, 65536, 32768)'),
           ((x, xyz, centres[:, :4], idx, kpts, 1.0), 'expected centres[B = 2,M = 5,3], got (2, 4, 3)'),
           ((x, xyz, centres, idx, kpts[:0], 1.0), 'expected kernel_points[K,3] with 1 <= K <= 32, got (0, 3)'),
           ((x, xyz, centres, idx, torch.zeros(33, 3), 1.0), 'expected kernel_points[K,3] with 1 <= K <= 32, got (33, 3)'),
           ((x, xyz, centres, idx, kpts[None], 1.0), 'expected kernel_points[K,3] with 1 <= K <= 32, got (1, 4, 3)'),
           ((x, xyz, centres, long_idx, kpts, 1.0), 'k must be <= 128, got 129'),
           ((x.double(), xyz, centres, idx.int(), kpts, 0.0), 'sigma must be a finite number > 0, got 0.0'),
           ((x, xyz, centres, idx, kpts, float('inf')), 'sigma must be a finite number > 0, got inf'),
           ((x, xyz, centres, idx, kpts, float('nan')), 'sigma must be a finite number > 0, got nan'),
           ((x, xyz, centres, idx, kpts, '1'), "sigma must be a finite number > 0, got '1'")]
    for args, text in val:
        assert raised(ValueError, ops.kpconv_aggregate, *args) == 'kpconv_aggregate: ' + text
        assert raised(ValueError, ops.kernel_point_conv, *args, weight) == 'kernel_point_conv: ' + text
    run = [((x.double(), xyz, centres, idx.int(), kpts, 1.0), 'x must be torch.float32, found torch.float64'),  # (shapes first)
           ((x, xyz.double(), centres, idx, kpts, 1.0), 'xyz must be torch.float32, found torch.float64'),
           ((x, xyz, centres.to('meta'), idx, kpts, 1.0), 'centres is on meta, expected cpu'),
           ((x, xyz, centres, idx, kpts.half(), 1.0), 'kernel_points must be torch.float32, found torch.float16'),
           ((x, xyz, centres, idx.int(), kpts, 1.0), 'idx must be torch.int64, found torch.int32'),
           ((x, xyz, centres, idx.to('meta'), kpts, 1.0), 'idx is on meta, expected cpu')]
    for args, text in run:
        assert raised(RuntimeError, ops.kpconv_aggregate, *args) == text
    for args, text in (((xyz[0], centres, idx, kpts, 1.0), 'expected xyz[B,N,3] with N >= 1, got (10, 3)'),
                       ((xyz, centres[:1], idx, kpts, 1.0), 'expected centres[B = 2,M = 5,3], got (1, 5, 3)'),
                       ((xyz, centres, idx, kpts, -1), 'sigma must be a finite number > 0, got -1')):
        assert raised(ValueError, ops.kernel_point_influence, *args) == 'kernel_point_influence: ' + text
    assert raised(RuntimeError, ops.kernel_point_influence, xyz, centres, idx.int(), kpts, 1.0) == 'idx must be torch.int64, found torch.int32'
    assert raised(ValueError, ops.kernel_point_conv, x, xyz, centres, idx, kpts, 1.0, weight[:3]) == \
        'kernel_point_conv: expected weight[K = 4,C = 6,O] with O >= 1, got (3, 6, 7)'
    assert raised(ValueError, ops.kernel_point_conv, x, xyz, centres, idx, kpts, 1.0, weight, torch.zeros(6)) == \
        'kernel_point_conv: expected bias[O = 7], got (6,)'


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued, sizes before pointers (no device memory is touched: the sentinel
    stays), in the words and the order of the checks."""
    from pointcloudcounterfactual_amd import _lib
    from tests.util import c_status

    L = _lib.lib
    buf = (ctypes.c_char * 64)(*([0x5a] * 64))
    p = ctypes.addressof(buf)
    EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)
    nan, inf = float('nan'), float('inf')

    def calls(b, c, n, m, k, kp, sigma, q=p):
        return (('kpconv_aggregate', L.pcc_kpconv_aggregate, (b, c, n, m, k, kp, q, q, q, q, q, sigma, q, None)),
                ('kpconv_aggregate_bwd', L.pcc_kpconv_aggregate_bwd, (b, c, n, m, k, kp, q, q, q, q, sigma, q, q, None)))

    # (b, c, n, m, k, kp, sigma): the first refusal in the order of the checks wins; null pointers do not hide a bad size
    cases = [((-1, 6, 8, 4, 2, 0, 0.0), 'bad size'), ((1, 0, 8, 4, 2, 5, 1.0), 'bad size'), ((1, 6, 0, 4, 2, 5, 1.0), 'bad size'),
             ((1, 6, 8, -1, 2, 5, 1.0), 'bad size'), ((1, 6, 8, 4, 0, 5, 1.0), 'bad size'),
             ((65536, 6, 8, 4, 2, 0, 1.0), 'batch too large'), ((1, 6, 8, 1 << 16, 1 << 15, 0, 1.0), 'list too long (m * k >= 2^31)'),
             ((1, 6, 8, 4, 129, 0, 0.0), 'kernel points must be 1..32'), ((1, 6, 8, 4, 2, 33, 1.0), 'kernel points must be 1..32'),
             ((0, 6, 8, 0, 2, -1, 1.0), 'kernel points must be 1..32'), ((1, 6, 8, 4, 129, 5, 0.0), 'k > 128'),
             ((0, 6, 8, 0, 129, 32, 1.0), 'k > 128'), ((1, 6, 8, 4, 2, 5, 0.0), 'sigma must be finite and > 0'),
             ((1, 6, 8, 4, 2, 5, -1.0), 'sigma must be finite and > 0'), ((1, 6, 8, 4, 2, 5, inf), 'sigma must be finite and > 0'),
             ((0, 6, 8, 0, 128, 1, nan), 'sigma must be finite and > 0')]
    for sizes, text in cases:
        for q in (p, None):
            for name, fn, args in calls(*sizes, q=q):
                assert c_status(L, fn, *args) == (EINVAL, f'{name}: {text}'), (name, sizes)
    b, c, n, m, k, kp = 1, 6, 8, 4, 2, 5
    for hole in range(6):
        args = [p] * 6
        args[hole] = None
        assert c_status(L, L.pcc_kpconv_aggregate, b, c, n, m, k, kp, *args[:5], 1.0, args[5], None) == (EINVAL, 'kpconv_aggregate: null pointer')
        assert c_status(L, L.pcc_kpconv_aggregate_bwd, b, c, n, m, k, kp, *args[:4], 1.0, *args[4:], None) == \
            (EINVAL, 'kpconv_aggregate_bwd: null pointer')
    assert c_status(L, L.pcc_kpconv_aggregate_bwd, b, c, n, 0, k, kp, p, p, p, p, 1.0, p, None, None) == \
        (EINVAL, 'kpconv_aggregate_bwd: null pointer')  # (m = 0 zero-fills grad_x: it must be there)
    # nothing to do: an empty batch, an empty list forward
    for name, fn, args in calls(0, c, n, m, k, kp, 1.0, q=None) + calls(b, c, n, 0, k, kp, 1.0, q=None)[:1]:
        assert c_status(L, fn, *args) == (0, ''), name
    assert L.pcc_last_status() == 0
    assert bytes(buf) == b'\x5a' * 64


def test_the_abi_the_header_and_the_switch_of_the_paths_are_bound():
    from pointcloudcounterfactual_amd import _lib

    hooks = open(os.path.join(ROOT, 'include', 'pcc_test_hooks.h')).read()
    assert re.search(r'PCC_TUNE_KEYS = 16\b', hooks) and len(_lib.TUNING) == 16  # (no new key: the paths obey interp_path)
    assert 'pcc_kpconv_aggregate' in hooks[hooks.index('PCC_TUNE_INTERP_PATH'):hooks.index('PCC_TUNE_KEYS')]
    header = open(os.path.join(ROOT, 'include', 'pcc_neighbour.h')).read()
    for name, nargs in zip(NAMES, (14, 14)):
        restype, argtypes = _lib.ABI[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert decl, name
        params = [a.strip() for a in decl.group(1).replace('\n', ' ').split(',')]
        assert len(params) == nargs and params[-1] == 'pcc_stream_t stream'
        for a, t in zip(params[:-1], argtypes[:-1]):
            assert (t is ctypes.c_int) == a.startswith('int '), (name, a)
            assert (t is ctypes.c_float) == (a.startswith('float ') and '*' not in a), (name, a)
            assert (t is ctypes.c_void_p) == ('*' in a), (name, a)
        assert hasattr(_lib.lib, name)
    assert ref.BOUNDARIES[-2] * 4 == 160 * 1024  # (one row of bins is a workgroup's LDS)
