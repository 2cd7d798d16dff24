"""CPU tests of ``neighbour_ops.neighbour_softmax`` / ``aggregate_points`` / ``attention_aggregate`` / ``vector_attention``:
the numpy reference (tests/attention_reference.py) against closed forms, against the interpolation reference and against a
float64 autograd composition; the torch path of CPU tensors against that reference -- word for word where the contract
fixes the words, inside the softmax bar otherwise; every argument error; the ABI and the header."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import attention_reference as ref
from tests import interpolate_reference as iref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('pcc_neighbour_softmax', 'pcc_neighbour_softmax_bwd', 'pcc_aggregate_points', 'pcc_aggregate_points_bwd')


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a))


def _case(seed, b, c, g, n, m, k, with_rel=True):
    x = ref.cloud(seed, n, b, c)
    idx = ref.random_list(seed + 1, b, n, m, k)
    logits = ref.gaussian(seed + 2, (b, g, m, k), 3.0)
    rel = ref.gaussian(seed + 3, (b, c, m, k)) if with_rel else None
    return x, idx, logits, rel


# ---- the reference against closed forms ------------------------------------------------------------------------------------


def test_reference_softmax_of_equal_logits_is_a_power_of_two():
    for p in range(8):
        k = (1 << p) + 3
        idx = np.full((1, 2, k), -1, dtype=np.int64)
        idx[:, :, 1:1 + (1 << p)] = 5  # 2^p valid slots
        logits = np.full((1, 3, 2, k), 1.7, dtype=np.float32)
        got = ref.softmax32(logits, idx, 9)
        want = np.where(ref.valid_slots(idx, 9)[:, None], np.float32(2.0 ** -p), np.float32(0))
        assert ref.same_words(got, np.broadcast_to(want, got.shape))
        assert ref.softmax_ratio(got, logits, idx, 9) == 0.0


def test_reference_forward_with_one_group_is_the_interpolation():
    for seed, (b, c, n, m, k) in enumerate(((3, 9, 65, 33, 5), (2, 8, 7, 65, 16), (1, 1, 1, 3, 1))):
        x, idx, _, _ = _case(seed, b, c, 1, n, m, k)
        w = ref.gaussian(seed + 9, (b, 1, m, k))
        assert ref.same_words(ref.forward(x, idx, w), iref.forward(x, idx, w[:, 0]))
        g = ref.gaussian(seed + 10, (b, c, m))
        assert ref.same_words(ref.grad_w(x, idx, g, 1)[:, 0], iref.grad_w(x, idx, g))


def _autograd64(x, idx, logits, rel, gout):
    """The three gradients and ``(attn, out)`` of the composition in float64 torch autograd."""
    b, c, n = x.shape
    g, m, k = logits.shape[1:]
    tx, tl = _t(x).double().requires_grad_(True), _t(logits).double().requires_grad_(True)
    tr = None if rel is None else _t(rel).double().requires_grad_(True)
    tidx = _t(idx)
    valid = (tidx >= 0) & (tidx < n)
    safe = torch.where(valid, tidx, torch.zeros_like(tidx))
    attn = torch.softmax(tl.masked_fill(~valid[:, None], float('-inf')), -1)
    attn = torch.where(valid[:, None], attn, torch.zeros((), dtype=torch.float64))
    v = torch.gather(tx, 2, safe.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)
    if tr is not None:
        v = v + tr
    out = (attn.repeat_interleave(c // g, dim=1) * v * valid[:, None]).sum(-1)
    out.backward(_t(gout).double())
    return tx.grad.numpy(), tl.grad.numpy(), None if tr is None else tr.grad.numpy(), attn.detach().numpy(), out.detach().numpy()


@pytest.mark.parametrize('with_rel', (False, True))
def test_reference_gradients_against_float64_autograd(with_rel):
    b, c, g, n, m, k = 2, 6, 3, 40, 17, 5
    x, idx, logits, rel = _case(20, b, c, g, n, m, k, with_rel)
    idx[0, :, 0] = np.arange(m) % n  # (every row of sample 0 has a valid slot; sample 1 keeps what the list gave it)
    gout = ref.gaussian(24, (b, c, m))
    gx64, gl64, gr64, attn64, out64 = _autograd64(x, idx, logits, rel, gout)
    attn = ref.softmax32(logits, idx, n)
    assert np.abs(attn - attn64).max() <= 16 * ref.U
    assert np.abs(ref.forward(x, idx, attn, rel) - out64).max() <= 64 * ref.U * np.abs(out64).max()
    ga = ref.grad_w(x, idx, gout, g, rel)
    gl = ref.softmax_bwd(attn, idx, n, ga)
    assert np.abs(gl - gl64).max() <= 256 * ref.U * max(1.0, np.abs(gl64).max())
    gx = ref.GroupedGradX(idx, attn, gout, n)
    assert np.abs(gx.gx - gx64).max() <= 64 * ref.U * max(1.0, np.abs(gx64).max())
    if with_rel:
        assert np.abs(ref.grad_rel(idx, attn, gout, n) - gr64).max() <= 16 * ref.U * max(1.0, np.abs(gr64).max())


def test_numpy_float32_softmax_is_well_inside_the_bar():
    worst = 0.0
    for seed, scale in enumerate((1.0, 3.0, 30.0)):
        for k in (1, 5, 16, 128):
            idx = ref.random_list(seed * 7 + k, 2, 11, 33, k)
            logits = ref.gaussian(seed + 40, (2, 3, 33, k), scale)
            logits[0, 0, ::4, ::3] = -np.inf
            worst = max(worst, ref.softmax_ratio(ref.softmax32(logits, idx, 11), logits, idx, 11))
    assert worst <= 0.5


# ---- the CPU path ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize('c,g', ref.CG_GRID)
def test_cpu_path_word_for_word(c, g):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for seed, (b, n, m, k) in enumerate(((3, 65, 33, 5), (1, 3, 65, 16), (2, 1025, 3, 17))):
        for with_rel in (False, True):
            x, idx, logits, rel = _case(seed + c, b, c, g, n, m, k, with_rel)
            w = ref.gaussian(seed + 50, (b, g, m, k))
            gout = ref.gaussian(seed + 51, (b, c, m))
            tx, tw = _t(x).requires_grad_(True), _t(w).requires_grad_(True)
            tr = None if rel is None else _t(rel).requires_grad_(True)
            out = ops.aggregate_points(tx, _t(idx), tw, tr)
            assert ref.same_words(out.detach().numpy(), ref.forward(x, idx, w, rel))
            out.backward(_t(gout))
            assert ref.same_words(tw.grad.numpy(), ref.grad_w(x, idx, gout, g, rel))
            if with_rel:
                assert ref.same_words(tr.grad.numpy(), ref.grad_rel(idx, w, gout, n))
            ref.GroupedGradX(idx, w, gout, n).check_bound(tx.grad.numpy())
            # the softmax: inside the bar; its backward word for word on its own output
            tl = _t(logits).requires_grad_(True)
            attn = ops.neighbour_softmax(tl, _t(idx), n)
            assert ref.softmax_ratio(attn.detach().numpy(), logits, idx, n) <= 1.0
            ga = ref.gaussian(seed + 52, (b, g, m, k))
            attn.backward(_t(ga))
            assert ref.same_words(tl.grad.numpy(), ref.softmax_bwd(attn.detach().numpy(), idx, n, ga))


def test_cpu_path_exact_grad_x_and_only_the_required_gradients():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, g, n, m, k = 2, 8, 2, 30, 40, 4
    x, idx, _, rel = _case(60, b, c, g, n, m, k)
    w = ref.dyadic(61, (b, g, m, k))
    gout = np.random.default_rng(62).integers(-8, 9, size=(b, c, m)).astype(np.float32)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        tx, tw, tr = (_t(a).requires_grad_(r) for a, r in zip((x, w, rel), need))
        ops.aggregate_points(tx, _t(idx), tw, tr).backward(_t(gout))
        assert [t.grad is not None for t in (tx, tw, tr)] == list(need)
        if need[0]:
            ref.GroupedGradX(idx, w, gout, n).check_exact(tx.grad.numpy())


def test_cpu_attention_aggregate_and_vector_attention():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, c, g, n, m, k = 2, 6, 3, 50, 21, 4
    x, idx, logits, rel = _case(70, b, c, g, n, m, k)
    gout = ref.gaussian(71, (b, c, m))
    tx, tl, tr = (_t(a).requires_grad_(True) for a in (x, logits, rel))
    out, attn = ops.attention_aggregate(tx, _t(idx), tl, tr, return_attention=True)
    a = attn.detach().numpy()
    assert ref.softmax_ratio(a, logits, idx, n) <= 1.0
    assert ref.same_words(out.detach().numpy(), ref.forward(x, idx, a, rel))
    out.backward(_t(gout))
    assert ref.same_words(tr.grad.numpy(), ref.grad_rel(idx, a, gout, n))
    assert ref.same_words(tl.grad.numpy(), ref.softmax_bwd(a, idx, n, ref.grad_w(x, idx, gout, g, rel)))
    ref.GroupedGradX(idx, a, gout, n).check_bound(tx.grad.numpy())
    assert torch.equal(ops.attention_aggregate(tx, _t(idx), tl, tr), out)

    # one layer's data flow against the composition written by hand
    torch.manual_seed(0)
    xyz, xyz_q = torch.rand(b, n, 3), torch.rand(b, m, 3)
    query, key = torch.randn(b, c, m), torch.randn(b, c, n)
    pos_net, attn_net = torch.nn.Conv2d(3, c, 1), torch.nn.Conv2d(c, g, 1)
    tidx = _t(idx)
    got = ops.vector_attention(xyz_q, xyz, query, key, tx, tidx, pos_net, attn_net)
    delta = pos_net(ops.group_points(xyz, tidx, centres=xyz_q, point_major=True))
    lg = attn_net(delta - ops.group_points(key, tidx, centres=query))
    want = ops.aggregate_points(tx, tidx, ops.neighbour_softmax(lg, tidx, n), delta)
    assert torch.equal(got, want) and got.shape == (b, c, m)


def test_cpu_non_finite_logits_follow_torch_softmax():
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    nan, inf = float('nan'), float('inf')
    idx = torch.tensor([[[0, 1, 2, -1], [0, 1, 2, -1], [0, 1, 2, -1], [0, 1, -1, 7], [-1, 9, -1, 7], [0, 1, 2, -1]]])
    logits = torch.tensor([[[[0.0, nan, 1.0, 5.0], [0.0, inf, 1.0, 5.0], [-inf, -inf, -inf, 0.0], [-inf, 2.0, nan, inf],
                             [1.0, 2.0, 3.0, 4.0], [1.0, -inf, 1.0, nan]]]])
    got = ops.neighbour_softmax(logits, idx, 3).numpy().view(np.uint32)[0, 0]
    NAN, HALF, ONE = 0x7fc00000, 0x3f000000, 0x3f800000
    assert got.tolist() == [[NAN, NAN, NAN, 0], [NAN, NAN, NAN, 0], [NAN, NAN, NAN, 0], [0, ONE, 0, 0], [0, 0, 0, 0], [HALF, 0, HALF, 0]]


def test_views_empty_shapes_and_exports():
    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for name in ('neighbour_softmax', 'aggregate_points', 'attention_aggregate', 'vector_attention'):
        assert name in pkg.__all__ and getattr(pkg, name) is getattr(ops, name)
    x, idx, logits, rel = (_t(a) for a in _case(80, 2, 8, 2, 20, 14, 6))
    vx, vi, vl, vr = x[:, :, ::2], idx[:, ::2], logits[:, :, ::2], rel[:, :, ::2]
    assert not vx.is_contiguous() and not vi.is_contiguous() and not vl.is_contiguous()
    assert torch.equal(ops.attention_aggregate(vx, vi, vl, vr),
                       ops.attention_aggregate(vx.contiguous(), vi.contiguous(), vl.contiguous(), vr.contiguous()))
    for bb, mm in ((0, 14), (2, 0)):
        out = ops.attention_aggregate(x[:bb], idx[:bb, :mm], logits[:bb, :, :mm], rel[:bb, :, :mm])
        assert out.shape == (bb, 8, mm) and out.dtype == torch.float32


# ---- argument errors -------------------------------------------------------------------------------------------------------


def test_argument_errors_word_for_word():
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from tests.util import raised

    x, idx = torch.zeros(2, 6, 10), torch.zeros(2, 5, 3, dtype=torch.int64)
    w, rel = torch.zeros(2, 3, 5, 3), torch.zeros(2, 6, 5, 3)
    ops.aggregate_points(x, idx, w, rel)
    ops.attention_aggregate(x, idx, w, rel)
    ops.neighbour_softmax(w, idx, 10)
    long_idx, long_w = torch.zeros(2, 5, 129, dtype=torch.int64), torch.zeros(2, 3, 5, 129)
    huge = torch.zeros(2, 1 << 16, 1 << 15, dtype=torch.int64, device='meta')
    val = [((x[0], idx, w, rel), 'expected x[B,C,N] with C >= 1 and N >= 1, got (6, 10)'),
           ((x[:, :0], idx, w, rel), 'expected x[B,C,N] with C >= 1 and N >= 1, got (2, 0, 10)'),
           ((x, idx[:1], w, rel), 'expected idx[B = 2,M,k] with k >= 1, got (1, 5, 3)'),
           ((x, idx[:, :, :0], w, rel), 'expected idx[B = 2,M,k] with k >= 1, got (2, 5, 0)'),
           ((x, huge, w, rel), 'idx[B,M,k] with M * k >= 2^31, got (2, 65536, 32768)'),
           ((x, idx, w[:, :, :4], rel), 'expected {w}[B = 2,G,M = 5,k = 3] with G >= 1, got (2, 3, 4, 3)'),
           ((x, idx, w[:, :0], rel), 'expected {w}[B = 2,G,M = 5,k = 3] with G >= 1, got (2, 0, 5, 3)'),
           ((x, idx, w[0], rel), 'expected {w}[B = 2,G,M = 5,k = 3] with G >= 1, got (3, 5, 3)'),
           ((x.double(), idx.int(), torch.zeros(2, 4, 5, 3), rel), 'the G = 4 groups of {w} do not divide the C = 6 channels of x'),
           ((x, idx, w, rel[:, :5]), 'expected rel[B,C,M,k] = (2, 6, 5, 3), got (2, 5, 5, 3)'),
           ((x, long_idx, long_w, None), 'k must be <= 128, got 129')]
    for fn, wname in ((ops.aggregate_points, 'weights'), (ops.attention_aggregate, 'logits')):
        for args, text in val:
            assert raised(ValueError, fn, *args) == f'{fn.__name__}: ' + text.format(w=wname)
        assert raised(RuntimeError, fn, x.double(), idx.int(), w, rel) == 'x must be torch.float32, found torch.float64'  # (shapes first)
        assert raised(RuntimeError, fn, x, idx.int(), w.double(), rel) == 'idx must be torch.int64, found torch.int32'
        assert raised(RuntimeError, fn, x, idx.to('meta'), w, rel) == 'idx is on meta, expected cpu'
        assert raised(RuntimeError, fn, x, idx, w.double(), rel) == f'{wname} must be torch.float32, found torch.float64'
        assert raised(RuntimeError, fn, x, idx, w.to('meta'), rel) == f'{wname} is on meta, expected cpu'
        assert raised(RuntimeError, fn, x, idx, w, rel.half()) == 'rel must be torch.float32, found torch.float16'
        assert raised(RuntimeError, fn, x, idx, w, rel.to('meta')) == 'rel is on meta, expected cpu'
    sm = [((w[0], idx, 10), 'expected logits[B,G,M,k] with G >= 1, got (3, 5, 3)'),
          ((w[:, :0], idx, 10), 'expected logits[B,G,M,k] with G >= 1, got (2, 0, 5, 3)'),
          ((w, idx[:1], 10), 'expected idx[B = 2,M,k] with k >= 1, got (1, 5, 3)'),
          ((w[:, :, :4], idx, 10), 'expected logits[B,G,M,k] = (2, 3, 5, 3), got (2, 3, 4, 3)'),
          ((long_w, long_idx, 10), 'k must be <= 128, got 129'),
          ((w.double(), idx, 0), 'n must be an integer >= 1, got 0'), ((w, idx, 2.0), 'n must be an integer >= 1, got 2.0'),
          ((w, idx, True), 'n must be an integer >= 1, got True')]
    for args, text in sm:
        assert raised(ValueError, ops.neighbour_softmax, *args) == 'neighbour_softmax: ' + text
    assert raised(RuntimeError, ops.neighbour_softmax, w.double(), idx.int(), 10) == 'logits must be torch.float32, found torch.float64'
    assert raised(RuntimeError, ops.neighbour_softmax, w, idx.int(), 10) == 'idx must be torch.int64, found torch.int32'
    assert raised(RuntimeError, ops.neighbour_softmax, w, idx.to('meta'), 10) == 'idx is on meta, expected cpu'


def test_c_abi_argument_checks_need_no_device():
    """PCC_EINVAL comes back before anything is enqueued, sizes before pointers (no device memory is touched: the sentinel
    stays), in the words and the order of the checks."""
    from pointcloudcounterfactual_amd import _lib
    from tests.util import c_status

    L = _lib.lib
    buf = (ctypes.c_char * 64)(*([0x5a] * 64))
    p = ctypes.addressof(buf)
    EINVAL = -22  # PCC_EINVAL (include/pcc_structural.h)

    def calls(b, c, g, n, m, k, q=p):
        return (('neighbour_softmax', L.pcc_neighbour_softmax, (b, g, n, m, k, q, q, q, None)),
                ('neighbour_softmax_bwd', L.pcc_neighbour_softmax_bwd, (b, g, n, m, k, q, q, q, q, None)),
                ('aggregate_points', L.pcc_aggregate_points, (b, c, g, n, m, k, q, q, q, q, q, None)),
                ('aggregate_points_bwd', L.pcc_aggregate_points_bwd, (b, c, g, n, m, k, q, q, q, q, q, q, q, q, None)))

    # (b, c, g, n, m, k): the first refusal in the order of the checks wins; null pointers do not hide a bad size
    cases = [((-1, 6, 3, 8, 4, 2), 'bad size'), ((1, 6, 3, 0, 4, 2), 'bad size'), ((1, 6, 3, 8, -1, 2), 'bad size'),
             ((1, 6, 3, 8, 4, 0), 'bad size'), ((65536, 6, 3, 8, 4, 2), 'batch too large'),
             ((1, 6, 3, 8, 1 << 16, 1 << 15), 'list too long (m * k >= 2^31)'), ((0, 6, 3, 8, 0, 129), 'k > 128'),
             ((1, 6, 3, 8, 4, 129), 'k > 128')]
    for sizes, text in cases:
        for q in (p, None):
            for name, fn, args in calls(*sizes, q=q):
                assert c_status(L, fn, *args) == (EINVAL, f'{name}: {text}'), (name, sizes)
    for sizes, text in (((1, 0, 1, 8, 4, 2), 'bad size'), ((1, 6, 4, 8, 4, 2), 'g must be >= 1 and divide c'),
                        ((1, 6, 0, 8, 4, 2), 'g must be >= 1 and divide c'), ((1, 6, 4, 8, 4, 129), 'g must be >= 1 and divide c')):
        for name, fn, args in calls(*sizes)[2:]:
            assert c_status(L, fn, *args) == (EINVAL, f'{name}: {text}'), (name, sizes)
    for name, fn, args in calls(1, 6, 0, 8, 4, 2)[:2]:
        assert c_status(L, fn, *args) == (EINVAL, f'{name}: bad size')  # (the softmax has no channels: g is its c)
    b, c, g, n, m, k = 1, 6, 3, 8, 4, 2
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        assert c_status(L, L.pcc_neighbour_softmax, b, g, n, m, k, *args, None) == (EINVAL, 'neighbour_softmax: null pointer')
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert c_status(L, L.pcc_neighbour_softmax_bwd, b, g, n, m, k, *args, None) == (EINVAL, 'neighbour_softmax_bwd: null pointer')
    for x, idx, w, out in ((None, p, p, p), (p, None, p, p), (p, p, None, p), (p, p, p, None)):
        assert c_status(L, L.pcc_aggregate_points, b, c, g, n, m, k, x, idx, w, None, out, None) == (EINVAL, 'aggregate_points: null pointer')
    for x, idx, w, go, gx, gw, gr in ((p, None, p, p, p, p, p), (p, p, None, p, p, p, p), (p, p, p, None, p, p, p), (None, p, p, p, p, p, p),
                                      (None, p, p, p, None, p, None)):
        assert c_status(L, L.pcc_aggregate_points_bwd, b, c, g, n, m, k, x, idx, w, None, go, gx, gw, gr, None) == \
            (EINVAL, 'aggregate_points_bwd: null pointer')
    # nothing to do: an empty batch, an empty list forward, no gradient asked for
    for name, fn, args in calls(0, c, g, n, m, k, q=None) + calls(b, c, g, n, 0, k, q=None)[:3]:
        assert c_status(L, fn, *args) == (0, ''), name
    assert L.pcc_aggregate_points_bwd(b, c, g, n, m, k, None, None, None, None, None, None, None, None, None) == 0
    assert L.pcc_aggregate_points_bwd(b, c, g, n, 0, k, None, None, None, None, None, None, p, p, None) == 0  # (m = 0: nothing to write)
    assert L.pcc_last_status() == 0
    assert bytes(buf) == b'\x5a' * 64


def test_the_abi_the_header_and_the_switch_of_the_paths_are_bound():
    from pointcloudcounterfactual_amd import _lib

    hooks = open(os.path.join(ROOT, 'include', 'pcc_test_hooks.h')).read()
    assert re.search(r'PCC_TUNE_INTERP_PATH = %d\b' % _lib.TUNING['interp_path'], hooks) and _lib.TUNING['interp_path'] == 15
    assert re.search(r'PCC_TUNE_KEYS = 16\b', hooks) and len(_lib.TUNING) == 16
    assert 'pcc_aggregate_points' in hooks[hooks.index('PCC_TUNE_INTERP_PATH'):hooks.index('PCC_TUNE_KEYS')]
    header = open(os.path.join(ROOT, 'include', 'pcc_neighbour.h')).read()
    for name, nargs in zip(NAMES, (9, 10, 12, 15)):
        restype, argtypes = _lib.ABI[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
        decl = re.search(r'\bint %s\(([^;]*)\);' % name, header)
        assert decl, name
        params = [a.strip() for a in decl.group(1).replace('\n', ' ').split(',')]
        assert len(params) == nargs and params[-1] == 'pcc_stream_t stream'
        for a, t in zip(params[:-1], argtypes[:-1]):
            assert (t is ctypes.c_int) == a.startswith('int '), (name, a)
            assert (t is ctypes.c_void_p) == ('*' in a), (name, a)
        assert hasattr(_lib.lib, name)
