"""GPU tests of the Sinkhorn divergence (``pcc_sinkhorn`` through the C ABI with guarded, NaN-prefilled buffers, and through
``losses.sinkhorn_divergence``) against the dense float64 reference of tests/sinkhorn_reference.py, in the error units
and bars stated there: the grid of sizes around every tile, group and slice boundary of the kernel, the closed forms,
determinism and independence of the batch, aliasing, a temperature far below the cloud's scale, every subset of the
outputs, non-finite input, the refusals, every column split forced through the test hook, and autograd."""

import contextlib
import ctypes
import itertools

import numpy as np
import pytest
import torch

from pointcloudcounterfactual_amd.losses import sinkhorn_divergence, torch_sinkhorn  # noqa: F401  (no feature, no test)
from tests import sinkhorn_reference as ref
from tests.which_ran import assert_only, ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5  # what the guard behind every output must keep
GUARD = 64
ALL = ('cost', 'pot_x', 'pot_y', 'grad_x', 'grad_y')
PCC_EINVAL = -22

# (n, m): the sizes the issue names, n != m in most pairs, and both sides of what the kernel has: the group of 8 columns
# (7, 8, 9), the tile of 256 columns and rows, which is also where a scan gets its second column slice (255, 256, 257),
# the third slice (512, 513) and the fifth (1024, 1025).  How many slices a scan is ALLOWED (split_for: 16, 8, 4, 2, 1 from
# rows = 32768, 65536, 131072, 262144 on; rows = n + m, twice that with debias) is test_product_split_boundaries' subject.
PAIRS = ((1, 1), (1, 2), (2, 3), (3, 1), (7, 9), (8, 8), (9, 63), (63, 64), (64, 65), (65, 63), (64, 64), (255, 256), (256, 257), (257, 255),
         (257, 1), (1, 257), (513, 512), (512, 513), (257, 1025), (1025, 513), (1024, 65), (2, 1025))
# (steps, debias): all six; a pair of the grid runs them all while it is small and two of them otherwise
CONFIGS = tuple(itertools.product((1, 2, 8), (True, False)))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same_words(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _shapes(b, n, m):
    return {'cost': (b,), 'pot_x': (b, n), 'pot_y': (b, m), 'grad_x': (b, n, 3), 'grad_y': (b, m, 3)}


_SPLIT = [0]  # the sinkhorn_split value in force: ``_call`` asserts the slice count the rule predicts under it


@contextlib.contextmanager
def _split(value):
    from pointcloudcounterfactual_amd import _lib

    with _lib.tuning('sinkhorn_split', value):
        _SPLIT[0] = value
        try:
            yield
        finally:
            _SPLIT[0] = 0


def _call(x, y, eps, debias=True, want=ALL):
    """``pcc_sinkhorn`` on device tensors for the outputs named in ``want`` (null pointers for the others): ``{name: numpy}``.
    The outputs start as NaN with sentinels behind them: every element must be written, nothing else.  The launch record
    must name the scans by the slice count ``ref.slices`` predicts, with the merge kernel exactly where that is above 1."""
    from pointcloudcounterfactual_amd import _lib

    b, n, m = x.shape[0], x.shape[1], y.shape[1]
    shapes = _shapes(b, n, m)
    bufs = {}
    for name in want:
        size = int(np.prod(shapes[name]))
        bufs[name] = torch.full((size + GUARD,), SENTINEL, dtype=torch.float32, device=x.device)
        bufs[name][:size] = float('nan')
    sched = (ctypes.c_float * len(eps))(*eps)
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_sinkhorn, 'sinkhorn', x.device, b, n, m, x.data_ptr(), y.data_ptr(), len(eps),
                                     ctypes.cast(sched, ctypes.c_void_p), int(debias),
                                     *[bufs[name].data_ptr() if name in bufs else None for name in ALL]))
    if b and want:
        assert_only(names, ref.scan_kernel(n, m, debias, _SPLIT[0]), 'sk_scan_kernel')
        assert ('sk_merge_kernel' in names) == (ref.slices(n, m, debias, _SPLIT[0]) > 1), names
    out = {}
    for name in want:
        host, size = bufs[name].cpu().numpy(), int(np.prod(shapes[name]))
        assert (host[size:] == np.float32(SENTINEL)).all(), name
        out[name] = host[:size].reshape(shapes[name]).copy()
    return out


def _run(cuda, x, y, eps, debias=True, want=ALL):
    return _call(_dev(x, cuda), _dev(y, cuda), eps, debias, want)


def _merge(worst, mult):
    for key, v in mult.items():
        worst[key] = max(worst.get(key, 0.0), v)


@pytest.mark.parametrize('case', range(len(PAIRS)))
def test_grid_inside_the_bars(cuda, case):
    """Potentials, cost and gradients over the grid; b in {1, 3} and the clouds' scale (1, 1e-3, 1000 around 300) rotate, the
    schedule is scaled by the diameter."""
    n, m = PAIRS[case]
    configs = range(6) if n * m <= 70000 else ((case % 6), (case + 3) % 6)
    worst = {}
    for k in configs:
        steps, debias = CONFIGS[k]
        b = (1, 3)[(case + k // 2) % 2]
        scale, centre = ref.SCALES[(case + k) % 3]
        x, y = ref.clouds(1000 * case + k, b, n, m, scale, centre)
        eps = ref.schedule(steps, ref.diameter(x, y))
        got = _run(cuda, x, y, eps, debias)
        mult = ref.Result(x, y, eps, debias).multiples(got)
        print(f'sinkhorn {n} x {m} b={b} T={steps} debias={debias} scale={scale}: {mult}')
        _merge(worst, mult)
    print(f'sinkhorn {n} x {m}: largest multiples {worst}')
    for key, bar in (('pot', ref.BAR_POT), ('cost', ref.BAR_COST), ('grad', ref.BAR_GRAD)):
        assert worst[key] <= bar, (n, m, worst)


def test_large_odd_sizes(cuda):
    """2049 x 2047, one cloud: nine column slices per scan, the last one of a single column resp. 255."""
    x, y = ref.clouds(77, 1, 2049, 2047)
    eps = ref.schedule(8, ref.diameter(x, y))
    mult = ref.Result(x, y, eps).check(_run(cuda, x, y, eps), 'large')
    print(f'sinkhorn 2049 x 2047: {mult}')


# (n, m) with debias off, where rows = n + m: both sides of 16 -> 8 slices and of 8 -> 4.  The second cloud is one point, so
# the dense reference is n x 1 while the y -> x scan has all n columns to cut.  (4 -> 2 needs n + m = 131072, or 65536 with
# debias, 2 -> 1 n = m = 65536 with debias: a dense n x n reference of 34 GB.  Those two allowances run forced, below.)
SPLIT_BOUNDARIES = ((32766, 1, 16), (32767, 1, 8), (65534, 1, 8), (65535, 1, 4), (65536, 1, 4))  # (the last: n at its limit)


@pytest.mark.parametrize('n,m,slices', SPLIT_BOUNDARIES)
def test_product_split_boundaries(cuda, n, m, slices):
    """The product's own choice of slices either side of the sizes where it changes, inside the bars; forcing the number
    of slices this test expects must return the product's words (which pins the choice itself)."""
    assert ref.slices(n, m, False) == slices  # (what ``_call`` holds the launch record to)
    for k, steps in enumerate((8, 2)):
        scale, centre = ref.SCALES[(n + k) % 3]
        x, y = ref.clouds(n + k, 1, n, m, scale, centre)
        eps = ref.schedule(steps, ref.diameter(x, y))
        xd, yd = _dev(x, cuda), _dev(y, cuda)
        got = _call(xd, yd, eps, False)
        mult = ref.Result(x, y, eps, False).check(got, (n, m, steps))
        print(f'sinkhorn {n} x {m} T={steps} scale={scale} (product: {slices} slices): {mult}')
        with _split(slices):
            forced = _call(xd, yd, eps, False)
        for name in ALL:
            assert _same_words(forced[name], got[name]), (name, n, m, steps)


def test_closed_forms(cuda):
    """n = m = 1, debiased: cost = |x - y|^2 / 2 and grad_x = x - y; m = 1, debias off: cost = mean_i C(x_i, y)."""
    x, y = ref.clouds(5, 3, 1, 1)
    for eps in ([0.3], ref.schedule(8, ref.diameter(x, y))):
        got = _run(cuda, x, y, eps)
        d = x.astype(np.float64) - y.astype(np.float64)
        c = 0.5 * (d * d).sum((1, 2))
        unit = (len(eps) + 2) * 2.0 ** -24 * c
        assert (np.abs(got['cost'] - c) <= ref.BAR_POT * unit).all()
        # (one softmax term: the kernel returns fl(x - y) exactly; 2^-23 |d| covers that rounding and the output's)
        assert (np.abs(got['grad_x'] - d) <= ref.BAR_GRAD * (unit / eps[-1])[:, None, None] * np.abs(d) + 2.0 ** -23 * np.abs(d)).all()
    x, y = ref.clouds(6, 2, 300, 1)
    for steps in (1, 8):
        got = _run(cuda, x, y, ref.schedule(steps, ref.diameter(x, y)), debias=False, want=('cost',))
        d = x.astype(np.float64) - y.astype(np.float64)
        c = 0.5 * (d * d).sum(-1)
        assert (np.abs(got['cost'] - c.mean(1)) <= ref.BAR_POT * (steps + 2) * 2.0 ** -24 * c.max(1)).all()


def test_determinism_and_independence_of_the_batch(cuda):
    """The same call twice, a cloud alone against the same cloud at position 2 of 3, and b = 1 against b = 3: identical words in
    all five outputs, without a column split and with one."""
    for n, m in ((200, 131), (700, 1300)):
        x, y = ref.clouds(n + m, 3, n, m)
        eps = ref.schedule(8, ref.diameter(x, y))
        first, second = _run(cuda, x, y, eps), _run(cuda, x, y, eps)
        alone, head = _run(cuda, x[2:], y[2:], eps), _run(cuda, x[:1], y[:1], eps)
        for name in ALL:
            assert _same_words(first[name], second[name]), (name, n, m)
            assert _same_words(first[name][2:], alone[name]), (name, n, m)
            assert _same_words(first[name][:1], head[name]), (name, n, m)


def test_aliased_clouds_cost_exactly_zero(cuda):
    for n in (100, 513):
        x, _ = ref.clouds(n, 2, n, n)
        xd = _dev(x, cuda)
        got = _call(xd, xd, ref.schedule(8, ref.diameter(x, x)))
        for name in ALL:
            assert (got[name].view(np.uint32) == 0).all(), (name, n)


def test_temperature_far_below_the_scale(cuda):
    """eps = 1e-6 diameter^2 at every step: the largest argument of a row is about 1e6 above most of the others, so a row
    whose terms were measured against a stale reference would sum to 0 and return an infinity.  Potentials finite and
    inside the bar; the gradients (one-hot plans) only have to be finite."""
    for k, (n, m) in enumerate(((300, 517), (64, 9))):
        scale, centre = ref.SCALES[k]
        x, y = ref.clouds(50 + k, 2, n, m, scale, centre)
        eps = [float(np.float32(1e-6 * ref.diameter(x, y) ** 2))] * 4
        got = _run(cuda, x, y, eps)
        for name in ALL:
            assert np.isfinite(got[name]).all(), name
        mult = ref.Result(x, y, eps).check({name: got[name] for name in ('cost', 'pot_x', 'pot_y')}, (n, m))
        print(f'sinkhorn eps = 1e-6 d^2, {n} x {m}: {mult}')


def test_every_subset_of_the_outputs(cuda):
    """Each of the 31 non-empty subsets returns the words of the full call (the guards are checked in ``_call``), debiased
    and not, without a column split and with one; with no output nothing is written."""
    for (n, m), debias in (((150, 90), True), ((150, 90), False), ((600, 300), True)):
        x, y = ref.clouds(n, 2, n, m)
        xd, yd, eps = _dev(x, cuda), _dev(y, cuda), ref.schedule(2, ref.diameter(x, y))
        full = _call(xd, yd, eps, debias)
        for k in range(1, 5):
            for want in itertools.combinations(ALL, k):
                got = _call(xd, yd, eps, debias, want)
                for name in want:
                    assert _same_words(got[name], full[name]), (want, name, n, debias)
        assert _call(xd, yd, eps, debias, ()) == {}


def test_non_finite_input_stays_in_its_cloud(cuda):
    """One cloud of three has a NaN and an infinite coordinate: the call returns, that cloud's cost is not finite, the other
    clouds' words are unchanged."""
    n, m = 400, 300
    x, y = ref.clouds(78, 3, n, m)
    eps = ref.schedule(8, ref.diameter(x, y))
    clean = _run(cuda, x, y, eps)
    x[1, 3, 0], y[1, 7, 2] = np.nan, np.inf
    sick = _run(cuda, x, y, eps)
    assert not np.isfinite(sick['cost'][1])
    for name in ALL:
        for k in (0, 2):
            assert _same_words(sick[name][k], clean[name][k]), (name, k)


def test_refusals_leave_the_buffers_alone(cuda):
    """``PCC_EINVAL`` for every size, schedule and null pointer the contract refuses; b = 0 is accepted."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    x = torch.zeros(8, 3, device=cuda)
    outs = [torch.full((64,), SENTINEL, device=cuda) for _ in ALL]
    stream = torch.cuda.current_stream(cuda).cuda_stream
    good = (ctypes.c_float * 2)(1.0, 0.5)

    def status(b, n, m, steps=2, eps=good, ptrs=None):
        ptrs = [x.data_ptr(), x.data_ptr()] if ptrs is None else ptrs
        return L.pcc_sinkhorn(b, n, m, *ptrs, steps, None if eps is None else ctypes.cast(eps, ctypes.c_void_p), 1, *[o.data_ptr() for o in outs], stream)

    for b, n, m in ((1, 0, 8), (1, 8, 0), (1, 65537, 8), (1, 8, 65537), (65536, 8, 8), (-1, 8, 8)):
        assert status(b, n, m) == PCC_EINVAL, (b, n, m)
    for steps in (0, 257):
        assert status(1, 8, 8, steps) == PCC_EINVAL, steps
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert status(1, 8, 8, eps=(ctypes.c_float * 2)(1.0, bad)) == PCC_EINVAL, bad
    assert status(1, 8, 8, eps=None) == PCC_EINVAL
    for missing in range(2):
        ptrs = [x.data_ptr(), x.data_ptr()]
        ptrs[missing] = None
        assert status(1, 8, 8, ptrs=ptrs) == PCC_EINVAL, missing
        assert L.pcc_last_error().decode() == 'sinkhorn: null pointer'
    assert status(0, 8, 8) == 0
    torch.cuda.synchronize()
    for o in outs:
        assert (o.cpu().numpy() == np.float32(SENTINEL)).all()


def test_every_split_inside_the_bars(cuda):
    """The number of column slices forced through the ``sinkhorn_split`` switch -- every value the product can choose
    (1, 2, 4, 8, 16), an odd one and one above the most the kernel takes -- against the reference, and against the
    product's choice (the switch at 0).  The orders of summation differ, so the words may: every variant is held to
    the reference's bars and its potentials to ``ref.BAR_SPLIT`` U of the product's."""
    for (n, m), debias in (((700, 1300), True), ((257, 4100), False)):
        x, y = ref.clouds(n * m, 2, n, m)
        eps = ref.schedule(8, ref.diameter(x, y))
        want = ref.Result(x, y, eps, debias)
        xd, yd = _dev(x, cuda), _dev(y, cuda)
        product = _call(xd, yd, eps, debias)
        # (4100 columns hold every slice count: there each allowance 1 .. 16 is also the number of slices taken)
        for split in (1, 2, 3, 4, 8, 16, 99) if debias else tuple(range(1, 17)) + (99,):
            assert debias or ref.slices(n, m, debias, split) == min(split, 16)
            with _split(split):
                got = _call(xd, yd, eps, debias)
            apart = max(float((np.abs(got[name].astype(np.float64) - product[name]) / want.U[:, None]).max()) for name in ('pot_x', 'pot_y'))
            print(f'sinkhorn {n} x {m} split {split}: {want.check(got, (n, m, split))}, {apart:.3f} U from the product')
            assert apart <= ref.BAR_SPLIT, (n, m, split, apart)


def test_python_layer(cuda):
    """``loss.backward()`` with a non-uniform upstream gradient, float32 and float64, against the C entry; ``requires_grad``
    on one input only; ``return_potentials``; the default diameter; a CPU tensor takes the torch path; a non-contiguous,
    wrong-dtype or wrong-device tensor raises through ``_lib.ptr``."""
    from pointcloudcounterfactual_amd import losses

    b, n, m = 3, 300, 200
    x, y = ref.clouds(91, b, n, m)
    eps = losses.sinkhorn_schedule(0.05, 0.5, ref.diameter(x, y))
    xd, yd = _dev(x, cuda), _dev(y, cuda)
    raw = _call(xd, yd, eps)
    up = np.array([1.0, -2.0, 0.5], dtype=np.float32)  # powers of two: scaling by them is exact
    for dtype in (torch.float32, torch.float64):
        tx, ty = xd.clone().requires_grad_(True), yd.clone().requires_grad_(True)
        loss = losses.sinkhorn_divergence(tx, ty)  # (the diameter rule gives the schedule above)
        assert loss.dtype == torch.float32 and _same_words(loss.detach().cpu().numpy(), raw['cost'])
        (loss.to(dtype) * _dev(up, cuda).to(dtype)).sum().backward()
        assert tx.grad.dtype == torch.float32
        assert _same_words(tx.grad.cpu().numpy(), raw['grad_x'] * up[:, None, None])
        assert _same_words(ty.grad.cpu().numpy(), raw['grad_y'] * up[:, None, None])
    for needs in ((True, False), (False, True)):
        tx, ty = xd.clone().requires_grad_(needs[0]), yd.clone().requires_grad_(needs[1])
        losses.sinkhorn_divergence(tx, ty, eps=eps).sum().backward()
        assert (tx.grad is not None, ty.grad is not None) == needs
        asked, name = (tx, 'grad_x') if needs[0] else (ty, 'grad_y')
        assert _same_words(asked.grad.cpu().numpy(), raw[name])
    with torch.no_grad():  # (inputs that require grad, no gradient work: the same cost)
        quiet = losses.sinkhorn_divergence(xd.clone().requires_grad_(True), yd, eps=eps)
    assert not quiet.requires_grad and _same_words(quiet.cpu().numpy(), raw['cost'])
    cost, p1, p2 = losses.sinkhorn_divergence(xd, yd, eps=eps, return_potentials=True)
    assert _same_words(cost.cpu().numpy(), raw['cost']) and _same_words(p1.cpu().numpy(), raw['pot_x']) and _same_words(p2.cpu().numpy(), raw['pot_y'])
    plain = losses.sinkhorn_divergence(xd, yd, eps=eps, debias=False)
    assert _same_words(plain.cpu().numpy(), _call(xd, yd, eps, False, ('cost',))['cost'])
    cpu_loss = losses.sinkhorn_divergence(torch.from_numpy(x), torch.from_numpy(y), eps=eps)
    want = ref.Result(x, y, eps)
    want.check({'cost': cpu_loss.numpy()})
    want.check(raw)
    with pytest.raises(RuntimeError, match='must be contiguous'):
        losses.sinkhorn_divergence(xd.transpose(0, 1).contiguous().transpose(0, 1), yd, eps=eps)
    with pytest.raises(RuntimeError, match='must be torch.float32'):
        losses.sinkhorn_divergence(xd.double(), yd.double(), eps=eps)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        losses.sinkhorn_divergence(xd, torch.from_numpy(y), eps=eps)
