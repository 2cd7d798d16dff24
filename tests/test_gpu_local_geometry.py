"""GPU tests of the local-geometry op (``pcc_local_geometry`` / ``pcc_local_covariance_bwd`` through the C ABI and through
``neighbour_ops.local_covariance`` / ``local_geometry`` / ``estimate_normals``) against the numpy reference of
tests/local_geometry_reference.py: ``mean`` and ``cov`` word for word, every output asked for alone, independence of the
rest of the cloud and of the batch, the eigen stage inside the contract's bars against float64 ``eigh`` of the kernel's own
``cov``, its conventions and degenerate cases, exact scaling by powers of two, and the backward word for word on inputs
whose intermediates are exact, inside the summation bound on Gaussian ones, and through autograd."""

import numpy as np
import pytest
import torch

from tests import local_geometry_reference as ref
from tests.which_ran import ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

SENTINEL = -1234.5  # what the guard behind every output must keep
GUARD = 64
SHAPES = {'mean': (3,), 'cov': (3, 3), 'eval': (3,), 'evec': (3, 3), 'curv': ()}
ALL = tuple(SHAPES)


def _dev(a, cuda):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _guarded(shape, fill, cuda):
    """A flat buffer of ``prod(shape)`` floats of ``fill`` with GUARD sentinels behind them."""
    flat = torch.full((int(np.prod(shape)) + GUARD,), SENTINEL, dtype=torch.float32, device=cuda)
    flat[:int(np.prod(shape))] = fill
    return flat


def _open(flat, shape):
    """The payload of a guarded buffer as numpy; the guard must be untouched."""
    host = flat.cpu().numpy()
    size = int(np.prod(shape))
    assert (host[size:] == np.float32(SENTINEL)).all()
    return host[:size].reshape(shape).copy()


def _forward(xyz, idx, want=ALL):
    """``pcc_local_geometry`` on device tensors ``xyz[b,n,3]``, ``idx[b,m,k]`` for the outputs named in ``want`` (null
    pointers for the others): ``{name: numpy}``.  The outputs start as NaN: every element must be written."""
    from pointcloudcounterfactual_amd import _lib

    b, n, _ = xyz.shape
    m, k = idx.shape[1:]
    bufs = {name: _guarded((b, m) + SHAPES[name], float('nan'), xyz.device) for name in want}
    ptrs = [bufs[name].data_ptr() if name in bufs else None for name in ALL]
    _lib.call(_lib.lib.pcc_local_geometry, 'local_geometry', xyz.device, b, n, m, k, xyz.data_ptr(), idx.data_ptr(), *ptrs)
    return {name: _open(bufs[name], (b, m) + SHAPES[name]) for name in want}


def _backward(xyz, idx, mean, grad_cov, grad_mean):
    """``pcc_local_covariance_bwd`` on device tensors (``grad_mean`` may be None): ``grad_xyz[b,n,3]`` as numpy."""
    from pointcloudcounterfactual_amd import _lib

    b, n, _ = xyz.shape
    m, k = idx.shape[1:]
    gx = _guarded((b, n, 3), float('nan'), xyz.device)
    _, names = ran(lambda: _lib.call(_lib.lib.pcc_local_covariance_bwd, 'local_covariance_bwd', xyz.device, b, n, m, k, xyz.data_ptr(),
                                     idx.data_ptr(), mean.data_ptr(), grad_cov.data_ptr(),
                                     None if grad_mean is None else grad_mean.data_ptr(), gx.data_ptr()))
    assert names == ({ref.bwd_kernel(n): 1} if b and m else {}), (n, names)  # (the side of the LDS boundary the rule predicts)
    return _open(gx, (b, n, 3))


def _same_words(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_forward(cuda, xyz, idx, what):
    """All five outputs of one call: mean and cov word for word, the eigen outputs inside the bars and the conventions."""
    got = _forward(_dev(xyz, cuda), _dev(idx, cuda))
    mean, cov = ref.mean_cov(xyz, idx)
    assert _same_words(got['mean'], mean), what
    assert _same_words(got['cov'], cov), what
    ref.EigenBars(cov).check(got['eval'], got['evec'], got['curv'])
    ref.check_conventions(cov, got['eval'], got['evec'], got['curv'])
    return got


def _grid():
    """(m, k, b): every m with every k; b in {1, 3} rotates."""
    j = 0
    for m in ref.M_GRID:
        for k in ref.K_GRID:
            yield m, k, (1, 3)[j % 2]
            j += 1


@pytest.mark.parametrize('n', ref.N_GRID)
def test_mean_and_cov_word_for_word(cuda, n):
    """Every m and k of the grid, about a tenth of the slots -1, n or 2^40."""
    xyz_all = ref.cloud(n, n)
    for m, k, b in _grid():
        idx = ref.random_list(31 * m + k + n, ref.B_MAX, n, m, k)[:b]
        _check_forward(cuda, xyz_all[:b], idx, (m, k, b))


def test_boundaries_m_above_n_and_ball_query_lists(cuda):
    """n on both sides of the one boundary the dispatch has in n (the backward's; the forward has none) at m = 65, k = 5,
    one m > n case, and a ``ball_query`` list of each pad (``pad='first'`` repeats the first index: it counts as often as
    it occurs)."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    for n in ref.BOUNDARIES:
        _check_forward(cuda, ref.cloud(n, n, 2), ref.random_list(n, 2, n, 65, 5), n)
    _check_forward(cuda, ref.cloud(5, 64, 3), ref.random_list(6, 3, 64, 300, 4), 'm > n')
    xyz = ref.cloud(7, 500, 2)
    xd = _dev(xyz, cuda)
    centres = xd[:, :130].contiguous()
    for pad in ('first', 'none'):
        idx = ops.ball_query(xd, centres, 0.6, 17, pad=pad).cpu().numpy()
        assert (idx < 0).any() == (pad == 'none')
        _check_forward(cuda, xyz, idx, pad)


def test_each_output_alone_equals_the_full_call(cuda):
    """Null pointers for the other four; the guards behind the outputs stay untouched (``_open``)."""
    for n, m, k, b in ((300, 257, 16, 2), (64, 65, 33, 3), (5, 3, 2, 1)):
        xyz, idx = ref.cloud(n + m, n, b), ref.random_list(n + k, b, n, m, k)
        xd, idxd = _dev(xyz, cuda), _dev(idx, cuda)
        full = _forward(xd, idxd)
        for name in ALL:
            alone = _forward(xd, idxd, (name,))
            assert _same_words(alone[name], full[name]), (name, n, m, k)
        pair = _forward(xd, idxd, ('eval', 'curv'))
        assert _same_words(pair['eval'], full['eval']) and _same_words(pair['curv'], full['curv'])
        assert _forward(xd, idxd, ()) == {}


def test_independence_of_the_rest_of_the_cloud_and_of_the_batch(cuda):
    """A cloud of 1000 points against the same cloud with 13 000 never-referenced points appended, and the same rows at
    another batch position among other clouds: identical words in all five outputs."""
    m, k = 300, 16
    xyz = ref.cloud(11, 1000, 1)
    idx = ref.random_list(12, 1, 1000, m, k, bad=False)
    idx[0, ::7, 3] = -1
    base = _forward(_dev(xyz, cuda), _dev(idx, cuda))
    longer = np.concatenate([xyz, ref.cloud(13, 13000, 1, scale=50.0)], 1)
    more = _forward(_dev(longer, cuda), _dev(idx, cuda))
    others = ref.cloud(14, 14000, 2)
    batch = np.concatenate([others[:1], others[1:], longer], 0)
    idx3 = np.concatenate([ref.random_list(15, 2, 14000, m, k), idx], 0)
    moved = _forward(_dev(batch, cuda), _dev(idx3, cuda))
    for name in ALL:
        assert _same_words(more[name], base[name]), name
        assert _same_words(moved[name][2:], base[name]), name


def test_eigen_accuracy_against_float64_of_the_kernels_own_cov(cuda):
    """The bars of the contract on the constructions of ``accuracy_cases``: every row takes part."""
    worst = dict.fromkeys(ref.EigenBars.BARS, 0.0)
    for name, (xyz, idx) in ref.accuracy_cases().items():
        got = _forward(_dev(xyz, cuda), _dev(idx, cuda))
        assert _same_words(got['cov'], ref.mean_cov(xyz, idx)[1]), name
        figures = ref.EigenBars(got['cov']).measure(got['eval'], got['evec'], got['curv'])
        print(f'{name}: ' + ', '.join(f'{key} {value:.2f} U' for key, value in figures.items()))
        for key, value in figures.items():
            worst[key] = max(worst[key], value)
            assert value <= ref.EigenBars.BARS[key], (name, key, value)
        ref.check_conventions(got['cov'], got['eval'], got['evec'], got['curv'])
    print('eigen stage, the largest: ' + ', '.join(f'{key} {value:.2f} U' for key, value in worst.items()))


def test_conventions_and_degenerate_cases(cuda):
    """On the kernel's own output: the plane z = 0.25 returns (0, 0, 1), +0.0 and +0.0 exactly; axis-aligned lines and
    boxes (decoupled axes); cnt = 0, cnt = 1 and all slots equal; a NaN coordinate poisons exactly the rows that refer
    to it."""
    rng = np.random.default_rng(21)
    n, m, k = 400, 200, 16
    flat = rng.random((1, n, 3)).astype(np.float32)
    flat[:, :, 2] = 0.25
    idx = rng.integers(0, n, size=(1, m, k), dtype=np.int64)
    got = _check_forward(cuda, flat, idx, 'plane')
    assert (got['evec'][:, :, 0] == np.array([0, 0, 1], dtype=np.float32)).all()
    assert (got['eval'][:, :, 0].view(np.uint32) == 0).all() and (got['curv'].view(np.uint32) == 0).all()
    line = np.zeros((1, n, 3), dtype=np.float32)
    line[:, :, 1] = rng.standard_normal(n)
    got = _check_forward(cuda, line, idx, 'line')
    assert (got['evec'][:, :, 2] == np.array([0, 1, 0], dtype=np.float32)).all() and (got['eval'][:, :, :2] == 0).all()
    box = rng.integers(-3, 4, size=(1, n, 3)).astype(np.float32) * np.array([1, 0, 2], dtype=np.float32)
    _check_forward(cuda, box, idx, 'box')
    few = idx.copy()
    few[0, 0::3] = -1                 # cnt = 0
    few[0, 1::3, 1:] = n              # cnt = 1
    few[0, 2::3] = few[0, 2::3, :1]   # all slots equal
    quarters = (rng.integers(-8, 9, size=(1, n, 3)) / 4).astype(np.float32)  # (k equal summands add up exactly)
    got = _check_forward(cuda, quarters, few, 'few')
    assert (got['cov'].view(np.uint32) == 0).all() and (got['eval'].view(np.uint32) == 0).all()
    assert (got['evec'] == np.eye(3, dtype=np.float32)).all() and (got['mean'][0, 0::3].view(np.uint32) == 0).all()
    sick = rng.standard_normal((2, n, 3)).astype(np.float32)
    sick[0, 77, 1] = np.nan
    sick[1, 5, 0] = np.inf
    idx2 = rng.integers(0, n, size=(2, m, k), dtype=np.int64)
    got = _check_forward(cuda, sick, idx2, 'nan')
    touched = np.stack([(idx2[0] == 77).any(1), (idx2[1] == 5).any(1)])
    assert touched.any() and not touched.all()
    for name in ('eval', 'evec', 'curv'):
        bad = (got[name].reshape(2, m, -1).view(np.uint32) == ref.NAN_WORD).all(2)
        assert np.array_equal(bad, touched), name
        assert np.isfinite(got[name][~touched]).all()


def test_scaling_by_powers_of_two_is_exact(cuda):
    """The cloud times 2^10 and times 2^-10: ``eval`` scaled by exactly 4^(+-10), identical words in ``evec`` and ``curv``."""
    xyz = ref.cloud(31, 2000, 2)
    idx = ref.random_list(32, 2, 2000, 500, 16)
    idxd = _dev(idx, cuda)
    base = _forward(_dev(xyz, cuda), idxd)
    for e in (10, -10):
        got = _forward(_dev(xyz * np.float32(2.0 ** e), cuda), idxd)
        assert _same_words(got['eval'], base['eval'] * np.float32(4.0 ** e)), e
        assert _same_words(got['evec'], base['evec']) and _same_words(got['curv'], base['curv']), e
        assert _same_words(got['cov'], base['cov'] * np.float32(4.0 ** e)) and _same_words(got['mean'], base['mean'] * np.float32(2.0 ** e))


def _check_exact_backward(cuda, seed, b, n, m, k):
    xyz, idx, mean, gc, gm = ref.exact_backward_inputs(seed, b, n, m, k)
    xd, idxd, md, gcd, gmd = (_dev(a, cuda) for a in (xyz, idx, mean, gc, gm))
    assert _same_words(_forward(xd, idxd, ('mean',))['mean'], mean)
    ref.GradXyz(xyz, idx, mean, gc, gm).check_exact(_backward(xd, idxd, md, gcd, gmd))
    ref.GradXyz(xyz, idx, mean, gc, None).check_exact(_backward(xd, idxd, md, gcd, None))


@pytest.mark.parametrize('n', ref.N_GRID)
def test_backward_word_for_word_on_exact_inputs(cuda, n):
    """Integer coordinates, rows with 1, 2, 4 or 8 valid slots, integer gradients: every intermediate is exact, so
    ``grad_xyz`` is the float64 result, +0.0 where nothing points; with and without ``grad_mean``."""
    for m, k, b in _grid():
        _check_exact_backward(cuda, 41 * m + k + n, b, n, m, k)


@pytest.mark.parametrize('n', ref.BOUNDARIES)
def test_backward_on_both_sides_of_the_lds_boundary(cuda, n):
    """LDS bins at n = 8192, global atomics at 8193; m = 2049 also splits a sample's rows over several workgroups."""
    _check_exact_backward(cuda, n, 2, n, 65, 5)
    _check_exact_backward(cuda, n + 1, 1, n, 2049, 3)


def test_backward_on_generic_inputs_is_inside_the_summation_bound(cuda):
    """Gaussian inputs: |got - ref64| <= gamma(deg + 4) * sum |terms| per element (tests/local_geometry_reference.py);
    one list whose rows all name the same point, so that every atomic collides."""
    rng = np.random.default_rng(51)
    worst = 0.0
    for n, m, k, b in ((65, 257, 5, 3), (1025, 257, 16, 2), (300, 300, 33, 2), (8193, 65, 3, 2), (3, 257, 3, 3)):
        xyz = ref.cloud(n, n, b, shift=0.25)
        for kind, idx in (('random', ref.random_list(n, b, n, m, k)), ('hub', np.full((b, m, k), n - 1, dtype=np.int64))):
            mean, _ = ref.mean_cov(xyz, idx)
            gc = rng.standard_normal((b, m, 3, 3)).astype(np.float32)
            gm = rng.standard_normal((b, m, 3)).astype(np.float32)
            xd, idxd, md, gcd, gmd = (_dev(a, cuda) for a in (xyz, idx, mean, gc, gm))
            for with_mean in (True, False):
                back = ref.GradXyz(xyz, idx, mean, gc, gm if with_mean else None)
                gx = _backward(xd, idxd, md, gcd, gmd if with_mean else None)
                worst = max(worst, back.ratio(gx))
                back.check_bound(gx)
    print(f'grad_xyz: the largest error is {worst:.2f} of the bound')


@pytest.mark.parametrize('use_cov,use_mean', [(True, True), (True, False), (False, True)])
def test_autograd_equals_the_c_entry(cuda, use_cov, use_mean):
    """``local_covariance(...).backward`` against ``pcc_local_covariance_bwd`` on the same gradients (exact inputs, so the
    atomics' order does not matter): ``grad_mean`` reaches the library only when ``mean`` was used, a zero ``grad_cov``
    when only ``mean`` was; the forward equals the CPU path word for word."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    b, n, m, k = 2, 300, 130, 8
    xyz, idx, mean, gc, gm = ref.exact_backward_inputs(61, b, n, m, k)
    x = _dev(xyz, cuda).requires_grad_(True)
    cov_d, mean_d = ops.local_covariance(x, _dev(idx, cuda), return_mean=True)
    cov_c, mean_c = ops.local_covariance(torch.from_numpy(xyz), torch.from_numpy(idx), return_mean=True)
    assert _same_words(cov_d.detach().cpu().numpy(), cov_c.numpy()) and _same_words(mean_d.detach().cpu().numpy(), mean_c.numpy())
    loss = ((cov_d * _dev(gc, cuda)).sum() if use_cov else 0) + ((mean_d * _dev(gm, cuda)).sum() if use_mean else 0)
    loss.backward()
    want = _backward(_dev(xyz, cuda), _dev(idx, cuda), _dev(mean, cuda), _dev(gc if use_cov else np.zeros_like(gc), cuda),
                     _dev(gm, cuda) if use_mean else None)
    assert np.array_equal(x.grad.cpu().numpy(), want)
    ref.GradXyz(xyz, idx, mean, gc if use_cov else np.zeros_like(gc), gm if use_mean else None).check_exact(x.grad.cpu().numpy())


def test_python_layer(cuda):
    """``local_geometry`` and ``estimate_normals`` on the device against the C entry and the CPU path; refusals before
    anything is allocated; empty calls; the m = 0 backward zero-fills."""
    from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops

    b, n, k = 2, 700, 16
    xyz = np.concatenate([ref.sphere(71, n)[None], ref.sphere(72, n)[None]])
    xd = _dev(xyz, cuda)
    idxd = ops.knn(xd.transpose(1, 2).contiguous(), k)
    want = _forward(xd, idxd)
    geo = ops.local_geometry(xd.clone().requires_grad_(True), idxd)
    assert geo.cov.requires_grad and geo.mean.requires_grad
    assert not geo.eigenvalues.requires_grad and not geo.eigenvectors.requires_grad and not geo.curvature.requires_grad
    for t, name in zip(geo, ALL):
        assert _same_words(t.detach().cpu().numpy(), want[name]), name
    cpu = ops.local_geometry(torch.from_numpy(xyz), idxd.cpu())
    assert _same_words(cpu.cov.numpy(), want['cov']) and _same_words(cpu.mean.numpy(), want['mean'])
    normals, curv = ops.estimate_normals(xd, k, viewpoint=torch.zeros(3, device=cuda), return_curvature=True)
    assert ((normals * xd).sum(-1) < -0.9).all() and _same_words(curv.cpu().numpy(), want['curv'])
    assert torch.equal(ops.estimate_normals(xd, k), geo.eigenvectors[:, :, 0])
    assert (np.abs((cpu.eigenvectors[:, :, 0].numpy() * want['evec'][:, :, 0]).sum(-1)) > 0.999).all()
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.local_geometry(xd, idxd.cpu())
    with pytest.raises(RuntimeError):
        ops.local_covariance(xd.double(), idxd)
    with pytest.raises(ValueError):
        ops.local_covariance(xd, idxd[:1])
    for eb, em in ((0, n), (b, 0)):
        xe = xd[:eb].clone().requires_grad_(True)
        empty = ops.local_geometry(xe, idxd[:eb, :em])
        assert empty.cov.shape == (eb, em, 3, 3) and empty.curvature.shape == (eb, em) and empty.cov.device == xd.device
        (empty.cov.sum() + empty.mean.sum()).backward()
        assert xe.grad.shape == xe.shape and (xe.grad == 0).all()
    gx = torch.full((b, n, 3), SENTINEL, device=cuda)
    _lib.call(_lib.lib.pcc_local_covariance_bwd, 'local_covariance_bwd', cuda, b, n, 0, k, None, None, None, None, None, gx.data_ptr())
    assert (gx.cpu().numpy().view(np.uint32) == 0).all()
