"""CPU tests of the Sinkhorn divergence: the float64 reference of tests/sinkhorn_reference.py against closed forms, the
temperature schedule, the float32 torch path of ``losses.sinkhorn_divergence`` inside the kernel's bars, autograd through
it, and the checks ``pcc_sinkhorn`` makes before any HIP call."""

import ctypes
import os

import numpy as np
import pytest
import torch

from pointcloudcounterfactual_amd.losses import sinkhorn_divergence, sinkhorn_schedule, torch_sinkhorn  # noqa: F401  (no feature, no test)
from tests import sinkhorn_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCC_OK, PCC_EINVAL = 0, -22
HOST_GRID = ((64, 65), (257, 129), (513, 300), (1025, 1024))  # the sizes the bars' float32 baseline was measured on


def test_reference_single_points_cost_half_the_squared_distance():
    """n = m = 1, debiased: p* = q* = 0 and f* + g* = C whatever the schedule: cost = |x - y|^2 / 2, grad_x = x - y."""
    rng = np.random.default_rng(0)
    x, y = rng.standard_normal((2, 1, 3)).astype(np.float32), rng.standard_normal((2, 1, 3)).astype(np.float32)
    for eps in ([0.3], [4.0, 1.0, 0.01], ref.schedule(8, 2.0)):
        r = ref.Result(x, y, eps)
        d = x.astype(np.float64) - y.astype(np.float64)
        assert np.allclose(r.cost, 0.5 * (d * d).sum((1, 2)), rtol=1e-14, atol=0)
        assert np.allclose(r.grad_x, d, rtol=1e-13, atol=1e-15) and np.allclose(r.grad_y, -d, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('steps', [1, 2, 8])
def test_reference_one_target_point_gives_the_mean_cost(steps):
    """m = 1, debias off: the plan is forced, cost = mean_i C(x_i, y) for any T >= 1."""
    x, y = ref.clouds(1, 2, 37, 1)
    r = ref.Result(x, y, ref.schedule(steps, ref.diameter(x, y)), debias=False)
    d = x.astype(np.float64) - y.astype(np.float64)
    assert np.allclose(r.cost, 0.5 * (d * d).sum(-1).mean(1), rtol=4e-15, atol=0)  # (holds to 4e-16: a margin of ten)


def test_reference_a_cloud_against_itself_costs_exactly_zero():
    x, _ = ref.clouds(2, 2, 50, 50)
    r = ref.Result(x, x, ref.schedule(8, ref.diameter(x, x)))
    assert (r.cost == 0).all() and (r.grad_x == 0).all() and (r.grad_y == 0).all() and (r.pot_x == 0).all()


def _converged(x64, y64, eps, steps):
    """The undebiased cost and potentials after ``steps`` symmetric rounds at one temperature, float64, one cloud."""
    c = ref.pair_cost(x64, y64)
    f, g = ref.softmin(eps, c)[0], ref.softmin(eps, c.T)[0]
    for _ in range(steps):
        f, g = 0.5 * (f + ref.softmin(eps, c, g)[0]), 0.5 * (g + ref.softmin(eps, c.T, f)[0])
    return f, g, c


def test_reference_plan_marginals_after_convergence():
    """4000 rounds at eps = 0.05: the plan a_i b_j exp((f_i + g_j - C_ij) / eps) has row sums 1/n and column sums 1/m."""
    x, y = ref.clouds(3, 1, 5, 6)
    f, g, c = _converged(x[0].astype(np.float64), y[0].astype(np.float64), 0.05, 4000)
    plan = np.exp((f[:, None] + g[None, :] - c) / 0.05) / (5 * 6)
    assert np.allclose(plan.sum(1), 1 / 5, rtol=1e-12) and np.allclose(plan.sum(0), 1 / 6, rtol=1e-12)


def test_reference_gradient_is_the_derivative_of_the_converged_cost():
    """n = 5, m = 6: the closed-form gradient (potentials held constant) against central differences of the converged
    debiased cost.  At convergence the potentials are stationary, so the two agree (envelope theorem)."""
    x, y = ref.clouds(4, 1, 5, 6)
    eps, steps, h = 0.05, 4000, 1e-6

    def cost(u, v):
        f, g, _ = _converged(u, v, eps, steps)
        p, _, _ = _converged(u, u, eps, steps)
        q, _, _ = _converged(v, v, eps, steps)
        return (f - p).mean() + (g - q).mean()

    r = ref.Result(x, y, [eps] * steps)
    x64, y64 = x[0].astype(np.float64), y[0].astype(np.float64)
    assert abs(r.cost[0] - cost(x64, y64)) < 1e-13
    for cloud, grad in ((0, r.grad_x[0]), (1, r.grad_y[0])):
        for i, c in ((0, 0), (2, 1), (4, 2)):
            step = np.zeros_like(y64 if cloud else x64)
            step[i, c] = h
            num = (cost(x64, y64 + step) - cost(x64, y64 - step)) / (2 * h) if cloud else (cost(x64 + step, y64) - cost(x64 - step, y64)) / (2 * h)
            assert abs(num - grad[i, c]) < 1e-8, (cloud, i, c, num, grad[i, c])


def test_schedule():
    got = sinkhorn_schedule(0.05, 0.5, 2.0)
    assert len(got) == 8 and np.allclose(got, [4, 4, 1, 0.25, 0.0625, 0.015625, 0.00390625, 0.0025], rtol=1e-12, atol=0)
    assert np.allclose(ref.schedule(8, 2.0), got, rtol=1e-7)  # (the grids' schedule is this one, rounded to float32)
    assert sinkhorn_schedule(3.0, 0.5, 2.0) == [4.0, 9.0]  # (blur above the diameter: an empty range)
    for bad in ((0.0, 0.5, 2.0), (0.05, 1.0, 2.0), (0.05, 0.5, float('inf'))):
        with pytest.raises(ValueError):
            sinkhorn_schedule(*bad)


def _torch_outputs(x, y, eps, debias):
    tx, ty = torch.from_numpy(x).requires_grad_(True), torch.from_numpy(y).requires_grad_(True)
    cost, p1, p2 = torch_sinkhorn(tx, ty, eps, debias, return_potentials=True)
    cost.sum().backward()
    return {'cost': cost.detach().numpy(), 'pot_x': p1.numpy(), 'pot_y': p2.numpy(), 'grad_x': tx.grad.numpy(), 'grad_y': ty.grad.numpy()}


@pytest.mark.parametrize('case', range(len(HOST_GRID)))
def test_torch_path_inside_the_bars(case):
    """``torch_sinkhorn`` against the float64 reference in the kernel's bars; the scale of the clouds and debias rotate."""
    n, m = HOST_GRID[case]
    worst = {}
    for k, (scale, centre) in enumerate(ref.SCALES):
        x, y = ref.clouds(10 * case + k, 1, n, m, scale, centre)
        eps, debias = ref.schedule(8, ref.diameter(x, y)), (case + k) % 3 != 0
        mult = ref.Result(x, y, eps, debias).check(_torch_outputs(x, y, eps, debias), (n, m, scale))
        worst = {key: max(worst.get(key, 0.0), v) for key, v in mult.items()}
    print(f'torch path {n} x {m}: largest multiples {worst}')


def test_torch_path_aliased_clouds_cost_exactly_zero():
    x, _ = ref.clouds(5, 2, 130, 130)
    tx = torch.from_numpy(x).requires_grad_(True)
    cost, p1, p2 = torch_sinkhorn(tx, tx, ref.schedule(8, ref.diameter(x, x)), return_potentials=True)
    cost.sum().backward()
    for t in (cost.detach(), p1, p2, tx.grad):
        assert (t.numpy().view(np.uint32) == 0).all()


@pytest.mark.parametrize('needs', [(True, False), (False, True), (True, True)])
def test_autograd_with_a_non_uniform_upstream_gradient(needs):
    """``loss.backward()`` with a float64 upstream gradient of powers of two (exact scaling) against the float64 gradient;
    an input that does not ask gets none; CPU tensors reach the torch path from the public name."""
    b, n, m = 3, 40, 33
    x, y = ref.clouds(6, b, n, m)
    eps = ref.schedule(8, 2.0)
    want = ref.Result(x, y, eps)
    tx, ty = torch.from_numpy(x).requires_grad_(needs[0]), torch.from_numpy(y).requires_grad_(needs[1])
    loss = sinkhorn_divergence(tx, ty, eps=eps)
    assert type(loss.grad_fn).__name__ == 'TorchSinkhornFunctionBackward' and loss.dtype == torch.float32
    up = np.array([1.0, -2.0, 0.5])
    (loss.double() * torch.from_numpy(up)).sum().backward()
    assert (tx.grad is not None, ty.grad is not None) == needs
    got = {'cost': loss.detach().numpy()}
    if needs[0]:
        got['grad_x'] = tx.grad.numpy() / up[:, None, None]
    if needs[1]:
        got['grad_y'] = ty.grad.numpy() / up[:, None, None]
    want.check(got)


def test_no_gradient_work_under_no_grad(monkeypatch):
    """``needs_input_grad`` stays True under ``torch.no_grad()``; the node must not compute gradients nobody can ask for."""
    from pointcloudcounterfactual_amd import losses

    seen = []
    run = losses.TorchSinkhornFunction.run
    monkeypatch.setattr(losses.TorchSinkhornFunction, 'run', staticmethod(lambda *a: (seen.append(a[4:6]), run(*a))[1]))
    x, y = (torch.from_numpy(a).requires_grad_(True) for a in ref.clouds(8, 1, 6, 5))
    with torch.no_grad():
        assert not sinkhorn_divergence(x, y, diameter=2.0).requires_grad
        assert not torch_sinkhorn(x, y, [1.0, 0.1]).requires_grad
    sinkhorn_divergence(x, y.detach(), diameter=2.0).sum().backward()
    assert seen == [(False, False), (False, False), (True, False)] and x.grad is not None


def test_public_function_arguments():
    x, y = (torch.from_numpy(a) for a in ref.clouds(7, 2, 20, 31))
    diam = ref.diameter(x.numpy(), y.numpy())
    assert torch.equal(sinkhorn_divergence(x, y), sinkhorn_divergence(x, y, eps=sinkhorn_schedule(0.05, 0.5, diam)))
    assert torch.equal(sinkhorn_divergence(x, y, diameter=3.0), torch_sinkhorn(x, y, sinkhorn_schedule(0.05, 0.5, 3.0)))
    cost, p1, p2 = sinkhorn_divergence(x, y, debias=False, return_potentials=True)
    assert p1.shape == (2, 20) and p2.shape == (2, 31) and not p1.requires_grad
    assert torch.allclose(cost, p1.mean(1) + p2.mean(1), rtol=1e-5)
    assert (sinkhorn_divergence(torch.ones(1, 4, 3), torch.ones(1, 4, 3)) == 0).all()  # (diameter 0)
    with pytest.raises(RuntimeError, match='t1 must be torch.float32'):
        sinkhorn_divergence(x.double(), y)
    for bad in ((x, y[:1]), (x[..., :2], y), (x[0], y[0]), (x[:, :0], y)):
        with pytest.raises(ValueError):
            sinkhorn_divergence(*bad)
    for eps in ([], [1.0, 0.0], [float('nan')], [1.0] * 257):
        with pytest.raises(ValueError):
            sinkhorn_divergence(x, y, eps=eps)


def test_entry_checks_before_any_launch():
    """``pcc_sinkhorn`` refuses bad sizes, a bad schedule and a null input with ``PCC_EINVAL`` before it touches the device
    (the device pointers are dummies, never dereferenced), accepts an empty batch, and enqueues nothing when no output is
    asked for."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    d = 0x1000
    good = (ctypes.c_float * 3)(4.0, 1.0, 0.25)

    def status(b, n, m, steps=3, x=d, y=d, eps=good, outs=(d, d, d, d, d)):
        rc = L.pcc_sinkhorn(b, n, m, x, y, steps, None if eps is None else ctypes.cast(eps, ctypes.c_void_p), 1, *outs, None)
        return rc, L.pcc_last_error().decode()

    for b, n, m in ((1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, -4, 4)):
        assert status(b, n, m) == (PCC_EINVAL, 'sinkhorn: bad size')
    for n, m in ((65537, 4), (4, 65537)):
        assert status(1, n, m) == (PCC_EINVAL, 'sinkhorn: cloud too large (n, m <= 65536)')
    for steps in (0, -1, 257):
        assert status(1, 4, 4, steps) == (PCC_EINVAL, 'sinkhorn: bad number of steps (1 .. PCC_SINKHORN_MAX_STEPS)')
    assert status(65536, 4, 4) == (PCC_EINVAL, 'sinkhorn: batch too large')
    for missing in ('x', 'y', 'eps'):
        assert status(1, 4, 4, **{missing: None}) == (PCC_EINVAL, 'sinkhorn: null pointer'), missing
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        assert status(1, 4, 4, eps=(ctypes.c_float * 3)(4.0, 1.0, bad)) == (PCC_EINVAL, 'sinkhorn: eps must be finite and > 0'), bad
    assert status(0, 4, 4) == (PCC_OK, '')
    assert status(0, 4, 4, x=None, y=None, eps=None) == (PCC_OK, '')
    assert status(2, 4, 4, outs=(None,) * 5) == (PCC_OK, '')
    assert status(2, 4, 4, 2, eps=(ctypes.c_float * 3)(4.0, 1.0, 0.0), outs=(None,) * 5) == (PCC_OK, '')  # eps[2] is not part of the schedule
    text = open(os.path.join(ROOT, 'include', 'pcc_structural.h')).read()
    assert '#define PCC_SINKHORN_MAX_STEPS 256' in text
    hooks = open(os.path.join(ROOT, 'include', 'pcc_test_hooks.h')).read()
    assert 'PCC_TUNE_SINKHORN_SPLIT = 0,' in hooks and _lib.TUNING['sinkhorn_split'] == 0
