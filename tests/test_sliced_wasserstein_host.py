"""CPU tests of the sliced Wasserstein loss: the torch path of ``losses.sliced_wasserstein`` against the numpy reference of
tests/sliced_wasserstein_reference.py word for word, the reference itself against closed forms in float64, autograd through
the torch path against the float64 gradient, and the checks ``pcc_sliced_wasserstein`` makes before any HIP call."""

import os

import numpy as np
import pytest
import torch

from pointcloudcounterfactual_amd.losses import sliced_wasserstein, torch_sliced_wasserstein  # noqa: F401  (no feature, no test)
from tests import sliced_wasserstein_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCC_OK, PCC_EINVAL = 0, -22


def _same_words(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _torch_path(x, y, theta):
    from pointcloudcounterfactual_amd.losses import torch_sliced_wasserstein

    cost, cost_p = torch_sliced_wasserstein(torch.from_numpy(x), torch.from_numpy(y), torch.from_numpy(theta), return_per_direction=True)
    return cost.numpy(), cost_p.numpy()


@pytest.mark.parametrize('n', ref.N_HOST)
def test_torch_path_equals_the_reference_word_for_word(n):
    """Every p of the reduced grid; b in {1, 3} and the clouds' scale rotate."""
    for j, p in enumerate(ref.P_HOST):
        b = (1, 3)[j % 2]
        scale, shift = ((1.0, 0.0), (1000.0, 300.0), (1e-3, 0.0))[j % 3]
        x, y = ref.clouds(100 * n + p, b, n, scale, shift)
        theta = ref.unit_directions(n + p, p)
        want = ref.Forward(x, y, theta)
        cost, cost_p = _torch_path(x, y, theta)
        assert _same_words(cost_p, want.cost_p), (n, p)
        assert _same_words(cost, want.cost), (n, p)


def test_torch_path_on_ties_signed_zeros_and_non_finite_input():
    """Lattice clouds with duplicates and zeros of both signs on directions with zero components: word for word; a cloud
    with NaN and infinite coordinates gets a NaN cost and leaves the others' words alone."""
    for n, p in ((65, 8), (256, 4)):
        x, y = ref.lattice_clouds(n, 3, n)
        theta = ref.dyadic_directions(p, p)
        want = ref.Forward(x, y, theta)
        cost, cost_p = _torch_path(x, y, theta)
        assert _same_words(cost_p, want.cost_p) and _same_words(cost, want.cost)
    x, y = ref.clouds(5, 3, 100)
    theta = ref.unit_directions(6, 9)
    clean = ref.Forward(x, y, theta)
    x[1, 3, 0], x[1, 50, 1], y[1, 7, 2] = np.nan, np.inf, -np.inf
    sick = ref.Forward(x, y, theta)
    cost, cost_p = _torch_path(x, y, theta)
    assert np.isnan(cost[1]) and np.isnan(sick.cost[1])
    for k in (0, 2):
        assert _same_words(cost[k], clean.cost[k]) and _same_words(cost_p[k], clean.cost_p[k]) and _same_words(sick.cost[k], clean.cost[k])


def test_reference_against_closed_forms():
    """In float64 terms: a translated cloud costs mean_p (theta_p . t)^2, a cloud against itself 0, and the order of a
    cloud's points does not matter (``cost_p`` word for word: the sorted values are the same)."""
    rng = np.random.default_rng(1)
    b, n, p = 2, 300, 16
    x, _ = ref.clouds(2, b, n)
    theta = ref.unit_directions(3, p)
    t = np.array([0.5, -0.25, 0.125], dtype=np.float32)
    moved = ref.Forward(x, (x + t).astype(np.float32), theta)
    expect = np.mean((theta.astype(np.float64) @ t.astype(np.float64)) ** 2)
    # d_r is a difference of two rounded projections of magnitude <= 6: |d_r - theta . t| <= delta = 1e-6 (five roundings
    # of 6 u), so d_r^2 is off by at most 2 |t| delta = 1.2e-6 against a cost of about 0.1, and the sums add gamma(n + p) =
    # 2e-5 relative: 1e-4 relative leaves a factor of three
    assert np.allclose(moved.cost.astype(np.float64), expect, rtol=1e-4, atol=0)
    same = ref.Forward(x, x.copy(), theta)
    assert (same.cost.view(np.uint32) == 0).all() and (same.cost_p.view(np.uint32) == 0).all()
    _, y = ref.clouds(4, b, n)
    base = ref.Forward(x, y, theta)
    shuffled = ref.Forward(x[:, rng.permutation(n)], y[:, rng.permutation(n)], theta)
    assert _same_words(shuffled.cost_p, base.cost_p) and _same_words(shuffled.cost, base.cost)


def test_reference_gradient_against_central_differences():
    """The float64 gradient for held permutations is the derivative of the float64 cost where the order does not change."""
    b, n, p = 1, 6, 5
    x, y = ref.clouds(7, b, n)
    theta = ref.unit_directions(8, p)
    fwd = ref.Forward(x, y, theta)
    grad = ref.Grad(fwd, theta)

    def cost64(xv, yv):
        a = np.sort(np.einsum('bnc,pc->bpn', xv, theta.astype(np.float64)), axis=2)
        c = np.sort(np.einsum('bnc,pc->bpn', yv, theta.astype(np.float64)), axis=2)
        return ((a - c) ** 2).sum((1, 2)) * float(fwd.inv)

    h = 1e-6
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    for j in range(n):
        for c in range(3):
            step = np.zeros_like(x64)
            step[0, j, c] = h
            num_x = (cost64(x64 + step, y64) - cost64(x64 - step, y64)) / (2 * h)
            num_y = (cost64(x64, y64 + step) - cost64(x64, y64 - step)) / (2 * h)
            # (the float32 d of the reference against the float64 one: a few 1e-7 relative to gradients of about 0.1)
            assert abs(num_x[0] - grad.gx[0, j, c]) < 1e-5 and abs(num_y[0] - grad.gy[0, j, c]) < 1e-5


@pytest.mark.parametrize('needs', [(True, True), (True, False), (False, True)])
def test_autograd_through_the_torch_path(needs):
    """``loss.backward()`` with a non-uniform float64 upstream gradient against the float64 gradient, inside the
    summation bound; an input that does not ask gets no gradient; CPU tensors reach the torch path from the public name."""
    from pointcloudcounterfactual_amd import losses

    b, n, p = 3, 129, 17
    x, y = ref.clouds(11, b, n)
    theta = ref.unit_directions(12, p)
    grad = ref.Grad(ref.Forward(x, y, theta), theta)
    tx, ty = torch.from_numpy(x).requires_grad_(needs[0]), torch.from_numpy(y).requires_grad_(needs[1])
    loss = losses.sliced_wasserstein(tx, ty, directions=torch.from_numpy(theta))
    assert type(loss.grad_fn).__name__ == 'TorchSlicedWassersteinFunctionBackward'
    assert _same_words(loss.detach().numpy(), ref.Forward(x, y, theta).cost)
    up = np.array([1.0, -2.0, 0.5])  # powers of two: the upstream scale is exact
    (loss.double() * torch.from_numpy(up)).sum().backward()
    got = [None if t.grad is None else t.grad.numpy() / up[:, None, None] for t in (tx, ty)]
    assert (got[0] is not None, got[1] is not None) == needs
    grad.check_bound(*got)


def test_random_directions_and_argument_checks():
    from pointcloudcounterfactual_amd import losses

    g = torch.Generator().manual_seed(3)
    theta = losses.random_directions(128, 'cpu', g)
    assert theta.shape == (128, 3) and theta.dtype == torch.float32
    assert torch.allclose(theta.norm(dim=1), torch.ones(128), atol=1e-6)
    assert torch.equal(theta, losses.random_directions(128, torch.device('cpu'), torch.Generator().manual_seed(3)))
    x = torch.zeros(2, 8, 3)
    assert losses.sliced_wasserstein(x, x, 4, generator=g).shape == (2,)
    with pytest.raises(RuntimeError, match='t1 must be torch.float32'):
        losses.sliced_wasserstein(x.double(), x, directions=theta)
    with pytest.raises(ValueError):
        losses.sliced_wasserstein(x, torch.zeros(2, 9, 3), directions=theta)
    with pytest.raises(ValueError):
        losses.sliced_wasserstein(x, x, directions=torch.zeros(4, 2))


def test_entry_checks_before_any_launch():
    """``pcc_sliced_wasserstein`` refuses bad sizes and a null input with ``PCC_EINVAL`` before it touches the device (the
    pointers are dummies, never dereferenced), accepts an empty batch, and enqueues nothing when no output is asked for."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    d = 0x1000

    def status(b, n, p, x=d, y=d, theta=d, outs=(d, d, d, d)):
        rc = L.pcc_sliced_wasserstein(b, n, p, x, y, theta, *outs, None)
        return rc, L.pcc_last_error().decode()

    assert status(1, 0, 4) == (PCC_EINVAL, 'sliced_wasserstein: bad size')
    assert status(1, 4, 0) == (PCC_EINVAL, 'sliced_wasserstein: bad size')
    assert status(-1, 4, 4) == (PCC_EINVAL, 'sliced_wasserstein: bad size')
    assert status(1, 8193, 4) == (PCC_EINVAL, 'sliced_wasserstein: cloud too large (n > PCC_SW_MAX_N)')
    assert status(65536, 4, 4) == (PCC_EINVAL, 'sliced_wasserstein: batch too large')
    assert status(65535, 4, 32769) == (PCC_EINVAL, 'sliced_wasserstein: too many slices (b * p >= 2^31)')
    for missing in range(3):
        ptrs = [None if i == missing else d for i in range(3)]
        assert status(1, 4, 4, *ptrs) == (PCC_EINVAL, 'sliced_wasserstein: null pointer'), missing
    assert status(0, 4, 4) == (PCC_OK, '')
    assert status(0, 4, 4, None, None, None) == (PCC_OK, '')
    assert status(2, 4, 4, outs=(None, None, None, None)) == (PCC_OK, '')
    text = open(os.path.join(ROOT, 'include', 'pcc_structural.h')).read()
    assert '#define PCC_SW_MAX_N 8192' in text and f'#define PCC_SW_CHUNK {ref.CHUNK}' in text
