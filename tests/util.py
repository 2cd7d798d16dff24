"""Synthetic clouds shared by tests, smoke and bench."""

from __future__ import annotations

import numpy as np


def ref_cloud(rng: np.random.Generator, b: int, n: int) -> np.ndarray:
    """Surface-like cloud: directions uniform on the sphere, radius U(0.3,1)^(1/3), centred, max-norm 1."""
    v = rng.standard_normal((b, n, 3))
    v /= np.linalg.norm(v, axis=2, keepdims=True) + 1e-12
    r = rng.uniform(0.3, 1.0, (b, n, 1)) ** (1.0 / 3.0)
    p = v * r
    p -= p.mean(axis=1, keepdims=True)
    p /= np.maximum(np.linalg.norm(p, axis=2).max(axis=1), 1e-12)[:, None, None]
    if n == 1:
        p = v * r  # a single point cannot be centred; keep it off the origin
    return p.astype(np.float32)


def recon_cloud(rng: np.random.Generator, ref: np.ndarray, m: int | None = None, sigma: float = 0.02) -> np.ndarray:
    """A 'trained autoencoder' output: row-permuted reference (optionally resampled to m points) + noise."""
    b, n, _ = ref.shape
    m = n if m is None else m
    out = np.empty((b, m, 3), np.float32)
    for i in range(b):
        perm = rng.permutation(n)
        idx = perm[np.arange(m) % n]
        out[i] = ref[i, idx] + rng.normal(0.0, sigma, (m, 3)).astype(np.float32)
    return out


def uniform_cloud(rng: np.random.Generator, b: int, n: int) -> np.ndarray:
    return rng.random((b, n, 3), dtype=np.float32)


def pair(seed: int, b: int, n: int, m: int | None = None, kind: str = 'recon'):
    rng = np.random.default_rng(seed)
    m = n if m is None else m
    if kind == 'uniform':
        return uniform_cloud(rng, b, n), uniform_cloud(rng, b, m)
    ref = ref_cloud(rng, b, m)
    return recon_cloud(rng, ref, n), ref


def raised(kind: type, fn, *args, **kwargs) -> str:
    """The message of the exception ``fn(*args, **kwargs)`` raises, which must be exactly a ``kind``."""
    try:
        fn(*args, **kwargs)
    except Exception as e:
        assert type(e) is kind, (type(e), kind, str(e))
        return str(e)
    raise AssertionError(f'{getattr(fn, "__name__", fn)} raised nothing')


def c_status(lib, fn, *args) -> tuple[int, str]:
    """``(return code, pcc_last_error())`` of one call into the C ABI."""
    rc = fn(*args)
    return rc, lib.pcc_last_error().decode()


MATCH_COST_RTOL = 1e-5  # the approximate EMD's cost against the float64 recurrence (tests/test_gpu_structural.py, smoke())


def check_match_cost(oracle, a: np.ndarray, b: np.ndarray, cost: np.ndarray, grad1: np.ndarray | None = None,
                     grad2: np.ndarray | None = None) -> None:
    """``match_cost`` of the clouds ``a``, ``b`` inside the bars of tests/test_gpu_structural.py and ``smoke()``: the cost
    MATCH_COST_RTOL relative to the float64 recurrence; the gradients within 3x the spread of the oracle's own legitimate
    float32 evaluations (exp modes 0-3) around the float64 gradients, floor 5e-5 of the largest component."""
    om64, _ = oracle.approxmatch_f64(a, b)
    np.testing.assert_allclose(cost, oracle.matchcost_f64(a, b, om64), rtol=MATCH_COST_RTOL)
    if grad1 is None:
        return
    h1, h2 = oracle.matchcostgrad_f64(a, b, om64)
    scale = max(np.abs(h1).max(), np.abs(h2).max())
    spread = 0.0
    try:
        for mode in (0, 1, 2, 3):
            oracle.set_exp_mode(mode)
            om, _ = oracle.approxmatch(a, b)
            f1, f2 = oracle.matchcostgrad(a, b, om)
            spread = max(spread, np.abs(f1 - h1).max(), np.abs(f2 - h2).max())
    finally:
        oracle.set_exp_mode(0)
    bar = max(3 * spread, 5e-5 * scale)
    assert np.abs(grad1 - h1).max() <= bar and np.abs(grad2 - h2).max() <= bar, (np.abs(grad1 - h1).max(), np.abs(grad2 - h2).max(), bar)


class host_independent_math:
    """Context manager: ``torch.sqrt`` / ``torch.exp`` of float32 tensors rounded from float64 while it is active.  Torch
    hands float32 sqrt / exp on the CPU to a vector-math library whose code path, and last bit, depends on the CPU
    vendor; rounded from float64 (sqrt exactly, exp to far below half a float32 ulp) the bits are the same on every
    host, so a golden vector made with it can be compared bit for bit anywhere."""

    def __enter__(self):
        import torch

        self._orig = torch.sqrt, torch.exp
        sqrt, exp = self._orig

        def wrap(fn):
            return lambda t, *a, **k: fn(t.double(), *a, **k).float() if t.dtype == torch.float32 else fn(t, *a, **k)

        torch.sqrt, torch.exp = wrap(sqrt), wrap(exp)
        return self

    def __exit__(self, *exc):
        import torch

        torch.sqrt, torch.exp = self._orig
        return False
