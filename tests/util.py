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
