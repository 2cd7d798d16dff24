"""GPU tests of the ball query (``pcc_ball_query`` through ``neighbour_ops.ball_query``) against the float64 reference of
tests/ball_query_reference.py: word for word where float32 is exact (lattice clouds, points exactly on the sphere
included), margin mode on generic clouds (bounds derived there), every kernel variant against the product's choice at the
sizes around every block, step and tile boundary, independence of batch, aliasing and the optional count, non-finite
input, the argument checks, and the CPU path against the kernel word for word."""

import numpy as np
import pytest
import torch

from tests.ball_query_reference import GENERIC_KINDS, GENERIC_SHAPES, BallReference, between_lattice, generic_cloud, kernel_of
from tests.fps_reference import lattice_cloud
from tests.which_ran import ran
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

RADII = (0.0625, 0.125, 0.25, 0.2, 10.0, float('inf'))  # 0.0625, 0.125, 0.25: lattice points exactly on the sphere
NSAMPLES = (1, 2, 31, 64, 65, 200)
PADS = ('first', 'none')
PATHS = (1, 2, 3, 4)  # ball_path values (include/pcc_test_hooks.h)
# the kernels walk the cloud in blocks of 64 and steps of 256 candidates; the LDS variants in tiles of 1024 and 4096
BOUNDARIES = sorted({c + d for c in (64, 256, 1024, 2048, 4096) for d in (-1, 0, 1)} | {8193})


def _ball(x, c, radius, nsample, pad, count=True):
    """numpy ``(idx, cnt)`` of device tensors ``x``, ``c``."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    out = ops.ball_query(x, c, radius, nsample, pad=pad, return_count=count)
    idx, cnt = out if count else (out, None)
    assert idx.dtype == torch.int64 and idx.shape == (x.shape[0], c.shape[1], nsample) and idx.device == x.device
    if not count:
        return idx.cpu().numpy()
    assert cnt.dtype == torch.int32 and cnt.shape == (x.shape[0], c.shape[1])
    return idx.cpu().numpy(), cnt.cpu().numpy()


def _forced(path, fn):
    """``fn()`` under ball_path = ``path`` (0: the product's choice), once its launch record holds the kernel of that
    variant and nothing else."""
    from pointcloudcounterfactual_amd import _lib

    with _lib.tuning('ball_path', path):
        got, names = ran(fn)
    assert set(names) == {kernel_of(path)}, (path, names)
    return got


def _lattice_centres(seed, x, m, between):
    """``m`` centres per cloud: points of the cloud itself (cycled when m > n), or points between lattice points."""
    if between:
        return between_lattice(seed, x.shape[0], m)
    return np.ascontiguousarray(x[:, np.arange(m) % x.shape[1]])


@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 129, 1025, 2049])
def test_exact_on_lattices(cuda, n):
    """Coordinates k/16 (centres also k/32): float32 is exact, so indices and counts equal the float64 reference word for
    word.  Balls smaller than, equal to and larger than nsample, empty balls (centres between the points of the 4^3 lattice
    at radius 0.0625), a first hit in the last partial block, duplicates everywhere."""
    for levels in (4, 16):
        x = lattice_cloud(1000 * levels + n, 3, n, levels)
        for m in (1, 3, 65):
            for between in (False, True):
                c = _lattice_centres(n + m, x, m, between)
                ref = BallReference(x, c)
                xs, cs = torch.from_numpy(x).to(cuda), torch.from_numpy(c).to(cuda)
                for radius in RADII:
                    for nsample in NSAMPLES:
                        for pad in PADS:
                            for b in (1, 3):
                                idx, cnt = _ball(xs[:b], cs[:b], radius, nsample, pad)
                                ref.check_exact(radius, nsample, pad, idx, cnt, rows=slice(0, b))


@pytest.mark.parametrize('kind', GENERIC_KINDS)
def test_generic_clouds_in_margin_mode(cuda, kind):
    """Uniform and Gaussian clouds, scaled by 100 and 1e-3 (radius alike) and translated by +50, centres = the first M
    points.  Ambiguous queries counted on the CPU for these cases: none, except 2 of 1536 (0.13 %) for gauss_+50 at radius
    0.5.  Radius 0.5 on the 2048 shape overflows nsample for most queries (the early exit)."""
    for b, n, m, r in GENERIC_SHAPES:
        x, scale = generic_cloud(11, b, n, kind)
        c = np.ascontiguousarray(x[:, :m])
        ref = BallReference(x, c)
        xs, cs = torch.from_numpy(x).to(cuda), torch.from_numpy(c).to(cuda)
        for radius in (r, 0.5) if n == 2048 else (r,):
            for k, nsample in enumerate((16, 64)):
                pad = PADS[k]
                idx, cnt = _ball(xs, cs, radius * scale, nsample, pad)
                ref.check_margin(radius * scale, nsample, pad, idx, cnt)
            idx, cnt = _ball(xs, cs, radius * scale, 64, 'first')
            ref.check_margin(radius * scale, 64, 'first', idx, cnt)


@pytest.mark.parametrize('n', BOUNDARIES)
def test_every_variant_gives_the_same_words(cuda, n):
    """Every variant forced through the ball_path switch against the product's choice, and that against the reference, just
    below, at and above every block, step and tile boundary.  37 queries: workgroups of 4 and of 16 queries both end in a
    partial one; at radius 0.2 some queries of a workgroup fill up tiles before the others."""
    for levels in (4, 16):
        x = lattice_cloud(31 * levels + n, 2, n, levels)
        for between in (False, True):
            c = _lattice_centres(n, x, 37, between)
            ref = BallReference(x, c)
            xs, cs = torch.from_numpy(x).to(cuda), torch.from_numpy(c).to(cuda)
            for radius in (0.125, 0.2, 10.0):
                for nsample, pad in ((1, 'none'), (31, 'first'), (200, 'first'), (200, 'none')):
                    base = _forced(0, lambda: _ball(xs, cs, radius, nsample, pad))
                    ref.check_exact(radius, nsample, pad, *base)
                    for path in PATHS:
                        got = _forced(path, lambda: _ball(xs, cs, radius, nsample, pad))
                        assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]), (levels, radius, nsample, pad, path)


def test_independence(cuda):
    """A batch against its clouds one by one and in another order; centres aliasing xyz; the call without the count."""
    n, m, nsample = 1025, 300, 24
    x, _ = generic_cloud(13, 5, n, 'gauss')
    xs = torch.from_numpy(x).to(cuda)
    cs = xs[:, :m].contiguous()
    for path in (0,) + PATHS:
        for pad in PADS:
            idx, cnt = _forced(path, lambda: _ball(xs, cs, 0.25, nsample, pad))
            again = _forced(path, lambda: _ball(xs, cs, 0.25, nsample, pad))
            assert np.array_equal(idx, again[0]) and np.array_equal(cnt, again[1])
            for i in (0, 2, 4):
                alone = _forced(path, lambda: _ball(xs[i:i + 1], cs[i:i + 1], 0.25, nsample, pad))
                assert np.array_equal(alone[0][0], idx[i]) and np.array_equal(alone[1][0], cnt[i])
            order = [2, 4, 0, 3, 1]
            moved = _forced(path, lambda: _ball(xs[order].contiguous(), cs[order].contiguous(), 0.25, nsample, pad))
            assert np.array_equal(moved[0], idx[order]) and np.array_equal(moved[1], cnt[order])
            fewer = _forced(path, lambda: _ball(xs, cs[:, 7:50].contiguous(), 0.25, nsample, pad))  # (other m, other slots)
            assert np.array_equal(fewer[0], idx[:, 7:50]) and np.array_equal(fewer[1], cnt[:, 7:50])
            assert np.array_equal(_forced(path, lambda: _ball(xs, cs, 0.25, nsample, pad, count=False)), idx)
            # centres = xyz, the same memory: every point is in its own ball
            self_idx, self_cnt = _forced(path, lambda: _ball(xs, xs, 0.25, nsample, pad))
            copy = _forced(path, lambda: _ball(xs, xs.clone(), 0.25, nsample, pad))
            assert np.array_equal(self_idx, copy[0]) and np.array_equal(self_cnt, copy[1])
            assert np.array_equal(self_idx[:, :m], idx) and (self_cnt >= 1).all()


def test_non_finite_input(cuda):
    """A NaN / +-inf candidate is never returned; a non-finite centre gets cnt = 0 and pure padding; a healthy cloud beside
    an all-NaN one is unaffected.  Lattice clouds: the reference is exact."""
    n, m = 300, 70
    x = lattice_cloud(14, 3, n, 4)
    bad = [0, 5, 63, 64, 128, 200, 299]
    x[0, bad] = [[np.nan, 0, 0], [0, np.inf, 0], [1, 1, -np.inf], [np.nan] * 3, [np.inf, -np.inf, 0], [0, 0, np.nan], [np.inf] * 3]
    x[1] = np.nan
    c = np.ascontiguousarray(x[:, :m])
    c[2, 9] = [0.5, np.nan, 0.5]
    c[2, 10] = [np.inf, 0.5, 0.5]
    ref = BallReference(x, c)
    xs, cs = torch.from_numpy(x).to(cuda), torch.from_numpy(c).to(cuda)
    for path in (0,) + PATHS:
        for radius in (0.3, float('inf')):
            for pad, fill in (('first', 0), ('none', -1)):
                idx, cnt = _forced(path, lambda: _ball(xs, cs, radius, 40, pad))
                ref.check_exact(radius, 40, pad, idx, cnt)
                for qi in range(m):
                    assert not np.isin(idx[0, qi, :cnt[0, qi]], bad).any()
                assert (cnt[1] == 0).all() and (idx[1] == fill).all()
                for bi, qi in ((0, 0), (0, 5), (0, 63), (0, 64), (2, 9), (2, 10)):
                    assert cnt[bi, qi] == 0 and (idx[bi, qi] == fill).all()
                assert cnt[2, 0] > 0
                alone = _forced(path, lambda: _ball(xs[2:], cs[2:], radius, 40, pad))
                assert np.array_equal(alone[0][0], idx[2]) and np.array_equal(alone[1][0], cnt[2])


def test_arguments(cuda):
    from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops

    x = torch.from_numpy(generic_cloud(15, 2, 300, 'uniform')[0]).to(cuda)
    c = x[:, :20].contiguous()
    good = ops.ball_query(x, c, 0.3, 8, return_count=True)
    for radius in (0, 0.0, -0.5, float('nan'), 1e-60, None):
        with pytest.raises(ValueError):
            ops.ball_query(x, c, radius, 8)
    for nsample in (0, -3, 8.0):
        with pytest.raises(ValueError):
            ops.ball_query(x, c, 0.3, nsample)
    for pad in ('zero', 1, None):
        with pytest.raises(ValueError):
            ops.ball_query(x, c, 0.3, 8, pad=pad)
    for bad_x, bad_c in ((x.transpose(1, 2).contiguous(), c), (x, c.transpose(1, 2).contiguous()), (x, c[:1]), (x[0], c[0])):
        with pytest.raises(ValueError):
            ops.ball_query(bad_x, bad_c, 0.3, 8)
    for bad_x, bad_c in ((x.double(), c), (x, c.half())):
        with pytest.raises(RuntimeError):
            ops.ball_query(bad_x, bad_c, 0.3, 8)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        ops.ball_query(x, c.cpu(), 0.3, 8)
    with pytest.raises(RuntimeError):
        ops.ball_query(x.cpu(), c, 0.3, 8)
    # the C ABI refuses null pointers and bad values before it enqueues anything
    L = _lib.lib
    out = torch.zeros((2, 20, 8), dtype=torch.int64, device=cuda)
    xp, cp, op = x.data_ptr(), c.data_ptr(), out.data_ptr()
    for args in ((2, 300, 20, 8, 0.3, 0, None, cp, op), (2, 300, 20, 8, 0.3, 0, xp, None, op), (2, 300, 20, 8, 0.3, 0, xp, cp, None),
                 (2, 300, 20, 8, 0.0, 0, xp, cp, op), (2, 300, 20, 8, float('nan'), 0, xp, cp, op), (2, 300, 20, 0, 0.3, 0, xp, cp, op),
                 (2, 300, 20, 8, 0.3, 2, xp, cp, op), (2, 0, 20, 8, 0.3, 0, xp, cp, op)):
        assert L.pcc_ball_query(*args, None, torch.cuda.current_stream(cuda).cuda_stream) != 0
        assert L.pcc_last_error().decode().startswith('ball_query:')
    torch.cuda.synchronize()
    assert (out == 0).all()  # nothing ran
    for ex, ec, shape in ((x[:0], c[:0], (0, 20, 8)), (x, c[:, :0], (2, 0, 8))):
        idx, cnt = ops.ball_query(ex, ec, 0.3, 8, return_count=True)
        assert idx.shape == shape and idx.dtype == torch.int64 and idx.device == x.device
        assert cnt.shape == shape[:2] and cnt.dtype == torch.int32
    # views that are not contiguous give the result of their contiguous copies; the library still answers after the refusals
    view = x[:, ::2, :]
    assert not view.is_contiguous()
    assert torch.equal(ops.ball_query(view, view[:, :30], 0.3, 8), ops.ball_query(view.contiguous(), view[:, :30].contiguous(), 0.3, 8))
    again = ops.ball_query(x, c, 0.3, 8, return_count=True)
    assert torch.equal(good[0], again[0]) and torch.equal(good[1], again[1])
    assert not good[0].requires_grad


def test_cpu_path_and_kernel_agree_word_for_word(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    lattice = lattice_cloud(17, 2, 1025, 16)
    generic, _ = generic_cloud(11, 3, 2048, 'uniform')
    shifted, _ = generic_cloud(11, 2, 300, 'gauss_+50')
    for x, m, radii in ((lattice, 65, (0.125, 0.2)), (generic, 512, (0.2, 0.5)), (shifted, 300, (0.3,))):
        x = torch.from_numpy(x)
        c = x[:, :m].contiguous()
        for radius in radii:
            for nsample, pad in ((16, 'first'), (64, 'none')):
                cpu = ops.ball_query(x, c, radius, nsample, pad=pad, return_count=True)
                gpu = ops.ball_query(x.to(cuda), c.to(cuda), radius, nsample, pad=pad, return_count=True)
                assert torch.equal(cpu[0], gpu[0].cpu()) and torch.equal(cpu[1], gpu[1].cpu()), (radius, nsample, pad)
