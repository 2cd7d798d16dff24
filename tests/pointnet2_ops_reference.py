"""The rules of ``pointnet2_ops.pointnet2_utils`` as plain numpy loops in float64, and the lattice inputs the tests use.

Coordinates are multiples of 1/16 in [0, 1): every squared distance is a multiple of 1/256 below 3 and exact in float32 in
any order of evaluation, ties really occur, and index results must match exactly."""

import numpy as np
import torch

RADIUS = 0.25  # r^2 = 16/256: lattice points sit exactly on the sphere, so the strict comparison is exercised


def words(t):
    """The bit patterns of a float32 tensor or of an array rounded to float32."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a.astype(np.float32, copy=False)).view(np.uint32)


def T(a):
    """An array as a CPU tensor."""
    return torch.from_numpy(np.ascontiguousarray(a))


def index_lists(seed, b, n, m, k):
    """``idx[b,m,k]`` int64 with repeated entries and entries outside ``[0, n)`` (-1, n, n + 7)."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, n, size=(b, m, k))
    idx[:, ::2, :] = idx[:, ::2, :1]  # every other row one index repeated
    bad = rng.random(size=idx.shape) < 0.2
    idx[bad] = rng.choice([-1, n, n + 7], size=int(bad.sum()))
    return idx.astype(np.int64)


def lattice_cloud(seed, b, n):
    """``xyz[b,n,3]`` float32, coordinates multiples of 1/16 in [0, 1)."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 16, size=(b, n, 3)) / 16.0).astype(np.float32)


def integer_features(seed, b, c, n, lim=8):
    """``[b,c,n]`` float32 of small integers: sums of a few of them (times dyadic weights) are exact in float32."""
    rng = np.random.default_rng(seed)
    return rng.integers(-lim, lim + 1, size=(b, c, n)).astype(np.float32)


def dyadic_weights(seed, b, n, k=3):
    """``[b,n,k]`` float32, multiples of 1/8 in [0, 1]."""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 9, size=(b, n, k)) / 8.0).astype(np.float32)


def _d2_row(points, q):
    """Squared distances of ``points[n,3]`` to ``q[3]`` in float64 (exact on the lattice)."""
    d = np.asarray(points, np.float64) - np.asarray(q, np.float64)
    return d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]


def furthest_point_sample(xyz, npoint):
    """Greedy loop from index 0, squared distances, the lowest index among equal maxima; a non-finite point is never chosen
    while another is left.  (The first ``t`` picks do not depend on ``npoint``.)"""
    b, n, _ = xyz.shape
    out = np.zeros((b, npoint), np.int32)
    for bi in range(b):
        finite = np.isfinite(xyz[bi]).all(-1)
        mind = np.where(finite, np.inf, -1.0)
        sel = 0
        for t in range(npoint):
            if t:
                sel = int(np.argmax(mind))  # (the first of equal maxima)
            out[bi, t] = sel
            with np.errstate(invalid='ignore'):
                d = _d2_row(xyz[bi], xyz[bi, sel])
            closer = finite & (d < mind)
            mind[closer] = d[closer]
    return out


def ball_query(radius, nsample, xyz, new_xyz):
    """A scan in index order: the first ``nsample`` points with d^2 < r^2 (r the float32 radius, r^2 one float32 product),
    the remaining slots the row's first hit, all 0 for an empty ball."""
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    r2 = float(np.float32(radius) * np.float32(radius))
    out = np.zeros((b, m, nsample), np.int32)
    for bi in range(b):
        for i in range(m):
            d = _d2_row(xyz[bi], new_xyz[bi, i])
            cnt = 0
            for j in range(n):
                if d[j] < r2:
                    if cnt == 0:
                        out[bi, i, :] = j
                    out[bi, i, cnt] = j
                    cnt += 1
                    if cnt == nsample:
                        break
    return out


def three_nn(unknown, known):
    """A stable argsort of the squared distances; ``dist`` their float64 roots; for m < 3 the missing slots are
    ``(+inf, 0)``."""
    b, n, _ = unknown.shape
    dist = np.full((b, n, 3), np.inf, np.float64)
    idx = np.zeros((b, n, 3), np.int32)
    for bi in range(b):
        for i in range(n):
            d = _d2_row(known[bi], unknown[bi, i])
            order = np.argsort(d, kind='stable')[:3]
            idx[bi, i, :len(order)] = order
            dist[bi, i, :len(order)] = np.sqrt(d[order])
    return dist, idx


def gather_operation(features, idx):
    b, c, n = features.shape
    out = np.zeros((b, c, idx.shape[1]), np.float64)
    for bi in range(b):
        for i in range(idx.shape[1]):
            j = int(idx[bi, i])
            if 0 <= j < n:
                out[bi, :, i] = features[bi, :, j]
    return out


def gather_operation_grad(grad, idx, n):
    b, c, _ = grad.shape
    out = np.zeros((b, c, n), np.float64)
    for bi in range(b):
        for i in range(idx.shape[1]):
            j = int(idx[bi, i])
            if 0 <= j < n:
                out[bi, :, j] += grad[bi, :, i]
    return out


def grouping_operation(features, idx):
    b, c, n = features.shape
    _, m, k = idx.shape
    out = np.zeros((b, c, m, k), np.float64)
    for bi in range(b):
        for i in range(m):
            for s in range(k):
                j = int(idx[bi, i, s])
                if 0 <= j < n:
                    out[bi, :, i, s] = features[bi, :, j]
    return out


def grouping_operation_grad(grad, idx, n):
    b, c, m, k = grad.shape
    out = np.zeros((b, c, n), np.float64)
    for bi in range(b):
        for i in range(m):
            for s in range(k):
                j = int(idx[bi, i, s])
                if 0 <= j < n:
                    out[bi, :, j] += grad[bi, :, i, s]
    return out


def three_interpolate(features, idx, weight):
    b, c, m = features.shape
    n, k = idx.shape[1:]
    out = np.zeros((b, c, n), np.float64)
    for bi in range(b):
        for i in range(n):
            for s in range(k):
                j = int(idx[bi, i, s])
                if 0 <= j < m:
                    out[bi, :, i] += np.float64(weight[bi, i, s]) * features[bi, :, j]
    return out


def three_interpolate_grad(grad, idx, weight, m):
    """The gradient of the features."""
    b, c, n = grad.shape
    k = idx.shape[2]
    out = np.zeros((b, c, m), np.float64)
    for bi in range(b):
        for i in range(n):
            for s in range(k):
                j = int(idx[bi, i, s])
                if 0 <= j < m:
                    out[bi, :, j] += np.float64(weight[bi, i, s]) * grad[bi, :, i]
    return out


def query_and_group(radius, nsample, xyz, new_xyz, features, use_xyz=True):
    """``[b,3+c,m,nsample]``: grouped coordinates minus the centre, then the grouped features."""
    idx = ball_query(radius, nsample, xyz, new_xyz)
    parts = []
    if use_xyz or features is None:
        g = grouping_operation(np.transpose(xyz, (0, 2, 1)), idx)
        parts.append(g - np.transpose(new_xyz, (0, 2, 1)).astype(np.float64)[:, :, :, None])
    if features is not None:
        parts.append(grouping_operation(features, idx))
    return np.concatenate(parts, 1)
