"""The ``pointops`` drop-in on CPU tensors against the numpy loops of tests/ragged_reference.py: indices exactly (int32), values
word for word on lattice inputs, gradients exactly on integer gradients with dyadic weights, the masked -1 slot, and the
documented refusals."""

import numpy as np
import pytest
import torch

import pointops
from tests import ragged_reference as R
from tests import unaligned_views_ragged  # noqa: F401  (registers the two entry points' cases before the registry suites read it)
from tests.unaligned_views import same_words


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _root(xyz, new_xyz, idx):
    """The float32 distances of a list: exact squared distances on the lattice, the correctly rounded root, +inf for -1."""
    d2 = ((xyz[np.maximum(idx, 0)].astype(np.float64) - new_xyz[:, None].astype(np.float64)) ** 2).sum(-1)
    return np.where(idx >= 0, np.sqrt(d2), np.inf).astype(np.float32)


def check_searches(dev, oracle_mod):
    xyz, offset, new_xyz, new_offset, _ = R.dropin_batch()
    tx, to, tq, tqo = (_t(a).to(dev) for a in (xyz, offset, new_xyz, new_offset))
    want = R.knn(oracle_mod, xyz, offset, new_xyz, new_offset)
    for nsample in (1, 3, 5, 16, 32):
        idx, dist = pointops.knn_query(nsample, tx, to, tq, tqo)
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and idx.shape == dist.shape == (len(new_xyz), nsample)
        assert np.array_equal(idx.cpu().numpy(), want[:, :nsample])
        assert same_words(dist.cpu(), _root(xyz, new_xyz, want[:, :nsample]))
    assert (want[9:13, 3:] == -1).all()  # the cloud of three points: a padded slot is (-1, +inf)
    idx, dist = pointops.knn_query(4, tx, to.int())
    assert np.array_equal(idx.cpu().numpy(), R.knn(oracle_mod, xyz, offset, k=4))
    ball = R.RaggedBall(xyz, offset, new_xyz, new_offset)
    for radius, nsample in ((0.25, 4), (0.3, 16), (1e-4, 3), (10.0, 50)):
        idx, dist = pointops.ball_query(nsample, radius, 0, tx, to, tq, tqo)
        ref = ball.query(radius, nsample, 'first')[0]
        assert idx.dtype == torch.int32 and np.array_equal(idx.cpu().numpy(), ref) and same_words(dist.cpu(), _root(xyz, new_xyz, ref))
    sel = pointops.farthest_point_sampling(tx, to, _t(np.array([7, 10, 20])).to(dev))
    assert sel.dtype == torch.int32 and sel.shape == (20,)
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    assert torch.equal(sel.long(), ops.farthest_point_sample_ragged(tx, to, _t(np.array([7, 10, 20])).to(dev)))
    assert torch.equal(pointops.offset2batch(to), ops.offset2batch(to)) and torch.equal(pointops.batch2offset(pointops.offset2batch(to)), to)


def check_grouping(dev, oracle_mod):
    xyz, offset, new_xyz, new_offset, feat = R.dropin_batch()
    tx, to, tq, tqo, tf = (_t(a).to(dev) for a in (xyz, offset, new_xyz, new_offset, feat))
    idx = R.knn(oracle_mod, xyz, offset, new_xyz, new_offset, k=5)
    assert (idx == -1).any()
    ti = _t(idx.astype(np.int32)).to(dev)
    grad = np.random.default_rng(1).integers(-3, 4, (len(new_xyz), 5, 3 + feat.shape[1])).astype(np.float32)
    for with_xyz in (False, True):
        leaf = tf.clone().requires_grad_(True)
        out = pointops.grouping(ti, leaf, tx, tq, with_xyz=with_xyz)
        want = R.grouping(idx, feat, xyz, new_xyz, with_xyz)
        assert out.shape == want.shape and out.is_contiguous() and same_words(out.detach().cpu(), want)
        assert (out.detach().cpu().numpy()[idx < 0] == 0).all()  # with_xyz masks the relative coordinates of a -1 slot too
        g = grad if with_xyz else grad[..., 3:]
        out.backward(_t(g).to(dev))
        assert np.array_equal(leaf.grad.cpu().numpy().astype(np.float64), R.grouping_grad(idx, g, len(xyz), with_xyz))
    # the self grouping (new_xyz = None) and the three spellings of query + group
    self_idx = R.knn(oracle_mod, xyz, offset, k=4)
    assert same_words(pointops.grouping(_t(self_idx).to(dev), tf, tx, with_xyz=True).cpu(), R.grouping(self_idx, feat, xyz, None, True))
    got, gi = pointops.knn_query_and_group(tf, tx, to, tq, tqo, nsample=5, with_xyz=True)
    assert np.array_equal(gi.cpu().numpy(), idx) and same_words(got.cpu(), R.grouping(idx, feat, xyz, new_xyz, True))
    got, gi = pointops.query_and_group(5, tx, tq, tf, None, to, tqo)
    assert np.array_equal(gi.cpu().numpy(), idx) and same_words(got.cpu(), R.grouping(idx, feat, xyz, new_xyz, True))
    got, gi = pointops.query_and_group(5, tx, tq, tf, ti, to, tqo, with_xyz=False)
    assert same_words(got.cpu(), R.grouping(idx, feat, xyz, new_xyz, False))
    got, gi = pointops.query_and_group(5, tx, tq, tf, ti, to, tqo, with_feat=False)
    assert same_words(got.cpu(), R.grouping(idx, feat, xyz, new_xyz, True)[..., :3])
    bidx = R.RaggedBall(xyz, offset, new_xyz, new_offset).query(0.3, 8, 'first')[0]
    got, gi = pointops.ball_query_and_group(tf, tx, to, tq, tqo, max_radio=0.3, min_radio=0, nsample=8)
    assert np.array_equal(gi.cpu().numpy(), bidx) and same_words(got.cpu(), R.grouping(bidx, feat, xyz, new_xyz, False))


def check_interpolation(dev, oracle_mod):
    xyz, offset, new_xyz, new_offset, feat = R.dyadic_interpolation_batch()
    grad = np.random.default_rng(2).integers(-3, 4, (len(new_xyz), feat.shape[1])).astype(np.float32)
    for k, clouds in ((1, slice(0, 3)), (2, slice(0, 3)), (3, slice(1, 3))):
        (lo, hi), (qlo, qhi) = (R.ranges(offset)[clouds.start][0], len(xyz)), (R.ranges(new_offset)[clouds.start][0], len(new_xyz))
        x, q, f, g = xyz[lo:hi], new_xyz[qlo:qhi], feat[lo:hi], grad[qlo:qhi]
        off, qoff = offset[clouds] - lo, new_offset[clouds] - qlo
        idx = R.knn(oracle_mod, x, off, q, qoff, k)
        w = R.interpolation_weights(idx, x, q)
        assert np.isin(w, (0, 0.5, 1)).all() and (w.sum(1) == 1).all()
        leaf = _t(f).to(dev).requires_grad_(True)
        out = pointops.interpolation(_t(x).to(dev), _t(q).to(dev), leaf, _t(off).to(dev), _t(qoff).to(dev), k=k)
        assert out.shape == (len(q), f.shape[1]) and out.is_contiguous()
        assert same_words(out.detach().cpu(), R.interpolation(idx, w, f).astype(np.float32)), k
        out.backward(_t(g).to(dev))
        assert np.array_equal(leaf.grad.cpu().numpy().astype(np.float64), R.interpolation_grad(idx, w, g, len(x))), k


def test_searches_and_sampling(oracle_mod):
    check_searches(torch.device('cpu'), oracle_mod)


def test_grouping_values_mask_and_gradients(oracle_mod):
    check_grouping(torch.device('cpu'), oracle_mod)


def test_interpolation_values_and_gradients(oracle_mod):
    check_interpolation(torch.device('cpu'), oracle_mod)


def test_documented_refusals():
    xyz, offset, new_xyz, new_offset, feat = (_t(a) for a in R.dropin_batch())
    with pytest.raises(NotImplementedError, match='min_radius'):
        pointops.ball_query(8, 0.3, 0.1, xyz, offset)
    with pytest.raises(ValueError, match=r'k must be an integer in \[1, 32\]'):
        pointops.knn_query(33, xyz, offset)
    with pytest.raises(ValueError, match='new_xyz comes with new_offset'):
        pointops.knn_query(3, xyz, offset, new_xyz)
    with pytest.raises(ValueError, match='more picks than it has points'):
        pointops.farthest_point_sampling(xyz, offset, torch.tensor([7, 11, 20]))
    with pytest.raises(NotImplementedError, match='dilation'):
        pointops.query_and_group(4, xyz, new_xyz, feat, None, offset, new_offset, dilation=1)
    with pytest.raises(ValueError, match=r'expected idx\[m,nsample\]'):
        pointops.grouping(torch.zeros(19, 4), feat, xyz, new_xyz)
    with pytest.raises(ValueError, match='offset must be non-decreasing'):
        pointops.knn_query(3, xyz, torch.tensor([40, 43, 59]))
    assert set(pointops.__all__) <= set(dir(pointops))
