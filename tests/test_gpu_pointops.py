"""The ``pointops`` drop-in on the accelerator: the checks of tests/test_pointops_host.py against the numpy loops on device
tensors (indices exactly, values word for word, gradients exactly), and the device against the CPU on generic clouds."""

import numpy as np
import pytest
import torch

import pointops
from tests import ragged_reference as R
from tests import test_pointops_host as H
from tests import unaligned_views_ragged  # noqa: F401  (registers the two entry points' cases before the registry suites read it)
from tests.unaligned_views import same_words

pytestmark = pytest.mark.gpu


def test_searches_and_sampling(cuda, oracle_mod):
    H.check_searches(cuda, oracle_mod)


def test_grouping_values_mask_and_gradients(cuda, oracle_mod):
    H.check_grouping(cuda, oracle_mod)


def test_interpolation_values_and_gradients(cuda, oracle_mod):
    H.check_interpolation(cuda, oracle_mod)


def test_device_against_cpu(cuda):
    """Lattice geometry (the two searches agree word for word there) with generic features: grouping is a copy and one
    subtraction, the same words on either device; the interpolation's weights are the same torch expressions on the same
    distances, and its sums the same float32 operations in slot order."""
    xyz, offset = R.batch(600, [300, 2, 65, 0, 129], 'lattice16')
    new_xyz, new_offset = R.batch(650, [70, 5, 64, 3, 1], 'lattice16')
    feat = np.random.default_rng(3).standard_normal((len(xyz), 7)).astype(np.float32)
    cpu = [torch.from_numpy(a) for a in (xyz, offset, new_xyz, new_offset, feat)]
    dev = [t.to(cuda) for t in cpu]
    for args in (cpu, dev):
        args[4] = args[4].clone().requires_grad_(True)
    grad = torch.from_numpy(np.random.default_rng(4).integers(-3, 4, (len(new_xyz), 6, 10)).astype(np.float32))
    out = {}
    for name, (x, o, q, qo, f) in (('cpu', cpu), ('dev', dev)):
        idx, dist = pointops.knn_query(6, x, o, q, qo)
        bidx, bdist = pointops.ball_query(6, 0.2, 0, x, o, q, qo)
        grouped = pointops.grouping(idx, f, x, q, with_xyz=True)
        grouped.backward(grad.to(grouped.device))
        ggrad, f.grad = f.grad.clone(), None
        new_feat = pointops.interpolation(x, q, f, o, qo, k=3)
        out[name] = [t.detach().cpu() for t in (idx, dist, bidx, bdist, grouped, ggrad, new_feat)]
    for a, b in zip(out['cpu'][:5], out['dev'][:5]):
        assert same_words(a, b)
    # the gradient of the grouping adds integers times nothing: gathered integer gradients, exact in any order
    assert torch.equal(out['cpu'][5], out['dev'][5])
    assert same_words(out['cpu'][6], out['dev'][6])
    assert (out['dev'][0][70:75, 2:] == -1).all() and (out['dev'][0][139:142] == -1).all()  # the cloud of two points, the empty cloud
