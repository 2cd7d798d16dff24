"""The registry of tests/unaligned_views.py, without a device: every entry point of the C ABI has a case or is exempt, every
case's shape meets the size condition of the gate it is aimed at, the two helpers do what they say, and every op with a CPU
path gives the same words on views off a 16-byte boundary as on the original tensors."""

import numpy as np
import pytest
import torch

from tests import unaligned_views as U
from tests import unaligned_views_cell_ragged, unaligned_views_grid_ragged, unaligned_views_ragged  # noqa: F401  (they register their cases:
# all 41 however this file is run)

IDS = [case.name for case in U.CASES]

# Tensors whose per-sample size cannot be a multiple of 16 bytes at the shape the case needs: no wide access is aimed at them.
RAGGED = {
    'grid_pool': {'seg', 'seg_out'},                                      # seg[b, m + 1] beside out[b, c, m] with m % 4 == 0
    'sparse_conv_c8_o16': {'nbr'}, 'sparse_conv_c8_o32': {'nbr'}, 'sparse_conv_c8_o64': {'nbr'},  # m = 33: the gate is on weight, which has no batch
    'sparse_conv_c5_o9': {'nbr', 'x', 'out', 'g'},                        # the VALU kernel: no wide access at all
}


def test_every_entry_point_has_a_case_or_is_exempt():
    from pointcloudcounterfactual_amd import _lib

    covered = U.covered()
    assert not covered & U.EXEMPT
    assert set(_lib.ABI) == covered | U.EXEMPT, (sorted(set(_lib.ABI) - covered - U.EXEMPT), sorted((covered | U.EXEMPT) - set(_lib.ABI)))
    assert len(set(IDS)) == len(IDS)
    assert all(case.anchor is not None for case in U.CASES), 'a case that ties its aligned result to nothing'


@pytest.mark.parametrize('case', U.CASES, ids=IDS)
def test_shape_meets_the_gate_and_keeps_every_sample_aligned(case):
    d = case.dims
    assert d['b'] == 2 and all(v <= 512 or case.name == 'matchcost' for v in d.values())
    assert case.gate is None or case.gate(d)
    ins = case.build(d)
    outs = [a for call in case.calls(d) for a in call.args if isinstance(a, U.Out)]
    assert len({a.name for a in outs}) == len(outs), 'two outputs of a case share a name'
    sized = [(k, tuple(v.shape), v.element_size()) for k, v in ins.items() if isinstance(v, torch.Tensor)]
    sized += [(a.name, a.shape, 8 if a.dtype == U.I64 else 4) for a in outs]
    for name, shape, size in sized:
        if len(shape) >= 2 and shape[0] == d['b'] and name not in RAGGED.get(case.name, ()):
            per_sample = int(np.prod(shape[1:])) * size
            assert per_sample < 16 or per_sample % 16 == 0, (name, shape)
    for call in case.calls(d):  # every named input exists, with the dtype the binding would ask for
        for a in call.args:
            assert not isinstance(a, str) or a in ins or any(o.name == a for o in outs), a
    for name in case.op_inputs:
        assert name in ins


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32, torch.int64])
def test_shifted_keeps_values_and_lands_where_it_says(dtype):
    t = torch.arange(24, dtype=dtype).view(2, 3, 4)
    for elements in (0, 1, 2, 3):
        v = U.shifted(t, elements)
        assert v.shape == t.shape and v.dtype == t.dtype and v.is_contiguous() and torch.equal(v, t)
        assert v.data_ptr() % 16 == (elements * t.element_size()) % 16
        assert v.data_ptr() != t.data_ptr()
    assert U.shifted(t).data_ptr() % 16 == t.element_size()


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32, torch.int64])
@pytest.mark.parametrize('elements', [0, 1, 3])
def test_guarded_detects_a_word_outside_and_a_word_left_unwritten(dtype, elements):
    def fresh():
        g = U.guarded((3, 5), dtype, 'cpu', elements)
        assert g.ptr() % 16 == (elements * g.tensor.element_size()) % 16 and g.tensor.dtype == dtype and g.tensor.shape == (3, 5)
        return g

    g = fresh()
    with pytest.raises(AssertionError, match='not written'):
        g.numpy()
    assert g.numpy(whole=False).shape == (3, 5)
    g.tensor.copy_(torch.arange(15).view(3, 5))
    assert np.array_equal(g.numpy(), np.arange(15).reshape(3, 5))
    g.tensor[1, 2] = float('nan') if dtype == torch.float32 else -1
    g.numpy()  # (an ordinary NaN is a written word)
    for at, what in ((g.lo - 1, 'before'), (g.hi, 'behind'), (0, 'before'), (g.flat.numel() - 1, 'behind')):
        g = fresh()
        g.tensor.zero_()
        g.flat[at] = 0
        with pytest.raises(AssertionError, match=what):
            g.numpy()


def test_words_tell_nan_payloads_and_the_sign_of_zero():
    a = np.array([0.0, np.nan], dtype=np.float32)
    b = a.copy()
    assert U.same_words(a, b)
    b.view(np.uint32)[1] = 0x7fc12345
    assert not U.same_words(a, b)
    assert not U.same_words(np.array([0.0], np.float32), np.array([-0.0], np.float32))
    assert not U.same_words(np.zeros(2, np.float32), np.zeros(3, np.float32))


@pytest.mark.parametrize('case', [c for c in U.CASES if c.cpu], ids=[c.name for c in U.CASES if c.cpu])
def test_cpu_path_gives_the_same_words_on_shifted_inputs(case):
    ins = case.build(case.dims)
    base = case.op(ins)
    assert base
    tensors = [k for k in case.op_inputs if ins[k] is not None]
    for shift in [{k: e} for k in tensors for e in U.SHIFTS[ins[k].dtype]] + [{k: 1 for k in tensors}]:
        got = case.op({k: (U.shifted(v, shift[k]) if k in shift else v) for k, v in ins.items()})
        for name, want in base.items():
            assert U.same_words(got[name], want), (shift, name)
