"""Every computing entry point of the C ABI on contiguous tensors off a 16-byte boundary (tests/unaligned_views.py).

Per case: every call once on aligned tensors, then once per tensor argument with that argument alone 4, 8 and 12 bytes past a
boundary (an int64 list: 8 bytes), then once with every argument shifted -- inputs as views into a fresh buffer, outputs as
guarded buffers whose body is shifted likewise.  Every output must equal the aligned call's word for word (bit patterns: NaN
payloads and the sign of zero count), with the guards intact and every word written.  The aligned result is tied to the op's
exact reference (the case's ``anchor``), so the misaligned result is tied to it too and not only to the kernel's other path.
Then the Python op, where there is one: the same comparison with each of its inputs -- the incoming gradient of the backward
among them -- shifted, and its aligned result against the C call's.  No tolerance is introduced here: every comparison is
equality, or a bound the op's reference module defines."""

import time

import pytest
import torch

from tests import unaligned_views as U
from tests import unaligned_views_cell_ragged, unaligned_views_grid_ragged, unaligned_views_ragged  # noqa: F401  (they register their cases:
# all 41 however this file is run)

pytestmark = pytest.mark.gpu


def _on(dev, ins):
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in ins.items()}


@pytest.mark.parametrize('case', U.CASES, ids=[case.name for case in U.CASES])
def test_misaligned_arguments_give_the_aligned_words(cuda, oracle_mod, case):
    t0 = time.perf_counter()
    d = case.dims
    ins = case.build(d)
    pool = _on(cuda, ins)
    record = {k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in ins.items()}
    subcalls = 0
    for call in case.calls(d):
        base = U.run_call(call, pool, cuda, {})
        shifts = U.variants(call, pool)
        for shift in shifts:
            got = U.run_call(call, pool, cuda, shift)
            for name, want in base.items():
                assert U.same_words(got[name], want), (call.symbol, call.tune, shift, name)
        subcalls += 1 + len(shifts)
        record.update(base)
        pool.update({k: torch.from_numpy(v).to(cuda) for k, v in base.items()})  # (a backward reads what its forward wrote)
    if case.op is not None:
        dev_ins = _on(cuda, ins)
        base = case.op(dev_ins)
        for name, want in base.items():
            assert name not in record or U.same_words(want, record[name]), f'{name}: the Python op and the C call differ'
            record.setdefault(name, want.detach().cpu().numpy())  # (what only the op computes is anchored under its name)
        tensors = [k for k in case.op_inputs if dev_ins[k] is not None]
        shifts = [{k: e} for k in tensors for e in U.SHIFTS[dev_ins[k].dtype]] + [{k: 1 for k in tensors}]
        for shift in shifts:
            got = case.op({k: (U.shifted(v, shift[k]) if k in shift else v) for k, v in dev_ins.items()})
            for name, want in base.items():
                assert U.same_words(got[name], want), ('op', shift, name)
        subcalls += 1 + len(shifts)
    assert case.anchor is not None, 'every case ties its aligned result to a reference'
    case.anchor(d, record, oracle_mod)
    if case.probe is not None:
        case.probe(d, _on(cuda, ins), cuda)
    torch.cuda.synchronize()
    print(f'{case.name}: {subcalls} sub-calls in {time.perf_counter() - t0:.2f} s')
