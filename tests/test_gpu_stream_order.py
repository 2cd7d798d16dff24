"""Every entry point of the C ABI and every Python op off the default stream, behind inputs that arrive late
(tests/stream_order.py: what each check sees, and what it cannot see).

Per case of the registry: every call on the default stream (the base words), then on a side stream with nothing pending, behind a delay kernel
and behind its own argument tensors, which are built on that stream; the call must return while the delay is still running
(hard for every symbol: ``stream_order.WAITS`` says where a sequence of calls on one stream cannot), and stream-ordered clones of
its outputs must equal the base words
bit for bit, guards intact, every word written.  Then the Python op, forward and backward, the same way.  Then every case
beside its neighbour in the registry on two streams at once, and the launches that only exist above the registry's shapes.
No tolerance anywhere: equality with the words of the default stream in the same process."""

import time

import pytest
import torch

from tests import stream_order as S
from tests import unaligned_views as U
from tests.which_ran import ran

pytestmark = pytest.mark.gpu

IDS = [case.name for case in S.CASES]


def _late_calls(cuda, case):
    """Every call of ``case`` late on a side stream against its default-stream words; -> the launch record of all of them."""
    base = S.solo(case, cuda)
    record = {}
    for i, call in enumerate(base.calls):
        (got, busy), names = ran(lambda: S.late_call(call, base.pools[i], cuda, S.DELAY_MS, case.name))
        # (hard for the symbols of S.WAITS too: alone on a drained stream none of them meets the runtime's condition)
        assert busy, f'{call.symbol} {call.tune}: returned only after the {S.DELAY_MS} ms delay on its stream had ended'
        assert set(got) == set(base.words[i])
        for name, want in base.words[i].items():
            assert U.same_words(got[name], want), (call.symbol, call.tune, name)
        for kernel, count in names.items():
            record[kernel] = record.get(kernel, 0) + count
    return record


@pytest.mark.parametrize('case', S.CASES, ids=IDS)
def test_late_inputs_on_a_side_stream_and_return_while_busy(cuda, case):
    t0 = time.perf_counter()
    _late_calls(cuda, case)
    worst = max((v, k[1]) for k, v in S.ENQUEUE_S.items() if k[0] == case.name)
    print(f'{case.name}: longest enqueue {worst[0] * 1e3:.3f} ms ({worst[1]}), {time.perf_counter() - t0:.2f} s')


@pytest.mark.parametrize('case', [c for c in S.CASES if c.op is not None], ids=[c.name for c in S.CASES if c.op is not None])
def test_python_op_forward_and_backward_on_a_side_stream(cuda, case):
    base = S.solo(case, cuda)
    got = S.late_op(case, base.op_ins, cuda, S.DELAY_MS)
    assert set(got) == set(base.op_words) and got
    for name, want in base.op_words.items():
        assert U.same_words(got[name], want), name


@pytest.mark.parametrize('pair', S.ring(), ids=[f'{a.name}+{b.name}' for a, b in S.ring()])
def test_two_cases_on_two_streams_at_once(cuda, pair):
    solos = [S.solo(case, cuda) for case in pair]
    got, busy = S.ring_pair(*pair, cuda)
    assert all(busy) or any(S.may_wait(case) for case in pair), 'a delay had ended before both cases were enqueued: the calls did not interleave'
    for case, base, words in zip(pair, solos, got):
        assert len(words) == len(base.calls)
        for call, have, want in zip(base.calls, words, base.words):
            assert set(have) == set(want)
            for name in want:
                assert U.same_words(have[name], want[name]), (case.name, call.symbol, call.tune, name)


@pytest.mark.parametrize('sized', S.SIZED, ids=[s.case.name for s in S.SIZED])
def test_launches_above_the_registry_shapes(cuda, sized):
    sized.launched(_late_calls(cuda, sized.case))


def test_registry_is_whole_and_the_delay_is_what_it_says(cuda):
    """All 41 cases however this file is run; and the calibrated delay lasts what it is asked to (within a quarter: the clock
    of the delay kernel against the event timer), so DELAY_MS is milliseconds."""
    assert {'knn_ragged', 'ball_query_ragged', 'grid_cluster_ragged', 'cell_neighbours_ragged'} <= set(IDS) and len(IDS) >= 41
    S.cycles_per_ms()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    S.delay(S.DELAY_MS)
    b.record()
    b.synchronize()
    assert 0.75 * S.DELAY_MS <= a.elapsed_time(b) <= 1.25 * S.DELAY_MS + 1.0, a.elapsed_time(b)
    S.side_stream(cuda)
    print(f'delay of {S.DELAY_MS} ms took {a.elapsed_time(b):.2f} ms; {len(S._SIDE)} of 16 side streams do not share the default stream\'s queue')
