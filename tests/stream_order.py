"""Every computing entry point of the C ABI on a stream that is not the default one, behind inputs that arrive late.

include/pcc_neighbour.h and include/pcc_structural.h promise that every entry enqueues on the caller's ``stream`` and returns
without synchronising.  The registry of tests/unaligned_views.py (41 cases: every computing symbol of ``_lib.ABI``, the Python
op and its backward, inputs whose results are exact words) is run here under the one execution-context variable the rest of the
suite leaves at its default:

* ``late_call``: a non-blocking side stream with nothing pending (``side_stream``); a delay kernel on it; the argument tensors built on it, so their fills and copies
  queue behind the delay; the call; a stream-ordered clone of every output.  A launch or memset that went to another stream
  ran while the delay did: it read input buffers nobody had filled yet, and what it wrote was overwritten by the output's late
  prefill -- the clones differ from the default-stream words, or a word reads as never written.  A lane of the library's own
  that is not joined back before the outputs are read is still running when the clone is taken.
* the delay's own event is asked the moment the library's function returns: still pending means the call came back while the
  stream was busy ("never synchronise"), and it means the late-input check was live for this very call.
* ``late_op``: the Python op, forward and backward, on inputs cloned onto the side stream behind the delay.
* ``ring_pair``: two cases on two streams, each behind its own delay, their calls enqueued alternately with no wait in between:
  the memory pool, the co-resident gate, the tuning switch and the thread-local error state under real interleaving.
* ``SIZED``: the launches that only exist above the registry's shapes, one late-input case each.

What this detects is a race, and it is only as good as the race it wins: a stray launch is seen because it runs DURING the
delay.  Where the runtime happens to order the other stream behind the side stream anyway (``side_stream`` sorts out the
streams that share a hardware queue with the default stream, not those that share one with a third stream), or the stray kernel neither reads an input nor writes an output (it touches the workspace only, and the workspace's
poison memset is on the right stream), the words come out right and nothing is seen.  The static companion in
tests/test_stream_order_host.py reads the launch sites for the literal cases; it is weaker still.  Equality with the
default-stream words is the bar everywhere: no tolerance is introduced.

Importable without a device (tests/test_stream_order_host.py)."""

from __future__ import annotations

import copy
import time
from typing import Any, Callable, NamedTuple

import numpy as np
import torch

from tests import unaligned_views as U
from tests import unaligned_views_cell_ragged, unaligned_views_grid_ragged, unaligned_views_ragged  # noqa: F401  (they register their cases)

# The delay in front of every late call, in milliseconds: at least 5x the longest host-side enqueue (argument building plus
# the call) measured over all cases on an MI355X host -- DESIGN.md 4y holds both numbers.  The busy-return assertion guards
# the choice on every call: a delay that ended before the call returned fails it.
DELAY_MS = 40.0

# Entry points that can return only after their stream has drained, because a call of the HIP runtime waits (never the library):
# symbol -> the runtime call and the condition.  One reason holds for all of them (timed alone in a stand-alone HIP
# program, no library and no torch, ROCm 7.0): they take a workspace from the library's memory pool and give it back with
# hipFreeAsync on their stream.  When an earlier call on the SAME stream has freed a block of a fitting size and that stream
# has not yet reached the free, hipMallocFromPoolAsync hands the very same block out again at once (same stream: no wait
# needed, none made) -- and the hipFreeAsync of that block at the end of the second call then waits on the host until the
# first free has been reached, that is until the stream has drained (200.0 ms behind a 200 ms kernel; every other call of
# the sequence 1-30 us; the same with the device's default pool and with each of the pool's three reuse policies off; a
# second block of another size, or the second call on another stream, does not wait).  A single call on a stream that holds
# no unfinished call of the library never meets the condition: ``late_call`` puts every call on a stream of its own, and its
# busy-return assertion is hard for every symbol, these included.  Only ``ring_pair``, which puts a whole case on one stream,
# waives its busy assertion where a stream carries two or more calls of this table.  The words are checked everywhere.
_POOL_FREE = ('hipFreeAsync of a pool block that an earlier, unfinished call on the same stream had freed and that '
              'hipMallocFromPoolAsync handed out again: waits until the stream reaches the first free')
WAITS: dict[str, str] = {symbol: _POOL_FREE for symbol in (
    'pcc_chamfer_emd', 'pcc_match_cost', 'pcc_approxmatch', 'approxmatch', 'pcc_approxmatch_cost',  # approxmatch.hip: every entry but _ws
    'pcc_matchcost', 'matchcost', 'pcc_matchcostgrad', 'matchcostgrad', 'pcc_matchcostgrad_scaled',  # matchcost.hip: the partial sums
    'pcc_sliced_wasserstein', 'pcc_sinkhorn', 'pcc_occupancy_grid', 'pcc_auction_forward',
    'pcc_knn', 'pcc_knn_cross', 'pcc_fps',                                                           # (fps: the memory path only)
    'pcc_voxelize', 'pcc_grid_cluster_ragged', 'pcc_bn_stats', 'pcc_bn_relu_bwd',
    'pcc_gather_neighbours_bwd', 'pcc_graph_features_bwd', 'pcc_neighbour_sum_bwd')}                # graph_ops.hip: the sorted scatters

ENQUEUE_S: dict[tuple[str, str], float] = {}  # (case, symbol) -> the longest host-side enqueue seen, seconds

_cycles_per_ms: float | None = None


def cycles_per_ms() -> float:
    """``torch.cuda._sleep`` cycles per millisecond on the current device: measured once per process between two events."""
    global _cycles_per_ms
    if _cycles_per_ms is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)  # (loads the kernel)
        torch.cuda.synchronize()
        cycles = 50_000_000
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        _cycles_per_ms = cycles / a.elapsed_time(b)
    return _cycles_per_ms


def delay(ms: float) -> torch.cuda.Event:
    """A kernel that spins for ``ms`` milliseconds on the current stream, and the event recorded right behind it."""
    torch.cuda._sleep(int(ms * cycles_per_ms()))
    gate = torch.cuda.Event()
    gate.record()
    return gate


_SIDE: list[torch.cuda.Stream] = []
_next_side = 0


def side_stream(dev: torch.device) -> torch.cuda.Stream:
    """The next of the side streams on which the race can be won.  The runtime multiplexes the streams of a process onto a few
    hardware queues, and a stream that shares its queue with the default stream runs a stray default-stream launch in the
    order of the host's calls, behind the delay: nothing to see.  (Found with a mutated library: a launch moved to stream 0
    passed on such a stream.)  So, once per process, sixteen streams of torch's pool are probed -- a short delay on the
    stream, a kernel on the default stream, a wait for that kernel: the stream qualifies if its delay is then still
    running -- and the calls go round the streams that qualified; every call still gets a stream no earlier work is pending on."""
    global _next_side
    if not _SIDE:
        assert torch.cuda.current_stream(dev) == torch.cuda.default_stream(dev)
        word = torch.zeros(1, device=dev)
        for _ in range(16):
            stream = torch.cuda.Stream(dev)
            with torch.cuda.stream(stream):
                gate = delay(5.0)
            word.add_(1.0)
            overtook = torch.cuda.Event()
            overtook.record()
            overtook.synchronize()
            if not gate.query() and all(stream != other for other in _SIDE):
                _SIDE.append(stream)
            stream.synchronize()
        assert len(_SIDE) >= 4, f'only {len(_SIDE)} of 16 side streams let a default-stream kernel overtake them'
    _next_side += 1
    return _SIDE[_next_side % len(_SIDE)]


def _on(dev: torch.device, ins: dict[str, Any]) -> dict[str, Any]:
    return {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in ins.items()}


class Solo(NamedTuple):
    """A case on the default stream, nothing else in flight: per call the pool it read (a backward reads what its forward
    wrote) and the words it gave; the op's inputs on the device and its results."""

    calls: list[U.Call]
    pools: list[dict[str, Any]]
    words: list[dict[str, np.ndarray]]
    op_ins: dict[str, Any]
    op_words: dict[str, np.ndarray]


_SOLO: dict[str, Solo] = {}


def solo(case: U.Case, dev: torch.device) -> Solo:
    """The default-stream run of ``case``, made once per process and shared: it also loads the code objects and fills the
    library's memory pool, so that no later call allocates device memory from the system."""
    if case.name not in _SOLO:
        ins = case.build(case.dims)
        pool = _on(dev, ins)
        calls, pools, words = case.calls(case.dims), [], []
        for call in calls:
            pools.append(dict(pool))
            words.append(U.run_call(call, pool, dev, {}))
            pool.update({k: torch.from_numpy(v).to(dev) for k, v in words[-1].items()})
        op_ins, op_words = _on(dev, ins), {}
        if case.op is not None:
            op_words = {k: U.words(v) for k, v in case.op(op_ins).items()}
        torch.cuda.synchronize(dev)
        _SOLO[case.name] = Solo(calls, pools, words, op_ins, op_words)
    return _SOLO[case.name]


def _cloned(pending: U.Pending) -> U.Pending:
    """Clones of a pending call's guarded outputs, guards included, enqueued on the current stream."""
    outs = []
    for a, g in pending.outs:
        twin = copy.copy(g)
        twin.flat = g.flat.clone()
        outs.append((a, twin))
    return U.Pending(outs, pending.alive)


def late_call(call: U.Call, pool: dict[str, Any], dev: torch.device, ms: float, tag: str = '') -> tuple[dict[str, np.ndarray], bool]:
    """``call`` on a side stream behind a delay of ``ms`` and behind its own inputs: the words of the stream-ordered
    clones of its outputs (guards intact, every word written), and whether the delay was still running the moment the
    library's function returned."""
    side = side_stream(dev)
    busy: list[bool] = []
    with torch.cuda.stream(side):
        gate = delay(ms)
        t0 = time.perf_counter()
        pending = U.enqueue_call(call, pool, dev, {}, returned=lambda: busy.append(not gate.query()))
        seconds = time.perf_counter() - t0
        clones = _cloned(pending)
    torch.cuda.synchronize(dev)
    key = (tag, call.symbol)
    ENQUEUE_S[key] = max(ENQUEUE_S.get(key, 0.0), seconds)
    return U.collect_call(clones), busy[0]


def late_op(case: U.Case, op_ins: dict[str, Any], dev: torch.device, ms: float) -> dict[str, np.ndarray]:
    """The Python op of ``case``, forward and backward, on a side stream behind a delay of ``ms``, its inputs cloned onto
    that stream behind the delay: the words of stream-ordered clones of everything it returns."""
    side = side_stream(dev)
    with torch.cuda.stream(side):
        delay(ms)
        late = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in op_ins.items()}
        got = {k: v.detach().clone() for k, v in case.op(late).items()}
    torch.cuda.synchronize(dev)
    return {k: U.words(v) for k, v in got.items()}


def ring() -> list[tuple[U.Case, U.Case]]:
    """Every case with the next one of the registry, the last with the first."""
    return [(case, U.CASES[(i + 1) % len(U.CASES)]) for i, case in enumerate(U.CASES)]


def ring_pair(a: U.Case, b: U.Case, dev: torch.device) -> tuple[list[list[dict[str, np.ndarray]]], list[bool]]:
    """``a`` on one side stream and ``b`` on another, each behind its own delay, their calls enqueued alternately with no
    wait until both are enqueued: per case the words of every call (stream-ordered clones), and whether each delay was
    still running when the last call had returned."""
    solos = (solo(a, dev), solo(b, dev))
    streams = (side_stream(dev), side_stream(dev))
    ms = DELAY_MS * (len(solos[0].calls) + len(solos[1].calls))
    gates = []
    for stream in streams:
        with torch.cuda.stream(stream):
            gates.append(delay(ms))
    clones: tuple[list[U.Pending], list[U.Pending]] = ([], [])
    for i in range(max(len(s.calls) for s in solos)):
        for which in (0, 1):
            if i < len(solos[which].calls):
                with torch.cuda.stream(streams[which]):
                    clones[which].append(_cloned(U.enqueue_call(solos[which].calls[i], solos[which].pools[i], dev, {})))
    busy = [not gate.query() for gate in gates]
    torch.cuda.synchronize(dev)
    return [[U.collect_call(c) for c in clones[which]] for which in (0, 1)], busy


def may_wait(case: U.Case) -> bool:
    """A stream that carries all of ``case`` can meet the condition of ``WAITS``: two or more of its calls free a pool block."""
    return sum(call.symbol in WAITS for call in case.calls(case.dims)) >= 2


def covered() -> set[str]:
    """The symbols the stream suite runs: it is parametrised over the whole registry."""
    return U.covered()


CASES = U.CASES  # (read after the three imports above: all of them, however the file that imports this one is run)


# ---- launches that only exist above the registry's shapes ----------------------------------------------------------------------
# The registry holds the smallest eligible shapes.  Read launcher by launcher, these are the entry points whose NUMBER of
# launches (not which instantiation) depends on the size or on a path the size selects; each gets one late-input case at the
# smallest shape an existing test names for that boundary, the path forced through its measurement switch where the product
# takes it only at sizes too large for a quick test:
#
#   pcc_knn_cross             candidates in slices: the sliced selection launch and the merge launch
#                             (tests/test_gpu_knn_stress.py: n = 300, knn_cross_split)
#   pcc_knn                   the wide path: a distance launch (c > 3) and a selection launch (tests/test_gpu_knn_wide.py, knn_wide)
#   pcc_sinkhorn              column slices: a merge launch behind every scan (tests/test_gpu_sinkhorn.py: 257 columns, sinkhorn_split)
#   pcc_match_cost            two lanes, the second on the library's own stream, joined back before the call's last launches; no
#                             resident fine-level launch, so one launch per pass and lane (tests/test_gpu_structural.py: b = 32,
#                             n = m = 2048 -- b >= 8 and b * n >= 32768; 16 samples x 32 tiles per lane exceed the chip)
#   pcc_fps                   the memory path: a workspace from the pool, freed on the stream (tests/test_gpu_fps.py, fps_path = 7)
#   pcc_segment_pool,         a third launch for the runs of more than 64 points, from n > 64 on (tests/test_gpu_grid_pool.py,
#   pcc_voxelize              tests/test_gpu_voxelize.py)
#   pcc_grid_cluster_ragged   one histogram, scan (three launches) and scatter per 8 bits of the key: 2 rounds at the registry's
#                             axis_bits = 4, 7 at axis_bits = 16 (tests/test_gpu_grid_ragged.py); the scan itself is three launches
#                             at every length
#
# The sorted searches (pcc_knn at c <= 3, pcc_chamfer_emd) launch the sort and the search at the registry's shapes already; above
# the sort's capacity they launch less, not more.


class Sized(NamedTuple):
    case: U.Case                                     # build and calls as in the registry: no op, no anchor
    launched: Callable[[dict[str, int]], None]       # the launch record of all its late calls holds the extra launches


def _has(*kernels: str) -> Callable[[dict[str, int]], None]:
    def launched(names: dict[str, int]) -> None:
        missing = [k for k in kernels if k not in names]
        assert not missing, f'{missing} did not launch: {names}'
    return launched


def _sized_knn(c: int) -> list[Sized]:
    from tests import knn_reference as kr

    d = dict(b=U.B, c=c, n=300, nq=48, k=4)
    assert kr.cross_slices(d['b'] * d['nq'], d['n'], 256, 2) == 2
    cross = U.Case(f'knn_cross_sliced_c{c}', d, U._knn_build(200 + c),
                   lambda d: [U.Call('pcc_knn_cross', [d['b'], d['c'], d['nq'], d['n'], d['k'], 'q', 'x', U.Out('indices', (d['b'], d['nq'], d['k']), U.I64),
                                                      U.Out('dist', (d['b'], d['nq'], d['k']))], tune=('knn_cross_split', 2))])
    wide = U.Case(f'knn_wide_c{c}', d, U._knn_build(210 + c),
                  lambda d: [U.Call('pcc_knn', [d['b'], d['c'], d['n'], d['k'], 'x', U.Out('indices', (d['b'], d['n'], d['k']), U.I64)], tune=('knn_wide', 1))])
    return [Sized(cross, _has(kr.wide_select(c, 4, True), kr.wide_merge(4))),
            Sized(wide, _has(kr.wide_select(c, 4), *(('knn_wide_dist_kernel',) if c > 3 else ())))]


def _sized_sinkhorn() -> Sized:
    from tests import sinkhorn_reference as ref

    d = dict(b=U.B, n=257, m=64)
    assert ref.slices(d['n'], d['m'], True, 2) == 2

    def build(d: dict[str, int]) -> dict[str, Any]:
        x, y = ref.clouds(12, d['b'], d['n'], d['m'])
        return {'p1': U._t(x), 'p2': U._t(y)}

    def calls(d: dict[str, int]) -> list[U.Call]:
        x, y = ref.clouds(12, d['b'], d['n'], d['m'])
        eps = ref.schedule(8, ref.diameter(x, y))
        import ctypes

        sched = (ctypes.c_float * len(eps))(*eps)  # host memory, read before the call returns
        return [U.Call('pcc_sinkhorn', [d['b'], d['n'], d['m'], 'p1', 'p2', len(eps), ctypes.cast(sched, ctypes.c_void_p), 1, U.Out('cost', (d['b'],)),
                                        U.Out('pot1', (d['b'], d['n'])), U.Out('pot2', (d['b'], d['m']))] + U._grad_outs(d['b'], d['n'], d['m']),
                       tune=('sinkhorn_split', 2))]

    return Sized(U.Case('sinkhorn_sliced', d, build, calls), _has(ref.scan_kernel(d['n'], d['m'], True, 2), 'sk_merge_kernel'))


def _sized_match_cost() -> Sized:
    def build(d: dict[str, int]) -> dict[str, Any]:
        from tests.util import pair

        p1, p2 = pair(31, d['b'], d['n'], d['m'], 'recon')  # (the clouds of test_calls_on_two_caller_streams_at_once, which holds
        return {'p1': U._t(p1), 'p2': U._t(p2)}            # their words equal from call to call)

    def launched(names: dict[str, int]) -> None:
        assert names.get('pair_finish_kernel') == 2 and names.get('am_pair_kernel<grad>') == 2, f'not two lanes: {names}'
        assert 'am_fine_persist_kernel' not in names, names

    d = dict(b=32, n=2048, m=2048)
    return Sized(U.Case('match_cost_two_lanes', d, build,
                        lambda d: [U.Call('pcc_match_cost', [d['b'], d['n'], d['m'], 'p1', 'p2', None, U.Out('cost', (d['b'],))]
                                          + U._grad_outs(d['b'], d['n'], d['m']))]), launched)


def _sized_fps() -> Sized:
    d = dict(b=U.B, n=64, m=8)
    return Sized(U.Case('fps_memory_path', d, U._sample_build,
                        lambda d: [U.Call('pcc_fps', [d['b'], d['n'], d['m'], 'xyz', 'start', U.Out('idx', (d['b'], d['m']), U.I64), U.Out('dist', (d['b'], d['m']))],
                                          tune=('fps_path', 7))]), _has('fps_mem_kernel'))


LONG_RUN = 80  # points of every cloud in its cell 0: a run of more than 64


def _sized_long_runs() -> Sized:
    def build(d: dict[str, int]) -> dict[str, Any]:
        from tests import grid_pool_reference as gref
        from tests import voxel_reference as vref

        rng = U._rng(190)
        b, c, n, m, res = (d[s] for s in ('b', 'c', 'n', 'm', 'res'))
        xyz = U._lattice(rng, b, n, 3, steps=1, reach=res)
        xyz[:, :LONG_RUN] = 0.0
        cell, order, counts = vref.voxel_index(xyz.numpy(), res, 0.0, res - 1.0)
        assert (counts.reshape(b, -1)[:, 0] >= LONG_RUN).all()
        _, seg, _ = gref.grid_cluster(cell, order, m)
        return {'x': U._ints(rng, b, c, n), 'cell': U._t(cell, np.int32), 'order': U._t(order, np.int32),
                'counts': U._t(counts.reshape(b, res, res, res), np.int32), 'seg': U._t(seg, np.int32)}

    def calls(d: dict[str, int]) -> list[U.Call]:
        b, c, n, m, res = (d[s] for s in ('b', 'c', 'n', 'm', 'res'))
        out = [U.Call('pcc_voxelize', [b, c, n, res, 'x', 'cell', 'order', 'counts', U.Out('grid_out', (b, c, res, res, res))])]
        for name, mode in U.POOL_MODES.items():
            out.append(U.Call('pcc_segment_pool', [b, c, n, m, mode, 'x', 'order', 'seg', U.Out('out_' + name, (b, c, m)),
                                                   U.Out('arg_out', (b, c, m), U.I32) if mode == 2 else None]))
        return out

    def launched(names: dict[str, int]) -> None:
        assert names.get('vox_long_kernel') == 1 and names.get('seg_long_kernel') == len(U.POOL_MODES), names

    return Sized(U.Case('long_runs', dict(b=U.B, c=12, n=128, m=8, res=2), build, calls), launched)


def _sized_grid_ragged() -> Sized:
    from tests import unaligned_views_grid_ragged as G

    def launched(names: dict[str, int]) -> None:
        assert names.get('rg_hist_kernel') == 7 and names.get('rg_scatter_kernel') == 7 and names.get('rg_scan_reduce_kernel') == 8, names

    d = dict(G.CASE_DIMS, axis_bits=16)  # the key: 2 bits of cloud + 48 of cell = 50 bits, 7 rounds of 8
    return Sized(U.Case('grid_cluster_ragged_7_rounds', d, G._build, lambda d: G._calls(d)[:1]), launched)


def sized() -> list[Sized]:
    return _sized_knn(3) + _sized_knn(8) + [_sized_sinkhorn(), _sized_match_cost(), _sized_fps(), _sized_long_runs(), _sized_grid_ragged()]


SIZED = sized()
