"""Contiguous tensors that start off a 16-byte boundary, for every computing entry point of the C ABI.

The binding layer (``_lib.ptr``) accepts any contiguous tensor of the right dtype; it does not look at the address.  A chunk of
a batch, a parameter inside a flattened buffer or a gradient ``torch.cat``'s backward hands on starts 4, 8 or 12 bytes past a
16-byte boundary, and the kernels take their 16-byte accesses only where the sizes AND the address allow it.  This module holds

* ``shifted(t, elements)``: the same values in a contiguous view that starts ``elements`` elements into a fresh buffer;
* ``guarded(shape, dtype, device, elements)``: a caller-provided output between sentinel words, prefilled with a word no kernel
  writes, its body ``elements`` elements off a 16-byte boundary;
* ``CASES``: per entry point of ``_lib.ABI`` (``EXEMPT`` lists those without a tensor argument) the inputs at the smallest
  shape at which every wide path is eligible in every sample -- every per-sample and per-row word count a multiple of 4, so
  that the aligned call is aligned in sample 1 too and the shifted call is misaligned in every sample --, the calls through
  the C ABI with every tensor argument named, the Python op where there is one, the size condition of the gate the case is
  aimed at, and the exact reference the aligned result is tied to.

Importable without a device: tests/test_unaligned_views_host.py checks the registry against ``_lib.ABI`` and the CPU paths,
tests/test_gpu_unaligned_views.py runs every case."""

from __future__ import annotations

import contextlib
import ctypes
from typing import Any, Callable, NamedTuple

import numpy as np
import torch

F32, I32, I64 = torch.float32, torch.int32, torch.int64
GUARD = 32                 # words of sentinel on either side of a guarded output
FLOAT_FILL = 0x7fdead00    # a NaN whose payload no kernel produces
INT_FILL = -7777
SHIFTS = {F32: (1, 2, 3), I32: (1, 2, 3), I64: (1,)}  # elements: 4, 8 and 12 bytes; 8 bytes for an int64 list

EXEMPT = {'pcc_version', 'pcc_last_error', 'pcc_last_status', 'pcc_profile_enable', 'pcc_profile_reset', 'pcc_profile_read', 'pcc_profile_names',
          'pcc_approxmatch_workspace_bytes', 'pcc_auction_status', 'pcc_test_inject_auction_failure',
          'pcc_test_inject_approxmatch_failure', 'pcc_test_set_tuning'}


def shifted(t: torch.Tensor, elements: int = 1) -> torch.Tensor:
    """A contiguous view with ``t``'s shape, dtype and values that starts ``elements`` elements into a fresh buffer."""
    buf = torch.empty(t.numel() + elements, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[elements:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (elements * t.element_size()) % 16
    return v


class guarded:
    """An output of ``shape`` inside a flat buffer with GUARD sentinel words on either side, its body ``elements`` elements
    past a 16-byte boundary.  Floats start as NaN with the payload FLOAT_FILL, integers as INT_FILL: ``numpy()`` asserts both
    guards intact and (``whole``) every body word written."""

    def __init__(self, shape: tuple[int, ...], dtype: torch.dtype, device: Any, elements: int = 0) -> None:
        self.is_float = dtype == F32
        numel = int(np.prod(shape))
        self.fill = FLOAT_FILL if self.is_float else INT_FILL
        self.flat = torch.full((numel + 2 * GUARD + elements,), self.fill, dtype=I32 if self.is_float else dtype, device=device)
        assert self.flat.data_ptr() % 16 == 0
        self.lo, self.hi = GUARD + elements, GUARD + elements + numel
        body = self.flat[self.lo:self.hi]
        self.tensor = (body.view(F32) if self.is_float else body).view(shape)
        assert self.tensor.is_contiguous() and self.tensor.data_ptr() % 16 == (elements * self.tensor.element_size()) % 16

    def ptr(self) -> int:
        return self.tensor.data_ptr()

    def numpy(self, whole: bool = True) -> np.ndarray:
        flat = self.flat.cpu().numpy()
        assert (flat[:self.lo] == self.fill).all(), 'a word before the output was overwritten'
        assert (flat[self.hi:] == self.fill).all(), 'a word behind the output was overwritten'
        body = flat[self.lo:self.hi].reshape(self.tensor.shape)
        assert not whole or not (body == self.fill).any(), 'an output word was not written'
        return body.view(np.float32) if self.is_float else body


def words(a: Any) -> np.ndarray:
    """The bit patterns of a tensor or array as integers of its width: NaN payloads and the sign of zero count."""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_words(a: Any, b: Any) -> bool:
    a, b = words(a), words(b)
    return a.shape == b.shape and bool((a == b).all())


class Out(NamedTuple):
    """A caller-provided output of a C call.  ``keep``: the part of it the contract defines (the rest is scratch)."""

    name: str
    shape: tuple[int, ...]
    dtype: torch.dtype = F32
    whole: bool = True
    keep: Callable[[np.ndarray], np.ndarray] | None = None


class Scratch(NamedTuple):
    """A 16-byte aligned workspace (never shifted: ``pcc_approxmatch_ws`` refuses a misaligned one) and its size in bytes."""

    nbytes: Callable[[], int]


class Call(NamedTuple):
    """One call through the C ABI.  ``args``: a str names an input tensor of the pool (``None`` in the pool: NULL), an ``Out`` a
    guarded output, anything else is passed as it is.  ``tune``: a measurement switch set around the call (a path switch).
    ``void``: one of the reference-named launchers, which report through ``pcc_last_status``."""

    symbol: str
    args: list[Any]
    tune: tuple[str, int] | None = None
    void: bool = False


class Case(NamedTuple):
    name: str
    dims: dict[str, int]
    build: Callable[[dict[str, int]], dict[str, Any]]             # CPU inputs by name
    calls: Callable[[dict[str, int]], list[Call]]
    op: Callable[[dict[str, Any]], dict[str, torch.Tensor]] | None = None  # the Python op (and its backward) on named inputs
    op_inputs: tuple[str, ...] = ()                                # the inputs the op reads
    cpu: bool = False                                              # the op has a CPU path
    gate: Callable[[dict[str, int]], bool] | None = None           # the size condition of the wide path the case is aimed at
    # the aligned result -- the outputs of the C calls and, under their own names, of the op -- against its reference
    anchor: Callable[[dict[str, int], dict[str, np.ndarray], Any], None] | None = None
    probe: Callable[[dict[str, int], dict[str, Any], Any], None] | None = None  # a check on the device beyond the words

    def symbols(self) -> set[str]:
        return {c.symbol for c in self.calls(self.dims)}


def tensor_args(call: Call, pool: dict[str, Any]) -> list[tuple[str, torch.dtype]]:
    """``(name, dtype)`` of every tensor the call touches: the inputs that are not NULL, then the outputs."""
    ins = [(a, pool[a].dtype) for a in call.args if isinstance(a, str) and pool[a] is not None]
    return ins + [(a.name, a.dtype) for a in call.args if isinstance(a, Out)]


def variants(call: Call, pool: dict[str, Any]) -> list[dict[str, int]]:
    """The shifts of one call: every tensor argument alone by each of its dtype's offsets, then all of them by one element."""
    names = tensor_args(call, pool)
    return [{name: e} for name, dtype in names for e in SHIFTS[dtype]] + [{name: 1 for name, _ in names}]


class Pending(NamedTuple):
    """A call that ``enqueue_call`` has made and nobody has waited for: its guarded outputs, and the argument tensors, which
    must outlive the kernels that read them."""

    outs: list[tuple[Out, guarded]]
    alive: list[torch.Tensor]


def enqueue_call(call: Call, pool: dict[str, Any], dev: torch.device, shift: dict[str, int],
                 returned: Callable[[], None] | None = None) -> Pending:
    """The call on the device tensors of ``pool``, the arguments named in ``shift`` that many elements off a 16-byte boundary
    (the others on one), built and enqueued on the current stream of ``dev`` without waiting for anything.  ``returned`` runs
    the moment the library's function has returned (tests/stream_order.py asks there whether the stream is still busy)."""
    from pointcloudcounterfactual_amd import _lib

    args: list[Any] = []
    outs: list[tuple[Out, guarded]] = []
    alive = []
    for a in call.args:
        if isinstance(a, str):
            t = pool[a]
            if t is None:
                args.append(None)
                continue
            v = shifted(t, shift.get(a, 0))
            alive.append(v)
            args.append(v.data_ptr())
        elif isinstance(a, Out):
            g = guarded(a.shape, a.dtype, dev, shift.get(a.name, 0))
            outs.append((a, g))
            args.append(g.ptr())
        elif isinstance(a, Scratch):
            nbytes = int(a.nbytes())
            ws = torch.zeros(nbytes + 16, dtype=torch.uint8, device=dev)
            assert ws.data_ptr() % 16 == 0
            alive.append(ws)
            args += [ws.data_ptr(), ctypes.c_size_t(nbytes)]
        else:
            args.append(a)
    fn = getattr(_lib.lib, call.symbol)
    with _lib.tuning(*call.tune) if call.tune else contextlib.nullcontext():
        with torch.cuda.device(dev):
            status = fn(*args, torch.cuda.current_stream(dev).cuda_stream)
        if returned is not None:
            returned()
        if call.void:
            assert status is None
            assert _lib.lib.pcc_last_status() == 0, _lib.lib.pcc_last_error()
        else:
            _lib.check(status, call.symbol)
    return Pending(outs, alive)


def collect_call(pending: Pending) -> dict[str, np.ndarray]:
    """The outputs of a call of ``enqueue_call`` as numpy, guards checked.  The caller has waited for the call: the copies
    to the host are made on the current stream, which need not be the call's."""
    got = {}
    for a, g in pending.outs:
        body = g.numpy(a.whole)
        got[a.name] = body if a.keep is None else a.keep(body)
    return got


def run_call(call: Call, pool: dict[str, Any], dev: torch.device, shift: dict[str, int]) -> dict[str, np.ndarray]:
    """``enqueue_call`` on the current stream, a wait for the device, and ``collect_call``."""
    pending = enqueue_call(call, pool, dev, shift)
    torch.cuda.synchronize(dev)
    return collect_call(pending)


# ---- inputs -------------------------------------------------------------------------------------------------------------------
# Integers, dyadic weights and lattice coordinates wherever a kernel adds with atomics: every partial sum is exact, so the
# words do not depend on the order and equality is the bar.

B = 2


def _rng(seed: int) -> np.random.Generator:
    return np.random.default_rng(seed)


def _t(a: Any, dtype: Any = np.float32) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype))


def _ints(rng: np.random.Generator, *shape: int) -> torch.Tensor:
    return _t(rng.integers(-4, 5, size=shape))


def _dyadic(rng: np.random.Generator, *shape: int) -> torch.Tensor:
    return _t(rng.choice(np.array([0, .5, -.5, 1, -1, 2, -2]), size=shape))


def _lattice(rng: np.random.Generator, *shape: int, steps: int = 16, reach: float = 1.0) -> torch.Tensor:
    """Coordinates on a lattice of ``steps`` per unit in ``[0, reach)``: differences, squares and their sums are exact."""
    return _t(rng.integers(0, int(steps * reach), size=shape) / float(steps))


def _cloud(rng: np.random.Generator, *shape: int) -> torch.Tensor:
    return _t(rng.random(shape))


def _list(rng: np.random.Generator, b: int, m: int, k: int, n: int, pad: float = 0.15) -> torch.Tensor:
    """``idx[b,m,k]`` int64 into n points, about ``pad`` of the slots -1 (the padding of ``ball_query(pad='none')``)."""
    idx = rng.integers(0, n, size=(b, m, k))
    idx[rng.random((b, m, k)) < pad] = -1
    return _t(idx, np.int64)


def _leaf(t: torch.Tensor | None) -> torch.Tensor | None:
    return None if t is None else t.detach().requires_grad_(True)


def _ops() -> Any:
    from pointcloudcounterfactual_amd import neighbour_ops

    return neighbour_ops


CASES: list[Case] = []


def _case(*args: Any, **kwargs: Any) -> None:
    CASES.append(Case(*args, **kwargs))


# ---- structural losses (include/pcc_structural.h) ---------------------------------------------------------------------------

def _pair_build(seed: int) -> Callable[[dict[str, int]], dict[str, Any]]:
    def build(d: dict[str, int]) -> dict[str, Any]:
        rng = _rng(seed)
        b, n, m = d['b'], d['n'], d['m']
        p1, p2 = _cloud(rng, b, n, 3), _cloud(rng, b, m, 3)
        dm = ((p1[:, :, None, :].double() - p2[:, None, :, :].double()) ** 2).sum(-1)
        return {'p1': p1, 'p2': p2, 'g1': _ints(rng, b, n), 'g2': _ints(rng, b, m), 'gl': _ints(rng, b) + 0.5, 'ge': _ints(rng, b) + 0.5,
                'idx1': dm.argmin(2).to(I32), 'idx2': dm.argmin(1).to(I32), 'theta': _dyadic(rng, d.get('p', 1), 3),
                'match': _cloud(rng, b, m, n)}
    return build


def _nn_outs(b: int, n: int, m: int, tag: str = '') -> list[Out]:
    return [Out('dist1' + tag, (b, n)), Out('idx1' + tag, (b, n), I32), Out('dist2' + tag, (b, m)), Out('idx2' + tag, (b, m), I32)]


def _nn_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    want = oracle.nndistance(p['p1'], p['p2'])
    for tag in ('', '_void'):
        for name, w in zip(('dist1', 'idx1', 'dist2', 'idx2'), want):
            assert same_words(p[name + tag], w), name + tag


_case('nndistance', dict(b=B, n=64, m=48), _pair_build(1),
      lambda d: [Call('pcc_nndistance', [d['b'], d['n'], 'p1', d['m'], 'p2'] + _nn_outs(d['b'], d['n'], d['m'])),
                 Call('nndistance', [d['b'], d['n'], 'p1', d['m'], 'p2'] + _nn_outs(d['b'], d['n'], d['m'], '_void'), void=True)],
      anchor=_nn_anchor)


def _lattice_pair_build(seed: int) -> Callable[[dict[str, int]], dict[str, Any]]:
    """The 'exact' inputs of tests/structural_grad_reference.py (the loss entries with ``mean``): coordinates on a lattice of
    1/16, nearest-neighbour lists of those clouds, integer gradients sized so that every sum the backward kernels form --
    they add scattered terms with LDS atomics -- is exact in float32 in any order."""
    def build(d: dict[str, int]) -> dict[str, Any]:
        from tests import structural_grad_reference as R

        inp = R.chamfer_inputs(d['b'], d['n'], d['m'], 'nn', 'exact', True, seed)
        out = {k: _t(inp[k]) for k in ('p1', 'p2', 'g1', 'g2', 'gemd')}
        out.update(idx1=_t(inp['idx1'], np.int32), idx2=_t(inp['idx2'], np.int32), gl=_t(inp['gloss']))
        return out
    return build


def _check_chamfer_grads(what: str, p: dict[str, np.ndarray], names: tuple[str, str], g1: np.ndarray, g2: np.ndarray, tail: bool = False) -> None:
    """``names`` against the float64 gradients of sum g1 dist1 + sum g2 dist2 along the lists in ``p`` (and, ``tail``, plus
    emd_grad * gemd), inside the derived bound of structural_grad_reference.py; word for word where its exact-mode premise
    (every sum below 2^24 quanta, a result that float32 holds) is met, which the reference checks on itself."""
    from tests import structural_grad_reference as R

    ref = R.chamfer_bwd_ref(p['p1'], p['p2'], p['idx1'], p['idx2'], g1, g2)
    for which, name in zip((1, 2), names):
        if tail:
            want, bound, mag = R.emd_tail_ref(ref, which, p[f'emd_grad{which}'], p['gemd'], p['p1'].shape[0])
        else:
            want, bound, mag = ref[f'grad{which}'], R.chamfer_bound(ref, which), ref[f'mag{which}']
        R.assert_close(f'{what} {name}', p[name], want, bound)
        if not tail:
            R.assert_exact(f'{what} {name}', want, mag)
            R.assert_words(f'{what} {name}', p[name], want.astype(np.float32))


def _nngrad_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    for tag in ('', '_void'):
        _check_chamfer_grads('nndistancegrad', p, ('grad1' + tag, 'grad2' + tag), p['g1'].astype(np.float64), p['g2'].astype(np.float64))


def _grad_outs(b: int, n: int, m: int, tag: str = '') -> list[Out]:
    return [Out('grad1' + tag, (b, n, 3)), Out('grad2' + tag, (b, m, 3))]


_case('nndistancegrad', dict(b=B, n=64, m=48), _lattice_pair_build(2),
      lambda d: [Call('pcc_nndistancegrad', [d['b'], d['n'], 'p1', d['m'], 'p2', 'g1', 'idx1', 'g2', 'idx2'] + _grad_outs(d['b'], d['n'], d['m'])),
                 Call('nndistancegrad', [d['b'], d['n'], 'p1', d['m'], 'p2', 'g1', 'idx1', 'g2', 'idx2'] + _grad_outs(d['b'], d['n'], d['m'], '_void'),
                      void=True)],
      anchor=_nngrad_anchor)


def _chamfer_loss_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any, tail: bool = False) -> None:
    from tests import structural_grad_reference as R

    b, n, m = d['b'], d['n'], d['m']
    want = oracle.nndistance(p['p1'], p['p2'])
    for name, w in zip(('dist1', 'idx1', 'dist2', 'idx2'), want):
        assert same_words(p[name], w), name
    # loss = mean dist1 + mean dist2 of the float32 distances: n + m non-negative terms added in some fixed order, two
    # divisions and one addition, so within gamma(n + m + 3) of the float64 value of the same expression
    loss64 = want[0].astype(np.float64).mean(1) + want[2].astype(np.float64).mean(1)
    R.assert_close('loss', p['loss'], loss64, R.g(n + m + 3.0) * loss64)
    l1, l2 = R.loss_gradients(p['gl'], b, n, m, True)
    _check_chamfer_grads('chamfer_emd_grad' if tail else 'chamfer_loss_grad', p, ('grad1', 'grad2'), l1, l2, tail)


_case('chamfer_loss', dict(b=B, n=64, m=48), _lattice_pair_build(3),
      lambda d: [Call('pcc_chamfer_loss', [d['b'], d['n'], 'p1', d['m'], 'p2', 1, Out('loss', (d['b'],))] + _nn_outs(d['b'], d['n'], d['m'])),
                 Call('pcc_chamfer_loss_grad', [d['b'], d['n'], 'p1', d['m'], 'p2', 'idx1', 'idx2', 'gl', 1, 1] + _grad_outs(d['b'], d['n'], d['m']))],
      anchor=_chamfer_loss_anchor)


def _chamfer_emd_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    # pcc_chamfer_emd is pcc_chamfer_loss + pcc_match_cost, "same outputs, same bits" (include/pcc_structural.h): the EMD
    # half is tied to pcc_match_cost's words on these clouds, and pcc_match_cost to float64 in its own case, on clouds of the
    # unit scale its bars are stated for.  (These lattice clouds span [-2, 2]^3: measured against the float64 recurrence their
    # cost is 1.04e-5 relative, where the bar of unit-scale clouds is 1e-5; the accuracy of the approximate EMD off the unit
    # scale is not what this case is about, and no bar is set for it here.)
    for name, twin in (('cost', 'mc_cost'), ('emd_grad1', 'mc_grad1'), ('emd_grad2', 'mc_grad2')):
        assert same_words(p[name], p[twin]), name
    _chamfer_loss_anchor(d, p, oracle, tail=True)


_case('chamfer_emd', dict(b=B, n=64, m=48), _lattice_pair_build(4),
      lambda d: [Call('pcc_chamfer_emd', [d['b'], d['n'], 'p1', d['m'], 'p2', 1, Out('loss', (d['b'],))] + _nn_outs(d['b'], d['n'], d['m'])
                      + [Out('cost', (d['b'],)), Out('emd_grad1', (d['b'], d['n'], 3)), Out('emd_grad2', (d['b'], d['m'], 3))]),
                 Call('pcc_match_cost', [d['b'], d['n'], d['m'], 'p1', 'p2', None, Out('mc_cost', (d['b'],)), Out('mc_grad1', (d['b'], d['n'], 3)),
                                         Out('mc_grad2', (d['b'], d['m'], 3))]),
                 Call('pcc_chamfer_emd_grad', [d['b'], d['n'], 'p1', d['m'], 'p2', 'idx1', 'idx2', 'gl', 1, 1, 'emd_grad1', 'emd_grad2', 'gemd', 1]
                      + _grad_outs(d['b'], d['n'], d['m']))],
      anchor=_chamfer_emd_anchor)


def _set_metrics() -> Any:
    from pointcloudcounterfactual_amd import set_metrics

    return set_metrics


def _chamfer_matrix_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    d_ab, d_ba = _set_metrics().pairwise_chamfer(i['p1'], i['p2'], directional=True)
    return {'d_ab': d_ab, 'd_ba': d_ba}


def _chamfer_matrix_build(d: dict[str, int]) -> dict[str, Any]:
    rng = _rng(5)
    return {'p1': _lattice(rng, d['b'], d['n'], 3), 'p2': _lattice(rng, d['b'], d['m'], 3)}


# lattice coordinates and n, m powers of two: every distance, every sum of them and both means are exact in float32, so the
# CPU path (float64, rounded once at the end) holds the kernel's words
_case('chamfer_matrix', dict(b=B, n=64, m=32), _chamfer_matrix_build,
      lambda d: [Call('pcc_chamfer_matrix', [d['b'], d['n'], 'p1', d['b'], d['m'], 'p2', 1, Out('d_ab', (d['b'], d['b'])), Out('d_ba', (d['b'], d['b']))])],
      op=_chamfer_matrix_op, op_inputs=('p1', 'p2'), cpu=True, anchor=lambda d, p, oracle: _cpu_anchor(_chamfer_matrix_op, ('d_ab', 'd_ba'))(d, p, oracle))


def _occupancy_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    sm = _set_metrics()
    return {'counts': sm.occupancy_grid(i['centred'], 4, per_cloud=True).to(I32), 'sphere': sm.occupancy_grid(i['centred'], 4, in_sphere=True).to(I32)}


def _occupancy_build(d: dict[str, int]) -> dict[str, Any]:
    return {'centred': _cloud(_rng(6), d['b'], d['n'], 3) - 0.5}


def _occupancy_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    want = _occupancy_op({'centred': torch.from_numpy(p['centred'])})  # the CPU path: the same float32 operations, the same integers
    assert same_words(p['counts'], want['counts']) and same_words(p['sphere'], want['sphere'])


_case('occupancy_grid', dict(b=B, n=64, res=4), _occupancy_build,
      lambda d: [Call('pcc_occupancy_grid', [d['b'], d['n'], 'centred', d['res'], -0.5, 1.0, 0, 1, Out('counts', (d['b'],) + (d['res'],) * 3, I32)]),
                 Call('pcc_occupancy_grid', [d['b'], d['n'], 'centred', d['res'], -0.5, 1.0, 1, 0, Out('sphere', (d['res'],) * 3, I32)])],
      op=_occupancy_op, op_inputs=('centred',), cpu=True, anchor=_occupancy_anchor)


def _backend() -> Any:
    from pointcloudcounterfactual_amd import backend

    return backend


def _ws_bytes(d: dict[str, int]) -> Callable[[], int]:
    def nbytes() -> int:
        from pointcloudcounterfactual_amd import _lib

        return int(_lib.lib.pcc_approxmatch_workspace_bytes(d['b'], d['n'], d['m']))
    return nbytes


def _am_outs(d: dict[str, int], tag: str) -> list[Out]:
    nm = d['n'] + d['m']  # temp: remainL | remainR are the contract's; the ratios behind them are the last level's scratch
    return [Out('match' + tag, (d['b'], d['m'], d['n'])), Out('temp' + tag, (d['b'], 2 * nm), whole=False, keep=lambda a: a[:, :nm].copy())]


def _approxmatch_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests.util import check_match_cost

    # the four entry points run the same passes: their words are the same; the float64 recurrence ties the cost
    for tag in ('_void', '_ws', '_cost'):
        assert same_words(p['match' + tag], p['match']) and same_words(p['temp' + tag], p['temp']), tag
    check_match_cost(oracle, p['p1'], p['p2'], p['cost'])


_case('approxmatch', dict(b=B, n=64, m=48), _pair_build(7),
      lambda d: [Call('pcc_approxmatch', [d['b'], d['n'], d['m'], 'p1', 'p2'] + _am_outs(d, '')),
                 Call('approxmatch', [d['b'], d['n'], d['m'], 'p1', 'p2'] + _am_outs(d, '_void'), void=True),
                 Call('pcc_approxmatch_ws', [d['b'], d['n'], d['m'], 'p1', 'p2'] + _am_outs(d, '_ws') + [Scratch(_ws_bytes(d))]),
                 Call('pcc_approxmatch_cost', [d['b'], d['n'], d['m'], 'p1', 'p2'] + _am_outs(d, '_cost') + [Out('cost', (d['b'],))])],
      gate=lambda d: d['n'] % 4 == 0, anchor=_approxmatch_anchor)


def _matchcost_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import structural_grad_reference as R

    ref, refs = R.match_ref(p['p1'], p['p2'], p['match']), R.match_ref(p['p1'], p['p2'], p['match'], p['gc'])
    for tag in ('', '_void'):
        R.assert_close('cost' + tag, p['cost' + tag], *ref['cost'])
        R.assert_close('grad1' + tag, p['grad1' + tag], *ref['grad1'])
        R.assert_close('grad2' + tag, p['grad2' + tag], *ref['grad2'])
    R.assert_close('grad1 scaled', p['grad1_scaled'], *refs['grad1'])
    R.assert_close('grad2 scaled', p['grad2_scaled'], *refs['grad2'])


def _matchcost_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import structural_grad_reference as R

    p1, p2, match, gc = R.match_inputs(d['b'], d['n'], d['m'], 'dense', 8)
    return {'p1': _t(p1), 'p2': _t(p2), 'match': _t(match), 'gc': _t(gc)}


def _matchcost_calls(d: dict[str, int]) -> list[Call]:
    head = [d['b'], d['n'], d['m'], 'p1', 'p2', 'match']
    return [Call('pcc_matchcost', head + [Out('cost', (d['b'],))]),
            Call('matchcost', head + [Out('cost_void', (d['b'],))], void=True),
            Call('pcc_matchcostgrad', head + _grad_outs(d['b'], d['n'], d['m'])),
            Call('matchcostgrad', head + _grad_outs(d['b'], d['n'], d['m'], '_void'), void=True),
            Call('pcc_matchcostgrad_scaled', head + ['gc'] + _grad_outs(d['b'], d['n'], d['m'], '_scaled'))]


# n = 1024: one whole slab of the gradient kernel, whose branch-free 16-byte body runs on whole slabs only
_case('matchcost', dict(b=B, n=1024, m=32), _matchcost_build, _matchcost_calls, gate=lambda d: d['n'] % 4 == 0 and d['n'] % 1024 == 0,
      anchor=_matchcost_anchor)


def _match_cost_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    cost, g1, g2 = _backend().MatchCostImplicit(i['p1'], i['p2'], True)
    return {'cost': cost, 'grad1': g1, 'grad2': g2}


def _match_cost_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests.util import check_match_cost

    check_match_cost(oracle, p['p1'], p['p2'], p['cost'], p['grad1'], p['grad2'])


_case('match_cost', dict(b=B, n=64, m=48), _pair_build(9),
      lambda d: [Call('pcc_match_cost', [d['b'], d['n'], d['m'], 'p1', 'p2', None, Out('cost', (d['b'],))] + _grad_outs(d['b'], d['n'], d['m']))],
      op=_match_cost_op, op_inputs=('p1', 'p2'), anchor=_match_cost_anchor)


def _sw_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    cost, cost_p, g1, g2 = _backend().SlicedWasserstein(i['p1'], i['p2'], i['theta'], True, True, True)
    return {'cost': cost, 'cost_p': cost_p, 'grad1': g1, 'grad2': g2}


def _sw_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import sliced_wasserstein_reference as ref

    x, y = ref.lattice_clouds(10, d['b'], d['n'])
    return {'p1': _t(x), 'p2': _t(y), 'theta': _t(ref.dyadic_directions(10, d['p']))}


def _sw_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import sliced_wasserstein_reference as ref

    # the costs are words of the contract; on lattice clouds under dyadic directions (n * p a power of two) every product
    # and partial sum of the gradients is exact, so they are the words of the float64 result
    fwd = ref.Forward(p['p1'], p['p2'], p['theta'])
    assert same_words(p['cost'], fwd.cost) and same_words(p['cost_p'], fwd.cost_p)
    ref.Grad(fwd, p['theta']).check_exact(p['grad1'], p['grad2'])


_case('sliced_wasserstein', dict(b=B, n=64, m=64, p=8), _sw_build,
      lambda d: [Call('pcc_sliced_wasserstein', [d['b'], d['n'], d['p'], 'p1', 'p2', 'theta', Out('cost', (d['b'],)), Out('cost_p', (d['b'], d['p']))]
                      + _grad_outs(d['b'], d['n'], d['m']))],
      op=_sw_op, op_inputs=('p1', 'p2', 'theta'), anchor=_sw_anchor)


def _sinkhorn_inputs(d: dict[str, int]) -> tuple[np.ndarray, np.ndarray, list[float]]:
    """The Gaussian clouds of tests/sinkhorn_reference.py and the default schedule of 8 temperatures for their diameter."""
    from tests import sinkhorn_reference as ref

    x, y = ref.clouds(11, d['b'], d['n'], d['m'])
    return x, y, ref.schedule(8, ref.diameter(x, y))


def _sinkhorn_build(d: dict[str, int]) -> dict[str, Any]:
    x, y, _ = _sinkhorn_inputs(d)
    return {'p1': _t(x), 'p2': _t(y)}


def _sinkhorn_op(d: dict[str, int]) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        cost, p1, p2, g1, g2 = _backend().Sinkhorn(i['p1'], i['p2'], _sinkhorn_inputs(d)[2], True, True, True, True)
        return {'cost': cost, 'pot1': p1, 'pot2': p2, 'grad1': g1, 'grad2': g2}
    return op


def _sinkhorn_calls(d: dict[str, int]) -> list[Call]:
    eps = _sinkhorn_inputs(d)[2]
    sched = (ctypes.c_float * len(eps))(*eps)  # host memory, read before the call returns
    return [Call('pcc_sinkhorn', [d['b'], d['n'], d['m'], 'p1', 'p2', len(eps), ctypes.cast(sched, ctypes.c_void_p), 1, Out('cost', (d['b'],)),
                                  Out('pot1', (d['b'], d['n'])), Out('pot2', (d['b'], d['m']))] + _grad_outs(d['b'], d['n'], d['m']))]


def _sinkhorn_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import sinkhorn_reference as ref

    # the dense float64 reference and the bars of the contract (BAR_POT, BAR_COST, BAR_GRAD in their units)
    ref.Result(p['p1'], p['p2'], _sinkhorn_inputs(d)[2]).check(
        {'cost': p['cost'], 'pot_x': p['pot1'], 'pot_y': p['pot2'], 'grad_x': p['grad1'], 'grad_y': p['grad2']}, 'sinkhorn')


_SINKHORN_DIMS = dict(b=B, n=64, m=48)
_case('sinkhorn', _SINKHORN_DIMS, _sinkhorn_build, _sinkhorn_calls, op=_sinkhorn_op(_SINKHORN_DIMS), op_inputs=('p1', 'p2'), anchor=_sinkhorn_anchor)


# ---- searches and samplers (include/pcc_neighbour.h) -------------------------------------------------------------------------

def _knn_build(seed: int) -> Callable[[dict[str, int]], dict[str, Any]]:
    def build(d: dict[str, int]) -> dict[str, Any]:
        rng = _rng(seed)
        # lattice coordinates: the squared distances of either form are exact in float32, so a float64 brute force knows them
        return {'x': _lattice(rng, d['b'], d['c'], d['n']), 'q': _lattice(rng, d['b'], d['c'], d['nq'])}
    return build


def _knn_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    want = oracle.knn_diff(p['x'], d['k']) if d['c'] <= 3 else oracle.knn_expanded(p['x'], d['k'])
    assert same_words(p['indices'], want)


def _knn_op(k: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    return lambda i: {'indices': _ops().knn(i['x'], k)}


for _c in (3, 8):  # the sorted difference-form search and the MFMA search
    _case(f'knn_c{_c}', dict(b=B, c=_c, n=64, nq=48, k=4), _knn_build(12 + _c),
          lambda d: [Call('pcc_knn', [d['b'], d['c'], d['n'], d['k'], 'x', Out('indices', (d['b'], d['n'], d['k']), I64)])],
          op=_knn_op(4), op_inputs=('x',), anchor=_knn_anchor)


def _knn_cross_op(k: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        idx, dist = _ops().knn_cross(i['q'], i['x'], k, return_distance=True)
        return {'indices': idx, 'dist': dist}
    return op


def _knn_cross_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    # queries that are the candidates themselves: knn_cross(x, x, k) is knn(x, k), which the oracle has
    want = oracle.knn_diff(p['x'], d['k']) if d['c'] <= 3 else oracle.knn_expanded(p['x'], d['k'])
    assert same_words(p['self_indices'], want)
    # q against x: the exact distances in float64, the k smallest by (distance, index) -- the contract's order
    dm = ((p['q'].astype(np.float64)[:, :, :, None] - p['x'].astype(np.float64)[:, :, None, :]) ** 2).sum(1)  # [b, nq, n]
    order = np.argsort(dm, axis=2, kind='stable')[:, :, :d['k']]
    assert same_words(p['indices'], order.astype(np.int64))
    assert same_words(p['dist'], np.take_along_axis(dm, order, 2).astype(np.float32))


for _c in (3, 8):
    _case(f'knn_cross_c{_c}', dict(b=B, c=_c, n=64, nq=48, k=4), _knn_build(20 + _c),
          lambda d: [Call('pcc_knn_cross', [d['b'], d['c'], d['nq'], d['n'], d['k'], 'q', 'x', Out('indices', (d['b'], d['nq'], d['k']), I64),
                                            Out('dist', (d['b'], d['nq'], d['k']))]),
                     Call('pcc_knn_cross', [d['b'], d['c'], d['n'], d['n'], d['k'], 'x', 'x', Out('self_indices', (d['b'], d['n'], d['k']), I64), None])],
          op=_knn_cross_op(4), op_inputs=('q', 'x'), anchor=_knn_cross_anchor)


def _sample_build(d: dict[str, int]) -> dict[str, Any]:
    rng = _rng(30)
    return {'xyz': _lattice(rng, d['b'], d['n'], 3), 'centres': _lattice(rng, d['b'], d['m'], 3), 'start': _t([3, 0], np.int32)}


def _fps_op(m: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        idx, dist = _ops().farthest_point_sample(i['xyz'], m, i['start'], return_distance=True)
        return {'idx': idx, 'dist': dist}
    return op


def _cpu_anchor(op: Callable[[dict[str, Any]], dict[str, torch.Tensor]], names: tuple[str, ...], aliases: dict[str, str] | None = None) -> Any:
    """The aligned result against the op's CPU path, word for word, for the outputs of which the op's contract says that the
    two agree so (``aliases``: pool name -> the op's name, for the outputs of a forced path)."""
    def anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
        want = op({k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in p.items()})
        for name in names:
            assert same_words(p[name], want[(aliases or {}).get(name, name)]), name
    return anchor


# lattice coordinates: every squared distance is exact, so the CPU loop's words are the kernel's whatever it contracts
_case('fps', dict(b=B, n=64, m=8), _sample_build,
      lambda d: [Call('pcc_fps', [d['b'], d['n'], d['m'], 'xyz', 'start', Out('idx', (d['b'], d['m']), I64), Out('dist', (d['b'], d['m']))])],
      op=_fps_op(8), op_inputs=('xyz', 'start'), cpu=True, anchor=_cpu_anchor(_fps_op(8), ('idx', 'dist')))


def _ball_op(nsample: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        idx, cnt = _ops().ball_query(i['xyz'], i['centres'], 0.3, nsample, pad='none', return_count=True)
        return {'idx': idx, 'cnt': cnt}
    return op


_case('ball_query', dict(b=B, n=64, m=8, k=4), _sample_build,
      lambda d: [Call('pcc_ball_query', [d['b'], d['n'], d['m'], d['k'], float(np.float32(0.3)), 1, 'xyz', 'centres', Out('idx', (d['b'], d['m'], d['k']), I64),
                                         Out('cnt', (d['b'], d['m']), I32)])],
      op=_ball_op(4), op_inputs=('xyz', 'centres'), cpu=True, anchor=_cpu_anchor(_ball_op(4), ('idx', 'cnt')))


# ---- grouping: group_fwd_kernel's gate, grouping.hip (m * k % 4 == 0, idx and out aligned) --------------------------------------

GROUP_PATHS = (0, 1, 2)  # the product's choice, the LDS path, the direct path


def _group_build(pm: bool, centre: bool) -> Callable[[dict[str, int]], dict[str, Any]]:
    def build(d: dict[str, int]) -> dict[str, Any]:
        rng = _rng(40 + 2 * pm + centre)
        b, c, n, m, k = (d[s] for s in 'bcnmk')
        lay = (lambda a: a.transpose(1, 2).contiguous()) if pm else (lambda a: a)
        return {'x': lay(_ints(rng, b, c, n)), 'centre': lay(_ints(rng, b, c, m)) if centre else None, 'idx': _list(rng, b, m, k, n),
                'g': _ints(rng, b, c, m, k)}
    return build


def _group_calls(pm: bool, centre: bool) -> Callable[[dict[str, int]], list[Call]]:
    def calls(d: dict[str, int]) -> list[Call]:
        b, c, n, m, k = (d[s] for s in 'bcnmk')
        out = []
        for path in GROUP_PATHS:
            tune = ('group_path', path) if path else None
            out.append(Call('pcc_group_points', [b, c, n, m, k, int(pm), 'x', 'idx', 'centre', Out(f'out{path}', (b, c, m, k)), c, 0], tune))
            out.append(Call('pcc_group_points_bwd', [b, c, n, m, k, int(pm), 'idx', 'g', c, 0, Out(f'grad_x{path}', (b, n, c) if pm else (b, c, n)),
                                                     Out(f'grad_centre{path}', (b, m, c) if pm else (b, c, m)) if centre else None], tune))
        return out
    return calls


def _group_op(pm: bool) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        x, centre = _leaf(i['x']), _leaf(i['centre'])
        out = _ops().group_points(x, i['idx'], centre, pm)
        out.backward(i['g'])
        return {'out0': out.detach(), 'grad_x0': x.grad, **({} if centre is None else {'grad_centre0': centre.grad})}
    return op


def _group_anchor(pm: bool, centre: bool) -> Any:
    def anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
        from tests import grouping_reference as ref

        cm = (lambda a: np.ascontiguousarray(a.transpose(0, 2, 1))) if pm else (lambda a: a)
        want = ref.forward(cm(p['x']), p['idx'], cm(p['centre']) if centre else None)
        back = ref.Backward(p['idx'], p['g'], d['n'])  # float64 of integers: exact
        for path in GROUP_PATHS:
            assert same_words(p[f'out{path}'], want), path
            assert np.array_equal(cm(p[f'grad_x{path}']).astype(np.float64), back.gx), path
            if centre:
                assert np.array_equal(cm(p[f'grad_centre{path}']).astype(np.float64), back.gc), path
    return anchor


for _pm in (False, True):
    for _centre in (False, True):
        _case(f"group_points_{'point' if _pm else 'channel'}_major{'_centre' if _centre else ''}", dict(b=B, c=12, n=16, m=12, k=3),
              _group_build(_pm, _centre), _group_calls(_pm, _centre), op=_group_op(_pm), op_inputs=('x', 'centre', 'idx', 'g'), cpu=True,
              gate=lambda d: d['m'] * d['k'] % 4 == 0 and d['k'] % 4 != 0, anchor=_group_anchor(_pm, _centre))


# ---- interpolate: interp_fwd_kernel's gate and the host's thread count, interpolate.hip (m % 4 == 0, out aligned) ----------------

def _interp_build(d: dict[str, int]) -> dict[str, Any]:
    rng = _rng(50)
    b, c, n, m, k = (d[s] for s in 'bcnmk')
    return {'x': _ints(rng, b, c, n), 'idx': _list(rng, b, m, k, n), 'w': _dyadic(rng, b, m, k), 'g': _ints(rng, b, c, m)}


def _interp_calls(d: dict[str, int]) -> list[Call]:
    b, c, n, m, k = (d[s] for s in 'bcnmk')
    out = []
    for path in GROUP_PATHS:
        tune = ('interp_path', path) if path else None
        out.append(Call('pcc_interpolate', [b, c, n, m, k, 'x', 'idx', 'w', Out(f'out{path}', (b, c, m)), c, 0], tune))
        out.append(Call('pcc_interpolate_bwd', [b, c, n, m, k, 'x', 'idx', 'w', 'g', c, 0, Out(f'grad_x{path}', (b, c, n)), Out(f'grad_w{path}', (b, m, k))],
                        tune))
    return out


def _interp_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    x, w = _leaf(i['x']), _leaf(i['w'])
    out = _ops().interpolate_points(x, i['idx'], w)
    out.backward(i['g'])
    return {'out0': out.detach(), 'grad_x0': x.grad, 'grad_w0': w.grad}


def _interp_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import interpolate_reference as ref

    want, want_gw = ref.forward(p['x'], p['idx'], p['w']), ref.grad_w(p['x'], p['idx'], p['g'])
    want_gx = ref.GradX(p['idx'], p['w'], p['g'], d['n']).gx  # float64 of dyadic products: exact
    for path in GROUP_PATHS:
        assert same_words(p[f'out{path}'], want) and same_words(p[f'grad_w{path}'], want_gw), path
        assert np.array_equal(p[f'grad_x{path}'].astype(np.float64), want_gx), path


_case('interpolate', dict(b=B, c=12, n=16, m=12, k=3), _interp_build, _interp_calls, op=_interp_op, op_inputs=('x', 'idx', 'w', 'g'), cpu=True,
      gate=lambda d: d['m'] % 4 == 0, anchor=_interp_anchor)


# ---- attention ------------------------------------------------------------------------------------------------------------------

def _attn_build(d: dict[str, int]) -> dict[str, Any]:
    rng = _rng(60)
    b, c, g, n, m, k = (d[s] for s in 'bcgnmk')
    return {'x': _ints(rng, b, c, n), 'idx': _list(rng, b, m, k, n), 'logits': _ints(rng, b, g, m, k), 'w': _dyadic(rng, b, g, m, k),
            'rel': _ints(rng, b, c, m, k), 'ga': _ints(rng, b, g, m, k), 'go': _ints(rng, b, c, m)}


def _attn_calls(d: dict[str, int]) -> list[Call]:
    b, c, g, n, m, k = (d[s] for s in 'bcgnmk')
    return [Call('pcc_neighbour_softmax', [b, g, n, m, k, 'idx', 'logits', Out('attn', (b, g, m, k))]),
            Call('pcc_neighbour_softmax_bwd', [b, g, n, m, k, 'idx', 'attn', 'ga', Out('grad_logits', (b, g, m, k))]),
            Call('pcc_aggregate_points', [b, c, g, n, m, k, 'x', 'idx', 'w', 'rel', Out('out', (b, c, m))]),
            Call('pcc_aggregate_points_bwd', [b, c, g, n, m, k, 'x', 'idx', 'w', 'rel', 'go', Out('grad_x', (b, c, n)), Out('grad_w', (b, g, m, k)),
                                              Out('grad_rel', (b, c, m, k))])]


def _attn_op(n: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        ops = _ops()
        logits, x, w, rel = _leaf(i['logits']), _leaf(i['x']), _leaf(i['w']), _leaf(i['rel'])
        attn = ops.neighbour_softmax(logits, i['idx'], n)
        attn.backward(i['ga'])
        out = ops.aggregate_points(x, i['idx'], w, rel)
        out.backward(i['go'])
        return {'attn': attn.detach(), 'grad_logits': logits.grad, 'out': out.detach(), 'grad_x': x.grad, 'grad_w': w.grad, 'grad_rel': rel.grad}
    return op


def _attn_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import attention_reference as ref

    # aggregate_points: the forward, grad_weights and grad_rel agree word for word with the CPU rule; grad_x is a sum of
    # dyadic products, exact in any order
    _cpu_anchor(_attn_op(d['n']), ('out', 'grad_w', 'grad_rel', 'grad_x'))(d, p, oracle)
    # the softmax inside the bar of its contract; its backward is float32 operations in slot order on the saved attn: words
    assert ref.softmax_ratio(p['attn'], p['logits'], p['idx'], d['n']) <= 1.0
    assert same_words(p['grad_logits'], ref.softmax_bwd(p['attn'], p['idx'], d['n'], p['ga']))


_case('attention', dict(b=B, c=12, g=3, n=16, m=12, k=4), _attn_build, _attn_calls, op=_attn_op(16),
      op_inputs=('x', 'idx', 'logits', 'w', 'rel', 'ga', 'go'), cpu=True, anchor=_attn_anchor)


# ---- kernel point convolution ---------------------------------------------------------------------------------------------------

KP_SIGMA = 2.0  # with kpconv_reference.lattice_geometry: every influence is 1, 0.5 or 0 exactly


def _kpconv_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import kpconv_reference as ref

    rng = _rng(70)
    b, c, n, m, k, kp = (d[s] for s in ('b', 'c', 'n', 'm', 'k', 'kp'))
    xyz, centres, kpts = ref.lattice_geometry(70, b, n, m, kp)
    return {'x': _ints(rng, b, c, n), 'xyz': _t(xyz), 'centres': _t(centres), 'idx': _list(rng, b, m, k, n), 'kpts': _t(kpts),
            'g': _ints(rng, b, kp * c, m)}


def _kpconv_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import kpconv_reference as ref

    # lattice geometry and integers: the forward's words are the numpy contract's, and every word the backward adds into a
    # bin and every partial sum is exact, so grad_x is the float64 sum's words in any order
    want, h = ref.kpconv(p['x'], p['xyz'], p['centres'], p['idx'], p['kpts'], KP_SIGMA)
    assert same_words(p['out'], want)
    ref.GradX(p['idx'], ref.slot_words(h, p['g'], d['c']), d['n']).check_exact(p['grad_x'])


def _kpconv_calls(d: dict[str, int]) -> list[Call]:
    b, c, n, m, k, kp = (d[s] for s in ('b', 'c', 'n', 'm', 'k', 'kp'))
    return [Call('pcc_kpconv_aggregate', [b, c, n, m, k, kp, 'xyz', 'centres', 'idx', 'x', 'kpts', KP_SIGMA, Out('out', (b, kp * c, m))]),
            Call('pcc_kpconv_aggregate_bwd', [b, c, n, m, k, kp, 'xyz', 'centres', 'idx', 'kpts', KP_SIGMA, 'g', Out('grad_x', (b, c, n))])]


def _kpconv_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    x = _leaf(i['x'])
    out = _ops().kpconv_aggregate(x, i['xyz'], i['centres'], i['idx'], i['kpts'], KP_SIGMA)
    out.backward(i['g'])
    return {'out': out.detach(), 'grad_x': x.grad}


_case('kpconv', dict(b=B, c=12, n=16, m=12, k=4, kp=5), _kpconv_build, _kpconv_calls, op=_kpconv_op,
      op_inputs=('x', 'xyz', 'centres', 'idx', 'kpts', 'g'), cpu=True, anchor=_kpconv_anchor)


# ---- local geometry: stage's gate, local_geometry.hip (whole rows, the list piece aligned) ---------------------------------------

def _geometry_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import local_geometry_reference as ref

    # integer coordinates, rows of 1, 2, 4 or 8 valid slots, grad_mean a multiple of the row's count: every intermediate
    # of the backward, which adds into a point's bin with LDS atomics, is exact in float32 in any order
    xyz, idx, _, gcov, gmean = ref.exact_backward_inputs(80 + d['k'], *(d[s] for s in 'bnmk'))
    return {'xyz': _t(xyz), 'idx': _t(idx, np.int64), 'gcov': _t(gcov), 'gmean': _t(gmean)}


def _geometry_calls(d: dict[str, int]) -> list[Call]:
    b, n, m, k = (d[s] for s in 'bnmk')
    return [Call('pcc_local_geometry', [b, n, m, k, 'xyz', 'idx', Out('mean', (b, m, 3)), Out('cov', (b, m, 3, 3)), Out('eval', (b, m, 3)),
                                        Out('evec', (b, m, 3, 3)), Out('curv', (b, m))]),
            Call('pcc_local_geometry', [b, n, m, k, 'xyz', 'idx', Out('mean_only', (b, m, 3)), None, None, None, None]),
            Call('pcc_local_covariance_bwd', [b, n, m, k, 'xyz', 'idx', 'mean', 'gcov', 'gmean', Out('grad_xyz', (b, n, 3))])]


def _geometry_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    xyz = _leaf(i['xyz'])
    cov, mean = _ops().local_covariance(xyz, i['idx'], return_mean=True)
    torch.autograd.backward((cov, mean), (i['gcov'], i['gmean']))
    return {'cov': cov.detach(), 'mean': mean.detach(), 'grad_xyz': xyz.grad}


def _geometry_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import local_geometry_reference as ref

    mean, cov = ref.mean_cov(p['xyz'], p['idx'])
    assert same_words(p['mean'], mean) and same_words(p['cov'], cov) and same_words(p['mean_only'], mean)
    ref.EigenBars(p['cov']).check(p['eval'], p['evec'], p['curv'])
    ref.check_conventions(p['cov'], p['eval'], p['evec'], p['curv'])
    ref.GradXyz(p['xyz'], p['idx'], p['mean'], p['gcov'], p['gmean']).check_exact(p['grad_xyz'])


for _k, _m, _n in ((3, 12, 16), (33, 4, 16)):  # rows of one LDS chunk, and rows of two (k > 32: neither chunk is a whole row)
    _case(f'local_geometry_k{_k}', dict(b=B, n=_n, m=_m, k=_k), _geometry_build, _geometry_calls, op=_geometry_op,
          op_inputs=('xyz', 'idx', 'gcov', 'gmean'), cpu=True, gate=lambda d: d['m'] * d['k'] % 2 == 0, anchor=_geometry_anchor)


# ---- voxels: vox_fwd_kernel<4>'s gate and devoxelize backward's LDS flush, voxelize.hip ----------------------------------------

def _voxel_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import voxel_reference as vref

    rng = _rng(90 + d['res'])
    b, c, n, res = (d[s] for s in ('b', 'c', 'n', 'res'))
    xyz = _lattice(rng, b, n, 3, steps=4, reach=res - 1 + 0.25)  # the grid lo = 0, extent = res - 1: inv = 1, dyadic corner weights
    xyz[0, 5, 1] = float('nan')
    cell, order, counts = vref.voxel_index(xyz.numpy(), res, 0.0, res - 1.0)
    return {'xyz': xyz, 'x': _ints(rng, b, c, n), 'cell': _t(cell, np.int32), 'order': _t(order, np.int32),
            'counts': _t(counts.reshape(b, res, res, res), np.int32), 'grid': _ints(rng, b, c, res, res, res), 'gg': _ints(rng, b, c, res, res, res),
            'go': _ints(rng, b, c, n)}


def _voxel_calls(d: dict[str, int]) -> list[Call]:
    b, c, n, res = (d[s] for s in ('b', 'c', 'n', 'res'))
    lo, extent = 0.0, res - 1.0
    return [Call('pcc_voxel_index', [b, n, 'xyz', res, lo, extent, Out('cell_out', (b, n), I32), Out('order_out', (b, n), I32),
                                     Out('counts_out', (b, res, res, res), I32)]),
            Call('pcc_voxelize', [b, c, n, res, 'x', 'cell', 'order', 'counts', Out('grid_out', (b, c, res, res, res))]),
            Call('pcc_voxelize_bwd', [b, c, n, res, 'cell', 'counts', 'gg', Out('grad_x', (b, c, n))]),
            Call('pcc_devoxelize', [b, c, n, res, lo, extent, 'grid', 'xyz', Out('out', (b, c, n))]),
            Call('pcc_devoxelize_bwd', [b, c, n, res, lo, extent, 'xyz', 'go', Out('grad_grid', (b, c, res, res, res))])]


def _voxel_op(res: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        ops = _ops()
        x, grid = _leaf(i['x']), _leaf(i['grid'])
        index = ops.voxel_index(i['xyz'], res, 0.0, res - 1.0)
        vox = ops.voxelize(x, ops.VoxelIndex(i['cell'], i['order'], i['counts']))
        vox.backward(i['gg'])
        out = ops.devoxelize(grid, i['xyz'], 0.0, res - 1.0)
        out.backward(i['go'])
        return {'cell_out': index.cell, 'order_out': index.order, 'counts_out': index.counts, 'grid_out': vox.detach(), 'grad_x': x.grad,
                'out': out.detach(), 'grad_grid': grid.grad}
    return op


def _voxel_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import voxel_reference as vref

    b, c, res = d['b'], d['c'], d['res']
    cell, order, counts = vref.voxel_index(p['xyz'], res, 0.0, res - 1.0)
    assert same_words(p['cell_out'], cell) and same_words(p['order_out'], order) and same_words(p['counts_out'].reshape(b, -1), counts)
    assert same_words(p['grid_out'].reshape(b, c, -1), vref.voxelize(p['x'], cell, counts))
    assert same_words(p['grad_x'], vref.voxelize_bwd(p['gg'].reshape(b, c, -1), cell, counts))
    assert same_words(p['out'], vref.devoxelize(p['grid'].reshape(b, c, -1), p['xyz'], res, 0.0, res - 1.0))
    # grad_grid: float atomics over dyadic weights times integers -- exact in any order, so the CPU autograd's words
    grid = torch.from_numpy(p['grid']).requires_grad_(True)
    _ops().devoxelize(grid, torch.from_numpy(p['xyz']), 0.0, res - 1.0).backward(torch.from_numpy(p['go']))
    assert np.array_equal(p['grad_grid'], grid.grad.numpy())


for _res in (2, 4):
    _case(f'voxel_res{_res}', dict(b=B, c=12, n=32, res=_res), _voxel_build, _voxel_calls, op=_voxel_op(_res),
          op_inputs=('xyz', 'x', 'cell', 'order', 'counts', 'grid', 'gg', 'go'), cpu=True, gate=lambda d: d['res'] ** 3 % 4 == 0, anchor=_voxel_anchor)


# ---- grid pooling: stage_rows peels a head of (4 - a) & 3 words, grid_pool.hip ---------------------------------------------------

POOL_MODES = {'mean': 0, 'sum': 1, 'max': 2}


def _pool_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import grid_pool_reference as gref
    from tests import voxel_reference as vref

    rng = _rng(100)
    b, c, n, m, res = (d[s] for s in ('b', 'c', 'n', 'm', 'res'))
    xyz = _lattice(rng, b, n, 3, steps=1, reach=res)
    xyz[1, 7, 0] = float('inf')
    cell, order, counts = vref.voxel_index(xyz.numpy(), res, 0.0, res - 1.0)
    cluster, seg, count = gref.grid_cluster(cell, order, m)
    ins = {'xyz': xyz, 'x': _ints(rng, b, c, n), 'cell': _t(cell, np.int32), 'order': _t(order, np.int32),
           'counts': _t(counts.reshape(b, res, res, res), np.int32), 'cluster': _t(cluster, np.int32), 'seg': _t(seg, np.int32),
           'count': _t(count, np.int32), 'g': _ints(rng, b, c, m)}
    ins['arg'] = _t(gref.segment_pool(ins['x'].numpy(), order, seg, gref.MAX)[1], np.int32)
    return ins


def _pool_calls(d: dict[str, int]) -> list[Call]:
    b, c, n, m, res = (d[s] for s in ('b', 'c', 'n', 'm', 'res'))
    out = [Call('pcc_grid_cluster', [b, n, m, 'cell', 'order', Out('cluster_out', (b, n), I32), Out('seg_out', (b, m + 1), I32), Out('count_out', (b,), I32)]),
           Call('pcc_cell_neighbours', [b, n, m, res, 3, 1, 'cell', 'order', 'seg', 'count', Out('nbr', (b, m, 27), I64)])]
    for name, mode in POOL_MODES.items():
        is_max = mode == 2
        out.append(Call('pcc_segment_pool', [b, c, n, m, mode, 'x', 'order', 'seg', Out('out_' + name, (b, c, m)),
                                             Out('arg_out', (b, c, m), I32) if is_max else None]))
        out.append(Call('pcc_segment_pool_bwd', [b, c, n, m, mode, 'cluster', 'seg', 'arg' if is_max else None, 'g', Out('grad_' + name, (b, c, n))]))
    return out


def _pool_op(m: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        ops = _ops()
        vindex = ops.VoxelIndex(i['cell'], i['order'], i['counts'])
        gindex = ops.grid_cluster(vindex, m=m)
        res = {'cluster_out': gindex.cluster, 'seg_out': gindex.seg, 'count_out': gindex.count,
               'nbr': ops.cell_neighbours(vindex, ops.GridIndex(i['cluster'], i['seg'], i['count'], i['order'])).nbr}
        for name in POOL_MODES:
            x = _leaf(i['x'])
            out = ops.segment_pool(x, ops.GridIndex(i['cluster'], i['seg'], i['count'], i['order']), name)
            out.backward(i['g'])
            res['out_' + name], res['grad_' + name] = out.detach(), x.grad
        return res
    return op


def _pool_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import grid_pool_reference as gref
    from tests import sparse_conv_reference as sref

    cluster, seg, count = gref.grid_cluster(p['cell'], p['order'], d['m'])
    assert same_words(p['cluster_out'], cluster) and same_words(p['seg_out'], seg) and same_words(p['count_out'], count)
    assert same_words(p['nbr'], sref.cell_neighbours(p['cell'], p['order'], seg, count, d['res'], 3, 1))
    for name, mode in POOL_MODES.items():
        out, arg = gref.segment_pool(p['x'], p['order'], seg, mode)
        assert same_words(p['out_' + name], out), name
        assert same_words(p['grad_' + name], gref.segment_pool_bwd(p['g'], cluster, seg, arg, mode)), name
    assert same_words(p['arg_out'], arg)


# c = 12: the second block of 8 channels starts 8 * n words into the sample
_case('grid_pool', dict(b=B, c=12, n=32, m=12, res=4), _pool_build, _pool_calls, op=_pool_op(12),
      op_inputs=('x', 'cell', 'order', 'counts', 'cluster', 'seg', 'count', 'g'), cpu=True, gate=lambda d: d['n'] % 4 == 0 and d['c'] > 8,
      anchor=_pool_anchor)


# ---- sparse convolution: launch_mfma's choice of the vector-load variant, sparse_conv.hip (o % NOT == 0, weight aligned) ---------

def _conv_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import sparse_conv_reference as sref

    b, c, o, m, taps = (d[s] for s in ('b', 'c', 'o', 'm', 't'))
    rng = _rng(110 + o)
    # a symmetric map (the backward's mirrored call needs one): every cell of a 4^3 grid but the last ones is a slot
    xyz = np.stack([sref.lattice_cloud(4)[0][:m] for _ in range(b)])
    xyz[1] = xyz[1][::-1]
    _, _, nbr = sref.build(xyz, 4, 0.0, 3.0, m, 3, 1)
    assert sref.is_symmetric(nbr)
    x, w, bias = sref.lattice_inputs(o, b, c, o, m, taps)
    return {'x': _t(x), 'nbr': _t(nbr, np.int64), 'weight': _t(w), 'bias': _t(bias), 'g': _ints(rng, b, o, m)}


def _conv_calls(d: dict[str, int]) -> list[Call]:
    b, c, o, m, taps = (d[s] for s in ('b', 'c', 'o', 'm', 't'))
    return [Call('pcc_sparse_conv', [b, c, o, m, m, taps, 'x', 'nbr', 'weight', 'bias', Out('out', (b, o, m))])]


def _conv_op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    ops = _ops()
    x, w, bias = _leaf(i['x']), _leaf(i['weight']), _leaf(i['bias'])
    cmap = ops.SparseConvMap(i['nbr'], torch.zeros(i['nbr'].shape[0], dtype=I32, device=i['nbr'].device), 3, 1)
    out = ops.sparse_conv(x, cmap, w, bias)
    out.backward(i['g'])
    return {'out': out.detach(), 'grad_x': x.grad, 'grad_weight': w.grad, 'grad_bias': bias.grad}


def _conv_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import sparse_conv_reference as sref

    assert sref.kernel_of(d['c'], d['o']).startswith('sparse_conv_mfma' if d['c'] >= 8 else 'sparse_conv_kernel')
    want, _, _ = sref.sparse_conv(p['x'], p['nbr'], p['weight'], p['bias'])
    assert np.array_equal(p['out'].astype(np.float64), want)
    # the op's gradients (integers and dyadic weights: exact in any order): grad_x by the scatter definition, the torch
    # compositions of grad_weight and grad_bias against the float64 sums
    assert np.array_equal(p['grad_x'].astype(np.float64), sref.grad_x_scatter(p['g'], p['nbr'], p['weight'], d['m']))
    gw, gb = sref.grad_weight_bias(p['x'], p['g'], p['nbr'])
    assert np.array_equal(p['grad_weight'].astype(np.float64), gw) and np.array_equal(p['grad_bias'].astype(np.float64), gb)


def _not_of(o: int) -> int:
    return 1 if o <= 16 else 2 if o <= 32 else 4


def _conv_probe(d: dict[str, int], pool: dict[str, Any], dev: torch.device) -> None:
    """Which variant of the MFMA kernel ran, from the launch profile: the vector loads of NOT weights exactly when weight
    starts on a 4 * NOT-byte boundary, the scalar loads otherwise -- the address term of launch_mfma's gate itself, which
    equal words alone would not pin if the hardware tolerates the misaligned load."""
    from pointcloudcounterfactual_amd import _lib
    from tests import sparse_conv_reference as sref

    name, call = sref.kernel_of(d['c'], d['o']), _conv_calls(d)[0]
    for elements in (0, 1, 2, 3):
        for shift in ({'weight': elements}, {'weight': elements, 'x': 1, 'nbr': 1, 'bias': 1, 'out': 1}):
            with _lib.profile() as read:
                run_call(call, pool, dev, shift)
                ran, scalar = read(name)[1], read(name + ' scalar weights')[1]
            assert (ran, scalar) == (1, int(4 * elements % (4 * _not_of(d['o'])) != 0)), (shift, ran, scalar)


for _c, _o in ((8, 16), (8, 32), (8, 64), (5, 9)):  # NOT = 1, 2, 4 of the MFMA kernel, and the VALU kernel
    _case(f'sparse_conv_c{_c}_o{_o}', dict(b=B, c=_c, o=_o, m=33, t=27), _conv_build, _conv_calls, op=_conv_op,
          op_inputs=('x', 'nbr', 'weight', 'bias', 'g'), cpu=True,
          gate=(lambda d: d['c'] >= 8 and d['o'] >= 16 and d['o'] % _not_of(d['o']) == 0) if _c >= 8 else None, anchor=_conv_anchor,
          probe=_conv_probe if _c >= 8 else None)


# ---- graph ops: graph_ops.hip's gates (n * k % 4 == 0 and k >= 4, n % 4 == 0) -----------------------------------------------------

def _graph_build(d: dict[str, int]) -> dict[str, Any]:
    rng = _rng(120)
    b, c, n, k = (d[s] for s in 'bcnk')
    x = _ints(rng, b, c, n)
    idx = _t(rng.integers(0, n, size=(b, n, k)), np.int64)
    nb = torch.gather(x, 2, idx.view(b, 1, n * k).expand(-1, c, -1)).view(b, c, n, k)
    first_max = (nb == nb.max(3, keepdim=True)[0]).to(I32).argmax(3)  # the winning slot j: the first of equal maxima
    return {'x': x, 'idx': idx, 'arg': first_max.to(I32), 'g4': _ints(rng, b, c, n, k), 'g8': _ints(rng, b, 2 * c, n, k), 'g3': _ints(rng, b, c, n)}


def _graph_calls(d: dict[str, int]) -> list[Call]:
    b, c, n, k = (d[s] for s in 'bcnk')
    head = [b, c, n, k]
    return [Call('pcc_gather_neighbours', head + ['x', 'idx', Out('gathered', (b, c, n, k))]),
            Call('pcc_gather_neighbours_bwd', head + ['idx', 'g4', Out('gathered_gx', (b, c, n))]),
            Call('pcc_graph_features', head + ['x', 'idx', Out('features', (b, 2 * c, n, k))]),
            Call('pcc_graph_features_bwd', head + ['idx', 'g8', Out('features_gx', (b, c, n))]),
            Call('pcc_graph_max_pool', head + ['x', 'idx', Out('pooled', (b, c, n)), Out('arg_out', (b, c, n), I32)]),
            Call('pcc_graph_max_pool_bwd', head + ['idx', 'arg_out', 'g3', Out('pooled_gx', (b, c, n))]),
            Call('pcc_neighbour_sum', head + ['x', 'idx', Out('summed', (b, c, n))]),
            Call('pcc_neighbour_sum_bwd', head + ['idx', 'g3', Out('summed_gx', (b, c, n))]),
            Call('pcc_neighbour_minmax_target', head + ['x', 'idx', Out('tsel', (b, 2, c, n), I64)]),
            Call('pcc_global_pool', [b, c, n, 'x', Out('gmax', (b, c)), Out('garg', (b, c), I32), Out('gmean', (b, c))])]


def _graph_op(k: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        from pointcloudcounterfactual_amd import edgeconv

        ops, res = _ops(), {}
        for name, fn, g in (('gathered', lambda t: ops.get_neighbours(t, i['idx'], k)[1], 'g4'),
                            ('features', lambda t: ops.get_graph_features(t, i['idx'], k)[1], 'g8'),
                            ('pooled', lambda t: ops.graph_max_pooling(t, i['idx'], k), 'g3'),
                            ('summed', lambda t: edgeconv.neighbour_sum(t, i['idx']), 'g3')):
            x = _leaf(i['x'])
            out = fn(x)
            out.backward(i[g])
            res[name], res[name + '_gx'] = out.detach(), x.grad
        res['gmax'] = ops.global_max_pool(i['x'])
        return res
    return op


def _graph_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    # integers: the CPU compositions are exact, whatever order either side adds in (max-pool's ties: equal values, equal sums)
    _cpu_anchor(_graph_op(d['k']), ('gathered', 'features', 'pooled', 'summed', 'gathered_gx', 'features_gx', 'summed_gx', 'gmax'))(d, p, oracle)
    x = p['x']
    assert same_words(p['arg_out'], p['arg'])
    assert np.array_equal(p['garg'], x.argmax(2)) and np.array_equal(p['gmean'].astype(np.float64), x.astype(np.float64).sum(2) / d['n'])
    want = np.zeros_like(x)
    winner = np.take_along_axis(np.broadcast_to(p['idx'][:, None], (d['b'], d['c'], d['n'], d['k'])), p['arg'][..., None].astype(np.int64), 3)[..., 0]
    np.add.at(want, (np.arange(d['b'])[:, None, None], np.arange(d['c'])[None, :, None], winner), p['g3'])
    assert np.array_equal(p['pooled_gx'], want)
    from tests import edgeconv_reference as eref

    assert same_words(p['tsel'], eref.minmax_target_reference(torch.from_numpy(x), torch.from_numpy(p['idx'])))


# n / 64 and the sum of n integers in [-4, 4] are exact: the mean is too
_case('graph_ops', dict(b=B, c=12, n=64, k=4), _graph_build, _graph_calls, op=_graph_op(4), op_inputs=('x', 'idx', 'g4', 'g8', 'g3'), cpu=True,
      gate=lambda d: d['n'] * d['k'] % 4 == 0 and d['k'] >= 4 and d['n'] % 4 == 0, anchor=_graph_anchor)


# ---- pairwise reductions ------------------------------------------------------------------------------------------------------------

def _pairwise_build(d: dict[str, int]) -> dict[str, Any]:
    rng = _rng(130)
    return {'p': _lattice(rng, d['b'], d['n'], d['d']), 'q': _lattice(rng, d['b'], d['m'], d['d']), 'g': _ints(rng, d['b'], d['n'])}


def _pairwise_calls(d: dict[str, int]) -> list[Call]:
    b, n, m, dim = d['b'], d['n'], d['m'], d['d']
    return [Call('pcc_pair_argmin', [b, n, m, dim, 'p', 'q', Out('idx', (b, n), I64), Out('val', (b, n))]),
            Call('pcc_pair_sqdist_sum', [b, n, m, dim, 'p', 'q', Out('sum', (b, n))]),
            Call('pcc_pair_sqdist_sum_bwd', [b, n, m, dim, 'p', 'q', 'g', Out('grad_p', (b, n, dim)), Out('grad_q', (b, m, dim))])]


def _pairwise_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    # lattice coordinates in [0, 1) and integer gradients: every distance, sum and gradient is exact in float32
    pp, q, g = (p[k].astype(np.float64) for k in ('p', 'q', 'g'))
    diff = pp[:, :, None, :] - q[:, None, :, :]
    dm = (diff ** 2).sum(-1)
    assert np.array_equal(p['idx'], dm.argmin(2)) and np.array_equal(p['val'], dm.min(2)) and np.array_equal(p['sum'], dm.sum(2))
    assert np.array_equal(p['grad_p'], (2 * g[:, :, None, None] * diff).sum(2)) and np.array_equal(p['grad_q'], (-2 * g[:, :, None, None] * diff).sum(1))


_case('pairwise', dict(b=B, n=64, m=48, d=4), _pairwise_build, _pairwise_calls, anchor=_pairwise_anchor)


# ---- BatchNorm + ReLU + residual: bnact.hip's gates (n % 4 == 0, every base aligned) ---------------------------------------------

BN_EPS = 1e-5


def _bn_build(d: dict[str, int]) -> dict[str, Any]:
    from tests import bn_pair_reference as R

    inp = R.bn_inputs(d['b'], d['c'], d['n'], (1, d['c']), 'exact', 140)
    return {k: inp[k] for k in ('z', 'gamma', 'beta', 'res', 'gy', 'mean', 'var')}


def _bn_calls(d: dict[str, int]) -> list[Call]:
    b, c, n = d['b'], d['c'], d['n']
    return [Call('pcc_bn_stats', [b, c, n, 'z', Out('mean_out', (c,)), Out('var_out', (c,))]),
            Call('pcc_bn_relu_res_fwd', [b, c, n, 'z', 'mean', 'var', BN_EPS, 'gamma', 'beta', 'res', c, 1, Out('y', (b, c, n))]),
            Call('pcc_bn_relu_bwd', [b, c, n, 'z', 'mean', 'var', BN_EPS, 'gamma', 'beta', 'gy', 0, Out('dz', (b, c, n)), Out('dgamma', (c,)), Out('dbeta', (c,))]),
            Call('pcc_bn_relu_bwd', [b, c, n, 'z', 'mean', 'var', BN_EPS, 'gamma', 'beta', 'gy', 1, Out('dz_train', (b, c, n)), Out('dgamma_train', (c,)),
                                     Out('dbeta_train', (c,))])]


def _bn_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import bn_pair_reference as R

    t = {k: torch.from_numpy(v) for k, v in p.items() if k in ('z', 'gamma', 'beta', 'res', 'gy', 'mean', 'var')}
    mean, var, bound_mean, bound_var = R.bn_stats_ref(t['z'])
    R.assert_close('mean', torch.from_numpy(p['mean_out']), mean, bound_mean)
    R.assert_close('var', torch.from_numpy(p['var_out']), var, bound_var)
    y, bound, _, _ = R.bn_fwd_ref(t['z'], t['mean'], t['var'], BN_EPS, t['gamma'], t['beta'], t['res'], 1)
    R.assert_close('y', torch.from_numpy(p['y']), y, bound)
    for tag, training in (('', False), ('_train', True)):
        ref = R.bn_bwd_ref(t['z'], t['mean'], t['var'], BN_EPS, t['gamma'], t['beta'], t['gy'], training)
        for name, key in (('dz', 'grad_z'), ('dgamma', 'grad_gamma'), ('dbeta', 'grad_beta')):
            R.assert_close(name + tag, torch.from_numpy(p[name + tag]), *ref[key])


_case('bn_relu', dict(b=B, c=16, n=256), _bn_build, _bn_calls, gate=lambda d: d['n'] % 4 == 0, anchor=_bn_anchor)


# ---- the auction (include/pcc_emd.h) ------------------------------------------------------------------------------------------------

def _auction_build(d: dict[str, int]) -> dict[str, Any]:
    rng = _rng(150)
    b, n = d['b'], d['n']
    xyz1, xyz2 = _cloud(rng, b, n, 3), _cloud(rng, b, n, 3)
    return {'xyz1': xyz1, 'xyz2': xyz2, 'gd': _ints(rng, b, n), 'assignment': _t(np.stack([rng.permutation(n) for _ in range(b)]), np.int32)}


def _auction_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    dist, ass, _, _ = oracle.auction_forward_ext(p['xyz1'], p['xyz2'], 0.005, 50)
    assert np.array_equal(p['ass_out'], ass) and same_words(p['dist'], dist)  # (as tests/test_gpu_auction_schedules.py)
    assert same_words(p['grad_xyz1'], oracle.auction_backward(p['xyz1'], p['xyz2'], p['gd'], p['assignment']))


_case('auction', dict(b=B, n=64), _auction_build,
      lambda d: [Call('pcc_auction_forward', [d['b'], d['n'], 'xyz1', 'xyz2', 0.005, 50, Out('dist', (d['b'], d['n'])), Out('ass_out', (d['b'], d['n']), I32)]),
                 Call('pcc_auction_backward', [d['b'], d['n'], 'xyz1', 'xyz2', 'gd', 'assignment', Out('grad_xyz1', (d['b'], d['n'], 3))])],
      anchor=_auction_anchor)


def covered() -> set[str]:
    return set().union(*(case.symbols() for case in CASES))
