"""The cases of the two ragged entry points (``pcc_knn_ragged``, ``pcc_ball_query_ragged``) in the registry of
tests/unaligned_views.py, kept in a module of their own: importing it appends them to ``unaligned_views.CASES`` (once), so that
tests/test_unaligned_views_host.py and tests/test_gpu_unaligned_views.py, unchanged, take them like every other case -- the
coverage check against ``_lib.ABI``, the shape check, the CPU paths on shifted views, and on the accelerator every tensor argument
4, 8 and 12 bytes off a 16-byte boundary against the aligned call.

The registry is a module-level list that the registry suites read when they are collected.  Every file that reads it
(tests/test_unaligned_views_host.py, tests/test_gpu_unaligned_views.py, tests/stream_order.py) imports this module, so the
cases are there however a file is run.

Lattice coordinates (exact distances, ties everywhere); two clouds of unequal size, the second longer than a query tile; b = 2 and
every dimension <= 512 as the registry asks; each case's anchor is tests/ragged_reference.py."""

from __future__ import annotations

from typing import Any, Callable

import numpy as np
import torch

from tests import unaligned_views as U
from tests.unaligned_views import I32, I64, Call, Out, same_words


def _ragged_build(d: dict[str, int]) -> dict[str, Any]:
    rng = U._rng(160)
    n, m = d['n'], d['m']
    return {'xyz': U._lattice(rng, n, 3), 'query': U._lattice(rng, m, 3), 'offset': U._t([n // 4 + 3, n], np.int32),
            'query_offset': U._t([m // 4 + 1, m], np.int32)}


def _knn_ragged_op(k: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        idx, dist = U._ops().knn_ragged(i['xyz'], i['offset'], k, i['query'], i['query_offset'], return_distance=True)
        return {'idx': idx, 'dist': dist}
    return op


def _knn_ragged_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import ragged_reference as R

    want = R.knn(oracle, p['xyz'], p['offset'], p['query'], p['query_offset'], d['k'])
    assert same_words(p['idx'], want) and (want >= 0).all()
    d64 = ((p['xyz'][want].astype(np.float64) - p['query'][:, None].astype(np.float64)) ** 2).sum(-1)  # exact on the lattice
    assert same_words(p['dist'], d64.astype(np.float32))
    assert same_words(p['self_idx'], R.knn(oracle, p['xyz'], p['offset'], k=d['k']))


def _ball_ragged_op(nsample: int) -> Callable[[dict[str, Any]], dict[str, torch.Tensor]]:
    def op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
        idx, cnt = U._ops().ball_query_ragged(i['xyz'], i['offset'], i['query'], i['query_offset'], 0.3, nsample, pad='none', return_count=True)
        return {'idx': idx, 'cnt': cnt}
    return op


def _ball_ragged_anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import ragged_reference as R

    ref = R.RaggedBall(p['xyz'], p['offset'], p['query'], p['query_offset'])
    ref.check_exact(float(np.float32(0.3)), d['k'], 'none', p['idx'], p['cnt'])
    ref.check_exact(float(np.float32(0.3)), d['k'], 'first', p['idx_first'], p['cnt'])


NAMES = ('knn_ragged', 'ball_query_ragged')

if not any(case.name in NAMES for case in U.CASES):
    U._case('knn_ragged', dict(b=U.B, n=96, m=80, k=4), _ragged_build,
            lambda d: [Call('pcc_knn_ragged', [d['b'], d['n'], d['m'], d['k'], 'xyz', 'offset', 'query', 'query_offset',
                                               Out('idx', (d['m'], d['k']), I64), Out('dist', (d['m'], d['k']))]),
                       Call('pcc_knn_ragged', [d['b'], d['n'], d['n'], d['k'], 'xyz', 'offset', 'xyz', 'offset',
                                               Out('self_idx', (d['n'], d['k']), I64), None])],
            op=_knn_ragged_op(4), op_inputs=('xyz', 'offset', 'query', 'query_offset'), cpu=True, anchor=_knn_ragged_anchor)
    U._case('ball_query_ragged', dict(b=U.B, n=96, m=80, k=4), _ragged_build,
            lambda d: [Call('pcc_ball_query_ragged', [d['b'], d['n'], d['m'], d['k'], float(np.float32(0.3)), 1, 'xyz', 'offset', 'query',
                                                      'query_offset', Out('idx', (d['m'], d['k']), I64), Out('cnt', (d['m'],), I32)]),
                       Call('pcc_ball_query_ragged', [d['b'], d['n'], d['m'], d['k'], float(np.float32(0.3)), 0, 'xyz', 'offset', 'query',
                                                      'query_offset', Out('idx_first', (d['m'], d['k']), I64), None])],
            op=_ball_ragged_op(4), op_inputs=('xyz', 'offset', 'query', 'query_offset'), cpu=True, anchor=_ball_ragged_anchor)
