"""The case of ``pcc_grid_cluster_ragged`` in the registry of tests/unaligned_views.py, kept in a module of its own: importing it
appends the case to ``unaligned_views.CASES`` (once), exactly as tests/unaligned_views_ragged.py does for the ragged searches, so
that tests/test_unaligned_views_host.py and tests/test_gpu_unaligned_views.py, unchanged, take it like every other case.

Every file that reads the registry (tests/test_unaligned_views_host.py, tests/test_gpu_unaligned_views.py,
tests/stream_order.py) imports this module, so the case is there however a file is run.

Lattice coordinates k/16 on a dyadic grid of 1/8 from the origin (every quotient exact); two clouds of unequal size; b = 2 and every
dimension <= 512 as the registry asks; one call at a capacity below the number of occupied cells (ranks dropped) and one at
capacity n (padded slots); the anchor is tests/grid_ragged_reference.py."""

from __future__ import annotations

from typing import Any

import numpy as np
import torch

from tests import unaligned_views as U
from tests.unaligned_views import I32, Call, Out, same_words

SIZE = 0.125
OUTS = ('cluster', 'order', 'seg', 'coord', 'new_offset', 'n_cells')


def _build(d: dict[str, int]) -> dict[str, Any]:
    rng = U._rng(170)
    n = d['n']
    xyz = U._lattice(rng, n, 3)
    xyz[5, 1] = float('nan')
    xyz[n - 1, 0] = -0.5  # below the start
    return {'xyz': xyz, 'offset': U._t([n // 4 + 3, n], np.int32), 'start': U._t(np.zeros((d['b'], 3))), 'features': U._ints(rng, n, d['c']),
            'g': U._ints(rng, d['m'], d['c'])}


def _outs(n: int, m: int, b: int, tag: str) -> list[Out]:
    shapes = {'cluster': (n,), 'order': (n,), 'seg': (m + 1,), 'coord': (m, 4), 'new_offset': (b,), 'n_cells': (1,)}
    return [Out(name + tag, shapes[name], I32) for name in OUTS]


def _calls(d: dict[str, int]) -> list[Call]:
    b, n, m, ab = d['b'], d['n'], d['m'], d['axis_bits']
    return [Call('pcc_grid_cluster_ragged', [b, n, m, ab, 'xyz', 'offset', 'start', SIZE] + _outs(n, m, b, '')),
            Call('pcc_grid_cluster_ragged', [b, n, n, ab, 'xyz', 'offset', 'start', SIZE] + _outs(n, n, b, '_full'))]


def _op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    ops = U._ops()
    d = CASE_DIMS
    feats = U._leaf(i['features'])
    pooled = ops.grid_pool_ragged(i['xyz'], feats, i['offset'], SIZE, 'mean', start=i['start'], m=d['m'], axis_bits=d['axis_bits'])
    pooled.features.backward(i['g'])
    index = pooled.grid.index
    return {'cluster': index.cluster[0], 'order': index.order[0], 'seg': index.seg[0], 'coord': pooled.grid.coord, 'new_offset': pooled.offset,
            'n_cells': pooled.grid.count, 'centres': pooled.xyz, 'pooled': pooled.features.detach(), 'grad': feats.grad}


def _anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import grid_ragged_reference as G

    full = G.grid_cluster(p['xyz'], p['offset'], p['start'], SIZE, d['n'], d['axis_bits'])
    want = G.cut(full, d['m'])
    assert d['m'] < int(full['n_cells'][0]) < d['n']  # the first call drops ranks, the second pads
    for name in OUTS:
        assert same_words(p[name], want[name]), name
        assert same_words(p[name + '_full'], full[name]), name
    if 'pooled' in p:  # (the Python op ran: exact sums of small integers over lattice points)
        order, seg = want['order'].astype(np.int64), want['seg'].astype(np.int64)
        for r in range(d['m']):
            run = order[seg[r]:seg[r + 1]]
            assert same_words(p['pooled'][r], (p['features'][run].astype(np.float64).sum(0) / len(run)).astype(np.float32))
            assert same_words(p['centres'][r], (p['xyz'][run].astype(np.float64).sum(0) / len(run)).astype(np.float32))
            assert same_words(p['grad'][run], np.broadcast_to((p['g'][r].astype(np.float64) / len(run)).astype(np.float32), (len(run), d['c'])))
        assert not p['grad'][want['cluster'] < 0].any()


CASE_DIMS = dict(b=U.B, n=96, m=40, c=4, axis_bits=4)

if not any(case.name == 'grid_cluster_ragged' for case in U.CASES):
    U._case('grid_cluster_ragged', CASE_DIMS, _build, _calls, op=_op, op_inputs=('xyz', 'offset', 'start', 'features', 'g'), cpu=True,
            anchor=_anchor)
