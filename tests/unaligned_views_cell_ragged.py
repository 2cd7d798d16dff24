"""The case of ``pcc_cell_neighbours_ragged`` in the registry of tests/unaligned_views.py, kept in a module of its own: importing it
appends the case to ``unaligned_views.CASES`` (once), exactly as tests/unaligned_views_grid_ragged.py does for the ragged grid index,
so that tests/test_unaligned_views_host.py and tests/test_gpu_unaligned_views.py, unchanged, take it like every other case.

Every file that reads the registry (tests/test_unaligned_views_host.py, tests/test_gpu_unaligned_views.py,
tests/stream_order.py) imports this module, so the case is there however a file is run.

``coord`` 4, 8 and 12 bytes off a 16-byte boundary takes the kernel's four dword loads per row, on the boundary its one 16-byte load;
``nbr`` 8 bytes off.  A scene of 280 cells in two clouds (more than one workgroup) at capacity 300 (padded slots) for K = 3, and at
capacity 200 with the count left at 280 (ranks dropped) for K = 5, dilation 2; the anchor is tests/cell_ragged_reference.py."""

from __future__ import annotations

from typing import Any

import numpy as np
import torch

from tests import unaligned_views as U
from tests.unaligned_views import I32, I64, Call, Out, same_words


def _build(d: dict[str, int]) -> dict[str, Any]:
    from tests import cell_ragged_reference as C

    coord, u = C.padded(C.scene(d['cells'], seed=180), d['m'])
    return {'coord': U._t(coord, np.int32), 'n_cells': U._t([u], np.int32)}


def _calls(d: dict[str, int]) -> list[Call]:
    return [Call('pcc_cell_neighbours_ragged', [d['m'], 3, 1, 'coord', 'n_cells', Out('nbr', (d['m'], 27), I64)]),
            Call('pcc_cell_neighbours_ragged', [d['cut'], 5, 2, 'coord', 'n_cells', Out('nbr5', (d['cut'], 125), I64)])]


def _grid(coord: torch.Tensor, count: torch.Tensor) -> Any:
    """A ``RaggedGrid`` around ``coord`` and ``count``: the map reads nothing else of it."""
    ops = U._ops()
    none = torch.zeros((1, 1), dtype=I32, device=coord.device)
    seg = torch.zeros((1, coord.shape[0] + 1), dtype=I32, device=coord.device)
    return ops.RaggedGrid(ops.GridIndex(none, seg, count, none), coord, count, count)


def _op(i: dict[str, Any]) -> dict[str, torch.Tensor]:
    ops = U._ops()
    d = CASE_DIMS
    full = ops.cell_neighbours_ragged(_grid(i['coord'], i['n_cells']), 3, 1)
    part = ops.cell_neighbours_ragged(_grid(i['coord'][:d['cut']], i['n_cells']), 5, 2)
    assert full.nbr.shape == (1, d['m'], 27) and part.nbr.shape == (1, d['cut'], 125) and full.count is i['n_cells']
    return {'nbr': full.nbr[0], 'nbr5': part.nbr[0]}


def _anchor(d: dict[str, int], p: dict[str, np.ndarray], oracle: Any) -> None:
    from tests import cell_ragged_reference as C

    u = int(p['n_cells'][0])
    assert d['cut'] < u == d['cells'] < d['m']  # the second call drops ranks, the first pads
    assert same_words(p['nbr'], C.cell_map(p['coord'], u, 3, 1))
    assert same_words(p['nbr5'], C.cut(C.cell_map(p['coord'], u, 5, 2), d['cut']))
    C.check_properties(p['nbr'], u, 3)
    C.check_properties(p['nbr5'], d['cut'], 5)


CASE_DIMS = dict(b=U.B, m=300, cells=280, cut=200)

if not any(case.name == 'cell_neighbours_ragged' for case in U.CASES):
    U._case('cell_neighbours_ragged', CASE_DIMS, _build, _calls, op=_op, op_inputs=('coord', 'n_cells'), cpu=True, anchor=_anchor)
