"""ctypes binding of ``libpcc_structural.so`` (the C ABI declared in ``include/pcc_structural.h``).

The library is hand-written HIP for gfx950; there is no CPU or PyTorch fallback.  If the shared
object has not been built (``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C pointcloudcounterfactual_amd/csrc``) importing this module raises ``ImportError``.
"""

from __future__ import annotations

import contextlib
import ctypes
import os
from typing import Any, Callable, Iterator

# torch FIRST: libpcc_structural.so needs libamdhip64.so.7, and the process must end up with ONE HIP runtime.  With
# torch imported before the library is loaded, the loader resolves that name to the runtime torch already brought in
# (the copy bundled in torch/lib); loaded the other way round, the library pulls /opt/rocm's copy, torch then loads
# its own, and launches through the first runtime on memory of the second fail with hipErrorNoDevice.
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('PCC_LIB_OVERRIDE') or os.path.join(_HERE, 'lib', 'libpcc_structural.so')  # override: A/B builds only

_vp = ctypes.c_void_p
_int = ctypes.c_int

# name -> (restype, argtypes); must list every symbol include/pcc_structural.h declares.
ABI: dict[str, tuple[object, list[object]]] = {
    'pcc_version': (ctypes.c_char_p, []),
    'pcc_last_error': (ctypes.c_char_p, []),
    'pcc_last_status': (_int, []),
    'pcc_profile_enable': (None, [_int]),
    'pcc_profile_reset': (None, []),
    'pcc_profile_read': (_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]),
    'pcc_profile_names': (ctypes.c_size_t, [ctypes.c_char_p, ctypes.c_size_t]),
    'nndistance': (None, [_int, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_nndistance': (_int, [_int, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'nndistancegrad': (None, [_int, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_nndistancegrad': (_int, [_int, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_chamfer_loss': (_int, [_int, _int, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_chamfer_loss_grad': (_int, [_int, _int, _vp, _int, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    'pcc_chamfer_emd': (_int, [_int, _int, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_chamfer_emd_grad': (_int, [_int, _int, _vp, _int, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp, _int, _vp, _vp, _vp]),
    'pcc_chamfer_matrix': (_int, [_int, _int, _vp, _int, _int, _vp, _int, _vp, _vp, _vp]),
    'pcc_occupancy_grid': (_int, [_int, _int, _vp, _int, ctypes.c_float, ctypes.c_float, _int, _int, _vp, _vp]),
    'approxmatch': (None, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_approxmatch': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_approxmatch_workspace_bytes': (ctypes.c_size_t, [_int, _int, _int]),
    'pcc_approxmatch_ws': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp]),
    'pcc_approxmatch_cost': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'matchcost': (None, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_matchcost': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'matchcostgrad': (None, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_matchcostgrad': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_matchcostgrad_scaled': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_match_cost': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_sliced_wasserstein': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_sinkhorn': (_int, [_int, _int, _int, _vp, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    # include/pcc_neighbour.h
    'pcc_knn': (_int, [_int, _int, _int, _int, _vp, _vp, _vp]),
    'pcc_knn_cross': (_int, [_int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_fps': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_ball_query': (_int, [_int, _int, _int, _int, ctypes.c_float, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_knn_ragged': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_ball_query_ragged': (_int, [_int, _int, _int, _int, ctypes.c_float, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_group_points': (_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    'pcc_group_points_bwd': (_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    'pcc_interpolate': (_int, [_int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _int, _int, _vp]),
    'pcc_interpolate_bwd': (_int, [_int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _int, _int, _vp, _vp, _vp]),
    'pcc_neighbour_softmax': (_int, [_int, _int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_neighbour_softmax_bwd': (_int, [_int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_aggregate_points': (_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_aggregate_points_bwd': (_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_kpconv_aggregate': (_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, ctypes.c_float, _vp, _vp]),
    'pcc_kpconv_aggregate_bwd': (_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp]),
    'pcc_local_geometry': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_local_covariance_bwd': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_voxel_index': (_int, [_int, _int, _vp, _int, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp]),
    'pcc_voxelize': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_voxelize_bwd': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_devoxelize': (_int, [_int, _int, _int, _int, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp]),
    'pcc_devoxelize_bwd': (_int, [_int, _int, _int, _int, ctypes.c_float, ctypes.c_float, _vp, _vp, _vp, _vp]),
    'pcc_grid_cluster': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_segment_pool': (_int, [_int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_segment_pool_bwd': (_int, [_int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_grid_cluster_ragged': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_cell_neighbours':(_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_sparse_conv': (_int, [_int, _int, _int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_cell_neighbours_ragged': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_gather_neighbours': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_gather_neighbours_bwd': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_graph_features': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_graph_features_bwd': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_graph_max_pool': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_graph_max_pool_bwd': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_global_pool': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_neighbour_sum': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_neighbour_sum_bwd': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_neighbour_minmax_target': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_pair_argmin': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    'pcc_pair_sqdist_sum': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_pair_sqdist_sum_bwd': (_int, [_int, _int, _int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    'pcc_bn_stats': (_int, [_int, _int, _int, _vp, _vp, _vp, _vp]),
    'pcc_bn_relu_res_fwd': (_int, [_int, _int, _int, _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, _int, _int, _vp, _vp]),
    'pcc_bn_relu_bwd': (_int, [_int, _int, _int, _vp, _vp, _vp, ctypes.c_float, _vp, _vp, _vp, _int, _vp, _vp, _vp, _vp]),
    # include/pcc_emd.h
    'pcc_auction_forward': (_int, [_int, _int, _vp, _vp, ctypes.c_float, _int, _vp, _vp, _vp]),
    'pcc_auction_status': (_int, []),
    'pcc_auction_backward': (_int, [_int, _int, _vp, _vp, _vp, _vp, _vp, _vp]),
    # include/pcc_test_hooks.h (inert without PCC_TEST_HOOKS=1)
    'pcc_test_inject_auction_failure': (_int, []),
    'pcc_test_inject_approxmatch_failure': (_int, []),
    'pcc_test_set_tuning': (_int, [_int, _int]),
}


def _load() -> ctypes.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f'{LIB_PATH} is missing: the HIP extension has not been built '
            '(run `make -C pointcloudcounterfactual_amd/csrc`); there is no fallback path.'
        )
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    return lib


lib = _load()


def check(status: int, what: str) -> None:
    """Raise the error the reference raises from its launchers (approxmatch.cu:303-306)."""
    if status != 0:
        msg = lib.pcc_last_error().decode() or f'HIP kernel failed : {status}'
        raise RuntimeError(f'{what}: {msg}')


def ptr(t: torch.Tensor | None, name: str, dtype: torch.dtype, device: torch.device) -> int | None:
    """``t.data_ptr()`` once ``t`` is a contiguous ``dtype`` tensor on exactly the CUDA device ``device``; ``None`` is
    passed through as NULL.  Every pointer handed to ``lib`` goes through here: a host pointer, another GPU's memory or
    8-byte indices read from a 4-byte buffer can fault the card, so they are refused before anything is enqueued.
    Reads tensor metadata only (no allocation, copy or synchronisation)."""
    if t is None:
        return None
    if t.device != device or device.type != 'cuda':
        if t.device.type != 'cuda':
            raise RuntimeError(f'{name} must be a CUDA tensor')
        raise RuntimeError(f'{name} is on {t.device}, expected {device}')
    if not t.is_contiguous():
        raise RuntimeError(f'{name} must be contiguous')
    if t.dtype != dtype:
        raise RuntimeError(f'{name} must be {dtype}, found {t.dtype}')
    return t.data_ptr()


def call(fn: Any, what: str, device: torch.device, *args: Any) -> None:
    """``fn(*args, stream)`` on ``device`` and its current stream, raising through ``check(status, what)``."""
    with torch.cuda.device(device):
        check(fn(*args, torch.cuda.current_stream(device).cuda_stream), what)


# include/pcc_test_hooks.h: measurement / bit-identity switches (inert unless PCC_TEST_HOOKS=1 is in the environment)
TUNING = {'am_nocull': 2, 'am_nosplit': 3, 'am_noresident': 4, 'edge_scatter': 5, 'nbrsum_scatter': 6,
          'auction_cluster': 7, 'knn_nosplit': 8, 'knn_wide': 9, 'knn_cross_split': 10, 'fps_path': 11, 'occupancy_path': 12,
          'ball_path': 13, 'group_path': 14, 'interp_path': 15, 'sw_path': 1, 'sinkhorn_split': 0}


def set_tuning(name: str, value: int) -> None:
    """Set a measurement switch of the library (0 = the product's behaviour); raises if the hooks are not armed."""
    if lib.pcc_test_set_tuning(TUNING[name], int(value)) != 1:
        raise RuntimeError('test hooks are not armed: set PCC_TEST_HOOKS=1 before the library is loaded')


@contextlib.contextmanager
def tuning(name: str, value: int) -> Iterator[None]:
    """``set_tuning(name, value)`` for the body of a ``with``; back to 0 behind it, whether or not the body raised: a
    switch left set would reach every call the process makes afterwards."""
    set_tuning(name, value)
    try:
        yield
    finally:
        set_tuning(name, 0)


@contextlib.contextmanager
def profile(mode: int = 1) -> Iterator[Callable[[str | bytes], tuple[float, int]]]:
    """The library's launch profile for the body of a ``with``: cleared and enabled on entry (``mode`` 1: one event pair
    around each launch), disabled and cleared behind it, whether or not the body raised.  Yields ``read(name)`` ->
    (microseconds per launch, launches) over the profile names that begin with ``name``; synchronise before reading.
    ``read.exact()`` -> {exact profile name: launches} of everything recorded so far, no prefix matching (it synchronises
    the device itself, so the record is complete)."""
    def read(name: str | bytes) -> tuple[float, int]:
        us, count = ctypes.c_double(), ctypes.c_int()
        lib.pcc_profile_read(name.encode() if isinstance(name, str) else name, ctypes.byref(us), ctypes.byref(count))
        return us.value, count.value

    def exact() -> dict[str, int]:
        torch.cuda.synchronize()
        need = lib.pcc_profile_names(None, 0)
        buf = ctypes.create_string_buffer(need)
        if lib.pcc_profile_names(buf, need) != need:
            raise RuntimeError('the launch record changed while it was read')
        return {name: int(count) for name, count in (line.split('\t') for line in buf.value.decode().splitlines())}

    read.exact = exact  # type: ignore[attr-defined]
    lib.pcc_profile_reset()
    lib.pcc_profile_enable(mode)
    try:
        yield read
    finally:
        lib.pcc_profile_enable(0)
        lib.pcc_profile_reset()
