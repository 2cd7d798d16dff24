"""CPU tests: the C-ABI library loads and exports every symbol include/*.h declares (no compute calls),
the host-side mirror reproduces the reference's argument checks, and the drop-in package surface exists."""

import ctypes
import glob
import os
import re
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    names = set()
    for h in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        text = re.sub(r'/\*.*?\*/', '', open(h).read(), flags=re.S)
        for m in re.finditer(r'^\s*(?:const\s+)?[A-Za-z_][\w\s\*]*?\b(\w+)\s*\([^;{]*\)\s*;', text, flags=re.M):
            names.add(m.group(1))
    return names


def test_header_symbols_are_exported_and_bound():
    from pointcloudcounterfactual_amd import _lib

    declared = _declared_symbols()
    assert {'nndistance', 'nndistancegrad', 'approxmatch', 'matchcost', 'matchcostgrad'} <= declared
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/ but not exported'
    assert declared == set(_lib.ABI), (declared ^ set(_lib.ABI))
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ' T ' in ln}
    assert exported == declared, f'library exports symbols outside the declared ABI: {exported ^ declared}'
    assert _lib.lib.pcc_version().decode().startswith('pcc_structural')


def test_header_compiles_as_c():
    """The ABI header is plain C (no torch / HIP types in the signatures)."""
    src = '#include "pcc_structural.h"\nint main(void){return (int)sizeof(pcc_stream_t) == 0;}\n'
    r = subprocess.run(['gcc', '-std=c99', '-Wall', '-Werror', '-fsyntax-only', '-I', os.path.join(ROOT, 'include'),
                        '-x', 'c', '-'], input=src, text=True, capture_output=True)
    assert r.returncode == 0, r.stderr


def test_workspace_query_is_host_only():
    from pointcloudcounterfactual_amd import _lib

    assert _lib.lib.pcc_approxmatch_workspace_bytes(0, 10, 10) == 0
    nbytes = _lib.lib.pcc_approxmatch_workspace_bytes(32, 2048, 2048)
    assert nbytes >= 32 * 9 * 4096 * 4  # at least the nine per-level ratio vectors


def test_backend_rejects_cpu_and_non_contiguous_like_the_reference():
    from pointcloudcounterfactual_amd import backend

    x = torch.zeros(2, 8, 3)
    for fn, args in ((backend.NNDistance, (x, x)), (backend.ApproxMatch, (x, x)),
                     (backend.MatchCost, (x, x, torch.zeros(2, 8, 8))),
                     (backend.MatchCostGrad, (x, x, torch.zeros(2, 8, 8))),
                     (backend.NNDistanceGrad, (x, x, torch.zeros(2, 8, dtype=torch.int32),
                                               torch.zeros(2, 8, dtype=torch.int32), torch.zeros(2, 8), torch.zeros(2, 8)))):
        with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
            fn(*args)


def test_drop_in_package_surface():
    import structural_losses
    from structural_losses import match_cost, nn_distance
    from structural_losses import structural_losses_backend as be

    assert structural_losses.__all__ == ['match_cost', 'nn_distance']
    assert callable(match_cost) and callable(nn_distance)
    for name in ('ApproxMatch', 'MatchCost', 'MatchCostGrad', 'NNDistance', 'NNDistanceGrad'):
        assert callable(getattr(be, name))
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        nn_distance(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        match_cost(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))


def test_chamfer_host_logic():
    from pointcloudcounterfactual_amd.losses import chamfer, torch_chamfer

    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        chamfer(torch.zeros(1, 4, 3), torch.zeros(1, 4, 3))
    g = torch.Generator().manual_seed(0)
    a, b = torch.rand(2, 50, 3, generator=g), torch.rand(2, 40, 3, generator=g)
    dense = ((a[:, :, None, :].double() - b[:, None, :, :].double()) ** 2).sum(-1)
    expect = dense.min(2)[0].sum(1) + dense.min(1)[0].sum(1)
    torch.testing.assert_close(torch_chamfer(a, b).double(), expect, rtol=1e-5, atol=1e-5)


BOUNDARY = os.path.join(ROOT, 'tests', 'golden', 'ref_boundary.json')  # recorded by tests/golden/make_golden.py


def _boundary(section):
    import json

    with open(BOUNDARY) as f:
        return json.load(f)[section]


def _arg(a, objs=None, bases=None):
    """A recorded argument back as a value: a LazyTensor by id, a tensor of the recorded shape and dtype (a view of the
    recorded layout into ``bases[storage]`` where the recording says which storage it viewed), a plain value."""
    if isinstance(a, dict) and 'lazy' in a:
        return objs[a['lazy']]
    if isinstance(a, dict) and 'shape' in a:
        if 'storage' in a:
            return bases[a['storage']].as_strided(a['shape'], a['stride'], a['offset'])
        return torch.zeros(a['shape'], dtype=getattr(torch, a['dtype']))
    return a


def test_reference_wrappers_bind_our_backend():
    """Boundary conformance: every backend name the reference's UNMODIFIED nn_distance.py / match_cost.py import exists
    in our drop-in backend, and every call they make in forward and backward (recorded with the reference's own argument
    shapes and dtypes in tests/golden/ref_boundary.json) is accepted and reaches our argument checks."""
    from structural_losses import structural_losses_backend as ours

    rec = _boundary('structural_losses_wrappers')
    assert set(rec) == {'nn_distance', 'match_cost'}
    assert rec['nn_distance']['imports'] == ['NNDistance', 'NNDistanceGrad']
    assert rec['match_cost']['imports'] == ['ApproxMatch', 'MatchCost', 'MatchCostGrad']
    for wrapper, r in rec.items():
        assert [c['fn'] for c in r['calls'] if c['fn'] in r['imports']] == [c['fn'] for c in r['calls']], wrapper
        for name in r['imports']:
            assert callable(getattr(ours, name, None)), (wrapper, name)
        for call in r['calls']:
            with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
                getattr(ours, call['fn'])(*[_arg(a) for a in call['args']])


def test_pykeops_shim_host_logic():
    """The drop-in ``pykeops`` package: expression shapes, role inference and error behaviour (no compute on CPU)."""
    import pykeops
    from pykeops.torch import LazyTensor

    from pointcloudcounterfactual_amd.keops_shim import SquareDistance

    pykeops.set_verbose(False)
    t1, t2 = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    dist = ((LazyTensor(t1[:, :, None, :]) - LazyTensor(t2[:, None, :, :])) ** 2).sum(-1)  # neighbour_ops.py:37-39
    assert isinstance(dist, SquareDistance) and dist.shape == (2, 5, 7)
    rev = ((LazyTensor(t2[:, None, :, :]) - LazyTensor(t1[:, :, None, :])) ** 2).sum(-1)
    assert rev.shape == (2, 5, 7)
    # quantize.py:22-26: a one-point cloud [B,1,1,D] against a codebook [B,1,K,D]
    q = ((LazyTensor(torch.zeros(4, 1, 4)[:, :, None, :]) - LazyTensor(torch.zeros(4, 16, 4)[:, None, :, :])) ** 2).sum(-1)
    assert q.shape == (4, 1, 16)
    for bad in (lambda: dist.argmin(axis=2), lambda: dist.sum(1), lambda: dist.argKmin(3, dim=2)):
        with pytest.raises((RuntimeError, NotImplementedError)):
            bad()  # CPU tensors: the reference never reaches PyKeOps off the accelerator
    with pytest.raises(NotImplementedError):
        (LazyTensor(t1[:, :, None, :]) - LazyTensor(t2[:, None, :, :])) ** 3
    with pytest.raises(NotImplementedError):
        LazyTensor(torch.zeros(2, 5, 7, 3))
    with pytest.raises(NotImplementedError):
        LazyTensor(t1[:, :, None, :]) - LazyTensor(t1[:, :, None, :])
    with pytest.raises(NotImplementedError):
        dist.argmin(axis=0)


def _replay(trace, lazy_tensor):
    """Apply a recorded sequence of LazyTensor operations to ``lazy_tensor``; returns the objects by id."""
    objs, extent = {}, {}
    for op in trace['ops']:
        for a in [*op['args'], *op['kwargs'].values()]:
            if isinstance(a, dict) and 'storage' in a:
                end = a['offset'] + sum((n - 1) * st for n, st in zip(a['shape'], a['stride'])) + 1
                extent[a['storage'], a['dtype']] = max(extent.get((a['storage'], a['dtype']), 0), end)
    bases = {sid: torch.zeros(n, dtype=getattr(torch, dt)) for (sid, dt), n in extent.items()}
    for i, op in enumerate(trace['ops']):
        args = [_arg(a, objs, bases) for a in op['args']]
        kwargs = {k: _arg(v, objs, bases) for k, v in op['kwargs'].items()}
        objs[i] = lazy_tensor(*args, **kwargs) if op['self'] is None else getattr(objs[op['self']], op['op'])(*args, **kwargs)
    return objs


def test_reference_neighbour_ops_binds_our_pykeops():
    """Boundary conformance: what the reference's UNMODIFIED src/utils/neighbour_ops.py takes from ``pykeops`` and does
    with it (recorded in tests/golden/ref_boundary.json) works on our drop-in: the names it imports, the call it makes at
    import time, and the LazyTensor operations of its pykeops_square_distance (our lazy distance; reductions need the
    accelerator) and pykeops_knn (the argKmin reduction reaches our CUDA check)."""
    import importlib

    import pykeops
    from pointcloudcounterfactual_amd.keops_shim import LazyTensor, SquareDistance

    assert pykeops.__file__.startswith(ROOT)
    rec = _boundary('neighbour_ops_pykeops')
    assert rec['imports'] == {'pykeops': ['pykeops'], 'pykeops.torch': ['LazyTensor']}
    assert importlib.import_module('pykeops.torch').LazyTensor is LazyTensor
    for c in rec['module_calls']:
        getattr(importlib.import_module(c['module']), c['name'])(*c['args'], **c['kwargs'])
    sq = rec['traces']['pykeops_square_distance']
    assert [op['op'] for op in sq['ops']] == ['LazyTensor', 'LazyTensor', '__sub__', '__pow__', 'sum']
    d = _replay(sq, LazyTensor)[sq['result']]
    assert isinstance(d, SquareDistance) and d.shape == (2, 6, 9)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        d.argmin(axis=2)
    kn = rec['traces']['pykeops_knn']
    assert kn['ops'][-1]['op'] == 'argKmin' and kn['result'] == len(kn['ops']) - 1
    objs = _replay({'ops': kn['ops'][:-1]}, LazyTensor)
    assert isinstance(objs[kn['ops'][-1]['self']], SquareDistance) and objs[kn['ops'][-1]['self']].shape == (1, 8, 8)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _replay(kn, LazyTensor)
    # CPU tensors take the reference's torch path: pykeops is never touched
    assert rec['traces']['knn_cpu'] == {'ops': [], 'result': None, 'result_shape': [1, 8, 2]}


def test_every_reference_import_from_neighbour_ops_resolves_here():
    """INTEGRATION.md section 4 promises ONE changed import per caller: every name any file of the reference imports
    from ``src.utils.neighbour_ops`` (metrics_and_losses.py:18, quantize.py:6, encoders.py:13, classifier.py:15,
    decoders.py:15, modelnet.py:18; read from the reference's source text with ``ast`` and recorded in
    tests/golden/ref_boundary.json) must be exported by ``pointcloudcounterfactual_amd.neighbour_ops``."""
    from pointcloudcounterfactual_amd import neighbour_ops as ours

    rec = _boundary('neighbour_ops_imports')
    wanted = rec['imported_names']
    assert {'pykeops_square_distance', 'torch_square_distance', 'get_graph_features', 'graph_max_pooling',
            'graph_filtering', 'index_k_neighbours'} <= set(wanted), wanted
    missing = {n: w for n, w in wanted.items() if not callable(getattr(ours, n, None))}
    assert not missing, missing
    # and the whole public surface of the reference's module
    ref_funcs = rec['functions']
    assert 'knn' in ref_funcs and 'get_local_covariance' in ref_funcs
    assert [n for n in ref_funcs if not callable(getattr(ours, n, None))] == []
    # host behaviour of the new exports (CPU tensors take the reference's dense path; the lazy one needs the accelerator)
    t1, t2 = torch.randn(2, 5, 3), torch.randn(2, 7, 3)
    dense = ours.square_distance(t1, t2)
    assert dense.shape == (2, 5, 7)
    assert torch.allclose(dense, ((t1[:, :, None, :] - t2[:, None, :, :]) ** 2).sum(-1), atol=1e-5)
    lazy = ours.pykeops_square_distance(t1, t2)
    assert lazy.shape == (2, 5, 7)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        lazy.argmin(axis=2)
    idx = ours.index_k_neighbours([t1[0].numpy(), t1[1].numpy()], 3)
    assert idx.shape == (2, 5, 3) and (idx[:, :, 0] == range(5)).all()


def test_neighbour_ops_package_keeps_the_public_surface():
    """``pointcloudcounterfactual_amd.neighbour_ops`` is a package of one module per op family, and the one name every
    caller imports from: each public name the single module had is an attribute of the package and of the same kind, and
    what the top-level package imports from it is the very object the package holds."""
    import ast

    import pointcloudcounterfactual_amd as pkg
    from pointcloudcounterfactual_amd import neighbour_ops as ours
    from torch.autograd import Function

    functions = {
        'aggregate_points', 'attention_aggregate', 'ball_query', 'cell_neighbours', 'cross_square_distance', 'devoxelize',
        'estimate_normals', 'farthest_point_sample', 'feature_propagation', 'get_graph_features', 'get_local_covariance',
        'get_neighbours', 'global_max_mean_pool', 'global_max_pool', 'graph_filtering', 'graph_max_pooling', 'grid_cluster',
        'grid_pool', 'grid_subsample', 'grid_unpool', 'group_points', 'hip_ball_query', 'hip_farthest_point_sample', 'hip_knn',
        'hip_knn_cross', 'hip_kpconv_aggregate', 'index_k_neighbours', 'interpolate_points', 'interpolation_weights',
        'kernel_point_conv', 'kernel_point_influence', 'kernel_point_layout', 'knn', 'knn_cross', 'kpconv_aggregate',
        'local_covariance', 'local_geometry', 'neighbour_softmax', 'point_voxel', 'pykeops_knn', 'pykeops_square_distance',
        'sample_and_group', 'segment_pool', 'self_square_distance', 'sparse_conv', 'square_distance', 'torch_aggregate_points',
        'torch_aggregate_points_bwd', 'torch_ball_query', 'torch_cell_neighbours', 'torch_devoxelize',
        'torch_farthest_point_sample', 'torch_grid_cluster', 'torch_group_points', 'torch_interpolate_points', 'torch_knn',
        'torch_knn_cross', 'torch_kpconv_aggregate', 'torch_kpconv_aggregate_bwd', 'torch_local_covariance',
        'torch_neighbour_softmax', 'torch_neighbour_softmax_bwd', 'torch_scatter_eigen', 'torch_segment_pool',
        'torch_segment_pool_bwd', 'torch_sparse_conv', 'torch_square_distance', 'torch_voxel_index', 'torch_voxelize',
        'vector_attention', 'voxel_index', 'voxelize'}
    autograd = {'AggregatedPoints', 'Devoxelized', 'Grouped', 'Indexed', 'Interpolated', 'KernelPointAggregated', 'LocalCovariance',
                'NeighbourSoftmax', 'SegmentPooled', 'SparseConvolved', 'Voxelized'}
    tuples = {'FeaturePropagation', 'GridIndex', 'GridPooled', 'IndexedOp', 'LocalGeometry', 'SampleAndGroup', 'SparseConvMap',
              'VoxelIndex'}
    layers = {'KernelPointConv', 'SubmanifoldConv3d'}
    constants = {'BALL_PAD': dict, 'F32': torch.dtype, 'I32': torch.dtype, 'I64': torch.dtype, 'KERNEL_SIZES': tuple,
                 'MAX_KERNEL_POINTS': int, 'MAX_LIST_K': int, 'MAX_VOXEL_POINTS': int, 'GATHER': ours.IndexedOp,
                 'GRAPH_FEATURES': ours.IndexedOp, 'GRAPH_MAX_POOL': ours.IndexedOp}
    missing = [n for n in functions | autograd | tuples | layers | set(constants) if not hasattr(ours, n)]
    assert missing == []
    assert [n for n in functions if type(getattr(ours, n)).__name__ != 'function'] == []
    assert [n for n in autograd if not issubclass(getattr(ours, n), Function)] == []
    assert [n for n in tuples if not (issubclass(getattr(ours, n), tuple) and hasattr(getattr(ours, n), '_fields'))] == []
    assert [n for n in layers if not issubclass(getattr(ours, n), torch.nn.Module)] == []
    assert [n for n, kind in constants.items() if type(getattr(ours, n)) is not kind] == []
    for n in autograd:  # the autograd node names seen in traces
        assert getattr(ours, n).__name__ == n
    # the top-level package re-exports the package's own objects
    tree = ast.parse(open(pkg.__file__).read())
    taken = [a.asname or a.name for node in tree.body if isinstance(node, ast.ImportFrom)
             and node.module == 'pointcloudcounterfactual_amd.neighbour_ops' for a in node.names]
    assert {'VoxelIndex', 'voxelize', 'sparse_conv', 'grid_pool'} <= set(taken), taken
    assert [n for n in taken if getattr(pkg, n) is not getattr(ours, n)] == []


def test_bench_starts_its_own_ranks(monkeypatch):
    """`bench.py --gpus N` without a launcher environment must start N ranks itself (reference: src/utils/parallel.py:37-53
    spawns its ranks): the parent builds a `torch.distributed.run` child command for N processes on 127.0.0.1 and relays
    its exit code -- checked here without a GPU by intercepting the child process."""
    import argparse
    import importlib
    import subprocess
    import sys

    bench = importlib.import_module('bench')
    seen = {}

    def fake_run(cmd, env=None, **_kw):
        seen['cmd'], seen['env'] = cmd, env
        return subprocess.CompletedProcess(cmd, 7)

    monkeypatch.setattr(subprocess, 'run', fake_run)
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '4', '--steps', '3', '--warmup', '1', '--via-launcher'])
    rc = bench.self_launch(argparse.Namespace(gpus=4))
    assert rc == 7
    cmd = seen['cmd']
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nproc-per-node=4' in cmd and '--nnodes=1' in cmd
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-6:] == ['--gpus', '4', '--steps', '3', '--warmup', '1'] and cmd[-7].endswith('bench.py')
    assert seen['env']['HSA_ENABLE_IPC_MODE_LEGACY'] == '0'


# The (b, c, n, k) graph entry points of include/pcc_neighbour.h: name -> (number of REQUIRED pointers, which come first,
# number of optional ones behind them).
GRAPH_ENTRIES = {
    'gather_neighbours': (3, 0), 'graph_features': (3, 0), 'graph_max_pool': (3, 1), 'neighbour_sum': (3, 0),
    'neighbour_minmax_target': (3, 0), 'gather_neighbours_bwd': (3, 0), 'graph_features_bwd': (3, 0),
    'graph_max_pool_bwd': (4, 0), 'neighbour_sum_bwd': (3, 0),
}
PCC_OK, PCC_EINVAL = 0, -22


def test_graph_entry_points_check_sizes_and_pointers_before_any_launch():
    """Every graph entry point refuses bad sizes and a NULL required pointer with ``PCC_EINVAL`` and its own message,
    and accepts an empty batch or cloud, before it touches the device (all of these return ahead of the first HIP call,
    so the pointers may be dummies).  The optional pointers (``argmax`` of ``pcc_graph_max_pool``, the three outputs of
    ``pcc_global_pool``) are NULL throughout and never the reason for a refusal."""
    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    dummy = 0x1000  # never dereferenced

    def status_and_error(fn, *args):
        rc = fn(*args, None)  # (default stream)
        return rc, L.pcc_last_error().decode()

    for name, (required, optional) in GRAPH_ENTRIES.items():
        fn = getattr(L, 'pcc_' + name)
        ptrs = [dummy] * required + [None] * optional
        for b, c, n, k in ((1, 0, 4, 2), (70000, 1, 4, 2), (1, 1, 65536, 32768)):
            assert status_and_error(fn, b, c, n, k, *ptrs) == (PCC_EINVAL, f'{name}: bad size'), (name, b, c, n, k)
        for missing in range(required):
            args = [None if i == missing else p for i, p in enumerate(ptrs)]
            assert status_and_error(fn, 1, 1, 4, 2, *args) == (PCC_EINVAL, f'{name}: null pointer'), (name, missing)
        for b, n in ((0, 4), (1, 0)):
            assert status_and_error(fn, b, 1, n, 2, *ptrs) == (PCC_OK, ''), (name, b, n)
            assert status_and_error(fn, b, 1, n, 2, *[None] * len(ptrs)) == (PCC_OK, ''), (name, b, n)

    pool = L.pcc_global_pool
    assert status_and_error(pool, 1, 1, 0, dummy, None, None, None) == (PCC_EINVAL, 'global_pool: bad size')
    assert status_and_error(pool, 1, 1, 4, None, None, None, None) == (PCC_EINVAL, 'global_pool: null pointer')
    assert status_and_error(pool, 0, 1, 4, dummy, None, None, None)[0] == PCC_OK
    assert status_and_error(pool, 1, 0, 4, dummy, None, None, None)[0] == PCC_OK


def test_tuning_scope_sets_the_switch_and_always_sets_it_back(monkeypatch):
    """``_lib.tuning`` is ``set_tuning(name, value)`` on entry and ``set_tuning(name, 0)`` on exit, also when the body
    raises; the body's exception is the caller's."""
    from pointcloudcounterfactual_amd import _lib

    calls = []
    monkeypatch.setattr(_lib, 'set_tuning', lambda name, value: calls.append((name, value)))
    with _lib.tuning('group_path', 2):
        assert calls == [('group_path', 2)]
    assert calls == [('group_path', 2), ('group_path', 0)]
    del calls[:]
    with pytest.raises(ZeroDivisionError):
        with _lib.tuning('group_path', 2):
            1 / 0
    assert calls == [('group_path', 2), ('group_path', 0)]


def test_profile_scope_brackets_the_body_and_always_closes(monkeypatch):
    """``_lib.profile(mode)`` is reset, enable(mode) on entry and enable(0), reset on exit, also when the body raises;
    ``read`` takes ``str`` or ``bytes`` and returns (microseconds per launch, launches) as the library wrote them."""
    from pointcloudcounterfactual_amd import _lib

    calls = []

    class Recorder:
        def pcc_profile_reset(self):
            calls.append('reset')

        def pcc_profile_enable(self, mode):
            calls.append(('enable', mode))

        def pcc_profile_read(self, name, us, count):
            calls.append(('read', name))
            us._obj.value, count._obj.value = 12.5, 3
            return 0

    monkeypatch.setattr(_lib, 'lib', Recorder())
    with _lib.profile(mode=2) as read:
        assert calls == ['reset', ('enable', 2)]
        got = [read('kp_bwd_kernel<direct>'), read(b'kp_bwd_kernel<lds> cb=4')]
    assert got == [(12.5, 3), (12.5, 3)] and [type(v) for v in got[0]] == [float, int]
    assert calls == ['reset', ('enable', 2), ('read', b'kp_bwd_kernel<direct>'), ('read', b'kp_bwd_kernel<lds> cb=4'),
                     ('enable', 0), 'reset']
    del calls[:]
    with pytest.raises(ZeroDivisionError):
        with _lib.profile():
            1 / 0
    assert calls == ['reset', ('enable', 1), ('enable', 0), 'reset']


def test_sampling_and_grouping_dtype_and_device_errors_word_for_word():
    """The two raises ``farthest_point_sample``, ``ball_query``, ``group_points`` and ``sample_and_group`` share
    (``_float32``, ``_same_device``) carry the tensor's name in the words of ``_lib.ptr``; where two apply, the first in the
    function's order of checks wins."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    f64, meta, i32 = '{} must be torch.float32, found torch.float64', '{} is on meta, expected cpu', 'idx must be torch.int64, found torch.int32'
    xyz, centres, start = torch.rand(2, 10, 3), torch.rand(2, 4, 3), torch.zeros(2, dtype=torch.int64)
    x, idx, c, feat = torch.zeros(2, 4, 10), torch.zeros(2, 5, 3, dtype=torch.int64), torch.zeros(2, 4, 5), torch.zeros(2, 4, 10)
    fps, ball, group, sag = ops.farthest_point_sample, ops.ball_query, ops.group_points, ops.sample_and_group
    cases = [(fps, (xyz.double(), 2), f64.format('xyz')), (fps, (xyz, 2, start.to('meta')), meta.format('start')),
             (fps, (xyz.double(), 2, start.to('meta')), f64.format('xyz')),
             (ball, (xyz.double(), centres, 1.0, 4), f64.format('xyz')), (ball, (xyz, centres.double(), 1.0, 4), f64.format('centres')),
             (ball, (xyz, centres.to('meta'), 1.0, 4), meta.format('centres')),
             (ball, (xyz, centres.double().to('meta'), 1.0, 4), f64.format('centres')),
             (group, (x.double(), idx), f64.format('x')), (group, (x, idx.int()), i32), (group, (x, idx, c.double()), f64.format('centres')),
             (group, (x, idx.to('meta')), meta.format('idx')), (group, (x, idx, c.to('meta')), meta.format('centres')),
             (group, (x.double(), idx.to('meta')), f64.format('x')), (group, (x, idx.int().to('meta'), c.double()), i32),
             (group, (x, idx.to('meta'), c.double()), meta.format('idx')),
             (sag, (xyz, feat.double(), 4, 0.5, 3), f64.format('features')), (sag, (xyz, feat.to('meta'), 4, 0.5, 3), meta.format('features')),
             (sag, (xyz.double(), feat.to('meta'), 4, 0.5, 3), f64.format('xyz')),
             (sag, (xyz, feat.double().to('meta'), 4, 0.5, 3), f64.format('features'))]
    for fn, args, expected in cases:
        with pytest.raises(RuntimeError) as e:
            fn(*args)
        assert str(e.value) == expected, (fn.__name__, expected)
