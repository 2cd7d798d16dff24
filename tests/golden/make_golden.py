#!/usr/bin/env python3
"""Generate the committed golden fixtures (run in the build container only; needs /root/reference).

Two families, both small ``.npz`` files of plain arrays (loaded with ``allow_pickle=False``):

``ref_neighbour_ops.npz``   inputs and outputs of the reference's OWN pure-torch functions in
    ``/root/reference/src/utils/neighbour_ops.py`` (torch_square_distance :43-50, self_square_distance :53-60,
    torch_knn :71-74, get_neighbours :85-94, graph_max_pooling :106-110, get_graph_features :113-119,
    graph_filtering :122-133), imported by file path and run on CPU, plus the two-line body of
    ``torch_chamfer`` (``src/train/metrics_and_losses.py:46-47``) evaluated over the imported
    ``torch_square_distance``.  The module imports ``pykeops`` at top level, which is not installed here and is
    never touched by the CPU functions; an empty placeholder module is registered for the import to succeed.
    These vectors pin the kNN / graph-op oracle and BASELINE config 1 (CPU sum-Chamfer).

``oracle_structural.npz``   outputs of ``oracle/structural_oracle.c`` for nndistance / nndistancegrad /
    approxmatch / matchcost / matchcostgrad on small seeded inputs.  The reference's CUDA kernels cannot be
    run here (no nvcc / NVIDIA GPU) and it ships no vectors, so these pin the restatement against regressions
    and give the GPU tests committed expected values; they are NOT outputs of the reference ("parity unpinned").

``ref_graph_filtering_ieee.npz``   the reference's graph_filtering on ``filt_x`` with float32 sqrt / exp rounded from
    float64 (``tests.util.host_independent_math``): the same bits on every host, for a bit-exact CPU comparison.

``ref_boundary.json``   what the reference's UNMODIFIED Python code does at the two boundaries this project replaces,
    recorded by running it against recording stand-ins (no source text is stored, only names, argument shapes and
    call order): the backend calls of its ``structural_losses`` wrappers (forward and backward), the ``pykeops``
    names its ``neighbour_ops.py`` imports and calls at import time, the LazyTensor operations its
    ``pykeops_square_distance`` / ``pykeops_knn`` apply, and every name any of its files imports from
    ``src.utils.neighbour_ops``.  tests/test_abi_and_host.py replays them against this project's drop-ins.
"""

import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = '/root/reference'


def load_reference_neighbour_ops():
    for name in ('pykeops', 'pykeops.torch'):
        if name not in sys.modules:
            mod = types.ModuleType(name)
            mod.set_verbose = lambda *_a, **_k: None  # type: ignore[attr-defined]
            mod.LazyTensor = object  # type: ignore[attr-defined]
            sys.modules[name] = mod
    spec = importlib.util.spec_from_file_location('ref_neighbour_ops', os.path.join(REF, 'src/utils/neighbour_ops.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_reference_fixture():
    ref = load_reference_neighbour_ops()
    out = {}
    g = torch.Generator().manual_seed(20261004)
    # Chamfer (config 1 flavour): [B,N,3] x [B,M,3]
    t1 = torch.rand(2, 96, 3, generator=g)
    t2 = torch.rand(2, 80, 3, generator=g)
    d = ref.torch_square_distance(t1, t2)
    out['cd_t1'], out['cd_t2'], out['cd_dist'] = t1.numpy(), t2.numpy(), d.numpy()
    out['cd_chamfer_sum'] = (torch.min(d, dim=-1)[0].sum(1) + torch.min(d, dim=-2)[0].sum(1)).numpy()
    # kNN / graph ops: x[B,C,N]
    for tag, (b, c, n, k) in {'c3': (2, 3, 64, 4), 'c3k20': (2, 3, 257, 20), 'c64': (2, 64, 200, 25)}.items():
        x = torch.randn(b, c, n, generator=g)
        out[f'{tag}_x'] = x.numpy()
        out[f'{tag}_k'] = np.int64(k)
        out[f'{tag}_selfdist'] = ref.self_square_distance(x).numpy()
        idx = ref.torch_knn(x, k)
        out[f'{tag}_knn'] = idx.numpy()
        idx2, feat = ref.get_graph_features(x, indices=torch.empty(0), k=k)
        assert torch.equal(idx, idx2)
        if c <= 3:  # the C=64 edge-feature tensor is 6.6 MB; its content is x[idx]-x | x, covered at C=3
            out[f'{tag}_graph_features'] = feat.numpy()
        out[f'{tag}_max_pool'] = ref.graph_max_pooling(x, indices=idx, k=k).numpy()
    xf = torch.rand(2, 3, 200, generator=g)
    out['filt_x'] = xf.numpy()
    out['filt_out'] = ref.graph_filtering(xf.clone(), k=4).numpy()
    # the same call with float32 sqrt / exp rounded from float64, bit-identical on every host (tests.util), in a file of
    # its own
    from tests.util import host_independent_math

    with host_independent_math():
        filt_out_ieee = ref.graph_filtering(xf.clone(), k=4).numpy()
    np.savez_compressed(os.path.join(HERE, 'ref_graph_filtering_ieee.npz'), filt_x=xf.numpy(), filt_out_ieee=filt_out_ieee)
    # get_local_covariance (:97-103) on the kNN the reference computes itself
    xc = torch.randn(2, 3, 150, generator=g)
    out['cov_x'] = xc.numpy()
    out['cov_k'] = np.int64(16)
    out['cov_out'] = ref.get_local_covariance(xc.clone(), indices=torch.empty(0), k=16).numpy()
    # BASELINE configs[0] at its exact shape (ModelNet40-like N=1024, B=4, Chamfer only, CPU reference path):
    # torch_square_distance (:43-50) + the torch_chamfer body (metrics_and_losses.py:46-47) and its autograd
    # gradients.  The [4,1024,1024] matrix itself (16 MiB) is not stored: its row / column minima and argmins are.
    from tests.util import pair

    a, c = pair(1234 + 1, 4, 1024, 1024, 'recon')
    t1 = torch.from_numpy(a).requires_grad_(True)
    t2 = torch.from_numpy(c).requires_grad_(True)
    d = ref.torch_square_distance(t1, t2)
    m1, m2 = torch.min(d, dim=-1), torch.min(d, dim=-2)
    loss = m1[0].sum(1) + m2[0].sum(1)
    loss.sum().backward()
    out['cfg1_t1'], out['cfg1_t2'] = a, c
    out['cfg1_dist1'], out['cfg1_idx1'] = m1[0].detach().numpy(), m1[1].numpy().astype(np.int32)
    out['cfg1_dist2'], out['cfg1_idx2'] = m2[0].detach().numpy(), m2[1].numpy().astype(np.int32)
    out['cfg1_chamfer_sum'] = loss.detach().numpy()
    out['cfg1_grad1'], out['cfg1_grad2'] = t1.grad.numpy(), t2.grad.numpy()
    np.savez_compressed(os.path.join(HERE, 'ref_neighbour_ops.npz'), **out)
    print('wrote ref_neighbour_ops.npz', {k: v.shape for k, v in out.items()})


def make_oracle_fixture():
    import oracle
    from tests.util import pair

    oracle.set_threads(4)
    out = {}
    for tag, (b, n, m, kind) in {
        'a': (2, 3, 5, 'uniform'), 'b': (2, 64, 64, 'recon'), 'c': (2, 257, 130, 'uniform'),
        'd': (1, 513, 512, 'recon'), 'e': (2, 128, 256, 'recon'),
    }.items():
        s1, s2 = pair(ord(tag), b, n, m, kind)
        d1, i1, d2, i2 = oracle.nndistance(s1, s2)
        rng = np.random.default_rng(ord(tag))
        g1 = rng.standard_normal((b, n)).astype(np.float32)
        g2 = rng.standard_normal((b, m)).astype(np.float32)
        gr1, gr2 = oracle.nndistancegrad(s1, s2, i1, i2, g1, g2)
        match, temp = oracle.approxmatch(s1, s2)
        cost = oracle.matchcost(s1, s2, match)
        mg1, mg2 = oracle.matchcostgrad(s1, s2, match)
        for k, v in dict(set1=s1, set2=s2, dist1=d1, idx1=i1, dist2=d2, idx2=i2, gdist1=g1, gdist2=g2, nngrad1=gr1,
                         nngrad2=gr2, match=match.astype(np.float32), temp=temp, cost=cost, mgrad1=mg1,
                         mgrad2=mg2).items():
            out[f'{tag}_{k}'] = v
    np.savez_compressed(os.path.join(HERE, 'oracle_structural.npz'), **out)
    print('wrote oracle_structural.npz', len(out), 'arrays')


def _describe(v, ids, storages=None):
    """JSON form of one recorded argument: a LazyTensor stand-in by id, a tensor by shape and dtype (with ``storages``:
    also which recorded storage it views, and how), a plain value."""
    if id(v) in ids:
        return {'lazy': ids[id(v)]}
    if isinstance(v, torch.Tensor):
        d = {'shape': list(v.shape), 'dtype': str(v.dtype).replace('torch.', '')}
        if storages is not None:
            d.update(storage=storages.setdefault(v.untyped_storage().data_ptr(), len(storages)), stride=list(v.stride()),
                     offset=v.storage_offset())
        return d
    return v


def record_structural_losses_wrappers():
    """Run the reference's nn_distance / match_cost (forward + backward) on CPU tensors against a recording backend
    that returns tensors of the shapes the reference's kernels return; record the backend calls in order."""
    pkg_dir = os.path.join(REF, 'external', 'pytorch_structural_losses', 'structural_losses')
    calls = []

    def recorder(name, make):
        def fn(*args):
            calls[-1]['calls'].append({'fn': name, 'args': [_describe(a, {}) for a in args]})
            return make(*args)
        return fn

    b = types.ModuleType('structural_losses.structural_losses_backend')
    b.NNDistance = recorder('NNDistance', lambda x, y: (torch.zeros(x.shape[:2]), torch.zeros(x.shape[:2], dtype=torch.int32),
                                                       torch.zeros(y.shape[:2]), torch.zeros(y.shape[:2], dtype=torch.int32)))
    b.NNDistanceGrad = recorder('NNDistanceGrad', lambda x, y, *_: (torch.zeros_like(x), torch.zeros_like(y)))
    b.ApproxMatch = recorder('ApproxMatch', lambda x, y: (torch.zeros(x.shape[0], y.shape[1], x.shape[1]),
                                                         torch.zeros(x.shape[0], (x.shape[1] + y.shape[1]) * 2)))
    b.MatchCost = recorder('MatchCost', lambda x, y, m: torch.zeros(x.shape[0]))
    b.MatchCostGrad = recorder('MatchCostGrad', lambda x, y, m: (torch.zeros_like(x), torch.zeros_like(y)))
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'structural_losses' or k.startswith('structural_losses.')}
    pkg = types.ModuleType('structural_losses')
    pkg.__path__ = [pkg_dir]
    sys.modules['structural_losses'] = pkg
    sys.modules['structural_losses.structural_losses_backend'] = b
    out = {}
    try:
        for name in ('nn_distance', 'match_cost'):
            spec = importlib.util.spec_from_file_location(f'structural_losses.{name}', os.path.join(pkg_dir, f'{name}.py'))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[spec.name] = mod
            spec.loader.exec_module(mod)
            x = torch.rand(2, 5, 3, requires_grad=True)
            y = torch.rand(2, 7, 3, requires_grad=True)
            calls.append({'wrapper': name, 'calls': []})
            res = getattr(mod, name)(x, y)
            res = res if isinstance(res, tuple) else (res,)
            sum(r.sum() for r in res).backward()
            imported = [n for n in vars(mod) if not n.startswith('_') and getattr(b, n, None) is vars(mod)[n]]
            out[name] = {'imports': sorted(imported), 'calls': calls[-1]['calls'],
                         'returns': [list(r.shape) for r in res]}
    finally:
        for k in [k for k in sys.modules if k == 'structural_losses' or k.startswith('structural_losses.')]:
            del sys.modules[k]
        sys.modules.update(saved)
    return out


def record_neighbour_ops_pykeops():
    """Import the reference's neighbour_ops.py against a recording ``pykeops``; record the names it takes from it, the
    calls it makes at import time, and the LazyTensor operations of pykeops_square_distance / pykeops_knn."""
    log = []
    module_calls = []
    storages = {}

    class Rec:
        def __init__(self, *args, **kwargs):
            self._record('LazyTensor', None, args, kwargs)

        def _record(self, op, src, args, kwargs):
            ids = {id(o): o._id for o in [src, *args] if isinstance(o, Rec)}
            self._id = len(log)
            log.append({'op': op, 'self': None if src is None else src._id, 'args': [_describe(a, ids, storages) for a in args],
                        'kwargs': {k: _describe(v, ids, storages) for k, v in kwargs.items()}})

        def _apply(self, op, *args, **kwargs):
            r = Rec.__new__(Rec)
            r._record(op, self, args, kwargs)
            return r

        def __getattr__(self, name):
            if name.startswith('_'):
                raise AttributeError(name)
            return lambda *a, **k: self._apply(name, *a, **k)

    for dunder in ('__add__', '__radd__', '__sub__', '__rsub__', '__mul__', '__rmul__', '__truediv__', '__pow__', '__neg__',
                   '__abs__'):
        setattr(Rec, dunder, (lambda d: lambda self, *a: self._apply(d, *a))(dunder))

    class RecModule(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith('__'):
                raise AttributeError(name)
            return lambda *a, **k: module_calls.append({'module': self.__name__, 'name': name, 'args': list(a),
                                                         'kwargs': k})

    pk, pkt = RecModule('pykeops'), RecModule('pykeops.torch')
    pkt.LazyTensor = Rec
    pk.torch = pkt
    saved = {k: sys.modules.pop(k) for k in ('pykeops', 'pykeops.torch') if k in sys.modules}
    sys.modules['pykeops'], sys.modules['pykeops.torch'] = pk, pkt
    try:
        spec = importlib.util.spec_from_file_location('ref_neighbour_ops_rec', os.path.join(REF, 'src/utils/neighbour_ops.py'))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k in ('pykeops', 'pykeops.torch'):
            sys.modules.pop(k, None)
        sys.modules.update(saved)
    imports = {'pykeops': [], 'pykeops.torch': [n for n in vars(mod) if vars(mod)[n] is Rec]}
    imports['pykeops'] = [n for n in vars(mod) if vars(mod)[n] is pk]
    traces = {}
    for name, call in (('pykeops_square_distance', lambda: mod.pykeops_square_distance(torch.zeros(2, 6, 3), torch.zeros(2, 9, 3))),
                       ('pykeops_knn', lambda: mod.pykeops_knn(torch.zeros(1, 3, 8), 2)),
                       ('knn_cpu', lambda: mod.knn(torch.zeros(1, 3, 8), 2))):
        del log[:]
        storages.clear()
        res = call()
        traces[name] = {'ops': list(log), 'result': res._id if isinstance(res, Rec) else None,
                        'result_shape': list(res.shape) if isinstance(res, torch.Tensor) else None}
    return {'imports': imports, 'module_calls': module_calls, 'traces': traces}


def record_neighbour_ops_imports():
    """Every name any file of the reference imports from ``src.utils.neighbour_ops`` (read with ``ast``: those modules
    need drytorch / python 3.13 and cannot be imported), and the functions that module defines."""
    import ast

    wanted: dict[str, list[str]] = {}
    for dirpath, _dirs, files in sorted(os.walk(REF)):
        for f in sorted(files):
            if not f.endswith('.py'):
                continue
            path = os.path.join(dirpath, f)
            src = open(path).read()
            try:
                tree = ast.parse(src)
            except SyntaxError:  # `type X = ...` statements of python 3.12+: imports still sit at the top
                tree = ast.parse('\n'.join(ln for ln in src.splitlines() if ln.startswith('from src.utils.neighbour_ops import')))
            for node in ast.walk(tree):
                if isinstance(node, ast.ImportFrom) and node.module == 'src.utils.neighbour_ops':
                    for a in node.names:
                        wanted.setdefault(a.name, []).append(os.path.relpath(path, REF))
    tree = ast.parse(open(os.path.join(REF, 'src/utils/neighbour_ops.py')).read())
    return {'imported_names': wanted, 'functions': [n.name for n in tree.body if isinstance(n, ast.FunctionDef)]}


def make_boundary_fixture():
    import json

    out = {'structural_losses_wrappers': record_structural_losses_wrappers(),
           'neighbour_ops_pykeops': record_neighbour_ops_pykeops(),
           'neighbour_ops_imports': record_neighbour_ops_imports()}
    with open(os.path.join(HERE, 'ref_boundary.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')
    print('wrote ref_boundary.json')


if __name__ == '__main__':
    make_reference_fixture()
    make_oracle_fixture()
    make_boundary_fixture()
