"""Every graph op of csrc/graph_ops.hip at every launch schedule, forward and backward, against float64 torch.

The launchers choose a schedule from n, k and LDS arithmetic (gather_fwd, edge_stream_bwd, scatter_bwd,
pcc_neighbour_sum_bwd).  Every case below names the branch it lands in, with the arithmetic in a comment; where two
branches differ in kernel name, the library's own profiler asserts that the named one ran, so a later change of a
threshold cannot silently leave a branch untested.

Two value modes:
  * exact  -- x and the upstream gradient are integers in [-8, 8].  Every sum a kernel forms is then exact in float32
              in any order, so every output and gradient must equal the float64 reference bit for bit: a dropped,
              duplicated or misrouted edge fails.  The many ties check the first-index rule of max / argmax / min-max.
  * random -- normal values.  Each element lies within gamma_m * sum|terms| of the reference, m = the number of terms
              that reach it and gamma_m = m u / (1 - m u), u = 2^-24: a bound that holds for any summation order.

Graphs are random index lists with hubs and a few ids outside [0, n) (-1, n, n + 5), which the kernels replace by the
point itself; large n then needs no kNN.
"""

import contextlib
import ctypes

import pytest
import torch

from tests.unaligned_views import shifted
# autouse fixture: a test of this module that tests/kernel_census.py names runs with the launch profile on from start to end
# (a pcc_profile_enable(0) inside it re-enables, so such a test cannot observe profiling off) and fails if a kernel mapped
# to it did not launch
from tests.which_ran import census_proof  # noqa: F401

pytestmark = pytest.mark.gpu

U = 2.0 ** -24  # unit roundoff of float32
OPS = ('gather', 'features', 'maxpool', 'nbrsum')

# Forward (gather_fwd): channels per workgroup CB = 8 / 4 / 2 / 1 while CB * n * 4 B fits 64 KiB (n <= 2048 / 4096 /
# 8192, then 1 up to the 160 KiB limit n = 40960).  The per-point modes (max / sum / min-max over k) stage the wave's
# index rows as 16-bit ids when rows + 2048 * k bytes fit 160 KiB = 163840 B, else read the int64 list ("unstaged").
# Gather / features take the 16-byte path when n * k % 4 == 0, k >= 4 and both bases are 16-byte aligned.
# Backward of gather / features (edge_stream_bwd): the stream needs P = (7680 // k) & ~63 >= 64 (k <= 120),
# n <= 32768 and the chunk sort's (2n + 7680) * 4 B <= 163584 B (n <= 16608); cb = 2 when 2 * (7680 + n) * 4 B <= 80 KiB
# (n <= 2560), else 1.  Otherwise the per-edge scatter (scatter_bwd_kernel).  Max-pool backward is always that scatter.
# Neighbour-sum backward: the sorted schedule for n <= 16384 (n * 8 B <= 128 KiB), else scatter_lds_kernel<nbrsum>.
#          (b, c, n, k, gather/features backward, neighbour-sum backward)
CASES = [
    # CB 8 (9600 B), k < 4: scalar path, staged (9600 + 6144); P = 2560 >= n: one chunk, cb 2
    pytest.param(2, 5, 300, 3, 'stream', 'sorted', id='fwd-cb8-scalar-staged_bwd-stream'),
    # n * k = 1505 is no multiple of 4: scalar path; staged; P = 1536 >= n, cb 2
    pytest.param(1, 3, 301, 5, 'stream', 'sorted', id='fwd-cb8-scalar-nk-odd_bwd-stream'),
    # c = 9: CB 8 plus a ragged block of one channel; 16-byte path; staged (65536 + 51200); P = 256: 8 chunks, cb 2
    pytest.param(2, 9, 2048, 25, 'stream', 'sorted', id='fwd-cb8-ragged-vec16-staged_bwd-stream-cb2'),
    # CB 4 (48000 B), staged (48000 + 81920); P = 192: 16 chunks, the last one ragged (120 points); cb 1 (n > 2560)
    pytest.param(1, 6, 3000, 40, 'stream', 'sorted', id='fwd-cb4-staged_bwd-stream-cb1-chunks'),
    # CB 8 (65536 B), unstaged (65536 + 131072 > 163840); P = 120 & ~63 = 64, cb 2
    pytest.param(1, 3, 2048, 64, 'stream', 'sorted', id='fwd-cb8-unstaged_bwd-stream-p64'),
    # CB 4 (65536 B), unstaged (65536 + 204800); P = 76 & ~63 = 64, cb 1
    pytest.param(1, 3, 4096, 100, 'stream', 'sorted', id='fwd-cb4-unstaged_bwd-stream-p64-cb1'),
    # CB 1 (36000 B; CB 2 would be 72000 > 65536), unstaged (36000 + 262144); P = 60 & ~63 = 0: per-edge scatter
    pytest.param(1, 2, 9000, 128, 'scatter', 'sorted', id='fwd-cb1-unstaged_bwd-scatter-k128'),
    # the neighbour-sum backward's limit: n = 16384 sorted, 16385 scatter (CB 1, staged: 65536 + 40960)
    pytest.param(1, 3, 16384, 20, 'stream', 'sorted', id='fwd-cb1-staged_bwd-nbrsum-sorted-limit'),
    pytest.param(1, 3, 16385, 20, 'stream', 'scatter', id='fwd-cb1-staged_bwd-nbrsum-scatter'),
    # the edge stream's LDS limit: chunk sort (2 * 16608 + 7680) * 4 = 163584 B fits, n = 16609 does not
    pytest.param(1, 2, 16608, 25, 'stream', 'scatter', id='fwd-cb1-staged_bwd-stream-lds-limit'),
    pytest.param(1, 2, 16609, 25, 'scatter', 'scatter', id='fwd-cb1-staged_bwd-scatter-past-lds-limit'),
    # CB 1 at the row tile's limit (40960 * 4 = 163840 B: no room to stage); every backward the scatter
    pytest.param(1, 2, 40960, 25, 'scatter', 'scatter', id='fwd-cb1-lds-limit-unstaged_bwd-scatter'),
]

# library profiler names of the backward schedules
BWD_KERNELS = {
    'stream': ('edge_stream_bwd_kernel<gather>', 'edge_stream_bwd_kernel<features>'),
    'scatter': ('scatter_bwd_kernel<gather>', 'scatter_bwd_kernel<features>'),
}
NBRSUM_KERNELS = {'sorted': 'nbrsum_bwd_sorted_kernel', 'scatter': 'scatter_lds_kernel<nbrsum>'}
ONCE_EACH = ('gather_lds_kernel<gather>', 'gather_lds_kernel<features>', 'gather_lds_kernel<maxpool>',
             'gather_lds_kernel<nbrsum>', 'gather_lds_kernel<minmax>', 'scatter_bwd_kernel<maxpool>')


def _lib():
    from pointcloudcounterfactual_amd import _lib

    return _lib


def _launches(prefix):
    """Launches recorded by the library's profiler whose kernel name starts with ``prefix``."""
    count = ctypes.c_int(0)
    _lib().lib.pcc_profile_read(prefix.encode(), None, ctypes.byref(count))
    return count.value


@contextlib.contextmanager
def _profiled():
    lib = _lib().lib
    lib.pcc_profile_enable(1)  # (also clears what an earlier call recorded)
    try:
        yield _launches
    finally:
        lib.pcc_profile_enable(0)


# ---- inputs ---------------------------------------------------------------------------------------------------------


def _values(gen, shape, mode):
    if mode == 'exact':
        return torch.randint(-8, 9, shape, generator=gen).float()
    return torch.randn(shape, generator=gen)


def _graph(gen, b, n, k):
    idx = torch.randint(0, n, (b, n, k), generator=gen)
    idx[:, :, 0] = 7 % n                      # a hub every point lists: its bin collects n edges
    idx[:, : n // 3, k - 1] = 3 % n           # a second hub
    idx[:, 1::97, k // 2] = -1                # ids outside [0, n): the kernels use the point itself
    idx[:, 5::89, (k - 1) // 2] = n
    idx[:, 11::101, k - 1] = n + 5
    return idx


def _inputs(b, c, n, k, mode, seed):
    gen = torch.Generator().manual_seed(seed)
    x = _values(gen, (b, c, n), mode)
    idx = _graph(gen, b, n, k)
    ws = {'gather': _values(gen, (b, c, n, k), mode), 'features': _values(gen, (b, 2 * c, n, k), mode),
          'maxpool': _values(gen, (b, c, n), mode), 'nbrsum': _values(gen, (b, c, n), mode)}
    return x, idx, ws


def _effective(idx, n):
    b, _, k = idx.shape
    self_idx = torch.arange(n).view(1, n, 1).expand(b, n, k)
    return torch.where((idx >= 0) & (idx < n), idx, self_idx)


# ---- float64 reference ----------------------------------------------------------------------------------------------


def _gathered(x, eff):
    """x[b, c, eff[b, i, j]] -> [b, c, n, k] (torch.gather)."""
    b, c, n = x.shape
    k = eff.shape[2]
    return torch.gather(x, 2, eff.reshape(b, 1, n * k).expand(b, c, n * k)).view(b, c, n, k)


def _scatter(vals, eff):
    """Edge values [b, c, n, k] summed into the bins of their targets -> [b, c, n] (scatter_add_)."""
    b, c, n, k = vals.shape
    out = torch.zeros(b, c, n, dtype=vals.dtype)
    return out.scatter_add_(2, eff.reshape(b, 1, n * k).expand(b, c, n * k), vals.reshape(b, c, n * k))


def _reference(x, eff, ws):
    """name -> (out, grad, out_terms, grad_terms) in float64; *_terms = (sum of |terms|, number of terms) per element,
    None where the result is exact in any mode (a max).  'minmax' -> tsel[b, 2, c, n]."""
    xd = x.double()
    b, c, n = x.shape
    k = eff.shape[2]
    nb = _gathered(xd, eff)
    xe = xd.unsqueeze(3).expand(b, c, n, k)
    one_e = torch.ones(b, c, n, k, dtype=torch.float64)
    indeg = _scatter(one_e, eff)
    ref = {}

    w = ws['gather'].double()
    ref['gather'] = (nb, _scatter(w, eff), (nb.abs(), 1.0), (_scatter(w.abs(), eff), indeg))

    w = ws['features'].double()
    w1, w2 = w[:, :c], w[:, c:]
    out = torch.cat([nb - xe, xe], 1)
    mag = torch.cat([nb.abs() + xe.abs(), xe.abs()], 1)
    cnt = torch.cat([2 * one_e, one_e], 1)
    grad = _scatter(w1, eff) + (w2 - w1).sum(3)
    gmag = _scatter(w1.abs(), eff) + (w2.abs() + w1.abs()).sum(3)
    ref['features'] = (out, grad, (mag, cnt), (gmag, indeg + 2 * k))

    w = ws['maxpool'].double()
    best, jmax = nb.max(dim=3)  # first maximum, as torch.max
    e4 = eff.unsqueeze(1).expand(b, c, n, k)
    tgt = torch.gather(e4, 3, jmax.unsqueeze(3))[..., 0]
    zero = torch.zeros(b, c, n, dtype=torch.float64)
    ref['maxpool'] = (best, zero.scatter_add(2, tgt, w), None,
                      (zero.scatter_add(2, tgt, w.abs()), zero.scatter_add(2, tgt, torch.ones_like(w))))

    w = ws['nbrsum'].double()
    we = w.unsqueeze(3).expand(b, c, n, k)
    ref['nbrsum'] = (nb.sum(3), _scatter(we, eff), (nb.abs().sum(3), float(k)), (_scatter(we.abs(), eff), indeg))

    jmin = nb.min(dim=3).indices
    ref['minmax'] = torch.stack([tgt, torch.gather(e4, 3, jmin.unsqueeze(3))[..., 0]], dim=1)
    return ref


def _compare(what, got, ref, terms, exact):
    got = got.double()
    assert got.shape == ref.shape, what
    if exact or terms is None:
        bad = got != ref
        assert not bad.any(), f'{what}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 reference'
        return
    mag, cnt = terms
    mu = torch.as_tensor(cnt, dtype=torch.float64) * U
    bound = mu / (1 - mu) * mag
    err = (got - ref).abs()
    bad = ~(err <= bound)  # (NaN fails)
    assert not bad.any(), (f'{what}: {int(bad.sum())} elements beyond gamma_m * sum|terms|; '
                           f'worst excess {float((err - bound)[bad].max())}')


# ---- the ops through their public wrappers -----------------------------------------------------------------------------


def _run_ops(x, idx, ws, dev):
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from pointcloudcounterfactual_amd.edgeconv import neighbour_minmax_target, neighbour_sum

    k = idx.shape[2]
    idx_d = idx.to(dev)
    fns = {
        'gather': lambda t: ops.get_neighbours(t, idx_d, k)[1],
        'features': lambda t: ops.get_graph_features(t, idx_d, k)[1],
        'maxpool': lambda t: ops.graph_max_pooling(t, idx_d, k),
        'nbrsum': lambda t: neighbour_sum(t, idx_d),
    }
    res = {}
    for name in OPS:
        t = x.to(dev, copy=True).requires_grad_(True)
        out = fns[name](t)
        out.backward(ws[name].to(dev))
        res[name] = (out.detach().cpu(), t.grad.cpu())
    res['minmax'] = neighbour_minmax_target(x.to(dev), idx_d).cpu()
    return res


def _check_all(tag, res, ref, exact):
    for name in OPS:
        out, grad = res[name]
        r_out, r_grad, t_out, t_grad = ref[name]
        _compare(f'{tag} {name} forward', out, r_out, t_out, exact)
        _compare(f'{tag} {name} backward', grad, r_grad, t_grad, exact)
    assert torch.equal(res['minmax'], ref['minmax']), f'{tag} neighbour_minmax_target'


@pytest.mark.parametrize('mode', ['exact', 'random'])
@pytest.mark.parametrize('b,c,n,k,es,ns', CASES)
def test_graph_ops_at_every_schedule(cuda, b, c, n, k, es, ns, mode):
    x, idx, ws = _inputs(b, c, n, k, mode, seed=n * 131 + k)
    names = (*ONCE_EACH, *BWD_KERNELS['stream'], *BWD_KERNELS['scatter'], *NBRSUM_KERNELS.values())
    with _profiled() as launches:
        res = _run_ops(x, idx, ws, cuda)
        ran = {p: launches(p) for p in names}
    for p in ONCE_EACH:
        assert ran[p] == 1, (p, ran)
    other = 'scatter' if es == 'stream' else 'stream'
    for want, dont in zip(BWD_KERNELS[es], BWD_KERNELS[other]):
        assert ran[want] == 1 and ran[dont] == 0, (want, ran)
    other = 'scatter' if ns == 'sorted' else 'sorted'
    assert ran[NBRSUM_KERNELS[ns]] == 1 and ran[NBRSUM_KERNELS[other]] == 0, ran
    _check_all(f'{mode} b={b} c={c} n={n} k={k}', res, _reference(x, _effective(idx, n), ws), mode == 'exact')


@pytest.mark.parametrize('b,c,n,k', [(2, 5, 300, 3), (2, 9, 2048, 25), (1, 6, 3000, 40)])
def test_scatter_switches_give_the_exact_bits(cuda, b, c, n, k):
    """The `edge_scatter` / `nbrsum_scatter` measurement switches send the backward of gather, features and neighbour
    sum to the per-edge scatter; on integer values that must give the float64 reference's bits, as the product's
    schedules do (test_graph_ops_at_every_schedule)."""
    x, idx, ws = _inputs(b, c, n, k, 'exact', seed=n * 7 + k)
    with _lib().tuning('edge_scatter', 1), _lib().tuning('nbrsum_scatter', 1), _profiled() as launches:
        res = _run_ops(x, idx, ws, cuda)
        assert launches('edge_stream_bwd_kernel') == 0 and launches('nbrsum_bwd_sorted_kernel') == 0
        for p in (*BWD_KERNELS['scatter'], NBRSUM_KERNELS['scatter']):
            assert launches(p) == 1, p
    _check_all(f'switched b={b} c={c} n={n} k={k}', res, _reference(x, _effective(idx, n), ws), True)


def test_misaligned_index_view_takes_the_scalar_path(cuda):
    """An index tensor that is a view at an 8-byte offset (contiguous, but not 16-byte aligned) sends gather / features to
    the per-edge scalar path; n * k % 4 == 0 here, so without the offset they would take the 16-byte path."""
    b, c, n, k = 2, 9, 2048, 25
    x, idx, ws = _inputs(b, c, n, k, 'exact', seed=5)
    view = shifted(idx.to(cuda))
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    res = _run_ops(x, view, ws, cuda)
    _check_all('misaligned', res, _reference(x, _effective(idx, n), ws), True)


def test_graph_ops_past_the_lds_limit_raise(cuda):
    """n = 40961 does not fit the LDS row tile / bins: every op raises the library's message and launches nothing."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops
    from pointcloudcounterfactual_amd.edgeconv import neighbour_minmax_target, neighbour_sum

    lib = _lib()
    L = lib.lib
    b, c, n, k = 1, 2, 40961, 4
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(b, c, n, generator=gen).to(cuda)
    idx = torch.randint(0, n, (b, n, k), generator=gen).to(cuda)
    g_edge = torch.zeros(b, 2 * c, n, k, device=cuda)
    g_pt = torch.zeros(b, c, n, device=cuda)
    arg = torch.zeros(b, c, n, dtype=torch.int32, device=cuda)
    gx = torch.zeros(b, c, n, device=cuda)
    st = torch.cuda.current_stream(cuda).cuda_stream
    fwd = [
        ('gather_neighbours', lambda: ops.get_neighbours(x, idx, k)),
        ('graph_features', lambda: ops.get_graph_features(x, idx, k)),
        ('graph_max_pool', lambda: ops.graph_max_pooling(x, idx, k)),
        ('neighbour_sum', lambda: neighbour_sum(x, idx)),
        ('neighbour_minmax_target', lambda: neighbour_minmax_target(x, idx)),
    ]
    bwd = [  # (the forwards raise, so the backward entry points are called through the ABI)
        ('gather_neighbours_bwd', lambda: L.pcc_gather_neighbours_bwd(b, c, n, k, idx.data_ptr(), g_edge.data_ptr(),
                                                                       gx.data_ptr(), st)),
        ('graph_features_bwd', lambda: L.pcc_graph_features_bwd(b, c, n, k, idx.data_ptr(), g_edge.data_ptr(),
                                                                 gx.data_ptr(), st)),
        ('graph_max_pool_bwd', lambda: L.pcc_graph_max_pool_bwd(b, c, n, k, idx.data_ptr(), arg.data_ptr(),
                                                                 g_pt.data_ptr(), gx.data_ptr(), st)),
        ('neighbour_sum_bwd', lambda: L.pcc_neighbour_sum_bwd(b, c, n, k, idx.data_ptr(), g_pt.data_ptr(),
                                                               gx.data_ptr(), st)),
    ]
    with _profiled() as launches:
        for name, fn in fwd:
            with pytest.raises(RuntimeError, match=rf'^{name}: graph op: n too large for the LDS row tile$'):
                fn()
        for name, fn in bwd:
            with pytest.raises(RuntimeError, match=rf'^{name}: graph op backward: n too large for the LDS bins$'):
                lib.check(fn(), name)
        assert launches('') == 0
    torch.cuda.synchronize()
    assert not gx.any()  # nothing was written


# ---- non-finite values: torch.max / torch.min / mean semantics --------------------------------------------------------


def _nan_equal(got, ref, what):
    torch.testing.assert_close(got, ref, rtol=0, atol=0, equal_nan=True, msg=what)


@pytest.mark.parametrize('n,k', [pytest.param(300, 8, id='staged'), pytest.param(2048, 64, id='unstaged')])
def test_graph_max_pooling_non_finite(cuda, n, k):
    """graph_max_pooling is x.max(dim=3) in the reference: NaN propagates with the first NaN's index, a row of -inf gives
    index 0.  A NaN at neighbour 0, at a later neighbour, two NaNs, +-inf, rows whose neighbours are all -inf: values
    and the gradient's routing (to the argmax edge of every (channel, point)) against torch.max on the gathered
    tensor."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    nan, inf = float('nan'), float('inf')
    b, c = 1, 4
    gen = torch.Generator().manual_seed(n + k)
    x = torch.randint(-8, 9, (b, c, n), generator=gen).float()
    x[0, :, :5] = torch.tensor([[nan, nan, inf, -inf, -inf],  # special values at points 0..4, per channel
                                [-inf, -inf, nan, -inf, nan],
                                [inf, -inf, -inf, -inf, -inf],
                                [1.0, 2.0, 3.0, 4.0, 5.0]])
    idx = torch.randint(5, n, (b, n, k), generator=gen)
    kind = torch.arange(n) % 8
    idx[0, kind == 0, 0] = 0                                 # a NaN at neighbour j = 0 (channel 0)
    idx[0, kind == 1, k // 2] = 0                            # ... at j > 0
    idx[0, kind == 2, 1] = 0                                 # two NaNs: the first one wins
    idx[0, kind == 2, k - 1] = 1
    idx[0, kind == 3, 2] = 2                                 # +inf and -inf
    idx[0, kind == 3, 0] = 3
    idx[0, kind == 4] = torch.tensor([3, 4]).repeat(k)[:k]   # every neighbour -inf (channels 0 and 2)
    idx[0, kind == 5, 1] = 2                                 # +inf twice (channel 0): the first one
    idx[0, kind == 5, k - 2] = 2
    idx[0, kind == 6, k - 1] = 4                             # a NaN at the last neighbour (channel 1)
    ref, jmax = torch.max(_gathered(x, idx), dim=3)
    w = torch.randint(-8, 9, (b, c, n), generator=gen).float()
    tgt = torch.gather(idx.unsqueeze(1).expand(b, c, n, k), 3, jmax.unsqueeze(3))[..., 0]
    ref_grad = torch.zeros(b, c, n, dtype=torch.float64).scatter_add_(2, tgt, w.double())

    t = x.to(cuda).requires_grad_(True)
    out = ops.graph_max_pooling(t, idx.to(cuda), k)
    _nan_equal(out.detach().cpu(), ref, 'graph_max_pooling values')
    out.backward(w.to(cuda))
    assert torch.equal(t.grad.cpu().double(), ref_grad), 'graph_max_pooling gradient routing'


def _global_rows(n, gen):
    """[2, 8, n]: all -inf; integer ties; two NaNs; +inf twice on -inf; ties across lanes; NaN last; ..."""
    nan, inf = float('nan'), float('inf')
    x = torch.randint(-8, 9, (2, 8, n), generator=gen).float()
    x[0, 0] = -inf                                  # all -inf: torch.max gives index 0
    x[0, 2, n // 2] = nan                           # two NaNs: the first one
    x[0, 2, n - 1] = nan
    x[0, 3] = -inf                                  # +inf at two positions in different lanes
    x[0, 3, (n * 2) // 3] = inf
    x[0, 3, n - 1] = inf
    x[0, 4] = 0.0                                   # ties across lanes
    x[0, 4, [n - 1, n // 3, 65 % n]] = 1.0
    x[0, 5, n - 1] = nan                            # NaN at the very end
    x[0, 6] = -inf                                  # one finite value after -inf
    x[0, 6, n - 1] = -3.0
    x[0, 7, 0] = inf                                # +inf and -inf: the mean is NaN
    x[0, 7, n - 1] = -inf
    x[1] = torch.randn(8, n, generator=gen)
    x[1, 1, n // 4] = nan
    x[1, 2] = -inf
    return x.contiguous()


@pytest.mark.parametrize('layout', ['aligned', 'offset'])
@pytest.mark.parametrize('n', [1, 3, 63, 64, 65, 4096, 4097])
def test_global_max_pool_non_finite(cuda, n, layout):
    """global_max_pool / global_max_mean_pool (x.max(dim=2), x.mean(dim=2)) on rows of -inf, NaNs, +-inf and ties
    across lanes, on the 16-byte path (n % 4 == 0, aligned) and the scalar one (n % 4 != 0, or a view 4 bytes off).
    The argmax is read through the ABI first and must lie in [0, n): only then does the backward scatter with it."""
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    lib = _lib()
    gen = torch.Generator().manual_seed(n)
    x = _global_rows(n, gen)
    b, c, _ = x.shape
    if layout == 'aligned':
        xd = x.to(cuda)
    else:
        xd = shifted(x.to(cuda))
        assert xd.is_contiguous() and xd.data_ptr() % 16 == 4
    ref, ref_arg = torch.max(x, dim=2)

    mx = torch.empty(b, c, device=cuda)
    arg = torch.full((b, c), -7, dtype=torch.int32, device=cuda)
    mean = torch.empty(b, c, device=cuda)
    lib.check(lib.lib.pcc_global_pool(b, c, n, xd.data_ptr(), mx.data_ptr(), arg.data_ptr(), mean.data_ptr(),
                                      torch.cuda.current_stream(cuda).cuda_stream), 'global_pool')
    a = arg.cpu().long()
    assert ((a >= 0) & (a < n)).all(), f'argmax outside [0, {n}): {a[(a < 0) | (a >= n)].tolist()}'
    assert torch.equal(a, ref_arg), (a, ref_arg)
    _nan_equal(mx.cpu(), ref, 'global max')

    # the mean against float64: a sum of n terms and one division
    ref_mean = x.double().mean(dim=2)
    got = mean.cpu().double()
    fin = torch.isfinite(ref_mean)
    _nan_equal(got[~fin], ref_mean[~fin], 'global mean, non-finite rows')
    mu = (n + 1) * U
    bound = mu / (1 - mu) * x.double().abs().sum(dim=2)[fin] / n
    assert ((got[fin] - ref_mean[fin]).abs() <= bound).all(), 'global mean'

    both = ops.global_max_mean_pool(xd).cpu()
    _nan_equal(both[:, :c], ref, 'global_max_mean_pool max')
    _nan_equal(both[:, c:], mean.cpu(), 'global_max_mean_pool mean')

    w = torch.randint(-8, 9, (b, c), generator=gen).float()
    t = xd.detach().clone().requires_grad_(True)
    ops.global_max_pool(t).backward(w.to(cuda))
    tr = x.clone().requires_grad_(True)
    torch.max(tr, dim=2)[0].backward(w)
    assert torch.equal(t.grad.cpu(), tr.grad), 'global_max_pool gradient routing'
