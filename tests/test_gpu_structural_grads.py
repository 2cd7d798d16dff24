"""The stored-index and stored-match gradient kernels against float64, through the C ABI: nn_bwd_range_kernel
(pcc_nndistancegrad, pcc_chamfer_loss_grad, pcc_chamfer_emd_grad) and am_row_kernel / am_grad_fused_kernel (pcc_matchcost,
pcc_matchcostgrad, pcc_matchcostgrad_scaled).  References, bounds (derived, not tuned) and case tables:
tests/structural_grad_reference.py; tests/test_structural_grad_bounds.py shows without a GPU that the bounds are
attainable and that the tables catch eight wrong kernels.  Outputs are pre-filled with NaN: every element must be written."""

import ctypes

import numpy as np
import pytest
import torch

from tests import structural_grad_reference as R
from tests.unaligned_views import shifted

pytestmark = pytest.mark.gpu

F32, I32 = torch.float32, torch.int32
PCC_EINVAL = -22
SENTINEL = -12345.0


def _lib():
    from pointcloudcounterfactual_amd import _lib as lib

    return lib


def _dev(x, cuda):
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda)


def _nan(cuda, *shape):
    return torch.full(shape, float('nan'), dtype=F32, device=cuda)


def _np(*ts):
    return tuple(t.cpu().numpy() for t in ts)


def _seed(*dims):
    return sum(d * w for d, w in zip(dims, (1009, 31, 7, 3)))


class Chamfer:
    """One case's inputs on the device and the three entries on them."""

    def __init__(self, cuda, inp):
        self.cuda, self.inp = cuda, inp
        self.b, self.n, self.m = inp['p1'].shape[0], inp['p1'].shape[1], inp['p2'].shape[1]
        self.d = {k: _dev(v, cuda) for k, v in inp.items()}

    def _call(self, name, args):
        lib = _lib()
        g1, g2 = _nan(self.cuda, self.b, self.n, 3), _nan(self.cuda, self.b, self.m, 3)
        p = lambda t, dt=F32: lib.ptr(t, name, dt, self.cuda)
        lib.call(getattr(lib.lib, name), name, self.cuda, *[p(*a) if isinstance(a, tuple) else a for a in args(g1, g2)])
        return _np(g1, g2)

    def nngrad(self, g1=None, g2=None):
        d = self.d
        g1 = d['g1'] if g1 is None else g1
        g2 = d['g2'] if g2 is None else g2
        return self._call('pcc_nndistancegrad', lambda o1, o2: [self.b, self.n, (d['p1'],), self.m, (d['p2'],), (g1,),
                                                               (d['idx1'], I32), (g2,), (d['idx2'], I32), (o1,), (o2,)])

    def lossgrad(self, mean, stride):
        d = self.d
        return self._call('pcc_chamfer_loss_grad', lambda o1, o2: [self.b, self.n, (d['p1'],), self.m, (d['p2'],),
                                                                  (d['idx1'], I32), (d['idx2'], I32), (d['gloss'],), stride,
                                                                  int(mean), (o1,), (o2,)])

    def emdgrad(self, mean, stride, estride, gemd=True):
        d = self.d
        return self._call('pcc_chamfer_emd_grad', lambda o1, o2: [self.b, self.n, (d['p1'],), self.m, (d['p2'],),
                                                                 (d['idx1'], I32), (d['idx2'], I32), (d['gloss'],), stride,
                                                                 int(mean), (d['emd1'],), (d['emd2'],),
                                                                 (d['gemd'],) if gemd else None, estride, (o1,), (o2,)])


def _nn_fn(cuda):
    from pointcloudcounterfactual_amd import backend

    def fn(p1, p2):
        _, i1, _, i2 = backend.NNDistance(_dev(p1, cuda), _dev(p2, cuda))
        return _np(i1, i2)

    return fn


def _check_pair(what, got, ref, exact, tails=None):
    """got (grad1, grad2) against the float64 reference (or the ChamferEMD tail); returns the worst error / bound."""
    worst = 0.0
    for which in (1, 2):
        if tails is None:
            want, bound, mag = ref[f'grad{which}'], R.chamfer_bound(ref, which), ref[f'mag{which}']
        else:
            want, bound, mag = tails[which - 1]
        if exact:
            R.assert_exact(f'{what} grad{which}', want, mag)
            R.assert_words(f'{what} grad{which}', got[which - 1], want.astype(np.float32))
        worst = max(worst, R.assert_close(f'{what} grad{which}', got[which - 1], want, bound))
    return worst


def _run_chamfer_entries(cuda, inp, mean, exact):
    """Every entry on one set of inputs against float64; returns the worst error / bound."""
    c = Chamfer(cuda, inp)
    b, n, m = c.b, c.n, c.m
    ref = lambda g1, g2: R.chamfer_bwd_ref(inp['p1'], inp['p2'], inp['idx1'], inp['idx2'], g1, g2)
    worst = _check_pair('nndistancegrad', c.nngrad(), ref(inp['g1'].astype(np.float64), inp['g2'].astype(np.float64)), exact)
    for stride in (1, 0):
        l1, l2 = R.loss_gradients(inp['gloss'], b, n, m, mean, stride)
        rl = ref(l1, l2)
        lg = c.lossgrad(mean, stride)
        worst = max(worst, _check_pair(f'chamfer_loss_grad mean={mean} stride={stride}', lg, rl, exact))
        if exact:  # the expanded grad_dist, formed outside: gloss / n is exact here
            ng = c.nngrad(_dev(l1.astype(np.float32), cuda), _dev(l2.astype(np.float32), cuda))
            R.assert_words('chamfer_loss_grad == nndistancegrad(expanded) grad1', lg[0], ng[0])
            R.assert_words('chamfer_loss_grad == nndistancegrad(expanded) grad2', lg[1], ng[1])
        for estride, gemd in ((1, True), (0, True), (1, False)):
            ge = inp['gemd'] if gemd else None
            tails = [R.emd_tail_ref(rl, w, inp[f'emd{w}'], ge, b, estride) for w in (1, 2)]
            eg = c.emdgrad(mean, stride, estride, gemd)
            worst = max(worst, _check_pair(f'chamfer_emd_grad mean={mean} strides={stride},{estride} gemd={gemd}', eg, rl, exact, tails))
            if exact:
                s = (inp['gemd'][np.arange(b) * estride] if gemd else np.ones(b, np.float32))[:, None, None]
                R.assert_words('chamfer_emd_grad == loss_grad + emd * grad_emd, grad1', eg[0], lg[0] + inp['emd1'] * s)
                R.assert_words('chamfer_emd_grad == loss_grad + emd * grad_emd, grad2', eg[1], lg[1] + inp['emd2'] * s)
    return worst


@pytest.mark.parametrize('kind', R.LIST_KINDS)
@pytest.mark.parametrize('name,b,n,m', R.CHAMFER_CASES, ids=R.CHAMFER_CASE_IDS)
def test_chamfer_backward_against_float64(cuda, name, b, n, m, kind):
    worst = 0.0
    for mode, mean in (('exact', False), ('exact', True), ('gauss', False), ('gauss', True)):
        inp = R.chamfer_inputs(b, n, m, kind, mode, mean, _seed(b, n, m), _nn_fn(cuda))
        assert inp['idx1'].min() >= 0 and inp['idx1'].max() < m and inp['idx2'].min() >= 0 and inp['idx2'].max() < n
        r = _run_chamfer_entries(cuda, inp, mean, mode == 'exact')
        worst = max(worst, r if mode == 'gauss' else 0.0)
    print(f'chamfer backward {name} {kind}: worst error / bound = {worst:.3f}')


def test_chamfer_backward_samples_are_independent(cuda):
    """A batch equals its samples one by one (another P: ceil(512 / b) changes) and a permuted batch, word for word in
    exact mode; one NaN and two infinite coordinates in one sample leave NaN exactly where float64 has it, and the other
    samples as they were."""
    b, n, m = 3, 257, 130
    inp = R.chamfer_inputs(b, n, m, 'uniform', 'exact', False, 11)
    whole = Chamfer(cuda, inp).nngrad()
    perm = np.array([2, 0, 1])
    shuffled = Chamfer(cuda, {k: v[perm] for k, v in inp.items()}).nngrad()
    for s in range(b):
        one = Chamfer(cuda, {k: v[s:s + 1] for k, v in inp.items()}).nngrad()
        for w in (0, 1):
            R.assert_words(f'sample {s} alone, grad{w + 1}', one[w][0], whole[w][s])
            R.assert_words(f'permuted batch, grad{w + 1}', shuffled[w][s], whole[w][perm[s]])
    sick = {k: v.copy() for k, v in inp.items()}
    sick['p1'][1, 5, 0] = np.nan
    sick['p2'][1, 7, 1] = np.inf
    sick['p1'][1, 9, 2] = -np.inf
    for entry in ('nngrad', 'lossgrad'):
        c = Chamfer(cuda, sick)
        if entry == 'nngrad':
            got, clean = c.nngrad(), whole
            g1, g2 = sick['g1'].astype(np.float64), sick['g2'].astype(np.float64)
        else:
            got, clean = c.lossgrad(0, 1), Chamfer(cuda, inp).lossgrad(0, 1)
            g1, g2 = R.loss_gradients(sick['gloss'], b, n, m, False)
        ref = R.chamfer_bwd_ref(sick['p1'], sick['p2'], sick['idx1'], sick['idx2'], g1, g2)
        for w in (1, 2):
            assert np.isnan(ref[f'grad{w}'][1]).any() and not np.isnan(ref[f'grad{w}'][[0, 2]]).any()
            R.assert_close(f'{entry} non-finite grad{w}', got[w - 1], ref[f'grad{w}'], R.chamfer_bound(ref, w))
            R.assert_words(f'{entry} healthy samples grad{w}', got[w - 1][[0, 2]], clean[w - 1][[0, 2]])


# ---- match cost and gradients -------------------------------------------------------------------------------------------------


class Match:
    def __init__(self, cuda, p1, p2, match, misaligned=False):
        self.cuda = cuda
        self.b, self.n, self.m = p1.shape[0], p1.shape[1], p2.shape[1]
        self.p1, self.p2 = _dev(p1, cuda), _dev(p2, cuda)
        if misaligned:  # a contiguous view 4 bytes past a 16-byte boundary: only the scalar kernels may run
            self.match = shifted(_dev(match, cuda))
            assert self.match.data_ptr() % 16 == 4 and self.match.is_contiguous()
        else:
            self.match = _dev(match, cuda)
            assert self.match.data_ptr() % 16 == 0

    def _args(self):
        lib = _lib()
        p = lambda t: lib.ptr(t, 'match test', F32, self.cuda)
        return lib, p, [self.b, self.n, self.m, p(self.p1), p(self.p2), p(self.match)]

    def cost(self):
        lib, p, args = self._args()
        out = _nan(self.cuda, self.b)
        lib.call(lib.lib.pcc_matchcost, 'pcc_matchcost', self.cuda, *args, p(out))
        return out.cpu().numpy()

    def grad(self, gc=None, scaled_entry=False):
        lib, p, args = self._args()
        g1, g2 = _nan(self.cuda, self.b, self.n, 3), _nan(self.cuda, self.b, self.m, 3)
        if gc is None and not scaled_entry:
            lib.call(lib.lib.pcc_matchcostgrad, 'pcc_matchcostgrad', self.cuda, *args, p(g1), p(g2))
        else:
            lib.call(lib.lib.pcc_matchcostgrad_scaled, 'pcc_matchcostgrad_scaled', self.cuda, *args,
                     None if gc is None else p(_dev(gc, self.cuda)), p(g1), p(g2))
        return _np(g1, g2)


def _check_match(what, mt, p1, p2, match, gc):
    """cost, gradients and scaled gradients inside their bounds; scaled == unscaled * gc, gc = 1 == unscaled and a second
    run == the first, word for word.  Returns ({'cost', 'grad1', 'grad2'} -> worst ratio, (cost, grad1, grad2))."""
    ref, refs = R.match_ref(p1, p2, match), R.match_ref(p1, p2, match, gc)
    cost, (g1, g2), (s1, s2) = mt.cost(), mt.grad(), mt.grad(gc)
    worst = {'cost': R.assert_close(f'{what} cost', cost, *ref['cost']),
             'grad1': max(R.assert_close(f'{what} grad1', g1, *ref['grad1']), R.assert_close(f'{what} grad1 scaled', s1, *refs['grad1'])),
             'grad2': max(R.assert_close(f'{what} grad2', g2, *ref['grad2']), R.assert_close(f'{what} grad2 scaled', s2, *refs['grad2']))}
    with np.errstate(invalid='ignore', over='ignore'):
        R.assert_words(f'{what} scaled grad1 == grad1 * gc', s1, g1 * gc[:, None, None])
        R.assert_words(f'{what} scaled grad2 == grad2 * gc', s2, g2 * gc[:, None, None])
    for ones in (np.ones(mt.b, np.float32), None):  # gc = 1, and the scaled entry's NULL = 1
        o1, o2 = mt.grad(ones, scaled_entry=True)
        R.assert_words(f'{what} gc = 1 grad1', o1, g1)
        R.assert_words(f'{what} gc = 1 grad2', o2, g2)
    R.assert_words(f'{what} cost, second run', mt.cost(), cost)
    again = mt.grad(gc)
    R.assert_words(f'{what} grad1, second run', again[0], s1)
    R.assert_words(f'{what} grad2, second run', again[1], s2)
    return worst, (cost, g1, g2)


def _match_both_paths(cuda, what, p1, p2, match, gc, worst):
    """_check_match on the aligned tensor and, where n % 4 == 0, on the misaligned view (the scalar variant: same
    arithmetic, same order, so the same words); folds the ratios into worst and returns the aligned outputs."""
    n = p1.shape[1]
    r, out = _check_match(what, Match(cuda, p1, p2, match), p1, p2, match, gc)
    worst.update({k: max(worst[k], r[k]) for k in worst})
    if n % 4 == 0:
        r, mis = _check_match(f'{what} misaligned', Match(cuda, p1, p2, match, misaligned=True), p1, p2, match, gc)
        worst.update({k: max(worst[k], r[k]) for k in worst})
        for a, c, w in zip(mis, out, ('cost', 'grad1', 'grad2')):
            R.assert_words(f'{what} misaligned == aligned, {w}', a, c)
    return out


@pytest.mark.parametrize('name,b,n,m', R.MATCH_CASES, ids=R.MATCH_CASE_IDS)
def test_match_kernels_against_float64(cuda, name, b, n, m):
    worst = {'cost': 0.0, 'grad1': 0.0, 'grad2': 0.0}
    for kind in ('dense', 'coincident'):
        p1, p2, match, gc = R.match_inputs(b, n, m, kind, _seed(b, n, m))
        out = _match_both_paths(cuda, f'{name} {kind}', p1, p2, match, gc, worst)
        if kind == 'coincident':
            assert all(np.isfinite(o).all() for o in out), 'd = 0 must leave finite gradients and cost'
    print(f'match {name}: worst error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('name', R.ORACLE_MATCH_CASES)
def test_match_kernels_on_the_oracles_match(cuda, oracle_mod, name):
    """The same checks with the CPU oracle's approxmatch output as `match`: the sparse, peaked tensor training produces."""
    _, b, n, m = next(c for c in R.MATCH_CASES if c[0] == name)
    p1, p2, _, gc = R.match_inputs(b, n, m, 'dense', _seed(b, n, m))
    match = np.ascontiguousarray(oracle_mod.approxmatch(p1, p2)[0], np.float32)
    assert match.shape == (b, m, n)
    worst = {'cost': 0.0, 'grad1': 0.0, 'grad2': 0.0}
    _match_both_paths(cuda, f'{name} oracle', p1, p2, match, gc, worst)
    print(f'match {name} (oracle match): worst error / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))


@pytest.mark.parametrize('name,b,n,m', R.MATCH_CASES, ids=R.MATCH_CASE_IDS)
def test_match_single_entries_at_every_tile_corner(cuda, name, b, n, m):
    """Every sample holds a non-zero on every corner row and every corner column of every row tile, slab and chunk
    (R.corner_match; the shorter of the two lists is cycled, the samples rotate the pairing) and nothing else: the
    gradients are non-zero in exactly the columns of grad1 and the rows of grad2 the entries select, exactly zero
    everywhere else, and inside the bounds where they are not."""
    match, where = R.corner_match(n, m, _seed(n, m))
    _, rows, cols = R.corner_entries(n, m)
    p1, p2, _, gc = R.match_inputs(match.shape[0], n, m, 'dense', _seed(n, m) + 1)
    _, (cost, g1, g2) = _check_match(f'{name} corners', Match(cuda, p1, p2, match), p1, p2, match, gc)
    hit1 = np.zeros(g1.shape[:2], bool)
    hit2 = np.zeros(g2.shape[:2], bool)
    for s, r, c in where:
        hit1[s, c] = hit2[s, r] = True
    assert (hit1.sum(1) == len(cols)).all() and (hit2.sum(1) == len(rows)).all(), 'a corner without an entry'
    assert ((g1 != 0).any(-1) == hit1).all(), 'grad1: a column other than the selected ones is non-zero, or a selected one is zero'
    assert ((g2 != 0).any(-1) == hit2).all(), 'grad2: a row other than the selected ones is non-zero, or a selected one is zero'
    assert (cost > 0).all()


def test_match_kernels_samples_are_independent(cuda):
    """The reductions are fixed-order and do not depend on b: a batch equals its samples one by one and a permuted batch
    word for word.  One NaN and two infinite coordinates in one sample: NaN exactly where float64 has it (with the
    kernel's fmax: a NaN squared distance counts as 1e-20), the other samples as they were."""
    b, n, m = 3, 1025, 33
    p1, p2, match, gc = R.match_inputs(b, n, m, 'dense', 21)
    run = lambda sel: (lambda mt: (mt.cost(),) + mt.grad(gc[sel]))(Match(cuda, p1[sel], p2[sel], match[sel]))
    whole = run(np.arange(b))
    perm = np.array([2, 0, 1])
    shuffled = run(perm)
    for s in range(b):
        one = run(np.array([s]))
        for w in range(3):
            R.assert_words(f'sample {s} alone, output {w}', one[w][0], whole[w][s])
            R.assert_words(f'permuted batch, output {w}', shuffled[w][s], whole[w][perm[s]])
    q1, q2 = p1.copy(), p2.copy()
    q1[1, 1024, 0] = np.nan  # the one column of the second slab
    q2[1, 3, 1] = np.inf
    q1[1, 2, 2] = -np.inf
    mt = Match(cuda, q1, q2, match)
    got = (mt.cost(),) + mt.grad(gc)
    ref = R.match_ref(q1, q2, match, gc)
    cref = R.match_ref(q1, q2, match)['cost']
    assert np.isnan(cref[0][1]) and np.isnan(ref['grad1'][0][1]).any() and np.isnan(ref['grad2'][0][1]).any()
    assert np.isfinite(ref['grad1'][0][1]).any(), 'a NaN coordinate stays in its own component'
    R.assert_close('non-finite cost', got[0], *cref)
    R.assert_close('non-finite grad1', got[1], *ref['grad1'])
    R.assert_close('non-finite grad2', got[2], *ref['grad2'])
    for w in range(3):
        R.assert_words(f'healthy samples, output {w}', got[w][[0, 2]], whole[w][[0, 2]])


# ---- the reference-named void launchers ---------------------------------------------------------------------------------------


def test_void_launchers_equal_their_pcc_twins(cuda):
    """nndistance, nndistancegrad, approxmatch, matchcost, matchcostgrad: the names the reference binds.  Same outputs
    as the pcc_* twin word for word, status 0 afterwards; a bad call leaves a non-zero status and a message naming the entry."""
    lib = _lib()
    L = lib.lib
    b, n, m = 2, 70, 33
    inp = R.chamfer_inputs(b, n, m, 'uniform', 'exact', False, 31)
    d = {k: _dev(v, cuda) for k, v in inp.items()}
    match = _dev(np.random.default_rng(3).random((b, m, n), dtype=np.float32), cuda)
    st = torch.cuda.current_stream(cuda).cuda_stream
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def outputs(kind):
        f = lambda *s: _nan(cuda, *s)
        i = lambda *s: torch.full(s, -1, dtype=I32, device=cuda)
        return {'nndistance': [f(b, n), i(b, n), f(b, m), i(b, m)], 'nndistancegrad': [f(b, n, 3), f(b, m, 3)],
                'approxmatch': [f(b, m, n), f(b, 2 * (n + m))], 'matchcost': [f(b)], 'matchcostgrad': [f(b, n, 3), f(b, m, 3)]}[kind]

    def args(kind, outs):
        o = [P(t) for t in outs]
        return {'nndistance': [b, n, P(d['p1']), m, P(d['p2'])] + o,
                'nndistancegrad': [b, n, P(d['p1']), m, P(d['p2']), P(d['g1']), P(d['idx1']), P(d['g2']), P(d['idx2'])] + o,
                'approxmatch': [b, n, m, P(d['p1']), P(d['p2'])] + o,
                'matchcost': [b, n, m, P(d['p1']), P(d['p2']), P(match)] + o,
                'matchcostgrad': [b, n, m, P(d['p1']), P(d['p2']), P(match)] + o}[kind]

    with torch.cuda.device(cuda):
        for kind in ('nndistance', 'nndistancegrad', 'approxmatch', 'matchcost', 'matchcostgrad'):
            twin, void = outputs(kind), outputs(kind)
            assert getattr(L, 'pcc_' + kind)(*args(kind, twin), st) == 0, L.pcc_last_error()
            assert getattr(L, kind)(*args(kind, void), st) is None
            assert L.pcc_last_status() == 0, (kind, L.pcc_last_error())
            torch.cuda.synchronize()
            for t, v in zip(twin, void):
                if t.dtype == I32:
                    assert torch.equal(t, v) and int(t.min()) >= 0, kind
                else:
                    full = t if kind != 'approxmatch' or t.dim() == 3 else t[:, : n + m]  # temp: remainL | remainR
                    assert not torch.isnan(full).any(), f'{kind}: an output element was not written'
                    R.assert_words(kind, v.cpu().numpy(), t.cpu().numpy())
            bad = args(kind, void)
            bad[1] = -1  # n
            getattr(L, kind)(*bad, st)
            assert L.pcc_last_status() != 0 and L.pcc_last_error().decode().startswith(kind + ':'), (kind, L.pcc_last_error())


# ---- arguments ------------------------------------------------------------------------------------------------------------------


def _entries(cuda, b, n, m):
    """name -> (argument list with tensors, positions of (sizes, required pointers, strides), output tensors)."""
    f = lambda *s: torch.full(s, SENTINEL, dtype=F32, device=cuda)
    z = lambda *s: torch.zeros(s, dtype=F32, device=cuda)
    zi = lambda *s: torch.zeros(s, dtype=I32, device=cuda)
    p1, p2, i1, i2 = z(b, n, 3), z(b, m, 3), zi(b, n), zi(b, m)
    out = {}

    def entry(fname, who, args, sizes, strides, nout=2):  # the last nout arguments are the sentinel-filled outputs
        out[fname] = (who, args, sizes, strides, args[-nout:])

    entry('pcc_nndistancegrad', 'nndistancegrad', [b, n, p1, m, p2, z(b, n), i1, z(b, m), i2, f(b, n, 3), f(b, m, 3)], (0, 1, 3), ())
    entry('pcc_chamfer_loss_grad', 'chamfer_loss_grad', [b, n, p1, m, p2, i1, i2, z(b), 1, 0, f(b, n, 3), f(b, m, 3)], (0, 1, 3), (8,))
    entry('pcc_chamfer_emd_grad', 'chamfer_emd_grad',
          [b, n, p1, m, p2, i1, i2, z(b), 1, 0, z(b, n, 3), z(b, m, 3), z(b), 1, f(b, n, 3), f(b, m, 3)], (0, 1, 3), (8, 13))
    entry('pcc_matchcost', 'matchcost', [b, n, m, p1, p2, z(b, m, n), f(b)], (0, 1, 2), (), 1)
    entry('pcc_matchcostgrad', 'matchcostgrad', [b, n, m, p1, p2, z(b, m, n), f(b, n, 3), f(b, m, 3)], (0, 1, 2), ())
    entry('pcc_matchcostgrad_scaled', 'matchcostgrad', [b, n, m, p1, p2, z(b, m, n), z(b), f(b, n, 3), f(b, m, 3)], (0, 1, 2), ())
    return out


def _status(cuda, fn, args):
    L = _lib().lib
    raw = [ctypes.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(cuda):
        rc = fn(*raw, torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize()
    return rc, L.pcc_last_error().decode()


def test_arguments_are_refused_before_anything_is_written(cuda):
    L = _lib().lib
    b, n, m = 2, 5, 3
    for fname, (who, args, sizes, strides, outs) in _entries(cuda, b, n, m).items():
        fn = getattr(L, fname)
        optional = {'pcc_matchcostgrad_scaled': {6}, 'pcc_chamfer_emd_grad': {12}}.get(fname, set())

        def refused(bad, what):
            rc, msg = _status(cuda, fn, bad)
            assert rc == PCC_EINVAL and msg.startswith(who + ':'), (fname, what, rc, msg)
            assert all(bool((o == SENTINEL).all()) for o in outs), f'{fname}: {what} was refused after an output was written'

        for pos in sizes:
            refused(args[:pos] + [-1] + args[pos + 1:], f'size {pos} = -1')
        for pos, a in enumerate(args):
            if isinstance(a, torch.Tensor) and pos not in optional:
                refused(args[:pos] + [None] + args[pos + 1:], f'null pointer {pos}')
        for pos in strides:
            for bad in (2, -1):
                refused(args[:pos] + [bad] + args[pos + 1:], f'stride {pos} = {bad}')
        rc, _ = _status(cuda, fn, [0] + args[1:])
        assert rc == 0 and all(bool((o == SENTINEL).all()) for o in outs), f'{fname}: b = 0 returns 0 and writes nothing'
        assert _status(cuda, fn, args)[0] == 0 and not any(bool((o == SENTINEL).any()) for o in outs), fname


def test_empty_clouds_behave_as_before(cuda):
    """n = 0 or m = 0: the Chamfer entries accept two empty clouds and refuse one; the match entries return zero cost and
    zero gradients for the cloud that has points."""
    L = _lib().lib
    b = 2
    for n, m in ((0, 0), (0, 4), (4, 0)):
        for fname, (who, args, sizes, strides, outs) in _entries(cuda, b, n, m).items():
            rc, msg = _status(cuda, getattr(L, fname), args)
            if fname.startswith('pcc_match'):
                assert rc == 0, (fname, n, m, msg)
                assert all(bool((o == 0).all()) for o in outs), f'{fname}: an empty sum is 0'
            elif n == 0 and m == 0:
                assert rc == 0, (fname, msg)
            else:
                assert (rc, msg) == (PCC_EINVAL, f'{who}: one cloud is empty'), (fname, n, m, rc, msg)


def test_match_entries_refuse_a_batch_their_grids_cannot_carry(cuda):
    """b = 65536 with n = m = 1: the launches carry the batch in grid.y / grid.z (at most 65535).  Refused by name before
    any allocation or launch; 65535 runs."""
    L = _lib().lib
    for b in (65536, 65535):
        for fname, (who, args, sizes, strides, outs) in _entries(cuda, b, 1, 1).items():
            if not fname.startswith('pcc_match'):
                continue
            rc, msg = _status(cuda, getattr(L, fname), args)
            if b > 65535:
                assert (rc, msg) == (PCC_EINVAL, f'{who}: batch too large'), (fname, rc, msg)
                assert all(bool((o == SENTINEL).all()) for o in outs)
            else:
                assert rc == 0, (fname, msg)
                assert all(bool((o == 0).all()) for o in outs), 'zero clouds, zero match: zero cost and gradients'
