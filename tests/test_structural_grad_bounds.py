"""The CPU half of tests/test_gpu_structural_grads.py: on every case of the tables of tests/structural_grad_reference.py a
float32 restatement of the kernels' formulas (the same rounding points, the LDS atomics as a shuffled sequential sum,
the fixed-order reductions in the kernels' order; correctly rounded roots in place of v_sqrt_f32 / v_rsq_f32) meets
every bound and, in exact mode, the float64 reference word for word -- so the bounds are attainable -- and eight
deliberately wrong variants miss a bound or the exact comparison on at least one case -- so the tables and the bounds
cannot hide such a kernel.  The restatement checks the slack of the bounds, not the kernels."""

import numpy as np
import pytest

from tests import structural_grad_reference as R


def _seed(*dims):
    return sum(d * w for d, w in zip(dims, (1009, 31, 7, 3)))


def test_cases_land_in_the_branches_they_are_named_for():
    want = {'p1-single': 1, 'p1-small': 1, 'p1-n1': 1, 'p2-uneven': 2, 'p8-by-b': 8, 'p1-by-b': 1, 'p3-lds-n5': 3,
            'p3-lds-m5': 3, 'p1-lds-full': 1, 'p32-workload': 32}
    for name, b, n, m in R.CHAMFER_CASES:
        assert R.bwd_ranges(b, n, m) == want[name], name
    assert R.bwd_ranges(1, 4, 4092) == 2  # one point more than 'p1-lds-full' takes the LDS floor
    assert [e for e in R.range_edges(5, 3)] == [0, 1, 3, 5]  # ranges of 1, 2 and 2 points
    assert R.range_edges(257, 2) == [0, 128, 257] and R.range_edges(130, 2) == [0, 65, 130]
    for kind in ('border', 'hub', 'uniform'):
        i1, i2 = R.index_lists(kind, 3, 257, 130, np.random.default_rng(0))
        assert i1.min() >= 0 and i1.max() < 130 and i2.min() >= 0 and i2.max() < 257
    i1, i2 = R.index_lists('border', 3, 257, 130, np.random.default_rng(0))
    assert set(np.unique(i1)) == {0, 64, 65, 129} and set(np.unique(i2)) == {0, 127, 128, 256}


def _chamfer_entries(inp, b, n, m, mean, mode):
    """(name, kwargs of chamfer_bwd_f32, float64 g1, g2, tail) for the three entries on one set of inputs."""
    out = [('nndistancegrad', dict(g1=inp['g1'], g2=inp['g2']), inp['g1'].astype(np.float64), inp['g2'].astype(np.float64), None)]
    for stride in (1, 0):
        l1, l2 = R.loss_gradients(inp['gloss'], b, n, m, mean, stride)
        out.append((f'chamfer_loss_grad mean={int(mean)} stride={stride}', dict(gloss=inp['gloss'], mean=mean, stride=stride), l1, l2, None))
        out.append((f'chamfer_emd_grad mean={int(mean)} stride={stride}',
                    dict(gloss=inp['gloss'], mean=mean, stride=stride, emd1=inp['emd1'], emd2=inp['emd2'], gemd=inp['gemd'],
                         gemd_stride=stride), l1, l2, stride))
    return out


def _check_chamfer(inp, b, n, m, mean, mode, wrong=None, seed=0):
    """Runs every entry of the restatement against its reference; returns the worst ratio (raises AssertionError)."""
    worst = 0.0
    for name, kw, g1, g2, tail in _chamfer_entries(inp, b, n, m, mean, mode):
        ref = R.chamfer_bwd_ref(inp['p1'], inp['p2'], inp['idx1'], inp['idx2'], g1, g2)
        got = R.chamfer_bwd_f32(inp['p1'], inp['p2'], inp['idx1'], inp['idx2'], seed=seed, wrong=wrong, **kw)
        for which in (1, 2):
            if tail is None:
                want, bound, mag = ref[f'grad{which}'], R.chamfer_bound(ref, which), ref[f'mag{which}']
            else:
                want, bound, mag = R.emd_tail_ref(ref, which, inp[f'emd{which}'], inp['gemd'], b, tail)
            what = f'{name} grad{which}'
            if mode == 'exact':
                R.assert_exact(what, want, mag)
                R.assert_words(what, got[which - 1], want.astype(np.float32))
            worst = max(worst, R.assert_close(what, got[which - 1], want, bound))
    return worst


@pytest.mark.parametrize('name,b,n,m', R.CHAMFER_CASES, ids=R.CHAMFER_CASE_IDS)
def test_chamfer_backward_restatement_meets_the_bounds(name, b, n, m):
    worst = 0.0
    for kind in R.LIST_KINDS:
        for mode, mean in (('exact', False), ('exact', True), ('gauss', False), ('gauss', True)):
            inp = R.chamfer_inputs(b, n, m, kind, mode, mean, _seed(b, n, m))
            assert inp['idx1'].min() >= 0 and inp['idx1'].max() < m and inp['idx2'].min() >= 0 and inp['idx2'].max() < n
            r = _check_chamfer(inp, b, n, m, mean, mode)
            if mode == 'gauss':
                worst = max(worst, r)
    print(f'chamfer backward {name}: worst error / bound of the float32 restatement = {worst:.3f}')
    assert worst <= 1.0


# the smallest cases first: a variant is caught as soon as one (case, list kind, mode) raises
_WRONG_CHAMFER = ['drop-range-last', 'mean-n-for-m', 'g1-for-g2', 'tail-unscaled']


@pytest.mark.parametrize('wrong', _WRONG_CHAMFER)
def test_wrong_chamfer_backward_is_caught(wrong):
    caught = []
    for name, b, n, m in R.CHAMFER_CASES[:4]:
        for kind in R.LIST_KINDS:
            for mode in ('exact', 'gauss'):
                inp = R.chamfer_inputs(b, n, m, kind, mode, True, _seed(b, n, m))
                try:
                    _check_chamfer(inp, b, n, m, True, mode, wrong=wrong)
                except AssertionError:
                    caught.append((name, kind, mode))
    print(f'{wrong}: caught on {len(caught)} (case, list, mode) combinations, first {caught[:3]}')
    assert caught, f'the wrong variant {wrong} meets every bound on every case: the tables do not reach it'
    # each variant must fall to both kinds of check somewhere: the derived bound and the word-for-word comparison
    assert {c[2] for c in caught} == {'exact', 'gauss'}, caught


def test_border_lists_are_what_catches_a_lost_range_end():
    """'drop-range-last' on the two-range case: the border lists put a third of all indices on a range's last element."""
    name, b, n, m = R.CHAMFER_CASES[3]
    inp = R.chamfer_inputs(b, n, m, 'border', 'exact', False, 1)
    with pytest.raises(AssertionError):
        _check_chamfer(inp, b, n, m, False, 'exact', wrong='drop-range-last')


def _match_variants(name, b, n, m, seed):
    yield 'dense', R.match_inputs(b, n, m, 'dense', seed)
    yield 'coincident', R.match_inputs(b, n, m, 'coincident', seed + 1)
    cm, _ = R.corner_match(n, m, seed + 2)
    p1, p2, _, gc = R.match_inputs(cm.shape[0], n, m, 'dense', seed + 3)
    yield 'corners', (p1, p2, cm, gc)


def _check_match(p1, p2, match, gc, wrong=None):
    worst = {}
    ref = R.match_ref(p1, p2, match)
    refs = R.match_ref(p1, p2, match, gc)
    cost = R.matchcost_f32(p1, p2, match, wrong=wrong if wrong in ('first-coords', 'skip-tile-last-row') else None)
    worst['cost'] = R.assert_close('cost', cost, *ref['cost'])
    gwrong = wrong
    g1, g2 = R.matchgrad_f32(p1, p2, match, wrong=gwrong)
    s1, s2 = R.matchgrad_f32(p1, p2, match, gc=gc, wrong=gwrong)
    worst['grad1'] = max(R.assert_close('grad1', g1, *ref['grad1']), R.assert_close('grad1 scaled', s1, *refs['grad1']))
    worst['grad2'] = max(R.assert_close('grad2', g2, *ref['grad2']), R.assert_close('grad2 scaled', s2, *refs['grad2']))
    return worst


@pytest.mark.parametrize('name,b,n,m', R.MATCH_CASES, ids=R.MATCH_CASE_IDS)
def test_match_restatement_meets_the_bounds(name, b, n, m):
    worst = {'cost': 0.0, 'grad1': 0.0, 'grad2': 0.0}
    for kind, (p1, p2, match, gc) in _match_variants(name, b, n, m, _seed(b, n, m)):
        r = _check_match(p1, p2, match, gc)
        worst = {k: max(worst[k], r[k]) for k in worst}
        if kind == 'coincident':
            g1, g2 = R.matchgrad_f32(p1, p2, match)
            assert np.isfinite(g1).all() and np.isfinite(g2).all()
    print(f'match {name}: worst error / bound of the float32 restatement: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert max(worst.values()) <= 1.0


def test_corner_entries_cover_every_tile_slab_and_chunk_edge():
    samples, rows, cols = R.corner_entries(4100, 130)
    assert rows == [0, 31, 32, 63, 64, 95, 96, 127, 128, 129]
    assert cols == [0, 1023, 1024, 2047, 2048, 3071, 3072, 4095, 4096, 4099]
    assert samples == 1
    assert R.corner_entries(4, 8200)[1][-4:] == [8160, 8191, 8192, 8199] and len(R.corner_entries(4, 8200)[1]) == 514
    for name, b, n, m in R.MATCH_CASES:  # what corner_match PLACES: every corner of every case, in every sample
        samples, rows, cols = R.corner_entries(n, m)
        match, where = R.corner_match(n, m, 0)
        assert match.shape == (samples, m, n) and match.nbytes <= max(2 << 20, 4 * n * m), name
        assert int((match != 0).sum()) == len(where) == len(set(where)), name
        for s in range(samples):
            assert sorted({r for t, r, c in where if t == s}) == rows, (name, s)
            assert sorted({c for t, r, c in where if t == s}) == cols, (name, s)
            assert set(zip(*np.nonzero(match[s]))) == {(r, c) for t, r, c in where if t == s}, (name, s)
    assert R.corner_match(1025, 33, 0)[0].shape[0] == 3  # cols 0, 1023, 1024; the rotations: each row corner meets each column corner


_WRONG_MATCH = ['drop-slab-last', 'first-coords', 'grad2-unscaled', 'skip-tile-last-row']


@pytest.mark.parametrize('wrong', _WRONG_MATCH)
def test_wrong_match_kernel_is_caught(wrong):
    caught = []
    for name, b, n, m in R.MATCH_CASES:
        if name not in ('n1-m130', 'n1023-m31', 'n1024-m32', 'n1025-m33'):  # the small cases are enough, and quick
            continue
        for kind, (p1, p2, match, gc) in _match_variants(name, b, n, m, _seed(b, n, m)):
            try:
                _check_match(p1, p2, match, gc, wrong=wrong)
            except AssertionError:
                caught.append((name, kind))
    print(f'{wrong}: caught on {len(caught)} (case, match) combinations, first {caught[:3]}')
    assert caught, f'the wrong variant {wrong} meets every bound on every case: the table does not reach it'
    assert any(kind == 'dense' for _, kind in caught), caught


def test_first_chunk_coordinates_in_the_cost_kernel_are_caught():
    """The cost kernel's chunks are 2048 columns: only n > 2048 can tell a second chunk that reads the first one's points."""
    name, b, n, m = next(c for c in R.MATCH_CASES if c[0] == 'n2049-m33')
    p1, p2, match, _ = R.match_inputs(b, n, m, 'dense', 5)
    match[:] = 0
    match[:, :, 2048] = 1.0  # all the mass on the one column of the second chunk
    ref = R.match_ref(p1, p2, match)
    R.assert_close('cost', R.matchcost_f32(p1, p2, match), *ref['cost'])
    with pytest.raises(AssertionError):
        R.assert_close('cost', R.matchcost_f32(p1, p2, match, wrong='first-coords'), *ref['cost'])


def test_match_entries_refuse_an_oversized_batch_before_touching_the_device():
    """b = 65536 with n = m = 1 is refused by name ahead of the first HIP call (so the pointers may be dummies and no
    GPU is needed): the launches of these entries carry the batch in grid.y / grid.z.  The five reference-named void
    launchers report a bad call through pcc_last_status / pcc_last_error under their own names."""
    import ctypes

    from pointcloudcounterfactual_amd import _lib

    L = _lib.lib
    keep = ctypes.create_string_buffer(64)
    d = ctypes.cast(keep, ctypes.c_void_p)
    for fn, who, args in ((L.pcc_matchcost, 'matchcost', [d] * 4), (L.pcc_matchcostgrad, 'matchcostgrad', [d] * 5),
                          (L.pcc_matchcostgrad_scaled, 'matchcostgrad', [d] * 6), (L.pcc_approxmatch, 'approxmatch', [d] * 4),
                          (L.pcc_approxmatch_cost, 'approxmatch_cost', [d] * 5),
                          (L.pcc_approxmatch_ws, 'approxmatch', [d, d, d, d, d, ctypes.c_size_t(64)]),
                          (L.pcc_match_cost, 'match_cost', [d] * 6)):
        assert fn(65536, 1, 1, *args, None) == -22 and L.pcc_last_error().decode() == f'{who}: batch too large', who
        assert fn(-1, 1, 1, *args, None) == -22 and L.pcc_last_error().decode() == f'{who}: bad size', who
        assert fn(0, 1, 1, *args, None) == 0 and L.pcc_last_status() == 0
    # pcc_chamfer_emd (b, n, xyz1, m, xyz2, mean, ...): the match_cost grids it launches carry the batch too
    emd = lambda b: L.pcc_chamfer_emd(b, 1, d, 1, d, 1, d, d, d, d, d, d, d, d, None)
    assert emd(65536) == -22 and L.pcc_last_error().decode() == 'chamfer_emd: batch too large'
    assert emd(-1) == -22 and L.pcc_last_error().decode() == 'chamfer_emd: negative size'
    assert emd(0) == 0 and L.pcc_last_status() == 0
    for fn, who, args in ((L.nndistance, 'nndistance', [1, -1, d, 1, d, d, d, d, d]),
                          (L.nndistancegrad, 'nndistancegrad', [1, -1, d, 1, d, d, d, d, d, d, d]),
                          (L.approxmatch, 'approxmatch', [1, -1, 1, d, d, d, d]), (L.matchcost, 'matchcost', [1, -1, 1, d, d, d, d]),
                          (L.matchcostgrad, 'matchcostgrad', [1, -1, 1, d, d, d, d, d])):
        assert fn(*args, None) is None
        assert L.pcc_last_status() == -22 and L.pcc_last_error().decode().startswith(who + ':'), who
