"""Float64 reference, case table, selection mask and error bar for the fused EdgeConv block (edgeconv.FusedEdgeConv).

Shared by tests/test_edgeconv_host.py (no GPU: the reference against closed forms, the mask budget of every case, the
module's CPU path) and tests/test_gpu_edgeconv.py (the HIP path).  Plain torch on the CPU; nothing here imports the package:
the module class and the edge-feature function of the float32 yardstick are handed in by the tests.

The block.  With ``feat = cat([x[idx] - x, x])`` ([B,2C,N,k]) and ``W = [Wa | Wb]`` ([C',2C]):

    z = W feat                                   (the 1x1 convolution, a matmul)
    y = gamma (z - mean) / sqrt(var + eps) + beta    mean, var over (b, n, j): the batch's (biased) in training mode, the
                                                     running ones in eval mode
    out = max_j act(y),  act = LeakyReLU(0.2) or the identity

`reference` evaluates exactly that in float64 and differentiates it with autograd.

The bar.  ``err(t) = max|t - ref| / max|ref|`` against float64, for the output, the four gradients (x, conv.weight,
bn.weight, bn.bias) and the two running statistics.  The yardstick is the same composition in float32 -- torch's own
conv2d / batch_norm / leaky_relu / max on the edge features, on the device and inputs of the code under test
(`unfused_float32`).  Required: ``err(fused) <= FACTOR max(err(unfused float32), FLOOR)`` with FACTOR = 16 and
FLOOR = 8u, u = 2^-24.  FACTOR is not derived: it lies between the ratios measured for the centred rewrite (<= 12) and the
uncentred one (70 .. 2700 off the origin); FLOOR keeps a quantity that comes out almost exact from setting a bar of 0.

The selection mask.  The gradient of a max jumps where the best two edges tie to rounding; no float32 evaluation can be
held to the float64 routing there.  From the float64 values only, per output element (b, c', n):
    gap = best - runner-up of sign(gamma_c') z over DISTINCT targets (a repeated target is the same edge value)
    tau = 8 (c + 4) u max_j ( sum_c |wa| (|x_t - xbar| + |x_n - xbar|) + sum_c |wb| |x_n| ),  xbar the per-sample mean
Elements with gap <= tau get cotangent 0 (which silences them completely, the statistics path included); nothing else is
masked, and forward comparisons mask nothing (the max value is continuous).  At most MASK_CAP = 2 % of a case's elements may
be masked: measured on the reference alone, <= 0.5 % for c <= 5 at every offset, <= 0.25 % for c = 16 at offsets 0 and 8
(1.9 % at offset 64: left out), <= 1.4 % for c = 64 at offsets 0 and 8 (10 % at offset 64: not a case).
"""

from __future__ import annotations

import math
from typing import Any, Callable, NamedTuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
FACTOR = 16.0
FLOOR = 8 * U
MASK_CAP = 0.02
FORWARD_ONLY = ('zero-gamma', 'forward')
EPS = 1e-5
MOMENTUM = 0.25  # (not BatchNorm's default 0.1)
QUANTITIES = ('out', 'grad_x', 'grad_conv', 'grad_gamma', 'grad_beta', 'running_mean', 'running_var')


class Case(NamedTuple):
    b: int
    c: int
    cout: int
    n: int
    k: int
    act: bool
    offset: float
    graph: str  # 'knn' | 'hub'
    special: str = ''  # '' | 'zero-gamma' | 'forward' (both forward only) | 'strided'

    @property
    def id(self) -> str:
        tail = f'-{self.special}' if self.special else ''
        return f'{self.b}x{self.c}x{self.cout}x{self.n}x{self.k}-off{self.offset:g}-{self.graph}{tail}'

    @property
    def seed(self) -> int:
        return (self.n * 131 + self.c * 17 + int(self.offset) * 7 + (self.graph == 'hub')) * 4 + len(self.special)


# (b, c, c', n, k): channel-block remainders (c' = 1, 7, 9, 16, 32, 64 against blocks of 8), n on both sides of 64, k = 1
# and k = n; act=False is the first-layer form
SHAPES = [(2, 3, 16, 200, 8, False), (2, 16, 32, 257, 20, True), (1, 64, 64, 512, 25, True), (3, 5, 9, 130, 4, True),
          (2, 8, 1, 65, 1, True), (1, 4, 7, 64, 64, True)]
OFFSETS = {0.0: (3, 16, 64, 5, 8, 4), 8.0: (3, 16, 64), 64.0: (3, 5)}  # offset -> the input channel counts it runs on

CASES = [Case(*s, off, g) for off, cs in OFFSETS.items() for s in SHAPES if s[1] in cs for g in ('knn', 'hub')]
ZERO_GAMMA_CASE = Case(3, 5, 9, 130, 4, True, 8.0, 'knn', 'zero-gamma')  # gamma[0] = 0.0, gamma[1] = -0.0: forward only
STRIDED_CASE = Case(2, 16, 32, 257, 20, True, 8.0, 'hub', 'strided')
GRAD_CASES = CASES + [STRIDED_CASE]
ALL_CASES = GRAD_CASES + [ZERO_GAMMA_CASE]


def knn_graph(x: torch.Tensor, k: int) -> torch.Tensor:
    """[B,N,k]: the k nearest points of every point, itself included (float64, brute force)."""
    p = x.double().transpose(1, 2)
    d = (p.unsqueeze(2) - p.unsqueeze(1)).pow(2).sum(-1)
    return d.topk(k, dim=2, largest=False).indices


def hub_graph(gen: torch.Generator, b: int, n: int, k: int) -> torch.Tensor:
    """Random targets, column 0 = point 0: rows repeat targets and point 0 has in-degree n."""
    idx = torch.randint(0, n, (b, n, k), generator=gen)
    idx[:, :, 0] = 0
    return idx


_CACHE: dict[Case, dict[str, Any]] = {}


def inputs(case: Case) -> dict[str, Any]:
    """The case's float32 tensors on the CPU (made once, never modified): x [B,C,N], idx [B,N,k], w [C',2C], gamma, beta,
    running_mean, running_var, cot [B,C',N]."""
    if case in _CACHE:
        return _CACHE[case]
    gen = torch.Generator().manual_seed(case.seed)
    b, c, cout, n, k = case.b, case.c, case.cout, case.n, case.k
    x = 0.3 * torch.randn(b, c, n, generator=gen) + case.offset
    idx = knn_graph(x, k) if case.graph == 'knn' else hub_graph(gen, b, n, k)
    bound = 1.0 / math.sqrt(2 * c)
    w = (torch.rand(cout, 2 * c, generator=gen) * 2 - 1) * bound
    gamma = torch.randn(cout, generator=gen)  # both signs
    if case.special == 'zero-gamma':
        gamma[0], gamma[1] = 0.0, -0.0
    beta = torch.randn(cout, generator=gen)
    d = {'x': x, 'idx': idx, 'w': w, 'gamma': gamma, 'beta': beta,
         'running_mean': 0.5 * torch.randn(cout, generator=gen) + 0.1 * case.offset,
         'running_var': torch.rand(cout, generator=gen) + 0.5, 'num_batches_tracked': 3,
         'cot': torch.randn(b, cout, n, generator=gen)}
    _CACHE[case] = d
    return d


def edge_features(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """cat([x[idx] - x, x]) [B,2C,N,k] by torch.gather."""
    b, c, n = x.shape
    k = idx.shape[2]
    nb = torch.gather(x, 2, idx.reshape(b, 1, n * k).expand(-1, c, -1)).view(b, c, n, k)
    xe = x.unsqueeze(3).expand(-1, -1, -1, k)
    return torch.cat([nb - xe, xe], dim=1)


def _edge_values(x: torch.Tensor, idx: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    b, _, n = x.shape
    k = idx.shape[2]
    return torch.matmul(w, edge_features(x, idx).reshape(b, -1, n * k)).view(b, w.shape[0], n, k)


def reference(d: dict[str, Any], act: bool, training: bool, cot: torch.Tensor | None = None) -> dict[str, Any]:
    """The unfused block in float64.  Returns 'out', and with a cotangent the four gradients; in training mode the updated
    running statistics (unbiased variance, momentum MOMENTUM); 'num_batches_tracked'."""
    x = d['x'].double().requires_grad_(True)
    w = d['w'].double().requires_grad_(True)
    gamma = d['gamma'].double().requires_grad_(True)
    beta = d['beta'].double().requires_grad_(True)
    rm, rv = d['running_mean'].double(), d['running_var'].double()
    z = _edge_values(x, d['idx'], w)
    res = {'running_mean': rm, 'running_var': rv, 'num_batches_tracked': d['num_batches_tracked'] + int(training)}
    if training:
        m = float(z.shape[0] * z.shape[2] * z.shape[3])
        mean = z.mean((0, 2, 3))
        var = (z - mean.view(1, -1, 1, 1)).pow(2).mean((0, 2, 3))
        res['running_mean'] = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
        res['running_var'] = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * m / max(m - 1.0, 1.0)
    else:
        mean, var = rm, rv
    y = (z - mean.view(1, -1, 1, 1)) / torch.sqrt(var.view(1, -1, 1, 1) + EPS) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    if act:
        y = torch.where(y < 0, 0.2 * y, y)  # (NaN stays NaN)
    out = y.max(dim=3).values
    res['out'] = out.detach()
    if cot is not None:
        gx, gw, gg, gb = torch.autograd.grad(out, (x, w, gamma, beta), cot.double())
        res.update(grad_x=gx, grad_conv=gw, grad_gamma=gg, grad_beta=gb)
    return res


def selection_mask(d: dict[str, Any]) -> torch.Tensor:
    """[B,C',N] bool: output elements whose best two distinct edges are within tau of each other (module docstring)."""
    x, idx, w = d['x'].double(), d['idx'], d['w'].double()
    b, c, n = x.shape
    k = idx.shape[2]
    s = _edge_values(x, idx, w) * torch.sign(d['gamma'].double()).view(1, -1, 1, 1)
    best, jb = s.max(dim=3)
    ie = idx.unsqueeze(1).expand(-1, w.shape[0], -1, -1)
    tb = torch.gather(ie, 3, jb.unsqueeze(3))
    runner = s.masked_fill(ie == tb, -math.inf).max(dim=3).values  # -inf: every edge of the row has the same target
    gap = best - runner
    dx = (x - x.mean(2, keepdim=True)).abs()
    dt = torch.gather(dx, 2, idx.reshape(b, 1, n * k).expand(-1, c, -1)).view(b, c, n, k)
    wa, wb = w[:, :c].abs(), w[:, c:].abs()
    spread = torch.matmul(wa, (dt + dx.unsqueeze(3)).reshape(b, c, n * k)).view(b, -1, n, k).max(dim=3).values
    tau = 8 * (c + 4) * U * (spread + torch.matmul(wb, x.abs()))
    return gap <= tau


def masked_cotangent(case: Case) -> tuple[torch.Tensor, float]:
    """(the case's cotangent with the masked elements set to 0, the masked share)."""
    d = inputs(case)
    if 'masked' not in d:
        mask = selection_mask(d)
        d['masked'] = (torch.where(mask, torch.zeros_like(d['cot']), d['cot']), float(mask.double().mean()))
    return d['masked']


_REF: dict[tuple[Case, bool], dict[str, Any]] = {}


def case_reference(case: Case, training: bool) -> dict[str, Any]:
    """`reference` of a committed case with its masked cotangent (no cotangent for the forward-only case); cached."""
    key = (case, training)
    if key not in _REF:
        cot = None if case.special in FORWARD_ONLY else masked_cotangent(case)[0]
        _REF[key] = reference(inputs(case), case.act, training, cot)
    return _REF[key]


# ---- the two float32 evaluations: the yardstick and the code under test --------------------------------------------------


def _strided(x: torch.Tensor, idx: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor, Callable[[], torch.Tensor]]:
    """x as a transposed [B,N,C] view three elements into its storage, idx as every other column of a wider list."""
    b, c, n = x.shape
    flat = torch.zeros(3 + b * n * c, dtype=x.dtype, device=x.device)
    flat[3:] = x.transpose(1, 2).reshape(-1)
    flat.requires_grad_(True)
    wide = idx.repeat_interleave(2, dim=2)
    return (flat[3:].view(b, n, c).transpose(1, 2), wide[:, :, ::2],
            lambda: flat.grad[3:].view(b, n, c).transpose(1, 2))


def _collect(out, x_grad, params, bufs, want_grad):
    res = {'out': out.detach().cpu()}
    if want_grad:
        res.update(grad_x=x_grad().cpu(), grad_conv=params[0].grad.reshape(params[0].shape[0], -1).cpu(),
                   grad_gamma=params[1].grad.cpu(), grad_beta=params[2].grad.cpu())
    res.update(running_mean=bufs[0].detach().cpu(), running_var=bufs[1].detach().cpu(), num_batches_tracked=int(bufs[2]))
    return res


def _device_inputs(case: Case, dev: Any, x_override: torch.Tensor | None, sample: int | None = None):
    d = inputs(case)
    x = (d['x'] if x_override is None else x_override).to(dev)
    idx = d['idx'].to(dev)
    if sample is not None:  # that sample alone, as a batch of one
        x, idx = x[sample:sample + 1], idx[sample:sample + 1]
    if case.special == 'strided':
        x, idx, x_grad = _strided(x, idx)
        assert not x.is_contiguous() and not idx.is_contiguous() and x.storage_offset() == 3
    else:
        x = x.clone().requires_grad_(True)
        x_grad = lambda: x.grad  # noqa: E731
    want_grad = case.special not in FORWARD_ONLY
    cot = masked_cotangent(case)[0].to(dev) if want_grad else None
    if cot is not None and sample is not None:
        cot = cot[sample:sample + 1]
    return d, x, idx, x_grad, cot


def unfused_float32(features: Callable[..., Any], case: Case, training: bool, dev: Any = 'cpu',
                    x_override: torch.Tensor | None = None) -> dict[str, Any]:
    """The yardstick: the composition the fused block replaces, in float32 on `dev`, with torch's own layers on the edge
    features of ``features(x, idx, k)[1]`` (neighbour_ops.get_graph_features)."""
    d, x, idx, x_grad, cot = _device_inputs(case, dev, x_override)
    w = d['w'].to(dev).view(case.cout, 2 * case.c, 1, 1).clone().requires_grad_(True)
    gamma = d['gamma'].to(dev).clone().requires_grad_(True)
    beta = d['beta'].to(dev).clone().requires_grad_(True)
    rm, rv = d['running_mean'].to(dev).clone(), d['running_var'].to(dev).clone()
    y = F.batch_norm(F.conv2d(features(x, idx, case.k)[1], w), rm, rv, gamma, beta, training, MOMENTUM, EPS)
    out = (F.leaky_relu(y, 0.2) if case.act else y).max(dim=3)[0]
    if cot is not None:
        out.backward(cot)
    return _collect(out, x_grad, (w, gamma, beta), (rm, rv, d['num_batches_tracked'] + int(training)), cot is not None)


def fused_float32(module_cls: Callable[..., Any], case: Case, training: bool, dev: Any = 'cpu',
                  x_override: torch.Tensor | None = None, sample: int | None = None) -> dict[str, Any]:
    """The code under test: ``module_cls`` (edgeconv.FusedEdgeConv) with the case's parameters and buffers on `dev`."""
    d, x, idx, x_grad, cot = _device_inputs(case, dev, x_override, sample)
    mod = module_cls(case.c, case.cout, act=case.act, momentum=MOMENTUM, eps=EPS)
    with torch.no_grad():
        mod.conv.weight.copy_(d['w'].view(case.cout, 2 * case.c, 1, 1))
        mod.bn.weight.copy_(d['gamma'])
        mod.bn.bias.copy_(d['beta'])
        mod.bn.running_mean.copy_(d['running_mean'])
        mod.bn.running_var.copy_(d['running_var'])
        mod.bn.num_batches_tracked.fill_(d['num_batches_tracked'])
    mod = mod.to(dev).train(training)
    out = mod(x, idx)
    if cot is not None:
        out.backward(cot)
    return _collect(out, x_grad, (mod.conv.weight, mod.bn.weight, mod.bn.bias),
                    (mod.bn.running_mean, mod.bn.running_var, mod.bn.num_batches_tracked), cot is not None)


def err(got: torch.Tensor, ref: torch.Tensor, where: torch.Tensor | None = None) -> float:
    """max|got - ref| / max|ref| (over `where` if given; NaN if anything compared is not finite)."""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if where is not None:
        got, ref = got[where], ref[where]
    if not ref.numel():
        return 0.0
    return float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def check_bar(tag: str, fused: dict[str, Any], unfused: dict[str, Any], ref: dict[str, Any],
              where: torch.Tensor | None = None) -> list[tuple[str, str, float, float, float]]:
    """Prints (tag, quantity, err fused, err unfused, ratio to the bar's base) for every quantity `ref` holds, then
    asserts ``err(fused) <= FACTOR max(err(unfused), FLOOR)`` for each and equal batch counters.  `where` restricts 'out'
    (the only quantity compared then) to the elements where the reference is finite."""
    rows, bad = [], []
    for q in QUANTITIES:
        if q not in ref or q not in fused or (where is not None and q != 'out'):
            continue
        ef = err(fused[q], ref[q], where if q == 'out' else None)
        eu = err(unfused[q], ref[q], where if q == 'out' else None)
        eu = eu if eu == eu else 0.0  # (a yardstick that is not finite where the reference is sets no bar)
        ratio = ef / max(eu, FLOOR)
        rows.append((tag, q, ef, eu, ratio))
        print(f'edgeconv-bar | {tag} | {q} | {ef:.3e} | {eu:.3e} | {ratio:.2f}')
        if not ef <= FACTOR * max(eu, FLOOR):  # (NaN fails)
            bad.append(f'{q}: fused {ef:.3e}, unfused float32 {eu:.3e}, ratio {ratio:.1f}')
    assert not bad, f'{tag}: beyond {FACTOR:g} x max(unfused float32, 8u): ' + '; '.join(bad)
    assert fused['num_batches_tracked'] == ref['num_batches_tracked'], (tag, fused['num_batches_tracked'])
    return rows


# ---- checks that the CPU and the GPU tests run alike ------------------------------------------------------------------------

NONFINITE_CASE = Case(2, 16, 32, 257, 20, True, 8.0, 'hub', 'forward')


def check_nonfinite(module_cls: Callable[..., Any], features: Callable[..., Any], dev: Any, value: float) -> None:
    """Eval mode, one coordinate of sample 0 set to `value` (NaN or +inf) at a point p that other points list at j > 0
    only.  The float64 reference is non-finite at p and -- for NaN in every channel, for +inf in the channels where
    sign(gamma) wa > 0 -- at every point that lists p; the module's output must be non-finite exactly there (NaN exactly
    where the reference is NaN if `value` is NaN; for +inf, NaN and inf need not coincide: inf - inf arises in different
    places in the two compositions), its finite elements inside the bar, and sample 1 untouched."""
    case = NONFINITE_CASE
    d = dict(inputs(case))
    p = int(d['idx'][0, 5, 3])
    assert p not in (0, 5) and not (d['idx'][0, :, 0] == p).any()
    x = d['x'].clone()
    x[0, 1, p] = value
    d['x'] = x
    want = reference(d, case.act, False)['out']
    fused = fused_float32(module_cls, case, False, dev, x_override=x)
    unfused = unfused_float32(features, case, False, dev, x_override=x)
    bad = ~want.isfinite()
    listing = (d['idx'][0] == p).any(dim=1)
    listing[p] = True  # (the point's own x_n is not finite, whether it lists itself or not)
    assert bad[0, :, p].all() and bad[0, :, 5].any() and not bad[0][:, ~listing].any() and not bad[1].any()
    if value != value:
        assert bad[0][:, listing].all() and torch.equal(want.isnan(), bad)
        assert torch.equal(fused['out'].isnan(), bad), f"{int((fused['out'].isnan() != bad).sum())} elements differ in NaN-ness"
    else:
        assert torch.equal(~fused['out'].isfinite(), bad), f"{int((fused['out'].isfinite() == bad).sum())} elements differ in finiteness"
    assert fused['out'][1].isfinite().all()
    check_bar(f'{dev} {"nan" if value != value else "inf"} eval', fused, unfused, {'out': want, 'num_batches_tracked': 3}, where=~bad)


def minmax_target_reference(y: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """tsel [B,2,C,N]: the target of the largest / smallest y among a point's neighbours, as torch.max / torch.min choose:
    the first NaN if there is one, the first of equal extrema otherwise."""
    b, c, n = y.shape
    k = idx.shape[2]
    nb = torch.gather(y.double(), 2, idx.reshape(b, 1, n * k).expand(-1, c, -1)).view(b, c, n, k)
    isn = nb.isnan()
    first_nan = isn.to(torch.int8).argmax(dim=3)  # (argmax returns the first of equal values)
    ie = idx.unsqueeze(1).expand(-1, c, -1, -1)
    sel = []
    for sign in (1.0, -1.0):
        j = torch.where(isn, -math.inf, sign * nb).argmax(dim=3)
        j = torch.where(isn.any(dim=3), first_nan, j)
        sel.append(torch.gather(ie, 3, j.unsqueeze(3))[..., 0])
    return torch.stack(sel, dim=1)


def minmax_special_inputs(c: int = 9, n: int = 130, k: int = 6) -> tuple[torch.Tensor, torch.Tensor]:
    """y [2,C,N] and idx [2,N,k] for the min/max target: normal values with, in sample 0, a NaN at point 1 (channels 0, 1),
    a second NaN at point 2 (channel 1), +inf at point 3 and -inf at point 4 (channel 2, and channel 0 next to the NaN);
    rows list them at j = 0, at j > 0, both NaNs in either order, a NaN after an inf, and a row of -inf only."""
    gen = torch.Generator().manual_seed(77)
    y = torch.randn(2, c, n, generator=gen)
    nan, inf = float('nan'), float('inf')
    y[0, 0, 1] = y[0, 1, 1] = y[0, 1, 2] = nan
    y[0, 2, 3] = y[0, 0, 3] = inf
    y[0, 2, 4] = y[0, 0, 4] = -inf
    idx = torch.randint(5, n, (2, n, k), generator=gen)  # (the special points are listed only where placed below)
    rows = torch.arange(n) % 8
    idx[0, rows == 0, 0] = 1                 # a NaN at j = 0
    idx[0, rows == 1, k - 1] = 1             # a NaN at the last neighbour
    idx[0, rows == 2, 2] = 1                 # two NaNs (channel 1): the first one's target
    idx[0, rows == 2, 4] = 2
    idx[0, rows == 3, 1] = 2                 # ... in the other order
    idx[0, rows == 3, 3] = 1
    idx[0, rows == 4, 1] = 3                 # +inf, then -inf, then a NaN (channel 0)
    idx[0, rows == 4, 2] = 4
    idx[0, rows == 4, 5] = 1
    idx[0, rows == 5, :] = 4                 # -inf only (channels 0, 2): target 4 at j = 0
    idx[0, rows == 6, 0] = 3                 # +inf twice: the first
    idx[0, rows == 6, 3] = 3
    return y, idx
