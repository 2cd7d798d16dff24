"""Timings of the all-pairs Chamfer matrix (pcc_chamfer_matrix through set_metrics.pairwise_chamfer), general and self
mode, beside the only way the paired surface can produce the same matrix, on the same GPU in the same process:
`losses.chamfer` over replicated pair batches (32 and 256 pairs per call, the replication included: it is part of that
way).  The variants of a row alternate round by round; a figure is the median over the rounds of the time of ONE whole
matrix inside a hipEvent bracket on the stream.  Also: pairwise_emd pairs/s at 32 pairs per call and at the default.
Output: profiles/chamfer_matrix_times.txt (or --out)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudcounterfactual_amd import losses  # noqa: E402
from pointcloudcounterfactual_amd import set_metrics as sm  # noqa: E402

dev = torch.device('cuda:0')


def bracket(fn):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)  # ms


def medians(variants, rounds=7, warm=1):
    """{name: (median, min, max)} in milliseconds; the variants alternate inside every round, and every round starts one
    variant later."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    names = list(variants)
    for r in range(rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            times[name].append(bracket(variants[name]))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def composed(a, b, pairs_per_call):
    """cd[S,R] through the paired loss: replicated pair batches of `pairs_per_call` pairs."""
    s, r = a.size(0), b.size(0)
    out = torch.empty(s * r, device=dev)
    for p0 in range(0, s * r, pairs_per_call):
        p = torch.arange(p0, min(p0 + pairs_per_call, s * r), device=dev)
        i, j = torch.div(p, r, rounding_mode='floor'), p % r
        out[p0:p0 + p.numel()] = losses.chamfer(a.index_select(0, i), b.index_select(0, j))
    return out.view(s, r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'chamfer_matrix_times.txt'))
    ap.add_argument('--sizes', type=int, nargs='+', default=[128, 400])
    ap.add_argument('--emd-clouds', type=int, default=64)
    args = ap.parse_args()
    torch.manual_seed(0)
    n = 2048
    lines = [f'{torch.cuda.get_device_name(0)}, uniform clouds, N = M = {n}; milliseconds per [S,R] matrix: median of 7 '
             'rounds (min-max), the variants of a row alternating']
    for size in args.sizes:
        a, b = torch.rand(size, n, 3, device=dev), torch.rand(size, n, 3, device=dev)
        ref = composed(a, b, 256)
        got = sm.pairwise_chamfer(a, b)
        worst = ((got - ref).abs() / ref).max().item()
        t = medians({'general': lambda: sm.pairwise_chamfer(a, b), 'self': lambda: sm.pairwise_chamfer(a),
                     'chamfer32': lambda: composed(a, b, 32), 'chamfer256': lambda: composed(a, b, 256)})
        line = f'S=R={size:4d}:'
        for name, label in (('general', 'pairwise_chamfer(a, b)'), ('self', 'pairwise_chamfer(a)'),
                            ('chamfer32', 'chamfer(), 32 pairs per call'), ('chamfer256', 'chamfer(), 256 pairs per call')):
            med, lo, hi = t[name]
            line += f'  {label} {med:9.2f} ({lo:.2f}-{hi:.2f})'
        pairs = size * size * float(n) * n
        line += (f'  [chamfer256 / general {t["chamfer256"][0] / t["general"][0]:.2f}x, chamfer32 / general '
                 f'{t["chamfer32"][0] / t["general"][0]:.2f}x, general / self {t["general"][0] / t["self"][0]:.2f}x; '
                 f'general: {pairs / t["general"][0] * 1e-9:.2f} T point pairs/s; max relative difference to chamfer() {worst:.1e}]')
        print(line, flush=True)
        lines.append(line)
    c = args.emd_clouds
    a, b = torch.rand(c, n, 3, device=dev), torch.rand(c, n, 3, device=dev)
    t = medians({'emd32': lambda: sm.pairwise_emd(a, b, pairs_per_call=32),
                 'emd_default': lambda: sm.pairwise_emd(a, b)})
    line = (f'pairwise_emd S=R={c}: 32 pairs per call {c * c / t["emd32"][0] * 1e3:9.0f} pairs/s ({t["emd32"][0]:.1f} ms), '
            f'{sm.DEFAULT_PAIRS_PER_CALL} pairs per call (default) {c * c / t["emd_default"][0] * 1e3:9.0f} pairs/s '
            f'({t["emd_default"][0]:.1f} ms)  [default / 32: {t["emd32"][0] / t["emd_default"][0]:.2f}x]')
    print(line, flush=True)
    lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
