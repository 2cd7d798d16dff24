"""Timings of the k-NN between two clouds (pcc_knn_cross, knn_wide.hip) beside the stock-torch composition on the same
GPU in the same process (expanded-form distances through bmm, then topk), beside the one-cloud search of the same shape
through the same kernels (`knn_cross(x, x)` beside `pcc_knn` with the `knn_wide` switch), and with the candidate axis
unsplit (`knn_cross_split` = 1) on the few-queries shapes.  The variants of a row alternate round by round; a figure is the median over the rounds of the mean
time per call inside a hipEvent bracket on the stream.  Output: profiles/knn_cross_times.txt (or --out)."""
import argparse
import os
import statistics
import sys

os.environ.setdefault('PCC_TEST_HOOKS', '1')  # the A/B switches of include/pcc_test_hooks.h

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pointcloudcounterfactual_amd import _lib  # noqa: E402
from pointcloudcounterfactual_amd import neighbour_ops as ops  # noqa: E402

dev = torch.device('cuda:0')


def bracket(fn, iters):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def medians(variants, iters, rounds=7, warm=3):
    """{name: (median, min, max)} in microseconds; the variants alternate inside every round, and every round starts
    one variant later, so that none always runs behind the same neighbour."""
    for fn in variants.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    names = list(variants)
    for r in range(rounds):
        for name in names[r % len(names):] + names[:r % len(names)]:
            times[name].append(bracket(variants[name], iters))
    return {name: (statistics.median(t), min(t), max(t)) for name, t in times.items()}


def torch_knn_cross(q, x, k):
    inner = -2 * torch.bmm(q.transpose(2, 1), x)
    d = inner + (x ** 2).sum(dim=1, keepdim=True) + (q ** 2).sum(dim=1).unsqueeze(2)
    return d.topk(k, dim=-1, largest=False)


def with_switch(name, value, fn):
    def run():
        with _lib.tuning(name, value):
            return fn()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'knn_cross_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, Gaussian clouds, q != x; microseconds per call: median of 7 rounds '
             '(min-max), the variants of a row alternating; indices and distances out']
    # (B, Nq, N, c, k, kind): 'same' rows also time the one-cloud search of that shape through the same kernels,
    # 'few' rows also time the unsplit schedule
    rows = [(32, 2048, 2048, 3, 20, 'same'), (32, 2048, 2048, 64, 20, 'same'), (32, 2048, 2048, 256, 20, 'same'),
            (32, 8192, 2048, 3, 3, ''), (1, 32, 1000000, 3, 16, 'few'), (1, 64, 200000, 256, 32, 'few')]
    for b, nq, n, c, k, kind in rows:
        q, x = torch.randn(b, c, nq, device=dev), torch.randn(b, c, n, device=dev)
        variants = {'cross': lambda: ops.hip_knn_cross(q, x, k, return_distance=True),
                    'torch': lambda: torch_knn_cross(q, x, k)}
        if kind == 'same':  # q = x: the same kernels and the same work as the one-cloud search (indices only, like it)
            variants['cross_xx'] = lambda: ops.hip_knn_cross(x, x, k)
            variants['self'] = with_switch('knn_wide', 1, lambda: ops.hip_knn(x, k))
        if kind == 'few':
            variants['unsplit'] = with_switch('knn_cross_split', 1, lambda: ops.hip_knn_cross(q, x, k, return_distance=True))
        t = medians(variants, iters=10 if b * nq * n >= 1 << 26 else 50)
        line = f'B={b:2d} Nq={nq:5d} N={n:8d} c={c:4d} k={k:3d}:'
        for name, label in (('cross', 'knn_cross'), ('torch', 'torch bmm+topk'), ('cross_xx', 'knn_cross(x, x)'),
                            ('self', 'pcc_knn(x), wide switch'),
                            ('unsplit', 'knn_cross, split forced to 1')):
            if name in t:
                med, lo, hi = t[name]
                line += f'  {label} {med:9.1f} ({lo:.1f}-{hi:.1f})'
        line += f'  [torch / cross {t["torch"][0] / t["cross"][0]:.1f}x'
        if 'self' in t:
            line += f', cross(x, x) / self {t["cross_xx"][0] / t["self"][0]:.3f}'
        if 'unsplit' in t:
            line += f', unsplit / split {t["unsplit"][0] / t["cross"][0]:.1f}x'
        line += ']'
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
