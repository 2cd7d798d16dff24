"""Timings of the sliced Wasserstein loss (pcc_sliced_wasserstein, sliced_wasserstein.hip) beside what a user writes
without it, on the same GPU in the same process:
  torch   the projection of both clouds as one matmul each, two torch.sort over [B,P,N], the difference of the sorted
          values, its square and a mean; the backward through autograd (a gather and a scatter per cloud).
Clouds are Gaussian [B,N,3], the directions P normalised Gaussian rows shared by the batch.  `fwd` is the forward alone
(no gradient asked for: the library takes its cost-only kernel), `f+b` the forward and the backward of both clouds from
`loss.sum()`.  At N = 2048 the other variant that holds the cloud (256 threads with 8 elements each, the sw_path switch of
include/pcc_test_hooks.h) is timed beside the product's (512 threads with 4).  The variants of a row alternate round by
round; a figure is the median over 7 rounds of the mean time per call inside a hipEvent bracket on the stream.  `kernels`
are the library's own per-launch averages (pcc_profile_enable(1): one event pair around each launch) over 5 further
forward + backward calls.  The last row puts match_cost and chamfer at (32, 2048) in the same table for scale.
Output: profiles/sliced_wasserstein_times.txt (or --out)."""
import argparse
import os
import sys

os.environ.setdefault('PCC_TEST_HOOKS', '1')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import _lib, losses  # noqa: E402
from time_knn_cross import medians, with_switch  # noqa: E402

dev = torch.device('cuda:0')


def torch_sw(x, y, theta):
    a = torch.sort(torch.matmul(x, theta.t()).transpose(1, 2), dim=2)[0]
    b = torch.sort(torch.matmul(y, theta.t()).transpose(1, 2), dim=2)[0]
    return ((a - b) ** 2).mean((1, 2))


def kernel_times(run):
    text = ''
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name, label in (('sw_slice_kernel', 'slices'), ('sw_finish_kernel', 'finish')):
            us, cnt = read(name)
            if cnt:
                text += f' {label} {us:.1f}'
    return text


def fwd(fn, *args):
    def run():
        with torch.no_grad():
            return fn(*[a.detach() if isinstance(a, torch.Tensor) else a for a in args])
    return run


def fwd_bwd(fn, x, y, *rest):
    def run():
        x.grad = None
        y.grad = None
        fn(x, y, *rest).sum().backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sliced_wasserstein_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, Gaussian clouds x, y [B,N,3], P unit directions shared by the batch; microseconds '
             'per call: median of 7 rounds (min-max), the variants of a row alternating']
    for b, n, p in ((32, 2048, 128), (32, 2048, 32), (32, 8192, 128), (1, 2048, 128)):
        x = torch.randn(b, n, 3, device=dev).requires_grad_(True)
        y = (torch.randn(b, n, 3, device=dev) * 0.8 + 0.1).requires_grad_(True)
        theta = losses.random_directions(p, dev)
        with torch.no_grad():  # the two formulations agree before they are timed
            assert torch.allclose(losses.sliced_wasserstein(x, y, directions=theta), torch_sw(x, y, theta), rtol=1e-4, atol=1e-6)

        def ours(x, y, theta):
            return losses.sliced_wasserstein(x, y, directions=theta)

        variants = {'ours_fwd': fwd(ours, x, y, theta), 'torch_fwd': fwd(torch_sw, x, y, theta),
                    'ours_fb': fwd_bwd(ours, x, y, theta), 'torch_fb': fwd_bwd(torch_sw, x, y, theta)}
        if n == 2048:  # the other variant that holds 2048 points: 256 threads with 8 elements each (sw_path 9)
            variants['e8_fwd'] = with_switch('sw_path', 9, variants['ours_fwd'])
            variants['e8_fb'] = with_switch('sw_path', 9, variants['ours_fb'])
        t = medians(variants, iters=5 if b * n * p > 1 << 24 else 20, rounds=7, warm=2)
        line = f'B={b:2d} N={n:5d} P={p:3d}:'
        for key, label in (('ours_fwd', 'fwd'), ('torch_fwd', 'torch fwd'), ('ours_fb', 'f+b'), ('torch_fb', 'torch f+b')):
            line += f'  {label} {t[key][0]:9.1f} ({t[key][1]:.1f}-{t[key][2]:.1f})'
        line += f'  [torch / ours: fwd {t["torch_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["torch_fb"][0] / t["ours_fb"][0]:.2f}x]'
        if 'e8_fb' in t:
            line += f'  256 threads x 8: fwd {t["e8_fwd"][0]:.1f} f+b {t["e8_fb"][0]:.1f}'
        line += '  kernels (f+b):' + kernel_times(variants['ours_fb'])
        print(line, flush=True)
        lines.append(line)
    b, n = 32, 2048
    x = torch.randn(b, n, 3, device=dev).requires_grad_(True)
    y = (torch.randn(b, n, 3, device=dev) * 0.8 + 0.1).requires_grad_(True)
    theta = losses.random_directions(128, dev)
    variants = {}
    for name, fn, rest in (('sliced_wasserstein P=128', losses.sliced_wasserstein, (128, theta)), ('match_cost', losses.match_cost, ()),
                           ('chamfer', losses.chamfer, ())):
        variants[name + ' fwd'], variants[name + ' f+b'] = fwd(fn, x, y, *rest), fwd_bwd(fn, x, y, *rest)
    t = medians(variants, iters=10, rounds=7, warm=2)
    line = f'for scale, B={b} N={n}:'
    for key, (med, lo, hi) in t.items():
        line += f'  {key} {med:.1f} ({lo:.1f}-{hi:.1f})'
    print(line, flush=True)
    lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
