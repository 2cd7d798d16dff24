"""Timings of the Sinkhorn divergence (pcc_sinkhorn, sinkhorn.hip) beside what a user writes without it, on the same GPU
in the same process:
  torch   the dense formulation of the same iteration: the cost matrices [B,N,M] once per call from the expanded form
          (torch.bmm), every smoothed minimum a torch.logsumexp over a [B,N,M] temporary, the T + 1 rounds before the last
          under no_grad, autograd through the last round only (the library's gradient convention).
Clouds are Gaussian x [B,N,3], y [B,M,3]; the schedule is the default one, sinkhorn_schedule(0.05, 0.5, diameter) with the
diameter measured once outside the timed region (8 temperatures, 10 all-pairs rounds).  `fwd` is the forward alone (no
gradient asked for), `f+b` the forward and the backward of both clouds from `loss.sum()`; `debias` on = the divergence
(four scans per round), off = the plain entropic cost (two).  At (32, 8192, 8192) the dense formulation is timed at B = 4,
where its temporaries fit comfortably, and the library at both B.  Where the library cuts the columns into slices, the
unsplit schedule (the sinkhorn_split switch of include/pcc_test_hooks.h at 1) is timed beside the product's.  The variants
of a row alternate round by round; a figure is the median over 7 rounds of the mean time per call inside a hipEvent
bracket on the stream.  `kernels` are the library's own per-launch averages (pcc_profile_enable(1)) over 5 further
debiased forward + backward calls.  The last row puts match_cost, sliced_wasserstein and chamfer at (32, 2048) in the same
table for scale.
Output: profiles/sinkhorn_times.txt (or --out)."""
import argparse
import math
import os
import sys

os.environ.setdefault('PCC_TEST_HOOKS', '1')

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import _lib, losses  # noqa: E402
from time_knn_cross import medians, with_switch  # noqa: E402
from time_sliced_wasserstein import fwd, fwd_bwd  # noqa: E402

dev = torch.device('cuda:0')


def pair_cost(u, v):
    return 0.5 * ((u * u).sum(-1)[:, :, None] + (v * v).sum(-1)[:, None, :] - 2 * torch.bmm(u, v.transpose(1, 2)))


def softmin(e, c, h):
    return -e * torch.logsumexp((h[:, None, :] - c) / e - math.log(c.size(2)), dim=2)


def torch_sinkhorn_dense(x, y, eps, debias):
    with torch.no_grad():
        scans = [(pair_cost(x, y), 1), (pair_cost(y, x), 0)] + ([(pair_cost(x, x), 2), (pair_cost(y, y), 3)] if debias else [])
        pots = [softmin(eps[0], c, torch.zeros_like(c[:, 0, :])) for c, _ in scans]
        for e in eps:
            pots = [0.5 * (h + softmin(e, c, pots[src])) for h, (c, src) in zip(pots, scans)]
    e, xd, yd = eps[-1], x.detach(), y.detach()
    cost = softmin(e, pair_cost(x, yd), pots[1]).mean(1) + softmin(e, pair_cost(y, xd), pots[0]).mean(1)
    if debias:
        cost = cost - softmin(e, pair_cost(x, xd), pots[2]).mean(1) - softmin(e, pair_cost(y, yd), pots[3]).mean(1)
    return cost


def kernel_times(run):
    text = ''
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name, label in (('sk_scan_kernel', 'round'), ('sk_merge_kernel', 'merge'), ('sk_scan_final_kernel', 'final round'),
                            ('sk_combine_kernel', 'combine'), ('sk_cost_kernel', 'cost')):
            us, cnt = read(name)
            if cnt:
                text += f' {label} {us:.1f}'
    return text


def clouds(b, n, m):
    x = torch.randn(b, n, 3, device=dev).requires_grad_(True)
    y = (torch.randn(b, m, 3, device=dev) * 0.8 + 0.3).requires_grad_(True)
    return x, y


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sinkhorn_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, Gaussian clouds x [B,N,3], y [B,M,3], sinkhorn_schedule(0.05, 0.5, diameter): 8 temperatures, '
             '10 rounds; microseconds per call: median of 7 rounds (min-max), the variants of a row alternating']
    for b, n, m, tb in ((32, 2048, 2048, 32), (32, 2048, 1024, 32), (1, 2048, 2048, 1), (32, 8192, 8192, 4)):
        x, y = clouds(b, n, m)
        both = torch.cat((x.detach().reshape(-1, 3), y.detach().reshape(-1, 3)))
        eps = losses.sinkhorn_schedule(0.05, 0.5, float((both.max(0).values - both.min(0).values).max()))
        tx, ty = (x, y) if tb == b else (x.detach()[:tb].clone().requires_grad_(True), y.detach()[:tb].clone().requires_grad_(True))
        for debias in (True, False):  # the two formulations agree before they are timed
            ours = losses.sinkhorn_divergence(tx, ty, eps=eps, debias=debias)
            dense = torch_sinkhorn_dense(tx, ty, eps, debias)
            assert torch.allclose(ours, dense, rtol=2e-3, atol=2e-4), (ours, dense)
            g_ours = torch.autograd.grad(ours.sum(), tx)[0]
            g_dense = torch.autograd.grad(dense.sum(), tx)[0]
            assert torch.allclose(g_ours, g_dense, rtol=1e-2, atol=1e-2 * float(g_dense.abs().max())), (g_ours - g_dense).abs().max()
            del ours, dense, g_ours, g_dense
        split = True  # (split_for cuts every shape of this table into column slices)
        line = f'B={b:2d} N={n:5d} M={m:5d}:'
        for debias in (True, False):
            def ours(x, y, debias=debias):
                return losses.sinkhorn_divergence(x, y, eps=eps, debias=debias)

            def dense(x, y, debias=debias):
                return torch_sinkhorn_dense(x, y, eps, debias)

            variants = {'ours_fwd': fwd(ours, x, y), 'torch_fwd': fwd(dense, tx, ty), 'ours_fb': fwd_bwd(ours, x, y), 'torch_fb': fwd_bwd(dense, tx, ty)}
            if tb != b:
                variants['small_fwd'], variants['small_fb'] = fwd(ours, tx, ty), fwd_bwd(ours, tx, ty)
            if split:
                variants['s1_fwd'] = with_switch('sinkhorn_split', 1, variants['ours_fwd'])
                variants['s1_fb'] = with_switch('sinkhorn_split', 1, variants['ours_fb'])
            t = medians(variants, iters=3 if n * m * b > 1 << 22 else 10, rounds=7, warm=1)
            line += f'  debias {"on" if debias else "off"}:'
            for key, label in (('ours_fwd', 'fwd'), ('ours_fb', 'f+b'), ('small_fwd', f'fwd at B={tb}'), ('small_fb', f'f+b at B={tb}'),
                               ('torch_fwd', f'torch fwd at B={tb}'), ('torch_fb', f'torch f+b at B={tb}'), ('s1_fwd', 'unsplit fwd'), ('s1_fb', 'unsplit f+b')):
                if key in t:
                    line += f'  {label} {t[key][0]:.1f} ({t[key][1]:.1f}-{t[key][2]:.1f})'
            base = 'small' if tb != b else 'ours'
            line += f'  [torch / ours at B={tb}: fwd {t["torch_fwd"][0] / t[base + "_fwd"][0]:.2f}x, f+b {t["torch_fb"][0] / t[base + "_fb"][0]:.2f}x]'
            if debias:
                kern = kernel_times(variants['ours_fb'])
        line += '  kernels (debias on, f+b):' + kern
        print(line, flush=True)
        lines.append(line)
        del x, y, tx, ty, variants
        torch.cuda.empty_cache()
    b, n = 32, 2048
    x, y = clouds(b, n, n)
    theta = losses.random_directions(128, dev)
    variants = {}
    for name, fn, rest in (('sinkhorn_divergence (diameter 8)', lambda x, y: losses.sinkhorn_divergence(x, y, diameter=8.0), ()),
                           ('match_cost', losses.match_cost, ()), ('sliced_wasserstein P=128', losses.sliced_wasserstein, (128, theta)),
                           ('chamfer', losses.chamfer, ())):
        variants[name + ' fwd'], variants[name + ' f+b'] = fwd(fn, x, y, *rest), fwd_bwd(fn, x, y, *rest)
    t = medians(variants, iters=5, rounds=7, warm=2)
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
