"""Timings of the grouping op (pcc_group_points / pcc_group_points_bwd, grouping.hip) beside what a user would write
without it, on the same GPU in the same process:
  torch   the composition of INTEGRATION.md before the op existed: the index list expanded to every channel, a gather per
          input, the subtraction of the centres, a cat; the backward through autograd (scatter_add with global float atomics).
Clouds are points on the unit sphere xyz[B,N,3] with Gaussian features[B,C,N]; centres are their farthest point samples and
the lists come from ball_query (pad = 'first'), so the op fills a [B,3+C,M,k] tensor in two calls (relative coordinates,
then the features); the last row groups the features alone along a knn_cross list of M other points (no centres).  At
radius 1e-4 every ball holds its centre only: every row is one index repeated.  `fwd` is the forward alone, `f+b` the
forward and the backward of all inputs (xyz, centres, features) from a fixed incoming gradient.  Both paths are forced
against each other through the group_path switch of include/pcc_test_hooks.h (lds / direct).  The variants of a row
alternate round by round; a figure is the median over 7 rounds of the mean time per call inside a hipEvent bracket on the
stream.  `write` is the forward's output stream, B * (3 + C) * M * k * 4 bytes, over the forward's time, and its share of
the 8 TB/s HBM peak.  Output: profiles/grouping_times.txt (or --out)."""
import argparse
import os
import sys

os.environ.setdefault('PCC_TEST_HOOKS', '1')  # the A/B switches of include/pcc_test_hooks.h

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import neighbour_ops as ops  # noqa: E402
from time_knn_cross import medians, with_switch  # noqa: E402

dev = torch.device('cuda:0')
HBM_PEAK = 8.0e12  # bytes per second


def torch_group(xyz, centres, feats, idx):
    """What a user writes without the op; `xyz` / `centres` None: the features alone."""
    b, m, k = idx.shape
    parts = []
    if xyz is not None:
        nb = xyz.gather(1, idx.reshape(b, m * k, 1).expand(-1, -1, 3)).view(b, m, k, 3)
        parts.append((nb - centres[:, :, None, :]).permute(0, 3, 1, 2))
    if feats is not None:
        c = feats.shape[1]
        parts.append(feats.gather(2, idx.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k))
    return torch.cat(parts, 1) if len(parts) > 1 else parts[0].contiguous()


def ours_group(xyz, centres, feats, idx):
    parts = (() if xyz is None else (xyz, centres, True)) + (() if feats is None else (feats, None, False))
    return ops.Grouped.apply(idx, *parts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grouping_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, points on the unit sphere xyz[B,N,3], features[B,C,N], M centres by farthest point '
             'sampling, lists by ball_query (pad first); out [B,3+C,M,k]; microseconds per call: median of 7 rounds (min-max), the '
             'variants of a row alternating']
    # (B, N, M, k, C, radius); radius None: a knn_cross list of M other points, the features alone
    rows = [(32, 2048, 512, 32, 64, 0.2), (32, 2048, 512, 32, 64, 1e-4), (32, 15000, 2048, 32, 64, 0.1), (32, 2048, 128, 64, 128, 0.4),
            (1, 15000, 2048, 32, 64, 0.1), (32, 2048, 8192, 3, 64, None)]
    for b, n, m, k, c, radius in rows:
        xyz = torch.nn.functional.normalize(torch.randn(b, n, 3, device=dev), dim=-1)
        feats = torch.randn(b, c, n, device=dev)
        if radius is None:
            q = torch.nn.functional.normalize(torch.randn(b, 3, m, device=dev), dim=1)
            idx = ops.knn_cross(q, xyz.transpose(1, 2).contiguous(), k)
            leaves = [None, None, feats.clone().requires_grad_(True)]
            out_c, note = c, 'knn_cross list, no centres'
        else:
            centres = torch.gather(xyz, 1, ops.farthest_point_sample(xyz, m)[:, :, None].expand(-1, -1, 3)).contiguous()
            idx, cnt = ops.ball_query(xyz, centres, radius, k, return_count=True)
            leaves = [xyz.clone().requires_grad_(True), centres.clone().requires_grad_(True), feats.clone().requires_grad_(True)]
            out_c, note = 3 + c, f'r={radius:g}, mean cnt {cnt.double().mean().item():.1f}'
        grad = torch.randn(b, out_c, m, k, device=dev)
        with torch.no_grad():  # the two formulations agree before they are timed
            assert torch.equal(ours_group(*leaves, idx), torch_group(*leaves, idx))

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn(*leaves, idx)
            return run

        def fwd_bwd(fn):
            def run():
                for t in leaves:
                    if t is not None:
                        t.grad = None
                fn(*leaves, idx).backward(grad)
            return run

        variants = {'fwd': fwd(ours_group), 'torch_fwd': fwd(torch_group), 'fb': fwd_bwd(ours_group), 'torch_fb': fwd_bwd(torch_group)}
        for path, name in ((1, 'lds'), (2, 'direct')):
            variants[name + '_fwd'] = with_switch('group_path', path, fwd(ours_group))
            variants[name + '_fb'] = with_switch('group_path', path, fwd_bwd(ours_group))
        big = b * out_c * m * k > 1 << 27
        t = medians(variants, iters=3 if big else 10, rounds=7, warm=2)
        nbytes = b * out_c * m * k * 4
        rate = nbytes / (t['fwd'][0] * 1e-6)
        line = f'B={b:2d} N={n:5d} M={m:4d} k={k:2d} C={c:3d} ({note}):'
        for key, label in (('fwd', 'fwd'), ('torch_fwd', 'torch fwd'), ('fb', 'f+b'), ('torch_fb', 'torch f+b')):
            line += f'  {label} {t[key][0]:9.1f} ({t[key][1]:.1f}-{t[key][2]:.1f})'
        line += (f'  [torch / ours: fwd {t["torch_fwd"][0] / t["fwd"][0]:.1f}x, f+b {t["torch_fb"][0] / t["fb"][0]:.1f}x; '
                 f'write {nbytes / 1e6:.0f} MB at {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f}% of peak]'
                 f'  paths: lds fwd {t["lds_fwd"][0]:.1f} f+b {t["lds_fb"][0]:.1f}, direct fwd {t["direct_fwd"][0]:.1f} f+b {t["direct_fb"][0]:.1f}')
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
