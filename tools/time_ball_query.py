"""Timings of the ball query (pcc_ball_query, ball_query.hip) beside what a user would write without it, on the same GPU in
the same process:
  (a) dense   the dense torch formulation of the set-abstraction layers: a [B,M,N] distance tensor (bmm, expanded form), an
              index tensor of the same size with the points outside set to N, a sort along N, the first nsample columns, the
              padding with the first column (for B = 32, N = 15000 in chunks of 4 clouds: the tensors of the whole batch
              would take tens of GB);
  (b) knn     knn_cross(k = min(nsample, 128)) and a distance mask: ANOTHER answer (the nearest, not the first in index
              order), timed only as the cost of the nearest alternative inside the library.
With --paths every kernel variant is timed too (the ball_path switch of include/pcc_test_hooks.h).  The variants of a row
alternate round by round; a figure is the median over 7 rounds of the mean time per call inside a hipEvent bracket on the
stream.  Clouds are points on the unit sphere (a surface); centres are their farthest point samples.  `scanned` is the mean
over the queries of (index of the last candidate a query needs + 1) / N: 1 for a query whose list does not fill.
Output: profiles/ball_query_times.txt (or --out)."""
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
PATHS = {1: 'direct/4', 2: 'direct/16', 3: 'lds/4x1024', 4: 'lds/16x4096'}


def dense_ball_query(xyz, centres, radius, nsample, chunk):
    """The dense formulation, `chunk` clouds at a time."""
    out = []
    n = xyz.shape[1]
    for b0 in range(0, xyz.shape[0], chunk):
        x, c = xyz[b0:b0 + chunk], centres[b0:b0 + chunk]
        d = -2 * torch.bmm(c, x.transpose(1, 2)) + (c ** 2).sum(-1)[:, :, None] + (x ** 2).sum(-1)[:, None, :]
        group = torch.arange(n, device=x.device).view(1, 1, n).repeat(c.shape[0], c.shape[1], 1)
        group[d >= radius * radius] = n
        group = group.sort(dim=-1)[0][:, :, :nsample]
        first = group[:, :, :1].expand(-1, -1, group.shape[2])
        out.append(torch.where(group == n, first, group))
    return torch.cat(out)


def knn_and_mask(q_cm, x_cm, radius, k):
    idx, dist = ops.hip_knn_cross(q_cm, x_cm, k, return_distance=True)
    return torch.where(dist < radius * radius, idx, idx[..., :1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ball_query_times.txt'))
    ap.add_argument('--paths', action='store_true', help='also time every kernel variant')
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, points on the unit sphere xyz[B,N,3], M centres by farthest point sampling, indices and '
             'counts out; microseconds per call: median of 7 rounds (min-max), the variants of a row alternating']
    # (B, N, M, nsample, radius); the last row: a radius below the spacing of the points, so no list fills and every query
    # scans the whole cloud
    rows = [(32, 2048, 512, 32, 0.2), (32, 2048, 128, 64, 0.4), (32, 15000, 2048, 32, 0.1), (1, 15000, 2048, 32, 0.1),
            (32, 2048, 512, 32, 1e-4)]
    for b, n, m, nsample, radius in rows:
        xyz = torch.nn.functional.normalize(torch.randn(b, n, 3, device=dev), dim=-1)
        centres = torch.gather(xyz, 1, ops.farthest_point_sample(xyz, m)[:, :, None].expand(-1, -1, 3)).contiguous()
        q_cm, x_cm = centres.transpose(1, 2).contiguous(), xyz.transpose(1, 2).contiguous()
        k = min(nsample, 128)
        chunk = 4 if b * m * n > 1 << 28 else b
        variants = {'ball': lambda: ops.ball_query(xyz, centres, radius, nsample, return_count=True),
                    'dense': lambda: dense_ball_query(xyz, centres, radius, nsample, chunk),
                    'knn': lambda: knn_and_mask(q_cm, x_cm, radius, k)}
        if args.paths:
            for path in PATHS:
                variants[path] = with_switch('ball_path', path, lambda: ops.ball_query(xyz, centres, radius, nsample, return_count=True))
        big = b * m * n > 1 << 28
        t = medians(variants, iters=1 if big else 10, rounds=7, warm=1 if big else 3)
        idx, cnt = ops.ball_query(xyz, centres, radius, nsample, return_count=True)
        last = torch.where(cnt == nsample, idx[..., -1] + 1, torch.full_like(idx[..., -1], n))
        line = (f'B={b:2d} N={n:5d} M={m:4d} nsample={nsample:2d} r={radius:g}:  ball_query {t["ball"][0]:9.1f} ({t["ball"][1]:.1f}-{t["ball"][2]:.1f})'
                f'  dense torch {t["dense"][0]:11.1f} ({t["dense"][1]:.1f}-{t["dense"][2]:.1f})'
                f'  knn_cross(k={k})+mask {t["knn"][0]:9.1f} ({t["knn"][1]:.1f}-{t["knn"][2]:.1f})'
                f'  [dense / ball {t["dense"][0] / t["ball"][0]:.0f}x, knn / ball {t["knn"][0] / t["ball"][0]:.1f}x; '
                f'scanned {last.double().mean().item() / n:.3f}, full lists {(cnt == nsample).double().mean().item():.3f}, '
                f'mean cnt {cnt.double().mean().item():.1f}]')
        if args.paths:
            line += '  variants:' + ''.join(f' {PATHS[p]} {t[p][0]:.1f}' for p in PATHS)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
