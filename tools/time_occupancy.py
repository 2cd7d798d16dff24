"""Timings of the voxel occupancy counts (pcc_occupancy_grid, occupancy.hip) beside the torch formulation a user would
write without it, on the same GPU in the same process: the separable cell rule as elementwise ops, then bincount (it
has no in_sphere form: beside an in_sphere row it is the same full-grid computation).  Every row also times the library's
two paths through the occupancy_path switch of include/pcc_test_hooks.h: the global-atomic path, and the LDS histogram
where the grid fits (res <= 32).  The variants of a row alternate round by round; a figure is the median over 7 rounds of
the mean time per call inside a hipEvent bracket on the stream.  Output: profiles/occupancy_times.txt (or --out)."""
import argparse
import os
import sys

os.environ.setdefault('PCC_TEST_HOOKS', '1')  # the A/B switches of include/pcc_test_hooks.h

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import set_metrics as sm  # noqa: E402
from time_knn_cross import medians, with_switch  # noqa: E402

dev = torch.device('cuda:0')


def torch_occupancy(clouds, res, per_cloud, lo=-0.5, extent=1.0):
    """Without the library: six elementwise launches, an index computation and bincount's own atomics."""
    s = clouds.size(0)
    ijk = torch.floor((clouds - lo) * ((res - 1) / extent) + 0.5).clamp(0, res - 1).long()
    flat = (ijk[..., 0] * res + ijk[..., 1]) * res + ijk[..., 2]
    if per_cloud:
        flat = flat + torch.arange(s, device=clouds.device)[:, None] * res ** 3
        return torch.bincount(flat.reshape(-1), minlength=s * res ** 3).view(s, res, res, res)
    return torch.bincount(flat.reshape(-1), minlength=res ** 3).view(res, res, res)


def bank(kind, s, n):
    if kind == 'uniform':  # [-0.7, 0.7]^3: at res 28 about four points in five leave their separable cell with in_sphere
        return torch.rand(s, n, 3, device=dev) * 1.4 - 0.7
    x = torch.randn(s, n, 3, device=dev) * 0.2  # 'normalised': every cloud scaled into the inscribed sphere
    return x / x.norm(dim=2).amax(dim=1)[:, None, None] * 0.499


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'occupancy_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, clouds[S,N,3], int64 counts out; microseconds per call: median of 7 rounds (min-max), the '
             'variants of a row alternating; occupancy = the product\'s choice of path, global / LDS = that path forced']
    # (kind, S, N, res, in_sphere, per_cloud)
    rows = [('normalised', 128, 2048, 28, False, False), ('normalised', 128, 2048, 28, True, False),
            ('normalised', 400, 2048, 28, False, False), ('normalised', 400, 2048, 28, True, False),
            ('uniform', 400, 2048, 28, True, False), ('normalised', 400, 2048, 28, False, True),
            ('normalised', 400, 2048, 64, False, False)]
    for kind, s, n, res, in_sphere, per_cloud in rows:
        x = bank(kind, s, n)

        def run():
            return sm.occupancy_grid(x, res, in_sphere, per_cloud)

        variants = {'occupancy': run, 'torch': lambda: torch_occupancy(x, res, per_cloud), 'global': with_switch('occupancy_path', 1, run)}
        if res <= 32:
            variants['LDS'] = with_switch('occupancy_path', 2, run)
        if not in_sphere:
            assert torch.equal(run(), torch_occupancy(x, res, per_cloud))
        t = medians(variants, iters=20)
        line = f'{kind:10s} S={s:3d} N={n:4d} res={res:2d} in_sphere={int(in_sphere)} per_cloud={int(per_cloud)}:'
        for name in ('occupancy', 'torch', 'global', 'LDS'):
            if name in t:
                med, lo, hi = t[name]
                line += f'  {name} {med:7.1f} ({lo:.1f}-{hi:.1f})'
        line += f'  [torch / occupancy {t["torch"][0] / t["occupancy"][0]:.1f}x'
        if 'LDS' in t:
            line += f', global / LDS {t["global"][0] / t["LDS"][0]:.2f}'
        line += ']'
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
