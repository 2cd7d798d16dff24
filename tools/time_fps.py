"""Timings of farthest point sampling (pcc_fps, fps.hip) beside the torch loop a user would write without it, on the same
GPU in the same process: per step the distances to the last pick, the running minimum and an argmax, every cloud of the
batch at once.  The two alternate round by round; a figure is the median over 7 rounds of the mean time per call inside a
hipEvent bracket on the stream.  With --paths every kernel variant that holds the shape is timed as well (the fps_path
switch of include/pcc_test_hooks.h): the figures the (block, P) table of DESIGN.md section 4d rests on.
Output: profiles/fps_times.txt (or --out)."""
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
PATHS = {1: ('64x4', 256), 2: ('256x4', 1024), 3: ('256x8', 2048), 4: ('512x8', 4096), 5: ('1024x8', 8192),
         6: ('1024x16', 16384), 7: ('memory', None)}


def torch_fps(xyz, m):
    """The loop without the library: about five small launches per selected point."""
    b, n, _ = xyz.shape
    rows = torch.arange(b, device=xyz.device)
    mind = torch.full((b, n), float('inf'), device=xyz.device)
    idx = torch.zeros((b, m), dtype=torch.int64, device=xyz.device)
    sel = torch.zeros(b, dtype=torch.int64, device=xyz.device)
    for t in range(m):
        idx[:, t] = sel
        d = ((xyz - xyz[rows, sel][:, None, :]) ** 2).sum(-1)
        mind = torch.minimum(mind, d)
        sel = mind.argmax(1)
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fps_times.txt'))
    ap.add_argument('--paths', action='store_true', help='also time every kernel variant that holds the shape')
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, Gaussian clouds xyz[B,N,3], m samples, indices and distances out; milliseconds per '
             'call: median of 7 rounds (min-max), fps and the torch loop alternating; us/pick = fps time / m']
    for b, n, m in ((32, 15000, 2048), (32, 2048, 512), (256, 2048, 1024), (1, 15000, 2048)):
        xyz = torch.randn(b, n, 3, device=dev)
        variants = {'fps': lambda: ops.farthest_point_sample(xyz, m, return_distance=True), 'torch': lambda: torch_fps(xyz, m)}
        if args.paths:
            for path, (_, cap) in PATHS.items():
                if cap is None or cap >= n:
                    variants[path] = with_switch('fps_path', path, lambda: ops.farthest_point_sample(xyz, m, return_distance=True))
        t = medians(variants, iters=1, rounds=7, warm=1)
        ms = {name: tuple(v / 1e3 for v in val) for name, val in t.items()}
        line = (f'B={b:3d} N={n:5d} m={m:4d}:  fps {ms["fps"][0]:8.3f} ({ms["fps"][1]:.3f}-{ms["fps"][2]:.3f})  '
                f'torch loop {ms["torch"][0]:8.2f} ({ms["torch"][1]:.2f}-{ms["torch"][2]:.2f})  '
                f'[torch / fps {t["torch"][0] / t["fps"][0]:.1f}x, {t["fps"][0] / m:.2f} us/pick]')
        if args.paths:
            line += '  variants:' + ''.join(f' {PATHS[p][0]} {ms[p][0]:.3f}' for p in PATHS if p in ms)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
