"""Timings of the ragged kernel map (neighbour_ops.cell_neighbours_ragged) and of the sparse convolution of a packed batch along it,
beside the torch formulation a user writes on the same GPU in the same process:
  map      hip: cell_neighbours_ragged(grid, K) -- one launch of cell_map_ragged<K>.  torch: the rows packed into int64 keys
           (c << 48 | i << 32 | j << 16 | k), the m * K^3 targets range-tested and packed, ONE torch.searchsorted over them, a gather
           and a mask.  The two maps are compared word for word before anything is timed.
  conv     hip: the map + sparse_conv_ragged (pcc_sparse_conv; backward: the same kernel on mirrored weights for the features,
           group_points + matmul per tap for the weight).  torch: the map above + group_points along it (the [m, K^3, C] tensor) + one
           matmul, the backward through autograd.  Forward, and forward + backward, at C = O = 64.
  for scale: the sparse_conv forward alone along a map that exists already.
Workloads (those of tools/time_grid_ragged.py, at its sizes): (i) 32 clouds of 2048 on the unit sphere, (ii) 32 clouds of 521-3992,
(iii) 8 clouds of 20884-54528, at size 0.05; (iv) one cloud of 100000 at sizes 0.05 and 0.02.  The level is
grid_pool_ragged(..., m=None): m = the occupied cells.  K = 3 and K = 5, dilation 1.
The variants of a row alternate round by round; a figure is the median over 7 rounds (min-max) of the mean time per call inside a
hipEvent bracket on the stream.  After every map row: microseconds per launch of the kernel from the library's launch profile, and the
rate at which it writes nbr (m * K^3 * 8 bytes).  No ratio is asserted: the tool writes what it measures, and marks a row the torch
form wins with ** **.  Output: profiles/cell_ragged_times.txt (or --out)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import _lib  # noqa: E402
from pointcloudcounterfactual_amd import neighbour_ops as ops  # noqa: E402
from time_knn_cross import medians  # noqa: E402

dev = torch.device('cuda:0')
C = 64


def torch_map(coord, ksize):
    m, h = coord.shape[0], (ksize - 1) // 2
    c = coord.long()
    key = (c[:, 0] << 48) | (c[:, 1] << 32) | (c[:, 2] << 16) | c[:, 3]
    d = torch.arange(-h, h + 1, device=coord.device)
    off = torch.stack(torch.meshgrid(d, d, d, indexing='ij'), -1).reshape(-1, 3)
    t = c[:, None, 1:] + off[None]
    inside = ((t >= 0) & (t < 65536)).all(-1)
    want = (c[:, None, 0] << 48) | (t[..., 0] << 32) | (t[..., 1] << 16) | t[..., 2]
    pos = torch.searchsorted(key, want.reshape(-1)).clamp(max=m - 1).view(m, -1)
    hit = inside & (key[pos] == want)
    return torch.where(hit, pos, torch.full((), -1, dtype=torch.int64, device=coord.device))


def torch_conv(x, nbr, weight, bias):
    """group_points along the map ([1, C, m, T], +0 in an empty tap) and one matmul."""
    m, taps = nbr.shape
    got = ops.group_points(x.t()[None], nbr[None])[0]  # [C, m, T]
    return got.permute(1, 2, 0).reshape(m, -1) @ weight.reshape(taps * weight.shape[1], -1) + bias


def backward_of(fn, leaves):
    def run():
        for t in leaves:
            t.grad = None
        fn().sum().backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cell_ragged_times.txt'))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    workloads = [('i', [2048] * 32, 0.05), ('ii', rng.integers(512, 4097, 32).tolist(), 0.05), ('iii', rng.integers(20000, 60001, 8).tolist(), 0.05),
                 ('iv', [100000], 0.05), ('iv', [100000], 0.02)]
    lines = [f'{torch.cuda.get_device_name(0)}, points on the unit sphere, seed 0; microseconds per call: median of 7 rounds (min-max), the variants '
             f'of a row alternating; C = O = {C}, dilation 1; hip = cell_neighbours_ragged (+ sparse_conv_ragged), torch = int64 keys + one searchsorted '
             '+ mask (+ group_points along the map + one matmul); a row torch wins is marked ** **']
    torch.manual_seed(0)
    for tag, sizes, size in workloads:
        b, n = len(sizes), sum(sizes)
        offset = torch.tensor(np.cumsum(sizes), device=dev)
        xyz = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1)
        grid = ops.grid_cluster_ragged(xyz, offset, size)
        coord, m = grid.coord, grid.coord.shape[0]
        x = torch.randn(m, C, device=dev).requires_grad_(True)
        for ksize in (3, 5):
            taps = ksize ** 3
            label = f'({tag}) B={b} n={n} size={size} m={m} K={ksize}'
            weight = (torch.randn(taps, C, C, device=dev) / (taps * C) ** 0.5).requires_grad_(True)
            bias = torch.randn(C, device=dev).requires_grad_(True)
            cmap = ops.cell_neighbours_ragged(grid, ksize)
            assert torch.equal(cmap.nbr[0], torch_map(coord, ksize)), label
            hip_conv = lambda: ops.sparse_conv_ragged(x, ops.cell_neighbours_ragged(grid, ksize), weight, bias)  # noqa: E731
            tor_conv = lambda: torch_conv(x, torch_map(coord, ksize), weight, bias)  # noqa: E731
            rows = [('map         ', {'hip': lambda: ops.cell_neighbours_ragged(grid, ksize), 'torch': lambda: torch_map(coord, ksize)}),
                    ('conv fwd    ', {'hip': hip_conv, 'torch': tor_conv}),
                    ('conv fwd+bwd', {'hip': backward_of(hip_conv, (x, weight, bias)), 'torch': backward_of(tor_conv, (x, weight, bias))})]
            results = {}
            for what, variants in rows:
                t = medians(variants, iters=3, rounds=7, warm=2)
                results[what] = t
                ratio = t['torch'][0] / t['hip'][0]
                mark = '**' if ratio < 1 else ''
                line = f'{mark}{label} {what}:'
                for name, v in t.items():
                    line += f'  {name} {v[0]:10.1f} ({v[1]:.1f}-{v[2]:.1f})'
                line += f'  [torch / hip {ratio:.2f}x]{mark}'
                print(line, flush=True)
                lines.append(line)
            t = medians({'sparse_conv': lambda: ops.sparse_conv_ragged(x.detach(), cmap, weight.detach(), bias.detach())}, iters=3, rounds=7, warm=2)
            alone, whole = t['sparse_conv'], results['map         ']['hip']
            with _lib.profile() as read:
                for _ in range(5):
                    ops.cell_neighbours_ragged(grid, ksize)
                torch.cuda.synchronize()
                us, count = read(f'cell_map_ragged<{ksize}>')
            line = (f'    {label} for scale: sparse_conv fwd alone {alone[0]:.1f} ({alone[1]:.1f}-{alone[2]:.1f}); the map call is {whole[0] / alone[0]:.2f}x of it; '
                    f'cell_map_ragged<{ksize}> {us:.1f} us per launch x {count}: nbr written at {m * taps * 8 / us / 1e3:.0f} GB/s')
            print(line, flush=True)
            lines.append(line)
            del weight, bias, cmap
            torch.cuda.empty_cache()
        del xyz, x, grid
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
