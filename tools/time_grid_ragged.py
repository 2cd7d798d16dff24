"""Timings of the ragged grid index and pooling (neighbour_ops.grid_cluster_ragged / grid_pool_ragged) beside the torch formulation
a Pointcept user writes on the same GPU in the same process:
  torch    key = (batch, div(xyz - start, size, rounding_mode='trunc')) packed into an int64, torch.unique(key, sorted=True,
           return_inverse=True, return_counts=True) (a device-wide sort and a host synchronisation), then index_add_ and a division for
           the mean of the coordinates and of the features; the backward through autograd.
  hip      grid_cluster_ragged(..., start, m=None): the kernels plus the one host read of the cell count, the outputs cut to U slots;
           grid_pool_ragged on top (segment_pool with b = 1).
  hip_pad  the index alone at m = n: no synchronisation, padded.
Both sides get `start` (and torch its `batch` vector) precomputed.  Columns: the index alone, index + pooling forward, and forward +
backward, at c = 64 channels, reduce = 'mean'.  Workloads (those of tools/time_ragged_search.py): (i) 32 clouds of 2048 on the unit
sphere, (ii) 32 clouds of 521-3992, (iii) 8 clouds of 20884-54528, at size 0.05; (iv) one cloud of 100000 at sizes 0.05 and 0.02.  Each
at the default axis_bits and at axis_bits = 10.  For scale, the rectangular grid_pool on workload (i) (resolution 40 over [-1, 1]).
The variants of a row alternate round by round; a figure is the median over 7 rounds (min-max) of the mean time per call inside a
hipEvent bracket on the stream.  After every default-axis_bits row: microseconds per launch and launches of every kernel of one index
call (the library's launch profile).  No ratio is asserted: the tool writes what it measures, and marks a row the torch form wins
with ** **.  Output: profiles/grid_ragged_times.txt (or --out)."""
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
KERNELS = ('rg_key_kernel', 'rg_hist_kernel', 'rg_scan_reduce_kernel', 'rg_scan_partials_kernel', 'rg_scan_down_kernel', 'rg_scatter_kernel',
           'rg_heads_kernel', 'rg_bounds_kernel', 'rg_emit_kernel')


def torch_index(xyz, batch, start, size):
    q = torch.div(xyz - start[batch], size, rounding_mode='trunc').long()
    key = (batch << 48) | (q[:, 0] << 32) | (q[:, 1] << 16) | q[:, 2]
    return torch.unique(key, sorted=True, return_inverse=True, return_counts=True)


def torch_pool(xyz, feats, batch, start, size):
    unique, inverse, counts = torch_index(xyz.detach(), batch, start, size)
    m = unique.shape[0]
    inv = counts.to(torch.float32)[:, None]
    centres = torch.zeros((m, 3), device=dev).index_add_(0, inverse, xyz) / inv
    pooled = torch.zeros((m, feats.shape[1]), device=dev).index_add_(0, inverse, feats) / inv
    return centres, pooled


def backward_of(fn, xyz, feats):
    def run():
        xyz.grad = feats.grad = None
        centres, pooled = fn()
        (centres.sum() + pooled.sum()).backward()
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grid_ragged_times.txt'))
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    workloads = [('i', [2048] * 32, 0.05), ('ii', rng.integers(512, 4097, 32).tolist(), 0.05), ('iii', rng.integers(20000, 60001, 8).tolist(), 0.05),
                 ('iv', [100000], 0.05), ('iv', [100000], 0.02)]
    lines = [f'{torch.cuda.get_device_name(0)}, points on the unit sphere, seed 0; microseconds per call: median of 7 rounds (min-max), the variants '
             f'of a row alternating; c = {C}, mean; torch = int64 key + torch.unique(sorted, inverse, counts) + index_add_, hip = '
             'grid_cluster_ragged / grid_pool_ragged with m=None (one host read), hip_pad = the index at m = n (no host read); a row torch wins is '
             'marked ** **']
    torch.manual_seed(0)
    for tag, sizes, size in workloads:
        b, n = len(sizes), sum(sizes)
        offset = torch.tensor(np.cumsum(sizes), device=dev)
        xyz = torch.nn.functional.normalize(torch.randn(n, 3, device=dev), dim=-1).requires_grad_(True)
        feats = torch.randn(n, C, device=dev).requires_grad_(True)
        batch = ops.offset2batch(offset)
        start = ops.ragged_grid_start(xyz, offset)
        x0 = xyz.detach()
        for bits in (None, 10):
            label = f'({tag}) B={b} n={n} size={size} axis_bits={ops.default_axis_bits(b) if bits is None else bits}'
            grid = ops.grid_cluster_ragged(x0, offset, size, start, axis_bits=bits)
            u = int(grid.count)
            # (torch divides by a scalar on the accelerator as a multiplication by its reciprocal: a point within an ulp of a
            # cell boundary can land in the neighbouring cell there, so its cell count may differ by a few)
            u_torch = torch_index(x0, batch, start, size)[0].shape[0]
            assert abs(u - u_torch) <= max(8, u // 1000), (u, u_torch)
            hip_pool = lambda: ops.grid_pool_ragged(xyz, feats, offset, size, 'mean', start=start, axis_bits=bits)[:2]  # noqa: E731
            tor_pool = lambda: torch_pool(xyz, feats, batch, start, size)  # noqa: E731
            rows = [('index      ', {'hip': lambda: ops.grid_cluster_ragged(x0, offset, size, start, axis_bits=bits),
                                     'hip_pad': lambda: ops.grid_cluster_ragged(x0, offset, size, start, m=n, axis_bits=bits),
                                     'torch': lambda: torch_index(x0, batch, start, size)}),
                    ('pool fwd   ', {'hip': hip_pool, 'torch': tor_pool}),
                    ('pool fwd+bwd', {'hip': backward_of(hip_pool, xyz, feats), 'torch': backward_of(tor_pool, xyz, feats)})]
            for what, variants in rows:
                t = medians(variants, iters=3, rounds=7, warm=2)
                ratio = t['torch'][0] / t['hip'][0]
                mark = '**' if ratio < 1 else ''
                line = f'{mark}{label} cells={u} (torch {u_torch}) {what}:'
                for name, v in t.items():
                    line += f'  {name} {v[0]:10.1f} ({v[1]:.1f}-{v[2]:.1f})'
                line += f'  [torch / hip {ratio:.2f}x]{mark}'
                print(line, flush=True)
                lines.append(line)
            if bits is None:
                with _lib.profile() as read:
                    ops.grid_cluster_ragged(x0, offset, size, start, m=n, axis_bits=bits)
                    torch.cuda.synchronize()
                    per = [(name, *read(name)) for name in KERNELS]
                line = f'    kernels of one index call ({label}): ' + ', '.join(f'{name[3:-7]} {us:.1f} us x {count}' for name, us, count in per)
                line += f'; sum {sum(us * count for _, us, count in per):.1f} us'
                print(line, flush=True)
                lines.append(line)
        if tag == 'i':
            rect, rfeat = x0.view(b, 2048, 3).contiguous(), feats.detach().view(b, 2048, C).transpose(1, 2).contiguous()
            t = medians({'grid_cluster': lambda: ops.grid_cluster(rect, 40, -1.0, 2.0), 'grid_pool': lambda: ops.grid_pool(rect, rfeat, 40, -1.0, 2.0, reduce='mean')},
                        iters=3, rounds=7, warm=2)
            line = f'(i) rectangular, for scale: B={b} N=2048 resolution=40 (m=None, one host read):'
            for name, v in t.items():
                line += f'  {name} {v[0]:10.1f} ({v[1]:.1f}-{v[2]:.1f})'
            print(line, flush=True)
            lines.append(line)
        del xyz, feats, x0
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
