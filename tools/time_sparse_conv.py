"""Timings of the submanifold sparse convolution (pcc_cell_neighbours, pcc_sparse_conv, sparse_conv.hip) beside the two
formulations a user would write without it, on the same GPU in the same process:
  (a) dense   voxelize -> torch.nn.functional.conv3d on the [B,C,R,R,R] grid -> gather at the occupied cells;
  (b) grouped group_points along the map ([B,C,m,K^3]: K^3 times the features) and one matmul; backward through autograd.
Clouds are N points on a sphere of radius 0.45 inside the cube [-0.5, 0.5]^3 (the surface a shape encoder sees) with Gaussian
features[B,C,N]; C = O.  The VoxelIndex, the GridIndex and the map are built beforehand for every variant.  `conv` is sparse_conv
on the ready level (the pooled features) -- what (b) computes --, `level` segment_pool('mean') + sparse_conv from the point
features -- what (a) computes.  `fwd` is the forward alone, `f+b` the forward and the backward from a fixed incoming gradient
with the gradients of features, weight and bias; `f+b(x)` asks for the gradient of the features only: the difference to `f+b`
is the weight gradient, a torch composition per tap that is not fused.  The variants of a row alternate round by round; a
figure is the median over 7 rounds of the mean time per call inside a hipEvent bracket on the stream.  `kernels` are the
library's own per-launch averages (pcc_profile_enable(1)) over 5 further calls of cell_neighbours and of the forward alone,
with the forward's achieved FLOP/s -- 2 * C * O per valid tap -- against the 157 TFLOP/s float32 peak; `skipped` is the share
of (tile of 16 slots, tap) pairs the kernel skips because the tap is empty for the whole tile, `filled` the share of slots that
hold a neighbour in the pairs it computes.
Output: profiles/sparse_conv_times.txt (or --out)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops  # noqa: E402
from time_knn_cross import medians  # noqa: E402

dev = torch.device('cuda:0')
LO, EXTENT = -0.5, 1.0
PEAK = 157e12
ROW_TILE = 16  # slots per tile of sparse_conv_mfma_kernel, which serves every shape below: an empty tap is skipped per tile


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sparse_conv_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, N points on a sphere of radius 0.45 in the cube [-0.5, 0.5]^3, features[B,C,N] pooled to the m '
             'occupied cells of the fullest cloud, C = O; microseconds per call: median of 7 rounds (min-max), the variants of a row alternating']
    # (B, C = O, N, R, K)
    rows = [(32, 64, 2048, 32, 3), (32, 64, 15000, 64, 3), (1, 64, 15000, 64, 3), (32, 32, 2048, 16, 5)]
    for b, c, n, res, ksize in rows:
        taps, h = ksize ** 3, (ksize - 1) // 2
        xyz = 0.45 * torch.nn.functional.normalize(torch.randn(b, n, 3, device=dev), dim=2)
        x = torch.randn(b, c, n, device=dev).requires_grad_(True)
        vindex = ops.voxel_index(xyz, res, LO, EXTENT)
        gindex = ops.grid_cluster(vindex)
        m = gindex.seg.shape[1] - 1
        cmap = ops.cell_neighbours(vindex, gindex, ksize)
        conv = ops.SubmanifoldConv3d(c, c, ksize).to(dev)
        weight, bias = conv.weight, conv.bias
        pooled = ops.segment_pool(x, gindex, 'mean').detach().requires_grad_(True)
        dense_w = weight.detach().view(ksize, ksize, ksize, c, c).permute(4, 3, 0, 1, 2).contiguous().requires_grad_(True)
        real = torch.arange(m, device=dev)[None, :] < gindex.count[:, None]
        # the flat cell of every slot (0 for a padded one: masked behind the gather)
        sorted_cell = torch.gather(vindex.cell.long(), 1, gindex.order.long())
        slot_cell = torch.where(real, torch.gather(sorted_cell, 1, gindex.seg[:, :m].long().clamp(max=n - 1)), torch.zeros((), dtype=torch.long, device=dev))
        g = torch.randn(b, c, m, device=dev)

        def ours(feats, wt=weight, bs=bias):
            return ops.sparse_conv(feats, cmap, wt, bs)

        def ours_level():
            return ours(ops.segment_pool(x, gindex, 'mean'))

        def dense():
            y = torch.nn.functional.conv3d(ops.voxelize(x, vindex), dense_w, bias, padding=h)
            return torch.where(real[:, None, :], torch.gather(y.view(b, c, -1), 2, slot_cell[:, None, :].expand(b, c, m)), y.new_zeros(()))

        def grouped():
            y = torch.einsum('bcmt,tco->bom', ops.group_points(pooled, cmap.nbr), weight) + bias[None, :, None]
            return torch.where(real[:, None, :], y, y.new_zeros(()))

        with torch.no_grad():  # the formulations agree before they are timed
            want = ours(pooled)
            assert torch.allclose(ours_level(), want) and torch.allclose(grouped(), want, rtol=1e-3, atol=1e-4)
            assert torch.allclose(dense(), want, rtol=1e-3, atol=1e-4)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def fwd_bwd(fn):
            def run():
                for t in (x, pooled, weight, bias, dense_w):
                    t.grad = None
                fn().backward(g)
            return run

        variants = {}
        for name, fn in (('conv', lambda: ours(pooled)), ('level', ours_level), ('dense', dense), ('grouped', grouped)):
            variants[name + '_fwd'] = fwd(fn)
            variants[name + '_fb'] = fwd_bwd(fn)
        variants['conv_fbx'] = fwd_bwd(lambda: ours(pooled, weight.detach(), bias.detach()))
        variants['map'] = lambda: ops.cell_neighbours(vindex, gindex, ksize)
        t = medians(variants, iters=3 if b * c * res ** 3 > 1 << 24 else 10, rounds=7, warm=2)

        def cell(name, kinds=(('fwd', 'fwd'), ('fb', 'f+b'))):
            return ' '.join(f'{label} {t[f"{name}_{kind}"][0]:.1f} ({t[f"{name}_{kind}"][1]:.1f}-{t[f"{name}_{kind}"][2]:.1f})' for kind, label in kinds)

        valid = cmap.nbr >= 0
        pad = (-m) % ROW_TILE
        tiles = torch.cat((valid, valid.new_zeros(b, pad, taps)), 1).view(b, -1, ROW_TILE, taps)
        computed = tiles.any(2)  # [b, tiles, taps]
        skipped = 1 - computed.float().mean().item()
        filled = valid.sum().item() / (computed.sum().item() * ROW_TILE)
        line = f'B={b:2d} C=O={c:3d} N={n:5d} R={res:2d} K={ksize} m={m:5d} cells={int(gindex.count.sum()):6d} valid taps {valid.float().mean().item():.3f}:'
        line += f'  conv {cell("conv")} f+b(x) {t["conv_fbx"][0]:.1f}  level {cell("level")}  (a) dense {cell("dense")}'
        line += f' [{t["dense_fwd"][0] / t["level_fwd"][0]:.2f}x fwd, {t["dense_fb"][0] / t["level_fb"][0]:.2f}x f+b]'
        line += f'  (b) grouped {cell("grouped")} [{t["grouped_fwd"][0] / t["conv_fwd"][0]:.2f}x fwd, {t["grouped_fb"][0] / t["conv_fb"][0]:.2f}x f+b]'
        line += f'  map {t["map"][0]:.1f} ({t["map"][1]:.1f}-{t["map"][2]:.1f})'
        with _lib.profile() as read:
            for _ in range(5):
                variants['map']()
                variants['conv_fwd']()
            torch.cuda.synchronize()
            map_us, conv_us = read('cell_nbr_kernel')[0], read('sparse_conv_')[0]  # (sparse_conv_mfma_kernel<..> at these widths)
        flops = 2.0 * valid.sum().item() * c * c
        line += f'  kernels: cell_nbr_kernel {map_us:.1f} sparse_conv_mfma_kernel {conv_us:.1f} ({flops / (conv_us * 1e-6) / 1e12:.2f} TFLOP/s over the valid taps, '
        line += f'{100 * flops / (conv_us * 1e-6) / PEAK:.1f}% of peak)  skipped {skipped:.3f} filled {filled:.3f}'
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
