"""Timings of the point-voxel ops (pcc_voxel_index, pcc_voxelize / _bwd, pcc_devoxelize / _bwd, voxelize.hip) beside the torch
formulation a user would write without them, on the same GPU in the same process:
  torch voxelize    the cell of every point, index_add_ of the features and of ones into [B * R^3, C] and [B * R^3], a division
                    and the permute to [B,C,R,R,R]; the backward through autograd;
  torch devoxelize  the trilinear corners of every point, eight gathers of [B,C,N], each multiplied by its weight and added; the
                    backward through autograd (scatter_add with global float atomics).
Clouds are N points on a sphere of radius 0.45 inside the cube [-0.5, 0.5]^3 (the surface a shape encoder sees) with Gaussian
features[B,C,N]; the last row puts every point of a cloud in one cell.  `voxelize` is voxel_index + voxelize from the cloud
(the torch side computes its cells too), `given index` the op alone on a ready VoxelIndex, `pair` one index, voxelize and
devoxelize at the same points (point_voxel with an identity network).  `fwd` is the forward alone, `f+b` the forward and
the backward from a fixed incoming gradient.  The variants of a row alternate round by round; a figure is the median over 7
rounds of the mean time per call inside a hipEvent bracket on the stream.  `kernels` are the library's own per-launch
averages (pcc_profile_enable(1)) over 5 further forward + backward calls of the pair, and for the two kernels that write a
dense grid the achieved bytes per second of that write, B * C * R^3 * 4 bytes over the kernel's time.
Output: profiles/voxelize_times.txt (or --out)."""
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
KERNELS = ('vox_index_wave_kernel', 'vox_index_lds_kernel', 'vox_start_kernel', 'vox_fwd_kernel', 'vox_long_kernel', 'vox_bwd_kernel',
           'devox_fwd_kernel', 'devox_bwd_lds_kernel', 'devox_bwd_global_kernel')
GRID_WRITERS = ('vox_fwd_kernel', 'devox_bwd_lds_kernel', 'devox_bwd_global_kernel')


def torch_voxelize(x, xyz, res):
    b, c, n = x.shape
    ijk = torch.floor((xyz - LO) * ((res - 1) / EXTENT) + 0.5).clamp(0, res - 1).long()
    flat = ((ijk[..., 0] * res + ijk[..., 1]) * res + ijk[..., 2] + torch.arange(b, device=x.device)[:, None] * res ** 3).view(-1)
    acc = x.new_zeros(b * res ** 3, c).index_add_(0, flat, x.transpose(1, 2).reshape(b * n, c))
    cnt = x.new_zeros(b * res ** 3).index_add_(0, flat, x.new_ones(b * n))
    return (acc / cnt.clamp(min=1)[:, None]).view(b, res ** 3, c).transpose(1, 2).reshape(b, c, res, res, res)


def torch_devoxelize(grid, xyz):
    b, c, res = grid.shape[:3]
    n = xyz.shape[1]
    t = ((xyz - LO) * ((res - 1) / EXTENT)).clamp(0, res - 1)
    base = t.floor().clamp(max=res - 2)
    w1 = t - base
    w, i0 = (1 - w1, w1), base.long()
    rows = grid.reshape(b, c, res ** 3)
    out = 0
    for e in range(8):
        di, dj, dk = e >> 2, (e >> 1) & 1, e & 1
        off = ((i0[..., 0] + di) * res + i0[..., 1] + dj) * res + i0[..., 2] + dk
        out = out + (w[di][..., 0] * w[dj][..., 1] * w[dk][..., 2])[:, None] * rows.gather(2, off[:, None].expand(b, c, n))
    return out


def kernel_times(run, grid_bytes):
    text = ''
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name in KERNELS:
            us, cnt = read(name)
            if cnt:
                text += f' {name} {us:.1f}'
                if name in GRID_WRITERS:
                    text += f' ({grid_bytes / (us * 1e-6) / 1e12:.2f} TB/s of grid written)'
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'voxelize_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, N points on a sphere of radius 0.45 in the cube [-0.5, 0.5]^3 with features[B,C,N], grid '
             '[B,C,R,R,R]; microseconds per call: median of 7 rounds (min-max), the variants of a row alternating']
    # (B, C, N, R, every point in one cell)
    rows = [(32, 64, 2048, 32, False), (32, 64, 15000, 32, False), (32, 128, 2048, 16, False), (8, 32, 2048, 64, False),
            (1, 64, 15000, 32, False), (32, 64, 2048, 32, True)]
    for b, c, n, res, one_cell in rows:
        if one_cell:
            xyz = 0.1 + 0.005 * torch.rand(b, n, 3, device=dev)
        else:
            xyz = 0.45 * torch.nn.functional.normalize(torch.randn(b, n, 3, device=dev), dim=2)
        x = torch.randn(b, c, n, device=dev).requires_grad_(True)
        grid = torch.randn(b, c, res, res, res, device=dev).requires_grad_(True)
        g_grid, g_out = torch.randn(b, c, res, res, res, device=dev), torch.randn(b, c, n, device=dev)
        index = ops.voxel_index(xyz, res, LO, EXTENT)
        with torch.no_grad():  # the formulations agree before they are timed
            assert torch.allclose(ops.voxelize(x, index), torch_voxelize(x, xyz, res), rtol=1e-4, atol=1e-5)
            assert torch.allclose(ops.devoxelize(grid, xyz, LO, EXTENT), torch_devoxelize(grid, xyz), rtol=1e-4, atol=1e-5)

        def fwd(fn, *a):
            def run():
                with torch.no_grad():
                    return fn(*a)
            return run

        def fwd_bwd(fn, leaf, grad, *a):
            def run():
                leaf.grad = None
                fn(*a).backward(grad)
            return run

        ours = {'vox': lambda: ops.voxelize(x, xyz, res, LO, EXTENT), 'voxi': lambda: ops.voxelize(x, index),
                'devox': lambda: ops.devoxelize(grid, xyz, LO, EXTENT),
                'pair': lambda: ops.point_voxel(x, xyz, res, lambda g: g, LO, EXTENT)}
        theirs = {'vox': lambda: torch_voxelize(x, xyz, res), 'devox': lambda: torch_devoxelize(grid, xyz),
                  'pair': lambda: torch_devoxelize(torch_voxelize(x, xyz, res), xyz)}
        leaf = {'vox': (x, g_grid), 'voxi': (x, g_grid), 'devox': (grid, g_out), 'pair': (x, g_out)}
        variants = {}
        for side, fns in (('ours', ours), ('torch', theirs)):
            for op, fn in fns.items():
                variants[f'{side}_{op}_fwd'] = fwd(fn)
                variants[f'{side}_{op}_fb'] = fwd_bwd(fn, *leaf[op])
        t = medians(variants, iters=3 if b * c * res ** 3 > 1 << 24 else 10, rounds=7, warm=2)
        line = f'B={b:2d} C={c:3d} N={n:5d} R={res:2d}{" one cell" if one_cell else "         "}:'
        for op, label in (('vox', 'voxelize'), ('devox', 'devoxelize'), ('pair', 'pair')):
            for kind, klabel in (('fwd', 'fwd'), ('fb', 'f+b')):
                o, th = t[f'ours_{op}_{kind}'], t[f'torch_{op}_{kind}']
                line += f'  {label} {klabel} {o[0]:.1f} ({o[1]:.1f}-{o[2]:.1f}) torch {th[0]:.1f} ({th[1]:.1f}-{th[2]:.1f}) [{th[0] / o[0]:.2f}x]'
        line += f'  voxelize given index: fwd {t["ours_voxi_fwd"][0]:.1f} f+b {t["ours_voxi_fb"][0]:.1f}'
        grid_bytes = b * c * res ** 3 * 4
        line += f'  grid {grid_bytes / 1e6:.0f} MB  kernels:' + kernel_times(fwd_bwd(ours['pair'], *leaf['pair']), grid_bytes)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
