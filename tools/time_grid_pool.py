"""Timings of grid pooling (pcc_grid_cluster, pcc_segment_pool / _bwd, grid_pool.hip) beside the torch formulation a user would
write without it, on the same GPU in the same process:
  torch grid pool   the cell of every point, torch.unique(b * R^3 + cell, return_inverse=True) -- a global sort, and a host
                    synchronisation for the number of occupied cells --, scatter_reduce_ amax of the features and mean of the
                    coordinates into [U, C] and [U, 3] (float atomics); the backward through autograd.
Clouds are N points on a sphere of radius 0.45 inside the cube [-0.5, 0.5]^3 (the surface a shape encoder sees) with Gaussian
features[B,C,N]; the last row puts every point of a cloud in one cell.  `grid_pool` is voxel_index + grid_cluster + the two
segment_pool calls from the cloud with m=None (one host synchronisation, like torch.unique's), `m given` the same with the
capacity passed in (no synchronisation), `given index` segment_pool('max') alone on a ready GridIndex.  `mean | voxelize`:
segment_pool('mean') and voxelize on the same index -- the same sums, written to m slots or to R^3 cells.  `fwd` is the forward
alone, `f+b` the forward and the backward from a fixed incoming gradient of the pooled features.  The variants of a row
alternate round by round; a figure is the median over 7 rounds of the mean time per call inside a hipEvent bracket on the
stream.  `kernels` are the library's own per-launch averages (pcc_profile_enable(1)) over 5 further forward + backward calls of
segment_pool('max') and segment_pool('mean'), with the achieved bytes per second of the two that move features: B * C * (N +
m) * 4 bytes -- x read once, out written once, or the reverse -- over the kernel's time.
Output: profiles/grid_pool_times.txt (or --out)."""
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
KERNELS = ('vox_index_wave_kernel', 'vox_index_lds_kernel', 'grid_cluster_kernel', 'seg_pool_lds_kernel', 'seg_pool_kernel', 'seg_long_kernel',
           'seg_pool_bwd_lds_kernel', 'seg_pool_bwd_kernel')
MOVERS = ('seg_pool_lds_kernel', 'seg_pool_kernel', 'seg_pool_bwd_lds_kernel', 'seg_pool_bwd_kernel')


def torch_grid_pool(x, xyz, res, reduce='amax'):
    """``(features[U,C], centres[U,3])`` over the occupied cells of the batch, cloud by cloud in ascending cell."""
    b, c, n = x.shape
    ijk = torch.floor((xyz - LO) * ((res - 1) / EXTENT) + 0.5).clamp(0, res - 1).long()
    flat = ((ijk[..., 0] * res + ijk[..., 1]) * res + ijk[..., 2] + torch.arange(b, device=x.device)[:, None] * res ** 3).view(-1)
    uniq, inv = torch.unique(flat, return_inverse=True)
    u = uniq.numel()
    feats = x.new_zeros(u, c).scatter_reduce_(0, inv[:, None].expand(-1, c), x.transpose(1, 2).reshape(b * n, c), reduce, include_self=False)
    centres = x.new_zeros(u, 3).scatter_reduce_(0, inv[:, None].expand(-1, 3), xyz.reshape(b * n, 3), 'mean', include_self=False)
    return feats, centres


def packed(padded, count):
    """``[B,C,m]`` -> ``[U,C]``: the kept slots of every cloud, cloud by cloud."""
    return torch.cat([padded[s, :, :int(k)].transpose(0, 1) for s, k in enumerate(count.tolist())])


def kernel_times(run, moved_bytes):
    text = ''
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name in KERNELS:
            us, cnt = read(name)
            if cnt:
                text += f' {name} {us:.1f}'
                if name in MOVERS:
                    text += f' ({moved_bytes / (us * 1e-6) / 1e12:.2f} TB/s)'
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'grid_pool_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, N points on a sphere of radius 0.45 in the cube [-0.5, 0.5]^3 with features[B,C,N], pooled to '
             '[B,C,m], m the occupied cells of the fullest cloud; microseconds per call: median of 7 rounds (min-max), the variants of a row '
             'alternating']
    # (B, C, N, R, every point in one cell)
    rows = [(32, 64, 2048, 32, False), (32, 64, 15000, 64, False), (1, 64, 15000, 64, False), (32, 64, 2048, 32, True)]
    for b, c, n, res, one_cell in rows:
        if one_cell:
            xyz = 0.1 + 0.005 * torch.rand(b, n, 3, device=dev)
        else:
            xyz = 0.45 * torch.nn.functional.normalize(torch.randn(b, n, 3, device=dev), dim=2)
        x = torch.randn(b, c, n, device=dev).requires_grad_(True)
        vindex = ops.voxel_index(xyz, res, LO, EXTENT)
        gindex = ops.grid_cluster(vindex)
        m = gindex.seg.shape[1] - 1
        total = int(gindex.count.sum())
        g_pool, g_torch, g_grid = torch.randn(b, c, m, device=dev), torch.randn(total, c, device=dev), torch.randn(b, c, res, res, res, device=dev)
        with torch.no_grad():  # the formulations agree before they are timed
            mine, theirs = ops.grid_pool(xyz, x, res, LO, EXTENT), torch_grid_pool(x, xyz, res)
            assert torch.equal(packed(mine.features, mine.count), theirs[0])
            assert torch.allclose(packed(mine.xyz.transpose(1, 2), mine.count), theirs[1], rtol=1e-4, atol=1e-6)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def fwd_bwd(fn, grad):
            def run():
                x.grad = None
                fn().backward(grad)
            return run

        variants = {}
        for name, fn, grad in (('ours_pool', lambda: ops.grid_pool(xyz, x, res, LO, EXTENT).features, g_pool),
                               ('ours_m', lambda: ops.grid_pool(xyz, x, res, LO, EXTENT, m=m).features, g_pool),
                               ('ours_index', lambda: ops.segment_pool(x, gindex, 'max'), g_pool),
                               ('ours_mean', lambda: ops.segment_pool(x, gindex, 'mean'), g_pool),
                               ('ours_vox', lambda: ops.voxelize(x, vindex), g_grid),
                               ('torch_pool', lambda: torch_grid_pool(x, xyz, res)[0], g_torch)):
            variants[name + '_fwd'] = fwd(fn)
            variants[name + '_fb'] = fwd_bwd(fn, grad)
        t = medians(variants, iters=3 if b * c * res ** 3 > 1 << 24 else 10, rounds=7, warm=2)

        def cell(name):
            return ' '.join(f'{label} {t[f"{name}_{kind}"][0]:.1f} ({t[f"{name}_{kind}"][1]:.1f}-{t[f"{name}_{kind}"][2]:.1f})' for kind, label in (('fwd', 'fwd'), ('fb', 'f+b')))

        line = f'B={b:2d} C={c:3d} N={n:5d} R={res:2d}{" one cell" if one_cell else "         "} m={m:5d} cells={total:6d}:'
        line += f'  grid_pool {cell("ours_pool")}  torch {cell("torch_pool")}'
        line += f' [{t["torch_pool_fwd"][0] / t["ours_pool_fwd"][0]:.2f}x fwd, {t["torch_pool_fb"][0] / t["ours_pool_fb"][0]:.2f}x f+b]'
        line += f'  m given {cell("ours_m")}  given index {cell("ours_index")}  mean {cell("ours_mean")} | voxelize {cell("ours_vox")}'

        def both():
            ops.grid_cluster(ops.voxel_index(xyz, res, LO, EXTENT), m=m)
            for reduce in ('max', 'mean'):
                x.grad = None
                ops.segment_pool(x, gindex, reduce).backward(g_pool)

        line += '  kernels:' + kernel_times(both, b * c * (n + m) * 4)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
