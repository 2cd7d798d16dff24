"""Timings of the pointnet2_ops drop-in (pointnet2_ops/pointnet2_modules.py) beside two other ways to run the same layers, on
the same GPU in the same process, with the same parameters:
  torch    the same modules with the six utils replaced by the pure-torch formulation a user without the extension writes:
           a loop for farthest point sampling, dense [B,M,N] distances (expanded form, one bmm), a masked index tensor, sort
           and slice for the ball query, expand + gather for the two gathers, topk of the dense distances for three_nn,
           expand + gather, multiply, sum for three_interpolate; backward through autograd.
  direct   the same layers calling neighbour_ops on int64 lists (farthest_point_sample, query_and_group, knn_cross,
           interpolate_points): what the adapter costs, i.e. its int32 <-> int64 conversions and extra gathers.
Clouds are points on the unit sphere xyz[B,N,3] with Gaussian features.  Rows: a single-scale set-abstraction module, a
three-scale one (radii 0.1 / 0.2 / 0.4, the same nsample and MLP per scale), a feature-propagation module, each at B = 32 and
B = 1.  `fwd` is the forward under no_grad, `f+b` the forward and the backward (parameters and input features) from a fixed
incoming gradient.  The modules are in training mode (BatchNorm on batch statistics).  The variants of a row alternate round
by round; a figure is the median over 7 rounds of the mean time per call inside a hipEvent bracket on the stream.  `diff` is
the largest absolute difference of a variant's forward output to the drop-in's: 0 where the lists agree; on the
feature-propagation rows the known points are a subset of the unknown ones, the expanded form rounds their zero distances to
about 1e-7 where the kernel's difference form gives exactly 0, and 1 / (dist + 1e-8) turns that into different weights.  No
threshold is asserted: the tool writes what it measures.  Output: profiles/pointnet2_ops_times.txt (or --out)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import neighbour_ops as ops  # noqa: E402
from pointnet2_ops import pointnet2_modules as pm  # noqa: E402
from time_knn_cross import medians  # noqa: E402

dev = torch.device('cuda:0')


# ---- the pure-torch formulation ---------------------------------------------------------------------------------------

def square_distance(a, b):
    """[B,M,N] squared distances of a[B,M,3] to b[B,N,3], expanded form."""
    d = -2 * torch.bmm(a, b.transpose(1, 2))
    d += (a ** 2).sum(-1)[:, :, None]
    d += (b ** 2).sum(-1)[:, None, :]
    return d


def torch_fps(xyz, npoint):
    b, n, _ = xyz.shape
    centroids = torch.zeros(b, npoint, dtype=torch.long, device=xyz.device)
    distance = torch.full((b, n), 1e10, device=xyz.device)
    farthest = torch.zeros(b, dtype=torch.long, device=xyz.device)
    rows = torch.arange(b, device=xyz.device)
    for i in range(npoint):
        centroids[:, i] = farthest
        centroid = xyz[rows, farthest][:, None, :]
        distance = torch.min(distance, ((xyz - centroid) ** 2).sum(-1))
        farthest = distance.max(-1)[1]
    return centroids


def torch_ball_query(radius, nsample, xyz, new_xyz):
    b, n, _ = xyz.shape
    m = new_xyz.shape[1]
    idx = torch.arange(n, device=xyz.device).view(1, 1, n).repeat(b, m, 1)
    idx[square_distance(new_xyz, xyz) >= radius ** 2] = n
    idx = idx.sort(-1)[0][:, :, :nsample]
    first = idx[:, :, :1].expand(-1, -1, idx.shape[2])
    return torch.where(idx == n, first, idx)


def torch_group(feats, idx):
    b, c, _ = feats.shape
    m, k = idx.shape[1:]
    return feats.gather(2, idx.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k)


def torch_sa(module, xyz, feats):
    """The forward of a set-abstraction module on the torch formulation, same MLPs."""
    sel = torch_fps(xyz, module.npoint)
    new_xyz = xyz.gather(1, sel[:, :, None].expand(-1, -1, 3))
    pooled = []
    for grouper, mlp in zip(module.groupers, module.mlps):
        idx = torch_ball_query(grouper.radius, grouper.nsample, xyz, new_xyz)
        grouped_xyz = torch_group(xyz.transpose(1, 2), idx) - new_xyz.transpose(1, 2)[:, :, :, None]
        pooled.append(torch.max(mlp(torch.cat((grouped_xyz, torch_group(feats, idx)), 1)), 3)[0])
    return torch.cat(pooled, 1)


def torch_fp(module, unknown, known, unknow_feats, known_feats):
    """The forward of a feature-propagation module on the torch formulation, same MLP."""
    d, idx = square_distance(unknown, known).topk(3, dim=-1, largest=False)
    recip = 1.0 / (d.clamp_min(0).sqrt() + 1e-8)
    weight = recip / recip.sum(2, keepdim=True)
    interpolated = (torch_group(known_feats, idx) * weight[:, None]).sum(-1)
    return module.mlp(torch.cat((interpolated, unknow_feats), 1).unsqueeze(-1)).squeeze(-1)


# ---- the same layers on neighbour_ops, int64 lists throughout ----------------------------------------------------------------

def direct_sa(module, xyz, feats):
    sel = ops.farthest_point_sample(xyz, module.npoint)
    new_xyz = torch.gather(xyz, 1, sel[:, :, None].expand(-1, -1, 3))
    pooled = []
    for grouper, mlp in zip(module.groupers, module.mlps):
        grouped = ops.query_and_group(xyz, new_xyz, feats, grouper.radius, grouper.nsample).grouped
        pooled.append(torch.max(mlp(grouped), 3)[0])
    return torch.cat(pooled, 1)


def direct_fp(module, unknown, known, unknow_feats, known_feats):
    idx, d2 = ops.knn_cross(unknown.transpose(1, 2), known.transpose(1, 2), 3, return_distance=True)
    recip = 1.0 / (d2.sqrt() + 1e-8)
    weight = recip / recip.sum(2, keepdim=True)
    interpolated = ops.interpolate_points(known_feats, idx, weight)
    return module.mlp(torch.cat((interpolated, unknow_feats), 1).unsqueeze(-1)).squeeze(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pointnet2_ops_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, points on the unit sphere, Gaussian features, modules in training mode; microseconds per '
             'call: median of 7 rounds (min-max), the variants of a row alternating; ours = pointnet2_ops module, torch = same '
             'module on the pure-torch utils, direct = same layers on neighbour_ops with int64 lists; diff = largest absolute '
             'difference of the forward outputs to ours']
    mlp = [64, 64, 128]
    rows = []
    for b in (32, 1):
        rows.append((f'SA  B={b:2d} N=2048 npoint=512 nsample=32 r=0.2 mlp={mlp}', 'sa', b,
                     lambda: pm.PointnetSAModule(mlp, npoint=512, radius=0.2, nsample=32)))
        rows.append((f'MSG B={b:2d} N=2048 npoint=512 nsample=32 r=(0.1,0.2,0.4) mlp={mlp} per scale', 'sa', b,
                     lambda: pm.PointnetSAModuleMSG(512, [0.1, 0.2, 0.4], [32, 32, 32], [mlp, mlp, mlp])))
        rows.append((f'FP  B={b:2d} n=2048 m=512 mlp=[256, 128] (192 interpolated + 64 skip channels)', 'fp', b,
                     lambda: pm.PointnetFPModule([256, 128])))
    for label, kind, b, make in rows:
        module = make().to(dev).train()
        xyz = torch.nn.functional.normalize(torch.randn(b, 2048, 3, device=dev), dim=-1)
        if kind == 'sa':
            feats = torch.randn(b, 64, 2048, device=dev, requires_grad=True)
            inputs = (xyz, feats)
            forms = {'ours': lambda m, *a: m(*a)[1], 'torch': torch_sa, 'direct': direct_sa}
        else:
            known = xyz[:, :512].contiguous()
            skip = torch.randn(b, 64, 2048, device=dev, requires_grad=True)
            known_feats = torch.randn(b, 192, 512, device=dev, requires_grad=True)
            inputs = (xyz, known, skip, known_feats)
            forms = {'ours': lambda m, *a: m(*a), 'torch': torch_fp, 'direct': direct_fp}
        leaves = [t for t in inputs if t.requires_grad] + list(module.parameters())
        with torch.no_grad():
            outs = {name: fn(module, *inputs) for name, fn in forms.items()}
        grad = torch.randn_like(outs['ours'])
        diff = {name: float((outs[name] - outs['ours']).abs().max()) for name in ('torch', 'direct')}

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn(module, *inputs)
            return run

        def fwd_bwd(fn):
            def run():
                for t in leaves:
                    t.grad = None
                fn(module, *inputs).backward(grad)
            return run

        variants = {}
        for name, fn in forms.items():
            variants[name + '_fwd'] = fwd(fn)
            variants[name + '_fb'] = fwd_bwd(fn)
        t = medians(variants, iters=3, rounds=7, warm=2)
        line = label + ':'
        for name in forms:
            for key, what in (('_fwd', 'fwd'), ('_fb', 'f+b')):
                v = t[name + key]
                line += f'  {name} {what} {v[0]:9.1f} ({v[1]:.1f}-{v[2]:.1f})'
        line += (f'  [torch / ours: fwd {t["torch_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["torch_fb"][0] / t["ours_fb"][0]:.2f}x; '
                 f'direct / ours: fwd {t["direct_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["direct_fb"][0] / t["ours_fb"][0]:.2f}x; '
                 f'diff torch {diff["torch"]:.2e} direct {diff["direct"]:.2e}]')
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
