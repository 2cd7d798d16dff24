"""Timings of the kernel point convolution (kpconv_aggregate / kernel_point_conv: pcc_kpconv_aggregate and its backward,
kpconv.hip) beside the two ways to the same result without it, on the same GPU in the same process:
  torch   the published PyTorch formulation: the neighbours' coordinates and features gathered into [B,M,k,3] and
          [B,C,M,k], the [B,M,k,K,3] differences, a square root, a clamp, and a [K,k] x [k,C] matmul per centre; its
          result stays in its own layout [B,M,K,C]; the backward through autograd;
  agg     the best composition of this library's ops: aggregate_points(x.repeat(1, K, 1), idx, h) with h[B,K,M,k] from
          kernel_point_influence (torch).
Clouds are N points uniform in [0,1)^3 with Gaussian features[B,C,N]; the M centres by farthest point sampling, the lists by
ball_query(pad='none') at the row's radius, kernel_point_layout(15, 0.66 radius), sigma = radius / 2.5; the last row is a
padded list (radius 1e-4: every ball holds its centre alone).  `fwd` is the forward alone, `f+b` the forward and the
backward into the features from a fixed incoming gradient; `+gemm` adds the convolution's matrix product with
weight[K,C,O = C] (and its gradient).  The variants of a row alternate round by round; a figure is the median over 7 rounds
of the mean time per call inside a hipEvent bracket on the stream.  `kernels` are the library's own per-launch averages
(pcc_profile_enable(1)) over 5 further calls: the forward kernel with the rate at which it writes its output (B K C M 4
bytes) as a share of the 8 TB/s HBM peak, and the backward kernel with its bins in LDS and on the direct path (interp_path
1 / 2).
`pairs` is the share of the (valid slot, kernel point) pairs with h > 0: the others are skipped.
Output: profiles/kpconv_times.txt (or --out)."""
import argparse
import os
import sys

os.environ.setdefault('PCC_TEST_HOOKS', '1')  # the A/B switches of include/pcc_test_hooks.h

import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops  # noqa: E402
from time_knn_cross import medians, with_switch  # noqa: E402

dev = torch.device('cuda:0')
HBM_PEAK = 8.0e12  # bytes per second
KP = 15


def torch_kpconv(x, xyz, centres, idx, kpts, sigma, weight=None):
    """[B,M,K,C] (or [B,O,M] with a weight): what a user writes in torch."""
    b, c, n = x.shape
    m, k = idx.shape[1:]
    valid, safe = idx >= 0, idx.clamp_min(0)
    nb = xyz.gather(1, safe.reshape(b, m * k, 1).expand(-1, -1, 3)).view(b, m, k, 3) - centres[:, :, None]
    dist = (nb[:, :, :, None, :] - kpts).square().sum(-1).sqrt()  # [B,M,k,K]
    h = (1.0 - dist / sigma).clamp_min(0.0) * valid[..., None]
    feats = x.gather(2, safe.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k).permute(0, 2, 3, 1)  # [B,M,k,C]
    agg = torch.matmul(h.transpose(2, 3), feats)  # [B,M,K,C]
    if weight is None:
        return agg
    return torch.matmul(agg.reshape(b, m, -1), weight.reshape(-1, weight.shape[2])).transpose(1, 2)


def agg_kpconv(x, xyz, centres, idx, kpts, sigma, weight=None):
    """[B, K * C, M] through aggregate_points, the features copied K times."""
    kp = kpts.shape[0]
    h = ops.kernel_point_influence(xyz, centres, idx, kpts, sigma).permute(0, 3, 1, 2).contiguous()
    agg = ops.aggregate_points(x.repeat(1, kp, 1), idx, h)
    return agg if weight is None else torch.matmul(weight.reshape(-1, weight.shape[2]).t(), agg)


def ours_kpconv(x, xyz, centres, idx, kpts, sigma, weight=None):
    if weight is None:
        return ops.kpconv_aggregate(x, xyz, centres, idx, kpts, sigma)
    return ops.kernel_point_conv(x, xyz, centres, idx, kpts, sigma, weight)


def profiled(run, names):
    """{name: microseconds per launch} of the library's kernels over 5 calls of ``run``."""
    out = {}
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name in names:
            us, cnt = read(name)
            if cnt:
                out[name] = us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kpconv_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, clouds of N points uniform in the unit cube with features[B,C,N], M centres by FPS, '
             f'ball_query(pad=none) lists, K = {KP} kernel points, sigma = radius / 2.5; out [B, K C, M]; microseconds per call: '
             'median of 7 rounds (min-max), the variants of a row alternating']
    # (B, N, M, k, C, radius)
    rows = [(32, 2048, 512, 32, 64, 0.2), (32, 2048, 2048, 32, 64, 0.2), (32, 15000, 2048, 32, 32, 0.1), (1, 15000, 2048, 32, 64, 0.1),
            (32, 2048, 2048, 32, 64, 1e-4)]
    for b, n, m, k, c, radius in rows:
        xyz = torch.rand(b, n, 3, device=dev)
        centres = torch.gather(xyz, 1, ops.farthest_point_sample(xyz, m)[:, :, None].expand(-1, -1, 3))
        idx = ops.ball_query(xyz, centres, radius, k, pad='none')
        work = 0.2 if radius < 0.01 else radius  # (the padded list keeps the geometry of the second row)
        kpts, sigma = ops.kernel_point_layout(KP, 0.66 * work).to(dev), work / 2.5
        h = ops.kernel_point_influence(xyz, centres, idx, kpts, sigma)
        valid = idx >= 0
        pairs = (h[valid] > 0).float().mean().item()
        x = torch.randn(b, c, n, device=dev).requires_grad_(True)
        weight = (torch.randn(KP, c, c, device=dev) / (KP * c) ** 0.5).requires_grad_(True)
        grad, grad_o = torch.randn(b, KP * c, m, device=dev), torch.randn(b, c, m, device=dev)
        common = (xyz, centres, idx, kpts, sigma)
        with torch.no_grad():  # the three formulations agree before they are timed
            ours = ours_kpconv(x, *common)
            assert torch.allclose(ours, agg_kpconv(x, *common), rtol=1e-4, atol=1e-4)
            assert torch.allclose(ours.view(b, KP, c, m), torch_kpconv(x, *common).permute(0, 2, 3, 1), rtol=1e-4, atol=1e-4)
            assert torch.allclose(ours_kpconv(x, *common, weight), torch_kpconv(x, *common, weight), rtol=1e-3, atol=1e-3)

        def fwd(fn, w):
            def run():
                with torch.no_grad():
                    return fn(x, *common, w)
            return run

        def fwd_bwd(fn, w):
            def run():
                x.grad = weight.grad = None
                out = fn(x, *common, w)
                g = grad_o if w is not None else grad
                if out.shape != g.shape:  # (torch's own layout [B,M,K,C])
                    g = g.view(b, KP, c, m).permute(0, 3, 1, 2)
                out.backward(g)
            return run

        big = b * m * k * c > 1 << 25
        head = f'B={b:2d} N={n:5d} M={m:4d} k={k} C={c:2d} r={radius:g} valid {valid.float().mean().item():.2f} pairs {pairs:.2f}'
        for w, tag in ((None, '     '), (weight, '+gemm')):
            variants = {}
            for name, fn in (('ours', ours_kpconv), ('torch', torch_kpconv), ('agg', agg_kpconv)):
                variants[name + '_fwd'], variants[name + '_fb'] = fwd(fn, w), fwd_bwd(fn, w)
            t = medians(variants, iters=3 if big else 10, rounds=7, warm=2)
            line = f'{head} {tag}:'
            for key, label in (('ours_fwd', 'fwd'), ('torch_fwd', 'torch fwd'), ('agg_fwd', 'agg fwd'), ('ours_fb', 'f+b'),
                               ('torch_fb', 'torch f+b'), ('agg_fb', 'agg f+b')):
                line += f'  {label} {t[key][0]:9.1f} ({t[key][1]:.1f}-{t[key][2]:.1f})'
            line += (f'  [torch / ours: fwd {t["torch_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["torch_fb"][0] / t["ours_fb"][0]:.2f}x; '
                     f'agg / ours: fwd {t["agg_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["agg_fb"][0] / t["ours_fb"][0]:.2f}x]')
            print(line, flush=True)
            lines.append(line)
        names = (b'kp_fwd_kernel', b'kp_bwd_kernel<lds>', b'kp_bwd_kernel<direct>')
        line = f'{head} kernels:'
        for path, label in ((1, 'lds'), (2, 'direct')):
            for name, us in profiled(with_switch('interp_path', path, fwd_bwd(ours_kpconv, None)), names).items():
                if b'fwd' in name and path == 2:
                    continue  # (the forward has one path)
                line += f'  {name.decode()} {us:.1f}'
                if b'fwd' in name:
                    rate = b * KP * c * m * 4 / (us * 1e-6)
                    line += f' ({rate / 1e12:.2f} TB/s of out = {100 * rate / HBM_PEAK:.0f}% of peak)'
        print(line, flush=True)
        lines.append(line)
        del h
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
