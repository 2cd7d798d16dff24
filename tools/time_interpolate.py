"""Timings of the interpolation op (pcc_interpolate / pcc_interpolate_bwd, interpolate.hip) beside the two ways to the same
result without it, on the same GPU in the same process:
  torch   what a user writes: the index list expanded to every channel, one gather of [B,C,M,k], a multiplication by the
          weights and a sum over k; the backward through autograd (scatter_add with global float atomics);
  group   what the library offered before: group_points(x, idx) (pcc_group_points), then (w[:, None] * grouped).sum(-1).
Sparse clouds are N points on the unit sphere with Gaussian features[B,C,N]; the M dense points are other points on it, the
lists come from knn_cross and the weights from interpolation_weights of its distances.  `fwd` is the forward alone, `f+b`
the forward and the backward of the features from a fixed incoming gradient; rows marked `+w` also ask for the gradient of
the weights.  Both paths are forced against each other through the interp_path switch of include/pcc_test_hooks.h
(lds / direct).  The variants of a row alternate round by round; a figure is the median over 7 rounds of the mean time per
call inside a hipEvent bracket on the stream.  `moved` is what the forward has to move once, x + idx + w + out =
B * (C * N + M * k * 12 + C * M) * 4-byte words (the list's indices are 8 bytes), over the forward's time, and its share of the
8 TB/s HBM peak.  `kernels` are the library's own per-launch averages (pcc_profile_enable(1): one event pair around each
launch) over 5 further forward + backward calls: the kernels without the calls' fixed cost, and the forward kernel's share
of the peak.  Output: profiles/interpolate_times.txt (or --out)."""
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


def torch_interp(x, idx, w):
    b, m, k = idx.shape
    c = x.shape[1]
    return (x.gather(2, idx.reshape(b, 1, m * k).expand(-1, c, -1)).view(b, c, m, k) * w[:, None]).sum(-1)


def group_interp(x, idx, w):
    return (w[:, None] * ops.group_points(x, idx)).sum(-1)


def kernel_times(run, fwd_bytes):
    text = ''
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name, label in (('interp_fwd_kernel<lds>', 'fwd'), ('interp_bwd_x_kernel<lds>', 'grad_x'), ('interp_bwd_w_kernel', 'grad_w')):
            us, cnt = read(name)
            if cnt:
                text += f' {label} {us:.1f}'
                if label == 'fwd':
                    text += f' ({100 * fwd_bytes / (us * 1e-6) / HBM_PEAK:.0f}% of peak)'
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'interpolate_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, N sparse points on the unit sphere with features[B,C,N], M dense points, lists by '
             'knn_cross, weights by interpolation_weights; out [B,C,M]; microseconds per call: median of 7 rounds (min-max), the '
             'variants of a row alternating']
    # (B, N, M, k, C, also the gradient of the weights)
    rows = [(32, 128, 512, 3, 512, False), (32, 512, 2048, 3, 256, False), (32, 512, 2048, 3, 256, True), (32, 2048, 15000, 3, 128, False),
            (1, 2048, 15000, 3, 128, False), (32, 512, 2048, 8, 256, False)]
    for b, n, m, k, c, w_grad in rows:
        sparse = torch.nn.functional.normalize(torch.randn(b, 3, n, device=dev), dim=1)
        dense = torch.nn.functional.normalize(torch.randn(b, 3, m, device=dev), dim=1)
        idx, dist = ops.knn_cross(dense, sparse, k, return_distance=True)
        x = torch.randn(b, c, n, device=dev).requires_grad_(True)
        w = ops.interpolation_weights(dist).requires_grad_(w_grad)
        grad = torch.randn(b, c, m, device=dev)
        with torch.no_grad():  # the three formulations agree before they are timed
            ours = ops.interpolate_points(x, idx, w)
            for other in (torch_interp, group_interp):
                assert torch.allclose(ours, other(x, idx, w), rtol=1e-5, atol=1e-5)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn(x, idx, w)
            return run

        def fwd_bwd(fn):
            def run():
                x.grad = None
                w.grad = None
                fn(x, idx, w).backward(grad)
            return run

        variants = {}
        for name, fn in (('ours', ops.interpolate_points), ('torch', torch_interp), ('group', group_interp)):
            variants[name + '_fwd'], variants[name + '_fb'] = fwd(fn), fwd_bwd(fn)
        for path, name in ((1, 'lds'), (2, 'direct')):
            variants[name + '_fwd'] = with_switch('interp_path', path, fwd(ops.interpolate_points))
            variants[name + '_fb'] = with_switch('interp_path', path, fwd_bwd(ops.interpolate_points))
        big = b * c * m * k > 1 << 26
        t = medians(variants, iters=3 if big else 10, rounds=7, warm=2)
        nbytes = b * (c * n + m * k * 3 + c * m) * 4
        rate = nbytes / (t['ours_fwd'][0] * 1e-6)
        line = f'B={b:2d} N={n:5d} M={m:5d} k={k} C={c:3d}{" +w" if w_grad else "   "}:'
        for key, label in (('ours_fwd', 'fwd'), ('torch_fwd', 'torch fwd'), ('group_fwd', 'group fwd'), ('ours_fb', 'f+b'),
                           ('torch_fb', 'torch f+b'), ('group_fb', 'group f+b')):
            line += f'  {label} {t[key][0]:9.1f} ({t[key][1]:.1f}-{t[key][2]:.1f})'
        line += (f'  [torch / ours: fwd {t["torch_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["torch_fb"][0] / t["ours_fb"][0]:.2f}x; '
                 f'group / ours: fwd {t["group_fwd"][0] / t["ours_fwd"][0]:.2f}x, f+b {t["group_fb"][0] / t["ours_fb"][0]:.2f}x; '
                 f'moved {nbytes / 1e6:.0f} MB at {rate / 1e12:.2f} TB/s = {100 * rate / HBM_PEAK:.0f}% of peak]'
                 f'  paths: lds fwd {t["lds_fwd"][0]:.1f} f+b {t["lds_fb"][0]:.1f}, direct fwd {t["direct_fwd"][0]:.1f} f+b {t["direct_fb"][0]:.1f}')
        line += '  kernels:' + kernel_times(fwd_bwd(ops.interpolate_points), nbytes)
        print(line, flush=True)
        lines.append(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
