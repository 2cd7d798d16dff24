"""Timings of the local-geometry op (pcc_local_geometry / pcc_local_covariance_bwd, local_geometry.hip) beside the torch
formulation a user writes today, on the same GPU in the same process:
  cov       ours: local_covariance(xyz, idx); torch: get_local_covariance's body along the list -- the index list expanded
            to three channels, one gather of [B,3,M,k], the mean subtracted, a matmul of M 3 x k by k x 3 products (the
            concatenation with x left out: it is not part of either);
  geometry  ours: local_geometry(xyz, idx), all five outputs; torch: the above plus torch.linalg.eigh of the [B,M,3,3]
            matrices (eigenvalues and eigenvectors; no sign rule, no curvature);
  f+b       forward and backward of the covariance from a fixed incoming gradient (torch: autograd of the above).
Clouds are N Gaussian points; the lists are k-NN lists (pcc_knn, or pcc_knn_cross from M other points where M != N), the
last row a ball_query list (pad='first', which the torch formulation can gather without a mask) around M points of the
cloud.  The variants of a row alternate round by round; a figure is the median over 7 rounds of the mean time per call
inside a hipEvent bracket on the stream.  `moved` is what the full forward has to move once, the index list and the five
outputs = B * M * (8 k + 100) bytes, over its time, and its share of the 8 TB/s HBM peak.  `kernels` are the library's own
per-launch averages (pcc_profile_enable(1): one event pair around each launch) over 5 further calls: the kernels without
the calls' fixed cost, and the forward kernel's share of the peak.  Output: profiles/local_geometry_times.txt (or --out)."""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pointcloudcounterfactual_amd import _lib, neighbour_ops as ops  # noqa: E402
from time_knn_cross import medians  # noqa: E402

dev = torch.device('cuda:0')
HBM_PEAK = 8.0e12  # bytes per second


def torch_cov(xyz, idx):
    b, m, k = idx.shape
    nb = xyz.transpose(1, 2).gather(2, idx.reshape(b, 1, m * k).expand(-1, 3, -1)).view(b, 3, m, k)
    nb = nb - nb.mean(3, keepdim=True)
    return torch.matmul(nb.transpose(1, 2), nb.permute(0, 2, 3, 1))


def torch_geometry(xyz, idx):
    return torch.linalg.eigh(torch_cov(xyz, idx))


def kernel_times(run, fwd_bytes):
    text = ''
    with _lib.profile() as read:
        for _ in range(5):
            run()
        torch.cuda.synchronize()
        for name, label in (('local_geometry_kernel', 'fwd'), ('local_covariance_bwd_kernel<lds>', 'bwd lds'),
                            ('local_covariance_bwd_kernel<direct>', 'bwd direct')):
            us, cnt = read(name)
            if cnt:
                text += f' {label} {us:.1f}'
                if label == 'fwd':
                    text += f' ({100 * fwd_bytes / (us * 1e-6) / HBM_PEAK:.1f}% of peak)'
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'local_geometry_times.txt'))
    args = ap.parse_args()
    torch.manual_seed(0)
    lines = [f'{torch.cuda.get_device_name(0)}, N Gaussian points, M rows of k neighbours (knn / knn_cross; `ball`: ball_query, '
             "pad='first'); microseconds per call: median of 7 rounds (min-max), the variants of a row alternating"]
    # (B, N, M, k, a ball_query list)
    rows = [(32, 2048, 2048, 16, False), (32, 2048, 2048, 32, False), (32, 15000, 15000, 16, False), (1, 15000, 15000, 16, False),
            (32, 2048, 512, 32, True)]
    for b, n, m, k, ball in rows:
        xyz = torch.randn(b, n, 3, device=dev).requires_grad_(True)
        with torch.no_grad():
            if ball:
                idx = ops.ball_query(xyz, xyz[:, :m].contiguous(), 0.5, k)
            elif m == n:
                idx = ops.knn(xyz.transpose(1, 2).contiguous(), k)
            else:
                idx = ops.knn_cross(torch.randn(b, 3, m, device=dev), xyz.transpose(1, 2).contiguous(), k)
            # the two formulations agree before they are timed
            ours = ops.local_geometry(xyz, idx)
            theirs = torch_cov(xyz, idx)
            assert torch.allclose(ours.cov, theirs, rtol=1e-4, atol=1e-4)
            assert torch.allclose(ours.eigenvalues, torch.linalg.eigvalsh(theirs), rtol=1e-4, atol=1e-4 * float(theirs.abs().max()))
        grad = torch.randn(b, m, 3, 3, device=dev)

        def fwd(fn):
            def run():
                with torch.no_grad():
                    return fn(xyz, idx)
            return run

        def fwd_bwd(fn):
            def run():
                xyz.grad = None
                fn(xyz, idx).backward(grad)
            return run

        variants = {'ours_cov': fwd(ops.local_covariance), 'torch_cov': fwd(torch_cov), 'ours_geo': fwd(ops.local_geometry),
                    'torch_geo': fwd(torch_geometry), 'ours_fb': fwd_bwd(ops.local_covariance), 'torch_fb': fwd_bwd(torch_cov)}
        torch.cuda.synchronize()
        clock = time.perf_counter()
        variants['torch_geo']()
        torch.cuda.synchronize()
        slow = time.perf_counter() - clock > 0.2  # (a batched eigh of seconds: one call per bracket)
        t = medians(variants, iters=1 if slow else 3 if b * m > 100000 else 10, rounds=7, warm=1 if slow else 2)
        nbytes = b * m * (8 * k + 100)
        rate = nbytes / (t['ours_geo'][0] * 1e-6)
        line = f'B={b:2d} N={n:5d} M={m:5d} k={k:2d}{" ball" if ball else "     "}:'
        for key, label in (('ours_cov', 'cov'), ('torch_cov', 'torch cov'), ('ours_geo', 'geometry'), ('torch_geo', 'torch cov+eigh'),
                           ('ours_fb', 'cov f+b'), ('torch_fb', 'torch cov f+b')):
            line += f'  {label} {t[key][0]:9.1f} ({t[key][1]:.1f}-{t[key][2]:.1f})'
        line += (f'  [torch / ours: cov {t["torch_cov"][0] / t["ours_cov"][0]:.2f}x, geometry {t["torch_geo"][0] / t["ours_geo"][0]:.2f}x, '
                 f'cov f+b {t["torch_fb"][0] / t["ours_fb"][0]:.2f}x; moved {nbytes / 1e6:.1f} MB at {rate / 1e12:.3f} TB/s = '
                 f'{100 * rate / HBM_PEAK:.1f}% of peak]')

        def both():  # one forward with all five outputs, one backward
            xyz.grad = None
            ops.local_geometry(xyz, idx).cov.backward(grad)

        line += '  kernels:' + kernel_times(both, nbytes)
        print(line, flush=True)
        lines.append(line)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:  # (row by row: a run that is cut short leaves what it measured)
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
