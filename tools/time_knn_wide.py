"""Timings of the wide k-NN path (knn_wide.hip: k > 32 or c > 128) at B = 32, N = 2048 against the stock-torch formula of
tools/time_knn.py (expanded-form distances through bmm, then topk).  Output: profiles/knn_wide_times.txt."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pointcloudcounterfactual_amd import neighbour_ops as ops  # noqa: E402

dev = torch.device('cuda:0')


def ev(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def torch_knn(x, k):
    inner = -2 * torch.bmm(x.transpose(2, 1), x)
    xx = (x ** 2).sum(dim=1, keepdim=True)
    return (inner + xx + xx.transpose(2, 1)).topk(k, dim=-1, largest=False)[1]


B, N = 32, 2048
torch.manual_seed(0)
print(f'{torch.cuda.get_device_name(0)}, B = {B}, N = {N}, Gaussian clouds; microseconds per call (mean of 20)')
for c, k in ((3, 40), (3, 64), (3, 128), (64, 40), (128, 64), (128, 128), (256, 20), (256, 40)):
    x = torch.randn(B, c, N, device=dev)
    t_hip = ev(lambda: ops.hip_knn(x, k))
    t_torch = ev(lambda: torch_knn(x, k), iters=5, warm=2)
    print(f'c={c:4d} k={k:4d}: wide path {t_hip:9.1f} us   stock torch bmm+topk {t_torch:9.1f} us   ({t_torch / t_hip:.1f}x)')
