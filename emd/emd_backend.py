"""The two functions of the reference's ``emd_backend`` pybind module (``external/emd/src/emd.cpp:14-30``) with their
argument lists, served by the persistent HIP auction kernel (``include/pcc_emd.h``).  The ten work tensors the
reference's seven kernels communicate through are accepted and left untouched: the auction state lives in LDS."""

from __future__ import annotations

import torch

from pointcloudcounterfactual_amd import _lib
from pointcloudcounterfactual_amd._lib import call, ptr

_L = _lib.lib
F32, I32 = torch.float32, torch.int32


def forward(xyz1, xyz2, dist, assignment, price=None, assignment_inv=None, bid=None, bid_increments=None,
            max_increments=None, unass_idx=None, unass_cnt=None, unass_cnt_sum=None, cnt_tmp=None, max_idx=None,
            eps: float = 0.005, iters: int = 50) -> int:
    """emd_cuda_forward (emd_cuda.cu:227-281): fills ``dist[B,n]`` and ``assignment[B,n]``; returns 1, or -1 with the
    reference's input errors (:235-248)."""
    b, n, _ = xyz1.shape
    if xyz2.shape[1] != n:
        print('Input Error! The two point clouds should have the same size.')
        return -1
    if b > 512:
        print('Input Error! The batch size should be less than 512.')
        return -1
    if n % 1024 != 0:
        print('Input Error! The size of the point clouds should be a multiple of 1024.')
        return -1
    dev = xyz1.device
    call(_L.pcc_auction_forward, 'emd forward', dev, b, n, ptr(xyz1, 'xyz1', F32, dev), ptr(xyz2, 'xyz2', F32, dev),
         float(eps), int(iters), ptr(dist, 'dist', F32, dev), ptr(assignment, 'assignment', I32, dev))
    return 1


def backward(xyz1, xyz2, gradxyz, graddist, idx) -> int:
    """emd_cuda_backward (emd_cuda.cu:301-315): ``gradxyz = 2 graddist (xyz1 - xyz2[idx])``."""
    b, n, _ = xyz1.shape
    dev = xyz1.device
    call(_L.pcc_auction_backward, 'emd backward', dev, b, n, ptr(xyz1, 'xyz1', F32, dev), ptr(xyz2, 'xyz2', F32, dev),
         ptr(graddist, 'graddist', F32, dev), ptr(idx, 'idx', I32, dev), ptr(gradxyz, 'gradxyz', F32, dev))
    return 1
