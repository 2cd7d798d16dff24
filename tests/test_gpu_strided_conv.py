"""GPU test of the strided and transposed sparse convolution between two voxel levels: no HIP kernel serves these ops yet, and
nothing falls back to torch on the accelerator, so every one of them refuses an accelerator tensor by name."""

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_accelerator_tensors_are_refused_not_served_by_torch(cuda):
    from pointcloudcounterfactual_amd import neighbour_ops as ops

    xyz = torch.rand(2, 100, 3) - 0.5
    vindex = ops.voxel_index(xyz, 8)
    gindex = ops.grid_cluster(vindex)
    coarse, cgindex, tap = ops.coarsen_level(vindex, gindex)
    smap = ops.stride_map(tap, cgindex)
    m_f, m_c = smap.up.shape[1], smap.down.shape[1]
    dvindex = ops.voxel_index(xyz.to(cuda), 8)
    dgindex = ops.grid_cluster(dvindex)
    dmap = ops.StrideMap(*(t.to(cuda) for t in smap))
    w = torch.zeros(8, 3, 4, device=cuda)
    calls = {'coarsen_level': lambda: ops.coarsen_level(dvindex, dgindex),
             'stride_map': lambda: ops.stride_map(tap.to(cuda), ops.GridIndex(*(t.to(cuda) for t in cgindex))),
             'strided_sparse_conv': lambda: ops.strided_sparse_conv(torch.zeros(2, 3, m_f, device=cuda), dmap, w),
             'sparse_conv_transpose': lambda: ops.sparse_conv_transpose(torch.zeros(2, 3, m_c, device=cuda), dmap, w),
             'sparse_conv_wgrad': lambda: ops.sparse_conv_wgrad(torch.zeros(2, 3, m_f, device=cuda), dmap.down, torch.zeros(2, 4, m_c, device=cuda))}
    for name, fn in calls.items():
        with pytest.raises(RuntimeError, match=f'{name}: no HIP kernel serves this op yet'):
            fn()
    assert torch.equal(dgindex.count.cpu(), gindex.count)  # (the fine level itself is served on both devices)
