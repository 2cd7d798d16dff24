"""``pointnet2_ops`` with the names and signatures of erikwijmans/Pointnet2_PyTorch's op package (a CUDA-only extension), on
this library's HIP kernels: ``pointnet2_ops.pointnet2_utils`` and ``pointnet2_ops.pointnet2_modules``."""

from pointnet2_ops import pointnet2_modules, pointnet2_utils  # noqa: F401

__version__ = '3.0.0'
