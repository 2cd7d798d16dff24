"""kNN-graph operations with the reference's Python API (``src/utils/neighbour_ops.py:63-133``).

On the accelerator every function runs hand-written HIP kernels through the C ABI
(``include/pcc_neighbour.h``); the reference uses PyKeOps there, which has no ROCm backend.  For CPU tensors the
functions follow the reference's own device dispatch (``neighbour_ops.py:29,65``) and evaluate its torch
formulas -- that is the reference's CPU path, not a fallback of the GPU path: an accelerator tensor never
leaves the device, and a missing HIP library is an ``ImportError``.

Layouts are the reference's: ``x[B,C,N]`` float32, ``indices[B,N,k]`` int64 (an empty ``indices`` tensor means
"compute the kNN now", ``:88-91``).

One module per op family; this file only re-exports them, so every caller imports from here.
"""

from pointcloudcounterfactual_amd.neighbour_ops._args import F32, I32, I64  # noqa: F401
from pointcloudcounterfactual_amd.neighbour_ops.search import (  # noqa: F401
    cross_square_distance, hip_knn, hip_knn_cross, index_k_neighbours, knn, knn_cross, pykeops_knn, pykeops_square_distance,
    self_square_distance, square_distance, torch_knn, torch_knn_cross, torch_square_distance)
from pointcloudcounterfactual_amd.neighbour_ops.sampling import (  # noqa: F401
    BALL_PAD, ball_query, farthest_point_sample, hip_ball_query, hip_farthest_point_sample, torch_ball_query,
    torch_farthest_point_sample)
from pointcloudcounterfactual_amd.neighbour_ops.ragged import (  # noqa: F401
    MAX_RAGGED_K, ball_query_ragged, batch2offset, farthest_point_sample_ragged, hip_ball_query_ragged, hip_knn_ragged, knn_ragged,
    offset2batch, offset2bincount, torch_ball_query_ragged, torch_knn_ragged)
from pointcloudcounterfactual_amd.neighbour_ops.grouping import (  # noqa: F401
    Grouped, QueryGrouped, SampleAndGroup, group_points, group_points_relative, query_and_group, sample_and_group,
    torch_group_points)
from pointcloudcounterfactual_amd.neighbour_ops.interpolate import (  # noqa: F401
    FeaturePropagation, Interpolated, feature_propagation, interpolate_points, interpolation_weights, torch_interpolate_points)
from pointcloudcounterfactual_amd.neighbour_ops.attention import (  # noqa: F401
    MAX_LIST_K, AggregatedPoints, NeighbourSoftmax, aggregate_points, attention_aggregate, neighbour_softmax, torch_aggregate_points,
    torch_aggregate_points_bwd, torch_neighbour_softmax, torch_neighbour_softmax_bwd, vector_attention)
from pointcloudcounterfactual_amd.neighbour_ops.kpconv import (  # noqa: F401
    MAX_KERNEL_POINTS, KernelPointAggregated, KernelPointConv, hip_kpconv_aggregate, kernel_point_conv, kernel_point_influence,
    kernel_point_layout, kpconv_aggregate, torch_kpconv_aggregate, torch_kpconv_aggregate_bwd)
from pointcloudcounterfactual_amd.neighbour_ops.voxel import (  # noqa: F401
    MAX_VOXEL_POINTS, Devoxelized, VoxelIndex, Voxelized, devoxelize, point_voxel, torch_devoxelize, torch_voxel_index, torch_voxelize,
    voxel_index, voxelize)
from pointcloudcounterfactual_amd.neighbour_ops.pooling import (  # noqa: F401
    GridIndex, GridPooled, SegmentPooled, grid_cluster, grid_pool, grid_subsample, grid_unpool, segment_pool, torch_grid_cluster,
    torch_segment_pool, torch_segment_pool_bwd)
from pointcloudcounterfactual_amd.neighbour_ops.ragged_grid import (  # noqa: F401
    GRID_RAGGED_TILE, MAX_AXIS_BITS, RaggedGrid, RaggedGridPooled, default_axis_bits, grid_cluster_ragged, grid_pool_ragged,
    grid_unpool_ragged, hip_grid_cluster_ragged, ragged_grid_start, torch_grid_cluster_ragged)
from pointcloudcounterfactual_amd.neighbour_ops.sparse import (  # noqa: F401
    KERNEL_SIZES, SparseConvMap, SparseConvolved, SubmanifoldConv3d, cell_neighbours, sparse_conv, torch_cell_neighbours,
    torch_sparse_conv)
from pointcloudcounterfactual_amd.neighbour_ops.ragged_sparse import (  # noqa: F401
    cell_neighbours_ragged, hip_cell_neighbours_ragged, sparse_conv_ragged, torch_cell_neighbours_ragged)
from pointcloudcounterfactual_amd.neighbour_ops.strided import (  # noqa: F401
    MAX_WGRAD_ROWS, STRIDE_TAPS, SparseConv3d, SparseConvTranspose3d, StrideMap, coarsen_level, sparse_conv_transpose,
    sparse_conv_wgrad, stride_map, strided_sparse_conv, torch_coarsen_cells, torch_sparse_conv_wgrad, torch_stride_map)
from pointcloudcounterfactual_amd.neighbour_ops.geometry import (  # noqa: F401
    LocalCovariance, LocalGeometry, estimate_normals, local_covariance, local_geometry, torch_local_covariance, torch_scatter_eigen)
from pointcloudcounterfactual_amd.neighbour_ops.graph import (  # noqa: F401
    GATHER, GRAPH_FEATURES, GRAPH_MAX_POOL, Indexed, IndexedOp, get_graph_features, get_local_covariance, get_neighbours,
    global_max_mean_pool, global_max_pool, graph_filtering, graph_max_pooling)
