"""MI355X-native structural losses for PointCloudCounterfactual's hot path.

Importing the package loads ``lib/libpcc_structural.so`` (hand-written HIP for gfx950); it raises
``ImportError`` if the library has not been built -- there is no CPU / PyTorch fallback.
"""

from pointcloudcounterfactual_amd import _lib, backend, set_metrics  # noqa: F401
from pointcloudcounterfactual_amd.losses import (  # noqa: F401
    MatchCostFunction,
    NNDistanceFunction,
    chamfer,
    chamfer_emd,
    match_cost,
    nn_distance,
    random_directions,
    sinkhorn_divergence,
    sinkhorn_schedule,
    sliced_wasserstein,
    torch_chamfer,
    torch_sinkhorn,
    torch_sliced_wasserstein,
)
from pointcloudcounterfactual_amd.neighbour_ops import (  # noqa: F401
    GridIndex,
    GridPooled,
    KernelPointConv,
    SparseConvMap,
    SubmanifoldConv3d,
    VoxelIndex,
    aggregate_points,
    attention_aggregate,
    ball_query,
    cell_neighbours,
    devoxelize,
    estimate_normals,
    farthest_point_sample,
    feature_propagation,
    grid_cluster,
    grid_pool,
    grid_subsample,
    grid_unpool,
    group_points,
    interpolate_points,
    interpolation_weights,
    kernel_point_conv,
    kernel_point_influence,
    kernel_point_layout,
    kpconv_aggregate,
    local_covariance,
    local_geometry,
    neighbour_softmax,
    point_voxel,
    sample_and_group,
    segment_pool,
    sparse_conv,
    vector_attention,
    voxel_index,
    voxelize,
)
from pointcloudcounterfactual_amd.set_metrics import jsd_between_sets, occupancy_grid  # noqa: F401

__all__ = ['match_cost', 'nn_distance', 'chamfer', 'chamfer_emd', 'torch_chamfer', 'MatchCostFunction', 'NNDistanceFunction',
           'backend', 'set_metrics', 'farthest_point_sample', 'ball_query', 'group_points', 'sample_and_group',
           'occupancy_grid', 'jsd_between_sets', 'interpolation_weights', 'interpolate_points', 'feature_propagation',
           'local_covariance', 'local_geometry', 'estimate_normals', 'sliced_wasserstein', 'torch_sliced_wasserstein',
           'random_directions', 'sinkhorn_divergence', 'sinkhorn_schedule', 'torch_sinkhorn', 'VoxelIndex', 'voxel_index',
           'voxelize', 'devoxelize', 'point_voxel', 'neighbour_softmax', 'aggregate_points', 'attention_aggregate',
           'vector_attention', 'kernel_point_layout', 'kernel_point_influence', 'kpconv_aggregate', 'kernel_point_conv',
           'KernelPointConv', 'GridIndex', 'GridPooled', 'grid_cluster', 'segment_pool', 'grid_pool', 'grid_subsample',
           'grid_unpool', 'SparseConvMap', 'cell_neighbours', 'sparse_conv', 'SubmanifoldConv3d']
