"""pcdet/ops/pointnet2/pointnet2_batch/pointnet2_utils.py under its own names, over dfu3d_amd.pointnet2_ops
(csrc/pointnet2_stage.hip): the same signatures and return types.  Recorded divergence: among points of
exactly equal running minimum farthest point sampling picks the lowest index; the reference's pick depends on its block
size."""
import torch
import torch.nn as nn

from .. import pointnet2_ops as ops


def furthest_point_sample(xyz, npoint):
    """xyz (B, N, 3) -> int32 (B, npoint)."""
    return ops.fps(xyz, npoint)[0]


farthest_point_sample = furthest_point_sample


def grouping_operation(features, idx):
    """features (B, C, N), idx int32 (B, npoint, nsample) -> (B, C, npoint, nsample)."""
    return ops.grouping(features, idx)


def gather_operation(features, idx):
    """features (B, C, N), idx int32 (B, npoint) -> (B, C, npoint): grouping with one sample per group."""
    return ops.grouping(features, idx.unsqueeze(-1)).squeeze(-1)


def three_nn(unknown, known):
    """unknown (B, n, 3), known (B, m, 3) -> dist (B, n, 3), idx int32 (B, n, 3)."""
    return ops.three_nn(unknown, known)


def three_interpolate(features, idx, weight):
    """features (B, C, m), idx (B, n, 3), weight (B, n, 3) -> (B, C, n)."""
    return ops.interpolate(features, idx, weight)


def ball_query(radius, nsample, xyz, new_xyz):
    """-> int32 (B, npoint, nsample)."""
    return ops.ball_query(xyz, new_xyz, [radius], [nsample])[0]


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, new_xyz, features=None, idx=None):
        """xyz (B, N, 3), new_xyz (B, npoint, 3), features (B, C, N) -> (B, 3 + C, npoint, nsample).  idx: the ball
        indices when the caller has them already (the SA module queries all its scales in one launch)."""
        assert features is not None or self.use_xyz, "Cannot have not features and not use xyz as a feature!"
        if idx is None:
            idx = ball_query(self.radius, self.nsample, xyz, new_xyz)
        return ops.query_group(xyz, new_xyz, features, idx, self.use_xyz)


class GroupAll(nn.Module):
    def __init__(self, use_xyz=True):
        super().__init__()
        self.use_xyz = use_xyz

    def forward(self, xyz, new_xyz, features=None):
        """-> (B, C + 3, 1, N); new_xyz is ignored."""
        parts = []
        if features is None or self.use_xyz:
            parts.append(xyz.transpose(1, 2).unsqueeze(2))
        if features is not None:
            parts.append(features.unsqueeze(2))
        return parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
