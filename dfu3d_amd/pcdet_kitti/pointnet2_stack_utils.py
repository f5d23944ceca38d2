"""pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py on csrc/pointstack_stage.hip: `ball_query`,
`grouping_operation`, `QueryAndGroup`, `farthest_point_sample` with the reference's arguments -- stacked tensors and
per-sample counts int32 (B) on the device.  The starts the stage wants are built once per count tensor
(point_stack_ops.starts_of) and kept on it.

Differences from the reference, all in layout and none in value: QueryAndGroup returns (3 + C, M, nsample), the order
the shared MLP's 1x1 convolution reads (the reference returns (M, 3 + C, nsample) and permutes); the coordinates may be
columns of a wider block (`points[:, 1:4]`) and are read in place; `grouping_operation` returns a permuted view."""
import torch
import torch.nn as nn

from .. import point_stack_ops as ops
from .. import pointnet2_ops as batched_ops


def ball_query(radius, nsample, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
    """-> idx int32 (M, nsample), sample-local; empty_ball_mask bool (M).  An empty ball's slots are 0."""
    (idx, empty), = ops.ball_query(xyz, ops.starts_of(xyz_batch_cnt), new_xyz, ops.starts_of(new_xyz_batch_cnt),
                                   [radius], [nsample])
    return idx, empty.bool()


def grouping_operation(features, features_batch_cnt, idx, idx_batch_cnt):
    """features (N, C), idx (M, nsample) sample-local -> (M, C, nsample), with the gradient of the features."""
    empty = torch.zeros(idx.shape[0], dtype=torch.uint8, device=idx.device)
    out = ops.query_group(None, ops.starts_of(features_batch_cnt), None, ops.starts_of(idx_batch_cnt), features, idx,
                          empty)
    return out.permute(1, 0, 2)


def farthest_point_sample(xyz, npoint):
    """xyz (B, N, 3) -> idx int32 (B, npoint): the batched op (pointnet2_ops.fps), as the reference's name promises."""
    return batched_ops.fps(xyz, npoint)[0]


furthest_point_sample = farthest_point_sample


class QueryAndGroup(nn.Module):
    def __init__(self, radius, nsample, use_xyz=True):
        super().__init__()
        self.radius, self.nsample, self.use_xyz = radius, nsample, use_xyz

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, ball=None):
        """-> new_features (3 + C, M, nsample) (use_xyz) or (C, M, nsample), idx (M, nsample).  ball: (idx, empty uint8)
        of this scale when the caller has queried all scales of its module in one launch."""
        start, cstart = ops.starts_of(xyz_batch_cnt), ops.starts_of(new_xyz_batch_cnt)
        if ball is None:
            (ball,) = ops.ball_query(xyz, start, new_xyz, cstart, [self.radius], [self.nsample])
        idx, empty = ball
        if features is None:
            assert self.use_xyz, "Cannot have not features and not use xyz as a feature!"
        out = ops.query_group(xyz, start, new_xyz, cstart, features, idx, empty)
        if not self.use_xyz:
            out = out[3:]
        return out, idx
