"""`RoIPointPool3d` and `RoIPointPool3dFunction` under the names of pcdet/ops/roipoint_pool3d/roipoint_pool3d_utils.py,
on the HIP kernels of csrc/roipoint_stage.hip (dfu3d_amd.roipoint_ops.pool): points (B, N, 3), point_features (B, N, C),
boxes3d (B, M, 7) -> pooled_features (B, M, S, 3 + C) with raw coordinates, pooled_empty_flag int32 (B, M).  The extra
width is added to the boxes' dims inside the kernel, in float32 as box_utils.enlarge_box3d adds it; no enlarged copy of
the boxes is made.  There is no backward, as in the reference."""
import torch

from .. import roipoint_ops


class RoIPointPool3dFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, point_features, boxes3d, pool_extra_width, num_sampled_points=512):
        if points.dim() != 3 or points.shape[2] != 3:
            raise ValueError("RoIPointPool3d: points must be (B, N, 3), got %s" % (tuple(points.shape),))
        pooled, empty = roipoint_ops.pool(points.contiguous(), point_features.contiguous(), boxes3d,
                                          pool_extra_width, num_sampled_points)
        ctx.mark_non_differentiable(empty)
        return pooled, empty

    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError


class RoIPointPool3d(torch.nn.Module):
    def __init__(self, num_sampled_points=512, pool_extra_width=1.0):
        super().__init__()
        self.num_sampled_points, self.pool_extra_width = num_sampled_points, pool_extra_width

    def forward(self, points, point_features, boxes3d):
        return RoIPointPool3dFunction.apply(points, point_features, boxes3d, self.pool_extra_width,
                                            self.num_sampled_points)
