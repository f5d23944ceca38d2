"""pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py: `StackSAModuleMSG` and `build_local_aggregation_module`,
with the reference's constructor arguments and parameter names (`groupers`, `mlps`), so a reference state dict loads
with strict=True.  Ball query and grouping run on csrc/pointstack_stage.hip: ONE ball launch serves all scales of a
module, one grouping launch per scale writes the (1, 3 + C, M, nsample) tensor the shared MLP reads -- no subtraction,
masked fill or permute in between.  The MLPs, the pooling and the concatenation are torch calls in the reference's
order."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import point_stack_ops as ops
from . import pointnet2_stack_utils
from .common_utils import cfg_get


def build_local_aggregation_module(input_channels, config):
    """-> (module, output channels).  The configuration is not written to (the reference prepends to its MLPS lists)."""
    name = cfg_get(config, 'NAME', 'StackSAModuleMSG')
    if name == 'StackSAModuleMSG':
        mlps = [[input_channels] + list(m) for m in cfg_get(config, 'MLPS')]
        layer = StackSAModuleMSG(radii=cfg_get(config, 'POOL_RADIUS'), nsamples=cfg_get(config, 'NSAMPLE'), mlps=mlps,
                                 use_xyz=True, pool_method='max_pool')
        return layer, sum(m[-1] for m in mlps)
    if name == 'VectorPoolAggregationModuleMSG':
        return VectorPoolAggregationModuleMSG(input_channels=input_channels, config=config), None
    raise NotImplementedError(name)


class StackSAModuleMSG(nn.Module):
    def __init__(self, *, radii, nsamples, mlps, use_xyz=True, pool_method='max_pool'):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        if pool_method not in ('max_pool', 'avg_pool'):
            raise NotImplementedError(pool_method)
        self.groupers, self.mlps = nn.ModuleList(), nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_stack_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz))
            spec = [spec[0] + (3 if use_xyz else 0)] + list(spec[1:])
            layers = []
            for cin, cout in zip(spec[:-1], spec[1:]):
                layers += [nn.Conv2d(cin, cout, kernel_size=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU()]
            self.mlps.append(nn.Sequential(*layers))
        self.pool_method = pool_method
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            if isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0)

    def ball_indices(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt):
        """[(idx, empty)] of every scale, DFU3D_STK_MAX_SCALES scales per launch (one launch for the usual two)."""
        start, cstart = ops.starts_of(xyz_batch_cnt), ops.starts_of(new_xyz_batch_cnt)
        out = []
        for i in range(0, len(self.groupers), ops.MAX_SCALES):
            g = self.groupers[i:i + ops.MAX_SCALES]
            out += ops.ball_query(xyz, start, new_xyz, cstart, [m.radius for m in g], [m.nsample for m in g])
        return out

    def forward(self, xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features=None, empty_voxel_set_zeros=True):
        """xyz (N, 3), new_xyz (M, 3), features (N, C) -> new_xyz, new_features (M, sum_k mlps[k][-1])."""
        balls = self.ball_indices(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt)
        pooled = []
        for grouper, mlp, ball in zip(self.groupers, self.mlps, balls):
            x, _ = grouper(xyz, xyz_batch_cnt, new_xyz, new_xyz_batch_cnt, features, ball=ball)
            x = mlp(x.unsqueeze(0))                                           # (1, mlp[-1], M, nsample)
            pool = F.max_pool2d if self.pool_method == 'max_pool' else F.avg_pool2d
            x = pool(x, kernel_size=[1, x.size(3)]).squeeze(-1)               # (1, mlp[-1], M)
            pooled.append(x.squeeze(0).permute(1, 0))
        return new_xyz, torch.cat(pooled, dim=1)


class VectorPoolAggregationModuleMSG(nn.Module):
    def __init__(self, input_channels, config):
        raise NotImplementedError("VectorPoolAggregationModuleMSG (PV-RCNN++) is not part of this package")
