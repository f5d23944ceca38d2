"""The set-abstraction and feature-propagation modules of pcdet/ops/pointnet2/pointnet2_batch/pointnet2_modules.py:
the same constructor arguments, the same parameter names (`groupers`, `mlps`, `mlp`), so a reference state dict loads
with strict=True.  Sampling, ball query, grouping, the three nearest neighbours and the interpolation run on
csrc/pointnet2_stage.hip; the shared MLPs, the pooling, the weights 1 / (dist + 1e-8) with their normalisation and the
concatenations are torch calls in the reference's order.  An SA module samples once (the sampled coordinates come out
of the same launch) and queries the balls of all its scales in one launch."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import pointnet2_ops as ops
from . import pointnet2_utils


def _shared_mlp(spec):
    layers = []
    for cin, cout in zip(spec[:-1], spec[1:]):
        layers += [nn.Conv2d(cin, cout, kernel_size=1, bias=False), nn.BatchNorm2d(cout), nn.ReLU()]
    return nn.Sequential(*layers)


class PointnetSAModuleMSG(nn.Module):
    """Set abstraction with multi-scale grouping.  npoint None: one group of all points (GroupAll)."""

    def __init__(self, *, npoint, radii, nsamples, mlps, bn=True, use_xyz=True, pool_method='max_pool'):
        super().__init__()
        assert len(radii) == len(nsamples) == len(mlps)
        if pool_method not in ('max_pool', 'avg_pool'):
            raise NotImplementedError(pool_method)
        self.npoint, self.pool_method = npoint, pool_method
        self.groupers, self.mlps = nn.ModuleList(), nn.ModuleList()
        for radius, nsample, spec in zip(radii, nsamples, mlps):
            self.groupers.append(pointnet2_utils.QueryAndGroup(radius, nsample, use_xyz=use_xyz) if npoint is not None
                                 else pointnet2_utils.GroupAll(use_xyz))
            self.mlps.append(_shared_mlp([spec[0] + (3 if use_xyz else 0)] + list(spec[1:])))

    def ball_indices(self, xyz, new_xyz):
        """The ball indices of every scale, DFU3D_PN2_MAX_SCALES scales per launch (one launch for the usual two)."""
        out = []
        for i in range(0, len(self.groupers), ops.MAX_SCALES):
            g = self.groupers[i:i + ops.MAX_SCALES]
            out += ops.ball_query(xyz, new_xyz, [m.radius for m in g], [m.nsample for m in g])
        return out

    def forward(self, xyz, features=None, new_xyz=None):
        """xyz (B, N, 3), features (B, C, N) -> new_xyz (B, npoint, 3), new_features (B, sum_k mlps[k][-1], npoint)."""
        if new_xyz is None and self.npoint is not None:
            new_xyz = ops.fps(xyz, self.npoint)[1]
        idx = self.ball_indices(xyz, new_xyz) if self.npoint is not None else None
        pooled = []
        for i, (grouper, mlp) in enumerate(zip(self.groupers, self.mlps)):
            x = grouper(xyz, new_xyz, features, idx=idx[i]) if idx is not None else grouper(xyz, new_xyz, features)
            x = mlp(x)                                                        # (B, mlp[-1], npoint, nsample)
            pool = F.max_pool2d if self.pool_method == 'max_pool' else F.avg_pool2d
            pooled.append(pool(x, kernel_size=[1, x.size(3)]).squeeze(-1))    # (B, mlp[-1], npoint)
        return new_xyz, torch.cat(pooled, dim=1)


class PointnetSAModule(PointnetSAModuleMSG):
    """Set abstraction with one scale."""

    def __init__(self, *, mlp, npoint=None, radius=None, nsample=None, bn=True, use_xyz=True, pool_method='max_pool'):
        super().__init__(mlps=[mlp], npoint=npoint, radii=[radius], nsamples=[nsample], bn=bn, use_xyz=use_xyz,
                         pool_method=pool_method)


class PointnetFPModule(nn.Module):
    """Feature propagation: the features of `known` interpolated at `unknown` from its three nearest neighbours."""

    def __init__(self, *, mlp, bn=True):
        super().__init__()
        self.mlp = _shared_mlp(list(mlp))

    def forward(self, unknown, known, unknow_feats, known_feats):
        """unknown (B, n, 3), known (B, m, 3), unknow_feats (B, C1, n), known_feats (B, C2, m) -> (B, mlp[-1], n)."""
        if known is not None:
            dist, idx = pointnet2_utils.three_nn(unknown, known)
            recip = 1.0 / (dist + 1e-8)
            x = pointnet2_utils.three_interpolate(known_feats, idx, recip / recip.sum(dim=2, keepdim=True))
        else:
            x = known_feats.expand(*known_feats.size()[0:2], unknown.size(1))
        if unknow_feats is not None:
            x = torch.cat([x, unknow_feats], dim=1)                           # (B, C2 + C1, n)
        return self.mlp(x.unsqueeze(-1)).squeeze(-1)
