"""PointNet2MSG, the point backbone of the reference's PointRCNN configuration
(pcdet/models/backbones_3d/pointnet2_backbone.py), with its state-dict keys (SA_modules.*, FP_modules.*).

batch_dict['points'] (B * N, 4 + C) [batch_idx, x, y, z, ...] with the samples stacked in order, N points each ->
batch_dict['point_features'] (B * N, FP_MLPS[0][-1]) and batch_dict['point_coords'] (B * N, 4).  The reference counts
the points of every sample on the host; here a row count that is no multiple of the batch size raises, and a kernel
checks on the device that row r carries sample r // N.  With check=True (the default) the status word of all the
launches of the forward is read ONCE, after the last of them; with check=False nothing is read from the device."""
import torch
import torch.nn as nn

from .. import pointnet2_ops as ops
from .._lib import Dfu3dError
from . import pointnet2_modules
from .base_bev_backbone import _get


class PointNet2MSG(nn.Module):
    def __init__(self, model_cfg, input_channels, check=True, **kwargs):
        super().__init__()
        self.model_cfg, self.check, self.status = model_cfg, check, None
        sa = _get(model_cfg, 'SA_CONFIG')
        npoints, fp_mlps = list(_get(sa, 'NPOINTS')), [list(m) for m in _get(model_cfg, 'FP_MLPS')]
        self.SA_modules = nn.ModuleList()
        channels = [input_channels - 3]                                   # features of level 0, 1, ...
        for k, npoint in enumerate(npoints):
            mlps = [[channels[-1]] + list(m) for m in _get(sa, 'MLPS')[k]]
            self.SA_modules.append(pointnet2_modules.PointnetSAModuleMSG(
                npoint=npoint, radii=list(_get(sa, 'RADIUS')[k]), nsamples=list(_get(sa, 'NSAMPLE')[k]), mlps=mlps,
                use_xyz=_get(sa, 'USE_XYZ', True)))
            channels.append(sum(m[-1] for m in mlps))
        self.FP_modules = nn.ModuleList()
        for k, mlp in enumerate(fp_mlps):                                 # level k + 1 propagated to level k
            above = fp_mlps[k + 1][-1] if k + 1 < len(fp_mlps) else channels[-1]
            self.FP_modules.append(pointnet2_modules.PointnetFPModule(mlp=[above + channels[k]] + mlp))
        self.num_point_features = fp_mlps[0][-1]

    def check_status(self):
        """Raises Dfu3dError if a launch of the last forward set a status bit (one host read)."""
        s = int(self.status.item()) if self.status is not None else 0
        if s:
            raise Dfu3dError("PointNet2MSG: status %d (%s)" % (s, ops.status_message(s)))

    def forward(self, batch_dict):
        batch_size, points = batch_dict['batch_size'], batch_dict['points']
        if points.dim() != 2 or points.shape[0] == 0 or points.shape[0] % batch_size != 0:
            raise Dfu3dError("PointNet2MSG: points %s are not %d samples of equal size"
                             % (tuple(points.shape), batch_size))
        points = points.contiguous()
        self.status = torch.zeros(1, dtype=torch.int32, device=points.device)
        with ops.status_scope(self.status):
            ops.check_batch(points, batch_size)
            xyz = points[:, 1:4].contiguous().view(batch_size, -1, 3)
            features = None
            if points.shape[1] > 4:
                features = points[:, 4:].reshape(batch_size, -1, points.shape[1] - 4).permute(0, 2, 1).contiguous()
            l_xyz, l_features = [xyz], [features]
            for sa in self.SA_modules:
                new_xyz, new_features = sa(l_xyz[-1], l_features[-1])
                l_xyz.append(new_xyz)
                l_features.append(new_features)
            for i in range(len(self.FP_modules), 0, -1):                  # level i into level i - 1
                l_features[i - 1] = self.FP_modules[i - 1](l_xyz[i - 1], l_xyz[i], l_features[i - 1], l_features[i])
        point_features = l_features[0].permute(0, 2, 1).contiguous()      # (B, N, C)
        batch_dict['point_features'] = point_features.view(-1, point_features.shape[-1])
        batch_dict['point_coords'] = torch.cat((points[:, 0:1], xyz.view(-1, 3)), dim=1)
        if self.check:
            self.check_status()
        return batch_dict
