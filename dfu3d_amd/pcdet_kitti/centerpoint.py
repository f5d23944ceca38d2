"""pcdet/models/detectors/centerpoint.py (over detector3d_template.py) assembled from this package's modules:
`vfe` (DynamicPillarVFE) -> `map_to_bev_module` (PointPillarScatter) -> `backbone_2d` (BaseBEVBackbone) -> `dense_head`
(CenterHeadModule), with the reference's submodule names and its `global_step` buffer, so a reference checkpoint's
'model_state' loads with strict=True.

`forward(batch_dict)` in training returns ({'loss': loss}, tb_dict, disp_dict) with tb_dict['loss_rpn'] (tb_dict is
read from the device in one copy); in evaluation (pred_dicts, recall_dict).  Module names of the config this package
does not have (a BACKBONE_3D, PFE, POINT_HEAD, ROI_HEAD entry, another VFE / MAP_TO_BEV / BACKBONE_2D / DENSE_HEAD name)
raise NotImplementedError naming them.

`CenterPoint(..., sparse_3d=True)` is the voxel model of cfgs/kitti_models/centerpoint.yaml: `vfe` (MeanVFE) ->
`backbone_3d` (VoxelBackBone8x / VoxelResBackBone8x on the sparse convolution stage) -> `map_to_bev_module`
(HeightCompression) -> `backbone_2d` -> `dense_head`.  Without the keyword those names raise as before."""
import os

import torch
import torch.nn as nn

from . import iou3d_nms_utils
from .base_bev_backbone import BaseBEVBackbone
from .center_head_module import CenterHeadModule
from .dynamic_pillar_vfe import DynamicPillarVFE, DynamicPillarVFESimple2D
from .height_compression import HeightCompression
from .mean_vfe import MeanVFE
from .pointpillar_scatter import PointPillarScatter, PointPillarScatter3d
from .spconv_backbone import VoxelBackBone8x, VoxelResBackBone8x
from .spconv_utils import find_all_spconv_keys


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg[key] if not default else cfg.get(key, default[0])
    return getattr(cfg, key) if not default else getattr(cfg, key, default[0])


MODULES = {
    'VFE': {'DynPillarVFE': DynamicPillarVFE, 'DynamicPillarVFE': DynamicPillarVFE,
            'DynamicPillarVFESimple2D': DynamicPillarVFESimple2D},
    'MAP_TO_BEV': {'PointPillarScatter': PointPillarScatter, 'PointPillarScatter3d': PointPillarScatter3d},
    'BACKBONE_2D': {'BaseBEVBackbone': BaseBEVBackbone},
    'DENSE_HEAD': {'CenterHead': CenterHeadModule},
}
ABSENT = ('BACKBONE_3D', 'PFE', 'POINT_HEAD', 'ROI_HEAD')
# what sparse_3d=True adds
SPARSE_MODULES = {
    'VFE': {'MeanVFE': MeanVFE},
    'BACKBONE_3D': {'VoxelBackBone8x': VoxelBackBone8x, 'VoxelResBackBone8x': VoxelResBackBone8x},
    'MAP_TO_BEV': {'HeightCompression': HeightCompression},
}


class _Dataset:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _module_class(model_cfg, section, sparse_3d=False, more=None, who="CenterPoint"):
    """more: {section: {name: class}} a detector built on this assembly accepts on top (SECONDNet: its dense head)."""
    cfg = _get(model_cfg, section, None)
    if cfg is None:
        return None, None
    name = _get(cfg, 'NAME')
    known = dict(MODULES.get(section, {}), **(SPARSE_MODULES.get(section, {}) if sparse_3d else {}))
    known.update((more or {}).get(section, {}))
    if name not in known:
        raise NotImplementedError("%s: %s.NAME = %r is not part of this package (it has %s)"
                                  % (who, section, name, ", ".join(sorted(known))))
    return cfg, known[name]


def adapt_spconv_weights(model, model_state):
    """detector3d_template.py _load_state_dict: a sparse convolution's weight in the 1.x layout (k, k, k, Cin, Cout)
    becomes the model's (Cout, k, k, k, Cin), by the transpose of the last two axes or by the permutation, whichever
    gives the parameter's shape; everything else is passed on as it is."""
    own, keys, out = model.state_dict(), find_all_spconv_keys(model), {}
    for key, val in model_state.items():
        if key in keys and key in own and own[key].shape != val.shape:
            native = val.transpose(-1, -2)
            if native.shape == own[key].shape:
                val = native.contiguous()
            elif val.dim() == 5 and val.permute(4, 0, 1, 2, 3).shape == own[key].shape:
                val = val.permute(4, 0, 1, 2, 3).contiguous()
        out[key] = val
    return out


class CenterPoint(nn.Module):
    MORE_MODULES = {}                # what a subclass accepts on top of MODULES / SPARSE_MODULES

    def __init__(self, model_cfg, num_class, dataset=None, sparse_3d=False, **kwargs):
        """dataset: an object with class_names, grid_size, point_cloud_range, voxel_size and
        point_feature_encoder.num_point_features -- or the same as keywords (num_point_features for the last).
        sparse_3d: accept MeanVFE, a BACKBONE_3D (VoxelBackBone8x, VoxelResBackBone8x) and HeightCompression."""
        super().__init__()
        if dataset is None:
            feats = kwargs.pop('num_point_features')
            dataset = _Dataset(point_feature_encoder=_Dataset(num_point_features=feats), **kwargs)
        self.model_cfg = model_cfg
        self.num_class = num_class
        self.dataset = dataset
        self.class_names = list(dataset.class_names)
        self.register_buffer('global_step', torch.LongTensor(1).zero_())
        absent = [s for s in ABSENT if _get(model_cfg, s, None) and not (sparse_3d and s == 'BACKBONE_3D')
                  and s not in self.MORE_MODULES]           # (a subclass builds the sections it names itself)
        if absent:
            raise NotImplementedError("CenterPoint: the config's %s is not part of this package" % ", ".join(absent))
        grid_size = [int(v) for v in dataset.grid_size]
        pc_range = [float(v) for v in dataset.point_cloud_range]
        voxel_size = [float(v) for v in dataset.voxel_size]
        self.module_list = []
        num_bev = None
        cfg, cls = _module_class(model_cfg, 'VFE', sparse_3d)
        self.vfe = None
        num_point_features = dataset.point_feature_encoder.num_point_features
        if cls is not None:
            self.vfe = cls(model_cfg=cfg, num_point_features=num_point_features,
                           point_cloud_range=pc_range, voxel_size=voxel_size, grid_size=grid_size)
            self.module_list.append(self.vfe)
        if sparse_3d:
            cfg, cls = _module_class(model_cfg, 'BACKBONE_3D', True)
            self.backbone_3d = None
            if cls is not None:
                if isinstance(self.vfe, MeanVFE):
                    num_point_features = self.vfe.get_output_feature_dim()
                self.backbone_3d = cls(model_cfg=cfg, input_channels=num_point_features, grid_size=grid_size,
                                       voxel_size=voxel_size, point_cloud_range=pc_range)
                self.module_list.append(self.backbone_3d)
        cfg, cls = _module_class(model_cfg, 'MAP_TO_BEV', sparse_3d)
        self.map_to_bev_module = None
        if cls is not None:
            self.map_to_bev_module = cls(model_cfg=cfg, grid_size=grid_size)
            num_bev = self.map_to_bev_module.num_bev_features
            self.module_list.append(self.map_to_bev_module)
        cfg, cls = _module_class(model_cfg, 'BACKBONE_2D')
        self.backbone_2d = None
        if cls is not None:
            self.backbone_2d = cls(model_cfg=cfg, input_channels=num_bev)
            num_bev = self.backbone_2d.num_bev_features
            self.module_list.append(self.backbone_2d)
        cfg, cls = _module_class(model_cfg, 'DENSE_HEAD', more=self.MORE_MODULES, who=type(self).__name__)
        self.dense_head = None
        if cls is not None:
            self.dense_head = cls(
                model_cfg=cfg, input_channels=num_bev if num_bev is not None else _get(cfg, 'INPUT_FEATURES'),
                num_class=num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1, class_names=self.class_names,
                grid_size=grid_size, point_cloud_range=pc_range, voxel_size=voxel_size,
                predict_boxes_when_training=bool(_get(model_cfg, 'ROI_HEAD', False)))
            self.module_list.append(self.dense_head)

    @property
    def mode(self):
        return 'TRAIN' if self.training else 'TEST'

    def update_global_step(self):
        self.global_step += 1

    def forward(self, batch_dict):
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        if self.training:
            loss, tb_dict, disp_dict = self.get_training_loss()
            return {'loss': loss}, tb_dict, disp_dict
        return self.post_processing(batch_dict)

    def get_training_loss(self):
        loss_rpn, tb_dict = self.dense_head.get_loss()
        tb_dict = {'loss_rpn': tb_dict['rpn_loss'], **tb_dict}          # the value get_loss read already: no second copy
        return loss_rpn, tb_dict, {}

    def post_processing(self, batch_dict):
        thresh_list = _get(_get(self.model_cfg, 'POST_PROCESSING'), 'RECALL_THRESH_LIST')
        final_pred_dict = batch_dict['final_box_dicts']
        recall_dict = {}
        for index in range(batch_dict['batch_size']):
            recall_dict = self.generate_recall_record(final_pred_dict[index]['pred_boxes'], recall_dict, index,
                                                      data_dict=batch_dict, thresh_list=thresh_list)
        return final_pred_dict, recall_dict

    @staticmethod
    def generate_recall_record(box_preds, recall_dict, batch_index, data_dict=None, thresh_list=None):
        """detector3d_template.py generate_recall_record: the ground-truth boxes of a sample (its trailing all-zero rows
        cut) that some prediction ('rcnn_%s') or roi ('roi_%s') overlaps by more than each threshold, accumulated."""
        if 'gt_boxes' not in data_dict:
            return recall_dict
        rois = data_dict['rois'][batch_index] if 'rois' in data_dict else None
        gt = data_dict['gt_boxes'][batch_index]
        if len(recall_dict) == 0:
            recall_dict = {'gt': 0}
            for t in thresh_list:
                recall_dict['roi_%s' % str(t)] = 0
                recall_dict['rcnn_%s' % str(t)] = 0
        nonzero = (gt.sum(dim=1) != 0).nonzero()
        gt = gt[:int(nonzero[-1]) + 1] if len(nonzero) else gt[:0]
        if gt.shape[0] > 0:
            iou_rcnn = iou3d_nms_utils.boxes_iou3d_gpu(box_preds[:, 0:7], gt[:, 0:7]) if box_preds.shape[0] > 0 else None
            iou_roi = iou3d_nms_utils.boxes_iou3d_gpu(rois[:, 0:7], gt[:, 0:7]) if rois is not None else None
            for t in thresh_list:
                if iou_rcnn is not None:
                    recall_dict['rcnn_%s' % str(t)] += int((iou_rcnn.max(dim=0)[0] > t).sum().item())
                if iou_roi is not None:
                    recall_dict['roi_%s' % str(t)] += int((iou_roi.max(dim=0)[0] > t).sum().item())
            recall_dict['gt'] += gt.shape[0]
        return recall_dict

    def adapt_spconv_weights(self, model_state):
        return adapt_spconv_weights(self, model_state)

    def load_params_from_file(self, filename, to_cpu=False, logger=None):
        """checkpoint['model_state'] into this model, strict: every key and shape must be this model's (a sparse
        convolution's weight may come in the 1.x layout: adapt_spconv_weights)."""
        if not os.path.isfile(filename):
            raise FileNotFoundError(filename)
        checkpoint = torch.load(filename, map_location=torch.device('cpu') if to_cpu else None)
        self.load_state_dict(adapt_spconv_weights(self, checkpoint['model_state']), strict=True)
        if logger is not None:
            logger.info('==> Loaded %d tensors from %s' % (len(checkpoint['model_state']), filename))
        return checkpoint
