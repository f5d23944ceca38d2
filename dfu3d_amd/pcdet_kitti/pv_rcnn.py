"""pcdet/models/detectors/pv_rcnn.py (over detector3d_template.py): the voxel assembly of
`CenterPoint(..., sparse_3d=True)` with AnchorHeadSingle as the dense head -- SECONDNet's -- and, around it, `pfe`
(VoxelSetAbstraction), `point_head` (PointHeadSimple) and `roi_head` (PVRCNNHead), in the template's order:
vfe -> backbone_3d -> map_to_bev_module -> pfe -> backbone_2d -> dense_head -> point_head -> roi_head.  The submodule
names and `global_step` are the reference's, so a reference checkpoint's 'model_state' loads with strict=True after
adapt_spconv_weights.

Inference only: `forward(batch_dict)` in eval mode returns (pred_dicts, recall_dict) through PointRCNN's batched
post_processing (the RoI head's `roi_labels` are the class labels); in training mode it raises NotImplementedError."""
from .anchor_head_single import AnchorHeadSingle
from .centerpoint import CenterPoint, _get, _module_class
from .point_head_simple import PointHeadSimple
from .point_rcnn import PointRCNN
from .pvrcnn_head import PVRCNNHead
from .voxel_set_abstraction import VoxelSetAbstraction


class PVRCNN(CenterPoint):
    MORE_MODULES = {'DENSE_HEAD': {'AnchorHeadSingle': AnchorHeadSingle}, 'PFE': {'VoxelSetAbstraction': VoxelSetAbstraction},
                    'POINT_HEAD': {'PointHeadSimple': PointHeadSimple}, 'ROI_HEAD': {'PVRCNNHead': PVRCNNHead}}

    def __init__(self, model_cfg, num_class, dataset=None, **kwargs):
        kwargs.pop('sparse_3d', None)
        super().__init__(model_cfg, num_class, dataset=dataset, sparse_3d=True, **kwargs)
        dataset, who = self.dataset, type(self).__name__
        cfg, cls = _module_class(model_cfg, 'PFE', more=self.MORE_MODULES, who=who)
        if cls is None:
            raise NotImplementedError("PVRCNN: the config has no PFE")
        self.pfe = cls(model_cfg=cfg, voxel_size=[float(v) for v in dataset.voxel_size],
                       point_cloud_range=[float(v) for v in dataset.point_cloud_range],
                       num_bev_features=self.map_to_bev_module.num_bev_features,
                       num_rawpoint_features=dataset.point_feature_encoder.num_point_features)
        cfg, cls = _module_class(model_cfg, 'POINT_HEAD', more=self.MORE_MODULES, who=who)
        before = _get(cfg, 'USE_POINT_FEATURES_BEFORE_FUSION', False)
        self.point_head = cls(model_cfg=cfg, num_class=num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1,
                              input_channels=self.pfe.num_point_features_before_fusion if before
                              else self.pfe.num_point_features)
        cfg, cls = _module_class(model_cfg, 'ROI_HEAD', more=self.MORE_MODULES, who=who)
        self.roi_head = cls(model_cfg=cfg, input_channels=self.pfe.num_point_features,
                            num_class=num_class if not _get(cfg, 'CLASS_AGNOSTIC', False) else 1)
        at = self.module_list.index(self.backbone_2d) if self.backbone_2d is not None else len(self.module_list)
        self.module_list = self.module_list[:at] + [self.pfe] + self.module_list[at:] + [self.point_head, self.roi_head]

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("PVRCNN.forward in training mode: target assignment and the losses of the point "
                                      "head and the RoI head are not part of this package")
        for cur_module in self.module_list:
            batch_dict = cur_module(batch_dict)
        return self.post_processing(batch_dict)

    select_predictions = PointRCNN.select_predictions
    post_processing = PointRCNN.post_processing
