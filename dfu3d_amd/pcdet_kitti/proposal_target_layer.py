"""ProposalTargetLayer of PointRCNN's second stage (pcdet/models/roi_heads/target_assigner/proposal_target_layer.py) on
dfu3d_amd.rcnn_target_ops: the best IoU of every RoI with a ground-truth box of its class in one launch for the batch,
the foreground / hard / easy subsampling in one more, the gathers and the labels in torch.  No parameters, no buffers,
nothing read from the device.

Divergences from the reference, all recorded in DESIGN.md row f-16: the random stream is torch's on the device (an
optional torch.Generator) instead of host NumPy and CPU randint -- the same distribution, a prefix of a uniform
permutation and uniform draws with replacement; a sample with neither a foreground nor a background RoI gets a row of
zeros and a bit in `status` (check_status() reads it) where the reference raises inside the step; equal best IoUs go to
the lowest ground-truth row and a NaN IoU never wins, which the reference leaves to torch.max."""
import torch
import torch.nn as nn

from .. import rcnn_target_ops


class ProposalTargetLayer(nn.Module):
    def __init__(self, roi_sampler_cfg, generator=None):
        super().__init__()
        self.roi_sampler_cfg = roi_sampler_cfg
        self.generator = generator                   # a torch.Generator on the RoIs' device, or None: the global one
        self._status = None                          # one int32 word on the device, made with the first forward

    def forward(self, batch_dict, sampled_inds=None):
        """batch_dict: rois (B, M, 7 + C), roi_scores (B, M), roi_labels (B, M), gt_boxes (B, G, 7 + C + 1) ->
        targets_dict: rois (B, R, 7 + C), gt_of_rois (B, R, 7 + C + 1), gt_iou_of_rois, roi_scores, roi_labels,
        reg_valid_mask, rcnn_cls_labels (all (B, R)), and the intermediate sampled_inds, max_overlaps, gt_assignment."""
        rois = batch_dict['rois']
        if self._status is None or self._status.device != rois.device:
            self._status = rcnn_target_ops.new_status(rois.device)
        with torch.no_grad():
            return rcnn_target_ops.proposal_targets(rois, batch_dict['roi_scores'], batch_dict['roi_labels'],
                                                    batch_dict['gt_boxes'], self.roi_sampler_cfg, generator=self.generator,
                                                    sampled_inds=sampled_inds, status=self._status)

    def check_status(self):
        """One read from the device: raises Dfu3dError if any forward since the layer was made met a sample without a
        foreground or background RoI."""
        return 0 if self._status is None else rcnn_target_ops.check_status(self._status)
