"""pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py under its names, on ONE call of the anchor
target stage (dfu3d_amd.anchor_target_ops -> csrc/anchor_stage.hip) for the whole batch: no loop over samples or classes,
no dense IoU matrix, no read from the device.

The stage states the reference's rule for the settings its shipped single-head configurations use.  Every other setting
raises NotImplementedError naming it: POS_FRACTION >= 0 (random sampling), NORM_BY_NUM_EXAMPLES, MATCH_HEIGHT,
USE_MULTIHEAD, a box coder other than the 7-column ResidualCoder, an ANCHOR_GENERATOR_CONFIG whose last class is not the
last of the class names (the reference files a box of class 0 under class_names[-1])."""
import torch

from .. import anchor_target_ops
from .box_coder_utils import ResidualCoder
from .common_utils import cfg_get


class AxisAlignedTargetAssigner(object):
    def __init__(self, model_cfg, class_names, box_coder, match_height=False):
        super().__init__()
        generator_cfg = cfg_get(model_cfg, 'ANCHOR_GENERATOR_CONFIG')
        target_cfg = cfg_get(model_cfg, 'TARGET_ASSIGNER_CONFIG')
        self.box_coder = box_coder
        self.match_height = match_height
        self.class_names = list(class_names)
        self.anchor_class_names = [cfg_get(c, 'class_name') for c in generator_cfg]
        pos_fraction = cfg_get(target_cfg, 'POS_FRACTION')
        self.pos_fraction = pos_fraction if pos_fraction >= 0 else None
        self.sample_size = cfg_get(target_cfg, 'SAMPLE_SIZE', None)
        self.norm_by_num_examples = cfg_get(target_cfg, 'NORM_BY_NUM_EXAMPLES')
        self.matched_thresholds = {cfg_get(c, 'class_name'): cfg_get(c, 'matched_threshold') for c in generator_cfg}
        self.unmatched_thresholds = {cfg_get(c, 'class_name'): cfg_get(c, 'unmatched_threshold') for c in generator_cfg}
        self.use_multihead = cfg_get(model_cfg, 'USE_MULTIHEAD', False)
        if self.pos_fraction is not None:
            raise NotImplementedError("AxisAlignedTargetAssigner: POS_FRACTION = %r >= 0 (random sampling of the anchors) "
                                      "is not part of this package" % (pos_fraction,))
        if self.norm_by_num_examples:
            raise NotImplementedError("AxisAlignedTargetAssigner: NORM_BY_NUM_EXAMPLES: True is not part of this package")
        if match_height:
            raise NotImplementedError("AxisAlignedTargetAssigner: MATCH_HEIGHT: True (the rotated 3-D IoU) is not part "
                                      "of this package")
        if self.use_multihead:
            raise NotImplementedError("AxisAlignedTargetAssigner: USE_MULTIHEAD: True is not part of this package")
        if not isinstance(box_coder, ResidualCoder) or box_coder.code_size != 7:
            raise NotImplementedError("AxisAlignedTargetAssigner: BOX_CODER must be the 7-column ResidualCoder, got %s "
                                      "with code_size %s" % (type(box_coder).__name__, getattr(box_coder, 'code_size', None)))
        unknown = [n for n in self.anchor_class_names if n not in self.class_names]
        if unknown or len(set(self.anchor_class_names)) != len(self.anchor_class_names):
            raise NotImplementedError("AxisAlignedTargetAssigner: ANCHOR_GENERATOR_CONFIG names %s; each must be one of "
                                      "the class names %s, once" % (self.anchor_class_names, self.class_names))
        if self.anchor_class_names[-1] != self.class_names[-1]:
            raise NotImplementedError("AxisAlignedTargetAssigner: the last entry of ANCHOR_GENERATOR_CONFIG (%r) must be "
                                      "the last class name (%r)" % (self.anchor_class_names[-1], self.class_names[-1]))
        self._flat = None

    def class_sets(self, all_anchors):
        """(anchors per location, matched, unmatched, 1-based class id) per entry of all_anchors."""
        return [(int(a.shape[3]) * int(a.shape[4]), self.matched_thresholds[n], self.unmatched_thresholds[n],
                 self.class_names.index(n) + 1) for n, a in zip(self.anchor_class_names, all_anchors)]

    def flat_anchors(self, all_anchors):
        """torch.cat(all_anchors, dim=-3) as (A, 7): y, x, then the classes one after another.  Kept for the next call
        with the same tensors, unchanged: the source tensors are held here (an address alone comes back from the
        allocator under other values) and compared by identity and by their version counter, which every in-place
        write moves."""
        src = list(all_anchors)
        versions = [a._version for a in src]
        kept = self._flat
        if (kept is None or len(kept[0]) != len(src) or any(a is not b for a, b in zip(kept[0], src))
                or kept[1] != versions):
            self._flat = (src, versions, torch.cat(src, dim=-3).view(-1, 7).contiguous())
        return self._flat[2]

    def assign_targets(self, all_anchors, gt_boxes_with_classes):
        """all_anchors: [(nz, ny, nx, #size, #rot, 7), ...] per anchor class; gt_boxes_with_classes (B, M, 8) ->
        {'box_cls_labels' int32 (B, A), 'box_reg_targets' (B, A, 7), 'reg_weights' (B, A)}."""
        assert len(all_anchors) == len(self.anchor_class_names)
        gt = gt_boxes_with_classes
        if gt.dtype != torch.float32 or not gt.is_contiguous():
            gt = gt.float().contiguous()
        labels, targets, weights = anchor_target_ops.assign_targets(self.flat_anchors(all_anchors),
                                                                    self.class_sets(all_anchors), gt)
        return {'box_cls_labels': labels, 'box_reg_targets': targets, 'reg_weights': weights}
