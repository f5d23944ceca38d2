"""The two CenterNet losses of pcdet/utils/loss_utils.py as modules on dfu3d_amd.center_loss_ops
(csrc/centerloss_stage.hip): `FocalLossCenterNet` and `RegLossCenterNet` with the reference's `forward` signatures and
return shapes, each one head of the kernels `CenterHead.get_loss` runs for all heads at once.

Divergence from the reference: `FocalLossCenterNet.forward` takes the heat map's LOGITS; the kernel applies the head's
clamp(sigmoid(x), 1e-4, 1 - 1e-4) itself (the reference's head does that before it calls the module).  Sums are fp64
with a fixed shape, so two runs give the same bits.

The losses of PointRCNN's two heads and of the anchor head -- `SigmoidFocalClassificationLoss`, `WeightedSmoothL1Loss`,
`WeightedCrossEntropyLoss` and `get_corner_loss_lidar` -- are plain torch with autograd, every float operation the reference's in its order; a fused
kernel for them in the manner of csrc/centerloss_stage.hip is not built."""
import math

import torch
import torch.nn as nn

from .. import center_loss_ops
from . import box_utils


class FocalLossCenterNet(nn.Module):
    def forward(self, out, target, mask=None):
        """out: (B, C, H, W) float32 logits, target the same shape -> the focal loss, 0-dim."""
        if mask is not None:
            raise NotImplementedError("FocalLossCenterNet: mask= is not supported (CenterHead.get_loss never passes it)")
        losses, _ = center_loss_ops.center_loss([out], [target], None, None, None, None)
        return losses[0]


class RegLossCenterNet(nn.Module):
    def forward(self, output, mask, ind=None, target=None):
        """output: (B, dim, H, W) float32, mask / ind: (B, max_objects) int64, target: (B, max_objects, dim) -> (dim,)."""
        if ind is None:
            raise NotImplementedError("RegLossCenterNet: ind=None (predictions already gathered) is not supported")
        _, chan = center_loss_ops.center_loss(None, None, [[output]], [target], [ind], [mask])
        return chan[0]


def _smooth_l1(diff, beta):
    """|x| below 1e-5 of beta, else 0.5 x^2 / beta under beta and |x| - 0.5 beta from it on."""
    size = diff.abs()
    return size if beta < 1e-5 else torch.where(size < beta, 0.5 * size ** 2 / beta, size - 0.5 * beta)


class SigmoidFocalClassificationLoss(nn.Module):
    """Sigmoid focal cross entropy per (anchor, class): alpha_t (1 - p_t)^gamma times the cross entropy of the logit."""

    def __init__(self, gamma=2.0, alpha=0.25):
        super().__init__()
        self.alpha, self.gamma = alpha, gamma

    @staticmethod
    def sigmoid_cross_entropy_with_logits(input, target):
        """max(x, 0) - x z + log(1 + exp(-|x|))."""
        return input.clamp(min=0) - input * target + torch.log1p(torch.exp(-input.abs()))

    def forward(self, input, target, weights):
        """input, target (..., #anchors, #classes), weights (..., #anchors) -> the weighted loss, the shape of input."""
        prob = torch.sigmoid(input)
        alpha_t = target * self.alpha + (1 - target) * (1 - self.alpha)
        miss = target * (1.0 - prob) + (1.0 - target) * prob
        loss = alpha_t * torch.pow(miss, self.gamma) * self.sigmoid_cross_entropy_with_logits(input, target)
        if weights.dim() == 2 or (weights.dim() == 1 and target.dim() == 2):
            weights = weights.unsqueeze(-1)
        assert weights.dim() == loss.dim()
        return loss * weights


class WeightedSmoothL1Loss(nn.Module):
    """Smooth L1 of (input - target) * code_weights per code, a NaN target replaced by the prediction (no loss, no
    gradient).  The code weights are a host tensor until the first call and follow the input's device from then on (the
    reference moves them to the GPU in __init__); they are no buffer: the state dict has no entry for them."""

    def __init__(self, beta=1.0 / 9.0, code_weights=None):
        super().__init__()
        self.beta = beta
        self.code_weights = None if code_weights is None else torch.tensor(code_weights, dtype=torch.float64).float()

    smooth_l1_loss = staticmethod(_smooth_l1)

    def forward(self, input, target, weights=None):
        """input, target (B, #anchors, #codes), weights (B, #anchors) or None -> (B, #anchors, #codes)."""
        target = torch.where(torch.isnan(target), input, target)
        diff = input - target
        if self.code_weights is not None:
            if self.code_weights.device != diff.device:
                self.code_weights = self.code_weights.to(diff.device)
            diff = diff * self.code_weights.view(1, 1, -1)
        loss = _smooth_l1(diff, self.beta)
        if weights is not None:
            assert weights.shape[0] == loss.shape[0] and weights.shape[1] == loss.shape[1]
            loss = loss * weights.unsqueeze(-1)
        return loss


def get_corner_loss_lidar(pred_bbox3d, gt_bbox3d):
    """(N, 7), (N, 7) -> (N): the mean over the eight corners of the smooth L1 (beta 1) of the corner distance, each
    corner against the nearer of the ground-truth box and the same box turned by pi."""
    assert pred_bbox3d.shape[0] == gt_bbox3d.shape[0]
    pred = box_utils.boxes_to_corners_3d(pred_bbox3d)
    turned = gt_bbox3d.clone()
    turned[:, 6] += math.pi
    dist = torch.min(torch.norm(pred - box_utils.boxes_to_corners_3d(gt_bbox3d), dim=2),
                     torch.norm(pred - box_utils.boxes_to_corners_3d(turned), dim=2))
    return _smooth_l1(dist, 1.0).mean(dim=1)


class WeightedCrossEntropyLoss(nn.Module):
    """The cross entropy of the logits against the arg max of a one-hot target, times a weight per anchor."""

    def forward(self, input, target, weights):
        """input, target (B, #anchors, #classes), weights (B, #anchors) -> (B, #anchors)."""
        return nn.functional.cross_entropy(input.permute(0, 2, 1), target.argmax(dim=-1), reduction='none') * weights
