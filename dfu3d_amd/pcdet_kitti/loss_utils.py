"""The two CenterNet losses of pcdet/utils/loss_utils.py as modules on dfu3d_amd.center_loss_ops
(csrc/centerloss_stage.hip): `FocalLossCenterNet` and `RegLossCenterNet` with the reference's `forward` signatures and
return shapes, each one head of the kernels `CenterHead.get_loss` runs for all heads at once.

Divergence from the reference: `FocalLossCenterNet.forward` takes the heat map's LOGITS; the kernel applies the head's
clamp(sigmoid(x), 1e-4, 1 - 1e-4) itself (the reference's head does that before it calls the module).  Sums are fp64
with a fixed shape, so two runs give the same bits."""
import torch.nn as nn

from .. import center_loss_ops


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
