"""The two box coders of the PointRCNN configuration under the names of pcdet/utils/box_coder_utils.py:
`PointResidualCoder` (PointHeadBox: a box against the point that predicts it and the mean size of its class) and
`ResidualCoder` (PointRCNNHead: a box against its RoI).  Plain torch on whatever device the inputs are on.

Both are one residual rule over columns [x, y, z, dx, dy, dz, angle..., extras...], stated once below (`_to_residual`,
`_from_residual`): with an anchor centre c, anchor dims s and `diag = sqrt(sx^2 + sy^2)`
    encode:  ((x - cx) / diag, (y - cy) / diag, (z - cz) / sz, log(d / s))
    decode:  (tx * diag + cx, ty * diag + cy, tz * sz + cz, exp(td) * s)
Every float operation is the reference's, in its order; only the statements are this package's.  The mean sizes are a
host tensor until the first call that needs them and follow the input's device from then on (the reference moves them to
the GPU in __init__, which a model built on the CPU cannot do).  As in the reference, encode_torch clamps the dims of
its inputs to 1e-5 IN PLACE."""
import torch

MIN_DIM = 1e-5


def _clamp_dims_(boxes):
    boxes[:, 3:6] = boxes[:, 3:6].clamp_min(MIN_DIM)


def _diag(size):
    return (size[..., 0:1] ** 2 + size[..., 1:2] ** 2).sqrt()


def _to_residual(boxes, centre, size):
    """boxes (..., 6+), anchor centre (..., 3) and dims (..., 3) -> the six residual columns."""
    plane = (boxes[..., 0:2] - centre[..., 0:2]) / _diag(size)
    height = (boxes[..., 2:3] - centre[..., 2:3]) / size[..., 2:3]
    return torch.cat((plane, height, (boxes[..., 3:6] / size).log()), dim=-1)


def _from_residual(code, centre, size):
    """The six residual columns back to centre and dims."""
    plane = code[..., 0:2] * _diag(size) + centre[..., 0:2]
    height = code[..., 2:3] * size[..., 2:3] + centre[..., 2:3]
    return torch.cat((plane, height, code[..., 3:6].exp() * size), dim=-1)


class ResidualCoder(object):
    """A box against an anchor box.  The angle is the difference of the headings, or with encode_angle_by_sincos the
    differences of their cosines and sines (code_size 8); columns beyond the heading are differences."""

    def __init__(self, code_size=7, encode_angle_by_sincos=False, **kwargs):
        self.encode_angle_by_sincos = encode_angle_by_sincos
        self.code_size = code_size + (1 if encode_angle_by_sincos else 0)

    def encode_torch(self, boxes, anchors):
        """boxes, anchors (N, 7 + C) -> (N, code_size + C)."""
        _clamp_dims_(anchors)
        _clamp_dims_(boxes)
        heading, anchor_heading = boxes[..., 6:7], anchors[..., 6:7]
        if self.encode_angle_by_sincos:
            angle = (heading.cos() - anchor_heading.cos(), heading.sin() - anchor_heading.sin())
        else:
            angle = (heading - anchor_heading,)
        return torch.cat((_to_residual(boxes, anchors[..., 0:3], anchors[..., 3:6]), *angle,
                          boxes[..., 7:] - anchors[..., 7:]), dim=-1)

    def decode_torch(self, box_encodings, anchors):
        """box_encodings (..., code_size + C), anchors (..., 7 + C) -> (..., 7 + C)."""
        anchor_heading = anchors[..., 6:7]
        if self.encode_angle_by_sincos:
            heading = torch.atan2(box_encodings[..., 7:8] + anchor_heading.sin(),
                                  box_encodings[..., 6:7] + anchor_heading.cos())
            extras = box_encodings[..., 8:]
        else:
            heading = box_encodings[..., 6:7] + anchor_heading
            extras = box_encodings[..., 7:]
        return torch.cat((_from_residual(box_encodings, anchors[..., 0:3], anchors[..., 3:6]), heading,
                          extras + anchors[..., 7:]), dim=-1)


class PointResidualCoder(object):
    """A box against a point: the anchor's centre is the point, its dims the mean size of the box's class (classes count
    from 1), or with use_mean_size=False no dims at all (plain offsets and log dims).  The heading is coded as
    (cos, sin): code_size 8; columns beyond the heading pass through."""

    def __init__(self, code_size=8, use_mean_size=True, **kwargs):
        self.code_size = code_size
        self.use_mean_size = use_mean_size
        if use_mean_size:
            self.mean_size = torch.tensor(kwargs['mean_size'], dtype=torch.float64).float()
            assert self.mean_size.min() > 0

    def _anchor_size(self, classes, like):
        if self.mean_size.device != like.device:
            self.mean_size = self.mean_size.to(like.device)
        return self.mean_size[classes - 1]

    def encode_torch(self, gt_boxes, points, gt_classes=None):
        """gt_boxes (N, 7 + C), points (N, 3), gt_classes (N) in [1, num_classes] -> (N, 8 + C)."""
        _clamp_dims_(gt_boxes)
        if self.use_mean_size:
            code = _to_residual(gt_boxes, points, self._anchor_size(gt_classes, gt_boxes))
        else:
            code = torch.cat((gt_boxes[..., 0:3] - points, gt_boxes[..., 3:6].log()), dim=-1)
        heading = gt_boxes[..., 6:7]
        return torch.cat((code, heading.cos(), heading.sin(), gt_boxes[..., 7:]), dim=-1)

    def decode_torch(self, box_encodings, points, pred_classes=None):
        """box_encodings (N, 8 + C), points (N, 3), pred_classes (N) in [1, num_classes] -> (N, 7 + C).  The reference
        asserts the largest class against the number of mean sizes on the host; here a class out of range is the
        indexing's own error on the device."""
        if self.use_mean_size:
            box = _from_residual(box_encodings, points, self._anchor_size(pred_classes, box_encodings))
        else:
            box = torch.cat((box_encodings[..., 0:3] + points, box_encodings[..., 3:6].exp()), dim=-1)
        heading = torch.atan2(box_encodings[..., 7:8], box_encodings[..., 6:7])
        return torch.cat((box, heading, box_encodings[..., 8:]), dim=-1)
