"""pcdet/models/dense_heads/target_assigner/anchor_generator.py under its names: per anchor class the block
(nz, ny, nx, #sizes, #rotations, 7) of anchors [x, y, z, dx, dy, dz, heading] over the feature map, z moved from the
bottom height to the box centre.

Divergence from the reference: nothing here calls .cuda().  The grid is always computed on the CPU -- torch.arange in
float32 there, so the anchors have the same bits whatever device the model lives on -- and then moved to `device`."""
import torch

from .common_utils import cfg_get


class AnchorGenerator(object):
    def __init__(self, anchor_range, anchor_generator_config, device=None):
        super().__init__()
        self.anchor_generator_cfg = anchor_generator_config
        self.anchor_range = anchor_range
        self.device = device
        self.anchor_sizes = [cfg_get(c, 'anchor_sizes') for c in anchor_generator_config]
        self.anchor_rotations = [cfg_get(c, 'anchor_rotations') for c in anchor_generator_config]
        self.anchor_heights = [cfg_get(c, 'anchor_bottom_heights') for c in anchor_generator_config]
        self.align_center = [cfg_get(c, 'align_center', False) for c in anchor_generator_config]
        assert len(self.anchor_sizes) == len(self.anchor_rotations) == len(self.anchor_heights)
        self.num_of_anchor_sets = len(self.anchor_sizes)

    def generate_anchors(self, grid_sizes):
        """grid_sizes: (nx, ny) per anchor class -> ([anchors per class], [anchors per location per class])."""
        assert len(grid_sizes) == self.num_of_anchor_sets
        r = self.anchor_range
        all_anchors, num_anchors_per_location = [], []
        for grid_size, sizes, rotations, heights, align_center in zip(
                grid_sizes, self.anchor_sizes, self.anchor_rotations, self.anchor_heights, self.align_center):
            num_anchors_per_location.append(len(rotations) * len(sizes) * len(heights))
            if align_center:
                x_stride, y_stride = (r[3] - r[0]) / grid_size[0], (r[4] - r[1]) / grid_size[1]
                x_offset, y_offset = x_stride / 2, y_stride / 2
            else:
                x_stride, y_stride = (r[3] - r[0]) / (grid_size[0] - 1), (r[4] - r[1]) / (grid_size[1] - 1)
                x_offset, y_offset = 0, 0
            x_shifts = torch.arange(r[0] + x_offset, r[3] + 1e-5, step=x_stride, dtype=torch.float32)
            y_shifts = torch.arange(r[1] + y_offset, r[4] + 1e-5, step=y_stride, dtype=torch.float32)
            z_shifts = x_shifts.new_tensor(heights)
            n_size, n_rot = len(sizes), len(rotations)
            rot = x_shifts.new_tensor(rotations)
            size = x_shifts.new_tensor(sizes)
            gx, gy, gz = torch.meshgrid([x_shifts, y_shifts, z_shifts], indexing='ij')
            anchors = torch.stack((gx, gy, gz), dim=-1)                                   # (nx, ny, nz, 3)
            anchors = anchors[:, :, :, None, :].repeat(1, 1, 1, n_size, 1)
            size = size.view(1, 1, 1, -1, 3).repeat([*anchors.shape[0:3], 1, 1])
            anchors = torch.cat((anchors, size), dim=-1)
            anchors = anchors[:, :, :, :, None, :].repeat(1, 1, 1, 1, n_rot, 1)
            rot = rot.view(1, 1, 1, 1, -1, 1).repeat([*anchors.shape[0:3], n_size, 1, 1])
            anchors = torch.cat((anchors, rot), dim=-1)                                   # (nx, ny, nz, #size, #rot, 7)
            anchors = anchors.permute(2, 1, 0, 3, 4, 5).contiguous()
            anchors[..., 2] += anchors[..., 5] / 2                                        # bottom height -> box centre
            all_anchors.append(anchors if self.device is None else anchors.to(self.device))
        return all_anchors, num_anchors_per_location
