"""The pieces of pcdet/utils/common_utils.py the anchor head and PV-RCNN need, under its names: `limit_period`,
`get_voxel_centers`; and `cfg_get`, the one
way the anchor modules read a configuration that may be the reference's EasyDict, a plain dict or an object."""
import numpy as np
import torch


def cfg_get(cfg, key, *default):
    """cfg[key] / cfg.key; with a default, that when the key is absent."""
    if isinstance(cfg, dict):
        return cfg[key] if not default else cfg.get(key, default[0])
    return getattr(cfg, key) if not default else getattr(cfg, key, default[0])


def limit_period(val, offset=0.5, period=np.pi):
    """val - floor(val / period + offset) * period, in the dtype of val (a NumPy array goes through torch and back)."""
    is_numpy = isinstance(val, np.ndarray)
    if is_numpy:
        val = torch.from_numpy(val).float()
    ans = val - torch.floor(val / period + offset) * period
    return ans.numpy() if is_numpy else ans


def get_voxel_centers(voxel_coords, downsample_times, voxel_size, point_cloud_range):
    """voxel_coords (N, 3) [z, y, x] -> the centres (N, 3) [x, y, z] of voxels `downsample_times` the size:
    (coords + 0.5) * (voxel_size * downsample_times) + point_cloud_range[0:3], in float32 in that order.  voxel_size and
    point_cloud_range: sequences as in the reference (copied to the device on every call), or tensors already there (a
    caller that must not touch the host keeps them)."""
    assert voxel_coords.shape[1] == 3
    voxel_centers = voxel_coords.flip(dims=[1]).float()             # [z, y, x] -> [x, y, z], no index tensor from the host

    def on_device(v):
        return v.to(voxel_centers.device) if isinstance(v, torch.Tensor) else torch.tensor(v, device=voxel_centers.device)
    voxel_size = on_device(voxel_size).float() * downsample_times
    pc_range = on_device(point_cloud_range[0:3]).float()
    return (voxel_centers + 0.5) * voxel_size + pc_range
