"""pcdet/models/backbones_2d/map_to_bev/height_compression.py: the encoded sparse tensor as a bird's-eye-view map
(B, C * D, H, W), channel c at depth z being map channel c * D + z.  The dense form comes from the PointPillarScatter
stage (SparseConvTensor.dense), forward and backward."""
import torch.nn as nn


def _get(cfg, key):
    return cfg[key] if isinstance(cfg, dict) else getattr(cfg, key)


class HeightCompression(nn.Module):
    def __init__(self, model_cfg, **kwargs):
        super().__init__()
        self.model_cfg = model_cfg
        self.num_bev_features = _get(self.model_cfg, 'NUM_BEV_FEATURES')

    def forward(self, batch_dict):
        """encoded_spconv_tensor -> spatial_features (B, C * D, H, W), spatial_features_stride."""
        volume = batch_dict['encoded_spconv_tensor'].dense()          # (B, C, D, H, W), canvas channel c * D + z underneath
        batch_dict.update(spatial_features=volume.flatten(1, 2),
                          spatial_features_stride=batch_dict['encoded_spconv_tensor_stride'])
        return batch_dict
