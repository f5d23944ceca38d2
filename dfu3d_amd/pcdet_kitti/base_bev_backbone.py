"""The 2-D backbone of pcdet/models/backbones_2d/base_bev_backbone.py (BaseBEVBackbone), torch only: the reference's
constructor arguments, forward keys ('spatial_features' -> 'spatial_features_2d', 'spatial_features_%dx') and
state-dict keys (blocks.i.j.*, deblocks.i.j.*), so a reference checkpoint loads as it is.  Every BatchNorm has
eps = 1e-3 and momentum = 0.01.  An UPSAMPLE_STRIDES entry below 1 is a strided convolution of stride round(1 / s);
one entry more than there are levels adds a transposed convolution over the concatenated maps."""
import torch
import torch.nn as nn


def _get(cfg, key, *default):
    if isinstance(cfg, dict):
        return cfg[key] if not default else cfg.get(key, default[0])
    return getattr(cfg, key) if not default else getattr(cfg, key, default[0])


def _norm_relu(channels):
    return [nn.BatchNorm2d(channels, eps=1e-3, momentum=0.01), nn.ReLU()]


def _block(c_in, c_out, stride, n_layers):
    layers = [nn.ZeroPad2d(1), nn.Conv2d(c_in, c_out, kernel_size=3, stride=stride, padding=0, bias=False)]
    layers += _norm_relu(c_out)
    for _ in range(n_layers):
        layers += [nn.Conv2d(c_out, c_out, kernel_size=3, padding=1, bias=False)] + _norm_relu(c_out)
    return nn.Sequential(*layers)


def _deblock(c_in, c_out, stride, conv_for_no_stride):
    if stride > 1 or (stride == 1 and not conv_for_no_stride):
        up = nn.ConvTranspose2d(c_in, c_out, stride, stride=stride, bias=False)
    else:
        down = int(round(1 / stride))
        up = nn.Conv2d(c_in, c_out, down, stride=down, bias=False)
    return nn.Sequential(up, *_norm_relu(c_out))


class BaseBEVBackbone(nn.Module):
    def __init__(self, model_cfg, input_channels):
        super().__init__()
        self.model_cfg = model_cfg
        layer_nums = list(_get(model_cfg, 'LAYER_NUMS', None) or [])
        layer_strides = list(_get(model_cfg, 'LAYER_STRIDES', None) or []) if layer_nums else []
        num_filters = list(_get(model_cfg, 'NUM_FILTERS', None) or []) if layer_nums else []
        assert len(layer_nums) == len(layer_strides) == len(num_filters)
        upsample_strides = list(_get(model_cfg, 'UPSAMPLE_STRIDES', None) or [])
        num_upsample_filters = list(_get(model_cfg, 'NUM_UPSAMPLE_FILTERS', None) or []) if upsample_strides else []
        assert len(upsample_strides) == len(num_upsample_filters)
        conv_for_no_stride = _get(model_cfg, 'USE_CONV_FOR_NO_STRIDE', False)
        c_in_list = [input_channels] + num_filters[:-1]
        self.blocks = nn.ModuleList()
        self.deblocks = nn.ModuleList()
        for idx in range(len(layer_nums)):
            self.blocks.append(_block(c_in_list[idx], num_filters[idx], layer_strides[idx], layer_nums[idx]))
            if upsample_strides:
                self.deblocks.append(_deblock(num_filters[idx], num_upsample_filters[idx], upsample_strides[idx],
                                              conv_for_no_stride))
        c_in = sum(num_upsample_filters)
        if len(upsample_strides) > len(layer_nums):
            last = upsample_strides[-1]
            self.deblocks.append(nn.Sequential(nn.ConvTranspose2d(c_in, c_in, last, stride=last, bias=False),
                                               *_norm_relu(c_in)))
        self.num_bev_features = c_in

    def forward(self, data_dict):
        spatial_features = data_dict['spatial_features']
        ups = []
        x = spatial_features
        for i, block in enumerate(self.blocks):
            x = block(x)
            data_dict_key = 'spatial_features_%dx' % int(spatial_features.shape[2] / x.shape[2])
            data_dict[data_dict_key] = x
            ups.append(self.deblocks[i](x) if len(self.deblocks) > 0 else x)
        if len(ups) > 1:
            x = torch.cat(ups, dim=1)
        elif len(ups) == 1:
            x = ups[0]
        if len(self.deblocks) > len(self.blocks):
            x = self.deblocks[-1](x)
        data_dict['spatial_features_2d'] = x
        return data_dict
