"""The voxel backbones of pcdet/models/backbones_3d/spconv_backbone.py on this package's sparse convolution:
`VoxelBackBone8x`, `VoxelResBackBone8x`, `SparseBasicBlock`, `post_act_block`.  What has to be the reference's is its
surface -- constructor arguments, `sparse_shape`, `num_point_features`, `backbone_channels`, the submodule names that
make the state-dict keys (golden G24), the `batch_dict` outputs -- and the arithmetic of a layer; the modules themselves
are built from one table of stages.

A backbone is `conv_input` and four stages `conv1` .. `conv4` of widths STAGE_WIDTHS (the last is 128 in the residual
form), then `conv_out`.  Stage i > 1 opens with a strided 3^3 layer (stride 2, padding DOWN_PADDING[i]) on a new level;
its units stay on that level: submanifold layer + norm + ReLU in the plain form (one in `conv1`, two elsewhere), two
SparseBasicBlocks in the residual form.  BatchNorm1d(eps=1e-3, momentum=0.01) and ReLU run in torch on the feature rows,
which are at exact size: ONE index plan per forward, for all layers (spconv_utils.chain_specs), and that plan's one read
from the device is where the levels' row counts come from.  With `n_voxels` in the batch (the padded form of
prepare_batch) the rows at or beyond that device count are never read and the features are cut to the count."""
from functools import partial

import torch.nn as nn

from . import spconv_utils as spconv

STAGES = ('conv1', 'conv2', 'conv3', 'conv4')
STAGE_WIDTHS = (16, 32, 64, 64)
DOWN_PADDING = {'conv2': 1, 'conv3': 1, 'conv4': (0, 1, 1)}
STRIDES = {'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}
CONVOLUTIONS = {'subm': lambda cin, cout, k, stride, padding, key: spconv.SubMConv3d(cin, cout, k, bias=False, indice_key=key),
                'spconv': lambda cin, cout, k, stride, padding, key: spconv.SparseConv3d(cin, cout, k, stride=stride,
                                                                                        padding=padding, bias=False, indice_key=key),
                'inverseconv': lambda cin, cout, k, stride, padding, key: spconv.SparseInverseConv3d(cin, cout, k, indice_key=key,
                                                                                                    bias=False)}


def _get(cfg, key, default):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


def post_act_block(in_channels, out_channels, kernel_size, indice_key=None, stride=1, padding=0, conv_type='subm',
                   norm_fn=None):
    """A bias-free convolution of `conv_type`, its norm and a ReLU, as children '0', '1', '2'."""
    if conv_type not in CONVOLUTIONS:
        raise NotImplementedError(conv_type)
    conv = CONVOLUTIONS[conv_type](in_channels, out_channels, kernel_size, stride, padding, indice_key)
    return spconv.SparseSequential(conv, norm_fn(out_channels), nn.ReLU())


class SparseBasicBlock(spconv.SparseModule):
    """relu(bn2(conv2(relu(bn1(conv1(x))))) + x) on one level; `downsample`, if given, maps x for the sum."""
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, bias=None, norm_fn=None, downsample=None, indice_key=None):
        super().__init__()
        if norm_fn is None:
            raise AssertionError("SparseBasicBlock needs a norm_fn")
        bias = True if bias is None else bias
        for n, cin in ((1, inplanes), (2, planes)):
            setattr(self, 'conv%d' % n, spconv.SubMConv3d(cin, planes, kernel_size=3, stride=stride, padding=1, bias=bias,
                                                          indice_key=indice_key))
            setattr(self, 'bn%d' % n, norm_fn(planes))
            if n == 1:
                self.relu = nn.ReLU()
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        y = self.conv1(x)
        y = self.conv2(y.replace_feature(self.relu(self.bn1(y.features))))
        skip = x if self.downsample is None else self.downsample(x)
        return y.replace_feature(self.relu(self.bn2(y.features) + skip.features))


class _VoxelBackBone8x(nn.Module):
    def __init__(self, model_cfg, input_channels, grid_size, residual, last_width):
        super().__init__()
        self.model_cfg = model_cfg
        nx, ny, nz = (int(v) for v in grid_size)
        self.sparse_shape = [nz + 1, ny, nx]                          # (z, y, x), one more cell in depth
        norm_fn = partial(nn.BatchNorm1d, eps=1e-3, momentum=0.01)
        use_bias = _get(model_cfg, 'USE_BIAS', None)
        widths = STAGE_WIDTHS[:3] + (last_width,)

        def unit(width, stage_no):
            if residual:
                return SparseBasicBlock(width, width, bias=use_bias, norm_fn=norm_fn, indice_key='res%d' % stage_no)
            return post_act_block(width, width, 3, norm_fn=norm_fn, padding=1, indice_key='subm%d' % stage_no)
        self.conv_input = post_act_block(input_channels, widths[0], 3, norm_fn=norm_fn, padding=1, indice_key='subm1')
        before = widths[0]
        for no, (name, width) in enumerate(zip(STAGES, widths), 1):
            layers = []
            if name in DOWN_PADDING:
                layers.append(post_act_block(before, width, 3, norm_fn=norm_fn, stride=2, padding=DOWN_PADDING[name],
                                             indice_key='spconv%d' % no, conv_type='spconv'))
            layers += [unit(width, no) for _ in range(2 if residual or no > 1 else 1)]
            setattr(self, name, spconv.SparseSequential(*layers))
            before = width
        self.conv_out = post_act_block(before, 128, (3, 1, 1), norm_fn=norm_fn, stride=(2, 1, 1),
                                       padding=_get(model_cfg, 'last_pad', 0), indice_key='spconv_down2', conv_type='spconv')
        self.num_point_features = 128
        self.backbone_channels = {'x_' + name: width for name, width in zip(STAGES, widths)}
        self._specs = None

    def forward(self, batch_dict):
        """batch_dict: batch_size, voxel_features (V, C), voxel_coords (V, 4) [b, z, y, x], optionally n_voxels (a device
        int: the rows that count) -> encoded_spconv_tensor (stride 8), multi_scale_3d_features, multi_scale_3d_strides."""
        if self._specs is None:
            self._specs = spconv.chain_specs(self)
        indices = batch_dict['voxel_coords'].int().contiguous()
        plan = spconv.plan_for(indices, batch_dict['batch_size'], self.sparse_shape, self._specs,
                               count=batch_dict.get('n_voxels'))
        first = plan.levels[0]
        x = spconv.SparseConvTensor(batch_dict['voxel_features'][:first.rows], first.indices, self.sparse_shape,
                                    batch_dict['batch_size'], plan=plan)
        x = self.conv_input(x)
        scales = {}
        for name in STAGES:
            x = getattr(self, name)(x)
            scales['x_' + name] = x
        batch_dict['encoded_spconv_tensor'] = self.conv_out(x)
        batch_dict['encoded_spconv_tensor_stride'] = 8
        batch_dict['multi_scale_3d_features'] = scales
        batch_dict['multi_scale_3d_strides'] = dict(STRIDES)
        return batch_dict


class VoxelBackBone8x(_VoxelBackBone8x):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__(model_cfg, input_channels, grid_size, residual=False, last_width=64)


class VoxelResBackBone8x(_VoxelBackBone8x):
    def __init__(self, model_cfg, input_channels, grid_size, **kwargs):
        super().__init__(model_cfg, input_channels, grid_size, residual=True, last_width=128)
