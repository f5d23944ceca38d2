"""The surface of the sparse-convolution library that pcdet's voxel backbones use (pcdet/utils/spconv_utils.py and the
`spconv` names behind it), on dfu3d_amd.sparse_conv_ops: SparseConvTensor, SubMConv3d, SparseConv3d, SparseSequential,
replace_feature, find_all_spconv_keys.  Weights are parameters of shape (Cout, kz, ky, kx, Cin), the 2.x layout, under
the same state-dict keys.

The tables a layer needs come from an index plan (sparse_conv_ops.build_plan: one read from the device).  A backbone
makes ONE plan for all its layers before the first of them runs (plan_for) and the tensors carry it along; a layer that
meets a tensor without a plan, or with one that lacks its geometry, makes a plan of its own for that one layer.  A
status bit of the plan raises Dfu3dError.

Divergences from that library: the row order of a strided layer's output is the header's (first seen over input row,
then offset), the summation order is the header's, and SparseInverseConv3d is not here."""
import math

import torch
import torch.nn as nn

from .. import bev_ops, sparse_conv_ops
from .._lib import Dfu3dError


class IndexPlan:
    """A sparse_conv_ops.Plan and, per (in_level, kernel, stride, padding, subm), its tables."""

    def __init__(self, plan, specs):
        self.plan = plan
        self.levels = plan.levels
        self.lookup = {tuple(sp): t for sp, t in zip(specs, plan.tables)}


def plan_for(indices, batch_size, spatial_shape, specs, count=None):
    """specs: sparse_conv_ops.LayerSpec list -> IndexPlan; raises on a status bit."""
    plan = sparse_conv_ops.build_plan(indices, count, batch_size, spatial_shape, specs)
    if plan.status:
        raise Dfu3dError("sparse convolution: index plan status %d (%s)"
                         % (plan.status, sparse_conv_ops.status_message(plan.status)))
    return IndexPlan(plan, specs)


class SparseConvTensor:
    def __init__(self, features, indices, spatial_shape, batch_size, plan=None, level=0):
        """features (N, C) float32, indices (N, 4) int32 [b, z, y, x], spatial_shape (D, H, W)."""
        self.features = features
        self.indices = indices
        self.spatial_shape = [int(v) for v in spatial_shape]
        self.batch_size = int(batch_size)
        self.plan = plan
        self.level = level

    def replace_feature(self, feature):
        return SparseConvTensor(feature, self.indices, self.spatial_shape, self.batch_size, self.plan, self.level)

    @property
    def spatial_size(self):
        return self.spatial_shape[0] * self.spatial_shape[1] * self.spatial_shape[2]

    def dense(self, channels_first=True):
        """(B, C, D, H, W): bev_ops.pillar_scatter with grid (W, H, D) writes canvas channel c * D + z."""
        D, H, W = self.spatial_shape
        feats = self.features.contiguous()
        canvas = bev_ops.pillar_scatter(feats, self.indices.contiguous(), self.batch_size, (W, H, D))
        out = canvas.view(self.batch_size, feats.shape[1], D, H, W)
        return out if channels_first else out.permute(0, 2, 3, 4, 1).contiguous()


def replace_feature(out, new_features):
    return out.replace_feature(new_features)


class SparseModule(nn.Module):
    pass


class SparseConvolution(SparseModule):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, subm=False,
                 indice_key=None):
        super().__init__()
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.subm, self.indice_key = bool(subm), indice_key
        spec = sparse_conv_ops.layer(0, kernel_size, stride, padding, subm)
        self.kernel_size, self.stride, self.padding = spec.kernel, spec.stride, spec.padding
        self.weight = nn.Parameter(torch.empty((self.out_channels,) + self.kernel_size + (self.in_channels,)))
        self.bias = nn.Parameter(torch.empty(self.out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1] * self.kernel_size[2])
            nn.init.uniform_(self.bias, -bound, bound)

    def spec(self, in_level):
        return sparse_conv_ops.LayerSpec(in_level, self.kernel_size, self.stride, self.padding, self.subm)

    def forward(self, x):
        plan, spec = x.plan, self.spec(x.level)
        if plan is None or tuple(spec) not in plan.lookup:
            spec = self.spec(0)
            plan = plan_for(x.indices.contiguous(), x.batch_size, x.spatial_shape, [spec])
        t = plan.lookup[tuple(spec)]
        feats = sparse_conv_ops.sparse_conv(x.features, self.weight, t)
        if self.bias is not None:
            feats = feats + self.bias
        lv = plan.levels[t.out_level]
        return SparseConvTensor(feats, lv.indices, lv.spatial_shape, x.batch_size, plan, t.out_level)


class SubMConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, 1, 0, bias, True, indice_key)


class SparseConv3d(SparseConvolution):
    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True, indice_key=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, bias, False, indice_key)


class SparseInverseConv3d(SparseModule):
    def __init__(self, *args, **kwargs):
        raise NotImplementedError("SparseInverseConv3d is not part of this package")


class SparseSequential(SparseModule):
    def __init__(self, *modules):
        super().__init__()
        for i, m in enumerate(modules):
            self.add_module(str(i), m)

    def __len__(self):
        return len(self._modules)

    def __getitem__(self, i):
        return list(self._modules.values())[i]

    def forward(self, x):
        for m in self._modules.values():
            if isinstance(m, SparseModule):
                x = m(x)
            elif isinstance(x, SparseConvTensor):
                if x.features.shape[0] != 0:
                    x = x.replace_feature(m(x.features))
            else:
                x = m(x)
        return x


def chain_specs(module):
    """The LayerSpecs of every convolution under `module`, in registration order, for a network that is one chain of
    levels (a submanifold layer stays on its level, a strided one moves to a new one, or to the one an equal layer
    made): what a voxel backbone gives plan_for."""
    specs, made, level, n_levels = [], {}, 0, 1
    for m in module.modules():
        if not isinstance(m, SparseConvolution):
            continue
        sp = m.spec(level)
        specs.append(sp)
        if not m.subm:
            key = tuple(sp)
            if key not in made:
                made[key] = n_levels
                n_levels += 1
            level = made[key]
    return specs


def find_all_spconv_keys(model, prefix=""):
    """The state-dict keys of every sparse convolution's weight under `model` (what a 1.x checkpoint holds in another
    layout), each with `prefix` and a dot in front if a prefix is given."""
    lead = prefix + "." if prefix else ""
    return {lead + name + ".weight" for name, m in model.named_modules() if name and isinstance(m, SparseConvolution)}
