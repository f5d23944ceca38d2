"""CPU: the torch modules that close the CenterPoint chain (BaseBEVBackbone, the convolutional half of CenterHead, the
assembled CenterPoint) against golden G16(b) and (c): the reference's outputs under its weights, its state-dict keys and
shapes, its initialisation rules."""
import json

import numpy as np
import pytest
import torch

from tests import centerpoint_cases as K


@pytest.fixture(scope="module")
def g16():
    g = K.golden()
    return g, json.loads(bytes(g["meta"]).decode())


def _full(**kw):
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    return CenterPoint(K.FULL_MODEL, len(K.FULL_CLASSES), **dict(K.FULL_DATASET, **kw))


def test_backbone_and_head_convolutions_reproduce_the_reference_outputs(g16):
    """The same torch calls in the same order under the same weights.  The capture ran the reference at 1 and at 16
    threads and stored the largest deviation between the two (meta['thread_deviation'], 0.0 for this golden): the
    comparison is bounded by four times that, which is equality of values when it is zero."""
    from dfu3d_amd.pcdet_kitti.base_bev_backbone import BaseBEVBackbone
    from dfu3d_amd.pcdet_kitti.center_head_module import CenterHeadModule
    g, meta = g16
    small, ds = K.SMALL_MODEL, K.SMALL_DATASET
    for model_cfg in (small, K.cfg(small)):                                         # dict and attribute access
        bb = BaseBEVBackbone(model_cfg['BACKBONE_2D'], input_channels=K.SMALL_INPUT[1])
        head = CenterHeadModule(model_cfg['DENSE_HEAD'], bb.num_bev_features, len(ds['class_names']), ds['class_names'],
                                ds['grid_size'], ds['point_cloud_range'], ds['voxel_size'], predict_boxes_when_training=False)
        for pre, mod in (('bb', bb), ('head', head)):
            assert list(mod.state_dict()) == meta['small_%s_keys' % pre]
            mod.load_state_dict({k: torch.from_numpy(g['small_%s_sd_%s' % (pre, k)]) for k in meta['small_%s_keys' % pre]},
                                strict=True)
            mod.eval()
        with torch.no_grad():
            d = bb({'spatial_features': torch.from_numpy(g['small_input'])})
            y = head.shared_conv(d['spatial_features_2d'])
            preds = [h(y) for h in head.heads_list]
        got = {'spatial_features_2d': d['spatial_features_2d']}
        for i, p in enumerate(preds):
            assert list(p) == ['center', 'center_z', 'dim', 'rot', 'hm']
            got.update({'head%d_%s' % (i, k): v for k, v in p.items()})
        assert sorted('small_out_' + k for k in got) == sorted(k for k in g if k.startswith('small_out_'))
        bound = 4 * meta['thread_deviation']
        for k, v in got.items():
            want = g['small_out_' + k]
            dev = float(np.abs(v.numpy().astype(np.float64) - want).max())
            print(k, tuple(want.shape), 'deviation', dev, 'bound', bound)
            assert v.numpy().shape == want.shape and dev <= bound, k
        assert sorted(k for k in d if k.startswith('spatial_features_')) == [
            'spatial_features_2d', 'spatial_features_2x', 'spatial_features_4x', 'spatial_features_8x']
        assert d['spatial_features_2d'].shape == (2, 24, K.SMALL_INPUT[2] // 4, K.SMALL_INPUT[3] // 4)


def test_full_config_state_dict_is_the_reference_one(g16):
    _, meta = g16
    model = _full()
    sd = model.state_dict()
    assert list(sd) == meta['full_keys']
    assert [list(v.shape) for v in sd.values()] == meta['full_shapes']
    assert all(v.device.type == 'cpu' for v in sd.values())
    assert sd['global_step'].dtype == torch.int64 and [n for n, _ in model.named_children()] == [
        'vfe', 'map_to_bev_module', 'backbone_2d', 'dense_head']
    # a checkpoint of these shapes loads strictly; one with a key more, or a shape off, does not
    rng = np.random.default_rng(0)
    state = {k: torch.from_numpy(np.asarray(rng.standard_normal(s), np.float32)).to(sd[k].dtype)
             for k, s in zip(meta['full_keys'], meta['full_shapes'])}
    state['global_step'] = torch.tensor([7])
    model.load_state_dict(state, strict=True)
    assert int(model.global_step) == 7
    model.update_global_step()
    assert int(model.global_step) == 8
    assert torch.equal(model.dense_head.heads_list[5].hm[1].weight, state['dense_head.heads_list.5.hm.1.weight'])
    with pytest.raises(RuntimeError):
        model.load_state_dict(dict(state, extra=torch.zeros(1)), strict=True)
    with pytest.raises(RuntimeError):
        model.load_state_dict(dict(state, **{'backbone_2d.blocks.0.1.weight': torch.zeros(64, 64, 3, 2)}), strict=True)


def test_checkpoint_file_round_trip_on_the_cpu(tmp_path):
    a, b = _full(), _full()
    path = str(tmp_path / 'ckpt.pth')
    torch.save({'model_state': a.state_dict(), 'epoch': 3}, path)
    ckpt = b.load_params_from_file(path, to_cpu=True)
    assert ckpt['epoch'] == 3
    for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    with pytest.raises(FileNotFoundError):
        b.load_params_from_file(str(tmp_path / 'missing.pth'))


def test_initialisation_rules():
    model = _full()
    head = model.dense_head
    assert len(head.heads_list) == 6 and head.predict_boxes_when_training is False
    assert head.shared_conv[0].bias is not None                                    # USE_BIAS_BEFORE_NORM
    for h, names in zip(head.heads_list, K.FULL_MODEL['DENSE_HEAD']['CLASS_NAMES_EACH_HEAD']):
        assert h.hm[-1].out_channels == len(names)
        assert torch.all(h.hm[-1].bias == np.float32(-2.19))
        for name in ('center', 'center_z', 'dim', 'rot'):
            fc = getattr(h, name)
            for m in fc.modules():
                if isinstance(m, torch.nn.Conv2d):
                    assert m.bias is not None and not m.bias.any(), name
            # Kaiming normal, fan_in = 64 * 9: a standard deviation of sqrt(2 / 576), far from the default's uniform one
            std = float(fc[0][0].weight.std())
            assert abs(std - (2 / 576) ** 0.5) < 0.1 * (2 / 576) ** 0.5, (name, std)
    for m in model.backbone_2d.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            assert m.eps == 1e-3 and m.momentum == 0.01
    assert head.shared_conv[1].eps == 1e-5 and head.shared_conv[1].momentum == 0.1          # BN_EPS / BN_MOM defaults
    # the stride-0.5 deblock is a strided convolution, the others are transposed
    kinds = [type(d[0]).__name__ for d in model.backbone_2d.deblocks]
    assert kinds == ['Conv2d', 'ConvTranspose2d', 'ConvTranspose2d'] and model.backbone_2d.deblocks[0][0].stride == (2, 2)


def test_bn_options_extra_deblock_and_absent_modules():
    from dfu3d_amd.pcdet_kitti.base_bev_backbone import BaseBEVBackbone
    from dfu3d_amd.pcdet_kitti.center_head_module import CenterHeadModule
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    ds = K.SMALL_DATASET
    cfg = dict(K.SMALL_MODEL['DENSE_HEAD'], BN_EPS=1e-3, BN_MOM=0.01, USE_BIAS_BEFORE_NORM=False)
    head = CenterHeadModule(cfg, 24, 3, ds['class_names'], ds['grid_size'], ds['point_cloud_range'], ds['voxel_size'])
    assert head.shared_conv[1].eps == 1e-3 and head.shared_conv[1].momentum == 0.01 and head.shared_conv[0].bias is None
    assert head.heads_list[0].center[0][0].bias is None and head.heads_list[0].center[0][1].eps == 1e-3
    bb = BaseBEVBackbone({'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [4, 8],
                          'UPSAMPLE_STRIDES': [1, 2, 2], 'NUM_UPSAMPLE_FILTERS': [4, 4, 4]}, input_channels=4)
    # one UPSAMPLE_STRIDES entry more than levels: the reference's trailing transposed convolution over sum(filters) maps
    assert len(bb.deblocks) == 3 and bb.num_bev_features == 12
    assert tuple(bb.state_dict()['deblocks.2.0.weight'].shape) == (12, 12, 2, 2)
    bb = BaseBEVBackbone({'LAYER_NUMS': [1, 1], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [4, 8],
                          'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [4, 4]}, input_channels=4).eval()
    with torch.no_grad():
        out = bb({'spatial_features': torch.zeros(1, 4, 8, 12)})
    assert out['spatial_features_2d'].shape == (1, 8, 8, 12) and out['spatial_features_2x'].shape == (1, 8, 4, 6)
    none = BaseBEVBackbone({}, input_channels=4)
    assert len(none.blocks) == 0 and none.num_bev_features == 0
    for section, entry in (('BACKBONE_3D', {'NAME': 'VoxelResBackBone8x'}), ('ROI_HEAD', {'NAME': 'PVRCNNHead'})):
        with pytest.raises(NotImplementedError, match=section):
            CenterPoint(dict(K.SMALL_MODEL, **{section: entry}), 3, **ds)
    with pytest.raises(NotImplementedError, match="HeightCompression"):
        CenterPoint(dict(K.SMALL_MODEL, MAP_TO_BEV={'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 8}), 3, **ds)

    class Encoder:
        num_point_features = 4

    class Dataset:
        class_names, grid_size = ds['class_names'], np.array(ds['grid_size'])
        point_cloud_range, voxel_size = np.array(ds['point_cloud_range'], np.float32), ds['voxel_size']
        point_feature_encoder = Encoder()
    m = CenterPoint(K.cfg(K.SMALL_MODEL), 3, Dataset())
    assert m.mode == 'TRAIN' and m.eval().mode == 'TEST' and len(m.module_list) == 4
