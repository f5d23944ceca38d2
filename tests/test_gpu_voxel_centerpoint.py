"""The voxel backbones, HeightCompression and CenterPoint(..., sparse_3d=True) on the GPU.

The backbones are compared with a DENSE emulation of the same modules in torch on the CPU: every sparse tensor is a
dense float64 block plus an occupancy mask, a submanifold layer is conv3d times the mask, a strided layer is conv3d with
the mask grown by the kernel's window, BatchNorm (evaluation mode) and ReLU act on the occupied cells.  Indices and shapes
of all five levels must equal the masks exactly; the features are compared relative to max|ref| per level, and this
package's error may be at most 8 times the error of torch's own float32 evaluation of the same dense model (a different
but equally long summation order).

Measured on an MI355X (grid 32 x 32 x 40, 700 voxels, B = 2), error relative to max|ref| at conv_out: VoxelBackBone8x
2.74e-7 against torch float32's 1.67e-7, VoxelResBackBone8x 5.26e-7 against 2.49e-7; the largest ratio over all levels is
2.1.  The test prints both numbers for every level.

The whole model's two runs from one seed are compared bit for bit with torch's own dense convolutions asked for their
deterministic algorithms (torch.backends.cudnn.deterministic).  Left to itself the vendor library's convolutions gave a
loss of 21.811937 in one run of this test and 21.811934 in the next (tests/test_gpu_centerpoint.py compares no two runs
for that reason); the part this package computes itself is compared without that switch."""
import numpy as np
import pytest

from tests import centerpoint_cases as C
from tests import ingest_cases as KC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = [32, 32, 40]
LEVELS = ('x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'out')


# ---- the dense emulation ------------------------------------------------------------------------------------------------
def dense_module(m, x, mask, dtype):
    """(features (B, C, D, H, W), mask (B, 1, D, H, W) bool) through module m of the sparse model, densely."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F
    from dfu3d_amd.pcdet_kitti import spconv_utils as S
    from dfu3d_amd.pcdet_kitti.spconv_backbone import SparseBasicBlock
    if isinstance(m, S.SparseConvolution):
        w = m.weight.detach().cpu().to(dtype).permute(0, 4, 1, 2, 3).contiguous()
        y = F.conv3d(x, w, stride=m.stride, padding=m.padding)
        if not m.subm:
            mask = F.conv3d(mask.to(torch.float64), torch.ones((1, 1) + m.kernel_size, dtype=torch.float64),
                            stride=m.stride, padding=m.padding) > 0
        if m.bias is not None:
            y = y + m.bias.detach().cpu().to(dtype).view(1, -1, 1, 1, 1)
        return y * mask, mask
    if isinstance(m, nn.BatchNorm1d):
        p = [t.detach().cpu().to(dtype).view(1, -1, 1, 1, 1) for t in (m.running_mean, m.running_var, m.weight, m.bias)]
        return ((x - p[0]) / torch.sqrt(p[1] + m.eps) * p[2] + p[3]) * mask, mask
    if isinstance(m, nn.ReLU):
        return torch.relu(x), mask
    if isinstance(m, SparseBasicBlock):
        y, _ = dense_module(m.conv1, x, mask, dtype)
        y, _ = dense_module(m.bn1, y, mask, dtype)
        y, _ = dense_module(m.conv2, torch.relu(y), mask, dtype)
        y, _ = dense_module(m.bn2, y, mask, dtype)
        return torch.relu(y + x), mask
    if isinstance(m, S.SparseSequential):
        for child in m._modules.values():
            x, mask = dense_module(child, x, mask, dtype)
        return x, mask
    raise TypeError(type(m))


def dense_backbone(bb, feats, coords, B, dtype):
    import torch
    D, H, W = bb.sparse_shape
    x = torch.zeros((B, feats.shape[1], D, H, W), dtype=dtype)
    mask = torch.zeros((B, 1, D, H, W), dtype=torch.bool)
    c = torch.from_numpy(coords).long()
    x[c[:, 0], :, c[:, 1], c[:, 2], c[:, 3]] = torch.from_numpy(feats).to(dtype)
    mask[c[:, 0], 0, c[:, 1], c[:, 2], c[:, 3]] = True
    out = {}
    x, mask = dense_module(bb.conv_input, x, mask, dtype)
    for name, stage in zip(LEVELS, (bb.conv1, bb.conv2, bb.conv3, bb.conv4, bb.conv_out)):
        x, mask = dense_module(stage, x, mask, dtype)
        out[name] = (x, mask)
    return out


def random_voxels(seed, n=700, B=2):
    rng = np.random.default_rng(seed)
    D, H, W = GRID[2], GRID[1], GRID[0]
    ids = rng.permutation(B * D * H * W)[:n]
    coords = np.stack([ids // (D * H * W), (ids // (H * W)) % D, (ids // W) % H, ids % W], 1).astype(np.int32)
    return rng.standard_normal((n, 4)).astype(np.float32), coords


def randomise_norms(model, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.1)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.1)


@pytest.mark.parametrize("name", ["VoxelBackBone8x", "VoxelResBackBone8x"])
def test_a_backbone_against_the_dense_float64_model(name):
    import torch
    from dfu3d_amd.pcdet_kitti import spconv_backbone
    from dfu3d_amd.pcdet_kitti.height_compression import HeightCompression
    torch.manual_seed(3)
    bb = getattr(spconv_backbone, name)({}, 4, GRID).eval()
    randomise_norms(bb, 4)
    feats, coords = random_voxels(5)
    ref = dense_backbone(bb, feats, coords, 2, torch.float64)
    low = dense_backbone(bb, feats, coords, 2, torch.float32)
    bb = bb.to(DEV)
    with torch.no_grad():
        batch = bb({'batch_size': 2, 'voxel_features': torch.from_numpy(feats).to(DEV),
                    'voxel_coords': torch.from_numpy(coords).to(DEV)})
        batch = HeightCompression({'NUM_BEV_FEATURES': 256})(batch)
    assert batch['encoded_spconv_tensor_stride'] == 8 and batch['multi_scale_3d_strides'] == {
        'x_conv1': 1, 'x_conv2': 2, 'x_conv3': 4, 'x_conv4': 8}
    tensors = dict(batch['multi_scale_3d_features'], out=batch['encoded_spconv_tensor'])
    shapes = {'x_conv1': [41, 32, 32], 'x_conv2': [21, 16, 16], 'x_conv3': [11, 8, 8], 'x_conv4': [5, 4, 4], 'out': [2, 4, 4]}
    for lv in LEVELS:
        t = tensors[lv]
        x64, mask = ref[lv]
        idx = t.indices.cpu().numpy().astype(np.int64)
        assert t.spatial_shape == shapes[lv] == list(mask.shape[2:]) and t.features.shape[1] == x64.shape[1]
        got_mask = torch.zeros_like(mask)
        got_mask[idx[:, 0], 0, idx[:, 1], idx[:, 2], idx[:, 3]] = True
        assert len(idx) == int(mask.sum()) and bool((got_mask == mask).all()), lv
        want = x64[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]].numpy()
        f32 = low[lv][0][idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]].numpy().astype(np.float64)
        got = t.features.cpu().numpy().astype(np.float64)
        scale = np.abs(want).max()
        err, err32 = np.abs(got - want).max() / scale, np.abs(f32 - want).max() / scale
        print("%s %s: %d sites, max|ref| %.3g, error / max|ref|: this package %.3g, torch float32 dense %.3g"
              % (name, lv, len(idx), scale, err, err32))
        assert scale > 0 and err <= 8 * err32, (lv, err, err32)
    # the padded form of prepare_batch: a -1 / NaN tail behind the device count `n_voxels` is never read, the same bits come out
    pad_c = np.concatenate([coords, np.full((45, 4), -1, np.int32)])
    pad_f = np.concatenate([feats, np.full((45, 4), np.nan, np.float32)])
    with torch.no_grad():
        padded = bb({'batch_size': 2, 'voxel_features': torch.from_numpy(pad_f).to(DEV),
                     'voxel_coords': torch.from_numpy(pad_c).to(DEV),
                     'n_voxels': torch.tensor([len(coords)], dtype=torch.int32, device=DEV)})
    got_pad = dict(padded['multi_scale_3d_features'], out=padded['encoded_spconv_tensor'])
    for lv in LEVELS:
        assert torch.equal(got_pad[lv].indices, tensors[lv].indices) and torch.equal(got_pad[lv].features, tensors[lv].features), lv
    # HeightCompression: the emulation's dense().view
    x64, mask = ref['out']
    sf = batch['spatial_features']
    assert tuple(sf.shape) == (2, 256, 4, 4) and batch['spatial_features_stride'] == 8
    want = x64.view(2, 256, 4, 4).numpy()
    got = sf.cpu().numpy().astype(np.float64)
    off = ~mask.expand(2, 128, 2, 4, 4).reshape(2, 256, 4, 4).numpy()
    assert not got[off].any() and np.abs(got - want).max() <= 8 * np.abs(low['out'][0].view(2, 256, 4, 4).numpy() - want).max()
    t = tensors['out']
    idx = t.indices.cpu().numpy()
    mine = np.zeros((2, 128, 2, 4, 4), np.float32)
    mine[idx[:, 0], :, idx[:, 1], idx[:, 2], idx[:, 3]] = t.features.cpu().numpy()
    assert sf.cpu().numpy().tobytes() == mine.reshape(2, 256, 4, 4).tobytes()


# ---- CenterPoint(..., sparse_3d=True) on a KITTI directory --------------------------------------------------------------
CLASSES = ['Car']
# the MODEL section of cfgs/kitti_models/centerpoint.yaml
MODEL = {
    'NAME': 'CenterPoint',
    'VFE': {'NAME': 'MeanVFE'},
    'BACKBONE_3D': {'NAME': 'VoxelResBackBone8x'},
    'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [5], 'LAYER_STRIDES': [1], 'NUM_FILTERS': [128],
                    'UPSAMPLE_STRIDES': [2], 'NUM_UPSAMPLE_FILTERS': [256]},
    'DENSE_HEAD': {
        'NAME': 'CenterHead', 'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': [['Car']], 'SHARED_CONV_CHANNEL': 64,
        'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
        'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'], 'HEAD_DICT': C.HEAD_DICT},
        'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': 4, 'NUM_MAX_OBJS': 500, 'GAUSSIAN_OVERLAP': 0.1, 'MIN_RADIUS': 2},
        'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'code_weights': [1.0] * 8}},
        'POST_PROCESSING': {'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': [-75.2, -75.2, -2, 75.2, 75.2, 4],
                            'MAX_OBJ_PER_SAMPLE': 500,
                            'NMS_CONFIG': {'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.7, 'NMS_PRE_MAXSIZE': 4096,
                                           'NMS_POST_MAXSIZE': 500}}},
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                        'EVAL_METRIC': 'kitti',
                        'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.01,
                                       'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
}
RANGE = C.SMALL_DATASET['point_cloud_range']                      # 32 x 24 x 4 m
VOXEL = [0.25, 0.25, 0.1]                                         # 128 x 96 x 40 cells: the depth ends at 2 as KITTI's does


def kitti_cfg():
    return {'DATA_SPLIT': {'train': 'train', 'test': 'train'},
            'INFO_PATH': {'train': ['kitti_infos_train.pkl'], 'test': ['kitti_infos_train.pkl']},
            'FOV_POINTS_ONLY': True, 'POINT_CLOUD_RANGE': RANGE,
            'DATA_PROCESSOR': [{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True},
                               {'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': {'train': False, 'test': False}},
                               {'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': VOXEL, 'MAX_POINTS_PER_VOXEL': 5,
                                'MAX_NUMBER_OF_VOXELS': {'train': 16000, 'test': 40000}}]}


@pytest.fixture(scope="module")
def kitti_root(tmp_path_factory):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import create_kitti_infos
    root = str(tmp_path_factory.mktemp("kitti_voxel"))
    KC.write_kitti(root, KC.all_frames(), split='train')
    plain = kitti_cfg()
    plain['DATA_PROCESSOR'] = plain['DATA_PROCESSOR'][:1]
    create_kitti_infos(plain, KC.CLASSES, root, root, workers=2)
    return root


def dataset(root, training):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    ds = KittiDataset(kitti_cfg(), CLASSES, training=training, root_path=root, device=DEV)
    ds.voxel_features_only = True
    return ds


def model_for(ds, seed):
    import torch
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    torch.manual_seed(seed)
    return CenterPoint(C.cfg(MODEL), len(CLASSES), dataset=ds, sparse_3d=True).to(DEV)


def one_step(ds, seed):
    """One training forward and backward over the six frames -> (model, loss, {name: grad}).  torch's own dense
    convolutions (the 2-D backbone and the head) are asked for their deterministic algorithms for the step."""
    import torch
    before = torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = True, False
    try:
        model = model_for(ds, seed).train()
        batch = next(iter(ds.batches(6)))
        assert 'voxel_features' in batch and 'voxels' not in batch
        ret, tb, _ = model(batch)
        ret['loss'].backward()
        torch.cuda.synchronize()
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before
    return model, float(ret['loss'].detach()), {k: p.grad.detach().cpu().numpy() for k, p in model.named_parameters()}


def sparse_part_step(ds, seed):
    """The part of the model this package computes itself -- vfe, backbone_3d, map_to_bev_module -- forward and, against
    a fixed random gradient of the map, backward -> (map, {name: grad}) as NumPy."""
    import torch
    model = model_for(ds, seed).train()
    batch = next(iter(ds.batches(6)))
    for m in (model.vfe, model.backbone_3d, model.map_to_bev_module):
        batch = m(batch)
    sf = batch['spatial_features']
    g = torch.Generator(device=DEV).manual_seed(seed)
    sf.backward(torch.randn(sf.shape, generator=g, device=DEV))
    torch.cuda.synchronize()
    return sf.detach().cpu().numpy(), {k: p.grad.detach().cpu().numpy() for k, p in model.backbone_3d.named_parameters()}


def test_centerpoint_voxel_model_trains_evaluates_and_reloads(kitti_root, tmp_path):
    """The test that shows the feature: before it the keyword did not exist and sparse_conv_ops did not import."""
    import torch
    from dfu3d_amd import sparse_conv_ops  # noqa: F401
    from dfu3d_amd.eval_utils.eval_utils import eval_one_epoch
    from dfu3d_amd.train_utils import train_utils as T
    from dfu3d_amd.train_utils.optimization import build_optimizer, build_scheduler
    from tests import optimizer_cases as OC
    ds = dataset(kitti_root, True)
    assert [int(v) for v in ds.grid_size] == [128, 96, 40]
    model, loss, grads = one_step(ds, 31)
    assert [type(m).__name__ for m in model.module_list] == ['MeanVFE', 'VoxelResBackBone8x', 'HeightCompression',
                                                             'BaseBEVBackbone', 'CenterHeadModule']
    assert model.backbone_3d.sparse_shape == [41, 96, 128]
    assert np.isfinite(loss) and loss > 0
    dead = [k for k, g in grads.items() if not np.isfinite(g).all() or not g.any()]
    assert not dead, dead
    # two runs from the same seed: first the sparse part alone, then the whole model
    (sf, g3), (sf2, g32) = sparse_part_step(ds, 33), sparse_part_step(ds, 33)
    assert sf.shape == (6, 256, 12, 16) and sf.any() and sf.tobytes() == sf2.tobytes()
    assert all(g3[k].any() and g3[k].tobytes() == g32[k].tobytes() for k in g3)
    _, loss2, grads2 = one_step(ds, 31)
    differ = [k for k in grads if grads[k].tobytes() != grads2[k].tobytes()]
    print("two runs of the whole model: loss %r and %r, %d of %d gradients differ: %s"
          % (loss, loss2, len(differ), len(grads), differ[:6]))
    assert loss2 == loss and not differ
    # the training loop: two iterations of three frames (one up, one down the cycle)
    loader = ds.batches(3)
    cfg = OC.optim_cfg(PCT_START=0.5)
    opt = build_optimizer(model, cfg)
    sched, _ = build_scheduler(opt, len(loader), 1, -1, cfg)
    rows = []

    class Tb:
        def add_scalar(self, tag, value, step):
            rows.append((tag, float(value), step))

    class Logger:
        def info(self, msg):
            pass
    T.train_model(model, opt, loader, T.model_fn_decorator(), sched, cfg, start_epoch=0, total_epochs=1, start_iter=0, rank=0,
                  tb_log=Tb(), ckpt_save_dir=tmp_path, logger=Logger(), logger_iter_interval=1)
    losses = [v for t, v, _ in rows if t == 'train/loss']
    assert len(losses) == 2 and np.isfinite(losses).all() and int(model.global_step) == 2
    # its own checkpoint, strict
    fresh = model_for(ds, 32)
    ck = fresh.load_params_from_file(str(tmp_path / 'checkpoint_epoch_1.pth'))
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in fresh.state_dict().items()) and 'model_state' in ck
    # evaluation: one step by hand to pred_dicts, then the epoch
    ev = dataset(kitti_root, False)
    fresh.eval()
    with torch.no_grad():
        for head in fresh.dense_head.heads_list:
            head.hm[-1].bias += 2.0                                   # an untrained head scores under the threshold
        pred, recall = fresh(next(iter(ev.batches(2))))
    assert len(pred) == 2 and all(set(p) >= {'pred_boxes', 'pred_scores', 'pred_labels'} for p in pred) and 'gt' in recall
    ret = eval_one_epoch(C.cfg({'MODEL': MODEL}), C.Cfg(save_to_file=False), fresh, ev.batches(2), 1, Logger(),
                         result_dir=tmp_path / 'eval')
    assert all(0.0 <= ret['recall/rcnn_' + t] <= 1.0 for t in ('0.3', '0.5', '0.7'))
