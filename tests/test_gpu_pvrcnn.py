"""GPU: VoxelSetAbstraction, PointHeadSimple and PVRCNNHead on golden G26, and a small PVRCNN over a KITTI directory.

On G26 (tests/golden/capture_pvrcnn_golden.py: the reference's modules on the CPU) the keypoints and every ball index are
equal; the float outputs are within d_hip <= max(4 * d_torch, 4 ulp at the golden's largest magnitude), d_torch being the
deviation of a plain formulation on the same GPU -- torch indexing with the GOLDEN's indices through the same layers --
the rule of goldens G20, G21 and G25.  Both deviations are printed.

The detector: the grid of tests/test_gpu_voxel_centerpoint.py, 64 keypoints, GRID_SIZE 3, NMS_POST_MAXSIZE 16."""
import copy

import numpy as np
import pytest

from tests import anchor_target_ref as AR
from tests import ingest_cases as KC
from tests import point_stack_ref as R
from tests.centerpoint_cases import Cfg, cfg
from tests.test_gpu_voxel_centerpoint import kitti_cfg
from tests.test_oracle_point_stack import SOURCES, g26  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _within(name, hip, plain, gold):
    hip, plain = hip.detach().cpu().numpy().reshape(gold.shape), plain.detach().cpu().numpy().reshape(gold.shape)
    d_hip, d_torch = float(np.abs(hip - gold).max()), float(np.abs(plain - gold).max())
    floor = 4.0 * float(np.spacing(np.float32(np.abs(gold).max())))
    print("G26 %-28s d_hip %.3g  d_torch %.3g  floor %.3g  (largest |golden| %.3g)" % (name, d_hip, d_torch, floor, np.abs(gold).max()))
    assert d_hip <= max(4.0 * d_torch, floor), (name, d_hip, d_torch, floor)


class Level:
    def __init__(self, indices, features):
        self.indices, self.features = indices, features


def modules_on_golden(g):
    import torch
    from dfu3d_amd.pcdet_kitti.point_head_simple import PointHeadSimple
    from dfu3d_amd.pcdet_kitti.pvrcnn_head import PVRCNNHead
    from dfu3d_amd.pcdet_kitti.voxel_set_abstraction import VoxelSetAbstraction
    pfe = VoxelSetAbstraction(R.G26_PFE, R.G26_VOXEL, R.G26_RANGE, num_bev_features=R.G26_BEV[0], num_rawpoint_features=4)
    head = PointHeadSimple(1, pfe.num_point_features_before_fusion, R.G26_POINT_HEAD)
    roi = PVRCNNHead(pfe.num_point_features, R.G26_ROI_HEAD, 1)
    for tag, model in (('pfe', pfe), ('point_head', head), ('roi_head', roi)):
        model.load_state_dict({k: torch.from_numpy(g['sd_%s_%s' % (tag, k)].copy()) for k in model.state_dict()}, strict=True)
        model.to(DEV).eval()
    pfe.check = True
    return pfe, head, roi


def golden_batch(g):
    import torch
    return dict(batch_size=R.G26_B, points=cu(g['points']), spatial_features=cu(g['spatial_features']),
                spatial_features_stride=R.G26_BEV_STRIDE,
                multi_scale_3d_features={n: Level(cu(g[n + '_indices']), cu(g[n + '_features'])) for n in R.G26_LEVEL_CHANNELS},
                rois=cu(g['rois']), roi_scores=torch.zeros(R.G26_B, R.G26_ROIS, device=DEV),
                roi_labels=torch.ones(R.G26_B, R.G26_ROIS, dtype=torch.long, device=DEV), has_class_labels=False)


def plain_sa(layer, xyz, start, ctr, cstart, feats, balls):
    """StackSAModuleMSG in torch indexing with given (idx, empty) per scale: gather, subtract, zero, MLP, max."""
    import torch
    rows_of = torch.repeat_interleave(torch.arange(len(cstart) - 1, device=DEV), (cstart[1:] - cstart[:-1]).long())
    out = []
    for mlp, (idx, empty) in zip(layer.mlps, balls):
        gidx = idx.long() + start[:-1].long()[rows_of][:, None]               # (M, ns) global rows
        grouped = torch.cat([xyz[gidx] - ctr[:, None, :], feats[gidx]], dim=-1)   # (M, ns, 3 + C)
        grouped = torch.where(empty.bool()[:, None, None], torch.zeros_like(grouped), grouped)
        x = mlp(grouped.permute(2, 0, 1).unsqueeze(0))
        out.append(x.max(dim=-1)[0].squeeze(0).t())
    return torch.cat(out, dim=1)


def test_modules_on_golden_g26(g26):  # noqa: F811
    import torch
    from dfu3d_amd import point_stack_ops as ops
    from dfu3d_amd.pcdet_kitti.common_utils import get_voxel_centers
    g = g26
    pfe, head, roi = modules_on_golden(g)
    K = R.G26_PFE['NUM_KEYPOINTS']
    with torch.no_grad():
        batch = roi(head(pfe(golden_batch(g))))
        assert int(pfe.status.item()) == 0
        kp = batch['point_coords']
        assert np.array_equal(kp.cpu().numpy().view(np.uint32), g['point_coords'].view(np.uint32))
        kcnt = torch.full((R.G26_B,), K, dtype=torch.int32, device=DEV)
        kstart = ops.starts(kcnt)
        # every ball index of every source, from the modules' own one-launch query; the plain formulation on the golden's
        plain_parts = []
        bev = ops.bev_sample(kp, cu(g['spatial_features']), R.G26_RANGE, R.G26_VOXEL, R.G26_BEV_STRIDE)
        assert np.array_equal(bev.cpu().numpy().view(np.uint32), g['bev_features'].view(np.uint32))
        plain_parts.append(cu(g['bev_features']))
        per_source = {}
        for src in SOURCES:
            if src == 'raw_points':
                layer, pts = pfe.SA_rawpoints, cu(g['points'])
                xyz, feats, col = pts[:, 1:4], pts[:, 4:].contiguous(), pts[:, 0]
            else:
                layer, ind = pfe.SA_layers[pfe.SA_layer_names.index(src)], cu(g[src + '_indices'])
                xyz = get_voxel_centers(ind[:, 1:4], R.G26_PFE['SA_LAYER'][src]['DOWNSAMPLE_FACTOR'], R.G26_VOXEL, R.G26_RANGE)
                feats, col = cu(g[src + '_features']), ind[:, 0]
            cnt, start = ops.counts(col, R.G26_B)
            balls = layer.ball_indices(xyz, cnt, kp[:, 1:4], kcnt)
            for s, (idx, empty) in enumerate(balls):
                assert np.array_equal(idx.cpu().numpy(), g['ball_%s_%d' % (src, s)]), (src, s)
                assert np.array_equal(empty.cpu().numpy(), g['empty_%s_%d' % (src, s)]), (src, s)
            gold_balls = [(cu(g['ball_%s_%d' % (src, s)]), cu(g['empty_%s_%d' % (src, s)])) for s in range(2)]
            per_source[src] = plain_sa(layer, xyz.contiguous(), start, cu(g['point_coords'])[:, 1:4], kstart, feats, gold_balls)
        plain_parts += [per_source[s] for s in SOURCES]                       # the forward's order: bev, raw points, the levels
        plain_before = torch.cat(plain_parts, dim=-1)
        plain_fused = pfe.vsa_point_feature_fusion(plain_before)
        plain_scores = torch.sigmoid(head.cls_layers(plain_before)).max(dim=-1)[0]
        _within('point_features_before_fusion', batch['point_features_before_fusion'], plain_before, g['point_features_before_fusion'])
        _within('point_features', batch['point_features'], plain_fused, g['point_features'])
        _within('point_cls_scores', batch['point_cls_scores'], plain_scores, g['point_cls_scores'])
        # the RoI head: grid points, the pooling's ball indices, pooled features, the decoded boxes
        glob, local = roi.get_global_grid_points_of_roi(batch['rois'], grid_size=2)
        _within('local_grid_points', local, cu(g['local_grid_points']), g['local_grid_points'])
        gold_glob = cu(g['global_grid_points'])
        rois = cu(g['rois']).view(-1, 7)
        cosa, sina = torch.cos(rois[:, 6:7]), torch.sin(rois[:, 6:7])
        loc = cu(g['local_grid_points'])
        plain_glob = torch.stack([loc[..., 0] * cosa - loc[..., 1] * sina, loc[..., 0] * sina + loc[..., 1] * cosa, loc[..., 2]],
                                 dim=-1) + rois[:, None, 0:3]
        _within('global_grid_points', glob, plain_glob, g['global_grid_points'])
        gcnt = torch.full((R.G26_B,), R.G26_ROIS * 8, dtype=torch.int32, device=DEV)
        gold_kp = cu(g['point_coords'])
        balls = roi.roi_grid_pool_layer.ball_indices(gold_kp[:, 1:4], kcnt, gold_glob.view(-1, 3), gcnt)
        for s, (idx, empty) in enumerate(balls):
            assert np.array_equal(idx.cpu().numpy(), g['ball_roi_grid_%d' % s]) and np.array_equal(empty.cpu().numpy(), g['empty_roi_grid_%d' % s])
        gold_balls = [(cu(g['ball_roi_grid_%d' % s]), cu(g['empty_roi_grid_%d' % s])) for s in range(2)]
        weighted = cu(g['point_features']) * cu(g['point_cls_scores']).view(-1, 1)
        plain_pooled = plain_sa(roi.roi_grid_pool_layer, gold_kp[:, 1:4].contiguous(), kstart, gold_glob.view(-1, 3),
                                ops.starts(gcnt), weighted, gold_balls).view(-1, 8, 16)
        gold_dict = dict(batch_size=R.G26_B, rois=cu(g['rois']), point_coords=gold_kp, point_features=cu(g['point_features']),
                         point_cls_scores=cu(g['point_cls_scores']))
        _within('pooled_features', roi.roi_grid_pool(gold_dict), plain_pooled, g['pooled_features'])
        shared = roi.shared_fc_layer(plain_pooled.permute(0, 2, 1).contiguous().view(plain_pooled.shape[0], -1, 1))
        p_cls = roi.cls_layers(shared).transpose(1, 2).contiguous().squeeze(1)
        p_reg = roi.reg_layers(shared).transpose(1, 2).contiguous().squeeze(1)
        # the plain decoding: ResidualCoder against the RoI at the origin, the rotation, the shift
        r = cu(g['rois'])
        q = p_reg.view(R.G26_B, -1, 7)
        diag = torch.sqrt(r[..., 3] ** 2 + r[..., 4] ** 2)
        lx, ly, lz = q[..., 0] * diag, q[..., 1] * diag, q[..., 2] * r[..., 5]
        c, s_ = torch.cos(r[..., 6]), torch.sin(r[..., 6])
        plain_box = torch.stack([lx * c - ly * s_ + r[..., 0], lx * s_ + ly * c + r[..., 1], lz + r[..., 2],
                                 torch.exp(q[..., 3]) * r[..., 3], torch.exp(q[..., 4]) * r[..., 4],
                                 torch.exp(q[..., 5]) * r[..., 5], q[..., 6] + r[..., 6]], dim=-1)
        _within('batch_cls_preds', batch['batch_cls_preds'], p_cls.view(R.G26_B, -1, 1), g['batch_cls_preds'])
        for col, name in enumerate(('x', 'y', 'z', 'dx', 'dy', 'dz', 'heading')):
            _within('batch_box_preds ' + name, batch['batch_box_preds'][..., col], plain_box[..., col], g['batch_box_preds'][..., col])
    assert batch['cls_preds_normalized'] is False and tuple(batch['batch_box_preds'].shape) == (R.G26_B, R.G26_ROIS, 7)


def test_forward_without_check_makes_no_host_read(g26):  # noqa: F811
    """No synchronisation and no device-to-host copy in the forward of the PFE, the point head and the RoI head (the RoIs
    given, so no NMS runs): torch's sync debug mode raises on any synchronising call of torch's own; the library itself
    never synchronises."""
    import torch
    pfe, head, roi = modules_on_golden(g26)
    pfe.check = False
    batch = golden_batch(g26)

    def step():
        with torch.no_grad():
            return roi(head(pfe(dict(batch))))
    step()                                                                 # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out['batch_box_preds']).all()) and int(pfe.status.item()) == 0


def test_stack_sa_module_backward_is_reproducible(g26):  # noqa: F811
    """StackSAModuleMSG as an autograd module: the gradient of the features through the grouping backward, twice."""
    import torch
    from dfu3d_amd import point_stack_ops as ops
    from dfu3d_amd.pcdet_kitti.pointnet2_stack_modules import StackSAModuleMSG
    torch.manual_seed(3)
    layer = StackSAModuleMSG(radii=[0.8, 1.6], nsamples=[4, 8], mlps=[[16, 8], [16, 8]]).to(DEV).eval()
    kp, feats = cu(g26['point_coords']), cu(g26['point_features'])
    kcnt = torch.full((R.G26_B,), 48, dtype=torch.int32, device=DEV)
    grid = cu(g26['global_grid_points']).view(-1, 3)
    gcnt = torch.full((R.G26_B,), R.G26_ROIS * 8, dtype=torch.int32, device=DEV)
    grads = []
    for _ in range(2):
        f = feats.clone().requires_grad_(True)
        st = torch.zeros(1, dtype=torch.int32, device=DEV)
        with ops.status_scope(st):
            _, out = layer(kp[:, 1:4], kcnt, grid, gcnt, f)
            out.square().sum().backward()
        assert int(st.item()) == 0 and f.grad.shape == feats.shape and bool(f.grad.abs().sum() > 0)
        grads.append(f.grad.cpu().numpy())
    assert np.array_equal(grads[0].view(np.uint32), grads[1].view(np.uint32))
    balls = [(cu(g26['ball_roi_grid_%d' % s]), cu(g26['empty_roi_grid_%d' % s])) for s in range(2)]
    f = feats.clone().requires_grad_(True)
    plain_sa(layer, kp[:, 1:4].contiguous(), ops.starts(kcnt), grid, ops.starts(gcnt), f, balls).square().sum().backward()
    ref = f.grad.cpu().numpy()
    assert np.abs(grads[0] - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())   # torch's own order of the same sums


# ---- PVRCNN on a KITTI directory ---------------------------------------------------------------------------------------------
PV_MODEL = dict(
    copy.deepcopy(AR.SECOND_MODEL), NAME='PVRCNN',
    PFE={'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': 64, 'NUM_OUTPUT_FEATURES': 32,
         'SAMPLE_METHOD': 'FPS', 'FEATURES_SOURCE': ['bev', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'raw_points'],
         'SA_LAYER': {
             'raw_points': {'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]},
             'x_conv1': {'DOWNSAMPLE_FACTOR': 1, 'MLPS': [[16, 16], [16, 16]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [16, 16]},
             'x_conv2': {'DOWNSAMPLE_FACTOR': 2, 'MLPS': [[32, 32], [32, 32]], 'POOL_RADIUS': [0.8, 1.2], 'NSAMPLE': [16, 32]},
             'x_conv3': {'DOWNSAMPLE_FACTOR': 4, 'MLPS': [[64, 16], [64, 16]], 'POOL_RADIUS': [1.2, 2.4], 'NSAMPLE': [16, 32]},
             'x_conv4': {'DOWNSAMPLE_FACTOR': 8, 'MLPS': [[64, 16], [64, 16]], 'POOL_RADIUS': [2.4, 4.8], 'NSAMPLE': [16, 32]}}},
    POINT_HEAD={'NAME': 'PointHeadSimple', 'CLS_FC': [32, 32], 'CLASS_AGNOSTIC': True, 'USE_POINT_FEATURES_BEFORE_FUSION': True},
    ROI_HEAD=dict(copy.deepcopy(R.G26_ROI_HEAD), SHARED_FC=[32, 32], CLS_FC=[32, 32], REG_FC=[32, 32],
                  NMS_CONFIG={'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 256,
                                       'NMS_POST_MAXSIZE': 16, 'NMS_THRESH': 0.7}},
                  ROI_GRID_POOL={'GRID_SIZE': 3, 'MLPS': [[16, 16], [16, 16]], 'POOL_RADIUS': [0.8, 1.6], 'NSAMPLE': [16, 16],
                                 'POOL_METHOD': 'max_pool'}))
PV_MODEL['POST_PROCESSING'] = dict(PV_MODEL['POST_PROCESSING'], SCORE_THRESH=0.05)


@pytest.fixture(scope="module")
def kitti_root(tmp_path_factory):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import create_kitti_infos
    root = str(tmp_path_factory.mktemp("kitti_pvrcnn"))
    KC.write_kitti(root, KC.all_frames(), split='train')
    plain = kitti_cfg()
    plain['DATA_PROCESSOR'] = plain['DATA_PROCESSOR'][:1]
    create_kitti_infos(plain, KC.CLASSES, root, root, workers=2)
    return root


def test_pvrcnn_evaluates_and_reloads(kitti_root, tmp_path):
    import torch
    from dfu3d_amd.eval_utils.eval_utils import eval_one_epoch
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    from dfu3d_amd.pcdet_kitti.pv_rcnn import PVRCNN
    ds = KittiDataset(kitti_cfg(), AR.CLASS_NAMES, training=False, root_path=kitti_root, device=DEV)
    ds.voxel_features_only = True
    assert [int(v) for v in ds.grid_size] == [128, 96, 40]
    torch.manual_seed(26)
    model = PVRCNN(cfg(PV_MODEL), len(AR.CLASS_NAMES), dataset=ds).to(DEV)
    assert [type(m).__name__ for m in model.module_list] == [
        'MeanVFE', 'VoxelBackBone8x', 'HeightCompression', 'VoxelSetAbstraction', 'BaseBEVBackbone', 'AnchorHeadSingle',
        'PointHeadSimple', 'PVRCNNHead']
    assert model.roi_head.shared_fc_layer[0].weight.shape[1] == 27 * 32
    with pytest.raises(NotImplementedError, match="training mode"):
        model.train()(next(iter(ds.batches(2))))
    model.eval()
    model.pfe.check = True                                                   # raises on any status bit of the stage
    with torch.no_grad():
        batch = next(iter(ds.batches(2)))
        pred, recall = model(batch)
    assert tuple(batch['rois'].shape) == (2, 16, 7) and tuple(batch['point_coords'].shape) == (128, 4)
    assert tuple(batch['point_features'].shape) == (128, 32) and tuple(batch['batch_box_preds'].shape) == (2, 16, 7)
    assert len(pred) == 2 and all(set(p) >= {'pred_boxes', 'pred_scores', 'pred_labels'} for p in pred) and 'gt' in recall
    for p in pred:
        n = p['pred_scores'].shape[0]
        assert 0 < n <= 16 and tuple(p['pred_boxes'].shape) == (n, 7)
        assert bool(torch.isfinite(p['pred_boxes']).all()) and bool(torch.isfinite(p['pred_scores']).all())
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())
    # its own state dict, strict
    torch.manual_seed(27)
    fresh = PVRCNN(cfg(PV_MODEL), len(AR.CLASS_NAMES), dataset=ds).to(DEV)
    assert list(fresh.state_dict()) == list(model.state_dict())
    fresh.load_state_dict(model.state_dict(), strict=True)
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in fresh.state_dict().items())

    class Logger:
        def info(self, msg):
            pass
    ret = eval_one_epoch(cfg({'MODEL': PV_MODEL}), Cfg(save_to_file=False), fresh.eval(), ds.batches(2), 1, Logger(),
                         result_dir=tmp_path / 'eval')
    assert all(0.0 <= ret['recall/rcnn_' + t] <= 1.0 for t in ('0.3', '0.5', '0.7'))
