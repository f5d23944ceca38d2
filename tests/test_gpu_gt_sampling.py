"""GPU: ground-truth sampling (dfu3d_gt_sample_collide + dfu3d_gt_sample_paste behind
dfu3d_amd.pcdet_kitti.database_sampler.DataBaseSampler) against G11 (the reference's own sampler), against the NumPy
restatement end to end, on planted geometry and on edge cases."""
import os

import numpy as np
import pytest
import torch

from tests import gt_sampling_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G11 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_gt_sampling.npz")
CENTERPOINT_GROUPS = ['Car:2', 'Truck:3', 'Construction_vehicle:7', 'Bus:4', 'Trailer:6', 'Barrier:2', 'Motorcycle:6',
                      'Bicycle:6', 'Pedestrian:2', 'Traffic_cone:2']


def _same(out, exp_points, exp_boxes, exp_names, tag):
    assert out["points"].dtype == np.float32 and exp_points.dtype == np.float32, tag
    assert np.array_equal(out["points"].view(np.uint32), exp_points.view(np.uint32)), tag
    assert out["gt_boxes"].dtype == exp_boxes.dtype and np.array_equal(out["gt_boxes"], exp_boxes), tag
    assert np.array_equal(out["gt_names"], exp_names), tag


def _g11_scene(g, ci, s):
    d = R.golden_scene(g, s)
    d["gt_boxes"] = d["gt_boxes"].astype(np.float64 if ci == 1 else np.float32)
    return d


@pytest.mark.parametrize("ci", [0, 1])
def test_g11_per_scene_and_batched(tmp_path, ci):
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    g = np.load(G11)
    R.database_from_golden(g, tmp_path)
    names = [str(c) for c in g["class_names"]]
    n = int(g["n_scenes"])
    seed = [11, 12][ci]
    smp = DataBaseSampler(tmp_path, R.golden_cfg(g, ci), names, device=DEV)
    np.random.seed(seed)
    per_scene = [smp(_g11_scene(g, ci, s)) for s in range(n)]
    rng_a = np.random.get_state()
    smp2 = DataBaseSampler(tmp_path, R.golden_cfg(g, ci), names, device=DEV)
    np.random.seed(seed)
    batched = smp2.sample_batch([_g11_scene(g, ci, s) for s in range(n)]).split()
    rng_b = np.random.get_state()
    for s in range(n):
        pre = "out/%d/%d/" % (ci, s)
        _same(per_scene[s], g[pre + "points"], g[pre + "gt_boxes"], g[pre + "gt_names"], ("call", s))
        _same(batched[s], g[pre + "points"], g[pre + "gt_boxes"], g[pre + "gt_names"], ("batch", s))
        assert "gt_boxes_mask" not in batched[s]
    for st in (rng_a, rng_b):
        assert np.array_equal(st[1], g["rng/%d/keys" % ci]) and st[2] == int(g["rng/%d/pos" % ci])


def _write_kitti(root, frames):
    """velodyne / calib / label_2 of synthetic frames (labels = the generator's boxes, in the camera frame)."""
    from dfu3d_amd import kitti_io, synth
    from dfu3d_amd.calibration import Calibration
    scenes = []
    for d in ("velodyne", "calib", "label_2"):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for f in range(frames):
        sc = synth.make_scene(f, H=90, W=160, M=1, cams=1, dense=False, k_min=30, k_max=40)
        sid = "%06d" % f
        pts = sc.points.numpy()
        pts.tofile(os.path.join(root, "velodyne", sid + ".bin"))
        cal = sc.calibs[0]
        kitti_io.write_calib(os.path.join(root, "calib", sid + ".txt"), cal.P2, cal.R0, cal.V2C)
        calib = Calibration(os.path.join(root, "calib", sid + ".txt"))
        b = np.asarray(sc.boxes3d, np.float64)
        bottom = b[:, :3].copy()
        bottom[:, 2] -= b[:, 5] / 2
        loc = calib.lidar_to_rect(bottom)
        lines = []
        for k in range(b.shape[0]):
            name = synth.BOX_TYPES[int(b[k, 7])][0]
            lines.append("%s 0.00 0 0.00 10.00 10.00 120.00 120.00 %.2f %.2f %.2f %.2f %.2f %.2f %.2f" % (
                name, b[k, 5], b[k, 4], b[k, 3], loc[k, 0], loc[k, 1], loc[k, 2], -b[k, 6] - np.pi / 2))
        with open(os.path.join(root, "label_2", sid + ".txt"), "w") as fh:
            fh.write("\n".join(lines) + "\n")
        scenes.append((pts, b))
    return scenes


def _centerpoint_cfg():
    return {'DB_INFO_PATH': ['kitti_dbinfos_train.pkl'], 'USE_SHARED_MEMORY': False,
            'PREPARE': {'filter_by_min_points': [g.split(':')[0] + ':5' for g in CENTERPOINT_GROUPS]},
            'SAMPLE_GROUPS': list(CENTERPOINT_GROUPS), 'NUM_POINT_FEATURES': 4, 'DATABASE_WITH_FAKELIDAR': False,
            'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'LIMIT_WHOLE_SCENE': True}


def test_end_to_end_64_scenes_equal_the_restatement(tmp_path):
    from dfu3d_amd import synth
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    from dfu3d_amd.pcdet_kitti.gt_database import create_groundtruth_database
    root = str(tmp_path / "kitti")
    scenes = _write_kitti(root, 64)
    infos = create_groundtruth_database(root, ["%06d" % f for f in range(64)], batch_frames=32)
    assert set(infos) <= set(t[0] for t in synth.BOX_TYPES)
    classes = [c for c in infos if any(i['num_points_in_gt'] >= 5 for i in infos[c])]
    assert len(classes) >= 4
    cfg = _centerpoint_cfg()

    def dicts():
        out = []
        for pts, b in scenes:
            assert pts.shape == (34720, 4)
            names = np.array([synth.BOX_TYPES[int(t)][0] for t in b[:, 7]])
            out.append({'points': pts.copy(), 'gt_boxes': b[:, :7].astype(np.float32), 'gt_names': names,
                        'gt_boxes_mask': np.ones(len(names), bool)})
        return out
    ref = R.RefSampler(root, cfg, classes)
    np.random.seed(5)
    exp = [ref(d)[0] for d in dicts()]
    smp = DataBaseSampler(root, cfg, classes, device=DEV)
    np.random.seed(5)
    got = smp.sample_batch(dicts()).split()
    pasted = 0
    for s in range(64):
        _same(got[s], exp[s]["points"], exp[s]["gt_boxes"], exp[s]["gt_names"], s)
        pasted += len(got[s]["gt_names"]) - len(scenes[s][1])
    assert pasted > 64


def _planted_db(root, boxes, names, npts=20):
    rng = np.random.default_rng(7)
    pts = []
    for b in boxes:
        p = np.zeros((npts, 4), np.float32)
        p[:, :3] = rng.uniform(-0.4, 0.4, (npts, 3)) * np.asarray(b[3:6])
        p[:, 3] = rng.random(npts)
        pts.append(p)
    R.write_database(root, names, np.asarray(boxes, np.float64), [npts] * len(boxes), pts)


def _cfg(groups, width=(0.0, 0.0, 0.0), limit=False):
    return {'DB_INFO_PATH': ['kitti_dbinfos_train.pkl'], 'PREPARE': {}, 'SAMPLE_GROUPS': groups,
            'NUM_POINT_FEATURES': 4, 'REMOVE_EXTRA_WIDTH': list(width), 'LIMIT_WHOLE_SCENE': limit}


def test_planted_near_touch_geometry(tmp_path):
    """Candidates 1 cm apart are both accepted, 1 cm overlapping collide -- as the exact area decides; scene points
    0.009 m outside a sampled box's face are removed (inside the 1e-2 margin), 0.011 m outside are kept."""
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    from oracle.iou3d_oracle import boxes_bev
    L, W, H = 4.0, 2.0, 1.5
    # group A: boxes 0 / 1 a centimetre apart (accepted both); group B: boxes 2 / 3 overlapping by a centimetre
    boxes = [[10.0, 0.0, -1.0, L, W, H, 0.0], [10.0 + L + 0.01, 0.0, -1.0, L, W, H, 0.0],
             [-10.0, 5.0, -1.0, L, W, H, 0.3], [-10.0 + (L - 0.01) * np.cos(0.3), 5.0 + (L - 0.01) * np.sin(0.3), -1.0,
                                                L, W, H, 0.3]]
    ov = boxes_bev(np.asarray(boxes, np.float32), np.asarray(boxes, np.float32), iou=False)
    assert ov[0, 1] == 0 and ov[2, 3] > 0.01
    _planted_db(tmp_path, boxes, ['Car', 'Car', 'Truck', 'Truck'])
    smp = DataBaseSampler(tmp_path, _cfg(['Car:2', 'Truck:2']), ['Car', 'Truck'], device=DEV)
    ref = R.RefSampler(tmp_path, _cfg(['Car:2', 'Truck:2']), ['Car', 'Truck'])
    # scene points around box 0's +x face / +y face / top, 9 mm and 11 mm outside
    b = boxes[0]
    face = []
    for dd in (0.009, 0.011):                                     # (the +x face is left out: box 1 lies 1 cm beyond it)
        for y in np.linspace(-0.8, 0.8, 9):
            face.append([b[0] - L / 2 - dd, y, -1.0, 0.5])
        for x in np.linspace(8.5, 11.5, 9):
            face.append([x, W / 2 + dd, -1.0, 0.5])
            face.append([x, -W / 2 - dd, -1.0, 0.5])
        face.append([b[0], 0.0, -1.0 + H / 2 + dd, 0.5])          # z has no margin: both outside
    pts = np.array(face, np.float32)
    d = {'points': pts, 'gt_boxes': np.zeros((0, 7), np.float32), 'gt_names': np.array([], '<U8'),
         'gt_boxes_mask': np.zeros(0, bool)}
    np.random.seed(1)
    exp = ref(dict(d))[0]
    np.random.seed(1)
    got = smp(dict(d))
    _same(got, exp["points"], exp["gt_boxes"], exp["gt_names"], "planted")
    assert list(got["gt_names"]).count('Car') == 2 and list(got["gt_names"]).count('Truck') == 0
    kept = got["points"][40:]                                       # after the two pasted Car objects
    n_in = len(pts) - len(kept)
    assert n_in == 27, n_in                                         # the 9 mm rows (3 x 9) go, the 11 mm rows stay


def test_edge_cases_and_determinism(tmp_path):
    """0 scene points, 0 accepted samples, n <= 0 groups, B = 256; the same batch twice gives the same bytes."""
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    rng = np.random.default_rng(3)
    boxes, names = [], []
    for k in range(40):
        boxes.append([rng.uniform(-40, 40), rng.uniform(-40, 40), -1.0, 4.0, 1.8, 1.5, rng.uniform(-3, 3)])
        names.append(['Car', 'Pedestrian'][k % 2])
    _planted_db(tmp_path, boxes, names, npts=30)
    cfg = _cfg(['Car:3', 'Pedestrian:2'], width=(0.2, 0.2, 0.0), limit=True)
    scenes = []
    for s in range(256):
        n = 0 if s % 17 == 0 else int(rng.integers(100, 3000))
        p = np.zeros((n, 4), np.float32)
        p[:, :2] = rng.uniform(-45, 45, (n, 2))
        p[:, 2] = rng.uniform(-2, 0, n)
        p[:, 3] = rng.random(n)
        if s % 13 == 0:                                              # every candidate collides
            gb, gn = np.array([[0, 0, -1, 300, 300, 3, 0]], np.float32), np.array(['Van'])
        elif s % 11 == 0:                                            # LIMIT_WHOLE_SCENE: both groups n <= 0
            gb = np.array([[60 + 6 * k, 60, -1, 4, 1.8, 1.5, 0] for k in range(5)], np.float32)
            gn = np.array(['Car', 'Car', 'Car', 'Pedestrian', 'Pedestrian'])
        else:
            gb, gn = np.zeros((0, 7), np.float32), np.array([], '<U10')
        scenes.append({'points': p, 'gt_boxes': gb, 'gt_names': gn, 'gt_boxes_mask': np.ones(len(gn), bool)})
    copy = lambda: [{k: v.copy() for k, v in d.items()} for d in scenes]
    ref = R.RefSampler(tmp_path, cfg, ['Car', 'Pedestrian'])
    np.random.seed(9)
    exp = [ref(d)[0] for d in copy()]
    outs = []
    for _ in range(2):
        smp = DataBaseSampler(tmp_path, cfg, ['Car', 'Pedestrian'], device=DEV)
        np.random.seed(9)
        batch = smp.sample_batch(copy())
        outs.append((batch.points[:int(batch.point_off[-1])].cpu().numpy().tobytes(), batch.split()))
    assert outs[0][0] == outs[1][0]
    for s in range(256):
        _same(outs[0][1][s], exp[s]["points"], exp[s]["gt_boxes"], exp[s]["gt_names"], s)
        _same(outs[1][1][s], exp[s]["points"], exp[s]["gt_boxes"], exp[s]["gt_names"], s)
    assert len(scenes[17]["points"]) == 0 and len(outs[0][1][17]["points"]) > 0      # 0 scene points + pasted objects
    assert np.array_equal(outs[0][1][13]["gt_names"], np.array(['Van']))
    assert np.array_equal(outs[0][1][11]["points"], scenes[11]["points"])


def test_more_slots_than_one_pass_of_the_offset_scan(tmp_path):
    """350 scenes of at most 2048 points are 350 x 3 slots (the pasted objects + two chunks of 1024 points): the one
    workgroup that scans the slot counts 1024 at a time carries its running total into a second pass, and the scenes
    from 342 on take their offsets from it."""
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    rng = np.random.default_rng(23)
    boxes = [[rng.uniform(-40, 40), rng.uniform(-40, 40), -1.0, 4.0, 1.8, 1.5, rng.uniform(-3, 3)] for _ in range(40)]
    _planted_db(tmp_path, boxes, [['Car', 'Pedestrian'][k % 2] for k in range(40)], npts=30)
    cfg = _cfg(['Car:3', 'Pedestrian:2'], width=(0.2, 0.2, 0.0))
    scenes = []
    for s in range(350):
        n = 2048 if s == 7 else int(rng.integers(40, 2049))
        p = np.zeros((n, 4), np.float32)
        p[:, :2] = rng.uniform(-45, 45, (n, 2))
        p[:, 2] = rng.uniform(-2, 0, n)
        p[:, 3] = rng.random(n)
        scenes.append({'points': p, 'gt_boxes': np.zeros((0, 7), np.float32), 'gt_names': np.array([], '<U10'),
                       'gt_boxes_mask': np.ones(0, bool)})
    slots = 1 + (max(len(d['points']) for d in scenes) + 1023) // 1024                 # per scene, as the stage cuts them
    assert slots == 3 and len(scenes) * slots > 1024                                   # what the test is for
    first_behind = -(-1024 // slots)                                                   # first scene whose slots all lie in pass two
    copy = lambda: [{k: v.copy() for k, v in d.items()} for d in scenes]
    ref = R.RefSampler(tmp_path, cfg, ['Car', 'Pedestrian'])
    np.random.seed(4)
    exp = [ref(d)[0] for d in copy()]
    smp = DataBaseSampler(tmp_path, cfg, ['Car', 'Pedestrian'], device=DEV)
    np.random.seed(4)
    got = smp.sample_batch(copy()).split()
    for s in range(len(scenes)):
        _same(got[s], exp[s]["points"], exp[s]["gt_boxes"], exp[s]["gt_names"], s)
    behind = range(first_behind, len(scenes))
    assert any(len(got[s]["gt_names"]) > 0 for s in behind)                            # objects are pasted there
    assert any(len(got[s]["points"]) > 30 * len(got[s]["gt_names"]) for s in behind)   # and scene points are kept
