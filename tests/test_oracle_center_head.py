"""CPU-only: the NumPy restatement of the CenterHead geometry (tests/center_head_ref.py) against golden G12, the
reference's own `assign_targets` and `decode_bbox_from_heatmap` (tests/golden/capture_center_head_golden.py), and the
host-side checks of the product's Python surface.

Bit for bit: cells, radii, inds, masks, target_boxes_src, target_boxes[:, 0:3] and the velocity columns, the heat maps
(fp64 NumPy exp, as the reference), and of the decode the order, labels, scores, xs, ys and every gathered column.
Within 1 float32 ulp: the log / cos / sin columns and atan2.  That bound is derived, not tuned: torch's CPU routines
are the 1.0-ulp SLEEF ones, the restatement evaluates in fp64 and rounds, and a correctly rounded value and a value within
1 ulp of the truth are at most one float apart."""
import json
import os

import numpy as np
import pytest

from tests import center_head_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g12_center_head.npz")
CFGS = {"A": ref.CFG_A, "B": ref.CFG_B}


@pytest.fixture(scope="module")
def g12():
    return np.load(GOLDEN)


def meta_of(g12):
    return json.loads(bytes(g12["meta"]).decode())


def dense_heatmap(g12, name, h, shape):
    hm = np.zeros(int(np.prod(shape)), np.float32)
    hm[g12["%s_h%d_hm_idx" % (name, h)]] = g12["%s_h%d_hm_val" % (name, h)]
    return hm.reshape(shape)


def check_assign(got, g12, name, exact_heat=True):
    """`got`: a ret_dict of NumPy arrays per head (+ optional 'draws').  Returns (bit-equal heat cells, all heat cells)."""
    cfg = CFGS[name]
    H, W = cfg["map_hw"]
    B = g12[name + "_gt_boxes"].shape[0]
    same = cells = 0
    assert got["heatmap_masks"] == []
    for h, names in enumerate(cfg["heads"]):
        key = "%s_h%d_" % (name, h)
        tb, want_tb = got["target_boxes"][h], g12[key + "target_boxes"]
        assert np.array_equal(got["inds"][h], g12[key + "inds"]) and got["inds"][h].dtype == np.int64, (name, h)
        assert np.array_equal(got["masks"][h], g12[key + "masks"]) and got["masks"][h].dtype == np.int64, (name, h)
        assert got["target_boxes_src"][h].tobytes() == g12[key + "target_boxes_src"].tobytes(), (name, h)
        assert tb.shape == want_tb.shape and tb.dtype == np.float32
        assert tb[..., 0:3].tobytes() == want_tb[..., 0:3].tobytes(), (name, h)
        assert tb[..., 8:].tobytes() == want_tb[..., 8:].tobytes(), (name, h)
        assert ref.ulp_diff(tb[..., 3:8], want_tb[..., 3:8]).max() <= 1, (name, h)
        if "draws" in got:
            assert np.array_equal(got["draws"][h], g12[key + "draws"]), (name, h)
        want_hm = dense_heatmap(g12, name, h, (B, len(names), H, W))
        hm = got["heatmaps"][h]
        assert hm.shape == want_hm.shape and hm.dtype == np.float32
        assert np.array_equal(hm != 0, want_hm != 0), (name, h)
        if exact_heat:
            assert hm.tobytes() == want_hm.tobytes(), (name, h)
        else:
            assert ref.ulp_diff(hm, want_hm).max() <= 1, (name, h)
        same += int((hm.view(np.uint32) == want_hm.view(np.uint32)).sum())
        cells += hm.size
    return same, cells


def check_decode(got, g12, i, b):
    """`got`: one sample's dict of NumPy arrays."""
    key = "D%d_s%d_" % (i, b)
    want = g12[key + "pred_boxes"]
    assert got["pred_labels"].dtype == np.int32 and np.array_equal(got["pred_labels"], g12[key + "pred_labels"])
    assert got["pred_scores"].tobytes() == g12[key + "pred_scores"].tobytes()
    assert got["pred_boxes"].shape == want.shape and got["pred_boxes"].dtype == np.float32
    cols = [c for c in range(want.shape[1]) if c != 6]
    assert got["pred_boxes"][:, cols].tobytes() == want[:, cols].tobytes()
    assert ref.ulp_diff(got["pred_boxes"][:, 6], want[:, 6]).max() <= 1
    if key + "pred_iou" in g12.files:
        assert got["pred_iou"].tobytes() == g12[key + "pred_iou"].tobytes()
    else:
        assert "pred_iou" not in got


def decode_case_inputs(g12, i):
    case = meta_of(g12)["decode_cases"][i]
    H, W = ref.CFG_A["map_hw"]
    d = ref.decode_inputs(case["seed"], case["B"], case["n_cls"], H, W, case["vel"], case["iou"])
    sums = np.asarray([v.astype(np.float64).sum() for v in d.values() if v is not None])
    assert np.array_equal(sums, g12["D%d_input_sums" % i]), "decode_inputs no longer makes the arrays G12 was captured on"
    return case, d


@pytest.mark.parametrize("name", ["A", "B"])
def test_assign_restatement_matches_reference(g12, name):
    got = ref.assign_targets(g12[name + "_gt_boxes"], CFGS[name])
    same, cells = check_assign(got, g12, name, exact_heat=True)
    assert same == cells
    drawn = sum(len(g12["%s_h%d_draws" % (name, h)]) for h in range(len(CFGS[name]["heads"])))
    assert drawn > 20                                     # the golden is not empty


def test_golden_scenes_cover_the_stated_cases(g12):
    """Padding between real rows, a dx = 0 box that keeps its src row but no slot, footprints clipped at the border and
    at a corner, a head with exactly NUM_MAX_OBJS boxes."""
    gt = g12["A_gt_boxes"]
    cls = gt[1, :, -1]
    first, last = np.flatnonzero(cls)[[0, -1]]
    assert (cls[first:last] == 0).any() and not gt[0].any()
    src, masks = g12["A_h0_target_boxes_src"], g12["A_h0_masks"]
    zero_dx = (src[2, :, 3] == 0) & (src[2, :, -1] == 1)
    assert zero_dx.any() and not masks[2][zero_dx].any()
    H, W = ref.CFG_A["map_hw"]
    draws = np.concatenate([g12["A_h%d_draws" % h] for h in range(6)])
    d2 = draws[draws[:, 0] == 2]
    assert (d2[:, 1] == 0).any() and (d2[:, 1] == W - 1).any() and (d2[:, 2] == 0).any() and (d2[:, 2] == H - 1).any()
    assert ((d2[:, 1] == 0) & (d2[:, 2] == 0)).any() and ((d2[:, 1] == W - 1) & (d2[:, 2] == H - 1)).any()
    assert masks[4].sum() == ref.CFG_A["num_max_objs"] == masks.shape[1]
    assert g12["B_h0_masks"][4].sum() == ref.CFG_B["num_max_objs"]
    assert g12["B_gt_boxes"].shape[2] == 10


@pytest.mark.parametrize("name", ["A", "B"])
def test_overflow_raises_as_the_reference_does(g12, name):
    cfg = CFGS[name]
    assert meta_of(g12)[name + "_over_exception"] == "RuntimeError"
    over = g12[name + "_over_gt_boxes"]
    assert over.shape[1] == cfg["num_max_objs"] + 1
    with pytest.raises(RuntimeError):
        ref.assign_targets(over, cfg)
    ref.assign_targets(over[:, :cfg["num_max_objs"]], cfg)          # exactly NUM_MAX_OBJS: no error


@pytest.mark.parametrize("i", [0, 1, 2])
def test_decode_restatement_matches_reference(g12, i):
    case, d = decode_case_inputs(g12, i)
    got = ref.decode_bbox_from_heatmap(
        d["heatmap"], d["rot_cos"], d["rot_sin"], d["center"], d["center_z"], d["dim"], ref.CFG_A["point_cloud_range"],
        ref.CFG_A["voxel_size"], ref.CFG_A["stride"], vel=d["vel"], iou=d["iou"], K=case["K"],
        score_thresh=case["score_thresh"], post_center_limit_range=meta_of(g12)["decode_limit"])
    lim = meta_of(g12)["decode_limit"]
    for b, r in enumerate(got):
        r.pop("order")
        check_decode(r, g12, i, b)
        assert 0 < len(r["pred_scores"]) < case["K"]
    # the thresholds drop rows on each of the six range sides (and on score where one is set)
    full = ref.decode_bbox_from_heatmap(
        d["heatmap"], d["rot_cos"], d["rot_sin"], d["center"], d["center_z"], d["dim"], ref.CFG_A["point_cloud_range"],
        ref.CFG_A["voxel_size"], ref.CFG_A["stride"], K=case["K"], post_center_limit_range=[-1e9] * 3 + [1e9] * 3)
    bx = np.concatenate([r["pred_boxes"] for r in full])
    for c in range(3):
        assert (bx[:, c] < lim[c]).any() and (bx[:, c] > lim[3 + c]).any()
    if case["score_thresh"] is not None:
        assert (np.concatenate([r["pred_scores"] for r in full]) <= case["score_thresh"]).any()


def test_decode_tie_rule_of_the_restatement():
    """A constant map: the K rows are the first K flat indices; NaN ranks first."""
    H, W = 4, 5
    heat = np.full((1, 2, H, W), 0.1, np.float32)
    heat[0, 1, 2, 3] = np.nan
    z = np.zeros((1, 1, H, W), np.float32)
    r = ref.decode_bbox_from_heatmap(heat, z + 1, z, np.zeros((1, 2, H, W), np.float32), z, np.ones((1, 3, H, W), np.float32),
                                     [0, 0, 0], [1, 1, 1], 1, K=6, post_center_limit_range=[-1e9] * 3 + [1e9] * 3)[0]
    assert r["order"].tolist() == [H * W + 2 * W + 3, 0, 1, 2, 3, 4]


def test_gaussian_radius_of_the_product_matches(g12):
    import torch
    from dfu3d_amd.pcdet_kitti import centernet_utils
    rng = np.random.default_rng(5)
    h, w = rng.uniform(0.1, 40, 4096).astype(np.float32), rng.uniform(0.1, 40, 4096).astype(np.float32)
    # torch's CPU sqrt is the math library's vector routine on some builds: below 1 ulp, but not correctly rounded (seen:
    # sqrt(float32 1036.2222) one float below the IEEE result); everything else in the formula is IEEE add / mul / div.
    # A root (b + sq) / 2 then moves by at most (ulp(sq) + ulp(b + sq)) / 2, and with sq <= |b| <= b2 = 2 (h + w) for
    # every root that is at most (1 + 2) / 2 = 1.5 steps of b2's binade; r3 cancels, so no bound in steps of r3 holds.
    for o in (0.1, 0.5, 0.7):
        got = centernet_utils.gaussian_radius(torch.from_numpy(h), torch.from_numpy(w), min_overlap=o).numpy()
        want = ref.gaussian_radius(h, w, o)
        assert (np.abs(got.astype(np.float64) - want) <= 1.5 * np.spacing(np.float32(2) * (h + w))).all()
        assert (got.view(np.uint32) == want.view(np.uint32)).mean() > 0.9


def test_product_host_side_checks():
    """circle_nms, K beyond the scores of a sample and K beyond the kernel's cap raise before anything is launched."""
    import torch
    from dfu3d_amd import stages
    from dfu3d_amd._lib import Dfu3dError
    from dfu3d_amd.pcdet_kitti import centernet_utils
    assert stages.CENTER_MAX_K >= 1024
    z = torch.zeros(1, 1, 40, 40)
    args = dict(rot_cos=z, rot_sin=z, center=torch.zeros(1, 2, 40, 40), center_z=z, dim=torch.zeros(1, 3, 40, 40),
                point_cloud_range=[0, 0, 0], voxel_size=[1, 1, 1], feature_map_stride=1,
                post_center_limit_range=[-1, -1, -1, 1, 1, 1])
    with pytest.raises(NotImplementedError):
        centernet_utils.decode_bbox_from_heatmap(z, circle_nms=True, K=10, **args)
    with pytest.raises(RuntimeError):
        centernet_utils.decode_bbox_from_heatmap(torch.zeros(1, 1, 2, 2), K=5, **args)
    with pytest.raises(Dfu3dError):
        centernet_utils.decode_bbox_from_heatmap(z, K=stages.CENTER_MAX_K + 1, **args)


def test_c_abi_rejects_bad_sizes_without_gpu():
    """dfu3d_center_decode: K above the cap is DFU3D_ERANGE, K above the scores of a sample DFU3D_EINVAL (host checks)."""
    import ctypes
    from dfu3d_amd import _lib
    L = _lib.lib()
    p = ctypes.c_void_p(256)                              # never dereferenced: the host checks return first
    dec = lambda n_cls, H, W, K: L.dfu3d_center_decode(p, p, p, p, p, p, None, None, 1, n_cls, H, W, K, 0.0, 0.0, 0.2, 0.2,  # noqa: E731
                                                       4, p, 0, 0.0, p, p, p, None, p, None)
    assert dec(2, 128, 64, 1025) == -3
    assert dec(1, 4, 4, 17) == -1
    assert L.dfu3d_center_assign(None, 1, 1, 7, p, 1, p, 1, 8, 8, 0.0, 0.0, 0.2, 0.2, 4, 500, 0.1, 2, p, p, p, p, p, p,
                                 None) == -1
