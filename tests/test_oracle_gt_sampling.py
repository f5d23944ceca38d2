"""CPU: the NumPy restatement of ground-truth sampling (tests/gt_sampling_ref.py) against G11, the reference's own
DataBaseSampler (tests/golden/capture_gt_sampling_golden.py); the product's host-side candidate draw against G11's
recorded candidate ids and final RNG state; the options the product does not support raise."""
import os

import numpy as np
import pytest

from tests import gt_sampling_ref as R

G11 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g11_gt_sampling.npz")


@pytest.fixture(scope="module")
def g11():
    return np.load(G11)


@pytest.fixture()
def db(g11, tmp_path):
    R.database_from_golden(g11, tmp_path)
    return tmp_path


def _drawn(g11, ci, s):
    pre = "out/%d/%d/" % (ci, s)
    cls, ids, ln = g11[pre + "drawn_classes"], g11[pre + "drawn_ids"], g11[pre + "drawn_len"]
    out, k = [], 0
    for c, n in zip(cls, ln):
        out.append((str(c), ids[k:k + n].tolist()))
        k += n
    return out


def _scene(g11, ci, s):
    d = R.golden_scene(g11, s)
    d["gt_boxes"] = d["gt_boxes"].astype(np.float64 if ci == 1 else np.float32)
    return d


@pytest.mark.parametrize("ci", [0, 1])
def test_restatement_equals_reference(g11, db, ci):
    cfg = R.golden_cfg(g11, ci)
    ref = R.RefSampler(db, cfg, [str(c) for c in g11["class_names"]])
    np.random.seed([11, 12][ci])
    accepted_any = rejected_any = 0
    for s in range(int(g11["n_scenes"])):
        d = _scene(g11, ci, s)
        out, drawn = ref(d)
        pre = "out/%d/%d/" % (ci, s)
        assert [(c, ids.tolist()) for c, ids in drawn] == _drawn(g11, ci, s), s
        assert out["points"].dtype == g11[pre + "points"].dtype
        assert np.array_equal(out["points"].view(np.uint32), g11[pre + "points"].view(np.uint32)), s
        assert out["gt_boxes"].dtype == g11[pre + "gt_boxes"].dtype and np.array_equal(out["gt_boxes"],
                                                                                         g11[pre + "gt_boxes"]), s
        assert np.array_equal(out["gt_names"], g11[pre + "gt_names"]), s
        n_new = len(out["gt_names"]) - int(d["gt_boxes_mask"].sum())
        accepted_any += len(out["gt_names"]) != len(d["gt_names"])
        rejected_any += sum(len(i) for _, i in drawn) > max(n_new, 0)
    assert accepted_any and rejected_any
    st = np.random.get_state()
    assert np.array_equal(st[1], g11["rng/%d/keys" % ci]) and st[2] == int(g11["rng/%d/pos" % ci])


@pytest.mark.parametrize("ci", [0, 1])
def test_product_candidate_draw_equals_reference(g11, db, ci):
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    sampler = DataBaseSampler(db, R.golden_cfg(g11, ci), [str(c) for c in g11["class_names"]], device="cpu")
    np.random.seed([11, 12][ci])
    wrapped = 0
    for s in range(int(g11["n_scenes"])):
        sel = sampler.select(R.golden_scene(g11, s)["gt_names"])
        got = [(c, ids.tolist()) for _, c, ids in sel]
        assert got == _drawn(g11, ci, s), s
        wrapped += any(len(ids) < int(sampler.sample_class_num[c]) for _, c, ids in sel) and ci == 1
    st = np.random.get_state()
    assert np.array_equal(st[1], g11["rng/%d/keys" % ci]) and st[2] == int(g11["rng/%d/pos" % ci])
    if ci == 1:
        assert wrapped                                   # a short slice before the pointer wrapped


def test_golden_covers_the_cases(g11):
    n = int(g11["n_scenes"])
    sizes = [len(g11["scene/%d/gt_names" % s]) for s in range(n)]
    assert 0 in sizes                                     # a scene with no boxes
    assert any(len(g11["scene/%d/points" % s]) == 0 for s in range(n))
    # the scene whose one huge box makes every candidate collide: drawn, nothing accepted
    s8 = [s for s in range(n) if sizes[s] == 1 and g11["scene/%d/gt_boxes" % s][0, 3] > 100][0]
    for ci in (0, 1):
        assert len(g11["out/%d/%d/drawn_ids" % (ci, s8)]) > 0
        assert np.array_equal(g11["out/%d/%d/gt_names" % (ci, s8)], g11["scene/%d/gt_names" % s8])
    assert R.golden_cfg(g11, 0)["LIMIT_WHOLE_SCENE"] and any(R.golden_cfg(g11, 1)["REMOVE_EXTRA_WIDTH"])
    assert g11["out/1/0/gt_boxes"].dtype == np.float64


def _cfg(g11, **kw):
    c = R.golden_cfg(g11, 0)
    c.update(kw)
    return c


@pytest.mark.parametrize("key,val", [("USE_ROAD_PLANE", True), ("IMG_AUG_TYPE", "kitti"),
                                     ("FILTER_OBJ_POINTS_BY_TIMESTAMP", True), ("DATABASE_WITH_FAKELIDAR", True)])
def test_unsupported_options_raise(g11, db, key, val):
    from dfu3d_amd._lib import Dfu3dError
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    with pytest.raises(Dfu3dError, match=key):
        DataBaseSampler(db, _cfg(g11, **{key: val}), ["Car"], device="cpu")


def test_use_shared_memory_is_accepted(g11, db):
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    DataBaseSampler(db, _cfg(g11, USE_SHARED_MEMORY=True), ["Car"], device="cpu")


def test_bad_inputs_raise(g11, db):
    from dfu3d_amd._lib import Dfu3dError
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    names = [str(c) for c in g11["class_names"]]
    with pytest.raises(Dfu3dError, match="NUM_POINT_FEATURES"):
        DataBaseSampler(db, _cfg(g11, NUM_POINT_FEATURES=5), names, device="cpu")      # the .bin sizes disagree
    smp = DataBaseSampler(db, _cfg(g11), names, device="cpu")
    d = R.golden_scene(g11, 0)
    state = np.random.get_state()
    with pytest.raises(Dfu3dError, match="NUM_POINT_FEATURES"):
        smp._prepare(dict(d, points=np.zeros((5, 5), np.float32)))
    with pytest.raises(Dfu3dError, match=r"\(N, 7\)"):
        smp._prepare(dict(d, gt_boxes=np.zeros((len(d["gt_names"]), 9), np.float32)))
    with pytest.raises(Dfu3dError, match="float32"):
        smp._prepare(dict(d, points=d["points"].astype(np.float64)))
    assert np.array_equal(np.random.get_state()[1], state[1])           # rejected before any draw
    # a .bin file of the wrong size
    info = smp.db_infos["Car"][0]
    with open(os.path.join(str(db), info["path"]), "ab") as f:
        f.write(b"\0" * 4)
    with pytest.raises(Dfu3dError, match="bytes"):
        DataBaseSampler(db, _cfg(g11), names, device="cpu")


def test_empty_database_for_a_sampled_class_raises(g11, db):
    from dfu3d_amd._lib import Dfu3dError
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    cfg = _cfg(g11, PREPARE={"filter_by_min_points": ["Cyclist:100000"]})
    smp = DataBaseSampler(db, cfg, ["Car", "Cyclist"], device="cpu")
    with pytest.raises(Dfu3dError, match="no Cyclist"):
        smp.select(np.array(["Car"]))
