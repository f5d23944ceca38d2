"""The point-sampling stage without a GPU: the agreement of csrc/dfu3d_smp.h with its binding, host-side argument
validation before any launch, the rule's restatement (tests/sample_points_ref.py) against the reference's recorded
outputs (golden G22) and against the statistics of a uniform draw, and the `sample_points` entry of DataProcessor."""
import ctypes
import glob
import importlib
import os

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_smp
from tests import sample_points_ref as S

SYMBOLS = ['dfu3d_sample_points', 'dfu3d_smp_scratch_bytes', 'dfu3d_smp_version']
POINTERS = ('points', 'point_cnt', 'sel', 'ord', 'rep', 'scratch', 'out', 'status')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_sample_points.npz")
RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
MASK = {'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}


def test_header_and_binding_agree():
    assert _lib_smp.HEADER == os.path.join(_build.CSRC, "dfu3d_smp.h") and _lib_smp.HEADER in _build._deps()
    assert "dfu3d_smp.h" not in os.listdir(_build.INCLUDE)
    assert _lib_smp.header_symbols() == SYMBOLS
    L = _lib_smp.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.dfu3d_smp_version() == _lib_smp.header_version() == 1
    K = _lib_smp.CONSTANTS
    assert all(k.startswith("DFU3D_SMP_") for k in K)
    assert K == {'DFU3D_SMP_VERSION': 1, 'DFU3D_SMP_LAUNCHES': 3, 'DFU3D_SMP_MAX_OUT': 16384, 'DFU3D_SMP_MAX_BATCH': 65535,
                 'DFU3D_SMP_MAX_ELEMS': 2 ** 31 - 1, 'DFU3D_SMP_EMPTY_SCENE': 1, 'DFU3D_SMP_BAD_COUNT': 2,
                 'DFU3D_SMP_SCENE_THREADS': 1024, 'DFU3D_SMP_GATHER_THREADS': 256}
    assert 1 <= K['DFU3D_SMP_LAUNCHES'] <= 3 and K['DFU3D_SMP_MAX_OUT'] >= 16384
    res, args = _lib_smp.SIGNATURES['dfu3d_sample_points']
    assert res is ctypes.c_int32 and len(args) == 15 and args[-1] is ctypes.c_void_p
    assert args[2:7] == [ctypes.c_int32] * 5 and args[11] is ctypes.c_size_t and ctypes.c_float not in args
    assert _lib_smp.SIGNATURES['dfu3d_smp_scratch_bytes'] == (ctypes.c_size_t, [ctypes.c_int32] * 3)
    assert _lib_smp.SIGNATURES['dfu3d_smp_version'] == (ctypes.c_int32, [])
    others = [os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_lib*.py"))]
    assert "_lib_smp" in others and "_lib_prop" in others and "_lib" in others
    for name in others:
        if name != "_lib_smp":
            mod = importlib.import_module("dfu3d_amd." + name)
            assert not set(_lib_smp.SIGNATURES) & set(mod.SIGNATURES), name
            assert not set(K) & set(mod.CONSTANTS), name
    own = open(_lib_smp.HEADER).read()
    for prefix in ('dfu3d_vfe', 'dfu3d_head', 'dfu3d_post', 'dfu3d_aug', 'dfu3d_bev', 'dfu3d_opt', 'dfu3d_ingest',
                   'dfu3d_pn2', 'dfu3d_roi', 'dfu3d_tgt', 'dfu3d_prop'):
        assert prefix not in own and prefix.upper() not in own, prefix
    from dfu3d_amd import point_sample_ops as ops
    assert (ops.LAUNCHES, ops.MAX_OUT) == (3, 16384) and ops.status_message(0) == "ok"
    assert "without points" in ops.status_message(1) and "point_cnt" in ops.status_message(3)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
    Fake.dfu3d_smp_version = object()
    with pytest.raises(_lib.Dfu3dError, match="fake.so does not export dfu3d_sample_points, dfu3d_smp_scratch_bytes"):
        _lib_smp.bind(Fake())


def _call(L, B=2, R=500, C=4, K=64, oc=4, nbytes=None, **ptr):
    p = {name: ctypes.c_void_p(16 * (k + 1)) for k, name in enumerate(POINTERS)}      # addresses no call may touch
    p.update(ptr)
    if nbytes is None:
        nbytes = L.dfu3d_smp_scratch_bytes(B, R, K) or 16
    return L.dfu3d_sample_points(p['points'], p['point_cnt'], B, R, C, K, oc, p['sel'], p['ord'], p['rep'], p['scratch'],
                                 nbytes, p['out'], p['status'], None)


def test_bad_arguments_return_before_any_launch():
    """Every call below passes pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_smp.lib()
    OK, EINVAL, ERANGE = (_lib.CONSTANTS[k] for k in ("DFU3D_OK", "DFU3D_EINVAL", "DFU3D_ERANGE"))
    K = _lib_smp.CONSTANTS
    for name in POINTERS:
        assert _call(L, **{name: None}) == EINVAL, name
    assert _call(L, B=-1) == EINVAL and _call(L, R=-1) == EINVAL
    assert _call(L, K=0) == EINVAL and _call(L, K=-4) == EINVAL
    assert _call(L, C=2, oc=2) == EINVAL and _call(L, C=0, oc=0) == EINVAL and _call(L, C=-1) == EINVAL
    assert _call(L, oc=2) == EINVAL and _call(L, oc=5) == EINVAL and _call(L, C=6, oc=7) == EINVAL and _call(L, oc=-1) == EINVAL
    assert _call(L, scratch=ctypes.c_void_p(24)) == EINVAL                        # not on 16 bytes
    need = L.dfu3d_smp_scratch_bytes(2, 500, 64)
    assert need > 0 and _call(L, nbytes=need - 1) == EINVAL and _call(L, nbytes=0) == EINVAL
    # nothing to do: no launch, and the scratch is not looked at
    assert _call(L, B=0) == OK and _call(L, B=0, R=0, nbytes=0) == OK and _call(L, B=0, R=0, points=None, sel=None) == OK
    assert _call(L, K=K['DFU3D_SMP_MAX_OUT'] + 1, nbytes=1 << 30) == ERANGE
    assert _call(L, B=K['DFU3D_SMP_MAX_BATCH'] + 1, K=1, nbytes=1 << 30) == ERANGE
    assert _call(L, R=2 ** 31 - 1, nbytes=1 << 40) == ERANGE                      # R * (1 + C)
    assert _call(L, R=2 ** 29, C=3, oc=3, nbytes=1 << 40) == ERANGE
    assert _call(L, B=65535, K=16384, nbytes=1 << 40) == ERANGE                   # B * K * (1 + out_cols)
    assert _call(L, B=32768, K=16384, C=3, oc=3, nbytes=1 << 40) == ERANGE
    # an out-of-range size wins over what is empty, an invalid one over both
    assert _call(L, B=0, K=K['DFU3D_SMP_MAX_OUT'] + 1) == ERANGE and _call(L, B=0, oc=2) == EINVAL


def test_scratch_bytes():
    L = _lib_smp.lib()
    K = _lib_smp.CONSTANTS
    for bad in ((-1, 64, 50), (2, -1, 50), (2, 64, 0), (2, 64, -3), (2, 64, K['DFU3D_SMP_MAX_OUT'] + 1),
                (K['DFU3D_SMP_MAX_BATCH'] + 1, 64, 50)):
        assert L.dfu3d_smp_scratch_bytes(*bad) == 0, bad
    sizes = [L.dfu3d_smp_scratch_bytes(B, 3000, 200) for B in range(0, 12)]
    assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] == 0 and all(s % 16 == 0 for s in sizes)
    # a byte per row rounded up to 16, six planes of K words and two words per scene, rounded up to 16 and no more
    assert [sizes[B] for B in (1, 4, 5)] == [3008 + -(-B * (200 * 24 + 8) // 16) * 16 for B in (1, 4, 5)]
    by_rows = [L.dfu3d_smp_scratch_bytes(3, R, 200) for R in (0, 1, 16, 17, 100000, 2 ** 31 - 1)]
    by_k = [L.dfu3d_smp_scratch_bytes(3, 1000, k) for k in (1, 2, 300, 16384)]
    assert all(a <= b for a, b in zip(by_rows, by_rows[1:])) and by_rows[0] < by_rows[2] < by_rows[3] < by_rows[-1]
    assert all(a < b for a, b in zip(by_k, by_k[1:]))
    big = L.dfu3d_smp_scratch_bytes(K['DFU3D_SMP_MAX_BATCH'], 2 ** 31 - 1, K['DFU3D_SMP_MAX_OUT'])
    assert big >= 65535 * 16384 * 24 + 2 ** 31 - 1                                # no 32-bit wrap-around


def golden():
    g = np.load(GOLDEN)
    return [(g["points_%d" % s], int(g["k_%d" % s]), g["rows_%d" % s]) for s in range(int(g["n_scenes"]))]


def words(rng, n, K):
    return tuple(rng.integers(0, 2 ** 32, s, dtype=np.uint64).astype(np.uint32) for s in (n, K, K))


def test_the_reference_outputs_keep_the_contract():
    scenes = golden()
    assert [(len(p), k) for p, k, _ in scenes] == [(96, 40), (96, 4), (96, 40), (96, 40), (40, 40), (30, 40), (20, 40), (7, 40)]
    for pts, K, rows in scenes:
        assert rows.shape == (4, K) and len({r.tobytes() for r in rows}) == 4          # four seeds, four different draws
        for r in rows:
            S.check_contract(pts[:, 0:3], r, K)
    # the contract notices what it is there for
    pts, K, rows = scenes[0]
    far = np.flatnonzero(~S.near_flags(pts[:, 0:3]))
    near = np.flatnonzero(S.near_flags(pts[:, 0:3]))
    bad = rows[0].copy()
    bad[np.flatnonzero(bad == far[0])[0]] = [i for i in near if i not in set(bad.tolist())][0]
    with pytest.raises(AssertionError, match="far row"):
        S.check_contract(pts[:, 0:3], bad, K)
    bad = rows[0].copy()
    bad[0] = bad[1]
    with pytest.raises(AssertionError, match="twice"):
        S.check_contract(pts[:, 0:3], bad, K)
    with pytest.raises(AssertionError):
        S.check_contract(scenes[5][0][:, 0:3], np.zeros(40, np.int64), 40)


def test_the_restatement_keeps_the_contract_on_the_same_scenes():
    rng = np.random.default_rng(1)
    for pts, K, _ in golden():
        for _ in range(4):
            sel, order, rep = words(rng, len(pts), K)
            rows = S.sample_rows(pts[:, 0:3], K, sel, order, rep)
            S.check_contract(pts[:, 0:3], rows, K)
            L = S.chosen_list(pts[:, 0:3], K, sel, rep)
            assert sorted(rows.tolist()) == sorted(L) and rows.tolist() == [L[j] for j in np.argsort(order, kind="stable")]


def test_the_near_flags_are_the_reference_s():
    """Where a scene has fewer than K far rows the reference keeps every far row in every draw and only some near ones:
    its outputs hold exactly the restatement's far rows in all four seeds, and every near row is missing in one of them.
    The depth boundary is among them: depth exactly 40 is far, the float32 neighbours below are near."""
    seen = 0
    for pts, K, rows in golden():
        near = S.near_flags(pts[:, 0:3])
        if len(pts) <= K or (~near).sum() >= K:
            continue
        always = np.array([all((r == i).any() for r in rows) for i in range(len(pts))])
        assert np.array_equal(always, ~near)
        seen += 1
    assert seen == 2
    pts = golden()[0][0]
    xyz = pts[:, 0:3]

    def flag_of(x, y):
        at = np.flatnonzero((xyz[:, 0] == np.float32(x)) & (xyz[:, 1] == np.float32(y)) & (xyz[:, 2] == 0))
        assert len(at) == 1
        return bool(S.near_flags(xyz)[at[0]])
    below = lambda v: np.nextafter(np.float32(v), np.float32(-np.inf))      # noqa: E731
    assert not flag_of(40.0, 0.0) and not flag_of(24.0, 32.0)
    assert flag_of(below(40.0), 0.0) and flag_of(24.0, below(below(below(32.0))))
    assert not S.near_flags(np.array([[np.nan, 0, 0], [0, np.inf, 0], [3e38, 0, 0]], np.float32)).any()


def test_frequencies_of_the_restatement():
    """4 096 seeded scenes, n = 64 near rows, K = 16: every row's inclusion frequency within 5 binomial standard deviations
    of K / n, its mean output slot within 5 standard deviations of (K - 1) / 2.  (Fixed seed: deterministic.)"""
    n, K, B = 64, 16, 4096
    rng = np.random.default_rng(4096)
    xyz = rng.uniform(-20, 20, (n, 3)).astype(np.float32)
    assert S.near_flags(xyz).all()
    rows = np.stack([S.sample_rows(xyz, K, *words(rng, n, K)) for _ in range(B)])
    S.check_frequencies(rows, n)
    # the check notices a bias of a few percent of a row, and a slot that prefers a row
    biased = rows.copy()
    biased[:400, 0] = 3
    with pytest.raises(AssertionError, match="inclusion"):
        S.check_frequencies(biased, n)
    sorted_rows = np.sort(rows, axis=1)
    with pytest.raises(AssertionError, match="slot"):
        S.check_frequencies(sorted_rows, n)


def test_every_branch_of_the_restatement_on_hand_written_words():
    xyz = np.zeros((5, 3), np.float32)
    xyz[:, 0] = [1, 50, 2, 60, 3]                                                  # rows 1 and 3 are far
    sel = np.array([7, 0, 7, 0, 1], np.uint32)
    rep = np.array([0, 2 ** 32 - 1, 2 ** 31, 1, 0, 0, 0, 0, 0, 0, 0, 0], np.uint32)
    assert S.chosen_list(xyz, 3, sel, rep) == [1, 3, 4]                            # F = 2 < K: both far rows, the smallest near one
    assert S.chosen_list(xyz, 4, sel, rep) == [0, 1, 3, 4]                         # ... then the tie at 7 goes to the lower row
    assert S.chosen_list(xyz, 2, sel, rep) == [1, 3]                               # F >= K: the smallest of ALL rows (here the far ones)
    assert S.chosen_list(xyz, 1, sel, rep) == [1]
    assert S.chosen_list(xyz, 5, sel, rep) == [0, 1, 2, 3, 4]
    assert S.chosen_list(xyz, 7, sel, rep) == [0, 1, 2, 3, 4, 1, 3]
    assert S.chosen_list(xyz, 10, sel, rep) == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4]      # K = 2n: no replacement yet
    assert S.chosen_list(xyz, 11, sel, rep) == [0, 1, 2, 3, 4, 0, 4, 2, 0, 0, 0]   # multiply-shift of rep
    assert S.chosen_list(xyz[:0], 3, sel[:0], rep) == []
    assert S.shuffle_slots(np.array([5, 0, 5, 2 ** 32 - 1, 0], np.uint32)).tolist() == [1, 4, 0, 2, 3]
    out, status, rows = S.sample_points_ref(np.concatenate([np.zeros((5, 1), np.float32), xyz], 1), [5, 0], 3, 3, sel,
                                            np.zeros((2, 3), np.uint32), np.zeros((2, 3), np.uint32))
    assert status == 1 and rows.tolist() == [[1, 3, 4], [-1, -1, -1]] and out[:, 0].tolist() == [0, 0, 0, 1, 1, 1]
    assert out[:3, 1].tolist() == [50, 60, 3] and not out[3:, 1:].any()


def test_data_processor_entry():
    from dfu3d_amd.pcdet_kitti import data_processor as DP
    assert 'sample_points' in DP.SUPPORTED
    with pytest.raises(NotImplementedError, match="NUM_POINTS is required"):
        DP.DataProcessor([MASK, {'NAME': 'sample_points'}], RANGE, True, 4)
    with pytest.raises(NotImplementedError, match="NUM_POINTS is required"):
        DP.DataProcessor([{'NAME': 'sample_points'}], RANGE, True, 4)
    entry = {'NAME': 'sample_points', 'NUM_POINTS': {'train': 16384, 'test': -1}}
    with pytest.raises(NotImplementedError, match="must come after mask_points_and_boxes_outside_range"):
        DP.DataProcessor([entry, MASK], RANGE, True, 4)
    with pytest.raises(NotImplementedError, match="must come after"):
        DP.DataProcessor([entry], RANGE, True, 4)
    with pytest.raises(_lib.Dfu3dError, match="NUM_POINTS 16385"):
        DP.DataProcessor([MASK, dict(entry, NUM_POINTS={'train': 16385, 'test': 1})], RANGE, True, 4)
    shuffle = {'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': {'train': True, 'test': False}}
    train = DP.DataProcessor([MASK, entry, shuffle], RANGE, True, 3)
    test = DP.DataProcessor([MASK, entry, shuffle], RANGE, False, 3)
    assert train.sample_count() == 16384 and test.sample_count() is None
    assert DP.DataProcessor([MASK], RANGE, True, 4).sample_count() is None
    # -1 is the identity (and touches no device)
    d = {'points': np.arange(12, dtype=np.float32).reshape(3, 4)}
    same = test.data_processor_queue[1](data_dict=d)
    assert same is d and same['points'].tolist() == np.arange(12).reshape(3, 4).tolist()


def test_kitti_dataset_feature_list(tmp_path):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    src = ['x', 'y', 'z', 'intensity']
    entry = {'NAME': 'sample_points', 'NUM_POINTS': {'train': 512, 'test': -1}}

    def ds(used, entries, training=True, src=src):
        cfg = {'DATA_SPLIT': {'train': 'train', 'test': 'val'}, 'INFO_PATH': {'train': [], 'test': []},
               'FOV_POINTS_ONLY': True, 'POINT_CLOUD_RANGE': RANGE, 'DATA_PROCESSOR': entries,
               'POINT_FEATURE_ENCODING': {'encoding_type': 'absolute_coordinates_encoding', 'used_feature_list': used,
                                          'src_feature_list': src}}
        return KittiDataset(cfg, ['Car'], training=training, root_path=tmp_path)
    assert ds(src, [MASK]).point_feature_encoder.num_point_features == 4
    assert ds(src, [MASK, entry]).point_feature_encoder.num_point_features == 4
    sampled = ds(src[:3], [MASK, entry])
    assert sampled.point_feature_encoder.num_point_features == 3
    assert sampled.data_processor.num_point_features == 3 and sampled.data_processor.sample_count() == 512
    for used, entries, training in ((src[:3], [MASK], True), (src[:3], [MASK, entry], False), (src[:2], [MASK, entry], True),
                                    (['x', 'z', 'y'], [MASK, entry], True), (['y', 'z', 'intensity'], [MASK, entry], True)):
        with pytest.raises(NotImplementedError, match="POINT_FEATURE_ENCODING"):
            ds(used, entries, training).point_feature_encoder
    with pytest.raises(NotImplementedError, match="POINT_FEATURE_ENCODING"):
        ds(src[:3], [MASK, entry], src=src + ['t']).point_feature_encoder
