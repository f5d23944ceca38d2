"""The anchor target stage and the SECOND detector without a GPU: the agreement of csrc/dfu3d_anc.h with its binding,
host-side argument validation before any launch, the restatement (tests/anchor_target_ref.py) and AnchorGenerator against
the reference's recorded run (golden G25) bit for bit, the cases of the GPU tests checked with the restatement, the
restatement's class sets on a flat block against its per-class form and against golden G27 (the reference's assigner at
uneven sets), the assigner's kept flat block after its source tensors changed, the head's
losses and decoding on the golden's predictions and targets (plain torch: they run on the CPU as well), SECONDNet's
state-dict keys, and the settings that raise."""
import ctypes
import glob
import importlib
import json
import os

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_anc
from tests import anchor_target_ref as R
from tests.centerpoint_cases import cfg

SYMBOLS = ['dfu3d_anc_scratch_bytes', 'dfu3d_anc_version', 'dfu3d_anchor_targets']
POINTERS = ('anchors', 'set_begin', 'matched', 'unmatched', 'class_id', 'gt_boxes', 'scratch', 'box_cls_labels',
            'box_reg_targets', 'reg_weights')
HOST = ('set_begin', 'matched', 'unmatched', 'class_id')        # read on the host during the call
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "g25_anchor_head.npz")
G27 = os.path.join(HERE, "golden", "g27_anchor_assigner.npz")
G24 = os.path.join(HERE, "golden", "g24_spconv_backbone_keys.json")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return g, json.loads(bytes(g['meta']).decode())


# ---- header, binding, validation ---------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    assert _lib_anc.HEADER == os.path.join(_build.CSRC, "dfu3d_anc.h") and _lib_anc.HEADER in _build._deps()
    assert "dfu3d_anc.h" not in os.listdir(_build.INCLUDE)
    assert _lib_anc.header_symbols() == SYMBOLS
    L = _lib_anc.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.dfu3d_anc_version() == _lib_anc.header_version() == 1
    K = _lib_anc.CONSTANTS
    assert all(k.startswith("DFU3D_ANC_") for k in K)
    assert K == {'DFU3D_ANC_VERSION': 1, 'DFU3D_ANC_LAUNCHES': 3, 'DFU3D_ANC_MAX_SETS': 8, 'DFU3D_ANC_MAX_BOXES': 512,
                 'DFU3D_ANC_MAX_BATCH': 65535, 'DFU3D_ANC_MAX_ELEMS': 2 ** 31 - 1, 'DFU3D_ANC_THREADS': 256}
    res, args = _lib_anc.SIGNATURES['dfu3d_anchor_targets']
    assert res is ctypes.c_int32 and len(args) == 17 and args[-1] is ctypes.c_void_p
    assert args[1:3] == [ctypes.c_int32] * 2 and args[7] is ctypes.c_int32 and args[9:11] == [ctypes.c_int32] * 2
    assert args[12] is ctypes.c_size_t and ctypes.c_float not in args and args.count(ctypes.c_void_p) == 11
    assert _lib_anc.SIGNATURES['dfu3d_anc_scratch_bytes'] == (ctypes.c_size_t, [ctypes.c_int32] * 3)
    assert _lib_anc.SIGNATURES['dfu3d_anc_version'] == (ctypes.c_int32, [])
    others = [os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_lib*.py"))]
    assert "_lib_anc" in others and "_lib_prop" in others and "_lib" in others
    for name in others:
        if name != "_lib_anc":
            mod = importlib.import_module("dfu3d_amd." + name)
            assert not set(_lib_anc.SIGNATURES) & set(mod.SIGNATURES), name
            assert not set(K) & set(mod.CONSTANTS), name
    own = open(_lib_anc.HEADER).read()
    for prefix in ('dfu3d_vox', 'dfu3d_vfe', 'dfu3d_head', 'dfu3d_post', 'dfu3d_aug', 'dfu3d_bev', 'dfu3d_opt', 'dfu3d_ingest',
                   'dfu3d_pn2', 'dfu3d_roi', 'dfu3d_tgt', 'dfu3d_prop', 'dfu3d_smp', 'dfu3d_hvox', 'dfu3d_spc'):
        assert prefix not in own and prefix.upper() not in own, prefix
    from dfu3d_amd import anchor_target_ops as ops
    assert (ops.LAUNCHES, ops.MAX_SETS, ops.MAX_BOXES) == (3, 8, 512)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
    Fake.dfu3d_anc_version = object()
    with pytest.raises(_lib.Dfu3dError, match="fake.so does not export dfu3d_anc_scratch_bytes, dfu3d_anchor_targets"):
        _lib_anc.bind(Fake())


def _call(L, A=600, per_loc=6, begin=(0, 2, 4, 6), hi=(0.6, 0.5, 0.5), lo=(0.45, 0.35, 0.35), ids=(1, 2, 3),
          S=None, B=2, M=9, nbytes=None, **ptr):
    p = {name: ctypes.c_void_p(16 * (k + 1)) for k, name in enumerate(POINTERS)}      # addresses no call may touch
    keep = ((ctypes.c_int32 * len(begin))(*begin), (ctypes.c_float * len(hi))(*hi),
            (ctypes.c_float * len(lo))(*lo), (ctypes.c_int32 * len(ids))(*ids))
    p.update({name: ctypes.cast(a, ctypes.c_void_p) for name, a in zip(HOST, keep)})
    p.update(ptr)
    if nbytes is None:
        nbytes = L.dfu3d_anc_scratch_bytes(B, A, M) or 16
    return L.dfu3d_anchor_targets(p['anchors'], A, per_loc, p['set_begin'], p['matched'], p['unmatched'], p['class_id'],
                                  len(ids) if S is None else S, p['gt_boxes'], B, M, p['scratch'], nbytes,
                                  p['box_cls_labels'], p['box_reg_targets'], p['reg_weights'], None)


def test_bad_arguments_return_before_any_launch():
    """Every call below passes device pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_anc.lib()
    OK, EINVAL, ERANGE = (_lib.CONSTANTS[k] for k in ("DFU3D_OK", "DFU3D_EINVAL", "DFU3D_ERANGE"))
    K = _lib_anc.CONSTANTS
    for name in POINTERS:
        assert _call(L, **{name: None}) == EINVAL, name
    assert _call(L, A=-6) == EINVAL and _call(L, B=-1) == EINVAL and _call(L, M=-1) == EINVAL
    assert _call(L, S=0) == EINVAL and _call(L, S=-2) == EINVAL and _call(L, per_loc=0) == EINVAL
    assert _call(L, A=601) == EINVAL                                               # no multiple of per_loc
    assert _call(L, begin=(1, 2, 4, 6)) == EINVAL and _call(L, begin=(0, 2, 4, 5)) == EINVAL
    assert _call(L, begin=(0, 2, 2, 6)) == EINVAL and _call(L, begin=(0, 4, 2, 6)) == EINVAL
    for bad in (float('nan'), float('inf'), float('-inf')):
        assert _call(L, hi=(0.6, bad, 0.5)) == EINVAL and _call(L, lo=(bad, 0.35, 0.35)) == EINVAL
    assert _call(L, hi=(0.6, 0.3, 0.5)) == EINVAL                             # unmatched above matched
    assert _call(L, ids=(1, 0, 3)) == EINVAL and _call(L, ids=(1, 2, 1)) == EINVAL and _call(L, ids=(1, -2, 3)) == EINVAL
    assert _call(L, scratch=ctypes.c_void_p(24)) == EINVAL                         # not on 16 bytes
    need = L.dfu3d_anc_scratch_bytes(2, 600, 9)
    assert need > 0 and _call(L, nbytes=need - 1) == EINVAL and _call(L, nbytes=0) == EINVAL
    # nothing to do: no launch, and the scratch is not looked at
    assert _call(L, B=0, nbytes=0) == OK and _call(L, A=0) == OK and _call(L, B=0, M=0, gt_boxes=None, nbytes=0) == OK
    nine = dict(begin=tuple(range(10)), hi=(0.5,) * 9, lo=(0.3,) * 9, ids=tuple(range(1, 10)), per_loc=9, A=900)
    assert _call(L, **nine) == ERANGE
    assert _call(L, M=K['DFU3D_ANC_MAX_BOXES'] + 1, nbytes=1 << 30) == ERANGE
    assert _call(L, B=K['DFU3D_ANC_MAX_BATCH'] + 1, nbytes=1 << 30) == ERANGE
    assert _call(L, A=6 * 2 ** 26, B=2, nbytes=1 << 30) == ERANGE                   # B * A * 7 = 2^31 * 2.6
    assert _call(L, A=2 ** 31 - 2, B=65535, nbytes=1 << 40) == ERANGE              # no 64-bit wrap-around
    # an out-of-range size wins over what is empty, an invalid one over both
    assert _call(L, B=0, M=K['DFU3D_ANC_MAX_BOXES'] + 1) == ERANGE and _call(L, B=0, A=601) == EINVAL


def test_scratch_bytes_grow_with_the_boxes_only():
    L = _lib_anc.lib()
    K = _lib_anc.CONSTANTS
    for bad in ((-1, 6, 9), (2, -6, 9), (2, 6, -1), (2, 6, K['DFU3D_ANC_MAX_BOXES'] + 1), (K['DFU3D_ANC_MAX_BATCH'] + 1, 6, 9),
                (0, 6, 9)):
        assert L.dfu3d_anc_scratch_bytes(*bad) == 0, bad
    assert L.dfu3d_anc_scratch_bytes(4, 6, 15) == L.dfu3d_anc_scratch_bytes(4, 211200, 15)       # A does not enter
    by_m = [L.dfu3d_anc_scratch_bytes(4, 600, M) for M in (0, 1, 15, 70, 512)]
    assert all(a < b for a, b in zip(by_m, by_m[1:])) and all(s % 16 == 0 for s in by_m) and by_m[0] > 0
    for B, M in ((1, 1), (4, 15), (3, 70), (65535, 512)):
        rows = B * M
        assert 28 * rows + 36 * B <= L.dfu3d_anc_scratch_bytes(B, 6, M) <= 28 * rows + 36 * B + 4 * 16


def test_ops_argument_checks():
    import torch
    from dfu3d_amd import anchor_target_ops as ops
    sets = [(2, 0.6, 0.45, 1)]
    with pytest.raises(_lib.Dfu3dError, match=r"anchors must have the shape \(A, 7\)"):
        ops.assign_targets(torch.zeros(4, 8), sets, torch.zeros(1, 2, 8))
    with pytest.raises(_lib.Dfu3dError, match=r"gt_boxes must have the shape \(B, M, 8\)"):
        ops.assign_targets(torch.zeros(4, 7), sets, torch.zeros(1, 2, 7))
    with pytest.raises(_lib.Dfu3dError, match="class_sets"):
        ops.assign_targets(torch.zeros(4, 7), [], torch.zeros(1, 2, 8))
    with pytest.raises(_lib.Dfu3dError, match="at most 8"):
        ops.assign_targets(torch.zeros(18, 7), [(1, 0.5, 0.3, k + 1) for k in range(9)], torch.zeros(1, 2, 8))
    with pytest.raises(_lib.Dfu3dError, match="DFU3D_ERANGE"):
        ops.assign_targets(torch.zeros(4, 7), sets, torch.zeros(1, 513, 8))
    with pytest.raises(_lib.Dfu3dError, match="must live on the GPU"):
        ops.assign_targets(torch.zeros(4, 7), sets, torch.zeros(1, 2, 8))
    per_loc, begin, matched, unmatched, ids = ops.set_arrays(R.class_sets(R.generate_anchors(R.G25_RANGE, [(12, 10)] * 3)[0]))
    assert per_loc == 6 and list(begin) == [0, 2, 4, 6] and list(ids) == [1, 2, 3]
    assert list(matched) == [np.float32(v) for v in (0.6, 0.5, 0.5)] and list(unmatched) == [np.float32(v) for v in (0.45, 0.35, 0.35)]


# ---- the restatement and the generator against the reference --------------------------------------------------------------------
def test_the_restatement_equals_the_reference(golden):
    g, meta = golden
    anchors, per_loc = R.generate_anchors(R.G25_RANGE, R.feature_map_sizes(R.G25_GRID))
    assert per_loc == [2, 2, 2] and sum(per_loc) == meta['num_anchors_per_location']
    for k, a in enumerate(anchors):
        assert a.shape == (1, 10, 12, 1, 2, 7) and np.array_equal(bits(a), bits(g['anchors%d' % k]))
    assert np.array_equal(bits(R.flat(anchors)), bits(g['anchors']))
    gt = g['gt_boxes']
    assert gt.shape == (R.G25_B, R.G25_M, 8) and not gt[0, 6:].any() and not gt[1, 1].any() and gt[1, 2].any() and not gt[2].any()
    rec = []
    labels, targets, weights = R.assign_targets(anchors, gt, record=rec)
    assert labels.dtype == np.int32 and np.array_equal(labels, g['box_cls_labels'])
    assert np.array_equal(bits(weights), bits(g['reg_weights'])) and np.array_equal(bits(targets), bits(g['box_reg_targets']))
    assert set(np.unique(labels[0])) == {-1, 0, 1, 2, 3} and (labels > 0).any(1).tolist() == [True, True, False]
    assert rec[5]['iou'].shape[1] == 1 and [r is None for r in rec[6:]] == [True, True, False]    # zero rows under Bicycle
    assert not targets[labels <= 0].any() and targets[labels > 0].any(1).all()


def test_the_cases_of_the_gpu_test_hold_their_conditions():
    res = R.check_cases()
    assert len(res) == 10 and all(lab.shape == (1, 13260) for lab, _, _ in res.values())


def test_assign_flat_equals_assign_targets(golden):
    """The class sets on a flat block (any extents) against the concatenation along the sizes axis, on G25's layout and on
    the layout of the cases: the same bits."""
    g, _ = golden
    anchors, _ = R.generate_anchors(R.G25_RANGE, R.feature_map_sizes(R.G25_GRID))
    pairs = [(anchors, g['gt_boxes'])]
    anchors = R.case_anchors()
    cs = R.cases()
    pairs.append((anchors, np.stack([cs[n] for n in cs])))
    for all_anchors, gt in pairs:
        want = R.assign_targets(all_anchors, gt)
        got = R.assign_flat_rows(R.flat(all_anchors), R.class_sets(all_anchors), gt)
        assert (want[0] > 0).any() and (want[0] == -1).any()
        assert all(u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(got[:3], want))
        assert np.array_equal(got[3], R.foreground_rows(all_anchors, gt))
        assert np.array_equal(R.foreground_rows_flat(R.flat(all_anchors), R.class_sets(all_anchors), gt), got[3])


def test_the_edge_cases_hold_their_conditions():
    res = R.check_edge_cases()
    assert list(res) == R.EDGE_NAMES and len(res) == 18
    assert sorted({c['flat'].shape[0] for c, _ in res.values()}) == [6, 126, 252, 504, 756, 768, 1536]
    assert {len(c['sets']) for c, _ in res.values()} == {1, 3, 8}
    big = R.check_big_m_cases()
    assert [g.shape[1] for g, _ in big.values()] == [512, 512, 257] and list(big) == R.BIG_M_NAMES
    assert all(w[0].shape == (1, 13260) for _, w in big.values())
    case, want = R.batch_limit_case()
    K = _lib_anc.CONSTANTS
    assert case['gt'].shape == (K['DFU3D_ANC_MAX_BATCH'], 1, 8) and want[1].shape == (65535, 6, 7) and (want[0][-1] > 0).any()


def test_the_restatement_equals_golden_g27():
    """The reference's assigner alone, five class names, anchor classes (3, 1, 5) with 3, 6 and 3 slots: every bit, through
    assign_targets and through assign_flat; and the fixture holds the conditions it was built for."""
    g = np.load(G27)
    meta = json.loads(bytes(g['meta']).decode())
    cfg27, names = R.G27_ANCHOR_CFG, R.G27_CLASS_NAMES
    assert meta['classes'] == names and meta['num_anchors_per_location'] == [3, 6, 3] and os.path.getsize(G27) <= os.path.getsize(GOLDEN)
    anchors, per_loc = R.generate_anchors(R.G27_RANGE, R.feature_map_sizes(R.G27_GRID, cfg27), cfg27)
    assert per_loc == [3, 6, 3] and [a.shape for a in anchors] == [(1, 17, 17, 1, 3, 7), (1, 17, 17, 2, 3, 7), (1, 17, 17, 1, 3, 7)]
    assert all(np.array_equal(bits(a), bits(g['anchors%d' % k])) for k, a in enumerate(anchors))
    assert np.array_equal(bits(R.flat(anchors)), bits(g['anchors']))
    gt = g['gt_boxes']
    assert np.array_equal(bits(gt), bits(R.g27_boxes())) and gt.shape == (R.G27_B, R.G27_M, 8)
    sets = R.class_sets(anchors, cfg27, names)
    assert sets == [(3, 0.5, 0.5, 3), (6, 0.5, 0.25, 1), (3, 0.75, 0.25, 5)]
    rec = []
    flat_out = R.assign_flat_rows(R.flat(anchors), sets, gt, rec)
    for got in (R.assign_targets(anchors, gt, cfg27, names), flat_out[:3]):
        assert got[0].dtype == np.int32 and np.array_equal(got[0], g['box_cls_labels'])
        assert np.array_equal(bits(got[2]), bits(g['reg_weights'])) and np.array_equal(bits(got[1]), bits(g['box_reg_targets']))
    # sample 0, the Car set: anchors that no box forces exactly on matched (positive) and exactly on unmatched (-1)
    r = rec[1]
    loose = np.setdiff1d(np.arange(len(r['best'])), r['forced'])
    assert any(r['best'][a] == 0.5 and r['labels'][a] == 1 for a in loose)
    assert any(r['best'][a] == 0.25 and r['labels'][a] == -1 for a in loose)
    # the Cyclist set has unmatched == matched: no -1 in any sample, and anchors on the shared value
    assert all(not (rec[3 * b]['labels'] == -1).any() for b in range(3)) and (rec[0]['best'] == 0.5).any()
    # sample 1: the rows of the classes 2 and 4 change nothing; a class-0 row forces an anchor to label 0 and wins an arg max
    assert sorted(set(gt[1, :, 7].astype(int).tolist())) == [0, 1, 2, 3, 4, 5]
    drop = [k for k in range(R.G27_M) if gt[1, k, 7] in (2, 4)]
    less = np.zeros_like(gt[1:2])
    keep = [k for k in range(R.G27_M) if k not in drop]
    less[0, :len(keep)] = gt[1, keep]
    assert len(drop) >= 3 and all(u.tobytes() == v[1:2].tobytes() for u, v in zip(R.assign_flat(R.flat(anchors), sets, less), flat_out[:3]))
    r = rec[3 + 2]
    zero = [k for k, row in enumerate(r['own']) if gt[1, row, 7] == 0 and gt[1, row, 3] > 0]
    assert any(r['top'][k] > 0 and (r['labels'][np.nonzero(r['iou'][:, k] == r['top'][k])[0]] == 0).all() for k in zero)
    truck = list(r['own']).index(3)
    assert any(r['arg'][a] in zero and 0 < r['iou'][a, truck] < r['best'][a] and r['labels'][a] == 0 for a in range(len(r['best'])))
    assert not gt[2, 9:].any() and not gt[1, 2].any() and (flat_out[0] > 0).any(1).all()


# ---- the assigner's flattened block follows its source tensors -----------------------------------------------------------------
FLAT_N = 3 * 10 * 12 * 2 * 7


def flat_sum(x):
    return float(x.double().sum())


def fresh_anchors(value):
    import torch
    return [torch.full((1, 10, 12, 1, 2, 7), float(value)) for _ in range(3)]


def new_assigner():
    from dfu3d_amd.pcdet_kitti.axis_aligned_target_assigner import AxisAlignedTargetAssigner
    from dfu3d_amd.pcdet_kitti.box_coder_utils import ResidualCoder
    return AxisAlignedTargetAssigner(cfg(R.HEAD_CFG), R.CLASS_NAMES, ResidualCoder())


def test_flat_anchors_after_an_in_place_change():
    import torch
    assigner, a = new_assigner(), fresh_anchors(1.0)
    first = assigner.flat_anchors(a)
    assert first.shape == (720, 7) and flat_sum(first) == FLAT_N
    a[0].add_(1.0)
    second = assigner.flat_anchors(a)
    assert flat_sum(second) == FLAT_N + FLAT_N // 3 and torch.equal(second, torch.cat(a, dim=-3).view(-1, 7))
    assert assigner.flat_anchors(a) is second
    a[2][0, 3, 4, 0, 1, 5] = 9.0                                               # through a view: the version moves as well
    assert flat_sum(assigner.flat_anchors(a)) == FLAT_N + FLAT_N // 3 + 8


def test_flat_anchors_after_new_tensors_of_the_same_shape():
    """The old tensors are dropped before the new ones are made, so the allocator may hand out the old addresses again."""
    assigner = new_assigner()
    for value in (1.0, 2.0, 3.0, 4.0):
        a = fresh_anchors(value)
        got = assigner.flat_anchors(a)
        assert flat_sum(got) == value * FLAT_N, value
        assert assigner.flat_anchors(a) is got
        del a, got
    a = fresh_anchors(5.0)
    a[1] = a[1] + 1.0                                                           # one entry of the list replaced
    assert flat_sum(assigner.flat_anchors(a)) == 5.0 * FLAT_N + FLAT_N // 3
    # whether the allocator does so is its business; memory the test owns states it: new tensors, the old addresses
    import torch
    mem = np.ones((3, 1, 10, 12, 1, 2, 7), np.float32)
    a = [torch.from_numpy(m) for m in mem]
    where = [t.data_ptr() for t in a]
    assert flat_sum(assigner.flat_anchors(a)) == FLAT_N
    del a
    mem *= 2.0
    a = [torch.from_numpy(m) for m in mem]
    assert [t.data_ptr() for t in a] == where and flat_sum(assigner.flat_anchors(a)) == 2.0 * FLAT_N


def test_flat_anchors_unchanged_is_one_cat(monkeypatch):
    import torch
    from dfu3d_amd.pcdet_kitti import axis_aligned_target_assigner as mod
    calls = []
    real = torch.cat
    monkeypatch.setattr(mod.torch, "cat", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assigner, a = new_assigner(), fresh_anchors(1.0)
    first = assigner.flat_anchors(a)
    assert all(assigner.flat_anchors(x) is first for x in (a, list(a), tuple(a), a)) and len(calls) == 1
    assert first.is_contiguous() and first.shape == (720, 7) and all(t._version == 0 for t in a)


def test_anchor_generator_equals_the_reference(golden):
    import torch
    from dfu3d_amd.pcdet_kitti.anchor_generator import AnchorGenerator
    from dfu3d_amd.pcdet_kitti.anchor_head_single import AnchorHeadTemplate
    g, _ = golden
    gen = AnchorGenerator(R.G25_RANGE, cfg(R.ANCHOR_CFG))
    anchors, per_loc = gen.generate_anchors([np.array(s) for s in R.feature_map_sizes(R.G25_GRID)])
    assert per_loc == [2, 2, 2]
    for k, a in enumerate(anchors):
        assert a.dtype == torch.float32 and a.device.type == 'cpu' and np.array_equal(bits(a.numpy()), bits(g['anchors%d' % k]))
    again, _ = AnchorHeadTemplate.generate_anchors(cfg(R.ANCHOR_CFG), R.G25_GRID, R.G25_RANGE)
    assert all(torch.equal(a, b) for a, b in zip(anchors, again))
    centred = [dict(c, align_center=True) for c in R.ANCHOR_CFG]
    got, _ = AnchorGenerator(R.G25_RANGE, centred).generate_anchors(R.feature_map_sizes(R.G25_GRID))
    want, _ = R.generate_anchors(R.G25_RANGE, R.feature_map_sizes(R.G25_GRID), centred)
    assert all(np.array_equal(bits(a.numpy()), bits(b)) for a, b in zip(got, want))


def test_box_utils_equal_the_restatement(golden):
    import torch
    from dfu3d_amd.pcdet_kitti import box_utils
    from dfu3d_amd.pcdet_kitti.common_utils import limit_period
    g, _ = golden
    a, b = g['anchors'], np.concatenate([g['gt_boxes'][0, :, :7], R.cases()['headings_at_quarter_turns'][:8, :7]])
    got = box_utils.boxes3d_nearest_bev_iou(torch.from_numpy(a), torch.from_numpy(b)).numpy()
    assert got.shape == (720, 17) and got.max() > 0.5 and np.array_equal(bits(got), bits(R.nearest_bev_iou(a, b)))
    rect = box_utils.boxes3d_lidar_to_aligned_bev_boxes(torch.from_numpy(b)).numpy()
    assert np.array_equal(bits(rect), bits(R.aligned_bev_boxes(b)))
    v = np.linspace(-7, 7, 57).astype(np.float32)
    assert np.array_equal(bits(limit_period(torch.from_numpy(v), 0.5, np.pi).numpy()), bits(R.limit_period(v)))
    assert limit_period(v).dtype == np.float32 and np.array_equal(bits(limit_period(v)), bits(R.limit_period(v)))


# ---- the head on the golden's predictions and targets (CPU: plain torch) -----------------------------------------------------------
def head_on_golden(g, device="cpu"):
    import torch
    from dfu3d_amd.pcdet_kitti.anchor_head_single import AnchorHeadSingle
    head = AnchorHeadSingle(cfg(R.HEAD_CFG), R.G25_CHANNELS, len(R.CLASS_NAMES), R.CLASS_NAMES, R.G25_GRID, R.G25_RANGE)
    head.load_state_dict({k[3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('sd_')}, strict=True)
    head = head.to(device).train()
    ret = head.forward_ret_dict
    for k in ('cls_preds', 'box_preds', 'dir_cls_preds'):
        ret[k] = torch.from_numpy(g[k]).to(device).requires_grad_()
    for k in ('box_cls_labels', 'box_reg_targets', 'reg_weights'):
        ret[k] = torch.from_numpy(g[k]).to(device)
    return head


def test_head_state_dict_and_losses_on_the_cpu(golden):
    import torch
    g, meta = golden
    head = head_on_golden(g)
    assert [[k, list(v.shape)] for k, v in head.state_dict().items()] == meta['state_dict_keys']
    assert [k for k, _ in meta['state_dict_keys']] == ['conv_cls.weight', 'conv_cls.bias', 'conv_box.weight', 'conv_box.bias',
                                                      'conv_dir_cls.weight', 'conv_dir_cls.bias']
    assert head.num_anchors_per_location == 6 and all(a.device.type == 'cpu' for a in head.anchors)
    loss, tb = head.get_loss()
    loss.backward()
    ret = head.forward_ret_dict
    # the same torch on the same CPU kernels: the same bits
    assert [tb[k] for k in ('rpn_loss', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir')] == g['loss'].tolist()
    for k in ('cls', 'loc', 'dir'):
        assert np.array_equal(bits(ret[k + '_loss_src'].detach().numpy()), bits(g[k + '_loss_src'])), k
    for k in ('cls_preds', 'box_preds', 'dir_cls_preds'):
        assert np.array_equal(bits(ret[k].grad.numpy()), bits(g['grad_' + k])), k
    with torch.no_grad():
        cls, box = head.generate_predicted_boxes(R.G25_B, ret['cls_preds'].detach(), ret['box_preds'].detach(),
                                                     ret['dir_cls_preds'].detach())
    assert np.array_equal(bits(cls.numpy()), bits(g['batch_cls_preds'])) and np.array_equal(bits(box.numpy()), bits(g['batch_box_preds']))
    fresh = type(head)(cfg(R.HEAD_CFG), 8, 3, R.CLASS_NAMES, R.G25_GRID, R.G25_RANGE)
    assert float(fresh.conv_cls.bias[0]) == pytest.approx(-np.log(99.0)) and float(fresh.conv_box.weight.std()) < 0.002


def test_weighted_cross_entropy_loss():
    import torch
    from dfu3d_amd.pcdet_kitti.loss_utils import WeightedCrossEntropyLoss
    x = torch.tensor([[[2.0, -1.0], [0.5, 0.5], [-3.0, 4.0]]])
    t = torch.tensor([[[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]]])
    w = torch.tensor([[1.0, 0.5, 0.0]])
    got = WeightedCrossEntropyLoss()(x, t, w)
    want = -(torch.log_softmax(x, -1) * t).sum(-1) * w
    assert got.shape == (1, 3) and torch.allclose(got, want, atol=1e-7) and got[0, 2] == 0


# ---- SECONDNet ----------------------------------------------------------------------------------------------------------------------
def second_net(model=None, **over):
    from dfu3d_amd.pcdet_kitti.second_net import SECONDNet
    kw = dict(class_names=R.CLASS_NAMES, grid_size=R.G25_GRID, point_cloud_range=R.G25_RANGE, voxel_size=[0.1, 0.1, 0.1],
              num_point_features=4)
    kw.update(over)
    return SECONDNet(cfg(model or R.SECOND_MODEL), len(kw['class_names']), **kw)


def test_second_net_state_dict_keys(golden):
    _, meta = golden
    model = second_net()
    assert [type(m).__name__ for m in model.module_list] == ['MeanVFE', 'VoxelBackBone8x', 'HeightCompression',
                                                             'BaseBEVBackbone', 'AnchorHeadSingle']
    sd = [(k, list(v.shape)) for k, v in model.state_dict().items()]
    g24 = json.load(open(G24))
    assert sd[0] == ('global_step', [1])
    assert [(k[len('backbone_3d.'):], s) for k, s in sd if k.startswith('backbone_3d.')] == [tuple(e) for e in map(tuple, g24['VoxelBackBone8x'])]
    head = [[k[len('dense_head.'):], s] for k, s in sd if k.startswith('dense_head.')]
    assert [k for k, _ in head] == [k for k, _ in meta['state_dict_keys']]
    assert head[0][1] == [18, 512, 1, 1] and head[2][1] == [42, 512, 1, 1] and head[4][1] == [12, 512, 1, 1]
    rest = [k for k, _ in sd[1:] if not k.startswith(('backbone_3d.', 'dense_head.'))]
    assert rest and all(k.startswith('backbone_2d.') for k in rest)
    assert not [k for k, _ in sd if 'anchor' in k]                                  # the anchors are no buffers
    # the other detectors take no anchor head, and this one no centre head
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    with pytest.raises(NotImplementedError, match="CenterPoint: DENSE_HEAD.NAME = 'AnchorHeadSingle'"):
        CenterPoint(cfg(R.SECOND_MODEL), 3, sparse_3d=True, class_names=R.CLASS_NAMES, grid_size=R.G25_GRID,
                    point_cloud_range=R.G25_RANGE, voxel_size=[0.1, 0.1, 0.1], num_point_features=4)
    with pytest.raises(NotImplementedError, match="SECONDNet: DENSE_HEAD.NAME = 'AnchorHeadMulti'"):
        second_net(dict(R.SECOND_MODEL, DENSE_HEAD=dict(R.HEAD_CFG, NAME='AnchorHeadMulti')))


def head_cfg(**over):
    c = dict(R.HEAD_CFG)
    for k, v in over.items():
        c[k] = dict(c[k], **v) if isinstance(v, dict) and isinstance(c.get(k), dict) else v
    return c


@pytest.mark.parametrize("over,names", [
    (dict(TARGET_ASSIGNER_CONFIG={'POS_FRACTION': 0.5}), "POS_FRACTION"),
    (dict(TARGET_ASSIGNER_CONFIG={'NORM_BY_NUM_EXAMPLES': True}), "NORM_BY_NUM_EXAMPLES"),
    (dict(TARGET_ASSIGNER_CONFIG={'MATCH_HEIGHT': True}), "MATCH_HEIGHT"),
    (dict(TARGET_ASSIGNER_CONFIG={'NAME': 'ATSS'}), "TARGET_ASSIGNER_CONFIG.NAME = 'ATSS'"),
    (dict(TARGET_ASSIGNER_CONFIG={'BOX_CODER': 'PreviousResidualDecoder'}), "BOX_CODER"),
    (dict(TARGET_ASSIGNER_CONFIG={'BOX_CODER_CONFIG': {'encode_angle_by_sincos': True}}), "BOX_CODER"),
    (dict(USE_MULTIHEAD=True), "USE_MULTIHEAD"),
    (dict(LOSS_CONFIG={'REG_LOSS_TYPE': 'WeightedL1Loss'}), "REG_LOSS_TYPE"),
    (dict(ANCHOR_GENERATOR_CONFIG=R.ANCHOR_CFG[::-1]), "last entry of ANCHOR_GENERATOR_CONFIG"),
    (dict(ANCHOR_GENERATOR_CONFIG=[R.ANCHOR_CFG[0], dict(R.ANCHOR_CFG[2], class_name='Truck')]), "ANCHOR_GENERATOR_CONFIG names"),
])
def test_unsupported_settings_raise(over, names):
    from dfu3d_amd.pcdet_kitti.anchor_head_single import AnchorHeadSingle
    with pytest.raises(NotImplementedError, match=names):
        AnchorHeadSingle(cfg(head_cfg(**over)), 8, 3, R.CLASS_NAMES, R.G25_GRID, R.G25_RANGE)
