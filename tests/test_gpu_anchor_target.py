"""GPU: the anchor target stage (dfu3d_amd.anchor_target_ops -> csrc/anchor_stage.hip) against golden G25 (the
reference's own assigner on the CPU) and against the NumPy restatement of tests/anchor_target_ref.py.

Labels and weights must be equal.  Regression targets of rows that are no foreground must be exactly 0.  Foreground
targets are within d_hip <= max(4 * d_torch, 4 ulp at the largest golden magnitude), d_torch being the deviation of the
plain ResidualCoder.encode_torch on the same GPU, fed with the box row the restatement encodes each anchor from -- the
rule of goldens G20 and G21.  (The IoU itself needs no margin: float32 operations that are correctly rounded on both
sides; an IoU that differed in one bit would show as a label at one of the thresholds or as a missing forced anchor.)

The cases (tests/anchor_target_ref.py: cases, each asserting there that its condition occurs) run over 65 x 34 locations
x 6 anchors = 13 260 anchors -- 51.8 workgroups -- with M = 70 rows, more than a wave: as single samples, as one batch,
twice for equal bits, and between guard bands with poisoned scratch."""
import numpy as np
import pytest

from tests import anchor_target_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_NAMES = ['no_box', 'trailing_zero_rows', 'interior_zero_row', 'class_without_box', 'box_out_of_range',
              'tiny_box_forced_on_ties', 'identical_boxes', 'forced_with_other_argmax', 'headings_at_quarter_turns',
              'seventy_boxes']


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def case_data():
    """The anchors of the cases, the rows of every case and the restatement's result for each, computed once."""
    anchors = R.case_anchors()
    want = R.check_cases(anchors)
    assert list(want) == CASE_NAMES
    return anchors, R.cases(), want


def run(all_anchors, gt):
    from dfu3d_amd import anchor_target_ops as ops
    return ops.assign_targets(cu(R.flat(all_anchors)), R.class_sets(all_anchors), cu(gt))


def compare(name, got, want, all_anchors, gt, class_sets=None, flat=None, rows=None):
    """got: the stage's three tensors; want: the golden's or the restatement's three arrays.  The anchors are all_anchors
    (per class, the KITTI sets), or the block `flat` with its class_sets; rows: the restatement's foreground rows where the
    caller has them already."""
    from dfu3d_amd.pcdet_kitti.box_coder_utils import ResidualCoder
    labels, targets, weights = (t.cpu().numpy() for t in got)
    assert labels.dtype == np.int32 and targets.dtype == np.float32 and weights.dtype == np.float32
    assert labels.shape == want[0].shape and targets.shape == want[1].shape and weights.shape == want[2].shape
    assert np.array_equal(labels, want[0]), (name, int((labels != want[0]).sum()))
    assert np.array_equal(bits(weights), bits(want[2])), name
    fg = labels > 0
    assert not bits(targets[~fg]).any(), name                          # exactly +0.0
    if not fg.any():
        return
    if flat is None:
        flat = R.flat(all_anchors)
        rows = R.foreground_rows(all_anchors, gt) if rows is None else rows
    elif rows is None:
        rows = R.foreground_rows_flat(flat, class_sets, gt)
    b, a = np.nonzero(fg)
    plain = ResidualCoder().encode_torch(cu(gt[b, rows[b, a], :7]), cu(flat[a])).cpu().numpy()
    gold = want[1][fg]
    d_hip, d_torch = float(np.abs(targets[fg] - gold).max()), float(np.abs(plain - gold).max())
    floor = 4.0 * float(np.spacing(np.float32(np.abs(gold).max())))
    print("%-28s %5d foreground rows  d_hip %.3g  d_torch %.3g  floor %.3g  (largest |golden| %.3g)"
          % (name, int(fg.sum()), d_hip, d_torch, floor, np.abs(gold).max()))
    assert d_hip <= max(4.0 * d_torch, floor), (name, d_hip, d_torch, floor)


def test_against_golden_g25():
    import os
    import torch
    from dfu3d_amd.pcdet_kitti.anchor_head_single import AnchorHeadSingle
    from tests.centerpoint_cases import cfg
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_anchor_head.npz"))
    anchors, _ = R.generate_anchors(R.G25_RANGE, R.feature_map_sizes(R.G25_GRID))
    want = (g['box_cls_labels'], g['box_reg_targets'], g['reg_weights'])
    compare("G25 stage", run(anchors, g['gt_boxes']), want, anchors, g['gt_boxes'])
    # through the head: its own anchors, moved with the module, and the assigner's dict
    head = AnchorHeadSingle(cfg(R.HEAD_CFG), R.G25_CHANNELS, 3, R.CLASS_NAMES, R.G25_GRID, R.G25_RANGE).to(DEV)
    assert all(a.device.type == 'cuda' for a in head.anchors)
    flat = torch.cat(head.anchors, dim=-3).view(-1, 7)
    assert np.array_equal(bits(flat.cpu().numpy()), bits(g['anchors']))
    d = head.assign_targets(cu(g['gt_boxes']))
    assert list(d) == ['box_cls_labels', 'box_reg_targets', 'reg_weights']
    compare("G25 head", (d['box_cls_labels'], d['box_reg_targets'], d['reg_weights']), want, anchors, g['gt_boxes'])
    again = head.assign_targets(cu(g['gt_boxes']))
    assert all(torch.equal(d[k], again[k]) for k in d)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_a_case_alone(case_data, name):
    anchors, rows, want = case_data
    gt = rows[name][None]
    compare(name, run(anchors, gt), want[name], anchors, gt)


def test_one_empty_row_alone(case_data):
    """B = 1, M = 1: the one zero row stays, filed under the last class set; every label is 0."""
    anchors, _, want = case_data
    gt = np.zeros((1, 1, 8), np.float32)
    got = run(anchors, gt)
    compare("one zero row", got, want['no_box'], anchors, gt)
    assert not got[0].any() and not got[1].any() and not got[2].any()
    none = run(anchors, np.zeros((2, 0, 8), np.float32))                          # M = 0: the reference's empty slice
    assert tuple(none[0].shape) == (2, 13260) and not none[0].any() and not none[1].any() and not none[2].any()


def test_the_cases_as_one_batch_twice_and_under_guards(case_data):
    """B = 10 in one call: every sample equals its single run's reference; a second run has the same bits; and between guard
    bands, with scratch and outputs full of 0xFF or of 0x00 on entry, the same bits again."""
    import torch
    from tests.test_gpu_guard_bands import both_poisons
    anchors, rows, want = case_data
    gt = np.stack([rows[n] for n in CASE_NAMES])
    stacked = tuple(np.concatenate([want[n][k] for n in CASE_NAMES]) for k in range(3))
    first = run(anchors, gt)
    compare("batch of ten", first, stacked, anchors, gt)
    second = run(anchors, gt)
    assert all(torch.equal(x, y) for x, y in zip(first, second))
    assert bits(first[1].cpu().numpy()).tobytes() == bits(second[1].cpu().numpy()).tobytes()
    out = both_poisons(lambda: run(anchors, gt), count=6)                 # anchors, boxes, three outputs, the scratch
    for x, y in zip(first, out):
        assert x.cpu().numpy().tobytes() == y.tobytes()


def test_the_real_shape_against_the_restatement():
    """200 x 176 locations, 211 200 anchors, B = 2, 15 boxes each of the three classes."""
    rng = np.random.default_rng(211200)
    rng_range = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
    anchors, per_loc = R.generate_anchors(rng_range, [(176, 200)] * 3)
    assert R.flat(anchors).shape == (211200, 7) and per_loc == [2, 2, 2]
    gt = np.zeros((2, 20, 8), np.float32)
    for b in range(2):
        for k in range(15):
            make = [R.car, R.ped, R.bike][k % 3]
            box = np.array(make(rng.uniform(2.0, 68.0), rng.uniform(-38.0, 38.0), rng.uniform(-np.pi, np.pi)), np.float32)
            box[3:6] *= rng.uniform(0.85, 1.15, 3).astype(np.float32)
            gt[b, k] = box
    want = R.assign_targets(anchors, gt)
    assert (want[0] > 0).sum(1).min() >= 15 and (want[0] == -1).any()
    compare("real shape", run(anchors, gt), want, anchors, gt)
