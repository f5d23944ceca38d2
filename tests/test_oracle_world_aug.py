"""CPU: the NumPy restatement of the world-augmentation row (tests/world_aug_ref.py) against golden G15, the reference's own
run.  Decisions, order, counts, class column and collate layout are equal; floats are equal bit for bit, except the
rotated coordinates of lists under 64 rows (the reference's matmul takes another rounding chain there), which stay
within 2^-23 (|x| + |y|) at the rotation, and downstream of it within that bound times the scale plus one float32
rounding step of the value for the scale product and one for the translation sum (2^-22 |v|)."""
import numpy as np
import pytest

from tests import world_aug_cases as W
from tests import world_aug_ref as R

CASES = [(ci, s) for ci in range(W.N_CFG) for s in range(W.n_scenes())]


def _close_after_rotation(got, want, x, y, scale):
    tol = W.rot_bound(x, y) * abs(scale) + 2.0 ** -22 * np.abs(want)
    assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol), np.abs(got - want).max()


@pytest.mark.parametrize("ci,s", CASES)
def test_steps_match_the_reference(ci, s):
    G = W.golden()
    p, b, _ = W.inputs(ci, s)
    _, _, _, ap, ab, steps = W.restated(ci)[0][s]
    d = W.drawn(ci, s)
    pre = 'step/%d/%d/' % (ci, s)
    # before the rotation everything is one exact operation
    assert W.same_bits(steps['flip'][1], G[pre + 'random_world_flip/gt_boxes'])
    fp, fb = steps['flip']
    rp, rb = steps['rotation']
    want_p, want_b = G[pre + 'random_world_rotation/xyz'], G[pre + 'random_world_rotation/gt_boxes']
    assert want_b.dtype == b.dtype and want_p.dtype == np.float32
    if len(p) >= 64:
        assert W.same_bits(rp[:, 0:3], want_p)
    else:
        assert W.same_bits(rp[:, 2], want_p[:, 2])
        for k in (0, 1):
            assert np.all(np.abs(rp[:, k] - want_p[:, k]) <= W.rot_bound(fp[:, 0], fp[:, 1]))
    if len(b) >= 64:
        assert W.same_bits(rb, want_b)
    else:
        exact = [k for k in range(b.shape[1]) if k not in (0, 1, 7, 8)]
        assert W.same_bits(rb[:, exact], want_b[:, exact])
        for k0 in range(0, b.shape[1], 7):
            x, y = fb[:, k0].astype(np.float32), fb[:, k0 + 1].astype(np.float32)
            for k in (k0, k0 + 1):
                assert np.all(np.abs(rb[:, k] - want_b[:, k]) <= W.rot_bound(x, y))
    # after it: scaling, translation and the wrap
    sc = d['noise_scale'] or 1.0
    want_p, want_b = G['aug/%d/%d/xyz' % (ci, s)], G[pre + 'random_world_translation/gt_boxes']
    tb = steps['translation'][1]
    if len(p) >= 64:
        assert W.same_bits(ap[:, 0:3], want_p)
    else:
        assert W.same_bits(ap[:, 2], want_p[:, 2])
        for k in (0, 1):
            _close_after_rotation(ap[:, k], want_p[:, k], fp[:, 0], fp[:, 1], sc)
    assert np.array_equal(ap[:, 3:], p[:, 3:])
    if len(b) >= 64:
        assert W.same_bits(tb, want_b)
        assert W.same_bits(steps['scaling'][1], G[pre + 'random_world_scaling/gt_boxes'])
    else:
        exact = [k for k in range(b.shape[1]) if k not in (0, 1, 7, 8)]
        assert W.same_bits(tb[:, exact], want_b[:, exact])
        for k0 in range(0, b.shape[1], 7):
            x, y = fb[:, k0].astype(np.float32), fb[:, k0 + 1].astype(np.float32)
            for k in (k0, k0 + 1):
                _close_after_rotation(tb[:, k], want_b[:, k], x, y, sc)


@pytest.mark.parametrize("ci,s", CASES)
def test_decisions_and_final_arrays_match_the_reference(ci, s):
    G = W.golden()
    p, b, names = W.inputs(ci, s)
    fp, fg, keep, ap, ab, steps = W.restated(ci)[0][s]
    d = W.drawn(ci, s)
    assert np.array_equal(R.point_mask(ap, W.pc_range(ci)), G['final/%d/%d/point_keep' % (ci, s)])
    want = G['final/%d/%d/gt_boxes' % (ci, s)]
    assert fg.shape == want.shape and fg.dtype == want.dtype
    assert W.same_bits(fg[:, -1], want[:, -1])                    # class column: which boxes, in which order
    # the heading wrap is float32 arithmetic on a value that is exact in both: all but the rotated columns are equal
    exact = [k for k in range(fg.shape[1]) if k not in (0, 1, 7, 8)]
    assert W.same_bits(fg[:, exact], want[:, exact])
    if len(b) >= 64:
        assert W.same_bits(fg, want)
    else:
        fb = steps['flip'][1][keep]
        for k0 in range(0, b.shape[1], 7):
            x, y = fb[:, k0].astype(np.float32), fb[:, k0 + 1].astype(np.float32)
            for k in (k0, k0 + 1):
                _close_after_rotation(fg[:, k], want[:, k], x, y, d['noise_scale'] or 1.0)
    if W.planted(ci, s):                                          # rotation exactly 0: planted faces decide alike, bit for bit
        assert W.same_bits(fg, want) and W.same_bits(ap[:, 0:3], G['aug/%d/%d/xyz' % (ci, s)])


@pytest.mark.parametrize("ci", range(W.N_CFG))
def test_collate_layout_matches_the_reference(ci):
    G = W.golden()
    pts, gt, point_cnt, gt_cnt = W.restated(ci)[1]
    assert pts.dtype == np.float32 and gt.dtype == np.float32
    assert np.array_equal(pts[:, 0].astype(np.int8), G['batch/%d/batch_index' % ci])
    want = G['batch/%d/gt_boxes' % ci]
    assert gt.shape == want.shape
    assert np.array_equal(gt[:, :, -1], want[:, :, -1])
    big = [s for s in range(W.n_scenes()) if len(W.inputs(ci, s)[1]) >= 64]
    assert W.same_bits(gt[big], want[big])
    assert np.array_equal(gt_cnt, [(want[s, :, -1] != 0).sum() for s in range(len(want))])
    assert int(point_cnt.sum()) == len(pts)


@pytest.mark.parametrize("ci", range(W.N_CFG))
def test_draw_world_params_follows_the_reference_rng(ci):
    from dfu3d_amd.pcdet_kitti.data_augmentor import DataAugmentor
    G = W.golden()
    augs = {pl: DataAugmentor('.', W.dataset_cfg(ci, pl)['DATA_AUGMENTOR'], W.class_names()) for pl in (False, True)}
    seed = {0: 151, 1: 152}[ci]                                # SEEDS of the capture script
    np.random.seed(seed)
    for s in range(W.n_scenes()):
        got = augs[W.planted(ci, s)].draw_world_params(W.inputs(ci, s)[1].shape[1])
        want = W.drawn(ci, s)
        assert [(a, bool(v)) for a, v in got['flips']] == want['flips']
        assert got['noise_rot'] == want['noise_rot']
        assert got['noise_scale'] == want['noise_scale']
        assert got['noise_translate'].dtype == np.float32 and got['noise_translate'].shape == (1, 3)
        assert W.same_bits(got['noise_translate'], want['noise_translate'])
    st = np.random.get_state()
    assert np.array_equal(st[1], G['rng/%d/keys' % ci]) and st[2] == int(G['rng/%d/pos' % ci])
