"""Golden G14 (the reference's CenterHead.get_loss and its autograd, tests/golden/capture_center_loss_golden.py) against
the NumPy restatement of the loss contract (tests/center_loss_ref.py): every loss and gradient within that output's d_ref
-- the distance of the reference's float32 arithmetic from the restatement's fp64 values, measured at capture -- plus one
float32 step for the restatement's own rounding."""
import json
import os

import numpy as np
import pytest

from tests import center_loss_ref as R


@pytest.fixture(scope="module")
def g14(golden_dir):
    g = np.load(os.path.join(golden_dir, "g14_center_loss.npz"))
    return g, json.loads(bytes(g["meta"]).decode())


@pytest.fixture(scope="module")
def restated(g14):
    g, _ = g14
    out = {}
    for name, case in R.CASES.items():
        targets = R.unpack_targets(name, g)
        preds = R.predictions(name, targets)
        fwd = R.forward(preds, targets, case['head_order'], case['weights'])
        hm64, reg = R.backward(preds, targets, case['head_order'], case['weights'], fwd)
        out[name] = (targets, preds, fwd, hm64, reg)
    return out


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_generated_inputs_match_their_checksums(g14, restated, name):
    g, _ = g14
    assert np.array_equal(R.input_sums(restated[name][1]), g[name + '_input_sums'])


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_reproduces_g14_losses(g14, restated, name):
    g, _ = g14
    fwd = restated[name][2]
    ref = g[name + '_losses']
    assert fwd['losses'].dtype == np.float32 and np.isfinite(ref).all()
    assert (np.abs(fwd['losses'].astype(np.float64) - ref) <= g[name + '_d_losses'] + R.ulp32(ref)).all()
    assert (np.abs(fwd['losses64'] - ref) <= g[name + '_d_losses']).all()          # what d_ref was measured as


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_restatement_reproduces_g14_gradients(g14, restated, name):
    g, _ = g14
    targets, _, _, hm64, reg = restated[name]
    for h in range(len(hm64)):
        idx, ref = g['%s_h%d_hm_grad_idx' % (name, h)], g['%s_h%d_hm_grad_val' % (name, h)]
        mine = hm64[h].astype(np.float32).reshape(-1)
        d = g[name + '_d_hm_grad'][h]
        d_elem = g['%s_h%d_hm_grad_d' % (name, h)]                                    # d_ref of each sampled element
        assert (np.abs(mine[idx].astype(np.float64) - ref) <= d_elem + R.ulp32(ref)).all(), h
        # the checksums over all N elements: N errors of at most d + one step of the largest element
        sums = g['%s_h%d_hm_grad_sums' % (name, h)]
        slack = mine.size * (d + R.ulp32(np.abs(mine).max()))
        assert abs(mine.astype(np.float64).sum() - sums[0]) <= slack and abs(np.abs(mine.astype(np.float64)).sum() - sums[1]) <= slack
        ref = g['%s_h%d_reg_grad' % (name, h)]
        at = R.at_slots(reg[h], R.CASES[name]['head_order'], targets['inds'][h])
        assert (np.abs(at.astype(np.float64) - ref) <= g[name + '_d_reg_grad'][h] + R.ulp32(ref)).all(), h


def test_g14_holds_the_scenes_the_contract_names(g14):
    g, meta = g14
    a, b = meta['A'], meta['B']
    assert any(f['num'] == 0 and f['num_pos'] == 0 for f in a)                       # a head with no box in the batch
    assert g['B_h0_masks'][0].all()                                                  # a full head
    assert any(f['shared_cells'] for f in a) and any(f['shared_cells'] for f in b)   # two boxes of a head in one cell
    assert b[0]['nan_targets'] == 1 and np.isnan(g['B_raw_losses'][-1])              # the reference's own answer: NaN
    assert all(f['clamped'] for f in a + b)                                          # logits beyond +-12
    assert all(f['pred_equals_target'] for f in a + b if f['num'])                   # pred == target at a slot
    assert g['C_h0_hm_idx'].max() < 35


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_d_ref_is_inside_the_bounds_of_the_number_formats(g14, restated, name):
    """d_ref is a measurement, so it is bounded itself: a formula error in the restatement would show as a d_ref beyond
    what float32 rounding of the reference's operations can produce (center_loss_ref.LOSS_STEPS, hm_grad_bound)."""
    g, _ = g14
    _, preds, _, hm64, _ = restated[name]
    assert (g[name + '_d_losses'] <= R.LOSS_STEPS * R.ulp32(g[name + '_losses'])).all()
    assert not g[name + '_d_reg_grad'].any()                                         # +-s_d: exact in both
    for h in range(len(hm64)):
        idx = g['%s_h%d_hm_grad_idx' % (name, h)]
        bound = R.hm_grad_bound(preds[h]['hm'].reshape(-1)[idx], hm64[h].reshape(-1)[idx])
        assert (g['%s_h%d_hm_grad_d' % (name, h)] <= bound).all(), h
        assert g[name + '_d_hm_grad'][h] >= g['%s_h%d_hm_grad_d' % (name, h)].max()
