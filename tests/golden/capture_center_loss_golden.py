"""Golden G14: the reference's own CenterHead loss (row f-8 of SURVEY.md section 8) -- `CenterHead.assign_targets` and
`CenterHead.get_loss` with `FocalLossCenterNet` / `RegLossCenterNet`, run unmodified on the CPU, and its autograd.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_center_loss_golden.py REFERENCE_ROOT      ->  tests/golden/g14_center_loss.npz

pcdet/utils/loss_utils.py, pcdet/models/model_utils/centernet_utils.py and pcdet/models/dense_heads/center_head.py are
imported UNMODIFIED as members of a package skeleton.  Import-time stand-ins: `numba` (its `jit` returns the function),
`model_nms_utils`, `pcdet.utils.box_utils` and `pcdet.ops.iou3d_nms.iou3d_nms_utils` (empty, unused on this path).  Both
methods are called on an object made with object.__new__(CenterHead) that carries only the attributes they read.

Cases A, B, C, their scenes and the seeded logits / regression maps: tests/center_loss_ref.py (CASES, scene,
predictions).  G14 stores no dense map: the targets sparsely, every loss scalar, the reference's float32 gradients (heat
maps: a seeded sample of elements plus fp64 checksums of all; regression maps: at every slot's cell, and the script
asserts that every other cell is zero), float64 sums of the generated inputs, and for every stored output d_ref, the
distance between the reference's float32 result and the restatement's fp64 result (per loss, per sampled heat-map
gradient element, per head for the regression gradients).  d_ref itself is asserted to lie inside the bounds that
tests/center_loss_ref.py derives from the number formats (LOSS_STEPS, hm_grad_bound), so a formula error in the
restatement cannot hide in it.

The NaN velocity of case B.  The reference's `_reg_loss` multiplies the NaN target by its zero `isnotnan` mask, which is
NaN again, so its loss for that channel, its total and every gradient come out NaN (stored as B_raw_losses).  The
contract skips such a channel.  The reference numbers case B is compared with are therefore taken from a second run in
which each NaN target is replaced by the prediction at that slot's cell: there the reference's own arithmetic gives that
(slot, channel) the contribution 0 to the loss and to the gradient, which is what skipping it means.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import center_head_ref as HR  # noqa: E402
from tests import center_loss_ref as R  # noqa: E402

HM_SAMPLE = 2048


class Cfg(dict):
    __getattr__ = dict.__getitem__


def load_reference():
    for name in ('pcdet', 'pcdet.models', 'pcdet.models.model_utils', 'pcdet.models.dense_heads', 'pcdet.utils', 'pcdet.ops',
                 'pcdet.ops.iou3d_nms'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        if '.' in name:
            setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    numba = types.ModuleType('numba')
    numba.jit = lambda *a, **k: (lambda fn: fn)
    sys.modules['numba'] = numba
    for name in ('pcdet.models.model_utils.model_nms_utils', 'pcdet.utils.box_utils', 'pcdet.ops.iou3d_nms.iou3d_nms_utils'):
        m = types.ModuleType(name)
        sys.modules[name] = m
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    lu = load('pcdet.utils.loss_utils', 'pcdet/utils/loss_utils.py')
    load('pcdet.models.model_utils.centernet_utils', 'pcdet/models/model_utils/centernet_utils.py')
    ch = load('pcdet.models.dense_heads.center_head', 'pcdet/models/dense_heads/center_head.py')
    return lu, ch


def make_head(lu, ch, case):
    cfg = case['cfg']
    head = object.__new__(ch.CenterHead)
    attrs = dict(
        model_cfg=Cfg(TARGET_ASSIGNER_CONFIG=Cfg(FEATURE_MAP_STRIDE=cfg['stride'], NUM_MAX_OBJS=cfg['num_max_objs'],
                                                 GAUSSIAN_OVERLAP=cfg['gaussian_overlap'], MIN_RADIUS=cfg['min_radius']),
                      LOSS_CONFIG=Cfg(LOSS_WEIGHTS=case['weights'])),
        class_names=cfg['class_names'], class_names_each_head=[list(h) for h in cfg['heads']],
        point_cloud_range=np.array(cfg['point_cloud_range'], dtype=np.float32), voxel_size=cfg['voxel_size'],
        separate_head_cfg=Cfg(HEAD_ORDER=case['head_order']), forward_ret_dict={},
        hm_loss_func=lu.FocalLossCenterNet(), reg_loss_func=lu.RegLossCenterNet())
    for k, v in attrs.items():
        object.__setattr__(head, k, v)
    return head


def run_reference(head, preds, targets):
    leaves = [{k: torch.from_numpy(v.copy()).requires_grad_() for k, v in d.items()} for d in preds]
    head.forward_ret_dict = {'pred_dicts': [dict(d) for d in leaves], 'target_dicts': targets}
    loss, tb = head.get_loss()
    loss.backward()
    n = len(preds)
    losses = np.asarray([tb[k % (h,)] for h in range(n) for k in ('hm_loss_head_%d', 'loc_loss_head_%d')] + [tb['rpn_loss']])
    assert loss.dtype == torch.float32
    grads = [{k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape, np.float32)) for k, v in d.items()} for d in leaves]
    return losses, grads


def main():
    lu, ch = load_reference()
    out, meta = {}, {'torch': torch.__version__, 'hm_sample': HM_SAMPLE}
    for name, case in R.CASES.items():
        cfg = case['cfg']
        H, W = cfg['map_hw']
        gt = R.scene(name)
        head = make_head(lu, ch, case)
        tg = head.assign_targets(torch.from_numpy(gt.copy()), feature_map_size=[H, W])
        mine = HR.assign_targets(gt, cfg)
        n = len(cfg['heads'])
        for key in ('heatmaps', 'target_boxes', 'inds', 'masks'):                     # original class ids == rewritten ones here
            for h in range(n):
                a, b = tg[key][h].numpy(), mine[key][h]
                if key == 'target_boxes':                                              # torch's float32 log / cos / sin: one step
                    assert np.array_equal(np.isnan(a), np.isnan(b)), (name, h)
                    assert HR.ulp_diff(np.nan_to_num(a), np.nan_to_num(b)).max() <= 1, (name, h)
                else:
                    assert np.array_equal(a, b), (name, key, h)
        targets = {k: [t.numpy() for t in tg[k]] for k in ('heatmaps', 'target_boxes', 'inds', 'masks')}
        preds = R.predictions(name, targets)
        out.update(R.pack_targets(name, targets))
        out[name + '_input_sums'] = R.input_sums(preds)
        nan_at = [np.argwhere(np.isnan(t)) for t in targets['target_boxes']]
        ref_targets = {k: [torch.from_numpy(t.copy()) for t in v] for k, v in targets.items()}
        if any(len(a) for a in nan_at):
            raw, _ = run_reference(head, preds, {k: [t.clone() for t in v] for k, v in ref_targets.items()})
            out[name + '_raw_losses'] = raw.astype(np.float32)
            assert np.isnan(raw[-1])
            for h, rows in enumerate(nan_at):
                stacked = np.concatenate([preds[h][k] for k in case['head_order']], axis=1)
                for b, k, c in rows:
                    ref_targets['target_boxes'][h][b, k, c] = float(stacked[b, c].reshape(-1)[targets['inds'][h][b, k]])
        losses, grads = run_reference(head, preds, ref_targets)
        fwd = R.forward(preds, targets, case['head_order'], case['weights'])
        hm64, reg = R.backward(preds, targets, case['head_order'], case['weights'], fwd)
        assert np.isfinite(losses).all()
        out[name + '_losses'] = losses.astype(np.float32)
        assert np.array_equal(out[name + '_losses'].astype(np.float64), losses)       # the reference's are float32 values
        out[name + '_d_losses'] = np.abs(losses - fwd['losses64'])
        print(name, 'loss d_ref in steps', out[name + '_d_losses'] / R.ulp32(losses))
        assert (out[name + '_d_losses'] <= R.LOSS_STEPS * R.ulp32(losses)).all(), name   # d_ref itself is bounded
        d_hm, d_reg, facts = [], [], []
        for h in range(n):
            g = grads[h]['hm'].reshape(-1)
            rs = np.random.RandomState(case['seed'] + 100 + h)
            idx = np.sort(rs.choice(g.size, min(g.size, HM_SAMPLE), replace=False)).astype(np.int32)
            out['%s_h%d_hm_grad_idx' % (name, h)] = idx
            out['%s_h%d_hm_grad_val' % (name, h)] = g[idx]
            out['%s_h%d_hm_grad_sums' % (name, h)] = np.asarray([g.astype(np.float64).sum(), np.abs(g.astype(np.float64)).sum()])
            d_elem = np.abs(g.astype(np.float64) - hm64[h].reshape(-1))
            out['%s_h%d_hm_grad_d' % (name, h)] = d_elem[idx]                       # d_ref of every sampled element
            bound = R.hm_grad_bound(preds[h]['hm'].reshape(-1), hm64[h].reshape(-1))
            print(name, h, 'hm grad d_ref / bound, worst', (d_elem / bound).max())
            assert (d_elem <= bound).all(), (name, h)
            d_hm.append(d_elem.max())
            ind = targets['inds'][h]
            ref_at = R.at_slots(grads[h], case['head_order'], ind)
            out['%s_h%d_reg_grad' % (name, h)] = ref_at
            d_reg.append(np.abs(ref_at.astype(np.float64) - R.at_slots(reg[h], case['head_order'], ind)).max())
            full = np.concatenate([grads[h][k] for k in case['head_order']], axis=1)
            full = full.reshape(full.shape[0], full.shape[1], -1).copy()
            valid = targets['masks'][h] != 0
            for b in range(full.shape[0]):
                full[b][:, ind[b][valid[b]]] = 0
            assert not full.any(), (name, h)                                           # zero off the target cells
            cells = [ind[b][valid[b]] for b in range(len(ind))]
            facts.append(dict(num=int(valid.sum()), num_pos=int(fwd['num_pos'][h]),
                              shared_cells=int(sum(len(c) - len(np.unique(c)) for c in cells)),
                              nan_targets=int(len(nan_at[h])),
                              clamped=int(((np.abs(preds[h]['hm']) > 12).sum())),
                              pred_equals_target=int((ref_at[valid] == 0).sum())))
        out[name + '_d_hm_grad'] = np.asarray(d_hm)
        out[name + '_d_reg_grad'] = np.asarray(d_reg)
        meta[name] = facts
        print(name, 'losses', losses, 'd', out[name + '_d_losses'].max(), 'd_hm', max(d_hm), 'd_reg', max(d_reg))
    a, b = meta['A'], meta['B']
    assert any(f['num'] == 0 and f['num_pos'] == 0 for f in a) and any(f['shared_cells'] for f in a)
    assert b[0]['num'] >= R.CASES['B']['cfg']['num_max_objs'] and any(f['nan_targets'] for f in b)
    assert all(f['clamped'] for f in a + b) and any(f['pred_equals_target'] for f in a + b)
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'g14_center_loss.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), meta)


if __name__ == '__main__':
    main()
