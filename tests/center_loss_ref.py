"""CPU restatement (NumPy) of the CenterHead loss of row f-8 under the numerics contract of include/dfu3d_head.h, the
seeded scenes and prediction maps of golden G14 (tests/golden/capture_center_loss_golden.py), and the sparse form G14
stores targets in.  Written from the formulas of the contract:

  p = clamp(float32(sigmoid64(x)), 1e-4f, float32(1 - 1e-4));  g == 1: log(p) (1 - p)^2;  g < 1: log(1 - p) p^2 (1 - g)^4,
  both in fp64 from the float32 p and g;  hm_loss = cls_weight * (num_pos > 0 ? -(S_pos + S_neg) / num_pos : -S_neg);
  S_d = sum over valid slots of |pred - target| (fp64, in slot order, samples in order; a NaN target is skipped);  loc_loss = loc_weight * sum_d
  code_weights[d] * S_d / max(num, 1);  every loss rounded to float32 once; total = float32 sum in head order.

`forward` returns the fp64 values before rounding next to the float32 ones, so that a capture can measure how far the
reference's float32 arithmetic is from them (d_ref)."""
import numpy as np

from tests.center_head_ref import CFG_A, CFG_B

f32 = np.float32
P_MIN, P_MAX = f32(1e-4), f32(1 - 1e-4)

CFG_C = dict(class_names=['Car'], heads=[['Car']], point_cloud_range=[0, 0, -3.0, 7.0, 5.0, 1.0],
             voxel_size=[1.0, 1.0, 4.0], stride=1, map_hw=(5, 7), num_max_objs=4, gaussian_overlap=0.1, min_radius=2, C=8)

CASES = {
    'A': dict(cfg=CFG_A, B=2, seed=1401, head_order=['center', 'center_z', 'dim', 'rot'],
              weights=dict(cls_weight=1.0, loc_weight=0.25, code_weights=[1.0] * 8)),
    'B': dict(cfg=CFG_B, B=2, seed=1402, head_order=['center', 'center_z', 'dim', 'rot', 'vel'],
              weights=dict(cls_weight=0.75, loc_weight=2.5,
                           code_weights=[1.0, 0.5, 1.25, 2.0, 1.0, 0.3, 0.2, 0.2, 1.5, 0.1])),
    'C': dict(cfg=CFG_C, B=1, seed=1403, head_order=['center', 'center_z', 'dim', 'rot'],
              weights=dict(cls_weight=1.0, loc_weight=1.0, code_weights=[1.0] * 8)),
}
CHANNELS = {'center': 2, 'center_z': 1, 'dim': 3, 'rot': 2, 'vel': 2}


def _box(rs, cfg, cls, x=None, y=None):
    r = cfg['point_cloud_range']
    row = [rs.uniform(r[0] + 1, r[3] - 1) if x is None else x, rs.uniform(r[1] + 1, r[4] - 1) if y is None else y,
           rs.uniform(r[2], r[5]), rs.uniform(0.5, 6.0), rs.uniform(0.5, 2.5), rs.uniform(0.8, 3.0), rs.uniform(-np.pi, np.pi)]
    if cfg['C'] == 10:
        row += [rs.uniform(-8, 8), rs.uniform(-8, 8)]
    return row + [cls]


def scene(name):
    """gt_boxes (B, M, C) float32 of a case.  A: no Barrier (head 3 is empty in the whole batch), two Cars in one cell.
    B: eight Cars in sample 0 (head 0 full: NUM_MAX_OBJS = 8), two Pedestrians in one cell, a NaN velocity.
    C: two boxes on the 5 x 7 map."""
    case = CASES[name]
    cfg, rs = case['cfg'], np.random.RandomState(case['seed'])
    if name == 'A':
        classes = [c for c in range(1, 11) if c != 6]
        s0 = [_box(rs, cfg, classes[k % len(classes)]) for k in range(30)]
        s0 += [_box(rs, cfg, 1, x=20.3, y=-7.1), _box(rs, cfg, 1, x=20.4, y=-7.2)]
        samples = [s0, [_box(rs, cfg, c) for c in (1, 2, 9, 10, 4)]]
    elif name == 'B':
        s0 = [_box(rs, cfg, 1) for _ in range(8)] + [_box(rs, cfg, 2, x=30.1, y=4.1), _box(rs, cfg, 2, x=30.2, y=4.2),
                                                      _box(rs, cfg, 3)]
        s0[2][7] = np.nan
        samples = [s0, [_box(rs, cfg, 3), _box(rs, cfg, 1)]]
    else:
        samples = [[_box(rs, cfg, 1, x=2.4, y=1.6), _box(rs, cfg, 1, x=5.5, y=3.5)]]
    M = max(len(s) for s in samples) + 1
    gt = np.zeros((len(samples), M, cfg['C']), f32)
    for b, s in enumerate(samples):
        gt[b, :len(s)] = np.asarray(s, f32)
    return gt


def predictions(name, targets):
    """Per head {'hm': logits, HEAD_ORDER's maps}, float32, from the case's seed: logits around the head's initial bias
    with a share beyond +-12 (the clamp is active on both sides), regression maps uniform; the prediction of channel 2
    at the first valid slot's cell of every head is set to its target (pred == target exactly)."""
    case = CASES[name]
    cfg, rs = case['cfg'], np.random.RandomState(case['seed'] + 50)
    H, W = cfg['map_hw']
    out = []
    for h, names in enumerate(cfg['heads']):
        hm = rs.normal(-2.19, 2.5, (case['B'], len(names), H, W)).astype(f32)
        far = rs.uniform(size=hm.shape)
        hm[far < 0.02] = f32(-14.5)
        hm[far > 0.98] = f32(13.25)
        d = {'hm': hm}
        for key in case['head_order']:
            d[key] = rs.uniform(-2.0, 2.0, (case['B'], CHANNELS[key], H, W)).astype(f32)
        valid = np.argwhere(np.asarray(targets['masks'][h]) != 0)
        if len(valid):
            b, k = valid[0]
            d['center_z'][b, 0].reshape(-1)[targets['inds'][h][b, k]] = targets['target_boxes'][h][b, k, 2]
        out.append(d)
    return out


def input_sums(preds):
    return np.asarray([d[k].astype(np.float64).sum() for d in preds for k in d])


def pack_targets(name, ret):
    """The per-head lists of an assign_targets result -> flat arrays for an .npz (heat maps as index + value)."""
    out = {}
    for h in range(len(ret['heatmaps'])):
        hm = np.asarray(ret['heatmaps'][h], f32)
        idx = np.flatnonzero(hm)
        out['%s_h%d_hm_idx' % (name, h)] = idx.astype(np.int32)
        out['%s_h%d_hm_val' % (name, h)] = hm.reshape(-1)[idx]
        out['%s_h%d_target_boxes' % (name, h)] = np.asarray(ret['target_boxes'][h], f32)
        out['%s_h%d_inds' % (name, h)] = np.asarray(ret['inds'][h], np.int64)
        out['%s_h%d_masks' % (name, h)] = np.asarray(ret['masks'][h], np.int64)
    return out


def unpack_targets(name, g):
    case = CASES[name]
    cfg = case['cfg']
    H, W = cfg['map_hw']
    ret = {'heatmaps': [], 'target_boxes': [], 'inds': [], 'masks': []}
    for h, names in enumerate(cfg['heads']):
        hm = np.zeros(case['B'] * len(names) * H * W, f32)
        hm[g['%s_h%d_hm_idx' % (name, h)]] = g['%s_h%d_hm_val' % (name, h)]
        ret['heatmaps'].append(hm.reshape(case['B'], len(names), H, W))
        for key in ('target_boxes', 'inds', 'masks'):
            ret[key].append(g['%s_h%d_%s' % (name, h, key)])
    return ret


def _sigmoid(x):
    with np.errstate(over='ignore'):
        s = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    p = np.minimum(np.maximum(s.astype(f32), P_MIN), P_MAX)
    return s, p


def _stack(d, head_order):
    return np.concatenate([d[k] for k in head_order], axis=1)


def _slots(pred, target, ind, mask):
    """valid (B, K), pred at the slots (B, K, D) float32, use (B, K, D): valid slot and target not NaN."""
    B, D = pred.shape[:2]
    hw = pred.shape[2] * pred.shape[3]
    valid = (mask != 0) & (ind >= 0) & (ind < hw)
    at = np.take_along_axis(pred.reshape(B, D, hw), np.where(valid, ind, 0)[:, None, :].repeat(D, 1), axis=2).transpose(0, 2, 1)
    return valid, at, valid[:, :, None] & ~np.isnan(target)


def forward(preds, targets, head_order, weights):
    """-> dict: 'losses' float32 (2n + 1), 'losses64' the fp64 values before rounding (the total: the fp64 sum),
    'chan' float32 (n, D), 'chan64', 'num_pos' (n), 'num' (n)."""
    n = len(preds)
    cw, lw, code_w = float(weights['cls_weight']), float(weights['loc_weight']), [float(w) for w in weights['code_weights']]
    l64, chan64, num_pos, num = np.zeros(2 * n + 1), [], np.zeros(n), np.zeros(n)
    for h, d in enumerate(preds):
        g = np.asarray(targets['heatmaps'][h], f32)
        _, p = _sigmoid(d['hm'])
        p, g64 = p.astype(np.float64), g.astype(np.float64)
        pos, neg = g == f32(1), g < f32(1)
        with np.errstate(divide='ignore', invalid='ignore'):
            s_pos = (np.log(p) * ((1 - p) * (1 - p)))[pos].sum()
            w = (1 - g64) * (1 - g64)
            s_neg = (np.log(1 - p) * (p * p) * (w * w))[neg].sum()
        num_pos[h] = pos.sum()
        l64[2 * h] = cw * (-(s_pos + s_neg) / num_pos[h] if num_pos[h] > 0 else -s_neg)
        target = np.asarray(targets['target_boxes'][h], f32)
        valid, at, use = _slots(_stack(d, head_order), target, targets['inds'][h], targets['masks'][h])
        num[h] = valid.sum()
        diff = np.where(use, np.abs(at.astype(np.float64) - np.where(use, target, 0).astype(np.float64)), 0.0)
        per_sample = np.add.accumulate(diff, axis=1)[:, -1]          # slot after slot, as the contract sums
        chan64.append(np.add.accumulate(per_sample, axis=0)[-1] / max(num[h], 1.0))
        loc = 0.0
        for k, c in enumerate(chan64[-1]):
            loc += code_w[k] * c
        l64[2 * h + 1] = lw * loc
    losses = l64.astype(f32)
    total = f32(0)
    for h in range(n):
        total = f32(total + f32(losses[2 * h] + losses[2 * h + 1]))
    losses[-1] = total
    l64[-1] = l64[:-1].sum()
    chan64 = np.asarray(chan64)
    return dict(losses=losses, losses64=l64, chan=chan64.astype(f32), chan64=chan64, num_pos=num_pos, num=num)


def backward(preds, targets, head_order, weights, fwd, grad_losses=None, grad_chan=None):
    """Gradients for the upstream gradients of `losses` (default: 1 on the total) and `chan` (default 0), float32 as the
    kernels read them.  -> (hm_grads64: per head the fp64 heat-map gradient before its one rounding,
    reg_grads: per head {name: float32 map}, bit-defined)."""
    n = len(preds)
    if grad_losses is None:
        grad_losses = np.zeros(2 * n + 1, f32)
        grad_losses[-1] = 1
    gl = np.asarray(grad_losses, f32).astype(np.float64)
    cw, lw, code_w = float(weights['cls_weight']), float(weights['loc_weight']), [float(w) for w in weights['code_weights']]
    hm_grads, reg_grads = [], []
    for h, d in enumerate(preds):
        g = np.asarray(targets['heatmaps'][h], f32)
        s, p32 = _sigmoid(d['hm'])
        s32 = s.astype(f32)
        p, g64 = p32.astype(np.float64), g.astype(np.float64)
        up = gl[2 * h] + gl[-1]
        scale = -(up * cw) / fwd['num_pos'][h] if fwd['num_pos'][h] > 0 else -(up * cw)
        q = 1 - p
        w = (1 - g64) * (1 - g64)
        with np.errstate(divide='ignore', invalid='ignore'):
            dt = np.where(g == f32(1), q * q / p - 2.0 * q * np.log(p),
                          np.where(g < f32(1), (w * w) * (2.0 * p * np.log(q) - p * p / q), 0.0))
        grad = scale * dt * (s * (1 - s))
        grad[~((s32 >= P_MIN) & (s32 <= P_MAX))] = 0.0
        grad[~((g == f32(1)) | (g < f32(1)))] = 0.0
        hm_grads.append(grad)
        # regression maps
        pred = _stack(d, head_order)
        B, D = pred.shape[:2]
        target = np.asarray(targets['target_boxes'][h], f32)
        ind = np.asarray(targets['inds'][h])
        valid, at, use = _slots(pred, target, ind, targets['masks'][h])
        up = gl[2 * h + 1] + gl[-1]
        den = max(fwd['num'][h], 1.0)
        gc = np.zeros(D) if grad_chan is None else np.asarray(grad_chan, f32)[h].astype(np.float64)
        sc = np.asarray([(up * lw * code_w[k] + gc[k]) / den for k in range(D)]).astype(f32)
        out = np.zeros(pred.shape, f32).reshape(B, D, -1)
        with np.errstate(invalid='ignore'):
            diff = at - np.where(use, target, 0).astype(f32)
        sgn = ((diff > 0).astype(f32) - (diff < 0).astype(f32))
        for b in range(B):
            for k in np.flatnonzero(valid[b]):                   # ascending slot order; float32 adds
                for c in range(D):
                    if use[b, k, c]:
                        out[b, c, ind[b, k]] = f32(out[b, c, ind[b, k]] + f32(sgn[b, k, c] * sc[c]))
        out = out.reshape(pred.shape)
        maps, c0 = {}, 0
        for key in head_order:
            maps[key] = out[:, c0:c0 + d[key].shape[1]]
            c0 += d[key].shape[1]
        reg_grads.append(maps)
    return hm_grads, reg_grads


def at_slots(grad_maps, head_order, ind):
    """The regression gradient maps of a head gathered at every slot's cell: (B, K, D)."""
    g = _stack(grad_maps, head_order)
    B, D = g.shape[:2]
    return np.take_along_axis(g.reshape(B, D, -1), np.asarray(ind)[:, None, :].repeat(D, 1), axis=2).transpose(0, 2, 1)


def ulp32(v):
    """The float32 step at |v| (arrays or scalars), as float64."""
    return np.spacing(np.abs(np.asarray(v, f32))).astype(np.float64)


# How far the reference's float32 arithmetic may be from the contract's fp64 values (a bound on d_ref, from the number
# formats, not from a measurement).  A loss: every term of a sum has one sign and carries at most 8 float32 roundings
# (sigmoid, log, 1 - p, two squares, three products): 4 steps relative; a pairwise float32 sum of N <= 2^18 terms adds at
# most log2(N) / 2 = 9 steps; the division, the weights and the additions of the parts 3 more: 16 steps of the loss.
LOSS_STEPS = 16


def hm_grad_bound(x, value):
    """Bound on |reference float32 heat-map gradient - contract fp64 gradient| of an element with logit x.  Three sources,
    all from the float32 format.  (1) Autograd forms the gradient from about a dozen float32 operations: 8 steps relative.
    (2) torch's float32 sigmoid is exp, add and divide, each within a step, so y = sigmoid(x) may be 4 half-steps
    (4 * 2^-24 relative) from the correctly rounded value the contract clamps.  y enters 1 - y twice, in the sigmoid
    backward's y (1 - y) and as p in the terms' (1 - p), and an error e in y is a relative error e y / (1 - y) of
    1 - y: 8 * 2^-24 y / (1 - y) together.  (3) The reference takes log(1 - p) of the float32 difference 1 - p, which is
    rounded to half a step of 1: an absolute error of 2^-24 in a logarithm of size about p, a relative error of 2^-24 / p
    in the negative term, where the contract's fp64 1 - p is exact.  With the clamp at 1e-4 and 1 - 1e-4 the last two are
    at most 8e4 * 2^-24 and 1e4 * 2^-24."""
    s = 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))
    p = np.minimum(np.maximum(s.astype(f32), P_MIN), P_MAX).astype(np.float64)
    return np.abs(value) * (8 * 2.0 ** -23 + 2.0 ** -24 * (8 * s / (1 - s) + 1 / p)) + np.finfo(f32).tiny
