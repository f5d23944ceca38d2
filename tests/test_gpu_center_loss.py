"""The CenterHead loss on the GPU (csrc/centerloss_stage.hip through center_loss_ops, loss_utils and CenterHead.get_loss)
against the NumPy restatement (tests/center_loss_ref.py) and golden G14.

Bounds.  The kernels evaluate the contract's fp64 formulas and round once, as the restatement does; the only freedom is
the order of the fp64 sums and the last bit of exp / log, both far below half a float32 step, so a loss or a heat-map
gradient is within ONE float32 step of the restatement.  The regression gradients are sums of +-s_d in a fixed order:
bit-equal.  Against G14 the bound is that output's d_ref (reference to restatement, measured at capture) plus that step."""
import numpy as np
import pytest

from tests import center_loss_ref as R
from tests.test_gpu_center_head import make_head
from tests.test_oracle_center_loss import g14  # noqa: F401

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def to_dev(preds, grad=True):
    torch = _torch()
    return [{k: torch.from_numpy(v).cuda().requires_grad_(grad) for k, v in d.items()} for d in preds]


def targets_dev(targets):
    torch = _torch()
    return {k: [torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in v] for k, v in targets.items()}


def loss_head(name, **over):
    case = R.CASES[name]
    head = make_head(case['cfg'])
    head.model_cfg['LOSS_CONFIG'] = dict(LOSS_WEIGHTS=dict(case['weights'], **over))
    return head


def within(a, b, steps=1, extra=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.abs(a - b) <= extra + steps * R.ulp32(b)).all())


@pytest.fixture(scope="module")
def cases(g14):  # noqa: F811
    """Per G14 case: targets, generated predictions, the restatement's forward and backward -- computed once."""
    g, _ = g14
    out = {}
    for name, case in R.CASES.items():
        targets = R.unpack_targets(name, g)
        preds = R.predictions(name, targets)
        fwd = R.forward(preds, targets, case['head_order'], case['weights'])
        out[name] = (targets, preds, fwd) + R.backward(preds, targets, case['head_order'], case['weights'], fwd)
    return out


def run_head(name, targets, preds, scale=None):
    head = loss_head(name)
    dev = to_dev(preds)
    loss, tb = head.get_loss(dev, targets_dev(targets), as_tensors=True)
    (loss if scale is None else scale * loss).backward()
    n = len(preds)
    losses = np.asarray([tb[k % h].item() for h in range(n) for k in ('hm_loss_head_%d', 'loc_loss_head_%d')] + [tb['rpn_loss'].item()],
                        np.float32)
    assert loss.dim() == 0 and loss.item() == tb['rpn_loss'].item()
    return losses, [{k: v.grad.cpu().numpy() for k, v in d.items()} for d in dev]


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_forward_and_backward_on_g14(g14, cases, name):  # noqa: F811
    g, _ = g14
    targets, preds, fwd, hm64, reg = cases[name]
    order = R.CASES[name]['head_order']
    losses, grads = run_head(name, targets, preds)
    print(name, 'losses', losses, 'restated', fwd['losses'], 'g14', g[name + '_losses'])
    assert within(losses, fwd['losses'])
    assert within(losses, g[name + '_losses'], extra=g[name + '_d_losses'])
    for h in range(len(preds)):
        mine = grads[h]['hm']
        want = hm64[h].astype(np.float32)
        print(name, h, 'hm grad max step', (np.abs(mine.astype(np.float64) - want) / R.ulp32(want)).max())
        assert within(mine, want)
        s = 1.0 / (1.0 + np.exp(-preds[h]['hm'].astype(np.float64)))
        clamped = (s.astype(np.float32) < R.P_MIN) | (s.astype(np.float32) > R.P_MAX)
        assert clamped.any() or name == 'C'
        assert not mine[clamped].any()
        idx = g['%s_h%d_hm_grad_idx' % (name, h)]
        assert within(mine.reshape(-1)[idx], g['%s_h%d_hm_grad_val' % (name, h)], extra=g['%s_h%d_hm_grad_d' % (name, h)])
        for key in order:                                    # every cell of every map: targets and zeroes alike
            assert np.array_equal(grads[h][key].view(np.uint32), np.ascontiguousarray(reg[h][key]).view(np.uint32)), (h, key)
        at = R.at_slots(grads[h], order, targets['inds'][h])
        assert within(at, g['%s_h%d_reg_grad' % (name, h)], extra=g[name + '_d_reg_grad'][h])


def random_case(seed, n_cls, B, H, W, n_max, full_same_ind=False, empty=False):
    """Targets and predictions made here: heat maps with ones, zeros, values in between and one value a step below 1;
    slots valid at random (none if `empty`, all with one ind if `full_same_ind`), a NaN target."""
    rs = np.random.RandomState(seed)
    order = ['center', 'center_z', 'dim', 'rot']
    targets = {'heatmaps': [], 'target_boxes': [], 'inds': [], 'masks': []}
    preds = []
    for c in n_cls:
        heat = np.where(rs.uniform(size=(B, c, H, W)) < 0.3, rs.uniform(size=(B, c, H, W)), 0).astype(np.float32)
        if not empty:
            heat[rs.uniform(size=heat.shape) < 0.1] = 1
            heat.reshape(-1)[0] = np.nextafter(np.float32(1), np.float32(0))
        mask = (rs.uniform(size=(B, n_max)) < 0.6).astype(np.int64)
        ind = rs.randint(0, H * W, (B, n_max)).astype(np.int64)
        if full_same_ind:
            mask[:], ind[:] = 1, (H * W) // 2
        if empty:
            mask[:] = 0
            heat[heat == 1] = 0.5
        tb = rs.uniform(-2, 2, (B, n_max, 8)).astype(np.float32)
        tb[0, 0, 3] = np.nan
        targets['heatmaps'].append(heat)
        targets['target_boxes'].append(tb)
        targets['inds'].append(ind)
        targets['masks'].append(mask)
        d = {'hm': rs.normal(-1, 4, (B, c, H, W)).astype(np.float32)}
        for key in order:
            d[key] = rs.uniform(-2, 2, (B, R.CHANNELS[key], H, W)).astype(np.float32)
        preds.append(d)
    return targets, preds, order


EDGES = [dict(hw=(1, 1)), dict(hw=(5, 7)), dict(hw=(7, 9)), dict(hw=(8, 8)), dict(hw=(5, 13)), dict(hw=(17, 241)),
         dict(hw=(8, 8), empty=True), dict(hw=(7, 9), full_same_ind=True, n_max=1024), dict(hw=(5, 13), B=3, scale=2.5)]


@pytest.mark.parametrize("edge", EDGES, ids=lambda e: "-".join("%s%s" % kv for kv in e.items()))
def test_edges_against_the_restatement(edge):
    """H * W in {1, 35, 63, 64, 65, 4097} (vector body and scalar tail), one and three classes, B = 1, every head empty,
    all 1024 slots valid on one cell, a heat value one step below 1, an upstream gradient of 2.5."""
    from dfu3d_amd import center_loss_ops
    torch = _torch()
    H, W = edge['hw']
    B, scale = edge.get('B', 1), edge.get('scale', 1.0)
    targets, preds, order = random_case(H * W + B, [1, 3], B, H, W, edge.get('n_max', 6),
                                        edge.get('full_same_ind', False), edge.get('empty', False))
    weights = dict(cls_weight=0.5, loc_weight=0.25, code_weights=[1.0, 1.0, 0.5, 2.0, 2.0, 2.0, 0.25, 0.25])
    fwd = R.forward(preds, targets, order, weights)
    up = np.zeros(5, np.float32)
    up[-1] = scale
    hm64, reg = R.backward(preds, targets, order, weights, fwd, grad_losses=up)
    dev, tg = to_dev(preds), targets_dev(targets)
    losses, _ = center_loss_ops.center_loss([d['hm'] for d in dev], tg['heatmaps'], [[d[k] for k in order] for d in dev],
                                            tg['target_boxes'], tg['inds'], tg['masks'], **weights)
    (scale * losses[-1]).backward()
    got = losses.detach().cpu().numpy()
    print(edge, got, fwd['losses'])
    assert np.isfinite(got).all() and within(got, fwd['losses'])
    if edge.get('empty'):
        assert not fwd['num'].any() and not fwd['num_pos'].any() and not got[1::2][:2].any()
    for h in range(2):
        assert within(dev[h]['hm'].grad.cpu().numpy(), hm64[h].astype(np.float32)), h
        for key in order:
            assert np.array_equal(dev[h][key].grad.cpu().numpy().view(np.uint32), np.ascontiguousarray(reg[h][key]).view(np.uint32)), (h, key)
    if edge.get('full_same_ind'):
        assert np.count_nonzero(dev[0]['dim'].grad.cpu().numpy()) <= 3 * B


def test_two_runs_give_the_same_bits(cases):
    targets, preds = cases['A'][:2]
    l0, g0 = run_head('A', targets, preds)
    l1, g1 = run_head('A', targets, preds)
    assert np.array_equal(l0.view(np.uint32), l1.view(np.uint32))
    for a, b in zip(g0, g1):
        for key in a:
            assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


def test_no_host_contact_from_assign_to_backward(cases):
    torch = _torch()
    targets, preds = cases['A'][:2]
    head = loss_head('A')
    gt = torch.from_numpy(R.scene('A')).cuda()
    dev = to_dev(preds)
    H, W = R.CASES['A']['cfg']['map_hw']
    head.get_loss(to_dev(preds), targets_dev(targets), as_tensors=True)[0].backward()      # library and kernels loaded
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        head.forward_ret_dict = {'pred_dicts': dev, 'target_dicts': head.assign_targets(gt, feature_map_size=[H, W])}
        loss, tb = head.get_loss(as_tensors=True)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in tb.values())
    hm_before = [d['hm'].detach().clone() for d in dev]
    loss2, floats = head.get_loss()
    assert sorted(floats) == sorted(tb) == sorted(['hm_loss_head_%d' % h for h in range(6)] + ['loc_loss_head_%d' % h for h in range(6)]
                                                  + ['rpn_loss'])
    assert all(isinstance(v, float) for v in floats.values())
    assert {k: v.item() for k, v in tb.items()} == floats and loss2.item() == floats['rpn_loss']
    assert all(torch.equal(a, d['hm']) for a, d in zip(hm_before, dev))                    # the logits are not overwritten


def composition(pred_dicts, tg, order, weights, dtype):
    """The contract's formulas as plain torch operations in `dtype`."""
    torch = _torch()
    total = 0
    for h, d in enumerate(pred_dicts):
        g = tg['heatmaps'][h].to(dtype)
        p = torch.clamp(torch.sigmoid(d['hm']), min=1e-4, max=1 - 1e-4)
        pos, neg = g.eq(1).to(dtype), g.lt(1).to(dtype)
        s = (torch.log(p) * (1 - p) ** 2 * pos).sum() + (torch.log(1 - p) * p ** 2 * (1 - g) ** 4 * neg).sum()
        n_pos = pos.sum()
        total = total + weights['cls_weight'] * (-s / torch.clamp_min(n_pos, 1.0))
        pred = torch.cat([d[k] for k in order], 1)
        B, D = pred.shape[:2]
        at = pred.reshape(B, D, -1).gather(2, tg['inds'][h][:, None, :].expand(-1, D, -1)).transpose(1, 2)
        t = tg['target_boxes'][h].to(dtype)
        use = (tg['masks'][h] != 0)[:, :, None] & ~torch.isnan(t)
        diff = torch.where(use, (at - torch.where(use, t, torch.zeros_like(t))).abs(), torch.zeros_like(t))
        chan = diff.sum((0, 1)) / torch.clamp_min((tg['masks'][h] != 0).sum().to(dtype), 1.0)
        total = total + weights['loc_weight'] * (chan * torch.tensor(weights['code_weights'], dtype=dtype, device=chan.device)).sum()
    return total


def test_module_level_and_standalone_losses(cases):
    """A shared conv and separate conv heads for case B through get_loss: the parameter gradients' distance from a
    float64 torch composition is at most four times the float32 composition's own distance (conv rounding dominates
    both).  FocalLossCenterNet / RegLossCenterNet alone equal head 0's parts."""
    import torch.nn as nn
    from dfu3d_amd import center_loss_ops
    from dfu3d_amd.pcdet_kitti import loss_utils
    torch = _torch()
    targets, preds = cases['B'][:2]
    case = R.CASES['B']
    order, weights = case['head_order'], case['weights']
    tg = targets_dev(targets)
    H, W = case['cfg']['map_hw']

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.shared = nn.Sequential(nn.Conv2d(6, 8, 3, padding=1), nn.ReLU())
            self.heads = nn.ModuleList([nn.ModuleDict({k: nn.Conv2d(8, c, 3, padding=1) for k, c in
                                                       [('hm', len(names))] + [(k, R.CHANNELS[k]) for k in order]})
                                        for names in case['cfg']['heads']])

        def forward(self, x):
            x = self.shared(x)
            return [{k: conv(x) for k, conv in head.items()} for head in self.heads]
    torch.manual_seed(14)
    net = Net().cuda()
    x = torch.randn(case['B'], 6, H, W, device='cuda')
    runs = {}
    for tag in ('hip', 'f32', 'f64'):
        m = Net().cuda()
        m.load_state_dict(net.state_dict())
        if tag == 'f64':
            m = m.double()
        out = m(x.double() if tag == 'f64' else x)
        if tag == 'hip':
            loss, _ = loss_head('B').get_loss(out, tg, as_tensors=True)
        else:
            loss = composition(out, tg, order, weights, torch.float64 if tag == 'f64' else torch.float32)
        loss.backward()
        runs[tag] = (loss.item(), [p.grad.double().cpu().numpy() for p in m.parameters()])
    print('module losses', {k: v[0] for k, v in runs.items()})
    for i, ref in enumerate(runs['f64'][1]):
        d_hip, d_f32 = np.abs(runs['hip'][1][i] - ref).max(), np.abs(runs['f32'][1][i] - ref).max()
        print('param', i, 'hip', d_hip, 'f32', d_f32)
        assert d_hip <= 4 * d_f32 + np.finfo(np.float32).tiny, (i, d_hip, d_f32)
    # standalone modules: one head of the same kernels with unit weights
    dev = to_dev(preds, grad=False)
    unit = dict(cls_weight=1.0, loc_weight=1.0, code_weights=[1.0] * 10)
    losses, chan = center_loss_ops.center_loss([d['hm'] for d in dev], tg['heatmaps'], [[d[k] for k in order] for d in dev],
                                               tg['target_boxes'], tg['inds'], tg['masks'], **unit)
    x0 = dev[0]['hm'].clone().requires_grad_()
    focal = loss_utils.FocalLossCenterNet()(x0, tg['heatmaps'][0])
    assert focal.dim() == 0 and focal.item() == losses[0].item()
    (3.0 * focal).backward()
    head0 = {k: v[:1] for k, v in targets.items()}
    np0 = [preds[0]]
    fwd0 = R.forward(np0, head0, order, unit)
    hm64, _ = R.backward(np0, head0, order, unit, fwd0, grad_losses=np.asarray([3, 0, 0], np.float32))
    assert within(x0.grad.cpu().numpy(), hm64[0].astype(np.float32))
    stacked = torch.cat([dev[0][k] for k in order], 1).requires_grad_()
    reg = loss_utils.RegLossCenterNet()(stacked, tg['masks'][0], tg['inds'][0], tg['target_boxes'][0])
    assert tuple(reg.shape) == (10,) and torch.equal(reg, chan[0])
    (reg * torch.arange(1.0, 11.0, device='cuda')).sum().backward()
    _, rg = R.backward(np0, head0, order, unit, fwd0, grad_losses=np.zeros(3, np.float32),
                       grad_chan=np.arange(1, 11, dtype=np.float32)[None])
    want = np.concatenate([rg[0][k] for k in order], 1)
    assert np.array_equal(stacked.grad.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32))


def test_refusals_launch_nothing(cases):
    from dfu3d_amd._lib import Dfu3dError
    from dfu3d_amd.pcdet_kitti import loss_utils
    torch = _torch()
    targets, preds = cases['C'][:2]
    tg, dev = targets_dev(targets), to_dev(preds, grad=False)
    head = loss_head('C')
    half = [dict(dev[0], hm=dev[0]['hm'].half())]
    with pytest.raises(Dfu3dError, match="float32"):
        head.get_loss(half, tg)
    with pytest.raises(NotImplementedError, match="IoU"):
        head.get_loss([dict(dev[0], iou=dev[0]['center_z'])], tg)
    head.model_cfg['IOU_REG_LOSS'] = True
    with pytest.raises(NotImplementedError, match="IoU"):
        head.get_loss(dev, tg)
    with pytest.raises(NotImplementedError, match="mask"):
        loss_utils.FocalLossCenterNet()(dev[0]['hm'], tg['heatmaps'][0], mask=torch.ones(1, 5, 7, device='cuda'))
    with pytest.raises(NotImplementedError, match="ind=None"):
        loss_utils.RegLossCenterNet()(dev[0]['dim'], tg['masks'][0], None, tg['target_boxes'][0])


def test_per_head_and_per_channel_upstream_gradients(cases):
    """Every entry of both outputs gets an upstream gradient of its own: the per-head entries of `losses`, the total and
    every (head, channel) of `chan` reach the right map with the right scale."""
    from dfu3d_amd import center_loss_ops
    torch = _torch()
    targets, preds = cases['B'][:2]
    case = R.CASES['B']
    order, weights = case['head_order'], case['weights']
    up = np.asarray([0.5, -2.0, 3.0, 0.25, 1.5], np.float32)
    gc = (np.arange(20, dtype=np.float32).reshape(2, 10) - 7) / 4
    fwd = R.forward(preds, targets, order, weights)
    hm64, reg = R.backward(preds, targets, order, weights, fwd, grad_losses=up, grad_chan=gc)
    dev, tg = to_dev(preds), targets_dev(targets)
    losses, chan = center_loss_ops.center_loss([d['hm'] for d in dev], tg['heatmaps'], [[d[k] for k in order] for d in dev],
                                               tg['target_boxes'], tg['inds'], tg['masks'], **weights)
    assert within(chan.detach().cpu().numpy(), fwd['chan'])
    ((losses * torch.from_numpy(up).cuda()).sum() + (chan * torch.from_numpy(gc).cuda()).sum()).backward()
    for h in range(2):
        assert within(dev[h]['hm'].grad.cpu().numpy(), hm64[h].astype(np.float32)), h
        for key in order:
            assert np.array_equal(dev[h][key].grad.cpu().numpy().view(np.uint32), np.ascontiguousarray(reg[h][key]).view(np.uint32)), (h, key)


def test_same_bits_for_any_alignment_of_the_maps(cases):
    """Logits, heat map and a regression map as contiguous views 4 bytes into their storage (no 16-byte loads possible):
    the partition of the sums does not depend on alignment, so losses and gradients are the bits of the aligned run."""
    from dfu3d_amd import center_loss_ops
    torch = _torch()
    targets, preds = cases['C'][:2]
    order, weights = R.CASES['C']['head_order'], R.CASES['B']['weights']
    weights = dict(weights, code_weights=weights['code_weights'][:8])
    big = random_case(77, [3], 2, 17, 241, 6)                                       # 3 * 2 * 4097 elements: body and tail
    for targets, preds in ((targets, preds), big[:2]):
        runs = []
        for shift in (0, 1):
            def shifted(a, grad):
                buf = torch.zeros(a.size + shift, dtype=torch.float32, device='cuda')
                buf[shift:] = torch.from_numpy(a).cuda().reshape(-1)
                buf.requires_grad_(grad)
                v = buf[shift:].view(a.shape)
                assert v.is_contiguous() and (v.data_ptr() % 16 == 0) == (shift == 0)
                return buf, v
            leaves = [{k: shifted(v, True) for k, v in d.items()} for d in preds]
            heats = [shifted(t, False)[1] for t in targets['heatmaps']]
            tg = targets_dev(targets)
            losses, _ = center_loss_ops.center_loss([d['hm'][1] for d in leaves], heats, [[d[k][1] for k in order] for d in leaves],
                                                    tg['target_boxes'], tg['inds'], tg['masks'], **weights)
            losses[-1].backward()
            runs.append((losses.detach().cpu().numpy(), [{k: d[k][0].grad[shift:].cpu().numpy() for k in d} for d in leaves]))
        assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
        for a, b in zip(runs[0][1], runs[1][1]):
            for key in a:
                assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key


def test_an_input_overwritten_before_backward_raises(cases):
    """The backward recomputes from the inputs, which are saved through autograd: an in-place write between forward and
    backward is an error, not the gradient of other values."""
    torch = _torch()
    targets, preds = cases['C'][:2]
    dev = to_dev(preds)
    hm = dev[0]['hm'] * 1.0
    loss, _ = loss_head('C').get_loss([dict(dev[0], hm=hm)], targets_dev(targets), as_tensors=True)
    hm.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()


def test_launch_counts(cases, monkeypatch):
    """In the build that counts every kernel launch of the library: 3 forward and 2 backward for one head and for six."""
    import ctypes
    from dfu3d_amd import _lib, _lib_head
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib_head, "_BOUND", _lib_head.bind(L))
    for name in ('C', 'A'):
        targets, preds = cases[name][:2]
        dev, tg = to_dev(preds), targets_dev(targets)
        head = loss_head(name)
        L.dfu3d_debug_launch_count(1)
        loss, _ = head.get_loss(dev, tg, as_tensors=True)
        fwd = int(L.dfu3d_debug_launch_count(1))
        loss.backward()
        bwd = int(L.dfu3d_debug_launch_count(1))
        assert (fwd, bwd) == (3, 2), (name, fwd, bwd)
        assert within(loss.item(), cases[name][2]['losses'][-1])
