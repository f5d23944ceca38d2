"""The fused optimiser step and the training surface without a GPU: the agreement of include/dfu3d_opt.h with its binding,
host-side argument validation before any launch, the schedules and the grouping against golden G17, the NumPy restatement
of the numerics contract against the reference's parameters, and the state dict both ways with torch.optim.Adam."""
import ctypes
import os
import re

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_opt
from tests import adam_step_ref as R
from tests import optimizer_cases as K

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch


@pytest.fixture(scope="module")
def G():
    return K.golden()


def test_header_and_binding_agree():
    assert _lib_opt.HEADER == os.path.join(_build.INCLUDE, "dfu3d_opt.h") and _lib_opt.HEADER in _build._deps()
    assert _lib_opt.header_symbols() == ['dfu3d_adam_step', 'dfu3d_opt_scratch_bytes', 'dfu3d_opt_version']
    L = _lib_opt.lib()
    assert L.dfu3d_opt_version() == _lib_opt.header_version() == 1
    text = open(_lib_opt.HEADER).read()
    proto = re.search(r"int dfu3d_adam_step\((.*?)\);", text, re.S).group(1)
    res, args = _lib_opt.SIGNATURES['dfu3d_adam_step']
    assert res is ctypes.c_int32 and len(args) == len(proto.split(",")) == 16
    assert args[4:12] == [ctypes.c_double] * 8 and args[1] is args[3] is ctypes.c_int32
    assert _lib_opt.SIGNATURES['dfu3d_opt_scratch_bytes'] == (ctypes.c_int64, [ctypes.c_int64])
    C = _lib_opt.CONSTANTS
    assert all(k.startswith("DFU3D_OPT_") for k in C)
    assert (C['DFU3D_OPT_CHUNK'], C['DFU3D_OPT_THREADS'], C['DFU3D_OPT_ST_NONFINITE']) == (4096, 256, 1)
    assert C['DFU3D_OPT_LAUNCHES'] in (2, 3)
    # the record layouts the Python side fills by hand
    T, Ck = _lib_opt.STRUCTS['dfu3d_opt_tensor'], _lib_opt.STRUCTS['dfu3d_opt_chunk']
    assert ctypes.sizeof(T) == 40 and [f[0] for f in T._fields_] == ['param', 'grad', 'exp_avg', 'exp_avg_sq', 'n']
    assert [T.param.offset, T.grad.offset, T.exp_avg.offset, T.exp_avg_sq.offset, T.n.offset] == [0, 8, 16, 24, 32]
    assert ctypes.sizeof(Ck) == 8 and (Ck.tensor.offset, Ck.start.offset) == (0, 4)
    assert not set(_lib_opt.SIGNATURES) & set(_lib.SIGNATURES)
    # the other headers do not know this one, and dfu3d.h is what it was
    for other in ("dfu3d.h", "dfu3d_vfe.h", "dfu3d_head.h", "dfu3d_post.h", "dfu3d_aug.h", "dfu3d_bev.h"):
        assert "dfu3d_opt" not in open(os.path.join(_build.INCLUDE, other)).read()
    assert len(_lib.SIGNATURES) == 46
    from dfu3d_amd import optim_ops
    assert (optim_ops.CHUNK, optim_ops.ST_NONFINITE, optim_ops.TENSOR_WORDS) == (4096, 1, 5)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
        dfu3d_opt_version = object()
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_adam_step, dfu3d_opt_scratch_bytes"):
        _lib_opt.bind(Fake())


def _step(L, table=P16, n_tensors=2, chunks=P16, n_chunks=3, lr=1e-3, beta1=0.9, beta2=0.99, eps=1e-8, wd=0.01, max_norm=10.0,
          bc1=0.1, bc2=0.01, scratch=P16, out=P16, status=P16):
    return L.dfu3d_adam_step(table, n_tensors, chunks, n_chunks, lr, beta1, beta2, eps, wd, max_norm, bc1, bc2, scratch, out,
                             status, None)


def test_bad_arguments_return_before_any_launch():
    L = _lib_opt.lib()
    EINVAL = _lib.CONSTANTS["DFU3D_EINVAL"]
    C = _lib_opt.CONSTANTS
    nan, inf = float('nan'), float('inf')
    bad = [dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=nan), dict(max_norm=inf), dict(lr=-1e-9), dict(lr=nan),
           dict(lr=inf), dict(beta1=-0.1), dict(beta1=1.0), dict(beta1=nan), dict(beta2=1.0), dict(beta2=-1e-3), dict(beta2=nan),
           dict(bc1=0.0), dict(bc1=1.0000001), dict(bc1=nan), dict(bc2=0.0), dict(bc2=-0.5), dict(bc2=1.5), dict(bc2=nan),
           dict(eps=-1.0), dict(eps=nan), dict(wd=nan), dict(wd=inf),
           dict(n_tensors=0), dict(n_tensors=-1), dict(n_tensors=C['DFU3D_OPT_MAX_TENSORS'] + 1),
           dict(n_chunks=0), dict(n_chunks=-1), dict(n_chunks=C['DFU3D_OPT_MAX_CHUNKS'] + 1),
           dict(table=None), dict(chunks=None), dict(scratch=None), dict(out=None), dict(status=None),
           dict(table=ctypes.c_void_p(20)), dict(chunks=ctypes.c_void_p(20)), dict(scratch=ctypes.c_void_p(20)),
           dict(out=ctypes.c_void_p(20)), dict(status=ctypes.c_void_p(18))]
    for kw in bad:
        assert _step(L, **kw) == EINVAL, kw


def test_scratch_bytes_at_its_limits():
    L = _lib_opt.lib()
    MAX = _lib_opt.CONSTANTS['DFU3D_OPT_MAX_CHUNKS']
    assert L.dfu3d_opt_scratch_bytes(0) == -1 and L.dfu3d_opt_scratch_bytes(-5) == -1
    assert L.dfu3d_opt_scratch_bytes(MAX + 1) == -1 and L.dfu3d_opt_scratch_bytes(1 << 40) == -1
    assert L.dfu3d_opt_scratch_bytes(1) == 8 and L.dfu3d_opt_scratch_bytes(MAX) == 8 * MAX


def test_chunk_map():
    from dfu3d_amd import optim_ops
    m = optim_ops.chunk_map([1, 4096, 4097, 8199])
    assert m.dtype == np.int32 and m.tolist() == [[0, 0], [1, 0], [2, 0], [2, 4096], [3, 0], [3, 4096], [3, 8192]]


class _Hyper:
    lr = mom = 0


def test_schedules_equal_the_reference(G):
    from dfu3d_amd.train_utils.optimization.learning_schedules_fastai import CosineAnnealing, OneCycle
    moms, div = list(K.OPTIMIZATION['MOMS']), K.OPTIMIZATION['DIV_FACTOR']
    for total, pct in K.ONE_CYCLE:
        h = _Hyper()
        s = OneCycle(h, total, K.LR, moms, div, pct)
        assert (h.lr, h.mom) == (K.LR / div, moms[0])
        for i in range(total):
            s.step(i)
            assert float(h.lr) == G['onecycle_%d_lr' % total][i] and float(h.mom) == G['onecycle_%d_mom' % total][i], (total, i)
    # the truncated border: 7 * 0.4 = 2.8 -> the second phase starts at step 2
    assert [p[:2] for p in OneCycle(_Hyper(), 7, K.LR, moms, div, 0.4).lr_phases] == [(0, 2), (2, 7)]
    c = K.COSINE
    h = _Hyper()
    s = CosineAnnealing(h, c['total_step'], c['total_epoch'], K.LR, moms, c['pct_start'], c['warmup_iter'])
    for i in range(c['total_step']):
        s.step(i, i // c['iters_per_epoch'])
        assert float(h.lr) == G['cosine_lr'][i] and float(h.mom) == G['cosine_mom'][i], i


def _optimizer(G, **over):
    from dfu3d_amd.train_utils.optimization import build_optimizer
    model = K.load_init(K.case_model(), G)
    return model, build_optimizer(model, K.optim_cfg(**over))


def test_grouping_and_order_equal_the_reference(G):
    import json
    from dfu3d_amd.train_utils.optimization.fastai_optim import OptimWrapper
    meta = json.loads(bytes(G['meta']).decode())
    model, opt = _optimizer(G)                                           # construction needs no GPU
    assert isinstance(opt, OptimWrapper)
    names = {id(p): n for n, p in model.named_parameters()}
    assert [[names[id(p)] for p in g['params']] for g in opt.param_groups] == meta['group_names'] == K.GROUP_NAMES
    assert [len(g['params']) for g in opt.param_groups] == [5, 4] and len(opt.params) == 9
    assert opt.names == [n for g in K.GROUP_NAMES for n in g]
    assert sorted(p.numel() for p in opt.params)[-1] == 5125
    assert (opt.lr, opt.mom, opt.beta, opt.wd, opt.max_norm) == (3e-3, 0.9, 0.99, 0.01, 10.0)
    opt.lr, opt.mom = 1e-4, 0.95
    assert all(g['lr'] == 1e-4 and g['betas'] == (0.95, 0.99) and g['weight_decay'] == 0 for g in opt.param_groups)
    _, opt2 = _optimizer(G, BETAS=[0.8, 0.9], GRAD_NORM_CLIP=35)
    assert (opt2.mom, opt2.beta, opt2.max_norm) == (0.8, 0.9, 35.0)
    # a frozen parameter is in no group
    model = K.case_model()
    model[3].bias.requires_grad_(False)
    from dfu3d_amd.train_utils.optimization import build_optimizer
    assert [len(g['params']) for g in build_optimizer(model, K.optim_cfg()).param_groups] == [4, 4]


def test_centerpoint_parameters_land_in_exactly_one_group():
    import torch
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    from dfu3d_amd.train_utils.optimization import build_optimizer
    from tests import centerpoint_cases as C
    torch.manual_seed(0)
    model = CenterPoint(C.cfg(C.SMALL_MODEL), len(C.SMALL_CLASSES), **C.SMALL_DATASET)
    opt = build_optimizer(model, K.optim_cfg())
    ids = [id(p) for p in opt.params]
    assert len(set(ids)) == len(ids) and set(ids) == {id(p) for p in model.parameters()}
    bn = {id(p) for m in model.modules() if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)) for p in m.parameters()}
    assert {id(p) for p in opt.param_groups[1]['params']} == bn and bn


def test_restatement_against_the_reference(G):
    """The float32 restatement of the contract, run with the reference's schedule and gradients, against the reference's
    parameters after 1, 4 and 10 steps: within t * (2^-22 |p| + 1e-5 LR) per element."""
    from dfu3d_amd.train_utils.optimization.learning_schedules_fastai import OneCycle
    init = [G['init_%d' % i] for i in range(9)]
    shapes = [p.shape for p in init]
    worst = 0.0
    for seed in K.SEEDS:
        ref = R.RefAdam(init, weight_decay=K.OPTIMIZATION['WEIGHT_DECAY'], max_norm=K.OPTIMIZATION['GRAD_NORM_CLIP'])
        h = _Hyper()
        sched = OneCycle(h, K.RUN[0], K.LR, list(K.OPTIMIZATION['MOMS']), K.OPTIMIZATION['DIV_FACTOR'], K.RUN[1])
        clipped = []
        for it in range(K.RUN[0]):
            sched.step(it)
            ref.step(K.gradients(seed, it, shapes), float(h.lr), float(h.mom), 0.99)
            clipped.append(float(ref.coef) < 1.0)
            t = it + 1
            if t in K.SNAPSHOTS:
                assert ref.steps == G['s%d_t%d_steps' % (seed, t)].tolist() == [t] * 9
                for i in range(9):
                    want = G['s%d_t%d_p%d' % (seed, t, i)]
                    err = np.abs(ref.p[i].astype(np.float64) - want)
                    lim = K.bound(t, want.astype(np.float64))
                    worst = max(worst, float((err / lim).max()))
                    print("seed %d step %d tensor %d: worst error / bound = %.3f" % (seed, t, i, float((err / lim).max())))
                    assert (err <= lim).all(), (seed, t, i, float((err / lim).max()))
        assert any(clipped) and not all(clipped)                         # clipping on and off
    print("worst error / bound:", worst)


def test_state_dict_both_ways_with_torch_adam(G):
    import torch
    model, opt = _optimizer(G)
    groups = [list(g['params']) for g in opt.param_groups]
    adam = torch.optim.Adam([{'params': g, 'lr': 0} for g in groups], betas=(0.9, 0.99))
    for g in adam.param_groups:
        g['lr'], g['betas'] = 2e-4, (0.93, 0.99)
    rng = np.random.default_rng(5)
    for _ in range(3):
        for p in opt.params:
            p.grad = torch.from_numpy(rng.standard_normal(tuple(p.shape)).astype(np.float32))
        adam.step()
    sd = adam.state_dict()
    opt.load_state_dict(sd)                                             # torch's extra keys are ignored
    assert opt.steps == [3] * 9 and (opt.lr, opt.mom, opt.beta) == (2e-4, 0.93, 0.99)
    for i, p in enumerate(opt.params):
        assert torch.equal(opt.exp_avg[i], adam.state[p]['exp_avg']) and torch.equal(opt.exp_avg_sq[i], adam.state[p]['exp_avg_sq'])
        assert opt.exp_avg[i] is not adam.state[p]['exp_avg']
    mine = opt.state_dict()
    assert sorted(mine) == ['param_groups', 'state'] and sorted(mine['state']) == list(range(9))
    assert [g['params'] for g in mine['param_groups']] == [[0, 1, 2, 3, 4], [5, 6, 7, 8]]
    assert all(sorted(g) == ['amsgrad', 'betas', 'eps', 'lr', 'params', 'weight_decay'] for g in mine['param_groups'])
    assert all(sorted(s) == ['exp_avg', 'exp_avg_sq', 'step'] and float(s['step']) == 3.0 for s in mine['state'].values())
    # and back into a fresh Adam over the same two groups
    model2 = K.load_init(K.case_model(), G)
    named = dict(model2.named_parameters())
    adam2 = torch.optim.Adam([{'params': [named[n] for n in g], 'lr': 0} for g in K.GROUP_NAMES])
    adam2.load_state_dict(mine)
    for n, p in zip([n for g in K.GROUP_NAMES for n in g], opt.params):
        s = adam2.state[named[n]]
        assert float(s['step']) == 3.0 and torch.equal(s['exp_avg'], adam.state[p]['exp_avg'])
        assert torch.equal(s['exp_avg_sq'], adam.state[p]['exp_avg_sq'])
    assert adam2.param_groups[0]['betas'] == (0.93, 0.99) and adam2.param_groups[1]['lr'] == 2e-4
    # a fresh optimiser has no state; wrong group sizes are refused
    _, fresh = _optimizer(G)
    assert fresh.state_dict()['state'] == {}
    with pytest.raises(ValueError):
        fresh.load_state_dict({'state': {}, 'param_groups': [dict(mine['param_groups'][0], params=[0, 1])] * 2})


def test_step_refuses_host_tensors(G):
    import torch
    from dfu3d_amd._lib import Dfu3dError
    _, opt = _optimizer(G)
    for p in opt.params:
        p.grad = torch.zeros_like(p)
    opt.lr = 1e-3
    with pytest.raises(Dfu3dError, match="on the GPU"):
        opt.step()
    assert opt.steps == [0] * 9


def test_other_branches():
    import torch
    from dfu3d_amd.train_utils import train_utils as T
    from dfu3d_amd.train_utils.optimization import build_optimizer, build_scheduler
    from dfu3d_amd.train_utils.optimization.fastai_optim import OptimWrapper
    from dfu3d_amd.train_utils.optimization.learning_schedules_fastai import CosineAnnealing, CosineWarmupLR, OneCycle
    model = K.case_model()
    adam = build_optimizer(model, K.optim_cfg(OPTIMIZER='adam'))
    assert type(adam) is torch.optim.Adam and adam.defaults['lr'] == K.LR and adam.defaults['weight_decay'] == 0.01
    sgd = build_optimizer(model, K.optim_cfg(OPTIMIZER='sgd'))
    assert type(sgd) is torch.optim.SGD and sgd.defaults['momentum'] == 0.9
    with pytest.raises(NotImplementedError):
        build_optimizer(model, K.optim_cfg(OPTIMIZER='lamb'))
    one = build_optimizer(model, K.optim_cfg())
    s, w = build_scheduler(one, 10, 2, -1, K.optim_cfg())
    assert isinstance(s, OneCycle) and w is None and s.total_step == 20 and one.lr == K.LR / 10
    cos = build_optimizer(model, K.optim_cfg(OPTIMIZER='adam_cosineanneal'))
    assert isinstance(cos, OptimWrapper)
    s, w = build_scheduler(cos, 10, 2, -1, K.optim_cfg(OPTIMIZER='adam_cosineanneal', WARMUP_ITER=5))
    assert isinstance(s, CosineAnnealing) and w is None
    s, w = build_scheduler(sgd, 10, 50, -1, K.optim_cfg(OPTIMIZER='sgd', LR_WARMUP=True))
    assert isinstance(s, torch.optim.lr_scheduler.LambdaLR) and isinstance(w, CosineWarmupLR) and w.T_max == 10
    assert s.lr_lambdas[0](0) == 1 and s.lr_lambdas[0](350) == 0.1 and s.lr_lambdas[0](450) == pytest.approx(0.01)
    with pytest.raises(NotImplementedError):
        OptimWrapper([[], []], wd=0.01, true_wd=False)
    # the loop: mixed precision and DistributedDataParallel are refused before anything runs
    with pytest.raises(NotImplementedError, match="use_amp"):
        T.train_model(model, one, [], None, None, K.optim_cfg(), 0, 1, 0, 0, None, None, use_amp=True)
    with pytest.raises(NotImplementedError, match="use_amp"):
        T.train_one_epoch(model, one, [], None, None, 0, K.optim_cfg(), 0, None, 1, None, use_amp=True)

    class DDP(torch.nn.parallel.DistributedDataParallel):
        def __init__(self):                                               # no process group: the type is what is looked at
            torch.nn.Module.__init__(self)
    with pytest.raises(NotImplementedError, match="DistributedDataParallel"):
        T.train_model(DDP(), one, [], None, None, K.optim_cfg(), 0, 1, 0, 0, None, None)
    with pytest.raises(NotImplementedError, match="DistributedDataParallel"):
        T.checkpoint_state(DDP(), one, 1, 1)
    state = T.checkpoint_state(model, one, 3, 30)
    assert sorted(state) == ['epoch', 'it', 'model_state', 'optimizer_state', 'version'] and (state['epoch'], state['it']) == (3, 30)


def test_checkpoint_holds_plain_values_only(G):
    """What a schedule sets (NumPy scalars) is stored as Python floats: a checkpoint loads under torch.load's default."""
    import io
    import torch
    from dfu3d_amd.train_utils import train_utils as T
    from dfu3d_amd.train_utils.optimization import build_scheduler
    model, opt = _optimizer(G)
    sched, _ = build_scheduler(opt, 10, 1, -1, K.optim_cfg())
    sched.step(3)
    assert type(opt.lr) is float and type(opt.mom) is float and opt.lr == G['onecycle_10_lr'][3]
    assert all(type(g['lr']) is float and type(g['betas'][0]) is float for g in opt.param_groups)
    buf = io.BytesIO()
    torch.save(T.checkpoint_state(model, opt, 1, 4), buf)
    buf.seek(0)
    ck = torch.load(buf)
    assert ck['optimizer_state']['param_groups'][0]['lr'] == opt.lr and ck['it'] == 4
