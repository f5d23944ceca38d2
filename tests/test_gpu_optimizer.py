"""GPU: the fused optimiser step (csrc/optim_stage.hip) bit for bit against the NumPy restatement of its contract
(tests/adam_step_ref.py), and the OptimWrapper built on it against the reference's parameters of golden G17."""
import numpy as np
import pytest

from tests import adam_step_ref as R
from tests import optimizer_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = np.float32(-7.25e10)
EPS, WD = 1e-8, 0.01
HYPER = [(1e-4, 0.95), (7e-4, 0.9), (1e-3, 0.85)]            # (lr, mom) of the three steps
SCALES = [30.0, 1e-3, 1.0]                                   # of the gradients of the three steps


@pytest.fixture(scope="module")
def G():
    return K.golden()


class Carved:
    """Tensors of the given lengths -- parameter, gradient and both moments each -- carved from ONE device buffer with
    at least four sentinel words between any two.  Every array starts on a 16-byte boundary, except that of tensor i
    with (i + variant) % 3 == 1 the parameter, and with (i + variant) % 3 == 2 the gradient, start 4 bytes past one."""

    def __init__(self, lengths, variant, seed):
        import torch
        rng = np.random.default_rng(seed)
        n = len(lengths)
        self.lengths = lengths
        self.no_grad = {0} if n == 3 else ({3} if n == 6 else set())
        self.zero_grad = {1} if n == 3 else ({2} if n == 6 else set())
        self.where, at = {}, 4
        for i, ln in enumerate(lengths):
            for kind in "pgmv":
                shift = 1 if (kind == "p" and (i + variant) % 3 == 1) or (kind == "g" and (i + variant) % 3 == 2) else 0
                self.where[i, kind] = (at + shift, at + shift + ln)
                at = (at + shift + ln + 3) // 4 * 4 + 4
        self.host = np.full(at, SENTINEL, np.float32)
        for i, ln in enumerate(lengths):
            p = rng.standard_normal(ln).astype(np.float32)
            p[-1] = np.float32(-0.0)
            self.put(i, "p", p)
            self.put(i, "m", np.zeros(ln, np.float32))
            self.put(i, "v", np.zeros(ln, np.float32))
            self.put(i, "g", np.zeros(ln, np.float32))
        self.dev = torch.from_numpy(self.host.copy()).to(DEV)
        assert self.dev.data_ptr() % 16 == 0
        self.params = [self.view(i, "p") for i in range(n)]
        for i, p in enumerate(self.params):
            if i not in self.no_grad:
                p.grad = self.view(i, "g")
        assert self.params[(1 - variant) % 3].data_ptr() % 16 == 4 if n >= 3 else True

    def view(self, i, kind):
        a, b = self.where[i, kind]
        return self.dev[a:b]

    def get(self, i, kind):
        a, b = self.where[i, kind]
        return self.host[a:b]

    def put(self, i, kind, values):
        a, b = self.where[i, kind]
        self.host[a:b] = values

    def gradients(self, rng, scale):
        """New gradient values, on the host copy and (in place: same addresses) on the device; None where there is none."""
        import torch
        out = []
        for i, ln in enumerate(self.lengths):
            if i in self.no_grad:
                out.append(None)
                continue
            g = np.zeros(ln, np.float32) if i in self.zero_grad else rng.standard_normal(ln).astype(np.float32) * np.float32(scale)
            g[0] = np.float32(-0.0) if ln > 1 else g[0]
            self.put(i, "g", g)
            self.view(i, "g").copy_(torch.from_numpy(g))
            out.append(g)
        return out


def run_three_steps(lengths, variant, check=True):
    """-> (bits of the whole buffer after the third step, [total_norm, coef] of every step as bits)."""
    import torch
    from dfu3d_amd import optim_ops
    c = Carved(lengths, variant, seed=170 + len(lengths))
    n = len(lengths)
    fused = optim_ops.FusedAdamStep(c.params, [c.view(i, "m") for i in range(n)], [c.view(i, "v") for i in range(n)])
    ref = R.RefAdam([c.get(i, "p") for i in range(n)], eps=EPS, weight_decay=WD)
    rng = np.random.default_rng(1700 + sum(lengths))
    all_grads = [[None if g is None else g.copy() for g in c.gradients(rng, s)] for s in SCALES]
    norms = [R.total_norm(g) for g in all_grads]
    # a bound between the steps' norms: clipping on in one step and off in another
    max_norm = float(np.sqrt(max(norms) * min(norms)))
    ref.max_norm = max_norm
    norm_bits, coefs = [], []
    for t, ((lr, mom), grads) in enumerate(zip(HYPER, all_grads), 1):
        for i, g in enumerate(grads):
            if g is not None:
                c.put(i, "g", g)
                c.view(i, "g").copy_(torch.from_numpy(g))
        fused.step(lr, mom, 0.99, EPS, WD, max_norm, 1 - mom ** t, 1 - 0.99 ** t)
        out = fused.norm.cpu().numpy()
        norm_bits.append(out.view(np.uint64).copy())
        if not check:
            continue
        dev_norm, dev_coef = float(out[0]), out[1]
        assert dev_norm == pytest.approx(norms[t - 1], rel=1e-12, abs=0.0), (t, dev_norm, norms[t - 1])
        want_coef = R.coef_of(dev_norm, max_norm)
        assert np.float64(want_coef) == dev_coef, (t, dev_coef, want_coef)
        coefs.append(float(dev_coef))
        ref.step(grads, lr, mom, 0.99, coef=dev_coef)
        for i in range(n):
            c.put(i, "p", ref.p[i])
            c.put(i, "m", ref.m[i])
            c.put(i, "v", ref.v[i])
        got = c.dev.cpu().numpy()
        if not np.array_equal(got.view(np.uint32), c.host.view(np.uint32)):
            for (i, kind), (a, b) in c.where.items():
                assert R.same_bits(got[a:b], c.host[a:b]), "step %d: tensor %d (%d elements) %s differs" % (t, i, lengths[i], kind)
            raise AssertionError("step %d: a sentinel word was written" % t)
        for i in c.no_grad:                                               # decayed only: moments untouched, no step taken
            assert ref.steps[i] == 0 and not c.get(i, "m").any() and not c.get(i, "v").any()
            assert R.same_bits(c.get(i, "p"), ref.p[i])
    if check:
        assert min(coefs) < 1.0 and max(coefs) == 1.0, coefs
        assert int(fused.status.item()) == 0 and fused.uploads == 1
    return c.dev.cpu().numpy().view(np.uint32), norm_bits


@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("lengths", K.LENGTH_LISTS, ids=lambda v: "-".join(map(str, v)))
def test_three_steps_bitwise(lengths, variant):
    run_three_steps(lengths, variant)


def test_two_runs_are_bit_equal():
    a, na = run_three_steps(K.LENGTH_LISTS[-1], 0, check=False)
    b, nb = run_three_steps(K.LENGTH_LISTS[-1], 0, check=False)
    assert np.array_equal(a, b) and all(np.array_equal(x, y) for x, y in zip(na, nb))


def _plain(lengths, seed):
    """Parameters, zero moments and a FusedAdamStep over ordinary tensors."""
    import torch
    from dfu3d_amd import optim_ops
    rng = np.random.default_rng(seed)
    host = [rng.standard_normal(n).astype(np.float32) for n in lengths]
    params = [torch.from_numpy(p.copy()).to(DEV) for p in host]
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    return rng, host, params, m, v, optim_ops.FusedAdamStep(params, m, v)


def _assert_equals_ref(ref, params, m, v):
    for i, p in enumerate(params):
        assert R.same_bits(p.cpu().numpy(), ref.p[i]), i
        assert R.same_bits(m[i].cpu().numpy(), ref.m[i]) and R.same_bits(v[i].cpu().numpy(), ref.v[i]), i


def test_launch_counts(monkeypatch):
    """In the build that counts every kernel launch of the library: DFU3D_OPT_LAUNCHES per step."""
    import ctypes
    import torch
    from dfu3d_amd import _lib, _lib_opt, optim_ops
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib_opt, "_BOUND", _lib_opt.bind(L))
    rng, host, params, m, v, fused = _plain([4095, 4096, 4097], 171)
    ref = R.RefAdam(host, eps=EPS, weight_decay=WD)
    for t in (1, 2):
        grads = [rng.standard_normal(len(p)).astype(np.float32) for p in host]
        for p, g in zip(params, grads):
            p.grad = torch.from_numpy(g).to(DEV)
        torch.cuda.synchronize()
        L.dfu3d_debug_launch_count(1)
        fused.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 1 - 0.9 ** t, 1 - 0.99 ** t)
        assert int(L.dfu3d_debug_launch_count(1)) == optim_ops.LAUNCHES == _lib_opt.CONSTANTS["DFU3D_OPT_LAUNCHES"]
        ref.step(grads, 1e-3, 0.9, 0.99, coef=fused.norm.cpu().numpy()[1])
    _assert_equals_ref(ref, params, m, v)


def test_nonfinite_sets_the_status_bit():
    import torch
    from dfu3d_amd import optim_ops
    from dfu3d_amd._lib import Dfu3dError
    rng, host, params, m, v, fused = _plain([5, 4097], 172)
    grads = [rng.standard_normal(len(p)).astype(np.float32) for p in host]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g).to(DEV)
    fused.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 0.1, 0.01)
    assert int(fused.status.item()) == 0
    fused.check_status()
    params[1].grad[4096] = float('inf')
    fused.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 1 - 0.81, 1 - 0.99 ** 2)
    out = fused.norm.cpu().numpy()
    assert int(fused.status.item()) == optim_ops.ST_NONFINITE and np.isinf(out[0]) and out[1] == 0.0
    p1 = params[1].cpu().numpy()
    assert np.isnan(p1[4096]) and np.isfinite(p1[:4096]).all() and np.isfinite(params[0].cpu().numpy()).all()
    with pytest.raises(Dfu3dError, match="not finite"):
        fused.check_status()
    assert int(fused.status.item()) == 0                                  # read and cleared
    params[1].grad[4096] = float('nan')
    fused.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 1 - 0.9 ** 3, 1 - 0.99 ** 3)
    out = fused.norm.cpu().numpy()
    assert int(fused.status.item()) == optim_ops.ST_NONFINITE and np.isnan(out[0]) and np.isnan(out[1])
    assert np.isnan(params[0].cpu().numpy()).all()                        # a NaN coefficient spreads, as in the reference


def test_table_is_rebuilt_when_a_gradient_moves():
    import torch
    rng, host, params, m, v, fused = _plain([5, 4097, 64], 173)
    ref = R.RefAdam(host, eps=EPS, weight_decay=WD)
    kept = []
    for t in (1, 2, 3):
        grads = [rng.standard_normal(len(p)).astype(np.float32) for p in host]
        if t == 3:
            grads[2] = None
        for p, g in zip(params, grads):
            kept.append(p.grad)
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)   # new tensors: new addresses
        fused.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 1 - 0.9 ** t, 1 - 0.99 ** t)
        assert fused.uploads == t
        ref.step(grads, 1e-3, 0.9, 0.99, coef=fused.norm.cpu().numpy()[1])
        _assert_equals_ref(ref, params, m, v)
    # same addresses, new values: no upload
    for p in params[:2]:
        p.grad.mul_(0.5)
    fused.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 1 - 0.9 ** 4, 1 - 0.99 ** 4)
    assert fused.uploads == 3


def test_refuses_what_the_kernels_cannot_take():
    import torch
    from dfu3d_amd import optim_ops
    from dfu3d_amd._lib import Dfu3dError
    p = torch.zeros(8, device=DEV)
    z = torch.zeros_like(p)
    with pytest.raises(Dfu3dError):
        optim_ops.FusedAdamStep([p.double()], [z], [z.clone()])
    with pytest.raises(Dfu3dError):
        optim_ops.FusedAdamStep([torch.zeros(4, 4, device=DEV).t()], [torch.zeros(4, 4, device=DEV)], [torch.zeros(4, 4, device=DEV)])
    with pytest.raises(Dfu3dError):
        optim_ops.FusedAdamStep([p], [z.cpu()], [z.clone()])
    with pytest.raises(Dfu3dError):
        optim_ops.FusedAdamStep([p], [z[:4]], [z.clone()])
    f = optim_ops.FusedAdamStep([p], [z], [z.clone()])
    p.grad = torch.zeros(8, device=DEV, dtype=torch.float32)[::1]
    f.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 0.1, 0.01)
    p.grad = torch.zeros(16, device=DEV)[::2]
    with pytest.raises(Dfu3dError, match="contiguous"):
        f.step(1e-3, 0.9, 0.99, EPS, WD, 10.0, 0.19, 0.02)
    with pytest.raises(Dfu3dError):                                       # the library's own validation
        p.grad = torch.zeros(8, device=DEV)
        f.step(1e-3, 0.9, 0.99, EPS, WD, 0.0, 0.19, 0.02)


def _case_optimizer(G, state=None):
    from dfu3d_amd.train_utils.optimization import build_optimizer, build_scheduler
    model = K.load_init(K.case_model().to(DEV), G)
    if state is not None:
        model.load_state_dict(state)
    opt = build_optimizer(model, K.optim_cfg())
    sched, _ = build_scheduler(opt, K.RUN[0], 1, -1, K.optim_cfg(PCT_START=K.RUN[1]))
    return model, [p for _, p in K.ordered_params(model)], opt, sched


def _set_grads(params, seed, it):
    import torch
    for p, g in zip(params, K.gradients(seed, it, [tuple(p.shape) for p in params])):
        p.grad = torch.from_numpy(g).to(DEV)


@pytest.mark.parametrize("seed", K.SEEDS)
def test_one_cycle_run_against_the_reference(G, seed):
    model, params, opt, sched = _case_optimizer(G)
    assert len(opt.params) == len(params) and all(a is b for a, b in zip(opt.params, params))
    norms = []
    for it in range(K.RUN[0]):
        sched.step(it)
        _set_grads(params, seed, it)
        assert opt.step() is None
        norms.append(opt.last_total_norm.clone())
        t = it + 1
        if t in K.SNAPSHOTS:
            assert opt.steps == G['s%d_t%d_steps' % (seed, t)].tolist()
            for i, p in enumerate(params):
                want = G['s%d_t%d_p%d' % (seed, t, i)].astype(np.float64)
                err = np.abs(p.detach().cpu().numpy().astype(np.float64) - want)
                lim = K.bound(t, want)
                print("seed %d step %d tensor %d: worst error / bound = %.3f" % (seed, t, i, float((err / lim).max())))
                assert (err <= lim).all(), (seed, t, i, float((err / lim).max()))
    opt.check_status()
    assert opt._fused.uploads == K.RUN[0]                                 # new gradient tensors every step
    norms = [float(x) for x in norms]
    want = [R.total_norm(K.gradients(seed, it, [tuple(p.shape) for p in params])) for it in range(K.RUN[0])]
    assert norms == pytest.approx(want, rel=1e-12) and min(norms) == 0.0 and max(norms) > 10.0 > sorted(norms)[1]
    # zero_grad zeroes in place: the addresses stay
    before = [p.grad.data_ptr() for p in params]
    opt.zero_grad()
    assert [p.grad.data_ptr() for p in params] == before and not any(bool(p.grad.any()) for p in params)


def test_state_dict_round_trip_through_a_file(G, tmp_path):
    """Four steps straight = two steps, torch.save / torch.load into a fresh model and optimiser, two steps: bit for bit."""
    import torch
    a_model, a_params, a_opt, a_sched = _case_optimizer(G)
    for it in range(4):
        a_sched.step(it)
        _set_grads(a_params, 3, it)
        a_opt.step()
    b_model, b_params, b_opt, b_sched = _case_optimizer(G)
    for it in range(2):
        b_sched.step(it)
        _set_grads(b_params, 3, it)
        b_opt.step()
    path = str(tmp_path / "half.pth")
    torch.save({'model_state': b_model.state_dict(), 'optimizer_state': b_opt.state_dict()}, path)
    ck = torch.load(path, map_location=DEV)
    c_model, c_params, c_opt, c_sched = _case_optimizer(G, state=ck['model_state'])
    c_opt.load_state_dict(ck['optimizer_state'])
    assert c_opt.steps == [2] * 9
    for it in range(2, 4):
        c_sched.step(it)
        _set_grads(c_params, 3, it)
        c_opt.step()
    assert c_opt.steps == a_opt.steps == [4] * 9
    for i in range(9):
        assert torch.equal(a_params[i], c_params[i]) and R.same_bits(a_params[i].detach().cpu().numpy(), c_params[i].detach().cpu().numpy()), i
        assert R.same_bits(a_opt.exp_avg[i].cpu().numpy(), c_opt.exp_avg[i].cpu().numpy()), i
        assert R.same_bits(a_opt.exp_avg_sq[i].cpu().numpy(), c_opt.exp_avg_sq[i].cpu().numpy()), i
    # and into torch's own Adam over the same groups
    adam = torch.optim.Adam([{'params': list(g['params']), 'lr': 0} for g in c_opt.param_groups])
    adam.load_state_dict(c_opt.state_dict())
    assert all(float(adam.state[p]['step']) == 4.0 and adam.state[p]['exp_avg'].is_cuda for p in c_params)


def test_diverging_step_counts_are_refused(G):
    model, params, opt, sched = _case_optimizer(G)
    sched.step(0)
    _set_grads(params, 3, 0)
    params[4].grad = None
    opt.step()
    assert opt.steps == [1, 1, 1, 1, 0, 1, 1, 1, 1]
    _set_grads(params, 3, 1)
    with pytest.raises(ValueError, match="3.bias"):
        opt.step()


def test_step_makes_no_host_read(G):
    import torch
    model, params, opt, sched = _case_optimizer(G)
    sched.step(0)
    _set_grads(params, 3, 0)
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        try:
            opt.step()                                                    # the first call: table upload included
            opt.zero_grad()
            opt.step()
            stepped = True
        except RuntimeError:
            stepped = False
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if honoured:
        assert stepped, "OptimWrapper.step synchronised with the device"
    assert opt.steps == [2] * 9 and bool(torch.isfinite(opt.last_total_norm))
