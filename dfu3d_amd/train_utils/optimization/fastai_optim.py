"""tools/train_utils/optimization/fastai_optim.py of the reference, backed by the fused step of dfu3d_amd/optim_ops.py.

`OptimWrapper` is the optimiser of the `adam_onecycle` / `adam_cosineanneal` recipes: gradient clipping by the global
norm (the reference's clip_grad_norm_ in train_one_epoch), true weight decay over every trainable parameter and Adam,
as ONE call of dfu3d_adam_step per step().  Parameter order and grouping are the reference's: the leaf modules of the
model in children() order, group 0 the trainable parameters of the leaves that are no batch norm, group 1 those of the
batch-norm leaves.

Restrictions, checked:
  * true_wd=True and bn_wd=True only (what build_optimizer asks for);
  * all parameters that have a gradient in one step() share one step count, otherwise ValueError names the parameter:
    the bias corrections are scalars of the call.  Counts diverge only for a parameter that is sometimes without a
    gradient; no model of this package has one;
  * float32 parameters on one GPU (optim_ops).  Construction, the hyper-parameter properties and the state dict need no
    GPU; step() does.

step() makes no host read and returns nothing; `last_total_norm` (the norm before clipping) and `status` are device
tensors, check_status() reads the status word and raises."""
from collections.abc import Iterable

import torch
from torch import nn

bn_types = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm)


def flatten_model(m):
    """The leaf modules of m in children() order (m itself when it has no children)."""
    kids = list(m.children())
    return [m] if not kids else [leaf for c in kids for leaf in flatten_model(c)]


def split_bn_bias(layer_groups):
    "Per layer group two groups: its children that are no batch norm, then its batch-norm children (`bn_types`)."
    out = []
    for group in layer_groups:
        kids = list(group.children())
        out += [nn.Sequential(*[c for c in kids if not isinstance(c, bn_types)]),
                nn.Sequential(*[c for c in kids if isinstance(c, bn_types)])]
    return out


def trainable_params(m):
    "The parameters of `m` that require a gradient, in parameters() order."
    return [p for p in m.parameters() if p.requires_grad]


def listify(p=None, q=None):
    "`p` as a list of the length of `q` (an int or a sequence); a single value is repeated."
    if p is None:
        p = []
    elif isinstance(p, str) or not isinstance(p, Iterable):
        p = [p]
    p = list(p)
    n = q if isinstance(q, int) else len(p) if q is None else len(q)
    if len(p) == 1:
        p = p * n
    assert len(p) == n, 'List len mismatch (%d vs %d)' % (len(p), n)
    return p


class OptimWrapper:
    "The fused clip + true weight decay + Adam step behind the reference's hyper-parameter surface."

    def __init__(self, param_groups, wd, true_wd=True, bn_wd=True, betas=(0.9, 0.99), eps=1e-8, max_norm=10.0, names=None):
        """param_groups: [non-batch-norm parameters, batch-norm parameters]; max_norm: the reference's GRAD_NORM_CLIP;
        names: {id(parameter): name} for messages."""
        if not (true_wd and bn_wd):
            raise NotImplementedError("OptimWrapper: only true_wd=True with bn_wd=True is implemented")
        groups = [list(g) for g in param_groups]
        if len(groups) != 2:
            raise ValueError("OptimWrapper: two parameter groups (non-batch-norm, batch-norm), got %d" % len(groups))
        self.true_wd, self.bn_wd = true_wd, bn_wd
        self.max_norm = float(max_norm)
        self.param_groups = [{'params': g, 'lr': 0, 'betas': (float(betas[0]), float(betas[1])), 'eps': float(eps),
                              'weight_decay': 0, 'amsgrad': False} for g in groups]
        self.params = [p for g in groups for p in g]
        if len(set(id(p) for p in self.params)) != len(self.params):
            raise ValueError("OptimWrapper: a parameter is in more than one group")
        names = names or {}
        self.names = [names.get(id(p), "parameter %d" % i) for i, p in enumerate(self.params)]
        self._lr, self._mom, self._beta, self._wd = [0.0], [float(betas[0])], [float(betas[1])], [float(wd)]
        self.steps = [0] * len(self.params)
        self.exp_avg = None
        self.exp_avg_sq = None
        self._fused = None
        self.last_total_norm = None
        self.status = None

    @classmethod
    def create(cls, opt_func, lr, layer_groups, **kwargs):
        """As the reference's: `layer_groups` is [nn.Sequential(*leaf modules)].  opt_func is looked at for the `betas` and
        `eps` keywords of a functools.partial over torch.optim.Adam; the step itself is the fused one."""
        layer_groups = list(layer_groups)
        if len(layer_groups) != 1:
            raise NotImplementedError("OptimWrapper: one layer group (the whole model), got %d" % len(layer_groups))
        kw = dict(getattr(opt_func, 'keywords', None) or {})
        for k in ('betas', 'eps'):
            if k in kw:
                kwargs.setdefault(k, kw[k])
        opt = cls([trainable_params(g) for g in split_bn_bias(layer_groups)], **kwargs)
        opt.lr, opt.opt_func = listify(lr, layer_groups), opt_func
        return opt

    def __repr__(self):
        return 'OptimWrapper over the fused Adam step (%d + %d tensors).\nTrue weight decay: %s' % (
            len(self.param_groups[0]['params']), len(self.param_groups[1]['params']), self.true_wd)

    # ---- hyper-parameters as properties --------------------------------------------------------------------------
    def _set(self, key, val):
        for g in self.param_groups:
            g[key] = val

    @property
    def lr(self):
        return self._lr[-1]

    @lr.setter
    def lr(self, val):
        self._lr = [float(v) for v in listify(val, self._lr)]       # (a schedule hands in NumPy scalars)
        self._set('lr', self._lr[-1])

    @property
    def mom(self):
        return self._mom[-1]

    @mom.setter
    def mom(self, val):
        self._mom = [float(v) for v in listify(val, self._mom)]
        self._set('betas', (self._mom[-1], self._beta[-1]))

    @property
    def beta(self):
        return self._beta[-1]

    @beta.setter
    def beta(self, val):
        if val is None:
            return
        self._beta = [float(v) for v in listify(val, self._beta)]
        self._set('betas', (self._mom[-1], self._beta[-1]))

    @property
    def wd(self):
        return self._wd[-1]

    @wd.setter
    def wd(self, val):
        self._wd = [float(v) for v in listify(val, self._wd)]          # true weight decay: the groups' weight_decay stays 0

    # ---- the optimiser's methods ---------------------------------------------------------------------------------
    def _moments(self):
        if self.exp_avg is None:
            self.exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
            self.exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]

    def step(self):
        "Clip by the global norm, decay every parameter, Adam on those that have a gradient: one fused call."
        from ... import optim_ops
        self._moments()
        moved = self._fused is not None and any(
            a is not b for a, b in zip(self._fused.exp_avg + self._fused.exp_avg_sq, self.exp_avg + self.exp_avg_sq))
        if self._fused is None or moved:
            self._fused = optim_ops.FusedAdamStep(self.params, self.exp_avg, self.exp_avg_sq, self.names)
            self.last_total_norm = self._fused.norm[0]
            self.status = self._fused.status
        with_grad = [i for i, p in enumerate(self.params) if p.grad is not None]
        step = self.steps[with_grad[0]] + 1 if with_grad else 1
        for i in with_grad:
            if self.steps[i] + 1 != step:
                raise ValueError("OptimWrapper.step: %s has taken %d steps, %s %d: parameters that have a gradient in one "
                                 "call must share one step count" % (self.names[i], self.steps[i],
                                                                     self.names[with_grad[0]], step - 1))
        beta1, beta2 = self.param_groups[0]['betas']
        self._fused.step(self.lr, beta1, beta2, self.param_groups[0]['eps'], self.wd, self.max_norm,
                         1 - beta1 ** step, 1 - beta2 ** step)
        for i in with_grad:
            self.steps[i] = step

    def zero_grad(self):
        "Zero the gradients in place: they keep their addresses, and the tensor table of the fused step stays valid."
        for p in self.params:
            if p.grad is not None:
                if p.grad.grad_fn is not None:
                    p.grad.detach_()
                else:
                    p.grad.requires_grad_(False)
                p.grad.zero_()

    def check_status(self):
        "One host read; raises Dfu3dError when a step met a gradient norm that is not finite."
        if self._fused is not None:
            self._fused.check_status()

    def clear(self):
        "Reset the state of the optimiser."
        self.steps = [0] * len(self.params)
        self.exp_avg = self.exp_avg_sq = None

    # ---- torch.optim.Adam's state dict over the two groups -----------------------------------------------------------
    def state_dict(self):
        state, groups, at = {}, [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != 'params'}
            d['params'] = list(range(at, at + len(g['params'])))
            at += len(g['params'])
            groups.append(d)
        for i, n in enumerate(self.steps):
            if n > 0:
                state[i] = {'step': torch.tensor(float(n)), 'exp_avg': self.exp_avg[i], 'exp_avg_sq': self.exp_avg_sq[i]}
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, state_dict):
        """A dict of state_dict()'s form, or one a torch.optim.Adam over the same two groups made (its other keys are
        ignored).  Moments are copied to the parameters' devices as float32."""
        groups = state_dict['param_groups']
        if [len(g['params']) for g in groups] != [len(g['params']) for g in self.param_groups]:
            raise ValueError("OptimWrapper.load_state_dict: groups of %s parameters, this optimiser has %s"
                             % ([len(g['params']) for g in groups], [len(g['params']) for g in self.param_groups]))
        ids = [i for g in groups for i in g['params']]
        steps = [0] * len(self.params)
        exp_avg = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        exp_avg_sq = [torch.zeros_like(p, memory_format=torch.contiguous_format) for p in self.params]
        for k, pid in enumerate(ids):
            s = state_dict['state'].get(pid)
            if s is None:
                continue
            if tuple(s['exp_avg'].shape) != tuple(self.params[k].shape):
                raise ValueError("OptimWrapper.load_state_dict: %s: moments of shape %s for a parameter of shape %s"
                                 % (self.names[k], tuple(s['exp_avg'].shape), tuple(self.params[k].shape)))
            steps[k] = int(s['step'])
            with torch.no_grad():
                exp_avg[k].copy_(s['exp_avg'])
                exp_avg_sq[k].copy_(s['exp_avg_sq'])
        self.steps, self.exp_avg, self.exp_avg_sq = steps, exp_avg, exp_avg_sq
        for mine, g in zip(self.param_groups, groups):
            mine['lr'], mine['eps'] = float(g['lr']), float(g['eps'])
            mine['betas'] = (float(g['betas'][0]), float(g['betas'][1]))
        g = self.param_groups[0]
        self._lr, self._mom, self._beta = [g['lr']], [g['betas'][0]], [g['betas'][1]]
