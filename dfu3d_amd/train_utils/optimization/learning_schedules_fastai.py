"""tools/train_utils/optimization/learning_schedules_fastai.py of the reference: the one-cycle and cosine-annealing
schedules that set `lr` and `mom` of an OptimWrapper before every iteration.

The values equal the reference's to the last bit (golden G17): phase borders are `int(start * total_step)`, truncated;
step() runs over EVERY phase whose start has passed and the last one wins; the cosine is numpy's."""
import math
from functools import partial

import numpy as np
import torch.optim.lr_scheduler as lr_sched


def _phases(phases, total_step):
    """((start fraction, function), ...) -> [(first step, end step, function)]: a phase ends where the next begins, the
    last one at total_step."""
    out = []
    for i, (start, func) in enumerate(phases):
        if out:
            assert out[-1][3] < start
        if isinstance(func, str):
            func = eval(func)
        end = int(phases[i + 1][0] * total_step) if i + 1 < len(phases) else total_step
        out.append((int(start * total_step), end, func, start))
    assert out[0][0] == 0
    return [p[:3] for p in out]


class LRSchedulerStep(object):
    def __init__(self, fai_optimizer, total_step, lr_phases, mom_phases):
        self.optimizer = fai_optimizer
        self.total_step = total_step
        self.lr_phases = _phases(lr_phases, total_step)
        self.mom_phases = _phases(mom_phases, total_step)

    def step(self, step, epoch=None):
        for start, end, func in self.lr_phases:
            if step >= start:
                self.optimizer.lr = func((step - start) / (end - start))
        for start, end, func in self.mom_phases:
            if step >= start:
                self.optimizer.mom = func((step - start) / (end - start))


def annealing_cos(start, end, pct):
    "From `start` to `end` along half a cosine as pct goes from 0.0 to 1.0."
    cos_out = np.cos(np.pi * pct) + 1
    return end + (start - end) / 2 * cos_out


class OneCycle(LRSchedulerStep):
    def __init__(self, fai_optimizer, total_step, lr_max, moms, div_factor, pct_start):
        self.lr_max = lr_max
        self.moms = moms
        self.div_factor = div_factor
        self.pct_start = pct_start
        low_lr = self.lr_max / self.div_factor
        lr_phases = ((0, partial(annealing_cos, low_lr, self.lr_max)),
                     (self.pct_start, partial(annealing_cos, self.lr_max, low_lr / 1e4)))
        mom_phases = ((0, partial(annealing_cos, *self.moms)),
                      (self.pct_start, partial(annealing_cos, *self.moms[::-1])))
        fai_optimizer.lr, fai_optimizer.mom = low_lr, self.moms[0]
        super().__init__(fai_optimizer, total_step, lr_phases, mom_phases)


class CosineWarmupLR(lr_sched._LRScheduler):
    def __init__(self, optimizer, T_max, eta_min=0, last_epoch=-1):
        self.T_max = T_max
        self.eta_min = eta_min
        super(CosineWarmupLR, self).__init__(optimizer, last_epoch)

    def get_lr(self, epoch=None):
        return [self.eta_min + (base_lr - self.eta_min) * (1 - math.cos(math.pi * self.last_epoch / self.T_max)) / 2
                for base_lr in self.base_lrs]


def linear_warmup(end, lr_max, pct):
    k = (1 - pct / end) * (1 - 0.33333333)
    return lr_max * (1 - k)


class CosineAnnealing(LRSchedulerStep):
    def __init__(self, fai_optimizer, total_step, total_epoch, lr_max, moms, pct_start, warmup_iter):
        self.lr_max = lr_max
        self.moms = moms
        self.pct_start = pct_start
        self.optimizer = fai_optimizer
        self.total_step = total_step
        self.warmup_iter = warmup_iter
        self.total_epoch = total_epoch
        fai_optimizer.lr, fai_optimizer.mom = lr_max, self.moms[0]
        self.mom_phases = _phases(((0, partial(annealing_cos, *self.moms)),
                                   (self.pct_start, partial(annealing_cos, *self.moms[::-1]))), total_step)

    def step(self, step, epoch):
        if step < self.warmup_iter:
            self.optimizer.lr = linear_warmup(self.warmup_iter, self.lr_max, step)
        else:
            self.optimizer.lr = annealing_cos(self.lr_max, self.lr_max * 0.001, epoch / self.total_epoch)
        for start, end, func in self.mom_phases:
            if step >= start:
                self.optimizer.mom = func((step - start) / (end - start))
