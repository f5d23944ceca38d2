"""tools/train_utils/optimization of the reference: build_optimizer and build_scheduler over an OPTIMIZATION config
(attribute access and .get, as an EasyDict has).  `adam_onecycle` and `adam_cosineanneal` get the fused optimiser
(fastai_optim.OptimWrapper, which also clips the gradient norm at GRAD_NORM_CLIP inside its step); `adam` and `sgd` get
torch's own."""
from functools import partial

import torch.nn as nn
import torch.optim as optim
import torch.optim.lr_scheduler as lr_sched

from .fastai_optim import OptimWrapper, flatten_model
from .learning_schedules_fastai import CosineAnnealing, CosineWarmupLR, OneCycle

DEFAULT_GRAD_NORM_CLIP = 10


def _get(cfg, key, default):
    return cfg.get(key, default) if hasattr(cfg, 'get') else getattr(cfg, key, default)


def build_optimizer(model, optim_cfg):
    if optim_cfg.OPTIMIZER == 'adam':
        return optim.Adam(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY)
    if optim_cfg.OPTIMIZER == 'sgd':
        return optim.SGD(model.parameters(), lr=optim_cfg.LR, weight_decay=optim_cfg.WEIGHT_DECAY,
                         momentum=optim_cfg.MOMENTUM)
    if optim_cfg.OPTIMIZER not in ('adam_onecycle', 'adam_cosineanneal'):
        raise NotImplementedError(optim_cfg.OPTIMIZER)
    betas = tuple(_get(optim_cfg, 'BETAS', (0.9, 0.99)))
    names = {id(p): n for n, p in model.named_parameters()}
    optimizer = OptimWrapper.create(partial(optim.Adam, betas=betas), 3e-3, [nn.Sequential(*flatten_model(model))],
                                    wd=optim_cfg.WEIGHT_DECAY, true_wd=True, bn_wd=True,
                                    max_norm=_get(optim_cfg, 'GRAD_NORM_CLIP', DEFAULT_GRAD_NORM_CLIP), names=names)
    from ...pcdet_kitti.centerpoint import CenterPoint
    if isinstance(model, CenterPoint):
        # the grouping walks leaf modules: a parameter held by a module that also has children would be left out
        grouped = sorted(names[id(p)] for p in optimizer.params)
        trainable = sorted(n for n, p in model.named_parameters() if p.requires_grad)
        assert grouped == trainable, sorted(set(trainable) ^ set(grouped))
    return optimizer


def build_scheduler(optimizer, total_iters_each_epoch, total_epochs, last_epoch, optim_cfg):
    total_steps = total_iters_each_epoch * total_epochs
    if optim_cfg.OPTIMIZER == 'adam_onecycle':
        return OneCycle(optimizer, total_steps, optim_cfg.LR, list(optim_cfg.MOMS), optim_cfg.DIV_FACTOR,
                        optim_cfg.PCT_START), None
    if optim_cfg.OPTIMIZER == 'adam_cosineanneal':
        return CosineAnnealing(optimizer, total_steps, total_epochs, optim_cfg.LR, list(optim_cfg.MOMS), optim_cfg.PCT_START,
                               optim_cfg.WARMUP_ITER), None
    decay_steps = [x * total_iters_each_epoch for x in optim_cfg.DECAY_STEP_LIST]

    def lr_lbmd(cur_epoch):
        cur_decay = 1
        for decay_step in decay_steps:
            if cur_epoch >= decay_step:
                cur_decay = cur_decay * optim_cfg.LR_DECAY
        return max(cur_decay, optim_cfg.LR_CLIP / optim_cfg.LR)

    lr_scheduler = lr_sched.LambdaLR(optimizer, lr_lbmd, last_epoch=last_epoch)
    lr_warmup_scheduler = None
    if optim_cfg.LR_WARMUP:
        # (the reference takes len() of total_iters_each_epoch here, an int: the count itself is what it means)
        lr_warmup_scheduler = CosineWarmupLR(optimizer, T_max=optim_cfg.WARMUP_EPOCH * total_iters_each_epoch,
                                             eta_min=optim_cfg.LR / optim_cfg.DIV_FACTOR)
    return lr_scheduler, lr_warmup_scheduler
