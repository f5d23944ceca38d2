"""Cases shared by tests/golden/capture_optimizer_golden.py and the optimiser tests: the case model, the OPTIMIZATION
block of centerpoint_nuscenes2kitti.yaml (typed in as a plain dict), the gradients of the golden runs, the schedule
settings of golden G17 and the length lists of the GPU test."""
import os

import numpy as np

from tests.centerpoint_cases import cfg

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g17_optimizer.npz")

OPTIMIZATION = {'BATCH_SIZE_PER_GPU': 4, 'NUM_EPOCHS': 20, 'OPTIMIZER': 'adam_onecycle', 'LR': 0.001, 'WEIGHT_DECAY': 0.01,
                'MOMENTUM': 0.9, 'MOMS': [0.95, 0.85], 'PCT_START': 0.4, 'DIV_FACTOR': 10, 'DECAY_STEP_LIST': [35, 45],
                'LR_DECAY': 0.1, 'LR_CLIP': 0.0000001, 'LR_WARMUP': False, 'WARMUP_EPOCH': 1, 'GRAD_NORM_CLIP': 10}
LR = OPTIMIZATION['LR']


def optim_cfg(**over):
    return cfg(dict(OPTIMIZATION, **over))


def case_model():
    """9 parameter tensors: 5 in the non-batch-norm group, 4 in the batch-norm group; one of 5125 elements (one full
    chunk and an odd tail).  The initial values of a test come from golden G17 (load_init), not from the seed."""
    import torch.nn as nn
    return nn.Sequential(nn.Conv2d(3, 8, 3, bias=False), nn.BatchNorm2d(8), nn.Sequential(nn.Linear(7, 5), nn.BatchNorm1d(5)),
                         nn.Linear(1025, 5))


GROUP_NAMES = [['0.weight', '2.0.weight', '2.0.bias', '3.weight', '3.bias'], ['1.weight', '1.bias', '2.1.weight', '2.1.bias']]
SEEDS = (3, 4, 5)
RUN = (10, 0.4)                                    # (total_step, pct_start) of the golden runs
SNAPSHOTS = (1, 4, 10)
GRAD_SCALES = [3, .01, 1, 1e-4, .5, 2, 0, 1, 30, 1e-3]     # per step: clipping on and off, one all-zero step
ZERO_GRAD_TENSOR = 1                               # this tensor's gradient is all zero in every step

ONE_CYCLE = [(10, 0.4), (7, 0.4), (1000, 0.4)]     # (total_step, pct_start)
COSINE = dict(total_step=20, total_epoch=2, iters_per_epoch=10, pct_start=0.4, warmup_iter=5)


def gradients(seed, step, shapes):
    """The gradients of step `step` (0-based) of the run `seed`, in the optimiser's parameter order."""
    rng = np.random.default_rng([seed, step])
    out = []
    for i, shape in enumerate(shapes):
        g = rng.standard_normal(shape).astype(np.float32) * np.float32(GRAD_SCALES[step])
        out.append(np.zeros(shape, np.float32) if i == ZERO_GRAD_TENSOR else g)
    return out


def bound(t, p):
    """|ours - reference| after t steps: two roundings of p per step with a factor 2 of room, and about ten float32
    roundings of an update of at most about 10 * lr."""
    return t * (2.0 ** -22 * np.abs(p) + 1e-5 * LR)


# ---- GPU test: tensors of these lengths carved from one buffer ----
LENGTH_LISTS = [[1], [3], [4], [5], [4095, 4096, 4097], [1, 1, 2, 64, 4097, 8199]]


def golden():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def ordered_params(model):
    """The model's parameters in the optimiser's order (group 0, then group 1), with their names."""
    named = dict(model.named_parameters())
    return [(n, named[n]) for g in GROUP_NAMES for n in g]


def load_init(model, G):
    import torch
    with torch.no_grad():
        for i, (n, p) in enumerate(ordered_params(model)):
            p.copy_(torch.from_numpy(G['init_%d' % i]).to(p.device))
    return model
