"""Golden G17: the reference's own adam_onecycle recipe (row f-12 of SURVEY.md section 8), run unmodified on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_optimizer_golden.py REFERENCE_ROOT      ->  tests/golden/g17_optimizer.npz

tools/train_utils/optimization (its __init__, fastai_optim.py and learning_schedules_fastai.py) is imported UNMODIFIED as
a package of its own; torch.nn.utils.clip_grad_norm_ is the clipping train_one_epoch does before optimizer.step().

(a) the parameter names of the two groups build_optimizer makes for tests/optimizer_cases.py case_model();
(b) lr and mom of every step of OneCycle for each (total_step, pct_start) of ONE_CYCLE, and of CosineAnnealing for COSINE;
(c) for every seed of SEEDS: the initial parameters (seeded, stored), and the parameters and Adam step counts after
    steps 1, 4 and 10 of a RUN one-cycle run under the gradients of optimizer_cases.gradients.
The fixture is data only."""
import importlib.util
import json
import os
import sys

import numpy as np
import torch
from torch.nn.utils import clip_grad_norm_

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import optimizer_cases as K  # noqa: E402


def load_reference():
    d = os.path.join(REF, 'tools', 'train_utils', 'optimization')
    spec = importlib.util.spec_from_file_location('ref_optimization', os.path.join(d, '__init__.py'),
                                                  submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules['ref_optimization'] = mod
    spec.loader.exec_module(mod)
    return mod


class Hyper:
    lr = mom = 0


def main():
    ref = load_reference()
    out, meta = {}, {'torch': torch.__version__}
    # (a)
    torch.manual_seed(1700)
    model = K.case_model()
    names = {id(p): n for n, p in model.named_parameters()}
    opt = ref.build_optimizer(model, K.optim_cfg())
    meta['group_names'] = [[names[id(p)] for p in g['params']] for g in opt.param_groups]
    assert meta['group_names'] == K.GROUP_NAMES, meta['group_names']
    for i, (n, p) in enumerate(K.ordered_params(model)):
        out['init_%d' % i] = p.detach().numpy().copy()
    # (b)
    for total, pct in K.ONE_CYCLE:
        h = Hyper()
        s = ref.OneCycle(h, total, K.LR, list(K.OPTIMIZATION['MOMS']), K.OPTIMIZATION['DIV_FACTOR'], pct)
        lrs, moms = [], []
        for i in range(total):
            s.step(i)
            lrs.append(float(h.lr))
            moms.append(float(h.mom))
        out['onecycle_%d_lr' % total], out['onecycle_%d_mom' % total] = np.array(lrs, np.float64), np.array(moms, np.float64)
    c = K.COSINE
    h = Hyper()
    s = ref.CosineAnnealing(h, c['total_step'], c['total_epoch'], K.LR, list(K.OPTIMIZATION['MOMS']), c['pct_start'],
                            c['warmup_iter'])
    lrs, moms = [], []
    for i in range(c['total_step']):
        s.step(i, i // c['iters_per_epoch'])
        lrs.append(float(h.lr))
        moms.append(float(h.mom))
    out['cosine_lr'], out['cosine_mom'] = np.array(lrs, np.float64), np.array(moms, np.float64)
    # (c)
    torch.set_num_threads(1)
    for seed in K.SEEDS:
        model = K.load_init(K.case_model(), out)
        params = [p for _, p in K.ordered_params(model)]
        opt = ref.build_optimizer(model, K.optim_cfg())
        sched, _ = ref.build_scheduler(opt, K.RUN[0], 1, -1, K.optim_cfg(PCT_START=K.RUN[1]))
        for it in range(K.RUN[0]):
            sched.step(it)
            for p, g in zip(params, K.gradients(seed, it, [tuple(p.shape) for p in params])):
                p.grad = torch.from_numpy(g)
            clip_grad_norm_(model.parameters(), K.OPTIMIZATION['GRAD_NORM_CLIP'])
            opt.step()
            if it + 1 in K.SNAPSHOTS:
                for i, p in enumerate(params):
                    out['s%d_t%d_p%d' % (seed, it + 1, i)] = p.detach().numpy().copy()
                out['s%d_t%d_steps' % (seed, it + 1)] = np.array([int(opt.opt.state[p]['step']) for p in params], np.int64)
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(K.PATH, **out)
    print(K.PATH, os.path.getsize(K.PATH))


if __name__ == '__main__':
    main()
