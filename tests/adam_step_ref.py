"""The numerics contract of include/dfu3d_opt.h restated in NumPy: every per-element operation one float32 operation,
the host constants formed in fp64 and rounded once, and the gradient norm as sqrt(math.fsum) in fp64 (the correctly
rounded sum: the stage's fixed-shape fp64 sum is compared with it to a relative 1e-12)."""
import math

import numpy as np

F = np.float32


def total_norm(grads):
    """sqrt of the correctly rounded sum of the exact fp64 squares of every element of every gradient (None: skipped)."""
    sq = [float(x) for g in grads if g is not None for x in np.square(np.asarray(g, np.float64)).ravel()]
    return math.sqrt(math.fsum(sq))


def coef_of(norm, max_norm):
    with np.errstate(all='ignore'):
        return F(np.minimum(1.0, np.float64(max_norm) / (np.float64(norm) + 1e-6)))


def constants(lr, beta1, beta2, eps, weight_decay, bc1, bc2):
    return dict(decay=F(1.0 - weight_decay * lr), b1=F(beta1), omb1=F(1.0 - beta1), b2=F(beta2), omb2=F(1.0 - beta2),
                step_size=F(lr / bc1), sqrt_bc2=F(math.sqrt(bc2)), eps=F(eps))


def element_step(p, g, m, v, coef, c):
    """-> (p2, m1, v1), float32 arrays; g None: the decay only, moments as they were."""
    p = np.asarray(p, F)
    if g is None:
        return p * c['decay'], m, v
    with np.errstate(all='ignore'):
        g1 = np.asarray(g, F) * F(coef)
        p1 = p * c['decay']
        m1 = c['b1'] * m + c['omb1'] * g1
        v1 = c['b2'] * v + c['omb2'] * (g1 * g1)
        d = np.sqrt(v1) / c['sqrt_bc2'] + c['eps']
        p2 = p1 - c['step_size'] * (m1 / d)
    assert p2.dtype == m1.dtype == v1.dtype == F
    return p2, m1, v1


class RefAdam:
    """The optimiser state of a list of tensors stepped by the restatement."""

    def __init__(self, params, eps=1e-8, weight_decay=0.01, max_norm=10.0):
        self.p = [np.array(p, F) for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.steps = [0] * len(self.p)
        self.eps, self.wd, self.max_norm = eps, weight_decay, max_norm
        self.norm = self.coef = None

    def step(self, grads, lr, beta1, beta2, coef=None):
        """coef: the device's (bitwise comparisons feed it back; the norm is checked on its own)."""
        with_grad = [i for i, g in enumerate(grads) if g is not None]
        step = self.steps[with_grad[0]] + 1 if with_grad else 1
        self.norm = total_norm(grads)
        self.coef = coef_of(self.norm, self.max_norm) if coef is None else F(coef)
        c = constants(lr, beta1, beta2, self.eps, self.wd, 1 - beta1 ** step, 1 - beta2 ** step)
        for i, g in enumerate(grads):
            self.p[i], self.m[i], self.v[i] = element_step(self.p[i], g, self.m[i], self.v[i], self.coef, c)
            if g is not None:
                assert self.steps[i] + 1 == step
                self.steps[i] = step


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))
