"""float64 restatement of torch_optimizer 0.3.0's `Ranger` (RAdam + Lookahead), independent of sr_amd.optim.

One instance is one parameter group.  `step(grads)` takes one gradient per parameter or None; a parameter without a gradient
is skipped entirely (its count does not advance, so each parameter keeps its own step count and Lookahead phase).  RAdam's
scalars are computed per parameter from this group's betas (the package caches them in a buffer shared by all groups)."""
import math

import numpy as np


def scalars(t, beta1, beta2, thr):
    """(N_sma, rectified, step size) of step t."""
    b2t = beta2 ** t
    n_max = 2.0 / (1.0 - beta2) - 1.0
    n = n_max - 2.0 * t * b2t / (1.0 - b2t)
    if n > thr:
        return n, True, math.sqrt((1.0 - b2t) * (n - 4.0) / (n_max - 4.0) * (n - 2.0) / n * n_max / (n_max - 2.0)) / (1.0 - beta1 ** t)
    return n, False, 1.0 / (1.0 - beta1 ** t)


class RangerRef:
    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0.0):
        self.p = [np.array(x, dtype=np.float64) for x in params]
        self.lr, self.alpha, self.k, self.thr, self.eps, self.wd = lr, alpha, k, N_sma_threshhold, eps, weight_decay
        self.b1, self.b2 = betas
        self.step_count = [0] * len(self.p)
        self.m = [np.zeros_like(x) for x in self.p]
        self.v = [np.zeros_like(x) for x in self.p]
        self.slow = [None] * len(self.p)

    def step(self, grads):
        for i, g in enumerate(grads):
            if g is None:
                continue
            g = np.asarray(g, dtype=np.float64)
            p = self.p[i]
            if self.slow[i] is None:
                self.slow[i] = p.copy()
            self.v[i] = self.b2 * self.v[i] + (1.0 - self.b2) * g * g
            self.m[i] = self.b1 * self.m[i] + (1.0 - self.b1) * g
            self.step_count[i] += 1
            t = self.step_count[i]
            _, rect, s = scalars(t, self.b1, self.b2, self.thr)
            if self.wd != 0:
                p = p - self.wd * self.lr * p
            if rect:
                p = p - s * self.lr * self.m[i] / (np.sqrt(self.v[i]) + self.eps)
            else:
                p = p - s * self.lr * self.m[i]
            if t % self.k == 0:
                self.slow[i] = self.slow[i] + self.alpha * (p - self.slow[i])
                p = self.slow[i].copy()
            self.p[i] = p
