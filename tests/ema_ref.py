"""Float64 numpy restatement of the exponential moving average of the weights, independent of the package:

    s += float64(float32(1 - decay)) * (p - s)          per update, with a count

The weight is the fp32 number the kernel reads (1 - decay formed in double, rounded once); everything else is float64.  `bound` is the
error an fp32 implementation of the same recurrence may have after N updates:

    one update is three fp32 roundings (p - s, w * that, s + that) of quantities of magnitude at most 2M, M the largest magnitude on
    the trajectory: under 3 * 2^-24 * 2M < 5 * 2^-24 * M of new error (the subnormal range aside); the error already in s is
    multiplied by decay <= 1, so errors add at most linearly:  N * 5 * 2^-24 * M  <  N * 2^-21 * M.
"""
import numpy as np


class EmaRef:
    def __init__(self, params, decay):
        self.w = np.float64(np.float32(1.0 - float(decay)))
        self.s = [np.array(p, dtype=np.float64) for p in params]
        self.count = 0
        self.mag = max([float(np.abs(s).max()) for s in self.s if s.size] + [0.0])      # largest magnitude on the trajectory

    def set_decay(self, decay):
        self.w = np.float64(np.float32(1.0 - float(decay)))

    def update(self, params):
        for s, p in zip(self.s, params):
            p = np.asarray(p, dtype=np.float64)
            s += self.w * (p - s)
            if p.size:
                self.mag = max(self.mag, float(np.abs(p).max()), float(np.abs(s).max()))
        self.count += 1

    def bound(self, n=None):
        return (self.count if n is None else n) * 2.0 ** -21 * self.mag
