"""Reference for gradient accumulation over a window of k micro-steps (numpy only; independent of the package).

The two rules, with `acc` zero at the start of a window:

    micro-steps 1 .. k-1 (ADD)    acc = acc + g
    micro-step  k        (FINAL)  g = (acc + g) * inv_k;  acc = 0          inv_k = float32(1 / k), the quotient formed in double

`window_f64` states them in float64 with the exact 1 / k (the mean of the window's gradients); `add_f32` / `final_f32` / `window_f32`
restate them in fp32 in the pinned order, every operation rounded on its own, which is what the kernel and the CPU path must give bit
for bit.  `bound` is the per-element distance the fp32 form may lie from the float64 mean."""
import numpy as np


def inv_k(k):
    return np.float32(1.0 / k)


def window_f64(grads):
    """The mean of `grads` (one array per micro-step) in float64."""
    acc = np.zeros_like(np.asarray(grads[0], dtype=np.float64))
    for g in grads:
        acc = acc + np.asarray(g, dtype=np.float64)
    return acc / float(len(grads))


def add_f32(acc, g):
    """ADD: the new acc."""
    acc, g = np.asarray(acc), np.asarray(g)
    assert acc.dtype == np.float32 and g.dtype == np.float32
    return acc + g


def final_f32(acc, g, k):
    """FINAL: (the new g, the new acc)."""
    acc, g = np.asarray(acc), np.asarray(g)
    assert acc.dtype == np.float32 and g.dtype == np.float32
    s = acc + g
    return s * inv_k(k), np.zeros_like(acc)


def window_f32(grads):
    """The final gradient of a window whose micro-steps deliver `grads`, in the pinned fp32 order."""
    k = len(grads)
    acc = np.zeros_like(np.asarray(grads[0], dtype=np.float32))
    for g in grads[:-1]:
        acc = add_f32(acc, g)
    out, acc = final_f32(acc, grads[-1], k)
    assert not acc.any()
    return out


def bound(grads):
    """(k + 2) * 2^-24 * (sum_j |g_j|) / k per element: k - 1 additions, the rounding of inv_k, one multiplication, and one unit of slack
    for second-order terms."""
    k = len(grads)
    return (k + 2) * 2.0 ** -24 * sum(np.abs(np.asarray(g, dtype=np.float64)) for g in grads) / k
