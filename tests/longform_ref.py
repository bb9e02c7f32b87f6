"""numpy-float64 restatement of the window layout and the cross-fade of long recordings (include/wesep_hip.h,
ws_window_rows / ws_xfade_ola), written from the definition, not from the kernels: the reference of
tests/test_longform_host_cpu.py and tests/test_longform_gpu.py.  Weights are exact rationals first and float64 second, so
"two regular neighbours add up to 1" can be asserted exactly."""
from fractions import Fraction

import numpy as np


def starts(n, S, O):
    """Window starts of a recording of n samples: window S, overlap O (0 <= O <= S // 2), hop S - O."""
    assert n >= 1 and S >= 1 and 0 <= O <= S // 2
    if n <= S:
        return [0]
    H = S - O
    W = 1 + (n - S + H - 1) // H
    return [w * H for w in range(W - 1)] + [n - S]


def weight(w, W, j, L, O):
    """g_w(j) as an exact rational: a ramp up over the first O samples unless w is the first window, a ramp down over the
    last O unless it is the last."""
    g = Fraction(1)
    if w > 0:
        g *= min(Fraction(1), Fraction(j + 1, O + 1))
    if w < W - 1:
        g *= min(Fraction(1), Fraction(L - j, O + 1))
    return g


def weights(W, L, O):
    """float64 [W][L] of the above"""
    up = np.minimum(1.0, (np.arange(L) + 1.0) / (O + 1.0))
    down = np.minimum(1.0, (L - np.arange(L, dtype=np.float64)) / (O + 1.0))
    g = np.ones((W, L))
    g[1:] *= up
    g[:-1] *= down
    return g


def gather(x, S, O):
    """x [n] -> the windows [W][min(n, S)] in float64"""
    x = np.asarray(x, dtype=np.float64)
    L = min(len(x), S)
    return np.stack([x[s:s + L] for s in starts(len(x), S, O)])


def xfade(y, n, S, O):
    """y [K][W][L] -> [K][n] float64: the weighted sum of the windows that cover a sample, ascending, over the sum of the
    weights."""
    y = np.asarray(y, dtype=np.float64)
    st = starts(n, S, O)
    K, W, L = y.shape
    assert W == len(st) and L == min(n, S)
    g = weights(W, L, O)
    num, den = np.zeros((K, n)), np.zeros(n)
    for w, s in enumerate(st):
        num[:, s:s + L] += g[w] * y[:, w]
        den[s:s + L] += g[w]
    assert (den > 0).all()
    return num / den
