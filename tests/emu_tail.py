"""The rule of the tail pool (include/wesep_engine.h "tail pool"; runtime/tail_pool.cc) restated in numpy, twice: `Tail` keeps a
slot's bookkeeping as the runtime does (N, F, E, the hold), `brute` maps a firing schedule to the output position by position.
Both work in float64 on whatever `separate` returns; the blend is hold + ramp (v - hold) with the float32 ramp of the runtime."""
import numpy as np


def ramp_of(C):
    """ramp[j] = float(j + 1) / float(C + 1), computed in float32 as the runtime computes it"""
    return (np.arange(1, C + 1, dtype=np.float32) / np.float32(C + 1)).astype(np.float32)


def estimate(x, separate, factor=None):
    """v [K][L] of one window x [L]: separate(x), or with a per-window factor f = factor(x): separate(x (1 / f)) f"""
    if factor is None:
        return np.asarray(separate(x), dtype=np.float64)
    f = factor(x)
    return np.asarray(separate(x * (1.0 / f)), dtype=np.float64) * f


class Tail:
    """One slot.  separate(x [L]) -> [K][L]; factor(x [L]) -> the window's factor (None: none)."""

    def __init__(self, K, S, C, warm, separate, factor=None):
        assert 0 <= C <= S // 2 and max(C, 1) <= warm <= S
        self.K, self.S, self.C, self.warm, self.separate, self.factor = K, S, C, warm, separate, factor
        self.x = np.zeros(0)
        self.N, self.F, self.E, self.fired, self.done = 0, 0, 0, False, False
        self.hold = np.zeros((K, C))
        self.ramp = ramp_of(C).astype(np.float64)
        self.windows = []            # (a, N) of every window run
        self.blends = []             # [t0, t1) of every range of positions that came out of a cross-fade
        self.terms = []              # (t0, hold [K][C], v [K][C]) of every cross-fade: what went into it

    def push(self, chunk):
        chunk = np.asarray(chunk, dtype=np.float64).reshape(-1)
        assert not self.done and len(chunk) >= 1
        if self.N + len(chunk) - self.E > self.S:
            raise ValueError("tick first")
        self.x = np.concatenate([self.x, chunk])
        self.N += len(chunk)

    def fires(self):
        return not self.done and self.N >= self.warm and (not self.fired or self.N - self.F >= max(self.C, 1))

    def _window(self):
        a = max(0, self.N - self.S)
        self.windows.append((a, self.N))
        return a, estimate(self.x[a:self.N], self.separate, self.factor)

    def _emit(self, a, v, stop):
        """positions [E, stop) of the window's estimate v, the first h cross-faded with the hold"""
        h = self.C if self.fired else 0
        out = v[:, self.E - a:stop - a].copy()
        if h:
            self.terms.append((self.E, self.hold.copy(), out[:, :h].copy()))
            out[:, :h] = self.hold + self.ramp * (out[:, :h] - self.hold)
            self.blends.append((self.E, self.E + h))
        return out

    def tick(self):
        """-> [K][m], or None when the slot does not fire"""
        if not self.fires():
            return None
        a, v = self._window()
        out = self._emit(a, v, self.N - self.C)
        self.hold = v[:, self.N - self.C - a:].copy()
        self.F, self.E, self.fired = self.N, self.N - self.C, True
        return out

    def flush(self):
        assert not self.done and self.N >= 1
        if not self.fired or self.N > self.F:
            a, v = self._window()
            out = self._emit(a, v, self.N)
        else:
            out = self.hold.copy()
        self.E = self.F = self.N
        self.done = True
        return out


def firings(ticks, n, S, C, warm):
    """the values of N at which a slot fires when it is ticked at the values `ticks` of N (ascending, <= n)"""
    out = []
    for N in ticks:
        assert N <= n and N - (out[-1] - C if out else 0) <= S, "the schedule overflows a window: tick first"
        if N >= warm and (not out or N - out[-1] >= max(C, 1)):
            out.append(N)
    return out


def brute(x, K, S, C, warm, ticks, separate, factor=None):
    """The whole output [K][n] of one recording x [n] ticked at the values `ticks` of N and flushed at n, position by position."""
    x = np.asarray(x, dtype=np.float64)
    n = len(x)
    fs = firings(ticks, n, S, C, warm)
    ends = fs + ([n] if not fs or n > fs[-1] else [])        # the windows: every firing, and the flush's if it runs one
    v = [estimate(x[max(0, f - S):f], separate, factor) for f in ends]
    at = lambda i, t: v[i][:, t - max(0, ends[i] - S)]      # window i's estimate of position t
    ramp = ramp_of(C).astype(np.float64)
    out = np.zeros((K, n))
    for t in range(n):
        # window i emits t: the first one that ends more than C samples behind t; the last window emits everything to n (the
        # flush's own window holds nothing back, and with n == F the last hold comes out as it is)
        i = 0
        while i < len(ends) - 1 and t >= ends[i] - C:
            i += 1
        if i > 0 and t < ends[i - 1]:                       # one of the C samples window i - 1 held back: cross-faded
            hold = at(i - 1, t)
            out[:, t] = hold + ramp[t - (ends[i - 1] - C)] * (at(i, t) - hold)
        else:
            out[:, t] = at(i, t)
    return out


def tick_forwards(lengths, K, S, max_rows):
    """The forwards of one tick as (rows, L) pairs: lengths = the window lengths L of its firing slots in ascending slot order.
    Full windows share forwards of at most max_rows rows; a slot in warm-up (L < S) runs in forwards of its own rows."""
    out = []
    full = K * sum(1 for L in lengths if L == S)
    out += [(min(max_rows, full - r), S) for r in range(0, full, max_rows)]
    for L in lengths:
        if L != S:
            out += [(min(max_rows, K - r), L) for r in range(0, K, max_rows)]
    return out
