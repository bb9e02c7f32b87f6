"""numpy restatement of the live-window contract (include/wesep_hip.h, ws_xfade_stream_fwd; include/wesep_engine.h,
ws_engine_live_*), written from the definition: the reference of tests/test_live_host_cpu.py and the driver of
tests/test_live_gpu.py.  S = window, O = overlap, H = S - O, N = samples pushed.
  windows_run(N)   N < S ? 0 : 1 + (N - S) // H      window w < Wr starts at w H
  emitted(N)       max(Wr - 1, 0) H                   the samples before the start of the newest window run
xfade_stream is ws_xfade_ola over [i0, i0 + count) with window w read from ring slot w % cap; Live is the emission rule
around it, with the separator replaced by a function of (window index, its samples)."""
import numpy as np


def windows_run(N, S, H):
    return 0 if N < S else 1 + (N - S) // H


def emitted(N, S, H):
    return max(windows_run(N, S, H) - 1, 0) * H


def total_windows(n, S, H):
    return 1 if n <= S else 1 + -(-(n - S) // H)


def xfade_stream(ring, S, O, i0, count, run, final=None, scale_ring=None):
    """ring [K][cap][S] -> out [K][count] in ring's dtype (float64 in the tests).  final: None while the recording runs --
    every covering window is regular with its tail ramp -- or (W, n).  Reads ring[:, w % cap] for covering windows only."""
    K, cap, _ = ring.shape
    H = S - O
    assert 0 <= O <= S // 2 and i0 >= 0 and count >= 0 and run >= 0
    if final is None:
        assert i0 + count <= max(run - 1, 0) * H, "a range past the windows run"
        W, L, last = run + 1, S, None
    else:
        W, n = final
        assert W == total_windows(n, S, H) == run and i0 + count <= n
        L = min(n, S)
        last = n - L
    o1 = O + 1.0
    # every window that covers a position of the range, ascending: each adds its weighted samples to the positions it covers,
    # so a position's terms are summed in ascending window order, as the definition says
    cover = []
    if count:
        cover = [(w, w * H) for w in range(0 if i0 < L else (i0 - L) // H + 1, min(W - 2, (i0 + count - 1) // H) + 1)]
        if last is not None and i0 + count - 1 >= last:
            cover.append((W - 1, last))
    num, den = np.zeros((K, count), ring.dtype), np.zeros(count)
    for w, start in cover:
        lo, hi = max(i0, start), min(i0 + count, start + L)          # the positions of the range inside the window
        j = np.arange(lo - start, hi - start)
        g = np.ones(len(j))
        if w > 0:
            g = np.minimum(1.0, (j + 1) / o1)
        if w < W - 1:
            g = g * np.minimum(1.0, (L - j) / o1)
        slot = w % cap
        v = ring[:, slot, lo - start:hi - start]
        if scale_ring is not None:
            v = v * scale_ring[slot]
        num[:, lo - i0:hi - i0] += g * v
        den[lo - i0:hi - i0] += g
    if cover:
        used = [w for w, _ in cover]
        assert min(used) >= run - cap and max(used) - min(used) < cap, "cap does not hold the windows of the range"
    return num / den if count else num


class Live:
    """The emission rule with `separate(w, x [L]) -> [K][L]` for a window: push(chunk) / flush() return [K][m]; ring slots no
    covering window owns stay NaN, so a read outside the contract shows."""

    def __init__(self, K, S, O, g_max, separate, scale=None, dtype=np.float64):
        self.K, self.S, self.O, self.H, self.g_max, self.cap = K, S, O, S - O, g_max, g_max + 3
        self.sep, self.scale, self.dtype = separate, scale, dtype
        self.reset()

    def reset(self):
        self.ring = np.full((self.K, self.cap, self.S), np.nan, self.dtype)
        self.scale_ring = None if self.scale is None else np.full(self.cap, np.nan, self.dtype)
        self.pend, self.base, self.N, self.Wr, self.E, self.done, self.groups = np.zeros(0, self.dtype), 0, 0, 0, 0, False, []

    def _run(self, w0, g, L):
        """windows w0 .. w0 + g - 1 of L samples into slots w0 % cap .. (never across the wrap)"""
        assert 1 <= g <= self.g_max and w0 % self.cap + g <= self.cap
        for w in range(w0, w0 + g):
            a = (w * self.H if L == self.S and not self._last else self.N - L) - self.base
            y = self.sep(w, self.pend[a:a + L])
            self.ring[:, w % self.cap, :] = np.nan            # what the slot held is gone
            self.ring[:, w % self.cap, :L] = y
            if self.scale is not None:
                self.scale_ring[w % self.cap] = self.scale(w)
        self.groups.append(g)

    def push(self, chunk):
        assert not self.done and len(chunk) >= 1
        self._last = False
        self.groups = []
        self.pend = np.concatenate([self.pend, np.asarray(chunk, self.dtype)])
        self.N += len(chunk)
        target, out = windows_run(self.N, self.S, self.H), []
        while self.Wr < target:
            g = min(target - self.Wr, self.g_max, self.cap - self.Wr % self.cap)
            self._run(self.Wr, g, self.S)
            self.Wr += g
            to = (self.Wr - 1) * self.H
            out.append(xfade_stream(self.ring, self.S, self.O, self.E, to - self.E, self.Wr, None, self.scale_ring))
            self.E = to
        assert self.E == emitted(self.N, self.S, self.H)
        self.pend, self.base = self.pend[self.E - self.base:], self.E
        assert len(self.pend) < self.S + self.H
        return np.concatenate(out, axis=1) if out else np.zeros((self.K, 0), self.dtype)

    def flush(self):
        assert not self.done and self.N >= 1
        n, self.groups = self.N, []
        self._last = True
        if n < self.S:
            self._run(0, 1, n)
            self.Wr = 1
        elif (n - self.S) % self.H:
            self._run(self.Wr, 1, self.S)
            self.Wr += 1
        out = xfade_stream(self.ring, self.S, self.O, self.E, n - self.E, self.Wr, (self.Wr, n), self.scale_ring)
        self.E, self.done = n, True
        return out


def schedules(n, seed):
    """packet schedules of a recording of n samples: 1-sample pushes, 160, seeded random 1 .. 3000 and 1 .. 40, one push"""
    rng = np.random.default_rng(seed)

    def rand(hi):
        out, left = [], n
        while left > 0:
            out.append(min(left, int(rng.integers(1, hi + 1))))
            left -= out[-1]
        return out

    return {"1": [1] * n, "160": [160] * (n // 160) + ([n % 160] if n % 160 else []), "random": rand(3000), "small": rand(40),
            "whole": [n]}
