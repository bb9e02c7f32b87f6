"""The rule of the rate tail pool (include/wesep_engine.h "rate tail pool"; runtime/rate_tail_pool.cc) restated in numpy from
the pieces it is made of: the whole-signal resampler and its streaming emission count (tests/resample_contract.py `reference`,
`emitted`), the tail pool's slot (tests/emu_tail.py `Tail`), and the resampler again on the way back.  `Counts` is the same rule
on integers alone: what every tick and the flush return, known before anything runs."""
import numpy as np

from tests import emu_tail as T
from tests import resample_contract as RC


def geometry(rate_in, rate_out):
    """(U, D, w, K); equal rates: the identity table U = D = K = 1, no delay"""
    return (1, 1, 0, 1) if rate_in == rate_out else RC.geometry(rate_in, rate_out)


def emitted(N, rate_in, rate_out):
    """outputs a streaming resampler has returned after N input samples"""
    U, D, w, _ = geometry(rate_in, rate_out)
    return U * max(0, (N - w) // D)


def out_len(N, rate_in, rate_out):
    U, D, _, _ = geometry(rate_in, rate_out)
    return -(-U * N // D)


def reference(x, rate_in, rate_out):
    """the whole signal x [n] resampled, float64 (equal rates: x itself)"""
    x = np.asarray(x, dtype=np.float64)
    if rate_in == rate_out or len(x) == 0:
        return x.copy() if rate_in == rate_out else np.zeros(0)
    return RC.reference(x, rate_in, rate_out)


def cap(S, rate, model_rate):
    """ws_engine_rate_tail_pool_cap: what B returns at most for a history below K_B and S new samples"""
    U, D, _, K = geometry(model_rate, rate)
    return ((K + S) // D + 2) * U


class Counts:
    """One slot on integers: Nc caller samples pushed; N, F, E at the model's rate; what B took and what came back."""

    def __init__(self, S, C, warm, rate, model_rate):
        self.S, self.C, self.warm, self.rate, self.model_rate = S, C, warm, rate, model_rate
        self.Nc, self.F, self.E, self.fired, self.done = 0, 0, 0, False, False
        self.b_n, self.returned = 0, 0

    @property
    def N(self):
        return emitted(self.Nc, self.rate, self.model_rate)

    def room(self):
        """the largest push that is not refused"""
        U, D, _, _ = geometry(self.rate, self.model_rate)
        return (D * (self.S + self.E)) // U - self.Nc          # ceil(U n / D) <= S + E  <=>  n <= floor(D (S + E) / U)

    def push(self, n):
        assert not self.done and n >= 1
        if out_len(self.Nc + n, self.rate, self.model_rate) - self.E > self.S:
            raise ValueError("tick first")
        self.Nc += n

    def fires(self):
        return not self.done and self.N >= self.warm and (not self.fired or self.N - self.F >= max(self.C, 1))

    def tick(self):
        """-> (window length L, samples returned at the caller's rate), or None when the slot does not fire"""
        if not self.fires():
            return None
        N = self.N
        self.b_n += N - self.C - self.E
        self.F, self.E, self.fired = N, N - self.C, True
        m = emitted(self.b_n, self.model_rate, self.rate) - self.returned
        self.returned += m
        return min(N, self.S), m

    def flush(self):
        """-> (the last window's length or 0 when only the hold comes out, samples returned)"""
        assert not self.done and self.Nc >= 1
        N = out_len(self.Nc, self.rate, self.model_rate)
        L = min(N, self.S) if not self.fired or N > self.F else 0
        self.b_n += N - self.E
        self.E = self.F = N
        m = min(self.Nc, out_len(self.b_n, self.model_rate, self.rate)) - self.returned
        self.returned += m
        self.done = True
        return L, m


class RateTail:
    """One slot on samples, float64.  separate(x [L]) -> [K][L] works at the model's rate."""

    def __init__(self, K, S, C, warm, rate, model_rate, separate):
        self.K, self.rate, self.model_rate = K, rate, model_rate
        self.counts = Counts(S, C, warm, rate, model_rate)
        self.tail = T.Tail(K, S, C, warm, separate)
        self.x = np.zeros(0)                    # what was pushed, at the caller's rate
        self.y = np.zeros((K, 0))               # what the tail pool emitted, at the model's rate
        self.returned = 0

    def _feed(self, final):
        """the model-rate samples the recording has now that the tail slot has not seen"""
        have = out_len(len(self.x), self.rate, self.model_rate) if final else emitted(len(self.x), self.rate, self.model_rate)
        if have > self.tail.N:
            # an output below the emission count has all of its taps: its value does not depend on what follows
            self.tail.push(reference(self.x, self.rate, self.model_rate)[self.tail.N:have])

    def _back(self, final):
        n = self.y.shape[1]
        have = min(len(self.x), out_len(n, self.model_rate, self.rate)) if final else emitted(n, self.model_rate, self.rate)
        out = np.stack([reference(row, self.model_rate, self.rate)[self.returned:have] for row in self.y]) if have > self.returned \
            else np.zeros((self.K, 0))
        self.returned = max(have, self.returned)
        return out

    def push(self, chunk):
        chunk = np.asarray(chunk, dtype=np.float64).reshape(-1)
        self.counts.push(len(chunk))
        self.x = np.concatenate([self.x, chunk])

    def tick(self):
        want = self.counts.tick()
        if want is None:
            return None
        self._feed(False)
        got = self.tail.tick()
        assert got is not None
        self.y = np.concatenate([self.y, got], axis=1)
        out = self._back(False)
        assert out.shape[1] == want[1]
        return out

    def flush(self):
        want = self.counts.flush()
        self._feed(True)
        self.y = np.concatenate([self.y, self.tail.flush()], axis=1)
        out = self._back(True)
        assert out.shape[1] == want[1]
        return out
