"""Host-side emulation of the streaming resampler: the contract of ws_resample_stream_fwd (its refusals included) in numpy,
and the host bookkeeping of wesep_amd.resample.StreamResampler / runtime/rate.cc on top of it -- two buffers used in turn,
64-bit counters on the host, buffer-relative offsets only into the "kernel".

Two emulations share the bookkeeping:
  EmuStream(values=True)   carries samples; the kernel is fp64 arithmetic in one fixed order per output (a function of the
                           taps and samples under it alone), so streamed and whole-signal results can be compared exactly.
  EmuStream(values=False)  carries sample INDICES; the kernel checks, per call and in O(1), that what the call would read is
                           what the whole-signal form reads for the same outputs (every tap on its own sample, skipped taps
                           only before sample 0 and, at a flush, behind the last sample) and returns the range of output
                           indices it produced.  A call that passes computes the whole-signal values by construction."""
import numpy as np

from tests import resample_contract as RC


class Refused(ValueError):
    pass


def _require(cond, msg):
    if not cond:
        raise Refused(msg)


def check_call(geom, lead, n_valid, final, g_first, n_out, hist_from, hist_len):
    """the size and range refusals of ws_resample_stream_fwd"""
    U, D, w, K = geom
    _require(n_valid > 0 and n_out >= 0 and hist_len >= 0 and n_out + hist_len > 0, "bad sizes")
    _require(0 <= lead <= w and g_first >= 0, "lead outside [0, w]")
    _require(hist_from >= 0 and hist_from + hist_len <= n_valid, "history leaves the valid samples")
    q_end = g_first * U + n_out
    if n_out > 0:
        if final:
            span = n_valid + lead - w
            _require(q_end <= (-(-U * span // D) if span > 0 else 0), "outputs past the end of the signal")
        else:
            _require(((q_end - 1) // U) * D - lead + K <= n_valid, "outputs need samples that are not valid and the end is not final")


def kernel_values(geom, taps, buf, lead, n_valid, final, g_first, n_out, memo=None, base=0):
    """[n_out] float64: per output the products of the taps (float64 [U, K]) that fall on buf[0, n_valid), summed in one
    fixed order.  A group's outputs are a function of (its samples, k_lo, k_hi) alone, so a caller that evaluates the same
    groups again and again may pass `memo` (a dict) and `base`, the signal's index of buf[0], which only names the entry:
    an entry is reused only when the samples now under the taps EQUAL the samples it was computed from."""
    U, D, w, K = geom
    out = np.zeros(n_out, dtype=np.float64)
    for i0 in range(0, n_out, U):
        g = g_first + i0 // U
        j0 = g * D - lead
        k_lo, k_hi = max(0, -j0), min(K, n_valid - j0)
        m = min(U, n_out - i0)
        if k_hi <= k_lo:
            continue
        seg = buf[j0 + k_lo:j0 + k_hi]
        if memo is not None:
            key = (base + j0 + k_lo, k_lo, k_hi)
            hit = memo.get(key)
            if hit is not None and len(hit[1]) >= m and np.array_equal(hit[0], seg):
                out[i0:i0 + m] = hit[1][:m]
                continue
        val = (taps[:m, k_lo:k_hi] * seg[None, :]).sum(axis=1)
        if memo is not None:
            memo[key] = (seg.copy(), val)
        out[i0:i0 + m] = val
    return out


def kernel_ranges(geom, buf0, lead, n_valid, final, g_first, n_out, n_total):
    """values=False: buf holds the indices buf0, buf0 + 1, ...; (first, last + 1) output index of the signal"""
    U, D, w, K = geom
    _require(lead == 0 or buf0 == 0, "taps before buf[0] are skipped, but buf[0] is not sample 0")
    c0 = buf0 + w - lead                                   # the signal's index of group 0's centre sample
    _require(c0 % D == 0, "the buffer does not start on a group")
    if final:
        _require(buf0 + n_valid == n_total, "taps behind the valid samples are skipped, but the signal does not end there")
    q0 = (c0 // D + g_first) * U
    return q0, q0 + n_out


class EmuStream:
    def __init__(self, rate_in, rate_out, max_push, values=True, memo=None):
        self.geom = RC.geometry(rate_in, rate_out)
        self.pair, self.max_push, self.values = (rate_in, rate_out), max_push, values
        self.taps = RC.taps32(rate_in, rate_out).astype(np.float64) if values else None      # the float-rounded table
        self.memo = memo
        K = self.geom[3]
        self.buf = [np.zeros(K - 1 + max_push, dtype=np.float64 if values else np.int64) for _ in range(2)]
        self.calls = 0
        self.reset()

    def reset(self):
        self.cur, self.h, self.n_in, self.groups = 0, 0, 0, 0

    def snapshot(self):
        return self.cur, self.h, self.n_in, self.groups, self.buf[self.cur][:self.h].copy()

    def restore(self, snap):
        self.cur, self.h, self.n_in, self.groups, hist = snap
        self.buf[self.cur][:self.h] = hist

    def history(self):
        return self.buf[self.cur][:self.h]

    def _step(self, piece, final):
        U, D, w, K = self.geom
        n = 0 if piece is None else len(piece)
        buf, h = self.buf[self.cur], self.h
        assert h + n <= len(buf)
        if n:
            buf[h:h + n] = piece
        N = self.n_in + n
        a0 = max(0, self.groups * D - w)
        lead = max(0, w - self.groups * D)
        if final:
            n_out, g_new, hist_from, hist_len = -(-U * N // D) - self.groups * U, self.groups, 0, 0
        else:
            g_new = max(0, (N - w) // D)
            n_out = (g_new - self.groups) * U
            hist_from = max(0, g_new * D - w) - a0
            hist_len = N - a0 - hist_from
        y = np.zeros(0) if self.values else (0, 0)
        if n_out or hist_len:
            check_call(self.geom, lead, h + n, final, 0, n_out, hist_from, hist_len)
            self.calls += 1
            if self.values:
                y = kernel_values(self.geom, self.taps, buf, lead, h + n, final, 0, n_out, self.memo, a0)
            elif n_out:
                y = kernel_ranges(self.geom, int(buf[0]), lead, h + n, final, 0, n_out, N)
            self.buf[1 - self.cur][:hist_len] = buf[hist_from:hist_from + hist_len]
        if not final:
            self.cur, self.h, self.groups = 1 - self.cur, hist_len, g_new
        self.n_in = N
        return y

    def push(self, chunk):
        outs = [self._step(chunk[o:o + self.max_push], False) for o in range(0, len(chunk), self.max_push)]
        if self.values:
            return np.concatenate(outs)
        outs = [o for o in outs if o[1] > o[0]]
        for a, b in zip(outs, outs[1:]):
            assert a[1] == b[0]
        return (outs[0][0], outs[-1][1]) if outs else (0, 0)

    def flush(self):
        if self.n_in == 0:
            return np.zeros(0) if self.values else (0, 0)
        return self._step(None, True)


def whole(x, rate_in, rate_out, memo=None):
    """the whole-signal form through the same kernel emulation: lead = w, final, group 0"""
    geom = RC.geometry(rate_in, rate_out)
    n_out = RC.out_len(len(x), rate_in, rate_out)
    check_call(geom, geom[2], len(x), True, 0, n_out, 0, 0)
    return kernel_values(geom, RC.taps32(rate_in, rate_out).astype(np.float64), np.asarray(x, dtype=np.float64), geom[2], len(x), True, 0,
                         n_out, memo, 0)
