"""Audio at the caller's sample rate: the device resampler (csrc/resample.hip; include/wesep_hip.h, "sample rates").

The filter is the published sinc_interp_hann design with lowpass_filter_width = 6 and rolloff = 0.99, as a polyphase table
made once on the host in double (ws_resample_taps).  One output sample is one dot product reduced in one fixed order, so a
stream's output is bit for bit the whole-signal result whatever the packet sizes."""
import numpy as np
import torch

from . import dev

_TAPS = {}


def geometry(rate_in, rate_out):
    """(U, D, w, K): D = rate_in / gcd, U = rate_out / gcd, w = ceil(6 D / (0.99 min(D, U))), K = 2 w + D."""
    return dev.resample_geom(rate_in, rate_out)


def taps_on(rate_in, rate_out, device):
    """The device copy of the tap table, cached per (rate_in, rate_out, device)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (int(rate_in), int(rate_out), device)
    t = _TAPS.get(key)
    if t is None:
        t = _TAPS[key] = torch.from_numpy(dev.resample_taps(rate_in, rate_out)).to(device).contiguous()
    return t


def out_len(n_in, rate_in, rate_out):
    """ceil(U n_in / D): the samples of resample() for n_in input samples."""
    U, D, _, _ = geometry(rate_in, rate_out)
    return -(-U * int(n_in) // D)


def resample(x, rate_in, rate_out):
    """x [R, n] float32 on the device (rows of any pitch) -> [R, ceil(U n / D)]:
    y[q] = sum_k taps[q % U][k] x[(q // U) D + k - w], x = 0 outside [0, n)."""
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("resample: x is [R, n] with n >= 1")
    R, n = x.shape
    y = torch.empty(R, out_len(n, rate_in, rate_out), device=x.device, dtype=torch.float32)
    dev.resample_fwd(x, n, rate_in, rate_out, taps_on(rate_in, rate_out, x.device), y)
    return y


class StreamResampler:
    """resample() on audio as it arrives.  Emission rule: after N input samples, U max(0, floor((N - w) / D)) outputs have
    been returned (a group of U outputs is final once its last tap, input sample g D + w + D - 1, has arrived); flush()
    returns the rest up to ceil(U N / D), with the zero extension of the whole-signal call.  The concatenation of every
    push() and the flush() is bit for bit resample() of the concatenated input.  State: the last < K input samples (from
    max(0, G D - w) on, G the groups returned), kept on the device in one of two buffers [rows, K - 1 + max_push] used in
    turn -- the launch that computes a push's outputs also moves the new history to the other buffer.  A chunk above
    max_push is taken in pieces.  The sample and group counters are Python ints; the kernel sees buffer offsets only."""

    def __init__(self, rows, rate_in, rate_out, max_push=4800, device="cuda"):
        self.rows, self.rate_in, self.rate_out, self.max_push = int(rows), int(rate_in), int(rate_out), int(max_push)
        if self.rows < 1 or self.max_push < 1:
            raise ValueError("StreamResampler: rows >= 1 and max_push >= 1")
        self.U, self.D, self.w, self.K = geometry(rate_in, rate_out)
        self.taps = taps_on(rate_in, rate_out, device)
        self._buf = [torch.zeros(self.rows, self.K - 1 + self.max_push, device=self.taps.device, dtype=torch.float32)
                     for _ in range(2)]
        self.reset()

    def reset(self):
        self._cur, self._h, self.n_in, self.groups, self.done = 0, 0, 0, 0, False

    @property
    def history(self):
        """[rows, h] (a view): the input samples kept, h < K"""
        return self._buf[self._cur][:, :self._h]

    def _step(self, piece, final):
        n = 0 if piece is None else piece.shape[1]
        buf, h = self._buf[self._cur], self._h
        if n:
            buf[:, h:h + n] = piece
        N = self.n_in + n
        a0 = max(0, self.groups * self.D - self.w)          # the signal's sample index of buf[:, 0]
        lead = max(0, self.w - self.groups * self.D)
        if final:
            n_out = -(-self.U * N // self.D) - self.groups * self.U
            g_new, hist_from, hist_len = self.groups, 0, 0
        else:
            g_new = max(0, (N - self.w) // self.D)
            n_out = (g_new - self.groups) * self.U
            hist_from = max(0, g_new * self.D - self.w) - a0
            hist_len = N - a0 - hist_from
        y = torch.empty(self.rows, n_out, device=buf.device, dtype=torch.float32)
        if n_out or hist_len:
            dev.resample_stream_fwd(buf, self.rate_in, self.rate_out, self.taps, lead, h + n, final, 0, n_out,
                                    y if n_out else None, hist_from, hist_len, self._buf[1 - self._cur] if hist_len else None)
        if not final:
            self._cur, self._h, self.groups = 1 - self._cur, hist_len, g_new
        self.n_in = N
        return y

    def push(self, chunk):
        """chunk [rows, n >= 1] on the device -> [rows, m], the samples that became final (m may be 0)."""
        if self.done:
            raise ValueError("StreamResampler.push: the stream was flushed (reset() starts another)")
        if chunk.dim() != 2 or chunk.shape[0] != self.rows or chunk.shape[1] < 1:
            raise ValueError(f"StreamResampler.push: chunk is {tuple(chunk.shape)}, expected [{self.rows}, n >= 1]")
        outs = [self._step(chunk[:, o:o + self.max_push], False) for o in range(0, chunk.shape[1], self.max_push)]
        return outs[0] if len(outs) == 1 else torch.cat(outs, dim=1)

    def flush(self):
        """The end of the signal: the outputs up to ceil(U N / D)."""
        if self.done:
            raise ValueError("StreamResampler.flush: the stream was flushed already")
        self.done = True
        if self.n_in == 0:
            return torch.empty(self.rows, 0, device=self.taps.device, dtype=torch.float32)
        return self._step(None, True)


def step_plan(geom, n_in, groups, h, n_new, final):
    """The arguments of one streaming step, from the counters alone (the rule of StreamResampler._step and runtime/rate.cc):
    (lead, n_valid, n_out, hist_from, hist_len, groups after the step) for n_new samples behind a history of h."""
    U, D, w, _ = geom
    N = n_in + n_new
    a0 = max(0, groups * D - w)
    lead = max(0, w - groups * D)
    if final:
        return lead, h + n_new, -(-U * N // D) - groups * U, 0, 0, groups
    g_new = max(0, (N - w) // D)
    hist_from = max(0, g_new * D - w) - a0
    return lead, h + n_new, (g_new - groups) * U, hist_from, N - a0 - hist_from, g_new


class StreamResamplerRows:
    """Many StreamResamplers with one row each, every row at its own pair of rates, in ONE launch per round
    (ws_resample_stream_rows_fwd).  pairs[i] = (rate_in, rate_out) of row i; a row with rate_in == rate_out runs the identity
    table U = D = K = 1 (no delay, no filter: its outputs are its inputs).  Per row the bookkeeping of StreamResampler; the
    histories of all rows live in one arena, two buffers [K_i - 1 + max_push] a row used in turn, and the tables of the
    distinct pairs in another.  A row's outputs are bit for bit those of StreamResampler(1, *pairs[i], max_push) fed the same
    chunks, whatever the other rows are and carry.  A chunk above max_push is taken in pieces: round j carries piece j of every
    row that has one."""

    def __init__(self, pairs, max_push=4800, device="cuda"):
        self.pairs, self.max_push = [(int(a), int(b)) for a, b in pairs], int(max_push)
        if not self.pairs or self.max_push < 1:
            raise ValueError("StreamResamplerRows: at least one row and max_push >= 1")
        device = torch.device(device)
        tables, self.geom, self._taps_off, off = [], [], [], {}
        for pair in self.pairs:
            ident = pair[0] == pair[1]
            self.geom.append((1, 1, 0, 1) if ident else geometry(*pair))
            key = "identity" if ident else pair
            if key not in off:
                off[key] = sum(t.size for t in tables)
                tables.append(np.ones(1, dtype=np.float32) if ident else dev.resample_taps(*pair).reshape(-1))
            self._taps_off.append(off[key])
        self.taps = torch.from_numpy(np.concatenate(tables)).to(device)
        self._ld = [g[3] - 1 + self.max_push for g in self.geom]
        self._base = [2 * sum(self._ld[:i]) for i in range(len(self.pairs))]
        self.buf = torch.zeros(2 * sum(self._ld), device=device, dtype=torch.float32)
        self.launches = 0
        self._st = [None] * len(self.pairs)
        for i in range(len(self.pairs)):
            self.reset(i)

    def reset(self, row):
        self._st[row] = dict(cur=0, h=0, n_in=0, groups=0, done=False)

    def _at(self, row, which):
        return self._base[row] + which * self._ld[row]

    def history(self, row):
        """[h] (a view): the input samples row `row` keeps, h < K"""
        st = self._st[row]
        o = self._at(row, st["cur"])
        return self.buf[o:o + st["h"]]

    def _round(self, pieces, final):
        """pieces: {row: [n] tensor} (final: {row: None}) -> {row: [m] tensor}"""
        plan, n_y = [], 0
        for row, piece in pieces.items():
            st, n = self._st[row], 0 if piece is None else piece.shape[0]
            o = self._at(row, st["cur"])
            if n:
                self.buf[o + st["h"]:o + st["h"] + n] = piece
            lead, n_valid, n_out, hist_from, hist_len, g_new = step_plan(self.geom[row], st["n_in"], st["groups"], st["h"], n, final)
            plan.append((row, n_y, n_out, hist_len, g_new, n))
            if n_out or hist_len:
                U, D, _, K = self.geom[row]
                plan[-1] += (dict(in_off=o, taps_off=self._taps_off[row], out_off=n_y, hist_off=self._at(row, 1 - st["cur"]), U=U, D=D,
                                  K=K, lead=lead, n_valid=n_valid, final=int(final), n_out=n_out, hist_from=hist_from,
                                  hist_len=hist_len),)
            n_y += n_out
        y = torch.empty(n_y, device=self.buf.device, dtype=torch.float32)
        table = [p[6] for p in plan if len(p) == 7]
        if table:
            dev.resample_stream_rows_fwd(table, self.buf, self.taps, y, self.buf)
            self.launches += 1
        out = {}
        for p in plan:
            row, y_off, n_out, hist_len, g_new, n = p[:6]
            st = self._st[row]
            if not final and len(p) == 7:
                st["cur"], st["h"], st["groups"] = 1 - st["cur"], hist_len, g_new
            st["n_in"] += n
            out[row] = y[y_off:y_off + n_out]
        return out

    def push(self, chunks):
        """chunks: {row: [n >= 1] tensor on the device} -> {row: [m] tensor}, the samples that became final (m may be 0)."""
        for row, c in chunks.items():
            if self._st[row]["done"]:
                raise ValueError(f"StreamResamplerRows.push: row {row} was flushed (reset({row}) starts another)")
            if c.dim() != 1 or c.shape[0] < 1:
                raise ValueError(f"StreamResamplerRows.push: the chunk of row {row} is {tuple(c.shape)}, expected [n >= 1]")
        outs = {row: [] for row in chunks}
        for j in range(max(-(-c.shape[0] // self.max_push) for c in chunks.values())):
            lo = j * self.max_push
            got = self._round({row: c[lo:lo + self.max_push] for row, c in chunks.items() if c.shape[0] > lo}, False)
            for row, y in got.items():
                outs[row].append(y)
        return {row: ys[0] if len(ys) == 1 else torch.cat(ys) for row, ys in outs.items()}

    def flush(self, rows):
        """The end of the signal of every row in `rows`, in one launch: {row: the outputs up to ceil(U N / D)}."""
        for row in rows:
            if self._st[row]["done"]:
                raise ValueError(f"StreamResamplerRows.flush: row {row} was flushed already")
            self._st[row]["done"] = True
        out = self._round({row: None for row in rows if self._st[row]["n_in"]}, True)
        empty = torch.empty(0, device=self.buf.device, dtype=torch.float32)
        return {row: out.get(row, empty) for row in rows}
