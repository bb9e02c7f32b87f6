"""Audio at the caller's sample rate: the device resampler (csrc/resample.hip; include/wesep_hip.h, "sample rates").

The filter is the published sinc_interp_hann design with lowpass_filter_width = 6 and rolloff = 0.99, as a polyphase table
made once on the host in double (ws_resample_taps).  One output sample is one dot product reduced in one fixed order, so a
stream's output is bit for bit the whole-signal result whatever the packet sizes."""
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
