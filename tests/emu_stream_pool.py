"""TEST INFRASTRUCTURE ONLY -- a torch restatement of the two stream-pool entry points of `wesep_amd.dev`
(csrc/stream.hip: tcn_mid_stream_rows_fwd, ola_stream_rows_fwd), stated from the header's contract and not from the kernels,
alongside tests/emu_stream.py and tests/emu_stream_fused.py.  It computes in the dtype of its inputs: float64 inputs make it
the reference the GPU tests compare the kernels with.  Written row by row and tap by tap -- the tables' rules (an entry that
names no slot skips the row, tc is clamped, frames behind tc[i] come out as zeros and (0, 1)) are spelled out, not vectorised
away."""
import torch


def _row(slot, t0, tc, i, nslots, Tc):
    """(state slot, first frame, valid frames) of row i after the header's rules for a table entry."""
    sl, first, n = int(slot[i]), int(t0[i]), min(max(int(tc[i]), 0), Tc)
    if not 0 <= sl < nslots or first < 0:
        n = 0
    return sl, first, n


def _prelu(v, a):
    return torch.where(v > 0, v, a.reshape(-1)[0] * v)


def tcn_mid_stream_rows_fwd(c, rb, a1, gamma1, beta1, wd, bd, a2, A, Tc, H, P, dil, eps, slot, t0, tc, ring, y2, st2):
    nslots, cap = ring.shape[0], ring.shape[1]
    assert ring.shape == (nslots, cap, H) and cap >= (P - 1) * dil + Tc and H % 4 == 0 and P % 2 == 1 and A >= 1
    before = c.clone()
    cs, yv, sv = c.reshape(A, Tc, H), y2.reshape(A, Tc, H), st2.reshape(A, Tc, 2)
    for i in range(A):
        sl, first, n = _row(slot, t0, tc, i, nslots, Tc)
        yv[i, n:] = 0.0
        sv[i, n:, 0] = 0.0
        sv[i, n:, 1] = 1.0
        if n == 0:
            continue
        y1 = _prelu(cs[i, :n] + (rb.reshape(nslots, H)[sl] if rb is not None else 0.0), a1)
        xn = (y1 - y1.mean(1, keepdim=True)) / torch.sqrt(y1.var(1, unbiased=False, keepdim=True) + eps) * gamma1 + beta1
        z = bd.expand(n, H).clone()
        for p in range(P):                                          # ascending p, the header's order
            off = (P - 1 - p) * dil
            for t in range(n):
                a = first + t - off
                if a < 0:                                           # before the start: no term, the ring is not read
                    continue
                z[t] += wd[:, p] * (xn[t - off] if off <= t else ring[sl, a % cap])
        y = _prelu(z, a2)
        yv[i, :n] = y
        sv[i, :n, 0] = y.mean(1)
        sv[i, :n, 1] = 1.0 / torch.sqrt(y.var(1, unbiased=False) + eps)
        ring[sl, (first + torch.arange(n)) % cap] = xn               # after every read of this row
    assert torch.equal(c, before) or torch.isnan(before).any()      # the contract: c is read only


def ola_stream_rows_fwd(frames, bias, A, Tc, Lk, hop, slot, t0, tc, carry, est):
    assert Lk >= hop and Lk % hop == 0 and A >= 1
    nslots, nc = carry.shape[0], Lk - hop
    fr, ev = frames.reshape(A, Tc, Lk), est.reshape(A, Tc * hop)
    b = bias.reshape(-1)[0] if bias is not None else 0.0
    for i in range(A):
        sl, _, n = _row(slot, t0, tc, i, nslots, Tc)
        ev[i, n * hop:] = 0.0
        if n == 0:                                                  # the carry row is neither read nor written
            continue
        full = torch.zeros(n * hop + nc, dtype=frames.dtype) + b
        full[:nc] = carry[sl]
        for t in range(n):                                          # ascending frame
            full[t * hop: t * hop + Lk] += fr[i, t]
        ev[i, :n * hop] = full[:n * hop]
        carry[sl] = full[n * hop:]
