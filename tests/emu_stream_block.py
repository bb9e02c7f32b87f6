"""TEST INFRASTRUCTURE ONLY -- a torch restatement of the two whole-block entry points of `wesep_amd.dev`
(csrc/stream_block.hip: tcn_block_stream_fwd, tcn_block_stream_rows_fwd), stated from the header's text and not from the
kernel, alongside tests/emu_stream_fused.py and tests/emu_stream_pool.py.  It computes in the dtype of its inputs: float64
inputs make it the reference the GPU tests compare the kernel with, float32 inputs the emulation that `install` plugs into
`wesep_amd.dev` so the host side of `ConvTasNetStreamer(block=True)` runs without a GPU.  Written row by row, frame by frame
and tap by tap: the tap rules and the tables' rules are spelled out, not vectorised away."""
import types

import torch

from tests import emu_stream_fused
from tests.emu_stream_pool import _prelu, _row


def _norm(v, eps, gamma, beta):
    """(v - mean) * (1 / sqrt(biased var + eps)) * gamma + beta over the channels of every frame of v [n, C]"""
    return (v - v.mean(1, keepdim=True)) * (1.0 / torch.sqrt(v.var(1, unbiased=False, keepdim=True) + eps)) * gamma + beta


def _block_row(xr, bias, W1, a1, gamma1, beta1, wd, bd, a2, gamma2, beta2, W2, b2, B, P, dil, eps, first, ring_row, outr):
    """n = xr.shape[0] frames of one row from absolute frame `first` on; ring_row [cap, H] is read, then written."""
    n, cap, H = xr.shape[0], ring_row.shape[0], W1.shape[0]
    xn = _norm(_prelu(xr @ W1[:, :B].T + bias, a1), eps, gamma1, beta1)
    z = bd.expand(n, H).clone()
    for p in range(P):                                              # ascending p
        off = (P - 1 - p) * dil
        for t in range(n):
            a = first + t - off
            if a < 0:                                               # before the start: no term, no read
                continue
            z[t] += wd[:, p] * (xn[t - off] if off <= t else ring_row[a % cap])      # a >= first: a chunk frame
    outr[:n] = xr + b2 + _norm(_prelu(z, a2), eps, gamma2, beta2) @ W2.T
    ring_row[(first + torch.arange(n)) % cap] = xn                  # after every read of this row


def _check(x, rb, W1, b1, wd, W2, Tc, B, H, P, dil, ring, out):
    cap = ring.shape[1]
    assert (rb is None) != (b1 is None) and W1.shape[0] == H and W1.shape[1] >= B and W1.shape[1] % 4 == 0
    assert B % 4 == 0 and H % 4 == 0 and P % 2 == 1 and P <= 7 and dil >= 1 and cap >= (P - 1) * dil + Tc
    assert ring.shape[2] == H and W2.shape == (B, H) and wd.shape == (H, P)
    assert out.data_ptr() != x.data_ptr()


def tcn_block_stream_fwd(x, rb, W1, b1, a1, gamma1, beta1, wd, bd, a2, gamma2, beta2, W2, b2, R, Tc, B, H, P, dil, eps, t0,
                         ring, out):
    _check(x, rb, W1, b1, wd, W2, Tc, B, H, P, dil, ring, out)
    assert ring.shape[0] == R and t0 >= 0
    before = x.clone()
    xs, ov = x.reshape(R, Tc, B), out.reshape(R, Tc, B)
    for r in range(R):
        _block_row(xs[r], rb.reshape(R, H)[r] if rb is not None else b1, W1, a1, gamma1, beta1, wd, bd, a2, gamma2, beta2, W2, b2,
                   B, P, dil, eps, t0, ring[r], ov[r])
    assert torch.equal(x, before)                                   # the contract: x is read only


def tcn_block_stream_rows_fwd(x, rb, W1, b1, a1, gamma1, beta1, wd, bd, a2, gamma2, beta2, W2, b2, A, Tc, B, H, P, dil, eps,
                              slot, t0, tc, ring, out):
    _check(x, rb, W1, b1, wd, W2, Tc, B, H, P, dil, ring, out)
    nslots = ring.shape[0]
    assert A >= 1 and nslots >= 1
    xs, ov = x.reshape(A, Tc, B), out.reshape(A, Tc, B)
    for i in range(A):
        sl, first, n = _row(slot, t0, tc, i, nslots, Tc)
        ov[i, n:] = 0.0
        if n == 0:                                                  # no state row is touched
            continue
        _block_row(xs[i, :n], rb.reshape(nslots, H)[sl] if rb is not None else b1, W1, a1, gamma1, beta1, wd, bd, a2, gamma2,
                   beta2, W2, b2, B, P, dil, eps, first, ring[sl], ov[i])


def install(monkeypatch, record=None):
    """tests/emu_stream_fused.install, then the two entry points above; record as there."""
    import wesep_amd.dev as dev
    emu_stream_fused.install(monkeypatch)
    monkeypatch.setattr(dev, "tcn_block_stream_fwd", tcn_block_stream_fwd)
    monkeypatch.setattr(dev, "tcn_block_stream_rows_fwd", tcn_block_stream_rows_fwd)
    if record is None:
        return
    for name, fn in list(vars(dev).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith("_"):
            monkeypatch.setattr(dev, name, emu_stream_fused._recorded(name, fn, record))
