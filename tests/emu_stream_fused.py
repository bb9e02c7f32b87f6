"""TEST INFRASTRUCTURE ONLY -- a torch-CPU emulation of `wesep_amd.dev.tcn_mid_stream_fwd` (csrc/stream.hip), stated from
the header's contract and not from the kernel, so that the host side of `ConvTasNetStreamer(fused=True)` can be checked
without a GPU.  `install` routes everything else through tests/emu_stream.py first, and can record the names of the
`dev` entry points a run calls (one name per C-ABI call on the device)."""
import types

import torch
import torch.nn.functional as F

from tests import emu_stream


def tcn_mid_stream_fwd(c, rb, a1, gamma1, beta1, wd, bd, a2, R, Tc, H, P, dil, eps, t0, ring, y2, st2):
    cap = ring.shape[1]
    assert ring.shape == (R, cap, H) and cap >= (P - 1) * dil + Tc and t0 >= 0 and H % 4 == 0 and P % 2 == 1
    before = c.clone()
    y1 = c.reshape(R, Tc, H) + (rb.reshape(R, 1, H) if rb is not None else 0.0)
    y1 = torch.where(y1 > 0, y1, a1.reshape(-1)[0] * y1)
    m1, v1 = y1.mean(2, keepdim=True), y1.var(2, unbiased=False, keepdim=True)
    xn = (y1 - m1) / torch.sqrt(v1 + eps) * gamma1 + beta1
    a = torch.arange(t0 - (P - 1) * dil, t0)
    past = torch.where((a >= 0)[None, :, None], ring[:, a % cap], torch.zeros(()))    # a < 0: a SELECTED zero
    seq = torch.cat([past, xn], 1).permute(0, 2, 1)
    z = F.conv1d(seq, wd.reshape(H, 1, P), bd, dilation=dil, groups=H).permute(0, 2, 1)
    y = torch.where(z > 0, z, a2.reshape(-1)[0] * z)
    y2.reshape(R, Tc, H)[:] = y
    st = st2.reshape(R * Tc, 2)
    st[:, 0] = y.mean(2).reshape(-1)
    st[:, 1] = (1.0 / torch.sqrt(y.var(2, unbiased=False) + eps)).reshape(-1)
    ring[:, (t0 + torch.arange(Tc)) % cap] = xn
    assert torch.equal(c, before)                                   # the contract: c is read only


def install(monkeypatch, record=None):
    """record: a list that receives the name of every `dev` function called (public callables of the module, after the
    emulations are in place), in call order."""
    import wesep_amd.dev as dev
    emu_stream.install(monkeypatch)
    monkeypatch.setattr(dev, "tcn_mid_stream_fwd", tcn_mid_stream_fwd)
    if record is None:
        return
    for name, fn in list(vars(dev).items()):
        if isinstance(fn, types.FunctionType) and not name.startswith("_"):
            monkeypatch.setattr(dev, name, _recorded(name, fn, record))


def _recorded(name, fn, record):
    def call(*a, **kw):
        record.append(name)
        return fn(*a, **kw)
    return call
