"""TEST INFRASTRUCTURE ONLY -- torch-CPU emulations of the two streaming entry points of `wesep_amd.dev`
(csrc/stream.hip), stated from the header's contract and not from the kernels: the host logic of
wesep_amd/streaming.py (pending samples, emission rule, rings, carry, flush) can then be checked against the model's own
whole-utterance forward on a machine without a GPU.  `install` routes everything else through tests/emu_dev.py first."""
import torch
import torch.nn.functional as F

from tests import emu_dev


def dwconv_stream_fwd(x, stats, gamma, beta, w, b, R, Tc, Cc, P, dil, st_div, t0, ring, y):
    cap = ring.shape[1]
    assert ring.shape == (R, cap, Cc) and cap >= (P - 1) * dil + Tc and t0 >= 0 and Cc % 4 == 0
    s = torch.arange(R * Tc) // st_div
    st = stats.reshape(-1, 2)
    xn = ((x.reshape(R * Tc, Cc) - st[s, 0:1]) * st[s, 1:2] * gamma + beta).reshape(R, Tc, Cc)
    a = torch.arange(t0 - (P - 1) * dil, t0)
    past = torch.where((a >= 0)[None, :, None], ring[:, a % cap], torch.zeros(()))    # a < 0: a SELECTED zero
    seq = torch.cat([past, xn], 1).permute(0, 2, 1)
    y.reshape(R, Tc, Cc)[:] = F.conv1d(seq, w.reshape(Cc, 1, P), b, dilation=dil, groups=Cc).permute(0, 2, 1)
    ring[:, (t0 + torch.arange(Tc)) % cap] = xn


def ola_stream_fwd(frames, bias, R, Tc, Lk, hop, carry, est):
    assert Lk >= hop and Lk % hop == 0
    nc, nfin = Lk - hop, Tc * hop
    full = torch.full((R, nfin + nc), float(bias.reshape(-1)[0]) if bias is not None else 0.0)
    if nc:
        full[:, :nc] = carry.reshape(R, nc)
    fr = frames.reshape(R, Tc, Lk)
    for t in range(Tc):
        full[:, t * hop: t * hop + Lk] += fr[:, t]
    est.reshape(R, nfin)[:] = full[:, :nfin]
    if nc:
        carry.reshape(R, nc)[:] = full[:, nfin:]


def install(monkeypatch):
    import wesep_amd.dev as dev
    emu_dev.install(monkeypatch)
    monkeypatch.setattr(dev, "dwconv_stream_fwd", dwconv_stream_fwd)
    monkeypatch.setattr(dev, "ola_stream_fwd", ola_stream_fwd)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))     # the models' own CUDA guards
