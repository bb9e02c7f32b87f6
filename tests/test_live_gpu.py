"""GPU: ws_xfade_stream_fwd (wesep_amd/csrc/longform.hip) against ws_xfade_ola on the same window estimates, bit
for bit: the ranges the live rule emits, read from a ring of g_max + 3 slots that wraps, every stale or unused slot NaN."""
import numpy as np
import pytest
import torch

from tests import emu_live as M
from tests.test_longform_gpu import SHAPES, _cuda
from wesep_amd import dev

pytestmark = pytest.mark.gpu
NAN = float("nan")
LIVE_SHAPES = SHAPES + [(64, 16, 64 + 3 * 48), (64, 16, 64 + 3 * 48 + 1), (64, 32, 300), (64, 0, 257), (65, 32, 400)]   # (S, O, n)


def _live_ranges(y, S, O, n, g_max, sc, d):
    """The rule of include/wesep_engine.h over the estimates y [K][W][L], windows entering the ring in groups of at most g_max:
    out [K][n], every range written by one ws_xfade_stream_fwd call; the calls made."""
    K, W, Lw = y.shape
    H, cap = S - O, g_max + 3
    ring = torch.full((K, cap, S), NAN, device=d)
    scale_ring = None if sc is None else torch.full((cap,), NAN, device=d)
    out = torch.full((K, n), NAN, device=d)
    flat = out.view(-1)

    def put(w, Lc):
        ring[:, w % cap] = NAN                                   # what the slot held is gone
        ring[:, w % cap, :Lc] = y[:, w, :Lc]
        if sc is not None:
            scale_ring[w % cap] = sc[w]

    run, E, calls = 0, 0, 0
    target = M.windows_run(n, S, H)
    while run < target:
        g = min(target - run, g_max, cap - run % cap)
        for w in range(run, run + g):
            put(w, S)
        run += g
        to = (run - 1) * H
        dev.xfade_stream_fwd(ring, K, cap, S, O, E, to - E, run, flat[E:], n, scale_ring=scale_ring)
        calls += to > E
        E = to
    if n < S:
        put(0, n)
        run = 1
    elif (n - S) % H:
        put(run, S)
        run += 1
    assert run == W
    dev.xfade_stream_fwd(ring, K, cap, S, O, E, n - E, run, flat[E:], n, final=(W, n), scale_ring=scale_ring)
    torch.cuda.synchronize()
    return out, calls + 1


@pytest.mark.parametrize("S,O,n", LIVE_SHAPES)
def test_xfade_stream_equals_xfade_ola_bit_for_bit(S, O, n):
    d = _cuda()
    K, H = 2, S - O
    W, Lw = M.total_windows(n, S, H), min(n, S)
    g = torch.Generator().manual_seed(3 * S + O + n)
    y = torch.randn(K, W, Lw, generator=g).to(d)
    for sc in (None, (0.5 + torch.rand(W, generator=g)).to(d)):
        want = torch.full((K, n), NAN, device=d)
        dev.xfade_ola(y, K, W, S, O, n, want, scale=sc)
        torch.cuda.synchronize()
        assert torch.isfinite(want).all()
        for g_max in (1, 3):
            got, calls = _live_ranges(y, S, O, n, g_max, sc, d)
            assert torch.isfinite(got).all(), (S, O, n, g_max)                       # complete, and no NaN slot was read
            assert torch.equal(got, want), (S, O, n, g_max, sc is not None, float((got - want).abs().max()))
            if W > g_max + 3:
                assert calls > 2                                                      # the ring wrapped


def test_xfade_stream_single_ranges_and_row_pitch():
    """One call over an inner range with a row pitch wider than the range: columns outside stay untouched."""
    d = _cuda()
    S, O, n, K, cap = 512, 128, 2000, 2, 8
    H, W = S - O, M.total_windows(2000, 512, 384)
    y = torch.randn(K, W, S, generator=torch.Generator().manual_seed(1)).to(d)
    want = torch.empty(K, n, device=d)
    dev.xfade_ola(y, K, W, S, O, n, want)
    ring = torch.full((K, cap, S), NAN, device=d)
    ring[:, :W] = y
    out = torch.full((K, 1000), NAN, device=d)
    dev.xfade_stream_fwd(ring, K, cap, S, O, 301, 777, W, out, 1000, final=(W, n))
    torch.cuda.synchronize()
    assert torch.equal(out[:, :777], want[:, 301:301 + 777]) and torch.isnan(out[:, 777:]).all()
    # while the recording runs, the range ends at the newest window's start; the weights there know no last window
    run = 3
    out = torch.full((K, (run - 1) * H), NAN, device=d)
    dev.xfade_stream_fwd(ring, K, cap, S, O, 0, (run - 1) * H, run, out, (run - 1) * H)
    ref = M.xfade_stream(ring.double().cpu().numpy(), S, O, 0, (run - 1) * H, run)
    torch.cuda.synchronize()
    assert np.abs(out.double().cpu().numpy() - ref).max() < 1e-5
    assert torch.equal(out, want[:, :(run - 1) * H])            # (windows 0 .. 2 are regular in the final layout too)
