"""CPU-only: live windows (runtime/live.cc, ws_xfade_stream_fwd).  The C ABI, the emission rule restated
(tests/emu_live.py) against the float64 cross-fade of tests/longform_ref.py, the dry-run launch plan of every architecture,
the refusals and `separate_main --dry_run --live_ms`.  The tests that touch the libraries, the binding or the tool fail on the
commit before (the symbols do not exist); the two tests of the rule itself compare tests/emu_live.py with
tests/longform_ref.py and state what the runtime has to do.  tests/test_live_gpu.py and tests/test_zzz_live_engine_gpu.py
hold the device to the same rule."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import emu_live as M
from tests import longform_ref as R
from wesep_amd import _lib as L
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
GEOMS = [(64, 16), (64, 0), (64, 32), (50, 7), (65, 32)]          # (S, O)
# the smallest containers the plans take, fixed embeddings: the ENGINE_CASES geometries of tests/test_longform_gpu.py
ENGINE_CASES = {
    "pBSRNN": ("BSRNN", dict(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False), 6000, 2048, 512),
    "ConvTasNet": ("ConvTasNet", dict(N=32, L=20, B=32, H=64, P=3, X=2, R=1), 5003, 2000, 500),
    "DPCCN": ("DPCCN", dict(tcn_blocks=1, tcn_layers=1), 9000, 4096, 1024),
    "TFGridNet": ("TFGridNet", dict(n_layers=1, emb_dim=128, emb_ks=1, emb_hs=1, lstm_hidden_units=64, spk_emb_dim=256), 5000, 2048,
                  512),
}
last = lambda: E.lib().ws_engine_last_error().decode()


def _container(tmp_path, arch):
    from wesep_amd.models import get_model
    name, kw = ENGINE_CASES[arch][:2]
    path = str(tmp_path / f"{arch}.wsw")
    export_engine(get_model(name)(joint_training=False, **kw), path)
    return path


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_live_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    m = re.search(r"^int\s+ws_xfade_stream_fwd\s*\(([^;]*)\);", header, flags=re.M)
    assert m, "ws_xfade_stream_fwd is not declared in wesep_hip.h"
    res, args = L._SIGS["ws_xfade_stream_fwd"]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(","))
    assert getattr(L.lib(), "ws_xfade_stream_fwd") is not None
    from wesep_amd import dev
    assert callable(dev.xfade_stream_fwd)
    eheader = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    for name in ("ws_engine_live_open", "ws_engine_live_push", "ws_engine_live_flush", "ws_engine_live_reset"):
        assert re.search(r"^int\s+" + name + r"\s*\(", eheader, flags=re.M), name
    assert re.search(r"^void\s+ws_engine_live_close\s*\(", eheader, flags=re.M)
    for name in ("ws_engine_live_open", "ws_engine_live_push", "ws_engine_live_flush", "ws_engine_live_reset", "ws_engine_live_close"):
        assert name in E.SYMBOLS and getattr(E.lib(), name) is not None
    assert re.search(r"^#define WS_LIVE_PUSH_CAP\(n, H\) \(\(\(n\) / \(H\) \+ 1\) \* \(H\)\)", eheader, flags=re.M)
    assert re.search(r"^#define WS_LIVE_FLUSH_CAP\(S, O\) \(2 \* \(S\) - \(O\)\)", eheader, flags=re.M)
    assert E.live_push_cap(100, 48) == 144 and E.live_flush_cap(64, 16) == 112
    assert callable(E.Engine.live) and all(callable(getattr(E.EngineLive, f)) for f in ("push", "flush", "reset", "close"))
    assert L.lib().ws_abi_version() == 20                     # new symbols only: neither ABI number moves
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


def test_xfade_stream_refuses_bad_arguments_before_any_launch():
    lib = L.lib()
    buf, buf2 = (ctypes.c_float * 8192)(), (ctypes.c_float * 8192)()
    p, p2 = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)
    err = lambda: lib.ws_last_error().decode()
    # ws_xfade_stream_fwd(ring, K, cap, S, O, scale_ring, i0, count, windows_run, final, W, n, out, ld_out, stream); S 64, O 16: H 48
    f = lambda *a: lib.ws_xfade_stream_fwd(*a, None)
    assert f(None, 2, 4, 64, 16, None, 0, 48, 2, 0, 0, 0, p2, 48) == -1 and "ring or out is NULL" in err()
    assert f(p, 2, 4, 64, 16, None, 0, 48, 2, 0, 0, 0, None, 48) == -1 and "ring or out is NULL" in err()
    assert f(p, 2, 4, 64, 33, None, 0, 10, 2, 0, 0, 0, p2, 48) == -1 and "overlap O=33 outside" in err()
    assert f(p, 2, 4, 64, -1, None, 0, 10, 2, 0, 0, 0, p2, 48) == -1 and "overlap O=-1 outside" in err()
    assert f(p, 2, 4, 64, 16, None, 0, -1, 2, 0, 0, 0, p2, 48) == -1 and "bad range" in err()
    assert f(p, 2, 4, 64, 16, None, 0, 49, 2, 0, 0, 0, p2, 49) == -1 and "reaches past the 48 samples that the 2 windows" in err()
    assert f(p, 2, 4, 64, 16, None, 0, 1, 0, 0, 0, 0, p2, 1) == -1 and "reaches past the 0 samples" in err()
    # windows 0 .. 5 are read by [0, 240) with 6 run: more than 4 slots; and [0, 48) with 6 run needs window 0, long gone
    assert f(p, 2, 4, 64, 16, None, 0, 240, 6, 0, 0, 0, p2, 240) == -1 and "cap=4 slots do not hold windows 0..4" in err()
    assert f(p, 2, 4, 64, 16, None, 0, 48, 6, 0, 0, 0, p2, 48) == -1 and "cap=4 slots do not hold" in err()
    # final: (W, n) must be the layout, with every window run
    assert f(p, 2, 4, 64, 16, None, 96, 70, 3, 1, 4, 166, p2, 70) == -1 and "a final range needs all W=4 windows" in err()
    assert f(p, 2, 4, 64, 16, None, 96, 70, 4, 1, 5, 166, p2, 70) == -1 and "a final range needs all W=5 windows" in err()
    assert f(p, 2, 4, 64, 16, None, 96, 71, 4, 1, 4, 166, p2, 71) == -1 and "reaches past the recording's n=166" in err()
    assert f(p, 2, 4, 64, 16, None, 0, 0, 2, 0, 0, 0, p2, 0) == 0                       # nothing to do: no launch


# ---- the emission rule, restated -----------------------------------------------------------------------------------------
def _reference(S, O, n, K, seed):
    """window estimates [K][W][L] (a function of the window's index and samples), per-window factors, and the float64 cross-fade"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n)
    st, Lw = R.starts(n, S, O), min(n, S)
    mixers = rng.standard_normal((K, 3))
    sep = lambda w, xs: np.stack([m[0] * xs + m[1] * np.cos(0.1 * (w + 1) * np.arange(len(xs))) + m[2] for m in mixers])
    y = np.stack([sep(w, x[s:s + Lw]) for w, s in enumerate(st)], axis=1)
    scale = lambda w: 0.5 + ((w * 7919) % 13) / 13.0
    return x, sep, scale, y


@pytest.mark.parametrize("S,O", GEOMS)
def test_emission_rule_equals_the_whole_recording_crossfade_exactly(S, O):
    """Every n from S - 5 to 5 S + 3.  The 1-sample schedule (n pushes each) runs on the lengths around the first window and
    the first hop and on three long ones; every other schedule runs on the whole range."""
    K, H = 2, S - O
    dense = set(range(S - 5, S + 3)) | {S + H - 1, S + H, S + H + 1, 2 * S, 3 * S + 1, 5 * S + 3}
    checked = on_a_hop = 0
    for n in range(S - 5, 5 * S + 4):
        x, sep, scale, y = _reference(S, O, n, K, 1000 * S + n)
        W = len(R.starts(n, S, O))
        on_a_hop += W >= 3 and (n - S) % H == 0                  # a flush that runs no further window
        want = R.xfade(y, n, S, O)
        want_s = R.xfade(y * np.array([scale(w) for w in range(W)])[None, :, None], n, S, O)
        for name, sched in M.schedules(n, n).items():
            if name == "1" and n not in dense:
                continue
            for g_max in (1, 2, 5):
                for sc, ref in ((None, want), (scale, want_s)):
                    lv = M.Live(K, S, O, g_max, sep, scale=sc)
                    parts, N = [], 0
                    for c in sched:
                        before = M.emitted(N, S, H)
                        got = lv.push(x[N:N + c])
                        N += c
                        assert got.shape == (K, M.emitted(N, S, H) - before)          # n_out = E(N_new) - E(N_old)
                        assert max(lv.groups, default=0) <= g_max
                        parts.append(got)
                    parts.append(lv.flush())
                    out = np.concatenate(parts, axis=1)
                    assert lv.Wr == W and out.shape == (K, n), (S, O, n, name, g_max)
                    assert np.isfinite(out).all(), (S, O, n, name, g_max)                  # no NaN slot was read
                    assert np.array_equal(out, ref), (S, O, n, name, g_max, np.abs(out - ref).max())
                    checked += 1
    assert checked == ((4 * S + 9) * 4 + len(dense)) * 3 * 2 and on_a_hop >= 3


def test_emitted_samples_have_every_covering_window_run_with_its_tail_ramp():
    for S, O in GEOMS:
        H = S - O
        for N in range(1, 6 * S):
            Wr, Em = M.windows_run(N, S, H), M.emitted(N, S, H)
            assert Wr == sum(1 for w in range(N) if w * H + S <= N)
            # whatever the final length n >= N: every window that covers a sample below E has run, and is not the last one
            for n in (N, N + 1, N + H - 1, N + H, N + 3 * S + 1):
                st = R.starts(n, S, O)
                if n < S:
                    assert Em == 0
                    continue
                for w, s in enumerate(st):
                    if s < Em:                                         # may cover an emitted sample
                        assert w < Wr and s == w * H and (w < len(st) - 1 or s >= Em)
            assert N - Em < S + H or Wr == 0                           # latency between S and S + H samples
            assert max(Wr - 2, 0) * H + S >= Em or Wr < 2              # windows >= Wr - 2 may still be needed, none older
            if Wr >= 3:
                assert (Wr - 3) * H + S <= Em


# ---- dry-run engines: counts ---------------------------------------------------------------------------------------------
def _push(h, x, cap):
    est, m = np.zeros((2, max(cap, 1)), np.float32), ctypes.c_int(-1)
    rc = E.lib().ws_engine_live_push(h, x.ctypes.data, len(x), est.ctypes.data, cap, ctypes.byref(m))
    return rc, m.value


def _flush(h, cap):
    est, m = np.zeros((2, max(cap, 1)), np.float32), ctypes.c_int(-1)
    rc = E.lib().ws_engine_live_flush(h, est.ctypes.data, cap, ctypes.byref(m))
    return rc, m.value


@needs_no_gpu
@pytest.mark.parametrize("arch", sorted(ENGINE_CASES))
def test_dry_run_live_counts(tmp_path, arch):
    _, _, n, S, O = ENGINE_CASES[arch]
    H, K = S - O, 2
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    emb = np.zeros((K, 256), np.float32)
    n_rect = {}
    for G in (1, 2, 4, 6, 8):
        eng.separate(np.ones((G, S), np.float32), np.zeros((G, 256), np.float32), E.ENROLL_EMBEDDING)
        n_rect[G] = eng.info("n_launches")
    for max_rows in (8, 1):
        g_max = max(1, max_rows // K)
        per_group = E.live_group_launches(K, max_rows)
        assert per_group == (3 if max_rows > 1 else 2)

        def launches(groups):      # the documented formula
            fw = lambda g: n_rect[K * g] if K * g <= max_rows else -(-K * g // max_rows) * n_rect[max_rows]
            return sum(fw(g) + per_group for g in groups) + 1

        def groups_of(w0, w1):     # groups of at most g_max windows, cut where the ring of g_max + 3 slots wraps
            out = []
            while w0 < w1:
                g = min(w1 - w0, g_max, g_max + 3 - w0 % (g_max + 3))
                out.append(g)
                w0 += g
            return out

        lv = eng.live(emb, E.ENROLL_EMBEDDING, S, O, max_rows)
        state = eng.info("live_state_bytes")
        assert state > K * (g_max + 3) * S * 4 and eng.info("n_launches") == 0        # fixed embeddings: no speaker stage
        counts = {}
        for name, sched in [(k, v) for k, v in M.schedules(n, 3).items() if k != "1"] + [("again", M.schedules(n, 3)["random"])]:
            if name == "again":
                lv.reset()
                assert eng.info("live_windows") == 0
            N, total, trace = 0, 0, []
            for c in sched:
                w_old, e_old = M.windows_run(N, S, H), M.emitted(N, S, H)
                got = lv.push(np.ones(c, np.float32))
                N += c
                w_new = M.windows_run(N, S, H)
                assert got.shape == (K, M.emitted(N, S, H) - e_old) and not got.any()   # a dry run computes nothing
                total += got.shape[1]
                gs = groups_of(w_old, w_new)
                assert eng.info("live_groups") == len(gs) and eng.info("live_windows") == w_new
                assert eng.info("n_launches") == (launches(gs) if gs else 0), (arch, name, N, gs)   # no window: no launch
                trace.append(eng.info("n_launches"))
                assert eng.info("live_state_bytes") == state
            tail = lv.flush()
            extra = [1] if N < S or (N - S) % H else []
            assert eng.info("n_launches") == launches(extra) and eng.info("live_groups") == len(extra)
            assert eng.info("live_windows") == len(R.starts(N, S, O))
            assert total + tail.shape[1] == n and eng.info("live_state_bytes") == state
            counts[name] = trace
            with pytest.raises(E.WesepHipError, match="ws_engine_live_push: the handle was flushed"):
                lv.push(np.ones(10, np.float32))
            with pytest.raises(E.WesepHipError, match="ws_engine_live_flush: the handle was flushed already"):
                lv.flush()
            lv.reset()
        assert counts["again"] == counts["random"]                      # reset, then the same pushes: the same counts
        # the same groups at different N: window 1 alone, and window 2 alone (both one window, neither at the wrap)
        lv.push(np.ones(S, np.float32))
        lv.push(np.ones(H, np.float32))
        a = eng.info("n_launches")
        lv.push(np.ones(H, np.float32))
        assert a == eng.info("n_launches") == launches([1])
        lv.close()
        # the state depends on (K, S, O, max_rows), not on the recording: 3 windows and 30
        for W in (3, 30):
            lv = eng.live(emb, E.ENROLL_EMBEDDING, S, O, max_rows)
            assert eng.info("live_state_bytes") == state
            lv.push(np.ones(S + (W - 1) * H, np.float32))
            assert eng.info("live_windows") == W and eng.info("live_state_bytes") == state
            lv.flush()
            lv.close()
    eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _open(eng, K, enroll, kind, elen, window, overlap, max_rows, lengths=None, out=True):
    h = ctypes.c_void_p()
    enroll = np.ascontiguousarray(enroll, np.float32)
    rc = E.lib().ws_engine_live_open(eng._h, K, enroll.ctypes.data, kind, elen, None if lengths is None else lengths.ctypes.data,
                                     window, overlap, max_rows, ctypes.byref(h) if out else None)
    return rc, h


@needs_no_gpu
def test_live_refusals(tmp_path):
    emb = np.zeros((2, 256), np.float32)
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    eng.separate(np.ones((1, 2048), np.float32), emb[:1], E.ENROLL_EMBEDDING)
    mark = eng.info("n_launches")                               # a refusal launches nothing: the counter stays
    bad = lambda *a, **k: _open(eng, *a, **k)[0] == -1 and eng.info("n_launches") == mark
    # every open-time refusal of ws_engine_separate_long, with its text
    assert bad(2, emb, E.ENROLL_EMBEDDING, 0, 500, 100, 3) and "T=500; T >= 512" in last()
    assert bad(2, emb, E.ENROLL_EMBEDDING, 0, 2048, 1025, 3) and "ws_engine_separate_long: overlap = 1025 outside [0, window / 2 = 1024]" in last()
    assert bad(2, emb, E.ENROLL_EMBEDDING, 0, 2048, -1, 3) and "overlap = -1 outside" in last()
    assert bad(2, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 0) and "ws_engine_separate_long: max_rows = 0" in last()
    assert bad(2, emb, E.ENROLL_SPEAKER, 0, 2048, 512, 3) and "kind 3 does not fit this model" in last()
    assert bad(2, emb, E.ENROLL_WAVE, 16000, 2048, 512, 3) and "kind 2 does not fit this model" in last()
    assert bad(2, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 3, lengths=np.array([1, 1], np.int32)) and "enroll_lengths given with fixed embeddings" in last()
    assert bad(0, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 3) and "ws_engine_live_open: bad arguments (K=0" in last()
    assert bad(2, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 3, out=False) and "out NULL" in last()
    assert E.lib().ws_engine_live_open(eng._h, 2, None, 0, 0, None, 2048, 512, 3, ctypes.byref(ctypes.c_void_p())) == -1 and "enroll NULL" in last()
    assert E.lib().ws_engine_live_open(None, 2, emb.ctypes.data, 0, 0, None, 2048, 512, 3, ctypes.byref(ctypes.c_void_p())) == -1 \
        and "ws_engine_live_open: null engine" in last()
    # push and flush
    rc, h = _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 3)
    assert rc == 0
    S, H = 2048, 1536
    x = np.ones(8000, np.float32)
    assert _push(None, x, 8000)[0] == -1 and "ws_engine_live_push: null handle" in last()
    assert _flush(None, 8000)[0] == -1 and "ws_engine_live_flush: null handle" in last()
    assert E.lib().ws_engine_live_reset(None) == -1 and "ws_engine_live_reset: null handle" in last()
    E.lib().ws_engine_live_close(None)
    m = ctypes.c_int(0)
    assert E.lib().ws_engine_live_push(h, None, 100, x.ctypes.data, 100, ctypes.byref(m)) == -1 and "chunk NULL" in last()
    assert E.lib().ws_engine_live_push(h, x.ctypes.data, 100, x.ctypes.data, 100, None) == -1 and "n_out NULL" in last()
    assert E.lib().ws_engine_live_push(h, x.ctypes.data, 0, x.ctypes.data, 100, ctypes.byref(m)) == -1 and "n=0 >= 1" in last()
    assert _flush(h, 4000)[0] == -1 and "ws_engine_live_flush: nothing was pushed" in last()
    assert _push(h, x[:S + H], 0) == (-1, -1) and "this push emits 1536 samples a row, est_cap is 0" in last()     # two windows: E = H
    assert E.lib().ws_engine_live_push(h, x.ctypes.data, S + H, None, 4000, ctypes.byref(m)) == -1 and "est is NULL" in last()
    assert eng.info("n_launches") == 0 and eng.info("live_windows") == 0             # nothing ran, nothing was taken
    # a flush below pBSRNN's minimum T: refused, the state intact -- a later push and flush succeed
    assert _push(h, x[:300], 0) == (0, 0)
    assert _flush(h, 4000)[0] == -1 and "T=300; T >= 512" in last() and eng.info("n_launches") == 0
    assert _push(h, x[:300], 0) == (0, 0)
    assert _flush(h, 599)[0] == -1 and "the flush emits 600 samples a row, est_cap is 599" in last()
    assert E.lib().ws_engine_live_flush(h, None, 4000, ctypes.byref(m)) == -1 and "est or n_out is NULL" in last()
    assert _flush(h, 600) == (0, 600) and eng.info("live_windows") == 1
    assert _push(h, x[:10], 100)[0] == -1 and "ws_engine_live_push: the handle was flushed" in last()
    assert _flush(h, 4000)[0] == -1 and "ws_engine_live_flush: the handle was flushed already" in last()
    assert E.lib().ws_engine_live_reset(h) == 0
    assert _push(h, x[:S + H + 1], E.live_push_cap(S + H + 1, H)) == (0, H)
    assert _flush(h, E.live_flush_cap(S, 512)) == (0, S + 1)
    E.lib().ws_engine_live_close(h)
    eng.close()
    # the refusals by architecture of ws_engine_separate_long
    eng = E.Engine(_container(tmp_path, "ConvTasNet"), dry_run=True)
    assert _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, 2005, 500, 8)[0] == -1 and "nearest valid windows are 2000 and 2010" in last()
    assert _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, 150, 30, 8)[0] == -1 and "Conv-TasNet needs T >= 160" in last()
    assert _open(eng, 2, emb, E.ENROLL_SPEAKER, 0, 2000, 500, 8)[0] == -1 and "a Conv-TasNet engine takes fixed embeddings" in last()
    assert _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, 2000, 500, 8, lengths=np.array([1, 1], np.int32))[0] == -1 \
        and "ws_engine_separate_long: per-row enrollment lengths are built for pBSRNN" in last()
    rc, h = _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, 2000, 500, 8)
    assert rc == 0 and _push(h, np.ones(100, np.float32), 0) == (0, 0)
    assert _flush(h, 4000)[0] == -1 and "Conv-TasNet needs T >= 160" in last()
    assert _push(h, np.ones(100, np.float32), 0) == (0, 0) and _flush(h, 4000) == (0, 200)
    E.lib().ws_engine_live_close(h)
    eng.close()
    eng = E.Engine(_container(tmp_path, "DPCCN"), dry_run=True)
    assert _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, 3900, 900, 8)[0] == -1 and "a DPCCN engine needs T >= 3968" in last()
    window = 128 * 9000                                     # 8 rows x 9001 frames x 257 x 160 >= 2^31; 1 row is far below
    assert _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, window, 0, 8)[0] == -1 and "R * frames * 257 * 160 below 2^31 (R=8" in last()
    eng.close()
    eng = E.Engine(_container(tmp_path, "TFGridNet"), dry_run=True)
    assert _open(eng, 2, emb, E.ENROLL_EMBEDDING, 0, 200, 50, 8)[0] == -1 and "ws_engine_separate: bad arguments (R=1, T=200" in last()
    eng.close()


# ---- separate_main --live_ms ---------------------------------------------------------------------------------------------
@needs_no_gpu
def test_separate_main_live_dry_run(tmp_path):
    from tests.test_ragged_host_cpu import _write_wav
    from tests.test_longform_host_cpu import _container as joint_container
    exe = os.path.join(ROOT, "runtime", "separate_main")
    assert os.path.exists(exe), "run python -m wesep_amd.build"
    model = joint_container(tmp_path, "pBSRNN")
    rng = np.random.default_rng(0)
    lens = (5000, 8000, 2048, 1000)
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1000 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 1000 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    base = [exe, "--wav_scp", str(scp), "--model", model, "--dry_run"]
    chunk = ["--chunk_seconds", "0.128", "--overlap_seconds", "0.032", "--chunk_rows", "3"]
    run = lambda extra: subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
    r = run(chunk + ["--live_ms", "100"])
    assert r.returncode == 0, r.stderr
    got = [tuple(map(int, re.search(r"\((\d+) pushes of (\d+) samples: (\d+) windows", l).groups()))
           for l in r.stdout.splitlines() if l.startswith("process:")]
    assert got == [(-(-n // 1600), 1600, len(E.long_windows(n, 2048, 512))) for n in lens]
    assert f"Total: process {sum(lens) * 1000 // 16000}ms audio" in r.stdout
    r2 = run(chunk + ["--live_ms", "100", "--jobs", "2"])
    assert r2.returncode == 0 and sorted(l.split()[1] for l in r2.stdout.splitlines() if l.startswith("process:")) == ["u0", "u1", "u2", "u3"]
    r = run(["--live_ms", "100"])
    assert r.returncode == 1 and "--live_ms needs --chunk_seconds S" in r.stderr
    for extra in (["--batch", "2"], ["--stream_ms", "10"], ["--stream_ms", "10", "--stream_pool", "2"], ["--stream_ms", "10", "--rate_pool", "2"]):
        r = run(chunk + ["--live_ms", "100"] + extra)
        assert r.returncode == 1 and "--live_ms conflicts with --batch N > 1, --stream_ms, --stream_pool and --rate_pool" in r.stderr, extra
    r = run(chunk + ["--live_ms", "0"])
    assert r.returncode == 1 and "--live_ms needs a positive packet length" in r.stderr
    r = run(["--chunk_seconds", "0.128", "--overlap_seconds", "0.1", "--live_ms", "100"])
    assert r.returncode == 1 and "overlap = 1600 outside" in r.stderr
    out = tmp_path / "out"
    out.mkdir()
    r = run(chunk + ["--live_ms", "100", "--resample", "--output_dir", str(out)])        # with --resample a dry run writes the files
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == sorted(f"u{i}-spk{k}.wav" for i in range(4) for k in (1, 2))
