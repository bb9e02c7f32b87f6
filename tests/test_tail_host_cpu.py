"""CPU-only: the tail pool (runtime/tail_pool.cc; ws_tail_emit_rows_fwd of longform.hip; DESIGN 7 "Tail pool").  The C ABI, the
kernel's refusals, the rule restated twice (tests/emu_tail.py: bookkeeping against position by position), the dry-run launch
plan of every architecture, the runtime's refusals and `separate_main --tail_ms`.  tests/test_zzz_tail_gpu.py holds the device
to the same rule."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import emu_tail as T
from tests.test_live_host_cpu import ENGINE_CASES, _container, needs_no_gpu
from wesep_amd import _lib as L
from wesep_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
last = lambda: E.lib().ws_engine_last_error().decode()
CALLS = ("ws_engine_tail_pool_open", "ws_engine_tail_pool_attach", "ws_engine_tail_pool_push", "ws_engine_tail_pool_tick",
         "ws_engine_tail_pool_flush", "ws_engine_tail_pool_detach", "ws_engine_tail_pool_close")


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_tail_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    name = "ws_tail_emit_rows_fwd"
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
    assert m, f"{name} is not declared in wesep_hip.h"
    res, args = L._SIGS[name]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
    assert getattr(L.lib(), name) is not None
    from wesep_amd import dev
    assert callable(dev.tail_emit_rows)
    # the descriptor, field for field
    assert L.TAIL_EMIT_ROW.itemsize == 56
    assert L.TAIL_EMIT_ROW.names == ("y_off", "hold_in_off", "hold_out_off", "out_off", "L", "p", "h", "m", "c_new", "scale")
    assert re.search(r"typedef struct ws_tail_emit_row \{\s*long long y_off, hold_in_off, hold_out_off, out_off;\s*int L, p, h, m, c_new;\s*"
                     r"float scale;\s*\} ws_tail_emit_row;", header)
    eheader = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    for name in CALLS[:-1]:
        assert re.search(r"^int\s+" + name + r"\s*\(", eheader, flags=re.M), name
    assert re.search(r"^void\s+ws_engine_tail_pool_close\s*\(", eheader, flags=re.M)
    for name in CALLS:
        assert name in E.SYMBOLS and getattr(E.lib(), name) is not None
    m = re.search(r"^#define WS_TAIL_TICK_LAUNCHES (\d+)\s", eheader, flags=re.M)
    assert m and int(m.group(1)) == E.TAIL_TICK_LAUNCHES == 2
    assert re.search(r"^#define WS_TAIL_CAP\(S\) \(S\)", eheader, flags=re.M)
    assert E.tail_launches([19, 19]) == 38 + 2 + 1
    assert callable(E.Engine.tail_pool) and callable(E.Engine.tail)
    assert all(callable(getattr(E.TailPool, f)) for f in ("attach", "push", "tick", "flush", "detach", "close"))
    assert L.lib().ws_abi_version() == 20                     # new symbols only: neither ABI number moves
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


# ---- the kernel's refusals -----------------------------------------------------------------------------------------------
def _emit_call(rows, C=16, n_y=2000, n_hold=400, n_out=1000, A=None, ramp=True, y=True, hold=True, out=True, d_rows=True):
    from wesep_amd import dev
    tab = dev.tail_emit_rows_table(rows) if rows else np.zeros(1, L.TAIL_EMIT_ROW)
    r, a, b, c = (ctypes.c_float * 64)(), (ctypes.c_float * 2000)(), (ctypes.c_float * 400)(), (ctypes.c_float * 1000)()
    vp = lambda buf, on: ctypes.cast(buf, ctypes.c_void_p) if on else None
    t = ctypes.c_void_p(tab.ctypes.data)
    rc = L.lib().ws_tail_emit_rows_fwd(t, t if d_rows else None, len(rows) if A is None else A, C, vp(r, ramp), vp(a, y), n_y, vp(b, hold), n_hold,
                                       vp(c, out), n_out, None)
    return rc, L.lib().ws_last_error().decode()


def test_tail_emit_rows_refuses_bad_tables_before_any_launch():
    # C 16.  Row 0: a window of 200 samples, the 100 from local index 84 come out (16 of them cross-faded), 16 are held back
    good = dict(y_off=3, hold_in_off=0, hold_out_off=16, out_off=1, L=200, p=84, h=16, m=100, c_new=16, scale=1.0)
    two = dict(good, y_off=300, hold_in_off=32, hold_out_off=48, out_off=200)
    refused = lambda r, text: r[0] == -1 and r[1].startswith("ws_tail_emit_rows_fwd: ") and text in r[1]
    assert refused(_emit_call([good], A=0), "A=0 is outside [1, 65535]")
    assert refused(_emit_call([good], A=65536), "A=65536 is outside [1, 65535]")
    for off in ("y", "hold", "out", "d_rows"):
        assert refused(_emit_call([good], **{off: False}), "rows, d_rows, y, hold or out is NULL"), off
    assert refused(_emit_call([good], ramp=False), "ramp is NULL with fade C=16")
    assert refused(_emit_call([good], C=-1), "fade C=-1 is negative")
    assert refused(_emit_call([good, dict(two, h=8)]), "row 1: h=8 held samples, the fade takes 0 or C=16")
    assert refused(_emit_call([good, dict(two, h=16, m=10, p=174)]), "row 1: h=16 held samples do not fit the m=10 emitted ones")
    assert refused(_emit_call([good, dict(two, c_new=8, p=92)]), "row 1: c_new=8 samples for the new hold, 0 or C=16")
    assert refused(_emit_call([good, dict(two, p=-1, L=115)]), "row 1: p=-1 is negative")
    assert refused(_emit_call([good, dict(two, L=201)]), "row 1: p + m + c_new = 84 + 100 + 16 is not the window's L=201")
    assert refused(_emit_call([good, dict(two, h=0, m=0, c_new=0, p=200)]), "row 1: nothing to do (m=0, c_new=0)")
    assert refused(_emit_call([good, dict(two, m=-1, h=0, p=185)]), "row 1: h=0 held samples do not fit the m=-1 emitted ones")
    assert refused(_emit_call([good, dict(two, y_off=1801)]), "row 1: y [1801, 1801 + 200) leaves the arena of 2000 floats")   # one float past
    assert refused(_emit_call([good, dict(two, y_off=-1)]), "row 1: y [-1,")
    assert refused(_emit_call([good, dict(two, hold_in_off=385)]), "row 1: hold_in [385, 385 + 16) leaves the arena of 400 floats")
    assert refused(_emit_call([good, dict(two, hold_out_off=385)]), "row 1: hold_out [385, 385 + 16) leaves the arena of 400 floats")
    assert refused(_emit_call([good, dict(two, out_off=901)]), "row 1: out [901, 901 + 100) leaves the arena of 1000 floats")
    assert refused(_emit_call([good, dict(two, out_off=100)]), "row 1: its out range overlaps the out range of row 0")
    assert refused(_emit_call([good, dict(two, hold_out_off=31)]), "row 1: its hold_out range overlaps the hold_out range of row 0")
    assert refused(_emit_call([good, dict(two, hold_in_off=17)]), "row 1: its hold_in range overlaps the hold_out range of row 0")
    assert refused(_emit_call([good, dict(two, hold_out_off=15)]), "row 1: its hold_out range overlaps the hold_in range of row 0")
    # (every call here is refused before a launch: the arenas are host memory.  Good tables, C == 0 without a ramp among them, run
    # in tests/test_zzz_tail_gpu.py)
    plain = dict(y_off=0, out_off=0, L=100, p=0, h=0, m=100, c_new=0)
    assert refused(_emit_call([dict(plain, h=16)], C=0, ramp=False), "row 0: h=16 held samples, the fade takes 0 or C=0")


# ---- the rule, restated twice ----------------------------------------------------------------------------------------------
K_, S_ = 2, 300


def _separator(seed):
    """row-independent, and a function of the LOCAL index too: two windows disagree about the same position"""
    mix = np.random.default_rng(seed).standard_normal((K_, 3))
    return lambda x: np.stack([m[0] * x + m[1] * np.cos(0.1 * np.arange(len(x))) + m[2] * x[::-1] for m in mix])


_factor = lambda x: 2.0 ** (int(np.abs(x).sum() * 7) % 5 - 2)      # powers of two: x * (1 / f) * f is x exactly


def _random_ticks(rng, n, C, warm, lo=1):
    """values of N at which a slot is ticked: steps that never leave more than a window waiting"""
    ticks, N, E, F = [], 0, 0, None
    while N < n:
        N += int(rng.integers(lo, max(lo, min(S_ - (N - E), n - N)) + 1))
        N = min(N, n)
        ticks.append(N)
        if N >= warm and (F is None or N - F >= max(C, 1)):
            F, E = N, N - C
    return ticks


def _run(x, C, warm, ticks, split, sep, fac):
    """the class fed packets of at most `split` samples, ticked at `ticks`, flushed at the end -> [K][n], and the slot"""
    tl, parts, N = T.Tail(K_, S_, C, warm, sep, fac), [], 0
    for t in ticks:
        while N < t:
            c = min(split, t - N)
            tl.push(x[N:N + c])
            N += c
        got = tl.tick()
        if got is not None:
            parts.append(got)
    parts.append(tl.flush())
    return np.concatenate(parts, axis=1), tl


@pytest.mark.parametrize("C", [0, 1, 128])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "factors"])
def test_tail_rule_bookkeeping_equals_position_by_position(C, scaled):
    rng = np.random.default_rng(40 + C)
    fac = _factor if scaled else None
    seen = set()
    for trial in range(12):
        n = int(rng.integers(1, 1400))
        warm = int(rng.integers(max(C, 1), S_ + 1))
        x = rng.standard_normal(n)
        ticks = _random_ticks(rng, n, C, warm)
        if trial % 3 == 0 and T.firings(ticks, n, S_, C, warm):
            n = T.firings(ticks, n, S_, C, warm)[-1]          # the recording ends at a firing: the flush finds N == F, the hold alone
            x, ticks = x[:n], [t for t in ticks if t <= n]
        sep = _separator(trial)
        got, tl = _run(x, C, warm, ticks, 10 ** 9, sep, fac)
        want = T.brute(x, K_, S_, C, warm, ticks, sep, fac)
        assert got.shape == want.shape == (K_, n)
        assert np.array_equal(got, want), (C, trial, np.abs(got - want).max())
        assert [e for _, e in tl.windows[:len(T.firings(ticks, n, S_, C, warm))]] == T.firings(ticks, n, S_, C, warm)
        seen |= {"blend"} if tl.blends else set()
        seen |= {"short"} if any(b - a < S_ for a, b in tl.windows[:-1]) else set()
        seen |= {"hold only"} if tl.fired and tl.windows[-1][1] == n and len(tl.windows) == len(T.firings(ticks, n, S_, C, warm)) else set()
    assert seen >= ({"blend", "short", "hold only"} if C else {"short", "hold only"}), seen


def test_tail_rule_does_not_depend_on_the_packet_split():
    rng = np.random.default_rng(5)
    n, C, warm = 1100, 64, 200
    x = rng.standard_normal(n)
    ticks = _random_ticks(rng, n, C, warm, lo=40)
    sep = _separator(3)
    runs = [_run(x, C, warm, ticks, split, sep, None)[0] for split in (10 ** 9, 1, 37)]
    assert runs[0].shape == (K_, n) and np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])
    tl = T.Tail(K_, S_, C, warm, sep)
    tl.push(x[:S_])
    with pytest.raises(ValueError, match="tick first"):
        tl.push(x[:1])
    assert tl.N == S_                                          # nothing of the refused push was taken


def test_tick_forwards_restated():
    assert T.tick_forwards([300, 300, 300], 2, 300, 8) == [(6, 300)]
    assert T.tick_forwards([300, 300, 300], 2, 300, 4) == [(4, 300), (2, 300)]
    assert T.tick_forwards([300, 250, 300], 2, 300, 8) == [(4, 300), (2, 250)]
    assert T.tick_forwards([250, 260], 3, 300, 2) == [(2, 250), (1, 250), (2, 260), (1, 260)]
    assert T.tick_forwards([], 2, 300, 8) == []


# ---- dry-run engines: counts ---------------------------------------------------------------------------------------------
@needs_no_gpu
@pytest.mark.parametrize("arch", sorted(ENGINE_CASES))
def test_dry_run_tail_pool_counts(tmp_path, arch):
    _, _, _, S, _ = ENGINE_CASES[arch]
    K, C, warm = 2, 128, S - 100
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    emb = np.zeros((K, 256), np.float32)
    plan = {}

    def count(fw):                                               # a forward's rectangular count, from ws_engine_separate itself
        if fw not in plan:
            eng.separate(np.ones(fw, np.float32), np.zeros((fw[0], 256), np.float32), E.ENROLL_EMBEDDING)
            plan[fw] = eng.info("n_launches")
        return plan[fw]

    ones = lambda m: np.ones(m, np.float32)
    for max_rows in (8, 4, 1):
        pool = eng.tail_pool(3, K, S, C, warm, max_rows)
        state = eng.info("tail_pool_state_bytes")
        assert state > 3 * K * S * 4 * 3 + 3 * 2 * K * C * 4
        slots = [pool.attach(emb, E.ENROLL_EMBEDDING) for _ in range(3)]
        assert slots == [0, 1, 2] and eng.info("n_launches") == 0
        model = [T.Tail(K, S, C, warm, lambda x: np.zeros((K, len(x)))) for _ in range(3)]

        def push(chunks):
            pool.push({s: ones(m) for s, m in chunks.items()})
            for s, m in chunks.items():
                model[s].push(np.ones(m))
            assert eng.info("tail_pool_state_bytes") == state

        def tick(named):
            got = pool.tick(named)
            lengths = [min(model[s].N, S) for s in sorted(named) if model[s].fires()]
            ref = {s: model[s].tick() for s in named}
            assert {s: v.shape for s, v in got.items()} == {s: v.shape for s, v in ref.items() if v is not None and v.shape[1] > 0}
            assert not any(v.any() for v in got.values())          # a dry run computes nothing
            fw = T.tick_forwards(lengths, K, S, max_rows)
            assert eng.info("tail_pool_forwards") == len(fw) and eng.info("tail_pool_rows") == K * len(lengths)
            assert eng.info("n_launches") == (E.tail_launches([count(f) for f in fw]) if fw else 0), (arch, max_rows, named, fw)
            assert eng.info("tail_pool_state_bytes") == state
            return fw

        push({0: S, 1: S, 2: warm - 1})
        assert tick([2]) == []                                     # nothing fires: no launch
        assert tick([0]) == [(min(K, max_rows), S)] * -(-K // max_rows)          # one firing slot
        assert tick([0]) == []                                     # nothing new since
        push({0: 300, 2: 50})
        fw = tick([0, 1, 2])                                       # two full slots and one in warm-up: its rows keep to themselves
        assert len(fw) == -(-2 * K // max_rows) + -(-K // max_rows) and fw[-1][1] == warm + 49
        push({0: 300, 1: 300, 2: 150})
        fw = tick([2, 0, 1])                                       # three full slots share their forwards, whatever order they are named in
        assert len(fw) == -(-3 * K // max_rows) and all(L == S for _, L in fw)
        assert tick([0, 1, 2]) == []
        # the flushes: N == F is the copy of the hold and the copy to the host; new audio runs one last window
        tail = pool.flush(0)
        assert tail.shape == model[0].flush().shape == (K, C) and eng.info("n_launches") == 2 and eng.info("tail_pool_forwards") == 0
        push({1: 100})
        tail = pool.flush(1)
        assert tail.shape == model[1].flush().shape == (K, C + 100)
        fw = T.tick_forwards([S], K, S, max_rows)
        assert eng.info("n_launches") == E.tail_launches([count(f) for f in fw]) and eng.info("tail_pool_forwards") == len(fw)
        with pytest.raises(E.WesepHipError, match="ws_engine_tail_pool_push: slot 1 .entry 0. was flushed"):
            pool.push({1: ones(10)})
        assert pool.tick() == {}                                   # None names the attached, unflushed slots: slot 2, which has nothing new
        assert eng.info("n_launches") == 0
        for s in slots:
            pool.detach(s)
            assert eng.info("tail_pool_state_bytes") == state
        # a recording shorter than warm: the flush runs it as one short window
        s = pool.attach(emb, E.ENROLL_EMBEDDING)
        assert s == 0                                              # the lowest free slot again
        lo = 3968 if arch == "DPCCN" else 600
        pool.push({s: ones(lo)})
        assert pool.tick([s]) == {} and pool.flush(s).shape == (K, lo)
        fw = T.tick_forwards([lo], K, S, max_rows)
        assert eng.info("n_launches") == E.tail_launches([count(f) for f in fw]) and eng.info("tail_pool_rows") == K
        pool.close()
    eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _popen(eng, slots, K, window, fade, warm, max_rows, out=True):
    h = ctypes.c_void_p()
    return E.lib().ws_engine_tail_pool_open(eng._h, slots, K, window, fade, warm, max_rows, ctypes.byref(h) if out else None), h


def _pattach(h, enroll, kind, elen, lengths=None, slot=True):
    s = ctypes.c_int(-1)
    enroll = np.ascontiguousarray(enroll, np.float32)
    rc = E.lib().ws_engine_tail_pool_attach(h, enroll.ctypes.data, kind, elen, None if lengths is None else lengths.ctypes.data,
                                            ctypes.byref(s) if slot else None)
    return rc, s.value


def _ppush(h, entries):
    """entries: (slot, samples) -> rc"""
    A = len(entries)
    data = [np.ones(max(m, 1), np.float32) for _, m in entries]
    ids, n = np.array([s for s, _ in entries], np.int32), np.array([m for _, m in entries], np.int32)
    cp = (ctypes.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
    return E.lib().ws_engine_tail_pool_push(h, A, ids.ctypes.data, ctypes.cast(cp, ctypes.c_void_p), n.ctypes.data)


def _ptick(h, entries, K=2):
    """entries: (slot, est_cap) -> rc, n_out"""
    A = len(entries)
    bufs = [np.zeros((K, max(c, 1)), np.float32) for _, c in entries]
    ids, caps, m = np.array([s for s, _ in entries], np.int32), np.array([c for _, c in entries], np.int32), np.full(max(A, 1), -1, np.int32)
    ep = (ctypes.c_void_p * max(A, 1))(*[b.ctypes.data for b in bufs])
    rc = E.lib().ws_engine_tail_pool_tick(h, A, ids.ctypes.data, ctypes.cast(ep, ctypes.c_void_p), caps.ctypes.data, m.ctypes.data)
    return rc, m.tolist()


def _pflush(h, slot, cap, K=2):
    est, m = np.zeros((K, max(cap, 1)), np.float32), ctypes.c_int(-1)
    return E.lib().ws_engine_tail_pool_flush(h, slot, est.ctypes.data, cap, ctypes.byref(m)), m.value


@needs_no_gpu
def test_tail_pool_refusals(tmp_path):
    emb = np.zeros((2, 256), np.float32)
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    eng.separate(np.ones((1, 2048), np.float32), emb[:1], E.ENROLL_EMBEDDING)
    mark = eng.info("n_launches")                               # a refusal launches nothing: the counter stays
    bad = lambda *a, **k: _popen(eng, *a, **k)[0] == -1 and eng.info("n_launches") == mark
    S, C, W = 2048, 128, 1000
    # open: the window checks of ws_engine_separate_long with their texts, and the pool's own
    assert bad(3, 2, 500, 100, 500, 3) and "T=500; T >= 512" in last()
    assert bad(3, 2, S, C, W, 0) and "ws_engine_separate_long: max_rows = 0" in last()
    assert bad(3, 2, S, 1025, S, 3) and "ws_engine_tail_pool_open: fade = 1025 outside [0, window / 2 = 1024]" in last()
    assert bad(3, 2, S, -1, S, 3) and "fade = -1 outside" in last()
    assert bad(3, 2, S, C, S + 1, 3) and "ws_engine_tail_pool_open: warm = 2049 outside [max(fade, 1) = 128, window = 2048]" in last()
    assert bad(3, 2, S, C, 127, 3) and "warm = 127 outside [max(fade, 1) = 128" in last()
    assert bad(3, 2, S, 0, 0, 3) and "warm = 0 outside [max(fade, 1) = 1" in last()
    assert bad(3, 2, S, C, 511, 3) and "T=511; T >= 512" in last()                  # the architecture's own lower bound on T
    assert bad(0, 2, S, C, W, 3) and "ws_engine_tail_pool_open: slots=0 is outside [1, 65535]" in last()
    assert bad(65536, 2, S, C, W, 3) and "slots=65536 is outside [1, 65535]" in last()
    assert bad(40000, 2, S, C, W, 8) and "40000 slots x 2 speakers = 80000 rows in a tick" in last()
    assert bad(3, 0, S, C, W, 3) and "ws_engine_tail_pool_open: bad arguments (K=0" in last()
    assert bad(3, 2, S, C, W, 3, out=False) and "out NULL" in last()
    assert E.lib().ws_engine_tail_pool_open(None, 3, 2, S, C, W, 3, ctypes.byref(ctypes.c_void_p())) == -1 and "ws_engine_tail_pool_open: null engine" in last()
    rc, h = _popen(eng, 2, 2, S, C, W, 3)
    assert rc == 0
    # attach: the enrollment checks of ws_engine_separate_long, NULL pointers, a full pool
    assert _pattach(h, emb, E.ENROLL_SPEAKER, 0)[0] == -1 and "kind 3 does not fit this model" in last()
    assert _pattach(h, emb, E.ENROLL_WAVE, 16000)[0] == -1 and "kind 2 does not fit this model" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, slot=False)[0] == -1 and "slot NULL" in last()
    assert E.lib().ws_engine_tail_pool_attach(h, None, 0, 0, None, ctypes.byref(ctypes.c_int())) == -1 and "enroll NULL" in last()
    assert _pattach(None, emb, E.ENROLL_EMBEDDING, 0)[0] == -1 and "ws_engine_tail_pool_attach: null pool" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 0) and _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 1)
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0)[0] == -1 and "ws_engine_tail_pool_attach: the pool is full: all 2 slots are attached" in last()
    mark = eng.info("n_launches")                               # (fixed embeddings: the attach launched nothing)
    assert mark == 0
    # push
    assert _ppush(None, [(0, 10)]) == -1 and "ws_engine_tail_pool_push: null pool" in last()
    assert _ppush(h, []) == -1 and "bad arguments (n_active=0 >= 1" in last()
    assert E.lib().ws_engine_tail_pool_push(h, 1, None, None, None) == -1 and "a NULL array" in last()
    assert _ppush(h, [(2, 10)]) == -1 and "slot 2 (entry 0) is not attached (the pool has 2 slots)" in last()
    assert _ppush(h, [(0, 10), (0, 10)]) == -1 and "slot 0 is named twice (entry 1)" in last()
    assert _ppush(h, [(0, 10), (1, 0)]) == -1 and "entry 1 (slot 1): n=0 >= 1" in last()
    # the overflow is found before ANY entry is appended: entry 0's packet is not taken either
    assert _ppush(h, [(0, S), (1, S + 1)]) == -1 and "entry 1 (slot 1): 2049 more samples make 2049 that have not come out, a window holds 2048: tick first" in last()
    assert _ppush(h, [(0, S)]) == 0 and _ppush(h, [(0, 1)]) == -1 and "tick first" in last()      # ... so slot 0 takes a whole window now, and no more
    assert eng.info("n_launches") == mark                         # no push launches
    # tick
    assert _ptick(None, [(0, S)])[0] == -1 and "ws_engine_tail_pool_tick: null pool" in last()
    assert _ptick(h, [])[0] == -1 and "bad arguments (n_active=0 >= 1" in last()
    assert E.lib().ws_engine_tail_pool_tick(h, 1, None, None, None, None) == -1 and "a NULL array" in last()
    assert _ptick(h, [(2, S)])[0] == -1 and "slot 2 (entry 0) is not attached" in last()
    assert _ptick(h, [(0, S), (0, S)])[0] == -1 and "slot 0 is named twice (entry 1)" in last()
    assert _ppush(h, [(1, W)]) == 0
    # est_cap of EVERY entry is checked before anything runs: entry 1 is short, so slot 0 does not fire either
    assert _ptick(h, [(0, S), (1, W - C - 1)])[0] == -1 and "entry 1 (slot 1) emits 872 samples a row, est_cap is 871" in last() \
        and "WS_TAIL_CAP(S) = 2048 always suffices" in last() and eng.info("n_launches") == mark
    assert _ptick(h, [(0, S - C), (1, W - C)]) == (0, [S - C, W - C]) and eng.info("tail_pool_rows") == 4
    assert _ptick(h, [(0, 0), (1, 0)]) == (0, [0, 0]) and eng.info("n_launches") == 0       # nothing new: no slot fires, no capacity is needed
    # flush: below pBSRNN's minimum T the slot stays as it was
    assert E.lib().ws_engine_tail_pool_detach(h, 1) == 0 and _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 1)
    assert _pflush(None, 0, S)[0] == -1 and "ws_engine_tail_pool_flush: null pool" in last()
    assert _pflush(h, 5, S)[0] == -1 and "slot 5 is not attached" in last()
    assert _pflush(h, 1, S)[0] == -1 and "slot 1: nothing was pushed" in last()
    assert _ppush(h, [(1, 300)]) == 0
    assert _pflush(h, 1, S)[0] == -1 and "T=300; T >= 512" in last()
    assert _ppush(h, [(1, 300)]) == 0                             # ... and goes on
    assert _pflush(h, 1, 599)[0] == -1 and "slot 1: the flush emits 600 samples a row, est_cap is 599" in last()
    assert E.lib().ws_engine_tail_pool_flush(h, 1, None, S, ctypes.byref(ctypes.c_int())) == -1 and "est or n_out is NULL" in last()
    assert _pflush(h, 1, 600) == (0, 600)
    assert _ppush(h, [(0, 10), (1, 10)]) == -1 and "slot 1 (entry 1) was flushed (detach it" in last()
    assert _ptick(h, [(1, S)])[0] == -1 and "slot 1 (entry 0) was flushed" in last()
    assert _pflush(h, 1, S)[0] == -1 and "slot 1 was flushed" in last()
    assert E.lib().ws_engine_tail_pool_detach(h, 1) == 0
    assert E.lib().ws_engine_tail_pool_detach(h, 1) == -1 and "ws_engine_tail_pool_detach: slot 1 is not attached" in last()
    assert E.lib().ws_engine_tail_pool_detach(None, 1) == -1 and "null pool" in last()
    assert _ppush(h, [(1, 10)]) == -1 and "slot 1 (entry 0) is not attached" in last()
    assert _pflush(h, 0, S) == (0, C) and eng.info("n_launches") == 2      # N == F: the hold
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 1)              # slot 0 is done, not free
    E.lib().ws_engine_tail_pool_close(h)
    E.lib().ws_engine_tail_pool_close(None)
    eng.close()
    # the refusals by architecture
    eng = E.Engine(_container(tmp_path, "ConvTasNet"), dry_run=True)
    assert _popen(eng, 2, 2, 2005, 100, 2005, 8)[0] == -1 and "nearest valid windows are 2000 and 2010" in last()
    assert _popen(eng, 2, 2, 2000, 100, 159, 8)[0] == -1 and "Conv-TasNet needs T >= 160" in last()
    rc, h = _popen(eng, 2, 2, 2000, 100, 160, 8)
    assert rc == 0 and _pattach(h, emb, E.ENROLL_SPEAKER, 0)[0] == -1 and "a Conv-TasNet engine takes fixed embeddings" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 0) and _ppush(h, [(0, 100)]) == 0
    assert _pflush(h, 0, 2000)[0] == -1 and "Conv-TasNet needs T >= 160" in last()
    assert _ppush(h, [(0, 100)]) == 0 and _pflush(h, 0, 2000) == (0, 200)
    E.lib().ws_engine_tail_pool_close(h)
    eng.close()
    eng = E.Engine(_container(tmp_path, "DPCCN"), dry_run=True)
    assert _popen(eng, 2, 2, 3900, 100, 3900, 8)[0] == -1 and "a DPCCN engine needs T >= 3968" in last()
    assert _popen(eng, 2, 2, 4096, 100, 3967, 8)[0] == -1 and "a DPCCN engine needs T >= 3968" in last()
    eng.close()


# ---- separate_main --tail_ms -----------------------------------------------------------------------------------------------
@needs_no_gpu
def test_separate_main_tail_dry_run(tmp_path):
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
    chunk = ["--chunk_seconds", "0.128", "--chunk_rows", "3"]
    run = lambda extra: subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
    pat = r"\(tail pool of (\d+) lines: (\d+) ticks, packets of (\d+) samples, fade (\d+),"
    for pool in ([], ["--tail_pool", "2"]):
        r = run(chunk + ["--tail_ms", "40", "--tail_warm_seconds", "0.05"] + pool)
        assert r.returncode == 0, r.stderr
        got = {l.split()[1]: tuple(map(int, re.search(pat, l).groups())) for l in r.stdout.splitlines() if l.startswith("process:")}
        # 640-sample packets, none cut: a line's ticks are its packets; the default fade is 10 ms
        assert got == {f"u{i}": (2 if pool else 1, -(-n // 640), 640, 160) for i, n in enumerate(lens)}, r.stdout
        m = re.search(r"^tail pool: (\d+) ticks, (\d+) rows, (\d+) forwards, (\d+) launches$", r.stdout, flags=re.M)
        assert m and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout
        # one lane: the lines' ticks add up; two lanes: u0 (8 ticks) and u1 (13) start together, u2 takes u0's lane (4), u3 follows (2)
        assert int(m.group(1)) == (sum(-(-n // 640) for n in lens) if not pool else 14), r.stdout
        assert f"Total: process {sum(lens) * 1000 // 16000}ms audio" in r.stdout
    # warm defaults to the window: a packet is cut where the window fills (2048 = 3 * 640 + 128), so u1 takes one more round
    r = run(chunk + ["--tail_ms", "40", "--tail_fade_ms", "2"])
    assert r.returncode == 0, r.stderr
    got = {l.split()[1]: tuple(map(int, re.search(pat, l).groups())) for l in r.stdout.splitlines() if l.startswith("process:")}
    assert got["u2"] == (1, 4, 640, 32) and got["u3"] == (1, 2, 640, 32) and got["u1"][1] >= 13, r.stdout
    r2 = run(chunk + ["--tail_ms", "40", "--tail_pool", "2", "--jobs", "2"])
    assert r2.returncode == 0 and sorted(l.split()[1] for l in r2.stdout.splitlines() if l.startswith("process:")) == ["u0", "u1", "u2", "u3"]
    # the flags' conflicts
    r = run(chunk + ["--tail_pool", "2"])
    assert r.returncode == 1 and "need --tail_ms M" in r.stderr
    r = run(["--tail_ms", "40"])
    assert r.returncode == 1 and "--tail_ms needs --chunk_seconds S" in r.stderr
    for extra in (["--batch", "2"], ["--stream_ms", "10"], ["--live_ms", "100"], ["--live_ms", "100", "--live_pool", "2"],
                  ["--stream_ms", "10", "--stream_pool", "2"], ["--stream_ms", "10", "--rate_pool", "2"]):
        r = run(chunk + ["--tail_ms", "40"] + extra)
        assert r.returncode == 1 and "--tail_ms conflicts with --batch N > 1, --stream_ms, --live_ms, --live_pool, --stream_pool and --rate_pool" in r.stderr, extra
    r = run(chunk + ["--tail_ms", "40", "--tail_pool", "0"])
    assert r.returncode == 1 and "--tail_pool needs a positive number of lines" in r.stderr
    r = run(chunk + ["--tail_ms", "40", "--tail_fade_ms", "100"])
    assert r.returncode == 1 and "fade = 1600 outside [0, window / 2 = 1024]" in r.stderr
    out = tmp_path / "out"
    out.mkdir()
    r = run(chunk + ["--tail_ms", "40", "--tail_pool", "3", "--resample", "--output_dir", str(out)])   # with --resample a dry run writes the files
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == sorted(f"u{i}-spk{k}.wav" for i in range(4) for k in (1, 2))
