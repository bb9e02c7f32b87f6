"""CPU-only: the live pool (runtime/live_pool.cc; ws_window_slots_fwd and ws_xfade_stream_rows_fwd of longform.hip; DESIGN 7
"Live pool").  The C ABI, the two kernels' refusals, the round rule restated (tests/emu_live_pool.py) against the solo rule
(tests/emu_live.py), the dry-run launch plan of every architecture, the runtime's refusals and `separate_main --live_pool`.
tests/test_zzz_live_pool_gpu.py holds the device to the same rule."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import emu_live as M
from tests import emu_live_pool as P
from tests.test_live_host_cpu import ENGINE_CASES, _container, needs_no_gpu
from wesep_amd import _lib as L
from wesep_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
last = lambda: E.lib().ws_engine_last_error().decode()
KERNELS = ("ws_window_slots_fwd", "ws_xfade_stream_rows_fwd")
CALLS = ("ws_engine_live_pool_open", "ws_engine_live_pool_attach", "ws_engine_live_pool_push", "ws_engine_live_pool_flush",
         "ws_engine_live_pool_detach", "ws_engine_live_pool_close")


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_live_pool_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    for name in KERNELS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        assert getattr(L.lib(), name) is not None
    from wesep_amd import dev
    assert callable(dev.window_slots_fwd) and callable(dev.xfade_stream_rows_fwd)
    # the descriptors, field for field: {long long src_off, dst_off; int len; float scale} and eight long long + int final
    assert L.WINDOW_SLOT_ROW.itemsize == 24 and L.WINDOW_SLOT_ROW.names == ("src_off", "dst_off", "len", "scale")
    assert L.XFADE_STREAM_ROW.itemsize == 72
    assert L.XFADE_STREAM_ROW.names[:9] == ("ring_off", "scale_off", "out_off", "i0", "count", "windows_run", "W", "n", "final")
    for struct, fields in (("ws_window_slot_row", r"long long src_off, dst_off;\s*int len;\s*float scale;"),
                           ("ws_xfade_stream_row", r"long long ring_off, scale_off, out_off, i0, count, windows_run, W, n;\s*int final;")):
        assert re.search(r"typedef struct " + struct + r" \{\s*" + fields + r"\s*\} " + struct + ";", header), struct
    eheader = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    for name in CALLS[:-1]:
        assert re.search(r"^int\s+" + name + r"\s*\(", eheader, flags=re.M), name
    assert re.search(r"^void\s+ws_engine_live_pool_close\s*\(", eheader, flags=re.M)
    for name in CALLS:
        assert name in E.SYMBOLS and getattr(E.lib(), name) is not None
    m = re.search(r"^#define WS_LIVE_POOL_ROUND_LAUNCHES (\d+)$", eheader, flags=re.M)
    assert m and int(m.group(1)) == E.LIVE_POOL_ROUND_LAUNCHES == P.ROUND_LAUNCHES
    assert E.live_pool_launches([[19], [19, 19]]) == 19 + 3 + 38 + 3 + 1
    assert callable(E.Engine.live_pool) and all(callable(getattr(E.LivePool, f)) for f in ("attach", "push", "flush", "detach", "close"))
    assert L.lib().ws_abi_version() == 20                     # new symbols only: neither ABI number moves
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


# ---- the kernels' refusals -----------------------------------------------------------------------------------------------
def _slots_call(rows, n_src=1000, n_dst=1000, A=None, src=True, dst=True, d_rows=True):
    from wesep_amd import dev
    tab = dev.window_slots_table(rows) if rows else np.zeros(1, L.WINDOW_SLOT_ROW)
    a, b = (ctypes.c_float * 1000)(), (ctypes.c_float * 1000)()
    t = ctypes.c_void_p(tab.ctypes.data)
    rc = L.lib().ws_window_slots_fwd(t, t if d_rows else None, len(rows) if A is None else A, ctypes.cast(a, ctypes.c_void_p) if src else None,
                                     n_src, ctypes.cast(b, ctypes.c_void_p) if dst else None, n_dst, None)
    return rc, L.lib().ws_last_error().decode()


def _fade_call(rows, S=48, O=16, cap=4, n_ring=2000, n_scale=16, n_out=1000, A=None, ring=True, out=True, scale=True):
    from wesep_amd import dev
    tab = dev.xfade_stream_rows_table(rows) if rows else np.zeros(1, L.XFADE_STREAM_ROW)
    a, b, c = (ctypes.c_float * 2000)(), (ctypes.c_float * 16)(), (ctypes.c_float * 1000)()
    t = ctypes.c_void_p(tab.ctypes.data)
    rc = L.lib().ws_xfade_stream_rows_fwd(t, t, len(rows) if A is None else A, S, O, cap, ctypes.cast(a, ctypes.c_void_p) if ring else None, n_ring,
                                          ctypes.cast(b, ctypes.c_void_p) if scale else None, n_scale,
                                          ctypes.cast(c, ctypes.c_void_p) if out else None, n_out, None)
    return rc, L.lib().ws_last_error().decode()


def test_window_slots_refuses_bad_tables_before_any_launch():
    good = dict(src_off=3, dst_off=0, len=48, scale=1.0)
    refused = lambda r, text: r[0] == -1 and r[1].startswith("ws_window_slots_fwd: ") and text in r[1]
    assert refused(_slots_call([good], A=0), "A=0 is outside [1, 65535]")
    assert refused(_slots_call([good], A=65536), "A=65536 is outside [1, 65535]")
    assert refused(_slots_call([good], src=False), "rows, d_rows, src or dst is NULL")
    assert refused(_slots_call([good], dst=False), "rows, d_rows, src or dst is NULL")
    assert refused(_slots_call([good], d_rows=False), "rows, d_rows, src or dst is NULL")
    assert refused(_slots_call([good, dict(good, len=0, dst_off=100)]), "row 1: bad args (len=0")
    assert refused(_slots_call([good, dict(good, src_off=953, dst_off=100)]), "row 1: src [953, 953 + 48) leaves the arena of 1000 floats")
    assert refused(_slots_call([good, dict(good, src_off=-1, dst_off=100)]), "row 1: src [-1,")
    assert refused(_slots_call([good, dict(good, dst_off=953)]), "row 1: dst [953, 953 + 48) leaves the arena of 1000 floats")   # one float past
    assert refused(_slots_call([good, dict(good, dst_off=47)]), "row 1: its dst range overlaps the dst range of row 0")
    # (every call above is refused before a launch: the arenas here are host memory.  Adjacent destination ranges and a shared
    # source are taken: tests/test_zzz_live_pool_gpu.py)


def test_xfade_stream_rows_refuses_bad_tables_before_any_launch():
    # S 48, O 16: H 32.  Row 0 is a good mid-recording row: 3 windows run make [0, 64) final
    good = dict(ring_off=0, out_off=0, i0=0, count=64, windows_run=3, final=0)
    final = dict(ring_off=192, out_off=100, i0=128, count=49, windows_run=6, final=1, W=6, n=177)      # 177 = 48 + 4 * 32 + 1: W = 6
    refused = lambda r, text: r[0] == -1 and r[1].startswith("ws_xfade_stream_rows_fwd: ") and text in r[1]
    assert refused(_fade_call([good], A=0), "A=0 is outside [1, 65535]")
    assert refused(_fade_call([good], ring=False), "rows, d_rows, ring or out is NULL")
    assert refused(_fade_call([good], out=False), "rows, d_rows, ring or out is NULL")
    assert refused(_fade_call([good], O=25), "overlap O=25 outside [0, S / 2] (S=48)")
    assert refused(_fade_call([good, dict(final, out_off=63)]), "row 1: its out range overlaps the out range of row 0")          # overlapping out
    assert refused(_fade_call([good, dict(final, out_off=952)]), "row 1: out [952, 952 + 49) leaves the arena of 1000 floats")   # one float past
    assert refused(_fade_call([good, dict(final, ring_off=1809)]), "row 1: ring [1809, 1809 + 4 * 48) leaves the arena of 2000 floats")
    assert refused(_fade_call([good, dict(final, scale_off=13)]), "row 1: scale_ring [13, 13 + 4) leaves the arena of 16 floats")
    assert refused(_fade_call([good, dict(final, scale_off=0)], scale=False), "row 1: scale_ring [0, 0 + 4)") \
        and "scale_ring is NULL" in L.lib().ws_last_error().decode()
    assert refused(_fade_call([good, dict(final, W=7)]), "row 1: a final range needs all W=7 windows of (n=177, S=48, O=16) run: 6 windows, 6 run")
    assert refused(_fade_call([good, dict(final, W=5, windows_run=5)]), "row 1: a final range needs all W=5 windows")             # not the layout's W
    assert refused(_fade_call([good, dict(final, count=50)]), "row 1: the range [128, 178) reaches past the recording's n=177")
    assert refused(_fade_call([dict(good, count=65), final]), "row 0: the range [0, 65) reaches past the 64 samples that the 3 windows run make final")
    assert refused(_fade_call([good, dict(good, out_off=500, count=-1)]), "row 1: bad range")
    assert refused(_fade_call([good, dict(good, out_off=500, i0=0, count=160, windows_run=6)]), "row 1: cap=4 slots do not hold windows 0..4")
    # a row with count == 0 is skipped, wherever its out_off points; a table of such rows launches nothing
    assert _fade_call([dict(good, count=0, out_off=10**9)])[0] == 0


# ---- the round rule, restated ----------------------------------------------------------------------------------------------
S_, O_, K_ = 48, 16, 2
LENGTHS = (200, 177, 31)          # 177 = S + 4 H + 1: the end-aligned last window overlaps two predecessors; 31 < S


def _separator(slot):
    """a row-independent stand-in: every target's row is a function of the window's index and its own samples"""
    mix = np.random.default_rng(100 + slot).standard_normal((K_, 3))
    return lambda w, x: np.stack([m[0] * x + m[1] * np.cos(0.1 * (w + 1) * np.arange(len(x))) + m[2] for m in mix])


_factor = lambda slot: (lambda w: 2.0 ** (((w + slot) * 7) % 5 - 2))       # powers of two: x * (1 / f) * f is x exactly


def _drive(pool, scheds, audio, attach_at, separators, factors, reattach=None):
    """Feeds slot i the packets of scheds[i] from push number attach_at[i] on, one packet a push for every slot in flight; a slot
    whose packets are used up is flushed.  reattach = (i, audio, sched): once slot i is flushed it is detached and attached again
    with that recording.  -> per recording its concatenated output, and the rounds of every push"""
    ids, pos, step, parts, rounds = {}, {}, {}, {}, []
    todo = {i: (audio[i], scheds[i]) for i in range(len(audio))}
    out, t = {}, 0
    while todo or ids:
        for i in [i for i in todo if attach_at[i] <= t]:
            x, sched = todo.pop(i)
            ids[i] = (pool.attach(separators[i], factors[i]), x, sched)
            pos[i], step[i], parts[i] = 0, 0, []
        chunks = {}
        for i, (slot, x, sched) in ids.items():
            chunks[slot] = x[pos[i]:pos[i] + sched[step[i]]]
        if chunks:
            got = pool.push(chunks)
            rounds.append(pool.rounds)
            for i, (slot, x, sched) in list(ids.items()):
                parts[i].append(got[slot])
                pos[i] += sched[step[i]]
                step[i] += 1
                if step[i] == len(sched):
                    parts[i].append(pool.flush(slot))
                    out[i] = np.concatenate(parts[i], axis=1)
                    pool.detach(slot)
                    del ids[i]
                    if reattach is not None and reattach[0] == i:
                        j = len(audio)
                        todo[j], attach_at[j] = (reattach[1], reattach[2]), t + 1
                        reattach = None
        t += 1
    return out, rounds


@pytest.mark.parametrize("max_rows", [1, 2, 8])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "factors"])
def test_pool_rule_equals_the_solo_rule_per_slot_exactly(max_rows, scaled):
    rng = np.random.default_rng(7)
    audio = [rng.standard_normal(n) for n in LENGTHS] + [rng.standard_normal(130)]         # the last one re-uses a slot
    names = ("random", "small", "160", "whole")
    scheds = [M.schedules(len(x), 11 + i)[names[i]] for i, x in enumerate(audio)]
    seps = [_separator(i) for i in range(4)]
    facs = [_factor(i) if scaled else None for i in range(4)]
    g_max = max(1, max_rows // K_)
    want = []
    for x, sched, sep, fac in zip(audio, scheds, seps, facs):
        lv, parts, N = M.Live(K_, S_, O_, g_max, sep, scale=fac), [], 0
        for c in sched:
            parts.append(lv.push(x[N:N + c]))
            N += c
        parts.append(lv.flush())
        want.append(np.concatenate(parts, axis=1))
    pool = P.Pool(3, K_, S_, O_, max_rows)
    got, rounds = _drive(pool, scheds[:3], audio[:3], {0: 0, 1: 2, 2: 5}, seps, facs, reattach=(2, audio[3], scheds[3]))
    assert sorted(got) == [0, 1, 2, 3]
    for i in range(4):
        assert got[i].shape == (K_, len(audio[i])) and np.isfinite(got[i]).all(), (i, max_rows)      # no NaN ring slot was read
        assert np.array_equal(got[i], want[i]), (i, max_rows, np.abs(got[i] - want[i]).max())
    # every forward holds at most max_rows rows, and a round's forwards are full but the last
    for push in rounds:
        for fw in push:
            assert all(f == max_rows for f in fw[:-1]) and all(1 <= f <= max_rows for f in fw)
    assert any(len(push) > 1 for push in rounds) or max_rows == 8      # "whole" owes several windows: more than one round
    # ring slots that no covering window owns stay NaN: the third recording ran one short window in ring slot 0 of its slot
    assert np.isnan(pool.ring).any()


def test_pool_rule_ring_slots_nobody_owns_stay_nan():
    pool = P.Pool(3, K_, S_, O_, 8)
    rng = np.random.default_rng(3)
    a, b = pool.attach(_separator(0)), pool.attach(_separator(1))
    pool.push({a: rng.standard_normal(S_ + 32), b: rng.standard_normal(31)})         # slot a: windows 0 and 1; slot b: none
    ring = pool.ring.reshape(3, K_, pool.cap, S_)
    assert np.isfinite(ring[a, :, :2]).all() and np.isnan(ring[a, :, 2:]).all() and np.isnan(ring[b]).all() and np.isnan(ring[2]).all()
    out = pool.flush(b)                                                               # the short window: 31 samples of ring slot 0
    assert out.shape == (K_, 31) and np.isfinite(out).all()
    ring = pool.ring.reshape(3, K_, pool.cap, S_)
    assert np.isfinite(ring[b, :, 0, :31]).all() and np.isnan(ring[b, :, 0, 31:]).all() and np.isnan(ring[b, :, 1:]).all()


# ---- dry-run engines: counts ---------------------------------------------------------------------------------------------
@needs_no_gpu
@pytest.mark.parametrize("arch", sorted(ENGINE_CASES))
def test_dry_run_live_pool_counts(tmp_path, arch):
    _, _, n, S, O = ENGINE_CASES[arch]
    H, K = S - O, 2
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    emb = np.zeros((K, 256), np.float32)
    plan = {}
    for G in range(1, 9):
        eng.separate(np.ones((G, S), np.float32), np.zeros((G, 256), np.float32), E.ENROLL_EMBEDDING)
        plan[G] = eng.info("n_launches")
    ones = lambda m: np.ones(m, np.float32)
    for max_rows in (8, 4, 1):
        pool = eng.live_pool(3, K, S, O, max_rows)
        state = eng.info("live_pool_state_bytes")
        assert state > 3 * K * (max(1, max_rows // K) + 3) * S * 4
        slots = [pool.attach(emb, E.ENROLL_EMBEDDING) for _ in range(3)]
        assert slots == [0, 1, 2] and eng.info("n_launches") == 0 and eng.info("live_pool_state_bytes") == state
        model = P.Pool(3, K, S, O, max_rows)                      # the round rule restated gives the forwards of every push
        for _ in range(3):
            model.attach(lambda w, x: np.zeros((K, len(x))))
        expect = lambda: P.launches(model.rounds, lambda rows: plan[rows])

        def push(chunks):
            got = pool.push({s: ones(m) for s, m in chunks.items()})
            ref = model.push({s: np.ones(m) for s, m in chunks.items()})
            assert {s: v.shape for s, v in got.items()} == {s: v.shape for s, v in ref.items()}
            assert not any(v.any() for v in got.values())          # a dry run computes nothing
            assert eng.info("live_pool_state_bytes") == state
            return got

        push({0: S - 1, 1: 10, 2: S - 1})
        assert eng.info("n_launches") == 0 and eng.info("live_pool_rounds") == 0 and eng.info("live_pool_forwards") == 0   # no window
        for part in ([0], [0, 1], [0, 1, 2]):                      # 1, 2 and 3 participating slots, one window each
            push({s: (1 if s == 0 and part == [0] else H if s in (0, 2) or part != [0, 1] else S - 10) for s in part})
            assert len(model.rounds) == 1 and sum(model.rounds[0]) == K * len(part), (part, model.rounds)
            assert eng.info("n_launches") == expect(), (arch, max_rows, part, model.rounds)
            assert eng.info("live_pool_rounds") == 1 and eng.info("live_pool_forwards") == len(model.rounds[0]) == -(-K * len(part) // max_rows)
        # one slot delivers a long packet beside short ones: several rounds, the count is still the formula
        push({0: 7 * H, 1: H, 2: 2 * H})
        assert len(model.rounds) > 1 and eng.info("n_launches") == expect() and eng.info("live_pool_rounds") == len(model.rounds)
        assert eng.info("live_pool_forwards") == sum(len(f) for f in model.rounds)
        for s in slots:                                           # the flushes: one more window (n_launches by the formula), or none (2)
            sl = model.sl[s]
            due = sl.N < S or (sl.N - S) % H != 0
            tail, ref = pool.flush(s), model.flush(s)
            assert tail.shape == ref.shape
            assert eng.info("n_launches") == (expect() if due else 2), (arch, max_rows, s)
            assert eng.info("live_pool_rounds") == 1 and eng.info("live_pool_forwards") == (len(model.rounds[0]) if due else 0)
            with pytest.raises(E.WesepHipError, match=f"ws_engine_live_pool_push: slot {s} .entry 0. was flushed"):
                pool.push({s: ones(10)})
            pool.detach(s)
            assert eng.info("live_pool_state_bytes") == state
        assert pool.attach(emb, E.ENROLL_EMBEDDING) == 0          # the lowest free slot again
        pool.close()
    eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _popen(eng, slots, K, window, overlap, max_rows, out=True):
    h = ctypes.c_void_p()
    return E.lib().ws_engine_live_pool_open(eng._h, slots, K, window, overlap, max_rows, ctypes.byref(h) if out else None), h


def _pattach(h, enroll, kind, elen, lengths=None, slot=True):
    s = ctypes.c_int(-1)
    enroll = np.ascontiguousarray(enroll, np.float32)
    rc = E.lib().ws_engine_live_pool_attach(h, enroll.ctypes.data, kind, elen, None if lengths is None else lengths.ctypes.data,
                                            ctypes.byref(s) if slot else None)
    return rc, s.value


def _ppush(h, entries, K=2):
    """entries: (slot, samples, est_cap) -> rc, n_out"""
    A = len(entries)
    data = [np.ones(max(m, 1), np.float32) for _, m, _ in entries]
    bufs = [np.zeros((K, max(c, 1)), np.float32) for _, _, c in entries]
    ids, n = np.array([s for s, _, _ in entries], np.int32), np.array([m for _, m, _ in entries], np.int32)
    caps, m = np.array([c for _, _, c in entries], np.int32), np.full(max(A, 1), -1, np.int32)
    cp = (ctypes.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
    ep = (ctypes.c_void_p * max(A, 1))(*[b.ctypes.data for b in bufs])
    rc = E.lib().ws_engine_live_pool_push(h, A, ids.ctypes.data, ctypes.cast(cp, ctypes.c_void_p), n.ctypes.data, ctypes.cast(ep, ctypes.c_void_p),
                                          caps.ctypes.data, m.ctypes.data)
    return rc, m.tolist()


def _pflush(h, slot, cap, K=2):
    est, m = np.zeros((K, max(cap, 1)), np.float32), ctypes.c_int(-1)
    return E.lib().ws_engine_live_pool_flush(h, slot, est.ctypes.data, cap, ctypes.byref(m)), m.value


@needs_no_gpu
def test_live_pool_refusals(tmp_path):
    emb = np.zeros((2, 256), np.float32)
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    eng.separate(np.ones((1, 2048), np.float32), emb[:1], E.ENROLL_EMBEDDING)
    mark = eng.info("n_launches")                               # a refusal launches nothing: the counter stays
    bad = lambda *a, **k: _popen(eng, *a, **k)[0] == -1 and eng.info("n_launches") == mark
    S, O, H = 2048, 512, 1536
    # open: the window checks of ws_engine_separate_long with their texts, and the pool's own
    assert bad(3, 2, 500, 100, 3) and "T=500; T >= 512" in last()
    assert bad(3, 2, S, 1025, 3) and "ws_engine_separate_long: overlap = 1025 outside [0, window / 2 = 1024]" in last()
    assert bad(3, 2, S, O, 0) and "ws_engine_separate_long: max_rows = 0" in last()
    assert bad(0, 2, S, O, 3) and "ws_engine_live_pool_open: slots=0 is outside [1, 65535]" in last()
    assert bad(65536, 2, S, O, 3) and "slots=65536 is outside [1, 65535]" in last()
    assert bad(30000, 2, S, O, 8) and "30000 slots x 2 speakers x 4 windows = 240000 rows in a round" in last()
    assert bad(3, 0, S, O, 3) and "ws_engine_live_pool_open: bad arguments (K=0" in last()
    assert bad(3, 2, S, O, 3, out=False) and "out NULL" in last()
    assert E.lib().ws_engine_live_pool_open(None, 3, 2, S, O, 3, ctypes.byref(ctypes.c_void_p())) == -1 and "ws_engine_live_pool_open: null engine" in last()
    rc, h = _popen(eng, 2, 2, S, O, 3)
    assert rc == 0
    # attach: the enrollment checks of ws_engine_separate_long, NULL pointers, a full pool
    assert _pattach(h, emb, E.ENROLL_SPEAKER, 0)[0] == -1 and "kind 3 does not fit this model" in last()
    assert _pattach(h, emb, E.ENROLL_WAVE, 16000)[0] == -1 and "kind 2 does not fit this model" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, lengths=np.array([1, 1], np.int32))[0] == -1 and "enroll_lengths given with fixed embeddings" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, slot=False)[0] == -1 and "slot NULL" in last()
    assert E.lib().ws_engine_live_pool_attach(h, None, 0, 0, None, ctypes.byref(ctypes.c_int())) == -1 and "enroll NULL" in last()
    assert _pattach(None, emb, E.ENROLL_EMBEDDING, 0)[0] == -1 and "ws_engine_live_pool_attach: null pool" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 0) and _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 1)
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0)[0] == -1 and "ws_engine_live_pool_attach: the pool is full: all 2 slots are attached" in last()
    # push
    assert _ppush(None, [(0, 10, 0)])[0] == -1 and "ws_engine_live_pool_push: null pool" in last()
    assert _ppush(h, [])[0] == -1 and "bad arguments (n_active=0 >= 1" in last()
    assert E.lib().ws_engine_live_pool_push(h, 1, None, None, None, None, None, None) == -1 and "a NULL array" in last()
    assert _ppush(h, [(2, 10, 0)])[0] == -1 and "slot 2 (entry 0) is not attached (the pool has 2 slots)" in last()
    assert _ppush(h, [(0, 10, 0), (0, 10, 0)])[0] == -1 and "slot 0 is named twice (entry 1)" in last()
    assert _ppush(h, [(0, 10, 0), (1, 0, 0)])[0] == -1 and "entry 1 (slot 1): n=0 >= 1" in last()
    # est_cap of EVERY entry is checked before anything is taken: entry 1 is short, entry 0's packet is not appended
    assert _ppush(h, [(0, S + H, H), (1, S + H, H - 1)])[0] == -1 and "entry 1 (slot 1) emits 1536 samples a row, est_cap is 1535" in last() \
        and "WS_LIVE_PUSH_CAP(n, H) = 4608 always suffices" in last()
    assert _ppush(h, [(0, S - 1, 0)]) == (0, [0]) and eng.info("n_launches") == 0          # ... so slot 0 is still before its first window
    assert _ppush(h, [(0, 1, 0), (1, 300, 0)]) == (0, [0, 0]) and eng.info("live_pool_forwards") == 1
    # flush: below pBSRNN's minimum T the slot stays as it was
    assert _pflush(None, 0, 4000)[0] == -1 and "ws_engine_live_pool_flush: null pool" in last()
    assert _pflush(h, 5, 4000)[0] == -1 and "slot 5 is not attached" in last()
    assert _pflush(h, 1, 4000)[0] == -1 and "T=300; T >= 512" in last()
    assert _ppush(h, [(1, 300, 0)]) == (0, [0])
    assert _pflush(h, 1, 599)[0] == -1 and "slot 1: the flush emits 600 samples a row, est_cap is 599" in last()
    assert E.lib().ws_engine_live_pool_flush(h, 1, None, 4000, ctypes.byref(ctypes.c_int())) == -1 and "est or n_out is NULL" in last()
    assert _pflush(h, 1, 600) == (0, 600)
    assert _ppush(h, [(0, 10, 0), (1, 10, 0)])[0] == -1 and "slot 1 (entry 1) was flushed (detach it" in last()
    assert _pflush(h, 1, 4000)[0] == -1 and "slot 1 was flushed" in last()
    assert E.lib().ws_engine_live_pool_detach(h, 1) == 0
    assert E.lib().ws_engine_live_pool_detach(h, 1) == -1 and "ws_engine_live_pool_detach: slot 1 is not attached" in last()
    assert E.lib().ws_engine_live_pool_detach(None, 1) == -1 and "null pool" in last()
    assert _ppush(h, [(1, 10, 0)])[0] == -1 and "slot 1 (entry 0) is not attached" in last()
    assert _pflush(h, 0, E.live_flush_cap(S, O)) == (0, S) and _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 1)     # slot 0 is done, not free
    E.lib().ws_engine_live_pool_close(h)
    E.lib().ws_engine_live_pool_close(None)
    eng.close()
    # the refusals by architecture of ws_engine_separate_long
    eng = E.Engine(_container(tmp_path, "ConvTasNet"), dry_run=True)
    assert _popen(eng, 2, 2, 2005, 500, 8)[0] == -1 and "nearest valid windows are 2000 and 2010" in last()
    rc, h = _popen(eng, 2, 2, 2000, 500, 8)
    assert rc == 0 and _pattach(h, emb, E.ENROLL_SPEAKER, 0)[0] == -1 and "a Conv-TasNet engine takes fixed embeddings" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, lengths=np.array([1, 1], np.int32))[0] == -1 \
        and "ws_engine_separate_long: per-row enrollment lengths are built for pBSRNN" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 0) and _ppush(h, [(0, 100, 0)]) == (0, [0])
    assert _pflush(h, 0, 4000)[0] == -1 and "Conv-TasNet needs T >= 160" in last()
    assert _ppush(h, [(0, 100, 0)]) == (0, [0]) and _pflush(h, 0, 4000) == (0, 200)
    E.lib().ws_engine_live_pool_close(h)
    eng.close()
    eng = E.Engine(_container(tmp_path, "DPCCN"), dry_run=True)
    assert _popen(eng, 2, 2, 3900, 900, 8)[0] == -1 and "a DPCCN engine needs T >= 3968" in last()
    assert _popen(eng, 2, 2, 128 * 9000, 0, 8)[0] == -1 and "R * frames * 257 * 160 below 2^31 (R=8" in last()
    eng.close()


# ---- separate_main --live_pool ---------------------------------------------------------------------------------------------
@needs_no_gpu
def test_separate_main_live_pool_dry_run(tmp_path):
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
    r = run(chunk + ["--live_ms", "100", "--live_pool", "2"])
    assert r.returncode == 0, r.stderr
    got = {l.split()[1]: tuple(map(int, re.search(r"\(live pool of (\d+) lines: (\d+) pushes of (\d+) samples", l).groups()))
           for l in r.stdout.splitlines() if l.startswith("process:")}
    assert got == {f"u{i}": (2, -(-n // 1600), 1600) for i, n in enumerate(lens)}
    # two lanes: u0 (4 pushes) and u1 (5) start together; u2 takes u0's lane at push 5, u3 takes u1's at push 6: 6 pushes in all
    m = re.search(r"^live pool: (\d+) pushes, (\d+) rounds, (\d+) forwards, (\d+) launches$", r.stdout, flags=re.M)
    assert m and int(m.group(1)) == 6, r.stdout
    windows = sum(len(E.long_windows(n, 2048, 512)) for n in lens)
    assert int(m.group(2)) <= windows and int(m.group(3)) <= windows     # a round's windows share forwards of 3 rows
    assert f"Total: process {sum(lens) * 1000 // 16000}ms audio" in r.stdout
    r2 = run(chunk + ["--live_ms", "100", "--live_pool", "2", "--jobs", "2"])
    assert r2.returncode == 0 and sorted(l.split()[1] for l in r2.stdout.splitlines() if l.startswith("process:")) == ["u0", "u1", "u2", "u3"]
    # the flag's conflicts
    r = run(chunk + ["--live_pool", "2"])
    assert r.returncode == 1 and "--live_pool needs --live_ms M" in r.stderr
    for extra in (["--batch", "2"], ["--stream_ms", "10"], ["--stream_ms", "10", "--stream_pool", "2"], ["--stream_ms", "10", "--rate_pool", "2"]):
        r = run(chunk + ["--live_ms", "100", "--live_pool", "2"] + extra)
        assert r.returncode == 1 and "--live_pool conflicts with --batch N > 1, --stream_ms, --stream_pool and --rate_pool" in r.stderr, extra
    r = run(chunk + ["--live_ms", "100", "--live_pool", "0"])
    assert r.returncode == 1 and "--live_pool needs a positive number of lines" in r.stderr
    r = run(["--live_ms", "100", "--live_pool", "2"])
    assert r.returncode == 1 and "--live_ms needs --chunk_seconds S" in r.stderr
    out = tmp_path / "out"
    out.mkdir()
    r = run(chunk + ["--live_ms", "100", "--live_pool", "3", "--resample", "--output_dir", str(out)])   # with --resample a dry run writes the files
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == sorted(f"u{i}-spk{k}.wav" for i in range(4) for k in (1, 2))
