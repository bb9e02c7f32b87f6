"""CPU-only: the live pool's store / run / due (runtime/live_pool.cc; include/wesep_engine.h "STORE, RUN, DUE"; DESIGN 7 "Live
pool").  The C ABI, the rule restated (tests/emu_live_defer.py) against the solo rule (tests/emu_live.py), the dry-run launch
arithmetic of every architecture against a push-driven twin pool, the refusals, `due` along a staggered schedule, and
`separate_main --live_pool N --live_hold_ms W`.  tests/test_zzz_live_defer_gpu.py holds the device to the same rule."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from tests import emu_live as M
from tests import emu_live_defer as D
from tests import emu_live_pool as P
from tests.test_live_host_cpu import ENGINE_CASES, _container, needs_no_gpu
from tests.test_live_pool_host_cpu import K_, LENGTHS, O_, S_, _factor, _pattach, _pflush, _popen, _ppush, _separator
from wesep_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
last = lambda: E.lib().ws_engine_last_error().decode()
CALLS = ("ws_engine_live_pool_store", "ws_engine_live_pool_run", "ws_engine_live_pool_due")


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_live_defer_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    for name in CALLS:
        assert re.search(r"^int\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in E.SYMBOLS and getattr(E.lib(), name) is not None
    for macro, fn in (("WS_LIVE_POOL_STORE_LIMIT", E.live_pool_store_limit), ("WS_LIVE_POOL_RUN_CAP", E.live_pool_run_cap)):
        assert re.search(r"^#define " + macro + r"\(S, H\) \(2 \* \(S\) \+ \(H\)\)", header, flags=re.M), macro
        assert fn(2048, 1536) == 2 * 2048 + 1536 == D.store_limit(2048, 1536) == D.run_cap(2048, 1536)
    assert all(callable(getattr(E.LivePool, f)) for f in ("store", "run", "due"))
    block = header[header.index("---- live pool (runtime/live_pool.cc"):header.index("typedef struct ws_live_pool ws_live_pool;")]
    assert "holding a complete window back" not in block and "plus whatever the caller holds" in block
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2       # new symbols only: the ABI number stays


# ---- the rule, restated: stored packets, held runs, final entries -- against the solo rule ----------------------------
@pytest.mark.parametrize("max_rows", [1, 2, 8])
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "factors"])
def test_deferred_rule_equals_the_solo_rule_per_slot_exactly(max_rows, scaled):
    """Three recordings (the last one shorter than a window) stored packet by packet at their own offsets; a run only when `due`
    reports an age of H / 2 or more, or when a recording has ended (it is then final in that run, beside the others' windows)."""
    rng = np.random.default_rng(7)
    audio = [rng.standard_normal(n) for n in LENGTHS]
    # packets of 1 .. 20 samples: with a run at an age of H / 2 = 16 at the latest, fewer than 16 + S + H + 20 = 116 samples are
    # pending after any store, below the store limit 2 S + H = 128
    scheds = []
    for x in audio:
        cuts = np.flatnonzero(rng.random(len(x) - 1) < 0.1) + 1
        cuts = np.unique(np.concatenate([cuts, np.arange(20, len(x), 20)]))
        scheds.append(np.diff(np.concatenate([[0], cuts, [len(x)]])).tolist())
        assert sum(scheds[-1]) == len(x) and 1 <= min(scheds[-1]) and max(scheds[-1]) <= 20
    seps = [_separator(i) for i in range(3)]
    facs = [_factor(i) if scaled else None for i in range(3)]
    H, g_max = S_ - O_, max(1, max_rows // K_)
    want = []
    for x, sched, sep, fac in zip(audio, scheds, seps, facs):
        lv, parts, N = M.Live(K_, S_, O_, g_max, sep, scale=fac), [], 0
        for c in sched:
            parts.append(lv.push(x[N:N + c]))
            N += c
        parts.append(lv.flush())
        want.append(np.concatenate(parts, axis=1))
    pool = D.Pool(3, K_, S_, O_, max_rows)
    slot = [pool.attach(seps[i], facs[i]) for i in range(3)]
    pos, step, parts, ended, shared = [0] * 3, [0] * 3, [[] for _ in range(3)], set(), 0
    start = (0, 3, 40)                                            # the step at which a recording starts
    t = 0
    while len(ended) < 3:
        chunks = {}
        for i in range(3):
            if t >= start[i] and step[i] < len(scheds[i]):
                c = scheds[i][step[i]]
                chunks[slot[i]] = audio[i][pos[i]:pos[i] + c]
                pos[i], step[i] = pos[i] + c, step[i] + 1
        if chunks:
            pool.store(chunks)
        final = [slot[i] for i in range(3) if step[i] == len(scheds[i]) and i not in ended]
        rows, age = pool.due()
        if final or age >= H // 2:
            ids = sorted({s for s in slot if pool.sl[s] is not None and not pool.sl[s].done and M.windows_run(pool.sl[s].N, S_, H) > pool.sl[s].Wr}
                         | set(final))
            got = pool.run(ids, final=final)
            shared += len(ids) > 1 and len(pool.rounds) >= 1
            for i in range(3):
                if slot[i] in got:
                    parts[i].append(got[slot[i]])
            ended |= {i for i in range(3) if slot[i] in final}
        t += 1
    assert shared > 0
    for i in range(3):
        got = np.concatenate(parts[i], axis=1)
        assert got.shape == (K_, len(audio[i])) and np.isfinite(got).all(), (i, max_rows)
        assert np.array_equal(got, want[i]), (i, max_rows, np.abs(got - want[i]).max())


def test_restated_push_and_flush_are_store_run_and_run_final():
    """tests/emu_live_defer.Pool.push / flush go through run(): they reproduce the parent emulation's outputs and rounds."""
    rng = np.random.default_rng(5)
    audio = [rng.standard_normal(n) for n in LENGTHS]
    a, b = P.Pool(3, K_, S_, O_, 4), D.Pool(3, K_, S_, O_, 4)
    for pool in (a, b):
        for i in range(3):
            pool.attach(_separator(i), _factor(i))
    pos = [0, 0, 0]
    for c in (17, 40, 9, 64, 31, 1, 50):
        chunks = {i: audio[i][pos[i]:pos[i] + c] for i in range(3) if pos[i] < len(audio[i])}
        ga, gb = a.push(chunks), b.push(chunks)
        assert a.rounds == b.rounds and all(np.array_equal(ga[i], gb[i]) for i in chunks)
        pos = [min(p + c, len(x)) for p, x in zip(pos, audio)]
    for i in range(3):
        assert np.array_equal(a.flush(i), b.flush(i)) and a.rounds == b.rounds


# ---- raw calls -----------------------------------------------------------------------------------------------------------
def _pstore(h, entries):
    """entries: (slot, samples) -> rc"""
    A = len(entries)
    data = [np.ones(max(m, 1), np.float32) for _, m in entries]
    ids, n = np.array([s for s, _ in entries], np.int32), np.array([m for _, m in entries], np.int32)
    cp = (ctypes.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
    return E.lib().ws_engine_live_pool_store(h, A, ids.ctypes.data, ctypes.cast(cp, ctypes.c_void_p), n.ctypes.data)


def _prun(h, entries, K=2):
    """entries: (slot, est_cap, final) -> rc, n_out"""
    A = len(entries)
    bufs = [np.zeros((K, max(c, 1)), np.float32) for _, c, _ in entries]
    ids, caps = np.array([s for s, _, _ in entries], np.int32), np.array([c for _, c, _ in entries], np.int32)
    fin, m = np.array([f for _, _, f in entries], np.int32), np.full(max(A, 1), -1, np.int32)
    ep = (ctypes.c_void_p * max(A, 1))(*[b.ctypes.data for b in bufs])
    rc = E.lib().ws_engine_live_pool_run(h, A, ids.ctypes.data, fin.ctypes.data, ctypes.cast(ep, ctypes.c_void_p), caps.ctypes.data, m.ctypes.data)
    return rc, m.tolist()


def _pdue(h):
    rows, age = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
    assert E.lib().ws_engine_live_pool_due(h, ctypes.byref(rows), ctypes.byref(age)) == 0
    return rows.value, age.value


def _counters(eng):
    return eng.info("n_launches"), eng.info("live_pool_rounds"), eng.info("live_pool_forwards")


# ---- store ------------------------------------------------------------------------------------------------------------------
@needs_no_gpu
def test_store_launches_nothing_and_carries_the_refusals_of_push(tmp_path):
    emb = np.zeros((2, 256), np.float32)
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    S, O, H = 2048, 512, 1536
    rc, h = _popen(eng, 3, 2, S, O, 8)
    assert rc == 0 and [_pattach(h, emb, E.ENROLL_EMBEDDING, 0) for _ in range(3)] == [(0, 0), (0, 1), (0, 2)]
    eng.separate(np.ones((1, S), np.float32), emb[:1], E.ENROLL_EMBEDDING)
    assert eng.info("n_launches") > 0
    assert _pstore(h, [(0, S + 10), (1, 300)]) == 0 and _counters(eng) == (0, 0, 0)          # a complete window waits: still no launch
    assert _pdue(h) == (2, 10)
    who = "ws_engine_live_pool_store: "
    assert _pstore(None, [(0, 10)]) == -1 and who + "null pool" in last()
    assert _pstore(h, []) == -1 and who + "bad arguments (n_active=0 >= 1" in last()
    assert E.lib().ws_engine_live_pool_store(h, 1, None, None, None) == -1 and who in last() and "a NULL array" in last()
    assert _pstore(h, [(3, 10)]) == -1 and who + "slot 3 (entry 0) is not attached (the pool has 3 slots)" in last()
    assert _pstore(h, [(0, 10), (0, 10)]) == -1 and who + "slot 0 is named twice (entry 1)" in last()
    assert _pstore(h, [(0, 10), (1, 0)]) == -1 and who + "entry 1 (slot 1): n=0 >= 1" in last()
    ids, n = np.array([0], np.int32), np.array([10], np.int32)
    cp = (ctypes.c_void_p * 1)(None)
    assert E.lib().ws_engine_live_pool_store(h, 1, ids.ctypes.data, ctypes.cast(cp, ctypes.c_void_p), n.ctypes.data) == -1 and "chunk NULL" in last()
    assert _pdue(h) == (2, 10)                                   # none of the refused calls appended anything
    # a flushed slot.  (The slot of a call that failed half way is refused by the same check_slot under the caller's name; a
    # dry-run engine offers no forward that fails, so -- as in tests/test_live_pool_host_cpu.py -- no test reaches that branch.)
    assert _pflush(h, 1, 4000)[0] == -1 and "T=300; T >= 512" in last()                      # refused: the slot stays as it was
    assert _pstore(h, [(1, 300)]) == 0 and _pflush(h, 1, 600) == (0, 600)
    assert _pstore(h, [(0, 10), (1, 10)]) == -1 and who + "slot 1 (entry 1) was flushed (detach it" in last()
    assert E.lib().ws_engine_live_pool_detach(h, 1) == 0
    assert _pstore(h, [(1, 10)]) == -1 and who + "slot 1 (entry 0) is not attached" in last()
    E.lib().ws_engine_live_pool_close(h)
    eng.close()


@needs_no_gpu
def test_store_backlog_bound_is_exact(tmp_path):
    emb = np.zeros((2, 256), np.float32)
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    S, O, H = 2048, 512, 1536
    limit = E.live_pool_store_limit(S, H)
    rc, h = _popen(eng, 2, 2, S, O, 8)
    assert rc == 0 and _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 0) and _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 1)
    assert _pstore(h, [(0, limit - 2), (1, 100)]) == 0
    # one sample more than the bound allows: refused, and NOTHING of the call was appended -- not slot 1's packet either
    assert _pstore(h, [(1, 50), (0, 2)]) == -1
    assert f"ws_engine_live_pool_store: entry 1 (slot 0): 2 more samples make {limit} pending, WS_LIVE_POOL_STORE_LIMIT(S, H) = {limit}: run first" in last()
    assert _pstore(h, [(1, 50), (0, 1)]) == 0                    # 2 S + H - 1 pending is accepted: the refused call left slot 0 at limit - 2
    assert _pstore(h, [(0, 1)]) == -1 and "run first" in last()
    # slot 1 holds 150 samples, not 200: a final run emits them all
    assert _prun(h, [(1, 149, 1)])[0] == -1 and "emits 150 samples a row, est_cap is 149" in last()
    # WS_LIVE_POOL_RUN_CAP suffices at the bound, for a regular and for a final entry; one below the emission is refused
    Wr = 1 + (limit - 1 - S) // H
    emitted = (Wr - 1) * H
    mark = _counters(eng)
    assert _prun(h, [(0, emitted - 1, 0)])[0] == -1 and eng.info("n_launches") == mark[0]
    assert f"ws_engine_live_pool_run: entry 0 (slot 0) emits {emitted} samples a row, est_cap is {emitted - 1}" in last() \
        and f"WS_LIVE_POOL_RUN_CAP(S, H) = {limit} always suffices" in last()
    assert _prun(h, [(0, E.live_pool_run_cap(S, H), 0)]) == (0, [emitted]) and eng.info("live_pool_rounds") >= 1
    E.lib().ws_engine_live_pool_detach(h, 0)
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0) == (0, 0) and _pstore(h, [(0, limit - 1)]) == 0
    assert _prun(h, [(0, limit - 2, 1)])[0] == -1 and f"emits {limit - 1} samples a row, est_cap is {limit - 2}" in last()
    assert _prun(h, [(0, E.live_pool_run_cap(S, H), 1)]) == (0, [limit - 1])
    E.lib().ws_engine_live_pool_close(h)
    eng.close()


# ---- run -----------------------------------------------------------------------------------------------------------------
@needs_no_gpu
@pytest.mark.parametrize("arch", sorted(ENGINE_CASES))
def test_store_then_run_counts_equal_push_on_a_twin(tmp_path, arch):
    _, _, n, S, O = ENGINE_CASES[arch]
    H, K = S - O, 2
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    emb = np.zeros((K, 256), np.float32)
    ones = lambda m: np.ones(m, np.float32)
    for max_rows in (8, 1):
        a, b = eng.live_pool(3, K, S, O, max_rows), eng.live_pool(3, K, S, O, max_rows)
        for pool in (a, b):
            assert [pool.attach(emb, E.ENROLL_EMBEDDING) for _ in range(3)] == [0, 1, 2]
        steps = [{0: S - 1, 1: 10, 2: S - 1}, {0: 1}, {0: H, 1: S - 10}, {0: H, 1: H, 2: H}, {0: S + H - 1, 1: H, 2: S}, {1: 5, 2: 5}]      # (slot 0 up to the store limit)
        for chunks in steps:
            want = a.push({s: ones(m) for s, m in chunks.items()})
            pushed = _counters(eng)
            b.store({s: ones(m) for s, m in chunks.items()})
            assert _counters(eng) == (0, 0, 0)
            got = b.run(list(chunks))
            assert _counters(eng) == pushed, (arch, max_rows, chunks)
            assert {s: v.shape for s, v in got.items()} == {s: v.shape for s, v in want.items()}
        assert _counters(eng) == (0, 0, 0) and b.run() == {} and b.due() == (0, 0)              # nothing ready: nothing launched
        for s in range(3):                                        # flush against run(final)
            want = a.flush(s)
            flushed = _counters(eng)
            got = b.run([s], final=[s])[s]
            assert _counters(eng) == flushed and got.shape == want.shape, (arch, max_rows, s)
            with pytest.raises(E.WesepHipError, match=f"ws_engine_live_pool_run: slot {s} .entry 0. was flushed"):
                b.run([s])
            with pytest.raises(E.WesepHipError, match=f"ws_engine_live_pool_store: slot {s} .entry 0. was flushed"):
                b.store({s: ones(3)})
        a.close()
        b.close()
    eng.close()


@needs_no_gpu
def test_run_refusals(tmp_path):
    emb = np.zeros((2, 256), np.float32)
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    S, O, H = 2048, 512, 1536
    rc, h = _popen(eng, 3, 2, S, O, 8)
    assert rc == 0 and [_pattach(h, emb, E.ENROLL_EMBEDDING, 0)[1] for _ in range(3)] == [0, 1, 2]
    who = "ws_engine_live_pool_run: "
    assert _prun(None, [(0, 0, 0)])[0] == -1 and who + "null pool" in last()
    assert _prun(h, [])[0] == -1 and who + "bad arguments (n_active=0 >= 1" in last()
    assert E.lib().ws_engine_live_pool_run(h, 1, None, None, None, None, None) == -1 and "a NULL array" in last()
    assert _prun(h, [(5, 0, 0)])[0] == -1 and who + "slot 5 (entry 0) is not attached" in last()
    assert _prun(h, [(0, 0, 0), (0, 0, 0)])[0] == -1 and who + "slot 0 is named twice (entry 1)" in last()
    assert _prun(h, [(0, 0, 0), (1, 4000, 1)])[0] == -1 and who + "slot 1: nothing was pushed" in last()      # final on a never-fed slot
    assert _prun(h, [(0, 0, 0), (1, 0, 0)]) == (0, [0, 0]) and _counters(eng) == (0, 0, 0)                    # nothing ready
    # est_cap of EVERY entry is checked before any launch: entry 1 is one short, nothing runs, slot 0's windows still wait
    assert _pstore(h, [(0, S + H), (1, S + H), (2, 300)]) == 0
    assert _prun(h, [(0, H, 0), (1, H - 1, 0)])[0] == -1 and who + "entry 1 (slot 1) emits 1536 samples a row, est_cap is 1535" in last()
    assert _counters(eng) == (0, 0, 0) and _pdue(h) == (8, H)
    # a short final recording below the architecture's minimum T: refused before anything runs, the slots stay as they were
    assert _prun(h, [(0, H, 0), (2, 4000, 1)])[0] == -1 and "T=300; T >= 512" in last() and _pdue(h) == (8, H)
    ids = np.array([0], np.int32)
    ep, caps, m = (ctypes.c_void_p * 1)(None), np.array([H], np.int32), np.zeros(1, np.int32)
    assert E.lib().ws_engine_live_pool_run(h, 1, ids.ctypes.data, None, ctypes.cast(ep, ctypes.c_void_p), caps.ctypes.data, m.ctypes.data) == -1 \
        and "est is NULL" in last()
    assert _prun(h, [(0, H, 0), (1, H, 0)]) == (0, [H, H]) and eng.info("live_pool_rounds") == 1        # final == all zeros / NULL: no slot ends
    assert _pstore(h, [(2, 300)]) == 0 and _prun(h, [(2, 600, 1)]) == (0, [600])
    assert _prun(h, [(2, 600, 0)])[0] == -1 and who + "slot 2 (entry 0) was flushed" in last()
    assert _ppush(h, [(2, 10, 0)])[0] == -1 and "ws_engine_live_pool_push: slot 2 (entry 0) was flushed" in last()
    assert _pflush(h, 2, 4000)[0] == -1 and "slot 2 was flushed" in last()
    assert _pdue(h) == (0, 0)
    E.lib().ws_engine_live_pool_close(h)
    eng.close()


# ---- due -----------------------------------------------------------------------------------------------------------------
def _staggered(S, H):
    """three slots, packets of `c` samples, slot i one step behind slot i - 1: no two windows complete in one packet round"""
    c = H // 3 + 1
    return c, lambda t: {i: c for i in range(3) if t >= i}


@needs_no_gpu
def test_due_follows_the_rule_and_changes_nothing(tmp_path):
    S, O = ENGINE_CASES["pBSRNN"][3:]
    H, K = S - O, 2
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    emb = np.zeros((K, 256), np.float32)
    c, at = _staggered(S, H)
    logs = []
    for query in (True, False):
        pool, model = eng.live_pool(3, K, S, O, 4), D.Pool(3, K, S, O, 4)
        for _ in range(3):
            pool.attach(emb, E.ENROLL_EMBEDDING)
            model.attach(lambda w, x: np.zeros((K, len(x))))
        log, seen = [], set()
        for t in range(24):
            chunks = at(t)
            pool.store({s: np.ones(m, np.float32) for s, m in chunks.items()})
            model.store({s: np.ones(m) for s, m in chunks.items()})
            rows, age = model.due()
            if query:
                for _ in range(2):                               # asking twice gives the same answer
                    assert pool.due() == (rows, age), t
                seen.add((rows // K, age > 0))
            if age >= H // 2 or t == 23:                         # the hold: the schedule is the emulation's, with and without queries
                ids = [s for s in range(3) if M.windows_run(model.sl[s].N, S, H) > model.sl[s].Wr]
                got, ref = pool.run(ids), model.run(ids)
                assert {s: v.shape for s, v in got.items()} == {s: v.shape for s, v in ref.items()}
                if query:
                    assert pool.due() == model.due() == (0, 0)
            log.append(_counters(eng))
        logs.append(log)
        if query:
            assert {n for n, _ in seen} >= {0, 1, 2, 3}          # none, one, two and three windows waiting were all met
        pool.close()
    assert logs[0] == logs[1] and any(l[1] for l in logs[0])
    eng.close()


# ---- sharing, as launch arithmetic ------------------------------------------------------------------------------------------
@needs_no_gpu
@pytest.mark.parametrize("arch", sorted(ENGINE_CASES))
def test_staggered_slots_share_one_round_and_a_final_slot_adds_no_forward(tmp_path, arch):
    _, _, _, S, O = ENGINE_CASES[arch]
    H, K = S - O, 2
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    emb = np.zeros((K, 256), np.float32)
    plan = {}
    for G in range(1, 9):
        eng.separate(np.ones((G, S), np.float32), np.zeros((G, 256), np.float32), E.ENROLL_EMBEDDING)
        plan[G] = eng.info("n_launches")
    short = S - 40
    eng.separate(np.ones((K, short), np.float32), emb, E.ENROLL_EMBEDDING)
    plan_short = {K: eng.info("n_launches")}
    eng.separate(np.ones((1, short), np.float32), emb[:1], E.ENROLL_EMBEDDING)
    plan_short[1] = eng.info("n_launches")
    ones = lambda m: np.ones(m, np.float32)
    c, at = _staggered(S, H)
    for max_rows in (8, 4, 1):
        held, pushed = eng.live_pool(4, K, S, O, max_rows), eng.live_pool(4, K, S, O, max_rows)
        for pool in (held, pushed):
            assert [pool.attach(emb, E.ENROLL_EMBEDDING) for _ in range(3)] == [0, 1, 2]
        rounds_pushed, t, first = 0, 0, []
        while held.due()[0] < 3 * K:                              # until the third slot's first window is complete
            chunks = {s: ones(m) for s, m in at(t).items()}
            held.store(chunks)
            pushed.push(chunks)
            r = eng.info("live_pool_rounds")
            assert r in (0, 1) and (r == 0 or eng.info("live_pool_forwards") == -(-K // max_rows))
            rounds_pushed += r
            first.append(r)
            t += 1
        assert rounds_pushed == 3 and max(first) == 1             # through push: three rounds, no two windows in one push
        assert held.due() == (3 * K, t * c - S)                   # slot 0 waits longest: t packets, its window 0 complete at S
        got = held.run()
        fw = [min(max_rows, 3 * K - r) for r in range(0, 3 * K, max_rows)]
        assert sorted(got) == [0, 1, 2] and _counters(eng) == (E.live_pool_launches([[plan[f] for f in fw]]), 1, -(-3 * K // max_rows))
        # two regular slots and one final slot with n >= S in one run: still one chain, the last window is a row among the others'
        N = [(t - i) * c for i in range(3)]
        more = {0: S + H - N[0], 1: S + H - N[1], 2: 7}            # slots 0 and 1 complete window 1; slot 2 ends off the hop grid
        assert (N[2] + 7 - S) % H != 0 and N[2] + 7 < S + H
        held.store({s: ones(m) for s, m in more.items()})
        assert held.due() == (2 * K, 0)
        got = held.run(final=[2])
        assert [got[s].shape for s in range(3)] == [(K, H), (K, H), (K, N[2] + 7)]
        assert _counters(eng) == (E.live_pool_launches([[plan[f] for f in fw]]), 1, -(-3 * K // max_rows)), (arch, max_rows)
        # the same through push and flush: the flush is a round of its own
        pushed.push({s: ones(m) for s, m in more.items()})
        assert eng.info("live_pool_rounds") == 1 and eng.info("live_pool_forwards") == -(-2 * K // max_rows)
        pushed.flush(2)
        assert eng.info("live_pool_rounds") == 1 and eng.info("live_pool_forwards") == -(-K // max_rows)
        # a short recording (n < S) ends beside two regular windows: one round, its rows in forwards of their own
        s3 = held.attach(emb, E.ENROLL_EMBEDDING)
        assert s3 == 3
        held.store({0: ones(H), 1: ones(H), s3: ones(short)})
        got = held.run(final=[s3])
        fw2 = [min(max_rows, 2 * K - r) for r in range(0, 2 * K, max_rows)]
        fw3 = [min(max_rows, K - r) for r in range(0, K, max_rows)]
        assert got[s3].shape == (K, short) and got[0].shape == (K, H)
        assert _counters(eng) == (E.live_pool_launches([[plan[f] for f in fw2] + [plan_short[f] for f in fw3]]), 1, len(fw2) + len(fw3))
        # a final slot that still owes a regular window: that window first, its end in the next round
        held.store({0: ones(H + 9)})
        held.run(final=[0])
        assert eng.info("live_pool_rounds") == 2 and eng.info("live_pool_forwards") == 2 * -(-K // max_rows)
        held.close()
        pushed.close()
    eng.close()


# ---- separate_main --live_pool N --live_hold_ms W ----------------------------------------------------------------------------
@needs_no_gpu
def test_separate_main_live_hold_dry_run(tmp_path):
    from tests.test_ragged_host_cpu import _write_wav
    from tests.test_longform_host_cpu import _container as joint_container
    exe = os.path.join(ROOT, "runtime", "separate_main")
    assert os.path.exists(exe), "run python -m wesep_amd.build"
    model = joint_container(tmp_path, "pBSRNN")
    rng = np.random.default_rng(0)
    lens = (5000, 8300, 6100, 9000, 2048, 1000, 7777)            # lanes take their next line at different rounds: staggered windows
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1000 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 1000 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    base = [exe, "--wav_scp", str(scp), "--model", model, "--dry_run"]
    chunk = ["--chunk_seconds", "0.128", "--overlap_seconds", "0.032", "--chunk_rows", "6", "--live_ms", "20"]      # S 2048, H 1536, packets of 320; a forward holds the three lines' rows
    run = lambda extra: subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
    total = {}
    for tag, extra in (("push", []), ("hold", ["--live_hold_ms", "96"])):
        r = run(chunk + ["--live_pool", "3"] + extra)
        assert r.returncode == 0, r.stderr
        got = {l.split()[1]: tuple(map(int, re.search(r"\(live pool of (\d+) lines: (\d+) pushes of (\d+) samples", l).groups()))
               for l in r.stdout.splitlines() if l.startswith("process:")}
        assert got == {f"u{i}": (3, -(-n // 320), 320) for i, n in enumerate(lens)}, (tag, r.stdout)      # every key once, the line as it was
        m = re.search(r"^live pool: (\d+) pushes, (\d+) rounds, (\d+) forwards, (\d+) launches$", r.stdout, flags=re.M)
        assert m, r.stdout
        total[tag] = tuple(map(int, m.groups()))
        total[tag] += (re.search(r"^Total: process (\d+)ms audio", r.stdout, flags=re.M).group(1),)
    print("separate_main --live_pool 3 (pushes, rounds, forwards, launches):", total)
    assert total["hold"][2] < total["push"][2] and total["hold"][1] < total["push"][1]
    assert total["hold"][4] == total["push"][4]                  # the same audio (a lane that waits for its last run takes its next line later)
    r = run(chunk + ["--live_hold_ms", "96"])
    assert r.returncode == 1 and "--live_hold_ms needs --live_pool N" in r.stderr
    r = run(["--chunk_seconds", "0.128", "--tail_ms", "20", "--live_hold_ms", "96"])
    assert r.returncode == 1 and "--live_hold_ms needs --live_pool N" in r.stderr
    r = run(chunk + ["--live_pool", "3", "--live_hold_ms", "-1"])
    assert r.returncode == 1 and "--live_hold_ms needs a hold of 0 ms or more" in r.stderr
    out = tmp_path / "out"
    out.mkdir()
    r = run(chunk + ["--live_pool", "3", "--live_hold_ms", "96", "--resample", "--output_dir", str(out)])
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(out)) == sorted(f"u{i}-spk{k}.wav" for i in range(len(lens)) for k in (1, 2))
