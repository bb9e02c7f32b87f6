"""CPU-only: the rate tail pool (runtime/rate_tail_pool.cc; ws_window_resample_rows_fwd of resample.hip; DESIGN 7 "Rate tail
pool").  The C ABI, the kernel's refusals on host buffers, the rule restated (tests/emu_rate_tail.py: samples against integers),
the dry-run counts and launch plan of pBSRNN, Conv-TasNet and DPCCN containers, the runtime's refusals and `separate_main
--tail_rate_pool`.  tests/test_zzz_rate_tail_gpu.py holds the device to the same rule."""
import ctypes
import os
import re
import subprocess
import wave

import numpy as np
import pytest

from tests import emu_rate_tail as RT
from tests import emu_tail as T
from tests.test_live_host_cpu import ENGINE_CASES, _container, needs_no_gpu
from wesep_amd import _lib as L
from wesep_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
last = lambda: E.lib().ws_engine_last_error().decode()
CALLS = ("ws_engine_rate_tail_pool_open", "ws_engine_rate_tail_pool_attach", "ws_engine_rate_tail_pool_cap", "ws_engine_rate_tail_pool_room",
         "ws_engine_rate_tail_pool_push", "ws_engine_rate_tail_pool_tick", "ws_engine_rate_tail_pool_flush", "ws_engine_rate_tail_pool_detach",
         "ws_engine_rate_tail_pool_close")
ARCHS = ("pBSRNN", "ConvTasNet", "DPCCN")
WARM = {"pBSRNN": 1000, "ConvTasNet": 500, "DPCCN": 3968}


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_rate_tail_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    name = "ws_window_resample_rows_fwd"
    m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
    assert m, f"{name} is not declared in wesep_hip.h"
    res, args = L._SIGS[name]
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")) == 10, name
    assert name in L.EXPORTED_SYMBOLS and getattr(L.lib(), name) is not None
    from wesep_amd import dev
    assert callable(dev.window_resample_rows)
    # the descriptor, field for field
    assert L.WINDOW_RESAMPLE_ROW.itemsize == 64
    assert L.WINDOW_RESAMPLE_ROW.names == ("in_off", "taps_off", "out_off", "U", "D", "K", "lead", "n_valid", "final", "g_first", "p_first",
                                           "L", "fill")
    assert re.search(r"typedef struct ws_window_resample_row \{\s*long long in_off, taps_off, out_off;\s*int U, D, K;\s*"
                     r"int lead, n_valid, final, g_first, p_first, L, fill;\s*\} ws_window_resample_row;", header)
    eheader = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    arity = {"open": 10, "attach": 8, "cap": 2, "room": 2, "push": 5, "tick": 6, "flush": 5, "detach": 2, "close": 1}
    for name in CALLS:
        m = re.search(r"^(int|void)\s+" + name + r"\s*\(([^;]*)\);", eheader, flags=re.M)
        assert m and (m.group(1) == "void") == name.endswith("close"), name
        fn = getattr(E.lib(), name)
        assert name in E.SYMBOLS and len(fn.argtypes) == len(m.group(2).split(",")) == arity[name.rsplit("_", 1)[1]], name
    m = re.search(r"^#define WS_RATE_TAIL_TICK_LAUNCHES (\d+)\s", eheader, flags=re.M)
    assert m and int(m.group(1)) == E.RATE_TAIL_TICK_LAUNCHES == 3
    assert E.rate_tail_launches([19, 19]) == 38 + 3 + 1
    assert callable(E.Engine.rate_tail_pool) and callable(E.Engine.rate_tail)
    assert all(callable(getattr(E.RateTailPool, f)) for f in ("attach", "push", "tick", "flush", "detach", "close", "cap", "room"))
    assert L.lib().ws_abi_version() == 20                     # new symbols only: neither ABI number moves
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


# ---- the kernel's refusals -----------------------------------------------------------------------------------------------
def _gather_call(rows, n_buf=4000, n_taps=600, n_y=3000, A=None, buf=True, taps=True, y=True, d_rows=True, same_arena=False):
    from wesep_amd import dev
    tab = dev.window_resample_rows_table(rows) if rows else np.zeros(1, L.WINDOW_RESAMPLE_ROW)
    a, b, c = (ctypes.c_float * 4000)(), (ctypes.c_float * 600)(), (ctypes.c_float * 3000)()
    vp = lambda x, on: ctypes.cast(x, ctypes.c_void_p) if on else None
    t = ctypes.c_void_p(tab.ctypes.data)
    rc = L.lib().ws_window_resample_rows_fwd(t, t if d_rows else None, len(rows) if A is None else A, vp(a, buf), n_buf, vp(b, taps), n_taps,
                                             vp(a if same_arena else c, y), n_buf if same_arena else n_y, None)
    return rc, L.lib().ws_last_error().decode()


def test_window_resample_rows_refuses_bad_tables_before_any_launch():
    # 48 kHz -> 16 kHz: U 1, D 3, w 19, K 41.  Row 0: 257 outputs from group 5 on need (5 + 256) 3 + 41 = 824 samples; 3 zeros behind
    good = dict(in_off=2, taps_off=1, out_off=3, U=1, D=3, K=41, lead=0, n_valid=824, final=0, g_first=5, p_first=0, L=257, fill=3)
    # 8 kHz -> 16 kHz: U 2, D 1, w 7, K 15.  Row 1: 100 outputs from phase 1 of group 3 end in group 53: 53 + 15 = 68 samples
    two = dict(in_off=1000, taps_off=100, out_off=400, U=2, D=1, K=15, lead=0, n_valid=68, final=0, g_first=3, p_first=1, L=100, fill=0)
    who = "ws_window_resample_rows_fwd"
    refused = lambda r, text: r[0] == -1 and r[1].startswith(who + ": ") and text in r[1]
    assert refused(_gather_call([good], A=0), "A=0 is outside [1, 65535]")
    assert refused(_gather_call([good], A=65536), "A=65536 is outside [1, 65535]")
    for off in ("buf", "taps", "y", "d_rows"):
        assert refused(_gather_call([good], **{off: False}), "rows, d_rows, buf, taps or y is NULL"), off
    assert refused(_gather_call([good], n_y=-1), "an arena length is negative")
    # the checks of ws_resample_stream_rows_fwd that apply, with the row index
    assert refused(_gather_call([good, dict(two, U=0)]), "row 1: U=0, D=1; U and D lie in [1, 1024]")
    assert refused(_gather_call([good, dict(two, D=1025)]), "row 1: U=2, D=1025; U and D lie in [1, 1024]")
    assert refused(_gather_call([good, dict(two, K=4097)]), "row 1: K=4097 taps per output sample; K lies in [1, 4096]")
    assert refused(_gather_call([good, dict(two, K=0)]), "row 1: K=0 taps per output sample")
    assert refused(_gather_call([good, dict(two, D=17)]), "row 1: K=15 is below D=17")
    assert refused(_gather_call([good, dict(two, K=16)]), "row 1: K - D = 15 is odd (K = 2 w + D)")
    assert refused(_gather_call([good, dict(two, n_valid=0)]), "row 1: bad sizes (n_valid=0 >= 1")
    assert refused(_gather_call([good, dict(two, L=-1)]), "row 1: bad sizes (n_valid=68 >= 1, L=-1")
    assert refused(_gather_call([good, dict(two, fill=-1)]), "fill=-1, one of them positive")
    assert refused(_gather_call([good, dict(two, L=0, fill=0)]), "L=0, fill=0, one of them positive")
    assert refused(_gather_call([good, dict(two, lead=8)]), "row 1: lead=8 outside [0, w=7]")
    assert refused(_gather_call([good, dict(two, lead=-1)]), "row 1: lead=-1 outside [0, w=7]")
    assert refused(_gather_call([good, dict(two, g_first=-1)]), "g_first=-1 negative")
    # the phase
    assert refused(_gather_call([good, dict(two, p_first=2)]), "row 1: p_first=2 is outside [0, U=2)")
    assert refused(_gather_call([good, dict(two, p_first=-1)]), "row 1: p_first=-1 is outside [0, U=2)")
    assert refused(_gather_call([dict(good, p_first=1)]), "row 0: p_first=1 is outside [0, U=1)")
    # final = 0: an output whose taps fall behind n_valid -- at the exact boundary
    assert refused(_gather_call([good, dict(two, n_valid=67)]), "row 1: outputs up to 107 need 68 valid samples, 67 are given and the end is not final")
    assert _gather_call([good, dict(two, L=101)])[0] != -1                                     # output 107 is still of group 53
    assert refused(_gather_call([good, dict(two, L=102)]), "row 1: outputs up to 109 need 69 valid samples, 68 are given")        # one more group
    assert refused(_gather_call([dict(good, n_valid=823)]), "row 0: outputs up to 262 need 824 valid samples, 823 are given")
    # final = 1: outputs past ceil(U (n_valid + lead - w) / D); 68 samples from group 0's first tap end the signal at output 2 (68 - 7) = 122
    assert refused(_gather_call([good, dict(two, final=1, n_valid=53)]), "row 1: outputs up to 107 asked, the 53 valid samples end the signal at output 92")
    assert refused(_gather_call([good, dict(two, final=1, L=116)]), "row 1: outputs up to 123 asked, the 68 valid samples end the signal at output 122")
    assert _gather_call([dict(good, final=1, n_valid=803)])[0] != -1                            # ceil((803 - 19) / 3) = 262: allowed
    assert refused(_gather_call([dict(good, final=1, n_valid=802)]), "row 0: outputs up to 262 asked, the 802 valid samples end the signal at output 261")
    # ranges that leave their arenas: one float past
    assert refused(_gather_call([good, dict(two, in_off=3933)]), "row 1: buf [3933, 3933 + 68) leaves the arena of 4000 floats")
    assert refused(_gather_call([good, dict(two, in_off=-1)]), "row 1: buf [-1,")
    assert refused(_gather_call([good, dict(two, taps_off=571)]), "row 1: taps [571, 571 + 2 * 15) leaves the arena of 600 floats")
    assert refused(_gather_call([good, dict(two, out_off=2901)]), "row 1: y [2901, 2901 + 100 + 0) leaves the arena of 3000 floats")
    assert refused(_gather_call([dict(good, out_off=2741)]), "row 0: y [2741, 2741 + 257 + 3) leaves the arena of 3000 floats")   # the zeros count
    assert refused(_gather_call([good, dict(two, out_off=-1)]), "row 1: y [-1,")
    # a destination that meets any other range of the call: another destination (its zeros included), a span (one arena)
    assert refused(_gather_call([good, dict(two, out_off=262)]), "row 1: its y range overlaps the y range of row 0")
    assert _gather_call([good, dict(two, out_off=263)])[0] != -1                                # right behind row 0's zeros
    assert refused(_gather_call([dict(good, out_off=2000), dict(two, out_off=1067)], same_arena=True), "row 1: its y range overlaps the buf range of row 1")
    assert refused(_gather_call([dict(good, out_off=2000), dict(two, out_off=825)], same_arena=True), "row 1: its y range overlaps the buf range of row 0")
    assert refused(_gather_call([dict(good, out_off=825)], same_arena=True), "row 0: its y range overlaps the buf range of row 0")
    # two rows may share a span: good tables are not refused for their arguments (rc -2: there is no device to launch on here)
    rc, _ = _gather_call([good, dict(two, in_off=2, out_off=300)])
    assert rc != -1


# ---- the rule, restated: samples against integers -----------------------------------------------------------------------
def _separator(K):
    return lambda x: np.stack([(k + 1) * x + 0.25 * np.cos(0.1 * np.arange(len(x))) for k in range(K)])


@pytest.mark.parametrize("rate", [8000, 16000, 22050, 44100, 48000])
def test_rate_tail_rule_counts_and_totals(rate):
    """The emulation on samples returns what the integers say, and a slot totals exactly the samples pushed -- B's uncropped total
    is never below N_c.  At the container's rate the samples are the plain tail rule's."""
    rng = np.random.default_rng(rate)
    K, S, C, warm = 2, 1000, 32, 500              # (22.05 kHz arrives in groups of 320 samples: a window must hold a few)
    for trial in range(3):
        n = int(rng.integers(1, 3 * S * rate // 16000))
        x = rng.standard_normal(n)
        slot = RT.RateTail(K, S, C, warm, rate, 16000, _separator(K))
        plain = T.Tail(K, S, C, warm, _separator(K))
        parts, plain_parts, pos = [], [], 0
        while pos < n:
            c = min(int(rng.integers(1, 500 * rate // 16000 + 2)), n - pos, slot.counts.room())
            assert c >= 1
            slot.push(x[pos:pos + c])
            pos += c
            got = slot.tick()
            parts += [] if got is None else [got]
            if rate == 16000:
                plain.push(x[pos - c:pos])
                got = plain.tick()
                plain_parts += [] if got is None else [got]
        # B's uncropped total, before the flush crops it
        n_model = RT.out_len(n, rate, 16000)
        assert RT.out_len(n_model, 16000, rate) >= n, (rate, n)
        parts.append(slot.flush())
        out = np.concatenate(parts, axis=1)
        assert out.shape == (K, n) and slot.counts.returned == n
        if rate == 16000:
            assert np.array_equal(out, np.concatenate(plain_parts + [plain.flush()], axis=1))
    c = RT.Counts(S, C, warm, rate, 16000)
    c.push(c.room())
    with pytest.raises(ValueError, match="tick first"):
        c.push(1)


# ---- dry-run engines: counts ---------------------------------------------------------------------------------------------
RATES = (8000, 16000, 44100, 48000)


@needs_no_gpu
@pytest.mark.parametrize("arch", ARCHS)
def test_dry_run_rate_tail_pool_counts(tmp_path, arch):
    _, _, _, S, _ = ENGINE_CASES[arch]
    K, C, warm = 2, 128, WARM[arch]
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    emb = np.zeros((K, 256), np.float32)
    plan = {}

    def count(fw):                                               # a forward's rectangular count, from ws_engine_separate itself
        if fw not in plan:
            eng.separate(np.ones(fw, np.float32), np.zeros((fw[0], 256), np.float32), E.ENROLL_EMBEDDING)
            plan[fw] = eng.info("n_launches")
        return plan[fw]

    for max_rows in (8, 1):
        pool = eng.rate_tail_pool(4, K, S, C, [8000, 44100, 48000], warm, max_rows)
        state = eng.info("rate_tail_pool_state_bytes")
        assert state > 4 * K * S * 4 * 2
        slot, model, pushed, got_n = {}, {}, {}, {}
        packets = {r: int(0.04 * r + 0.5) for r in RATES}
        life = {8000: 14, 16000: 11, 44100: 12, 48000: 9}            # rounds a recording lives: flushes at different rounds
        added, hold_only = [], False
        t = 0
        while t < 2 * len(RATES) or model:
            if t % 2 == 0 and t // 2 < len(RATES):                  # attaches two rounds apart
                r = RATES[t // 2]
                slot[r] = pool.attach(emb, E.ENROLL_EMBEDDING, r)
                assert eng.info("n_launches") == 0 and pool.cap(slot[r]) == RT.cap(S, r, 16000)
                model[r], pushed[r], got_n[r] = RT.Counts(S, C, warm, r, 16000), 0, 0
                model[r].born = t
            chunks = {}
            for r, m in model.items():
                assert pool.room(slot[r]) == m.room()
                c = min(packets[r], m.room())
                chunks[slot[r]] = np.ones(c, np.float32)
                m.push(c)
                pushed[r] += c
            pool.push(chunks)
            assert eng.info("rate_tail_pool_state_bytes") == state
            firing = sorted((slot[r], r) for r, m in model.items() if m.fires())
            want = {r: m.tick() for r, m in model.items()}
            got = pool.tick()
            lengths = [want[r][0] for _, r in firing]
            assert {s: v.shape for s, v in got.items()} == {slot[r]: (K, w[1]) for r, w in want.items() if w is not None and w[1] > 0}, (arch, t)
            for r, w in want.items():
                got_n[r] += w[1] if w else 0
            fw = T.tick_forwards(lengths, K, S, max_rows)
            assert eng.info("rate_tail_pool_forwards") == len(fw) and eng.info("rate_tail_pool_rows") == K * len(lengths)
            # the header's formula; a tick in which nothing fires launches nothing
            n_launches = eng.info("n_launches")                     # (count() runs the engine: read the tick's counter first)
            assert n_launches == (E.rate_tail_launches([count(f) for f in fw]) if fw else 0), (arch, max_rows, t, fw)
            if fw:
                added.append((len(firing), n_launches - sum(count(f) for f in fw)))
            assert eng.info("rate_tail_pool_state_bytes") == state
            for r in [r for r, m in model.items() if t - m.born + 1 == life[r]]:
                L_last, n_last = model[r].flush()
                tail = pool.flush(slot[r])
                assert tail.shape == (K, n_last) and (L_last > 0 or r == 16000)
                fw = T.tick_forwards([L_last], K, S, max_rows) if L_last else []
                # (only the slot at the container's rate can end on a firing: the copy of its hold, B, the copy to the host)
                n_launches = eng.info("n_launches")
                assert eng.info("rate_tail_pool_forwards") == len(fw)
                assert n_launches == (E.rate_tail_launches([count(f) for f in fw]) if fw else 3), (arch, r)
                hold_only |= not fw
                got_n[r] += n_last
                assert got_n[r] == pushed[r] > 0, (arch, r)             # each slot totals exactly the samples pushed
                pool.detach(slot[r])
                assert eng.info("rate_tail_pool_state_bytes") == state
                del model[r]
            t += 1
        # one firing slot and three or four: what the pool adds to the forwards is the same
        assert {a for _, a in added} == {E.RATE_TAIL_TICK_LAUNCHES + 1} and min(f for f, _ in added) == 1 and max(f for f, _ in added) >= 3, added
        assert hold_only
        pool.close()
    eng.close()


@needs_no_gpu
def test_dry_run_engine_rate_tail_returns_what_it_was_given(tmp_path):
    """Engine.rate_tail: one recording, chunks of any size (one longer than the slot takes: cut to `room`, a tick between the
    pieces); the ticks and the flush total exactly the samples pushed, at every rate."""
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    emb = np.zeros((2, 256), np.float32)
    for rate in RATES:
        tail = eng.rate_tail(emb, E.ENROLL_EMBEDDING, 2048, 128, rate, warm=1000)
        sizes = [1, 5000 * rate // 16000, 333, 2 * 2048 * rate // 16000 + 7, 40 * rate // 1000]
        parts = [tail.push(np.ones(n, np.float32)) for n in sizes] + [tail.flush()]
        assert all(p.shape[0] == 2 for p in parts) and sum(p.shape[1] for p in parts) == sum(sizes), rate
        assert parts[1].shape[1] > 0
        tail.close()
    with pytest.raises(E.WesepHipError, match="a slot at this rate never fires"):
        eng.rate_tail(emb, E.ENROLL_EMBEDDING, 2048, 128, 8000, warm=2048)
    eng.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def _popen(eng, slots, K, window, fade, warm, max_rows, rates=(8000, 48000), out=True):
    h = ctypes.c_void_p()
    r = np.array(rates, np.int32)
    return E.lib().ws_engine_rate_tail_pool_open(eng._h, slots, K, window, fade, warm, max_rows, r.ctypes.data, len(r),
                                                 ctypes.byref(h) if out else None), h


def _pattach(h, enroll, kind, elen, rate, enroll_rate=0, slot=True):
    s = ctypes.c_int(-1)
    enroll = np.ascontiguousarray(enroll, np.float32)
    rc = E.lib().ws_engine_rate_tail_pool_attach(h, enroll.ctypes.data, kind, elen, None, enroll_rate, rate, ctypes.byref(s) if slot else None)
    return rc, s.value


def _ppush(h, entries):
    A = len(entries)
    data = [np.ones(max(m, 1), np.float32) for _, m in entries]
    ids, n = np.array([s for s, _ in entries], np.int32), np.array([m for _, m in entries], np.int32)
    cp = (ctypes.c_void_p * max(A, 1))(*[x.ctypes.data for x in data])
    return E.lib().ws_engine_rate_tail_pool_push(h, A, ids.ctypes.data, ctypes.cast(cp, ctypes.c_void_p), n.ctypes.data)


def _ptick(h, entries, K=2):
    A = len(entries)
    bufs = [np.zeros((K, max(c, 1)), np.float32) for _, c in entries]
    ids, caps, m = np.array([s for s, _ in entries], np.int32), np.array([c for _, c in entries], np.int32), np.full(max(A, 1), -1, np.int32)
    ep = (ctypes.c_void_p * max(A, 1))(*[b.ctypes.data for b in bufs])
    rc = E.lib().ws_engine_rate_tail_pool_tick(h, A, ids.ctypes.data, ctypes.cast(ep, ctypes.c_void_p), caps.ctypes.data, m.ctypes.data)
    return rc, m.tolist()


def _pflush(h, slot, cap, K=2):
    est, m = np.zeros((K, max(cap, 1)), np.float32), ctypes.c_int(-1)
    return E.lib().ws_engine_rate_tail_pool_flush(h, slot, est.ctypes.data, cap, ctypes.byref(m)), m.value


@needs_no_gpu
def test_rate_tail_pool_refusals(tmp_path):
    emb = np.zeros((2, 256), np.float32)
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    eng.separate(np.ones((1, 2048), np.float32), emb[:1], E.ENROLL_EMBEDDING)
    mark = eng.info("n_launches")                               # a refusal launches nothing: the counter stays
    bad = lambda *a, **k: _popen(eng, *a, **k)[0] == -1 and eng.info("n_launches") == mark
    S, C, W = 2048, 128, 1000
    who = "ws_engine_rate_tail_pool_"
    # open: the tail pool's checks under this family's name, and the rates
    assert bad(3, 2, 500, 100, 500, 3) and "T=500; T >= 512" in last()
    assert bad(3, 2, S, 1025, S, 3) and who + "open: fade = 1025 outside [0, window / 2 = 1024]" in last()
    assert bad(3, 2, S, C, S + 1, 3) and who + "open: warm = 2049 outside [max(fade, 1) = 128, window = 2048]" in last()
    assert bad(3, 2, S, C, 511, 3) and "T=511; T >= 512" in last()
    assert bad(0, 2, S, C, W, 3) and who + "open: slots=0 is outside [1, 65535]" in last()
    assert bad(40000, 2, S, C, W, 8) and "40000 slots x 2 speakers = 80000 rows in a tick" in last()
    assert bad(3, 0, S, C, W, 3) and who + "open: bad arguments (K=0" in last()
    assert bad(3, 2, S, C, W, 3, out=False) and "out NULL" in last()
    assert bad(3, 2, S, C, W, 3, rates=(8000, 0)) and who + "open: rates[1]: " in last() and "must be positive" in last()
    assert bad(3, 2, S, C, W, 3, rates=(16001,)) and "rates[0]: " in last() and "U and D may not exceed 1024" in last()
    assert E.lib().ws_engine_rate_tail_pool_open(eng._h, 3, 2, S, C, W, 3, None, 2, ctypes.byref(ctypes.c_void_p())) == -1 and "rates is NULL" in last()
    rc, h = _popen(eng, 3, 2, S, C, W, 3)
    assert rc == 0
    # attach: an unlisted rate gets the accepted ones; the rate pool's and the tail pool's refusals
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 44100)[0] == -1 and \
        who + "attach: sample_rate=44100 is not one of the rates this pool was opened with (accepted: 16000, 8000, 48000)" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 8000, enroll_rate=8000)[0] == -1 and "only a waveform enrollment (WS_ENROLL_WAVE) has a sample rate" in last()
    assert _pattach(h, emb, E.ENROLL_SPEAKER, 0, 8000)[0] == -1 and "kind 3 does not fit this model" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 8000, slot=False)[0] == -1 and "slot NULL" in last()
    assert _pattach(None, emb, E.ENROLL_EMBEDDING, 0, 8000)[0] == -1 and who + "attach: null pool" in last()
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 8000) == (0, 0) and _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 48000) == (0, 1)
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 16000) == (0, 2)
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 16000)[0] == -1 and who + "attach: the pool is full: all 3 slots are attached" in last()
    assert eng.info("n_launches") == 0
    cap8, cap48 = RT.cap(S, 8000, 16000), RT.cap(S, 48000, 16000)
    assert E.lib().ws_engine_rate_tail_pool_cap(h, 0) == cap8 and E.lib().ws_engine_rate_tail_pool_cap(h, 1) == cap48
    assert E.lib().ws_engine_rate_tail_pool_cap(h, 7) == -1 and E.lib().ws_engine_rate_tail_pool_room(h, 7) == -1
    # push: the overflow rule at its exact boundary.  8 kHz: ceil(2 n) <= 2048; 48 kHz: ceil(n / 3) <= 2048
    assert _ppush(h, [(0, 10), (0, 10)]) == -1 and "slot 0 is named twice (entry 1)" in last()
    assert _ppush(h, [(0, 10), (1, 0)]) == -1 and "entry 1 (slot 1): n=0 >= 1" in last()
    assert E.lib().ws_engine_rate_tail_pool_room(h, 0) == 1024 and E.lib().ws_engine_rate_tail_pool_room(h, 1) == 6144
    # the overflow is found before ANY entry is appended: entry 0's packet is not taken either
    assert _ppush(h, [(0, 1024), (1, 6145)]) == -1 and who + "push: entry 1 (slot 1): 6145 more samples at 48000 Hz make 2049 at the container's " \
        "rate that have not come out, a window holds 2048: tick first" in last()
    assert _ppush(h, [(0, 1025)]) == -1 and "1025 more samples at 8000 Hz make 2050" in last()
    assert _ppush(h, [(0, 1024), (1, 6144)]) == 0 and _ppush(h, [(0, 1)]) == -1 and "tick first" in last()
    assert E.lib().ws_engine_rate_tail_pool_room(h, 0) == 0
    assert eng.info("n_launches") == 0                            # no push launches
    # tick: est_cap of EVERY entry is checked before anything runs.  Slot 0 has N = 2 (1024 - 7) = 2034 and emits 2034 - 128 = 1906
    # at the container's rate, of which B returns floor((1906 - 13) / 2) = 946; slot 1: N = (6144 - 19) / 3 = 2041, 1913 into B,
    # 3 (1913 - 7) = 5718 out
    assert _ptick(h, [(0, cap8), (0, cap8)])[0] == -1 and "slot 0 is named twice (entry 1)" in last()
    assert _ptick(h, [(0, cap8), (1, 5717)])[0] == -1 and who + "tick: entry 1 (slot 1) emits 5718 samples a row, est_cap is 5717" in last() \
        and f"ws_engine_rate_tail_pool_cap(pool, 1) = {cap48} always suffices" in last() and eng.info("n_launches") == 0
    assert _ptick(h, [(0, 946), (1, 5718), (2, 0)]) == (0, [946, 5718, 0]) and eng.info("rate_tail_pool_rows") == 4
    assert _ptick(h, [(0, 0), (1, 0)]) == (0, [0, 0]) and eng.info("n_launches") == 0       # nothing new: no slot fires
    assert E.lib().ws_engine_rate_tail_pool_room(h, 0) == (2048 + 1906) // 2 - 1024
    # flush
    assert _pflush(h, 2, S)[0] == -1 and "slot 2: nothing was pushed" in last()
    assert _pflush(h, 0, 1024 - 946 - 1)[0] == -1 and who + "flush: slot 0: the flush emits 78 samples a row, est_cap is 77" in last()
    assert _pflush(h, 0, 78) == (0, 78)                           # 946 + 78 = the 1024 pushed
    assert _ppush(h, [(0, 10)]) == -1 and "slot 0 (entry 0) was flushed (detach it" in last()
    assert _pflush(h, 0, S)[0] == -1 and "slot 0 was flushed" in last()
    assert _pflush(h, 1, cap48) == (0, 6144 - 5718)
    assert E.lib().ws_engine_rate_tail_pool_detach(h, 0) == 0
    assert E.lib().ws_engine_rate_tail_pool_detach(h, 0) == -1 and who + "detach: slot 0 is not attached" in last()
    # a short recording below pBSRNN's minimum T: the flush is refused and the slot goes on
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 8000) == (0, 0) and _ppush(h, [(0, 150)]) == 0
    assert _pflush(h, 0, S)[0] == -1 and "T=300; T >= 512" in last()
    assert _ppush(h, [(0, 150)]) == 0 and _pflush(h, 0, S) == (0, 300)
    E.lib().ws_engine_rate_tail_pool_close(h)
    E.lib().ws_engine_rate_tail_pool_close(None)
    # a rate whose slots could never fire: warm = S leaves the filter's look-ahead no room
    rc, h = _popen(eng, 2, 2, S, C, S, 3)
    assert rc == 0 and _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 16000) == (0, 0)
    assert _pattach(h, emb, E.ENROLL_EMBEDDING, 0, 8000)[0] == -1 and "a slot at this rate never fires: warm = 2048" in last() and "warm <= 2034" in last()
    E.lib().ws_engine_rate_tail_pool_close(h)
    eng.close()
    # a TF-GridNet container is refused by name
    eng = E.Engine(_container(tmp_path, "TFGridNet"), dry_run=True)
    assert _popen(eng, 2, 2, 2048, 128, 1000, 3)[0] == -1 and who + "open: a TF-GridNet container is not taken" in last()
    eng.close()


# ---- separate_main --tail_rate_pool ----------------------------------------------------------------------------------------
@needs_no_gpu
def test_separate_main_tail_rate_pool_dry_run(tmp_path):
    from tests.test_ragged_host_cpu import _write_wav
    from tests.test_longform_host_cpu import _container as joint_container
    exe = os.path.join(ROOT, "runtime", "separate_main")
    assert os.path.exists(exe), "run python -m wesep_amd.build"
    model = joint_container(tmp_path, "pBSRNN")
    rng = np.random.default_rng(0)
    files = ((8000, 4000), (16000, 4800), (48000, 19200), (8000, 1600))       # 500 + 300 + 400 + 200 ms
    lines = []
    for i, (sr, n) in enumerate(files):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n), sr)
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, (20000 + 1000 * i) * sr // 16000), sr)
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 1000 * i), 16000 if i == 2 else sr)     # line 2: a pair at two rates
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    out = tmp_path / "out"
    out.mkdir()
    base = [exe, "--wav_scp", str(scp), "--model", model, "--dry_run"]
    chunk = ["--chunk_seconds", "0.128", "--chunk_rows", "3"]
    run = lambda extra: subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
    r = run(chunk + ["--tail_ms", "40", "--tail_rate_pool", "2", "--output_dir", str(out)])
    assert r.returncode == 0, r.stderr
    pat = r"\(rate tail pool of 2 lines: (\d+) Hz, (\d+) ticks, packets of (\d+) samples, fade (\d+),"
    got = {l.split()[1]: tuple(map(int, re.search(pat, l).groups())) for l in r.stdout.splitlines() if l.startswith("process:")}
    assert {k: (v[0], v[2], v[3]) for k, v in got.items()} == {f"u{i}": (sr, sr * 40 // 1000, 160) for i, (sr, _) in enumerate(files)}, r.stdout
    assert all(got[f"u{i}"][1] >= -(-n // (sr * 40 // 1000)) for i, (sr, n) in enumerate(files))        # a cut packet adds a tick
    m = re.search(r"^rate tail pool: (\d+) ticks, (\d+) rows, (\d+) forwards, (\d+) launches$", r.stdout, flags=re.M)
    assert m and int(m.group(2)) > 0 and int(m.group(3)) > 0, r.stdout
    assert "Total: process 1400ms audio" in r.stdout
    # the files are written at each mixture's rate and length
    assert sorted(os.listdir(out)) == sorted(f"u{i}-spk{k}.wav" for i in range(4) for k in (1, 2))
    for i, (sr, n) in enumerate(files):
        for k in (1, 2):
            with wave.open(str(out / f"u{i}-spk{k}.wav"), "rb") as w:
                assert (w.getframerate(), w.getnframes()) == (sr, n), (i, k)
    # the conflicts, by name
    r = run(chunk + ["--tail_rate_pool", "2"])
    assert r.returncode == 1 and "--tail_rate_pool needs --tail_ms M" in r.stderr
    r = run(["--tail_ms", "40", "--tail_rate_pool", "2"])
    assert r.returncode == 1 and "--tail_ms needs --chunk_seconds S" in r.stderr
    r = run(chunk + ["--tail_ms", "40", "--tail_rate_pool", "2", "--tail_pool", "2"])
    assert r.returncode == 1 and "--tail_rate_pool conflicts with --tail_pool" in r.stderr
    r = run(chunk + ["--tail_ms", "40", "--tail_rate_pool", "2", "--resample"])
    assert r.returncode == 1 and "--tail_rate_pool conflicts with --resample" in r.stderr
    r = run(chunk + ["--tail_ms", "40", "--tail_rate_pool", "0"])
    assert r.returncode == 1 and "--tail_rate_pool needs a positive number of lines" in r.stderr
    for extra in (["--batch", "2"], ["--stream_ms", "10"], ["--live_ms", "100"], ["--stream_ms", "10", "--rate_pool", "2"]):
        r = run(chunk + ["--tail_ms", "40", "--tail_rate_pool", "2"] + extra)
        assert r.returncode == 1 and "--tail_ms conflicts with --batch N > 1, --stream_ms, --live_ms, --live_pool, --stream_pool and --rate_pool" in r.stderr, extra
    r = run(chunk + ["--tail_ms", "40", "--tail_rate_pool", "2", "--tail_warm_seconds", "0.128"])
    assert r.returncode == 1 and "a slot at this rate never fires" in r.stderr
    # the existing messages are untouched: without --resample a plain tail pool still refuses a file at another rate
    r = run(chunk + ["--tail_ms", "40", "--tail_pool", "2"])
    assert r.returncode == 1 and "u0: sample rate is not 16000" in r.stderr
    r = run(chunk + ["--tail_pool", "2"])
    assert r.returncode == 1 and "need --tail_ms M" in r.stderr
