"""CPU: the four streaming front ends of the native runtime -- solo stream, stream pool, rate stream, rate pool -- traced call by
call on a dry-run engine, with block_kernel off and on, against a table recorded BEFORE they were rebuilt on one launch chain, one
state block and one emission rule (stream_frontends_frozen.json: what this same trace gave at commit c3dbeea).  After every
call: the samples returned per row or slot and ws_engine_info("n_launches"); after open and at the end: stream_state_bytes and
arena_bytes; the push caps for n in {0, 1, 160, 4800}.  The rate front ends get a packet longer than max_push.
The failure schedule: a group that fails half way (H = 4100, above the kernels' limit, as in
test_a_half_finished_push_bars_the_pool_until_its_slots_are_detached), its slots detached, then a push that succeeds.
  rate pool  its push already released the work arena on every path at c3dbeea: "after_failure" is the arena_bytes of a FRESH
             engine for the same successful push ("fresh"; that push allocates more than the failed group did, so the figure is
             its own), then and now
  pool       the one line that differs from c3dbeea on purpose: a failed group now gives its work-arena allocations back, where it
             used to leave them live under everything allocated later.  With H = 4100 no push that allocates can succeed, so no
             fresh engine can be compared; the table holds the failed push's own peak ("failed_peak", as recorded at c3dbeea),
             which the attaches and the push that follow must not raise.  c3dbeea gave failed_peak + the attach's embedding
             buffer there and at "end" (the json's "_c3dbeea_after_failure")."""
import json
import os

import numpy as np
import pytest

from tests.test_stream_pool_cpu import EMB, KW, PACKETS, _export, needs_no_gpu
from wesep_amd import engine as E

G, SR = 4, 16000
CAPS = (0, 1, 160, 4800)
RATES = (8000, 48000, SR, 44100)
FRONTS = ("stream", "pool", "rate_stream_8000", "rate_stream_16000", "rate_pool", "pool_failure", "rate_pool_failure")
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stream_frontends_frozen.json")


def _pool_rounds(pool, slots, rates, note):
    for k, p in enumerate(PACKETS):                                  # not every slot in every round
        chunks = {s: np.zeros(max(1, p * r // SR), np.float32) for s, r in zip(slots, rates) if (k + s) % 4 != 3}
        out = pool.push(chunks)
        note(f"push{k}", [out[s].shape[0] if s in out else -1 for s in slots])
    for s in slots:
        note(f"flush{s}", pool.flush(s).shape[0])


def _after(pool, attach, c):
    """what follows the detaches: both slots attached again, and a push of three short packets that completes no frame"""
    d, e = attach(0), attach(1)
    return [v.shape[0] for v in pool.push({c: np.zeros(20, np.float32), d: np.zeros(70, np.float32), e: np.zeros(70, np.float32)}).values()]


def _failure(pool, attach, note, sizes):
    """a and b fail half way in their first group; they are detached, and the pool takes calls again"""
    a, b, c = attach(0), attach(1), attach(2)
    note("small", pool.push({c: np.zeros(50, np.float32)})[c].shape[0])
    with pytest.raises(E.WesepHipError, match="H=4100 above"):
        pool.push({a: np.zeros(340, np.float32), b: np.zeros(165, np.float32)})
    sizes("failed_peak")
    pool.detach(a)
    pool.detach(b)
    note("after", _after(pool, attach, c))
    sizes("after_failure")


def _trace(tmp_path, front, bk):
    """every record is [what, value, n_launches] or [what, stream_state_bytes, arena_bytes]"""
    rec = []
    failure = front.endswith("_failure")
    eng = E.Engine(_export(tmp_path, **(dict(H=4100, X=1, R=1) if failure else {})), dry_run=True)
    note = lambda what, v: rec.append([what, v, eng.info("n_launches")])
    sizes = lambda what: rec.append([what, eng.info("stream_state_bytes"), eng.info("arena_bytes")])
    if front == "stream" or front.startswith("rate_stream"):
        rate = int(front.split("_")[-1]) if front != "stream" else SR
        enroll = np.stack([EMB, EMB])
        if front == "stream":
            st = eng.stream(2, enroll, E.ENROLL_EMBEDDING, max_chunk_frames=G, block_kernel=bk)
        else:
            st = eng.rate_stream(2, enroll, E.ENROLL_EMBEDDING, rate, max_chunk_frames=G, max_push=1000, block_kernel=bk)
            note("caps", [st.push_cap(n) for n in CAPS])
        note("open", 0)
        sizes("open")
        for k, p in enumerate(PACKETS):
            note(f"push{k}", st.push(np.zeros((2, max(1, p * rate // SR)), np.float32)).shape[1])
        note("flush", st.flush().shape[1])
        st.reset()
        note("again", st.push(np.zeros((2, 400 * rate // SR), np.float32)).shape[1])
        st.close()
    elif front in ("pool", "rate_pool"):
        rated = front == "rate_pool"
        pool = eng.rate_pool(4, RATES, max_chunk_frames=G, max_push=4800, block_kernel=bk) if rated else \
            eng.stream_pool(4, max_chunk_frames=G, block_kernel=bk)
        rates = RATES if rated else (SR,) * 4
        attach = lambda i: pool.attach(EMB, E.ENROLL_EMBEDDING, rates[i]) if rated else pool.attach(EMB, E.ENROLL_EMBEDDING)
        sizes("open")
        slots = []
        for i in range(4):
            slots.append(attach(i))
            note(f"attach{i}", slots[-1])
        if rated:
            note("caps", [[pool.push_cap(s, n) for n in CAPS] for s in slots])
        _pool_rounds(pool, slots, rates, note)
        pool.detach(1)
        note("attach_again", attach(0))                              # the freed slot, at slot 0's rate, at sample 0
        note("again", pool.push({1: np.zeros(400 * rates[0] // SR, np.float32)})[1].shape[0])
        pool.close()
    elif front == "pool_failure":
        pool = eng.stream_pool(3, max_chunk_frames=G, block_kernel=bk)
        _failure(pool, lambda i: pool.attach(EMB, E.ENROLL_EMBEDDING), note, sizes)
        pool.close()
    else:
        # max_push = 200000 sizes the staging block of resampler A: the three rows of the push that follows the failure take more
        # of the arena than the two rows and the group of the failed one, so arena_bytes is that push's own figure
        fresh = E.Engine(_export(tmp_path, name="f.wsw", H=4100, X=1, R=1), dry_run=True)
        for e in (fresh, eng):
            pool = e.rate_pool(3, [8000], max_chunk_frames=G, max_push=200000, block_kernel=bk)
            attach = lambda i, pool=pool: pool.attach(EMB, E.ENROLL_EMBEDDING, (8000, SR, 8000)[i])
            if e is fresh:                                           # the same calls without the failed push
                a, b, c = attach(0), attach(1), attach(2)
                pool.push({c: np.zeros(50, np.float32)})
                pool.detach(a), pool.detach(b)
                _after(pool, attach, c)
                rec.append(["fresh", e.info("stream_state_bytes"), e.info("arena_bytes")])
            else:
                _failure(pool, attach, note, sizes)
            pool.close()
        fresh.close()
    sizes("end")
    eng.close()
    return rec


@needs_no_gpu
@pytest.mark.parametrize("block_kernel", [False, True])
@pytest.mark.parametrize("front", FRONTS)
def test_the_trace_of_a_front_end_is_what_it_was_before_the_rebuild(tmp_path, front, block_kernel):
    want = json.load(open(TABLE))[f"{front}/{int(block_kernel)}"]
    got = json.loads(json.dumps(_trace(tmp_path, front, block_kernel)))
    for g, w in zip(got, want):
        assert g == w, (front, block_kernel, g, w)
    assert len(got) == len(want)
    if front == "rate_pool_failure":                                 # the failed group's allocations went back to the arena
        by = {r[0]: r for r in got}
        assert by["after_failure"][2] == by["fresh"][2] > by["failed_peak"][2], by
    if front == "pool_failure":
        by = {r[0]: r for r in got}
        assert by["after_failure"][2] == by["failed_peak"][2], by
