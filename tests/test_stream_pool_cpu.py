"""CPU: the stream pool of the native runtime (ws_engine_pool_*, include/wesep_engine.h) on a dry-run engine and the real
libraries: the emission rule per slot for a schedule in which three slots attach at different rounds and push packets of
different sizes, the launch figure per group, one group per round whatever the number of slots, the constant state size,
every refusal by message, and `separate_main --stream_ms 10 --stream_pool 3 --dry_run`.  Nothing is computed in a dry run.
Without the feature every test fails (no symbol, no flag)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
KW = dict(N=32, L=20, B=32, H=64, P=3, X=3, R=2, spk_emb_dim=256)
S, LMAX, LWIN, G = 10, 160, 20, 4
GROUP = 3 * KW["R"] * KW["X"] + 9           # WS_POOL_GROUP_LAUNCHES(R, X)
PACKETS = (7, 160, 1, 333, 4000, 159, 10, 41)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _export(tmp_path, joint=False, name="c.wsw", **kw):
    from wesep_amd.models import get_model
    m = get_model("ConvTasNet")(**dict(KW, joint_training=joint, causal=True, norm="cLN", **kw))
    path = str(tmp_path / name)
    export_engine(m, path)
    return path


def _frames(n):
    return (n - LMAX) // S + 1 if n >= LMAX else 0


EMB = np.zeros(256, np.float32)


@needs_no_gpu
def test_emission_rule_launches_and_state_over_a_three_slot_schedule(tmp_path):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    pool = eng.stream_pool(3, max_chunk_frames=G)
    state = eng.info("stream_state_bytes")
    assert state > 0
    pushed, slots = {}, []
    order = {0: PACKETS, 1: PACKETS[::-1], 2: PACKETS[3:] + PACKETS[:3]}      # the same packets in different orders
    for rnd in range(len(PACKETS) + 4):
        if rnd in (0, 2, 4):                                         # attach at different rounds
            s = pool.attach(EMB, E.ENROLL_EMBEDDING)
            assert s == len(slots)
            slots.append(s)
            pushed[s] = 0
        chunks = {}
        for s in slots[::-1] if rnd % 2 else slots:                  # the order of the entries changes, too
            k = rnd - 2 * s
            if 0 <= k < len(PACKETS):
                chunks[s] = np.zeros(order[s][k], np.float32)
        if not chunks:
            continue
        before = {s: _frames(pushed[s]) for s in chunks}
        out = pool.push(chunks)
        assert set(out) == set(chunks)
        owed = []
        for s, x in chunks.items():
            pushed[s] += x.shape[0]
            new = _frames(pushed[s]) - before[s]
            owed.append(new)
            assert out[s].shape == (new * S,), (rnd, s, out[s].shape)
        n = eng.info("n_launches")
        groups = n // GROUP
        assert n == groups * GROUP                                    # a multiple of WS_POOL_GROUP_LAUNCHES
        assert groups == -(-max(owed) // G)                          # the longest row sets the number of groups, not A
        if 0 < max(owed) <= G:
            assert groups == 1, (rnd, owed)
        assert eng.info("stream_state_bytes") == state
    for s in slots:
        tail = pool.flush(s)
        Tp = (pushed[s] - LWIN) // S + 1
        assert _frames(pushed[s]) * S + tail.shape[0] == (Tp - 1) * S + LWIN and tail.shape[0] <= E.STREAM_FLUSH_CAP
        assert eng.info("n_launches") % GROUP == 0
    pool.detach(1)
    assert pool.attach(EMB, E.ENROLL_EMBEDDING) == 1                 # the freed slot is taken again, at sample 0
    assert pool.push({1: np.zeros(170, np.float32)})[1].shape == (20,)
    assert eng.info("stream_state_bytes") == state                   # no growth over pushes, detach and re-attach
    pool.close()
    eng.close()


@needs_no_gpu
@pytest.mark.parametrize("A", [1, 2, 5, 8])
def test_a_round_in_which_every_slot_owes_at_most_G_frames_is_one_group(tmp_path, A):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    pool = eng.stream_pool(8, max_chunk_frames=G)
    slots = [pool.attach(EMB, E.ENROLL_EMBEDDING) for _ in range(A)]
    pool.push({s: np.zeros(160 + s, np.float32) for s in slots})     # the first frame of every slot
    assert eng.info("n_launches") == GROUP
    out = pool.push({s: np.zeros(10 * (1 + s % G), np.float32) for s in slots})       # 1 .. G frames, unequal
    assert eng.info("n_launches") == GROUP == E.pool_group_launches(KW["R"], KW["X"])
    assert [out[s].shape[0] for s in slots] == [10 * (1 + s % G) for s in slots]
    out = pool.push({slots[0]: np.zeros(3, np.float32)})             # no frame completes: nothing is launched
    assert eng.info("n_launches") == 0 and out[slots[0]].shape == (0,)
    pool.close()
    eng.close()


@needs_no_gpu
def test_refusals(tmp_path):
    from wesep_amd.models import get_model
    gpath = str(tmp_path / "g.wsw")
    export_engine(get_model("ConvTasNet")(**dict(KW, joint_training=False)), gpath)
    geng = E.Engine(gpath, dry_run=True)
    with pytest.raises(E.WesepHipError, match="ws_engine_pool_open: this Conv-TasNet container is non-causal with gLN; streaming "
                                              "needs causal blocks with cLN"):
        geng.stream_pool(2)
    geng.close()
    eng = E.Engine(_export(tmp_path), dry_run=True)
    with pytest.raises(E.WesepHipError, match="slots=0, a pool has at least one"):
        eng.stream_pool(0)
    for g in (0, 65537):
        with pytest.raises(E.WesepHipError, match=rf"max_chunk_frames={g} is outside \[1, 65536\]"):
            eng.stream_pool(2, max_chunk_frames=g)
    with pytest.raises(E.WesepHipError, match="slots=1000000 with max_chunk_frames=64 reaches 2\\^31 elements"):
        eng.stream_pool(1000000, max_chunk_frames=64)
    pool = eng.stream_pool(2, max_chunk_frames=G)
    x = np.zeros(400, np.float32)
    with pytest.raises(E.WesepHipError, match="slot 0 .entry 0. is not attached"):
        pool.push({0: x})
    with pytest.raises(E.WesepHipError, match="takes fixed embeddings"):                 # a wrong enrollment kind
        pool.attach(np.zeros(9000, np.float32), E.ENROLL_WAVE)
    a, b = pool.attach(EMB, E.ENROLL_EMBEDDING), pool.attach(EMB, E.ENROLL_EMBEDDING)
    assert (a, b) == (0, 1)
    with pytest.raises(E.WesepHipError, match="the pool is full: all 2 slots are attached"):
        pool.attach(EMB, E.ENROLL_EMBEDDING)
    with pytest.raises(E.WesepHipError, match="slot 5 .entry 1. is not attached .the pool has 2 slots."):
        pool.push({0: x, 5: x})
    with pytest.raises(E.WesepHipError, match="n_active=0"):
        pool.push({})
    with pytest.raises(E.WesepHipError, match="entry 1 .slot 1.: n=0 >= 1"):
        pool.push({0: x, 1: x[:0]})
    # a slot named twice: through the C ABI (a dict cannot say it)
    import ctypes as C
    ids, n, caps, m = (np.array(v, np.int32) for v in ([0, 0], [400, 400], [400, 400], [0, 0]))
    cp, ep = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data), (C.c_void_p * 2)(*[np.zeros(400, np.float32).ctypes.data] * 2)
    assert E.lib().ws_engine_pool_push(pool._h, 2, ids.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data, C.cast(ep, C.c_void_p),
                                       caps.ctypes.data, m.ctypes.data) == -1
    assert "slot 0 is named twice (entry 1)" in E.lib().ws_engine_last_error().decode()
    with pytest.raises(E.WesepHipError, match="slot 0: 0 samples were pushed, fewer than the encoder window L = 20"):
        pool.flush(0)
    pool.push({0: x[:19]})
    with pytest.raises(E.WesepHipError, match="19 samples were pushed"):
        pool.flush(0)
    with pytest.raises(E.WesepHipError, match="entry 0 .slot 0. emits 260 samples, est_cap is 259"):     # 419 samples: 26 frames
        pool.push({0: x, 1: x}, est_cap={0: 259, 1: 400})
    out = pool.push({0: x, 1: x}, est_cap={0: 260, 1: 400})          # the refused push left both slots as they were
    assert out[0].shape == (260,) and out[1].shape == (250,)
    with pytest.raises(E.WesepHipError, match="the flush emits"):
        pool.flush(0, est_cap=5)
    assert pool.flush(0).shape[0] == ((419 - 20) // 10) * 10 + 20 - 260
    with pytest.raises(E.WesepHipError, match="slot 0 .entry 0. was flushed"):            # push after flush
        pool.push({0: x})
    with pytest.raises(E.WesepHipError, match="slot 0 was flushed already"):
        pool.flush(0)
    assert pool.push({1: x[:10]})[1].shape == (10,)                   # the other slot goes on
    pool.detach(0)
    with pytest.raises(E.WesepHipError, match="ws_engine_pool_detach: slot 0 is not attached"):
        pool.detach(0)
    with pytest.raises(E.WesepHipError, match="ws_engine_pool_flush: slot 0 is not attached"):
        pool.flush(0)
    assert pool.attach(EMB, E.ENROLL_EMBEDDING) == 0
    pool.close()
    eng.close()


@needs_no_gpu
def test_a_half_finished_push_bars_the_pool_until_its_slots_are_detached(tmp_path):
    """A push that fails half way leaves its slots marked; every call but detach and close is refused until they are
    detached.  The failure here: a container with H above WS_TCN_MID_MAXH, which the fused middle refuses at its first launch
    -- after the framing GEMMs of the group have been issued."""
    eng = E.Engine(_export(tmp_path, H=4100, X=1, R=1), dry_run=True)
    pool = eng.stream_pool(3, max_chunk_frames=G)
    a, b, c = (pool.attach(EMB, E.ENROLL_EMBEDDING) for _ in range(3))
    assert pool.push({c: np.zeros(100, np.float32)})[c].shape == (0,)          # no frame, no launch: fine
    with pytest.raises(E.WesepHipError, match="H=4100 above 4096"):
        pool.push({a: np.zeros(170, np.float32), b: np.zeros(165, np.float32)})
    with pytest.raises(E.WesepHipError, match="an earlier call on this pool failed half way with slot 0 in it"):
        pool.push({c: np.zeros(10, np.float32)})
    with pytest.raises(E.WesepHipError, match="ws_engine_pool_attach: an earlier call on this pool failed half way"):
        pool.attach(EMB, E.ENROLL_EMBEDDING)
    pool.detach(a)
    with pytest.raises(E.WesepHipError, match="failed half way with slot 1 in it"):
        pool.flush(c)
    pool.detach(b)
    assert pool.push({c: np.zeros(10, np.float32)})[c].shape == (0,)           # the pool takes calls again
    pool.close()
    eng.close()


def _write_wav(path, x, sr=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


@needs_no_gpu
def test_separate_main_stream_pool_dry_run_and_refusals(tmp_path):
    exe = os.path.join(ROOT, "runtime", "separate_main")
    model = _export(tmp_path, joint=True, N=256)
    rng = np.random.default_rng(1)
    lines, lens = [], {"u1": 3203, "u2": 1600, "u3": 4000, "u4": 170, "u5": 2411}
    for key, n in lens.items():
        _write_wav(tmp_path / f"{key}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"{key}_e1.wav", rng.integers(-3000, 3000, 900))
        _write_wav(tmp_path / f"{key}_e2.wav", rng.integers(-3000, 3000, 1000))
        lines.append(f"{key} {tmp_path}/{key}.wav {tmp_path}/{key}_e1.wav {tmp_path}/{key}_e2.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    run = lambda *a: subprocess.run([exe, "--wav_scp", str(scp), "--dry_run", "--model", model, *a], capture_output=True, text=True,
                                    timeout=120)
    r = run("--stream_ms", "10", "--stream_pool", "3")
    assert r.returncode == 0, r.stderr
    for key, n in lens.items():
        assert f"process: {key} RTF:" in r.stdout and f"(pool of 3 lines: {-(-n // 160)} pushes of 160 samples" in r.stdout, r.stdout
    assert "pool: " in r.stdout
    # 10 ms is 16 frames a round, 64 a group: every round is one group, whatever the number of lines in it
    rounds, launches = (int(v) for v in r.stdout.split("pool: ")[1].split(" launches")[0].split(" rounds, "))
    group = 3 * KW["R"] * KW["X"] + 9
    flush_groups = sum(1 for n in lens.values() if (n - 20) // 10 + 1 > _frames(n)) * 2
    assert launches == (rounds + flush_groups) * group
    assert rounds < sum(-(-n // 160) for n in lens.values())         # lines shared rounds
    r = run("--stream_pool", "3")
    assert r.returncode == 1 and "--stream_pool needs --stream_ms" in r.stderr
    r = run("--stream_ms", "10", "--stream_pool", "3", "--batch", "2")
    assert r.returncode == 1 and "--stream_pool conflicts with --batch" in r.stderr
    r = run("--stream_ms", "10", "--stream_pool", "3", "--chunk_seconds", "1")
    assert r.returncode == 1 and "--stream_pool conflicts" in r.stderr
    r = run("--stream_ms", "10", "--stream_pool", "0")
    assert r.returncode == 1 and "positive number of lines" in r.stderr
    r = run("--stream_ms", "10")                                     # without --stream_pool nothing changes
    assert r.returncode == 0 and "pool" not in r.stdout and "(21 pushes of 160 samples" in r.stdout
