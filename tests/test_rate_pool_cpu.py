"""CPU: the rate pool of the native runtime (ws_engine_rate_pool_*, include/wesep_engine.h) on a dry-run engine and the real
libraries: the symbols and launch macros, the emission rule per slot with slots at 8, 48, 16 and 44.1 kHz in one pool, the
total after the flush, a packet longer than max_push, the launch figure of a round for 1, 2 and 4 active slots and for one
or three distinct rates, the constant state size, and every refusal by message.  In a dry run nothing is computed, but every
entry point validates its arguments -- the host tables of the rows kernels included, so the pool's bookkeeping (offsets,
histories, pending samples) is checked by the kernels' own refusals.  Without the feature every test fails (no symbol)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import resample_contract as RC
from tests.test_stream_pool_cpu import EMB, KW, PACKETS, _export
from wesep_amd import engine as E

needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G, L, SR = 4, 20, 16000
GROUP = E.pool_group_launches(KW["R"], KW["X"]) + 2
NAMES = ("ws_engine_rate_pool_open", "ws_engine_rate_pool_attach", "ws_engine_rate_pool_push", "ws_engine_rate_pool_push_cap",
         "ws_engine_rate_pool_flush", "ws_engine_rate_pool_detach", "ws_engine_rate_pool_close")


def _emitted(n, rate):
    return RC.rate_stream_emitted(n, rate, SR, L) if rate != SR else RC.plain_emitted(n, L)


def _total(n, rate):
    return RC.rate_stream_total(n, rate, SR, L) if rate != SR else RC.plain_total(n, L)


def test_rate_pool_symbols_and_launch_macros():
    header = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    for name in NAMES:
        assert re.search(r"^(int|void)\s+" + name + r"\s*\(", header, flags=re.M), name
        assert name in E.SYMBOLS and getattr(E.lib(), name) is not None
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2
    assert "#define WS_RATE_POOL_GROUP_LAUNCHES(R, X) (WS_POOL_GROUP_LAUNCHES(R, X) + 2)" in header
    assert "#define WS_RATE_POOL_BLOCK_GROUP_LAUNCHES(R, X) (WS_POOL_BLOCK_GROUP_LAUNCHES(R, X) + 2)" in header
    assert f"#define WS_RATE_POOL_PIECE_LAUNCHES {E.RATE_POOL_PIECE_LAUNCHES}" in header
    assert f"#define WS_RATE_POOL_BLOCK_PIECE_LAUNCHES {E.RATE_POOL_BLOCK_PIECE_LAUNCHES}" in header
    assert E.rate_pool_group_launches(4, 8) == E.pool_group_launches(4, 8) + 2
    assert E.rate_pool_block_group_launches(4, 8) == E.pool_block_group_launches(4, 8) + 2


@needs_no_gpu
@pytest.mark.parametrize("block_kernel", [False, True])
def test_emission_rule_and_state_with_four_rates_in_one_pool(tmp_path, block_kernel):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    rates = [8000, 48000, SR, 44100]
    pool = eng.rate_pool(4, [8000, 48000, 44100], max_chunk_frames=G, max_push=4800, block_kernel=block_kernel)
    state = eng.info("stream_state_bytes")
    assert state > 0
    slots = [pool.attach(EMB, E.ENROLL_EMBEDDING, r) for r in rates]
    assert slots == [0, 1, 2, 3] and eng.info("stream_state_bytes") == state
    pushed = dict.fromkeys(slots, 0)
    for k, p in enumerate(PACKETS):
        chunks = {s: np.zeros(max(1, p * r // SR), np.float32) for s, r in zip(slots, rates) if (k + s) % 4 != 3}     # not every slot every round
        out = pool.push(chunks)
        assert set(out) == set(chunks)
        for s, x in chunks.items():
            before = _emitted(pushed[s], rates[s])
            pushed[s] += x.shape[0]
            assert out[s].shape == (_emitted(pushed[s], rates[s]) - before,), (k, s)
            assert out[s].shape[0] <= pool.push_cap(s, x.shape[0])
        assert eng.info("stream_state_bytes") == state
    for s in slots:
        tail = pool.flush(s)
        assert _emitted(pushed[s], rates[s]) + tail.shape[0] == _total(pushed[s], rates[s]) <= pushed[s]
        assert tail.shape[0] <= pool.push_cap(s, 0) and eng.info("stream_state_bytes") == state
    pool.detach(1)
    assert pool.attach(EMB, E.ENROLL_EMBEDDING, 8000) == 1            # the freed 48 kHz slot, now at 8 kHz, at sample 0
    assert pool.push({1: np.zeros(200, np.float32)})[1].shape == (_emitted(200, 8000),)
    assert eng.info("stream_state_bytes") == state
    pool.close()
    eng.close()


@needs_no_gpu
def test_a_packet_longer_than_max_push_is_taken_in_pieces(tmp_path):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    pool = eng.rate_pool(2, [8000, 48000], max_chunk_frames=G, max_push=480)
    a, b = pool.attach(EMB, E.ENROLL_EMBEDDING, 48000), pool.attach(EMB, E.ENROLL_EMBEDDING, 8000)
    out = pool.push({a: np.zeros(12000, np.float32), b: np.zeros(80, np.float32)})       # 25 pieces of a beside one of b
    assert out[a].shape == (_emitted(12000, 48000),) and out[b].shape == (_emitted(80, 8000),)
    n = eng.info("n_launches")
    # piece j ends at 480 (j + 1) samples of a: resampler A runs when it emits, the groups are ceil(new frames / G), the
    # compaction and resampler B run when a frame ran; b rides in piece 0 and adds nothing to the count
    want, frames = 0, 0
    for j in range(25):
        done = RC.plain_emitted(RC.emitted(480 * (j + 1), 48000, SR), L) // 10
        new_a = RC.emitted(480 * (j + 1), 48000, SR) - RC.emitted(480 * j, 48000, SR)
        want += (1 if new_a or j == 0 else 0) + GROUP * -(-(done - frames) // G) + (2 if done > frames else 0)
        frames = done
    assert frames > 16 * 23 and n == want, (n, want)
    out = pool.push({a: np.zeros(481, np.float32)})
    assert out[a].shape == (_emitted(12481, 48000) - _emitted(12000, 48000),)
    pool.close()
    eng.close()


@needs_no_gpu
@pytest.mark.parametrize("block_kernel", [False, True])
def test_the_launches_of_a_round_do_not_depend_on_slots_or_rates(tmp_path, block_kernel):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    group = (E.rate_pool_block_group_launches if block_kernel else E.rate_pool_group_launches)(KW["R"], KW["X"])
    piece = E.RATE_POOL_BLOCK_PIECE_LAUNCHES if block_kernel else E.RATE_POOL_PIECE_LAUNCHES
    figures = []
    for rates in ([8000], [48000, 48000], [SR, SR, SR, SR], [8000, 48000, SR, 8000], [48000, SR]):
        pool = eng.rate_pool(4, [8000, 48000], max_chunk_frames=G, max_push=4800, block_kernel=block_kernel)
        slots = [pool.attach(EMB, E.ENROLL_EMBEDDING, r) for r in rates]
        pool.push({s: np.zeros(r // 50, np.float32) for s, r in zip(slots, rates)})       # 20 ms: the first frames
        pool.push({s: np.zeros(r // 400, np.float32) for s, r in zip(slots, rates)})      # 2.5 ms in mid-stream: 4 frames, one group
        figures.append(eng.info("n_launches"))
        pool.close()
    assert figures == [group + piece] * 5, figures
    eng.close()


@needs_no_gpu
def test_refusals(tmp_path):
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    gpath = str(tmp_path / "g.wsw")
    export_engine(get_model("ConvTasNet")(**dict(KW, joint_training=False)), gpath)
    geng = E.Engine(gpath, dry_run=True)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_open: this Conv-TasNet container is non-causal with gLN"):
        geng.rate_pool(2, [8000])
    geng.close()
    eng = E.Engine(_export(tmp_path), dry_run=True)
    with pytest.raises(E.WesepHipError, match=r"ws_engine_rate_pool_open: unknown flag bits 0x2"):
        E.RatePool(eng, 2, [8000], flags=3)
    with pytest.raises(E.WesepHipError, match=r"ws_engine_rate_pool_open: bad arguments \(slots=0 in \[1, 65535\]"):
        eng.rate_pool(0, [8000])
    for mp in (0, (1 << 24) + 1):
        with pytest.raises(E.WesepHipError, match=rf"max_push={mp} in \[1, 2\^24\]"):
            eng.rate_pool(2, [8000], max_push=mp)
    with pytest.raises(E.WesepHipError, match=r"ws_engine_rate_pool_open: rates\[1\]: ws_resample_geom: 16001 -> 16000 reduces to U=16000, D=16001"):
        eng.rate_pool(2, [8000, 16001])
    with pytest.raises(E.WesepHipError, match=r"rates\[0\]: ws_resample_geom: rate_in=0"):
        eng.rate_pool(2, [0])
    with pytest.raises(E.WesepHipError, match=r"max_chunk_frames=0 is outside \[1, 65536\]"):
        eng.rate_pool(2, [8000], max_chunk_frames=0)
    pool = eng.rate_pool(2, [8000, 48000], max_chunk_frames=G, max_push=4800)
    x = np.zeros(400, np.float32)
    with pytest.raises(E.WesepHipError, match=r"ws_engine_rate_pool_attach: sample_rate=44100 is not one of the rates this pool was opened "
                                              r"with \(accepted: 16000, 8000, 48000\)"):
        pool.attach(EMB, E.ENROLL_EMBEDDING, 44100)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_attach: enroll_rate=8000 with enrollment kind 0: only a waveform enrollment"):
        pool.attach(EMB, E.ENROLL_EMBEDDING, 8000, enroll_rate=8000)
    with pytest.raises(E.WesepHipError, match="takes fixed embeddings"):
        pool.attach(np.zeros(9000, np.float32), E.ENROLL_WAVE, 8000)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_push: slot 0 .entry 0. is not attached"):
        pool.push({0: x}, est_cap={0: 400})
    a, b = pool.attach(EMB, E.ENROLL_EMBEDDING, 8000), pool.attach(EMB, E.ENROLL_EMBEDDING, SR)
    assert (a, b) == (0, 1)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_attach: the pool is full: all 2 slots are attached"):
        pool.attach(EMB, E.ENROLL_EMBEDDING, 48000)
    with pytest.raises(E.WesepHipError, match="n_active=0"):
        pool.push({})
    with pytest.raises(E.WesepHipError, match="entry 1 .slot 1.: n=0 >= 1"):
        pool.push({0: x, 1: x[:0]})
    ids, n, caps, m = (np.array(v, np.int32) for v in ([0, 0], [400, 400], [900, 900], [0, 0]))
    cp, ep = (C.c_void_p * 2)(x.ctypes.data, x.ctypes.data), (C.c_void_p * 2)(*[np.zeros(900, np.float32).ctypes.data] * 2)
    assert E.lib().ws_engine_rate_pool_push(pool._h, 2, ids.ctypes.data, C.cast(cp, C.c_void_p), n.ctypes.data, C.cast(ep, C.c_void_p),
                                            caps.ctypes.data, m.ctypes.data) == -1
    assert "ws_engine_rate_pool_push: slot 0 is named twice (entry 1)" in E.lib().ws_engine_last_error().decode()
    with pytest.raises(E.WesepHipError, match="slot 0: 0 samples were pushed, 0 at the container's rate, fewer than the encoder window L = 20"):
        pool.flush(0)
    pool.push({0: x[:9]})
    with pytest.raises(E.WesepHipError, match="slot 0: 9 samples were pushed, 18 at the container's rate"):
        pool.flush(0)
    emit = _emitted(409, 8000)
    with pytest.raises(E.WesepHipError, match=rf"entry 0 .slot 0. emits {emit} samples, est_cap is {emit - 1} "
                                              rf".ws_engine_rate_pool_push_cap.pool, 0, 400. = \d+ always suffices"):
        pool.push({0: x, 1: x}, est_cap={0: emit - 1, 1: 400})
    out = pool.push({0: x, 1: x}, est_cap={0: emit, 1: 400})          # the refused push left both slots as they were
    assert out[0].shape == (emit,) and out[1].shape == (RC.plain_emitted(400, L),)
    with pytest.raises(E.WesepHipError, match=r"the flush emits \d+ samples, est_cap is 5 .ws_engine_rate_pool_push_cap.pool, 0, 0."):
        pool.flush(0, est_cap=5)
    assert pool.flush(0).shape[0] == _total(409, 8000) - emit
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_push: slot 0 .entry 0. was flushed"):
        pool.push({0: x})
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_flush: slot 0 was flushed already"):
        pool.flush(0)
    assert pool.push({1: x[:10]})[1].shape == (10,)                   # the other slot goes on
    pool.detach(0)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_detach: slot 0 is not attached"):
        pool.detach(0)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_flush: slot 0 is not attached"):
        pool.flush(0)
    assert pool.push_cap(0, 10) == -1 and pool.push_cap(1, 10) > 0
    assert pool.attach(EMB, E.ENROLL_EMBEDDING, 48000) == 0
    pool.close()
    eng.close()


@needs_no_gpu
def test_a_half_finished_push_bars_the_pool_until_its_slots_are_detached(tmp_path):
    """the pool's own rule (tests/test_stream_pool_cpu.py), through the rate pool: H above WS_TCN_MID_MAXH fails a group half way"""
    eng = E.Engine(_export(tmp_path, H=4100, X=1, R=1), dry_run=True)
    pool = eng.rate_pool(3, [8000], max_chunk_frames=G)
    a, b, c = (pool.attach(EMB, E.ENROLL_EMBEDDING, r) for r in (8000, SR, 8000))
    assert pool.push({c: np.zeros(50, np.float32)})[c].shape == (0,)            # no frame: fine
    with pytest.raises(E.WesepHipError, match="H=4100 above 4096"):
        pool.push({a: np.zeros(100, np.float32), b: np.zeros(165, np.float32)})
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_push: an earlier call on this pool failed half way with slot 0 in it"):
        pool.push({c: np.zeros(10, np.float32)})
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_attach: an earlier call on this pool failed half way"):
        pool.attach(EMB, E.ENROLL_EMBEDDING, 8000)
    pool.detach(a)
    with pytest.raises(E.WesepHipError, match="failed half way with slot 1 in it"):
        pool.flush(c)
    pool.detach(b)
    assert pool.push({c: np.zeros(10, np.float32)})[c].shape == (0,)            # the pool takes calls again
    pool.close()
    eng.close()


@needs_no_gpu
def test_waveform_enrollment_at_another_rate(tmp_path):
    eng = E.Engine(_export(tmp_path, joint=True, N=256), dry_run=True)
    pool = eng.rate_pool(2, [8000], max_chunk_frames=G)
    s = pool.attach(np.zeros(450, np.float32), E.ENROLL_WAVE, 8000, enroll_rate=8000)     # 900 samples at the container's rate
    plain = eng.info("n_launches")
    t = pool.attach(np.zeros(900, np.float32), E.ENROLL_WAVE, 8000)
    assert (s, t) == (0, 1) and plain == eng.info("n_launches") + 1                       # the enrollment's resampling is one launch
    pool.detach(0)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_pool_attach: ws_resample_geom: rate_in=-5"):
        pool.attach(np.zeros(450, np.float32), E.ENROLL_WAVE, 8000, enroll_rate=-5)
    assert pool.attach(np.zeros(450, np.float32), E.ENROLL_WAVE, 8000, enroll_rate=8000) == 0
    pool.close()
    eng.close()


def _wav_info(path):
    import wave
    with wave.open(str(path), "rb") as w:
        return w.getframerate(), w.getnframes()


@needs_no_gpu
def test_separate_main_rate_pool_dry_run_and_refusals(tmp_path):
    import subprocess
    from tests.test_stream_pool_cpu import _write_wav
    exe = os.path.join(ROOT, "runtime", "separate_main")
    model = _export(tmp_path, joint=True, N=256)
    rng = np.random.default_rng(1)
    files = {"u8": (8000, 2001), "u48": (48000, 9613), "u16": (SR, 3203)}        # (rate, samples); enrollments at other rates again
    lines = []
    for key, (rate, n) in files.items():
        _write_wav(tmp_path / f"{key}.wav", rng.integers(-3000, 3000, n), sr=rate)
        _write_wav(tmp_path / f"{key}_e1.wav", rng.integers(-3000, 3000, 900), sr=SR)
        _write_wav(tmp_path / f"{key}_e2.wav", rng.integers(-3000, 3000, 600), sr=8000)
        lines.append(f"{key} {tmp_path}/{key}.wav {tmp_path}/{key}_e1.wav {tmp_path}/{key}_e2.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    out = tmp_path / "out"
    out.mkdir()
    run = lambda *a: subprocess.run([exe, "--wav_scp", str(scp), "--dry_run", "--model", model, "--output_dir", str(out), *a],
                                    capture_output=True, text=True, timeout=120)
    for extra in ([], ["--stream_block"]):
        r = run("--stream_ms", "10", "--rate_pool", "2", *extra)
        assert r.returncode == 0, r.stderr
        for key, (rate, n) in files.items():
            packet = rate // 100
            assert f"process: {key} RTF:" in r.stdout, r.stdout
            assert f"(rate pool of 2 lines: {-(-n // packet)} pushes of {packet} samples at {rate} Hz" in r.stdout, r.stdout
            for k in (1, 2):
                assert _wav_info(out / f"{key}-spk{k}.wav") == (rate, n), key     # the mixture's rate and length
        rounds, launches = (int(v) for v in r.stdout.split("rate pool: ")[1].split(" launches")[0].split(" rounds, "))
        assert rounds < sum(-(-n // (rate // 100)) for rate, n in files.values()) and launches > 0       # lines shared rounds
    r = run("--rate_pool", "2")
    assert r.returncode == 1 and "--rate_pool needs --stream_ms" in r.stderr
    r = run("--stream_ms", "10", "--rate_pool", "2", "--stream_pool", "2")
    assert r.returncode == 1 and "--rate_pool conflicts with --stream_pool" in r.stderr
    r = run("--stream_ms", "10", "--rate_pool", "2", "--batch", "2")
    assert r.returncode == 1 and "--rate_pool conflicts with --batch N > 1 and --chunk_seconds" in r.stderr
    r = run("--stream_ms", "10", "--rate_pool", "2", "--chunk_seconds", "0.2")
    assert r.returncode == 1 and "--rate_pool conflicts with --batch N > 1 and --chunk_seconds" in r.stderr
    r = run("--stream_ms", "10", "--rate_pool", "0")
    assert r.returncode == 1 and "--rate_pool needs a positive number of lines" in r.stderr
    # the old refusal is still there
    r = run("--resample", "--stream_ms", "10", "--stream_pool", "2")
    assert r.returncode == 1 and "--resample conflicts with --stream_pool" in r.stderr and "--rate_pool" in r.stderr
