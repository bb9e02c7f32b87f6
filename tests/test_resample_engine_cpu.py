"""CPU: audio at the caller's sample rate through the engine's dry run (no GPU): ws_engine_resample, ws_engine_separate_rate
on a small container of every architecture (launch figures and refusals), the rate stream's emission rule, push_cap, launch
figures and state size, and `separate_main --resample --dry_run`.  Without the feature every test fails (no symbol)."""
import os
import subprocess
import wave

import numpy as np
import pytest

from tests import resample_contract as RC
from tests.test_longform_host_cpu import ARCHS, _container
from tests.test_stream_pool_cpu import KW, _export, _write_wav, needs_no_gpu
from wesep_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RX, L, S = KW["R"] * KW["X"], KW["L"], KW["L"] // 2
EMB2 = np.zeros((2, 256), np.float32)


@needs_no_gpu
def test_engine_resample_dry_run_and_refusals(tmp_path):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    for pair in RC.PAIRS:
        y = eng.resample(np.zeros((3, 1999), np.float32), *pair)
        assert y.shape == (3, RC.out_len(1999, *pair)) and eng.info("n_launches") == 1
    with pytest.raises(E.WesepHipError, match="ws_engine_resample: ws_resample_geom: rate_in=0 and rate_out=16000 must be positive"):
        eng.resample(np.zeros((1, 10), np.float32), 0, 16000)
    with pytest.raises(E.WesepHipError, match="ws_engine_resample: ws_resample_geom: 16000 -> 16001 reduces to U=16001, D=16000"):
        eng.resample(np.zeros((1, 10), np.float32), 16000, 16001)
    x, y, m = np.zeros((1, 100), np.float32), np.zeros((1, 199), np.float32), E.C.c_int(0)
    assert E.lib().ws_engine_resample(eng._h, x.ctypes.data, 1, 100, 8000, 16000, y.ctypes.data, 199, E.C.byref(m)) == -1
    assert "ws_engine_resample: 100 samples at 8000 Hz are 200 samples a row at 16000 Hz, y_cap is 199" in E.lib().ws_engine_last_error().decode()
    assert E.lib().ws_engine_resample(eng._h, None, 1, 100, 8000, 16000, y.ctypes.data, 199, E.C.byref(m)) == -1
    assert "ws_engine_resample: x, y or n_out is NULL" in E.lib().ws_engine_last_error().decode()
    eng.close()


def _text(exc):
    return str(exc.value).split("): ", 1)[1]


@needs_no_gpu
@pytest.mark.parametrize("arch", list(ARCHS))
def test_separate_rate_launches_and_refusals(tmp_path, arch):
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    T = ARCHS[arch][2]
    wave16 = np.zeros((2, 16000), np.float32)
    eng.separate(np.zeros((2, T), np.float32), wave16, E.ENROLL_WAVE)
    plain = eng.info("n_launches")
    assert plain > 0
    # at the model's rate it IS ws_engine_separate
    assert eng.separate_rate(np.zeros((2, T), np.float32), wave16, E.ENROLL_WAVE, 16000).shape == (2, T)
    assert eng.info("n_launches") == plain
    eng.separate_rate(np.zeros((2, T), np.float32), wave16, E.ENROLL_WAVE, 16000, enroll_rate=16000)
    assert eng.info("n_launches") == plain
    # 8 kHz and 48 kHz mixtures of the same duration; the enrollment at the model's rate, then at 8 kHz
    for rate in (8000, 48000):
        Tr = T * rate // 16000
        assert RC.out_len(Tr, rate, 16000) == T
        est = eng.separate_rate(np.zeros((2, Tr), np.float32), wave16, E.ENROLL_WAVE, rate)
        assert est.shape == (2, Tr) and eng.info("n_launches") == plain + E.separate_rate_launches(True, False) == plain + 2
        eng.separate_rate(np.zeros((2, Tr), np.float32), np.zeros((2, 8000), np.float32), E.ENROLL_WAVE, rate, enroll_rate=8000)
        assert eng.info("n_launches") == plain + E.separate_rate_launches(True, True) == plain + 3
    eng.separate_rate(np.zeros((2, T), np.float32), np.zeros((2, 8000), np.float32), E.ENROLL_WAVE, 16000, enroll_rate=8000)
    assert eng.info("n_launches") == plain + E.separate_rate_launches(False, True) == plain + 1
    # refusals, by name, before any launch
    with pytest.raises(E.WesepHipError, match=r"ws_engine_separate_rate: enroll_rate=8000 with enrollment kind 1: only a waveform enrollment"):
        eng.separate_rate(np.zeros((2, T), np.float32), np.zeros((2, 100, 80), np.float32), E.ENROLL_FBANK, 8000, enroll_rate=8000)
    with pytest.raises(E.WesepHipError, match="ws_engine_separate_rate: ws_resample_geom: 16001 -> 16000 reduces to U=16000, D=16001"):
        eng.separate_rate(np.zeros((2, T), np.float32), wave16, E.ENROLL_WAVE, 16001)
    with pytest.raises(E.WesepHipError, match="ws_engine_separate_rate: ws_resample_geom: rate_in=-1"):
        eng.separate_rate(np.zeros((2, T), np.float32), wave16, E.ENROLL_WAVE, -1)
    with pytest.raises(E.WesepHipError, match="ws_engine_separate_rate: ws_resample_geom: 7 -> 16000 reduces to U=16000, D=7"):
        eng.separate_rate(np.zeros((2, T), np.float32), np.zeros((2, 100), np.float32), E.ENROLL_WAVE, 16000, enroll_rate=7)
    # a T whose resampled length is below the architecture's minimum: the architecture's own message
    short = 8 if arch == "ConvTasNet" else 100
    with pytest.raises(E.WesepHipError) as own:
        eng.separate(np.zeros((2, 2 * short), np.float32), wave16, E.ENROLL_WAVE)
    with pytest.raises(E.WesepHipError) as rated:
        eng.separate_rate(np.zeros((2, short), np.float32), wave16, E.ENROLL_WAVE, 8000)
    assert _text(rated) == _text(own) and "ws_engine_separate" in _text(own)
    eng.close()


def _chunkings(n, seed):
    rng = np.random.default_rng(seed)
    rnd, left = [], n
    while left:
        c = int(min(left, rng.integers(1, 4001)))
        rnd.append(c)
        left -= c
    cut = lambda k: [k] * (n // k) + ([n % k] if n % k else [])
    return {"all160": cut(160), "all7": cut(7), "random": rnd, "one": [n]}


@needs_no_gpu
@pytest.mark.parametrize("rate,n", [(8000, 2003), (48000, 9001)])
def test_rate_stream_emission_rule(tmp_path, rate, n):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    for name, chunks in _chunkings(n, rate).items():
        st = eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, rate, max_chunk_frames=64, max_push=1000)
        state = eng.info("stream_state_bytes")
        assert state > 0
        seen = total = 0
        for c in chunks:
            out = st.push(np.zeros((2, c), np.float32))
            seen += c
            want = RC.rate_stream_emitted(seen, rate, 16000, L) - RC.rate_stream_emitted(seen - c, rate, 16000, L)
            assert out.shape == (2, want), (name, seen, c)
            assert want <= st.push_cap(c)
            total += want
            assert eng.info("stream_state_bytes") == state
        out = st.flush()
        total += out.shape[1]
        assert out.shape[1] <= st.push_cap(0)
        assert total == RC.rate_stream_total(n, rate, 16000, L) <= n, (name, total)
        with pytest.raises(E.WesepHipError, match="ws_engine_rate_stream_push: the stream was flushed"):
            st.push(np.zeros((2, 10), np.float32))
        st.reset()
        assert st.push(np.zeros((2, 7), np.float32)).shape == (2, 0)
        st.close()
    eng.close()


@needs_no_gpu
@pytest.mark.parametrize("rate,n", [(8000, 80), (48000, 480), (8000, 7), (48000, 1601)])
def test_push_cap_is_never_exceeded_over_every_start_phase(tmp_path, rate, n):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    U, D, _, _ = RC.geometry(rate, 16000)
    st = eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, rate, max_push=600)
    cap = st.push_cap(n)
    worst = 0
    for phase in range(0, 3 * max(D, U) * S):
        st.reset()
        seen = 700 * rate // 16000 + phase                   # past the start-up of the three stages
        st.push(np.zeros((2, seen), np.float32))
        for _ in range(3):
            m = st.push(np.zeros((2, n), np.float32)).shape[1]
            seen += n
            assert m <= cap, (phase, seen, m, cap)
            worst = max(worst, m)
    print(f"rate {rate}, pushes of {n}: at most {worst} samples returned, push_cap {cap}")
    assert worst > 0 or n < 10
    st.close()
    eng.close()


@needs_no_gpu
@pytest.mark.parametrize("block_kernel", [False, True])
def test_rate_stream_launches_state_and_refusals(tmp_path, block_kernel):
    eng = E.Engine(_export(tmp_path), dry_run=True)
    group = (RX + 10) if block_kernel else (3 * RX + 10)
    plain = eng.stream(2, EMB2, E.ENROLL_EMBEDDING, max_chunk_frames=64, block_kernel=block_kernel)
    plain_state = eng.info("stream_state_bytes")
    plain.push(np.zeros((2, 400), np.float32))
    plain.push(np.zeros((2, 160), np.float32))
    assert eng.info("n_launches") == group                   # 16 frames, one group
    plain.close()
    for rate, n in ((8000, 80), (48000, 480)):
        st = eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, rate, max_chunk_frames=64, max_push=n, block_kernel=block_kernel)
        state = eng.info("stream_state_bytes")
        assert state > plain_state
        for _ in range(8):                                   # past the start: every push then hands A, the stream and B samples
            st.push(np.zeros((2, n), np.float32))
        for _ in range(3):
            out = st.push(np.zeros((2, n), np.float32))
            assert out.shape[1] > 0
            assert eng.info("n_launches") == group + E.RATE_STREAM_PIECE_LAUNCHES == group + 2
            assert eng.info("stream_state_bytes") == state
        st.push(np.zeros((2, 3 * n), np.float32))            # above max_push: three pieces
        assert eng.info("n_launches") == 3 * (group + 2)
        with pytest.raises(E.WesepHipError, match="ws_engine_rate_stream_push: this push emits"):
            st.push(np.zeros((2, n), np.float32), est_cap=1)
        st.close()
    # at the container's rate a rate stream is the plain stream
    st = eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, 16000, max_chunk_frames=64, block_kernel=block_kernel)
    assert eng.info("stream_state_bytes") == plain_state
    st.push(np.zeros((2, 400), np.float32))
    assert st.push(np.zeros((2, 160), np.float32)).shape == (2, 160) and eng.info("n_launches") == group
    assert st.push_cap(333) == E.stream_push_cap(333, L) and st.push_cap(0) == E.STREAM_FLUSH_CAP
    st.close()
    # refusals
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_stream_open: enroll_rate=8000 with enrollment kind 0"):
        eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, 8000, enroll_rate=8000)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_stream_open: ws_resample_geom: 16001 -> 16000 reduces to"):
        eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, 16001)
    with pytest.raises(E.WesepHipError, match=r"ws_engine_rate_stream_open: bad arguments \(rows=2, max_push=0"):
        eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, 8000, max_push=0)
    h = E.C.c_void_p()
    assert E.lib().ws_engine_rate_stream_open(eng._h, 2, EMB2.ctypes.data, E.ENROLL_EMBEDDING, 0, 0, 64, 6, 8000, 100, E.C.byref(h)) == -1
    assert "ws_engine_stream_open_ex: unknown flag bits 0x6 (known: WS_STREAM_BLOCK_KERNEL = 1)" in E.lib().ws_engine_last_error().decode()
    st = eng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, 8000)
    st.push(np.zeros((2, 5), np.float32))
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_stream_flush: 5 samples were pushed, 10 at the container's rate, fewer than"):
        st.flush()
    st.close()
    eng.close()
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    gpath = str(tmp_path / "g.wsw")
    export_engine(get_model("ConvTasNet")(**dict(KW, joint_training=False)), gpath)
    geng = E.Engine(gpath, dry_run=True)
    with pytest.raises(E.WesepHipError, match="ws_engine_rate_stream_open: this Conv-TasNet container is non-causal with gLN"):
        geng.rate_stream(2, EMB2, E.ENROLL_EMBEDDING, 8000)
    geng.close()


def _wav_info(path):
    with wave.open(str(path), "rb") as w:
        return w.getframerate(), w.getnframes()


@needs_no_gpu
def test_separate_main_resample_dry_run(tmp_path):
    exe = os.path.join(ROOT, "runtime", "separate_main")
    stream_model = _export(tmp_path, joint=True, N=256)
    batch_model = _container(tmp_path, "pBSRNN")
    rng = np.random.default_rng(1)
    files = {"u8": (8000, 4001), "u44": (44100, 11025)}          # (rate, samples); enrollments at other rates again
    lines = []
    for key, (rate, n) in files.items():
        _write_wav(tmp_path / f"{key}.wav", rng.integers(-3000, 3000, n), sr=rate)
        _write_wav(tmp_path / f"{key}_e1.wav", rng.integers(-3000, 3000, 9000), sr=8000)
        _write_wav(tmp_path / f"{key}_e2.wav", rng.integers(-3000, 3000, 22050), sr=22050)
        lines.append(f"{key} {tmp_path}/{key}.wav {tmp_path}/{key}_e1.wav {tmp_path}/{key}_e2.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))

    def run(model, out, *a):
        os.makedirs(out, exist_ok=True)
        return subprocess.run([exe, "--wav_scp", str(scp), "--dry_run", "--model", model, "--output_dir", str(out), *a],
                              capture_output=True, text=True, timeout=300)

    modes = {"plain": (batch_model, []), "batch": (batch_model, ["--batch", "2"]), "chunk": (batch_model, ["--chunk_seconds", "0.2"]),
             "stream": (stream_model, ["--stream_ms", "10"]), "stream_block": (stream_model, ["--stream_ms", "10", "--stream_block"]),
             "plain_tasnet": (stream_model, [])}
    for name, (model, extra) in modes.items():
        out = tmp_path / f"out_{name}"
        r = run(model, out, "--resample", *extra)
        assert r.returncode == 0, (name, r.stderr)
        for key, (rate, n) in files.items():
            assert f"process: {key} RTF:" in r.stdout, (name, r.stdout)
            for k in (1, 2):
                assert _wav_info(out / f"{key}-spk{k}.wav") == (rate, n), (name, key)
        if name.startswith("stream"):
            assert f"({-(-4001 // 80)} pushes of 80 samples" in r.stdout and f"({-(-11025 // 441)} pushes of 441 samples" in r.stdout, r.stdout
    # without --resample: the old error, nothing written
    r = run(batch_model, tmp_path / "out_none")
    assert r.returncode == 1 and "sample rate is not 16000" in r.stderr
    assert not os.listdir(tmp_path / "out_none")
    r = run(stream_model, tmp_path / "out_none", "--stream_ms", "10")
    assert r.returncode == 1 and "sample rate is not 16000" in r.stderr
    # the pool is not rate-aware
    r = run(stream_model, tmp_path / "out_none", "--resample", "--stream_ms", "10", "--stream_pool", "2")
    assert r.returncode == 1 and "--resample conflicts with --stream_pool" in r.stderr


@needs_no_gpu
def test_separate_rate_holds_one_turn_under_serialize(tmp_path):
    """WS_ENGINE_SERIALIZE=1: ws_engine_separate_rate holds the device's turn over its three steps and ws_engine_separate's own
    turn nests in it (the same thread does not lock twice); the launch figure is the same as without the lock."""
    import sys
    path = _container(tmp_path, "pBSRNN")
    code = ("import numpy as np\n"
            "from wesep_amd import engine as E\n"
            f"eng = E.Engine({path!r}, dry_run=True)\n"
            "w = np.zeros((2, 16000), np.float32)\n"
            "eng.separate(np.zeros((2, 2048), np.float32), w, E.ENROLL_WAVE)\n"
            "plain = eng.info('n_launches')\n"
            "eng.separate_rate(np.zeros((2, 1024), np.float32), np.zeros((2, 8000), np.float32), E.ENROLL_WAVE, 8000, enroll_rate=8000)\n"
            "assert eng.info('n_launches') == plain + 3, (eng.info('n_launches'), plain)\n"
            "st_ok = eng.separate(np.zeros((2, 2048), np.float32), w, E.ENROLL_WAVE)\n"          # the lock was released
            "print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, cwd=ROOT,
                       env=dict(os.environ, WS_ENGINE_SERIALIZE="1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr
