"""CPU: causal cLN Conv-TasNet / SpEx+ containers and the streaming API of the native runtime (ws_engine_stream_*,
include/wesep_engine.h) on a dry-run engine and the real libraries: export and metadata, the whole-utterance plan through
argument validation, the emission rule for several chunkings, the launch count per group, every refusal of the header.
Nothing is computed in a dry run.  Without the feature the first step fails: the export raises."""
import numpy as np
import pytest
import torch

from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
KW = dict(N=256, L=20, B=64, H=128, P=3, X=3, R=2, spk_emb_dim=256)
S, LMAX, LWIN = 10, 160, 20
TOTAL = 12345
GROUP = 3 * KW["R"] * KW["X"] + 10          # WS_STREAM_GROUP_LAUNCHES(R, X)


def _export(tmp_path, joint, name="c.wsw", **kw):
    from wesep_amd.models import get_model
    m = get_model("ConvTasNet")(**dict(KW, joint_training=joint, causal=True, norm="cLN", **kw))
    path = str(tmp_path / name)
    export_engine(m, path)
    return path


def _enroll(joint, rows):
    if joint:
        return np.zeros((rows, 9000), np.float32), E.ENROLL_WAVE
    return np.zeros((rows, 256), np.float32), E.ENROLL_EMBEDDING


def _chunkings(total=TOTAL):
    rng = np.random.RandomState(7)
    rnd, left = [], total
    while left > 0:
        n = min(left, int(rng.randint(1, 4001)))
        rnd.append(n)
        left -= n
    even = lambda n: [n] * (total // n) + ([total % n] if total % n else [])
    return {"all160": even(160), "all7": even(7), "random1to4000": rnd, "one": [total]}


def _frames(n):
    return (n - LMAX) // S + 1 if n >= LMAX else 0


def test_header_states_the_launch_figure_and_the_sizing_formulas():
    import os
    import re
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "wesep_engine.h")).read()
    assert re.search(r"#define WS_STREAM_GROUP_LAUNCHES\(R, X\) \(3 \* \(R\) \* \(X\) \+ 10\)", header)
    assert re.search(r"#define WS_STREAM_PUSH_CAP\(n, L\) \(\(\(n\) / \(\(L\) / 2\) \+ 1\) \* \(\(L\) / 2\)\)", header)
    assert "#define WS_STREAM_FLUSH_CAP 160" in header and "#define WS_ENGINE_ABI_VERSION 2" in header
    assert GROUP <= 3 * KW["R"] * KW["X"] + 16
    for n in (1, 7, 9, 10, 11, 159, 160, 161, 4000):                  # the push bound covers the worst phase of the hop
        worst = max(_frames(N + n) - _frames(N) for N in range(0, 400)) * S
        assert worst <= E.stream_push_cap(n, LWIN)


def test_export_refusals_name_their_reason():
    from wesep_amd.models import get_model
    small = dict(N=32, L=20, B=32, H=64, P=3, X=2, R=1, joint_training=False)
    with pytest.raises(NotImplementedError, match="gLN only"):
        export_engine(get_model("ConvTasNet")(**small, norm="cLN"), "/dev/null")
    with pytest.raises(NotImplementedError, match="causal.*whole utterance"):
        export_engine(get_model("ConvTasNet")(**small, causal=True), "/dev/null")
    with pytest.raises(NotImplementedError, match="causal"):
        export_engine(get_model("ConvTasNet")(**small, causal=True, norm="BN"), "/dev/null")


@needs_no_gpu
@pytest.mark.parametrize("joint", [False, True], ids=["fixed-embeddings", "spex-plus"])
def test_causal_cln_container_loads_and_its_plans_validate(tmp_path, joint):
    eng = E.Engine(_export(tmp_path, joint), dry_run=True)
    assert eng.info("arch") == 1 and eng.info("causal") == 1 and eng.info("norm") == 1 and eng.info("streaming") == 1
    assert eng.info("N") == 256 and eng.info("L") == 20 and eng.info("joint_training") == int(joint)
    enroll, kind = _enroll(joint, 2)
    counts = set()
    for T in (16000, 12345, 160):
        est = eng.separate(np.ones((2, T), np.float32), enroll, kind)
        assert est.shape == (2, T) and not est.any()
        counts.add(eng.info("n_launches"))
    assert len(counts) == 1
    est = eng.separate_long(np.ones(20000, np.float32), enroll, kind, window=8000, overlap=1000, max_rows=4)
    assert est.shape == (2, 20000) and eng.info("long_windows") == 3
    st = eng.stream(2, enroll, kind, max_chunk_frames=64)
    assert eng.info("stream_state_bytes") > 0
    st.close()
    eng.close()


@needs_no_gpu
@pytest.mark.parametrize("chunking", sorted(_chunkings()))
def test_emission_rule_and_launch_count(tmp_path, chunking):
    eng = E.Engine(_export(tmp_path, False), dry_run=True)
    enroll, kind = _enroll(False, 2)
    G = 64
    st = eng.stream(2, enroll, kind, max_chunk_frames=G)
    state = eng.info("stream_state_bytes")
    x = np.zeros((2, TOTAL), np.float32)
    pos, emitted = 0, 0
    for n in _chunkings()[chunking]:
        before = _frames(pos)
        y = st.push(x[:, pos:pos + n])
        pos += n
        new = _frames(pos) - before
        assert y.shape == (2, new * S), (pos, n, y.shape)
        emitted += y.shape[1]
        assert emitted == _frames(pos) * S
        groups = eng.info("n_launches") // GROUP
        assert eng.info("n_launches") == groups * GROUP and (groups == 0) == (new == 0)
        if 0 < new <= G and n <= G * S:                                 # one group: the header's figure, whatever n is
            assert groups == 1, (n, new, groups)
        assert groups >= -(-new // G)
    Tp = (TOTAL - LWIN) // S + 1
    tail = st.flush()
    assert emitted + tail.shape[1] == (Tp - 1) * S + LWIN
    assert tail.shape[1] <= E.STREAM_FLUSH_CAP
    assert eng.info("stream_state_bytes") == state                     # the state does not grow with the pushes
    st.close()
    eng.close()


@needs_no_gpu
def test_one_group_pushes_cost_the_same_for_every_chunk_size(tmp_path):
    eng = E.Engine(_export(tmp_path, True), dry_run=True)
    enroll, kind = _enroll(True, 1)
    seen = set()
    for n in (10, 40, 160, 640):
        st = eng.stream(1, enroll, kind, max_chunk_frames=64)
        st.push(np.zeros((1, 160), np.float32))                         # the first frame
        assert eng.info("n_launches") == GROUP
        st.push(np.zeros((1, n), np.float32))
        seen.add(eng.info("n_launches"))
        st.close()
    assert seen == {GROUP}
    eng.close()


@needs_no_gpu
def test_refusals(tmp_path):
    from wesep_amd.models import get_model
    # a gLN container loads and separates, and cannot stream
    gpath = str(tmp_path / "g.wsw")
    export_engine(get_model("ConvTasNet")(**dict(KW, joint_training=False)), gpath)
    geng = E.Engine(gpath, dry_run=True)
    assert geng.info("streaming") == 0 and geng.info("causal") == 0 and geng.info("norm") == 0
    with pytest.raises(E.WesepHipError, match="non-causal with gLN; streaming needs causal blocks with cLN"):
        geng.stream(2, np.zeros((2, 256), np.float32), E.ENROLL_EMBEDDING)
    geng.close()
    eng = E.Engine(_export(tmp_path, False), dry_run=True)
    emb = np.zeros((2, 256), np.float32)
    with pytest.raises(E.WesepHipError, match="takes fixed embeddings"):                 # a wrong enrollment kind
        eng.stream(2, np.zeros((2, 9000), np.float32), E.ENROLL_WAVE)
    with pytest.raises(E.WesepHipError, match="bad arguments"):
        eng.stream(2, emb, E.ENROLL_EMBEDDING, max_chunk_frames=0)
    st = eng.stream(2, emb, E.ENROLL_EMBEDDING, max_chunk_frames=16)
    x = np.zeros((2, 400), np.float32)
    with pytest.raises(E.WesepHipError, match="fewer than the encoder window L = 20"):   # flush before L samples
        st.flush()
    st.push(x[:, :19])
    with pytest.raises(E.WesepHipError, match="19 samples were pushed"):
        st.flush()
    with pytest.raises(E.WesepHipError, match="emits 260 samples a row, est_cap is 259"):  # 419 samples: 26 frames
        st.push(x, est_cap=259)
    y = st.push(x, est_cap=260)                                          # the refused push left the stream as it was
    assert y.shape == (2, 260)
    with pytest.raises(E.WesepHipError, match="emits"):
        st.flush(est_cap=5)
    assert st.flush().shape[1] == ((419 - 20) // 10) * 10 + 20 - 260
    with pytest.raises(E.WesepHipError, match="the stream was flushed"):                 # push after flush
        st.push(x)
    with pytest.raises(E.WesepHipError, match="flushed already"):
        st.flush()
    st.reset()
    assert st.push(x[:, :170]).shape == (2, 20)
    with pytest.raises(ValueError, match="expected"):
        st.push(x[:1])
    st.close()
    eng.close()


@needs_no_gpu
def test_separate_between_pushes_and_two_streams(tmp_path):
    eng = E.Engine(_export(tmp_path, False), dry_run=True)
    emb = np.zeros((2, 256), np.float32)
    a = eng.stream(2, emb, E.ENROLL_EMBEDDING, max_chunk_frames=8)
    b = eng.stream(2, emb, E.ENROLL_EMBEDDING, max_chunk_frames=32)
    x = np.zeros((2, 1000), np.float32)
    assert a.push(x[:, :500]).shape == (2, 350)
    eng.separate(np.ones((2, 16000), np.float32), emb, E.ENROLL_EMBEDDING)
    eng.separate_long(np.ones(20000, np.float32), emb, E.ENROLL_EMBEDDING, window=8000, overlap=1000, max_rows=4)
    assert b.push(x[:, :165]).shape == (2, 10)
    assert a.push(x[:, 500:]).shape == (2, 500)
    assert eng.info("n_launches") % GROUP == 0 and eng.info("n_launches") >= GROUP * -(-50 // 8)    # 50 frames, 8 a group
    assert a.flush().shape == (2, 1000 - 850) and b.flush().shape[1] == ((165 - 20) // 10) * 10 + 20 - 10
    a.close()
    b.close()
    eng.close()


def _write_wav(path, x, sr=16000):
    import wave
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


@needs_no_gpu
def test_separate_main_stream_ms_dry_run_and_refusals(tmp_path):
    import os
    import subprocess
    from wesep_amd.models import get_model
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "runtime", "separate_main")
    model = _export(tmp_path, True)
    rng = np.random.default_rng(1)
    for name, n in (("mix", 8000), ("e1", 9000), ("e2", 9500)):
        _write_wav(tmp_path / f"{name}.wav", rng.integers(-3000, 3000, n))
    scp = tmp_path / "wav.scp"
    scp.write_text(f"utt1 {tmp_path}/mix.wav {tmp_path}/e1.wav {tmp_path}/e2.wav\n")
    run = lambda *a: subprocess.run([exe, "--wav_scp", str(scp), "--dry_run", *a], capture_output=True, text=True, timeout=120)
    r = run("--model", model, "--stream_ms", "10")
    assert r.returncode == 0, r.stderr
    # 8000 samples in 50 pushes of 160; the first completes 1 frame, every later one 16: one group each
    assert f"process: utt1" in r.stdout and f"(50 pushes of 160 samples, {(50 + 1) * GROUP} launches" in r.stdout
    r = run("--model", model, "--stream_ms", "10", "--batch", "2")
    assert r.returncode == 1 and "--stream_ms conflicts with --batch" in r.stderr
    r = run("--model", model, "--stream_ms", "10", "--chunk_seconds", "1")
    assert r.returncode == 1 and "--stream_ms conflicts" in r.stderr
    r = run("--model", model, "--stream_ms", "0")
    assert r.returncode == 1 and "positive chunk length" in r.stderr
    gln = str(tmp_path / "g.wsw")
    export_engine(get_model("ConvTasNet")(**dict(KW, joint_training=True)), gln)
    r = run("--model", gln, "--stream_ms", "10")
    assert r.returncode == 1 and "this model cannot stream" in r.stderr
