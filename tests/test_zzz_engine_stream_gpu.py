"""GPU: causal cLN Conv-TasNet / SpEx+ in the native runtime -- the whole-utterance plan (runtime/tasnet_plan.cc) and the
streaming API (runtime/stream.cc) against the Python model's forward on the same device, whose causal blocks and cLN are
pinned to the reference's fixtures.  rel < 1e-4: the bound tests/test_zzz_engine_separators_gpu.py holds an engine plan to.
The engines are created with WS_ENGINE_POISON=1: every arena allocation and the stream's state start as NaN, so a plan that
reads memory no launch has written shows up as a non-finite output.  Measured values are printed
(profiles/engine_stream.md records them)."""
import os
import subprocess
import wave

import numpy as np
import pytest
import torch

from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, T, S, LWIN = 2, 1603, 10, 20
T_OUT = ((T - LWIN) // S) * S + LWIN
_CASES = {}


def _chunkings(total=T):
    g = torch.Generator().manual_seed(11)
    rnd, left = [], total
    while left > 0:
        n = min(left, int(torch.randint(1, 401, (1,), generator=g)))
        rnd.append(n)
        left -= n
    even = lambda n: [n] * (total // n) + ([total % n] if total % n else [])
    return {"all160": even(160), "all7": even(7), "random1to400": rnd, "one": [total]}


def _case(joint, tmp_path_factory):
    """(engine, Python forward [ROWS, T_OUT], Engine.separate's rows, mixture, enrollment, kind): made once per container."""
    if joint in _CASES:
        return _CASES[joint]
    from tests.test_engine_gpu import _cuda
    from wesep_amd.models import get_model
    d = _cuda()
    torch.manual_seed(17 + int(joint))
    model = get_model("ConvTasNet")(N=256 if joint else 32, L=20, B=32, H=64, P=3, X=3, R=2, spk_emb_dim=256, causal=True,
                                    norm="cLN", joint_training=joint)
    path = str(tmp_path_factory.mktemp("stream") / "c.wsw")
    export_engine(model, path)
    os.environ["WS_ENGINE_POISON"] = "1"
    try:
        eng = E.Engine(path)
    finally:
        del os.environ["WS_ENGINE_POISON"]
    model = model.to(d).eval()
    g = torch.Generator().manual_seed(5)
    x = 0.1 * torch.randn(ROWS, T, generator=g)
    if joint:
        enroll, kind = 0.1 * torch.randn(ROWS, 900, generator=g), E.ENROLL_WAVE
    else:
        enroll, kind = torch.randn(ROWS, 256, generator=g), E.ENROLL_EMBEDDING
    with torch.no_grad():
        ref = model(x.to(d), enroll.to(d))[0].cpu()
    sep = eng.separate(x.numpy(), enroll.numpy(), kind)
    _CASES[joint] = (eng, ref, sep, x.numpy(), enroll.numpy(), kind)
    return _CASES[joint]


def _rel(a, b):
    from tests.test_engine_gpu import rel
    return rel(a, b)


def _run(st, x, sizes):
    outs, pos = [], 0
    for n in sizes:
        outs.append(st.push(x[:, pos:pos + n]))
        pos += n
        assert sum(o.shape[1] for o in outs) == (max(0, (pos - 160) // S + 1) * S if pos >= 160 else 0)
    outs.append(st.flush())
    return np.concatenate(outs, 1)


@pytest.mark.parametrize("joint", [False, True], ids=["fixed-embeddings", "spex-plus"])
def test_whole_utterance_plan_matches_python_model(joint, tmp_path_factory):
    eng, ref, sep, x, enroll, kind = _case(joint, tmp_path_factory)
    assert eng.info("causal") == 1 and eng.info("norm") == 1 and eng.info("streaming") == 1
    assert ref.shape == (ROWS, T_OUT) and sep.shape == (ROWS, T) and np.isfinite(sep).all() and float(ref.abs().max()) > 0
    assert not sep[:, T_OUT:].any()
    e = _rel(sep[:, :T_OUT], ref)
    print(f"engine causal cLN separate joint={joint}: rel L2 vs Python forward {e:.3e}")
    assert e < 1e-4
    long = eng.separate_long(x[0], enroll, kind, window=800, overlap=200, max_rows=4)
    assert long.shape == (ROWS, T) and np.isfinite(long).all()


@pytest.mark.parametrize("chunking", sorted(_chunkings()))
@pytest.mark.parametrize("joint", [False, True], ids=["fixed-embeddings", "spex-plus"])
def test_stream_matches_separate_and_python_model(joint, chunking, tmp_path_factory):
    eng, ref, sep, x, enroll, kind = _case(joint, tmp_path_factory)
    st = eng.stream(ROWS, enroll, kind, max_chunk_frames=16)
    got = _run(st, x, _chunkings()[chunking])
    groups = eng.info("n_launches")
    st.close()
    assert got.shape == (ROWS, T_OUT) and np.isfinite(got).all()
    e1, e2 = _rel(got, sep[:, :T_OUT]), _rel(got, ref)
    print(f"engine stream joint={joint} {chunking}: rel L2 vs Engine.separate {e1:.3e}, vs Python forward {e2:.3e}")
    assert e1 < 1e-4 and e2 < 1e-4
    assert groups % (3 * 2 * 3 + 10) == 0


@pytest.mark.parametrize("joint", [False, True], ids=["fixed-embeddings", "spex-plus"])
def test_reset_reproduces_the_outputs_bit_for_bit(joint, tmp_path_factory):
    eng, ref, sep, x, enroll, kind = _case(joint, tmp_path_factory)
    st = eng.stream(ROWS, enroll, kind, max_chunk_frames=16)
    a = _run(st, x, _chunkings()["random1to400"])
    st.reset()
    b = _run(st, x, _chunkings()["random1to400"])
    st.close()
    assert np.array_equal(a, b) and np.isfinite(a).all()


def test_two_interleaved_streams_give_what_each_gives_alone(tmp_path_factory):
    eng, ref, sep, x, enroll, kind = _case(False, tmp_path_factory)
    other = np.ascontiguousarray(enroll[::-1] * 0.5 + 0.1)
    y = np.ascontiguousarray(x[::-1] * 0.7)
    sizes = _chunkings()["random1to400"]
    alone = []
    for xx, en, G in ((x, enroll, 16), (y, other, 32)):
        st = eng.stream(ROWS, en, kind, max_chunk_frames=G)
        alone.append(_run(st, xx, sizes))
        st.close()
    assert not np.array_equal(alone[0], alone[1])
    sa, sb = eng.stream(ROWS, enroll, kind, max_chunk_frames=16), eng.stream(ROWS, other, kind, max_chunk_frames=32)
    oa, ob, pos = [], [], 0
    for i, n in enumerate(sizes):
        oa.append(sa.push(x[:, pos:pos + n]))
        if i == 2:                                                       # another engine call between two pushes
            eng.separate(x, enroll, kind)
        ob.append(sb.push(y[:, pos:pos + n]))
        pos += n
    oa.append(sa.flush())
    ob.append(sb.flush())
    sa.close()
    sb.close()
    assert np.array_equal(np.concatenate(oa, 1), alone[0])
    assert np.array_equal(np.concatenate(ob, 1), alone[1])


def _write_wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


def test_separate_main_stream_ms_matches_the_plain_run(tmp_path):
    from tests.test_engine_gpu import _cuda
    from wesep_amd.models import get_model
    _cuda()
    torch.manual_seed(23)
    model = get_model("ConvTasNet")(N=256, L=20, B=32, H=64, P=3, X=3, R=2, spk_emb_dim=256, causal=True, norm="cLN",
                                    joint_training=True)
    path = str(tmp_path / "c.wsw")
    export_engine(model, path)
    rng = np.random.default_rng(3)
    lines = []
    for key, n in (("a", 3203), ("b", 1600)):
        _write_wav(tmp_path / f"{key}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"{key}_e1.wav", rng.integers(-3000, 3000, 900))
        _write_wav(tmp_path / f"{key}_e2.wav", rng.integers(-3000, 3000, 1000))
        lines.append(f"{key} {tmp_path}/{key}.wav {tmp_path}/{key}_e1.wav {tmp_path}/{key}_e2.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    exe = os.path.join(ROOT, "runtime", "separate_main")
    outs = {}
    for tag, extra in (("plain", []), ("stream", ["--stream_ms", "10"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = {f: np.fromfile(out / f, dtype=np.float32) for f in sorted(os.listdir(out)) if f.endswith(".f32")}
        assert sorted(os.listdir(out)) == sorted(f"{k}-spk{i}.{ext}" for k in "ab" for i in (1, 2) for ext in ("wav", "f32"))
    for f, plain in outs["plain"].items():
        got = outs["stream"][f]
        assert got.shape == plain.shape and np.isfinite(got).all() and float(np.abs(plain).max()) > 0
        e = _rel(got, plain)
        print(f"separate_main --stream_ms 10 {f}: rel L2 vs the plain run {e:.3e}")
        assert e < 1e-4
