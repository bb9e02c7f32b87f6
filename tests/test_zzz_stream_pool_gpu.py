"""GPU: the stream pool of the native runtime (runtime/stream_pool.cc, ws_engine_pool_*) -- a three-slot schedule with a
late attach, unequal packets (one slot pushes 10 ms while another pushes 250 ms), a flush in the middle of the run and a
detach followed by a re-attach of the same slot with another enrollment.  Every slot's concatenated output is compared with
a solo `Engine.stream(1, ...)` fed the same packets and with `Engine.separate` on the whole signal: rel < 1e-4, the bound
tests/test_zzz_engine_stream_gpu.py holds stream-vs-separate to (the measured worst case is printed, and whether the pool
is bit-identical to the solo stream -- not asserted there: the GEMMs see another M).

Asserted bit for bit, because the launch shapes are identical: the same schedule twice; the same schedule with the OTHER
slots' audio replaced by other data and by inf / NaN packets (isolation); a pool with one attached slot against a solo
rows = 1 stream with the same max_chunk_frames and packets.  The engine is created with WS_ENGINE_POISON=1: every arena
allocation and the pool's state start as NaN, so state no launch has written would show up in an output."""
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
S, LWIN, G = 10, 20, 4
_CASES = {}

# key -> samples; packets per key, in push order (160 = 10 ms, 4000 = 250 ms at 16 kHz)
LENGTHS = {"a": 1603, "b": 4571, "c": 977, "d": 700}
PACKETS = {"a": [160] * 10 + [3], "b": [7, 160, 4000, 1, 333, 60, 10], "c": [333, 160, 1, 160, 323], "d": [160, 7, 160, 373]}
# the rounds: "a" and "b" start together, "c" attaches late, "a" is flushed in the middle of the run, its slot is detached
# and re-attached to "d" (another enrollment) while "b" and "c" are in mid-stream
SCHEDULE = [("attach", "a"), ("attach", "b"), ("push", "a", "b"), ("push", "b", "a"), ("attach", "c"), ("push", "a", "b", "c"),
            ("push", "c", "a"), ("push", "a"), ("push", "a", "b"), ("push", "a"), ("push", "a", "c"), ("push", "a"), ("push", "a"),
            ("push", "a", "b"), ("flush", "a"), ("detach", "a"), ("attach", "d"), ("push", "d", "c", "b"), ("push", "d"),
            ("push", "c", "d"), ("push", "d", "b"), ("flush", "c"), ("flush", "b"), ("flush", "d")]


def t_out(n):
    return ((n - LWIN) // S) * S + LWIN


def _engine(joint, tmp_path_factory):
    """(engine, signals, enrollments, kind): made once per container."""
    if joint in _CASES:
        return _CASES[joint]
    from tests.test_engine_gpu import _cuda
    from wesep_amd.models import get_model
    _cuda()
    torch.manual_seed(29 + int(joint))
    model = get_model("ConvTasNet")(N=256 if joint else 32, L=20, B=32, H=64, P=3, X=3, R=2, spk_emb_dim=256, causal=True,
                                    norm="cLN", joint_training=joint)
    path = str(tmp_path_factory.mktemp("pool") / "c.wsw")
    export_engine(model, path)
    os.environ["WS_ENGINE_POISON"] = "1"
    try:
        eng = E.Engine(path)
    finally:
        del os.environ["WS_ENGINE_POISON"]
    g = torch.Generator().manual_seed(7)
    x = {k: (0.1 * torch.randn(n, generator=g)).numpy() for k, n in LENGTHS.items()}
    if joint:
        enroll, kind = {k: (0.1 * torch.randn(900, generator=g)).numpy() for k in LENGTHS}, E.ENROLL_WAVE
    else:
        enroll, kind = {k: torch.randn(256, generator=g).numpy() for k in LENGTHS}, E.ENROLL_EMBEDDING
    _CASES[joint] = (eng, x, enroll, kind)
    return _CASES[joint]


def _rel(a, b):
    from tests.test_engine_gpu import rel
    return rel(a, b)


def run_schedule(eng, x, enroll, kind, schedule=SCHEDULE, packets=PACKETS, slots=3):
    """{key: the concatenation of what the key's pushes and its flush returned}"""
    pool = eng.stream_pool(slots, max_chunk_frames=G)
    state = eng.info("stream_state_bytes")
    slot, pos, nxt, out = {}, {}, {}, {}
    for ev, *keys in schedule:
        if ev == "attach":
            k = keys[0]
            slot[k], pos[k], nxt[k], out[k] = pool.attach(enroll[k], kind), 0, 0, []
        elif ev == "push":
            chunks = {}
            for k in keys:
                n = packets[k][nxt[k]]
                chunks[slot[k]] = x[k][pos[k]:pos[k] + n]
                pos[k], nxt[k] = pos[k] + n, nxt[k] + 1
            got = pool.push(chunks)
            assert eng.info("n_launches") % E.pool_group_launches(2, 3) == 0
            for k in keys:
                out[k].append(got[slot[k]])
                assert sum(o.shape[0] for o in out[k]) == (max(0, (pos[k] - 160) // S + 1) * S if pos[k] >= 160 else 0)
        elif ev == "flush":
            out[keys[0]].append(pool.flush(slot[keys[0]]))
        else:
            pool.detach(slot[keys[0]])
    assert eng.info("stream_state_bytes") == state
    pool.close()
    assert all(nxt[k] == len(packets[k]) and pos[k] == x[k].shape[0] for k in out)
    return {k: np.concatenate(v) for k, v in out.items()}


def _solo(eng, xk, ek, kind, sizes):
    st = eng.stream(1, ek[None], kind, max_chunk_frames=G)
    outs, pos = [], 0
    for n in sizes:
        outs.append(st.push(xk[None, pos:pos + n]))
        pos += n
    outs.append(st.flush())
    st.close()
    return np.concatenate(outs, 1)[0]


def _base(tmp_path_factory):
    """The schedule's outputs on the fixed-embedding container, and each key's solo stream: computed once."""
    if "base" not in _CASES:
        eng, x, enroll, kind = _engine(False, tmp_path_factory)
        _CASES["base"] = (run_schedule(eng, x, enroll, kind), {k: _solo(eng, x[k], enroll[k], kind, PACKETS[k]) for k in LENGTHS})
    return _CASES["base"]


def test_schedule_matches_the_solo_stream_and_separate(tmp_path_factory):
    eng, x, enroll, kind = _engine(False, tmp_path_factory)
    assert all(sum(PACKETS[k]) == n for k, n in LENGTHS.items()) and 4000 in PACKETS["b"] and 160 in PACKETS["a"]
    got, solo = _base(tmp_path_factory)
    worst, same = 0.0, True
    for k, n in LENGTHS.items():
        sep = eng.separate(x[k][None], enroll[k][None], kind)[0, :t_out(n)]
        assert got[k].shape == solo[k].shape == (t_out(n),) and np.isfinite(got[k]).all() and float(np.abs(sep).max()) > 0
        e1, e2 = _rel(got[k], solo[k]), _rel(got[k], sep)
        same = same and np.array_equal(got[k], solo[k])
        worst = max(worst, e1, e2)
        print(f"stream pool slot '{k}' ({n} samples): rel L2 vs the solo stream {e1:.3e}, vs Engine.separate {e2:.3e}")
        assert e1 < 1e-4 and e2 < 1e-4
    print(f"stream pool schedule: worst rel L2 {worst:.3e}; bit-identical to the solo streams: {same}")


def test_the_same_schedule_twice_repeats_the_bits(tmp_path_factory):
    eng, x, enroll, kind = _engine(False, tmp_path_factory)
    got, _ = _base(tmp_path_factory)
    again = run_schedule(eng, x, enroll, kind)
    assert all(np.array_equal(got[k], again[k]) for k in LENGTHS)


@pytest.mark.parametrize("other", ["other-data", "inf-and-nan"])
def test_a_slot_does_not_see_what_the_other_slots_carry(other, tmp_path_factory):
    """Isolation: with the other slots' audio replaced (same packet sizes, so the same launches), the observed slot's bits stay."""
    eng, x, enroll, kind = _engine(False, tmp_path_factory)
    got, _ = _base(tmp_path_factory)
    for seen in ("b", "d"):
        y = {}
        for k, v in x.items():
            if k == seen:
                y[k] = v
            elif other == "other-data":
                y[k] = np.ascontiguousarray(v[::-1] * 3.0 + 0.25)
            else:
                y[k] = v.copy()
                y[k][5::7] = np.inf
                y[k][6::11] = np.nan
                y[k][300:420] = -np.inf
        res = run_schedule(eng, y, enroll, kind)
        assert np.array_equal(res[seen], got[seen]) and np.isfinite(res[seen]).all(), (other, seen)
        assert other != "other-data" or not np.array_equal(res["c"], got["c"])


def test_a_pool_of_one_slot_is_the_solo_stream_bit_for_bit(tmp_path_factory):
    eng, x, enroll, kind = _engine(False, tmp_path_factory)
    _, solo = _base(tmp_path_factory)
    for k in ("a", "b"):
        one = run_schedule(eng, x, enroll, kind, [("attach", k)] + [("push", k)] * len(PACKETS[k]) + [("flush", k)], slots=1)
        assert np.array_equal(one[k], solo[k]), k


def test_spex_plus_two_slots_with_waveform_enrollment(tmp_path_factory):
    eng, x, enroll, kind = _engine(True, tmp_path_factory)
    sched = [("attach", "a"), ("push", "a"), ("attach", "c"), ("push", "c", "a")] + [("push", "a", "c")] * 4 + \
            [("flush", "c")] + [("push", "a")] * 5 + [("flush", "a")]
    got = run_schedule(eng, x, enroll, kind, sched, slots=2)
    for k in ("a", "c"):
        solo = _solo(eng, x[k], enroll[k], kind, PACKETS[k])
        e = _rel(got[k], solo)
        print(f"stream pool SpEx+ slot '{k}': rel L2 vs the solo stream {e:.3e}, bit-identical {np.array_equal(got[k], solo)}")
        assert got[k].shape == (t_out(LENGTHS[k]),) and np.isfinite(got[k]).all() and e < 1e-4


def _write_wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


def test_separate_main_stream_pool_matches_stream_ms_alone(tmp_path):
    from tests.test_engine_gpu import _cuda
    from wesep_amd.models import get_model
    _cuda()
    torch.manual_seed(23)
    model = get_model("ConvTasNet")(N=256, L=20, B=32, H=64, P=3, X=3, R=2, spk_emb_dim=256, causal=True, norm="cLN",
                                    joint_training=True)
    path = str(tmp_path / "c.wsw")
    export_engine(model, path)
    rng = np.random.default_rng(3)
    lines, lens = [], {"a": 3203, "b": 1600, "c": 2411, "d": 170, "e": 977}
    for key, n in lens.items():
        _write_wav(tmp_path / f"{key}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"{key}_e1.wav", rng.integers(-3000, 3000, 900))
        _write_wav(tmp_path / f"{key}_e2.wav", rng.integers(-3000, 3000, 1000))
        lines.append(f"{key} {tmp_path}/{key}.wav {tmp_path}/{key}_e1.wav {tmp_path}/{key}_e2.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    exe = os.path.join(ROOT, "runtime", "separate_main")
    outs = {}
    for tag, extra in (("stream", ["--stream_ms", "10"]), ("pool", ["--stream_ms", "10", "--stream_pool", "3"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = {f: np.fromfile(out / f, dtype=np.float32) for f in sorted(os.listdir(out)) if f.endswith(".f32")}
        assert sorted(os.listdir(out)) == sorted(f"{k}-spk{i}.{ext}" for k in lens for i in (1, 2) for ext in ("wav", "f32"))
    worst = 0.0
    for f, solo in outs["stream"].items():
        got = outs["pool"][f]
        assert got.shape == solo.shape and np.isfinite(got).all() and float(np.abs(solo).max()) > 0
        worst = max(worst, _rel(got, solo))
    print(f"separate_main --stream_ms 10 --stream_pool 3: worst rel L2 vs --stream_ms 10 alone {worst:.3e}")
    assert worst < 1e-4
