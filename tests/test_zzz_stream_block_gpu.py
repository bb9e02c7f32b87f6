"""GPU: WS_STREAM_BLOCK_KERNEL in the native runtime (runtime/stream.cc, runtime/stream_pool.cc) on the small container of
tests/test_zzz_stream_pool_gpu.py (N 32 / L 20 / B 32 / H 64 / P 3 / X 3 / R 2), `max_chunk_frames` 4, WS_ENGINE_POISON=1.

Within the existing bound (rel L2 <= 1e-4): the flagged stream against the unflagged stream and against `Engine.separate`
on the whole signal; one SpEx+ joint container with two pool slots, flagged against unflagged; `separate_main --stream_ms 10
--stream_block --stream_pool 3` against `--stream_ms 10` on five short wavs.

Bit for bit (`np.array_equal`), which the block kernel makes a property of the separator -- every frame's products are
reduced in one fixed order wherever the frame sits: the flagged stream under two packet schedules (10 ms packets against
random 1 to 4000 samples); a flagged pool slot against a flagged solo rows = 1 stream, with three slots, a late attach, a
250 ms packet beside a 10 ms one, a flush in mid-run and a detach / re-attach; the same with the other slots' audio replaced
by other data and by inf / NaN."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests.test_zzz_stream_pool_gpu import G, LENGTHS, PACKETS, S, SCHEDULE, _engine, _rel, _write_wav, t_out
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def run_schedule(eng, x, enroll, kind, schedule=SCHEDULE, packets=PACKETS, slots=3, block_kernel=True):
    """{key: the concatenation of what the key's pushes and its flush returned}, on a pool opened with the flag"""
    pool = eng.stream_pool(slots, max_chunk_frames=G, block_kernel=block_kernel)
    group = E.pool_block_group_launches(2, 3) if block_kernel else E.pool_group_launches(2, 3)
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
            assert eng.info("n_launches") % group == 0
            for k in keys:
                out[k].append(got[slot[k]])
                assert sum(o.shape[0] for o in out[k]) == (max(0, (pos[k] - 160) // S + 1) * S if pos[k] >= 160 else 0)
        elif ev == "flush":
            out[keys[0]].append(pool.flush(slot[keys[0]]))
        else:
            pool.detach(slot[keys[0]])
    assert eng.info("stream_state_bytes") == state
    pool.close()
    return {k: np.concatenate(v) for k, v in out.items()}


def solo(eng, xk, ek, kind, sizes, block_kernel=True):
    st = eng.stream(1, ek[None], kind, max_chunk_frames=G, block_kernel=block_kernel)
    group = E.stream_block_group_launches(2, 3) if block_kernel else 3 * 2 * 3 + 10
    outs, pos = [], 0
    for n in sizes:
        outs.append(st.push(xk[None, pos:pos + n]))
        assert eng.info("n_launches") % group == 0
        pos += n
    outs.append(st.flush())
    st.close()
    return np.concatenate(outs, 1)[0]


def _base(tmp_path_factory):
    """The flagged schedule's outputs and each key's flagged solo stream on the fixed-embedding container: computed once."""
    if "base" not in _CACHE:
        eng, x, enroll, kind = _engine(False, tmp_path_factory)
        _CACHE["base"] = (run_schedule(eng, x, enroll, kind), {k: solo(eng, x[k], enroll[k], kind, PACKETS[k]) for k in LENGTHS})
    return _CACHE["base"]


def test_flagged_stream_against_the_unflagged_stream_and_separate(tmp_path_factory):
    eng, x, enroll, kind = _engine(False, tmp_path_factory)
    _, flagged = _base(tmp_path_factory)
    for k, n in LENGTHS.items():
        plain = solo(eng, x[k], enroll[k], kind, PACKETS[k], block_kernel=False)
        sep = eng.separate(x[k][None], enroll[k][None], kind)[0, :t_out(n)]
        assert flagged[k].shape == plain.shape == (t_out(n),) and np.isfinite(flagged[k]).all() and float(np.abs(sep).max()) > 0
        e1, e2 = _rel(flagged[k], plain), _rel(flagged[k], sep)
        print(f"block stream '{k}' ({n} samples): rel L2 vs the unflagged stream {e1:.3e}, vs Engine.separate {e2:.3e}")
        assert e1 <= 1e-4 and e2 <= 1e-4


def test_flagged_stream_bits_do_not_depend_on_the_packet_schedule(tmp_path_factory):
    eng, x, enroll, kind = _engine(False, tmp_path_factory)
    k, n = "b", LENGTHS["b"]
    ten_ms = [160] * (n // 160) + ([n % 160] if n % 160 else [])
    g, rnd, left = torch.Generator().manual_seed(17), [], n
    while left > 0:
        m = min(left, int(torch.randint(1, 4001, (1,), generator=g)))
        rnd.append(m)
        left -= m
    a, b = solo(eng, x[k], enroll[k], kind, ten_ms), solo(eng, x[k], enroll[k], kind, rnd)
    assert len(rnd) > 1 and rnd != ten_ms and a.shape == (t_out(n),) and np.isfinite(a).all()
    assert np.array_equal(a, b), float(np.abs(a - b).max())
    assert np.array_equal(a, _base(tmp_path_factory)[1][k])                          # and PACKETS["b"]: a third schedule


def test_flagged_pool_slot_is_the_flagged_solo_stream_bit_for_bit(tmp_path_factory):
    got, alone = _base(tmp_path_factory)
    assert 4000 in PACKETS["b"] and 160 in PACKETS["a"] and ("detach", "a") in SCHEDULE
    for k, n in LENGTHS.items():
        assert got[k].shape == (t_out(n),) and np.isfinite(got[k]).all()
        assert np.array_equal(got[k], alone[k]), (k, float(np.abs(got[k] - alone[k]).max()))


@pytest.mark.parametrize("other", ["other-data", "inf-and-nan"])
def test_flagged_pool_slot_with_other_audio_beside_it(other, tmp_path_factory):
    eng, x, enroll, kind = _engine(False, tmp_path_factory)
    _, alone = _base(tmp_path_factory)
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
        assert np.array_equal(res[seen], alone[seen]) and np.isfinite(res[seen]).all(), (other, seen)


def test_spex_plus_two_slots_flagged_against_unflagged(tmp_path_factory):
    eng, x, enroll, kind = _engine(True, tmp_path_factory)
    sched = [("attach", "a"), ("push", "a"), ("attach", "c"), ("push", "c", "a")] + [("push", "a", "c")] * 4 + \
            [("flush", "c")] + [("push", "a")] * 5 + [("flush", "a")]
    got = run_schedule(eng, x, enroll, kind, sched, slots=2)
    plain = run_schedule(eng, x, enroll, kind, sched, slots=2, block_kernel=False)
    for k in ("a", "c"):
        e = _rel(got[k], plain[k])
        print(f"block pool SpEx+ slot '{k}': rel L2 vs the unflagged pool {e:.3e}")
        assert got[k].shape == (t_out(LENGTHS[k]),) and np.isfinite(got[k]).all() and e <= 1e-4


def test_separate_main_stream_block_pool_matches_stream_ms_alone(tmp_path):
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
    for tag, extra in (("stream", ["--stream_ms", "10"]), ("block", ["--stream_ms", "10", "--stream_block", "--stream_pool", "3"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = {f: np.fromfile(out / f, dtype=np.float32) for f in sorted(os.listdir(out)) if f.endswith(".f32")}
        assert sorted(os.listdir(out)) == sorted(f"{k}-spk{i}.{ext}" for k in lens for i in (1, 2) for ext in ("wav", "f32"))
    worst = 0.0
    for f, ref in outs["stream"].items():
        got = outs["block"][f]
        assert got.shape == ref.shape and np.isfinite(got).all() and float(np.abs(ref).max()) > 0
        worst = max(worst, _rel(got, ref))
    print(f"separate_main --stream_ms 10 --stream_block --stream_pool 3: worst rel L2 vs --stream_ms 10 alone {worst:.3e}")
    assert worst <= 1e-4
