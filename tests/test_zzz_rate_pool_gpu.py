"""GPU: the rate pool of the native runtime (runtime/rate_pool.cc, ws_engine_rate_pool_*) -- the schedule of
tests/test_zzz_stream_pool_gpu.py (a late attach, a 250 ms packet beside 10 ms packets, a flush in mid-run, the freed slot
attached again) with the slots at 8 kHz, 48 kHz and 16 kHz and the re-attached one at ANOTHER rate.  Default path: every
key's output bit for bit a solo Engine.rate_stream(1, ...) with the same max_chunk_frames, max_push, packets and flags; the
16 kHz slot bit for bit a plain StreamPool slot; isolation; a 44.1 kHz slot (the global-table path) beside an 8 kHz one;
against the composition resample -> separate -> resample within the streamer's 1e-4.  block_kernel=True: bit for bit
Engine.resample -> flagged stream -> Engine.resample, cropped, under fixed and random packets.  Launch figures and the
constant state size on the device.  The engine runs with WS_ENGINE_POISON=1 (tests/test_zzz_stream_pool_gpu.py)."""
import numpy as np
import pytest
import torch

from tests import resample_contract as RC
from tests.test_zzz_stream_pool_gpu import LENGTHS, PACKETS, SCHEDULE, _engine, _rel
from wesep_amd import engine as E

pytestmark = pytest.mark.gpu
G, MAX_PUSH, L = 16, 1500, 20
RATE = {"a": 8000, "b": 48000, "c": 16000, "d": 48000}         # "d" takes the slot "a" (8 kHz) leaves
_CASES = {}


def _scaled(rate):
    """the pool tests' lengths and packets at `rate` (a packet of 160 is 10 ms, 4000 is 250 ms)"""
    return {k: [max(1, p * rate // 16000) for p in PACKETS[k]] for k in PACKETS}


def _setup(tmp_path_factory):
    if "setup" not in _CASES:
        eng, _, enroll, kind = _engine(False, tmp_path_factory)
        packets = {k: _scaled(RATE[k])[k] for k in RATE}
        g = torch.Generator().manual_seed(17)
        x = {k: (0.1 * torch.randn(sum(packets[k]), generator=g)).numpy() for k in RATE}
        _CASES["setup"] = (eng, x, enroll, kind, packets)
    return _CASES["setup"]


def run_schedule(eng, x, enroll, kind, packets, rate=RATE, schedule=SCHEDULE, slots=3, block_kernel=False, check_launches=True):
    pool = eng.rate_pool(slots, sorted(set(rate.values())), max_chunk_frames=G, max_push=MAX_PUSH, block_kernel=block_kernel)
    state = eng.info("stream_state_bytes")
    group = (E.rate_pool_block_group_launches if block_kernel else E.rate_pool_group_launches)(2, 3)
    slot, pos, nxt, out = {}, {}, {}, {}
    for ev, *keys in schedule:
        if ev == "attach":
            k = keys[0]
            slot[k], pos[k], nxt[k], out[k] = pool.attach(enroll[k], kind, rate[k]), 0, 0, []
        elif ev == "push":
            chunks, before = {}, {}
            for k in keys:
                n = packets[k][nxt[k]]
                before[k] = pos[k]
                chunks[slot[k]] = x[k][pos[k]:pos[k] + n]
                pos[k], nxt[k] = pos[k] + n, nxt[k] + 1
            got = pool.push(chunks)
            launches = eng.info("n_launches")
            for k in keys:
                out[k].append(got[slot[k]])
                assert got[slot[k]].shape[0] == RC.rate_stream_emitted(pos[k], rate[k], 16000, L) - RC.rate_stream_emitted(before[k], rate[k], 16000, L) \
                    if rate[k] != 16000 else got[slot[k]].shape[0] == RC.plain_emitted(pos[k], L) - RC.plain_emitted(before[k], L)
            if check_launches and all(packets[k][nxt[k] - 1] <= MAX_PUSH for k in keys):
                # one piece: the groups of the slot that owes most, and at most the piece's three calls -- whatever the slots and rates
                assert launches % group <= E.RATE_POOL_PIECE_LAUNCHES, (keys, launches)
        elif ev == "flush":
            out[keys[0]].append(pool.flush(slot[keys[0]]))
        else:
            pool.detach(slot[keys[0]])
        assert eng.info("stream_state_bytes") == state
    pool.close()
    assert all(nxt[k] == len(packets[k]) and pos[k] == x[k].shape[0] for k in out)
    return {k: np.concatenate(v) for k, v in out.items()}


def _solo(eng, xk, ek, kind, rate, sizes, block_kernel=False):
    st = eng.rate_stream(1, ek[None], kind, rate, max_chunk_frames=G, max_push=MAX_PUSH, block_kernel=block_kernel)
    outs, pos = [], 0
    for n in sizes:
        outs.append(st.push(xk[None, pos:pos + n]))
        pos += n
    outs.append(st.flush())
    st.close()
    return np.concatenate(outs, 1)[0]


def _base(tmp_path_factory):
    if "base" not in _CASES:
        eng, x, enroll, kind, packets = _setup(tmp_path_factory)
        _CASES["base"] = run_schedule(eng, x, enroll, kind, packets)
    return _CASES["base"]


def test_every_slot_is_its_solo_rate_stream_bit_for_bit(tmp_path_factory):
    eng, x, enroll, kind, packets = _setup(tmp_path_factory)
    got = _base(tmp_path_factory)
    for k, rate in RATE.items():
        solo = _solo(eng, x[k], enroll[k], kind, rate, packets[k])
        n = x[k].shape[0]
        total = RC.rate_stream_total(n, rate, 16000, L) if rate != 16000 else RC.plain_total(n, L)
        assert got[k].shape == solo.shape == (total,) and np.isfinite(got[k]).all() and float(np.abs(solo).max()) > 0
        print(f"rate pool slot '{k}' at {rate} Hz ({n} samples): rel L2 vs the solo rate stream {_rel(got[k], solo):.3e}")
        assert np.array_equal(got[k], solo), (k, rate)


def test_the_container_rate_slot_is_a_plain_pool_slot(tmp_path_factory):
    eng, x, enroll, kind, packets = _setup(tmp_path_factory)
    got = _base(tmp_path_factory)
    pool = eng.stream_pool(1, max_chunk_frames=G)
    s = pool.attach(enroll["c"], kind)
    outs, pos = [], 0
    for n in packets["c"]:
        outs.append(pool.push({s: x["c"][pos:pos + n]})[s])
        pos += n
    outs.append(pool.flush(s))
    pool.close()
    plain = np.concatenate(outs)
    assert got["c"].shape == plain.shape and np.array_equal(got["c"], plain)


@pytest.mark.parametrize("other", ["other-data", "inf-and-nan"])
def test_a_slot_does_not_see_what_the_other_slots_carry(other, tmp_path_factory):
    eng, x, enroll, kind, packets = _setup(tmp_path_factory)
    got = _base(tmp_path_factory)
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
        res = run_schedule(eng, y, enroll, kind, packets)
        assert np.array_equal(res[seen], got[seen]) and np.isfinite(res[seen]).all(), (other, seen)
        assert other != "other-data" or not np.array_equal(res["c"], got["c"])


def test_a_44100_slot_beside_an_8000_one(tmp_path_factory):
    """the global-table path through the engine: about 0.25 s at 44.1 kHz in 10 ms packets, beside an 8 kHz slot"""
    eng, _, enroll, kind, _ = _setup(tmp_path_factory)
    rate = {"a": 44100, "b": 8000}
    packets = {"a": [441] * 25 + [7], "b": [80] * 20 + [333]}
    g = torch.Generator().manual_seed(19)
    x = {k: (0.1 * torch.randn(sum(packets[k]), generator=g)).numpy() for k in rate}
    sched = [("attach", "a"), ("attach", "b")] + [("push", "a", "b")] * 21 + [("flush", "b")] + [("push", "a")] * 5 + [("flush", "a")]
    got = run_schedule(eng, x, enroll, kind, packets, rate=rate, schedule=sched, slots=2)
    for k in rate:
        solo = _solo(eng, x[k], enroll[k], kind, rate[k], packets[k])
        assert got[k].shape == solo.shape == (RC.rate_stream_total(x[k].shape[0], rate[k], 16000, L),) and np.array_equal(got[k], solo), k


def _packets(n, lo, hi, seed):
    rng, out = np.random.default_rng(seed), []
    while n:
        out.append(int(min(n, rng.integers(lo, hi + 1))))
        n -= out[-1]
    return out


def _composition(eng, ek, kind, xk, rate, block_kernel, streamed):
    """Engine.resample -> the stream (flagged) or whole-utterance separate -> Engine.resample, cropped to the samples pushed"""
    if rate == 16000:                   # the container's own rate: no resampler on either side
        return eng.separate(xk[None], ek[None], kind)[0, :RC.plain_total(xk.shape[0], L)]
    x_m = eng.resample(xk[None], rate, 16000)
    if streamed:
        st = eng.stream(1, ek[None], kind, max_chunk_frames=G, block_kernel=block_kernel)
        y_m = np.concatenate([st.push(x_m), st.flush()], axis=1)
        st.close()
    else:
        y_m = eng.separate(x_m, ek[None], kind)
        y_m = y_m[:, :RC.plain_total(x_m.shape[1], L)]
    return eng.resample(y_m, 16000, rate)[0, :xk.shape[0]]


@pytest.mark.parametrize("name", ["fixed", "random"])
def test_flagged_slots_are_the_composition_bit_for_bit(name, tmp_path_factory):
    eng, _, enroll, kind, _ = _setup(tmp_path_factory)
    rate = {"a": 8000, "b": 48000}
    n = {"a": 3001, "b": 12007}
    g = torch.Generator().manual_seed(23)
    x = {k: (0.1 * torch.randn(n[k], generator=g)).numpy() for k in rate}
    if name == "fixed":
        packets = {k: [rate[k] // 100] * (n[k] // (rate[k] // 100)) + ([n[k] % (rate[k] // 100)] if n[k] % (rate[k] // 100) else []) for k in rate}
    else:
        packets = {k: _packets(n[k], 1, 4000, 4 + i) for i, k in enumerate(rate)}
    rounds = max(len(p) for p in packets.values())
    sched = [("attach", "a"), ("attach", "b")]
    for j in range(rounds):
        sched.append(("push",) + tuple(k for k in rate if j < len(packets[k])))
    sched += [("flush", "a"), ("flush", "b")]
    got = run_schedule(eng, x, enroll, kind, packets, rate=rate, schedule=sched, slots=2, block_kernel=True, check_launches=False)
    for k in rate:
        total = RC.rate_stream_total(n[k], rate[k], 16000, L)
        ref = _composition(eng, enroll[k], kind, x[k], rate[k], True, True)
        assert got[k].shape == (total,) and ref.shape[0] >= total and np.isfinite(got[k]).all()
        assert np.array_equal(got[k], ref[:total]), (name, k)


def test_default_path_against_the_whole_utterance_composition(tmp_path_factory):
    eng, x, enroll, kind, _ = _setup(tmp_path_factory)
    got = _base(tmp_path_factory)
    for k, rate in RATE.items():
        ref = _composition(eng, enroll[k], kind, x[k], rate, False, False)
        e = _rel(got[k], ref[:got[k].shape[0]])
        print(f"rate pool slot '{k}' at {rate} Hz: rel L2 against resample -> separate -> resample {e:.3e}")
        assert e <= 1e-4, (k, e)


@pytest.mark.parametrize("block_kernel", [False, True])
def test_launch_figures_and_state_on_the_device(block_kernel, tmp_path_factory):
    eng, _, enroll, kind, _ = _setup(tmp_path_factory)
    group = (E.rate_pool_block_group_launches if block_kernel else E.rate_pool_group_launches)(2, 3)
    piece = E.RATE_POOL_BLOCK_PIECE_LAUNCHES if block_kernel else E.RATE_POOL_PIECE_LAUNCHES
    assert group == (E.pool_block_group_launches if block_kernel else E.pool_group_launches)(2, 3) + 2 and piece == 3
    figures = []
    for rates in ([8000], [8000, 16000], [8000, 16000, 48000, 8000]):
        pool = eng.rate_pool(4, [8000, 48000], max_chunk_frames=G, max_push=MAX_PUSH, block_kernel=block_kernel)
        state = eng.info("stream_state_bytes")
        slots = [pool.attach(enroll["a"], kind, r) for r in rates]
        pool.push({s: np.zeros(r // 50, np.float32) for s, r in zip(slots, rates)})          # 20 ms: the first frames
        pool.push({s: np.zeros(r // 100, np.float32) for s, r in zip(slots, rates)})         # 10 ms in mid-stream: one group
        figures.append(eng.info("n_launches"))
        assert eng.info("stream_state_bytes") == state
        pool.flush(slots[0])
        pool.detach(slots[0])
        assert pool.attach(enroll["b"], kind, 48000) == slots[0] and eng.info("stream_state_bytes") == state
        pool.close()
    assert figures == [group + piece] * 3, figures


def test_separate_main_rate_pool_matches_resample_stream_ms_alone(tmp_path):
    """three lines at 8, 48 and 16 kHz, two at a time through one rate pool, against `--resample --stream_ms 10` line by line"""
    import os
    import subprocess
    from tests.test_engine_gpu import _cuda
    from tests.test_zzz_stream_pool_gpu import ROOT, _write_wav
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    _cuda()
    torch.manual_seed(23)
    model = get_model("ConvTasNet")(N=256, L=20, B=32, H=64, P=3, X=3, R=2, spk_emb_dim=256, causal=True, norm="cLN", joint_training=True)
    path = str(tmp_path / "c.wsw")
    export_engine(model, path)
    rng = np.random.default_rng(3)
    lines, files = [], {"u8": (8000, 1601), "u48": (48000, 7213), "u16": (16000, 2411)}
    for key, (rate, n) in files.items():
        _write_wav(tmp_path / f"{key}.wav", rng.integers(-3000, 3000, n), sr=rate)
        _write_wav(tmp_path / f"{key}_e1.wav", rng.integers(-3000, 3000, 900))
        _write_wav(tmp_path / f"{key}_e2.wav", rng.integers(-3000, 3000, 500), sr=8000)
        lines.append(f"{key} {tmp_path}/{key}.wav {tmp_path}/{key}_e1.wav {tmp_path}/{key}_e2.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    exe = os.path.join(ROOT, "runtime", "separate_main")
    outs = {}
    for tag, extra in (("stream", ["--resample", "--stream_ms", "10"]), ("pool", ["--stream_ms", "10", "--rate_pool", "2"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out", *extra],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs[tag] = {f: np.fromfile(out / f, dtype=np.float32) for f in sorted(os.listdir(out)) if f.endswith(".f32")}
        assert sorted(os.listdir(out)) == sorted(f"{k}-spk{i}.{ext}" for k in files for i in (1, 2) for ext in ("wav", "f32"))
    worst = 0.0
    for f, solo in outs["stream"].items():
        got = outs["pool"][f]
        assert got.shape == solo.shape == (files[f.split("-")[0]][1],) and np.isfinite(got).all() and float(np.abs(solo).max()) > 0
        worst = max(worst, _rel(got, solo))
    print(f"separate_main --stream_ms 10 --rate_pool 2: worst rel L2 vs --resample --stream_ms 10 alone {worst:.3e}")
    assert worst < 1e-4
