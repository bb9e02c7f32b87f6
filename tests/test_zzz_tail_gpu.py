"""GPU: the tail pool (runtime/tail_pool.cc; ws_tail_emit_rows_fwd of longform.hip; DESIGN 7 "Tail pool").  The emission kernel
against its contract over a sweep of tables; every architecture with three slots attached at different times against the rule
restated (tests/emu_tail.py) on the same engine's ws_engine_separate of every window alone -- bit for bit outside the
cross-fades with one row per forward, to the rounding of other row counts otherwise; a slot's bits against what the other slots
carry; enroll once at attach; `separate_main --tail_ms` against Engine.tail."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import emu_tail as T
from tests.test_longform_gpu import ENGINE_CASES, SPK, _cuda, _model, rel
from wesep_amd import dev
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
# what the three spelled-out roundings -- v = fl(y scale), d = fl(v - hold), out = fma(ramp, d, hold) -- allow against the
# float64 restatement hold + ramp (v - hold) on the same fp32 v: |d| 2^-24 from the difference, |out| 2^-24 <= (|v| + |hold|) 2^-24
# from the fma, ramp <= 1; twice that sum, doubled once more for the float64 side's own order of operations
BLEND_BOUND = 4 * 2.0 ** -24


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- the kernel ------------------------------------------------------------------------------------------------------
def _row_kinds(C, h):
    """(L, p, m, c_new): a row of several workgroups; only held samples come out; the flush of a long window; L = C; 700 samples"""
    kinds = [(5000, 1234, 5000 - 1234 - C, C), (700, 700 - h - C, h, C), (5000, 0, 5000, 0), (700, 13, 700 - 13 - C, C)]
    if C > 0:
        kinds.append((C, 0, C if h else 0, 0 if h else C))       # the whole window is the cross-fade, or the first hold
    return [k for k in kinds if k[2] + k[3] >= 1 and k[2] >= h]


def _emit_case(d, g, C, h, scale, kinds, poison_row=None):
    """the arenas (NaN-prefilled where the kernel writes), the table and the expected values of one launch"""
    rows, y_parts, hold_parts, expect = [], [], [], []
    y_at, hold_at, out_at = 1, 2, 3                               # odd first offsets: no alignment is assumed
    for i, (L, p, m, c_new) in enumerate(kinds):
        y = torch.randn(L, generator=g).numpy()
        if i == poison_row:
            y[::3], y[1::6], y[4::6] = np.nan, np.inf, -np.inf        # two samples of three
        hold = torch.randn(h, generator=g).numpy()
        rows.append(dict(y_off=y_at, hold_in_off=hold_at, hold_out_off=hold_at + h + 1, out_off=out_at, L=L, p=p, h=h, m=m, c_new=c_new,
                         scale=scale))
        v = y.astype(np.float32) * np.float32(scale)
        expect.append(dict(v=v[p:p + m], hold=hold, new=v[p + m:p + m + c_new], row=rows[-1]))
        y_parts.append((y_at, y))
        hold_parts.append((hold_at, hold))
        y_at += L + 1 + i % 3
        hold_at += h + c_new + 2 + i % 2
        out_at += m + 1 + i % 4                                   # out offsets of every residue mod 4
    ys, holds = np.full(y_at + 5, NAN, np.float32), np.full(hold_at + 5, NAN, np.float32)
    for o, x in y_parts:
        ys[o:o + len(x)] = x
    for o, x in hold_parts:
        holds[o:o + len(x)] = x
    return rows, expect, torch.from_numpy(ys).to(d), torch.from_numpy(holds).to(d), holds, torch.full((out_at + 5,), NAN, device=d)


def _check_emit(C, h, expect, holds0, hold, out, ramp, tag):
    hold, out = hold.cpu().numpy(), out.cpu().numpy()
    w_out, w_hold = np.zeros(len(out), bool), np.zeros(len(hold), bool)
    worst = 0.0
    for i, e in enumerate(expect):
        r = e["row"]
        got = out[r["out_off"]:r["out_off"] + r["m"]]
        new = hold[r["hold_out_off"]:r["hold_out_off"] + r["c_new"]]
        w_out[r["out_off"]:r["out_off"] + r["m"]] = True
        w_hold[r["hold_out_off"]:r["hold_out_off"] + r["c_new"]] = True
        assert _same_bits(got[h:], e["v"][h:]), (tag, i, "plain positions")
        assert _same_bits(new, e["new"]), (tag, i, "new hold")
        if h:
            v, hd = e["v"][:h].astype(np.float64), e["hold"].astype(np.float64)
            with np.errstate(invalid="ignore"):                    # (the row whose y holds NaN and inf)
                ref = hd + ramp.astype(np.float64) * (v - hd)
            fin = np.isfinite(ref)
            assert np.array_equal(np.isnan(got[:h]), np.isnan(ref)), (tag, i)
            err, bound = np.abs(got[:h].astype(np.float64)[fin] - ref[fin]), BLEND_BOUND * (np.abs(v) + np.abs(hd))[fin]
            worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()) if fin.any() else 0.0)
            assert (err <= bound).all(), (tag, i, float(err.max()))
    # nothing outside the named ranges was written: the NaNs stay, the hold the rows read is as it was
    assert np.isnan(out[~w_out]).all(), tag
    assert _same_bits(hold[~w_hold], holds0[~w_hold]), tag
    return worst


@pytest.mark.parametrize("C", [0, 1, 3, 256])
def test_tail_emit_rows_contract(C):
    d = _cuda()
    g = torch.Generator().manual_seed(31 + C)
    ramp = T.ramp_of(C)
    d_ramp = torch.from_numpy(ramp).to(d) if C else None
    worst = 0.0
    for h in sorted({0, C}):
        kinds = _row_kinds(C, h)
        for scale in (1.0, 0.37):
            # A = 1: every kind of row as a launch of its own
            for k in kinds:
                rows, expect, y, hold, holds0, out = _emit_case(d, g, C, h, scale, [k])
                dev.tail_emit_rows(rows, C, d_ramp, y, hold, out)
                torch.cuda.synchronize()
                worst = max(worst, _check_emit(C, h, expect, holds0, hold, out, ramp[:h], (C, h, scale, k)))
            # A = 5: the kinds in one launch (the first one twice when there are four), one row's y holding NaN and inf -- and
            # the same launch with that row's y finite: the other rows return the same bits
            five = (kinds + kinds)[:5]
            runs = []
            for poison in (1, None):
                gg = torch.Generator().manual_seed(1000 * C + 10 * h + int(scale * 100))
                rows, expect, y, hold, holds0, out = _emit_case(d, gg, C, h, scale, five, poison_row=poison)
                assert len(rows) == 5
                dev.tail_emit_rows(rows, C, d_ramp, y, hold, out)
                torch.cuda.synchronize()
                worst = max(worst, _check_emit(C, h, expect, holds0, hold, out, ramp[:h], (C, h, scale, "A=5", poison)))
                runs.append((rows, hold.cpu().numpy(), out.cpu().numpy()))
            for i, r in enumerate(runs[0][0]):
                if i == 1:                                        # the row that carried them
                    mine = np.concatenate([runs[0][2][r["out_off"]:r["out_off"] + r["m"]],
                                           runs[0][1][r["hold_out_off"]:r["hold_out_off"] + r["c_new"]]])
                    assert not np.isfinite(mine).all() or len(mine) < 3
                    continue
                for arena, off, cnt in ((2, "out_off", "m"), (1, "hold_out_off", "c_new")):
                    assert _same_bits(runs[0][arena][r[off]:r[off] + r[cnt]], runs[1][arena][r[off]:r[off] + r[cnt]]), (C, h, scale, i)
    print(f"ws_tail_emit_rows_fwd C={C}: worst cross-fade error {worst:.3f} of the bound 4 * 2^-24 (|v| + |hold|)")


# ---- engines -----------------------------------------------------------------------------------------------------------
WARM = {"pBSRNN": 1000, "ConvTasNet": 500, "DPCCN": 3968, "TFGridNet": 1000}
CYCLES = {"DPCCN": ((700, 1300, 333), (1000,), (900, 1100, 513))}
FADE = 128


def _schedule(lens, cycles, attach_at, S, C, warm):
    """Rounds of a run: recording i is attached in round attach_at[i]; every round pushes each recording in flight its next packet
    (its cycle's next size, cut to what is left and to what a window still holds) and ticks them all; a recording whose samples
    are used up is flushed and detached.  -> [(attach [i], {i: (pos, n)}, flush [i])], and per round the window lengths that fire"""
    model = {}
    pos, step, rounds, fired = {}, {}, [], []
    todo, t = list(range(len(lens))), 0
    while todo or model:
        att = [i for i in todo if attach_at[i] <= t]
        for i in att:
            todo.remove(i)
            model[i], pos[i], step[i] = T.Tail(1, S, C, warm, lambda x: np.zeros((1, len(x)))), 0, 0
        packets = {}
        for i, m in model.items():
            c = min(cycles[i][step[i] % len(cycles[i])], lens[i] - pos[i], S - (m.N - m.E))
            packets[i] = (pos[i], c)
            m.push(np.zeros(c))
            pos[i] += c
            step[i] += 1
        fired.append([min(m.N, S) for i, m in sorted(model.items()) if m.fires()])
        for m in model.values():
            m.tick()
        done = [i for i in model if pos[i] == lens[i]]
        for i in done:
            del model[i]
        rounds.append((att, packets, done))
        t += 1
    return rounds, fired


def _replay(rounds, audio, attach, push, tick, flush):
    """-> per recording the concatenated output of its ticks and its flush"""
    slot, parts = {}, {i: [] for i in range(len(audio))}
    for att, packets, done in rounds:
        for i in att:
            slot[i] = attach(i)
        push({slot[i]: audio[i][p:p + c] for i, (p, c) in packets.items()})
        got = tick([slot[i] for i in packets])
        for i in packets:
            if slot[i] in got:
                parts[i].append(got[slot[i]])
        for i in done:
            parts[i].append(flush(slot.pop(i)))
    return [np.concatenate(p, axis=1) for p in parts.values()]


def _run_pool(eng, c, fade, max_rows, audio=None, rounds=None, log=None):
    audio, rounds = c["audio"] if audio is None else audio, c["rounds"] if rounds is None else rounds
    pool = eng.tail_pool(3, c["K"], c["S"], fade, c["warm"], max_rows)

    def tick(named):
        got = pool.tick(named)
        if log is not None:
            log.append((eng.info("tail_pool_forwards"), eng.info("tail_pool_rows"), eng.info("n_launches")))
        return got

    def flush(s):
        out = pool.flush(s)
        pool.detach(s)
        return out

    out = _replay(rounds, audio, lambda i: pool.attach(c["embs"][i], E.ENROLL_EMBEDDING), pool.push, tick, flush)
    pool.close()
    return out


def _run_emu(eng, c, fade, rounds):
    """the rule restated, on ws_engine_separate of every window alone: one row [1][L] per target with the slot's embedding"""
    tails = {}

    def attach(i):
        sep = lambda x, i=i: np.concatenate([eng.separate(x[None].astype(np.float32), c["embs"][i][k:k + 1], E.ENROLL_EMBEDDING)
                                             for k in range(c["K"])])
        tails[i] = T.Tail(c["K"], c["S"], fade, c["warm"], sep)
        return i

    def push(chunks):
        for i, x in chunks.items():
            tails[i].push(x)

    def tick(named):
        got = {i: tails[i].tick() for i in named}
        return {i: v for i, v in got.items() if v is not None and v.shape[1] > 0}

    out = _replay(rounds, c["audio"], attach, push, tick, lambda i: tails[i].flush())
    return out, [tails[i].blends for i in range(len(c["audio"]))], [tails[i].terms for i in range(len(c["audio"]))]


@pytest.fixture(scope="module", params=sorted(ENGINE_CASES))
def tail_case(request, tmp_path_factory):
    """One engine, three recordings of about three windows attached in rounds 0, 1 and 3 with their own packet cycles, and the rule
    restated on the engine's own ws_engine_separate with fade 128: shared by the tests below."""
    _cuda()
    arch = request.param
    name, kw, _, S, _ = ENGINE_CASES[arch]
    path = str(tmp_path_factory.mktemp("tail") / f"{arch}.wsw")
    export_engine(_model(name, 11, joint_training=False, **kw), path)
    eng = E.Engine(path)
    g = torch.Generator().manual_seed(9)
    K, lens = (2 if arch == "pBSRNN" else 1), (3 * S, 3 * S - 700, 2 * S + 1)
    audio = [(0.1 * torch.randn(m, generator=g)).numpy() for m in lens]
    embs = [torch.randn(K, 256, generator=g).numpy() for _ in lens]
    cycles = CYCLES.get(arch, ((700, 1300, 333), (640,), (900, 1100, 513)))
    c = dict(arch=arch, eng=eng, audio=audio, embs=embs, S=S, K=K, lens=lens, warm=WARM[arch], cycles=cycles)
    c["rounds"], c["fired"] = _schedule(lens, cycles, {0: 0, 1: 1, 2: 3}, S, FADE, c["warm"])
    c["ref"], c["blends"], c["terms"] = _run_emu(eng, c, FADE, c["rounds"])
    yield c
    eng.close()


def test_tail_one_row_per_forward_is_the_rule_on_separate(tail_case):
    c = tail_case
    # the run asserts its own coverage: a tick fired two slots or more, a window shorter than S fired
    assert max(len(f) for f in c["fired"]) >= 2 and any(L < c["S"] for f in c["fired"] for L in f), c["fired"]
    log = []
    got = _run_pool(c["eng"], c, FADE, 1, log=log)
    assert [fw for fw, _, _ in log] == [c["K"] * len(f) for f in c["fired"]]           # one row per forward
    assert [rows for _, rows, _ in log] == [c["K"] * len(f) for f in c["fired"]]
    for i, n in enumerate(c["lens"]):
        ref, mask = c["ref"][i], np.zeros(n, bool)
        for a, b in c["blends"][i]:
            mask[a:b] = True
        assert mask.any() and int(mask.sum()) % FADE == 0          # every slot emitted a non-empty cross-fade
        assert got[i].shape == ref.shape == (c["K"], n)             # exactly n samples per target
        assert np.isfinite(got[i]).all() and np.abs(got[i]).max() > 0
        assert np.array_equal(got[i][:, ~mask].astype(np.float64), ref[:, ~mask]), (c["arch"], i, rel(got[i], ref))
        for t0, hold, v in c["terms"][i]:                           # inside the cross-fades: the bound the three roundings imply
            err = np.abs(got[i][:, t0:t0 + FADE].astype(np.float64) - (hold + T.ramp_of(FADE).astype(np.float64) * (v - hold)))
            assert (err <= BLEND_BOUND * (np.abs(v) + np.abs(hold))).all(), (c["arch"], i, t0, float(err.max()))
    assert c["eng"].info("cluster_fallbacks") == 0


def test_tail_eight_rows_per_forward_against_the_rule(tail_case):
    """Which rows share a forward depends on the other slots: the bound the live-pool tests hold against forwards over other row
    counts."""
    c = tail_case
    got = _run_pool(c["eng"], c, FADE, 8)
    for i, n in enumerate(c["lens"]):
        assert got[i].shape == (c["K"], n) and np.isfinite(got[i]).all() and np.abs(got[i]).max() > 0
        for k in range(c["K"]):
            e = rel(got[i][k], c["ref"][i][k])
            print(f"tail pool {c['arch']} max_rows 8, recording {i}, target {k}: rel {e:.2e} against the rule on ws_engine_separate")
            assert e < 1e-4, (c["arch"], i, k, e)
    assert c["eng"].info("cluster_fallbacks") == 0


def test_tail_three_full_slots_share_one_forward(tail_case):
    c = tail_case
    eng, S, K = c["eng"], c["S"], c["K"]
    pool = eng.tail_pool(3, K, S, FADE, c["warm"], max_rows=8)
    slots = [pool.attach(e, E.ENROLL_EMBEDDING) for e in c["embs"]]
    x = c["audio"][0]
    pool.push({slots[0]: x[:S], slots[1]: x[100:100 + S], slots[2]: x[200:200 + S - 1]})
    pool.push({slots[2]: x[:1]})                                  # other packet sizes, the same tick
    eng.separate(np.stack([x[:S]] * 3 * K), np.concatenate(c["embs"]), E.ENROLL_EMBEDDING)
    n_rect = eng.info("n_launches")
    out = pool.tick()
    assert eng.info("tail_pool_forwards") == 1 and eng.info("tail_pool_rows") == 3 * K
    assert eng.info("n_launches") == E.tail_launches([n_rect])
    assert [out[s].shape for s in slots] == [(K, S - FADE)] * 3
    assert pool.tick() == {} and eng.info("n_launches") == 0     # nothing new: no slot fires
    pool.close()
    assert eng.info("cluster_fallbacks") == 0


def test_tail_fade_zero(tail_case):
    """fade 0: no hold, no cross-fade -- every sample is one window's, bit for bit (one architecture, the one with two targets)"""
    c = tail_case
    if c["arch"] != "pBSRNN":
        return
    rounds, fired = _schedule(c["lens"], c["cycles"], {0: 0, 1: 1, 2: 3}, c["S"], 0, c["warm"])
    ref, blends, _ = _run_emu(c["eng"], c, 0, rounds)
    got = _run_pool(c["eng"], c, 0, 1, rounds=rounds)
    assert not any(blends)
    for i, n in enumerate(c["lens"]):
        assert got[i].shape == (c["K"], n) and np.array_equal(got[i].astype(np.float64), ref[i]), (i, rel(got[i], ref[i]))


def test_tail_slots_do_not_depend_on_what_the_other_slots_carry(tail_case):
    """The same rounds -- so the same rows in every forward -- with recording 1's audio replaced by other data, then by NaN and inf:
    recordings 0 and 2 return the same bits.  Asserted where the rectangular plan keeps its rows apart in every launch
    (Conv-TasNet, pBSRNN); printed for DPCCN and TF-GridNet, as for the live pool (profiles/live_pool.md)."""
    c = tail_case
    g = torch.Generator().manual_seed(77)
    other = (0.3 * torch.randn(c["lens"][1], generator=g)).numpy()
    bad = other.copy()
    bad[::7], bad[3::11] = np.nan, np.inf
    runs = [_run_pool(c["eng"], c, FADE, 8, audio=[c["audio"][0], x1, c["audio"][2]]) for x1 in (c["audio"][1], other, bad)]
    for name, r in (("other data", runs[1]), ("NaN / inf", runs[2])):
        same = all(np.array_equal(r[i], runs[0][i]) for i in (0, 2))
        finite = all(np.isfinite(r[i]).all() for i in (0, 2))
        print(f"tail pool {c['arch']} max_rows 8, recording 1 fed {name}: recordings 0 and 2 {'keep' if same else 'CHANGE'} their bits"
              f"{'' if finite else ' (not finite)'}")
        if c["arch"] in ("ConvTasNet", "pBSRNN"):
            assert same and finite, (c["arch"], name, [rel(r[i], runs[0][i]) for i in (0, 2)])
    assert not np.array_equal(runs[1][1], runs[0][1])


# ---- enroll once ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joint_engine(tmp_path_factory):
    _cuda()
    path = str(tmp_path_factory.mktemp("tailj") / "j.wsw")
    export_engine(_model("BSRNN", 13, num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False, **SPK), path)
    eng = E.Engine(path)
    yield eng, path
    eng.close()


def test_tail_speaker_stage_runs_at_attach_only(joint_engine):
    eng, _ = joint_engine
    g = torch.Generator().manual_seed(29)
    n, S = 5000, 2048
    mix, wave = (0.1 * torch.randn(n, generator=g)).numpy(), (0.1 * torch.randn(2, 20000, generator=g)).numpy()

    def run(enroll, kind):
        pool = eng.tail_pool(2, 2, S, FADE, 1000, max_rows=3)
        s = pool.attach(enroll, kind)
        n_attach, parts, launches = eng.info("n_launches"), [], []
        for p in range(0, n, 700):
            pool.push({s: mix[p:p + 700]})
            parts.append(pool.tick().get(s, np.zeros((2, 0), np.float32)))
            launches.append(eng.info("n_launches"))
        parts.append(pool.flush(s))
        launches.append(eng.info("n_launches"))
        pool.close()
        return np.concatenate(parts, axis=1), launches, n_attach

    a, la, n_wave = run(wave, E.ENROLL_WAVE)
    emb = eng.embed(wave, E.ENROLL_WAVE)
    n_embed = eng.info("n_launches")
    b, lb, n_spk = run(emb, E.ENROLL_SPEAKER)
    assert n_spk == 0 and n_wave == n_embed > 0                  # the encoder's launches appear at attach, once
    assert la == lb and la[0] == 0 and max(la) > 0               # ... and in no tick: the counts are the fixed-embedding ones
    assert a.shape == (2, n) and np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, b)


# ---- separate_main --tail_ms -----------------------------------------------------------------------------------------------
def test_separate_main_tail_writes_what_engine_tail_returns(joint_engine, tmp_path):
    from tests.test_ragged_speaker_gpu import _write_wav
    eng, path = joint_engine
    exe = os.path.join(ROOT, "runtime", "separate_main")
    rng = np.random.default_rng(4)
    lines, data = [], {}
    for i, n in enumerate((5000, 8000, 2048, 1500)):
        m, a, b = rng.integers(-3000, 3000, n), rng.integers(-3000, 3000, 20000 + 1111 * i), rng.integers(-3000, 3000, 30000 - 999 * i)
        for tag, x in (("mix", m), ("a", a), ("b", b)):
            _write_wav(tmp_path / f"{tag}{i}.wav", x)
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
        data[f"u{i}"] = (m, a, b)
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    out = tmp_path / "out"
    out.mkdir()
    # 40 ms packets and 40 ms of warm-up: a line fires at every tick, so no packet is ever cut
    r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out", "--chunk_seconds", "0.128",
                        "--chunk_rows", "1", "--tail_ms", "40", "--tail_fade_ms", "8", "--tail_warm_seconds", "0.04", "--tail_pool", "2"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    f32 = lambda x: (np.asarray(x, np.float32) / np.float32(32768.0)).astype(np.float32)
    for key, (m, a, b) in data.items():
        ne = min(len(a), len(b))
        tail = eng.tail(np.stack([f32(a[:ne]), f32(b[:ne])]), E.ENROLL_WAVE, 2048, 128, warm=640, max_rows=1)
        mix = f32(m)
        parts = [tail.push(mix[p:p + 640]) for p in range(0, len(mix), 640)] + [tail.flush()]
        tail.close()
        want = np.concatenate(parts, axis=1)
        assert want.shape == (2, len(m)) and np.abs(want).max() > 0
        for k in range(2):
            got = np.frombuffer((out / f"{key}-spk{k + 1}.f32").read_bytes(), dtype=np.float32)
            assert np.array_equal(got, want[k]), (key, k, rel(got, want[k]))
