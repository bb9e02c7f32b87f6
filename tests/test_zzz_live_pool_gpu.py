"""GPU: the live pool (runtime/live_pool.cc; ws_window_slots_fwd and ws_xfade_stream_rows_fwd of longform.hip; DESIGN 7 "Live
pool").  The two table-driven kernels bit for bit against their solo forms, row by row; every architecture with three slots
at their own positions against ws_engine_separate_long per slot -- bit for bit with one row per forward, to the rounding of
other row counts otherwise; a slot's bits against what the other slots carry; a flush alone against the whole-utterance call;
enroll once at attach; `separate_main --live_pool` against `--live_ms`."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import emu_live as M
from tests.test_longform_gpu import ENGINE_CASES, SPK, _cuda, _model, rel
from wesep_amd import dev
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
S_, O_, H_, CAP = 48, 16, 32, 4


# ---- kernels ---------------------------------------------------------------------------------------------------------
def _ring_with(windows, L, g, d):
    """one target's ring [CAP][S], NaN but for the first L samples of the slots of `windows`"""
    ring = torch.full((CAP, S_), NAN)
    for w in windows:
        ring[w % CAP, :L] = torch.randn(L, generator=g)
    return ring.to(d)


def test_xfade_stream_rows_is_the_solo_call_row_by_row():
    d = _cuda()
    g = torch.Generator().manual_seed(17)
    # (windows whose estimates the ring holds, their length, the row): mid-recording; a range whose windows wrap the ring,
    # twice -- two targets that share one factor ring; the final end-aligned range of n = 177 = S + 4 H + 1 (its last window
    # overlaps two predecessors); the final short window n = 31 < S; a row with count = 0
    cases = [
        ((0, 1, 2), S_, dict(i0=0, count=64, windows_run=3, final=0), None),
        ((2, 3, 4, 5), S_, dict(i0=96, count=64, windows_run=6, final=0), 0),
        ((3, 4, 5), S_, dict(i0=128, count=49, windows_run=6, final=1, W=6, n=177), 1),
        ((0,), 31, dict(i0=0, count=31, windows_run=1, final=1, W=1, n=31), None),
        ((0, 1, 2), S_, dict(i0=64, count=0, windows_run=3, final=0), None),
        ((2, 3, 4, 5), S_, dict(i0=96, count=64, windows_run=6, final=0), 0),
    ]
    rings = [_ring_with(w, L, g, d) for w, L, _, _ in cases]
    ring = torch.cat([r.reshape(-1) for r in rings])
    scale_ring = (0.5 + torch.rand(2 * CAP, generator=g)).to(d)
    scale_ring[CAP + 2] = NAN                                   # window 2 of the final recording covers nothing of [128, 177)
    out = torch.full((400,), NAN, device=d)
    rows, at = [], 3                                            # an odd first offset: no alignment of out is assumed
    for i, (_, _, r, f) in enumerate(cases):
        rows.append(dict(r, ring_off=i * CAP * S_, scale_off=-1 if f is None else f * CAP, out_off=at))
        at += r["count"] + 5
    dev.xfade_stream_rows_fwd(rows, S_, O_, CAP, ring, out, scale_ring=scale_ring)
    torch.cuda.synchronize()
    written = torch.zeros(400, dtype=torch.bool)
    for i, ((_, _, r, f), row) in enumerate(zip(cases, rows)):
        got = out[row["out_off"]:row["out_off"] + r["count"]]
        written[row["out_off"]:row["out_off"] + r["count"]] = True
        if r["count"] == 0:
            continue
        sc = None if f is None else scale_ring[f * CAP:(f + 1) * CAP]
        solo = torch.full((r["count"],), NAN, device=d)
        dev.xfade_stream_fwd(rings[i].reshape(1, CAP, S_), 1, CAP, S_, O_, r["i0"], r["count"], r["windows_run"], solo, r["count"],
                             final=(r["W"], r["n"]) if r["final"] else None, scale_ring=sc)
        torch.cuda.synchronize()
        assert torch.isfinite(got).all(), i                                      # no NaN slot, sample or factor was read
        assert torch.equal(got, solo), (i, float((got - solo).abs().max()))
        ref = M.xfade_stream(rings[i].double().cpu().numpy().reshape(1, CAP, S_), S_, O_, r["i0"], r["count"], r["windows_run"],
                             (r["W"], r["n"]) if r["final"] else None, None if sc is None else sc.double().cpu().numpy())
        err = float(np.abs(got.double().cpu().numpy() - ref[0]).max())
        print(f"ws_xfade_stream_rows_fwd row {i}: max abs error against the float64 restatement {err:.2e}")
        assert err < 1e-5, (i, err)
    assert torch.isnan(out.cpu()[~written]).all()               # nothing outside the rows' ranges was written


def test_window_slots_is_window_rows_per_slot():
    d = _cuda()
    g = torch.Generator().manual_seed(23)
    # slot 0: n = 200 at an odd source start, its six windows (the end-aligned one starts at 152) with per-window factors;
    # slot 1: n = 177 without factors; slot 2: the short window n = 31 (len % 4 != 0), destination at an odd offset
    lens, bases = (200, 177, 31), (3, 211, 401)
    src = torch.full((450,), NAN)
    xs = []
    for n, b in zip(lens, bases):
        xs.append(torch.randn(n, generator=g))
        src[b:b + n] = xs[-1]
    src = src.to(d)
    fac = 0.5 + torch.rand(6, generator=g)
    rows, want, at = [], [], 0
    for i, (n, b) in enumerate(zip(lens, bases)):
        W, L = M.total_windows(n, S_, H_), min(n, S_)
        ref = torch.full((W, L), NAN, device=d)
        dev.window_rows(xs[i].to(d), n, W, S_, H_, 1, ref, scale=fac[:W].to(d) if i == 0 else None)
        if i == 2:
            at += 1
        for w in range(W):
            rows.append(dict(src_off=b + min(w * H_, max(n - S_, 0)), dst_off=at, len=L, scale=float(fac[w]) if i == 0 else 1.0))
            want.append((at, ref[w]))
            at += L
    dst = torch.full((at + 7,), NAN, device=d)
    dev.window_slots_fwd(rows, src, dst)
    torch.cuda.synchronize()
    written = torch.zeros(at + 7, dtype=torch.bool)
    for o, ref in want:
        assert torch.isfinite(ref).all() and torch.equal(dst[o:o + len(ref)], ref), o
        written[o:o + len(ref)] = True
    assert torch.isnan(dst.cpu()[~written]).all() and int((~written).sum()) == 8


# ---- engines -----------------------------------------------------------------------------------------------------------
def _feed(pool, eng, audio, embs, scheds, late=2, log=None):
    """Slots 0 and 1 are attached at once, recording `late` once slot 0 has run two windows; every push carries the next packet
    of every recording in flight, a recording whose packets are used up is flushed.  -> the concatenated output per recording;
    log: (participants, n_launches, rounds, forwards) per push"""
    S, H = pool.window, pool.window - pool.overlap
    slot, pos, step, parts, out = {}, {}, {}, {}, {}
    waiting = list(range(len(audio)))
    while waiting or slot:
        for i in list(waiting):
            if i != late or pos.get(0, 0) >= S + H or 0 in out:
                slot[i], pos[i], step[i], parts[i] = pool.attach(embs[i], E.ENROLL_EMBEDDING), 0, 0, []
                waiting.remove(i)
        got = pool.push({slot[i]: audio[i][pos[i]:pos[i] + scheds[i][step[i]]] for i in slot})
        if log is not None:
            log.append((len(slot), eng.info("n_launches"), eng.info("live_pool_rounds"), eng.info("live_pool_forwards")))
        for i in list(slot):
            parts[i].append(got[slot[i]])
            pos[i] += scheds[i][step[i]]
            step[i] += 1
            if step[i] == len(scheds[i]):
                parts[i].append(pool.flush(slot[i]))
                out[i] = np.concatenate(parts[i], axis=1)
                pool.detach(slot.pop(i))
    return out


def _cycle(n, sizes):
    out = []
    while sum(out) < n:
        out.append(min(sizes[len(out) % len(sizes)], n - sum(out)))
    return out


@pytest.fixture(scope="module", params=sorted(ENGINE_CASES))
def pool_case(request, tmp_path_factory):
    """One engine, three recordings of n, n - 700 and S + 1 samples with their own enrollments and packet schedules, and
    ws_engine_separate_long of each with 1 and 8 rows per forward: shared by the tests below."""
    _cuda()
    arch = request.param
    name, kw, n, S, O = ENGINE_CASES[arch]
    path = str(tmp_path_factory.mktemp("lpool") / f"{arch}.wsw")
    export_engine(_model(name, 11, joint_training=False, **kw), path)
    eng = E.Engine(path)
    g = torch.Generator().manual_seed(9)
    K, lens = 2, (n, n - 700, S + 1)
    audio = [(0.1 * torch.randn(m, generator=g)).numpy() for m in lens]
    embs = [torch.randn(K, 256, generator=g).numpy() for _ in lens]
    # packets of three sizes in turn, packets of 640, three packets: all three recordings are in flight for a few pushes
    scheds = [_cycle(lens[0], (900, 1100, 513)), _cycle(lens[1], (640,)), [S - 100, 60, 41]]
    long1 = [eng.separate_long(x, e, E.ENROLL_EMBEDDING, S, O, 1) for x, e in zip(audio, embs)]
    long8 = [eng.separate_long(x, e, E.ENROLL_EMBEDDING, S, O, 8) for x, e in zip(audio, embs)]
    yield dict(arch=arch, eng=eng, audio=audio, embs=embs, scheds=scheds, S=S, O=O, K=K, lens=lens, long1=long1, long8=long8)
    eng.close()


def test_pool_one_row_per_forward_is_separate_long_bit_for_bit_per_slot(pool_case):
    c = pool_case
    pool = c["eng"].live_pool(3, c["K"], c["S"], c["O"], max_rows=1)
    log = []
    got = _feed(pool, c["eng"], c["audio"], c["embs"], c["scheds"], log=log)
    pool.close()
    assert max(p for p, _, _, _ in log) == 3                     # all three slots in flight for a while
    for i in range(3):
        assert got[i].shape == (c["K"], c["lens"][i]) and np.isfinite(got[i]).all() and np.abs(got[i]).max() > 0
        assert np.array_equal(got[i], c["long1"][i]), (c["arch"], i, rel(got[i], c["long1"][i]))
    assert c["eng"].info("cluster_fallbacks") == 0


def test_pool_eight_rows_per_forward_against_separate_long_per_slot(pool_case):
    """Which rows share a forward depends on the other slots, so the forwards run over other row counts than
    ws_engine_separate_long's: the bound of test_live_eight_rows_per_forward_against_separate_long."""
    c = pool_case
    pool = c["eng"].live_pool(3, c["K"], c["S"], c["O"], max_rows=8)
    got = _feed(pool, c["eng"], c["audio"], c["embs"], c["scheds"])
    pool.close()
    for i in range(3):
        assert got[i].shape == (c["K"], c["lens"][i]) and np.isfinite(got[i]).all() and np.abs(got[i]).max() > 0
        for k in range(c["K"]):
            e = rel(got[i][k], c["long8"][i][k])
            print(f"live pool {c['arch']} max_rows 8, recording {i}, speaker {k}: rel {e:.2e} against ws_engine_separate_long")
            assert e < 1e-4, (c["arch"], i, k, e)
    assert c["eng"].info("cluster_fallbacks") == 0


@pytest.mark.parametrize("max_rows", [8, 4, 1])
def test_pool_windows_of_three_slots_share_their_forwards(pool_case, max_rows):
    """A push in which all three slots complete a window: one round, ceil(6 / max_rows) forwards, whatever the slots' positions."""
    c = pool_case
    eng, S, H, K = c["eng"], c["S"], c["S"] - c["O"], c["K"]
    pool = eng.live_pool(3, K, S, c["O"], max_rows=max_rows)
    slots = [pool.attach(e, E.ENROLL_EMBEDDING) for e in c["embs"]]
    x = c["audio"][0]
    out = pool.push({slots[0]: x[:S + H - 1], slots[1]: x[:S - 1], slots[2]: x[:S - 1]})        # slot 0 is one window ahead
    assert [v.shape[1] for v in out.values()] == [0, 0, 0] and eng.info("live_pool_rounds") == 1
    out = pool.push({s: x[:1] for s in slots})
    assert eng.info("live_pool_rounds") == 1 and eng.info("live_pool_forwards") == -(-3 * K // max_rows)
    assert [out[s].shape for s in slots] == [(K, H), (K, 0), (K, 0)]
    out = pool.push({s: x[:10] for s in slots})
    assert eng.info("n_launches") == 0 and eng.info("live_pool_rounds") == 0 and eng.info("live_pool_forwards") == 0
    pool.close()
    assert eng.info("cluster_fallbacks") == 0


def test_pool_slots_do_not_depend_on_what_the_other_slots_carry(pool_case):
    """The same schedules -- so the same rows in every forward -- with slot 1's audio replaced by other data, then by NaN and inf:
    slots 0 and 2 return the same bits.  Asserted where the rectangular plan keeps its rows apart in every launch (Conv-TasNet,
    pBSRNN); printed for DPCCN and TF-GridNet (profiles/live_pool.md)."""
    c = pool_case
    g = torch.Generator().manual_seed(77)
    other = (0.3 * torch.randn(c["lens"][1], generator=g)).numpy()
    bad = other.copy()
    bad[::7], bad[3::11] = np.nan, np.inf
    runs = []
    for x1 in (c["audio"][1], other, bad):
        pool = c["eng"].live_pool(3, c["K"], c["S"], c["O"], max_rows=8)
        runs.append(_feed(pool, c["eng"], [c["audio"][0], x1, c["audio"][2]], c["embs"], c["scheds"]))
        pool.close()
    for name, r in (("other data", runs[1]), ("NaN / inf", runs[2])):
        same = all(np.array_equal(r[i], runs[0][i]) for i in (0, 2))
        finite = all(np.isfinite(r[i]).all() for i in (0, 2))
        print(f"live pool {c['arch']} max_rows 8, slot 1 fed {name}: slots 0 and 2 {'keep' if same else 'CHANGE'} their bits"
              f"{'' if finite else ' (not finite)'}")
        if c["arch"] in ("ConvTasNet", "pBSRNN"):
            assert same and finite, (c["arch"], name, [rel(r[i], runs[0][i]) for i in (0, 2)])
    assert not np.array_equal(runs[1][1], runs[0][1])


def test_pool_flush_alone_is_the_whole_utterance_call(pool_case):
    c = pool_case
    pool = c["eng"].live_pool(2, c["K"], c["S"], c["O"], max_rows=8)
    busy = pool.attach(c["embs"][1], E.ENROLL_EMBEDDING)
    pool.push({busy: c["audio"][1][:c["S"] + 10]})                    # another slot in mid-recording
    for n in (c["S"], c["S"] - 40):
        mix = c["audio"][0][:n]
        s = pool.attach(c["embs"][0], E.ENROLL_EMBEDDING)
        first = pool.push({s: mix})[s]
        got = np.concatenate([first, pool.flush(s)], axis=1)
        pool.detach(s)
        want = c["eng"].separate(np.stack([mix] * c["K"]), c["embs"][0], E.ENROLL_EMBEDDING)
        assert first.shape[1] == 0 and np.abs(want).max() > 0 and np.array_equal(got, want), (c["arch"], n)
    pool.close()


# ---- enroll once ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joint_engine(tmp_path_factory):
    _cuda()
    path = str(tmp_path_factory.mktemp("lpoolj") / "j.wsw")
    export_engine(_model("BSRNN", 13, num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False, **SPK), path)
    eng = E.Engine(path)
    yield eng, path
    eng.close()


def test_pool_speaker_stage_runs_at_attach_only(joint_engine):
    eng, _ = joint_engine
    g = torch.Generator().manual_seed(29)
    n, S, O = 6000, 2048, 512
    mix, wave = (0.1 * torch.randn(n, generator=g)).numpy(), (0.1 * torch.randn(2, 20000, generator=g)).numpy()
    sched = M.schedules(n, 2)["random"]

    def run(enroll, kind):
        pool = eng.live_pool(2, 2, S, O, max_rows=3)
        s = pool.attach(enroll, kind)
        n_attach, parts, launches, N = eng.info("n_launches"), [], [], 0
        for c in sched:
            parts.append(pool.push({s: mix[N:N + c]})[s])
            launches.append(eng.info("n_launches"))
            N += c
        parts.append(pool.flush(s))
        launches.append(eng.info("n_launches"))
        pool.close()
        return np.concatenate(parts, axis=1), launches, n_attach

    a, la, n_wave = run(wave, E.ENROLL_WAVE)
    emb = eng.embed(wave, E.ENROLL_WAVE)
    n_embed = eng.info("n_launches")
    b, lb, n_spk = run(emb, E.ENROLL_SPEAKER)
    assert n_spk == 0 and n_wave == n_embed > 0                  # the encoder's launches appear at attach, once
    assert la == lb                                              # ... and in no push
    assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, b)
    e = rel(a, eng.separate_long(mix, wave, E.ENROLL_WAVE, S, O, 3))
    print(f"live pool joint pBSRNN max_rows 3 against ws_engine_separate_long: rel {e:.2e}")
    assert e < 1e-4


# ---- separate_main --live_pool ---------------------------------------------------------------------------------------------
def test_separate_main_live_pool_writes_the_files_of_the_live_run(joint_engine, tmp_path):
    from tests.test_ragged_speaker_gpu import _write_wav
    _, path = joint_engine
    exe = os.path.join(ROOT, "runtime", "separate_main")
    rng = np.random.default_rng(4)
    lines = []
    for i, n in enumerate((5000, 8000, 2048, 1500)):
        m, a, b = rng.integers(-3000, 3000, n), rng.integers(-3000, 3000, 20000 + 1111 * i), rng.integers(-3000, 3000, 30000 - 999 * i)
        for tag, x in (("mix", m), ("a", a), ("b", b)):
            _write_wav(tmp_path / f"{tag}{i}.wav", x)
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    chunk = ["--chunk_seconds", "0.128", "--overlap_seconds", "0.032", "--chunk_rows", "1", "--live_ms", "100"]
    outs = {}
    for tag, extra in (("live", []), ("pool", ["--live_pool", "2"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out"] + chunk + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        outs[tag] = out
    names = sorted(os.listdir(outs["live"]))
    assert names == sorted(os.listdir(outs["pool"])) and len(names) == 16           # the same files, by name
    for name in names:
        a, b = (outs["live"] / name).read_bytes(), (outs["pool"] / name).read_bytes()
        if name.endswith(".f32"):
            assert np.abs(np.frombuffer(a, dtype=np.float32)).max() > 0
        assert a == b, name
