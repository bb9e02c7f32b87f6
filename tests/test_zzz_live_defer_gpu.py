"""GPU: the live pool's store / run / due (runtime/live_pool.cc; include/wesep_engine.h "STORE, RUN, DUE"; DESIGN 7 "Live pool").
Every architecture with three staggered recordings fed by store and run on a hold: bit for bit ws_engine_separate_long with one
row per forward; bit for bit the push-driven pool when run follows every store (the same rows in the same forwards); fuller
forwards and the same answer to the rounding of other row counts with a hold; a final entry beside other slots' windows; a
slot's bits against what the other slots carry; `separate_main --live_pool N --live_hold_ms W` against `--live_pool N`."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_longform_gpu import rel
from tests.test_zzz_live_pool_gpu import joint_engine, pool_case  # noqa: F401  (fixtures: the engines, recordings and references)
from wesep_amd import engine as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATE = 3                                  # the packet round at which the third recording starts


def _session(c, how, max_rows, audio=None):
    """The three recordings of the case through one pool of three slots: recordings 0 and 1 from round 0, recording 2 from round
    LATE; every round gives each recording in flight its next packet.
      push       pool.push(packets); a recording that has ended is flushed
      store_run  pool.store(packets), pool.run(the slots of the packets); a recording that has ended: run([slot], final=[slot])
      hold       pool.store(packets); a run only when due() reports oldest_age >= H / 2 or a recording has ended -- the ended
                 ones are final in that run, beside the other slots' windows
    -> (the concatenated output per recording, (rounds, forwards) of every call that launched, windows waiting at each hold run)"""
    eng, S, H = c["eng"], c["S"], c["S"] - c["O"]
    audio = c["audio"] if audio is None else audio
    pool = eng.live_pool(3, c["K"], S, c["O"], max_rows=max_rows)
    slot, pos, step, parts, out, log, waited = {}, {}, {}, {}, {}, [], []
    note = lambda: log.append((eng.info("live_pool_rounds"), eng.info("live_pool_forwards"))) if eng.info("live_pool_rounds") else None
    t = 0
    while len(out) < 3:
        for i in range(3):
            if i not in slot and i not in out and t >= (LATE if i == 2 else 0):
                slot[i], pos[i], step[i], parts[i] = pool.attach(c["embs"][i], E.ENROLL_EMBEDDING), 0, 0, []
        feeding = [i for i in slot if step[i] < len(c["scheds"][i])]
        chunks = {slot[i]: audio[i][pos[i]:pos[i] + c["scheds"][i][step[i]]] for i in feeding}
        for i in feeding:
            pos[i] += c["scheds"][i][step[i]]
            step[i] += 1
        ended = [i for i in slot if step[i] == len(c["scheds"][i])]
        if how == "push":
            got = pool.push(chunks)
            note()
            for i in feeding:
                parts[i].append(got[slot[i]])
            for i in ended:
                parts[i].append(pool.flush(slot[i]))
                note()
        elif how == "store_run":
            pool.store(chunks)
            assert eng.info("n_launches") == 0
            got = pool.run(list(chunks))
            note()
            for i in feeding:
                parts[i].append(got[slot[i]])
            for i in ended:
                parts[i].append(pool.run([slot[i]], final=[slot[i]])[slot[i]])
                note()
        else:
            if chunks:
                pool.store(chunks)
            rows, age = pool.due()
            if ended or age >= H // 2:
                waited.append(rows // c["K"])
                got = pool.run(final=[slot[i] for i in ended])
                note()
                for i in slot:
                    if slot[i] in got:
                        parts[i].append(got[slot[i]])
        for i in ended:
            out[i] = np.concatenate(parts[i], axis=1)
            pool.detach(slot.pop(i))
        t += 1
    pool.close()
    return out, log, waited


@pytest.fixture(scope="module")
def defer_case(pool_case):
    """pool_case with its sessions computed once per (driver, max_rows) and shared by the tests below"""
    cache = {}

    def session(how, max_rows):
        if (how, max_rows) not in cache:
            cache[(how, max_rows)] = _session(pool_case, how, max_rows)
        return cache[(how, max_rows)]

    return dict(pool_case, session=session)


def test_held_runs_one_row_per_forward_are_separate_long_bit_for_bit(defer_case):
    c = defer_case
    got, log, waited = c["session"]("hold", 1)
    assert max(waited) >= 2                                      # a run that found windows of several slots waiting
    for i in range(3):
        assert got[i].shape == (c["K"], c["lens"][i]) and np.isfinite(got[i]).all() and np.abs(got[i]).max() > 0
        assert np.array_equal(got[i], c["long1"][i]), (c["arch"], i, rel(got[i], c["long1"][i]))
    assert c["eng"].info("cluster_fallbacks") == 0


def test_store_then_run_is_push_bit_for_bit_with_eight_rows(defer_case):
    """run after every store names the slots of the packets: the rows of every forward are those of the push, so are the bits."""
    c = defer_case
    a, la, _ = c["session"]("push", 8)
    b, lb, _ = c["session"]("store_run", 8)
    assert la == lb and len(la) > 3
    for i in range(3):
        assert np.abs(a[i]).max() > 0 and np.array_equal(a[i], b[i]), (c["arch"], i, rel(b[i], a[i]))


def test_held_runs_fill_the_forwards_and_give_the_same_answer(defer_case):
    """The bound of test_pool_eight_rows_per_forward_against_separate_long_per_slot: forwards over other row counts."""
    c = defer_case
    got, log, waited = c["session"]("hold", 8)
    _, twin, _ = c["session"]("push", 8)
    for i in range(3):
        assert got[i].shape == (c["K"], c["lens"][i]) and np.isfinite(got[i]).all() and np.abs(got[i]).max() > 0
        for k in range(c["K"]):
            e = rel(got[i][k], c["long8"][i][k])
            print(f"live pool on a hold, {c['arch']} max_rows 8, recording {i}, speaker {k}: rel {e:.2e} against ws_engine_separate_long")
            assert e < 1e-4, (c["arch"], i, k, e)
    held, pushed = sum(f for _, f in log), sum(f for _, f in twin)
    print(f"live pool {c['arch']} max_rows 8: {held} forwards in {len(log)} held runs, {pushed} in {len(twin)} pushes and flushes")
    assert held < pushed and max(waited) >= 2
    assert c["eng"].info("cluster_fallbacks") == 0


def test_final_entry_shares_the_round_of_the_other_slots(pool_case):
    c = pool_case
    eng, S, H, K = c["eng"], c["S"], c["S"] - c["O"], c["K"]
    a0, a1, a2 = c["audio"]                                       # a2 has S + 1 samples: its last window is end-aligned at 1
    for max_rows in (1, 8):
        held, twin = eng.live_pool(3, K, S, c["O"], max_rows=max_rows), eng.live_pool(3, K, S, c["O"], max_rows=max_rows)
        for pool in (held, twin):
            assert [pool.attach(e, E.ENROLL_EMBEDDING) for e in c["embs"]] == [0, 1, 2]
        first = {0: a0[:S], 1: a1[:S + 5], 2: a2}
        held.store(first)
        assert held.due() == (3 * K, 5)
        got = [held.run()]
        assert (eng.info("live_pool_rounds"), eng.info("live_pool_forwards")) == (1, -(-3 * K // max_rows))
        second = {0: a0[S:S + H], 1: a1[S + 5:S + H]}
        held.store(second)
        assert held.due() == (2 * K, 0)
        got.append(held.run(final=[2]))                          # two regular windows and slot 2's last one: one round, one chain
        assert (eng.info("live_pool_rounds"), eng.info("live_pool_forwards")) == (1, -(-3 * K // max_rows)), (c["arch"], max_rows)
        want = [twin.push(first), twin.push(second)]
        tail = twin.flush(2)
        assert (eng.info("live_pool_rounds"), eng.info("live_pool_forwards")) == (1, -(-K // max_rows))      # ... a round of its own
        ended = np.concatenate([got[0][2], got[1][2]], axis=1)
        ref = np.concatenate([want[0][2], tail], axis=1)
        assert ended.shape == (K, S + 1) and np.abs(ended).max() > 0
        if max_rows == 1:                                        # one row per forward: whatever shares the round, the same bits
            assert np.array_equal(ended, ref) and np.array_equal(ended, c["long1"][2]), (c["arch"], rel(ended, ref))
            assert all(np.array_equal(got[j][s], want[j][s]) for j in (0, 1) for s in (0, 1))
        else:
            assert rel(ended, ref) < 1e-4, (c["arch"], rel(ended, ref))
        with pytest.raises(E.WesepHipError, match="ws_engine_live_pool_store: slot 2 .entry 0. was flushed"):
            held.store({2: a2[:10]})
        # a short recording (n < S) ended by `final` beside two regular windows: forwards of its own rows, the whole-utterance call's bits
        held.close()
        held = eng.live_pool(3, K, S, c["O"], max_rows=max_rows)
        assert [held.attach(e, E.ENROLL_EMBEDDING) for e in c["embs"]] == [0, 1, 2]
        mix, s = a2[:S - 40], 2
        held.store({0: a0[:S - 7], 1: a1[:S], s: mix[:100]})
        held.store({0: a0[S - 7:S], s: mix[100:]})
        out = held.run(final=[s])
        assert (eng.info("live_pool_rounds"), eng.info("live_pool_forwards")) == (1, -(-2 * K // max_rows) + -(-K // max_rows))
        if K <= max_rows:
            whole = eng.separate(np.stack([mix] * K), c["embs"][2], E.ENROLL_EMBEDDING)
            assert np.abs(whole).max() > 0 and np.array_equal(out[s], whole), (c["arch"], max_rows, rel(out[s], whole))
        assert out[0].shape == out[1].shape == (K, 0) and out[s].shape == (K, S - 40) and np.isfinite(out[s]).all()
        held.close()
        twin.close()
    assert eng.info("cluster_fallbacks") == 0


def test_held_slots_do_not_depend_on_what_the_other_slots_carry(defer_case):
    """test_pool_slots_do_not_depend_on_what_the_other_slots_carry through store / run: the schedule -- so the rows of every
    forward -- is fixed, slot 1's audio is replaced by other data, then by NaN and inf.  Asserted where the rectangular plan keeps
    its rows apart in every launch (Conv-TasNet, pBSRNN); printed for DPCCN and TF-GridNet."""
    import torch
    c = defer_case
    g = torch.Generator().manual_seed(77)
    other = (0.3 * torch.randn(c["lens"][1], generator=g)).numpy()
    bad = other.copy()
    bad[::7], bad[3::11] = np.nan, np.inf
    base = c["session"]("hold", 8)[0]
    for name, x1 in (("other data", other), ("NaN / inf", bad)):
        r = _session(c, "hold", 8, audio=[c["audio"][0], x1, c["audio"][2]])[0]
        same = all(np.array_equal(r[i], base[i]) for i in (0, 2))
        finite = all(np.isfinite(r[i]).all() for i in (0, 2))
        print(f"live pool on a hold, {c['arch']} max_rows 8, slot 1 fed {name}: slots 0 and 2 {'keep' if same else 'CHANGE'} their bits"
              f"{'' if finite else ' (not finite)'}")
        if c["arch"] in ("ConvTasNet", "pBSRNN"):
            assert same and finite, (c["arch"], name, [rel(r[i], base[i]) for i in (0, 2)])
        assert not np.array_equal(r[1], base[1])


# ---- separate_main --live_pool N --live_hold_ms W ----------------------------------------------------------------------------
def test_separate_main_live_hold_writes_the_files_of_the_live_pool_run(joint_engine, tmp_path):
    from tests.test_ragged_speaker_gpu import _write_wav
    _, path = joint_engine
    exe = os.path.join(ROOT, "runtime", "separate_main")
    rng = np.random.default_rng(4)
    lines = []
    for i, n in enumerate((5000, 8000, 2048, 1500, 6100)):
        m, a, b = rng.integers(-3000, 3000, n), rng.integers(-3000, 3000, 20000 + 1111 * i), rng.integers(-3000, 3000, 30000 - 999 * i)
        for tag, x in (("mix", m), ("a", a), ("b", b)):
            _write_wav(tmp_path / f"{tag}{i}.wav", x)
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    chunk = ["--chunk_seconds", "0.128", "--overlap_seconds", "0.032", "--live_ms", "20", "--live_pool", "2"]      # hop 96 ms
    outs, forwards = {}, {}
    for rows in ("1", "4"):
        for tag, extra in (("pool", []), ("hold", ["--live_hold_ms", "96"])):
            out = tmp_path / (tag + rows)
            out.mkdir()
            r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out", "--chunk_rows", rows]
                               + chunk + extra, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr + r.stdout
            outs[tag + rows] = out
            forwards[tag + rows] = int([l for l in r.stdout.splitlines() if l.startswith("live pool:")][0].split()[6])
    print("separate_main forwards:", forwards)
    assert forwards["hold4"] < forwards["pool4"]
    names = sorted(os.listdir(outs["pool1"]))
    assert len(names) == 20 and all(sorted(os.listdir(o)) == names for o in outs.values())
    for name in names:
        a, b = (outs["pool1"] / name).read_bytes(), (outs["hold1"] / name).read_bytes()
        assert a == b, name                                      # one row per forward: bit-identical files
        if name.endswith(".f32"):
            x, y = (np.frombuffer((outs[t] / name).read_bytes(), dtype=np.float32) for t in ("pool4", "hold4"))
            assert np.abs(x).max() > 0 and x.shape == y.shape and rel(y, x) < 1e-4, (name, rel(y, x))
