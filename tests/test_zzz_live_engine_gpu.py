"""GPU: live windows in the native runtime (runtime/live.cc).  Every architecture fed packets of any size
against ws_engine_separate_long on the concatenated input -- bit for bit with one row per forward, to the rounding of other
row counts otherwise; a flush alone against the whole-utterance call; enroll once; other engine calls between two pushes;
`separate_main --live_ms` against `--chunk_seconds`."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import emu_live as M
from tests.test_longform_gpu import ENGINE_CASES, SPK, _cuda, _model, rel
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _feed(lv, mix, sched):
    """the concatenation of every push and the flush; the launches of every call"""
    eng, parts, launches, N = lv._engine, [], [], 0
    for c in sched:
        parts.append(lv.push(mix[N:N + c]))
        launches.append(eng.info("n_launches"))
        N += c
    parts.append(lv.flush())
    launches.append(eng.info("n_launches"))
    return np.concatenate(parts, axis=1), launches


@pytest.fixture(scope="module", params=sorted(ENGINE_CASES))
def live_case(request, tmp_path_factory):
    """One engine, one recording, its ws_engine_separate_long with 1 and 8 rows per forward: shared by the tests below."""
    _cuda()
    arch = request.param
    name, kw, n, S, O = ENGINE_CASES[arch]
    path = str(tmp_path_factory.mktemp("live") / f"{arch}.wsw")
    export_engine(_model(name, 11, joint_training=False, **kw), path)
    eng = E.Engine(path)
    g = torch.Generator().manual_seed(5)
    K = 2
    mix, emb = (0.1 * torch.randn(n, generator=g)).numpy(), torch.randn(K, 256, generator=g).numpy()
    long1 = eng.separate_long(mix, emb, E.ENROLL_EMBEDDING, S, O, 1)
    long8 = eng.separate_long(mix, emb, E.ENROLL_EMBEDDING, S, O, 8)
    yield dict(arch=arch, eng=eng, mix=mix, emb=emb, n=n, S=S, O=O, K=K, long1=long1, long8=long8, sched=M.schedules(n, 7))
    eng.close()


@pytest.mark.parametrize("sched", ["160", "random", "whole"])
def test_live_one_row_per_forward_is_separate_long_bit_for_bit(live_case, sched):
    c = live_case
    lv = c["eng"].live(c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], max_rows=1)
    got, _ = _feed(lv, c["mix"], c["sched"][sched])
    assert c["eng"].info("live_windows") == len(E.long_windows(c["n"], c["S"], c["O"]))
    lv.close()
    assert got.shape == (c["K"], c["n"]) and np.isfinite(got).all() and np.abs(got).max() > 0
    assert np.array_equal(got, c["long1"]), (c["arch"], sched, rel(got, c["long1"]))


@pytest.mark.parametrize("sched", ["160", "random", "whole"])
def test_live_eight_rows_per_forward_against_separate_long(live_case, sched):
    """Groups form differently (a live group holds whole windows of both targets), so the forwards run over other row counts:
    the bound test_engine_separate_long_group_size_does_not_matter uses for the same cause."""
    c = live_case
    lv = c["eng"].live(c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], max_rows=8)
    got, _ = _feed(lv, c["mix"], c["sched"][sched])
    lv.close()
    assert got.shape == (c["K"], c["n"]) and np.isfinite(got).all() and np.abs(got).max() > 0
    for k in range(c["K"]):
        e = rel(got[k], c["long8"][k])
        print(f"live {c['arch']} max_rows 8, packets {sched}, speaker {k}: rel {e:.2e} against ws_engine_separate_long")
        assert e < 1e-4, (c["arch"], sched, k, e)


@pytest.mark.parametrize("K,max_rows", [(1, 4), (3, 2)], ids=["one-target-groups-of-4", "three-targets-two-rows"])
def test_live_other_group_shapes_against_separate_long(live_case, K, max_rows):
    """K = 1, max_rows = 4: one forward writes up to four consecutive ring slots itself, and the ring of 7 wraps.  K = 3,
    max_rows = 2: a window's rows go in two forwards, then one strided copy into the ring.  Forwards over other row counts
    than ws_engine_separate_long's: the bound of the test above."""
    c = live_case
    g = torch.Generator().manual_seed(31 * K + max_rows)
    mix = np.concatenate([c["mix"], 0.5 * c["mix"][::-1], c["mix"], c["mix"][: c["n"] // 2]])          # 10 - 14 windows
    emb = torch.randn(K, 256, generator=g).numpy()
    want = c["eng"].separate_long(mix, emb, E.ENROLL_EMBEDDING, c["S"], c["O"], max_rows)
    W = len(E.long_windows(len(mix), c["S"], c["O"]))
    assert W > max(1, max_rows // K) + 3 and np.abs(want).max() > 0
    for name, sched in (("whole", [len(mix)]), ("random", M.schedules(len(mix), 9)["random"])):
        lv = c["eng"].live(emb, E.ENROLL_EMBEDDING, c["S"], c["O"], max_rows=max_rows)
        got, _ = _feed(lv, mix, sched)
        lv.close()
        assert got.shape == want.shape and np.isfinite(got).all()
        for k in range(K):
            e = rel(got[k], want[k])
            print(f"live {c['arch']} K {K} max_rows {max_rows}, packets {name}, speaker {k}: rel {e:.2e} against ws_engine_separate_long")
            assert e < 1e-4, (c["arch"], K, max_rows, name, k, e)


def test_live_flush_alone_is_the_whole_utterance_call(live_case):
    c = live_case
    for n in (c["S"], c["S"] - 40):
        mix = c["mix"][:n]
        lv = c["eng"].live(c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], max_rows=8)
        first = lv.push(mix)
        got = np.concatenate([first, lv.flush()], axis=1)
        lv.close()
        want = c["eng"].separate(np.stack([mix] * c["K"]), c["emb"], E.ENROLL_EMBEDDING)
        assert first.shape[1] == 0 and np.abs(want).max() > 0 and np.array_equal(got, want), (c["arch"], n)


def test_other_engine_calls_between_pushes_do_not_disturb_a_live_handle(live_case):
    c = live_case
    eng, sched = c["eng"], c["sched"]["random"]
    lv = eng.live(c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], max_rows=1)
    parts, N = [], 0
    for i, p in enumerate(sched):
        parts.append(lv.push(c["mix"][N:N + p]))
        N += p
        if i % 2 == 0:
            eng.separate(c["mix"][None, :c["S"]], c["emb"][:1], E.ENROLL_EMBEDDING)
        else:
            eng.separate_long(c["mix"][:c["S"] + 100], c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], 2)
    parts.append(lv.flush())
    assert np.array_equal(np.concatenate(parts, axis=1), c["long1"]), c["arch"]
    lv.reset()                                                   # the same packets again: the same bits
    again, _ = _feed(lv, c["mix"], sched)
    lv.close()
    assert np.array_equal(again, c["long1"]), c["arch"]


# ---- enroll once ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joint_engine(tmp_path_factory):
    _cuda()
    path = str(tmp_path_factory.mktemp("livej") / "j.wsw")
    export_engine(_model("BSRNN", 13, num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False, **SPK), path)
    eng = E.Engine(path)
    yield eng, path
    eng.close()


def test_live_speaker_stage_runs_at_open_only(joint_engine):
    eng, _ = joint_engine
    g = torch.Generator().manual_seed(29)
    n, S, O = 6000, 2048, 512
    mix, wave = (0.1 * torch.randn(n, generator=g)).numpy(), (0.1 * torch.randn(2, 20000, generator=g)).numpy()
    sched = M.schedules(n, 2)["random"]
    lv = eng.live(wave, E.ENROLL_WAVE, S, O, max_rows=3)
    n_open = eng.info("n_launches")
    a, la = _feed(lv, mix, sched)
    lv.close()
    emb = eng.embed(wave, E.ENROLL_WAVE)
    n_embed = eng.info("n_launches")
    lv = eng.live(emb, E.ENROLL_SPEAKER, S, O, max_rows=3)
    assert eng.info("n_launches") == 0 and n_open == n_embed > 0          # the encoder's launches appear at open, once
    b, lb = _feed(lv, mix, sched)
    lv.close()
    assert la == lb                                                        # ... and in no push
    assert np.isfinite(a).all() and np.abs(a).max() > 0 and np.array_equal(a, b)
    want = eng.separate_long(mix, wave, E.ENROLL_WAVE, S, O, 3)
    e = rel(a, want)
    print(f"live joint pBSRNN max_rows 3 against ws_engine_separate_long: rel {e:.2e}")
    assert e < 1e-4


# ---- separate_main --live_ms ---------------------------------------------------------------------------------------------
def test_separate_main_live_writes_the_files_of_the_chunked_run(joint_engine, tmp_path):
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
    chunk = ["--chunk_seconds", "0.128", "--overlap_seconds", "0.032", "--chunk_rows", "1"]
    outs = {}
    for tag, extra in (("chunked", []), ("live", ["--live_ms", "100"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out"] + chunk + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        outs[tag] = out
    names = sorted(os.listdir(outs["chunked"]))
    assert names == sorted(os.listdir(outs["live"])) and len(names) == 16           # the same files, by name
    for name in names:
        if name.endswith(".f32"):
            a, b = np.fromfile(outs["chunked"] / name, dtype=np.float32), np.fromfile(outs["live"] / name, dtype=np.float32)
            assert np.abs(a).max() > 0 and np.array_equal(a, b), name
