"""CPU: ragged batches (per-row lengths through the pBSRNN forward) without a GPU -- the new C-ABI symbols and their
argument contracts in the built libraries, the engine's dry run of ws_engine_separate_ragged through the real
libwesep_hip.so validation, `separate_main --batch`, and the host logic (length -> frame tables, packing of rows, the
per-row peak normalisation, the refusals of the Python surface) against plain numpy."""
import ctypes
import os
import re
import subprocess
import wave

import numpy as np
import pytest
import torch

from wesep_amd import _lib as L
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
SPK = dict(joint_training=True, spk_feat=True,
           spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False))
FIXED = dict(num_repeat=2, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False)
NEW_SYMBOLS = ("ws_stft_bandsplit_len", "ws_group_stats_len", "ws_gemm_p2b_len", "ws_istft_ola_len")


def _model(**kw):
    from wesep_amd.models import get_model
    return get_model("BSRNN")(**kw)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_length_aware_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name      # the binding has the declared arity
        assert getattr(lib, name) is not None
        # the rectangular entry point it extends keeps its declaration and binding
        assert name[:-4] in L._SIGS and re.search(r"^int\s+" + name[:-4] + r"\s*\(", header, flags=re.M)
    # the engine: new entry point, new ABI number on both sides
    eh = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    assert re.search(r"int\s+ws_engine_separate_ragged\s*\(\s*ws_engine\*\s*e,\s*const float\*\s*mix,\s*int R,\s*int T,\s*"
                     r"const int\*\s*lengths,\s*const void\*\s*enroll,\s*int enroll_kind,\s*int enroll_len,\s*"
                     r"const int\*\s*enroll_lengths,\s*float\*\s*est\)", eh)
    assert "ws_engine_separate_ragged" in E.SYMBOLS and hasattr(ctypes.CDLL(E.LIB_PATH), "ws_engine_separate_ragged")
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


def test_length_aware_entry_points_refuse_bad_arguments_before_any_launch():
    """WS_ERR_INVALID comes from the host-side checks, which run without a device.  The length TABLES are device memory
    and are checked where the lengths are host values (the engine, dev.ragged_tables); a missing table is refused here."""
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    ib = (ctypes.c_int * 64)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ib, ctypes.c_void_p)
    err = lambda: lib.ws_last_error().decode()
    geo = L.GroupsGeom()
    geo.gs1, geo.rs, geo.ngroups, geo.gdiv, geo.L, geo.W, geo.nbands = 512, 128, 2, 1, 4, 128, 1
    assert lib.ws_group_stats_len(p, ctypes.byref(geo), None, 1, 1e-7, p, None) == -1 and "ws_group_stats_len" in err()
    assert lib.ws_group_stats_len(p, ctypes.byref(geo), ip, 0, 1e-7, p, None) == -1
    bad_geo = L.GroupsGeom()
    assert lib.ws_group_stats_len(p, ctypes.byref(bad_geo), ip, 1, 1e-7, p, None) == -1 and "bad geometry" in err()
    a = L.GemmP2BArgs()
    a.A, a.Wpack, a.C = p, p, p
    a.sm.nseq, a.sm.sq_div, a.sm.L, a.sm.sq_s2 = 32, 1 << 30, 4, 4
    a.lda, a.N, a.K = 128, 64, 128
    assert lib.ws_gemm_p2b_len(ctypes.byref(a), None, 1, None) == -1 and "steps" in err()
    assert lib.ws_gemm_p2b_len(ctypes.byref(a), ip, 0, None) == -1
    a.K = 64                                                  # the checks of ws_gemm_p2b hold for the _len form, under its name
    assert lib.ws_gemm_p2b_len(ctypes.byref(a), ip, 1, None) == -1 and "ws_gemm_p2b_len: K must be 128" in err()
    assert lib.ws_gemm_p2b(ctypes.byref(a), None) == -1 and "ws_gemm_p2b: K must be 128" in err()
    bands = L.Bands()
    bands.band_of_bin, bands.band_f0, bands.band_bw, bands.nband, bands.nbins = ip, ip, ip, 32, 257
    assert lib.ws_stft_bandsplit_len(p, 2, 256, ip, ctypes.byref(bands), p, None) == -1        # T <= win / 2, as before
    assert "ws_stft_bandsplit_len: T=256 must exceed the reflect pad 256" in err()
    assert lib.ws_stft_bandsplit(p, 2, 256, ctypes.byref(bands), p, None) == -1
    assert "ws_stft_bandsplit: T=256 must exceed the reflect pad 256" in err()                # the message it always gave
    assert lib.ws_istft_ola_len(p, 2, 5, 4000, ip, p, None) == -1 and "ws_istft_ola_len: Tf=5 does not match T=4000" in err()
    assert lib.ws_istft_ola(p, 2, 5, 4000, p, None) == -1 and "ws_istft_ola: Tf=5 does not match T=4000" in err()


# ---- the engine's dry run ---------------------------------------------------------------------------------------------
@needs_no_gpu
def test_dry_run_separate_ragged_fixed_embeddings(tmp_path):
    path = str(tmp_path / "m.wsw")
    export_engine(_model(joint_training=False, **FIXED), path)
    eng = E.Engine(path, dry_run=True)
    rng = np.random.default_rng(0)
    emb = [np.zeros(256, np.float32)] * 4
    counts = set()
    for lengths in ((16000, 12345, 4096, 9999), (16000, 16000, 16000, 16000), (16000, 512, 513, 640), (16000, 15999, 8000, 700)):
        est = eng.separate_ragged([rng.standard_normal(n).astype(np.float32) for n in lengths], emb, E.ENROLL_EMBEDDING)
        assert [len(x) for x in est] == list(lengths) and not any(x.any() for x in est)       # a dry run computes nothing
        counts.add(eng.info("n_launches"))
    assert len(counts) == 1, counts                      # for fixed (R, T) the plan does not depend on the lengths
    # odd R and the geometry whose time view has nseq % 64 != 0 (R = 3: 96 sequences, the streaming branch)
    eng.separate_ragged([np.zeros(n, np.float32) for n in (4096, 3000, 2048)], emb[:3], E.ENROLL_EMBEDDING)
    eng.separate_ragged([np.zeros(777, np.float32)], emb[:1], E.ENROLL_EMBEDDING)
    # lengths = NULL is ws_engine_separate: same validation, same plan
    R, T = 2, 12345
    mix, e2, est = np.zeros((R, T), np.float32), np.zeros((R, 256), np.float32), np.zeros((R, T), np.float32)

    def call(lengths, T=T):
        ln = None if lengths is None else np.asarray(lengths, np.int32)          # (kept alive across the call)
        return E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, R, T, None if ln is None else ln.ctypes.data,
                                                 e2.ctypes.data, E.ENROLL_EMBEDDING, 0, None, est.ctypes.data)

    assert call(None) == 0
    n_null = eng.info("n_launches")
    eng.separate(mix, e2, E.ENROLL_EMBEDDING)
    assert eng.info("n_launches") == n_null
    assert call(None, T=300) == -1 and "T >= 512" in E.lib().ws_engine_last_error().decode()
    # lengths below what the surface demands of T, above the row pitch: WS_ERR_INVALID, naming row and value
    for bad in ((12345, 256), (12345, 511), (12346, 4000), (0, 4000), (-5, 4000)):
        assert call(bad) == -1, bad
        assert "lengths[" in E.lib().ws_engine_last_error().decode()
    assert call((512, 12345)) == 0
    # enroll_lengths make no sense for fixed embeddings
    el = np.array([10, 10], np.int32)
    assert E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, R, T, None, e2.ctypes.data, E.ENROLL_EMBEDDING, 0,
                                             el.ctypes.data, est.ctypes.data) == -1
    with pytest.raises(ValueError, match="one enrollment per mixture row"):
        eng.separate_ragged([np.zeros(4000, np.float32)] * 2, emb[:1], E.ENROLL_EMBEDDING)
    eng.close()


@needs_no_gpu
def test_dry_run_separate_ragged_joint_model_with_enroll_lengths(tmp_path):
    path = str(tmp_path / "j.wsw")
    export_engine(_model(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                         spk_model="ResNet18", **SPK), path)
    eng = E.Engine(path, dry_run=True)
    mixes = [np.zeros(n, np.float32) for n in (16000, 9000, 12345)]
    eng.separate(np.zeros((3, 16000), np.float32), np.zeros((3, 98, 80), np.float32), E.ENROLL_FBANK)
    n_rect = eng.info("n_launches")
    est = eng.separate_ragged(mixes, [np.zeros((t, 80), np.float32) for t in (98, 120, 33)], E.ENROLL_FBANK)
    assert [len(x) for x in est] == [16000, 9000, 12345]
    assert eng.info("n_launches") > n_rect                     # the speaker stage ran once per enrollment row
    n_fbank = eng.info("n_launches")
    eng.separate_ragged(mixes, [np.zeros(n, np.float32) for n in (24001, 16000, 30000)], E.ENROLL_WAVE)
    assert eng.info("n_launches") > n_fbank                    # + the kaldi fbank / CMN launches per row
    with pytest.raises(E.WesepHipError, match="too short for the speaker encoder"):
        eng.separate_ragged(mixes, [np.zeros((t, 80), np.float32) for t in (98, 5, 33)], E.ENROLL_FBANK)
    with pytest.raises(E.WesepHipError, match="shorter than one"):
        eng.separate_ragged(mixes, [np.zeros(n, np.float32) for n in (24001, 100, 30000)], E.ENROLL_WAVE)
    with pytest.raises(E.WesepHipError, match="does not fit"):
        eng.separate_ragged(mixes, [np.zeros(256, np.float32)] * 3, E.ENROLL_EMBEDDING)
    # an enrollment length beyond the row pitch of the enrollment buffer
    mix, fb, est = np.zeros((2, 8000), np.float32), np.zeros((2, 50, 80), np.float32), np.zeros((2, 8000), np.float32)
    ln, el = np.array([8000, 6000], np.int32), np.array([50, 51], np.int32)
    assert E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, 2, 8000, ln.ctypes.data, fb.ctypes.data, E.ENROLL_FBANK,
                                             50, el.ctypes.data, est.ctypes.data) == -1
    assert "exceeds the row pitch" in E.lib().ws_engine_last_error().decode()
    eng.close()


@needs_no_gpu
def test_dry_run_separate_ragged_is_refused_for_other_architectures(tmp_path):
    from wesep_amd.models import get_model
    path = str(tmp_path / "tas.wsw")
    export_engine(get_model("ConvTasNet")(N=32, L=20, B=32, H=64, P=3, X=2, R=1, joint_training=False), path)
    eng = E.Engine(path, dry_run=True)
    assert eng.info("arch") == 1
    with pytest.raises(E.WesepHipError, match="pBSRNN"):
        eng.separate_ragged([np.zeros(8000, np.float32), np.zeros(6000, np.float32)], [np.zeros(256, np.float32)] * 2,
                            E.ENROLL_EMBEDDING)
    # without lengths the new entry point is the old one, for every architecture
    mix, emb, est = np.zeros((2, 8000), np.float32), np.zeros((2, 256), np.float32), np.zeros((2, 8000), np.float32)
    assert E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, 2, 8000, None, emb.ctypes.data, E.ENROLL_EMBEDDING, 0,
                                             None, est.ctypes.data) == 0
    eng.close()


# ---- separate_main --batch --------------------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


def scp_groups(n_lines, batch):
    """The batching rule of separate_main --batch: N consecutive lines of the scp per forward, the last group short."""
    return [list(range(i, min(i + batch, n_lines))) for i in range(0, n_lines, batch)]


def test_scp_grouping_rule():
    assert scp_groups(5, 3) == [[0, 1, 2], [3, 4]] and scp_groups(4, 4) == [[0, 1, 2, 3]] and scp_groups(3, 8) == [[0, 1, 2]]
    assert [len(g) for g in scp_groups(64, 16)] == [16] * 4


@needs_no_gpu
def test_separate_main_batch_dry_run(tmp_path):
    exe = os.path.join(ROOT, "runtime", "separate_main")
    assert os.path.exists(exe), "run python -m wesep_amd.build"
    model = str(tmp_path / "j.wsw")
    export_engine(_model(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                         spk_model="ResNet18", **SPK), model)
    rng = np.random.default_rng(0)
    lens = (24000, 16000, 40000, 8000, 12352)           # (whole milliseconds: the total is printed rounded)
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1000 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 1000 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    total = f"Total: process {sum(lens) * 1000 // 16000}ms audio"
    r = subprocess.run([exe, "--wav_scp", str(scp), "--model", model, "--dry_run", "--batch", "3"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    proc = [l for l in r.stdout.splitlines() if l.startswith("process:")]
    assert [l.split()[1] for l in proc] == [f"u{i}" for i in range(5)]            # every key, in scp order with one job
    assert ["batch of 3" in l for l in proc] == [True] * 3 + [False] * 2 and "batch of 2" in proc[4]
    assert total in r.stdout and "[dry run]" in r.stdout
    # with worker threads: each takes the next N lines
    r = subprocess.run([exe, "--wav_scp", str(scp), "--model", model, "--dry_run", "--batch=2", "--jobs", "2"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert sorted(l.split()[1] for l in r.stdout.splitlines() if l.startswith("process:")) == [f"u{i}" for i in range(5)]
    assert total in r.stdout
    # --batch 1 is the path the tool always had (one utterance per call of the reference runtime's entry point)
    r1 = subprocess.run([exe, "--wav_scp", str(scp), "--model", model, "--dry_run", "--batch", "1"], capture_output=True,
                        text=True, timeout=120)
    r0 = subprocess.run([exe, "--wav_scp", str(scp), "--model", model, "--dry_run"], capture_output=True, text=True, timeout=120)
    strip = lambda out: [re.sub(r"RTF: [0-9.]+", "RTF", l) for l in out.splitlines() if l.startswith("process:")]
    assert r1.returncode == 0 and r0.returncode == 0 and strip(r1.stdout) == strip(r0.stdout) and "batch of" not in r1.stdout
    r = subprocess.run([exe, "--wav_scp", str(scp), "--model", model, "--dry_run", "--batch", "0"], capture_output=True, text=True)
    assert r.returncode == 1 and "--batch" in r.stderr
    # a mixture below the engine's 512 samples is refused with the row named, not computed
    _write_wav(tmp_path / "short.wav", rng.integers(-3000, 3000, 300))
    bad = tmp_path / "bad.scp"
    bad.write_text(lines[0] + f"s {tmp_path}/short.wav {tmp_path}/a0.wav {tmp_path}/b0.wav\n")
    r = subprocess.run([exe, "--wav_scp", str(bad), "--model", model, "--dry_run", "--batch", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and "lengths[2] = 300" in r.stderr


# ---- host logic against numpy -----------------------------------------------------------------------------------------
def test_frame_tables_and_row_packing_against_numpy():
    from wesep_amd import dev
    lengths = [16000, 12345, 4096, 9999, 512, 257, 383, 384]
    want = np.array([1 + n // 128 for n in lengths])
    assert np.array_equal(E.frames_of(lengths), want)
    # frames of a row = frames torch.stft gives that row alone (centred framing)
    for n in (257, 383, 384, 4096, 9999):
        assert torch.stft(torch.zeros(n), 512, 128, window=torch.hann_window(512), return_complex=True).shape[-1] == 1 + n // 128
    ln, tf = dev.ragged_tables(lengths, 16000, torch.device("cpu"))
    assert ln.dtype == tf.dtype == torch.int32 and ln.tolist() == lengths and tf.tolist() == want.tolist()
    assert dev.ragged_tables(np.array(lengths), 16000, torch.device("cpu"))[1].tolist() == want.tolist()
    assert dev.ragged_tables(torch.tensor(lengths), 16000, torch.device("cpu"))[0].tolist() == lengths
    for bad, T in (([16000, 256], 16000), ([16001], 16000), ([0], 4000), ([], 4000)):
        with pytest.raises(L.WesepHipError, match="lengths"):
            dev.ragged_tables(bad, T, torch.device("cpu"))
    # the per-group length of the three GroupNorms over time: group g = r * K + band reads table[g // K]
    K = 32
    per_group = np.repeat(want[:4], K)
    assert all(per_group[g] == tf[g // K] for g in range(4 * K))
    # rows -> rectangle + lengths
    rng = np.random.default_rng(1)
    rows = [rng.standard_normal(n).astype(np.float32) for n in (700, 4000, 513)]
    rect, n = E.pack_rows(rows)
    assert rect.shape == (3, 4000) and n.dtype == np.int32 and n.tolist() == [700, 4000, 513]
    for r, x in enumerate(rows):
        assert np.array_equal(rect[r, :len(x)], x) and not rect[r, len(x):].any()
    fb, n = E.pack_rows([np.ones((98, 80)), np.ones((33, 80))])
    assert fb.shape == (2, 98, 80) and n.tolist() == [98, 33] and fb[1, 33:].sum() == 0
    with pytest.raises(ValueError):
        E.pack_rows([np.ones((98, 80)), np.ones((33, 40))])
    with pytest.raises(ValueError):
        E.pack_rows([])


def test_peak_normalisation_over_the_valid_part_of_each_row():
    from wesep_amd.bin.infer import peak_normalise_rows
    rng = np.random.default_rng(2)
    out = rng.standard_normal((3, 1000)).astype(np.float32)
    lengths = [1000, 400, 700]
    out[1, 400:] = 0
    out[2, 700:] = 0
    out[2, :700] = -np.abs(out[2, :700])                        # a row without a positive sample keeps its scale
    got = peak_normalise_rows(out, lengths)
    for r, n in enumerate(lengths):
        row = out[r, :n]
        want = row / np.abs(row).max() * 0.9 if row.max() > 0 else row      # infer.py:118-128 on the row alone
        assert np.allclose(got[r, :n], want, rtol=0, atol=1e-7) and not got[r, n:].any()
    assert abs(np.abs(got[1]).max() - 0.9) < 1e-6


def test_python_surface_refuses_what_is_out_of_scope():
    from wesep_amd import functional as F_
    m = _model(num_repeat=1, use_spk_transform=False, spk_fuse_type="multiply", multi_fuse=False, joint_training=False)
    wav, emb = torch.zeros(2, 4000), torch.zeros(2, 256)
    with pytest.raises(L.WesepHipError, match="inference"):           # ragged training is out of scope: refused, not ignored
        m(wav, emb, lengths=[4000, 3000])
    with torch.no_grad():
        with pytest.raises(L.WesepHipError, match="lengths for 2 rows"):
            m(wav, emb, lengths=[4000, 3000, 2000])
        with pytest.raises(L.WesepHipError, match="no CPU path"):
            m(wav, emb, lengths=[4000, 3000])
    with pytest.raises(TypeError):                                   # keyword only: the reference's call signature is untouched
        m(wav, emb, [4000, 3000])
    z = torch.zeros(1, 32, 9, 128)
    blk = m.separator.separation[1].band_rnn
    with pytest.raises(L.WesepHipError, match="inference"):
        blk(z, "time", frames=torch.tensor([9], dtype=torch.int32))


def test_ragged_plan_takes_a_branch_over_precomputed_gates(monkeypatch):
    """make_plan(ragged=True): never 'fused' / 'cluster2' (they project inside the recurrence and know no lengths), and
    blstm_forward refuses step counts on those branches instead of ignoring them."""
    from wesep_amd import blstm_core, dev
    from wesep_amd.functional import _view_maps
    monkeypatch.setattr(dev, "cu_count", lambda device: 256)
    d = torch.device("cpu")
    for R, Tf, rect, ragged in ((2, 126, "cluster2", "cluster"), (3, 126, "stream", "stream"), (2, 20, "stream", "stream"),
                                (66, 20, "fused", "stream"), (32, 126, "cluster2", "cluster")):
        seq = _view_maps("time", R, 32, Tf, 128)[2]
        assert blstm_core.make_plan(seq, d, False).fwd == rect, (R, Tf)
        assert blstm_core.make_plan(seq, d, False, ragged=True).fwd == ragged, (R, Tf)
    seq = _view_maps("time", 2, 32, 126, 128)[2]
    plan = blstm_core.make_plan(seq, d, False)
    with pytest.raises(L.WesepHipError, match="step counts"):
        blstm_core.blstm_forward(plan, lambda kind: (None, None), torch.zeros(2 * 32 * 126, 128), seq, None, None,
                                 steps=(torch.zeros(2, dtype=torch.int32), 32))
