"""CPU: long recordings in the native runtime without a GPU -- the new symbols and their argument contracts in the built
libraries, the window layout and the cross-fade restated in numpy float64 (tests/longform_ref.py), the engine's dry run of
ws_engine_embed / ws_engine_separate_long / WS_ENROLL_SPEAKER through the real libwesep_hip.so validation for all four
architectures (launch counts: the speaker stage runs once, a group is a rectangular call), the refusals, and
`separate_main --dry_run --chunk_seconds`."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import longform_ref as R
from wesep_amd import _lib as L
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
SPK = dict(joint_training=True, spk_model="ResNet18", spk_feat=True,
           spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False))
# (model, arguments, window, overlap): tiny containers, one per architecture, each with its own speaker stage
ARCHS = {
    "pBSRNN": ("BSRNN", dict(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False, **SPK), 2048, 512),
    "ConvTasNet": ("ConvTasNet", dict(N=256, L=20, B=64, H=128, P=3, X=2, R=1, spk_emb_dim=256, joint_training=True), 2000, 500),
    "DPCCN": ("DPCCN", dict(tcn_blocks=1, tcn_layers=1, spk_emb_dim=256, **SPK), 4096, 1024),
    "TFGridNet": ("TFGridNet", dict(n_layers=1, emb_dim=128, emb_ks=1, emb_hs=1, lstm_hidden_units=64, spk_emb_dim=256, **SPK),
                  2048, 512),
}
# launches of ws_engine_separate(R = 2, T = window, waveform enrollment of 16000 samples) on the commit before this one
PARENT_LAUNCHES = {"pBSRNN": 74, "ConvTasNet": 55, "DPCCN": 430, "TFGridNet": 104}
SWEEP = [(512, 512, 128), (513, 512, 128), (2000, 512, 128), (1537, 512, 0), (5000, 516, 258), (513, 512, 100), (5003, 2000, 500),
         (100, 512, 128), (1, 1, 0), (7, 3, 1), (1025, 512, 256), (40001, 4000, 1000), (9000, 4096, 1024)]


def _container(tmp_path, arch, **kw):
    from wesep_amd.models import get_model
    name, args, _, _ = ARCHS[arch]
    path = str(tmp_path / f"{arch}{len(kw)}.wsw")
    export_engine(get_model(name)(**{**args, **kw}), path)
    return path


last = lambda: E.lib().ws_engine_last_error().decode()


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_longform_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    lib = L.lib()
    for name in ("ws_window_rows", "ws_xfade_ola"):
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        assert getattr(lib, name) is not None
    from wesep_amd import dev
    assert callable(dev.window_rows) and callable(dev.xfade_ola)
    eheader = open(os.path.join(ROOT, "include", "wesep_engine.h")).read()
    assert re.search(r"^#define WS_ENROLL_SPEAKER 3\b", eheader, flags=re.M) and E.ENROLL_SPEAKER == 3
    for name in ("ws_engine_embed", "ws_engine_separate_long"):
        assert re.search(r"^int\s+" + name + r"\s*\(", eheader, flags=re.M), name
        assert name in E.SYMBOLS and getattr(E.lib(), name) is not None
    assert callable(E.Engine.embed) and callable(E.Engine.separate_long) and callable(E.long_windows)
    assert lib.ws_abi_version() == 20                        # new symbols only: neither ABI number moves
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


def test_longform_kernels_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    buf, buf2 = (ctypes.c_float * 8192)(), (ctypes.c_float * 8192)()
    p, p2 = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)
    err = lambda: lib.ws_last_error().decode()
    # ws_window_rows(x, n, W, S, H, reps, scale, rows, stream)
    assert lib.ws_window_rows(None, 2000, 4, 512, 384, 2, None, p2, None) == -1 and "ws_window_rows: x or rows is NULL" in err()
    assert lib.ws_window_rows(p, 2000, 4, 512, 384, 2, None, None, None) == -1 and "ws_window_rows" in err()
    assert lib.ws_window_rows(p, 2000, 7, 512, 255, 2, None, p2, None) == -1 and "ws_window_rows: hop H=255" in err()   # O = 257 > S / 2
    assert lib.ws_window_rows(p, 2000, 3, 512, 513, 2, None, p2, None) == -1 and "ws_window_rows: hop H=513" in err()   # O < 0
    assert lib.ws_window_rows(p, 2000, 4, 512, 384, 2, None, p2, None) == -1 and "ws_window_rows: W=4 does not match" in err() \
        and "5 windows" in err()
    assert lib.ws_window_rows(p, 512, 2, 512, 384, 2, None, p2, None) == -1 and "1 windows" in err()                    # n <= S: one
    assert lib.ws_window_rows(p, 0, 1, 512, 384, 2, None, p2, None) == -1 and "ws_window_rows: bad args" in err()
    assert lib.ws_window_rows(p, 2000, 5, 512, 384, 0, None, p2, None) == -1 and "ws_window_rows: bad args" in err()
    # ws_xfade_ola(y, K, W, S, O, n, scale, out, stream)
    assert lib.ws_xfade_ola(None, 2, 5, 512, 128, 2000, None, p2, None) == -1 and "ws_xfade_ola: y or out is NULL" in err()
    assert lib.ws_xfade_ola(p, 2, 5, 512, 128, 2000, None, None, None) == -1 and "ws_xfade_ola" in err()
    assert lib.ws_xfade_ola(p, 2, 7, 512, 257, 2000, None, p2, None) == -1 and "ws_xfade_ola: overlap O=257 outside" in err()
    assert lib.ws_xfade_ola(p, 2, 5, 512, -1, 2000, None, p2, None) == -1 and "ws_xfade_ola: overlap O=-1" in err()
    assert lib.ws_xfade_ola(p, 2, 4, 512, 128, 2000, None, p2, None) == -1 and "ws_xfade_ola: W=4 does not match" in err()
    assert lib.ws_xfade_ola(p, 0, 5, 512, 128, 2000, None, p2, None) == -1 and "ws_xfade_ola: bad args" in err()


# ---- the layout and the cross-fade, restated ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,S,O", SWEEP)
def test_window_layout_properties(n, S, O):
    st = R.starts(n, S, O)
    assert st == E.long_windows(n, S, O)                                        # the Python surface states the same layout
    H, Lw = S - O, min(n, S)
    W = 1 if n <= S else 1 + -(-(n - S) // H)
    assert len(st) == W
    assert all(b > a for a, b in zip(st, st[1:])) and st[0] == 0               # ascending
    assert all(0 <= s and s + Lw <= n for s in st)                              # every window has its full length inside [0, n)
    if n > S:
        assert st[-1] == n - S and all(s == w * H for w, s in enumerate(st[:-1]))
    covered = np.zeros(n, int)
    for s in st:
        covered[s:s + Lw] += 1
    assert covered.min() >= 1                                                   # the union is [0, n)
    assert covered.max() <= -(-S // H) + 1                                      # at most ceil(S / H) + 1 terms per sample
    # two regular neighbours (w, w + 1 < W - 1, or a last window that happens to sit on the grid): the ramps add up to exactly 1
    for w in range(W - 1):
        if st[w + 1] - st[w] != H:
            continue
        for j in range(O):                                                      # sample st[w + 1] + j: local H + j and j
            others = [v for v in range(W) if v not in (w, w + 1) and st[v] <= st[w + 1] + j < st[v] + Lw]
            if not others:
                assert R.weight(w, W, H + j, Lw, O) + R.weight(w + 1, W, j, Lw, O) == Fraction(1)
    g = R.weights(W, Lw, O)
    assert (g > 0).all() and g.max() <= 1.0
    assert all(abs(g[w][j] - float(R.weight(w, W, j, Lw, O))) < 1e-15 for w in range(W) for j in (0, min(O, Lw - 1) // 2, min(O, Lw - 1), Lw // 2, Lw - 1))
    rng = np.random.default_rng(n + S + O)
    x = rng.standard_normal(n)
    back = R.xfade(np.stack([R.gather(x, S, O)] * 2), n, S, O)                  # a partition of unity: xfade(windows(x)) = x
    assert back.shape == (2, n) and np.abs(back - x).max() < 1e-12


def test_triple_overlap_case_is_in_the_sweep():
    st = R.starts(5003, 2000, 500)
    assert st == [0, 1500, 3000, 3003]                                          # the last window overlaps its predecessor by 1997
    assert sum(s <= 3400 < s + 2000 for s in st) == 3                           # ... and a third window with it
    with pytest.raises(ValueError):
        E.long_windows(1000, 512, 257)


# ---- the engine's refusals -----------------------------------------------------------------------------------------------
def _long(eng, n, K, enroll, kind, elen, window, overlap, max_rows, mix=None):
    mix = np.ones(n, np.float32) if mix is None else mix
    est = np.zeros((K, n), np.float32)
    enroll = np.ascontiguousarray(enroll, np.float32)
    return E.lib().ws_engine_separate_long(eng._h, mix.ctypes.data, n, K, enroll.ctypes.data, kind, elen, None, window, overlap,
                                           max_rows, est.ctypes.data)


@needs_no_gpu
def test_separate_long_and_embed_refusals(tmp_path):
    from wesep_amd.models import get_model
    path = str(tmp_path / "fixed.wsw")
    export_engine(get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                                     joint_training=False), path)
    eng = E.Engine(path, dry_run=True)
    emb = np.zeros((2, 256), np.float32)
    assert _long(eng, 6000, 2, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 3) == 0
    assert _long(eng, 6000, 2, emb, E.ENROLL_EMBEDDING, 0, 500, 100, 3) == -1 and "T=500; T >= 512" in last()   # pBSRNN's own message
    assert _long(eng, 6000, 2, emb, E.ENROLL_EMBEDDING, 0, 2048, 1025, 3) == -1 and "overlap = 1025 outside [0, window / 2 = 1024]" in last()
    assert _long(eng, 6000, 2, emb, E.ENROLL_EMBEDDING, 0, 2048, -1, 3) == -1 and "overlap = -1 outside" in last()
    assert _long(eng, 6000, 2, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 0) == -1 and "max_rows = 0" in last()
    assert _long(eng, 6000, 0, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 3) == -1 and "ws_engine_separate_long: bad arguments" in last()
    # kind 3 is what ws_engine_embed returned: a container that takes fixed embeddings has no such thing
    for n in (6000, 2048):
        assert _long(eng, n, 2, emb, E.ENROLL_SPEAKER, 0, 2048, 512, 3) == -1 and "kind 3 does not fit this model" in last()
    mix, est = np.ones((2, 4000), np.float32), np.zeros((2, 4000), np.float32)
    assert E.lib().ws_engine_separate(eng._h, mix.ctypes.data, 2, 4000, emb.ctypes.data, E.ENROLL_SPEAKER, 0, est.ctypes.data) == -1 \
        and "kind 3 does not fit this model (joint_training = 0)" in last()
    assert E.lib().ws_engine_separate(eng._h, mix.ctypes.data, 2, 4000, emb.ctypes.data, 4, 0, est.ctypes.data) == -1 \
        and "kind 4 does not fit this model" in last()                                       # outside 0-3: the message it always had
    assert E.lib().ws_engine_separate(eng._h, mix.ctypes.data, 2, 4000, emb.ctypes.data, E.ENROLL_WAVE, 16000, est.ctypes.data) == -1 \
        and "kind 2 does not fit this model" in last()
    with pytest.raises(E.WesepHipError, match="ws_engine_embed: this container takes fixed embeddings"):
        eng.embed(np.zeros((2, 16000), np.float32), E.ENROLL_WAVE)
    eng.close()


@needs_no_gpu
def test_separate_long_refusals_by_architecture(tmp_path):
    from wesep_amd.models import get_model
    emb = np.zeros((2, 256), np.float32)
    # Conv-TasNet: a window must end where a frame ends
    path = str(tmp_path / "tas.wsw")
    export_engine(get_model("ConvTasNet")(N=32, L=20, B=32, H=64, P=3, X=2, R=1, joint_training=False), path)
    eng = E.Engine(path, dry_run=True)
    assert _long(eng, 5003, 2, emb, E.ENROLL_EMBEDDING, 0, 2000, 500, 8) == 0
    assert eng.info("long_windows") == 4 and eng.info("long_forwards") == 1
    assert _long(eng, 5003, 2, emb, E.ENROLL_EMBEDDING, 0, 2005, 500, 8) == -1 and "nearest valid windows are 2000 and 2010" in last()
    assert _long(eng, 5003, 2, emb, E.ENROLL_EMBEDDING, 0, 150, 30, 8) == -1 and "Conv-TasNet needs T >= 160" in last()
    assert _long(eng, 5003, 2, emb, E.ENROLL_SPEAKER, 0, 2000, 500, 8) == -1 and "a Conv-TasNet engine takes fixed embeddings" in last()
    eng.close()
    # DPCCN: its minimum T, and the 2^31 guard on a GROUP (the whole-utterance call refuses such a recording outright)
    path = str(tmp_path / "dp.wsw")
    export_engine(get_model("DPCCN")(tcn_blocks=1, tcn_layers=1, joint_training=False), path)
    eng = E.Engine(path, dry_run=True)
    assert _long(eng, 9000, 2, emb, E.ENROLL_EMBEDDING, 0, 3900, 900, 8) == -1 and "a DPCCN engine needs T >= 3968" in last()
    window = 128 * 9000                                     # 8 rows x 9001 frames x 257 x 160 >= 2^31; 1 row is far below
    assert _long(eng, 4 * window, 2, emb, E.ENROLL_EMBEDDING, 0, window, 0, 8) == -1 and "R * frames * 257 * 160 below 2^31 (R=8" in last()
    eng.close()
    path = str(tmp_path / "tfg.wsw")
    export_engine(get_model("TFGridNet")(n_layers=1, emb_dim=128, emb_ks=1, emb_hs=1, lstm_hidden_units=64, spk_emb_dim=256,
                                         joint_training=False), path)
    eng = E.Engine(path, dry_run=True)
    assert _long(eng, 5000, 2, emb, E.ENROLL_EMBEDDING, 0, 200, 50, 8) == -1 and "ws_engine_separate: bad arguments (R=1, T=200" in last()
    assert _long(eng, 5000, 2, emb, E.ENROLL_EMBEDDING, 0, 2048, 512, 8) == 0
    eng.close()


# ---- the engine's dry run: launch counts -------------------------------------------------------------------------------
@needs_no_gpu
@pytest.mark.parametrize("arch", sorted(ARCHS))
def test_dry_run_speaker_stage_runs_once_and_a_group_is_a_rectangular_call(tmp_path, arch):
    """Fails on the commit before: neither entry point exists."""
    _, _, S, O = ARCHS[arch]
    eng = E.Engine(_container(tmp_path, arch), dry_run=True)
    K, max_rows, H = 2, 3, S - O
    wave = np.zeros((K, 16000), np.float32)
    rect = np.ones((K, S), np.float32)
    eng.separate(rect, wave, E.ENROLL_WAVE)
    before = eng.info("n_launches")
    assert before == PARENT_LAUNCHES[arch] and eng.info("long_windows") == 0 == eng.info("long_forwards")
    emb = eng.embed(wave, E.ENROLL_WAVE)
    n_embed = eng.info("n_launches")
    assert emb.shape == (K, 256) and n_embed > 0
    # the rectangular call with the embedding handed in: the same launches without the speaker stage
    n_rect = {}
    for G in (1, 2, 3):
        eng.separate(np.ones((G, S), np.float32), np.zeros((G, 256), np.float32), E.ENROLL_SPEAKER)
        n_rect[G] = eng.info("n_launches")
    assert n_rect[2] == before - n_embed
    for W, n in ((1, S), (2, S + 1), (5, S + 4 * H - 3)):
        assert len(E.long_windows(n, S, O)) == W
        est = eng.separate_long(np.ones(n, np.float32), wave, E.ENROLL_WAVE, S, O, max_rows)
        assert est.shape == (K, n) and not est.any()                                  # a dry run computes nothing
        n_wave = eng.info("n_launches")
        forwards = -(-K * W // max_rows)
        assert (eng.info("long_windows"), eng.info("long_forwards")) == (W, forwards), (arch, W)
        eng.separate_long(np.ones(n, np.float32), emb, E.ENROLL_SPEAKER, S, O, max_rows)
        n_spk = eng.info("n_launches")
        assert n_wave - n_spk == n_embed, (arch, W, n_wave, n_spk, n_embed)          # the speaker stage ran once, over K rows
        assert (eng.info("long_windows"), eng.info("long_forwards")) == (W, forwards)
        if W == 1:
            assert n_spk == n_rect[K]                                                 # n <= window: ws_engine_separate on [K][n]
        else:
            sizes = [min(max_rows, K * W - g0) for g0 in range(0, K * W, max_rows)]
            assert n_spk == sum(n_rect[G] for G in sizes) + 2, (arch, W, sizes, n_spk)  # + the gather and the cross-fade
    # one window, more speakers than max_rows: the windowed path with W = 1
    eng.separate_long(np.ones(S - 5, np.float32), emb, E.ENROLL_SPEAKER, S, O, 1)
    assert (eng.info("long_windows"), eng.info("long_forwards")) == (1, 2)
    eng.separate(rect, wave, E.ENROLL_WAVE)
    assert eng.info("n_launches") == before and eng.info("long_windows") == 0         # the rectangular call is what it was
    eng.close()


@needs_no_gpu
def test_dry_run_embed_with_enroll_lengths_takes_the_ragged_pass(tmp_path):
    eng = E.Engine(_container(tmp_path, "pBSRNN"), dry_run=True)
    assert eng.info("ragged_speaker") == 1
    rows = [np.zeros(16000, np.float32), np.zeros(12000, np.float32), np.zeros(9000, np.float32)]
    eng.embed(rows, E.ENROLL_WAVE)
    n_ragged = eng.info("n_launches")
    eng.embed(rows[0][None], E.ENROLL_WAVE)
    n_one = eng.info("n_launches")
    assert n_ragged < 3 * n_one                                # one pass over all rows, not one per row
    est = eng.separate_long(np.ones(6000, np.float32), rows[:2], E.ENROLL_WAVE, 2048, 512, 3)
    assert est.shape == (2, 6000) and eng.info("long_windows") == 4 and eng.info("long_forwards") == 3
    eng.close()


# ---- separate_main --chunk_seconds ---------------------------------------------------------------------------------------
@needs_no_gpu
def test_separate_main_chunked_dry_run(tmp_path):
    from tests.test_ragged_host_cpu import _write_wav
    exe = os.path.join(ROOT, "runtime", "separate_main")
    assert os.path.exists(exe), "run python -m wesep_amd.build"
    model = _container(tmp_path, "pBSRNN")
    rng = np.random.default_rng(0)
    lens = (5000, 8000, 2048)
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1000 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 1000 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    base = [exe, "--wav_scp", str(scp), "--model", model, "--dry_run"]
    chunk = ["--chunk_seconds", "0.128", "--overlap_seconds", "0.032", "--chunk_rows", "3"]
    plain = subprocess.run(base, capture_output=True, text=True, timeout=120)
    r = subprocess.run(base + chunk, capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and r.returncode == 0, r.stderr
    keys = lambda out: [l.split()[1] for l in out.splitlines() if l.startswith("process:")]
    assert keys(r.stdout) == keys(plain.stdout) == ["u0", "u1", "u2"]                  # the same outputs, by name
    want = [(len(E.long_windows(n, 2048, 512)), -(-2 * len(E.long_windows(n, 2048, 512)) // 3)) for n in lens]
    got = [tuple(map(int, re.search(r"\((\d+) windows in (\d+) forwards", l).groups()))
           for l in r.stdout.splitlines() if l.startswith("process:")]
    assert got == want == [(3, 2), (5, 4), (1, 1)]
    assert f"Total: process {sum(lens) * 1000 // 16000}ms audio" in r.stdout
    r = subprocess.run(base + chunk + ["--batch", "2"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--chunk_seconds and --batch 2 conflict" in r.stderr
    r = subprocess.run(base + ["--chunk_seconds", "0.128", "--overlap_seconds", "0.1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "overlap = 1600 outside" in r.stderr
    r = subprocess.run(base + ["--sample_rate", "8000"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "sample rate" in r.stderr                              # the error the tool always had
