"""CPU: ragged batches through the TF-GridNet plan of the native runtime (arch 3) without a GPU -- the new C-ABI symbols
and their argument contracts in the built library, the engine's dry run of ws_engine_separate_ragged through the real
libwesep_hip.so validation (launch counts that depend on neither the lengths nor the row count), the refusals, and
`separate_main --dry_run --batch` on a TF-GridNet container."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from wesep_amd import _lib as L
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
NEW_SYMBOLS = ("ws_flat_stats_len", "ws_ola_norm_len", "ws_transpose_batched", "ws_heads_merge_fwd")
SPK = dict(joint_training=True, spk_model="ResNet18", spk_feat=True,
           spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False))
GRID = dict(n_layers=1, emb_dim=128, emb_ks=1, emb_hs=1, lstm_hidden_units=64, spk_emb_dim=256)
VARIANTS = {"fixed": dict(joint_training=False),
            "fixed-film-transform": dict(joint_training=False, spk_fuse_type="FiLM", use_spk_transform=True),
            "joint-resnet18": SPK}


def _container(tmp_path, variant, **kw):
    from wesep_amd.models import get_model
    path = str(tmp_path / f"{variant}.wsw")
    export_engine(get_model("TFGridNet")(**{**GRID, **VARIANTS[variant], **kw}), path)
    return path


def _enroll(variant, R):
    if variant == "joint-resnet18":
        return [np.zeros((98 + 7 * r, 80), np.float32) for r in range(R)], E.ENROLL_FBANK
    return [np.zeros(256, np.float32)] * R, E.ENROLL_EMBEDDING


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_ragged_gridnet_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name      # the binding has the declared arity
        assert getattr(lib, name) is not None
    from wesep_amd import dev
    for name in ("flat_stats_len", "ola_norm_len", "transpose_batched", "heads_merge_fwd"):
        assert callable(getattr(dev, name))
    assert lib.ws_abi_version() == 20                        # new symbols only: the ABI number does not move
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


def test_ragged_gridnet_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    buf2 = (ctypes.c_float * 4096)()
    ib = (ctypes.c_int * 64)()
    p, p2, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p), ctypes.cast(ib, ctypes.c_void_p)
    err = lambda: lib.ws_last_error().decode()
    assert lib.ws_flat_stats_len(p, 2, 1024, None, 128, 1e-5, 1, p, p, None) == -1 and "glen table is NULL" in err()
    assert lib.ws_flat_stats_len(p, 2, 1024, ip, 126, 1e-5, 1, p, p, None) == -1 and "per_step=126" in err()   # % 4
    assert lib.ws_flat_stats_len(p, 2, 1024, ip, 96, 1e-5, 1, p, p, None) == -1 and "divides" in err()
    assert lib.ws_flat_stats_len(p, 2, 1024, ip, 128, 1e-5, 0, p, p, None) == -1
    assert lib.ws_ola_norm_len(p, p, 2, 17, 128, 1024, None, p2, None) == -1 and "lengths table is NULL" in err()
    assert lib.ws_ola_norm_len(p, p, 2, 16, 128, 1024, ip, p2, None) == -1 and "Tf=16 does not match T=1024" in err()
    assert lib.ws_ola_norm_len(p, p, 2, 129, 12, 768, ip, p2, None) == -1 and "multiple of 8" in err()
    assert lib.ws_transpose_batched(p, 2, 36, 30, p2, None) == -1 and "multiples of 4" in err()
    assert lib.ws_transpose_batched(p, 2, 36, 32, p, None) == -1                               # in place
    assert lib.ws_heads_merge_fwd(p, 4, 2, 10, 30, p2, None) == -1 and "ws_heads_merge_fwd" in err()
    assert lib.ws_heads_merge_fwd(None, 4, 2, 10, 32, p2, None) == -1


# ---- the engine's dry run ---------------------------------------------------------------------------------------------
@needs_no_gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_dry_run_separate_ragged_tfgridnet(tmp_path, variant):
    """Fails before the ragged TF-GridNet plan existed: arch 3 was refused with WS_ERR_INVALID."""
    eng = E.Engine(_container(tmp_path, variant), dry_run=True)
    assert eng.info("arch") == 3 and eng.info("ragged_separator") == 1
    T = 4096
    counts = {}
    # R = 4 and R = 6 take the same recurrence branches.  Intra-frame path (R * 65 frames of 65 bins): 9 and 13 tiles of
    # 32 sequences, WS_LSTM_BF16X3_BLK16 streaming (2 * tiles <= 128; a dry run has no CUs, so never the cluster).
    # Inter-frame path (R * 65 sequences of 65 frames): the same tile counts, the same branch, its gates from
    # ws_gemm_p2b_len.  So the counts of the two can differ only by launches issued per row.
    for R, sets in ((4, ((4096, 3000, 2048, 256), (4096, 4096, 4096, 4096), (4096, 257, 300, 4095))),
                    (6, ((4096, 3000, 2048, 256, 999, 1500),))):
        enroll, kind = _enroll(variant, R)
        for lengths in sets:
            est = eng.separate_ragged([np.ones(n, np.float32) for n in lengths], enroll, kind)
            assert [len(x) for x in est] == list(lengths) and not any(x.any() for x in est)   # a dry run computes nothing
            counts.setdefault(R, set()).add(eng.info("n_launches"))
    assert len(counts[4]) == 1, counts                     # for fixed (R, T) the plan does not depend on the lengths
    if variant != "joint-resnet18":                        # (the ResNet front-end transposes one enrollment row per launch)
        assert counts[4] == counts[6], counts              # no launch per row
    # one row; a row count whose inter-frame path leaves BLK16 (R = 64: 130 tiles -> BLK streaming, never the fused kernel)
    enroll, kind = _enroll(variant, 64)
    eng.separate_ragged([np.ones(777, np.float32)], enroll[:1], kind)
    eng.separate_ragged([np.ones(1024 - 3 * r, np.float32) for r in range(64)], enroll, kind)
    eng.close()


@needs_no_gpu
def test_rectangular_call_keeps_its_launch_count(tmp_path):
    """A call without lengths is the plan the engine always had.  Its launch count, as counted on the commit before the
    ragged plan (49 for R = 2, 57 for R = 3 with one block): 5 ahead of the blocks (pad, STFT, conv, statistics, norm), 1
    fusion Linear; per block fusion 1, 2 * 4 on the BLSTM paths (row LayerNorm, p2b, recurrence, b2p), QKV 1, heads 3,
    logits + softmax + values 3, G transposes, nh * R column copies, and projection, PReLU, statistics, norm, residual 5;
    deconv 1 and dft_istft's 5 (GEMM, overlap-add, copy, envelope, copy)."""
    eng = E.Engine(_container(tmp_path, "fixed"), dry_run=True)
    emb = np.zeros((3, 256), np.float32)
    for R, T in ((2, 4096), (3, 2048)):
        eng.separate(np.ones((R, T), np.float32), emb[:R], E.ENROLL_EMBEDDING)
        G = 4 * R
        assert eng.info("n_launches") == 5 + 1 + (1 + 8 + 1 + 3 + 3 + G + G + 5) + 1 + 5 == (49, 57)[R - 2], (R, T)
        n_rect = eng.info("n_launches")
        # lengths = NULL through the ragged entry point is the same call
        mix, est = np.ones((R, T), np.float32), np.zeros((R, T), np.float32)
        assert E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, R, T, None, emb.ctypes.data, E.ENROLL_EMBEDDING, 0,
                                                 None, est.ctypes.data) == 0
        assert eng.info("n_launches") == n_rect
        # the ragged plan of the same rectangle: one launch for each loop, + 2 tail selections, - 3 behind the synthesis GEMM
        eng.separate_ragged([np.ones(T, np.float32)] * R, list(emb[:R]), E.ENROLL_EMBEDDING)
        assert eng.info("n_launches") == n_rect - 2 * G + 2 + 2 - 3 == 34, (R, T, eng.info("n_launches"))
    eng.close()


@needs_no_gpu
def test_ragged_refusals(tmp_path):
    from wesep_amd.models import get_model
    eng = E.Engine(_container(tmp_path, "fixed"), dry_run=True)
    R, T = 2, 4000
    mix, emb, est = np.ones((R, T), np.float32), np.zeros((R, 256), np.float32), np.zeros((R, T), np.float32)
    last = lambda: E.lib().ws_engine_last_error().decode()

    def call(lengths, enroll_lengths=None):
        ln = np.asarray(lengths, np.int32)
        el = None if enroll_lengths is None else np.asarray(enroll_lengths, np.int32)
        return E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, R, T, ln.ctypes.data, emb.ctypes.data,
                                                 E.ENROLL_EMBEDDING, 0, None if el is None else el.ctypes.data, est.ctypes.data)

    assert call((4000, 256)) == 0                                              # 2 * n_fft: the shortest row the model takes
    for bad, msg in (((4000, 255), "lengths[1] = 255 outside [256, T = 4000]"), ((4001, 4000), "lengths[0] = 4001 outside"),
                     ((0, 4000), "lengths[0] = 0"), ((4000, -7), "lengths[1] = -7")):
        assert call(bad) == -1 and msg in last(), (bad, last())
    assert call((4000, 3000), (10, 10)) == -1 and "fixed embeddings" in last()
    eng.close()
    # n_fft = 16 (9 bins; E = 8 query channels per head): the bound follows the model
    eng = E.Engine(_container(tmp_path, "fixed", n_fft=16, stride=8, attn_approx_qk_dim=72), dry_run=True)
    mix, est = np.ones((R, 600), np.float32), np.zeros((R, 600), np.float32)
    T = 600
    assert call((600, 32)) == 0
    assert call((600, 31)) == -1 and "lengths[1] = 31 outside [32, T = 600]" in last()
    eng.close()
    # the separators without a ragged plan are refused as before, by name
    for name, kw, arch in (("ConvTasNet", dict(N=32, L=20, B=32, H=64, P=3, X=2, R=1), 1),
                           ("DPCCN", dict(tcn_blocks=1, tcn_layers=1), 2)):
        path = str(tmp_path / f"{name}.wsw")
        export_engine(get_model(name)(joint_training=False, **kw), path)
        eng = E.Engine(path, dry_run=True)
        assert eng.info("arch") == arch and eng.info("ragged_separator") == 0
        with pytest.raises(E.WesepHipError, match="pBSRNN"):
            eng.separate_ragged([np.ones(8000, np.float32), np.ones(6000, np.float32)], [np.zeros(256, np.float32)] * 2,
                                E.ENROLL_EMBEDDING)
        eng.close()


# ---- separate_main --batch --------------------------------------------------------------------------------------------
@needs_no_gpu
@pytest.mark.parametrize("sort", [False, True])
def test_separate_main_batch_dry_run_tfgridnet(tmp_path, sort):
    from tests.test_ragged_host_cpu import _write_wav
    exe = os.path.join(ROOT, "runtime", "separate_main")
    assert os.path.exists(exe), "run python -m wesep_amd.build"
    model = _container(tmp_path, "joint-resnet18")
    rng = np.random.default_rng(0)
    lens = (8000, 4000, 12000, 2000, 6400)              # (whole milliseconds: the total is printed rounded)
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1000 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 1000 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    cmd = [exe, "--wav_scp", str(scp), "--model", model, "--dry_run", "--batch", "3"] + (["--sort_by_length"] if sort else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    proc = [l for l in r.stdout.splitlines() if l.startswith("process:")]
    order = sorted(range(5), key=lambda i: -lens[i]) if sort else list(range(5))
    assert [l.split()[1] for l in proc] == [f"u{i}" for i in order]               # every key once, in processing order
    for l in proc:                                                                   # the line format the tool always had
        assert re.fullmatch(r"process: u\d RTF: [0-9.]+ \(batch of [32]: \d+ launches, \d+ MiB arena\) \[dry run\]", l), l
    assert ["batch of 3" in l for l in proc] == [True] * 3 + [False] * 2
    assert f"Total: process {sum(lens) * 1000 // 16000}ms audio" in r.stdout
