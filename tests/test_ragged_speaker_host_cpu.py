"""CPU: the ragged speaker stage (enrollments of any length in one encoder pass) without a GPU -- the new C-ABI
symbols and their argument contracts in the built library, the per-layer width tables against torch's own convolution
output sizes, the masking plan restated in torch fp64 with exact equality, the engine's dry run (launch counts of the
batched stage, of the one-row-at-a-time loop, of an encoder that is not covered), `separate_main --sort_by_length`, and
the refusals of the Python surface."""
import ctypes
import os
import re
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from wesep_amd import _lib as L
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_no_gpu = pytest.mark.skipif(torch.cuda.is_available(), reason="the engine's dry run is refused when a GPU is visible")
NEW_SYMBOLS = ("ws_bn_prelu_fwd_len", "ws_tstp_fwd_len", "ws_astp_fwd_len", "ws_time_mean_len", "ws_cmn_len",
               "ws_tail_select_len", "ws_preemph_pad_len")
# the enrollment frame counts of the engine tests and the widths that end at 2 and 3 frames after three stride-2 stages
LENGTH_SETS = ((98, 120, 33), (120, 77, 98), tuple(range(9, 18)), (398, 251, 300))
RESNET_SPK = dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False)


def _bsrnn(**kw):
    from wesep_amd.models import get_model
    return get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False, **kw)


def _joint(spk_model, spk_args, **kw):
    return _bsrnn(joint_training=True, spk_feat=True, spk_model=spk_model, spk_args=spk_args, **kw)


# ---- the C ABI -------------------------------------------------------------------------------------------------------
def test_ragged_speaker_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    lib = L.lib()
    for name in NEW_SYMBOLS:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        assert getattr(lib, name) is not None
        assert "int*" in m.group(1).replace(" *", "*"), name                  # every one of them takes a length table
    assert lib.ws_abi_version() == L.ABI_VERSION == 20                        # new entry points only
    for base in ("ws_bn_prelu_fwd", "ws_tstp_fwd", "ws_astp_fwd", "ws_preemph_pad"):
        assert base in L._SIGS and re.search(r"^int\s+" + base + r"\s*\(", header, flags=re.M)
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2


def test_ragged_speaker_entry_points_refuse_bad_arguments_before_any_launch():
    """WS_ERR_INVALID comes from the host-side checks, which run without a device.  The tables are device memory: their
    VALUES are checked where they are host values (the engine, dev.length_table); a missing table is refused here."""
    lib = L.lib()
    buf = (ctypes.c_float * 4096)()
    ib = (ctypes.c_int * 64)()
    p, ip = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(ib, ctypes.c_void_p)
    err = lambda: lib.ws_last_error().decode()
    bn = lambda M, C, rpr, W, tab: lib.ws_bn_prelu_fwd_len(p, p, p, p, None, p, M, C, rpr, W, tab, p, p, None)
    assert bn(24, 8, 12, 4, None) == -1 and "ws_bn_prelu_fwd_len" in err() and "NULL" in err()
    for M, C, rpr, W in ((24, 8, 12, 0), (24, 8, 12, -3), (24, 8, 12, 5), (24, 8, 12, 24), (24, 8, 7, 7), (24, 6, 12, 4)):
        assert bn(M, C, rpr, W, ip) == -1 and "ws_bn_prelu_fwd_len" in err(), (M, C, rpr, W)
    assert lib.ws_tstp_fwd_len(p, 2, 3, 8, 4, None, 1e-7, p, None) == -1 and "ws_tstp_fwd_len" in err() and "NULL" in err()
    assert lib.ws_tstp_fwd_len(p, 2, 3, 0, 4, ip, 1e-7, p, None) == -1 and "ws_tstp_fwd_len" in err()
    assert lib.ws_astp_fwd_len(p, p, 2, 8, 4, None, 1e-7, p, p, None) == -1 and "ws_astp_fwd_len" in err() and "NULL" in err()
    assert lib.ws_astp_fwd_len(p, None, 2, 8, 4, ip, 1e-7, p, p, None) == -1 and "ws_astp_fwd_len" in err()
    assert lib.ws_time_mean_len(p, 2, 8, 4, None, p, None) == -1 and "ws_time_mean_len" in err() and "NULL" in err()
    assert lib.ws_time_mean_len(p, 2, 0, 4, ip, p, None) == -1 and "ws_time_mean_len" in err()
    assert lib.ws_cmn_len(p, 2, 8, 4, None, p, None) == -1 and "ws_cmn_len" in err() and "NULL" in err()
    assert lib.ws_cmn_len(p, 0, 8, 4, ip, p, None) == -1 and "ws_cmn_len" in err()
    assert lib.ws_tail_select_len(p, 2, 8, 4, None, p, None) == -1 and "ws_tail_select_len" in err() and "NULL" in err()
    assert lib.ws_tail_select_len(p, 2, 8, 6, ip, p, None) == -1 and "ws_tail_select_len" in err()          # C % 4
    assert lib.ws_preemph_pad_len(p, 2, 600, 256, 1112, 0.97, None, p, None) == -1 and "ws_preemph_pad_len" in err()
    assert "NULL" in err()
    assert lib.ws_preemph_pad_len(p, 2, 256, 256, 1112, 0.97, ip, p, None) == -1 and "ws_preemph_pad_len" in err()   # T <= pad
    assert lib.ws_preemph_pad_len(p, 2, 600, 256, 1111, 0.97, ip, p, None) == -1                                     # ldo
    # the rectangular entry points keep their own messages
    assert lib.ws_bn_prelu_fwd(p, p, p, p, None, p, 24, 6, p, p, None) == -1 and "ws_bn_prelu_fwd: bad args" in err()


def test_host_length_checks_of_the_python_wrappers():
    from wesep_amd import dev
    cpu = torch.device("cpu")
    assert dev.length_table([5, 9, 3], 3, 9, cpu).tolist() == [5, 9, 3]
    assert dev.length_table(np.array([5, 9]), 2, 9, cpu).dtype == torch.int32
    for bad, R, hi, lo in (([5, 10], 2, 9, 1), ([0, 4], 2, 9, 1), ([5], 2, 9, 1), ([256, 300], 2, 400, 257)):
        with pytest.raises(L.WesepHipError, match="lengths"):
            dev.length_table(bad, R, hi, cpu, lo=lo)
    with pytest.raises(L.WesepHipError):          # the wrappers want device tables: there is no CPU path
        dev.tail_select_len(torch.zeros(2, 8, 4), 2, 8, 4, torch.zeros(2, dtype=torch.int32), torch.zeros(2, 8, 4))


# ---- width tables against torch's own output sizes -----------------------------------------------------------------------
def _torch_widths(L0, num_blocks, bottleneck):
    """Output widths of every convolution of the forward, in launch order, from F.conv2d on the row alone."""
    one = lambda k: torch.ones(1, 1, k, k)
    conv = lambda x, k, s, p: F.conv2d(x, one(k), stride=s, padding=p)
    y = conv(torch.zeros(1, 1, 8, L0), 3, 1, 1)
    out = [y.shape[-1]]
    first = True
    for li, n in enumerate(num_blocks):
        for bi in range(n):
            s = 2 if (li > 0 and bi == 0) else 1
            if s != 1 or (bottleneck and first):
                out.append(conv(y, 1, s, 0).shape[-1])
            first = False
            if bottleneck:
                o1 = conv(y, 1, 1, 0)
                o2 = conv(o1, 3, s, 1)
                y = conv(o2, 1, 1, 0)
                out += [o1.shape[-1], o2.shape[-1], y.shape[-1]]
            else:
                o1 = conv(y, 3, s, 1)
                y = conv(o1, 3, 1, 1)
                out += [o1.shape[-1], y.shape[-1]]
    return out


@pytest.mark.parametrize("name,bottleneck", [("ResNet18", False), ("ResNet34", False), ("ResNet50", True)])
def test_width_tables_match_conv2d_output_sizes_on_the_row_alone(name, bottleneck):
    from oracle import resnet_oracle as RO
    from wesep_amd.models.resnet import ragged_widths
    nb = RO.NUM_BLOCKS[name]
    for lengths in LENGTH_SETS:
        tabs = ragged_widths(lengths, nb, bottleneck)
        for r, n in enumerate(lengths):
            assert [t[r] for t in tabs] == _torch_widths(n, nb, bottleneck), (name, n)
    assert ragged_widths([9], nb, bottleneck)[-1] == [2] and ragged_widths([17], nb, bottleneck)[-1] == [3]
    # the 1x1 stride-s shortcut and the 3x3 stride-s convolution beside it agree on every width
    from wesep_amd.dev import conv_widths
    w = list(range(1, 400))
    assert conv_widths(w, 1, 2, 0) == conv_widths(w, 3, 2, 1) and conv_widths(w, 3, 1, 1) == w == conv_widths(w, 1, 1, 0)


# ---- the masking plan, restated in torch fp64: exact equality ----------------------------------------------------------
def _mini_resnet(seed):
    """Stem + five BasicBlocks, three stride-2 stages with 1x1 shortcuts, eval-mode BatchNorm with random statistics."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)

    def bn(c):
        return dict(w=1 + 0.2 * rnd(c), b=0.3 * rnd(c), rm=0.2 * rnd(c), rv=0.5 + torch.rand(c, generator=g, dtype=torch.float64))

    net = dict(stem=(0.5 * rnd(4, 1, 3, 3), bn(4)), blocks=[])
    inp = 4
    for planes, s in ((4, 1), (8, 2), (8, 1), (16, 2), (16, 2)):
        blk = dict(s=s, c1=(0.3 * rnd(planes, inp, 3, 3), bn(planes)), c2=(0.3 * rnd(planes, planes, 3, 3), bn(planes)), sc=None)
        if s != 1 or inp != planes:
            blk["sc"] = (0.5 * rnd(planes, inp, 1, 1), bn(planes))
        net["blocks"].append(blk)
        inp = planes
    return net


def _mini_forward(net, x, widths=None):
    """x [R, 1, H, W].  widths: the masked rectangle -- after every conv + BN + activation the tail of each row is
    SELECTED to zero at the row's own output width (torch.where: NaN does not survive); None: the plain network."""
    out_w = lambda w, k, s, p: [(v + 2 * p - k) // s + 1 for v in w]

    def select(y, w):
        if w is None:
            return y
        keep = torch.arange(y.shape[-1])[None, :] < torch.tensor(w)[:, None]
        return torch.where(keep[:, None, None, :], y, torch.zeros((), dtype=y.dtype))

    def cba(x, res, conv, s, relu, w_out):
        wgt, b = conv
        y = F.conv2d(x, wgt, stride=s, padding=wgt.shape[-1] // 2)
        y = F.batch_norm(y, b["rm"], b["rv"], b["w"], b["b"], False, 0.1, 1e-5)
        if res is not None:
            y = y + res
        return select(F.relu(y) if relu else y, w_out)

    w = widths
    if w is not None:
        x = select(x, w)
    w = out_w(w, 3, 1, 1) if w is not None else None
    y = cba(x, None, net["stem"], 1, True, w)
    for blk in net["blocks"]:
        w1 = out_w(w, 3, blk["s"], 1) if w is not None else None
        sc = y
        if blk["sc"] is not None:
            assert w is None or out_w(w, 1, blk["s"], 0) == w1
            sc = cba(y, None, blk["sc"], blk["s"], False, w1)
        o = cba(y, None, blk["c1"], blk["s"], True, w1)
        w = out_w(w1, 3, 1, 1) if w is not None else None
        y = cba(o, sc, blk["c2"], 1, True, w)
    return y, w


@pytest.mark.parametrize("lengths", LENGTH_SETS)
def test_masked_rectangle_equals_every_row_alone_exactly_in_fp64(lengths):
    net = _mini_resnet(7)
    g = torch.Generator().manual_seed(len(lengths))
    H, W = 8, max(lengths)
    rows = [torch.randn(1, 1, H, n, generator=g, dtype=torch.float64) for n in lengths]
    rect = torch.full((len(lengths), 1, H, W), float("nan"), dtype=torch.float64)        # the tail is poison
    for r, x in enumerate(rows):
        rect[r, :, :, :x.shape[-1]] = x[0]
    y, w = _mini_forward(net, rect, list(lengths))
    for r, x in enumerate(rows):
        ref, _ = _mini_forward(net, x)
        assert ref.shape[-1] == w[r], (lengths[r], ref.shape[-1], w[r])                  # the formula's final width
        assert torch.equal(y[r, :, :, :w[r]], ref[0]), lengths[r]                        # difference 0
        assert torch.equal(y[r, :, :, w[r]:], torch.zeros_like(y[r, :, :, w[r]:]))       # the tail is exactly 0
    if 9 in lengths:
        assert w[lengths.index(9)] == 2


# ---- the engine's dry run ---------------------------------------------------------------------------------------------
_COUNT_SCRIPT = r"""
import sys, json
import numpy as np
from wesep_amd import engine as E
path, Te = sys.argv[1], [int(v) for v in sys.argv[2].split(",")]
eng = E.Engine(path, dry_run=True)
mixes = [np.zeros(n, np.float32) for n in (16000, 9000, 12345)][:len(Te)]
eng.separate_ragged(mixes, [np.zeros((t, 80), np.float32) for t in Te], E.ENROLL_FBANK)
print(json.dumps([eng.info("ragged_speaker"), eng.info("n_launches")]))
"""


def _loop_count(path, Te):
    """[ragged_speaker, n_launches] of the same call in a process with WS_ENGINE_RAGGED_SPK=0 (read once per process)."""
    import json
    env = dict(os.environ, WS_ENGINE_RAGGED_SPK="0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _COUNT_SCRIPT, path, ",".join(str(t) for t in Te)], capture_output=True,
                       text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout.strip().splitlines()[-1])


def _stage_counts(tmp_path, spk_model, spk_args, emb_dim):
    """(engine of the joint container, separator launches of a ragged (3, 16000) call, speaker-stage launches of one row of
    98 / 120 / 33 frames):
    the separator alone is the same separator with fixed embeddings; one row's speaker stage is what a one-row joint call
    adds to it."""
    path = str(tmp_path / "j.wsw")
    export_engine(_joint(spk_model, spk_args, spk_emb_dim=emb_dim), path)
    fixed = str(tmp_path / "f.wsw")
    export_engine(_bsrnn(joint_training=False, spk_emb_dim=emb_dim), fixed)
    mixes = [np.zeros(n, np.float32) for n in (16000, 9000, 12345)]
    fx = E.Engine(fixed, dry_run=True)
    fx.separate_ragged(mixes, [np.zeros(emb_dim, np.float32)] * 3, E.ENROLL_EMBEDDING)
    n_sep3 = fx.info("n_launches")
    fx.separate(np.zeros((1, 16000), np.float32), np.zeros((1, emb_dim), np.float32), E.ENROLL_EMBEDDING)
    n_sep1 = fx.info("n_launches")
    fx.close()
    eng = E.Engine(path, dry_run=True)
    per_row = {}
    for te in (98, 120, 33):
        eng.separate(np.zeros((1, 16000), np.float32), np.zeros((1, te, 80), np.float32), E.ENROLL_FBANK)
        per_row[te] = eng.info("n_launches") - n_sep1
    return path, eng, mixes, n_sep3, per_row


@needs_no_gpu
@pytest.mark.parametrize("spk_model,spk_args,emb", [
    ("ResNet34", RESNET_SPK, 256),
    ("ECAPA_TDNN_c512", dict(feat_dim=80, embed_dim=192, pooling_func="ASTP"), 192)], ids=["resnet34_tstp", "ecapa_c512_astp"])
def test_dry_run_batched_speaker_stage_launch_counts(tmp_path, spk_model, spk_args, emb):
    path, eng, mixes, n_sep, per_row = _stage_counts(tmp_path, spk_model, spk_args, emb)
    assert len(set(per_row.values())) == 1, per_row    # one row's speaker stage does not depend on its frame count
    n_spk1 = per_row[98]
    assert eng.info("ragged_speaker") == 1
    counts = set()
    for Te in ((98, 120, 33), (120, 77, 98), (120, 120, 120), (120, 9, 17)):
        eng.separate_ragged(mixes, [np.zeros((t, 80), np.float32) for t in Te], E.ENROLL_FBANK)
        counts.add(eng.info("n_launches"))
    assert len(counts) == 1, counts                    # for a fixed rectangle the plan does not depend on the lengths
    n_batched = counts.pop()
    print(f"{spk_model}: separator {n_sep}, speaker stage of one row {n_spk1}, ragged call of 3 rows {n_batched}")
    assert n_batched - n_sep < 1.25 * n_spk1 < 3 * n_spk1                 # one pass, not three
    # against the rectangular call of the same (R, T): + the tail select of the uploaded features; the SE mean of
    # ECAPA-TDNN is one length-aware launch instead of the three of the rectangular mean
    eng.separate(np.zeros((3, 16000), np.float32), np.zeros((3, 120, 80), np.float32), E.ENROLL_FBANK)
    assert n_batched - eng.info("n_launches") == (1 if spk_model.startswith("ResNet") else 1 - 3 * 2)
    # waveform enrollment: + the front-end, still one pass
    eng.separate_ragged(mixes, [np.zeros(n, np.float32) for n in (24001, 16000, 30000)], E.ENROLL_WAVE)
    n_wave = eng.info("n_launches")
    assert n_batched < n_wave < n_batched + 16
    # the refusals of the loop hold per row, with their messages
    with pytest.raises(E.WesepHipError, match="too short for the speaker encoder"):
        eng.separate_ragged(mixes, [np.zeros((t, 80), np.float32) for t in (98, 5, 33)], E.ENROLL_FBANK)
    with pytest.raises(E.WesepHipError, match="shorter than one"):
        eng.separate_ragged(mixes, [np.zeros(n, np.float32) for n in (24001, 100, 30000)], E.ENROLL_WAVE)
    eng.close()
    # WS_ENGINE_RAGGED_SPK=0: one enrollment at a time -- the separator plus one row's speaker stage per row
    flag, n_loop = _loop_count(path, (98, 120, 33))
    assert flag == 0 and n_loop == n_sep + sum(per_row.values()), (n_loop, n_sep, per_row)
    assert n_batched < n_loop


@needs_no_gpu
def test_dry_run_mel_frontend_model_takes_the_batched_stage(tmp_path):
    path = str(tmp_path / "m.wsw")
    export_engine(_bsrnn(joint_training=True, spk_feat=False, spk_model="ResNet18", spk_args=RESNET_SPK), path)
    eng = E.Engine(path, dry_run=True)
    assert eng.info("ragged_speaker") == 1
    mixes = [np.zeros(n, np.float32) for n in (16000, 9000)]
    counts = set()
    for ns in ((24001, 16000), (24001, 24001), (24001, 1100)):
        eng.separate_ragged(mixes, [np.zeros(n, np.float32) for n in ns], E.ENROLL_WAVE)
        counts.add(eng.info("n_launches"))
    assert len(counts) == 1, counts
    with pytest.raises(E.WesepHipError, match="longer than the 256-sample reflect padding"):
        eng.separate_ragged(mixes, [np.zeros(n, np.float32) for n in (24001, 256)], E.ENROLL_WAVE)
    eng.close()


@needs_no_gpu
def test_dry_run_campplus_and_mhastp_keep_the_loop(tmp_path):
    for sub, spk_model, spk_args, emb in (("c", "CAMPPlus", dict(feat_dim=80, embed_dim=512, pooling_func="TSTP"), 512),
                                          ("m", "ResNet18", dict(RESNET_SPK, pooling_func="MHASTP"), 256)):
        (tmp_path / sub).mkdir()
        path, eng, mixes, n_sep, per_row = _stage_counts(tmp_path / sub, spk_model, spk_args, emb)
        assert eng.info("ragged_speaker") == 0
        eng.separate_ragged(mixes, [np.zeros((t, 80), np.float32) for t in (98, 120, 33)], E.ENROLL_FBANK)
        assert eng.info("n_launches") == n_sep + sum(per_row.values()), spk_model      # one enrollment at a time, as before
        eng.close()


# ---- separate_main --sort_by_length ----------------------------------------------------------------------------------
def _write_wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


def sorted_groups(lens, batch):
    """The rule of --sort_by_length: lines ordered by mixture sample count, longest first, stable; grouped N at a time."""
    order = np.argsort(-np.asarray(lens), kind="stable")
    return [order[i:i + batch].tolist() for i in range(0, len(lens), batch)]


def test_sorted_grouping_rule():
    assert sorted_groups([5, 9, 5, 7], 3) == [[1, 3, 0], [2]]                  # ties keep the scp order
    assert sorted_groups([1, 2, 3], 8) == [[2, 1, 0]]


@needs_no_gpu
def test_separate_main_sort_by_length_dry_run(tmp_path):
    exe = os.path.join(ROOT, "runtime", "separate_main")
    assert os.path.exists(exe), "run python -m wesep_amd.build"
    model = str(tmp_path / "j.wsw")
    export_engine(_joint("ResNet18", RESNET_SPK), model)
    rng = np.random.default_rng(0)
    lens = (24000, 16000, 40000, 8000, 12352, 16000, 40000)
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1000 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 1000 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    run = lambda *extra: subprocess.run([exe, "--wav_scp", str(scp), "--model", model, "--dry_run", *extra],
                                        capture_output=True, text=True, timeout=120)
    total = f"Total: process {sum(lens) * 1000 // 16000}ms audio"
    r = run("--batch", "3", "--sort_by_length")
    assert r.returncode == 0, r.stderr
    proc = [l for l in r.stdout.splitlines() if l.startswith("process:")]
    keys = [l.split()[1] for l in proc]
    assert sorted(keys) == sorted(f"u{i}" for i in range(len(lens)))                     # every key once
    want = sorted_groups(lens, 3)
    assert keys == [f"u{i}" for g in want for i in g]                                    # processing order = the rule's order
    sizes = [int(re.search(r"batch of (\d+)", l).group(1)) for l in proc]
    assert sizes == [len(g) for g in want for _ in g]                                    # ... grouped as the rule groups
    assert total in r.stdout
    # with the flag off: the format the tool always printed, line for line
    r0 = run("--batch", "3")
    assert r0.returncode == 0
    out = r0.stdout.splitlines()
    for i, l in enumerate(out[:len(lens)]):
        b = 3 if i < 6 else 1
        assert re.fullmatch(rf"process: u{i} RTF: [0-9.]+ \(batch of {b}: \d+ launches, \d+ MiB arena\) \[dry run\]", l), l
    assert re.fullmatch(r"Total: process \d+ms audio taken \d+ms\.", out[len(lens)]) and out[len(lens) + 1].startswith("RTF: ")
    assert len(out) == len(lens) + 2
    # without --batch the flag is accepted and changes nothing
    strip = lambda s: [re.sub(r"RTF: [0-9.]+|taken \d+ms", "", l) for l in s.splitlines()]
    ra, rb = run("--sort_by_length"), run()
    assert ra.returncode == 0 and rb.returncode == 0 and strip(ra.stdout) == strip(rb.stdout)
    # the rule reads the headers: a mixture that is not a wav file is reported before any forward
    bad = tmp_path / "bad.scp"
    (tmp_path / "junk.wav").write_bytes(b"not a wav")
    bad.write_text(lines[0] + f"s {tmp_path}/junk.wav {tmp_path}/a0.wav {tmp_path}/b0.wav\n")
    r = subprocess.run([exe, "--wav_scp", str(bad), "--model", model, "--dry_run", "--batch", "2", "--sort_by_length"],
                       capture_output=True, text=True)
    assert r.returncode == 1 and "not a RIFF/WAVE file" in r.stderr and "process:" not in r.stdout


# ---- the Python surface ------------------------------------------------------------------------------------------------
def test_python_surface_lengths_are_inference_only_and_name_what_is_not_built():
    from wesep_amd.models.resnet import get_speaker_model
    x = torch.zeros(2, 40, 80)
    res = get_speaker_model("ResNet18")(feat_dim=80, embed_dim=64, pooling_func="TSTP", two_emb_layer=False)
    eca = get_speaker_model("ECAPA_TDNN_c512")(feat_dim=80, embed_dim=64)
    for m in (res, eca):
        m.train()
        with torch.no_grad(), pytest.raises(L.WesepHipError, match="inference"):
            m(x, lengths=[40, 30])                                     # training mode: batch statistics over ragged rows
        m.eval()
        with pytest.raises(L.WesepHipError, match="inference"):
            m(x, lengths=[40, 30])                                     # gradients enabled
        with torch.no_grad(), pytest.raises(L.WesepHipError, match="no CPU path"):
            m(x, lengths=[40, 30])
    for make in (lambda: get_speaker_model("ResNet18")(feat_dim=80, embed_dim=64, pooling_func="MHASTP", two_emb_layer=False),
                 lambda: get_speaker_model("ECAPA_TDNN_c512")(feat_dim=80, embed_dim=64, pooling_func="MQMHASTP")):
        m = make().eval()
        with torch.no_grad(), pytest.raises(NotImplementedError, match="MHASTP"):
            m(x, lengths=[40, 30])
    # BSRNN: keyword only, inference only, joint models only, CAM++ refused by name
    fixed = _bsrnn(joint_training=False).eval()
    wav, emb = torch.zeros(2, 4000), torch.zeros(2, 256)
    with pytest.raises(TypeError):
        fixed(wav, emb, None, [40, 30])
    with torch.no_grad(), pytest.raises(L.WesepHipError, match="fixed embeddings"):
        fixed._speaker(emb, [40, 30])
    joint = _joint("ResNet18", RESNET_SPK)
    with pytest.raises(L.WesepHipError, match="inference"):
        joint.eval()._speaker(torch.zeros(2, 40, 80), [40, 30])
    with torch.no_grad(), pytest.raises(L.WesepHipError, match="inference"):
        joint.train()._speaker(torch.zeros(2, 40, 80), [40, 30])
    cam = _joint("CAMPPlus", dict(feat_dim=80, embed_dim=512, pooling_func="TSTP"), spk_emb_dim=512).eval()
    with torch.no_grad(), pytest.raises(NotImplementedError, match="CAMPPlus"):
        cam._speaker(torch.zeros(2, 40, 80), [40, 30])
    import inspect
    from wesep_amd.bin import infer
    from wesep_amd.modules.common.frontend import fbank_frontend, frontend_frames
    assert "enroll_lengths" in inspect.signature(infer.extract).parameters
    assert "lengths" in inspect.signature(fbank_frontend).parameters
    assert frontend_frames([257, 383, 384, 16000]) == [3, 3, 4, 126]
