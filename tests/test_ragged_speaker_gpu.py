"""GPU: the ragged speaker stage -- enrollments of any length in one encoder pass.  Every comparison is against
something other than the code under test: the rectangular kernel on the row alone, numpy fp64 on the truncated row, the
torch restatements of oracle/, the same engine with the one-row-at-a-time loop (WS_ENGINE_RAGGED_SPK=0, a process of its
own), the Python model on the row alone.  The bounds are those of the tests that cover the rectangular paths:
1e-5 (test_tstp_matches_torch), 1e-3 against the oracles (test_resnet18_matches_oracle), 1e-4 between two device paths
(the ragged engine tests).  Tails are poisoned with NaN wherever the caller owns them."""
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest
import torch

from wesep_amd import dev
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _tab(v, d):
    return torch.tensor(list(v), dtype=torch.int32, device=d)


# ---- kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,H,W,C,widths,with_res,slope", [
    (3, 5, 24, 32, (24, 7, 1), True, 0.0),          # ResNet layout [R][H][W][C], residual, ReLU
    (4, 1, 120, 64, (98, 120, 33, 2), False, 1.0),  # TDNN layout (H = 1), identity activation
    (9, 10, 17, 128, tuple(range(9, 18)), True, 0.0)])
def test_masked_epilogue_is_bn_prelu_fwd_on_each_row_alone_bit_for_bit(R, H, W, C, widths, with_res, slope):
    d = _cuda()
    g = torch.Generator().manual_seed(R * 100 + W)
    x = torch.randn(R, H, W, C, generator=g)
    res = torch.randn(R, H, W, C, generator=g) if with_res else None
    for r, w in enumerate(widths):                                       # what lies behind a row's width is poison
        x[r, :, w:] = NAN
        if with_res:
            res[r, :, w:] = NAN
    st = torch.stack([0.3 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)]).to(d)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(d), (0.3 * torch.randn(C, generator=g)).to(d)
    a = torch.full((1,), slope, device=d)
    xd, rd = x.to(d), (res.to(d) if with_res else None)
    u, y = torch.full_like(xd, 7.0), torch.full_like(xd, 7.0)
    dev.bn_prelu_fwd_len(xd, st, gamma, beta, rd, a, R * H * W, C, H * W, W, _tab(widths, d), u, y)
    torch.cuda.synchronize()
    for r, w in enumerate(widths):
        xr = xd[r, :, :w].contiguous()
        rr = rd[r, :, :w].contiguous() if with_res else None
        ur, yr = torch.empty_like(xr), torch.empty_like(xr)
        dev.bn_prelu_fwd(xr, st, gamma, beta, rr, a, H * w, C, ur, yr)
        assert torch.equal(y[r, :, :w], yr) and torch.equal(u[r, :, :w], ur), (r, w)          # bit for bit
        assert not y[r, :, w:].any() and not u[r, :, w:].any(), (r, w)                       # exact zeros behind
        assert torch.isfinite(yr).all()


def test_length_aware_tstp_vs_numpy_fp64_on_the_truncated_row():
    d = _cuda()
    g = torch.Generator().manual_seed(2)
    for R, Fq, T, C, tl in ((3, 5, 17, 8, (17, 2, 9)), (4, 10, 50, 256, (50, 13, 2, 31)), (3, 1, 120, 1536, (98, 120, 33))):
        x = torch.randn(R, Fq, T, C, generator=g) * 2 + 1
        for r, n in enumerate(tl):
            x[r, :, n:] = NAN
        stats = torch.empty(R, 2 * C * Fq, device=d)
        dev.tstp_fwd_len(x.to(d), R, Fq, T, C, _tab(tl, d), stats)
        alone = torch.empty(1, 2 * C * Fq, device=d)
        for r, n in enumerate(tl):
            v = x[r, :, :n].double().numpy()                              # [F, n, C]
            mean = v.mean(1).T.reshape(-1)                                # feature index c * F + f
            std = np.sqrt(v.var(1, ddof=1) + 1e-7).T.reshape(-1)
            e = rel(stats[r], np.concatenate([mean, std]))
            dev.tstp_fwd(x[r, :, :n].contiguous().to(d), 1, Fq, n, C, alone)
            same = torch.equal(stats[r], alone[0])
            print(f"tstp_len R={R} F={Fq} C={C} row {r} ({n} of {T}): rel vs fp64 {e:.2e}; bit-identical to ws_tstp_fwd alone: {same}")
            assert e < 1e-5, (r, n, e)
            assert rel(stats[r], alone[0]) < 1e-6


def test_length_aware_astp_vs_numpy_fp64_on_the_truncated_row():
    d = _cuda()
    g = torch.Generator().manual_seed(3)
    for R, T, C, tl in ((3, 17, 8, (17, 2, 9)), (3, 120, 1536, (98, 120, 33))):
        x, lg = torch.randn(R, T, C, generator=g) * 2 + 1, 2 * torch.randn(R, T, C, generator=g)
        for r, n in enumerate(tl):
            x[r, n:] = NAN
            lg[r, n:] = NAN
        out, aux = torch.empty(R, 2 * C, device=d), torch.empty(R, 4 * C, device=d)
        dev.astp_fwd_len(x.to(d), lg.to(d), R, T, C, _tab(tl, d), out, aux)
        o1, a1 = torch.empty(1, 2 * C, device=d), torch.empty(1, 4 * C, device=d)
        for r, n in enumerate(tl):
            v, l = x[r, :n].double().numpy(), lg[r, :n].double().numpy()
            al = np.exp(l - l.max(0))
            al /= al.sum(0)
            mean = (al * v).sum(0)
            std = np.sqrt(np.maximum((al * v * v).sum(0) - mean ** 2, 1e-7))
            e = rel(out[r], np.concatenate([mean, std]))
            dev.astp_fwd(x[r, :n].contiguous().to(d), lg[r, :n].contiguous().to(d), 1, n, C, o1, a1)
            print(f"astp_len C={C} row {r} ({n} of {T}): rel vs fp64 {e:.2e}; bit-identical to ws_astp_fwd alone: "
                  f"{torch.equal(out[r], o1[0])}")
            assert e < 1e-5, (r, n, e)
            assert torch.isfinite(aux[r]).all()


def test_length_aware_cmn_time_mean_and_tail_select_vs_numpy_fp64():
    d = _cuda()
    g = torch.Generator().manual_seed(4)
    for R, T, C, tl in ((3, 120, 80, (98, 120, 33)), (4, 37, 512, (37, 1, 8, 20)), (2, 301, 60, (300, 9))):
        x = torch.randn(R, T, C, generator=g) * 3 - 2
        for r, n in enumerate(tl):
            x[r, n:] = NAN
        xd, tab = x.to(d), _tab(tl, d)
        y, mean, sel = torch.full_like(xd, 7.0), torch.empty(R, C, device=d), torch.full_like(xd, 7.0)
        dev.cmn_len(xd, R, T, C, tab, y)
        dev.time_mean_len(xd, R, T, C, tab, mean)
        dev.tail_select_len(xd, R, T, C, tab, sel)
        inplace = xd.clone()
        dev.cmn_len(inplace, R, T, C, tab, inplace)
        assert torch.equal(inplace, y)                                    # y may be x
        for r, n in enumerate(tl):
            v = x[r, :n].double().numpy()
            assert rel(mean[r], v.mean(0)) < 1e-5
            e = rel(y[r, :n], v - v.mean(0))
            print(f"cmn_len C={C} row {r} ({n} of {T}): rel vs fp64 {e:.2e}")
            assert e < 1e-5, (r, n, e)
            assert not y[r, n:].any() and not sel[r, n:].any()            # exact zeros, not NaN * 0
            assert torch.equal(sel[r, :n], xd[r, :n])


def test_length_aware_preemph_pad_turns_at_the_rows_own_end():
    d = _cuda()
    g = torch.Generator().manual_seed(5)
    R, T, pad, coef = 3, 4000, 256, 0.97
    lens = (4000, 257, 1234)
    ldo = -(-(T + 2 * pad) // 4) * 4
    x = torch.randn(R, T, generator=g)
    for r, n in enumerate(lens):
        x[r, n:] = NAN
    out = torch.full((R, ldo), 7.0, device=d)
    out[:, T + 2 * pad:] = 0
    dev.preemph_pad_len(x.to(d), R, T, pad, ldo, coef, _tab(lens, d), out)
    for r, n in enumerate(lens):
        v = x[r, :n].double().numpy()
        yv = v - coef * np.concatenate([v[1:2], v[:-1]])
        ref = np.pad(yv, pad, mode="reflect")
        assert rel(out[r, :n + 2 * pad], ref) < 1e-6, r
        assert not out[r, n + 2 * pad:].any(), r
        alone = torch.zeros(1, n + 2 * pad, device=d)
        dev.preemph_pad(x[r:r + 1, :n].contiguous().to(d), 1, n, pad, n + 2 * pad, coef, alone)
        assert torch.equal(out[r, :n + 2 * pad], alone[0]), r             # the rectangular kernel on the row alone, bit for bit


# ---- the Python encoders with lengths= ---------------------------------------------------------------------------------
def _randomise_running_stats(params, seed):
    g = torch.Generator().manual_seed(seed)
    for k, v in params.items():
        if k.endswith("running_mean"):
            v.copy_(0.2 * torch.randn(v.shape, generator=g))
        elif k.endswith("running_var"):
            v.copy_(0.5 + torch.rand(v.shape, generator=g))


def _check_rows(model, oracle_fwd, x, lengths, d, what, pick=lambda o: o[-1] if isinstance(o, tuple) else o):
    """model(rect with NaN tails, lengths=) row by row: against the oracle on the truncated row (1e-3) and against the
    same module on the row alone (1e-4; reported: bit-identical or not)."""
    rect = x.clone()
    for r, n in enumerate(lengths):
        rect[r, n:] = NAN
    with torch.no_grad():
        got = pick(model(rect.to(d), lengths=list(lengths)))
        assert torch.isfinite(got).all(), what
        for r, n in enumerate(lengths):
            row = x[r:r + 1, :n].contiguous()
            alone = pick(model(row.to(d)))[0]
            ref = pick(oracle_fwd(row))[0]
            e_or, e_al = rel(got[r], ref), rel(got[r], alone)
            print(f"{what} row {r} ({n} of {x.shape[1]} frames): rel vs oracle {e_or:.2e}, vs the row alone {e_al:.2e}, "
                  f"bit-identical to the row alone: {torch.equal(got[r], alone)}")
            assert e_or < 1e-3, (what, r, e_or)
            assert e_al < 1e-4, (what, r, e_al)


@pytest.mark.parametrize("name,two_emb,pooling,lengths", [
    ("ResNet18", False, "TSTP", (98, 120, 33)),
    ("ResNet18", False, "TSTP", tuple(range(9, 18))),
    ("ResNet50", True, "TSTP", (120, 77, 98)),
    ("ResNet18", False, "TSDP", (64, 17, 40)),
    ("ResNet18", False, "ASTP", (64, 17, 40))], ids=["basic", "basic_9_to_17", "bottleneck_two_emb", "tsdp", "astp"])
def test_resnet_with_lengths_matches_oracle_and_the_row_alone(name, two_emb, pooling, lengths):
    from oracle import resnet_oracle as RO
    from wesep_amd.models.resnet import get_speaker_model
    d = _cuda()
    bott = name in RO.BOTTLENECK
    kw = dict(num_blocks=RO.NUM_BLOCKS[name], m=32, feat_dim=16, embed_dim=64)
    params = RO.synth_params(5, bottleneck=bott, two_emb_layer=two_emb, pooling=pooling, **kw)
    _randomise_running_stats(params, 6)
    model = get_speaker_model(name)(feat_dim=16, embed_dim=64, pooling_func=pooling, two_emb_layer=two_emb)
    model.load_state_dict(params, strict=True)
    model = model.to(d).eval()
    x = torch.randn(len(lengths), max(lengths), 16, generator=torch.Generator().manual_seed(9))
    oracle = lambda row: RO.resnet_forward(params, row, num_blocks=kw["num_blocks"], m=32, training=False, bottleneck=bott,
                                           two_emb_layer=two_emb, pooling=pooling)
    _check_rows(model, oracle, x, lengths, d, f"{name} {pooling}")


@pytest.mark.parametrize("glob,emb_bn,lengths", [(False, False, (98, 120, 33)), (True, True, (120, 77, 98))],
                         ids=["c512", "glob_c512_emb_bn"])
def test_ecapa_with_lengths_matches_oracle_and_the_row_alone(glob, emb_bn, lengths):
    from oracle import ecapa_oracle as EO
    from wesep_amd.models.ecapa_tdnn import ECAPA_TDNN
    d = _cuda()
    params = EO.synth_params(7, channels=512, feat_dim=80, embed_dim=192, global_context_att=glob, emb_bn=emb_bn)
    _randomise_running_stats(params, 8)
    model = ECAPA_TDNN(channels=512, feat_dim=80, embed_dim=192, global_context_att=glob, emb_bn=emb_bn)
    model.load_state_dict(params, strict=True)
    model = model.to(d).eval()
    x = torch.randn(len(lengths), max(lengths), 80, generator=torch.Generator().manual_seed(10))
    oracle = lambda row: EO.ecapa_forward(params, row, global_context_att=glob, emb_bn=emb_bn, training=False)
    _check_rows(model, oracle, x, lengths, d, f"ECAPA-TDNN c512 glob={glob}")


def test_fbank_frontend_with_lengths_matches_the_row_alone():
    from wesep_amd.models import get_model
    from wesep_amd.modules.common.frontend import fbank_frontend, frontend_frames
    d = _cuda()
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                               joint_training=True, spk_feat=False, spk_model="ResNet18",
                               spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False)).to(d)
    lens = (24001, 16000, 1100)
    wav = 0.1 * torch.randn(3, max(lens), generator=torch.Generator().manual_seed(11))
    rect = wav.clone()
    for r, n in enumerate(lens):
        rect[r, n:] = NAN
    feats = fbank_frontend(rect.to(d), model.preEmphasis, model.spk_encoder, lengths=list(lens))
    for r, (n, te) in enumerate(zip(lens, frontend_frames(lens))):
        alone = fbank_frontend(wav[r:r + 1, :n].contiguous().to(d), model.preEmphasis, model.spk_encoder)[0]
        e = rel(feats[r, :te], alone)
        print(f"fbank_frontend(lengths=) row {r} ({n} samples, {te} frames): rel vs the row alone {e:.2e}")
        assert alone.shape[0] == te and e < 1e-4 and not feats[r, te:].any()


# ---- the engine --------------------------------------------------------------------------------------------------------
_LOOP_SCRIPT = r"""
import sys
import numpy as np
from wesep_amd import engine as E
path, npz, out = sys.argv[1:4]
z = np.load(npz)
eng = E.Engine(path)
assert eng.info("ragged_speaker") == 0
mix, enroll = np.ascontiguousarray(z["mix"]), np.ascontiguousarray(z["enroll"])
lengths, elens = np.ascontiguousarray(z["lengths"]), np.ascontiguousarray(z["elens"])
est = np.zeros_like(mix)
rc = E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, mix.shape[0], mix.shape[1], lengths.ctypes.data,
                                       enroll.ctypes.data, int(z["kind"]), enroll.shape[1], elens.ctypes.data, est.ctypes.data)
assert rc == 0, E.lib().ws_engine_last_error()
np.save(out, est)
"""


def _ragged_call(eng, mix, lengths, enroll, kind, elens):
    est = np.zeros_like(mix)
    rc = E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, mix.shape[0], mix.shape[1], lengths.ctypes.data,
                                           enroll.ctypes.data, kind, enroll.shape[1], elens.ctypes.data, est.ctypes.data)
    assert rc == 0, E.lib().ws_engine_last_error().decode()
    return est


def _loop_arm(tmp_path, path, mix, lengths, enroll, kind, elens, tag):
    """The same call on the same container in a fresh process with WS_ENGINE_RAGGED_SPK=0 (read once per process)."""
    npz, out = str(tmp_path / f"in_{tag}.npz"), str(tmp_path / f"out_{tag}.npy")
    np.savez(npz, mix=mix, lengths=lengths, enroll=enroll, elens=elens, kind=kind)
    r = subprocess.run([sys.executable, "-c", _LOOP_SCRIPT, path, npz, out], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, WS_ENGINE_RAGGED_SPK="0", PYTHONPATH=ROOT), cwd=ROOT)
    assert r.returncode == 0, r.stderr
    return np.load(out)


@pytest.mark.parametrize("spk_model,spk_feat,spk_args,emb", [
    ("ResNet18", True, dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False), 256),
    ("ResNet18", False, dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False), 256),
    ("ECAPA_TDNN_GLOB_c512", True, dict(feat_dim=80, embed_dim=192, pooling_func="ASTP"), 192)],
    ids=["resnet18_kaldi", "resnet18_mel", "ecapa_glob_kaldi"])
def test_engine_enroll_lengths_batched_stage_vs_loop_and_python_rows(tmp_path, spk_model, spk_feat, spk_args, emb):
    from wesep_amd.models import get_model
    from wesep_amd.utils.funcs import apply_cmvn, compute_fbank
    d = _cuda()
    torch.manual_seed(5)
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                               joint_training=True, spk_model=spk_model, spk_feat=spk_feat, spk_args=spk_args, spk_emb_dim=emb)
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.2)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    path = str(tmp_path / "j.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    assert eng.info("ragged_speaker") == 1
    model = model.to(d).eval()
    g = torch.Generator().manual_seed(3)
    lengths = np.array([20000, 12345, 7000], np.int32)
    wav = 0.1 * torch.randn(3, 20000, generator=g)
    mix = wav.numpy().copy()
    for r, n in enumerate(lengths):
        mix[r, n:] = NAN
    cases = []
    if spk_feat:
        te = np.array([120, 77, 98], np.int32)
        fb = torch.randn(3, 120, 80, generator=g)
        for r, n in enumerate(te):
            fb[r, :n] -= fb[r, :n].mean(0, keepdim=True)
        cases.append(("fbank", E.ENROLL_FBANK, fb, te))
    ns = np.array([30001, 24000, 16123], np.int32)
    cases.append(("wave", E.ENROLL_WAVE, 0.1 * torch.randn(3, 30001, generator=g), ns))
    for tag, kind, enr, elens in cases:
        rect = enr.numpy().copy()
        for r, n in enumerate(elens):
            rect[r, n:] = NAN                                             # the caller's tail: poison
        est = _ragged_call(eng, mix, lengths, rect, kind, elens)
        loop = _loop_arm(tmp_path, path, mix, lengths, rect, kind, elens, tag)
        with torch.no_grad():
            py = model(torch.nan_to_num(torch.from_numpy(mix)).to(d), torch.from_numpy(rect).to(d),
                       lengths=lengths.tolist(), enroll_lengths=elens.tolist())[0].cpu().numpy() \
                if (kind == E.ENROLL_FBANK or not spk_feat) else None
        for r, n in enumerate(lengths):
            assert np.isfinite(est[r, :n]).all() and not est[r, n:].any()
            row = enr[r:r + 1, :int(elens[r])].contiguous().to(d)
            with torch.no_grad():
                if kind == E.ENROLL_WAVE and spk_feat:
                    row = apply_cmvn(compute_fbank(row, dither=0.0))
                ref = model(wav[r:r + 1, :n].contiguous().to(d), row)[0][0]
            e_loop, e_py = rel(est[r, :n], loop[r, :n]), rel(est[r, :n], ref)
            msg = f"engine {spk_model} {tag} row {r}: rel vs the loop {e_loop:.2e} " \
                  f"(bit-identical: {np.array_equal(est[r, :n], loop[r, :n])}), vs the Python model on the row alone {e_py:.2e}"
            if py is not None:
                e_pr = rel(py[r, :n], ref)
                msg += f"; BSRNN.forward(enroll_lengths=) vs the row alone {e_pr:.2e}"
                assert e_pr < 1e-4, (tag, r, e_pr)
            print(msg)
            assert e_loop < 1e-4, (tag, r, e_loop)
            assert e_py < 1e-4, (tag, r, e_py)
    eng.close()


def _write_wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


def test_separate_main_batch_4_sorted_against_batch_1(tmp_path):
    from wesep_amd.models import get_model
    _cuda()
    exe = os.path.join(ROOT, "runtime", "separate_main")
    torch.manual_seed(8)
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                               joint_training=True, spk_model="ResNet18", spk_feat=True,
                               spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False))
    path = str(tmp_path / "j.wsw")
    export_engine(model, path)
    rng = np.random.default_rng(4)
    lens = (24000, 16000, 33333, 8000, 12345, 20480)
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1111 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 999 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    outs = {}
    for tag, extra in (("b1", ["--batch", "1"]), ("b4s", ["--batch", "4", "--sort_by_length"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        outs[tag] = (out, r.stdout)
    order = np.argsort(-np.asarray(lens), kind="stable")
    keys = [l.split()[1] for l in outs["b4s"][1].splitlines() if l.startswith("process:")]
    assert keys == [f"u{i}" for i in order]
    assert sorted(os.listdir(outs["b1"][0])) == sorted(os.listdir(outs["b4s"][0]))         # the same files, by name
    for i, n in enumerate(lens):
        for k in (1, 2):
            a = np.fromfile(outs["b1"][0] / f"u{i}-spk{k}.f32", dtype=np.float32)
            b = np.fromfile(outs["b4s"][0] / f"u{i}-spk{k}.f32", dtype=np.float32)
            e = rel(b, a)
            print(f"separate_main --batch 4 --sort_by_length vs --batch 1, u{i} spk{k} ({n} samples): rel {e:.2e}")
            assert a.shape == b.shape == (n,) and e < 1e-4, (i, k, e)
