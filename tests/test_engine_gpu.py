"""GPU: the native runtime (runtime/*.cc behind include/wesep_engine.h) against the Python module tree on the
same device (same kernels, weights packed once instead of per call -> agreement to rounding), against the CPU oracle,
and the `separate_main` tool end to end."""
import os
import subprocess
import wave

import numpy as np
import pytest
import torch

from oracle import bsrnn_oracle as O
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPK_ARGS = dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False)


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


@pytest.mark.parametrize("kw,seed", [
    (dict(num_repeat=2, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False), 11),
    (dict(num_repeat=2, spk_fuse_type="FiLM", multi_fuse=True, use_spk_transform=False), 12),
    (dict(num_repeat=1, spk_fuse_type="additive", multi_fuse=False, use_spk_transform=True), 13),
    (dict(num_repeat=1, spk_fuse_type="concat", multi_fuse=True, use_spk_transform=False), 14)],
    ids=["multiply", "FiLM", "additive_xform", "concat"])
def test_engine_matches_python_model_and_oracle(tmp_path, kw, seed):
    from wesep_amd.models import get_model
    d = _cuda()
    cfg = O.BSRNNConfig(**kw)
    params = O.synth_params(cfg, seed)
    model = get_model("BSRNN")(joint_training=False, **kw)
    model.load_state_dict(params, strict=True)
    path = str(tmp_path / "m.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    model = model.to(d).eval()
    first = None
    for R, T in ((2, 16000), (3, 12345), (1, 4096), (2, 16000)):          # ragged, odd rows, repeat of the first geometry
        wav, _, emb = O.synth_batch(2 * ((R + 1) // 2), T, seed + T)
        wav, emb = wav[:R].contiguous(), emb[:R].contiguous()
        est = eng.separate(wav.numpy(), emb.numpy(), E.ENROLL_EMBEDDING)
        with torch.no_grad():
            ref = model(wav.to(d), emb.to(d))[0]
        assert rel(est, ref) < 1e-4, (R, T)
        if T <= 12345:
            assert rel(est, O.bsrnn_forward(params, cfg, wav, emb)) < 1e-3, (R, T)
        if first is None:
            first = est
    assert eng.info("n_launches") > 0 and eng.info("arena_bytes") > 0
    eng.close()


def _joint(tmp_path, spk_model, d, seed=5, spk_args=SPK_ARGS, **kw):
    from wesep_amd.models import get_model
    torch.manual_seed(seed)
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                               joint_training=True, spk_model=spk_model, spk_feat=True, spk_args=spk_args, **kw)
    with torch.no_grad():                                   # non-trivial BatchNorm running statistics
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.2)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    path = str(tmp_path / "j.wsw")
    export_engine(model, path)
    return model.to(d).eval(), E.Engine(path)


@pytest.mark.parametrize("spk_model", ["ResNet18", "ResNet34"])
def test_engine_joint_model_fbank_and_waveform_enrollment(tmp_path, spk_model):
    from wesep_amd.utils.funcs import apply_cmvn, compute_fbank
    d = _cuda()
    model, eng = _joint(tmp_path, spk_model, d)
    g = torch.Generator().manual_seed(3)
    wav = 0.1 * torch.randn(2, 20000, generator=g)
    fbank = torch.randn(2, 120, 80, generator=g)
    fbank = fbank - fbank.mean(1, keepdim=True)
    with torch.no_grad():
        ref = model(wav.to(d), fbank.to(d))[0]
    assert rel(eng.separate(wav.numpy(), fbank.numpy(), E.ENROLL_FBANK), ref) < 1e-4
    enroll = 0.1 * torch.randn(2, 30001, generator=g)       # length not a multiple of 4: scalar-load GEMM path
    with torch.no_grad():
        fb = apply_cmvn(compute_fbank(enroll.to(d), dither=0.0))
        ref = model(wav.to(d), fb)[0]
    est = eng.separate(wav.numpy(), enroll.numpy(), E.ENROLL_WAVE)
    assert rel(est, ref) < 1e-4
    # the reference runtime's call: int16 in, one mixture, two enrollments cut to the shorter one
    mix16 = (wav[0] * 32768).round().clamp(-32768, 32767).to(torch.int16)
    e16 = (enroll * 32768).round().clamp(-32768, 32767).to(torch.int16)
    out = eng.forward_pcm16(mix16.numpy(), e16[0].numpy(), e16[1, :29000].numpy())
    m = (mix16.float() / 32768).repeat(2, 1)
    en = (e16[:, :29000].float() / 32768).contiguous()
    assert rel(out, eng.separate(m.numpy(), en.numpy(), E.ENROLL_WAVE)) < 1e-6
    eng.close()


@pytest.mark.parametrize("spk_model,emb_bn", [("ECAPA_TDNN_GLOB_c512", False), ("ECAPA_TDNN_c512", True)])
def test_engine_ecapa_joint_model(tmp_path, spk_model, emb_bn):
    """The published `bsrnn_ecapa_vox1` layout (wesep/cli/hub.py:86-95): pBSRNN + wespeaker ECAPA-TDNN through the native
    runtime vs the Python module tree in eval mode (same kernels), fbank and raw-waveform enrollment, ragged lengths."""
    from wesep_amd.utils.funcs import apply_cmvn, compute_fbank
    d = _cuda()
    model, eng = _joint(tmp_path, spk_model, d, seed=6, spk_emb_dim=192,
                        spk_args=dict(feat_dim=80, embed_dim=192, pooling_func="ASTP", emb_bn=emb_bn))
    assert eng.info("spk_kind") == 1
    g = torch.Generator().manual_seed(4)
    for R, Te in ((2, 120), (3, 77)):
        wav = 0.1 * torch.randn(R, 12000, generator=g)
        fbank = torch.randn(R, Te, 80, generator=g)
        fbank = fbank - fbank.mean(1, keepdim=True)
        with torch.no_grad():
            ref, emb = model(wav.to(d), fbank.to(d))
        assert float(emb.std()) > 1e-3                     # the embedding is alive (not a constant of the biases)
        assert rel(eng.separate(wav.numpy(), fbank.numpy(), E.ENROLL_FBANK), ref) < 1e-4, (R, Te)
    enroll = 0.1 * torch.randn(2, 20001, generator=g)
    wav = 0.1 * torch.randn(2, 12000, generator=g)
    with torch.no_grad():
        ref = model(wav.to(d), apply_cmvn(compute_fbank(enroll.to(d), dither=0.0)))[0]
    assert rel(eng.separate(wav.numpy(), enroll.numpy(), E.ENROLL_WAVE), ref) < 1e-4
    eng.close()


def test_engine_raw_audio_joint_model(tmp_path):
    """spk_feat = False: the engine's in-model front-end (PreEmphasis + MelSpectrogram + log + CMN) vs the Python one."""
    from wesep_amd.models import get_model
    d = _cuda()
    torch.manual_seed(7)
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                               joint_training=True, spk_model="ResNet18", spk_feat=False, spk_args=SPK_ARGS)
    path = str(tmp_path / "r.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    model = model.to(d).eval()
    g = torch.Generator().manual_seed(8)
    wav = 0.1 * torch.randn(2, 12000, generator=g)
    for Tw in (16000, 12345):
        enroll = 0.1 * torch.randn(2, Tw, generator=g)
        with torch.no_grad():
            ref = model(wav.to(d), enroll.to(d))[0]
        assert rel(eng.separate(wav.numpy(), enroll.numpy(), E.ENROLL_WAVE), ref) < 1e-4, Tw
    eng.close()


def test_separate_main_end_to_end(tmp_path):
    d = _cuda()
    model, eng = _joint(tmp_path, "ResNet18", d)
    rng = np.random.default_rng(1)
    sig = {"mix": rng.integers(-4000, 4000, 24000), "e1": rng.integers(-4000, 4000, 32000),
           "e2": rng.integers(-4000, 4000, 36000)}
    for name, x in sig.items():
        with wave.open(str(tmp_path / f"{name}.wav"), "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(x.astype(np.int16).tobytes())
    (tmp_path / "wav.scp").write_text(f"utt1 {tmp_path}/mix.wav {tmp_path}/e1.wav {tmp_path}/e2.wav\n")
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    r = subprocess.run([os.path.join(ROOT, "runtime", "separate_main"), "--wav_scp", str(tmp_path / "wav.scp"),
                        "--model", str(tmp_path / "j.wsw"), "--output_dir", str(out_dir)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "process: utt1 RTF:" in r.stdout and "Total: process 1500ms audio" in r.stdout
    want = eng.forward_pcm16(sig["mix"].astype(np.int16), sig["e1"].astype(np.int16), sig["e2"].astype(np.int16))
    for i, name in enumerate(("utt1-spk1.wav", "utt1-spk2.wav")):
        with wave.open(str(out_dir / name), "rb") as w:
            assert w.getframerate() == 16000 and w.getnchannels() == 1 and w.getnframes() == 24000
            got = np.frombuffer(w.readframes(24000), dtype=np.int16).astype(np.float32)
        assert np.abs(got - np.clip(np.round(want[i] * 32768), -32768, 32767)).max() <= 1.0
    # concurrent engines (one per worker thread) produce the same files
    (tmp_path / "wav4.scp").write_text("".join(f"c{i} {tmp_path}/mix.wav {tmp_path}/e1.wav {tmp_path}/e2.wav\n"
                                               for i in range(4)))
    r = subprocess.run([os.path.join(ROOT, "runtime", "separate_main"), "--wav_scp", str(tmp_path / "wav4.scp"),
                        "--model", str(tmp_path / "j.wsw"), "--output_dir", str(out_dir), "--jobs", "2"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # byte-identical although the two engines OVERLAP on the GPU (round 3: the library has no packed FP32 instructions, the
    # victim class of the cross-stream disturbance -- profiles/r03_kernel_race.md; round 2 needed a per-device lock here)
    # -- unless a cluster recurrence timed out and the streaming kernels took over (different MFMA order, reported on
    # stdout): then within one 16-bit step
    ref = np.frombuffer((out_dir / "utt1-spk1.wav").read_bytes()[44:], dtype=np.int16).astype(np.int32)
    for i in range(4):
        got = np.frombuffer((out_dir / f"c{i}-spk1.wav").read_bytes()[44:], dtype=np.int16).astype(np.int32)
        if "a cluster recurrence timed out" in r.stdout:
            assert np.abs(got - ref).max() <= 1, r.stdout
        else:
            assert np.array_equal(got, ref), (int(np.abs(got - ref).max()), int((got != ref).sum()), r.stdout)
    eng.close()


def test_engine_reads_no_uninitialised_arena_memory(tmp_path, monkeypatch):
    """WS_ENGINE_POISON=1 starts every arena allocation as NaN: a launch plan that reads memory no kernel has written
    (padding slots, scratch, a stale stack frame) would turn the estimate into NaN instead of making it depend on what
    the arena held before -- which is what two engines sharing a GPU see.  Same bits as the unpoisoned run."""
    d = _cuda()
    model, eng = _joint(tmp_path, "ResNet18", d)
    g = torch.Generator().manual_seed(11)
    wav = 0.1 * torch.randn(2, 24000, generator=g)          # time view: one 64-sequence cluster; band view: padded tiles
    enroll = 0.1 * torch.randn(2, 30001, generator=g)
    want = eng.separate(wav.numpy(), enroll.numpy(), E.ENROLL_WAVE)
    eng.close()
    monkeypatch.setenv("WS_ENGINE_POISON", "1")
    eng2 = E.Engine(str(tmp_path / "j.wsw"))
    for _ in range(2):                                       # second call: the consolidated arena
        got = eng2.separate(wav.numpy(), enroll.numpy(), E.ENROLL_WAVE)
        assert np.isfinite(got).all()
        assert np.array_equal(got, want)
    eng2.close()


@pytest.mark.parametrize("joint", [False, True], ids=["fixed-embeddings", "spex-plus"])
def test_convtasnet_engine_matches_python_model(tmp_path, joint):
    """Conv-TasNet / SpEx+ launch plan of the native runtime (arch 1) against the Python module tree in eval mode on
    the same device: the same kernels in the same order, so agreement to rounding.  The engine returns the first of
    the three estimates, zero-extended to the mixture length."""
    from wesep_amd.models import get_model
    d = _cuda()
    torch.manual_seed(21 + int(joint))
    kw = dict(N=256, L=20, B=128, H=256, P=3, X=4, R=2, spk_emb_dim=256, joint_training=joint)
    model = get_model("ConvTasNet")(**kw)
    with torch.no_grad():                                   # non-trivial affine parameters and running statistics
        for name, p in model.named_parameters():
            if name.endswith(("norm_1.weight", "norm_2.weight", "lnorm1.weight", "lnorm2.weight", "ln.weight",
                              "batch_norm1.weight", "batch_norm2.weight", "aux_enc3.0.weight")):
                p.uniform_(0.5, 1.5)
            elif name.endswith(("norm_1.bias", "norm_2.bias", "lnorm1.bias", "lnorm2.bias", "ln.bias", "batch_norm1.bias",
                                "batch_norm2.bias", "aux_enc3.0.bias")):
                p.normal_(0.0, 0.1)
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.2)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    path = str(tmp_path / "t.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    assert eng.info("arch") == 1
    model = model.to(d).eval()
    g = torch.Generator().manual_seed(3)
    for R, T in ((2, 16000), (3, 12345), (1, 4000), (2, 16000)):
        wav = 0.1 * torch.randn(R, T, generator=g)
        if joint:
            enroll, kind = 0.1 * torch.randn(R, 9000 + 37 * R, generator=g), E.ENROLL_WAVE
        else:
            enroll, kind = torch.randn(R, 256, generator=g), E.ENROLL_EMBEDDING
        est = eng.separate(wav.numpy(), enroll.numpy(), kind)
        with torch.no_grad():
            ref = model(wav.to(d), enroll.to(d))[0]
        n = ref.shape[-1]
        assert n <= T and rel(est[:, :n], ref) < 1e-5, (R, T, rel(est[:, :n], ref))
        assert not est[:, n:].any()
    assert eng.info("n_launches") > 0 and eng.info("arena_bytes") > 0
    eng.close()
