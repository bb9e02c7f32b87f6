"""GPU: long recordings in the native runtime (runtime/longform.cc, wesep_amd/csrc/longform.hip).  The two
kernels against the numpy-float64 restatement of tests/longform_ref.py and as a partition of unity; ws_engine_separate_long
of every architecture against the float64 cross-fade of the same engine's whole-utterance call on every window alone;
"enroll once" (ws_engine_embed + WS_ENROLL_SPEAKER) bit for bit against the call with the raw enrollment; and
`separate_main --chunk_seconds` against Engine.separate_long.  Measured values: profiles/longform.md."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import longform_ref as R
from wesep_amd import dev
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
SHAPES = [(512, 128, 2000), (512, 0, 1537), (516, 258, 5000), (512, 100, 513), (512, 128, 512), (2000, 500, 5003)]   # (S, O, n)
SPK = dict(joint_training=True, spk_model="ResNet18", spk_feat=True,
           spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False))
# (model, arguments, n, window, overlap): the smallest models the plans take, fixed embeddings
ENGINE_CASES = {
    "pBSRNN": ("BSRNN", dict(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False), 6000, 2048, 512),
    "ConvTasNet": ("ConvTasNet", dict(N=32, L=20, B=32, H=64, P=3, X=2, R=1), 5003, 2000, 500),
    "DPCCN": ("DPCCN", dict(tcn_blocks=1, tcn_layers=1), 9000, 4096, 1024),
    "TFGridNet": ("TFGridNet", dict(n_layers=1, emb_dim=128, emb_ks=1, emb_hs=1, lstm_hidden_units=64, spk_emb_dim=256), 5000, 2048,
                  512),
}


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def _model(name, seed, **kw):
    """A model with non-trivial normalisation parameters, running statistics and FiLM layers (they start at 1 / 0 / zero)."""
    from wesep_amd.models import get_model
    torch.manual_seed(seed)
    model = get_model(name)(**kw)
    with torch.no_grad():
        for pname, p in model.named_parameters():
            leaf = pname.rsplit(".", 2)[-2] if pname.count(".") else ""
            if "gamma_fcs" in pname or "beta_fcs" in pname:
                p.normal_(0.0, 0.05)
            elif "norm" in leaf.lower() or leaf in ("ln", "bn"):
                p.uniform_(0.5, 1.5) if pname.endswith(("weight", "gamma")) else p.normal_(0.0, 0.1)
        for bname, buf in model.named_buffers():
            if bname.endswith("running_mean"):
                buf.normal_(0.0, 0.2)
            elif bname.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    return model


# ---- kernels ---------------------------------------------------------------------------------------------------------
def _gather_dev(x, S, O, reps, d, scale=None):
    n = len(x)
    st, Lw, H = R.starts(n, S, O), min(n, S), S - O
    rows = torch.full((reps, len(st), Lw), NAN, device=d)
    dev.window_rows(torch.from_numpy(x).to(d), n, len(st), S, H, reps, rows, scale=scale)
    torch.cuda.synchronize()
    return rows


@pytest.mark.parametrize("S,O,n", SHAPES)
def test_kernels_vs_numpy_fp64(S, O, n):
    d = _cuda()
    K = 2
    g = torch.Generator().manual_seed(S + O + n)
    x = torch.randn(n, generator=g).numpy()
    st, Lw = R.starts(n, S, O), min(n, S)
    W = len(st)
    rows = _gather_dev(x, S, O, K, d).cpu().numpy()
    want = R.gather(x, S, O)
    assert np.array_equal(rows, np.stack([want.astype(np.float32)] * K))            # a copy: every window once per speaker
    y = torch.randn(K, W, Lw, generator=g)
    out = torch.full((K, n), NAN, device=d)
    dev.xfade_ola(y.to(d), K, W, S, O, n, out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    ref = R.xfade(y.numpy(), n, S, O)
    e = rel(out, ref)
    worst = float(np.abs(out - ref).max() / np.abs(ref).max())
    print(f"ws_xfade_ola S {S} O {O} n {n} (W {W}): rel {e:.2e}, worst element / max {worst:.2e}")
    assert np.isfinite(out).all()                                                    # every out[k][i] is written
    assert e < 1e-5, (S, O, n, e)
    # the per-window factors of the TF-GridNet plan: exact fp32 products on the way in, the same reference on the way out
    sc = (0.5 + torch.rand(W, generator=g)).to(d)
    rows_s = _gather_dev(x, S, O, K, d, scale=sc).cpu().numpy()
    assert np.array_equal(rows_s, rows * sc.cpu().numpy()[None, :, None])
    out_s = torch.full((K, n), NAN, device=d)
    dev.xfade_ola(y.to(d), K, W, S, O, n, out_s, scale=sc)
    torch.cuda.synchronize()
    e = rel(out_s.cpu().numpy(), R.xfade(y.numpy().astype(np.float64) * sc.cpu().numpy().astype(np.float64)[None, :, None], n, S, O))
    print(f"ws_xfade_ola with per-window factors: rel {e:.2e}")
    assert e < 1e-5, (S, O, n, e)


@pytest.mark.parametrize("S,O,n", SHAPES)
def test_partition_of_unity_on_the_device(S, O, n):
    """xfade_ola(window_rows(x)) = x.  out = fl(fl(fl(g1 x) + fl(g2 x)) / fl(g1 + g2)) with the SAME rounded g in both
    sums: four roundings of 2^-24 each, 2.4e-7 relative (x has one sign in both terms: no cancellation); 1e-6 leaves 4 x."""
    d = _cuda()
    g = torch.Generator().manual_seed(7 * S + O + n)
    x = torch.randn(n, generator=g).numpy()
    K, W = 2, len(R.starts(n, S, O))
    rows = _gather_dev(x, S, O, K, d)
    out = torch.full((K, n), NAN, device=d)
    dev.xfade_ola(rows, K, W, S, O, n, out)
    torch.cuda.synchronize()
    out = out.cpu().numpy()
    err = np.abs(out.astype(np.float64) - x[None].astype(np.float64)) / np.abs(x[None].astype(np.float64))
    print(f"partition of unity S {S} O {O} n {n}: worst |out - x| / |x| {err.max():.2e}")
    assert np.isfinite(out).all() and (err <= 1e-6).all(), (S, O, n, err.max())


# ---- the engine, one case per architecture ----------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(ENGINE_CASES))
def engine_case(request, tmp_path_factory):
    """One engine, one recording, one ws_engine_separate_long call and its float64 reference from the whole-utterance call
    on every window alone: shared by the tests below."""
    _cuda()
    arch = request.param
    name, kw, n, S, O = ENGINE_CASES[arch]
    path = str(tmp_path_factory.mktemp("lf") / f"{arch}.wsw")
    export_engine(_model(name, 11, joint_training=False, **kw), path)
    eng = E.Engine(path)
    g = torch.Generator().manual_seed(5)
    K = 2
    mix, emb = (0.1 * torch.randn(n, generator=g)).numpy(), torch.randn(K, 256, generator=g).numpy()
    max_rows = 3 if arch == "pBSRNN" else 8
    est = eng.separate_long(mix, emb, E.ENROLL_EMBEDDING, S, O, max_rows)
    info = (eng.info("long_windows"), eng.info("long_forwards"))
    st = R.starts(n, S, O)
    y = np.stack([np.stack([eng.separate(mix[None, s:s + S], emb[k:k + 1], E.ENROLL_EMBEDDING)[0] for s in st]) for k in range(K)])
    yield dict(arch=arch, eng=eng, mix=mix, emb=emb, est=est, ref=R.xfade(y, n, S, O), n=n, S=S, O=O, K=K, max_rows=max_rows,
               info=info, W=len(st))
    eng.close()


def test_engine_separate_long_vs_fp64_crossfade_of_the_windows_alone(engine_case):
    c = engine_case
    assert c["info"] == (c["W"], -(-c["K"] * c["W"] // c["max_rows"]))
    assert c["est"].shape == (c["K"], c["n"]) and np.isfinite(c["est"]).all()
    for k in range(c["K"]):
        e = rel(c["est"][k], c["ref"][k])
        print(f"ws_engine_separate_long {c['arch']} n {c['n']} S {c['S']} O {c['O']} (W {c['W']}, max_rows {c['max_rows']}), "
              f"speaker {k}: rel {e:.2e}")
        assert np.abs(c["ref"][k]).max() > 0
        assert e < 1e-4, (c["arch"], k, e)


def test_engine_separate_long_group_size_does_not_matter(engine_case):
    c = engine_case
    one = c["eng"].separate_long(c["mix"], c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], 1)
    assert c["eng"].info("long_forwards") == c["K"] * c["W"]
    eight = c["eng"].separate_long(c["mix"], c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], 8)
    assert c["eng"].info("long_forwards") == -(-c["K"] * c["W"] // 8)
    for k in range(c["K"]):
        e = rel(one[k], eight[k])
        print(f"ws_engine_separate_long {c['arch']}: max_rows 1 vs 8, speaker {k}: rel {e:.2e}")
        assert e < 1e-4, (c["arch"], k, e)


def test_engine_separate_long_of_one_window_is_the_whole_utterance_call(engine_case):
    c = engine_case
    for n in (c["S"], c["S"] - 40):
        mix = c["mix"][:n]
        a = c["eng"].separate_long(mix, c["emb"], E.ENROLL_EMBEDDING, c["S"], c["O"], 8)
        b = c["eng"].separate(np.stack([mix] * c["K"]), c["emb"], E.ENROLL_EMBEDDING)
        assert np.abs(b).max() > 0 and np.array_equal(a, b), (c["arch"], n)


# ---- enroll once ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def joint_engine(tmp_path_factory):
    _cuda()
    path = str(tmp_path_factory.mktemp("lfj") / "j.wsw")
    export_engine(_model("BSRNN", 13, num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False, **SPK), path)
    eng = E.Engine(path)
    yield eng, path
    eng.close()


@pytest.mark.parametrize("kind,rows", [(E.ENROLL_FBANK, 2), (E.ENROLL_FBANK, 3), (E.ENROLL_WAVE, 2), (E.ENROLL_WAVE, 3)],
                         ids=["fbank-2", "fbank-3", "wave-2", "wave-3"])
def test_enroll_once_is_bit_for_bit_the_call_with_the_raw_enrollment(joint_engine, kind, rows):
    eng, _ = joint_engine
    g = torch.Generator().manual_seed(17 + rows)
    T = 4000
    wav = (0.1 * torch.randn(rows, T, generator=g)).numpy()
    if kind == E.ENROLL_FBANK:
        enroll, elen = torch.randn(rows, 120, 80, generator=g).numpy(), np.array([120, 77, 98][:rows], np.int32)
    else:
        enroll, elen = (0.1 * torch.randn(rows, 20000, generator=g)).numpy(), np.array([20000, 12345, 16000][:rows], np.int32)
    for r in range(rows):
        enroll[r, elen[r]:] = NAN                                     # what the caller left behind a length reaches nothing
    pitch = enroll.shape[1]
    direct = np.full_like(wav, NAN)
    rc = E.lib().ws_engine_separate_ragged(eng._h, wav.ctypes.data, rows, T, None, enroll.ctypes.data, kind, pitch, elen.ctypes.data,
                                           direct.ctypes.data)
    assert rc == 0, E.lib().ws_engine_last_error().decode()
    emb = eng.embed(enroll, kind, lengths=elen)
    assert emb.shape == (rows, 256) and np.isfinite(emb).all() and np.abs(emb).max() > 0
    again = eng.separate(wav, emb, E.ENROLL_SPEAKER)
    assert np.isfinite(direct).all() and np.abs(direct).max() > 0
    assert np.array_equal(again, direct)
    # the same through the windowed call: K = rows target speakers of one recording
    mix = wav.reshape(-1)[:6000]
    est = np.full((rows, 6000), NAN, np.float32)
    rc = E.lib().ws_engine_separate_long(eng._h, mix.ctypes.data, 6000, rows, enroll.ctypes.data, kind, pitch, elen.ctypes.data, 2048,
                                         512, 3, est.ctypes.data)
    assert rc == 0, E.lib().ws_engine_last_error().decode()
    n_raw = eng.info("n_launches")
    est_spk = eng.separate_long(mix, emb, E.ENROLL_SPEAKER, 2048, 512, 3)
    assert eng.info("n_launches") < n_raw                             # no speaker stage
    assert np.isfinite(est).all() and np.abs(est).max() > 0 and np.array_equal(est, est_spk)


# ---- separate_main --chunk_seconds ---------------------------------------------------------------------------------------
def test_separate_main_chunked_against_engine_separate_long(joint_engine, tmp_path):
    from tests.test_ragged_speaker_gpu import _write_wav
    eng, path = joint_engine
    exe = os.path.join(ROOT, "runtime", "separate_main")
    rng = np.random.default_rng(4)
    lens = (5000, 8000, 2048)
    data, lines = [], []
    for i, n in enumerate(lens):
        m, a, b = rng.integers(-3000, 3000, n), rng.integers(-3000, 3000, 20000 + 1111 * i), rng.integers(-3000, 3000, 30000 - 999 * i)
        for tag, x in (("mix", m), ("a", a), ("b", b)):
            _write_wav(tmp_path / f"{tag}{i}.wav", x)
        data.append((m, a, b))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    outs = {}
    for tag, extra in (("whole", []), ("chunked", ["--chunk_seconds", "0.128", "--overlap_seconds", "0.032", "--chunk_rows", "3"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        outs[tag] = out
    assert sorted(os.listdir(outs["whole"])) == sorted(os.listdir(outs["chunked"]))       # the same files, by name
    for i, (m, a, b) in enumerate(data):
        ne = min(len(a), len(b))
        enr = np.stack([a[:ne], b[:ne]]).astype(np.float32) / 32768.0
        want = eng.separate_long(m.astype(np.float32) / 32768.0, enr, E.ENROLL_WAVE, 2048, 512, 3)
        for k in (1, 2):
            got = np.fromfile(outs["chunked"] / f"u{i}-spk{k}.f32", dtype=np.float32)
            e = rel(got, want[k - 1])
            print(f"separate_main --chunk_seconds 0.128 vs Engine.separate_long, u{i} spk{k} ({len(m)} samples): rel {e:.2e}")
            assert got.shape == (len(m),) and np.abs(want).max() > 0 and e < 1e-4, (i, k, e)


def test_extract_engine_windowed_normalises_the_assembled_estimate(joint_engine):
    from wesep_amd.bin.infer import extract_engine
    eng, _ = joint_engine
    g = torch.Generator().manual_seed(23)
    wav, fb = (0.1 * torch.randn(2, 6000, generator=g)).numpy(), torch.randn(2, 100, 80, generator=g).numpy()
    lengths = [6000, 4500]
    got = extract_engine(eng, wav, fb, lengths=lengths, window=2048)               # overlap defaults to window // 4
    for r, n in enumerate(lengths):
        raw = eng.separate_long(wav[r, :n], fb[r:r + 1], E.ENROLL_FBANK, 2048, 512)[0]
        assert np.abs(raw).max() > 0 and not got[r, n:].any()
        assert np.allclose(got[r, :n], raw / np.abs(raw).max() * 0.9, rtol=1e-6, atol=0)   # one peak per recording, not per window
