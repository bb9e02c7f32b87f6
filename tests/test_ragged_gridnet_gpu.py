"""GPU: ragged batches through the TF-GridNet plan of the native runtime (runtime/gridnet_plan.cc).  The four
new kernels against numpy float64 on the truncated row (NaN behind every length) or bit for bit against the loops they
replace; the engine's ragged call against the same engine on every row alone, against the CPU oracle on the truncated row,
with exact zeros behind every length and NaN-poisoned tails; the recurrence branches a ragged inter-frame path can take;
`separate_main --batch 4` against `--batch 1`.  Measured values: profiles/ragged_gridnet.md."""
import os
import subprocess

import numpy as np
import pytest
import torch

from wesep_amd import dev
from wesep_amd import engine as E
from wesep_amd.bin.export_engine import export_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
GRID = dict(n_fft=128, stride=64, lstm_hidden_units=64, attn_n_head=4, attn_approx_qk_dim=512, emb_dim=128, emb_ks=1, emb_hs=1)
SMALL_BINS = dict(n_fft=16, stride=8, attn_approx_qk_dim=72)         # 9 bins, E = 8: what the cluster recurrence's inter path needs
SPK = dict(joint_training=True, spk_model="ResNet18", spk_feat=True,
           spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False))


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _tab(v, d):
    return torch.tensor(list(v), dtype=torch.int32, device=d)


# ---- kernels ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nchunk", [1, 7])
def test_flat_stats_len_vs_numpy_fp64_on_the_truncated_row(nchunk):
    d = _cuda()
    g = torch.Generator().manual_seed(21)
    R, Tf, QC, frames = 3, 33, 65 * 128, (33, 5, 17)
    x = torch.randn(R, Tf, QC, generator=g) * 2 + 0.5
    for r, n in enumerate(frames):
        x[r, n:] = NAN
    stats = torch.full((R, 2), NAN, device=d)
    dev.flat_stats_len(x.to(d), R, Tf * QC, _tab(frames, d), QC, stats, nchunk=nchunk)
    stats = stats.cpu().numpy()
    worst = 0.0
    for r, n in enumerate(frames):
        v = x[r, :n].double().numpy()
        worst = max(worst, abs(stats[r, 0] - v.mean()), abs(stats[r, 1] * np.sqrt(v.var() + dev.LN_EPS) - 1))
    print(f"ws_flat_stats_len nchunk {nchunk}: worst error {worst:.2e}")
    assert worst < 1e-5
    # a table entry outside [1, Tf] is clamped, not followed: 0 reads one frame, 99 the whole group
    x = torch.nan_to_num(x, nan=1.0)
    st2 = torch.full((R, 2), NAN, device=d)
    dev.flat_stats_len(x.to(d), R, Tf * QC, _tab((0, 99, -3), d), QC, st2, nchunk=nchunk)
    st2 = st2.cpu().numpy()
    for r, n in enumerate((1, Tf, 1)):
        assert abs(st2[r, 0] - x[r, :n].double().mean().item()) < 1e-5


@pytest.mark.parametrize("n,T,lengths", [(128, 2048, (2048, 1999, 777, 256)), (128, 2001, (2001, 1024, 256)),
                                         (16, 600, (600, 333, 32)), (16, 599, (599, 96))])
def test_ola_norm_len_vs_numpy_fp64(n, T, lengths):
    d = _cuda()
    g = torch.Generator().manual_seed(22)
    R, hop, Tf = len(lengths), n // 2, 1 + T // (n // 2)
    fr = torch.randn(R, Tf, n, generator=g)
    for r, ln in enumerate(lengths):
        fr[r, 1 + ln // hop:] = NAN
    win = torch.hann_window(n)                                    # periodic: 0.5 - 0.5 cos(2 pi k / n)
    est = torch.full((R, T), NAN, device=d)
    dev.ola_norm_len(fr.to(d), win.to(d), R, Tf, n, T, _tab(lengths, d), est)
    est = est.cpu().numpy()
    w2 = win.double().numpy() ** 2
    for r, ln in enumerate(lengths):
        tfr = 1 + ln // hop
        y, env = np.zeros((tfr - 1) * hop + n), np.zeros((tfr - 1) * hop + n)
        for t in range(tfr):
            y[t * hop:t * hop + n] += fr[r, t].double().numpy()
            env[t * hop:t * hop + n] += w2
        want = y[hop:hop + ln] / env[hop:hop + ln]                 # (the envelope is zero only at sample 0, which the trim drops)
        e = rel(est[r, :ln], want)
        print(f"ws_ola_norm_len n {n} T {T} row {r} ({ln} samples): rel {e:.2e}")
        assert e < 1e-5 and np.isfinite(est[r]).all()
        assert not est[r, ln:].any()                               # exact zeros from the length on


def test_batched_transpose_and_head_merge_are_the_loops_they_replace_bit_for_bit():
    d = _cuda()
    g = torch.Generator().manual_seed(23)
    nh, R, Tp, Q, cp = 4, 2, 36, 65, 32
    G, Dv = nh * R, Q * cp
    va = torch.randn(G, Tp, Dv, generator=g).to(d)
    got, want = torch.full((G, Dv, Tp), NAN, device=d), torch.full((G, Dv, Tp), NAN, device=d)
    dev.transpose_batched(va, G, Tp, Dv, got)
    for i in range(G):                                             # the rectangular plan's loop: one ws_transpose per (head, row)
        dev.transpose(va, Tp, Dv, Dv, want, src_off=i * Tp * Dv, dst_off=i * Tp * Dv)
    assert torch.equal(got, want) and torch.equal(got, va.transpose(1, 2))
    # a shape with partial tiles on both axes and more tiles than one block walks
    src = torch.randn(3, 100, 68, generator=g).to(d)
    dst = torch.full((3, 68, 100), NAN, device=d)
    dev.transpose_batched(src, 3, 100, 68, dst)
    assert torch.equal(dst, src.transpose(1, 2))
    ov = torch.randn(nh, R, Tp, Q, cp, generator=g).to(d)
    o = torch.full((R, Tp, Q, nh * cp), NAN, device=d)
    dev.heads_merge_fwd(ov, nh, R, Tp * Q, cp, o)
    want = torch.full_like(o, NAN)
    for h in range(nh):                                            # the loop of strided copies, one per (head, row)
        for r in range(R):
            want[r, :, :, h * cp:(h + 1) * cp] = ov[h, r]
    assert torch.equal(o, want)


# ---- the engine --------------------------------------------------------------------------------------------------------
def _oracle_engine(tmp_path, seed, **kw):
    from oracle import tfgridnet_oracle as TG
    from wesep_amd.models import get_model
    cfg = TG.TFGridNetConfig(**kw)
    params = TG.synth_params(cfg, seed)
    model = get_model("TFGridNet")(**kw, joint_training=False)
    model.load_state_dict(params, strict=True)
    path = str(tmp_path / f"g{seed}.wsw")
    export_engine(model, path)
    return E.Engine(path), cfg, params


def _ragged(eng, wav, lengths, emb, poison=NAN):
    """The ragged call on the rectangle, with `poison` behind every length of the caller's buffer."""
    mix = np.array(wav, dtype=np.float32, copy=True)
    for r, n in enumerate(lengths):
        mix[r, n:] = poison
    ln = np.asarray(lengths, np.int32)
    emb = np.ascontiguousarray(emb, dtype=np.float32)
    est = np.full_like(mix, NAN)
    rc = E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, mix.shape[0], mix.shape[1], ln.ctypes.data, emb.ctypes.data,
                                           E.ENROLL_EMBEDDING, 0, None, est.ctypes.data)
    assert rc == 0, E.lib().ws_engine_last_error().decode()
    return est


def _check_rows(eng, est, wav, lengths, emb, what):
    """every row against the same engine's rectangular call on that row alone; zeros behind; finite.  Returns the worst."""
    worst = 0.0
    for r, n in enumerate(lengths):
        alone = eng.separate(wav[r:r + 1, :n], emb[r:r + 1], E.ENROLL_EMBEDDING)[0]
        e = rel(est[r, :n], alone)
        worst = max(worst, e)
        assert np.abs(alone).max() > 0
        assert np.isfinite(est[r]).all() and not est[r, n:].any(), (what, r)
        assert e < 1e-4, (what, r, n, e)
    return worst


@pytest.fixture(scope="module")
def main_case(tmp_path_factory):
    """T = 2048, lengths (2048, 1999, 1024, 777, 256): a full row, frame counts that are no multiples of 4 (32, 13, 5), a length
    on a hop boundary, the minimum 2 * n_fft.  One engine, one ragged call, shared by the tests below."""
    _cuda()
    eng, cfg, params = _oracle_engine(tmp_path_factory.mktemp("rg"), 62, n_layers=2, spk_fuse_type="multiply", **GRID)
    g = torch.Generator().manual_seed(8)
    lengths, T = (2048, 1999, 1024, 777, 256), 2048
    wav, emb = (0.1 * torch.randn(5, T, generator=g)).numpy(), torch.randn(5, 256, generator=g).numpy()
    est = _ragged(eng, wav, lengths, emb)
    yield dict(eng=eng, cfg=cfg, params=params, lengths=lengths, T=T, wav=wav, emb=emb, est=est)
    eng.close()


def test_engine_ragged_rows_match_the_row_alone_with_zero_tails(main_case):
    c = main_case
    worst = _check_rows(c["eng"], c["est"], c["wav"], c["lengths"], c["emb"], "main")
    print(f"ragged TF-GridNet engine vs the row alone, lengths {c['lengths']}: worst rel {worst:.2e}")
    assert c["eng"].info("cluster_fallbacks") == 0


def test_engine_ragged_rows_match_the_oracle_on_the_truncated_row(main_case):
    from oracle import tfgridnet_oracle as TG
    c = main_case
    for r, n in enumerate(c["lengths"]):
        with torch.no_grad():
            ref = TG.tfgridnet_forward(c["params"], c["cfg"], torch.from_numpy(c["wav"][r:r + 1, :n].copy()),
                                       torch.from_numpy(c["emb"][r:r + 1]))[0]
        e = rel(c["est"][r, :n], ref)
        print(f"ragged TF-GridNet engine vs the oracle on the truncated row {r} ({n} samples): rel {e:.2e}")
        assert e < 1e-3, (r, n, e)


def test_engine_ragged_ignores_what_lies_behind_a_length(main_case):
    """NaN, Inf or zeros behind the lengths of the caller's buffer: the same valid outputs, bit for bit (nothing there is read)."""
    c = main_case
    for poison in (0.0, float("inf")):
        est = _ragged(c["eng"], c["wav"], c["lengths"], c["emb"], poison=poison)
        assert np.array_equal(est, c["est"]), poison


def test_engine_ragged_with_full_lengths_is_the_rectangular_call(main_case):
    c = main_case
    eng, T = c["eng"], c["T"]
    rect = eng.separate(c["wav"], c["emb"], E.ENROLL_EMBEDDING)
    est = _ragged(eng, c["wav"], (T,) * 5, c["emb"])
    e = rel(est, rect)
    # every length-aware reduction of a full row walks the same elements in the same order as the rectangular plan's, and
    # R = 5 keeps the inter-frame BLSTM on the same (BLK16 streaming) branch in both
    print(f"ragged TF-GridNet engine with all lengths = T vs the rectangular call: rel {e:.2e}, "
          f"bit-identical: {np.array_equal(est, rect)}")
    assert e < 1e-4 and np.isfinite(est).all()


def test_engine_ragged_takes_precomputed_gates_where_the_rectangle_takes_the_fused_recurrence(tmp_path):
    """R = 32, T = 1024: 2080 inter-frame sequences (65 tiles: not BLK16; 2080 % 64 != 0: not the cluster), the fused
    recurrence in the rectangular plan, which knows no step counts -- the ragged plan streams over ws_gemm_p2b_len's gates."""
    _cuda()
    eng, _, _ = _oracle_engine(tmp_path, 63, n_layers=1, spk_fuse_type="additive", **GRID)
    g = torch.Generator().manual_seed(9)
    R, T = 32, 1024
    lengths = [256 + (768 * r) // (R - 1) for r in range(R)]
    lengths[5], lengths[11] = 1024, 257
    wav, emb = (0.1 * torch.randn(R, T, generator=g)).numpy(), torch.randn(R, 256, generator=g).numpy()
    est = _ragged(eng, wav, lengths, emb)
    worst = _check_rows(eng, est, wav, lengths, emb, "streaming")
    print(f"ragged TF-GridNet engine, R = 32 (BLK streaming over precomputed gates) vs the row alone: worst rel {worst:.2e}")
    eng.close()


def test_engine_ragged_inter_frame_path_on_the_cluster_recurrence(tmp_path):
    """n_fft = 16, stride = 8, R = 64, T = 600: 576 inter-frame sequences of 76 steps -- a multiple of 64 on at most 144 CUs
    with 64 steps or more, the cluster recurrence, fed by ws_gemm_p2b_len."""
    _cuda()
    eng, _, _ = _oracle_engine(tmp_path, 64, n_layers=1, spk_fuse_type="multiply", **{**GRID, **SMALL_BINS})
    g = torch.Generator().manual_seed(10)
    R, T = 64, 600
    lengths = [600 - 9 * r for r in range(R)]                    # 600 ... 33
    lengths[-1] = 32                                             # the minimum, 2 * n_fft
    wav, emb = (0.1 * torch.randn(R, T, generator=g)).numpy(), torch.randn(R, 256, generator=g).numpy()
    est = _ragged(eng, wav, lengths, emb)
    fallbacks = eng.info("cluster_fallbacks")
    worst = _check_rows(eng, est, wav, lengths, emb, "cluster")
    print(f"ragged TF-GridNet engine, cluster recurrence on the inter-frame path vs the row alone: worst rel {worst:.2e}, "
          f"cluster fall-backs {fallbacks}")
    assert fallbacks == 0
    eng.close()


def _joint_model(seed):
    from wesep_amd.models import get_model
    torch.manual_seed(seed)
    model = get_model("TFGridNet")(n_layers=1, emb_dim=128, emb_ks=1, emb_hs=1, lstm_hidden_units=64, spk_emb_dim=256, **SPK)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith(("gamma", "norm.weight", "conv.1.weight")):
                p.uniform_(0.5, 1.5)
            elif name.endswith(("beta", "norm.bias", "conv.1.bias")):
                p.normal_(0.0, 0.1)
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.2)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    return model


def test_engine_ragged_joint_resnet18_with_enroll_lengths(tmp_path):
    _cuda()
    path = str(tmp_path / "j.wsw")
    export_engine(_joint_model(5), path)
    eng = E.Engine(path)
    g = torch.Generator().manual_seed(3)
    lengths, te = np.array([4000, 2345, 1000], np.int32), np.array([120, 77, 98], np.int32)
    wav = (0.1 * torch.randn(3, 4000, generator=g)).numpy()
    fb = torch.randn(3, 120, 80, generator=g).numpy()
    mix, rect = wav.copy(), fb.copy()
    for r in range(3):
        mix[r, lengths[r]:] = NAN                                 # the caller's tails: poison, on both inputs
        rect[r, te[r]:] = NAN
    est = np.full_like(mix, NAN)
    rc = E.lib().ws_engine_separate_ragged(eng._h, mix.ctypes.data, 3, 4000, lengths.ctypes.data, rect.ctypes.data, E.ENROLL_FBANK,
                                           120, te.ctypes.data, est.ctypes.data)
    assert rc == 0, E.lib().ws_engine_last_error().decode()
    for r, n in enumerate(lengths):
        alone = eng.separate(wav[r:r + 1, :n], fb[r:r + 1, :te[r]], E.ENROLL_FBANK)[0]
        e = rel(est[r, :n], alone)
        print(f"ragged TF-GridNet engine, joint ResNet18 with enroll_lengths, row {r}: rel vs the row alone {e:.2e}")
        assert np.isfinite(est[r]).all() and not est[r, n:].any() and np.abs(alone).max() > 0
        assert e < 1e-4, (r, e)
    eng.close()


def test_separate_main_batch_4_against_batch_1_tfgridnet(tmp_path):
    from tests.test_ragged_speaker_gpu import _write_wav
    _cuda()
    exe = os.path.join(ROOT, "runtime", "separate_main")
    path = str(tmp_path / "j.wsw")
    export_engine(_joint_model(8), path)
    rng = np.random.default_rng(4)
    lens = (8000, 5000, 6400, 3333)
    lines = []
    for i, n in enumerate(lens):
        _write_wav(tmp_path / f"mix{i}.wav", rng.integers(-3000, 3000, n))
        _write_wav(tmp_path / f"a{i}.wav", rng.integers(-3000, 3000, 20000 + 1111 * i))
        _write_wav(tmp_path / f"b{i}.wav", rng.integers(-3000, 3000, 30000 - 999 * i))
        lines.append(f"u{i} {tmp_path}/mix{i}.wav {tmp_path}/a{i}.wav {tmp_path}/b{i}.wav\n")
    scp = tmp_path / "wav.scp"
    scp.write_text("".join(lines))
    outs = {}
    for tag, extra in (("b1", ["--batch", "1"]), ("b4", ["--batch", "4"])):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        outs[tag] = out
    assert sorted(os.listdir(outs["b1"])) == sorted(os.listdir(outs["b4"]))                # the same files, by name
    for i, n in enumerate(lens):
        for k in (1, 2):
            a = np.fromfile(outs["b1"] / f"u{i}-spk{k}.f32", dtype=np.float32)
            b = np.fromfile(outs["b4"] / f"u{i}-spk{k}.f32", dtype=np.float32)
            e = rel(b, a)
            print(f"separate_main --batch 4 vs --batch 1 (TF-GridNet), u{i} spk{k} ({n} samples): rel {e:.2e}")
            assert a.shape == b.shape == (n,) and e < 1e-4, (i, k, e)
