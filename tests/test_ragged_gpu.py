"""GPU: ragged batches -- a length per row through the pBSRNN forward, so that every row of a batch comes out as that row
does alone.  References are never the code under test: torch.stft / torch.istft / fp64 nn.LSTM for the kernels, the CPU
oracle on the TRUNCATED row (one row at a time) and the committed reference fixtures for the model, the Python model for
the engine.  Tolerances are the ones the project already uses for the same comparisons: WAV_TOL = 1e-3 against oracle /
fixture (tests/test_bsrnn_gpu.py), 1e-4 engine against the Python model and block against its fp64 reference
(tests/test_engine_gpu.py, test_resrnn_block_vs_oracle), 1e-3 for h of a recurrence against torch's fp64 LSTM
(tests/test_cluster2_gpu.py), 2e-6 / 5e-6 for the STFT / iSTFT kernels against torch (tests/test_kernels_gpu.py)."""
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
WAV_TOL = 1e-3
H, N, K = 256, 128, 32
NAN = float("nan")


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _bands(d):
    from wesep_amd import dev
    bw = O.band_widths(16000, 512)
    return bw, dev.BandTables(bw, d)


def _tables(lengths, T, d):
    from wesep_amd import dev
    return dev.ragged_tables(lengths, T, d)


def _bandsplit_ref(wav):
    """torch.stft of ONE row -> [Tf, 514] in the band-split layout."""
    spec = torch.stft(wav[None], 512, 128, window=torch.hann_window(512), return_complex=True)[0]      # [257, Tf]
    ref = torch.empty(spec.shape[1], 514)
    f0 = 0
    for b in O.band_widths(16000, 512):
        ref[:, 2 * f0:2 * f0 + b] = spec.real[f0:f0 + b].t()
        ref[:, 2 * f0 + b:2 * f0 + 2 * b] = spec.imag[f0:f0 + b].t()
        f0 += b
    return ref


# ---- kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths,T", [((4000, 3000, 777, 257), 4000), ((16000, 12345, 4096, 9999), 16000),
                                       ((3968, 3969, 4095), 4100)])
def test_ragged_stft_bandsplit_vs_torch_per_row(lengths, T):
    from wesep_amd import dev
    d = _cuda()
    g = torch.Generator().manual_seed(T)
    R = len(lengths)
    wav = 0.1 * torch.randn(R, T, generator=g)
    for r, n in enumerate(lengths):
        wav[r, n:] = NAN                                        # nothing behind a row's end may be read
    bw, bt = _bands(d)
    Tf = 1 + T // 128
    ln, tf = _tables(lengths, T, d)
    xbs = torch.full((R * Tf, 514), NAN, device=d)
    dev.stft_bandsplit(wav.to(d), bt, xbs, lengths=ln)
    xbs = xbs.view(R, Tf, 514).cpu()
    alone = torch.full((Tf, 514), NAN, device=d)
    for r, n in enumerate(lengths):
        ref = _bandsplit_ref(wav[r, :n])
        tfr = 1 + n // 128
        assert ref.shape[0] == tfr
        e = rel(xbs[r, :tfr], ref)
        print(f"ragged stft row {r} (len {n} of {T}): rel vs torch.stft {e:.2e}")
        assert e < 2e-6, (r, e)
        assert not xbs[r, tfr:].any(), r                        # the frames behind the row's end are zeros (finite)
        # and bit for bit what the rectangular entry point gives that row alone
        dev.stft_bandsplit(wav[r:r + 1, :n].contiguous().to(d), bt, alone[:tfr])
        assert torch.equal(xbs[r, :tfr], alone[:tfr].cpu()), r


def test_rectangular_stft_and_ola_are_untouched_by_a_full_length_table():
    """lengths[r] = T for every row: the length-aware entry points give the bits of the rectangular ones."""
    from wesep_amd import dev
    d = _cuda()
    g = torch.Generator().manual_seed(9)
    R, T = 3, 4000
    Tf = 1 + T // 128
    wav = (0.1 * torch.randn(R, T, generator=g)).to(d)
    bw, bt = _bands(d)
    ln, tf = _tables([T] * R, T, d)
    a, b = torch.empty(R * Tf, 514, device=d), torch.empty(R * Tf, 514, device=d)
    dev.stft_bandsplit(wav, bt, a)
    dev.stft_bandsplit(wav, bt, b, lengths=ln)
    assert torch.equal(a, b)
    frames = torch.randn(R * Tf, 512, generator=g).to(d)
    ea, eb = torch.empty(R, T, device=d), torch.empty(R, T, device=d)
    dev.istft_ola(frames, R, Tf, T, ea)
    dev.istft_ola(frames, R, Tf, T, eb, lengths=ln)
    assert torch.equal(ea, eb)
    x = torch.randn(R, K, Tf, N, generator=g).to(d)
    geo = dev.Geom(R * K, 1, Tf * N, 0, N, Tf, N, K)
    sa, sb = torch.empty(R * K, 2, device=d), torch.empty(R * K, 2, device=d)
    dev.group_stats(x, geo, sa)
    dev.group_stats(x, geo, sb, glen=tf, glen_div=K)
    assert torch.equal(sa, sb)


def test_length_aware_group_stats_vs_numpy():
    """The three GroupNorm sites over time: BN[i] (per-band widths on the band-split spectrogram), ResRNN.norm in the time
    view and mask[i]'s norm (a (row, band) group over Tf x 128)."""
    from wesep_amd import dev
    d = _cuda()
    g = torch.Generator().manual_seed(17)
    lengths, T = (4000, 3000, 777, 2049), 4000
    R, Tf = len(lengths), 1 + T // 128
    ln, tf = _tables(lengths, T, d)
    eps = float(np.finfo(np.float32).eps)
    bw, bt = _bands(d)
    # BN: xbs [R, Tf, 514], group (r, band) = Tf_r frames x 2 bw columns
    xbs = torch.randn(R, Tf, 514, generator=g) * 2 + 0.5
    for r, n in enumerate(lengths):
        xbs[r, 1 + n // 128:] = NAN
    geo = dev.Geom(R * K, K, Tf * 514, 0, 514, Tf, 128, K, bt.bw2, bt.off2)
    stats = torch.full((R * K, 2), NAN, device=d)
    dev.group_stats(xbs.to(d), geo, stats, glen=tf, glen_div=K)
    stats = stats.cpu().numpy().reshape(R, K, 2)
    x64 = xbs.double().numpy()
    f0 = 0
    worst = 0.0
    for k, b in enumerate(bw):
        for r, n in enumerate(lengths):
            v = x64[r, :1 + n // 128, 2 * f0:2 * f0 + 2 * b]
            want = (v.mean(), 1.0 / np.sqrt(v.var() + eps))
            worst = max(worst, abs(stats[r, k, 0] - want[0]), abs(stats[r, k, 1] / want[1] - 1))
        f0 += b
    print(f"length-aware BN statistics: worst error {worst:.2e}")
    assert worst < 1e-5
    # ResRNN.norm (time view) / mask norm: z [R, K, Tf, 128]
    z = torch.randn(R, K, Tf, N, generator=g) * 1.5 - 0.3
    for r, n in enumerate(lengths):
        z[r, :, 1 + n // 128:] = NAN
    for geo in (dev.Geom(R * K, 1, Tf * N, 0, N, Tf, N), dev.Geom(R * K, 1, Tf * N, 0, N, Tf, N, K)):
        stats = torch.full((R * K, 2), NAN, device=d)
        dev.group_stats(z.to(d), geo, stats, glen=tf, glen_div=K)
        stats = stats.cpu().numpy().reshape(R, K, 2)
        z64 = z.double().numpy()
        worst = 0.0
        for r, n in enumerate(lengths):
            v = z64[r, :, :1 + n // 128].reshape(K, -1)
            worst = max(worst, np.abs(stats[r, :, 0] - v.mean(1)).max(), np.abs(stats[r, :, 1] * np.sqrt(v.var(1) + eps) - 1).max())
        print(f"length-aware (row, band) statistics: worst error {worst:.2e}")
        assert worst < 1e-5


def _resrnn_case(R, Tf, seed):
    from wesep_amd.models.bsrnn import ResRNN
    torch.manual_seed(seed)
    blk = ResRNN(N, 2 * N)
    with torch.no_grad():
        blk.norm.weight.add_(0.1 * torch.randn(N))
        blk.norm.bias.add_(0.1 * torch.randn(N))
    return blk, torch.randn(R, K, Tf, N)


def _resrnn_ref64(blk, z_row):
    """fp64 torch on ONE truncated row: z_row [K, L, N] -> (h [K, L, 2H], out [K, L, N])."""
    sd = {k: v.detach().double() for k, v in blk.state_dict().items()}
    lstm = torch.nn.LSTM(N, H, batch_first=True, bidirectional=True).double()
    lstm.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("rnn.")})
    x = z_row.double()
    xn = torch.nn.functional.group_norm(x.transpose(1, 2), 1, sd["norm.weight"], sd["norm.bias"],
                                        float(torch.finfo(torch.float32).eps)).transpose(1, 2)
    with torch.no_grad():
        h, _ = lstm(xn)
    return h, x + h @ sd["proj.weight"].t() + sd["proj.bias"]


@pytest.mark.parametrize("R,Tf,frames,branch", [
    (2, 126, (126, 97), "cluster"),            # 64 sequences, long: the weight-stationary cluster kernel on precomputed gates
    (4, 70, (70, 64, 9, 33), "cluster"),
    (3, 126, (100, 126, 5), "stream"),         # nseq % 64 != 0: the streaming kernel, 16-sequence workgroups
    (2, 40, (40, 17), "stream"),               # short sequences
    (66, 12, None, "stream")],                 # > 2048 sequences: 32-sequence workgroups (rectangular calls fuse here)
    ids=["cluster_r2", "cluster_r4", "stream_r3", "stream_short", "stream_blk32"])
def test_ragged_time_view_blstm_vs_torch_fp64_per_truncated_sequence(R, Tf, frames, branch):
    """Every forward branch that accepts lengths: the hidden states of every valid step against torch's fp64 nn.LSTM run on
    the truncated sequence (the reverse direction must start at the sequence's own last step with zero state), and the
    block's output against the fp64 block; whatever the tail of the input holds."""
    from wesep_amd import dev
    from wesep_amd import functional as F_
    d = _cuda()
    if frames is None:
        frames = tuple(1 + (5 * r) % Tf for r in range(R))
    blk, z = _resrnn_case(R, Tf, 3 + R)
    for r, n in enumerate(frames):
        z[r, :, n:] = 1e4 * torch.randn(K, Tf - n, N)          # finite garbage behind the row's end (the contract for activations)
    blk = blk.to(d)
    tf = torch.tensor(frames, dtype=torch.int32, device=d)
    with torch.no_grad():
        out, stats, plan, W, saved = F_._resrnn_blk_fwd(z.to(d), "time", blk.norm.weight, blk.norm.bias,
                                                        tuple(p.detach() for p in blk._wparams()), None, False, frames=tf)
    assert plan.fwd == branch, plan
    seq = F_._view_maps("time", R, K, Tf, N)[2]
    h = dev.from_blocked(saved[2].view(-1, 2 * H // 4, 32, 4), seq, R * K * Tf, split=True).view(R, K, Tf, 2 * H).cpu()
    assert torch.isfinite(out).all() and torch.isfinite(h).all()
    blk = blk.cpu()
    worst_h = worst_o = 0.0
    for r, n in enumerate(frames):
        h_ref, o_ref = _resrnn_ref64(blk, z[r, :, :n])
        worst_h, worst_o = max(worst_h, rel(h[r, :, :n], h_ref)), max(worst_o, rel(out[r, :, :n], o_ref))
        assert not h[r, :, n:, H:].any(), r                    # the reverse direction crosses the tail with zero state
    print(f"ragged time view {branch} R={R} Tf={Tf}: worst h rel vs torch fp64 {worst_h:.2e}, block out {worst_o:.2e}")
    assert worst_h < 1e-3 and worst_o < 1e-4, (worst_h, worst_o)


@pytest.mark.parametrize("lengths,T", [((4000, 3000, 777, 2049), 4000), ((16000, 12345, 4096, 9999), 16000)])
def test_ragged_istft_vs_torch_per_row(lengths, T):
    from wesep_amd import dev
    d = _cuda()
    g = torch.Generator().manual_seed(T + 1)
    R, Tf = len(lengths), 1 + T // 128
    bw, bt = _bands(d)
    wav = 0.1 * torch.randn(R, T, generator=g)
    m3 = torch.randn(R, Tf, 1028, generator=g)
    ln, tf = _tables(lengths, T, d)
    xbs = torch.empty(R * Tf, 514, device=d)
    dev.stft_bandsplit(wav.to(d), bt, xbs, lengths=ln)
    frames = torch.empty(R * Tf, 512, device=d)
    dev.mask_istft_frames(xbs, m3.view(R * Tf, 1028).to(d), R, Tf, bt, frames)
    frames = frames.view(R, Tf, 512)
    for r, n in enumerate(lengths):
        frames[r, 1 + n // 128:] = NAN                         # the frames behind a row's end must not be read
    est = torch.full((R, T), NAN, device=d)
    dev.istft_ola(frames.view(R * Tf, 512), R, Tf, T, est, lengths=ln)
    est = est.cpu()
    for r, n in enumerate(lengths):
        tfr = 1 + n // 128
        spec = torch.stft(wav[r:r + 1, :n], 512, 128, window=torch.hann_window(512), return_complex=True)     # [1, 257, tfr]
        bands, f0 = [], 0
        for b in bw:
            o = m3[r, :tfr, 4 * f0:4 * f0 + 4 * b].reshape(tfr, 2, 2, b).permute(1, 2, 3, 0)              # 2, 2, b, tfr
            m = o[0] * torch.sigmoid(o[1])
            xb = spec[0, f0:f0 + b]
            bands.append(torch.complex(xb.real * m[0] - xb.imag * m[1], xb.real * m[1] + xb.imag * m[0]))
            f0 += b
        ref = torch.istft(torch.cat(bands, 0)[None], 512, 128, window=torch.hann_window(512), length=n)[0]
        e = rel(est[r, :n], ref)
        print(f"ragged istft row {r} (len {n} of {T}): rel vs torch.istft {e:.2e}")
        assert e < 5e-6, (r, e)
        assert not est[r, n:].any(), r


# ---- model ------------------------------------------------------------------------------------------------------------
def _build(cfg_kw, seed, d):
    from wesep_amd.models import get_model
    cfg = O.BSRNNConfig(**cfg_kw)
    params = O.synth_params(cfg, seed)
    model = get_model("BSRNN")(
        spk_emb_dim=cfg.spk_emb_dim, sr=cfg.sr, win=cfg.win, stride=cfg.stride, feature_dim=cfg.feature_dim,
        num_repeat=cfg.num_repeat, use_spk_transform=cfg.use_spk_transform, spk_fuse_type=cfg.spk_fuse_type,
        multi_fuse=cfg.multi_fuse, joint_training=False)
    model.load_state_dict(params, strict=True)
    return cfg, params, model.to(d).eval()


def _oracle_rows(params, cfg, wav, emb, lengths):
    """The CPU oracle, one row at a time on the truncated row."""
    with torch.no_grad():
        return [O.bsrnn_forward(params, cfg, wav[r:r + 1, :n].contiguous(), emb[r:r + 1])[0] for r, n in enumerate(lengths)]


@pytest.mark.parametrize("kw,seed", [(dict(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False), 11),
                                     (dict(num_repeat=2, spk_fuse_type="FiLM", multi_fuse=True), 12)],
                         ids=["multiply", "FiLM_multi"])
def test_ragged_model_every_row_vs_oracle_on_the_truncated_row(kw, seed):
    d = _cuda()
    cfg, params, model = _build(kw, seed, d)
    T = 16000
    wav, _, emb = O.synth_batch(4, T, seed + 7)
    for lengths in ((16000, 12345, 4096, 9999), (16000, 16000, 16000, 16000)):
        w = wav.clone()
        for r, n in enumerate(lengths):
            w[r, n:] = 0.0
        with torch.no_grad():
            est = model(w.to(d), emb.to(d), lengths=list(lengths))[0].cpu()
        refs = _oracle_rows(params, cfg, w, emb, lengths)
        for r, n in enumerate(lengths):
            e = rel(est[r, :n], refs[r])
            print(f"ragged model {kw['spk_fuse_type']} lengths {lengths} row {r}: rel vs oracle on the truncated row {e:.2e}")
            assert e < WAV_TOL, (lengths, r, e)
            assert not est[r, n:].any()
        if len(set(lengths)) == 1:
            # all rows full: against the rectangular call of the same model (it runs the cluster2 branch of the time view,
            # the ragged call the cluster branch over precomputed gates: the engine / Python-model bound)
            with torch.no_grad():
                rect = model(w.to(d), emb.to(d))[0].cpu()
            e = rel(est, rect)
            print(f"ragged model {kw['spk_fuse_type']} all lengths = T vs lengths=None: rel {e:.2e}, identical {torch.equal(est, rect)}")
            assert e < 1e-4, e


@pytest.mark.parametrize("name", ["bsrnn_multiply_r2_t4000", "bsrnn_film_multi_r2_t3000"])
def test_fixture_rows_inside_a_wider_ragged_batch_reproduce_the_reference(name, golden_dir):
    """The real reference's output (tests/golden) for rows that sit in a wider batch beside longer rows."""
    from oracle.make_golden import CASES
    d = _cuda()
    kw, R, T, seed = CASES[name]
    cfg, params, model = _build(kw, seed, d)
    wav, _, emb = O.synth_batch(R, T, seed)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    Tw = 2 * T + 77
    other_w, _, other_e = O.synth_batch(2, Tw, seed + 100)
    big = torch.zeros(R + 2, Tw)
    rows = (1, 3) if R == 2 else tuple(range(1, R + 1))
    lengths = [Tw - 500] * (R + 2)
    lengths[0] = Tw
    big[0], big[2] = other_w[0], other_w[1]
    big[2, Tw - 500:] = 0
    e_all = torch.zeros(R + 2, emb.shape[1])
    e_all[0], e_all[2] = other_e[0], other_e[1]
    for i, r in enumerate(rows):
        big[r, :T] = wav[i]
        lengths[r] = T
        e_all[r] = emb[i]
    with torch.no_grad():
        est = model(big.to(d), e_all.to(d), lengths=lengths)[0].cpu()
    got = torch.stack([est[r, :T] for r in rows])
    e = rel(got, torch.from_numpy(g["est"]))
    print(f"{name} inside a [{R + 2}, {Tw}] ragged batch: rel vs the reference fixture {e:.2e}")
    assert e < WAV_TOL, e
    assert not est[rows[0], T:].any() and torch.isfinite(est).all()


def test_poisoned_tails_do_not_reach_valid_outputs():
    """mix[r][len_r:] = NaN: same valid outputs (bit-identical when no cluster recurrence fell back between the two runs -- a
    fall-back recomputes a layer on other arithmetic -- else < 1e-4), all finite, zeros behind len_r."""
    from wesep_amd import dev
    d = _cuda()
    cfg, params, model = _build(dict(num_repeat=2, spk_fuse_type="FiLM", multi_fuse=True), 12, d)
    T, lengths = 16000, [16000, 12345, 4096, 9999]
    wav, _, emb = O.synth_batch(4, T, 31)
    clean = wav.clone()
    poison = wav.clone()
    for r, n in enumerate(lengths):
        clean[r, n:] = 0.0
        poison[r, n:] = NAN
    poison[2, 5000] = float("inf")
    sc = dev._cluster_scratch(d)
    with torch.no_grad():
        a = model(clean.to(d), emb.to(d), lengths=lengths)[0]
        torch.cuda.synchronize()
        st0 = sc.status.clone()
        b = model(poison.to(d), emb.to(d), lengths=lengths)[0]
        torch.cuda.synchronize()
    moved = not torch.equal(st0, sc.status) or bool(st0.any())
    a, b = a.cpu(), b.cpu()
    assert torch.isfinite(b).all()
    for r, n in enumerate(lengths):
        assert not b[r, n:].any()
    e = rel(b, a)
    print(f"poisoned tails: rel {e:.2e}, identical {torch.equal(a, b)}, cluster status moved {moved}")
    if moved:
        assert e < 1e-4, e
    else:
        assert torch.equal(a, b)


# ---- engine -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,seed", [
    (dict(num_repeat=2, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False), 11),
    (dict(num_repeat=1, spk_fuse_type="FiLM", multi_fuse=True, use_spk_transform=True), 12)], ids=["multiply", "FiLM_xform"])
def test_engine_separate_ragged_matches_python_model_and_oracle(tmp_path, kw, seed):
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
    # R even (64 / 128 sequences: cluster), R odd (96 sequences, nseq % 64 != 0: the streaming branch), one row
    for lengths in ((16000, 12345, 4096, 9999), (12345, 8000, 12000), (5000,), (9999, 9999)):
        R, T = len(lengths), max(lengths)
        wav, _, emb = O.synth_batch(2 * ((R + 1) // 2), T, seed + T + R)
        wav, emb = wav[:R].contiguous(), emb[:R].contiguous()
        mixes = [wav[r, :n].numpy() for r, n in enumerate(lengths)]
        est = eng.separate_ragged(mixes, list(emb.numpy()), E.ENROLL_EMBEDDING)
        f0 = eng.info("cluster_fallbacks")
        poisoned = wav.clone()
        for r, n in enumerate(lengths):
            poisoned[r, n:] = NAN
        with torch.no_grad():
            py = model(poisoned.to(d), emb.to(d), lengths=list(lengths))[0].cpu()       # the ragged Python model
        for r, n in enumerate(lengths):
            with torch.no_grad():
                alone = model(wav[r:r + 1, :n].contiguous().to(d), emb[r:r + 1].to(d))[0][0].cpu()   # the row as a batch of one
            e_py, e_alone = rel(est[r], py[r, :n]), rel(est[r], alone)
            print(f"engine ragged {kw['spk_fuse_type']} lengths {lengths} row {r}: vs ragged Python model {e_py:.2e}, "
                  f"vs the Python model on the row alone {e_alone:.2e}")
            assert est[r].shape == (n,) and e_py < 1e-4 and e_alone < 1e-4, (lengths, r, e_py, e_alone)
            if n <= 12345:
                assert rel(est[r], O.bsrnn_forward(params, cfg, wav[r:r + 1, :n].contiguous(), emb[r:r + 1])[0]) < WAV_TOL
        # the rectangle's raw output: zeros behind every row, finite everywhere, whatever the tails held
        rect, ln = E.pack_rows(mixes)
        rect[np.arange(rect.shape[1])[None, :] >= ln[:, None]] = np.nan
        raw = np.zeros_like(rect)
        e2 = np.ascontiguousarray(emb.numpy())
        assert E.lib().ws_engine_separate_ragged(eng._h, rect.ctypes.data, R, T, ln.ctypes.data, e2.ctypes.data,
                                                 E.ENROLL_EMBEDDING, 0, None, raw.ctypes.data) == 0
        assert np.isfinite(raw).all()
        same = eng.info("cluster_fallbacks") == f0
        for r, n in enumerate(lengths):
            assert not raw[r, n:].any()
            assert np.array_equal(raw[r, :n], est[r]) if same else rel(raw[r, :n], est[r]) < 1e-4
    eng.close()


def test_engine_separate_ragged_joint_model_with_enroll_lengths(tmp_path):
    """fbank and waveform enrollments of different lengths: one speaker-encoder pass per row, then one separator pass."""
    from wesep_amd.models import get_model
    from wesep_amd.utils.funcs import apply_cmvn, compute_fbank
    d = _cuda()
    torch.manual_seed(5)
    model = get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                               joint_training=True, spk_model="ResNet18", spk_feat=True,
                               spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False))
    with torch.no_grad():
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0.0, 0.2)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    path = str(tmp_path / "j.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    model = model.to(d).eval()
    g = torch.Generator().manual_seed(3)
    lengths = (20000, 12345, 7000)
    wav = 0.1 * torch.randn(3, 20000, generator=g)
    mixes = [wav[r, :n].numpy() for r, n in enumerate(lengths)]
    fbs = []
    for te in (120, 77, 98):
        fb = torch.randn(te, 80, generator=g)
        fbs.append(fb - fb.mean(0, keepdim=True))
    est = eng.separate_ragged(mixes, [f.numpy() for f in fbs], E.ENROLL_FBANK)
    for r, n in enumerate(lengths):
        with torch.no_grad():
            ref = model(wav[r:r + 1, :n].contiguous().to(d), fbs[r][None].to(d))[0][0]
        e = rel(est[r], ref)
        print(f"engine ragged joint fbank row {r}: rel vs the Python model on the row alone {e:.2e}")
        assert e < 1e-4, (r, e)
    enr = [0.1 * torch.randn(n, generator=g) for n in (30001, 24000, 16123)]
    est = eng.separate_ragged(mixes, [x.numpy() for x in enr], E.ENROLL_WAVE)
    for r, n in enumerate(lengths):
        with torch.no_grad():
            fb = apply_cmvn(compute_fbank(enr[r][None].to(d), dither=0.0))
            ref = model(wav[r:r + 1, :n].contiguous().to(d), fb)[0][0]
        e = rel(est[r], ref)
        print(f"engine ragged joint wave row {r}: rel vs the Python model on the row alone {e:.2e}")
        assert e < 1e-4, (r, e)
    eng.close()


def _write_wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


def test_separate_main_batch_4_against_batch_1(tmp_path):
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
    for batch in (1, 4):
        out = tmp_path / f"out{batch}"
        out.mkdir()
        r = subprocess.run([exe, "--wav_scp", str(scp), "--model", path, "--output_dir", str(out), "--raw_out", "--batch",
                            str(batch)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr + r.stdout
        outs[batch] = out
    assert sorted(os.listdir(outs[1])) == sorted(os.listdir(outs[4]))            # the same files, by name
    for i, n in enumerate(lens):
        for k in (1, 2):
            a = np.fromfile(outs[1] / f"u{i}-spk{k}.f32", dtype=np.float32)
            b = np.fromfile(outs[4] / f"u{i}-spk{k}.f32", dtype=np.float32)
            e = rel(b, a)
            print(f"separate_main --batch 4 vs --batch 1, u{i} spk{k} ({n} samples): rel {e:.2e}")
            assert a.shape == b.shape == (n,) and e < 1e-4, (i, k, e)
            with wave.open(str(outs[4] / f"u{i}-spk{k}.wav")) as w:
                assert w.getnframes() == n and w.getframerate() == 16000
