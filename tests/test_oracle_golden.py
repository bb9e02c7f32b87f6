"""CPU: pin `oracle/bsrnn_oracle.py` against fixtures produced by the REAL reference
(`oracle/make_golden.py`).  Tolerances: the oracle and the reference execute the
same torch CPU kernels in (almost) the same order, so agreement is ~1e-6."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import bsrnn_oracle as O
from oracle.make_golden import CASES


def _run_oracle(name):
    kw, R, T, seed = CASES[name]
    cfg = O.BSRNNConfig(**kw)
    params = {k: v.requires_grad_(True) for k, v in O.synth_params(cfg, seed).items()}
    wav, tgt, emb = O.synth_batch(R, T, seed)
    est = O.bsrnn_forward(params, cfg, wav, emb)
    loss = O.sisdr_loss(est, tgt)
    loss.backward()
    return cfg, params, wav, tgt, emb, est, loss


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_matches_reference_fixture(name, golden_dir):
    path = os.path.join(golden_dir, name + ".npz")
    assert os.path.exists(path), "fixture missing: run python -m oracle.make_golden"
    g = np.load(path)
    cfg, params, wav, tgt, emb, est, loss = _run_oracle(name)
    # inputs and weights regenerate bit-identically
    assert np.array_equal(g["wav"], wav.numpy())
    assert np.array_equal(g["emb"], emb.numpy())
    chk = sum(float(v.detach().double().abs().sum()) for v in params.values())
    assert abs(chk - float(g["param_checksum"])) <= 1e-9 * abs(chk)
    # forward
    ref = g["est"]
    rel = np.linalg.norm(est.detach().numpy() - ref) / np.linalg.norm(ref)
    assert rel < 1e-5, rel
    assert abs(loss.item() - float(g["loss"])) < 1e-4          # dB
    # backward: every parameter gradient
    assert list(g["names"]) == list(params.keys())
    for k, p in params.items():
        gn = float(g["gnorm/" + k])
        mine = p.grad.reshape(-1)
        assert abs(float(mine.double().norm()) - gn) <= 2e-4 * gn + 1e-9, k
        head = g["ghead/" + k]
        assert np.allclose(mine[:16].numpy(), head, rtol=2e-3, atol=2e-4 * gn / np.sqrt(mine.numel()) + 1e-10), k
        if "gfull/" + k in g.files:
            full = g["gfull/" + k]
            err = np.linalg.norm(mine.numpy() - full) / (np.linalg.norm(full) + 1e-30)
            assert err < 2e-4, (k, err)


def test_fixture_set_complete(golden_dir):
    have = {os.path.basename(p)[:-4] for p in glob.glob(os.path.join(golden_dir, "*.npz"))}
    assert set(CASES) <= have


def test_sisdr_matches_numpy_metric():
    """auraloss restatement vs the reference's own numpy SI-SNR (score.py:7-21)."""
    g = torch.Generator().manual_seed(3)
    t = torch.randn(3, 16000, generator=g)
    for snr_db in (-5.0, 0.0, 10.0, 30.0):
        n = torch.randn(3, 16000, generator=g) * (10 ** (-snr_db / 20))
        x = 0.7 * t + n
        a = -O.sisdr_loss(x, t).item()
        b = np.mean([O.cal_sisnr_np(t[i].numpy(), x[i].numpy()) for i in range(3)])
        assert abs(a - b) < 1e-3


def test_adam_restatement_matches_torch():
    torch.manual_seed(0)
    p = torch.randn(300)
    ref = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=1e-3, weight_decay=1e-4)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in range(1, 4):
        g = torch.randn(300)
        ref.grad = g.clone()
        opt.step()
        O.adam_l2_step_(p, g, m, v, step, 1e-3, weight_decay=1e-4)
    assert torch.allclose(p, ref.detach(), rtol=1e-6, atol=1e-7)


def test_lr_schedule_endpoints():
    assert abs(O.exponential_decrease_lr(0, 1000, 1e-3, 2.5e-5) - 1e-3) < 1e-12
    assert abs(O.exponential_decrease_lr(1000, 1000, 1e-3, 2.5e-5) - 2.5e-5) < 1e-12


# ---- Conv-TasNet / SpEx+ ----------------------------------------------
from oracle import convtasnet_oracle as CT  # noqa: E402
from oracle.make_golden import TASNET_CASES  # noqa: E402


def run_tasnet_oracle(name):
    kw, R, T, seed = TASNET_CASES[name]
    from oracle.make_golden import ENROLL_LEN
    cfg = CT.ConvTasNetConfig(**kw)
    params = {k: (v if CT.is_buffer(k) else v.requires_grad_(True)) for k, v in CT.synth_params(cfg, seed).items()}
    wav, tgt, emb = O.synth_batch(R, T, seed)
    bufs = {}
    if cfg.joint_training:
        emb, label = CT.synth_enrollment(R, ENROLL_LEN, cfg.spksInTrain, seed)
    ests = CT.convtasnet_forward(params, cfg, wav, emb, training=True, new_buffers=bufs)
    loss = CT.spexplus_loss(ests, tgt, label) if cfg.multi_task else CT.multiscale_sisdr_loss(ests, tgt)
    loss.backward()
    params["__new_buffers__"] = bufs
    return cfg, params, wav, tgt, emb, ests, loss


@pytest.mark.parametrize("name", sorted(TASNET_CASES))
def test_tasnet_oracle_matches_reference_fixture(name, golden_dir):
    path = os.path.join(golden_dir, name + ".npz")
    assert os.path.exists(path), "fixture missing: run python -m oracle.make_golden"
    g = np.load(path)
    cfg, params, wav, tgt, emb, ests, loss = run_tasnet_oracle(name)
    bufs = params.pop("__new_buffers__")
    assert np.array_equal(g["wav"], wav.numpy())
    assert np.array_equal(g["emb"], emb.numpy())
    chk = sum(float(v.detach().double().abs().sum()) for v in params.values())
    assert abs(chk - float(g["param_checksum"])) <= 1e-9 * abs(chk)
    if cfg.multi_task:
        assert np.allclose(ests[3].detach().numpy(), g["logits"], rtol=1e-4, atol=1e-5)
    for k, v in bufs.items():       # BatchNorm running statistics after the step
        assert np.allclose(v.numpy(), g["buf/" + k], rtol=1e-5, atol=1e-6), k
    assert not cfg.joint_training or len(bufs) == 12
    params = {k: v for k, v in params.items() if not CT.is_buffer(k)}
    for i, est in enumerate(ests[:3]):
        ref = g[f"est{i + 1}"]
        rel = np.linalg.norm(est.detach().numpy() - ref) / np.linalg.norm(ref)
        assert rel < 1e-5, (i, rel)
    assert abs(loss.item() - float(g["loss"])) < 1e-4          # dB
    assert list(g["names"]) == list(params.keys())
    # the loss is invariant to a DC offset of the estimate, so d/d(decoder bias) is pure rounding noise:
    # gradients are compared with an absolute floor of 1e-6 of the largest gradient norm
    floor = 2e-6 * max(float(g["gnorm/" + k]) for k in params)
    for k, p in params.items():
        gn = float(g["gnorm/" + k])
        mine = p.grad.reshape(-1)
        assert abs(float(mine.double().norm()) - gn) <= 2e-4 * gn + floor, k
        if "gfull/" + k in g.files:
            full = g["gfull/" + k]
            err = np.linalg.norm(mine.numpy() - full)
            assert err < 2e-4 * np.linalg.norm(full) + floor, (k, err)


# ---- DPCCN: oracle pinned ahead of the HIP path ------------------------------------
from oracle import dpccn_oracle as DP  # noqa: E402
from oracle.make_golden import DPCCN_CASES  # noqa: E402


@pytest.mark.parametrize("name", sorted(DPCCN_CASES))
def test_dpccn_oracle_matches_reference_fixture(name, golden_dir):
    path = os.path.join(golden_dir, name + ".npz")
    assert os.path.exists(path), "fixture missing: run python -m oracle.make_golden"
    g = np.load(path)
    kw, R, T, seed = DPCCN_CASES[name]
    cfg = DP.DPCCNConfig(**kw)
    params = {k: v.requires_grad_(True) for k, v in DP.synth_params(cfg, seed).items()}
    wav, tgt, emb = O.synth_batch(R, T, seed)
    assert np.array_equal(g["wav"], wav.numpy()) and np.array_equal(g["emb"], emb.numpy())
    chk = sum(float(v.detach().double().abs().sum()) for v in params.values())
    assert abs(chk - float(g["param_checksum"])) <= 1e-9 * abs(chk)
    est = DP.dpccn_forward(params, cfg, wav, emb)
    loss = O.sisdr_loss(est, tgt)
    loss.backward()
    ref = g["est"]
    assert np.linalg.norm(est.detach().numpy() - ref) / np.linalg.norm(ref) < 1e-4
    assert abs(loss.item() - float(g["loss"])) < 1e-3          # dB
    assert list(g["names"]) == list(params.keys())
    floor = 1e-5 * max(float(g["gnorm/" + k]) for k in params)
    for k, p in params.items():
        gn = float(g["gnorm/" + k])
        assert abs(float(p.grad.double().norm()) - gn) <= 2e-3 * gn + floor, k


# ---- TF-GridNet: oracle pinned ahead of the HIP path -------------------------------
from oracle import tfgridnet_oracle as TG  # noqa: E402
from oracle.make_golden import TFGRIDNET_CASES, tfgridnet_batch  # noqa: E402


@pytest.mark.parametrize("name", sorted(TFGRIDNET_CASES))
def test_tfgridnet_oracle_matches_reference_fixture(name, golden_dir):
    path = os.path.join(golden_dir, name + ".npz")
    assert os.path.exists(path), "fixture missing: run python -m oracle.make_golden"
    g = np.load(path)
    kw, R, T, seed = TFGRIDNET_CASES[name]
    cfg = TG.TFGridNetConfig(**kw)
    params = {k: v.requires_grad_(True) for k, v in TG.synth_params(cfg, seed).items()}
    wav, tgt, emb = tfgridnet_batch(cfg, R, T, seed)
    assert np.array_equal(g["wav"], wav.numpy()) and np.array_equal(g["emb"], emb.numpy())
    chk = sum(float(v.detach().double().abs().sum()) for v in params.values())
    assert abs(chk - float(g["param_checksum"])) <= 1e-9 * abs(chk)
    est = TG.tfgridnet_forward(params, cfg, wav, emb)
    loss = O.sisdr_loss(est, tgt)
    loss.backward()
    ref = g["est"]
    assert np.linalg.norm(est.detach().numpy() - ref) / np.linalg.norm(ref) < 1e-4
    assert abs(loss.item() - float(g["loss"])) < 1e-3          # dB
    assert list(g["names"]) == list(params.keys())
    floor = 1e-5 * max(float(g["gnorm/" + k]) for k in params)
    for k, p in params.items():
        gn = float(g["gnorm/" + k])
        assert abs(float(p.grad.double().norm()) - gn) <= 2e-3 * gn + floor, k


def test_bsrnn_multi_oracle_matches_reference_fixture(golden_dir):
    """`BSRNN_Multi` (bsrnn_multi_optim.py:300-470): the oracle's two-pass composition against the fixture produced by
    the real reference module (third-party ResNet / MelSpectrogram stood in for by the restatements, see
    make_golden.MULTI_CASES)."""
    from oracle.make_golden import MULTI_CASES, MULTI_LOSS_WEIGHT, multi_embed_fn, synth_multi_params
    for name, (kw, spk_model, R, T, Tw, seed) in MULTI_CASES.items():
        g = np.load(os.path.join(golden_dir, name + ".npz"))
        cfg = O.BSRNNConfig(**kw)
        params = synth_multi_params(cfg, spk_model, seed)
        chk = sum(float(v.double().abs().sum()) for v in params.values())
        assert abs(chk - float(g["param_checksum"])) <= 1e-9 * abs(chk)
        p = {k: (v.clone().requires_grad_(True) if v.is_floating_point() and "running_" not in k else v.clone())
             for k, v in params.items()}
        wav, tgt, _ = O.synth_batch(R, T, seed)
        assert np.array_equal(g["wav"], wav.numpy())
        enroll = torch.from_numpy(g["enroll"])
        embed, second_in = multi_embed_fn(p, spk_model), []

        def embed_fn(w):
            # the second pass embeds the first pass's estimate, a -50 dB signal whose fbank and BatchNorm over 2 rows
            # amplify rounding ~30x (4.5e-7 in s -> 1.4e-5 in self_s; a host with other CPU kernels reached 1.8e-4 in
            # self_s).  So it embeds the reference's own estimate, the input the reference's second pass saw, once `w`
            # is shown to be this pass's estimate (below); each pass is then held to 1e-4 on the reference's inputs
            if w is enroll:
                return embed(w)
            second_in.append(w)
            return embed(torch.from_numpy(g["est"]))

        s, self_s, e1, e2 = O.bsrnn_multi_forward(p, cfg, wav, enroll, embed_fn)
        assert len(second_in) == 1 and torch.equal(second_in[0], s.detach())
        for got, key in ((s, "est"), (self_s, "self_est"), (e1, "emb1"), (e2, "emb2")):
            ref = g[key]
            assert np.linalg.norm(got.detach().numpy() - ref) / np.linalg.norm(ref) < 1e-4, key
        loss = MULTI_LOSS_WEIGHT[0] * O.sisdr_loss(s, tgt) + MULTI_LOSS_WEIGHT[1] * O.sisdr_loss(self_s, tgt)
        # self_s is scored at -50 dB SI-SDR: a 1e-5 difference in it is 3e-3 dB in its loss (conditioning, not a defect)
        assert abs(loss.item() - float(g["loss"])) < 1e-2
        loss.backward()
        for k in g["names"]:
            gn = float(g["gnorm/" + str(k)])
            assert abs(float(p[str(k)].grad.norm()) - gn) <= 1e-2 * gn + 1e-7, k
