"""GPU: the T-split MHASTP / MQMHASTP kernels (csrc/mhastp.hip, ws_mhastp_fwd_split / _bwd_split) against the fp64
restatement and against the per-(row, head) grid, whole ECAPA-TDNN and CAM++ encoders with MHASTP / MQMHASTP / ASTP
against tests/encoder_pooling_ref.py (embedding and every parameter gradient), a jointly trained BSRNN step per new
encoder x pool (finite, bit-for-bit repeatable) and the launches the 1-D encoders make."""
import pytest
import torch

from tests import encoder_pooling_ref as ER

pytestmark = pytest.mark.gpu


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def maxrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _pool_pair(name, C, seed, **kw):
    from wesep_amd.models import resnet as MR
    ref = ER.make_pool(name, C, seed, **kw)
    ours = getattr(MR, name)(in_dim=C, **kw)
    ours.load_state_dict({k: v.float() for k, v in ref.state_dict().items()}, strict=True)
    return ours, ref


def _grad_errs(ours, ref):
    """Per-tensor relative gradient error; the last attention bias (exact gradient zero: a shift of every logit of a
    softmax over T) is measured against the largest gradient instead, as in tests/test_mhastp_gpu.py."""
    refp = dict(ref.named_parameters())
    gmax = max(float(p.grad.norm()) for p in refp.values())
    last = "att_1.bias" if any(k.endswith("att_1.weight") for k in refp) else "att_0.bias"
    return {k: float(p.grad.norm()) / gmax if k.endswith(last) else rel(p.grad, refp[k].grad)
            for k, p in ours.named_parameters()}


LAYER_CASES = [(name, kw, R, T) for name, kw in (("MHASTP", {}), ("MHASTP", dict(d_s=2)), ("MQMHASTP", {}))
               for R in (1, 3) for T in (1, 37, 398)]


@pytest.mark.parametrize("name,kw,R,T", LAYER_CASES)
def test_split_kernels_match_fp64(name, kw, R, T):
    d = _cuda()
    C = 512
    ours, ref = _pool_pair(name, C, seed=R + T, **kw)
    ours = ours.to(d)
    g = torch.Generator().manual_seed(100 + R + T)
    x = torch.relu(torch.randn(R, C, T, generator=g, dtype=torch.float64)) + 0.1 * torch.randn(R, C, T, generator=g,
                                                                                              dtype=torch.float64)
    xd = x.permute(0, 2, 1).reshape(R * T, C).float().to(d).requires_grad_(True)        # [R*T, C] channels-last
    out = ours.run(xd, R, 1, T, split=True)
    probe = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * probe.float().to(d)).sum().backward()
    xr = x.clone().requires_grad_(True)
    outr = ref(xr)
    (outr * probe).sum().backward()
    err = maxrel(out, outr)
    errs = {"dx": rel(xd.grad.view(R, T, C).permute(0, 2, 1), xr.grad)}
    if T == 1:      # a softmax over one frame is 1 whatever the logit: every attention gradient is exactly zero
        errs.update({k: float(p.grad.norm()) / float(xr.grad.norm()) for k, p in ours.named_parameters()})
    else:
        errs.update(_grad_errs(ours, ref))
    worst = max(errs, key=errs.get)
    # the same data on the per-(row, head) grid
    ours2 = ours
    x2 = xd.detach().clone().requires_grad_(True)
    out2 = ours2.run(x2, R, 1, T, split=False)
    print(f"{name} {kw} R={R} T={T}: out {err:.1e}, worst gradient {errs[worst]:.1e} ({worst}), "
          f"split vs unsplit {maxrel(out, out2):.1e}")
    if T == 1:
        # var = E[x^2] - mean^2 of a single frame is zero up to the rounding of mean^2 (~1e-7 relative), the size of
        # the 1e-7 floor itself: the std half is sqrt(floor + rounding), so it is held to the floor's scale; the
        # per-(row, head) kernels compute the same bits (split vs unsplit below)
        dm = ours.n_query[0].d_model if name == "MQMHASTP" else ours.d_model
        a, b = (t.detach().double().cpu().view(R, -1, 2, dm) for t in (out, outr))     # [R][Q*H][mean, std][dm]
        mean_err = float((a[:, :, 0] - b[:, :, 0]).abs().max() / b.abs().max())
        std_abs = float((a[:, :, 1] - b[:, :, 1]).abs().max())
        assert mean_err < 1e-6 and std_abs < 5e-4, (mean_err, std_abs)
        # the exact attention gradients are zero; what is left is that rounding of var times dvar = dstd / (2 std)
        assert errs["dx"] < 5e-5 and errs[worst] < 2e-3, (worst, errs[worst])
    else:
        assert err < 1e-6, err
        assert errs[worst] < 5e-5, (worst, errs[worst])
    assert maxrel(out, out2) < 1e-6
    (out2 * probe.float().to(d)).sum().backward()
    assert rel(xd.grad, x2.grad) < 1e-6


def test_split_counts_do_not_change_the_result():
    """Forced split counts 1 .. T on one input: every one within 1e-6 of the unsplit forward, dx within 1e-6."""
    from wesep_amd import dev
    from wesep_amd.functional_resnet import _mhastp_pack
    d = _cuda()
    R, T, C, Q, H = 2, 53, 512, 2, 8
    ours, _ = _pool_pair("MQMHASTP", C, seed=9)
    ours = ours.to(d)
    params = [p for q in ours.n_query for p in q.att_params()]
    dm = C // H
    P1 = dev.mhastp_block_floats(2, dm, dm)
    pack = _mhastp_pack(params, Q * H, 2, dm, 1, dm, P1, d)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(R * T, C, generator=g).to(d)
    dout = torch.randn(R, Q * H * 2 * dm, generator=g).to(d)
    out0, aux0 = torch.empty(R, Q * H * 2 * dm, device=d), torch.empty(R * Q * H * 4, dm, device=d)
    dev.mhastp_fwd(x, pack, R, 1, T, C, Q, H, 2, dm, out0, aux0)
    dx0 = torch.empty_like(x)
    dev.mhastp_bwd(x, pack, aux0, dout, R, 1, T, C, Q, H, 2, dm, dx0)
    for n in (1, 2, 3, 4, 7, 53):
        out, aux = torch.empty_like(out0), torch.empty_like(aux0)
        assert dev.mhastp_fwd_split(x, pack, R, 1, T, C, Q, H, 2, dm, out, aux, tsplit=n) == n
        dx = torch.empty_like(x)
        dev.mhastp_bwd_split(x, pack, aux, dout, R, 1, T, C, Q, H, 2, dm, dx, tsplit=n)
        torch.cuda.synchronize()
        assert maxrel(out, out0) < 1e-6, n
        assert maxrel(dx, dx0) < 1e-6, n


def _trunk_errs(model_grads, ref_grads, skip):
    return {k: rel(g, ref_grads[k]) for k, g in model_grads.items() if not k.endswith(skip)}


@pytest.mark.parametrize("name,pool", [("ECAPA_TDNN_c512", "MHASTP"), ("ECAPA_TDNN_c512", "MQMHASTP"),
                                       ("ECAPA_TDNN_c512", "ASTP"), ("ECAPA_TDNN_GLOB_c1024", "MHASTP"),
                                       ("ECAPA_TDNN_GLOB_c1024", "ASTP")])
def test_ecapa_matches_restatement(name, pool):
    from wesep_amd.models.resnet import get_speaker_model
    d = _cuda()
    glob, ch = "GLOB" in name, 1024 if "c1024" in name else 512
    sd, rpool = ER.ecapa_state_dict(pool, channels=ch, glob=glob, seed=23)
    model = get_speaker_model(name)(feat_dim=80, embed_dim=192, pooling_func=pool)
    model.load_state_dict(sd, strict=True)
    model = model.to(d).train()
    g = torch.Generator().manual_seed(24)
    x, probe = torch.randn(32, 64, 80, generator=g), torch.randn(32, 192, generator=g)   # 32 rows: see test_ecapa_gpu
    emb = model(x.to(d))
    (emb * probe.to(d)).sum().backward()
    p = {k: (v.double().clone() if ER.EO.is_buffer(k) else v.double().clone().requires_grad_(True))
         for k, v in sd.items() if not k.startswith("pool.")}
    ref = ER.ecapa_forward(p, rpool, x.double())
    (ref * probe.double()).sum().backward()
    refg = {k: v.grad for k, v in p.items() if v.requires_grad}
    refg.update({"pool." + k: v.grad for k, v in rpool.named_parameters()})
    errs = _trunk_errs({k: v.grad for k, v in model.named_parameters()}, refg, ("att_1.bias", "linear2.bias"))
    vals = sorted(errs.values())
    worst = max(errs, key=errs.get)
    head = max(errs[k] for k in errs if k.startswith(("linear.", "bn.", "pool.")))
    print(f"{name} {pool}: emb {rel(emb, ref):.1e}, median {vals[len(vals) // 2]:.1e}, worst {errs[worst]:.1e} ({worst}), "
          f"head {head:.1e}")
    # the bounds of tests/test_ecapa_gpu.py (split-bf16 trunk against fp64 through 26 BatchNorms; MI355X: emb 2e-5,
    # median 5e-3 .. 8e-3, worst 1.8e-2 on conv biases, linear / bn / pool 3.6e-5 .. 4.8e-5)
    assert rel(emb, ref) < 1e-3
    assert vals[len(vals) // 2] < 1e-2 and errs[worst] < 6e-2, (worst, errs[worst])
    assert head < 5e-4


@pytest.mark.parametrize("pool", ("MHASTP", "MQMHASTP", "ASTP"))
def test_campplus_matches_restatement(monkeypatch, pool):
    from tests.test_campplus_gpu import _record_relu_masks
    from wesep_amd.models import campplus as MC
    d = _cuda()
    blocks = ((2, 3, 1), (2, 3, 2), (1, 3, 2))
    sd, rpool = ER.campplus_state_dict(pool, embed_dim=64, seed=36, blocks=blocks, feat_dim=16)
    model = ER.small_campplus(MC, blocks, pool, feat_dim=16, embed_dim=64)
    model.load_state_dict(sd, strict=True)
    model = model.to(d).train()
    g = torch.Generator().manual_seed(136)
    R = 16
    x, probe = torch.randn(R, 230, 16, generator=g), torch.randn(R, 64, generator=g)
    masks = _record_relu_masks(monkeypatch, MC, R)
    emb = model(x.to(d))
    (emb * probe.to(d)).sum().backward()
    p = {k: (v.double().clone() if ER.CO.is_buffer(k) else v.double().clone().requires_grad_(True))
         for k, v in sd.items() if not k.startswith(("pool.", "xvector.stats."))}
    ref = ER.campplus_forward(p, rpool, x.double(), blocks=blocks, relu_masks=masks)
    (ref * probe.double()).sum().backward()
    refg = {k: v.grad for k, v in p.items() if v.requires_grad}
    for k, v in rpool.named_parameters():
        refg["pool." + k] = refg["xvector.stats." + k] = v.grad
    errs = _trunk_errs({k: v.grad for k, v in model.named_parameters()}, refg, ("att_1.bias", "linear2.bias"))
    worst = max(errs, key=errs.get)
    print(f"CAM++ {pool}: emb {rel(emb, ref):.1e}, worst gradient {errs[worst]:.1e} ({worst})")
    assert rel(emb, ref) < 1e-3
    assert errs[worst] < 2e-3, (worst, errs[worst])        # tests/test_campplus_gpu.py's bound


def _bsrnn(spk_model, pool):
    from wesep_amd.models import get_model
    E = 512 if spk_model == "CAMPPlus" else 192
    return get_model("BSRNN")(num_repeat=1, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                              joint_training=True, spk_feat=True, spk_model=spk_model, spk_emb_dim=E,
                              spk_args=dict(feat_dim=80, embed_dim=E, pooling_func=pool))


JOINT = [("ECAPA_TDNN_c512", "MHASTP"), ("ECAPA_TDNN_c512", "MQMHASTP"), ("ECAPA_TDNN_c512", "TSDP"),
         ("CAMPPlus", "ASTP"), ("CAMPPlus", "MQMHASTP"), ("CAMPPlus", "TAP")]


@pytest.mark.parametrize("spk_model,pool", JOINT)
def test_joint_step_is_finite_and_repeatable(spk_model, pool):
    d = _cuda()
    torch.manual_seed(5)
    model = _bsrnn(spk_model, pool).to(d).train()
    g = torch.Generator().manual_seed(6)
    wav, fb = torch.randn(2, 16000, generator=g).to(d), torch.randn(2, 200, 80, generator=g).to(d)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    grads = []
    for _ in range(2):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        est, _ = model(wav, fb)
        est.pow(2).mean().backward()
        grads.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    pool_grads = [k for k in grads[0] if ".pool." in k or ".stats." in k]
    assert bool(pool_grads) == (pool not in ("TSTP", "TAP", "TSDP"))
    for k, v in grads[0].items():
        assert torch.isfinite(v).all(), k
        assert torch.equal(v, grads[1][k]), k
    if pool_grads:
        assert any(float(grads[0][k].norm()) > 0 for k in pool_grads)


@pytest.mark.parametrize("spk_model,pool", [("ECAPA_TDNN_c512", "MQMHASTP"), ("CAMPPlus", "MHASTP")])
def test_launches_use_the_split_grid(monkeypatch, spk_model, pool):
    """One split forward (two launches inside) and one split backward per step; the per-(row, head) grid is not used."""
    import wesep_amd.dev as dev
    d = _cuda()
    calls = []
    real = dev._call

    def spy(name, *args):
        calls.append(name)
        return real(name, *args)
    monkeypatch.setattr(dev, "_call", spy)
    from wesep_amd.models.resnet import get_speaker_model
    enc = get_speaker_model(spk_model)(feat_dim=80, embed_dim=192, pooling_func=pool).to(d).train()
    emb = enc(torch.randn(4, 150, 80, device=d))
    emb.sum().backward()
    torch.cuda.synchronize()
    mh = [c for c in calls if "mhastp" in c]
    assert mh.count("ws_mhastp_fwd_split") == 1 and mh.count("ws_mhastp_bwd_split") == 1, mh
    assert "ws_mhastp_fwd" not in mh and "ws_mhastp_bwd" not in mh
    n_pack = mh.count("ws_mhastp_pack")
    assert n_pack == (16 if pool == "MQMHASTP" else 2)                 # one per (query, head), once per weight version
    calls.clear()
    enc(torch.randn(4, 150, 80, device=d))
    assert "ws_mhastp_pack" not in calls
