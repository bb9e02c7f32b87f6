"""The speaker-fusion affine folded into the time-view ResRNN (functional.film_fold, dev.Film): every folded kernel against
"affine_fwd, then the same kernel without the descriptor", and one training step of the model with the fold on and off.

The folded consumers form z' = z * (a0 + a[r]) + b[r] with the fused multiply-add affine_fwd executes (csrc/common.h ws_film),
so everything that only READS z' is held to bit identity.  The two new sums, da = sum d(z') z and db = sum d(z') over the K * Tf
positions of a row, are held to the accumulation form of the normalisation contracts (tests/norm_contract.py,
profiles/norm_contract.md): an n-term fp32 sum in any order, |error| <= eps_for(False, n) * sum |terms|, n = K * Tf, against
an fp64 sum of the same fp32 d(z') and z.

Measured on one MI355X (error / bound, worst element; printed by the tests below):
  kernel level   R = 2, K = 32, Tf = 9:  FiLM da 0.0022, db 0.0015; multiply da 0.0018; additive db 0.0018
                 R = 3, K = 4, Tf = 5:   FiLM da 0.0653, db 0.0359; multiply da 0.0406; additive db 0.0463
  model level    the eight FiLM Linear weight / bias gradients: 0.0277 of their bound at the worst element;
                 peak allocated memory above the arm's start 881.13 MB folded, 898.31 MB unfolded: 17.18 MB less, the two z'
                 of this fixture being 16.52 MB."""
import gc

import pytest
import torch

from tests.gemm_contract import eps_for

pytestmark = pytest.mark.gpu

N = 128
SHAPES = [(2, 32, 9), (3, 4, 5)]          # two full tiles, odd row count | nseq = 12 < 32: rows share a block, padded slots
MODES = ["FiLM", "multiply", "additive"]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_CASES = {}


def _case(dims, mode):
    """Operands of one (shape, fuse type), made once and left unchanged: z, the affine's rows, z' from affine_fwd, and the
    statistics of z' from the plain kernel."""
    key = (dims, mode)
    if key in _CASES:
        return _CASES[key]
    from wesep_amd import dev
    from wesep_amd.functional import _view_maps
    d = _cuda()
    R, K, Tf = dims
    g = torch.Generator().manual_seed(1000 * R + 10 * Tf + MODES.index(mode))
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(d)
    z = rnd(R, K, Tf, N) + 0.3
    a = rnd(R, N, scale=0.5) if mode != "additive" else None
    b = rnd(R, N, scale=0.5) if mode != "multiply" else None
    a0 = 0.0 if mode == "multiply" else 1.0
    geo, smap, seq, _ = _view_maps("time", R, K, Tf, N)
    P = R * K * Tf
    zp = torch.empty_like(z)
    dev.affine_fwd(z, a, b, a0, P, K * Tf, N, zp)
    stats = torch.empty(geo.ngroups, 2, device=d)
    dev.group_stats(zp, geo, stats)
    c = dict(d=d, R=R, K=K, Tf=Tf, P=P, z=z, a=a, b=b, a0=a0, zp=zp, geo=geo, smap=smap, seq=seq, stats=stats,
             film=dev.Film(a, b, a0, K * Tf), off=dev.Film(None, None, 1.0, K * Tf),
             gamma=rnd(N) + 1.0, beta=rnd(N, scale=0.1), dxn=rnd(P, N), dout=rnd(R, K, Tf, N), rnd=rnd)
    _CASES[key] = c
    return c


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", SHAPES)
def test_affine_fwd_is_one_fma(dims, mode):
    """affine_fwd itself goes through ws_film: z * (a0 + a) + b with a single rounding of the product-sum."""
    c = _case(dims, mode)
    R, K, Tf = dims
    a = (c["a"] if c["a"] is not None else torch.zeros(R, N, device=c["d"])).view(R, 1, 1, N)
    b = (c["b"] if c["b"] is not None else torch.zeros(R, N, device=c["d"])).view(R, 1, 1, N)
    scale = (c["a0"] + a).float()                                   # fp32 sum, as the kernel forms it
    ref = (c["z"].double() * scale.double() + b.double()).float()   # exact product-sum (53 bits hold 24 x 24 + add), rounded once
    assert torch.equal(c["zp"], ref)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", SHAPES)
def test_group_stats_folded(dims, mode):
    from wesep_amd import dev
    c = _case(dims, mode)
    st = torch.full_like(c["stats"], float("nan"))
    dev.group_stats(c["z"], c["geo"], st, film=c["film"])
    assert torch.equal(st, c["stats"])
    st0, st1 = torch.empty_like(st), torch.empty_like(st)           # a null descriptor is the plain call
    dev.group_stats(c["z"], c["geo"], st0)
    dev.group_stats(c["z"], c["geo"], st1, film=c["off"])
    assert torch.equal(st0, st1)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", SHAPES)
def test_relay_and_x_projection_folded(dims, mode):
    """gemm_p2b: A_bl / A_bl16 of the relay and the pre-activations of the x-projection; padded slots stay exact zeros."""
    from wesep_amd import dev
    c = _case(dims, mode)
    d, seq = c["d"], c["seq"]
    nb = dev.bl_num_blocks(seq)
    norm = dict(stats=c["stats"], gamma=c["gamma"], beta=c["beta"], stat_map=c["smap"])
    Nout = 64
    wp = torch.empty(Nout * N, device=d)
    dev.pack_w(c["rnd"](Nout, N, scale=0.05), Nout, N, N, wp, order=0)

    def run(A, **kw):
        Ab = torch.full((nb, 32 * N), float("nan"), device=d)
        Ab16 = torch.full((dev.blh_floats(nb, N),), float("nan"), device=d)
        dev.gemm_p2b(A=A, lda=N, sm=seq, Wpack=None, N=0, C_out=None, A_bl=Ab, A_bl16=Ab16, **norm, **kw)
        Cx = torch.full((nb, 32 * Nout), float("nan"), device=d)
        dev.gemm_p2b(A=A, lda=N, sm=seq, Wpack=wp, N=Nout, C_out=Cx, **norm, **kw)
        return Ab, Ab16, Cx

    ref, got = run(c["zp"].view(-1, N)), run(c["z"].view(-1, N), film=c["film"])
    for r_, g_ in zip(ref, got):
        assert not torch.isnan(g_).any()
        assert torch.equal(r_.view(torch.int32), g_.view(torch.int32))
    _, valid = dev.bl_positions(seq, d)
    pad = ~valid.view(nb, 1, 32, 1).expand(nb, N // 4, 32, 4)
    assert (dims == (3, 4, 5)) == bool(pad.any())
    assert (got[0].view(nb, N // 4, 32, 4)[pad] == 0).all() and (got[2].view(nb, Nout // 4, 32, 4)[pad[:, :Nout // 4]] == 0).all()
    for r_, g_ in zip(run(c["z"].view(-1, N)), run(c["z"].view(-1, N), film=c["off"])):
        assert torch.equal(r_.view(torch.int32), g_.view(torch.int32))


@pytest.mark.parametrize("a_fmt", [0, 4])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", SHAPES)
def test_projection_residual_folded(dims, mode, a_fmt):
    """gemm_b2p: out = h Wp^T + bias + film(z) against the same call over the materialised z'."""
    from wesep_amd import dev
    c = _case(dims, mode)
    d, seq, P = c["d"], c["seq"], c["P"]
    Kd = 512
    nb = dev.bl_num_blocks(seq)
    W, bias = c["rnd"](N, Kd, scale=0.05), c["rnd"](N)
    wp = torch.empty(N * Kd, device=d)
    dev.pack_w(W, N, Kd, Kd, wp, order=1, f16=a_fmt == 4)
    if a_fmt == 4:      # two fp16 planes (hi, lo) of nb blocks each, as float32 storage
        A = torch.cat([c["rnd"](nb * 32 * Kd, scale=0.3).half(), c["rnd"](nb * 32 * Kd, scale=1e-4).half()]).view(torch.float32)
    else:
        A = dev.to_blocked(c["rnd"](P, Kd, scale=0.3), seq, split=True)

    def run(Rr, **kw):
        out = torch.full((P, N), float("nan"), device=d)
        dev.gemm_b2p(A=A, K=Kd, sm=seq, Wpack=wp, C_out=out, ldc=N, bias=bias, R=Rr, a_fmt=a_fmt, **kw)
        return out

    ref, got = run(c["zp"].view(P, N)), run(c["z"].view(P, N), film=c["film"])
    assert not torch.isnan(got).any() and torch.equal(ref, got)
    assert torch.equal(run(c["z"].view(P, N)), run(c["z"].view(P, N), film=c["off"]))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("dims", SHAPES)
def test_groupnorm_backward_folded(dims, mode):
    """gn_bwd_reduce and gn_bwd_apply_pg with the fold against affine_fwd -> reduce -> apply_pg -> affine_bwd."""
    from wesep_amd import dev
    from wesep_amd.functional import _affine_splits
    c = _case(dims, mode)
    d, geo, R, K, Tf, P = c["d"], c["geo"], c["R"], c["K"], c["Tf"], c["P"]
    z, zp, a, b, a0 = c["z"], c["zp"], c["a"], c["b"], c["a0"]
    ng = geo.ngroups
    words = lambda n: torch.zeros(n, device=d, dtype=torch.int32)
    new = lambda *s: torch.full(s, float("nan"), device=d)

    ab_ref, ab = new(ng, 2), new(ng, 2)
    dev.gn_bwd_reduce(zp, c["dxn"], c["stats"], geo, ab_ref, gamma=c["gamma"])
    dev.gn_bwd_reduce(z, c["dxn"], c["stats"], geo, ab, gamma=c["gamma"], film=c["film"])
    assert torch.equal(ab, ab_ref)
    ab0 = new(ng, 2)
    dev.gn_bwd_reduce(z, c["dxn"], c["stats"], geo, ab0, gamma=c["gamma"])
    dev.gn_bwd_reduce(z, c["dxn"], c["stats"], geo, ab, gamma=c["gamma"], film=c["off"])
    assert torch.equal(ab, ab0)

    # unfolded: d(z') from apply_pg over z', then the affine's own backward
    tg = dev.tree_groups(ng)
    dzp, dgb_ref = new(R, K, Tf, N), new(2, N)
    dev.gn_bwd_apply_pg(zp, c["dxn"], c["stats"], ab_ref, geo, dzp, c["gamma"], new(ng + tg, 2, N), dgb_ref, words(1 + tg),
                        res=c["dout"])
    ns = _affine_splits(K * Tf)
    dz_ref = new(R, K, Tf, N)
    da_ref, db_ref = (new(R, N) if a is not None else None), (new(R, N) if b is not None else None)
    dev.affine_bwd(dzp, z, a, a0, P, K * Tf, N, ns, dz_ref, new(ns, R, N) if a is not None else None,
                   new(ns, R, N) if b is not None else None, da=da_ref, db=db_ref, counter=words(R))
    # folded
    dz, dgb = new(R, K, Tf, N), new(2, N)
    da, db = (new(R, N) if a is not None else None), (new(R, N) if b is not None else None)
    fcounter = words(R)
    dev.gn_bwd_apply_pg(z, c["dxn"], c["stats"], ab_ref, geo, dz, c["gamma"], new(ng + tg, 2, N), dgb, words(1 + tg),
                        res=c["dout"], film=c["film"], fslab=new(ng, 2, N), da=da, db=db, fcounter=fcounter)
    assert torch.equal(dgb, dgb_ref)
    assert torch.equal(dz, dz_ref)
    assert int(fcounter.abs().sum()) == 0                         # the per-row counters are left at zero
    e = eps_for(False, K * Tf)
    for name, got, terms in (("da", da, dzp.double() * z.double()), ("db", db, dzp.double())):
        if got is None:
            continue
        ref, S = terms.sum(dim=(1, 2)), terms.abs().sum(dim=(1, 2))
        ratio = float(((got.double() - ref).abs() / (e * S)).max())
        print(f"film fold {dims} {mode}: {name} worst error / bound = {ratio:.4f}")
        assert ratio <= 1.0, (name, ratio)
    # null descriptor: the plain kernel's outputs
    dz0, dgb0, dz1, dgb1 = new(R, K, Tf, N), new(2, N), new(R, K, Tf, N), new(2, N)
    dev.gn_bwd_apply_pg(z, c["dxn"], c["stats"], ab0, geo, dz0, c["gamma"], new(ng + tg, 2, N), dgb0, words(1 + tg), res=c["dout"])
    dev.gn_bwd_apply_pg(z, c["dxn"], c["stats"], ab0, geo, dz1, c["gamma"], new(ng + tg, 2, N), dgb1, words(1 + tg), res=c["dout"],
                        film=c["off"], fslab=new(ng, 2, N), fcounter=words(R))
    assert torch.equal(dz0, dz1) and torch.equal(dgb0, dgb1)


def test_training_step_folded_equals_unfolded(monkeypatch):
    """One training step of the small FiLM / multi_fuse fixture of tests/test_bsrnn_gpu.py with WESEP_FILM_FOLD=1 and =0 from
    the same seed: waveforms, loss and every parameter gradient bit-identical, except the four FiLM Linear tensors per fuse layer,
    whose operand (da, db) is summed in another order -- those against an fp64 recomputation from the same d(z')."""
    from oracle import bsrnn_oracle as O
    import wesep_amd.functional as F_
    from wesep_amd import dev
    from wesep_amd.functional import SISDRFn
    from tests.test_bsrnn_gpu import _build
    d = _cuda()
    kw = dict(num_repeat=2, spk_fuse_type="FiLM", multi_fuse=True, use_spk_transform=False)
    wav, tgt, emb = O.synth_batch(4, 16000, 11)
    caps = {"1": [], "0": []}
    arm = []
    real = F_.AffineFn

    class Spy:       # the unfolded arm's affine launches: input and incoming gradient of every fuse layer
        @staticmethod
        def apply(x, a, b, a0):
            out = real.apply(x, a, b, a0)
            rec = dict(z=x.detach().cpu())
            out.register_hook(lambda g_: rec.__setitem__("dzp", g_.detach().cpu()))
            caps[arm[-1]].append(rec)
            return out

    # Peak memory of an arm = the high-water mark of its step ABOVE what is allocated when the arm starts.  Every result is kept on
    # the host, so no arm's clones sit in the other's figure; an unmeasured step comes first, so that what the process keeps for
    # good (zeroed counter words, the fall-back scratch of the cluster recurrence) exists before either measured arm.
    res = {}
    wav_d, tgt_d, emb_d = wav.to(d), tgt.to(d), emb.to(d)
    for label, fold in (("warm", "1"), ("1", "1"), ("0", "0")):
        monkeypatch.setenv("WESEP_FILM_FOLD", fold)
        monkeypatch.setattr(F_, "AffineFn", Spy)
        arm.append(fold)
        caps[fold].clear()
        cfg, params, model = _build(kw, 8, d)
        model.train()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        est, _ = model(wav_d, emb_d)
        loss = SISDRFn.apply(est, tgt_d, 1e-8)
        loss.backward()
        torch.cuda.synchronize()
        res[label] = dict(est=est.detach().cpu(), loss=loss.detach().cpu(), peak=torch.cuda.max_memory_allocated() - base,
                          grads={n: p.grad.detach().cpu() for n, p in model.named_parameters()})
        del model, est, loss
    assert not caps["1"]                                            # the folded arm launched no affine ...
    caps = caps["0"]                                                # ... the unfolded arm one per fuse layer
    assert len(caps) == 2 and all("dzp" in r_ for r_ in caps)
    on, off = res["1"], res["0"]
    assert torch.equal(on["est"], off["est"]) and torch.equal(on["loss"], off["loss"])
    film_names = [n for n in on["grads"] if ".fc.gamma_fcs." in n or ".fc.beta_fcs." in n]
    assert len(film_names) == 8
    for n in on["grads"]:
        if n not in film_names:
            assert torch.equal(on["grads"][n], off["grads"][n]), n
    zp_bytes = sum(r_["z"].numel() * 4 for r_ in caps)             # the z' of the two fuse layers: what the fold no longer keeps
    print(f"film fold model: peak above the arm's start {on['peak'] / 1e6:.2f} MB folded, {off['peak'] / 1e6:.2f} MB unfolded "
          f"(difference {(off['peak'] - on['peak']) / 1e6:.2f} MB; the two z' are {zp_bytes / 1e6:.2f} MB)")
    assert on["peak"] <= off["peak"]
    # the four FiLM Linear gradients per fuse layer: dW = d(operand)^T e, dbias = column sums, d(operand) = da | db
    e64 = emb.double()
    R = e64.shape[0]
    eg = eps_for(dev.gemm_mode() == "bf16x3", R)
    layers = sorted({n.split(".fc.")[0] for n in film_names}, key=lambda s: int(s.rsplit(".", 1)[1]))
    worst = 0.0
    for prefix, rec in zip(layers, caps):
        z64, g64 = rec["z"].double(), rec["dzp"].double()
        n_terms = z64.shape[1] * z64.shape[2]
        for fc, terms in (("gamma_fcs", g64 * z64), ("beta_fcs", g64)):
            op, S = terms.sum(dim=(1, 2)), terms.abs().sum(dim=(1, 2))        # [R, N]: fp64 operand, scale of its fp32 sum
            E = eps_for(False, n_terms) * S                                    # bound of the fp32 operand
            refs = {"weight": (op.t() @ e64, E.t() @ e64.abs() + eg * ((op.abs() + E).t() @ e64.abs())),
                    "bias": (op.sum(0), E.sum(0) + eps_for(False, R) * (op.abs() + E).sum(0))}
            for leaf, (ref, bound) in refs.items():
                got = on["grads"][f"{prefix}.fc.{fc}.0.{leaf}"].double()
                ratio = float(((got - ref).abs() / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (prefix, fc, leaf, ratio)
    print(f"film fold model: FiLM Linear gradients, worst error / bound = {worst:.4f}")
