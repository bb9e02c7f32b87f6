"""CPU checks of the feature-map contract suite (tests/map_contract.py): nothing here needs a GPU.

  - the generator: every legal pair of dimension values is in a case, every pair left out names its rule, every dispatch
    target of INST is reached by MIN_PER_TARGET cases, the case count stays under the cap, two calls give the same list;
  - SECOND OPINION: the float64 reference equals an independent statement to 1e-12 relative on every case -- F.unfold /
    F.fold, F.avg_pool2d and its autograd, F.interpolate(mode="bilinear", align_corners=False) and its autograd,
    F.instance_norm + F.elu under autograd (the sums -> finalize -> apply chain and the backward pair, evaluated at the
    float64 statistics), torch.softmax under autograd, einsum for freq_linear, torch's own tanh / sigmoid / elu backward;
  - perfect(b, ref) passes the checker, and correct fp32 arithmetic stays inside the bounds: every output of every case
    emulated in float32 with its sums sequential and pairwise (bilinear with the fp32 coordinate arithmetic of bl_src and the
    fp32 window of bl_window); the worst err / bound per entry is printed;
  - tests/emu_dev.py, extended by the single entries it lacked, stays inside the bounds through the same calls;
  - SENSITIVITY: every planted defect of map_contract.DEFECTS is refused on at least one case of its entry, by the reference
    alone (this is what fixes the suite's size condition, CAP);
  - every case passes the argument checks of the real libwesep_hip.so (tests/abi_dryrun.py), and the argument sets the
    library refuses come back WS_ERR_INVALID."""
import pytest
import torch
import torch.nn.functional as F

from tests import abi_dryrun
from tests import gemm_contract as gc
from tests import map_contract as mc

F64 = torch.float64
MAX_CASES_PER_ENTRY = 80


def _close(a, b, what, cond=1.0, floor=0.0):
    """1e-12 relative to the largest value -- times `cond` where the float64 statement itself cancels (the one-pass variance
    E[u^2] - mean^2 of offset or constant data loses E[u^2] / (var + eps) of its 1e-16)."""
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    tol = 1e-12 * max(cond * float(b.abs().max()), floor, 1e-300)      # floor: the size of the terms that cancel in b
    assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)


def _nchw(x, B, H, W, C):
    return x.reshape(B, H, W, C).permute(0, 3, 1, 2)


def _cl(y):
    return y.permute(0, 2, 3, 1).reshape(-1)


@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_generator_covers_pairs_and_targets(entry):
    cs = mc.cases(entry)
    assert len(cs) <= MAX_CASES_PER_ENTRY, len(cs)
    assert [c.name for c in cs] == [c.name for c in mc.cases(entry)]
    inv = mc.invalid_pairs(entry)
    assert not [w for w in inv.values() if w.startswith("UNNAMED")], inv
    covered = set()
    for c in cs:
        if all(k in c.dims for k in mc.DIMS[entry]) and all(c.dims[k] in mc.DIMS[entry][k] for k in c.dims):
            covered |= mc.pairs_of(entry, c.dims)
    missing = [p for p in mc.all_pairs(entry) if p not in covered and p not in inv]
    assert not missing, missing[:5]
    count = {}
    for c in cs:
        assert c.targets == mc._targets(entry, c.dims)
        for t in c.targets:
            count[t] = count.get(t, 0) + 1
    for t in mc.INST[entry]:
        assert count.get(t, 0) >= min(gc.MIN_PER_TARGET, len(cs)), (t, count.get(t, 0))


def test_total_case_count_and_seam_values():
    assert sum(len(mc.cases(e)) for e in mc.ENTRIES) <= 800
    assert any(c.dims["sz"] == 32 for c in mc.cases("avgpool_fwd")) and any(c.dims["sz"] == 32 for c in mc.cases("avgpool_bwd"))
    ts = {(c.dims["C"], mc.sb_T(c.dims)) for c in mc.cases("scale_bf_bwd")}
    assert {(8, 127), (8, 128), (8, 129), (8, 256), (8, 257), (64, 15), (64, 17), (64, 33), (6, 42), (1028, 3)} <= ts, sorted(ts)
    # suite condition: no sum above CAP leaves without its spike, groups of the norm entries far below it
    assert max(mc.NORM_P) <= mc.CAP
    for c in mc.cases("scale_bf_bwd"):
        b = mc.build(c)
        sp = b.spec
        x = b.views(b.bufs)["x"][:sp["B"] * sp["T"] * sp["F"] * sp["C"]]
        assert (sp["T"] * sp["C"] > mc.CAP) == bool(x.abs().max() > 400), c.name


def _second_opinion(b):
    e, sp = b.case.entry, b.spec
    t = b.views(b.bufs)
    v = mc.compute(e, sp, t, F64)
    if e == "im2col":
        R, H, W, C, k = sp["R"], sp["H"], sp["W"], sp["C"], sp["k"]
        u = F.unfold(_nchw(t["x"][:R * H * W * C].double(), R, H, W, C), k, padding=sp["p"], stride=(sp["sh"], sp["sw"]))
        L = u.shape[-1]
        _close(v["patches"], u.reshape(R, C, k * k, L).permute(0, 3, 2, 1), "unfold")
    elif e == "col2im":
        R, H, W, C, k = sp["R"], sp["H"], sp["W"], sp["C"], sp["k"]
        Ho, Wo = mc.conv_geom(sp)
        dp = t["dpatches"][:R * Ho * Wo * k * k * C].double()
        u = dp.reshape(R, Ho * Wo, k * k, C).permute(0, 3, 2, 1).reshape(R, C * k * k, Ho * Wo)
        _close(v["dx"], _cl(F.fold(u, (H, W), k, padding=sp["p"], stride=(sp["sh"], sp["sw"]))), "fold")
    elif e in ("elu_fwd", "elu_bwd"):
        x = t["x"][:sp["n"]].double().requires_grad_(True)
        y = F.elu(x)
        if e == "elu_fwd":
            _close(v["y"], y, "elu")
        else:
            _close(v["dx"], torch.autograd.grad((y * t["dy"][:sp["n"]].double()).sum(), x)[0], "elu'")
    elif e == "inorm_finalize":
        G, P, C = sp["G"], sp["P"], sp["C"]
        s = t["sums"][:G * 2 * C].reshape(G, 2, C).double()
        mean = s[:, 0] / P
        _close(v["stats"][:, 0], mean, "mean")
        var = (s[:, 1] / P - mean ** 2).clamp_min(0)
        _close(v["stats"][:, 1], var.add(sp["eps"]).rsqrt(), "rstd", float((s[:, 1] / P / (var + sp["eps"])).max()))
    elif e in ("inorm_apply", "inorm_bwd_apply", "in_act_sums", "in_act_apply", "in_act_bwd_apply"):
        _second_opinion_norm(b, t)
    elif e in ("avgpool_fwd", "avgpool_bwd"):
        B, H, W, C, sz = sp["B"], sp["H"], sp["W"], sp["C"], sp["sz"]
        x = (t["x"][:B * H * W * C].double() if e == "avgpool_fwd" else torch.zeros(B * H * W * C, dtype=F64)).requires_grad_(True)
        y = F.avg_pool2d(_nchw(x, B, H, W, C), sz)
        if e == "avgpool_fwd":
            _close(v["y"], _cl(y), "avg_pool2d")
        else:
            dy = _nchw(t["dy"][:y.numel()].double(), B, H // sz, W // sz, C)
            _close(v["dx"], torch.autograd.grad((y * dy).sum(), x)[0], "avg_pool2d'")
    elif e in ("bilinear_fwd", "bilinear_bwd"):
        B, h, w, H, W, C = sp["B"], sp["h"], sp["w"], sp["H"], sp["W"], sp["C"]
        x = (t["x"][:B * h * w * C].double() if e == "bilinear_fwd" else torch.zeros(B * h * w * C, dtype=F64)).requires_grad_(True)
        y = F.interpolate(_nchw(x, B, h, w, C), size=(H, W), mode="bilinear", align_corners=False)
        if e == "bilinear_fwd":
            _close(v["y"], _cl(y), "interpolate")
        else:
            dy = _nchw(t["dy"][:B * H * W * C].double(), B, H, W, C)
            _close(v["dx"], torch.autograd.grad((y * dy).sum(), x)[0], "interpolate'")
    elif e in ("scale_bf_fwd", "scale_bf_bwd"):
        B, T, Fq, C = sp["B"], sp["T"], sp["F"], sp["C"]
        x = t["x"][:B * T * Fq * C].reshape(B, T, Fq, C).double().requires_grad_(True)
        s = t["s"][:B * Fq].reshape(B, 1, Fq, 1).double().requires_grad_(True)
        y = x * s if sp["mode"] == 0 else x + s
        if e == "scale_bf_fwd":
            _close(v["y"], y, "y")
        else:
            dx, ds = torch.autograd.grad((y * t["dy"][:y.numel()].reshape(y.shape).double()).sum(), (x, s))
            _close(v["dx"], dx, "dx")
            _close(v["ds"], ds, "ds")
    elif e == "freq_linear":
        B, T, Fq, C = sp["B"], sp["T"], sp["F"], sp["C"]
        x = t["x"][:B * T * Fq * C].reshape(B, T, Fq, C).double()
        Wm = t["W"][:Fq * sp["ldw"]].reshape(Fq, sp["ldw"])[:, :Fq].double()
        _close(v["y"], torch.einsum("gf,btfc->btgc", Wm, x) + t["rb"][:B * Fq].reshape(B, 1, Fq, 1).double(), "einsum")
    elif e in ("softmax_fwd", "softmax_bwd"):
        rows, n = sp["rows"], sp["n"]
        sc = float(torch.tensor(sp["scale"], dtype=torch.float32))
        if e == "softmax_fwd":
            _close(v["y"], torch.softmax(sc * t["x"][:rows * n].reshape(rows, n).double(), 1), "softmax")
        else:       # dx in terms of y: autograd through log-free softmax at logits that reproduce y
            y, dy = t["y"][:rows * n].reshape(rows, n).double(), t["dy"][:rows * n].reshape(rows, n).double()
            J = torch.diag_embed(y) - y.unsqueeze(2) * y.unsqueeze(1)
            _close(v["dx"], sc * torch.einsum("rij,rj->ri", J, dy), "softmax'", floor=float((abs(sc) * y * (dy.abs() + (dy * y).abs().sum(1, keepdim=True))).max()))
    elif e == "rowbias_act":
        rows, C = sp["rows"], sp["C"]
        pre = t["x"][:rows * C].reshape(rows, C).double()
        if sp["rb"]:
            pre = pre + t["rb"][:-(-rows // sp["rpr"]) * C].reshape(-1, C).double().repeat_interleave(sp["rpr"], 0)[:rows]
        _close(v["y"], torch.tanh(pre) if sp["act"] == 1 else torch.sigmoid(pre), "act")
    elif e == "act_bwd":
        y, dy = t["y"][:sp["n"]].double(), t["dy"][:sp["n"]].double()
        z = (torch.atanh(y) if sp["act"] == 1 else torch.logit(y)).requires_grad_(True)
        g = torch.autograd.grad(((torch.tanh(z) if sp["act"] == 1 else torch.sigmoid(z)) * dy).sum(), z)[0]
        a, bb = v["dx"].reshape(-1), g.reshape(-1)
        assert float((a - bb).abs().max()) <= 1e-9 * max(float(bb.abs().max()), 1e-300)      # atanh / logit of an fp32 y near 1
    else:
        raise AssertionError(e)


def _second_opinion_norm(b, t):
    """The chain in float64 at the float64 statistics against F.instance_norm + F.elu under autograd."""
    e, sp = b.case.entry, b.spec
    G, P, C, flags, eps = sp["G"], sp["P"], sp["C"], sp["flags"], sp["eps"]
    if e == "inorm_bwd_apply":
        return _second_opinion_inorm_bwd(b, t)
    x = t["x"][:G * P * C].reshape(G, P, C).double().requires_grad_(True)
    u = F.elu(x) if flags & 1 else x
    ud = u.detach()
    cond = float(((ud * ud).mean(1) / (((ud * ud).mean(1) - ud.mean(1) ** 2).clamp_min(0) + eps)).max()) * (1 + float(ud.abs().max()))
    n = F.instance_norm(u.permute(0, 2, 1), eps=eps).permute(0, 2, 1) if P > 1 else (u - u) / torch.sqrt(torch.tensor(eps, dtype=F64))
    y = F.elu(n) if flags & 2 else n
    # the suite's own chain: forward sums -> finalize -> (apply | backward sums -> bwd_apply), all float64
    spf = dict(sp, bwd=False, nsplit=1)
    sums = mc.compute("in_act_sums", spf, {"x": t["x"]}, F64)["slab"][0]
    stats = mc.compute("inorm_finalize", sp, {"sums": sums.reshape(-1)}, F64)["stats"]
    t2 = dict(t, stats=stats.reshape(-1))
    if e in ("inorm_apply", "in_act_apply"):
        _close(mc.compute(e, sp, t2, F64)["y"], y, "y", cond, float(ud.abs().max() * stats[:, 1].max()))
        return
    if e == "in_act_sums" and not sp["bwd"]:
        _close(mc.compute("in_act_apply", sp, t2, F64)["y"], y, "y from the sums", cond, float(ud.abs().max() * stats[:, 1].max()))
        return
    spb = dict(sp, bwd=True, nsplit=3)
    dyv = mc._rows(t["dy"], G * P, sp["ldd"], sp["dy_off"], C).reshape(G, P, C).double()
    (dx,) = torch.autograd.grad((y * dyv).sum(), x)
    bs = mc.compute("in_act_sums", spb, t2, F64)["slab"].sum(0)
    got = mc.compute("in_act_bwd_apply", dict(sp, lddx=C, dx_off=0), dict(t2, sums=bs.reshape(-1)), F64)["dx"]
    a, bb = got.reshape(-1), dx.reshape(-1)
    # constant groups: autograd divides 0 by sqrt(eps) chains of ~316 per factor; the tolerance follows the gradient's scale
    tol = 1e-12 * cond * max(float(bb.abs().max()), float(dyv.abs().max()) / eps ** 0.5)
    assert float((a - bb).abs().max()) <= tol, (float((a - bb).abs().max()), tol)


def _second_opinion_inorm_bwd(b, t):
    sp = b.spec
    G, P, C, eps = sp["G"], sp["P"], sp["C"], sp["eps"]
    # x is not an operand of ws_inorm_bwd_apply: rebuild one that has exactly these statistics and this y
    st = t["stats"][:G * 2 * C].reshape(G, 2, C).double()
    y, dy = t["y"][:G * P * C].reshape(G, P, C).double(), t["dy"][:G * P * C].reshape(G, P, C).double()
    sm = t["sums"][:G * 2 * C].reshape(G, 2, C).double()
    assert float((sm[:, 0] - dy.sum(1)).abs().max()) <= 2.0 ** -23 * float(dy.abs().sum(1).max())      # uploaded as fp32
    got = mc.compute("inorm_bwd_apply", sp, dict(t, sums=torch.stack([dy.sum(1), (dy * y).sum(1)], 1).reshape(-1)), F64)["dx"]
    want = st[:, 1:2] * (dy - dy.mean(1, keepdim=True) - y * (dy * y).mean(1, keepdim=True))
    _close(got, want, "dx")
    if P > 1 and b.case.dims["data"] == "gauss":      # and autograd through F.instance_norm where y is its output
        x = (y / st[:, 1:2] + st[:, 0:1]).requires_grad_(True)
        yy = F.instance_norm(x.permute(0, 2, 1), eps=eps).permute(0, 2, 1)
        (dx,) = torch.autograd.grad((yy * dy).sum(), x)
        assert float((got - dx).abs().max()) <= 2e-5 * float(dx.abs().max())      # y and stats are fp32 roundings: 1e-7 * rstd terms


@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_reference_equals_torch_float64_and_perfect_outputs_pass(entry):
    for c in mc.cases(entry):
        b = mc.build(c)
        _second_opinion(b)
        ref = mc.reference(b)
        assert mc.verify(b, ref, mc.perfect(b, ref)) <= 1.0, c.name


WORST = {}


@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_fp32_emulation_stays_inside_the_bounds(entry):
    worst = (0.0, "")
    for c in mc.cases(entry):
        b = mc.build(c)
        ref = mc.reference(b)
        for order in mc.ORDERS:
            r = mc.verify(b, ref, mc.emulate(b, ref, order), what=f"{entry} {c.name} [{order}]")
            if r > worst[0]:
                worst = (r, f"{c.name} [{order}]")
    WORST[entry] = worst
    print(f"{entry}: worst err / bound of the fp32 emulation {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0


@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_emu_dev_stays_inside_the_bounds(entry):
    """tests/emu_dev.py (the fp32 library-call emulation the host-path tests run the models on) through the same calls."""
    from tests import emu_dev
    worst = (0.0, "")
    for c in mc.cases(entry):
        b = mc.build(c)
        ref = mc.reference(b)
        t = {k: v.clone() for k, v in b.bufs.items()}
        mc.run(emu_dev, b, t)
        if "tmp" in t:
            t["tmp"][torch.isnan(t["tmp"])] = 0.0      # emu_dev has no scratch
        r = mc.verify(b, ref, t, what=f"emu_dev {entry} {c.name}")
        if r > worst[0]:
            worst = (r, c.name)
    print(f"{entry}: worst err / bound of emu_dev {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("entry,defect", [(e, d) for e, ds in mc.DEFECTS.items() for d in ds])
def test_planted_defect_is_refused(entry, defect):
    caught = []
    for c in mc.cases(entry):
        b = mc.build(c)
        ref = mc.reference(b)
        try:
            mc.verify(b, ref, mc.emulate(b, ref, "seq", defect))
        except mc.ContractViolation as v:
            caught.append((c.name, v.kind))
    print(f"{entry} {defect}: refused on {len(caught)} of {len(mc.cases(entry))} cases")
    assert caught, f"{entry}: the planted defect {defect} passes every case"


def test_unwritten_and_overwritten_outputs_are_refused():
    b = mc.build(mc.cases("im2col")[0])
    ref = mc.reference(b)
    good = mc.perfect(b, ref)
    for name, kind, edit in (("patches", "nan", lambda t: t.__setitem__(int(b.start["patches"]), float("nan"))),
                             ("patches", "sentinel", lambda t: t.__setitem__(3, 0.0))):
        bad = {k: v.clone() for k, v in good.items()}
        edit(bad[name])
        with pytest.raises(mc.ContractViolation) as ei:
            mc.verify(b, ref, bad)
        assert ei.value.kind == kind
    c1 = next(c for c in mc.cases("im2col") if c.dims["ldp"] == "kk+3")
    b = mc.build(c1)
    ref = mc.reference(b)
    bad = mc.perfect(b, ref)
    bad["patches"][b.start["patches"] + b.spec["k"] ** 2] = 0.0          # the first padding column of row 0
    with pytest.raises(mc.ContractViolation) as ei:
        mc.verify(b, ref, bad)
    assert ei.value.kind == "sentinel"


def test_dispatch_mirrors_agree_with_the_source_text():
    import os
    src = open(os.path.join(os.path.dirname(__file__), "..", "wesep_amd", "csrc", "conv2d.hip")).read()
    assert "C % 4 == 0 && C <= 1024 && 256 % (C / 4) == 0" in src          # sb_vec
    assert src.count("n <= 1024 && n % 4 == 0 && ((size_t)") == 2         # softmax_vec
    assert "const int per = (P + nsplit - 1) / nsplit;" in src and "const int nq = min(256, c4n - cz);" in src
    assert "(long long)Fq * C <= 16384" in src
    assert "b > 65536 ? 65536 : b" in src                                  # the grid-stride seam of the GPU test


@pytest.mark.parametrize("entry", mc.ENTRIES)
def test_every_case_passes_the_library_contract(entry, monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    n = 0
    for c in mc.cases(entry):
        b = mc.build(c)
        mc.run(dev, b, b.bufs)
        n += 1
    abi_dryrun.assert_contracts_hold(calls, at_least=n)
    assert len(calls) == n


def test_invalid_argument_sets_are_refused(monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    t = torch.zeros(1 << 16)
    for name, call in mc.refusals(dev, t):
        del calls[:]
        call()
        assert calls and calls[0][1] == abi_dryrun.WS_ERR_INVALID, (name, calls)
