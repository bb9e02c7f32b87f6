"""CPU checks of the training-step contract suite (tests/step_contract.py): nothing here needs a GPU.

  - the generator: every legal pair of dimension values is in a case, every pair left out names its rule, every dispatch
    target of INST is reached by MIN_PER_TARGET cases (the grid-cap case of affine_fwd exactly once), the listed seam values
    are all there, two calls give the same list;
  - SECOND OPINION: the float64 reference equals independent statements to 1e-12 relative on every case -- torch autograd on
    oracle.bsrnn_oracle.sisdr_loss for the loss, for c1 / c2 and for the gradient with a non-unit gout; clip_gradients_ and
    adam_l2_step_ of the oracle; tests/emu_dev.py's heads_fwd / heads_bwd and tstp_bwd; autograd on the affine.  Where the two
    sides differ by construction the tolerance says so at its place: the SI-SDR gradient is compared at 1e-9 of its largest
    element (autograd differentiates through the means, the closed form cancels them), the oracle clips with the float64 norm
    and divides by float64 bias corrections where the contract has fp32 ones (u relative), LayerNorm's eps is a C float;
  - perfect(b, ref) passes the checker, and correct fp32 arithmetic stays inside the bounds: every output of every case
    emulated in float32 with its sums sequential and pairwise; the worst err / bound per entry is printed;
  - CONDITION: the derived bound on sisdr_dB stays below 1e-2 dB on every ordinary regime at T <= 2048;
  - SENSITIVITY: every planted defect of step_contract.DEFECTS is refused on at least one case of its entry, by the reference
    alone (the SI-SDR defects: on an ordinary regime);
  - the dispatch mirrors of INST agree with the source text;
  - every case passes the argument checks of the real libwesep_hip.so (tests/abi_dryrun.py), and the argument sets the
    library refuses come back WS_ERR_INVALID."""
import math
import os
import warnings

import pytest
import torch

from oracle import bsrnn_oracle as orc
from tests import abi_dryrun, emu_dev
from tests import gemm_contract as gc
from tests import step_contract as sc

F64 = torch.float64
MAX_CASES_PER_ENTRY = 100


def _close(a, b, what, floor=0.0):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    tol = 1e-12 * max(float(b.abs().max()) if b.numel() else 0.0, floor, 1e-300)
    assert a.shape == b.shape and float((a - b).abs().max() if b.numel() else 0.0) <= tol, (what, float((a - b).abs().max()), tol)


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_generator_covers_pairs_and_targets(entry):
    cs = sc.cases(entry)
    assert len(cs) <= MAX_CASES_PER_ENTRY, len(cs)
    assert [c.name for c in cs] == [c.name for c in sc.cases(entry)]
    inv = sc.invalid_pairs(entry)
    assert not [w for w in inv.values() if w.startswith("UNNAMED")], inv
    covered = set()
    for c in cs:
        covered |= sc.pairs_of(entry, c.dims)
    missing = [p for p in sc.all_pairs(entry) if p not in covered and p not in inv]
    assert not missing, missing[:5]
    for d, vals in sc.DIMS[entry].items():
        assert {c.dims[d] for c in cs} >= set(vals), (d, vals)
    count = {}
    for c in cs:
        assert c.targets == sc._targets(entry, c.dims)
        for t in c.targets:
            count[t] = count.get(t, 0) + 1
    for t in sc.INST[entry]:
        if t in sc.EXACT_COUNT:
            assert count.get(t, 0) == sc.EXACT_COUNT[t], (t, count.get(t, 0))
        else:
            assert count.get(t, 0) >= min(gc.MIN_PER_TARGET, len(cs)), (t, count.get(t, 0))
    assert set(count) <= set(sc.INST[entry]), set(count) - set(sc.INST[entry])


def test_total_case_count_and_seam_values():
    assert sum(len(sc.cases(e)) for e in sc.ENTRIES) <= 700
    big = [c for c in sc.cases("affine_fwd") if "affine_fwd[grid cap]" in c.targets]
    assert len(big) == 1 and big[0].dims["R"] * big[0].dims["rpr"] * big[0].dims["N"] // 4 == 4194560
    ab = sc.cases("affine_bwd")
    assert {c.dims["N"] for c in ab if "affine_bwd_kernel" in c.targets} == {1, 3, 126, 127}
    assert any(c.dims["R"] == 1 and not c.dims["dz_in"] for c in ab) and any(not c.dims["zin"] and c.dims["dadb"] for c in ab)
    for e in ("sisdr_fwd", "sisdr_bwd"):
        cs = sc.cases(e)
        assert {c.dims["regime"] for c in cs} == set(sc.ORDINARY + sc.ILL)
        for c in cs:          # suite condition: no row above CAP without its spike
            b = sc.build(c)
            assert (c.dims["T"] > sc.CAP) == bool(b.views(b.bufs)["est"].abs().max() > 400), c.name
        assert sum(1 for c in cs if c.dims["regime"] in sc.ORDINARY and c.dims["T"] <= sc.CAP) >= 10
    assert any(c.dims["gout"] == -2.5 and c.dims["R"] > 1 for c in sc.cases("sisdr_bwd"))
    for c in sc.cases("grad_norms"):
        b = sc.build(c)
        assert (c.dims["numel"] > sc.CAP and c.dims["poison"] == "none") <= bool(b.views(b.bufs)["g0"].abs().max() > 40), c.name
    ca = sc.cases("clip_adam_step")
    assert any(sc.build(c).spec["lag"] is not None and sc.build(c).spec["lag"] >= c.dims["step"] for c in ca if "clip_adam_kernel[step_lag]" in c.targets)
    clipped = set()
    for c in ca:          # the clip value clips some tensors and not others; some case leaves a gradient bit-untouched next to a scaled one
        b = sc.build(c)
        if b.spec["clip"] > 0 and not sc._skipped(b.spec):
            clipped |= {sc._coef32(b.spec, i, b.views(b.bufs)) < 1.0 for i in range(len(b.spec["numel"])) if i != b.spec["null"]}
    assert clipped == {True, False}
    gcm = {(c.dims["g0"], c.dims["skip1"]) for c in sc.cases("guard_commit")}
    assert gcm == {(g, s) for g in (0, 1, 9) for s in ("null", "zero", "set")}
    for e in ("heads_fwd", "heads_bwd"):
        ws = {c.dims["Q"] * c.dims["nh"] * c.dims["ch"] for c in sc.cases(e)}
        assert {28, 4096, 4100, 9216} <= ws, sorted(ws)
        for c in sc.cases(e):
            assert c.dims["Q"] * c.dims["ch"] <= sc.CAP
            x = sc.build(c).views(sc.build(c).bufs)["x"]
            assert bool((x == 0).any()) or x.numel() < 11
    hb = sc.cases("heads_bwd")
    assert any(sc.hd_nwg(c.dims) > c.dims["B"] * c.dims["T"] for c in hb) and any(sc.hd_nwg(c.dims) == 1 and c.dims["B"] * c.dims["T"] > 1 for c in hb)
    assert {c.dims["T"] for c in sc.cases("tstp_bwd")} == {1, 2, 9}


def _sisdr_second_opinion(b, v, bwd):
    sp, t = b.spec, b.views(b.bufs)
    R, T = sp["R"], sp["T"]
    eps = float(sc._f32(sp["eps"]))
    x = t["est"].reshape(R, T).double().requires_grad_(True)
    tg = t["tgt"].reshape(R, T).double()
    loss = orc.sisdr_loss(x, tg, eps)
    if not bwd:
        rs = v["rowstat"]
        _close(v["loss"], loss, "loss", 1.0)
        # c1 / c2 against autograd: d loss / d x = (c1 tc + c2 res) / R
        gx = torch.autograd.grad(loss, x)[0]
        tcn = tg - rs[:, 1:2]
        res = (x.detach() - rs[:, 0:1]) - rs[:, 2:3] * tcn
        mine = (rs[:, 3:4] * tcn + rs[:, 4:5] * res) / R
        # autograd differentiates the means as well; the closed form is its projection: both are mean-free in exact arithmetic
        _close(mine, gx, "c1 / c2", float(gx.abs().max()) * 1e3 + float(mine.abs().max()) * 1e3)
        return
    go = float(t["gout"][0])
    # at the uploaded fp32 rowstat the closed form is evaluated as is; autograd is the check of the form at float64 statistics
    rs64 = sc._sisdr_rows(sp, t, F64, "seq")
    v64 = sc.compute("sisdr_bwd", sp, dict(t, rowstat=rs64.reshape(-1)), F64)
    gx = torch.autograd.grad(loss * go, x)[0]
    _close(v64["dest"], gx, "gradient", float(gx.abs().max()) * 1e3)


def _second_opinion(b):
    e, sp = b.case.entry, b.spec
    t = b.views(b.bufs)
    v = sc.compute(e, sp, t, F64)
    if e in ("affine_fwd", "affine_bwd"):
        R, rpr, N = sp["R"], sp["rpr"], sp["N"]
        M = R * rpr
        z = t["z" if e == "affine_fwd" else ("z_in" if sp["zin"] else "dz")].reshape(M, N).double().requires_grad_(True)
        a = (t["a"].reshape(R, N).double() if sp["a"] else torch.zeros(R, N, dtype=F64)).requires_grad_(True)
        bb = (t["b"].reshape(R, N).double() if e == "affine_fwd" and sp["b"] else torch.zeros(R, N, dtype=F64)).requires_grad_(True)
        out = z * (float(sc._f32(sp["a0"])) + a.repeat_interleave(rpr, 0)) + bb.repeat_interleave(rpr, 0)
        if e == "affine_fwd":
            s32 = (float(sc._f32(sp["a0"])) + a.detach()).float().double().repeat_interleave(rpr, 0)          # a0 + a rounds first, as in the kernel
            want = z.detach() * s32 + bb.detach().repeat_interleave(rpr, 0)
            assert bool(((v["out"] - want).abs() <= 2.0 ** -24 * want.abs() * (1 + 1e-9)).all()), "one rounding of the float64 expression"
            assert torch.equal(v["out"], v["out"].float().double())
            return
        dz = t["dz"].reshape(M, N).double()
        gz, ga, gb = torch.autograd.grad((out * dz).sum(), (z, a, bb))
        if sp["dz_in"]:
            _close(v["dz_in"], gz, "dz_in")
        fl = float(dz.abs().max() * (1 + z.detach().abs().max())) * 8
        _close(v["db_slab"].sum(0), gb, "db slab", fl)
        if sp["zin"]:
            _close(v["da_slab"].sum(0), ga, "da slab", fl)
        if sp["dadb"]:
            _close(v["db"], gb, "db", fl)
            if sp["zin"]:
                _close(v["da"], ga, "da", fl)
    elif e in ("sisdr_fwd", "sisdr_bwd"):
        if sp["regime"] in sc.ORDINARY and sp["T"] > 1:          # (the closed form is ill-conditioned elsewhere by construction)
            _sisdr_second_opinion(b, v, e == "sisdr_bwd")
    elif e == "grad_norms":
        for i, n in enumerate(sp["numel"]):
            if i == sp["null"]:
                assert float(v["norms"][i]) == 0.0
            elif sp["poison"] in ("none", "overflow") or i:
                _close(v["norms"][i], list(orc.clip_gradients_({"g": t[f"g{i}"].double().clone()}, 1e30).values())[0] * torch.ones((), dtype=F64), "norm")
    elif e == "clip_adam_step":
        if sc._skipped(sp):
            for k, x in v.items():
                if k[0] in "pgmv":
                    assert torch.equal(x, t[k].double()), k
            return
        for i, n in enumerate(sp["numel"]):
            if i == sp["null"]:
                continue
            g = t[f"g{i}"].double().clone()
            if sp["clip"] > 0:
                # (the oracle clips with the float64 norm, the contract with fp32 arithmetic on the uploaded norm: 1e-6 apart)
                orc.clip_gradients_({"g": g}, sp["clip"])
                assert float((v[f"g{i}"] - g).abs().max()) <= 1e-6 * float(g.abs().max()), "clip"
            g = v[f"g{i}"].clone()
            if sp["clip_only"]:
                continue
            p, m, vv = (t[f"{k}{i}"].double().clone() for k in "pmv")
            f = lambda k: float(sc._f32(sp[k]))          # noqa: E731
            step = sp["step"] if sp["lag"] is None else max(sp["step"] - sp["lag"], 1)
            orc.adam_l2_step_(p, g, m, vv, step, f("lr"), f("beta1"), f("beta2"), f("eps"), f("wd"))
            _close(v[f"m{i}"], m, "exp_avg")
            _close(v[f"v{i}"], vv, "exp_avg_sq")
            # (bc1 / bc2_sqrt are fp32 in the contract, float64 in the oracle: 2^-24 relative on the update)
            assert float((v[f"p{i}"] - p).abs().max()) <= 3 * sc.U * float((p - t[f"p{i}"].double()).abs().max()) + 1e-12 * float(p.abs().max()), "param"
    elif e == "guard_commit":
        g = torch.tensor(sp["guard"])
        s1 = None if sp["skip1"] is None else torch.tensor([sp["skip1"]])
        from tests import emu_optim
        for it in (1, 2):
            emu_optim.guard_commit(g, s1)
            assert v[f"guard{it}"].tolist() == g.tolist()
    elif e in ("heads_fwd", "heads_bwd"):
        B, T, Tp, Q, nh, ch = (sp[k] for k in ("B", "T", "Tp", "Q", "nh", "ch"))
        D = Q * ch
        x = torch.nan_to_num(t["x"].double(), nan=0.0)
        if e == "heads_fwd":
            y, st = torch.zeros(nh * B * Tp * D, dtype=F64), torch.zeros(nh * B * T * 2, dtype=F64)
            emu_dev.heads_fwd(x, sp["ldx"], sp["x_off"], t["slope"].double(), t["gamma"].double(), t["beta"].double(), B, T, Tp, Q, nh, ch, y, st)
            # (eps is the C float 1e-5 in the contract, the double 1e-5 in the stand-in: 2.5e-13 apart)
            _close(v["y"], y, "y", float(y.abs().max()) * 100)
            _close(v["stats"], st, "stats", float(st.abs().max()) * 100)
        else:
            dx = torch.zeros(B * T * Q * sp["lddx"], dtype=F64)
            dy = torch.nan_to_num(t["dy"].double(), nan=0.0)
            dg, db, ds = emu_dev.heads_bwd(x, sp["ldx"], sp["x_off"], dy, t["slope"].double(), t["gamma"].double(), t["stats"].double(), B, T, Tp, Q,
                                           nh, ch, dx, sp["lddx"], sp["dx_off"])
            _close(v["dx"], dx.reshape(-1, sp["lddx"])[:, sp["dx_off"]:sp["dx_off"] + nh * ch], "dx")
            fl = float(dy.abs().max()) * 1e2
            _close(v["dgamma"], dg, "dgamma", fl)
            _close(v["dbeta"], db, "dbeta", fl)
            _close(v["dslope"], ds, "dslope", fl * 10)
            _close(v["slab"].sum(0)[:2 * Q * nh * ch], torch.cat([v["dgamma"].reshape(nh, Q, ch).permute(1, 0, 2).reshape(-1),
                                                                   v["dbeta"].reshape(nh, Q, ch).permute(1, 0, 2).reshape(-1)]), "slab", fl)
    elif e == "tstp_bwd":
        n = sp["R"] * sp["F"] * sp["T"] * sp["C"]
        dx = torch.zeros(n, dtype=F64)
        emu_dev.tstp_bwd(t["x"].double(), t["stats"].double(), t["dstats"].double(), sp["R"], sp["F"], sp["T"], sp["C"], dx)
        _close(v["dx"], dx, "dx")
    else:
        raise AssertionError(e)


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_reference_equals_second_opinions_and_perfect_outputs_pass(entry):
    for c in sc.cases(entry):
        b = sc.build(c)
        _second_opinion(b)
        ref = sc.reference(b)
        assert set(ref) == set(k for k in b.alias) | set(n for n in b.outs if n not in b.alias.values()) | set(b.extras), c.name
        assert sc.verify(b, ref, *sc.perfect(b, ref)) <= 1.0, c.name


def test_tstp_bwd_is_the_gradient_of_mean_and_std():
    """autograd through mean / sqrt(unbiased var + eps) at float64 statistics, T > 1."""
    for c in sc.cases("tstp_bwd"):
        b = sc.build(c)
        sp, t = b.spec, b.views(b.bufs)
        R, Fq, T, C = sp["R"], sp["F"], sp["T"], sp["C"]
        if T == 1:
            continue
        x = t["x"].reshape(R, Fq, T, C).double().requires_grad_(True)
        mean, sd = x.mean(2), torch.sqrt(x.var(2, unbiased=True) + sc.TSTP_EPS)
        st = torch.stack([mean.permute(0, 2, 1), sd.permute(0, 2, 1)], 1)
        want = torch.autograd.grad((st * t["dstats"].reshape(st.shape).double()).sum(), x)[0]
        got = sc.compute("tstp_bwd", sp, dict(t, stats=st.detach().reshape(-1)), F64)["dx"]
        _close(got, want, "tstp'", float(want.abs().max()) * 10)


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_fp32_emulation_stays_inside_the_bounds(entry):
    worst = (0.0, "")
    for c in sc.cases(entry):
        b = sc.build(c)
        ref = sc.reference(b)
        for order in sc.ORDERS:
            r = sc.verify(b, ref, *sc.emulate(b, ref, order), what=f"{entry} {c.name} [{order}]")
            if r > worst[0]:
                worst = (r, f"{c.name} [{order}]")
    print(f"{entry}: worst err / bound of the fp32 emulation {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0


def test_ordinary_sisdr_bound_is_below_the_named_tolerance():
    worst = 0.0
    n = 0
    for c in sc.cases("sisdr_fwd"):
        if c.dims["regime"] in sc.ORDINARY and c.dims["T"] <= sc.CAP:
            b = sc.build(c)
            bd = sc.reference(b)["rowstat"].bound.reshape(-1, 8)[:, 5]
            worst = max(worst, float(bd.max()))
            n += 1
            assert float(bd.max()) < sc.SISDR_TOL_DB, (c.name, float(bd.max()))
    print(f"ordinary SI-SDR regimes: {n} cases, widest bound on sisdr_dB {worst:.3e} dB")
    assert n >= 10


@pytest.mark.parametrize("entry,defect", [(e, d) for e, ds in sc.DEFECTS.items() for d in ds])
def test_planted_defect_is_refused(entry, defect):
    caught = []
    pool = [c for c in sc.cases(entry) if entry not in sc.ORDINARY_ONLY or c.dims["regime"] in sc.ORDINARY]
    pool = [c for c in pool if "affine_fwd[grid cap]" not in c.targets]
    for c in pool:
        b = sc.build(c)
        ref = sc.reference(b)
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                sc.verify(b, ref, *sc.emulate(b, ref, "seq", defect))
        except sc.ContractViolation as v:
            caught.append((c.name, v.kind))
    print(f"{entry} {defect}: refused on {len(caught)} of {len(pool)} cases")
    assert caught, f"{entry}: the planted defect {defect} passes every case"


def test_every_entry_has_a_planted_defect():
    assert set(sc.DEFECTS) == set(sc.ENTRIES)
    assert sum(len(v) for v in sc.DEFECTS.values()) >= 30
    for e in ("affine_bwd", "sisdr_fwd", "grad_norms", "clip_adam_step", "heads_fwd", "heads_bwd"):          # the kernels with a seam
        assert len(sc.DEFECTS[e]) >= 2


def test_unwritten_and_overwritten_outputs_are_refused():
    b = sc.build(next(c for c in sc.cases("heads_bwd") if c.dims["lddx"] != "ldx" and "heads_bwd[idle workgroups]" in c.targets))
    ref = sc.reference(b)
    good, extra = sc.perfect(b, ref)
    for kind, at in (("nan", int(b.start["dx"]) + b.spec["dx_off"]), ("sentinel", int(b.start["dx"]))):          # (column 0: outside the write set)
        bad = {k: v.clone() for k, v in good.items()}
        bad["dx"][at] = float("nan") if kind == "nan" else 0.0
        with pytest.raises(sc.ContractViolation) as ei:
            sc.verify(b, ref, bad, extra)
        assert ei.value.kind == kind
    ex2 = dict(extra, slab=extra["slab"].clone())
    ex2["slab"][-3] = 1e-30          # the slab row of a workgroup that owns no row is an exact zero
    with pytest.raises(sc.ContractViolation) as ei:
        sc.verify(b, ref, good, ex2)
    assert ei.value.kind == "exact"
    b = sc.build(next(c for c in sc.cases("clip_adam_step") if "clip_adam_kernel[skipped]" in c.targets))
    ref = sc.reference(b)
    bad, extra = sc.perfect(b, ref)
    bad["p0"][b.start["p0"]] += 1e-7          # a skipped launch leaves the weights to the bit
    with pytest.raises(sc.ContractViolation) as ei:
        sc.verify(b, ref, bad, extra)
    assert ei.value.kind == "exact"
    b = sc.build(next(c for c in sc.cases("grad_norms") if c.dims["poison"] == "overflow"))
    ref = sc.reference(b)
    bad, extra = sc.perfect(b, ref)
    bad["norms"][b.start["norms"]] = 1.0          # a finite norm of squares that overflow
    with pytest.raises(sc.ContractViolation):
        sc.verify(b, ref, bad, extra)


def test_dispatch_mirrors_agree_with_the_source_text():
    root = os.path.join(os.path.dirname(__file__), "..", "wesep_amd", "csrc")
    ew = open(os.path.join(root, "elementwise.hip")).read()
    hd = open(os.path.join(root, "heads.hip")).read()
    assert "if (N % 4 == 0)\n    hipLaunchKernelGGL(affine_bwd4_kernel" in ew          # N % 4
    assert "const int chunk = (rows_per_r + nsplit - 1) / nsplit;" in ew and ew.count("for (int j = lo + rl; j < hi; j += 16)") == 1
    assert "for (int j = lo + rl; j < hi; j += 2)" in ew
    assert "if (blocks > 16384) blocks = 16384;" in ew          # the grid cap of affine_fwd
    assert ew.count("i < T; i += 1024") == 3 and "for (int r = threadIdx.x; r < R; r += 64)" in ew          # the 1024-thread passes, the 64-lane mean
    assert "for (long long i = threadIdx.x; i < t.numel; i += 1024)" in ew          # the norm loop
    assert "dim3(ntensors, 16), dim3(256)" in ew and "i += (long long)gridDim.y * blockDim.x" in ew          # the 16 x 256 stride
    assert "const double eff = (double)max(step - (int)lag, 1);" in ew
    assert hd.count("if (a->Q * a->nh * a->ch <= 4096)") == 2 and "<= 9216" in hd and "#define HD_MAXH 8" in hd          # W <= 4096
    assert "heads_fwd_kernel<12, 3>" in hd and "heads_bwd_kernel<12, 3>" in hd


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_every_case_passes_the_library_contract(entry, monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    n = 0
    for c in sc.cases(entry):
        if "affine_fwd[grid cap]" in c.targets:
            continue
        b = sc.build(c)
        sc.run(dev, b, b.bufs)
        n += 1
    abi_dryrun.assert_contracts_hold(calls, at_least=n)


def test_invalid_argument_sets_are_refused(monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    t = torch.zeros(1 << 16)
    for name, call in sc.refusals(dev, t):
        del calls[:]
        call()
        assert calls and calls[0][1] == abi_dryrun.WS_ERR_INVALID, (name, calls)


def test_fma_rounds_once():
    """_fma32 against exact rational arithmetic on values built to land on fp32 ties of the float64 sum."""
    from fractions import Fraction
    g = torch.Generator().manual_seed(5)
    z, s = torch.randn(4000, generator=g).double().float().double(), torch.randn(4000, generator=g).float().double()
    p = (z * s)
    mid = (p.float().double() + torch.nextafter(p.float(), torch.full((4000,), math.inf)).double()) / 2          # an fp32 tie
    bb = ((mid - p).float().double())          # b that brings z s + b next to the tie
    got = sc._fma32(z, s, bb)
    for i in range(0, 4000, 7):
        exact = Fraction(float(z[i])) * Fraction(float(s[i])) + Fraction(float(bb[i]))
        lo = torch.tensor(float(exact)).float()
        cands = [lo, torch.nextafter(lo, torch.tensor(math.inf)), torch.nextafter(lo, torch.tensor(-math.inf))]
        best = min(cands, key=lambda c: abs(Fraction(float(c)) - exact))
        ties = sorted(abs(Fraction(float(c)) - exact) for c in cands)
        if ties[0] != ties[1]:
            assert float(got[i]) == float(best), i
