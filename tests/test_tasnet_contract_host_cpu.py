"""CPU checks of the Conv-TasNet / SpEx+ contract suite (tests/tasnet_contract.py): nothing here needs a GPU.

  - the generator: every legal pair of dimension values is in a case, every pair left out names its rule, every dispatch
    target of INST is reached by MIN_PER_TARGET cases (the three geometries above 64 KB of LDS exactly once each), the listed
    seam values are all there, two calls give the same list;
  - SECOND OPINION: the float64 reference equals torch's own operators to 1e-12 relative on every case -- F.prelu, F.conv1d
    (groups = C, dilated, "same" and causal padding), F.conv_transpose1d, F.batch_norm (training mode, running statistics),
    F.max_pool1d, F.cross_entropy, each with its autograd for the backward entries;
  - perfect(b, ref) passes the checker, and correct fp32 arithmetic stays inside the bounds: every output of every case
    emulated in float32 with its sums sequential and pairwise; the worst err / bound per entry is printed;
  - SENSITIVITY: every planted defect of tasnet_contract.DEFECTS is refused on at least one case of its entry, by the
    reference alone (this is what fixes the suite's size condition, CAP);
  - every case passes the argument checks of the real libwesep_hip.so (tests/abi_dryrun.py), and the argument sets the
    library refuses come back WS_ERR_INVALID."""
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

from tests import abi_dryrun
from tests import gemm_contract as gc
from tests import tasnet_contract as tc

F64 = torch.float64
MAX_CASES_PER_ENTRY = 80


def _close(a, b, what, floor=0.0):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    tol = 1e-12 * max(float(b.abs().max()) if b.numel() else 0.0, floor, 1e-300)
    assert a.shape == b.shape and float((a - b).abs().max() if b.numel() else 0.0) <= tol, (what, float((a - b).abs().max()), tol)


@pytest.mark.parametrize("entry", tc.ENTRIES)
def test_generator_covers_pairs_and_targets(entry):
    cs = tc.cases(entry)
    assert len(cs) <= MAX_CASES_PER_ENTRY, len(cs)
    assert [c.name for c in cs] == [c.name for c in tc.cases(entry)]
    inv = tc.invalid_pairs(entry)
    assert not [w for w in inv.values() if w.startswith("UNNAMED")], inv
    covered = set()
    for c in cs:
        covered |= tc.pairs_of(entry, c.dims)
    missing = [p for p in tc.all_pairs(entry) if p not in covered and p not in inv]
    assert not missing, missing[:5]
    for d, vals in tc.DIMS[entry].items():          # and every single value (entries of one dimension have no pairs)
        assert {c.dims[d] for c in cs} >= set(vals), (d, vals)
    count = {}
    for c in cs:
        assert c.targets == tc._targets(entry, c.dims)
        for t in c.targets:
            count[t] = count.get(t, 0) + 1
    for t in tc.INST[entry]:
        if t in tc.EXACT_COUNT:
            assert count.get(t, 0) == tc.EXACT_COUNT[t], (t, count.get(t, 0))
        else:
            assert count.get(t, 0) >= min(gc.MIN_PER_TARGET, len(cs)), (t, count.get(t, 0))
    assert set(count) <= set(tc.INST[entry]), set(count) - set(tc.INST[entry])


def test_total_case_count_and_seam_values():
    assert sum(len(tc.cases(e)) for e in tc.ENTRIES) <= 800
    big = sorted((c.dims["C"], c.dims["P"]) for c in tc.cases("dwconv_bwd") if tc.dw_lds(c.dims["C"], c.dims["P"]) > 65536)
    assert big == [(768, 7), (776, 5), (776, 7)], big
    assert [tc.dw_lds(*cp) for cp in big] == [73728, 73728, 98304]
    assert [tc.dw_lanes(C) for C in tc.DW["C"]] == [64, 64, 128, 192, 256, 256]
    assert tc.cs_layout(12) == [(3, 85)] and tc.cs_layout(1028) == [(256, 1), (1, 256)]
    assert [tc.bn_lx(C) for C in tc.BN["C"]] == [1, 4, 8, 8, 64, 256]
    dw = tc.cases("dwconv_bwd")
    assert any(c.dims["dil"] * (c.dims["P"] - 1) // 2 >= c.dims["Tp"] and c.dims["P"] > 1 for c in dw)
    assert any(tc.dw_split(c.dims)[0] * tc.dw_split(c.dims)[1] > c.dims["R"] * c.dims["Tp"] + tc.dw_split(c.dims)[1] for c in dw)
    pb = {(c.dims["n4"], c.dims["nslab"]) for c in tc.cases("prelu_bwd")}
    assert {(1, 3), (1, 7), (255, 7), (1030, 1), (1030, 3)} <= pb, sorted(pb)
    assert any(c.dims["rpr"] == "7" and c.dims["M"] == 20 for c in tc.cases("bcast_rows"))
    ce = tc.cases("cross_entropy")
    assert {c.dims["data"] for c in ce} == {"gauss", "+80", "-80", "equal"} and {c.dims["label"] for c in ce} >= {"0", "S-1"}
    for c in ce:
        b = tc.build(c)
        assert all(0 <= v < b.spec["S"] for v in b.spec["label"]), c.name
    for e in ("maxpool3_fwd", "maxpool3_bwd"):          # windows with two and with three equal maxima
        ties = set()
        for c in tc.cases(e):
            b = tc.build(c)
            sp = b.spec
            win = b.views(b.bufs)["x"].reshape(sp["R"], sp["T"], sp["C"])[:, :3 * (sp["T"] // 3)].reshape(sp["R"], -1, 3, sp["C"])
            ties |= set((win == win.max(2, keepdim=True).values).sum(2).unique().tolist())
        assert ties == {1, 2, 3}, (e, ties)
    for e in ("maskmul_fwd", "maskmul_bwd"):
        m = torch.cat([tc.build(c).views(tc.build(c).bufs)["m"] for c in tc.cases(e)])
        assert bool((m == 0).any()) and bool((m < 0).any()) and bool((m > 0).any())
    for c in tc.cases("prelu_fwd") + tc.cases("prelu_bwd"):          # values exactly 0 in the pre-activation
        b = tc.build(c)
        v = tc.compute(c.entry, b.spec, b.views(b.bufs), F64)
        pre = v["x"] if "x" in v else b.views(b.bufs)["pre" if c.entry == "prelu_bwd" else "x"]
        assert bool((pre == 0).any()) or pre.numel() <= 4, c.name
    # suite condition: no sum above CAP leaves without its spike
    for e, key in (("prelu_bwd", "dy"), ("sum_partial", "x")):
        for c in tc.cases(e):
            b = tc.build(c)
            assert (b.spec["n"] > tc.CAP) == bool(b.views(b.bufs)[key].abs().max() > 400), c.name
    for e in ("chan_sums", "dwconv_bwd", "bn_stats", "bn_bwd", "norm_ab", "cross_entropy", "ola_fwd"):
        for c in tc.cases(e):
            d = c.dims
            n = {"chan_sums": d.get("rpg"), "dwconv_bwd": d.get("R", 0) * d.get("Tp", 0), "bn_stats": d.get("M"), "bn_bwd": d.get("M"),
                 "norm_ab": d.get("C"), "cross_entropy": d.get("S"), "ola_fwd": 9}[e]
            assert n <= tc.CAP, c.name


def _xn64(sp, t):
    M, C = sp["R"] * sp["Tp"], sp["C"]
    nst = M // sp["st_div"]
    st = t["stats"][:2 * nst].reshape(nst, 2).double().repeat_interleave(sp["st_div"], 0)
    x = t["x"][:M * C].reshape(M, C).double()
    return (x - st[:, 0:1]) * st[:, 1:2] * t["gamma"][:C].double() + t["beta"][:C].double()


def _dwconv(sp, xn, w, b):
    """F.conv1d on [R, C, T']: "same" padding, or the causal Conv1DBlock (padding dil (P - 1) on both sides, the tail cut)."""
    R, Tp, C, P, dil = sp["R"], sp["Tp"], sp["C"], sp["P"], sp["dil"]
    xi = xn.reshape(R, Tp, C).permute(0, 2, 1)
    pad = dil * (P - 1) if sp["causal"] else dil * (P - 1) // 2
    y = F.conv1d(xi, w.reshape(C, 1, P), b, dilation=dil, padding=pad, groups=C)[:, :, :Tp]
    return y.permute(0, 2, 1).reshape(R * Tp, C)


def _second_opinion(b):
    e, sp = b.case.entry, b.spec
    t = b.views(b.bufs)
    v = tc.compute(e, sp, t, F64)
    if e == "prelu_fwd":
        rows, C = sp["rows"], sp["C"]
        pre = t["x"][:rows * C].reshape(rows, C).double()
        if sp["rb"]:
            pre = pre + t["rb"].reshape(-1, C).double().repeat_interleave(sp["rpr"], 0)[:rows]
            _close(v["x"], pre, "pre")
        _close(v["y"], F.prelu(pre, t["a"].double()), "prelu")
    elif e == "prelu_bwd":
        pre, a = t["pre"].double().requires_grad_(True), t["a"].double().requires_grad_(True)
        dx, da = torch.autograd.grad((F.prelu(pre, a) * t["dy"].double()).sum(), (pre, a))
        _close(v["dx"], dx, "prelu'")
        _close(v["slab"].sum(0), da, "d slope", float((t["dy"].double() * t["pre"].double()).abs().max()))
        _close(v["da"], da, "d slope", float((t["dy"].double() * t["pre"].double()).abs().max()))
    elif e in ("dwconv_fwd", "dwconv_bwd"):
        C, P, M = sp["C"], sp["P"], sp["R"] * sp["Tp"]
        xn = _xn64(sp, t).requires_grad_(True)
        w = t["w"].reshape(C, P).double().requires_grad_(True)
        bb = (t["b"].double() if e == "dwconv_fwd" else torch.zeros(C, dtype=F64)).requires_grad_(True)
        y = _dwconv(sp, xn, w, bb)
        if e == "dwconv_fwd":
            _close(v["y"], y, "conv1d")
        else:
            dxn, dw, db = torch.autograd.grad((y * t["dy"].reshape(M, C).double()).sum(), (xn, w, bb))
            _close(v["dxn"], dxn, "conv1d' x")
            fl = float((t["dy"].double().abs().max() * xn.detach().abs().max()))
            _close(v["dw"], dw, "conv1d' w", fl * 8)
            _close(v["db"], db, "conv1d' b", fl)
            _close(v["slab"].sum(0).reshape(P + 1, C)[:P].t(), dw, "slab", fl * 8)
    elif e == "chan_sums":
        C, rpg, ng = sp["C"], sp["rpg"], sp["ng"]
        g = t["g"].reshape(ng, rpg, C).double()
        xh = torch.zeros_like(g)
        if sp["mode"] != "g":
            xh = t["x"].reshape(ng * rpg, C).double()
            if sp["mode"] == "gxs":
                st = t["stats"].reshape(-1, 2).double().repeat_interleave(sp["st_div"], 0)
                xh = (xh - st[:, 0:1]) * st[:, 1:2]
            xh = xh.reshape(ng, rpg, C)
        want = torch.stack([g.sum(1), torch.einsum("grc,grc->gc", g, xh)], 1)
        _close(v["slab"].sum(0), want, "sums", float((g.abs() * (1 + xh.abs())).max()) * 8)
        _close(v["sums"], want, "sums", float((g.abs() * (1 + xh.abs())).max()) * 8)
    elif e == "norm_ab":
        C, ng = sp["C"], sp["ng"]
        _close(v["ab"], torch.einsum("gkc,c->gk", t["sums"].reshape(ng, 2, C).double(), t["gamma"].double()) / sp["npg"], "ab")
    elif e == "norm_bwd_apply":
        rows, C, sd = sp["rows"], sp["C"], sp["st_div"]
        st, ab = (t[k].reshape(-1, 2).double().repeat_interleave(sd, 0) for k in ("stats", "ab"))
        xh = (t["x"].reshape(rows, C).double() - st[:, 0:1]) * st[:, 1:2]
        want = st[:, 1:2] * (t["dxn"].reshape(rows, C).double() * t["gamma"].double() - ab[:, 0:1] - xh * ab[:, 1:2])
        _close(v["dx"], want + (t["res"].reshape(rows, C).double() if sp["res"] else 0), "dx")
    elif e in ("maskmul_fwd", "maskmul_bwd"):
        rows, N, ldw, off = sp["rows"], sp["N"], sp["ldw"], sp["w_off"]
        w = t["w"].reshape(rows, ldw)[:, off:off + N].double().requires_grad_(True)
        m = t["m"].reshape(rows, N).double()
        if e == "maskmul_fwd":
            _close(v["s"], w * m, "s")
        else:
            pre = torch.where(m > 0, m, -torch.ones_like(m)).requires_grad_(True)          # a pre-activation whose ReLU is max(m, 0)
            ds = t["ds"].reshape(rows, N).double()
            dm = torch.autograd.grad((w * torch.relu(pre) * ds).sum(), pre)[0]
            _close(v["dm"], dm, "dm")
            _close(v["dw"], ds * m, "dw")
    elif e == "relu_mask":
        _close(v["d"], t["d"].double() * (t["y"] > 0), "relu'")
    elif e in ("ola_fwd", "ola_bwd"):
        R, Tp, L, hop, Tout = sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"]
        fr = (t["frames"].double() if e == "ola_fwd" else torch.zeros(R * Tp * L, dtype=F64)).requires_grad_(True)
        est = F.conv_transpose1d(fr.reshape(R, Tp, L).transpose(1, 2), torch.eye(L, dtype=F64).unsqueeze(1), stride=hop)[:, 0]
        if e == "ola_fwd":
            _close(v["est"], est[:, :Tout] + (t["bias"].double() if sp["bias"] else 0), "conv_transpose1d")
        else:
            full = est.shape[1]
            dest = torch.zeros(R, max(full, Tout), dtype=F64)
            dest[:, :Tout] = t["dest"].reshape(R, Tout).double()
            _close(v["dframes"], torch.autograd.grad((est * dest[:, :full]).sum(), fr)[0], "conv_transpose1d'")
    elif e == "sum_partial":
        _close(v["tot"], t["x"].double().sum(), "sum", float(t["x"].abs().max()) * 8)
        _close(v["slab"].sum(), t["x"].double().sum(), "sum", float(t["x"].abs().max()) * 8)
    elif e == "bn_stats":
        M, C = sp["M"], sp["C"]
        x = t["x"].reshape(M, C).double()
        eps, mom = float(tc._f32(tc.BN_EPS)), float(tc._f32(tc.BN_MOM))
        rm = t["running_mean"].double().clone() if sp["run"] else torch.zeros(C, dtype=F64)
        rv = t["running_var"].double().clone() if sp["run"] else torch.ones(C, dtype=F64)
        y = F.batch_norm(x, rm, rv, training=True, momentum=mom, eps=eps)
        _close(v["stats"][0], x.mean(0), "mean")
        _close(v["stats"][1], 1 / torch.sqrt(x.var(0, unbiased=False) + eps), "rstd")
        _close((x - v["stats"][0]) * v["stats"][1], y, "batch_norm")
        if sp["run"]:
            _close(v["running_mean"], rm, "running_mean")
            _close(v["running_var"], rv, "running_var")
    elif e == "bn_prelu_fwd":
        M, C = sp["M"], sp["C"]
        x = t["x"].reshape(M, C).double()
        st = t["stats"].reshape(2, C).double()
        eps = 1e-5
        u = F.batch_norm(x, st[0], 1 / st[1] ** 2 - eps, t["gamma"].double(), t["beta"].double(), training=False, eps=eps)
        if sp["res"]:
            u = u + t["res"].reshape(M, C).double()
        fl = float(((x - st[0]) * st[1] * t["gamma"].double()).abs().max()) * 1e2          # 1 / rstd^2 - eps + eps cancels
        _close(v["u"], u, "batch_norm", fl)
        _close(v["y"], F.prelu(v["u"], t["a"].double()), "prelu")
    elif e == "bn_bwd":
        M, C = sp["M"], sp["C"]
        x = t["x"].reshape(M, C).double().requires_grad_(True)
        gm = t["gamma"].double().requires_grad_(True)
        bt = torch.zeros(C, dtype=F64, requires_grad=True)
        eps = 1e-5
        xd = x.detach()
        exact = torch.stack([xd.mean(0), 1 / torch.sqrt(xd.var(0, unbiased=False) + eps)])
        v = tc.compute(e, sp, dict(t, stats=exact.reshape(-1)), F64)          # at the float64 statistics autograd sees
        y = F.batch_norm(x, None, None, gm, bt, training=True, eps=eps)
        dx, dg, db = torch.autograd.grad((y * t["du"].reshape(M, C).double()).sum(), (x, gm, bt))
        fl = float(t["du"].abs().max() * (1 + ((xd - exact[0]) * exact[1]).abs().max())) * 8
        _close(v["sums"][0], db, "dbeta", fl)
        _close(v["sums"][1], dg, "dgamma", fl)
        _close(v["slab"].sum(0), torch.cat([db, dg]), "slab", fl)
        _close(v["dx"], dx, "batch_norm'", fl * float((t["gamma"].double() * exact[1]).abs().max()))
    elif e in ("maxpool3_fwd", "maxpool3_bwd"):
        R, T, C = sp["R"], sp["T"], sp["C"]
        x = t["x"].reshape(R, T, C).double().requires_grad_(True)
        y = F.max_pool1d(x.permute(0, 2, 1), 3).permute(0, 2, 1)
        if e == "maxpool3_fwd":
            _close(v["y"], y, "max_pool1d")
        else:
            _close(v["dx"], torch.autograd.grad((y * t["dy"].reshape(y.shape).double()).sum(), x)[0], "max_pool1d'")
    elif e == "bcast_rows":
        M, C = sp["M"], sp["C"]
        _close(v["out"], t["src"].reshape(-1, C).double().repeat_interleave(sp["rpr"], 0)[:M] * float(tc._f32(sp["scale"])), "bcast")
    elif e == "cross_entropy":
        R, S = sp["R"], sp["S"]
        z = t["logits"].reshape(R, S).double().requires_grad_(True)
        loss = F.cross_entropy(z, torch.tensor(sp["label"]))
        _close(v["loss"], loss, "cross_entropy", float(z.detach().abs().max()))
        _close(v["dlogits"], torch.autograd.grad(loss, z)[0], "cross_entropy'", 1.0 / R)
    else:
        raise AssertionError(e)


@pytest.mark.parametrize("entry", tc.ENTRIES)
def test_reference_equals_torch_float64_and_perfect_outputs_pass(entry):
    for c in tc.cases(entry) + ([tc.plain_case(entry)] if entry in tc.PLAIN else []):
        b = tc.build(c)
        _second_opinion(b)
        ref = tc.reference(b)
        assert set(ref) == set(k for k in b.alias) | set(n for n in b.outs if n not in b.alias.values()) | set(b.extras), c.name
        assert tc.verify(b, ref, *tc.perfect(b, ref)) <= 1.0, c.name


@pytest.mark.parametrize("entry", tc.ENTRIES)
def test_fp32_emulation_stays_inside_the_bounds(entry):
    worst = (0.0, "")
    for c in tc.cases(entry):
        b = tc.build(c)
        ref = tc.reference(b)
        for order in tc.ORDERS:
            r = tc.verify(b, ref, *tc.emulate(b, ref, order), what=f"{entry} {c.name} [{order}]")
            if r > worst[0]:
                worst = (r, f"{c.name} [{order}]")
    print(f"{entry}: worst err / bound of the fp32 emulation {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0


@pytest.mark.parametrize("entry,defect", [(e, d) for e, ds in tc.DEFECTS.items() for d in ds])
def test_planted_defect_is_refused(entry, defect):
    caught = []
    for c in tc.cases(entry):
        b = tc.build(c)
        ref = tc.reference(b)
        try:
            with warnings.catch_warnings():          # numpy's overflow warning of cross_entropy without its max is the defect showing
                warnings.simplefilter("ignore")
                tc.verify(b, ref, *tc.emulate(b, ref, "seq", defect))
        except tc.ContractViolation as v:
            caught.append((c.name, v.kind))
    print(f"{entry} {defect}: refused on {len(caught)} of {len(tc.cases(entry))} cases")
    assert caught, f"{entry}: the planted defect {defect} passes every case"


def test_every_entry_has_a_planted_defect():
    assert set(tc.DEFECTS) == set(tc.ENTRIES)


def test_unwritten_and_overwritten_outputs_are_refused():
    b = tc.build(tc.cases("dwconv_fwd")[0])
    ref = tc.reference(b)
    good, extra = tc.perfect(b, ref)
    for kind, edit in (("nan", lambda t: t.__setitem__(int(b.start["y"]), float("nan"))), ("sentinel", lambda t: t.__setitem__(3, 0.0))):
        bad = {k: v.clone() for k, v in good.items()}
        edit(bad["y"])
        with pytest.raises(tc.ContractViolation) as ei:
            tc.verify(b, ref, bad, extra)
        assert ei.value.kind == kind
    c1 = next(c for c in tc.cases("maskmul_bwd") if c.dims["ld_dw"] == "3N")
    b = tc.build(c1)
    ref = tc.reference(b)
    bad, extra = tc.perfect(b, ref)
    bad["dw"][b.start["dw"]] = 0.0          # column 0 of row 0: outside [N, 2N)
    with pytest.raises(tc.ContractViolation) as ei:
        tc.verify(b, ref, bad, extra)
    assert ei.value.kind == "sentinel"
    c2 = next(c for c in tc.cases("chan_sums") if "chan_sums[empty split]" in c.targets)
    b = tc.build(c2)
    ref = tc.reference(b)
    good, extra = tc.perfect(b, ref)
    extra = dict(extra, slab=extra["slab"].clone())
    extra["slab"][-1] = 1e-30          # a split that owns no row is an exact zero
    with pytest.raises(tc.ContractViolation) as ei:
        tc.verify(b, ref, good, extra)
    assert ei.value.kind == "exact"


def test_dispatch_mirrors_agree_with_the_source_text():
    src = open(os.path.join(os.path.dirname(__file__), "..", "wesep_amd", "csrc", "tasnet.hip")).read()
    assert "const int nq = min(256, c4n - cz);" in src and "const int nrl = 256 / nq;" in src          # cs_layout
    assert "const int per = (rows_per_group + nsplit - 1) / nsplit;" in src
    assert "while (lx < (C >> 2)) lx <<= 1;" in src and "return lx > 256 ? 256 : lx;" in src          # bn_lx
    assert "const int threads = C / 4 >= 256 ? 256 : ((C / 4 + 63) / 64) * 64;" in src          # dw_lanes
    assert "(size_t)(DW_RY - 1) * (P + 1) * threads * sizeof(f32x4)" in src and "#define DW_RY 4" in src          # dw_lds
    assert "for (int k = y; k < nsplit; k += 4)" in src          # bn_final_kernel's fold over 4 lanes
    assert "for (int j = threadIdx.x; j < S; j += 256)" in src          # ce_kernel's stride
    assert src.count("i < n4; i += (long long)gridDim.x * 256") == 1 and "i < n; i += (long long)gridDim.x * 256" in src
    assert "hipFuncAttributeMaxDynamicSharedMemorySize" in src


@pytest.mark.parametrize("entry", tc.ENTRIES)
def test_every_case_passes_the_library_contract(entry, monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    n = 0
    for c in tc.cases(entry) + ([tc.plain_case(entry)] if entry in tc.PLAIN else []):
        b = tc.build(c)
        tc.run(dev, b, b.bufs, plain=c.name.startswith("plain"))
        n += 1
    abi_dryrun.assert_contracts_hold(calls, at_least=n)


def test_invalid_argument_sets_are_refused(monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    t = torch.zeros(1 << 16)
    for name, call in tc.refusals(dev, t):
        del calls[:]
        call()
        assert calls and calls[0][1] == abi_dryrun.WS_ERR_INVALID, (name, calls)
