"""CPU checks of the normalisation contract suite (tests/norm_contract.py): nothing here needs a GPU.

  - SECOND OPINION: on every generated case the float64 gather reference equals torch's own group norm / layer norm in
    float64 (torch.native_group_norm for the statistics, F.group_norm / F.layer_norm with autograd for dx and the parameter
    sums) to 1e-12 relative; the groups are gathered into dense tensors for the comparison, and the reference is evaluated
    at the float64 statistics (the suite itself feeds it the fp32 rounding the kernels are given);
  - perfect(b, ref) passes the checker on every case;
  - correct fp32 arithmetic stays inside the bounds: every output of every case emulated with its sums taken sequentially,
    pairwise, and over 256 strided lanes + a tree; the worst err / bound per entry is printed;
  - every generated case passes the WS_REQUIRE rules of the real libwesep_hip.so (tests/abi_dryrun.py), and the invalid
    argument sets the header refuses come back WS_ERR_INVALID;
  - SENSITIVITY: each planted defect is refused on at least one generated case of its entry;
  - the generator is deterministic, every instantiation has MIN_PER_TARGET cases, invalid_pairs names a rule for every pair,
    the dispatch mirrors agree with the source text, the suite's size conditions hold."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests import abi_dryrun
from tests import gemm_contract as gc
from tests import norm_contract as nc

F64 = torch.float64
ALL = nc.ENTRIES + (nc.COMPOSED,)


def _close(a, b, what):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    tol = 1e-12 * max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)


def _exact_views(b):
    """The tensors the reference reads, with the statistics (and ab) as float64 instead of their fp32 rounding."""
    t = dict(b.views(b.bufs))
    sp, e = b.spec, b.case.entry
    if e in ("rowln_bwd",):
        fw = nc.ref_rowln_fwd(sp, dict(t, beta=torch.zeros(sp["W"])))["stats"]
        st = fw.S.reshape(-1, 2).clone()
        st[:, 0] = fw.val.reshape(-1, 2)[:, 0]
        t["stats"] = st.reshape(-1)
    elif "stats" in t and e not in ("group_stats", "rowln_fwd", "flat_stats", "flat_stats_len"):
        sr = nc.ref_group_stats(sp, t)["stats"]
        st = sr.S.reshape(-1, 2).clone()
        st[:, 0] = sr.val.reshape(-1, 2)[:, 0]
        t["stats"] = st.reshape(-1)
        if "ab" in t:
            t["ab"] = nc.ref_gn_bwd_reduce(sp, t)["ab"].val
    return t


def _torch_stats(v, eps):
    _, m, r = torch.native_group_norm(v.reshape(1, -1, 1), None, None, 1, v.numel(), 1, 1, eps)
    return m.reshape(()), r.reshape(())


def _xhat(x, eps):
    """GroupNorm(1, C) of one dense group [L, W_g] (F.group_norm refuses a single element: F.layer_norm over all of it)"""
    if x.numel() == 1:
        return F.layer_norm(x, tuple(x.shape), eps=eps)
    return F.group_norm(x.reshape(1, 1, *x.shape), 1, eps=eps).reshape(x.shape)


def _second_opinion_group(b, t, ref):
    sp, e, geo = b.spec, b.case.entry, b.spec["geo"]
    nb, W = geo["nbands"], geo["W"]
    if e == nc.COMPOSED:
        e = "gn_bwd_apply"
    if e == "group_stats":
        for g in range(geo["ngroups"]):
            idx, _, _ = nc.group_index(geo, g, nc._glen_rows(sp, g))
            m, r = _torch_stats(t["x"][idx].double(), sp["eps"])
            _close(ref["stats"].val[2 * g], m, "mean")
            _close(ref["stats"].S[2 * g + 1], r, "rstd")
        return
    gam = [torch.ones(W, dtype=F64, requires_grad=True) for _ in range(nb)]
    bet = [torch.zeros(W, dtype=F64, requires_grad=True) for _ in range(nb)]
    dxs, idxs = [], []
    loss = torch.zeros((), dtype=F64)
    for g in range(geo["ngroups"]):
        idx, band, Wg = nc.group_index(geo, g)
        x = t["x"][idx].double().requires_grad_(True)
        d = t["dxn"][idx].double() + (t["dxn2"][idx].double() if "dxn2" in t else 0)
        xh = _xhat(x, sp["eps"])
        gm = nc._gamma(sp, t, band, Wg) if "gamma" in t else torch.ones(Wg, dtype=F64)
        # y = xhat * (gamma * probe) + beta-probe: d/d(probe) = dgamma / gamma-free sums, d/dx = dx
        y = xh * gm * 1.0
        (dx,) = torch.autograd.grad((y * d).sum(), x, retain_graph=False)
        dxs.append(dx.reshape(-1) + (t["res"][idx].double().reshape(-1) if "res" in t else 0))
        idxs.append(idx.reshape(-1))
        xh2 = _xhat(t["x"][idx].double(), sp["eps"])
        loss = loss + ((xh2 * gam[band][:Wg] + bet[band][:Wg]) * d).sum()
    if "dx" in ref:
        r = ref["dx"]
        assert torch.equal(r.idx, torch.cat(idxs))
        _close(r.val, torch.cat(dxs), "dx")
    grads = [torch.zeros(W, dtype=F64) if v is None else v for v in torch.autograd.grad(loss, gam + bet, allow_unused=True)]
    sums = torch.stack([torch.stack([grads[k], grads[nb + k]]) for k in range(nb)]).reshape(-1)     # [band][dgamma, dbeta][W]
    for key in ("slab", "pslab", "pout"):
        if key in ref:
            _close(ref[key].val, sums, key)
    if e == "gn_bwd_reduce":        # ab through the dx it implies (apply with these means equals autograd's dx)
        t2 = dict(t, ab=ref["ab"].val)
        _close(nc._dx_ref(sp, t2, False).val, torch.cat(dxs), "dx from ab")


def _second_opinion(b):
    sp, e = b.spec, b.case.entry
    t = _exact_views(b)
    ref = nc.REFS["gn_bwd_apply" if e == nc.COMPOSED else e](sp, t)
    if e in nc.GROUP_ENTRIES or e == nc.COMPOSED:
        return _second_opinion_group(b, t, ref)
    if e in ("flat_stats", "flat_stats_len"):
        for g, cnt in enumerate(nc.flat_counts(sp)):
            m, r = _torch_stats(t["x"][g * sp["n"]: g * sp["n"] + cnt].double(), sp["eps"])
            _close(ref["stats"].val[2 * g], m, "mean")
            _close(ref["stats"].S[2 * g + 1], r, "rstd")
        return
    M, W = sp["M"], sp["W"]
    x = t["x"][:M * W].reshape(M, W).double().requires_grad_(True)
    g = t["gamma"][:W].double().requires_grad_(True)
    bt = (t["beta"][:W].double() if "beta" in t else torch.zeros(W, dtype=F64)).requires_grad_(True)
    y = F.layer_norm(x, (W,), g, bt, sp["eps"])
    if e == "rowln_fwd":
        _close(ref["y"].val, y, "y")
        _, m, r = torch.native_layer_norm(x.detach(), (W,), None, None, sp["eps"])
        _close(ref["stats"].val[0::2], m, "mean")
        _close(ref["stats"].S[1::2], r, "rstd")
        return
    dy = t["dy"][:M * W].reshape(M, W).double()
    dx, dg, db = torch.autograd.grad((y * dy).sum(), (x, g, bt))
    _close(ref["dx"].val, dx + (t["res"][:M * W].reshape(M, W).double() if "res" in t else 0), "dx")
    _close(ref["tot"].val, torch.stack([db, dg]), "tot")


@pytest.mark.parametrize("entry", ALL)
def test_reference_equals_torch_float64_and_perfect_outputs_pass(entry):
    for c in nc.cases(entry):
        b = nc.build(c)
        _second_opinion(b)
        ref = nc.reference(b)
        after, extra = nc.perfect(b, ref)
        assert nc.verify(b, ref, after, extra) <= 1.0, c.name
        for r in ref.values():
            assert bool(torch.isfinite(r.bound).all()) and bool(torch.isfinite(r.val).all()), c.name


@pytest.mark.parametrize("entry", nc.ENTRIES)
def test_correct_fp32_arithmetic_stays_inside_the_bounds_in_three_orders(entry):
    worst = {o: (0.0, "") for o in nc.ORDERS}
    for c in nc.cases(entry):
        b = nc.build(c)
        ref = nc.reference(b)
        for o in nc.ORDERS:
            after, extra = nc.emulate(b, o)
            r = nc.verify(b, ref, after, extra)
            if r > worst[o][0]:
                worst[o] = (r, c.name)
    print(f"fp32 emulation, worst err / bound of {entry}: " + ", ".join(f"{o} {v[0]:.3f} ({v[1]})" for o, v in worst.items()))
    assert all(v[0] <= 1.0 for v in worst.values())


@pytest.mark.parametrize("entry", nc.ENTRIES)
def test_garbage_outside_the_contract_changes_no_reference_and_no_emulated_bit(entry):
    for c in nc.cases(entry)[::3]:
        b, bg = nc.build(c), nc.build(c, garbage=True)
        (a, x), (ag, xg) = nc.emulate(b, "pairwise"), nc.emulate(bg, "pairwise")
        assert torch.equal(nc.output_bits(b, a, x), nc.output_bits(bg, ag, xg)), c.name


@pytest.mark.parametrize("entry", nc.ENTRIES)
def test_every_case_passes_the_library_contract(entry, monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    n = 0
    for c in nc.cases(entry):
        b = nc.build(c)
        if entry == "rowln_bwd":        # the wrapper reduces the slabs itself: ws_rowln_grid has to work without a device
            assert dev.L.lib().ws_rowln_grid(b.spec["M"], b.spec["W"]) == nc.rowln_grid(b.spec["M"], b.spec["W"])
        nc.run(dev, b, b.bufs, "cpu")
        n += 2 if entry == "rowln_bwd" else 1
    abi_dryrun.assert_contracts_hold(calls, at_least=n)
    assert len(calls) == n


def test_invalid_argument_sets_are_refused(monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    t = torch.zeros(1 << 16)
    for name, call in nc.refusals(dev, t, "cpu"):
        del calls[:]
        call()
        assert calls and calls[0][1] == abi_dryrun.WS_ERR_INVALID, (name, calls)


def test_flat_stats_keeps_its_chunk_rule_without_an_override(monkeypatch):
    from wesep_amd import dev
    seen = []
    monkeypatch.setattr(dev, "_call", lambda name, *a: seen.append((name, a[4])))
    monkeypatch.setattr(dev, "_chk", lambda *a, **k: None)
    x = torch.zeros(8)
    for ng, n, want in ((1, 4096, 1), (1, 65536, 4), (3, 1 << 22, 170), (600, 1 << 20, 1)):
        dev.flat_stats(x, ng, n, x)
        assert seen[-1] == ("ws_flat_stats", want), (ng, n, seen[-1])
    dev.flat_stats(x, 1, 4096, x, nchunk=65)
    assert seen[-1][1] == 65


# ------------------------------------------------------------------------------------------------------------
# planted defects
# ------------------------------------------------------------------------------------------------------------
def _caught(entry, plant, kinds=("bound", "nan"), only=None):
    """(cases refused, cases tried) of `entry`: a planted defect raises ContractViolation `bound`, or `nan` where it makes the
    kernel read the poison (rows behind glen, a gap between two bands)."""
    n, tried = 0, 0
    for c in nc.cases(entry):
        if only is not None and not only(c):
            continue
        b = nc.build(c)
        ref = nc.reference(b)
        planted = plant(b, ref)
        if planted is None:
            continue
        tried += 1
        try:
            nc.verify(b, ref, *planted)
        except gc.ContractViolation as ex:
            assert ex.kind in kinds, (c.name, str(ex))
            n += 1
    return n, tried


def _by_reference(defect, entry=None):
    return lambda b, ref: nc.perfect(b, nc.reference(b, defect=defect))


DEFECTS = [
    ("one-pass variance in fp32", "group_stats", _by_reference("one_pass"), None),
    ("unbiased variance", "group_stats", _by_reference("unbiased"), None),
    ("n = L * geo.W instead of the band's width", "group_stats", _by_reference("n_geoW"), lambda c: c.dims["W"] == "tab"),
    ("n = L * geo.W in the backward means", "gn_bwd_reduce", _by_reference("n_geoW"), lambda c: c.dims["W"] == "tab"),
    ("glen ignored", "group_stats", _by_reference("glen_ignored"), lambda c: c.dims["glen"] in ("ones", "mixed")),
    ("glen[g] instead of glen[g / glen_div]", "group_stats", _by_reference("glen_g"),
     lambda c: c.dims["glen"] == "mixed" and c.dims["glen_div"] == "K"),
    ("the last quad of a group dropped", "group_stats", _by_reference("drop_last_quad"), None),
    ("band_off[g % gdiv] where gdiv != nbands", "group_stats", _by_reference("off_gdiv"), lambda c: c.dims["geom"] == "bandsplit2"),
    ("band_off[g % gdiv] in the backward", "gn_bwd_reduce", _by_reference("off_gdiv"), lambda c: c.dims["geom"] == "bandsplit2"),
    ("gamma_tab[0] for every band", "gn_bwd_reduce", _by_reference("gamma_tab0"), lambda c: c.dims["gamma"] == "tab"),
    ("ab halves swapped", "gn_bwd_apply", _by_reference("ab_swapped"), None),
    ("res skipped", "gn_bwd_apply", _by_reference("res_skipped"), lambda c: c.dims["res"] == "sep"),
    ("odd rows dropped from the parameter sums (generic)", "gn_param_grad", _by_reference("odd_rows_dropped"), lambda c: c.dims["L"] > 1),
    ("odd rows dropped from the parameter sums (apply_pg)", "gn_bwd_apply_pg", _by_reference("odd_rows_dropped"), lambda c: c.dims["L"] > 1),
    ("odd rows dropped from the parameter sums (fused)", "gn_bwd_fused", _by_reference("odd_rows_dropped"), None),
    ("an empty chunk counted with its stale mean", "flat_stats", _by_reference("stale_empty_chunk"), None),
    ("an empty chunk counted with its stale mean (len)", "flat_stats_len", _by_reference("stale_empty_chunk"), None),
]


@pytest.mark.parametrize("name,entry,plant,only", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_checker_refuses_the_planted_defect(name, entry, plant, only):
    n, tried = _caught(entry, plant, only=only)
    print(f"planted defect '{name}': refused on {n} of {tried} cases of {entry}")
    assert n >= 1 and tried >= 1


def _pout_misses_last_row(b, ref):
    if "pout" not in ref or ref["pslab"].rows.shape[0] < 2:
        return None
    after, extra = nc.perfect(b, ref)
    p, s0 = ref["pslab"], b.start["pslab"]
    after["pslab"][p.rows[-1] + s0] = after["pslab"][p.rows[0] + s0]      # the whole sum is the LAST workgroup's share
    after["pslab"][p.rows[0] + s0] = 0.0
    after["pout"][b.start["pout"]: b.start["pout"] + 256] = 0.0           # ... and pout is the sum of the others
    return after, extra


def _rowln_stops_at_the_grid(b, ref):
    sp = b.spec
    stop = 2048 * (256 // nc.rowln_lpr(sp["W"]))
    if sp["M"] <= stop:
        return None
    after, extra = nc.perfect(b, ref)
    key = "y" if "y" in ref else b.alias.get("dx", "dx")
    s0 = b.start[key]
    after[key][s0 + stop * sp["W"]: s0 + sp["M"] * sp["W"]] = b.bufs[key][s0 + stop * sp["W"]: s0 + sp["M"] * sp["W"]]
    return after, extra


def test_checker_refuses_the_launch_and_row_seam_defects():
    for entry in ("gn_bwd_apply_pg", "gn_bwd_fused"):
        n, tried = _caught(entry, _pout_misses_last_row)
        print(f"planted defect 'the last workgroup's pslab row missing from pout': refused on {n} of {tried} cases of {entry}")
        assert n >= 1 and n == tried
    for entry in ("rowln_fwd", "rowln_bwd"):
        n, tried = _caught(entry, _rowln_stops_at_the_grid, kinds=("nan",))
        print(f"planted defect 'the rowln loop stops at 2048 * RPB rows': refused on {n} of {tried} cases of {entry}")
        assert n == tried == 4
    # a store outside the write set: a gap between two bands, a row tail, the float behind stats
    c = next(c for c in nc.cases("gn_bwd_apply") if c.dims["geom"] == "bandsplit" and not c.dims["alias"])
    b = nc.build(c)
    ref = nc.reference(b)
    after, extra = nc.perfect(b, ref)
    after["dx"][b.start["dx"] + b.spec["geo"]["band_off"][0] + 2] = 0.0     # the float behind band 0 (width 2) of the first row
    with pytest.raises(gc.ContractViolation) as ex:
        nc.verify(b, ref, after, extra)
    assert ex.value.kind == "sentinel"
    c = nc.cases("gn_param_grad")[0]
    b = nc.build(c)
    ref = nc.reference(b)
    after, extra = nc.perfect(b, ref)
    after["slab"][b.start["slab"] + ref["slab"].rows.numel()] = 0.0
    with pytest.raises(gc.ContractViolation) as ex:
        nc.verify(b, ref, after, extra)
    assert ex.value.kind == "sentinel"


# ------------------------------------------------------------------------------------------------------------
# generator
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", nc.ENTRIES)
def test_every_pair_of_values_occurs_or_is_ruled_out_by_name(entry):
    cs, inv = gc.cases(entry), nc.invalid_pairs(entry)
    assert len(cs) <= gc.MAX_CASES
    covered = set()
    for c in cs:
        assert gc.violated(entry, c.dims) is None
        covered |= gc.pairs_of(entry, c.dims)
    for pr in gc.all_pairs(entry):
        assert (pr in covered) != (pr in inv), pr
    names = {r[0] for r in gc.RULES[entry]}
    for pr, why in inv.items():
        assert not why.startswith("UNNAMED") and any(n in why for n in names), (pr, why)
    again = gc._CACHE.pop(entry)
    assert [c.dims for c in gc.cases(entry)] == [c.dims for c in again[0]], "the case list is not deterministic"


def test_every_instantiation_is_covered_and_the_mirrors_match_the_source():
    for entry in nc.ENTRIES:
        cs = nc.cases(entry)
        for inst in nc.INST[entry]:
            n = sum(1 for c in cs if inst in c.targets)
            assert n >= gc.MIN_PER_TARGET, (inst, n)
        assert {t for c in cs for t in c.targets} == set(nc.INST[entry])
    src = open(os.path.join(os.path.dirname(__file__), "..", "wesep_amd", "csrc", "norm.hip")).read()
    assert ("return !g->band_w && !g->band_off && g->W % 4 == 0 && g->rs % 4 == 0 && g->gs1 % 4 == 0 && g->gs2 % 4 == 0;") in src
    assert "if (geo->nbands == 1 && geo->W == 128 && geom_vec4(geo))" in src
    assert "return W > 128 ? 64 : W > 64 ? 32 : W > 32 ? 16 : 8;" in src and "#define ROWLN_GRID_MAX 2048" in src
    assert "v.band = g % geo.nbands;" in src and "(geo.band_off ? geo.band_off[v.band] : 0)" in src


def test_the_suite_conditions_hold():
    """Group sizes (CAP unless a spike is carried), offset data at n <= 1024, aligned vectorised cases, glen inside [1, L],
    the seam cases present, buffers small."""
    for entry in nc.ENTRIES:
        for c in nc.cases(entry):
            b = nc.build(c)
            d, sp = c.dims, b.spec
            spike = d["data"] in nc.SPIKES
            if "geo" in sp:
                geo = sp["geo"]
                big = max(nc.group_index(geo, g)[0].numel() for g in range(geo["ngroups"]))
                assert big <= nc.CAP or spike, c.name
                assert d["data"] != "offset" or big <= 1024, c.name
                if nc.geom_vec4(geo):
                    assert all(s % 4 == 0 for s in b.start.values()), c.name
                if sp.get("glen") is not None:
                    assert all(1 <= v <= geo["L"] for v in sp["glen"]), c.name
            elif "n" in sp:
                assert sp["n"] <= nc.CAP or spike, c.name
            assert sum(v.numel() for v in b.bufs.values()) * 4 <= 48 << 20, c.name
    assert sorted(b_["L"] * b_["W"] // 4 for b_ in nc.EXTRA["group_stats"]) == [255, 256, 257, 513]
    for entry in ("rowln_fwd", "rowln_bwd"):
        big = [c for c in nc.cases(entry) if c.dims["M"] == "grid+1"]
        assert sorted(nc.rowln_lpr(c.dims["W"]) for c in big) == [8, 16, 32, 64]
        for c in big:
            M = nc.rowln_M(c.dims)
            assert M * c.dims["W"] * 4 <= 8 << 20 and nc.rowln_grid(M, c.dims["W"]) == 2048 and c.dims["data"] == "spike-last"
    empty = [c for c in nc.cases("flat_stats") if nc.flat_nchunk(c.dims) > c.dims["n"] // 4]
    assert len(empty) >= 5 and any(nc.flat_nchunk(c.dims) > 64 for c in nc.cases("flat_stats"))
