"""CPU checks of the 3 x 3 halo-convolution contract suite (tests/conv3x3_contract.py): nothing here needs a GPU.

  - the float64 gather reference agrees with tests/emu_dev.py (F.conv2d / conv2d_weight) on every case, within the bounds:
    forward, per-split slabs, reduced sums, the two composed cases; ref_conv3x3_pack decodes to the source weights within
    2^-17 |w| and equals dev.conv3x3_pack on CPU tensors bit for bit;
  - the emulation fed large finite garbage in everything the contract does not read gives the same bits;
  - every generated case passes the WS_REQUIRE rules of the real libwesep_hip.so (tests/abi_dryrun.py), and deliberately invalid
    argument sets come back WS_ERR_INVALID with the promised message;
  - pair coverage, instantiation coverage and the size limits hold;
  - SENSITIVITY: the checker refuses every planted defect below.  The last column is the Frobenius ratio rel() that
    tests/test_dpccn_gpu.py holds below 2e-5 (on the sum of the slabs for the weight gradient, on the decoded hi + lo for the
    pack): the defects marked MISSED would have passed it (profiles/conv3x3_contract.md has the table of the run)."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import abi_dryrun, emu_dev
from tests import conv3x3_contract as cc
from tests import gemm_contract as gc

GUARD = gc.GUARD
ALL = cc.ENTRIES + (cc.COMPOSED,)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _case(entry, **dims):
    base = {d: v[0] for d, v in gc.DIMS[entry].items()}
    base.update(dims)
    assert gc.violated(entry, base) is None, gc.violated(entry, base)
    return gc.Case(entry, "hand-" + "-".join(str(v) for v in dims.values()), base, gc.PLANNERS[entry](base, 77), 77)


# ------------------------------------------------------------------------------------------------------------
# every case: emulation, garbage, dry run, coverage
# ------------------------------------------------------------------------------------------------------------
def _reduced_ok(b, ref, after):
    """emu_dev.reduce_slabs over the emulated slabs against the summed reference."""
    worst, nsplit = 0.0, b.kw["nsplit"]
    for key, name in b.out_keys.items():
        n = ref[key].idx.numel() // nsplit
        stride = (b.bufs[name].numel() - 2 * GUARD) // nsplit
        out = torch.full((n + 2 * GUARD,), gc.SENT)
        out[GUARD:GUARD + n] = float("nan")
        before = out.clone()
        emu_dev.reduce_slabs(after[name][GUARD:], nsplit, stride, n, out, out_off=GUARD)
        worst = max(worst, gc.check(out, before, gc.reduced(ref[key], nsplit), f"{b.case.name} reduced {key}", GUARD))
    return worst


@pytest.mark.parametrize("entry", ALL)
def test_reference_agrees_with_the_cpu_emulation_on_every_case(entry):
    from wesep_amd import dev
    for c in cc.cases(entry):
        b = cc.build(c)
        ref = cc.reference(b)
        after = cc.emulate(b)
        assert cc.verify(b, ref, cc.perfect(b, ref)) <= 1.0
        if entry == "conv3x3_pack":
            p = cc._pack_kwargs(b.packs[0], after)
            Cin, Cout = p["Cin"], p["Cout"]
            Wl = after["Wpack"][GUARD:GUARD + Cout * 9 * Cin].reshape(Cout, 9 * Cin)           # the emulation's plain rows
            assert torch.equal(Wl.reshape(Cout, 9, Cin), torch.from_numpy(cc.logical_w(p["srcs"], Cin, Cout, p["flip"]))), c.name
            assert torch.equal(dev.conv3x3_pack(Wl, Cin, Cout).view(torch.int16), ref["pack"]), c.name
            dec, w = cc.pack_decode(ref["pack"], Cin, Cout), Wl.reshape(Cout, 9, Cin).double()
            assert bool(((dec - w).abs() <= 2.0 ** -17 * w.abs()).all()), c.name
            assert bool(torch.isfinite(w).all()) and float(w.abs().max()) <= 16 and float(w[w != 0].abs().min()) >= 2.0 ** -20
            continue
        assert cc.verify(b, ref, after) <= 1.0, c.name
        if entry == "conv3x3_wgrad":
            assert _reduced_ok(b, ref, after) <= 1.0, c.name
        assert all(bool(torch.isfinite(r.bound).all()) and bool(torch.isfinite(r.val).all()) for r in ref.values())


@pytest.mark.parametrize("entry", ALL)
def test_the_emulation_selects_garbage_away(entry):
    for c in cc.cases(entry):
        b, bg = cc.build(c), cc.build(c, garbage=True)
        a, ag = cc.emulate(b), cc.emulate(bg)
        if entry == "conv3x3_pack":
            n = b.packs[0]["Cout"] * 9 * b.packs[0]["Cin"]
            assert torch.equal(a["Wpack"][GUARD:GUARD + n], ag["Wpack"][GUARD:GUARD + n]), c.name
            assert torch.equal(cc.reference(b)["pack"], cc.reference(bg)["pack"]), c.name
            continue
        assert torch.equal(cc.output_bits(b, a), cc.output_bits(bg, ag)), c.name


@pytest.mark.parametrize("entry", ALL)
def test_every_case_passes_the_library_contract(entry, monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    n = 0
    for c in cc.cases(entry):
        b = cc.build(c)
        cc.run(dev, b, b.bufs, "cpu")
        n += len(b.packs) + (entry != "conv3x3_pack")
    abi_dryrun.assert_contracts_hold(calls, at_least=n)
    assert len(calls) == n


def _raw(fn, struct, **fields):
    from wesep_amd import _lib as L
    from wesep_amd import dev
    a = struct()
    for k, v in fields.items():
        setattr(a, k, dev._p(v) if isinstance(v, torch.Tensor) else v)
    rc = getattr(L.lib(), fn)(C.byref(a), C.c_void_p(0))
    return rc, L.lib().ws_last_error().decode()


def test_invalid_argument_sets_are_refused_with_the_promised_message():
    from wesep_amd import _lib as L
    t = torch.zeros(1 << 16)
    fwd = dict(X=t, W=t, Y=t, ldx=8, ldw=0, ldy=8, B=1, H=2, Wd=3, Cin=8, Cout=8)
    wg = dict(G=t, X=t, slab=t, bslab=t, ldg=8, ldx=8, slab_stride=8 * 9 * 8, bslab_stride=8, B=1, H=31, Wd=5, Wx=5, sw=1, Cin=8, Nn=8,
              nsplit=2, tiles_per_split=2)
    bad = [
        ("ws_conv3x3", L.Conv3x3Args, dict(fwd, Cin=6), "Cin % 4, Cout % 4, Cout <= 1024 (got 6, 8)"),
        ("ws_conv3x3", L.Conv3x3Args, dict(fwd, Cout=1028, ldy=1028), "Cout <= 1024 (got 8, 1028)"),
        ("ws_conv3x3", L.Conv3x3Args, dict(fwd, ldy=4), "ldy >= Cout"),
        ("ws_conv3x3_wgrad", L.Conv3x3WgradArgs, dict(wg, Wx=9), "image width 9, gradient width 5 = (Wx - 1) / sw + 1"),
        ("ws_conv3x3_wgrad", L.Conv3x3WgradArgs, dict(wg, sw=3, Wx=13), "stride 3 along w (1 or 2)"),
        ("ws_conv3x3_wgrad", L.Conv3x3WgradArgs, dict(wg, nsplit=1, tiles_per_split=3), "1 splits of 3 tiles do not cover the 4 tiles"),
        ("ws_conv3x3_wgrad", L.Conv3x3WgradArgs, dict(wg, slab_stride=8 * 9 * 8 - 4), "slab strides"),
        ("ws_conv3x3_wgrad", L.Conv3x3WgradArgs, dict(wg, bslab_stride=4), "slab strides"),
    ]
    for fn, struct, fields, msg in bad:
        rc, text = _raw(fn, struct, **fields)
        assert rc == abi_dryrun.WS_ERR_INVALID and msg in text, (fn, rc, text, msg)
    for fields in (fwd, wg):           # the two base sets themselves reach the launch
        rc, text = _raw("ws_conv3x3" if fields is fwd else "ws_conv3x3_wgrad", L.Conv3x3Args if fields is fwd else L.Conv3x3WgradArgs,
                        **fields)
        assert rc not in (0, abi_dryrun.WS_ERR_INVALID), (rc, text)
    for nsrc, col_off, cols, msg in ((1, 4, 8, "source 0 does not lie inside the 8 columns"), (1, -4, 8, "does not lie inside"),
                                     (6, 0, 8, "ws_conv3x3_pack: bad arguments"), (1, 0, 8, None)):
        a = L.Conv3x3PackArgs()
        for k in range(5):
            a.src[k].w, a.src[k].s_row, a.src[k].s_col, a.src[k].s_tap = C.c_void_p(t.data_ptr()), 72, 9, 1
            a.src[k].col_off, a.src[k].cols = (col_off, cols) if k == 0 else (0, 1)
        a.out, a.Cin, a.Cout, a.nsrc, a.flip = C.c_void_p(t.data_ptr()), 8, 8, nsrc, 0
        rc = L.lib().ws_conv3x3_pack(C.byref(a), C.c_void_p(0))
        text = L.lib().ws_last_error().decode()
        if msg is None:
            assert rc not in (0, abi_dryrun.WS_ERR_INVALID), (rc, text)
        else:
            assert rc == abi_dryrun.WS_ERR_INVALID and msg in text, (nsrc, col_off, rc, text)


def test_the_wrappers_check_the_column_ranges_and_keep_their_defaults(monkeypatch):
    """dev.conv3x3_wgrad: x_off is checked like g_off; slab_stride / bslab_stride / x_off = 0 pass what the wrapper passed before."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    made = []

    class Recorded(L.Conv3x3WgradArgs):
        def __init__(self):
            super().__init__()
            made.append(self)
    monkeypatch.setattr(L, "Conv3x3WgradArgs", Recorded)
    b = cc.build(_case("conv3x3_wgrad", H=31, Wd=5, Cin=20, Nn=12, bslab=1, ldx="80", x_off="4", strides="padded"))
    kw = b.kwargs(b.bufs)
    dev.conv3x3_wgrad(**kw)
    dev.conv3x3_wgrad(**{k: v for k, v in kw.items() if k not in ("slab_stride", "bslab_stride", "x_off")})
    seen = [(a.X, a.slab_stride, a.bslab_stride) for a in made]
    assert seen[0] == (kw["X"].data_ptr() + 16, 12 * 9 * 20 + 12, 16) and seen[1] == (kw["X"].data_ptr(), 12 * 9 * 20, 12)
    assert len(calls) == 2
    for off in (2, 64):
        with pytest.raises(L.WesepHipError, match="conv3x3_wgrad X"):
            dev.conv3x3_wgrad(**dict(kw, x_off=off))
    with pytest.raises(L.WesepHipError, match="conv3x3_pack_srcs: out holds"):
        dev.conv3x3_pack_srcs([(kw["X"], 0, 72, 9, 1, 0, 8)], 8, 8, out=torch.zeros(16))


@pytest.mark.parametrize("entry", cc.ENTRIES)
def test_every_pair_of_values_occurs_or_is_ruled_out_by_name(entry):
    cs, inv = cc.cases(entry), cc.invalid_pairs(entry)
    assert len(cs) <= gc.MAX_CASES
    covered = set()
    for c in cs:
        assert gc.violated(entry, c.dims) is None
        covered |= gc.pairs_of(entry, c.dims)
    for pr in gc.all_pairs(entry):
        assert (pr in covered) != (pr in inv), pr           # exactly one of the two
    assert not [p for p, why in inv.items() if why.startswith("UNNAMED")]
    again = gc._CACHE.pop(entry)
    assert [c.dims for c in cc.cases(entry)] == [c.dims for c in again[0]], "the case list is not deterministic"


def test_every_instantiation_is_covered():
    """The seven conv3x3_kernel instantiations ws_conv3x3 can pick with no environment override, the four weight-gradient
    kernels, the pack kernel; nothing else is ever named."""
    assert len(cc.C3_INST) == 7 and len(cc.WG3_INST) == 4
    for entry in cc.ENTRIES:
        cs = cc.cases(entry)
        for inst in cc.INST[entry]:
            n = sum(1 for c in cs if inst in c.targets)
            assert n >= gc.MIN_PER_TARGET, (inst, n)
        assert {t for c in cs for t in c.targets} == set(cc.INST[entry])
    assert {t for c in cc.cases(cc.COMPOSED) for t in c.targets} <= set(cc.C3_INST + cc.PK3_INST)
    # the dispatcher mirror against the source text
    src = open(os.path.join(os.path.dirname(__file__), "..", "wesep_amd", "csrc", "conv3x3.hip")).read()
    names = {"conv3x3_kernel<" + m.replace(" ", "") + ">" for m in re.findall(r"c3_launch<([^>]*)>\(a, s\)", src)}
    assert names == set(cc.C3_INST), names
    names = {m.replace(" ", "") for m in re.findall(r"hipLaunchKernelGGL\((conv3x3_wgrad\w*<\d>)", src)}
    assert names == set(cc.WG3_INST), names
    assert "const bool wide = a->Wd >= 100;" in src and "a->Cin > C3_CC" in src and "a->Nn <= 16 && v16" in src


def test_case_sizes_splits_and_operand_mix():
    from wesep_amd import dev
    for c in cc.cases("conv3x3") + cc.cases(cc.COMPOSED):
        assert c.dims["B"] * c.dims["H"] * c.dims["Wd"] <= 25200, c.name
    kinds = {}
    for c in cc.cases("conv3x3_wgrad"):
        d = c.dims
        nt = cc.wgrad_tiles(d["B"], d["H"], d["Wd"])
        assert nt == dev.conv3x3_wgrad_tiles(d["B"], d["H"], d["Wd"])
        ns, tps = cc.wg3_split(d["split"], nt)
        assert ns * tps >= nt
        if d["split"] == "one":
            assert ns == 1
        elif d["split"] == "exact":
            assert tps == 1 and ns == nt
        elif d["split"] == "ragged":
            assert nt % tps != 0 and ns == -(-nt // tps) and ns > 1
        else:
            assert (ns - 2) * tps >= nt                     # at least two trailing splits own no tile
        kinds[d["split"]] = kinds.get(d["split"], 0) + 1
    assert all(kinds[k] >= 5 for k in ("one", "exact", "ragged", "over")), kinds
    for c in cc.cases("conv3x3_pack"):
        b = cc.build(c)
        p = cc._pack_kwargs(b.packs[0], b.bufs)
        cols = sorted((s[5], s[5] + s[6]) for s in p["srcs"])
        assert all(a[1] <= b_[0] for a, b_ in zip(cols, cols[1:])) and cols[0][0] >= 0 and cols[-1][1] <= p["Cin"], c.name   # disjoint
        assert (sum(hi - lo for lo, hi in cols) < p["Cin"]) == (c.dims["cover"] == "gap"), c.name
        for k in range(len(cols)):                          # every source element the gather does not name is NaN
            named = int(torch.isfinite(b.bufs[f"S{k}"]).sum())
            assert named == p["Cout"] * 9 * p["srcs"][k][6], c.name


def test_the_case_list_pins_every_select_the_kernels_rely_on():
    """A select is pinned by a case in which the value it masks is poison (NaN in the plain build), not data that only meets a
    zero weight: the lanes of the last 16- / 32-channel chunk behind Cin and of the last output tile behind Nn have to fall
    on columns outside the range (x_off + Cin < ldx, g_off + Nn < ldg); image borders are poison in every case (the guards
    in front of the first and behind the last image) and a neighbouring image's data where B = 3."""
    def count(entry, fn):
        return sum(1 for c in cc.cases(entry) if fn(c.dims, cc.build(c).kw))
    assert count("conv3x3", lambda d, kw: d["Cin"] % 16 and kw["x_off"] + d["Cin"] < kw["ldx"]) >= 10       # halo_load: c < Cin
    assert count("conv3x3", lambda d, kw: d["B"] == 3 and d["H"] % 32 and d["Wd"] % 8) >= 10                # hh / ww selects, tile ends
    assert count("conv3x3", lambda d, kw: d["Cout"] % 32 and kw["y_off"] + d["Cout"] < kw["ldy"]) >= 10     # the n < Cout store guard
    assert count("conv3x3", lambda d, kw: d["Cout"] in (68, 100, 132)) >= 10                                # three / four / five 32-tiles
    for big in (0, 1):      # both weight-gradient kernels
        pick = lambda d: (d["Nn"] > 16) == bool(big)
        assert count("conv3x3_wgrad", lambda d, kw: pick(d) and d["Cin"] % 32 and kw["x_off"] + d["Cin"] < kw["ldx"]) >= 5   # c < Cin
        assert count("conv3x3_wgrad", lambda d, kw: pick(d) and d["Nn"] % 32 and kw["g_off"] + d["Nn"] < kw["ldg"]) >= 5     # n < nn
        assert count("conv3x3_wgrad", lambda d, kw: pick(d) and d["H"] % 30 and d["Wd"] % 4 and d["B"] == 3) >= 3            # ii / hh / ww
        assert count("conv3x3_wgrad", lambda d, kw: pick(d) and d["split"] == "over") >= 2
        assert count("conv3x3_wgrad", lambda d, kw: pick(d) and d["strides"] == "padded" and d["bslab"]) >= 3
    # and the reference says so: without the c < Cin select these cases come out NaN
    hit = 0
    for c in cc.cases("conv3x3"):
        b = cc.build(c)
        if c.dims["Cin"] % 16 and b.kw["x_off"] + c.dims["Cin"] < b.kw["ldx"]:
            assert bool(torch.isnan(cc.reference(b, defect="no_cin_select")["Y"].val).any()), c.name
            hit += 1
    assert hit >= 10


# ------------------------------------------------------------------------------------------------------------
# planted defects
# ------------------------------------------------------------------------------------------------------------
RESULTS = {}


def _rel_of(b, ref, after, key):
    if b.case.entry == "conv3x3_pack":
        p = b.packs[0]
        n = ref["pack"].numel() // 2
        got = cc.pack_decode(after["Wpack"][GUARD:GUARD + n].contiguous().view(torch.int16), p["Cin"], p["Cout"])
        return rel(got, cc.pack_decode(ref["pack"], p["Cin"], p["Cout"]))
    r = ref[key]
    got, val = after[b.out_keys[key]][r.idx + GUARD].double(), r.val
    if b.case.entry == "conv3x3_wgrad":         # what the existing test compares: the sum of the slabs
        ns = b.kw["nsplit"]
        got, val = got.reshape(ns, -1).sum(0), val.reshape(ns, -1).sum(0)
    return rel(got, val)


def _judge(name, b, ref, after, kind, key="Y"):
    RESULTS[name] = _rel_of(b, ref, after, key)
    with pytest.raises(gc.ContractViolation) as e:
        cc.verify(b, ref, after)
    assert e.value.kind == kind, (name, str(e.value))
    print(f"planted defect '{name}': refused as {kind}; rel() = {RESULTS[name]:.1e}")


def test_checker_refuses_the_planted_forward_defects():
    b = cc.build(_case("conv3x3", H=33, Wd=9, B=3, Cin=20, Cout=36, ldx="80", x_off="4", ldy="160", y_off="4", bias=1, R="alias"))
    ref = cc.reference(b)
    ok = cc.perfect(b, ref)
    assert cc.verify(b, ref, ok) <= 1.0
    for name, defect, kind in (("the c < Cin select missing (NaN meets a zero weight)", "no_cin_select", "nan"),
                               ("tap right of w = Wd - 1 reads pixel (h + 1, 0)", "wrap_w", "bound"),
                               ("tap above h = 0 reads the previous image's last row", "wrap_h", "bound"),
                               ("ky and kx swapped", "kykx", "bound"),
                               ("forward: lo terms dropped", "drop_lo", "bound"),
                               ("bias missing from the last channel quad", "bias_last_quad", "bound"),
                               ("R read with stride Cout instead of ldy", "R_stride", "bound")):
        _judge(name, b, ref, cc.perfect(b, cc.reference(b, defect=defect)), kind)
    bad = {k: v.clone() for k, v in ok.items()}
    bad["Y"][GUARD + 4 + 36] = 0.0
    _judge("a store into the ldy tail", b, ref, bad, "sentinel")
    bad = {k: v.clone() for k, v in ok.items()}
    M = 3 * 33 * 9
    rows = bad["Y"][GUARD:GUARD + M * 160].view(M, 160)
    rows[:, 40:44] = rows[:, 36:40]
    _judge("channel quad n >= Cout of the padded tile stored", b, ref, bad, "sentinel")


def test_checker_refuses_the_planted_weight_gradient_defects():
    dims = dict(H=61, Wd=9, sw="2-Wx-even", B=3, Cin=36, Nn=20, ldg="Nn+4", g_off="4", ldx="Cin+4", x_off="4", bslab=1, strides="padded")
    b = cc.build(_case("conv3x3_wgrad", split="ragged", **dims))
    ref = cc.reference(b)
    ok = cc.perfect(b, ref)
    assert cc.verify(b, ref, ok) <= 1.0 and b.kw["nsplit"] == 3
    for name, defect, key in (("tiles assigned to splits row-fastest", "row_fastest", "slab"),
                              ("a split running one tile past its end", "plus_one", "slab"),
                              ("bslab summed once per input chunk", "bias_per_chunk", "bslab"),
                              ("image column w + kx - 1 under sw = 2", "sw_ignored", "slab"),
                              ("the seam row between two 30-row tiles counted twice", "seam_twice", "slab"),
                              ("weight gradient: lo terms dropped", "drop_lo", "slab")):
        _judge(name, b, ref, cc.perfect(b, cc.reference(b, defect=defect)), "bound", key=key)
    bad = {k: v.clone() for k, v in ok.items()}
    bad["slab"][GUARD + 20 * 9 * 36: GUARD + 20 * 9 * 36 + 4] = 1.0
    _judge("slab rows n >= Nn stored", b, ref, bad, "sentinel", key="slab")
    be = cc.build(_case("conv3x3_wgrad", split="over", **dims))
    refe = cc.reference(be)
    ns = be.kw["nsplit"]
    assert bool(refe["slab"].exact.reshape(ns, -1)[-2:].all()) and not bool(refe["slab"].exact.reshape(ns, -1)[:-2].any())
    bad = cc.perfect(be, refe)
    bad["slab"][GUARD + (ns - 1) * be.kw["slab_stride"]: GUARD + (ns - 1) * be.kw["slab_stride"] + 20 * 9 * 36] = float("nan")
    _judge("an empty split left unwritten", be, refe, bad, "nan", key="slab")
    bad = cc.perfect(be, refe)
    bad["slab"][GUARD + (ns - 1) * be.kw["slab_stride"] + 7] = 1e-30
    _judge("an empty split not exactly zero", be, refe, bad, "exact", key="slab")


def test_checker_refuses_the_planted_pack_defects():
    b = cc.build(_case("conv3x3_pack", Cin=20, Cout=68, nsrc=2, flip=1, layout="padded", cover="gap"))
    ref = cc.reference(b)
    ok = cc.perfect(b, ref)
    assert cc.verify(b, ref, ok) == 0.0
    for name, defect in (("pack: flip ignored", "flip_ignored"), ("pack: hi and lo parts swapped", "swap_parts")):
        _judge(name, b, ref, cc.perfect(b, cc.reference(b, defect=defect)), "exact", key="pack")
    ntp, nch, nfl = cc.pack_geometry(20, 68)
    assert ntp == 4
    bits = ref["pack"].clone().reshape(nch, 9, ntp, 2, 64, 8)
    bits[:, :, 3, 0] = 0x3F80                                         # 1.0 in every hi element of the fourth tile
    _judge("pack: the odd padded tile left non-zero", b, ref, cc.perfect(b, {"pack": bits.reshape(-1)}), "exact", key="pack")
    p = cc._pack_kwargs(b.packs[0], b.bufs)
    covered = torch.zeros(20, dtype=torch.bool)
    for s in p["srcs"]:
        covered[s[5]:s[5] + s[6]] = True
    gap = int((~covered).nonzero()[0])
    bits = ref["pack"].clone().reshape(nch, 9, ntp, 2, 2, 32, 8)      # chunk tap t part half l31 j
    bits[gap // 16, :, :, :, (gap % 16) // 8, :, gap % 8] = 0x7FC0    # what the buffer held
    _judge("pack: an uncovered column left uninitialised", b, ref, cc.perfect(b, {"pack": bits.reshape(-1)}), "exact", key="pack")
    bad = {k: v.clone() for k, v in ok.items()}
    bad["Wpack"][GUARD + nfl] = 0.0
    _judge("pack: a float behind conv3x3_pack_floats written", b, ref, bad, "sentinel", key="pack")


def test_zz_what_the_frobenius_ratio_would_have_missed():
    """rel() < 2e-5 is the bound tests/test_dpccn_gpu.py holds these kernels to."""
    if len(RESULTS) < 20:          # run alone: plant the defects first
        test_checker_refuses_the_planted_forward_defects()
        test_checker_refuses_the_planted_weight_gradient_defects()
        test_checker_refuses_the_planted_pack_defects()
    missed = sorted(k for k, v in RESULTS.items() if v < 2e-5)
    print(f"MISSED by rel() < 2e-5: {len(missed)} of {len(RESULTS)} planted defects:", missed)
    for k in ("a store into the ldy tail", "channel quad n >= Cout of the padded tile stored", "tiles assigned to splits row-fastest",
              "slab rows n >= Nn stored", "pack: the odd padded tile left non-zero"):
        assert k in missed, (k, RESULTS[k])
