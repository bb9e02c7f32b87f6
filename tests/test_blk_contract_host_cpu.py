"""CPU checks of the blocked-layout contract suite (tests/blk_contract.py): nothing here needs a GPU.

  - the index formulas written out from the header (positions, bl_index, BLS / BLH decoding) agree with wesep_amd.dev's
    to_blocked / from_blocked / bl_positions / bls_pack / blh_* helpers;
  - the float64 reference agrees with tests/emu_blk.py (gemm_p2b with steps, gemm_b2p, gemm_tnb per split, pack_w) on
    every case, within the bounds;
  - every generated case passes the WS_REQUIRE rules of the real libwesep_hip.so (tests/abi_dryrun.py), and deliberately
    invalid argument sets come back WS_ERR_INVALID with the promised message -- a16_out with a_fmt 1, 2, 3 among them;
  - pair coverage, instantiation coverage and the size limits hold;
  - every bound constant is shown from both sides: constructed operands reach a stated fraction of it and never exceed
    it, and dropping the lo term lies outside it on the generator's operands;
  - SENSITIVITY: the checker refuses every planted defect below (mutated copies of the perfect output).  The last column is
    the Frobenius ratio rel() over the write set, which tests/test_kernels_gpu.py and tests/test_gates_h2_gpu.py hold
    below 4e-5: the defects marked MISSED would have passed it (profiles/blk_contract.md has the table of the run)."""
import pytest
import torch

from tests import abi_dryrun, emu_blk
from tests import blk_contract as bc
from tests import gemm_contract as gc

U = gc.U


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _case(entry, **dims):
    base = {d: v[0] for d, v in gc.DIMS[entry].items()}
    base.update(dims)
    assert gc.violated(entry, base) is None, gc.violated(entry, base)
    return gc.Case(entry, "hand-" + "-".join(str(v) for v in dims.values()), base, gc.PLANNERS[entry](base, 77), 77)


# ------------------------------------------------------------------------------------------------------------
# formats and index formulas
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["time", "band", "gaps1", "gaps3"])
@pytest.mark.parametrize("nseq,nvalid", [(1, "0"), (33, "0"), (33, "n-1"), (64, "n-31"), (100, "1")])
def test_index_formulas_agree_with_the_dev_helpers(kind, nseq, nvalid):
    from wesep_amd import dev
    sm, P = bc.seq_map(kind, nseq, 3, nvalid)
    pos, valid, _, _ = bc.positions(sm)
    dpos, dvalid = dev.bl_positions(sm, "cpu")
    assert torch.equal(valid.reshape(-1), dvalid) and torch.equal((pos * valid).reshape(-1), dpos)
    assert pos[valid].unique().numel() == int(valid.sum()), "the map is not injective on its valid slots"
    g = torch.Generator().manual_seed(1)
    x = torch.randn(P, 8, generator=g)
    nblk = pos.shape[0]
    xb = dev.to_blocked(x, sm)
    mine = torch.where(valid.unsqueeze(-1), x[pos], torch.zeros(()))
    assert torch.equal(bc.to_bl(mine), xb.reshape(-1))
    assert torch.equal(xb.reshape(-1)[bc.bl_index(nblk, 8)], mine)                       # the formula itself
    assert torch.equal(bc.from_bl(xb, nblk, 8), mine)
    back = dev.from_blocked(xb, sm, P)
    assert torch.equal(back[pos[valid]], x[pos[valid]])
    xs = dev.to_blocked(x, sm, split=True)
    assert torch.equal(bc.bls_encode(xb).view(torch.int32), xs.view(torch.int32))
    assert torch.equal(bc.bls_decode(xs)[0].float(), dev.bls_unpack(xs))
    for pack, unpack, dt in ((dev.blh_f16_pack, dev.blh_f16_unpack, torch.float16), (dev.blh_bf16_pack, dev.blh_bf16_unpack, torch.bfloat16)):
        buf = pack(xb)
        assert torch.equal(bc.from_bl(bc.h2(buf, dt), nblk, 8).float(), bc.from_bl(unpack(buf, nblk, 8), nblk, 8))
        assert torch.equal(bc.h2(buf, dt).reshape(-1)[bc.bl_index(nblk, 8)], mine.to(dt))


def test_pack_reference_holds_the_weights():
    """hi + lo of the unit formula is W' to 2^-17 (bf16) / 2^-22 + the subnormal floor (fp16 of 256 w); the FP8 plane's
    remainders and exponents reconstruct 256 w - hi exactly (they are the operands the codes are rounded from)."""
    for c in bc.cases("pack_w"):
        b = bc.build(c)
        kw = b.kwargs(b.bufs, "cpu")
        N, K = kw["N"], kw["K"]
        w = bc.logical_w(kw["W"], N, K, kw["ldw"], kw["trans"], kw["w_off"]).double()
        assert torch.equal(w.float(), b.W), c.name
        ref = bc.reference(b)["pack"]
        nt, ks = torch.arange(N // 32), torch.arange(K // 16)
        if int(kw["f16"]) == 2:
            hi = ref["hi"].view(torch.float16).double()           # [st][i][nt][lane][j]
            k = (64 * torch.arange(K // 64).view(-1, 1, 1, 1, 1) + 16 * torch.arange(4).view(1, -1, 1, 1, 1) +
                 8 * (torch.arange(64) >> 5).view(1, 1, 1, -1, 1) + torch.arange(8).view(1, 1, 1, 1, -1))
            n = 32 * torch.arange(4).view(1, 1, -1, 1, 1) + (torch.arange(64) & 31).view(1, 1, 1, -1, 1)
            n, k = torch.broadcast_tensors(n, k)
            assert ((hi - 256 * w[n, k]).abs() <= 2.0 ** -11 * (256 * w[n, k]).abs() + 2.0 ** -25).all()
            assert float(ref["rem"].abs().max()) < float(torch.exp2(ref["E"] + 8).max())
            continue
        dt = torch.float16 if kw["f16"] else torch.bfloat16
        u = ref.view(dt).double().reshape(-1, 2, 64, 8)             # [r][part][lane][j]
        r = torch.arange(u.shape[0])
        t, s = (r // (K // 16), r % (K // 16)) if kw["order"] == 0 else (r % (N // 32), r // (N // 32))
        n = (32 * t.view(-1, 1, 1) + (torch.arange(64) & 31).view(1, -1, 1)).expand(-1, 64, 8)
        k = 16 * s.view(-1, 1, 1) + 8 * (torch.arange(64) >> 5).view(1, -1, 1) + torch.arange(8).view(1, 1, -1)
        sc = 256.0 if kw["f16"] else 1.0
        err = (u[:, 0] + u[:, 1] - sc * w[n, k]).abs()
        tol = (2.0 ** -22 if kw["f16"] else 2.0 ** -17) * (sc * w[n, k]).abs() + (2.0 ** -25 if kw["f16"] else 0.0)
        assert (err <= tol).all(), (c.name, float((err / tol.clamp_min(1e-300)).max()))


# ------------------------------------------------------------------------------------------------------------
# every case: emulation, dry run, coverage
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", bc.ENTRIES)
def test_reference_agrees_with_the_cpu_emulation_on_every_case(entry):
    for c in bc.cases(entry):
        b = bc.build(c)
        ref = bc.reference(b)
        after = bc.emulate(b)
        if entry == "pack_w":      # the emulation keeps the logical matrix: it is the W' the reference packs
            kw = b.kwargs(after, "cpu")
            assert torch.equal(emu_blk._PACKS[kw["out"].data_ptr()], bc.logical_w(kw["W"], kw["N"], kw["K"], kw["ldw"], kw["trans"], kw["w_off"]))
            continue
        assert bc.verify(b, ref, after) <= 1.0
        assert bc.verify(b, ref, bc.perfect(b, ref)) <= 1.0
        assert all(bool(torch.isfinite(r.bound).all()) and bool(torch.isfinite(r.val).all()) for r in ref.values() if isinstance(r, gc.Ref))


@pytest.mark.parametrize("entry", ["gemm_p2b", "gemm_b2p"])
def test_the_emulation_selects_garbage_away(entry):
    for c in bc.cases(entry)[::4]:
        b, bg = bc.build(c), bc.build(c, garbage=True)
        a, ag = bc.emulate(b), bc.emulate(bg)
        for n in b.outs:
            if n != "a16_out":
                assert torch.equal(a[n].view(torch.int32), ag[n].view(torch.int32)), (c.name, n)
        assert bc.verify(bg, bc.reference(bg), ag) <= 1.0


@pytest.mark.parametrize("entry", bc.ENTRIES)
def test_every_case_passes_the_library_contract(entry, monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    n = 0
    for c in bc.cases(entry):
        b = bc.build(c)
        bc.run(dev, b, b.bufs, "cpu")
        n += 1 + (b.pack is not None and entry != "pack_w")
    abi_dryrun.assert_contracts_hold(calls, at_least=n)


def test_invalid_argument_sets_are_refused_with_the_promised_message(monkeypatch):
    from wesep_amd import _lib as L
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    p2b = bc.build(_case("gemm_p2b", nseq=33, L=2, N=64))
    b2p = bc.build(_case("gemm_b2p", nseq=33, L=2, K=64, a_fmt=0))
    b2p2 = bc.build(_case("gemm_b2p", nseq=33, L=2, K=64, a_fmt=2))
    tnb = bc.build(_case("gemm_tnb", ta=3, ntile=1, L=3))
    tnb2 = bc.build(_case("gemm_tnb", ta=3, ntile=1, L=3, g_fmt=2))
    pk = bc.build(_case("pack_w", kind="f16f8", N=128, K=64, order=1))
    k1, k2, k22, k3, k32, kp = [x.kwargs(x.bufs) for x in (p2b, b2p, b2p2, tnb, tnb2, pk)]
    spare = torch.zeros(1 << 16)
    word = torch.zeros(1, dtype=torch.int32)
    bad = [
        (dev.gemm_p2b, dict(k1, N=96), "N % 64"),
        (dev.gemm_p2b, dict(k1, lda=130), "lda"),
        (dev.gemm_p2b, dict(k1, K=64), "K must be 128"),
        (dev.gemm_p2b, dict(k1, Wpack=None), "null pointer"),
        (dev.gemm_p2b, dict(k1, N=0, Wpack=None, C_out=None), "null pointer"),
        (dev.gemm_p2b, dict(k1, steps=torch.ones(64, dtype=torch.int32), steps_div=-1), "steps_div"),
        (dev.gemm_b2p, dict(k2, ldc=126), "ldc"),
        (dev.gemm_b2p, dict(k2, K=96), "K % 64"),
        (dev.gemm_b2p, dict(k2, a_fmt=2), "need amax"),
        (dev.gemm_tnb, dict(k3, a0_shift=1), "only A1 can be shifted"),
        (dev.gemm_tnb, dict(k3, a1_cols=128), "128 or 384"),
        (dev.gemm_tnb, dict(k3, nsplit=1, blocks_per_split=2), "bad block split"),
        (dev.gemm_tnb, dict(k3, g_off=2), "G column range"),
        (dev.gemm_tnb, dict(k3, g_fmt=2), "needs amax"),
        (dev.gemm_tnb, dict(k3, a_fmt=1), "a_fmt = 1"),
        (dev.gemm_tnb, dict(k32, a_fmt=1, aslab=spare), "a_fmt = 1"),
        (dev.gemm_tnb, dict(k32, A1=None, a1_cols=0), "built for 384"),
    ]
    for fn, kw, msg in bad:
        del calls[:]
        fn(**kw)
        (what, rc, text), = calls
        assert rc == abi_dryrun.WS_ERR_INVALID and msg in text, (what, rc, text, msg)
    for kind, N, K, order, msg in ((0, 48, 64, 0, "N % 32"), (1, 64, 24, 1, "K % 16"), (0, 64, 64, 2, "order"), (2, 64, 64, 1, "N = 128"),
                                   (2, 128, 96, 1, "K % 64")):
        del calls[:]
        dev.pack_w(kp["W"], N, K, K, spare, order=order, f16=kind)
        (what, rc, text), = calls
        assert rc == abi_dryrun.WS_ERR_INVALID and msg in text, (what, rc, text, msg)
    # a16_out goes with a_fmt 0: the wrapper and the library say the same (the header: "a_fmt 0 only")
    import ctypes as C
    for fmt, kw in ((1, k2), (2, k22), (3, k22)):
        with pytest.raises(L.WesepHipError, match="a16_out goes with a_fmt = 0"):
            dev.gemm_b2p(**dict(kw, a_fmt=fmt, a16_out=spare, amax=word))
        a = L.GemmB2PArgs()
        a.A, a.Wpack, a.C, a.a16_out = dev._p(kw["A"]), dev._p(kw["Wpack"]), dev._p(kw["C_out"]), dev._p(spare)
        a.sm = dev._smc(kw["sm"])
        a.ldc, a.N, a.K, a.a_fmt, a.amax = kw["ldc"], 128, kw["K"], fmt, C.c_void_p(word.data_ptr())
        rc = L.lib().ws_gemm_b2p(C.byref(a), C.c_void_p(0))
        assert rc == abi_dryrun.WS_ERR_INVALID and "a16_out goes with a_fmt 0" in L.lib().ws_last_error().decode(), (fmt, rc)


@pytest.mark.parametrize("entry", bc.ENTRIES)
def test_every_pair_of_values_occurs_or_is_ruled_out_by_name(entry):
    cs, inv = bc.cases(entry), bc.invalid_pairs(entry)
    assert len(cs) <= gc.MAX_CASES
    covered = set()
    for c in cs:
        assert gc.violated(entry, c.dims) is None
        covered |= gc.pairs_of(entry, c.dims)
    for pr in gc.all_pairs(entry):
        assert (pr in covered) != (pr in inv), pr           # exactly one of the two
    assert not [p for p, why in inv.items() if why.startswith("UNNAMED")]
    again = gc._CACHE.pop(entry)
    assert [c.dims for c in bc.cases(entry)] == [c.dims for c in again[0]], "the case list is not deterministic"


def test_every_instantiation_is_covered():
    """Four of gemm_b2p_kernel, two of gemm_p2b_kernel, the ten of ws_gemm_tnb that do not depend on WS_TNB_GDEPTH, the
    three pack kernels; nothing else is ever named."""
    assert len(bc.B2P_INST) == 4 and len(bc.P2B_INST) == 2 and len(bc.TNB_INST) == 10
    for entry in bc.ENTRIES:
        cs = bc.cases(entry)
        for inst in bc.INST[entry]:
            n = sum(1 for c in cs if inst in c.targets)
            assert n >= gc.MIN_PER_TARGET, (inst, n)
        assert {t for c in cs for t in c.targets} == set(bc.INST[entry])
    # the dispatcher mirror against the source text: every launch line of ws_gemm_tnb names one of them or a depth-2 variant
    import os
    import re
    src = open(os.path.join(os.path.dirname(__file__), "..", "wesep_amd", "csrc", "gemm_blk.hip")).read()
    body = src[src.index('extern "C" int ws_gemm_tnb'):]
    names = {m.replace(" ", "") for m in re.findall(r"hipLaunchKernelGGL\(\(?(gemm_tnb\w*<[^>]*>)", body)}
    assert {n for n in names if not re.search(r",2>$", n)} == set(bc.TNB_INST), names
    assert len([n for n in names if re.search(r",2>$", n)]) == 2            # WS_TNB_GDEPTH=2: diagnostics, left out


def test_case_sizes_and_operand_mix():
    for entry in ("gemm_p2b", "gemm_b2p"):
        for c in bc.cases(entry):
            b = bc.build(c)
            sm = b.kw["sm"]
            _, P = bc.seq_map(c.dims["map"], c.dims["nseq"], c.dims["L"], c.dims["nvalid"])
            assert P <= 8192 and b.kw["K"] <= 2048, c.name
            if entry == "gemm_b2p" and c.dims["a_fmt"] >= 2:        # every stored scaled-fp16 value is finite
                assert bool(torch.isfinite(bc.h2(b.bufs["A"][gc.GUARD:-gc.GUARD], torch.float16).float()).all()), c.name
            pos, valid, _, _ = bc.positions(sm)
            if c.dims["map"].startswith("gaps") and int(valid.sum()) > 1:
                assert P > int(valid.sum()), c.name                                # rows no slot maps to exist
    for c in bc.cases("gemm_tnb"):
        b = bc.build(c)
        assert b.kw["g_width"] <= 2048 and b.kw["nblk"] * 32 <= 8192
        if c.dims["g_fmt"] == 2:
            assert bool(torch.isfinite(bc.h2(b.bufs["G"][gc.GUARD:-gc.GUARD], torch.float16).float().nan_to_num(0.0)).all())
            if c.dims["a_fmt"] == 0 and c.dims["f16env"] == "unset":       # the fp16 instruction's precondition
                assert float(bc.bls_decode(b.bufs["A0"][gc.GUARD:-gc.GUARD])[0].nan_to_num(0.0).abs().max()) < 1023
    a = gc.draw(gc.gen(3), 400, 128)
    assert float(a.abs().max()) > 500 and float((a == 0).float().mean()) > 0.02 and bool((a < 0).any())
    kinds = {c.dims["split"]: bc.tnb_split(c.dims["split"], c.dims["ntile"] * c.dims["L"], c.dims["g_geom"][2] // 128)
             + (c.dims["ntile"] * c.dims["L"],) for c in bc.cases("gemm_tnb") if c.dims["ntile"] * c.dims["L"] >= 6}
    assert kinds["one"][0] == 1
    assert kinds["exact"][0] > 1 and kinds["exact"][0] * kinds["exact"][1] == kinds["exact"][2]
    assert kinds["partial"][2] % kinds["partial"][1] != 0
    assert (kinds["empty"][0] - 1) * kinds["empty"][1] >= kinds["empty"][2]         # the last split owns no block


# ------------------------------------------------------------------------------------------------------------
# the bound constants, from both sides
# ------------------------------------------------------------------------------------------------------------
def _worst_pairs():
    """fp32 numbers just below the midpoint between two bf16 neighbours (lo = 2^-8 hi, nearly), in any binade position."""
    g = torch.Generator().manual_seed(0)
    base = 1 + 2.0 ** -8 - 2.0 ** -17 * torch.rand(4000, generator=g, dtype=torch.float64)
    a = (base * (1 + torch.randint(0, 127, (4000,), generator=g) / 128.0)).float()
    return a, a.flip(0), g


def test_split_constants_lie_between_half_of_and_the_stated_bound():
    a, w, g = _worst_pairs()
    x = torch.cat([a, gc.draw(g, 200, 200).reshape(-1)])
    y = x.flip(0)
    for xs, ys, lo_frac in ((a, w, True), (x, y, False)):
        xh, xl = bc.split_bf16(xs)
        yh, yl = bc.split_bf16(ys)
        xh, xl, yh, yl = [t.double() for t in (xh, xl, yh, yl)]
        # b2p a_fmt 0 / tnb g_fmt 0: A is the STORED pair xh + xl; against a weight split from fp32 (b2p) or another pair (tnb)
        stored = xh + xl
        got = xh * yh + xl * yh + xh * yl
        e_b2p = (got - stored * ys.double()).abs() / (stored * ys.double()).abs().clamp_min(1e-300)
        e_tnb = (got - stored * (yh + yl)).abs() / (stored * (yh + yl)).abs().clamp_min(1e-300)
        # b2p a_fmt 1: bf16 A, hi / lo weights
        e_b1 = (xh * (yh + yl) - xh * ys.double()).abs() / (xh * ys.double()).abs().clamp_min(1e-300)
        assert float(e_b2p.max()) <= 1.5 * 2.0 ** -16 and float(e_tnb.max()) <= 2.0 ** -16 and float(e_b1.max()) <= 2.0 ** -17
        if lo_frac:
            assert float(e_b2p.max()) > 0.6 * 1.5 * 2.0 ** -16, float(e_b2p.max()) / (1.5 * 2.0 ** -16)
            assert float(e_tnb.max()) > 0.9 * 2.0 ** -16, float(e_tnb.max()) * 2.0 ** 16
    # the weight's own 2^-17: a remainder just below half an ulp of lo
    wv = (1 + 2.0 ** -8 + 2.0 ** -17 * (1 - 2.0 ** -6 * torch.rand(2000, generator=g, dtype=torch.float64))).float()
    h, l = bc.split_bf16(wv)
    r = (wv.double() - h.double() - l.double()).abs() / wv.double()
    assert 0.45 * 2.0 ** -17 < float(r.max()) <= 2.0 ** -17, float(r.max()) * 2.0 ** 17


def test_fp16_pack_constant_and_floor():
    """256 w = hi + lo to 2^-22, and to 2^-25 absolute where the remainder is an fp16 subnormal.  Reached to one half: the
    remainder is at most half an ulp of hi, which puts it one binade lower than the derivation assumes -- the arithmetic
    gives 2^-23; the stated constant is kept."""
    g = torch.Generator().manual_seed(2)
    w = ((1 + 2.0 ** -11 + 2.0 ** -23) * torch.exp2(torch.randint(-6, 7, (4000,), generator=g).double()) / 256).float()
    w = torch.cat([w, gc.draw(g, 100, 100).reshape(-1) * 0.01, 1e-4 * torch.randn(4000, generator=g)])
    hi, rem, lo = bc.split_f16(w)
    err = (256 * w.double() - hi.double() - lo.double()).abs()
    bound = 2.0 ** -22 * (256 * w.double()).abs() + 2.0 ** -25
    assert (err <= bound).all()
    assert float((err[:4000] / (256 * w[:4000].double())).max()) > 0.49 * 2.0 ** -22
    sub = rem.abs() < 2.0 ** -14
    assert bool(sub.any()) and float(err[sub].max()) > 0.4 * 2.0 ** -25
    assert float((256 * w.double() - hi.double()).abs().max()) > 2.0 ** -12 * float((256 * w[:4000].double()).min())    # lo matters


def test_e4m3_rounding_constants():
    """|q(x) - x| <= 2^-4 |x| for e4m3 normals (reached), <= 2^-10 below 2^-6 (reached): the constants of the a_fmt 3 bound."""
    g = torch.Generator().manual_seed(4)
    x = torch.cat([torch.exp2(8 * torch.rand(20000, generator=g) - 6) * (1 + 1 / 16 - 1e-3), torch.rand(20000, generator=g) * 2.0 ** -6])
    x = x[x < 240]
    q = x.to(torch.float8_e4m3fn).float()
    err = (q - x).abs().double()
    n = x >= 2.0 ** -6
    assert (err[n] <= 2.0 ** -4 * x[n].double()).all() and float((err[n] / x[n]).max()) > 0.9 * 2.0 ** -4 / (1 + 1 / 16)
    assert (err[~n] <= 2.0 ** -10).all() and float(err[~n].max()) > 0.9 * 2.0 ** -10


def test_fp16_lift_truncation_floor():
    """tnb g_fmt 2 on the fp16 instruction: a bf16 term t times 2^6, converted with round-toward-zero, is exact while
    2^-14 <= |64 t| <= 65504 and loses < 2^-30 below (reached to 90 %)."""
    g = torch.Generator().manual_seed(6)
    t = (torch.randn(20000, generator=g) * torch.exp2(-30 * torch.rand(20000, generator=g))).bfloat16().double()
    lifted = t * 64
    f = torch.where(lifted.abs() >= 2.0 ** -14, lifted, torch.trunc(lifted * 2.0 ** 24) * 2.0 ** -24)     # fp16 RTZ of an 8-bit number
    assert bool((f.float().half().double() == f).all())             # what comes out is an fp16 number
    err = (f / 64 - t).abs()
    assert float(err.max()) < 2.0 ** -30 and float(err.max()) > 0.9 * 2.0 ** -30
    assert float(bc.split_bf16(torch.tensor([1020.0]))[0] * 64) <= 65504 < float(bc.split_bf16(torch.tensor([1022.0]))[0] * 64)


def _ratio(b, ref, after):
    try:
        return bc.verify(b, ref, after)
    except gc.ContractViolation as e:
        return e


@pytest.mark.parametrize("a_fmt", [0, 1, 2, 3])
def test_dropping_the_lo_term_of_the_weights_lies_outside_the_b2p_bound(a_fmt):
    b = bc.build(_case("gemm_b2p", nseq=65, L=3, K=512, a_fmt=a_fmt, bias=1))
    ref = bc.reference(b)
    wrong = bc.ref_gemm_b2p(W=b.W, drop_lo=True, **b.kwargs(b.bufs, "cpu"))
    e = _ratio(b, ref, bc.perfect(b, wrong))
    assert isinstance(e, gc.ContractViolation) and e.kind == "bound", e


@pytest.mark.parametrize("dims", [dict(g_fmt=0, ta=1), dict(g_fmt=0, ta=3), dict(g_fmt=1, ta=3), dict(g_fmt=2, ta=3),
                                  dict(g_fmt=2, ta=3, f16env="0")])
def test_dropping_the_lo_terms_lies_outside_the_tnb_bound(dims):
    b = bc.build(_case("gemm_tnb", ntile=2, L=3, **dims))
    ref = bc.reference(b)
    wrong = bc.ref_gemm_tnb(f16env=b.f16env, drop_lo=True, **b.kwargs(b.bufs, "cpu"))
    e = _ratio(b, ref, bc.perfect(b, wrong))
    assert isinstance(e, gc.ContractViolation) and e.kind == "bound", e


def test_dropping_the_lo_term_lies_outside_the_p2b_bound():
    b = bc.build(_case("gemm_p2b", nseq=65, L=3, N=192, bias=1))
    ref = bc.reference(b)
    t = {k: v.clone() for k, v in b.bufs.items()}
    t["A"] = t["A"].bfloat16().float()
    e = _ratio(b, ref, bc.perfect(b, bc.reference(b, t)))
    assert isinstance(e, gc.ContractViolation) and e.kind == "bound", e


# ------------------------------------------------------------------------------------------------------------
# planted defects
# ------------------------------------------------------------------------------------------------------------
RESULTS = {}


def _judge(name, b, ref, after, kind, key="C"):
    r = ref[key]
    name_ = b.out_keys[key]
    k = b.kinds[name_]
    if k in ("f32", "bls"):
        got = after[name_][r.idx + b.base(name_)]
        got = bc.bls_decode(got)[0] if k == "bls" else got
        RESULTS[name] = rel(got, r.val)
    with pytest.raises(gc.ContractViolation) as e:
        bc.verify(b, ref, after)
    assert e.value.kind == kind, (name, str(e.value))
    print(f"planted defect '{name}': refused as {kind}; rel() = {RESULTS.get(name, float('nan')):.1e}")


def test_checker_refuses_the_planted_p2b_defects():
    b = bc.build(_case("gemm_p2b", nseq=65, L=7, map="band", nvalid="n-31", N=192, bias=1, A_bl=1, A_bl16=1, amax="zero",
                       steps="mixed", steps_div=1))
    ref = bc.reference(b)
    ok = bc.perfect(b, ref)
    assert bc.verify(b, ref, ok) <= 1.0
    pos, valid, seq, step = bc.positions(b.kw["sm"])
    live = valid & (step < b.bufs["steps"][seq].long())
    N, base = 192, b.base("C")
    idx = bc.bl_index(pos.shape[0], N)
    bias = b.bufs["P"][gc.GUARD:gc.GUARD + N]

    bad = {k: v.clone() for k, v in ok.items()}
    blk, slot = [int(v) for v in (~valid).nonzero()[0]]
    bad["C"][base + idx[blk, slot]] = bias
    _judge("bias in a padded slot of C", b, ref, bad, "exact")

    t = {k: v.clone() for k, v in b.bufs.items()}
    t["steps"] = (t["steps"] - 1).clamp_min(1)
    _judge("steps off by one", b, ref, bc.perfect(b, bc.reference(b, t)), "bound")

    t = {k: v.clone() for k, v in b.bufs.items()}
    bad = {k: v.clone() for k, v in ok.items()}
    raw = (torch.arange(pos.shape[0]) // 7 * 32).view(-1, 1) + torch.arange(32).view(1, -1)      # the slot's own sequence index
    blk, slot = [int(v) for v in ((raw >= b.kw["sm"].nvalid) & (raw < b.kw["sm"].nseq)).nonzero()[0]]
    src = int(live.reshape(-1).nonzero()[0])
    bad["C"][base + idx[blk, slot]] = ok["C"][base + idx.reshape(-1, N)[src]]
    _judge("nvalid ignored (a sequence >= nvalid written)", b, ref, bad, "exact")

    bad = {k: v.clone() for k, v in ok.items()}
    bad["amax"][16] = 0x3A800000          # 2^-10: far below max |C|
    _judge("amax too small", b, ref, bad, "amax")
    bad = {k: v.clone() for k, v in ok.items()}
    bad["amax"][16] = bc._fbits(1.5 * ref["amax"][1])
    _judge("amax including a padded slot", b, ref, bad, "amax")

    bad = {k: v.clone() for k, v in ok.items()}
    bad["A_bl"][gc.GUARD + pos.shape[0] * 32 * 128 + 5] = 0.0
    _judge("one sentinel word overwritten behind nblk", b, ref, bad, "sentinel")

    bad = {k: v.clone() for k, v in ok.items()}
    j = int(live.reshape(-1).nonzero()[3])
    w = bad["A_bl"][gc.GUARD + bc.bl_index(pos.shape[0], 128).reshape(-1, 128)[j]]
    bad["A_bl"][gc.GUARD + bc.bl_index(pos.shape[0], 128).reshape(-1, 128)[j]] = (w.view(torch.int32) & -65536).view(torch.float32)
    _judge("A_bl written as bf16 hi only", b, ref, bad, "exact", key="A_bl")

    b2 = bc.build(_case("gemm_p2b", nseq=33, L=2, N=64, amax="above"))
    ref2 = bc.reference(b2)
    bad = bc.perfect(b2, ref2)
    bad["amax"][16] = bc._fbits(0.5 * (ref2["amax"][0] + ref2["amax"][1]))
    _judge("amax overwritten instead of maxed", b2, ref2, bad, "amax")

    b3 = bc.build(_case("gemm_p2b", nseq=33, L=2, N=64, amax="zero", run_if=0))
    ref3 = bc.reference(b3)
    assert ref3 == {}
    bad = {k: v.clone() for k, v in b3.bufs.items()}
    bad["amax"][16] = 1
    with pytest.raises(gc.ContractViolation):
        bc.verify(b3, ref3, bad)


def test_checker_refuses_the_planted_b2p_defects():
    b = bc.build(_case("gemm_b2p", nseq=65, L=3, map="gaps3", nvalid="n-1", K=128, a_fmt=0, a16_out=1, ldc=132))
    ref = bc.reference(b)
    ok = bc.perfect(b, ref)
    assert bc.verify(b, ref, ok) <= 1.0
    bad = {k: v.clone() for k, v in ok.items()}
    cells = b.bufs["A"][gc.GUARD:gc.GUARD + ref["a16_out"].idx.numel()]
    hi_only = (cells.view(torch.int32) & -65536).view(torch.float32).half()
    assert not torch.equal(hi_only.view(torch.int16), ref["a16_out:bits"])
    bad["a16_out"].view(torch.int16)[2 * gc.GUARD: 2 * gc.GUARD + hi_only.numel()] = hi_only.view(torch.int16)
    _judge("a16_out written as fp16(hi)", b, ref, bad, "exact", key="a16_out")
    bad = {k: v.clone() for k, v in ok.items()}
    bad["C"][gc.GUARD + 128] = 0.0            # the ldc - N tail of the first row
    _judge("ldc tail overwritten", b, ref, bad, "sentinel")
    pos, valid, seq, _ = bc.positions(b.kw["sm"])
    bad = {k: v.clone() for k, v in ok.items()}
    row = int(pos[valid].max()) + 1           # where sequence nvalid's first row would be is beyond: use an unmapped hole row
    hole = sorted(set(range(int(pos[valid].max()))) - set(pos[valid].tolist()))[0]
    bad["C"][gc.GUARD + hole * 132: gc.GUARD + hole * 132 + 128] = 1.0
    _judge("a row no slot maps to written", b, ref, bad, "sentinel")
    del row
    b2 = bc.build(_case("gemm_b2p", nseq=65, L=3, K=128, a_fmt=2))
    ref2 = bc.reference(b2)
    wrong = ref2["C"]._replace(val=0.5 * ref2["C"].val)
    _judge("the scale undone with 2 S", b2, ref2, bc.perfect(b2, {"C": wrong}), "bound")
    for fmt in range(4):
        bf = bc.build(_case("gemm_b2p", nseq=65, L=3, K=512, a_fmt=fmt, bias=1))
        wrong = bc.ref_gemm_b2p(W=bf.W, drop_lo=True, **bf.kwargs(bf.bufs, "cpu"))
        _judge(f"b2p a_fmt {fmt}: lo term of the weights dropped", bf, bc.reference(bf), bc.perfect(bf, wrong), "bound")


def test_checker_refuses_the_planted_tnb_defects():
    b = bc.build(_case("gemm_tnb", ta=3, ntile=2, L=3, a1_shift=1, split="partial", bslab=1, aslab=1, g_geom=(512, 256, 256)))
    ref = bc.reference(b)
    kw = b.kwargs(b.bufs, "cpu")
    assert bc.verify(b, ref, bc.perfect(b, ref)) <= 1.0
    for name, defect in (("shift read unshifted instead of zeroed at a tile's last step", "unmasked"),
                         ("shift reading the neighbouring tile's block", "neighbour"),
                         ("split boundary off by one block", "split")):
        _judge(name, b, ref, bc.perfect(b, bc.ref_gemm_tnb(defect=defect, **kw)), "bound", key="slab")
    bm = bc.build(_case("gemm_tnb", ta=3, ntile=2, L=3, a1_shift=-1, split="partial"))
    _judge("shift -1 not zeroed at a tile's first step", bm, bc.reference(bm),
           bc.perfect(bm, bc.ref_gemm_tnb(defect="neighbour", **bm.kwargs(bm.bufs, "cpu"))), "bound", key="slab")
    _judge("g_off ignored", b, ref, bc.perfect(b, bc.ref_gemm_tnb(**dict(kw, g_off=0))), "nan", key="slab")
    be = bc.build(_case("gemm_tnb", ta=1, ntile=2, L=3, split="empty"))
    refe = bc.reference(be)
    bad = bc.perfect(be, refe)
    n = refe["slab"].idx.numel() // be.kw["nsplit"]
    bad["slab"][gc.GUARD + (be.kw["nsplit"] - 1) * n: gc.GUARD + be.kw["nsplit"] * n] = float("nan")
    _judge("empty split left unwritten", be, refe, bad, "nan", key="slab")
    bad = bc.perfect(be, refe)
    bad["slab"][gc.GUARD + be.kw["nsplit"] * n + 3] = 0.0
    _judge("slab behind nsplit written", be, refe, bad, "sentinel", key="slab")
    for dims in (dict(g_fmt=0), dict(g_fmt=1), dict(g_fmt=2), dict(g_fmt=2, f16env="0")):
        bf = bc.build(_case("gemm_tnb", ta=3, ntile=2, L=3, **dims))
        wrong = bc.ref_gemm_tnb(f16env=bf.f16env, drop_lo=True, **bf.kwargs(bf.bufs, "cpu"))
        _judge(f"tnb {dims}: lo terms dropped", bf, bc.reference(bf), bc.perfect(bf, wrong), "bound", key="slab")


def test_zz_what_the_frobenius_ratio_would_have_missed():
    """rel() < 4e-5 is the bound the suite held these kernels to so far."""
    if len(RESULTS) < 15:          # run alone: plant the defects first
        test_checker_refuses_the_planted_p2b_defects()
        test_checker_refuses_the_planted_b2p_defects()
        test_checker_refuses_the_planted_tnb_defects()
    missed = sorted(k for k, v in RESULTS.items() if v < 4e-5)
    print("MISSED by rel() < 4e-5:", missed)
    for k in ("bias in a padded slot of C", "one sentinel word overwritten behind nblk", "ldc tail overwritten",
              "slab behind nsplit written", "a row no slot maps to written"):
        assert k in missed, (k, RESULTS[k])
