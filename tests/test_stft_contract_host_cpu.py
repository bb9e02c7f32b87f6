"""CPU checks of the STFT / iSTFT / overlap-add contract suite (tests/stft_contract.py): nothing here needs a GPU.

  - GENERATOR: every valid pair of dimension values is covered, invalid_pairs names a rule for every exclusion, the lists
    are the same on every call, every branch tag has its cases;
  - SECOND OPINION: on every case the float64 index-arithmetic reference equals torch's own operators in float64 to 1e-12
    relative: torch.stft per row (at T = lengths[r] for ragged tables); torch.istft of the masked spectrum for
    mask_istft_frames followed by istft_ola; float64 autograd through torch.istft for mask_istft_bwd; F.fold (torch's
    overlap-add) for istft_ola over free frames, ola_norm_len and ola_fwd, its autograd for ola_bwd;
  - the reference itself, rounded to fp32, passes the checker on every case;
  - EMULATION: correct fp32 arithmetic in the kernels' own order -- the 8 x 8 x 8 decomposition with a float32 twiddle table
    and the float32 window 0.5f - 0.5f * tw[n].x for the FFT entries -- stays inside the bounds on every case; the worst
    err / bound per entry is printed (profiles/stft_contract.md records it);
  - SENSITIVITY: each planted defect is refused on at least one generated case of its entry, counts printed; the one
    defect that is mathematically invisible (Im of Nyquist kept in the inverse) is shown to be an identity instead;
  - the derived constants are what the docstring says;
  - every generated case passes the WS_REQUIRE rules of the real libwesep_hip.so (tests/abi_dryrun.py), the invalid
    argument sets come back WS_ERR_INVALID, and the composed tests of the GPU file run on the emulation."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import gemm_contract as gc
from tests import stft_contract as sc

F64 = torch.float64
HANN = torch.hann_window(sc.NFFT, periodic=True, dtype=F64)


def _close(a, b, what):
    a, b = torch.as_tensor(a).detach().double().reshape(-1), torch.as_tensor(b).detach().double().reshape(-1)
    tol = 1e-12 * max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)


def _generated(entry):
    return [c for c in sc.cases(entry) if not c.name.startswith("x")]


# ---------------------------------------------------------------------------------------------- generator
@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_every_valid_pair_is_covered_and_every_exclusion_is_named(entry):
    cs = _generated(entry)
    covered = set().union(*[gc.pairs_of(entry, c.dims) for c in cs])
    invalid = sc.invalid_pairs(entry)
    for pr in gc.all_pairs(entry):
        assert (pr in covered) != (pr in invalid), pr
    assert not any(w.startswith("UNNAMED") for w in invalid.values()), invalid
    for c in cs:
        assert gc.violated(entry, c.dims) is None
    saved = gc._CACHE.pop(entry)
    try:
        again = gc.cases(entry)
    finally:
        gc._CACHE[entry] = saved
    assert [(c.name, c.dims, c.targets, c.seed) for c in again] == [(c.name, c.dims, c.targets, c.seed) for c in saved[0]]
    print(f"{entry}: {len(cs)} generated cases, {len(invalid)} excluded pairs: {sorted(set(invalid.values()))}")


def test_every_branch_has_its_cases():
    for e in sc.ENTRIES:
        count = {t: 0 for t in sc.INST[e]}
        for c in sc.cases(e):
            for t in c.targets:
                assert t in count, (e, t)
                count[t] += 1
        assert all(v >= 1 for v in count.values()), (e, count)
    nf = {c.dims["R"] * (1 + c.dims["T"] // 128) for c in sc.cases("stft_bandsplit")}
    assert set(sc.NFRAMES) <= nf
    mixed = {c.dims["bands"] for c in sc.cases("stft_bandsplit") if c.dims["lengths"] == "mixed"}
    assert mixed == set(sc.BANDS)
    for c in sc.cases("stft_bandsplit") + sc.cases("istft_ola"):
        ln = sc.length_table(c.dims["lengths"], c.dims["T"], c.dims["R"], c.seed)
        assert ln is None or all(257 <= v <= c.dims["T"] for v in ln), c.name
        if c.dims["lengths"] == "mixed":
            assert {257, c.dims["T"] - 1, c.dims["T"]} <= set(ln) and any(v % 128 == 127 for v in ln), (c.name, ln)
    seen = set()
    for c in sc.cases("ola_norm_len"):
        T, hop = sc.on_T(c.dims), c.dims["n"] // 2
        seen |= {("T%4", T % 4), ("T%hop", min(T % hop, 2) if T % hop != hop - 1 else "hop-1")}
    assert {("T%4", k) for k in range(4)} <= seen and {("T%hop", 0), ("T%hop", 1), ("T%hop", "hop-1")} <= seen


def test_constants_follow_their_derivation():
    assert sc.TABLE_DIFF <= 2.0 ** -25
    assert sc.TW_ERR == math.sqrt(2) * (sc.TABLE_DIFF + gc.U) and sc.D_W == (sc.TABLE_DIFF + gc.U) / 2 + gc.U / 2
    assert sc.EPS_FFT == math.ceil(3 * (4 + math.sqrt(5)) + 2 * (math.sqrt(5) + sc.TW_ERR / gc.U) + 1) * gc.U
    assert sc.D_SIG == 8 * gc.U
    # the envelope's lower bound over every T of the suite and every length the tables hold
    for T in sc.TS:
        for Tr in {T, 257, T - 1, (T - 1) // 128 * 128}:
            if Tr >= 257:
                _, _, e, de, _ = sc._ola_terms(None, T, Tr // 128)
                assert e[:Tr].min() >= sc.E_MIN * (1 - 1e-12) and de[:Tr].max() <= 20 * gc.U
    print({k: round(v, 4) for k, v in sc.CONSTANTS.items()})


# ---------------------------------------------------------------------------------------------- second opinion
def _fold(fr, hop):
    """torch's overlap-add of frames [Tp, L] -> [(Tp - 1) * hop + L]"""
    Tp, L = fr.shape
    return F.fold(fr.t().reshape(1, L, Tp), (1, (Tp - 1) * hop + L), (1, L), stride=(1, hop)).reshape(-1)


def _torch_spectrum(sp, t, m3):
    re, im, mc = (torch.from_numpy(a) for a in sc.band_cols(sp["widths"]))
    NF = sp["R"] * sp["Tf"]
    xbs = torch.from_numpy(t["xbs"][:NF * 514]).reshape(NF, 514)
    mre = m3[:, mc[0]] * torch.sigmoid(m3[:, mc[2]])
    mim = m3[:, mc[1]] * torch.sigmoid(m3[:, mc[3]])
    return torch.complex(xbs[:, re] * mre - xbs[:, im] * mim, xbs[:, re] * mim + xbs[:, im] * mre).reshape(sp["R"], sp["Tf"], 257)


def _torch_istft(Y, T):
    return torch.stack([torch.istft(y.t(), 512, 128, window=HANN, center=True, length=T) for y in Y])


def _second_opinion(case):
    b = sc.build(case)
    sp, e = b.spec, case.entry
    t = b.views(b.bufs)
    ref = sc.reference(b)
    if e == "stft_bandsplit":
        re, im, _ = sc.band_cols(sp["widths"])
        got = ref["xbs"].val.reshape(sp["R"], sp["Tf"], 514)
        for r, Tr in enumerate(sc._lens(sp)):
            X = torch.stft(torch.from_numpy(t["wav"][r * sp["T"]: r * sp["T"] + Tr]), 512, 128, window=HANN, center=True,
                           pad_mode="reflect", return_complex=True).t()
            assert X.shape[0] == 1 + Tr // 128
            _close(torch.cat([got[r, :X.shape[0]][:, re], got[r, :X.shape[0]][:, im]]), torch.cat([X.real, X.imag]), "spectrum")
            assert not got[r, X.shape[0]:].any()
    elif e == "mask_istft_frames":
        NF = sp["R"] * sp["Tf"]
        m3 = torch.from_numpy(t["m3"][:NF * 1028]).reshape(NF, 1028)
        want = _torch_istft(_torch_spectrum(sp, t, m3), sp["T"])
        pad = np.concatenate([ref["frames"].val.numpy(), np.full(sc.GUARD, np.nan)])
        _close(sc.ref_ola(dict(sp, lens=None), {"frames": pad})["wav"].val, want, "frames + ola against torch.istft")
    elif e == "mask_istft_bwd":
        NF = sp["R"] * sp["Tf"]
        m3 = torch.from_numpy(t["m3"][:NF * 1028].copy()).reshape(NF, 1028).requires_grad_(True)
        est = _torch_istft(_torch_spectrum(sp, t, m3), sp["T"])
        (g,) = torch.autograd.grad((est * torch.from_numpy(t["dwav"][:sp["R"] * sp["T"]]).reshape(sp["R"], sp["T"])).sum(), m3)
        _close(ref["dm3"].val, g, "dm3 against autograd through torch.istft")
    elif e == "istft_ola":
        fr = torch.from_numpy(t["frames"][:sp["R"] * sp["Tf"] * 512]).reshape(sp["R"], sp["Tf"], 512)
        got = ref["wav"].val.reshape(sp["R"], sp["T"])
        for r, Tr in enumerate(sc._lens(sp)):
            n = 1 + Tr // 128
            y = _fold(fr[r, :n], 128) / _fold((HANN * HANN).expand(n, 512), 128)
            _close(got[r, :Tr], y[256:256 + Tr], "ola")
            assert not got[r, Tr:].any()
    elif e == "ola_norm_len":
        n, hop = sp["n"], sp["n"] // 2
        fr = torch.from_numpy(t["frames"][:sp["R"] * sp["Tf"] * n]).reshape(sp["R"], sp["Tf"], n)
        w = torch.from_numpy(t["win"][:n])
        got = ref["est"].val.reshape(sp["R"], sp["T"])
        for r, ln in enumerate(sp["lens"]):
            k = 1 + ln // hop
            y = _fold(fr[r, :k], hop) / _fold((w * w).expand(k, n), hop)
            _close(got[r, :ln], y[hop:hop + ln], "ola_norm_len")
            assert not got[r, ln:].any()
    else:
        R, Tp, L, hop, Tout = sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"]
        if e == "ola_fwd":
            fr = torch.from_numpy(t["frames"][:R * Tp * L]).reshape(R, Tp, L)
            want = torch.stack([_fold(f, hop)[:Tout] for f in fr]) + (float(t["bias"][0]) if sp["bias"] else 0.0)
            _close(ref["est"].val, want, "ola_fwd")
        else:
            fr = torch.zeros(R, Tp, L, dtype=F64, requires_grad=True)
            est = torch.stack([_fold(f, hop)[:Tout] for f in fr])
            (g,) = torch.autograd.grad((est * torch.from_numpy(t["dest"][:R * Tout]).reshape(R, Tout)).sum(), fr)
            assert torch.equal(ref["dframes"].val, g.reshape(-1))
    assert sc.verify(b, ref, sc.planted(b, ref)) <= 1.0


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_reference_agrees_with_torch_in_float64_and_passes_its_own_check(entry):
    for c in sc.cases(entry):
        _second_opinion(c)


# ---------------------------------------------------------------------------------------------- emulation
def test_fft_emulation_is_the_kernels_decomposition():
    x = (np.random.default_rng(0).standard_normal((5, 512)) + 1j * np.random.default_rng(1).standard_normal((5, 512)))
    X = sc.fft512_32(x.astype(np.complex64))
    want = np.fft.fft(x.astype(np.complex64).astype(np.complex128), axis=1)
    assert np.abs(X - want).max() < 1e-5 * np.abs(want).max()
    d = np.zeros((1, 512), dtype=np.complex64)
    d[0, 3] = 1
    assert np.abs(sc.fft512_32(d)[0] - sc.TW64[(3 * np.arange(512)) % 512]).max() < 4 * gc.U


@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_correct_fp32_arithmetic_stays_inside_the_bounds(entry):
    worst, dense = (0.0, ""), (0.0, "")
    for c in sc.cases(entry):
        b = sc.build(c)
        r = sc.verify(b, sc.reference(b), sc.emulated(b))
        worst = max(worst, (r, c.name))
        if c.dims.get("data") == "gauss" and c.dims.get("mask", "gauss") == "gauss":
            dense = max(dense, (r, c.name))
    print(f"{entry}: worst err / bound of the fp32 emulation {worst[0]:.3f} ({worst[1]}); on Gaussian data {dense[0]:.4f} ({dense[1]})")
    assert worst[0] <= 1.0


# ---------------------------------------------------------------------------------------------- planted defects
@pytest.mark.parametrize("name,entry,where,what", sc.DEFECTS, ids=[f"{d[1]}-{d[0]}" for d in sc.DEFECTS])
def test_planted_defect_is_refused(name, entry, where, what):
    cs = [c for c in _generated(entry) if where is None or where(c)]
    assert cs, "no case can show the defect"
    refused, kinds = 0, set()
    for c in cs:
        b = sc.build(c)
        ref, bad = sc.reference(b), sc.reference(b, defect=name)
        if name in sc.INVISIBLE:
            for k in ref:
                _close(bad[k].val, ref[k].val, what)
            continue
        try:
            sc.verify(b, ref, sc.planted(b, bad))
        except sc.ContractViolation as ex:
            refused += 1
            kinds.add(ex.kind)
    print(f"{what} [{entry}]: refused on {refused} of {len(cs)} ({', '.join(sorted(kinds))})")
    assert refused >= 1 or name in sc.INVISIBLE


def test_stores_outside_the_write_set_are_refused():
    """A store by an idle wave of the last workgroup (frame-0 values one row behind the last frame) and a single float behind
    the last row: both land in the sentinels."""
    n = 0
    for c in sc.cases("stft_bandsplit"):
        if "stft_bandsplit_kernel[last workgroup with idle waves]" not in c.targets:
            continue
        b = sc.build(c)
        ref = sc.reference(b)
        size = b.sizes["xbs"]
        for lo, hi in ((size, size + 514), (size, size + 1)):
            after = sc.planted(b, ref)
            after["xbs"][sc.GUARD + lo:sc.GUARD + hi] = after["xbs"][sc.GUARD:sc.GUARD + hi - lo]
            with pytest.raises(sc.ContractViolation) as ex:
                sc.verify(b, ref, after)
            assert ex.value.kind == "sentinel"
        n += 1
    assert n >= 8
    print(f"idle-wave store / float behind the last row: sentinel on {n} of {n}")


# ---------------------------------------------------------------------------------------------- the GPU test's own code
def test_gpu_test_bodies_on_the_emulation(monkeypatch):
    """The composed tests of tests/test_stft_contract_gpu.py with the fp32 emulation standing in for the device, so that
    their first run on a GPU tests the kernels and not the test code."""
    from tests import test_stft_contract_gpu as tg

    def launch(b, d, entry=None, lens="spec"):
        keep, case = b.spec.get("lens"), b.case
        if not isinstance(lens, str):       # the kernels' clamps
            b.spec["lens"] = [min(max(v, 257 if case.entry == "stft_bandsplit" else 0), b.spec["T"]) for v in lens]
        if entry:
            b.case = sc.Case(entry, case.name, case.dims, case.targets, case.seed)
        try:
            return sc.emulated(b)
        finally:
            b.spec["lens"], b.case = keep, case
    monkeypatch.setattr(tg, "_launch", launch)
    monkeypatch.setattr(tg, "_cuda", lambda: torch.device("cpu"))
    monkeypatch.setattr(tg, "WORST", {})
    for c in sc.cases(sc.COMPOSED):
        tg.test_round_trip_with_a_unit_mask_reconstructs_the_input(c)
    for bands in sc.BANDS:
        tg.test_valid_frames_of_a_ragged_row_are_those_of_the_row_alone(bands)
        tg.test_backward_is_the_adjoint_of_the_forward(bands)
    for e in ("stft_bandsplit", "istft_ola", "ola_norm_len"):
        tg.test_length_entries_outside_the_range_stay_inside_their_rows(e)
    tg._run(sc.cases("ola_fwd")[0])
    assert all(v[0] <= 1.0 for v in tg.WORST.values()) and len(tg.WORST) >= 8


# ---------------------------------------------------------------------------------------------- the C ABI's own rules
@pytest.mark.parametrize("entry", sc.ENTRIES)
def test_every_generated_case_passes_the_entry_points_own_rules(entry, monkeypatch):
    """Every case reaches the launch of the real libwesep_hip.so (tests/abi_dryrun.py): no WS_REQUIRE refuses it."""
    from tests import abi_dryrun
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    cs = _generated(entry)
    for c in cs:
        b = sc.build(c)
        sc.run(dev, b, b.bufs, "cpu")
    abi_dryrun.assert_contracts_hold(calls, at_least=len(cs))
    assert len(calls) == len(cs)


def test_invalid_argument_sets_are_refused(monkeypatch):
    from tests import abi_dryrun
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    t = torch.zeros(1 << 16)
    for name, call in sc.refusals(dev, t, "cpu"):
        del calls[:]
        call()
        assert calls and calls[0][1] == abi_dryrun.WS_ERR_INVALID, (name, calls)
