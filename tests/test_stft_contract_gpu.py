"""Contract sweep of the STFT / iSTFT / overlap-add kernels on the GPU (tests/stft_contract.py): every generated case goes
through wesep_amd.dev -> libwesep_hip.so (ws_stft_bandsplit, ws_stft_bandsplit_len, ws_mask_istft_frames, ws_istft_ola,
ws_istft_ola_len, ws_mask_istft_bwd, ws_ola_norm_len, ws_ola_fwd, ws_ola_bwd) inside guarded allocations and is held
against the float64 index arithmetic that restates include/wesep_hip.h:
  - every element of a write set inside its bound (stft_contract's docstring derives them), exact zeros where the contract
    says zero (tail frames, samples from lengths[r] on, ola_bwd past Tout), no NaN left in a write set (it starts as NaN);
  - every other word of every output allocation bit-identical to its sentinel;
  - a second launch into fresh buffers gives the same bits;
  - 3e30 instead of the NaN poison in everything the contract does not read -- guards, samples from lengths[r] on, frames
    from 1 + lengths[r] / hop on -- leaves the outputs unchanged to the bit.
Composed on the device outputs: the round trip stft -> mask (unit) -> frames -> overlap-add, every stage judged at the
device output of the one before, and the reconstruction of the input inside the propagated bounds; the valid frames of a
ragged row bit for bit those of the row alone; <mask_istft_bwd(u), v> against the float64 directional derivative of
<istft(mask m + h v), u>.  Length tables with entries outside (256, T]; the WS_REQUIRE refusals.  The last test writes the
case counts and the worst err / bound per kernel and branch to stft_contract.json in $WESEP_TEST_OUT (default: the system's
temporary directory); profiles/stft_contract.md is where the figures of a run are recorded.  No kernel is broken to show a
catch: tests/test_stft_contract_host_cpu.py plants the defects into reference outputs."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

from tests import gemm_contract as gc
from tests import stft_contract as sc

pytestmark = pytest.mark.gpu

WORST = {}     # kernel / branch -> [worst err / bound, cases, the case that gave it]
G = gc.GUARD


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _note(case, ratio, targets=None):
    for t in targets or case.targets:
        w = WORST.setdefault(t, [0.0, 0, ""])
        if ratio > w[0]:
            w[0], w[2] = ratio, f"{case.entry} {case.name}"
        w[1] += 1


def _launch(b, d, entry=None, lens="spec"):
    """One launch into fresh device buffers; returns every allocation (CPU)."""
    from wesep_amd import dev
    t = {k: v.to(d) for k, v in b.bufs.items()}
    sc.run(dev, b, t, d, entry, lens)
    torch.cuda.synchronize()
    return {n: (v.cpu() if n in b.outs else b.bufs[n]) for n, v in t.items()}


def _run(case):
    d = _cuda()
    b = sc.build(case)
    ref = sc.reference(b)
    after = _launch(b, d)
    worst = sc.verify(b, ref, after)
    after2 = _launch(b, d)
    assert torch.equal(sc.output_bits(b, after), sc.output_bits(b, after2)), f"{case.name}: two launches differ"
    bg = sc.build(case, garbage=True)
    afterg = _launch(bg, d)
    assert torch.equal(sc.output_bits(b, after), sc.output_bits(bg, afterg)), f"{case.name}: garbage outside the contract reached the output"
    print(f"{case.entry} {case.name}: worst err / bound {worst:.3f}")
    _note(case, worst)


@pytest.mark.parametrize("case", sc.cases("stft_bandsplit"), ids=lambda c: c.name)
def test_stft_bandsplit_contract(case):
    _run(case)


@pytest.mark.parametrize("case", sc.cases("mask_istft_frames"), ids=lambda c: c.name)
def test_mask_istft_frames_contract(case):
    _run(case)


@pytest.mark.parametrize("case", sc.cases("istft_ola"), ids=lambda c: c.name)
def test_istft_ola_contract(case):
    _run(case)


@pytest.mark.parametrize("case", sc.cases("mask_istft_bwd"), ids=lambda c: c.name)
def test_mask_istft_bwd_contract(case):
    _run(case)


@pytest.mark.parametrize("case", sc.cases("ola_norm_len"), ids=lambda c: c.name)
def test_ola_norm_len_contract(case):
    _run(case)


@pytest.mark.parametrize("case", sc.cases("ola_fwd"), ids=lambda c: c.name)
def test_ola_fwd_contract(case):
    _run(case)


@pytest.mark.parametrize("case", sc.cases("ola_bwd"), ids=lambda c: c.name)
def test_ola_bwd_contract(case):
    _run(case)


def _stage(case, entry, sp, ins, out, n, d):
    """One stage of a chain: `entry` over the natural arrays `ins`, judged against the reference evaluated at exactly these
    inputs.  Returns (worst ratio, the output as float32 numpy, its Ref)."""
    b = sc.SBuilt(sc.Case(entry, f"{case.name} {entry}", case.dims, (), case.seed))
    b.spec = dict(sp)
    for k, a in ins.items():
        sc._input(b, k, a, sc.NAN)
    sc._output(b, out, n)
    ref = sc.reference(b, entry=entry)
    after = _launch(b, d, entry)
    return sc.verify(b, ref, after), after[out][G:G + n].numpy().copy(), ref[out]


def _unit_mask(widths, NF):
    _, _, mc = sc.band_cols(widths)
    m = np.zeros((NF, 4 * sc.NBIN), dtype=np.float32)
    m[:, mc[0]] = 1.0
    m[:, np.concatenate([mc[2], mc[3]])] = 30.0
    return m


@pytest.mark.parametrize("case", sc.cases(sc.COMPOSED), ids=lambda c: c.name)
def test_round_trip_with_a_unit_mask_reconstructs_the_input(case):
    """stft_bandsplit -> mask_istft_frames (o[0] = 1, o[bw] = 0, gates +30) -> istft_ola, every stage fed the DEVICE output
    of the one before and held to the bound at those inputs; the result against the input inside the three bounds carried
    through the float64 pipeline: an error e_k in a spectrum value reaches a frame sample with |coefficient| <= c_k w_n / 512,
    a frame error reaches a sample divided by the envelope; sigmoid(30) misses 1 by 9.4e-14."""
    d = _cuda()
    b = sc.build(case)
    sp = b.spec
    R, T, Tf = sp["R"], sp["T"], sp["Tf"]
    NF = R * Tf
    x = b.bufs["wav"][G:G + R * T].numpy()
    r0, xbs, ref0 = _stage(case, "stft_bandsplit", sp, {"wav": x}, "xbs", NF * 514, d)
    r1, fr, ref1 = _stage(case, "mask_istft_frames", sp, {"xbs": xbs, "m3": _unit_mask(sp["widths"], NF)}, "frames", NF * 512, d)
    r2, wav, ref2 = _stage(case, "istft_ola", sp, {"frames": fr}, "wav", R * T, d)
    re, im, _ = sc.band_cols(sp["widths"])
    b0 = ref0.bound.numpy().reshape(NF, 514)
    e_spec = (sc._CK[None, :] * (b0[:, re] + b0[:, im])).sum(1)[:, None] / sc.NFFT * sc.WIN[None, :]
    e_fr = (ref1.bound.numpy().reshape(NF, 512) + e_spec).reshape(R, Tf, 512)
    tol = np.zeros((R, T))
    for r in range(R):
        y, _, e, _, _ = sc._ola_terms(e_fr[r], T, T // 128)
        tol[r] = y / e
    tol = tol + ref2.bound.numpy().reshape(R, T) + 1e-13 * np.abs(x.reshape(R, T))
    err = np.abs(wav.astype(np.float64).reshape(R, T) - x.astype(np.float64).reshape(R, T))
    r3 = float((err / np.maximum(tol, 1e-300)).max())
    print(f"{case.name}: stft {r0:.3f}, frames {r1:.3f}, ola {r2:.3f}, reconstruction {r3:.3f}")
    _note(case, max(r0, r1, r2, r3), ("composed: round trip",))
    assert max(r0, r1, r2, r3) <= 1.0


@pytest.mark.parametrize("bands", sc.BANDS)
def test_valid_frames_of_a_ragged_row_are_those_of_the_row_alone(bands):
    d = _cuda()
    case = sc.Case("stft_bandsplit", f"ragged-{bands}", dict(T=1000, R=4, bands=bands, lengths="mixed", data="gauss"), (), 9100)
    b = sc.build(case)
    sp = b.spec
    after = _launch(b, d)
    xbs = after["xbs"][G:G + b.sizes["xbs"]].reshape(sp["R"], sp["Tf"], 514)
    assert sorted(sp["lens"]) == [257, 895, 999, 1000]
    for r, Tr in enumerate(sp["lens"]):
        ntf = 1 + Tr // 128
        alone = sc.SBuilt(case)
        alone.spec = dict(sp, R=1, T=Tr, Tf=ntf, lens=None)
        sc._input(alone, "wav", b.bufs["wav"][G + r * sp["T"]:G + r * sp["T"] + Tr].numpy(), sc.NAN)
        sc._output(alone, "xbs", ntf * 514)
        one = _launch(alone, d, "stft_bandsplit")["xbs"][G:G + ntf * 514].reshape(ntf, 514)
        assert torch.equal(xbs[r, :ntf].view(torch.int32), one.view(torch.int32)), f"row {r} (length {Tr})"
        assert not xbs[r, ntf:].any()
    _note(case, 0.0, ("composed: ragged row = row alone",))


@pytest.mark.parametrize("bands", sc.BANDS)
def test_backward_is_the_adjoint_of_the_forward(bands):
    """<mask_istft_bwd(u), v> on the device against the float64 central difference of h -> <istft(mask (m + h v)), u>.  Two
    bounds: sum_i bound_i |v_i| of the backward, and the truncation of the difference, h^2 / 6 * sup |f'''| with f linear in
    o * sigmoid(gate): |d^3/dh^3| <= |dm| (3 |v_o| v_g^2 sup|s''| + |o| |v_g|^3 sup|s'''|), sup|s''| < 0.1, sup|s'''| <= 0.125."""
    d = _cuda()
    case = sc.Case("mask_istft_bwd", f"adjoint-{bands}", dict(T=513, R=2, bands=bands, data="gauss", spec="gauss", mask="gauss"), (), 9200)
    b = sc.build(case)
    sp = b.spec
    ref = sc.reference(b)["dm3"]
    after = _launch(b, d)
    assert sc.verify(b, {"dm3": ref}, after) <= 1.0
    n = b.sizes["dm3"]
    g = after["dm3"][G:G + n].double().numpy()
    v = np.random.default_rng(5).standard_normal(n)
    t = b.views(b.bufs)
    u = t["dwav"][:sp["R"] * sp["T"]]
    h = 1e-3

    def f(m):
        fr = sc.ref_frames(sp, {"xbs": t["xbs"], "m3": m})["frames"].val.numpy()
        wav = sc.ref_ola(sp, {"frames": np.concatenate([fr, np.zeros(G)])})["wav"].val.numpy()
        return float(wav @ u)
    m = t["m3"][:n]
    D = (f(m + h * v) - f(m - h * v)) / (2 * h)
    _, _, mc = sc.band_cols(sp["widths"])
    Xr, Xi, o0, o1, s0, s1 = sc._masked(sp, t, sp["R"] * sp["Tf"])
    val, vm = ref.val.numpy().reshape(-1, 1028), v.reshape(-1, 1028)
    f3 = 0.0
    for c, o, s in ((0, o0, s0), (1, o1, s1)):
        dm = np.abs(val[:, mc[c]]) / s
        f3 += float((dm * (0.3 * np.abs(vm[:, mc[c]]) * vm[:, mc[2 + c]] ** 2 + 0.125 * np.abs(o) * np.abs(vm[:, mc[2 + c]]) ** 3)).sum())
    tol = float(ref.bound.numpy() @ np.abs(v)) + h * h / 6 * f3 + 1e-10 * float(np.abs(val).reshape(-1) @ np.abs(v))
    err = abs(float(g @ v) - D)
    print(f"{case.name}: <bwd(u), v> = {float(g @ v):.9e}, derivative {D:.9e}, err / tolerance {err / tol:.3f}")
    _note(case, err / tol, ("composed: adjoint",))
    assert err <= tol


def _bad_table_case(entry):
    if entry == "ola_norm_len":
        return sc.Case(entry, "bad-table", dict(n=16, T=33, R=5, lengths="full", data="gauss"), (), 9300), 8
    return sc.Case(entry, "bad-table", dict(T=1000, R=5, bands="uneven", lengths="full", data="gauss"), (), 9300), 128


@pytest.mark.parametrize("entry", ["stft_bandsplit", "istft_ola", "ola_norm_len"])
def test_length_entries_outside_the_range_stay_inside_their_rows(entry):
    """Table entries 0, 256 (the scaled 2 * hop) and T + 5 among two valid rows: a finite write set, intact sentinels, and the
    valid rows bit-equal to the run whose other rows are valid too.  (The entries the kernels clamp -- ws_stft_bandsplit_len to
    [257, T], ws_istft_ola_len to [1, T], ws_ola_norm_len to [0, T] -- are inside a full row of valid data here.)"""
    d = _cuda()
    case, hop = _bad_table_case(entry)
    b = sc.build(case)
    T = b.spec["T"]
    valid = [T - 3, 2 * hop + 1]
    good = _launch(b, d, lens=[T, valid[0], T, T, valid[1]])
    bad = _launch(b, d, lens=[0, valid[0], 2 * hop, T + 5, valid[1]])
    out = b.outs[0]
    n = b.sizes[out]
    rows_bad, rows_good = bad[out][G:G + n].reshape(5, -1), good[out][G:G + n].reshape(5, -1)
    assert bool(torch.isfinite(rows_bad).all()), "a NaN of the write set or of a guard survived"
    keep = torch.ones(bad[out].numel(), dtype=torch.bool)
    keep[G:G + n] = False
    assert torch.equal(bad[out].view(torch.int32)[keep], b.bufs[out].view(torch.int32)[keep]), "sentinels changed"
    for r in (1, 4):
        assert torch.equal(rows_bad[r].view(torch.int32), rows_good[r].view(torch.int32)), f"row {r}"
    _note(case, 0.0, (f"{entry}: length table with entries outside the range",))


def test_invalid_argument_sets_are_refused_and_launch_nothing():
    """Every refusal raises, and the output tensor it was handed is untouched afterwards."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    t = torch.full((1 << 16,), gc.SENT, device=d)
    for name, call in sc.refusals(dev, t, d):
        with pytest.raises(L.WesepHipError):
            call()
        torch.cuda.synchronize()
        assert bool((t == gc.SENT).all()), f"{name}: the refused call wrote"


def test_zz_write_worst_ratios():
    """Last in the file: the case count, the worst err / bound and the case that gave it, per kernel and branch ->
    $WESEP_TEST_OUT/stft_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "stft_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1], "worst_case": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
