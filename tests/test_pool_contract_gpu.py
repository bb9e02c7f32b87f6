"""Contract sweep of the speaker pooling and the ragged speaker stage on the GPU (tests/pool_contract.py): every generated case goes
through wesep_amd.dev -> libwesep_hip.so (conv2d.hip: ws_tstp_fwd, ws_astp_fwd / bwd, ws_seg_sums / scale, ws_preemph_pad,
ws_power_spec, ws_log_eps; mhastp.hip: ws_mhastp_pack / fwd / bwd / fwd_split / bwd_split; ragged_spk.hip: the seven *_len entry
points) inside guarded allocations and is held against the float64 index arithmetic that restates include/wesep_hip.h:
  - every element of a write set inside its bound, std inside the image of its variance interval, the weight-gradient slabs as
    float64 sums over their splits; bit-exact where the contract is a copy, a selection or a zero;
  - no NaN left in a write set, every other word of every output allocation bit-identical to its sentinel;
  - a second launch into fresh buffers gives the same bits;
  - large finite garbage instead of the NaN poison in everything the contract does not read leaves the outputs unchanged.
Identities that hold bit for bit, each read from the code: the split forward at tsplit = 1 is the one-launch forward (the merge
of one split multiplies by expf(0) = 1 and adds to 0); the split backward gives the same dx, work and dpack for every tsplit
(a frame's arithmetic does not depend on its tile); tstp / astp / preemph_pad with a full-length table are their plain entry
points; bn_prelu_fwd_len on valid rows is ws_bn_prelu_fwd.  Composed on the device's own intermediates: pack -> fwd -> bwd (and
the split pair) against the float64 gradient of the restatement, astp_fwd -> astp_bwd, tstp_fwd -> tstp_bwd, the adjoint pair
seg_sums / seg_scale, preemph_pad -> framing -> power_spec -> log_eps.  The last test writes the case count and the worst err /
bound per instantiation to pool_contract.json in $WESEP_TEST_OUT (default: the system's temporary directory);
profiles/pool_contract.md records the figures of a run.  No case passes arguments a valid caller could not, and no kernel is
broken to show a catch: tests/test_pool_contract_host_cpu.py plants the defects into the emulation."""
import json
import math
import os
import tempfile

import pytest
import torch

from tests import map_contract as mc
from tests import pool_contract as pc
from tests import step_contract as sc
from tests.gemm_contract import SENT, Case, eps_for

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")
U = pc.U
WORST = {}     # instantiation -> [worst err / bound, cases, the case that gave it]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _note(case, ratio, targets=None):
    for t in targets or case.targets:
        w = WORST.setdefault(t, [0.0, 0, ""])
        if ratio >= w[0]:
            w[0], w[2] = ratio, f"{case.entry} {case.name}"
        w[1] += 1


def _launch(b, d, mod=pc, **kw):
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    extra = mod.run(dev, b, t, d, **kw)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in t.items()}, {n: v.cpu() for n, v in (extra or {}).items()}


def _run(case):
    d = _cuda()
    b = pc.build(case)
    ref = pc.reference(b)
    after, extra = _launch(b, d)
    worst = pc.verify(b, ref, after, extra)
    bits = pc.output_bits(b, after, extra)
    assert torch.equal(bits, pc.output_bits(b, *_launch(b, d))), f"{case.name}: two launches differ"
    bg = pc.build(case, garbage=True)
    assert torch.equal(bits, pc.output_bits(bg, *_launch(bg, d))), f"{case.name}: garbage outside the contract reached the output"
    print(f"{case.entry} {case.name}: worst err / bound {worst:.3f}")
    _note(case, worst)
    return b, ref, after


def _same_bits(case, after, plain, keys, what):
    for k in keys:
        assert torch.equal(after[k].view(torch.int32), plain[k].view(torch.int32)), f"{case.name}: {k} differs from {what}"


def _identity(case, b, after):
    """The bit-for-bit identity of the case's entry, where it has one (module docstring)."""
    e, d = case.entry, _cuda()
    if e == "mhastp_fwd_split" and b.spec["tsplit"] == 1:
        _same_bits(case, after, _launch(b, d, plain=True)[0], ("out", "aux"), "ws_mhastp_fwd")
    elif e == "mhastp_bwd_split":          # every tsplit: dx, work, slab and dpack
        _same_bits(case, after, _launch(b, d, plain=True)[0], b.outs, "ws_mhastp_bwd")
    elif e in FULL_TABLE and case.dims["tab"] == "full":
        _same_bits(case, after, _launch(b, d, plain=True)[0], FULL_TABLE[e], "the plain entry point")
    elif e == "bn_prelu_fwd_len":          # valid rows: ws_bn_prelu_fwd on the same buffers with the poison behind the widths taken out
        clean = pc.build(case)
        for k in ("x", "res"):
            if k in clean.bufs:
                clean.bufs[k] = torch.nan_to_num(clean.bufs[k], nan=0.5)
        plain, _ = _launch(clean, d, plain=True)
        sp = b.spec
        m = torch.arange(sp["R"] * sp["rpr"])
        valid = ((m % sp["W"]) < pc.lens(e, sp)[m // sp["rpr"]])[:, None].expand(-1, sp["C"]).reshape(-1)
        for k in ("u", "y"):
            got, want = b.views(after)[k], clean.views(plain)[k]
            assert torch.equal(got[valid].view(torch.int32), want[valid].view(torch.int32)), f"{case.name}: {k} differs from ws_bn_prelu_fwd"


FULL_TABLE = {"tstp_fwd_len": ("stats",), "astp_fwd_len": ("out", "aux"), "preemph_pad_len": ("out",)}


@pytest.mark.parametrize("entry", pc.ENTRIES)
def test_entry_contract(entry):
    """Every case of the entry (a fraction of a second each; the whole entry in a few seconds); every failing case is named."""
    failed = []
    for case in pc.cases(entry):
        try:
            b, _, after = _run(case)
            _identity(case, b, after)
        except AssertionError as err:          # ContractViolation is one
            failed.append(f"{case.name}: {err}")
    assert not failed, f"{entry}: {len(failed)} of {len(pc.cases(entry))} cases fail\n" + "\n".join(failed)


def test_tail_select_len_over_the_grid_cap():
    """R T C / 4 = 32768 x 256 + 3 quads: the grid-stride loop's second trip and its three-quad tail.  The one case near workload
    size: one launch, judged bit for bit on the device."""
    from wesep_amd import dev
    d = _cuda()
    case = pc.GRID_CAP_CASE
    R, T, C = (case.dims[k] for k in ("R", "T", "C"))
    tab = pc.make_table("mixed", R, 0, T, case.seed)
    g = torch.Generator().manual_seed(case.seed)
    x = torch.rand(R, T, C, generator=g).to(d)
    n = torch.tensor(tab, device=d).clamp(0, T)
    live = torch.arange(T, device=d)[None, :] < n[:, None]
    x[~live] = NAN
    G = 1024
    y = torch.full((R * T * C + 2 * G,), SENT, device=d)
    dev.tail_select_len(x, R, T, C, torch.tensor(tab, dtype=torch.int32, device=d), y[G:G + R * T * C])
    torch.cuda.synchronize()
    want = torch.where(live[:, :, None], x, torch.zeros((), device=d)).reshape(-1)
    assert torch.equal(y[G:-G].view(torch.int32), want.view(torch.int32))
    assert bool((y[:G] == SENT).all()) and bool((y[-G:] == SENT).all())
    _note(case, 0.0)


# ------------------------------------------------------------------------------------------------------------
# composed
# ------------------------------------------------------------------------------------------------------------
def _mk(entry, spec, ins, outs, inplace=()):
    """A hand-built case: operands `ins` (name -> values), outputs `outs` (name -> floats), operands written `inplace`."""
    b = pc.TBuilt(Case(entry, "chain", {}, ("composed",), 0))
    b.spec.update(spec)
    for k, v in ins.items():
        mc._input(b, k, v, NAN)
    for k, n in outs.items():
        mc._output(b, k, n)
    for k in inplace:
        mc._alias(b, k, k, torch.arange(b.size[k]))
    return b


def _sensitivity(fn, a, B):
    """sum_j |fn(a + B_j e_j) - fn(a)|: the first-order reach of a perturbation |da_j| <= B_j of the forward quantities a."""
    base = fn(a)
    tot = {k: torch.zeros_like(v) for k, v in base.items()}
    for j in range(a.numel()):
        if float(B[j]) == 0.0:
            continue
        a2 = a.clone()
        a2[j] += B[j]
        for k, v in fn(a2).items():
            tot[k] += (v - base[k]).abs()
    return base, tot


def _against_float64(name, got, want, stage_bound, reach):
    """|device - float64 chain| <= the stage's own bound + 1.01 x the first-order reach of the forward's bound (second order: 1 %)."""
    err = (got.double().reshape(-1) - want.reshape(-1)).abs()
    tol = stage_bound.reshape(-1) + 1.01 * reach.reshape(-1) + pc.TINY
    ratio = float((err / tol).max())
    assert ratio <= 1.0, (name, ratio)
    return ratio


@pytest.mark.parametrize("Q,layers,dsk,tsplit", [(1, 2, "1", None), (2, 2, "dm", 2), (2, 1, "dm", None), (3, 1, "1", 3)])
def test_chain_mhastp_pack_forward_backward_against_the_float64_gradient(Q, layers, dsk, tsplit):
    """ws_mhastp_pack -> fwd -> bwd (tsplit: the split pair) on the device's own pack and aux, MHASTP (Q = 1) and MQMHASTP.  Every
    stage is judged by its own reference at the operands it met; dx and dpack also against the float64 backward at the float64
    aux, with the forward's derived bound on aux carried to first order (_sensitivity)."""
    from wesep_amd import dev
    d = _cuda()
    R, F_, T, Ch, H = 2, 2, 19, 3, 2
    dm = F_ * Ch
    ds = 1 if dsk == "1" else dm
    sp = dict(R=R, F=F_, T=T, Ch=Ch, C=Ch * H, Q=Q, H=H, layers=layers, ds=ds, TTf=pc.mh_tt(dm, layers, ds, False), TTb=pc.mh_tt(dm, layers, ds, True),
              regime="gauss", wgrad=1, nsplit=3)
    if tsplit:
        sp["tsplit"] = tsplit
    g = torch.Generator().manual_seed(4100 + Q)
    x = torch.randn(R, F_, T, Ch * H, generator=g)
    weights = pc.mh_weights(g, sp, "gauss", None)
    P1 = pc.mh_block_floats(layers, ds, dm)
    pack = torch.empty(Q * H * P1, device=d)
    for i, (W1, b1, W2, b2) in enumerate(weights):          # one launch per (query, head) block
        dev.mhastp_pack(W1.to(d), b1.to(d), None if W2 is None else W2.to(d), None if b2 is None else b2.to(d), F_, Ch, layers, ds, pack[i * P1:(i + 1) * P1])
    torch.cuda.synchronize()
    assert torch.equal(pack.cpu(), pc.mh_pack(sp, weights))
    n_aux, n_out = R * Q * H * 4 * dm, R * Q * H * 2 * dm
    fe, be = ("mhastp_fwd_split", "mhastp_bwd_split") if tsplit else ("mhastp_fwd", "mhastp_bwd")
    b1_ = _mk(fe, sp, dict(x=x, pack=pack.cpu()), dict(out=n_out, aux=n_aux, **({"part": tsplit * n_aux} if tsplit else {})))
    r1 = pc.reference(b1_)
    a1, _ = _launch(b1_, d)
    w1 = pc.verify(b1_, r1, a1, what="chain fwd")
    aux_dev = b1_.views(a1)["aux"]
    dout = torch.randn(R, Q, H, 2, dm, generator=g)
    M = R * T
    outs = dict(dx=x.numel(), work=M * Q * H * (pc.mh_n1(layers, ds) + (64 + ds if layers == 2 else 0)), slab=3 * Q * H * P1, dpack=Q * H * P1)
    b2_ = _mk(be, sp, dict(x=x, pack=pack.cpu(), aux=aux_dev, dout=dout), outs)
    r2 = pc.reference(b2_)
    a2, _ = _launch(b2_, d)
    w2 = pc.verify(b2_, r2, a2, what="chain bwd")
    t64 = b2_.views(b2_.bufs)
    aux64 = pc.compute("mhastp_fwd", sp, t64, F64)["aux"].reshape(-1)
    fn = lambda a: {k: v for k, v in pc.compute("mhastp_bwd", sp, dict(t64, aux=a), F64).items() if k in ("dx", "dpack")}          # noqa: E731
    B = (r1["aux"].val - aux64).abs() + r1["aux"].bound
    want, reach = _sensitivity(fn, aux64, B)
    got = b2_.views(a2)
    w3 = max(_against_float64(k, got[k], want[k], r2[k].bound, reach[k]) for k in ("dx", "dpack"))
    print(f"MHASTP chain Q{Q} layers {layers} ds {dsk} tsplit {tsplit}: stages {w1:.3f} {w2:.3f}, against the float64 gradient {w3:.3f}")
    _note(Case("chain", f"mhastp-{Q}-{layers}-{dsk}-{tsplit}", {}, (), 0), max(w1, w2, w3), ("composed",))


def test_chain_astp_forward_backward_against_the_float64_gradient():
    d = _cuda()
    R, T, C = 3, 37, 65
    g = torch.Generator().manual_seed(4200)
    x, lg = torch.randn(R, T, C, generator=g), torch.randn(R, T, C, generator=g)
    sp = dict(R=R, T=T, C=C, regime="gauss")
    b1 = _mk("astp_fwd", sp, dict(x=x, lg=lg), dict(out=R * 2 * C, aux=R * 4 * C))
    r1 = pc.reference(b1)
    a1, _ = _launch(b1, d)
    w1 = pc.verify(b1, r1, a1, what="chain astp_fwd")
    v1 = b1.views(a1)
    dout = torch.randn(R, 2 * C, generator=g)
    b2 = _mk("astp_bwd", sp, dict(x=x, lg=lg, out=v1["out"], aux=v1["aux"], dout=dout), dict(dx=R * T * C, dlg=R * T * C))
    r2 = pc.reference(b2)
    a2, _ = _launch(b2, d)
    w2 = pc.verify(b2, r2, a2, what="chain astp_bwd")
    t64 = b2.views(b2.bufs)
    f64 = pc.compute("astp_fwd", sp, t64, F64)
    a64 = torch.cat([f64["out"].reshape(-1), f64["aux"].reshape(-1)])
    br = f64["aux"][:, 3] - f64["aux"][:, 2] ** 2 > pc.FLOOR32
    fn = lambda a: pc.compute("astp_bwd", dict(sp, branch=br), dict(t64, out=a[:R * 2 * C], aux=a[R * 2 * C:]), F64)          # noqa: E731
    B = torch.cat([(r1[k].val - f64[k].reshape(-1)).abs() + r1[k].bound for k in ("out", "aux")])
    want, reach = _sensitivity(fn, a64, B)
    got = b2.views(a2)
    w3 = max(_against_float64(k, got[k], want[k], r2[k].bound, reach[k]) for k in ("dx", "dlg"))
    print(f"ASTP chain: stages {w1:.3f} {w2:.3f}, against the float64 gradient {w3:.3f}")
    _note(Case("chain", "astp", {}, (), 0), max(w1, w2, w3), ("composed",))


def test_chain_tstp_forward_backward_against_the_float64_gradient():
    d = _cuda()
    R, Fq, T, C = 2, 3, 9, 7
    g = torch.Generator().manual_seed(4300)
    x = torch.randn(R, Fq, T, C, generator=g) + 0.5
    sp = dict(R=R, F=Fq, T=T, C=C, eps=1e-7)
    b1 = _mk("tstp_fwd", sp, dict(x=x), dict(stats=R * 2 * C * Fq))
    r1 = pc.reference(b1)
    a1, _ = _launch(b1, d)
    w1 = pc.verify(b1, r1, a1, what="chain tstp_fwd")
    ds = torch.randn(R, 2, C * Fq, generator=g)
    b2 = _mk("tstp_bwd", sp, dict(x=x, stats=b1.views(a1)["stats"], dstats=ds), dict(dx=x.numel()))
    b2.extras = []
    r2 = sc.reference(b2)
    a2, _ = _launch(b2, d, mod=sc)
    w2 = sc.verify(b2, r2, a2, {}, what="chain tstp_bwd")
    t64 = b2.views(b2.bufs)
    s64 = pc.compute("tstp_fwd", sp, t64, F64)["stats"].reshape(-1)
    fn = lambda a: sc.compute("tstp_bwd", sp, dict(t64, stats=a), F64)          # noqa: E731
    want, reach = _sensitivity(fn, s64, (r1["stats"].val - s64).abs() + r1["stats"].bound)
    w3 = _against_float64("dx", b2.views(a2)["dx"], want["dx"], r2["dx"].bound, reach["dx"])
    xr = x.double().requires_grad_(True)
    st = torch.stack([xr.mean(2).permute(0, 2, 1).reshape(R, -1), torch.sqrt(xr.var(2, unbiased=True) + float(pc._f32(1e-7))).permute(0, 2, 1).reshape(R, -1)], 1)
    auto = torch.autograd.grad((st * ds.double()).sum(), xr)[0].reshape(-1)
    assert float((auto - want["dx"]).abs().max()) <= 1e-11 * float(auto.abs().max())
    print(f"TSTP chain: stages {w1:.3f} {w2:.3f}, against the float64 gradient {w3:.3f}")
    _note(Case("chain", "tstp", {}, (), 0), max(w1, w2, w3), ("composed",))


@pytest.mark.parametrize("T,seg_len", [(101, 3), (7, 100), (199, 2)])
def test_seg_sums_and_seg_scale_are_adjoint(T, seg_len):
    """<seg_sums(a), m> = <a, seg_scale(m)>: seg_scale without x is a copy (exact), so the two sides differ by what seg_sums'
    bound allows: sum |m| e(seg_len + 1) sum_seg |a|."""
    d = _cuda()
    R, C = 2, 12
    nseg = -(-T // seg_len)
    g = torch.Generator().manual_seed(4400 + T)
    a, m = torch.randn(R, T, C, generator=g), torch.randn(R, nseg, C, generator=g)
    b1 = _mk("seg_sums", dict(R=R, T=T, C=C, seg_len=seg_len, b=0), dict(a=a), dict(out=R * nseg * C))
    b2 = _mk("seg_scale", dict(R=R, T=T, C=C, seg_len=seg_len, x=0, alias=0), dict(m=m), dict(out=R * T * C))
    a1, _ = _launch(b1, d)
    a2, _ = _launch(b2, d)
    r1 = pc.reference(b1)
    w = max(pc.verify(b1, r1, a1), pc.verify(b2, pc.reference(b2), a2))
    lhs = float((b1.views(a1)["out"].double() * m.double().reshape(-1)).sum())
    rhs = float((a.double().reshape(-1) * b2.views(a2)["out"].double()).sum())
    tol = float((m.double().reshape(-1).abs() * r1["out"].bound).sum()) + 1e-12 * float((a.double().abs().reshape(R, T, C) * 1.0).sum())
    print(f"adjoint T{T} seg_len {seg_len}: {lhs!r} vs {rhs!r}, |diff| / tol {abs(lhs - rhs) / tol:.3f}")
    assert abs(lhs - rhs) <= tol
    _note(Case("chain", f"seg-adjoint-{T}-{seg_len}", {}, (), 0), max(w, abs(lhs - rhs) / tol), ("composed",))


def test_chain_front_end_against_float64():
    """ws_preemph_pad -> (float64 framing and DFT of the device's padded signal, uploaded as fp32 spectra) -> ws_power_spec ->
    ws_log_eps.  Every device stage is judged at the operands it met; the log power against the float64 chain from x, with the
    pre-emphasis bound carried through the DFT (|basis| B), the fp32 rounding of the spectra (u) and the power into the log."""
    d = _cuda()
    R, T, pad, nfft, hop, coef, eps = 2, 50, 8, 16, 4, 0.97, 1e-6
    nf, Tp = nfft // 2 + 1, T + 2 * pad
    g = torch.Generator().manual_seed(4500)
    x = torch.randn(R, T, generator=g)
    sp1 = dict(R=R, T=T, pad=pad, ldo=Tp + 5, coef=coef)
    b1 = _mk("preemph_pad", sp1, dict(x=x), {})
    mc._output(b1, "out", R * sp1["ldo"], torch.arange(R)[:, None] * sp1["ldo"] + torch.arange(Tp)[None, :])
    r1 = pc.reference(b1)
    a1, _ = _launch(b1, d)
    w1 = pc.verify(b1, r1, a1, what="chain preemph_pad")
    nfr = (Tp - nfft) // hop + 1
    k = torch.arange(nfft, dtype=F64)
    win = 0.54 - 0.46 * torch.cos(2 * math.pi * k / nfft)
    ang = 2 * math.pi * torch.arange(nf, dtype=F64)[:, None] * k[None, :] / nfft
    Bc, Bs = win * torch.cos(ang), -win * torch.sin(ang)          # [nf, nfft]

    def spectra(padded, bound):
        fr = padded.unfold(1, nfft, hop)[:, :nfr]          # [R, nfr, nfft]
        fb = bound.unfold(1, nfft, hop)[:, :nfr]
        return fr @ Bc.t(), fr @ Bs.t(), fb @ Bc.abs().t(), fb @ Bs.abs().t()
    dev_pad = b1.views(a1)["out"].double().reshape(R, sp1["ldo"])[:, :Tp]
    re, im, _, _ = spectra(dev_pad, torch.zeros(R, Tp, dtype=F64))
    M, lds, ldp = R * nfr, 2 * nf + 2, nf + 3
    spec = torch.zeros(M, lds)
    spec[:, 0:2 * nf:2], spec[:, 1:2 * nf:2] = re.reshape(M, nf).float(), im.reshape(M, nf).float()
    rd = torch.zeros(M, lds, dtype=torch.bool)
    rd[:, :2 * nf] = True
    b2 = _mk("power_spec", dict(M=M, nf=nf, lds=lds, ldp=ldp), {}, dict(p=M * ldp))
    mc._input(b2, "spec", spec, NAN, rd)
    r2 = pc.reference(b2)
    a2, _ = _launch(b2, d)
    w2 = pc.verify(b2, r2, a2, what="chain power_spec")
    p_dev = b2.views(a2)["p"].reshape(M, ldp)[:, :nf].contiguous()
    b3 = _mk("log_eps", dict(n=M * nf, eps=eps), dict(x=p_dev), {}, inplace=("x",))
    r3 = pc.reference(b3)
    a3, _ = _launch(b3, d)
    w3 = pc.verify(b3, r3, a3, what="chain log_eps")
    # the float64 chain from x, and what the stages' bounds allow at its end
    want_pad = r1["out"].val.reshape(R, Tp)
    re64, im64, d_re, d_im = spectra(want_pad, r1["out"].bound.reshape(R, Tp))
    d_re, d_im = d_re + U * re64.abs() * (1 + U), d_im + U * im64.abs() * (1 + U)          # uploaded as fp32
    p64 = re64 ** 2 + im64 ** 2
    d_p = 2 * re64.abs() * d_re + d_re ** 2 + 2 * im64.abs() * d_im + d_im ** 2
    d_p = d_p + 4 * U * (p64 + d_p)          # power_spec's own roundings
    e32 = float(pc._f32(eps))
    want = torch.log(p64 + e32)
    tol = -torch.log1p(-(d_p / (p64 + e32)).clamp(max=0.5)) + U * (1 + 4 * U) + pc.D_LOG * want.abs()
    err = (b3.views(a3)["x"].double().reshape(want.shape) - want).abs()
    w4 = float((err / tol).max())
    print(f"front-end chain: stages {w1:.3f} {w2:.3f} {w3:.3f}, against float64 {w4:.3f}")
    assert w4 <= 1.0
    _note(Case("chain", "front-end", {}, (), 0), max(w1, w2, w3, w4), ("composed",))


def test_invalid_argument_sets_are_refused_and_launch_nothing():
    """Every refusal raises (the return code), and the tensor it was handed is untouched afterwards."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    t = torch.full((1 << 16,), SENT, device=d)
    for name, call in pc.refusals(dev, t, d):
        with pytest.raises(L.WesepHipError):
            call()
        torch.cuda.synchronize()
        assert bool((t == SENT).all()), f"{name}: the refused call wrote"


def test_zz_write_worst_ratios():
    """Last in the file: the case count, the worst err / bound and the case that gave it, per instantiation ->
    $WESEP_TEST_OUT/pool_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "pool_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1], "worst_case": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
    assert eps_for(False, 0) == 8 * U
