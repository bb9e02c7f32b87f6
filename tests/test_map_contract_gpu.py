"""Contract sweep of the feature-map kernels of conv2d.hip on the GPU (tests/map_contract.py): every generated case goes
through wesep_amd.dev -> libwesep_hip.so (ws_im2col_hw, ws_col2im_hw, ws_elu_fwd / bwd, ws_inorm_finalize / apply / bwd_apply,
ws_in_act_sums / apply / bwd_apply, ws_avgpool_fwd / bwd, ws_bilinear_fwd / bwd, ws_scale_bf_fwd / bwd, ws_freq_linear_fwd,
ws_softmax_rows_fwd / bwd, ws_rowbias_act_fwd, ws_act_bwd) inside guarded allocations and is held against the float64 index
arithmetic that restates include/wesep_hip.h:
  - every element of a write set inside its bound, rstd inside its interval (map_contract's docstring derives both), the
    in_act_sums slab as float64 sums over its splits; bit-exact where the contract is a copy; exact zeros on padding taps,
    uncovered pixels, the dropped avgpool tail and the splits that own no row;
  - no NaN left in a write set (it starts as NaN; dx aliasing dy: as that operand);
  - every other word of every output allocation bit-identical to its sentinel: ldp padding, the columns outside
    [off, off + C) of a strided y / dx, guards; the scratch of ws_bilinear_bwd is written inside its extent only;
  - a second launch into fresh buffers gives the same bits;
  - large finite garbage instead of the NaN poison in everything the contract does not read leaves the outputs unchanged.
Composed: the chains dev.inorm_fwd -> inorm_bwd, dev.in_act_fwd -> in_act_bwd (several nsplit, strided y / dy / dx),
avgpool -> bilinear and softmax fwd -> bwd, every stage fed the device output of the one before, with propagated bounds; the
adjoint identities of im2col / col2im, avgpool and bilinear in float64 accumulation; in_act with flags = 0 against inorm; the
reduced in_act sums under every nsplit; softmax rows summing to 1; the fwd4 and the scalar softmax kernels on the same row; the
square wrappers ws_im2col / ws_col2im against the _hw entries; the grid-stride seam of the 65536-block launches on ws_elu_fwd.
The last test writes the case count and the worst err / bound per instantiation to map_contract.json in the directory
$WESEP_TEST_OUT (default: the system's temporary directory); profiles/map_contract.md records the figures of a run.  No case
passes arguments a valid caller could not, no misaligned pointer goes to a vectorised entry, and no kernel is broken to show a
catch: tests/test_map_contract_host_cpu.py plants the defects into the emulation."""
import json
import os
import tempfile

import pytest
import torch

from tests import gemm_contract as gc
from tests import map_contract as mc
from tests.gemm_contract import GUARD, SENT, U, Case, check, eps_for

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = float("nan")
WORST = {}     # instantiation -> [worst err / bound, cases, the case that gave it]


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


def _launch(b, d, entry=None):
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    mc.run(dev, b, t, entry)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in t.items()}


def _run(case):
    d = _cuda()
    b = mc.build(case)
    ref = mc.reference(b)
    after = _launch(b, d)
    worst = mc.verify(b, ref, after)
    assert torch.equal(mc.output_bits(b, after), mc.output_bits(b, _launch(b, d))), f"{case.name}: two launches differ"
    bg = mc.build(case, garbage=True)
    assert torch.equal(mc.output_bits(b, after), mc.output_bits(bg, _launch(bg, d))), \
        f"{case.name}: garbage outside the contract reached the output"
    print(f"{case.entry} {case.name}: worst err / bound {worst:.3f}")
    _note(case, worst)
    return b, ref, after


def _sweep(entry):
    return pytest.mark.parametrize("case", mc.cases(entry), ids=lambda c: c.name)


@_sweep("im2col")
def test_im2col_contract(case):
    _run(case)


@_sweep("col2im")
def test_col2im_contract(case):
    _run(case)


@_sweep("elu_fwd")
def test_elu_fwd_contract(case):
    _run(case)


@_sweep("elu_bwd")
def test_elu_bwd_contract(case):
    _run(case)


@_sweep("inorm_finalize")
def test_inorm_finalize_contract(case):
    _run(case)


@_sweep("inorm_apply")
def test_inorm_apply_contract(case):
    _run(case)


@_sweep("inorm_bwd_apply")
def test_inorm_bwd_apply_contract(case):
    _run(case)


@_sweep("in_act_sums")
def test_in_act_sums_contract(case):
    _run(case)


@_sweep("in_act_apply")
def test_in_act_apply_contract(case):
    _run(case)


@_sweep("in_act_bwd_apply")
def test_in_act_bwd_apply_contract(case):
    _run(case)


@_sweep("avgpool_fwd")
def test_avgpool_fwd_contract(case):
    _run(case)


@_sweep("avgpool_bwd")
def test_avgpool_bwd_contract(case):
    _run(case)


@_sweep("bilinear_fwd")
def test_bilinear_fwd_contract(case):
    _run(case)


@_sweep("bilinear_bwd")
def test_bilinear_bwd_contract(case):
    _run(case)


@_sweep("scale_bf_fwd")
def test_scale_bf_fwd_contract(case):
    _run(case)


@_sweep("scale_bf_bwd")
def test_scale_bf_bwd_contract(case):
    _run(case)


@_sweep("freq_linear")
def test_freq_linear_contract(case):
    _run(case)


@_sweep("softmax_fwd")
def test_softmax_fwd_contract(case):
    b, ref, after = _run(case)
    sp, r = b.spec, ref["y"]
    y = after["y"][b.start["y"]:][:sp["rows"] * sp["n"]].double().reshape(sp["rows"], sp["n"])
    tol = r.bound.reshape(sp["rows"], sp["n"]).sum(1)
    assert bool(((y.sum(1) - 1).abs() <= tol).all()), f"{case.name}: a row does not sum to 1 within {float(tol.max()):.2e}"


@_sweep("softmax_bwd")
def test_softmax_bwd_contract(case):
    _run(case)


@_sweep("rowbias_act")
def test_rowbias_act_contract(case):
    _run(case)


@_sweep("act_bwd")
def test_act_bwd_contract(case):
    _run(case)


# ------------------------------------------------------------------------------------------------------------
# composed
# ------------------------------------------------------------------------------------------------------------
def _mk(entry, spec, ins, outs):
    """A hand-built case: operands `ins` (name -> values), outputs `outs` (name -> (floats, write set or None))."""
    b = mc.MBuilt(Case(entry, "chain", {}, ("composed",), 0))
    b.spec.update(spec)
    for k, v in ins.items():
        mc._input(b, k, v, NAN)
    for k, (n, widx) in outs.items():
        mc._output(b, k, n, widx)
    return b


def _stage(d, entry, spec, ins, outs):
    """One stage of a chain through the single entry: checked against the reference at exactly these operands.  Returns
    (worst ratio, name -> the tensor the call left, the reference)."""
    b = _mk(entry, spec, ins, outs)
    ref = mc.reference(b)
    after = _launch(b, d)
    worst = mc.verify(b, ref, after, what=f"chain {entry}")
    return worst, {k: after[k][b.start[k]:][:outs[k][0]] for k in outs}, ref


def _guarded(d, data=None, n=0):
    """(device tensor inside guards, the whole allocation): an operand (data) or an output of n floats (NaN)."""
    t = gc.alloc(data.numel() if data is not None else n, SENT)
    m = data.numel() if data is not None else n
    t[GUARD:GUARD + m] = data.reshape(-1) if data is not None else NAN
    a = t.to(d)
    return a[GUARD:GUARD + m], a


def _guards_kept(a, n, what):
    c = a.cpu()
    assert bool((c[:GUARD] == SENT).all()) and bool((c[GUARD + n:] == SENT).all()), f"{what}: a guard changed"


NORM_CHAINS = [(3, 33, 12, "gauss"), (1, 257, 16, "gauss"), (2, 64, 256, "offset"), (3, 2, 1028, "gauss"), (2, 31, 4, "const"),
               (1, 1, 8, "gauss")]


def _chain_fwd_check(x64, flags, stats_dev, y_dev, eps):
    """The statistics and y a chain (sums -> finalize -> apply) leaves for x, against the exact float64 values with the
    propagated bounds of map_contract's docstring.  Returns the worst ratio."""
    G, P, C = x64.shape
    u = mc._elu(x64) if flags & 1 else x64
    sref, (mean, d_m, lo, hi) = mc.chain_stats_ref(u, eps, bool(flags & 1))
    st = stats_dev.cpu().reshape(-1)
    w0 = check(st, st, sref, "chain stats", 0)
    rstd = 1 / torch.sqrt((((u * u).mean(1) - mean * mean).clamp_min(0)) + eps)
    d_r = torch.maximum(hi - rstd, rstd - lo)
    du = mc.D_EXPM1 * u.abs() * (x64 <= 0) if flags & 1 else torch.zeros_like(u)
    um = (u - mean.unsqueeze(1)).abs()
    n = (u - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    dn = (du + d_m.unsqueeze(1)) * hi.unsqueeze(1) + um * d_r.unsqueeze(1) + 2 * U * um * hi.unsqueeze(1)
    y = mc._elu(n) if flags & 2 else n
    bound = dn + (mc.D_EXPM1 * y.abs() if flags & 2 else 0) + U * y.abs()
    yc = y_dev.cpu().reshape(-1)
    w1 = check(yc, yc, mc._ref(torch.arange(y.numel()), y, y.abs(), bound), "chain y", 0)
    return max(w0, w1)


@pytest.mark.parametrize("G,P,C,data", NORM_CHAINS)
def test_chain_inorm_fwd_bwd_and_in_act_with_flags_0(G, P, C, data):
    """dev.inorm_fwd -> dev.inorm_bwd with propagated bounds; dev.in_act_fwd / in_act_bwd with flags = 0 meet the same ones."""
    from wesep_amd import dev
    d = _cuda()
    g = gc.gen(700 + P)
    x = mc._norm_data(g, G, P, C, data)
    dy = torch.randn(G, P, C, generator=g)
    xd, xa = _guarded(d, x)
    dyd, _ = _guarded(d, dy)
    worst = 0.0
    for which in ("inorm", "in_act"):
        yd, ya = _guarded(d, n=G * P * C)
        st = dev.inorm_fwd(xd, G, P, C, yd) if which == "inorm" else dev.in_act_fwd(xd, G, P, C, 0, yd)
        torch.cuda.synchronize()
        _guards_kept(ya, G * P * C, f"{which} y")
        worst = max(worst, _chain_fwd_check(x.double(), 0, st, yd, mc.IN_EPS))
        # backward, judged at the DEVICE y and statistics: the sums are the kernel's own (e(P) each)
        dxd, dxa = _guarded(d, n=G * P * C)
        if which == "inorm":
            dev.inorm_bwd(yd, dyd, st, G, P, C, dxd)
        else:
            dev.in_act_bwd(xd, dyd, st, G, P, C, 0, dxd)
        torch.cuda.synchronize()
        _guards_kept(dxa, G * P * C, f"{which} dx")
        s64 = st.cpu().double()
        rstd = s64[:, 1:2]
        y64 = yd.cpu().double().reshape(G, P, C) if which == "inorm" else (x.double() - s64[:, 0:1]) * rstd
        dn = torch.zeros_like(y64) if which == "inorm" else 2 * U * y64.abs()
        d64 = dy.double()
        s0, s1 = d64.mean(1, keepdim=True), (d64 * y64).mean(1, keepdim=True)
        a0, a1 = d64.abs().mean(1, keepdim=True), (d64 * y64).abs().mean(1, keepdim=True)
        ref = rstd * (d64 - s0 - y64 * s1)
        S = rstd.abs() * (d64.abs() + s0.abs() + (y64 * s1).abs())
        eP = eps_for(False, P)
        bound = eps_for(False, 0) * S + rstd.abs() * (eP * a0 + y64.abs() * (eP * a1 + (d64.abs() * dn).mean(1, keepdim=True)) + dn * s1.abs())
        o = dxd.cpu().reshape(-1)
        worst = max(worst, check(o, o, mc._ref(torch.arange(o.numel()), ref, S, bound), f"{which} chain dx", 0))
    print(f"inorm chain G{G} P{P} C{C} {data}: worst err / bound {worst:.3f}")
    _note(Case("chain", f"inorm-{G}-{P}-{C}-{data}", {}, (), 0), worst, ("composed",))


@pytest.mark.parametrize("flags", [1, 2, 3])
@pytest.mark.parametrize("G,P,C,data", NORM_CHAINS)
def test_chain_in_act_fwd_bwd(G, P, C, data, flags):
    """dev.in_act_fwd -> dev.in_act_bwd at several nsplit, y / dy / dx in a column range of a wider map: the statistics and y
    with propagated bounds; the backward sums and dx through the single entries at the DEVICE statistics."""
    from wesep_amd import dev
    d = _cuda()
    g = gc.gen(900 + 7 * P + flags)
    x = mc._norm_data(g, G, P, C, data)
    ld, off = 2 * C + 4, C + 4
    dyw = torch.randn(G * P, ld, generator=g)
    xd, _ = _guarded(d, x)
    worst = 0.0
    stats = []
    for ns in (None, 1, 3, P + 1):
        yd, ya = _guarded(d, n=G * P * ld)
        st = dev.in_act_fwd(xd, G, P, C, flags, yd, y_ld=ld, y_off=off, nsplit=ns)
        torch.cuda.synchronize()
        yc = ya.cpu()[GUARD:GUARD + G * P * ld].reshape(G * P, ld)
        assert bool(torch.isnan(yc[:, :off]).all()) and bool(torch.isnan(yc[:, off + C:]).all()), "columns outside [off, off + C) written"
        _guards_kept(ya, G * P * ld, "in_act y")
        worst = max(worst, _chain_fwd_check(x.double(), flags, st, yc[:, off:off + C].contiguous(), mc.IN_EPS))
        stats.append(st.cpu())
    # backward at the statistics of the default split: sums (every nsplit) and dx through the single entries
    st = stats[0]
    spec = dict(G=G, P=P, C=C, flags=flags, eps=mc.IN_EPS, bwd=True, ldd=ld, ldd_arg=ld, dy_off=off)
    sums = None
    for ns in (1, 3, 7, P, P + 1):
        w, out, ref = _stage(d, "in_act_sums", dict(spec, nsplit=ns), dict(x=x, dy=dyw, stats=st), dict(slab=(ns * G * 2 * C, None)))
        worst = max(worst, w)
        red = out["slab"].double().reshape(ns, -1).sum(0)
        if sums is not None:      # any nsplit gives the same reduced sums: both lie within the bound of the exact sum
            assert bool(((red - sums).abs() <= 2 * ref["slab"].bound).all()), f"nsplit {ns}: the reduced sums moved"
        sums = red
    w, out, _ = _stage(d, "in_act_bwd_apply", dict(spec, lddx=ld, lddx_arg=ld, dx_off=off),
                       dict(x=x, dy=dyw, stats=st, sums=sums.float()),
                       dict(dx=(G * P * ld, torch.arange(G * P)[:, None] * ld + off + torch.arange(C)[None, :])))
    worst = max(worst, w)
    # and the wrapper: the same dx within the propagated bound of its own sums
    dyd, _ = _guarded(d, dyw)
    dxd, dxa = _guarded(d, n=G * P * ld)
    dev.in_act_bwd(xd, dyd, st.to(d), G, P, C, flags, dxd, dy_ld=ld, dy_off=off, dx_ld=ld, dx_off=off, nsplit=3)
    torch.cuda.synchronize()
    _guards_kept(dxa, G * P * ld, "in_act dx")
    b = _mk("in_act_sums", dict(spec, nsplit=1), dict(x=x, dy=dyw, stats=st), {})
    sref = mc.reference(b, entry="in_act_sums")["slab"]
    b2 = _mk("in_act_bwd_apply", dict(spec, lddx=ld, lddx_arg=ld, dx_off=off), dict(x=x, dy=dyw, stats=st, sums=torch.zeros(G * 2 * C)), {})
    t64 = {k: v.double() for k, v in b2.bufs.items()}
    t64["sums"][b2.start["sums"]:][:G * 2 * C] = sref.val
    r = mc.reference(b2, t64)["dx"]
    _, _, n, _, rstd, _, _, _, _ = mc._in_act_errs(b2.spec, b2.views(t64))
    sb = sref.bound.reshape(G, 2, C)
    extra = rstd.abs() * (sb[:, 0:1] + n.abs() * sb[:, 1:2]) / P * (mc._elud(x.double()) if flags & 1 else 1)
    r = r._replace(bound=r.bound * (1 + 2 * U) + extra.reshape(-1) * (1 + eps_for(False, 3)))
    before = gc.alloc(G * P * ld, SENT)
    before[GUARD:GUARD + G * P * ld] = NAN
    worst = max(worst, check(dxa.cpu(), before, r, "in_act_bwd dx", GUARD))
    print(f"in_act chain G{G} P{P} C{C} {data} flags {flags}: worst err / bound {worst:.3f}")
    _note(Case("chain", f"in_act-{G}-{P}-{C}-{data}-{flags}", {}, (), 0), worst, ("composed",))


@pytest.mark.parametrize("sz,H,W,C", [(2, 9, 13, 4), (3, 9, 9, 8), (32, 64, 96, 4)])
def test_chain_avgpool_bilinear_and_the_adjoint_identities(sz, H, W, C):
    """avgpool -> bilinear back to (H, W) as DPCCN's pooling branch runs them, then both adjoints; <A x, g> = <x, A' g> in float64
    accumulation within the summed bounds of the two sides."""
    d = _cuda()
    B = 2
    g = gc.gen(1100 + sz)
    h, w = H // sz, W // sz
    x, gy = torch.randn(B * H * W * C, generator=g), torch.randn(B * H * W * C, generator=g)
    gp = torch.randn(B * h * w * C, generator=g)
    pool = dict(B=B, H=H, W=W, C=C, sz=sz)
    bl = dict(B=B, h=h, w=w, H=H, W=W, C=C)
    w1, o1, r1 = _stage(d, "avgpool_fwd", pool, dict(x=x), dict(y=(B * h * w * C, None)))
    w2, o2, r2 = _stage(d, "bilinear_fwd", bl, dict(x=o1["y"]), dict(y=(B * H * W * C, None)))
    w3, o3, r3 = _stage(d, "bilinear_bwd", bl, dict(dy=gy), dict(dx=(B * h * w * C, None), tmp=(B * H * w * C, None)))
    w4, o4, r4 = _stage(d, "avgpool_bwd", pool, dict(dy=o3["dx"]), dict(dx=(B * H * W * C, None)))
    w5, o5, r5 = _stage(d, "avgpool_bwd", pool, dict(dy=gp), dict(dx=(B * H * W * C, None)))
    for name, lhs, rhs, tol in (
            ("avgpool", (o1["y"].double() * gp.double()).sum(), (x.double() * o5["dx"].double()).sum(),
             (r1["y"].bound * gp.double().abs()).sum() + (r5["dx"].bound * x.double().abs()).sum()),
            ("bilinear", (o2["y"].double() * gy.double()).sum(), (o1["y"].double() * o3["dx"].double()).sum(),
             (r2["y"].bound * gy.double().abs()).sum() + (r3["dx"].bound * o1["y"].double().abs()).sum())):
        assert abs(float(lhs - rhs)) <= float(tol), f"{name}: <A x, g> - <x, A' g> = {float(lhs - rhs):.3e}, tolerance {float(tol):.3e}"
    worst = max(w1, w2, w3, w4, w5)
    print(f"avgpool {sz} -> bilinear {h}x{w} -> {H}x{W}: worst err / bound {worst:.3f}")
    _note(Case("chain", f"pool-{sz}-{H}-{W}-{C}", {}, (), 0), worst, ("composed",))


@pytest.mark.parametrize("img,k,stride,p,C", [("13x37", 3, (2, 2), 1, 4), ("13x37", 5, (1, 2), 0, 12), ("3x5", 1, (3, 3), 0, 4),
                                               ("Tx1", 3, (2, 1), 3, 16)])
def test_im2col_col2im_adjoint_and_the_square_wrappers(img, k, stride, p, C):
    from wesep_amd import dev
    d = _cuda()
    H, W = mc.IMG[img]
    R = 2
    sp = dict(R=R, H=H, W=W, C=C, k=k, sh=stride[0], sw=stride[1], p=p, ldp=k * k * C)
    Ho, Wo = mc.conv_geom(sp)
    M = R * Ho * Wo
    g = gc.gen(1300 + k)
    x, pt = torch.randn(R * H * W * C, generator=g), torch.randn(M * k * k * C, generator=g)
    w1, o1, _ = _stage(d, "im2col", sp, dict(x=x), dict(patches=(M * k * k * C, None)))
    w2, o2, r2 = _stage(d, "col2im", sp, dict(dpatches=pt), dict(dx=(R * H * W * C, None)))
    lhs, rhs = (o1["patches"].double() * pt.double()).sum(), (x.double() * o2["dx"].double()).sum()
    tol = (r2["dx"].bound * x.double().abs()).sum()      # im2col is exact; 1e-12: the two float64 accumulations themselves
    assert abs(float(lhs - rhs)) <= float(tol) + 1e-12 * float((x.double() * o2["dx"].double()).abs().sum()), (float(lhs - rhs), float(tol))
    if stride[0] == stride[1]:      # ws_im2col / ws_col2im are the _hw entries with sh = sw: the same bits
        a, aa = _guarded(d, n=M * k * k * C)
        dev.im2col(x.to(d), R, H, W, C, k, stride[0], p, a, k * k * C)
        b_, ba = _guarded(d, n=R * H * W * C)
        dev.col2im(pt.to(d), R, H, W, C, k, stride[0], p, b_)
        torch.cuda.synchronize()
        assert torch.equal(a.cpu().view(torch.int32), o1["patches"].view(torch.int32)) and torch.equal(b_.cpu().view(torch.int32), o2["dx"].view(torch.int32))
        _guards_kept(aa, M * k * k * C, "ws_im2col")
        _guards_kept(ba, R * H * W * C, "ws_col2im")
    _note(Case("chain", f"conv-{img}-{k}", {}, (), 0), max(w1, w2), ("composed",))


def test_square_im2col_single_channel_with_padded_rows():
    """ws_im2col with C = 1 and ldp > k*k: the same bits as ws_im2col_hw, the padding columns untouched."""
    from wesep_amd import dev
    d = _cuda()
    sp = dict(R=2, H=13, W=37, C=1, k=3, sh=2, sw=2, p=1, ldp=12)
    Ho, Wo = mc.conv_geom(sp)
    M = 2 * Ho * Wo
    x = torch.randn(2 * 13 * 37, generator=gc.gen(1400))
    widx = torch.arange(M)[:, None] * 12 + torch.arange(9)[None, :]
    _, o1, _ = _stage(d, "im2col", sp, dict(x=x), dict(patches=(M * 12, widx)))
    a, aa = _guarded(d, n=M * 12)
    a.fill_(SENT)
    dev.im2col(x.to(d), 2, 13, 37, 1, 3, 2, 1, a, 12)
    torch.cuda.synchronize()
    got = a.cpu().reshape(M, 12)
    assert torch.equal(got[:, :9], o1["patches"].reshape(M, 12)[:, :9]) and bool((got[:, 9:] == SENT).all())
    _guards_kept(aa, M * 12, "ws_im2col C = 1")


@pytest.mark.parametrize("n,scale,data", [(1024, 0.37, "gauss"), (256, -2.0, "spread60"), (4, 1.0, "dominant"), (1020, 1.0, "equal")])
def test_chain_softmax_and_both_kernel_pairs_on_the_same_rows(n, scale, data):
    """softmax fwd -> bwd at the device y; the fwd4 / bwd4 kernels (aligned) and the scalar ones (one float in) on the same rows."""
    from wesep_amd import dev
    d = _cuda()
    rows = 3
    c = Case("softmax_fwd", "chain", dict(n=n, rows=rows, scale=scale, data=data, align=0), ("composed",), 1500 + n)
    b = mc.build(c)
    x = b.views(b.bufs)["x"][:rows * n]
    sp = dict(rows=rows, n=n, scale=scale)
    w1, o1, r1 = _stage(d, "softmax_fwd", sp, dict(x=x), dict(y=(rows * n, None)))
    dy = torch.randn(rows * n, generator=gc.gen(1600 + n))
    w2, o2, r2 = _stage(d, "softmax_bwd", sp, dict(y=o1["y"], dy=dy), dict(dx=(rows * n, None)))
    # the scalar kernels: every operand one float into a 16-byte aligned allocation
    buf = {k: torch.full((rows * n + 8,), SENT, device=d) for k in ("x", "y", "dy", "dx")}
    buf["x"][1:1 + rows * n] = x.to(d)
    buf["dy"][1:1 + rows * n] = dy.to(d)
    v = {k: t[1:1 + rows * n] for k, t in buf.items()}
    assert all(t.data_ptr() % 16 == 4 for t in v.values())
    dev.softmax_rows_fwd(v["x"], rows, n, scale, v["y"])
    ys = v["y"].clone()
    v["y"].copy_(o1["y"].to(d))      # the backward pair on the SAME y
    dev.softmax_rows_bwd(v["y"], v["dy"], rows, n, scale, v["dx"])
    torch.cuda.synchronize()
    for k in ("y", "dx"):
        c_ = buf[k].cpu()
        assert float(c_[0]) == SENT and bool((c_[1 + rows * n:] == SENT).all()), f"scalar softmax {k}: wrote outside its rows"
    assert bool(((ys.cpu().double() - o1["y"].double()).abs() <= 2 * r1["y"].bound).all()), "fwd4 and the scalar forward disagree"
    assert bool(((v["dx"].cpu().double() - o2["dx"].double()).abs() <= 2 * r2["dx"].bound).all()), "bwd4 and the scalar backward disagree"
    _note(c, max(w1, w2), ("composed",))


def test_grid_stride_seam_of_the_65536_block_launches():
    """n = 4 * (65536 * 256 + 3) floats through ws_elu_fwd: the launch is capped at 65536 blocks of 256 threads, so the last
    three quads are second-trip work of threads 0..2.  The input repeats a tile of 4096 values: the first tile is judged
    against float64, every later tile must be bit-identical to the first."""
    from wesep_amd import dev
    d = _cuda()
    n, T = 4 * (65536 * 256 + 3), 4096
    tile = torch.randn(T, generator=gc.gen(1700)) * 3
    tile[::5] = tile[::5].abs()
    xa = torch.full((n + 2 * GUARD,), SENT, device=d)
    ya = torch.full((n + 2 * GUARD,), SENT, device=d)
    reps = -(-n // T)
    xa[GUARD:GUARD + n] = tile.to(d).repeat(reps)[:n]
    ya[GUARD:GUARD + n] = NAN
    dev.elu_fwd(xa[GUARD:GUARD + n], ya[GUARD:GUARD + n])
    torch.cuda.synchronize()
    y = ya[GUARD:GUARD + n]
    first = y[:T].cpu()
    r = mc.reference(_mk("elu_fwd", dict(n=T), dict(x=tile), dict(y=(T, None))))["y"]
    worst = check(first, first, r, "first tile", 0)
    full = (n // T) * T
    assert bool((y[:full].view(torch.int32).reshape(-1, T) == y[:T].view(torch.int32)).all()), "a later tile differs from the first"
    assert torch.equal(y[full:].view(torch.int32), y[:n - full].view(torch.int32)), "the tail behind the last whole tile differs"
    assert bool((ya[:GUARD] == SENT).all()) and bool((ya[GUARD + n:] == SENT).all()), "a guard changed"
    _note(Case("elu_fwd", "grid-stride", {}, (), 0), worst, ("elu_fwd_kernel[second trip]",))


def test_invalid_argument_sets_are_refused_and_launch_nothing():
    """Every refusal raises (the return code), and the tensor it was handed is untouched afterwards."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    t = torch.full((1 << 16,), SENT, device=d)
    for name, call in mc.refusals(dev, t):
        with pytest.raises(L.WesepHipError):
            call()
        torch.cuda.synchronize()
        assert bool((t == SENT).all()), f"{name}: the refused call wrote"


def test_zz_write_worst_ratios():
    """Last in the file: the case count, the worst err / bound and the case that gave it, per instantiation ->
    $WESEP_TEST_OUT/map_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "map_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1], "worst_case": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
