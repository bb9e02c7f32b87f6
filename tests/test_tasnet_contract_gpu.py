"""Contract sweep of the Conv-TasNet / SpEx+ kernels of tasnet.hip on the GPU (tests/tasnet_contract.py): every generated case
goes through wesep_amd.dev -> libwesep_hip.so (ws_prelu_fwd / bwd, ws_dwconv_ex_fwd / bwd, ws_chan_sums, ws_norm_ab,
ws_norm_bwd_apply_cl, ws_maskmul_fwd / bwd, ws_relu_mask, ws_ola_fwd / bwd, ws_sum_partial, ws_bn_stats, ws_bn_prelu_fwd,
ws_bn_bwd, ws_maxpool3_fwd / bwd, ws_bcast_rows, ws_cross_entropy) inside guarded allocations and is held against the float64
index arithmetic that restates include/wesep_hip.h:
  - every element of a write set inside its bound, rstd inside its interval (tasnet_contract's docstring derives both), every
    slab as float64 sums over its splits with the split counts of the case, not of the wrapper; bit-exact where the contract is
    a copy or a selection; exact zeros in the slabs of splits and blocks that own nothing, in the second row of chan_sums
    without x, on maxpool3_bwd's tail rows and behind Tout;
  - no NaN left in a write set (it starts as NaN; an output that aliases an operand: as that operand);
  - every other word of every output allocation bit-identical to its sentinel: the columns outside the N written of dw, guards;
  - a second launch into fresh buffers gives the same bits;
  - large finite garbage instead of the NaN poison in everything the contract does not read leaves the outputs unchanged.
The three geometries at which dwconv_bwd_w_kernel takes more than 64 KB of dynamic LDS are cases of the dwconv_bwd sweep.  The
plain wrappers ws_dwconv_fwd / ws_dwconv_bwd give the bits of the _ex entries with causal = 0.  Composed: dwconv_ex_bwd ->
chan_sums -> norm_ab -> norm_bwd_apply_cl (the gLN backward of a Conv1DBlock) and bn_stats -> bn_prelu_fwd -> bn_bwd, every
stage fed the device output of the one before and judged at exactly those operands; the adjoint identities of ola_fwd / ola_bwd
and of dwconv_fwd / dwconv_bwd's dxn in float64 accumulation.  The last test writes the case count and the worst err / bound
per instantiation to tasnet_contract.json in the directory $WESEP_TEST_OUT (default: the system's temporary directory);
profiles/tasnet_contract.md records the figures of a run.  No case passes arguments a valid caller could not, and no kernel is
broken to show a catch: tests/test_tasnet_contract_host_cpu.py plants the defects into the emulation."""
import json
import os
import tempfile

import pytest
import torch

from tests import map_contract as mc
from tests import tasnet_contract as tc
from tests.gemm_contract import SENT, Case

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
        if ratio >= w[0]:
            w[0], w[2] = ratio, f"{case.entry} {case.name}"
        w[1] += 1


def _launch(b, d, plain=False):
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    extra = tc.run(dev, b, t, d, plain=plain)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in t.items()}, {n: v.cpu() for n, v in extra.items()}


def _run(case):
    d = _cuda()
    b = tc.build(case)
    ref = tc.reference(b)
    after, extra = _launch(b, d)
    worst = tc.verify(b, ref, after, extra)
    bits = tc.output_bits(b, after, extra)
    assert torch.equal(bits, tc.output_bits(b, *_launch(b, d))), f"{case.name}: two launches differ"
    bg = tc.build(case, garbage=True)
    assert torch.equal(bits, tc.output_bits(bg, *_launch(bg, d))), f"{case.name}: garbage outside the contract reached the output"
    print(f"{case.entry} {case.name}: worst err / bound {worst:.3f}")
    _note(case, worst)
    return b, ref, after, extra


def _sweep(entry):
    return pytest.mark.parametrize("case", tc.cases(entry), ids=lambda c: c.name)


@_sweep("prelu_fwd")
def test_prelu_fwd_contract(case):
    b, _, after, _ = _run(case)
    if b.spec["rb"]:      # y on the positive side is the pre-activation the kernel saved, to the bit
        v = b.views(after)
        n = b.spec["rows"] * b.spec["C"]
        pos = v["x"][:n] > 0
        assert torch.equal(v["y"][:n][pos], v["x"][:n][pos]), f"{case.name}: y differs from the saved pre-activation where it is positive"


@_sweep("prelu_bwd")
def test_prelu_bwd_contract(case):
    _run(case)


@_sweep("dwconv_fwd")
def test_dwconv_fwd_contract(case):
    _run(case)


@_sweep("dwconv_bwd")
def test_dwconv_bwd_contract(case):
    _run(case)


@_sweep("chan_sums")
def test_chan_sums_contract(case):
    _run(case)


@_sweep("norm_ab")
def test_norm_ab_contract(case):
    _run(case)


@_sweep("norm_bwd_apply")
def test_norm_bwd_apply_contract(case):
    _run(case)


@_sweep("maskmul_fwd")
def test_maskmul_fwd_contract(case):
    _run(case)


@_sweep("maskmul_bwd")
def test_maskmul_bwd_contract(case):
    _run(case)


@_sweep("relu_mask")
def test_relu_mask_contract(case):
    _run(case)


@_sweep("ola_fwd")
def test_ola_fwd_contract(case):
    _run(case)


@_sweep("ola_bwd")
def test_ola_bwd_contract(case):
    _run(case)


@_sweep("sum_partial")
def test_sum_partial_contract(case):
    _run(case)


@_sweep("bn_stats")
def test_bn_stats_contract(case):
    _run(case)


@_sweep("bn_prelu_fwd")
def test_bn_prelu_fwd_contract(case):
    _run(case)


@_sweep("bn_bwd")
def test_bn_bwd_contract(case):
    _run(case)


@_sweep("maxpool3_fwd")
def test_maxpool3_fwd_contract(case):
    _run(case)


@_sweep("maxpool3_bwd")
def test_maxpool3_bwd_contract(case):
    _run(case)


@_sweep("bcast_rows")
def test_bcast_rows_contract(case):
    _run(case)


@_sweep("cross_entropy")
def test_cross_entropy_contract(case):
    b, ref, after, _ = _run(case)
    sp = b.spec
    dl = b.views(after)["dlogits"].double().reshape(sp["R"], sp["S"])
    tol = ref["dlogits"].bound.reshape(sp["R"], sp["S"]).sum(1)
    assert bool((dl.sum(1).abs() <= tol).all()), f"{case.name}: a row of dlogits does not sum to 0 within {float(tol.max()):.2e}"


@pytest.mark.parametrize("entry", sorted(tc.PLAIN))
def test_plain_dwconv_wrappers_are_the_ex_entries_with_causal_0(entry):
    d = _cuda()
    c = tc.plain_case(entry)
    b = tc.build(c)
    ref = tc.reference(b)
    after, extra = _launch(b, d, plain=True)
    ref = {k: v for k, v in ref.items() if k not in ("dw", "db")}          # the plain call hands back the slab alone
    b.extras = [k for k in b.extras if k in extra]
    worst = tc.verify(b, ref, after, extra)
    ex_after, ex_extra = _launch(b, d)
    assert torch.equal(tc.output_bits(b, after, extra), tc.output_bits(b, ex_after, ex_extra)), f"ws_{entry} differs from the _ex entry with causal = 0"
    _note(c, worst)


# ------------------------------------------------------------------------------------------------------------
# composed
# ------------------------------------------------------------------------------------------------------------
def _mk(entry, spec, ins, outs, extras=()):
    """A hand-built case: operands `ins` (name -> values), outputs `outs` (name -> floats), the wrapper's `extras`."""
    b = tc.TBuilt(Case(entry, "chain", {}, ("composed",), 0))
    b.spec.update(spec)
    for k, v in ins.items():
        mc._input(b, k, v, NAN)
    for k, n in outs.items():
        mc._output(b, k, n)
    b.extras += list(extras)
    return b


def _stage(d, entry, spec, ins, outs, extras=()):
    """One stage of a chain through the single entry, checked against the reference at exactly these operands.  Returns (worst
    ratio, name -> what the call left, the reference)."""
    b = _mk(entry, spec, ins, outs, extras)
    ref = tc.reference(b)
    after, extra = _launch(b, d)
    worst = tc.verify(b, ref, after, extra, what=f"chain {entry}")
    left = {k: after[k][b.start[k]:][:n] for k, n in outs.items()}
    left.update(extra)
    return worst, left, ref


@pytest.mark.parametrize("R,Tp,C,P,dil,causal,splits", [(3, 7, 24, 3, 2, 0, (5, 5)), (2, 53, 260, 5, 8, 1, (36, 3)), (1, 2, 1028, 3, 1, 0, (4, 1))])
def test_chain_gln_backward_of_a_conv1d_block(R, Tp, C, P, dil, causal, splits):
    """dwconv_ex_bwd -> chan_sums -> norm_ab -> norm_bwd_apply_cl as functional_tasnet composes the gLN backward."""
    d = _cuda()
    g = torch.Generator().manual_seed(2100 + C)
    M = R * Tp
    x = torch.randn(M, C, generator=g) + 0.5
    st = tc._stats_of(x, R).float()
    gamma, beta, w, dy = torch.randn(C, generator=g) + 1.0, torch.randn(C, generator=g), torch.randn(C, P, generator=g), torch.randn(M, C, generator=g)
    geo = dict(R=R, Tp=Tp, C=C, P=P, dil=dil, st_div=Tp, causal=bool(causal), nsplit=splits[0], rps=splits[1])
    w1, o1, _ = _stage(d, "dwconv_bwd", geo, dict(dy=dy, x=x, stats=st, gamma=gamma, beta=beta, w=w), dict(dxn=M * C), ("slab", "dw", "db"))
    w2, o2, _ = _stage(d, "chan_sums", dict(C=C, rpg=Tp, ng=R, nsplit=3, mode="gxs", st_div=Tp), dict(g=o1["dxn"], x=x, stats=st), {}, ("slab", "sums"))
    w3, o3, _ = _stage(d, "norm_ab", dict(C=C, ng=R, npg=Tp * C), dict(sums=o2["sums"], gamma=gamma), dict(ab=2 * R))
    w4, _, _ = _stage(d, "norm_bwd_apply", dict(rows=M, C=C, st_div=Tp, res=0), dict(x=x, dxn=o1["dxn"], stats=st, ab=o3["ab"], gamma=gamma), dict(dx=M * C))
    worst = max(w1, w2, w3, w4)
    print(f"gLN backward R{R} Tp{Tp} C{C} P{P}: worst err / bound {worst:.3f}")
    _note(Case("chain", f"gln-{R}-{Tp}-{C}-{P}", {}, (), 0), worst, ("composed",))


@pytest.mark.parametrize("M,C,nsplit,res", [(257, 12, 5, 1), (3, 1028, 4, 0), (33, 256, 3, 1)])
def test_chain_bn_stats_prelu_and_backward(M, C, nsplit, res):
    d = _cuda()
    g = torch.Generator().manual_seed(2200 + C)
    x, du = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    gamma, beta = torch.randn(C, generator=g) + 1.0, torch.randn(C, generator=g)
    w1, o1, _ = _stage(d, "bn_stats", dict(M=M, C=C, nsplit=nsplit, run=0), dict(x=x), dict(stats=2 * C))
    ins = dict(x=x, stats=o1["stats"], gamma=gamma, beta=beta, a=torch.tensor([0.25]))
    if res:
        ins["res"] = torch.randn(M, C, generator=g)
    w2, _, _ = _stage(d, "bn_prelu_fwd", dict(M=M, C=C, res=res), ins, dict(u=M * C, y=M * C))
    w3, _, _ = _stage(d, "bn_bwd", dict(M=M, C=C, nsplit=nsplit), dict(x=x, stats=o1["stats"], gamma=gamma, du=du), dict(dx=M * C), ("slab", "sums"))
    worst = max(w1, w2, w3)
    print(f"bn chain M{M} C{C}: worst err / bound {worst:.3f}")
    _note(Case("chain", f"bn-{M}-{C}", {}, (), 0), worst, ("composed",))


@pytest.mark.parametrize("L,hop,Tp,Tout", [(80, 10, 41, 480), (5, 2, 41, 83), (3, 5, 7, 33)])
def test_adjoint_identity_of_the_overlap_add(L, hop, Tp, Tout):
    """<ola_fwd(f), e> = <f, ola_bwd(e)> without bias, in float64 accumulation within the summed bounds of the two sides."""
    d = _cuda()
    R = 2
    g = torch.Generator().manual_seed(2300 + L)
    f, e = torch.randn(R * Tp * L, generator=g), torch.randn(R * Tout, generator=g)
    sp = dict(R=R, Tp=Tp, L=L, hop=hop, Tout=Tout, bias=0)
    w1, o1, r1 = _stage(d, "ola_fwd", sp, dict(frames=f), dict(est=R * Tout))
    w2, o2, r2 = _stage(d, "ola_bwd", sp, dict(dest=e), dict(dframes=R * Tp * L))
    lhs, rhs = (o1["est"].double() * e.double()).sum(), (f.double() * o2["dframes"].double()).sum()
    tol = (r1["est"].bound * e.double().abs()).sum() + (r2["dframes"].bound * f.double().abs()).sum()
    assert abs(float(lhs - rhs)) <= float(tol), (float(lhs - rhs), float(tol))
    _note(Case("chain", f"ola-{L}-{hop}", {}, (), 0), max(w1, w2), ("composed",))


@pytest.mark.parametrize("R,Tp,C,P,dil,causal", [(3, 7, 24, 3, 2, 0), (2, 53, 260, 7, 8, 1), (2, 53, 40, 5, 1, 0)])
def test_adjoint_identity_of_the_depthwise_convolution(R, Tp, C, P, dil, causal):
    """<dwconv_fwd(x) - b, g> = <xn, dwconv_bwd's dxn(g)> in float64 accumulation within the summed bounds of the two sides."""
    d = _cuda()
    g = torch.Generator().manual_seed(2400 + C)
    M = R * Tp
    x = torch.randn(M, C, generator=g) + 0.5
    st = tc._stats_of(x, R).float()
    gamma, beta, w, bias = (torch.randn(C, generator=g) + 1.0, torch.randn(C, generator=g), torch.randn(C, P, generator=g), torch.randn(C, generator=g))
    gy = torch.randn(M, C, generator=g)
    geo = dict(R=R, Tp=Tp, C=C, P=P, dil=dil, st_div=Tp, causal=bool(causal), nsplit=1, rps=M)
    ops = dict(x=x, stats=st, gamma=gamma, beta=beta, w=w)
    w1, o1, r1 = _stage(d, "dwconv_fwd", geo, dict(ops, b=bias), dict(y=M * C))
    w2, o2, r2 = _stage(d, "dwconv_bwd", geo, dict(ops, dy=gy), dict(dxn=M * C), ("slab", "dw", "db"))
    b = _mk("dwconv_fwd", geo, dict(ops, b=bias), {})
    xn, _ = tc._xn(geo, b.views(b.bufs), F64)
    lhs = ((o1["y"].double().reshape(M, C) - bias.double()) * gy.double()).sum()
    rhs = (xn * o2["dxn"].double().reshape(M, C)).sum()
    tol = (r1["y"].bound.reshape(M, C) * gy.double().abs()).sum() + (r2["dxn"].bound.reshape(M, C) * xn.abs()).sum()
    assert abs(float(lhs - rhs)) <= float(tol), (float(lhs - rhs), float(tol))
    _note(Case("chain", f"dwconv-{Tp}-{C}-{P}", {}, (), 0), max(w1, w2), ("composed",))


def test_invalid_argument_sets_are_refused_and_launch_nothing():
    """Every refusal raises (the return code), and the tensor it was handed is untouched afterwards."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    t = torch.full((1 << 16,), SENT, device=d)
    for name, call in tc.refusals(dev, t, d):
        with pytest.raises(L.WesepHipError):
            call()
        torch.cuda.synchronize()
        assert bool((t == SENT).all()), f"{name}: the refused call wrote"


def test_zz_write_worst_ratios():
    """Last in the file: the case count, the worst err / bound and the case that gave it, per instantiation ->
    $WESEP_TEST_OUT/tasnet_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "tasnet_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1], "worst_case": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
