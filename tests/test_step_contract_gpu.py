"""Contract sweep of the training-step kernels on the GPU (tests/step_contract.py): every generated case goes through
wesep_amd.dev -> libwesep_hip.so (ws_affine_fwd / bwd, ws_sisdr_fwd / bwd, ws_grad_norms, ws_clip_adam_step, ws_guard_commit,
ws_heads_fwd / bwd, ws_tstp_bwd) inside guarded allocations and is held against the float64 index arithmetic that restates
include/wesep_hip.h:
  - every element of a write set inside its bound, the SI-SDR row statistics and rstd inside their intervals (step_contract's
    docstring derives them), every slab as float64 sums over its splits / workgroups; bit-exact where the contract is one fma,
    an integer, or "untouched": a skipped or clip_only launch, a NULL-grad entry, a gradient with coef == 1, the padded frames of
    heads_fwd, the slab rows of splits and workgroups that own nothing;
  - no NaN left in a write set (it starts as NaN; an output that aliases an operand: as that operand);
  - every other word of every output allocation bit-identical to its sentinel: the columns of dx outside the heads, guards;
  - a second launch into fresh buffers gives the same bits;
  - large finite garbage instead of the NaN poison in everything the contract does not read leaves the outputs unchanged.
Composed: sisdr_fwd -> sisdr_bwd on the device's own rowstat against the float64 gradient of the loss; grad_norms ->
clip_adam_step -> guard_commit over three steps with a poisoned gradient in the middle one.  The last test writes the case count
and the worst err / bound per instantiation to step_contract.json in the directory $WESEP_TEST_OUT (default: the system's
temporary directory); profiles/step_contract.md records the figures of a run.  No case passes arguments a valid caller could
not, and no kernel is broken to show a catch: tests/test_step_contract_host_cpu.py plants the defects into the emulation."""
import json
import os
import tempfile

import pytest
import torch

from oracle import bsrnn_oracle as orc
from tests import map_contract as mc
from tests import step_contract as sc
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


def _launch(b, d):
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    extra = sc.run(dev, b, t, d)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in t.items()}, {n: v.cpu() for n, v in extra.items()}


def _run(case):
    d = _cuda()
    b = sc.build(case)
    ref = sc.reference(b)
    after, extra = _launch(b, d)
    worst = sc.verify(b, ref, after, extra)
    bits = sc.output_bits(b, after, extra)
    assert torch.equal(bits, sc.output_bits(b, *_launch(b, d))), f"{case.name}: two launches differ"
    if "affine_fwd[grid cap]" not in case.targets:          # (the one case at workload size: two launches are enough)
        bg = sc.build(case, garbage=True)
        assert torch.equal(bits, sc.output_bits(bg, *_launch(bg, d))), f"{case.name}: garbage outside the contract reached the output"
    print(f"{case.entry} {case.name}: worst err / bound {worst:.3f}")
    _note(case, worst)
    return b, ref, after, extra


def _sweep(entry):
    return pytest.mark.parametrize("case", sc.cases(entry), ids=lambda c: c.name)


@_sweep("affine_fwd")
def test_affine_fwd_contract(case):
    _run(case)


@_sweep("affine_bwd")
def test_affine_bwd_contract(case):
    _run(case)


@_sweep("sisdr_fwd")
def test_sisdr_fwd_contract(case):
    b, _, after, _ = _run(case)
    assert bool(torch.isfinite(b.views(after)["rowstat"][:b.spec["R"] * 8]).all()), f"{case.name}: a row statistic is not finite"


@_sweep("sisdr_bwd")
def test_sisdr_bwd_contract(case):
    _run(case)


@_sweep("grad_norms")
def test_grad_norms_contract(case):
    _run(case)


@_sweep("clip_adam_step")
def test_clip_adam_step_contract(case):
    _run(case)


@_sweep("guard_commit")
def test_guard_commit_contract(case):
    _run(case)


@_sweep("heads_fwd")
def test_heads_fwd_contract(case):
    _run(case)


@_sweep("heads_bwd")
def test_heads_bwd_contract(case):
    _run(case)


@_sweep("tstp_bwd")
def test_tstp_bwd_contract(case):
    _run(case)


# ------------------------------------------------------------------------------------------------------------
# composed
# ------------------------------------------------------------------------------------------------------------
def _mk(entry, spec, ins, outs, extras=(), inplace=()):
    """A hand-built case: operands `ins` (name -> values), outputs `outs` (name -> floats), operands written `inplace`."""
    b = sc.TBuilt(Case(entry, "chain", {}, ("composed",), 0))
    b.spec.update(spec)
    for k, v in ins.items():
        mc._input(b, k, v, NAN)
    for k, n in outs.items():
        mc._output(b, k, n)
    for k in inplace:
        mc._alias(b, k, k, torch.arange(b.size[k]))
    b.extras += list(extras)
    return b


@pytest.mark.parametrize("R,T,regime,gout", [(3, 1025, "10dB", -2.5), (65, 63, "30dB", 1.0), (2, 2048, "-5dB", 0.5)])
def test_chain_sisdr_forward_and_backward_against_the_float64_gradient(R, T, regime, gout):
    """sisdr_bwd on the rowstat the device's sisdr_fwd left.  Judged twice: at exactly those fp32 operands (the entry's own
    bound), and against autograd on the float64 loss with the forward's derived intervals carried to first order:
    |d dest| <= |go| (D_c1 |tc| + |c1| D_mt + D_c2 |res| + |c2| (D_mx + D_alpha |tc| + |alpha| D_mt)), D = the distance of a row
    statistic from its float64 value that the interval allows (x 1.01 for the second-order terms)."""
    d = _cuda()
    g = torch.Generator().manual_seed(3100 + T)
    x, tg, eps = sc.sisdr_data(g, R, T, regime)
    sp = dict(R=R, T=T, eps=eps, regime=regime)
    b1 = _mk("sisdr_fwd", sp, dict(est=x, tgt=tg), dict(rowstat=R * 8, loss=1))
    r1 = sc.reference(b1)
    a1, _ = _launch(b1, d)
    w1 = sc.verify(b1, r1, a1, {}, what="chain sisdr_fwd")
    rowstat = b1.views(a1)["rowstat"]
    b2 = _mk("sisdr_bwd", sp, dict(est=x, tgt=tg, rowstat=rowstat, gout=torch.tensor([gout])), dict(dest=R * T))
    r2 = sc.reference(b2)
    a2, _ = _launch(b2, d)
    w2 = sc.verify(b2, r2, a2, {}, what="chain sisdr_bwd")
    xd = x.double().requires_grad_(True)
    loss = orc.sisdr_loss(xd, tg.double(), float(sc._f32(eps)))
    want = torch.autograd.grad(loss * gout, xd)[0]
    rs = sc.compute("sisdr_fwd", sp, b1.views(b1.bufs), F64)["rowstat"]
    D = (r1["rowstat"].val.reshape(R, 8) - rs).abs() + r1["rowstat"].bound.reshape(R, 8)
    tcn = tg.double() - rs[:, 1:2]
    res = (x.double() - rs[:, 0:1]) - rs[:, 2:3] * tcn
    go = abs(gout) / R
    tol = r2["dest"].bound.reshape(R, T) + 1.01 * go * (D[:, 3:4] * tcn.abs() + rs[:, 3:4].abs() * D[:, 1:2] + D[:, 4:5] * res.abs() + rs[:, 4:5].abs() * (
        D[:, 0:1] + D[:, 2:3] * tcn.abs() + rs[:, 2:3].abs() * D[:, 1:2]))
    err = (b2.views(a2)["dest"].double().reshape(R, T) - want).abs()
    ratio = float((err / tol).max())
    print(f"sisdr chain R{R} T{T} {regime}: stages {w1:.3f} {w2:.3f}, against the float64 gradient {ratio:.3f}; loss {float(b1.views(a1)['loss'][0]):.6f} "
          f"vs {float(loss):.6f}")
    assert ratio <= 1.0
    _note(Case("chain", f"sisdr-{R}-{T}-{regime}", {}, (), 0), max(w1, w2, ratio), ("composed",))


def test_chain_three_optimizer_steps_with_a_poisoned_one_in_the_middle():
    """grad_norms -> clip_adam_step -> guard_commit as FusedClipAdam issues them, three steps, the second with an Inf in one
    gradient: that step leaves weights and moments to the bit and is counted in guard[1..3]; the third step's bias corrections
    are those of step 2 (step - lag).  Every launch is judged by the entry's own reference at the operands it met."""
    from wesep_amd import dev
    d = _cuda()
    g = torch.Generator().manual_seed(3200)
    numel = [4097, 300, 7]
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4, clip_only=0, skip1=None, null=-1, numel=numel)
    state = {}
    for i, n in enumerate(numel):
        state[f"p{i}"], state[f"m{i}"], state[f"v{i}"] = torch.randn(n, generator=g), torch.zeros(n), torch.zeros(n)
    guard = torch.zeros(4, dtype=torch.int32, device=d)
    worst = 0.0
    for step in (1, 2, 3):
        grads = {f"g{i}": torch.randn(n, generator=g) * (0.1 * 3 ** i) for i, n in enumerate(numel)}
        poisoned = step == 2
        if poisoned:
            grads["g1"][11] = float("inf")
        # grad_norms at these gradients
        bn = _mk("grad_norms", dict(numel=numel, null=-1, guard=0, poison="inf" if poisoned else "none", nonfinite=[1] if poisoned else []),
                 grads, dict(norms=len(numel)), ("guard",))
        tn = {k: v.clone().to(d) for k, v in bn.bufs.items()}
        vn = bn.views(tn)
        guard[0] = 0
        g_before = guard.cpu().tolist()
        dev.grad_norms(sc._table([((vn["norms"], vn[f"g{i}"], None, None), n) for i, n in enumerate(numel)], d), len(numel), vn["norms"], guard)
        torch.cuda.synchronize()
        after = {k: v.cpu() for k, v in tn.items()}
        rn = sc.reference(bn)
        rn["guard"] = sc._exact(torch.tensor([1 if poisoned else 0] + g_before[1:], dtype=F64))
        worst = max(worst, sc.verify(bn, rn, after, {"guard": guard.cpu().float()}, what=f"step {step} grad_norms"))
        norms = bn.views(after)["norms"].clone()
        clip = float(sc._f32(float(norms[0]) * 0.5)) if not poisoned else 1.0          # half the first norm: clips the tensors above it, leaves the smallest untouched
        lag = int(guard[3])
        spec = dict(hyper, step=step, lag=lag, skip0=int(guard[0]), clip=clip)
        ins = dict(state, **grads, norms=torch.nan_to_num(norms, nan=0.0, posinf=3e38))
        ba = _mk("clip_adam_step", spec, ins, {}, ("skip0", "lag"), inplace=[f"{k}{i}" for i in range(len(numel)) for k in "pgmv"])
        ta = {k: v.clone().to(d) for k, v in ba.bufs.items()}
        va = ba.views(ta)
        tab = sc._table([((va[f"p{i}"], va[f"g{i}"], va[f"m{i}"], va[f"v{i}"]), n) for i, n in enumerate(numel)], d)
        dev.clip_adam_step(tab, len(numel), va["norms"], clip, hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"], hyper["wd"], step,
                           skip=(guard[0:1], None), step_lag=guard[3:4])
        dev.guard_commit(guard)
        torch.cuda.synchronize()
        after = {k: v.cpu() for k, v in ta.items()}
        ra = sc.reference(ba)
        worst = max(worst, sc.verify(ba, ra, after, {"skip0": torch.tensor([float(spec["skip0"])]), "lag": torch.tensor([float(lag)])},
                                     what=f"step {step} clip_adam_step"))
        left = ba.views(after)
        if poisoned:
            for k in state:
                assert torch.equal(left[k].view(torch.int32), state[k].view(torch.int32)), f"the poisoned step changed {k}"
        state = {k: left[k].clone() for k in state}
    assert guard.cpu().tolist() == [0, 1, 0, 1], guard.cpu().tolist()          # one step skipped, none in a row at the end, lag 1
    assert sc._adam_scalars(dict(hyper, step=3, lag=1))[:2] == sc._adam_scalars(dict(hyper, step=2, lag=None))[:2]
    print(f"optimizer chain: worst err / bound {worst:.3f}")
    _note(Case("chain", "optimizer-3-steps", {}, (), 0), worst, ("composed",))


def test_invalid_argument_sets_are_refused_and_launch_nothing():
    """Every refusal raises (the return code), and the tensor it was handed is untouched afterwards."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    t = torch.full((1 << 16,), SENT, device=d)
    for name, call in sc.refusals(dev, t, d):
        with pytest.raises(L.WesepHipError):
            call()
        torch.cuda.synchronize()
        assert bool((t == SENT).all()), f"{name}: the refused call wrote"


def test_zz_write_worst_ratios():
    """Last in the file: the case count, the worst err / bound and the case that gave it, per instantiation ->
    $WESEP_TEST_OUT/step_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "step_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1], "worst_case": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
