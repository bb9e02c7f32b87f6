"""Contract sweep of the normalisation kernels on the GPU (tests/norm_contract.py): every generated case goes through
wesep_amd.dev -> libwesep_hip.so (ws_group_stats, ws_group_stats_len, ws_gn_bwd_reduce, ws_gn_bwd_apply, ws_gn_param_grad,
ws_gn_bwd_apply_pg, ws_gn_bwd_fused2, ws_rowln_fwd, ws_rowln_bwd, ws_flat_stats, ws_flat_stats_len) inside guarded allocations
and is held against the float64 gather that restates include/wesep_hip.h:
  - every element of a write set inside its bound, rstd inside its interval (norm_contract's docstring derives both); outputs
    whose split assignment the header leaves open (ws_gn_param_grad slabs, pslab, the rowln_bwd slab) as float64 sums over
    the splits / workgroups; pout and the [2, W] sum dev.rowln_bwd returns once more against the rows the kernel left;
  - exact zeros in the slabs of splits that own no group and in the columns [band_w[b], W);
  - no NaN left in a write set (it starts as NaN; dx aliasing dxn / dy: as that operand); the counter words zero;
  - every other word of every output allocation bit-identical to its sentinel: gaps between bands, row tails up to rs, rows of
    other groups, guards, everything behind stats / ab / slabs / pout (the ceil(nwg / 32) scratch rows of pslab excepted);
  - a second launch into fresh buffers gives the same bits;
  - large finite garbage instead of the NaN poison in everything the contract does not read -- rows behind glen, columns
    outside the bands, gamma beyond the band's width, guards -- leaves the outputs unchanged to the bit.
The composed cases chain group_stats -> gn_bwd_reduce -> gn_bwd_apply (+ gn_param_grad), and group_stats -> gn_bwd_fused
where the geometry allows it, each stage fed the device output of the one before and checked against the reference
evaluated at those inputs.  The last test writes the case count and the worst err / bound per instantiation to
norm_contract.json in the directory $WESEP_TEST_OUT (default: the system's temporary directory); profiles/norm_contract.md
is where the figures of a run are recorded.  No case passes arguments a valid caller could not, and no kernel is broken to
show a catch: tests/test_norm_contract_host_cpu.py plants the defects into reference outputs."""
import json
import os
import tempfile

import pytest
import torch

from tests import gemm_contract as gc
from tests import norm_contract as nc

pytestmark = pytest.mark.gpu

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


def _launch(b, d, entry=None, bufs=None):
    """One launch into fresh device buffers; returns every allocation (CPU), what the call left outside them (CPU) and the
    device tensors."""
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in (bufs or b.bufs).items()}
    extra = nc.run(dev, b, t, d, entry)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in t.items()}, {k: v.cpu() for k, v in extra.items()}, t


def _run(case):
    d = _cuda()
    b = nc.build(case)
    ref = nc.reference(b)
    after, extra, _ = _launch(b, d)
    worst = nc.verify(b, ref, after, extra)
    after2, extra2, _ = _launch(b, d)
    assert torch.equal(nc.output_bits(b, after, extra), nc.output_bits(b, after2, extra2)), f"{case.name}: two launches differ"
    bg = nc.build(case, garbage=True)
    afterg, extrag, _ = _launch(bg, d)
    assert torch.equal(nc.output_bits(b, after, extra), nc.output_bits(bg, afterg, extrag)), \
        f"{case.name}: garbage outside the contract reached the output"
    print(f"{case.entry} {case.name}: worst err / bound {worst:.3f}")
    _note(case, worst)


@pytest.mark.parametrize("case", nc.cases("group_stats"), ids=lambda c: c.name)
def test_group_stats_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("gn_bwd_reduce"), ids=lambda c: c.name)
def test_gn_bwd_reduce_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("gn_bwd_apply"), ids=lambda c: c.name)
def test_gn_bwd_apply_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("gn_param_grad"), ids=lambda c: c.name)
def test_gn_param_grad_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("gn_bwd_apply_pg"), ids=lambda c: c.name)
def test_gn_bwd_apply_pg_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("gn_bwd_fused"), ids=lambda c: c.name)
def test_gn_bwd_fused_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("rowln_fwd"), ids=lambda c: c.name)
def test_rowln_fwd_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("rowln_bwd"), ids=lambda c: c.name)
def test_rowln_bwd_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("flat_stats"), ids=lambda c: c.name)
def test_flat_stats_contract(case):
    _run(case)


@pytest.mark.parametrize("case", nc.cases("flat_stats_len"), ids=lambda c: c.name)
def test_flat_stats_len_contract(case):
    _run(case)


def _stage(b, d, entry, bufs, outs, spec=None):
    """One stage of a chain: `entry` over `bufs` (CPU allocations; `outs`: name -> (floats, write set) of fresh outputs),
    checked against the reference evaluated at exactly these inputs.  Returns (worst ratio, the allocations afterwards)."""
    keep = (dict(b.bufs), dict(b.start), list(b.outs), dict(b.spec))
    try:
        b.bufs, b.outs = dict(bufs), []
        b.spec.update(spec or {})
        for name, (n, widx) in outs.items():
            nc._out(b, name, n, widx, b.start["x"] if name == "dx" else gc.GUARD)
        ref = nc.reference(b, entry=entry)
        after, extra, _ = _launch(b, d, entry)
        return nc.verify(b, ref, after, extra, what=f"{b.case.name} {entry}"), after
    finally:
        b.bufs, b.start, b.outs, b.spec = keep[0], keep[1], keep[2], keep[3]


@pytest.mark.parametrize("case", nc.cases(nc.COMPOSED), ids=lambda c: c.name)
def test_the_chain_composed_as_the_models_run_it(case):
    """group_stats -> gn_bwd_reduce -> gn_bwd_apply (+ gn_param_grad), and group_stats -> gn_bwd_fused where the geometry is
    the fused kernel's: every stage reads the DEVICE output of the one before."""
    d = _cuda()
    b = nc.build(case)
    geo = b.spec["geo"]
    ng = geo["ngroups"]
    widx = torch.cat([nc.group_index(geo, g)[0].reshape(-1) for g in range(ng)])
    ins = {k: v for k, v in b.bufs.items() if k in ("x", "dxn", "gamma", "res")}
    all2 = torch.arange(2 * ng)
    r0, a = _stage(b, d, "group_stats", {"x": ins["x"]}, {"stats": (2 * ng, all2)})
    stats = torch.full_like(b.bufs["stats"], float("nan"))
    stats[gc.GUARD:gc.GUARD + 2 * ng] = a["stats"][gc.GUARD:gc.GUARD + 2 * ng]
    r1, a = _stage(b, d, "gn_bwd_reduce", dict(ins, stats=stats), {"ab": (2 * ng, all2)})
    ab = torch.full_like(b.bufs["ab"], float("nan"))
    ab[gc.GUARD:gc.GUARD + 2 * ng] = a["ab"][gc.GUARD:gc.GUARD + 2 * ng]
    r2, _ = _stage(b, d, "gn_bwd_apply", dict(ins, stats=stats, ab=ab), {"dx": (geo["span"], widx)})
    worst = [("group_stats", r0), ("gn_bwd_reduce", r1), ("gn_bwd_apply", r2)]
    if geo["W"] <= 128 and ng % geo["nbands"] == 0:
        n = 2 * geo["nbands"] * 2 * geo["W"]
        r3, _ = _stage(b, d, "gn_param_grad", dict(ins, stats=stats), {"slab": (n, torch.arange(n))}, {"nsplit": 2})
        worst.append(("gn_param_grad", r3))
    if geo["nbands"] == 1 and geo["W"] == 128 and geo["L"] % 2 == 0 and geo["L"] <= 32 and nc.geom_vec4(geo):
        nwg = -(-ng // 4)
        r4, _ = _stage(b, d, "gn_bwd_fused", dict(ins, stats=stats),
                       {"dx": (geo["span"], widx), "pslab": ((nwg + 1) * 256 + 64, torch.arange(nwg * 256)), "pout": (256, torch.arange(256))},
                       {"nwg": nwg, "pout": 1, "counter": 2})
        worst.append(("gn_bwd_fused", r4))
    print(f"{case.name}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst))
    _note(case, max(v for _, v in worst), ("composed",))
    assert max(v for _, v in worst) <= 1.0


def test_invalid_argument_sets_are_refused_and_launch_nothing():
    """Every refusal raises, and the output tensor it was handed is untouched afterwards."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    t = torch.full((1 << 16,), gc.SENT, device=d)
    for name, call in nc.refusals(dev, t, d):
        with pytest.raises(L.WesepHipError):
            call()
        torch.cuda.synchronize()
        assert bool((t == gc.SENT).all()), f"{name}: the refused call wrote"


def test_zz_write_worst_ratios():
    """Last in the file: the case count, the worst err / bound and the case that gave it, per instantiation ->
    $WESEP_TEST_OUT/norm_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "norm_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1], "worst_case": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
