"""Contract sweep of the 3 x 3 halo convolutions on the GPU (tests/conv3x3_contract.py): every generated case goes through the
C ABI (wesep_amd.dev -> libwesep_hip.so: ws_conv3x3_pack, ws_conv3x3, ws_conv3x3_wgrad) inside guarded allocations and is held,
element by element, against the float64 gather that restates include/wesep_hip.h:
  - |out - ref| <= eps_for(True, K) * S + 2^-24 |R| for every element of the write set (bslab: eps_for(False, K));
  - exact zeros in every slab and bslab of a split that owns no tile; the weight pack bit for bit;
  - no NaN left in a write set (it starts as NaN; with R aliasing Y as the residual);
  - every other word of every output allocation bit-identical to the sentinel it held: ldy tails, the columns outside
    [y_off, y_off + Cout), slab rows behind Nn*9*Cin up to slab_stride, bslab behind Nn, the floats behind
    conv3x3_pack_floats, the guards;
  - a second launch into fresh buffers gives the same bits;
  - with large finite garbage instead of the NaN poison in everything the contract does not read -- X columns outside
    [x_off, x_off + Cin), G columns outside [g_off, g_off + Nn), R outside the write set, the guards -- the outputs do not
    change by a bit.
The weight operand of every forward case is packed on the device by ws_conv3x3_pack from its fp32 matrix.  Weight-gradient
cases are checked per split and once more after dev.reduce_slabs.  The last test writes the case count and the worst err / bound
per kernel instantiation to conv3x3_contract.json in the directory $WESEP_TEST_OUT (default: the system's temporary directory);
profiles/conv3x3_contract.md is where the figures of a run are recorded.  No kernel is broken to demonstrate a catch:
tests/test_conv3x3_contract_host_cpu.py plants the defects into reference outputs."""
import json
import os
import tempfile

import pytest
import torch

from tests import conv3x3_contract as cc
from tests import gemm_contract as gc

pytestmark = pytest.mark.gpu

WORST = {}     # instantiation -> [worst err / bound, cases, the case that gave it]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _note(case, ratio):
    for t in case.targets:
        w = WORST.setdefault(t, [0.0, 0, ""])
        if t not in cc.PK3_INST and ratio > w[0]:           # (the pack is compared as bits: it has no ratio)
            w[0], w[2] = ratio, f"{case.entry} {case.name}"
        w[1] += 1


def _launch(b, d):
    """One launch into fresh device buffers; returns every allocation (CPU) and the device tensors."""
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    cc.run(dev, b, t, d)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in t.items()}, t


def _check_reduced(case, b, ref, t, d):
    """dev.reduce_slabs over the splits of slab and bslab, against the summed reference."""
    from wesep_amd import dev
    worst, nsplit = 0.0, b.kw["nsplit"]
    for key, name in b.out_keys.items():
        n = ref[key].idx.numel() // nsplit
        stride = (b.bufs[name].numel() - 2 * gc.GUARD) // nsplit
        out = torch.full((n + 2 * gc.GUARD,), gc.SENT, device=d)
        before = out.cpu()
        before[gc.GUARD:gc.GUARD + n] = float("nan")
        out.copy_(before)
        dev.reduce_slabs(t[name][gc.GUARD:], nsplit, stride, n, out, out_off=gc.GUARD)
        torch.cuda.synchronize()
        worst = max(worst, gc.check(out, before, gc.reduced(ref[key], nsplit), f"{case.name} reduced {key}", gc.GUARD))
    return worst


def _run(case):
    d = _cuda()
    b = cc.build(case)
    ref = cc.reference(b)
    after, t = _launch(b, d)
    worst = cc.verify(b, ref, after)
    if case.entry == "conv3x3_wgrad":
        worst = max(worst, _check_reduced(case, b, ref, t, d))
    after2, _ = _launch(b, d)
    assert torch.equal(cc.output_bits(b, after), cc.output_bits(b, after2)), f"{case.name}: two launches differ"
    if case.entry != "conv3x3_pack":        # the pack of a forward case is an operand here: bit for bit as well
        for p in b.packs:
            pk = cc._pack_kwargs(p, after)
            bits = cc.ref_conv3x3_pack(**cc._pack_kwargs(p, b.bufs))
            assert torch.equal(pk["out"].contiguous().view(torch.int16), bits), f"{case.name}: the weight pack differs from the unit formula"
    bg = cc.build(case, garbage=True)
    afterg, _ = _launch(bg, d)
    assert torch.equal(cc.output_bits(b, after), cc.output_bits(bg, afterg)), f"{case.name}: garbage outside the contract reached the output"
    _note(case, worst)


@pytest.mark.parametrize("case", cc.cases("conv3x3_pack"), ids=lambda c: c.name)
def test_conv3x3_pack_contract(case):
    _run(case)


@pytest.mark.parametrize("case", cc.cases("conv3x3"), ids=lambda c: c.name)
def test_conv3x3_contract(case):
    _run(case)


@pytest.mark.parametrize("case", cc.cases("conv3x3_wgrad"), ids=lambda c: c.name)
def test_conv3x3_wgrad_contract(case):
    _run(case)


@pytest.mark.parametrize("case", cc.cases(cc.COMPOSED), ids=lambda c: c.name)
def test_pack_and_convolution_composed_as_the_dense_block_does(case):
    """A layer's forward from its [co][ci][3][3] weight, and the input gradient of a channel block (two layers' weights side by
    side, flip = 1, X = dY, Y = R) against the float64 gather of the adjoint."""
    _run(case)


def test_zz_write_worst_ratios():
    """Last in the file: the case count, the worst err / bound and the case that gave it, per instantiation ->
    $WESEP_TEST_OUT/conv3x3_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "conv3x3_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1], "worst_case": v[2]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
