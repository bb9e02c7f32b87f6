"""Contract sweep of the generic GEMM family on the GPU (tests/gemm_contract.py): every generated case goes through the
C ABI (wesep_amd.dev -> libwesep_hip.so) inside guarded allocations and is held, element by element, against the float64
restatement of include/wesep_hip.h:
  - |out - ref| <= eps * S' for every element of the write set (the derived bound of gemm_contract's docstring);
  - exact equality where a mask says zero (ReLU derivative, clearly negative ReLU input);
  - no NaN left in the write set (it starts as NaN);
  - every other element of the output allocation bit-identical to the sentinel it held (row padding, the columns
    between strided blocks, the guards);
  - a second launch into fresh buffers gives the same bits.
TN / conv_wgrad results are checked per split slab and once more after dev.reduce_slabs; every conv_wgrad case also runs
through ws_gemm_tn with conv.on.  The last test writes the worst err / bound per kernel instantiation to
gemm_contract.json in the directory $WESEP_TEST_OUT (default: the system's temporary directory); profiles/gemm_contract.md
holds the figures of the run this file was added with.

What the case list pins, by construction (the kernels are not broken on a shared machine to demonstrate it):
  - the `vm && vk && vt` select of gemm_nt_bf16_kernel::store_tile: the loads are unconditional with clamped addresses,
    the select is what makes them contribute zero.  Without `vk` the float4s behind K of the last k-tile (K % 32 != 0:
    K = 4, 28, 36, 100, 132 and most k*k*C) repeat columns 0..3 of the row against columns 0..3 of W -- whole products too
    many; without `vt` a masked tap contributes pixel (0, 0) -- every mode-0 case with p > 0 and every mode-1 case
    differs far outside the bound; `vm` alone only guards accumulator rows the epilogue never stores: rows >= M are
    covered by the sentinel check instead (M = 1, 31, 33, 127, 129, 257, 1001);
  - the `(hn & csh) == 0` test of mode 1: every mode-1 case with sh = 2 or sw = 2 (strides (1,2), (2,1), (2,2) are paired
    with every k, dil, p, C, ldp and image) has odd hn / wn whose halved index lies inside the image;
  - the `avalid` masking of gemm_tn_bf16_kernel: every shift case (+-1, +-10) in split-bf16 mode has sequences whose
    first / last step must contribute zero while row m + shift_rows holds finite data of the neighbouring sequence;
  - the `n < Nn` guard of conv_wgrad_kernel's store: Nn = 4, 8, 16 leave accumulator rows 4..31 / 8..31 / 16..31 whose
    store would land in rows n >= Nn of the slab = the next split's slab or the sentinel guard behind the last one."""
import json
import os
import tempfile

import pytest
import torch

from tests import gemm_contract as gc

pytestmark = pytest.mark.gpu

WORST = {}     # instantiation -> [worst err / bound, cases]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _note(case, ratio):
    for t in case.targets:
        w = WORST.setdefault(t, [0.0, 0])
        w[0] = max(w[0], ratio)
    return ratio


def _count(case):
    for t in case.targets:
        WORST.setdefault(t, [0.0, 0])[1] += 1


def _launch(case, b, d, entry=None, remap=None):
    """One launch into fresh device buffers; returns the output allocations (CPU) and the device tensors."""
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    kw = b.kwargs(t, d)
    if remap is not None:
        kw = remap(kw)
    getattr(dev, entry or case.entry)(**kw)
    torch.cuda.synchronize()
    return {n: t[n].cpu() for n in b.outs}, t, kw


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _check_all(case, b, ref, outs, what):
    worst = 0.0
    for key, name in b.out_keys.items():
        worst = max(worst, gc.check(outs[name], b.bufs[name], ref[key], f"{what} {key}", b.base(name)))
    return worst


def _check_reduced(case, b, ref, t, d, nsplit, strides):
    """dev.reduce_slabs over the splits of every group's block, against the summed reference."""
    from wesep_amd import dev
    worst, pos = 0.0, {"slab": 0, "bslab": 0}
    for (oo, cnt, bo, nn) in b.blocks:
        for key, off, n in (("slab", oo, cnt), ("bslab", bo, nn)):
            if key not in ref:
                continue
            r = ref[key]
            piece = gc.Ref(*[x[pos[key]:pos[key] + nsplit * n] for x in r[:5]])
            pos[key] += nsplit * n
            red = gc.reduced(piece, nsplit)
            out = torch.full((n + 2 * gc.GUARD,), gc.SENT, device=d)
            before = out.cpu()
            before[gc.GUARD:gc.GUARD + n] = float("nan")
            out.copy_(before)
            src = t[b.out_keys[key]][b.base(b.out_keys[key]) + off:]
            dev.reduce_slabs(src, nsplit, strides[key], n, out, out_off=gc.GUARD)
            torch.cuda.synchronize()
            worst = max(worst, gc.check(out, before, red, f"{case.name} reduced {key}", gc.GUARD))
    return worst


def _run(case):
    d = _cuda()
    b = gc.build(case)
    ref = gc.reference(b)
    _count(case)
    outs, t, kw = _launch(case, b, d)
    worst = _check_all(case, b, ref, outs, case.name)
    if case.entry in ("gemm_tn", "conv_wgrad"):
        nn, kk = b.blocks[0][3], b.blocks[0][1] // b.blocks[0][3]
        strides = ({"slab": kw["slab_stride"], "bslab": kw.get("bslab_stride", 0)} if case.entry == "gemm_tn"
                   else {"slab": nn * kk, "bslab": nn})
        worst = max(worst, _check_reduced(case, b, ref, t, d, kw["nsplit"], strides))
    outs2, _, _ = _launch(case, b, d)
    for n in b.outs:
        assert _same_bits(outs[n], outs2[n]), f"{case.name}: {n} differs between two launches"
    if case.entry == "conv_wgrad":      # the same arguments through ws_gemm_tn with conv.on
        outs3, _, _ = _launch(case, b, d, entry="gemm_tn", remap=gc.wgrad_as_gemm_tn)
        worst = max(worst, _check_all(case, b, ref, outs3, case.name + " via gemm_tn"))
    _note(case, worst)


@pytest.mark.parametrize("case", gc.cases("gemm_nt"), ids=lambda c: c.name)
def test_gemm_nt_contract(case):
    _run(case)


@pytest.mark.parametrize("case", gc.cases("gemm_tn"), ids=lambda c: c.name)
def test_gemm_tn_contract(case):
    _run(case)


@pytest.mark.parametrize("case", gc.cases("conv_wgrad"), ids=lambda c: c.name)
def test_conv_wgrad_contract(case):
    _run(case)


@pytest.mark.parametrize("case", gc.cases("reduce_slabs"), ids=lambda c: c.name)
def test_reduce_slabs_contract(case):
    _run(case)


def test_conv_wgrad_above_64_kb_of_lds_on_two_devices():
    """k = 3, C = 80 takes 122 880 bytes of dynamic LDS: the function's limit has to be raised on EVERY device that launches
    it, not once per process.  The same case on device 0 and then on device 1, both held to the reference."""
    _cuda()
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    dims = dict(Nn=16, ldg="Nn", split="one", bias=1, k=3, stride=(1, 1), dil=1, p="k/2", C=80, ldp="0", img="3x5")
    case = gc.Case("conv_wgrad", "two-devices-k3-C80-Nn16", dims, (gc.WG_INST[0],), 4242)
    b = gc.build(case)
    ref = gc.reference(b)
    for i in (0, 1):
        d = torch.device(f"cuda:{i}")
        with torch.cuda.device(d):
            outs, _, _ = _launch(case, b, d)
        assert _check_all(case, b, ref, outs, f"{case.name} on device {i}") <= 1.0


def test_zz_write_worst_ratios():
    """Last in the file: the worst err / bound and the case count per instantiation -> $WESEP_TEST_OUT/gemm_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "gemm_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
