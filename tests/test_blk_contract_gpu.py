"""Contract sweep of the blocked-layout GEMM family on the GPU (tests/blk_contract.py): every generated case goes through
the C ABI (wesep_amd.dev -> libwesep_hip.so: ws_pack_w*, ws_gemm_p2b, ws_gemm_p2b_len, ws_gemm_b2p, ws_gemm_tnb) inside guarded
allocations and is held, element by element, against the float64 restatement of include/wesep_hip.h:
  - |out - ref| <= the derived bound of blk_contract's docstring for every element of the write set;
  - exact zeros in padded slots and in the slots a steps[] table cuts off; bit-exact A_bl / A_bl16 (no GroupNorm), a16_out
    and weight packs;
  - amax raised to the maximum of C, never lowered, untouched by a launch predicated off;
  - no NaN left in a write set (it starts as NaN);
  - every other word of every output allocation bit-identical to the sentinel it held: ldc tails, rows of C no slot maps
    to, the eight blocks behind the last block of a BL / BLH buffer (the waves the grid rounds up to), the slab behind
    nsplit, the guards;
  - with run_if pointing at 0 every output allocation, amax included, is bit-identical to its initial state;
  - a second launch into fresh buffers gives the same bits;
  - with large finite garbage in everything the contract does not read (padded slots of A, rows of cut-off steps, unmapped
    rows, lda tails, unused stat slots) the outputs do not change by a bit.
The weight operand of every GEMM case is packed on the device by the pack entry point of its format.  ws_gemm_tnb results
are checked per split and once more after dev.reduce_slabs.  The last test writes the worst err / bound and the case count per
kernel instantiation to blk_contract.json in the directory $WESEP_TEST_OUT (default: the system's temporary directory);
profiles/blk_contract.md is where the figures of a run are recorded.  No kernel is broken to demonstrate a catch:
tests/test_blk_contract_host_cpu.py plants the defects into emulated outputs."""
import json
import os
import tempfile

import pytest
import torch

from tests import blk_contract as bc
from tests import gemm_contract as gc

pytestmark = pytest.mark.gpu

WORST = {}     # instantiation -> [worst err / bound, cases]


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _note(case, ratio, count=True):
    for t in case.targets:
        w = WORST.setdefault(t, [0.0, 0])
        w[0] = max(w[0], ratio)
        w[1] += int(count)


def _launch(b, d):
    """One launch into fresh device buffers; returns every allocation (CPU) and the device tensors."""
    from wesep_amd import dev
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    bc.run(dev, b, t, d)
    torch.cuda.synchronize()
    return {n: v.cpu() for n, v in t.items()}, t


def _check_reduced(case, b, ref, t, d):
    """dev.reduce_slabs over the splits of every output, against the summed reference."""
    from wesep_amd import dev
    worst, nsplit = 0.0, b.kw["nsplit"]
    for key, name in b.out_keys.items():
        r = ref[key]
        n = r.idx.numel() // nsplit
        red = gc.reduced(r, nsplit)
        out = torch.full((n + 2 * gc.GUARD,), gc.SENT, device=d)
        before = out.cpu()
        before[gc.GUARD:gc.GUARD + n] = float("nan")
        out.copy_(before)
        dev.reduce_slabs(t[name][b.base(name):], nsplit, n, n, out, out_off=gc.GUARD)
        torch.cuda.synchronize()
        worst = max(worst, gc.check(out, before, red, f"{case.name} reduced {key}", gc.GUARD))
    return worst


def _run(case):
    d = _cuda()
    b = bc.build(case)
    ref = bc.reference(b)
    after, t = _launch(b, d)
    worst = bc.verify(b, ref, after)
    if case.entry == "gemm_tnb":
        worst = max(worst, _check_reduced(case, b, ref, t, d))
    after2, _ = _launch(b, d)
    assert torch.equal(bc.output_bits(b, after), bc.output_bits(b, after2)), f"{case.name}: two launches differ"
    _note(case, worst)


@pytest.mark.parametrize("case", bc.cases("pack_w"), ids=lambda c: c.name)
def test_pack_w_contract(case):
    _run(case)


@pytest.mark.parametrize("case", bc.cases("gemm_p2b"), ids=lambda c: c.name)
def test_gemm_p2b_contract(case):
    _run(case)


@pytest.mark.parametrize("case", bc.cases("gemm_b2p"), ids=lambda c: c.name)
def test_gemm_b2p_contract(case):
    _run(case)


@pytest.mark.parametrize("case", bc.cases("gemm_tnb"), ids=lambda c: c.name)
def test_gemm_tnb_contract(case):
    _run(case)


@pytest.mark.parametrize("case", bc.cases("gemm_p2b") + bc.cases("gemm_b2p"), ids=lambda c: c.entry + "-" + c.name)
def test_what_the_contract_does_not_read_is_selected_away(case):
    """Large finite values where the plain build holds NaN or zeros -- padded slots of the BL operand, the rows of cut-off
    steps and of sequences >= nvalid, unmapped rows, lda tails, unused stat slots, R outside the write set: C, A_bl, A_bl16
    and amax come out with the same bits.  (a16_out relays the padded slots of A: it is compared in the plain run only.)"""
    d = _cuda()
    b, bg = bc.build(case), bc.build(case, garbage=True)
    after, _ = _launch(b, d)
    afterg, _ = _launch(bg, d)
    for name in b.outs:
        if name == "a16_out":
            continue
        assert torch.equal(after[name].view(torch.int32), afterg[name].view(torch.int32)), f"{case.name}: {name} changed"
    bc.verify(bg, bc.reference(bg), afterg)


def test_a16_out_is_refused_with_any_other_a_fmt():
    """Header, library and dev.gemm_b2p agree: a16_out goes with a_fmt 0 (the library's own check, past the wrapper's)."""
    from wesep_amd import _lib as L
    from wesep_amd import dev
    d = _cuda()
    case = next(c for c in bc.cases("gemm_b2p") if c.dims["a_fmt"] == 1)
    b = bc.build(case)
    t = {k: v.clone().to(d) for k, v in b.bufs.items()}
    kw = b.kwargs(t, d)
    spare = torch.zeros(dev.bl_num_blocks(kw["sm"]) * 32 * kw["K"] // 2 + 16, device=d)
    for fmt in (1, 2, 3):
        a = L.GemmB2PArgs()
        a.A, a.Wpack, a.C, a.a16_out = dev._p(kw["A"]), dev._p(t["Wpack"]), dev._p(kw["C_out"]), dev._p(spare)
        a.sm = dev._smc(kw["sm"])
        a.ldc, a.N, a.K, a.a_fmt = kw["ldc"], 128, kw["K"], fmt
        a.amax = dev._p(t["Wpack"])
        rc = L.lib().ws_gemm_b2p(__import__("ctypes").byref(a), L.stream_ptr())
        assert rc == -1 and "a16_out goes with a_fmt 0" in L.lib().ws_last_error().decode(), (fmt, rc)
        with pytest.raises(L.WesepHipError, match="a16_out goes with a_fmt = 0"):
            dev.gemm_b2p(**{**kw, "a_fmt": fmt, "a16_out": spare, "amax": t["Wpack"].view(torch.int32)[:1]})
    torch.cuda.synchronize()
    assert float(spare.abs().max()) == 0.0


def test_zz_write_worst_ratios():
    """Last in the file: the worst err / bound and the case count per instantiation -> $WESEP_TEST_OUT/blk_contract.json."""
    _cuda()
    assert WORST, "the sweep above did not run in this process"
    out = os.environ.get("WESEP_TEST_OUT") or tempfile.gettempdir()
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "blk_contract.json"), "w") as f:
        json.dump({k: {"worst_err_over_bound": v[0], "cases": v[1]} for k, v in sorted(WORST.items())}, f, indent=1)
    assert all(v[0] <= 1.0 for v in WORST.values())
