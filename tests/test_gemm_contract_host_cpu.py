"""CPU checks of the GEMM contract suite (tests/gemm_contract.py): nothing here needs a GPU.

  - the float64 reference agrees with independent plain torch (F.linear with every epilogue; F.conv2d / F.conv_transpose2d
    forward, input and weight gradients by autograd for every (k, stride, dil, p) of the generator, ldp > C included;
    dilated F.conv1d for the one-row view; torch.roll for the shift) and with tests/emu_dev.py (fp32) on every case;
  - every generated case passes the WS_REQUIRE rules of the real libwesep_hip.so (tests/abi_dryrun.py), and a list of
    deliberately invalid argument sets comes back WS_ERR_INVALID with the message the library promises;
  - the pairwise and per-instantiation coverage conditions of the generator hold;
  - SENSITIVITY: the checker passes a torch emulation of the split-bf16 product (three terms, fp32 accumulation in chunks
    of 16) and refuses every planted defect below.  The last column is the Frobenius ratio rel() the suite used so far
    (tests/test_kernels_gpu.py, bound 4e-5) for the same wrong output: the defects marked MISSED would have passed it.

      defect                                                          checker      rel()
      (none: the split-bf16 emulation itself)                         passes       4.4e-06
      one of the three split terms dropped                            bound        1.6e-03
      last partial k-tile dropped (K = 100)                           bound        1.7e-01
      row 128 of the output taken from row 127                        bound        1.1e-01
      stat index off by one group on the first row of a group         bound        5.1e-02
      mode 0 tap read instead of zeroed: top / bottom / left / right  bound        3.3e-01 2.6e-01 6.1e-04 5.2e-04
      mode 1 tap read instead of zeroed: top / bottom / left / right  bound        3.0e-01 2.2e-01 6.0e-04 4.3e-04
      mode-1 tap with an inexact division accepted                    bound        1.7e+00
      shift -1 / +1 / -10 / +10 not zeroed at a sequence's end        bound        2.1e-03 1.6e+00 1.7e-03 5.9e-03
      empty split left unwritten                                      nan          nan (rel() < 4e-5 is false: caught)
      empty split written as 1e-30 instead of 0                       bound        2.6e-08 MISSED
      ReLU derivative using >=                                        exact        6.2e-01
      bias added once per k-tile instead of after the sum             bound        3.5e-05 MISSED
      one sentinel overwritten                                        sentinel     4.3e-06 MISSED
      one element off by 1e-3 relative in a 1001 x 260 output         bound        4.3e-06 MISSED
    (operands with mixed scales, as the generator draws them: rows x1e3 carry the Frobenius norm, which is how a bias
    counted four times stays below 4e-5.)
"""
import pytest
import torch
import torch.nn.functional as F

from tests import abi_dryrun, emu_dev
from tests import gemm_contract as gc

NA, BIG = gc.NA, gc.BIG
ENTRIES = ("gemm_nt", "gemm_tn", "conv_wgrad", "reduce_slabs")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rnd(g, *shape):
    return torch.randn(*shape, generator=g).float()


def close(a, b, S=None):
    tol = 1e-12 * (S if S is not None else b.abs().max() + 1)
    assert ((a - b).abs() <= tol).all(), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------
# reference vs plain torch
# ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act,useT,useR", [(0, 0, 0), (1, 0, 0), (2, 0, 0), (1, 1, 1), (0, 1, 0), (4, 1, 1), (2, 0, 1), (4, 1, 0)])
def test_reference_is_linear_with_every_epilogue(act, useT, useR):
    g = torch.Generator().manual_seed(3)
    M, N, K = 37, 13, 22
    A, W, b, R, T = rnd(g, M, K), rnd(g, N, K), rnd(g, N), rnd(g, M, N), torch.tanh(rnd(g, M, N))
    if act == 4:
        T = torch.where(torch.rand(M, N, generator=g) < 0.2, torch.zeros(()), rnd(g, M, N))
    ref = gc.ref_gemm_nt(A=A, a_rows=(BIG, 0, K), M=M, C_out=torch.zeros(M, N), c_rows=(BIG, 0, N), N=N, K=K, W=W, ldw=K,
                         bias=b, R=R if useR else None, T=T if useT else None, act=act, vec=0, mode="f32")["C"]
    v = F.linear(A.double(), W.double(), b.double())
    v = torch.tanh(v) if act == 1 else torch.relu(v) if act == 2 else v
    if useT:
        v = v * ((T > 0).double() if act == 4 else 1 - T.double() ** 2)
    if useR:
        v = v + R.double()
    assert torch.equal(ref.idx, torch.arange(M * N))
    close(ref.val.view(M, N), v)
    S = A.double().abs() @ W.double().abs().t() + b.double().abs()
    close(ref.S.view(M, N), S)
    if act == 4:
        assert torch.equal(ref.exact.view(M, N), T <= 0)


def _cl(x):          # [R, C, H, W] -> channels-last rows [R*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _img(x_nchw, ldp):
    """Channels-last image with pixel stride ldp (NaN behind the C channels)."""
    R, C, H, W = x_nchw.shape
    out = torch.full((R * H * W, ldp or C), float("nan"))
    out[:, :C] = _cl(x_nchw).float()
    return out.reshape(-1)


VIEWS = [(k, s, dil, p) for k in gc.CONV_DIMS["k"] for s in gc.CONV_DIMS["stride"] for dil in gc.CONV_DIMS["dil"]
         for p in sorted({0, k // 2, dil * (k // 2)})]


@pytest.mark.parametrize("k,stride,dil,p", VIEWS, ids=lambda v: str(v).replace(" ", ""))
def test_reference_is_conv2d_and_conv_transpose2d(k, stride, dil, p):
    g = torch.Generator().manual_seed(k * 100 + dil * 10 + p)
    Rn, C, N, H, W = 2, 4, 8, 13, 15
    sh, sw = stride
    ldp = (C + 4) if (k + dil + p + sh) % 2 else 0
    x = rnd(g, Rn, C, H, W).double().requires_grad_()
    # ---- Conv2d: forward = mode 0 on the input; input gradient = mode 1 on dy; weight gradient = TN over the mode-0 view
    if H + 2 * p - dil * (k - 1) - 1 >= 0:
        w = rnd(g, N, C, k, k).double().requires_grad_()
        y = F.conv2d(x, w, stride=stride, padding=p, dilation=dil)
        Ho, Wo = y.shape[2:]
        dy = rnd(g, *y.shape).double()
        dx, dw = torch.autograd.grad(y, (x, w), dy)
        K, M = k * k * C, Rn * Ho * Wo
        view = (0, H, W, C, Ho, Wo, k, sh, sw, p, dil, ldp)
        xf = _img(x.detach(), ldp)
        ref = gc.ref_gemm_nt(A=xf, a_rows=(BIG, 0, K), M=M, C_out=torch.zeros(M * N), c_rows=(BIG, 0, N), N=N, K=K,
                             W=w.detach().permute(0, 2, 3, 1).reshape(N, K).float(), ldw=K, vec=3, mode="bf16x3", conv=view)["C"]
        close(ref.val.view(M, N), _cl(y.detach()), ref.S.view(M, N) + 1e-3)
        Kb, Mb = k * k * N, Rn * H * W
        ref = gc.ref_gemm_nt(A=_cl(dy).float().reshape(-1), a_rows=(BIG, 0, Kb), M=Mb, C_out=torch.zeros(Mb * C),
                             c_rows=(BIG, 0, C), N=C, K=Kb, W=w.detach().permute(1, 2, 3, 0).reshape(C, Kb).float(), ldw=Kb,
                             vec=3, mode="bf16x3", conv=(1, Ho, Wo, N, H, W, k, sh, sw, p, dil, 0))["C"]
        close(ref.val.view(Mb, C), _cl(dx), ref.S.view(Mb, C) + 1e-3)
        rows = -(-M // 32 // 2) * 32
        ns = -(-M // rows)
        kw = dict(M=M, slab=torch.zeros(ns * N * K), nsplit=ns, conv=view)
        tn = gc.ref_gemm_tn(G=_cl(dy).float().reshape(-1), g_rows=(BIG, 0, N), A=xf, a_rows=(BIG, 0, K), slab_stride=N * K,
                            rows_per_split=rows, Nn=N, Kk=K, bslab=torch.zeros(ns * N), bslab_stride=N, mode="bf16x3", **kw)
        wg = gc.ref_conv_wgrad(G=_cl(dy).float().reshape(-1), ldg=N, X=xf, Nn=N, tiles_per_split=rows // 32,
                               bslab=torch.zeros(ns * N), **kw)
        for r in (tn, wg):
            close(r["slab"].val.view(ns, N, K).sum(0), dw.permute(0, 2, 3, 1).reshape(N, K), r["slab"].S.view(ns, N, K).sum(0) + 1e-3)
            close(r["bslab"].val.view(ns, N).sum(0), dy.sum((0, 2, 3)), r["bslab"].S.view(ns, N).sum(0) + 1e-3)
        assert torch.equal(tn["slab"].val, wg["slab"].val) and torch.equal(tn["slab"].idx, wg["slab"].idx)
    # ---- ConvTranspose2d: forward = mode 1 on the input; input gradient = mode 0 on dy; weight gradient = TN with G = x
    Ho, Wo = (H - 1) * sh - 2 * p + dil * (k - 1) + 1, (W - 1) * sw - 2 * p + dil * (k - 1) + 1
    if Ho >= 1 and Wo >= 1:
        wt = rnd(g, C, N, k, k).double().requires_grad_()
        y = F.conv_transpose2d(x, wt, stride=stride, padding=p, dilation=dil)
        assert tuple(y.shape[2:]) == (Ho, Wo)
        dy = rnd(g, *y.shape).double()
        dx, dwt = torch.autograd.grad(y, (x, wt), dy)
        K, M = k * k * C, Rn * Ho * Wo
        ref = gc.ref_gemm_nt(A=_img(x.detach(), ldp), a_rows=(BIG, 0, K), M=M, C_out=torch.zeros(M * N), c_rows=(BIG, 0, N),
                             N=N, K=K, W=wt.detach().permute(1, 2, 3, 0).reshape(N, K).float(), ldw=K, vec=3, mode="bf16x3",
                             conv=(1, H, W, C, Ho, Wo, k, sh, sw, p, dil, ldp))["C"]
        close(ref.val.view(M, N), _cl(y.detach()), ref.S.view(M, N) + 1e-3)
        Kb, Mb = k * k * N, Rn * H * W
        view = (0, Ho, Wo, N, H, W, k, sh, sw, p, dil, 0)
        ref = gc.ref_gemm_nt(A=_cl(dy).float().reshape(-1), a_rows=(BIG, 0, Kb), M=Mb, C_out=torch.zeros(Mb * C),
                             c_rows=(BIG, 0, C), N=C, K=Kb, W=wt.detach().permute(0, 2, 3, 1).reshape(C, Kb).float(), ldw=Kb,
                             vec=3, mode="bf16x3", conv=view)["C"]
        close(ref.val.view(Mb, C), _cl(dx), ref.S.view(Mb, C) + 1e-3)
        tn = gc.ref_gemm_tn(G=_cl(x.detach()).float().reshape(-1), g_rows=(BIG, 0, C), A=_cl(dy).float().reshape(-1),
                            a_rows=(BIG, 0, Kb), M=Mb, slab=torch.zeros(C * Kb), slab_stride=C * Kb, nsplit=1,
                            rows_per_split=Mb, Nn=C, Kk=Kb, mode="bf16x3", conv=view)["slab"]
        close(tn.val.view(C, Kb), dwt.permute(0, 2, 3, 1).reshape(C, Kb), tn.S.view(C, Kb) + 1e-3)


@pytest.mark.parametrize("k,dil", [(1, 1), (3, 1), (3, 2), (3, 3), (5, 2), (5, 3)])
def test_reference_one_row_view_is_dilated_conv1d(k, dil):
    g = torch.Generator().manual_seed(k + dil)
    Rn, T, C, N = 2, 23, 4, 6
    x, w1 = rnd(g, Rn, T, C), rnd(g, N, C, k)
    y = F.conv1d(x.double().permute(0, 2, 1), w1.double(), dilation=dil, padding=dil * (k // 2))   # [R, N, T]
    W2 = rnd(g, N, k, k, C)                      # the rows ky != k/2 fall outside the one-row image: any value
    W2[:, k // 2] = w1.permute(0, 2, 1)
    K, M = k * k * C, Rn * T
    ref = gc.ref_gemm_nt(A=x.reshape(-1), a_rows=(BIG, 0, K), M=M, C_out=torch.zeros(M * N), c_rows=(BIG, 0, N), N=N, K=K,
                         W=W2.reshape(N, K), ldw=K, vec=3, mode="bf16x3",
                         conv=(0, 1, T, C, 1, T, k, 1, 1, dil * (k // 2), dil, 0))["C"]
    close(ref.val.view(Rn, T, N), y.permute(0, 2, 1), ref.S.view(Rn, T, N) + 1e-3)


@pytest.mark.parametrize("seq_div,seq_len,sign", [(1, 5, -1), (1, 5, 1), (10, 4, -1), (10, 4, 1)])
def test_reference_shift_is_a_roll_with_the_wrapped_step_zeroed(seq_div, seq_len, sign):
    g = torch.Generator().manual_seed(11)
    outer, Nn, Kk = 3, 8, 6
    M = outer * seq_len * seq_div
    G, A = rnd(g, M, Nn), rnd(g, M, Kk)
    ref = gc.ref_gemm_tn(G=G, g_rows=(BIG, 0, Nn), A=A, a_rows=(BIG, 0, Kk), M=M, slab=torch.zeros(Nn * Kk),
                         slab_stride=Nn * Kk, nsplit=1, rows_per_split=M, Nn=Nn, Kk=Kk, shift_rows=sign * seq_div,
                         seq_div=seq_div, seq_len=seq_len, mode="f32")["slab"]
    A4 = torch.roll(A.double().view(outer, seq_len, seq_div, Kk), -sign, dims=1)
    A4[:, -1 if sign > 0 else 0] = 0
    close(ref.val.view(Nn, Kk), G.double().t() @ A4.reshape(M, Kk))


def test_reference_reduce_slabs_is_a_sum():
    g = torch.Generator().manual_seed(1)
    slab = rnd(g, 5, 40)
    ref = gc.ref_reduce_slabs(slab, 5, 40, 33, torch.zeros(100), w=4, ldo=9, out_off=3)["out"]
    i = torch.arange(33)
    assert torch.equal(ref.idx, 3 + (i // 4) * 9 + i % 4)
    close(ref.val, slab.double()[:, :33].sum(0))


# ------------------------------------------------------------------------------------------------------------
# every case: emulation, dry run, coverage
# ------------------------------------------------------------------------------------------------------------
def _emu_kwargs(entry, kw):
    if kw.get("conv") is not None and entry != "conv_wgrad":     # the emulation takes the image at offset 0
        kw = dict(kw, A=kw["A"].reshape(-1)[kw["a_off"]:], a_off=0)
    return kw


@pytest.mark.parametrize("entry", ENTRIES)
def test_reference_agrees_with_the_cpu_emulation_on_every_case(entry):
    for c in gc.cases(entry):
        b = gc.build(c)
        ref = gc.reference(b)
        t = {k: v.clone() for k, v in b.bufs.items()}
        getattr(emu_dev, entry)(**_emu_kwargs(entry, b.kwargs(t, "cpu")))
        for key, name in b.out_keys.items():
            gc.check(t[name], b.bufs[name], ref[key], c.name, b.base(name))


@pytest.mark.parametrize("entry", ENTRIES)
def test_every_case_passes_the_library_contract(entry, monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    for c in gc.cases(entry):
        b = gc.build(c)
        kw = b.kwargs(b.bufs, "cpu")
        getattr(dev, entry)(**kw)
        if entry == "conv_wgrad":
            dev.gemm_tn(**gc.wgrad_as_gemm_tn(kw))
    abi_dryrun.assert_contracts_hold(calls, at_least=len(gc.cases(entry)))


def _case(entry, **dims):
    base = {d: (NA if d in gc.CONV_SUB and entry != "conv_wgrad" else v[0]) for d, v in gc.DIMS[entry].items()}
    base.update(dims)
    assert gc.violated(entry, base) is None, gc.violated(entry, base)
    return gc.Case(entry, "hand", base, (), 77)


def test_invalid_argument_sets_are_refused_with_the_promised_message(monkeypatch):
    from wesep_amd import dev
    calls = abi_dryrun.install(monkeypatch)
    conv = dict(conv="m0", M=NA, K=NA, a_rows=NA, k=3, stride=(1, 1), dil=1, p="k/2", C=4, ldp="0", img="3x5")
    ntc = gc.build(_case("gemm_nt", mode="bf16x3", vec=3, N=12, **conv))
    plain = gc.build(_case("gemm_nt", mode="bf16x3", vec=3, N=12, K=32))
    tn = gc.build(_case("gemm_tn", mode="bf16x3", M=257, Nn=16, Kk=32))
    tnc = gc.build(_case("gemm_tn", mode="bf16x3", Nn=16, **{("Kk" if k == "K" else k): v for k, v in conv.items()}))
    wg = gc.build(_case("conv_wgrad"))
    some_table = torch.zeros(72 * 3, dtype=torch.uint8)
    bad = [
        (dev.gemm_nt, dict(ntc.kwargs(ntc.bufs), groups=some_table, ngroups=3,
                           max_n=12), "no groups"),
        (dev.gemm_nt, dict(plain.kwargs(plain.bufs), vec=3 | 8, N=10), "N % 4 == 0"),
        (dev.gemm_nt, dict(plain.kwargs(plain.bufs), vec=3 | 8, mode="f32"), "vec 15"),
        (dev.gemm_nt, dict(plain.kwargs(plain.bufs), M=0), "M=0"),
        (dev.gemm_tn, dict(tn.kwargs(tn.bufs), nsplit=2, rows_per_split=100), "splits do not cover M"),
        (dev.gemm_tn, dict(tn.kwargs(tn.bufs), Nn=6), "multiple of 4"),
        (dev.gemm_tn, dict(tn.kwargs(tn.bufs), shift_rows=-10, seq_div=10, seq_len=4), "whole sequences"),
        (dev.gemm_tn, dict(tnc.kwargs(tnc.bufs), shift_rows=1), "no shift"),
        (dev.gemm_tn, dict(tnc.kwargs(tnc.bufs), mode="f32"), "split-bf16"),
        (dev.conv_wgrad, dict(wg.kwargs(wg.bufs), nsplit=1, tiles_per_split=1), "splits do not cover M"),
        (dev.conv_wgrad, dict(wg.kwargs(wg.bufs), ldg=6), "ldg"),
        (dev.conv_wgrad, dict(wg.kwargs(wg.bufs), Nn=36, ldg=36), "Nn in 4..32"),
    ]
    for fn, kw, msg in bad:
        del calls[:]
        fn(**kw)
        (what, rc, text), = calls
        assert rc == abi_dryrun.WS_ERR_INVALID and msg in text, (what, rc, text, msg)


@pytest.mark.parametrize("entry", ENTRIES[:3])
def test_every_pair_of_values_occurs_or_is_ruled_out_by_name(entry):
    cs, inv = gc.cases(entry), gc.invalid_pairs(entry)
    assert len(cs) <= gc.MAX_CASES
    covered = set()
    for c in cs:
        assert gc.violated(entry, c.dims) is None
        covered |= gc._pairs_of(entry, c.dims)
    for pr in gc.all_pairs(entry):
        assert (pr in covered) != (pr in inv), pr           # exactly one of the two
    assert not [p for p, why in inv.items() if why.startswith("UNNAMED")]
    for pr, why in inv.items():                             # a named pair really is invalid: no case holds it
        assert pr not in covered, (pr, why)
    again = gc._CACHE.pop(entry)
    assert [c.dims for c in gc.cases(entry)] == [c.dims for c in again[0]], "the case list is not deterministic"


def test_every_instantiation_and_epilogue_is_covered():
    for entry in ENTRIES:
        cs = gc.cases(entry)
        assert len(cs) <= gc.MAX_CASES
        for inst in gc.INST[entry]:
            n = sum(1 for c in cs if inst in c.targets)
            assert n >= gc.MIN_PER_TARGET, (inst, n)
        assert {t for c in cs for t in c.targets} <= set(gc.INST[entry]) | set(gc.EPI)
    nt = gc.cases("gemm_nt")
    for epi in gc.EPI:
        hit = [c for c in nt if epi in c.targets and c.dims["mode"] == "bf16x3" and len([t for t in c.targets if t in gc.EPI]) == 1]
        for act in (0, 1, 2, 4):
            assert any(c.dims["act"] == act for c in hit), (epi, act)
            for what in ({"T": 1}, {"R": "sep"}, {"R": "alias"}):
                assert any(c.dims["act"] == act and all(c.dims[k] == v for k, v in what.items()) for c in hit), (epi, act, what)


def test_case_sizes_and_operand_mix():
    for entry in ENTRIES[:3]:
        for c in gc.cases(entry)[::7]:
            b = gc.build(c)
            kw = b.kw
            assert kw["M"] <= 4096 and kw.get("K", kw.get("Kk", 0)) <= 2048
            for name, t in b.bufs.items():
                if name in b.outs:      # guards of an output: the sentinel, bit for bit
                    assert (t[:gc.GUARD] == gc.SENT).all() and (t[-gc.GUARD:] == gc.SENT).all()
                else:
                    assert torch.isnan(t[:gc.GUARD]).all() and torch.isnan(t[-gc.GUARD:]).all()
    x = gc.draw(torch.Generator().manual_seed(0), 400, 300)
    assert (x == 0).float().mean() > 0.02 and 0.4 < (x > 0).float().mean() < 0.6
    assert x.abs().max() > 300 and x[x != 0].abs().min() < 1e-4
    b = gc.build(gc.cases("gemm_nt")[0])
    r = gc.reference(b)["C"]
    assert float((r.val.abs() / r.S.clamp_min(1e-30)).median()) < 0.9, "S is a trivial multiple of |ref|"


# ------------------------------------------------------------------------------------------------------------
# sensitivity
# ------------------------------------------------------------------------------------------------------------
def split3(a, w, terms=3, chunk=16, bias=None, bias_per_chunk_of=0):
    """a [M, K] x w [N, K]^T as the split-bf16 kernels compute it: hi / lo, three products, fp32 accumulation."""
    ah, wh = a.bfloat16().float(), w.bfloat16().float()
    al, wl = (a - ah).bfloat16().float(), (w - wh).bfloat16().float()
    acc = torch.zeros(a.shape[0], w.shape[0])
    for k0 in range(0, a.shape[1], chunk):
        s = slice(k0, k0 + chunk)
        acc = acc + ah[:, s] @ wh[:, s].t()
        if terms >= 2:
            acc = acc + ah[:, s] @ wl[:, s].t()
        if terms >= 3:
            acc = acc + al[:, s] @ wh[:, s].t()
        if bias_per_chunk_of and k0 % bias_per_chunk_of == 0:
            acc = acc + bias
    return acc


def emulate_nt(b, **defect):
    """fp32 output allocation of a plain (no groups / norm / conv) NT case, computed like the split-bf16 kernel."""
    kw = b.kwargs({k: v.clone() for k, v in b.bufs.items()})
    M, N, K = kw["M"], kw["N"], kw["K"]
    m = torch.arange(M)
    a = kw["A"][(kw["a_off"] + gc._row_off(m, kw["a_rows"])).unsqueeze(1) + torch.arange(K)]
    w = kw["W"][kw["w_off"] + torch.arange(N).unsqueeze(1) * kw["ldw"] + torch.arange(K)]
    if defect.get("drop_tail"):
        a = a.clone()
        a[:, K // 32 * 32:] = 0
    bias = kw["bias"] if kw.get("bias") is not None else torch.zeros(N)
    per = defect.get("bias_per_tile", 0)
    v = split3(a, w, terms=defect.get("terms", 3), bias=bias, bias_per_chunk_of=per)
    if not per:
        v = v + bias
    if kw["act"] == 1:
        v = torch.tanh(v)
    if kw["act"] == 2:
        v = torch.relu(v)
    cidx = (kw["c_off"] + gc._row_off(m, kw["c_rows"])).unsqueeze(1) + torch.arange(N)
    if kw.get("T") is not None:
        t = kw["T"][cidx]
        if kw["act"] == 4:
            v = v * ((t >= 0) if defect.get("relu_ge") else (t > 0)).float()
        else:
            v = v * (1 - t * t)
    if kw.get("R") is not None:
        v = v + kw["R"][cidx]
    if "row_from" in defect:
        dst, src = defect["row_from"]
        v[dst] = v[src]
    if "one_off" in defect:
        r = gc.reference(b)["C"]
        j = int((r.val.abs() / r.S.clamp_min(1e-30)).argmax())
        v.view(-1)[j] *= 1 + defect["one_off"]
    out = kw["C_out"].clone()
    out[cidx] = v
    return out


def test_split_product_error_lies_between_2_to_minus_16_and_2_to_minus_15():
    """The constant of the split-bf16 bound, from the arithmetic: operands just below the midpoint between two bf16
    numbers leave lo = 2^-8 * hi (nearly), so the dropped lo * lo term alone is 2^-16 of the product and the two
    representation errors come on top: a correctly rounded three-term product exceeds 2^-16 |a||w| (the constant the
    issue stated) and stays below 2^-15 |a||w| (the constant of gemm_contract.eps_for)."""
    g = torch.Generator().manual_seed(0)
    base = 1 + 2.0 ** -8 - 2.0 ** -17 * torch.rand(4000, generator=g, dtype=torch.float64)   # just below 1 + half an ulp
    a = (base * (1 + torch.randint(0, 127, (4000,), generator=g) / 128.0)).float()          # any bf16 neighbourhood
    w = a.flip(0)
    ah, wh = a.bfloat16().float(), w.bfloat16().float()
    al, wl = (a - ah).bfloat16().float(), (w - wh).bfloat16().float()
    got = ah.double() * wh.double() + ah.double() * wl.double() + al.double() * wh.double()   # the three terms, exactly
    err = ((got - a.double() * w.double()).abs() / (a.double() * w.double()).abs())
    assert float(err.max()) > 2.0 ** -16, float(err.max())
    x = torch.cat([a, gc.draw(g, 200, 200).reshape(-1)])
    y = x.flip(0)
    xh, yh = x.bfloat16().float(), y.bfloat16().float()
    xl, yl = (x - xh).bfloat16().float(), (y - yh).bfloat16().float()
    got = xh.double() * yh.double() + xh.double() * yl.double() + xl.double() * yh.double()
    assert ((got - x.double() * y.double()).abs() <= 2.0 ** -15 * (x.double() * y.double()).abs()).all()


PLAIN = dict(mode="bf16x3", vec=3, M=1001, N=260, K=100, a_rows="padded", c_rows="two", bias=1)
RESULTS = {}


def _judge(name, b, out, key="C", expect="bound"):
    ref = gc.reference(b)[key]
    buf = b.out_keys[key]
    got = out.reshape(-1)[ref.idx + b.base(buf)]
    RESULTS[name] = rel(got, ref.val)
    print(f"rel() of '{name}': {RESULTS[name]:.1e}")
    if expect is None:
        return gc.check(out, b.bufs[buf], ref, name, b.base(buf))
    with pytest.raises(gc.ContractViolation) as e:
        gc.check(out, b.bufs[buf], ref, name, b.base(buf))
    assert e.value.kind == expect, (name, str(e.value))


def _with_ref_values(b, ref, key="C"):
    """The output allocation a perfectly rounding kernel leaves for `ref`."""
    buf = b.out_keys[key]
    out = b.bufs[buf].clone()
    out[ref.idx + b.base(buf)] = ref.val.float()
    return out


@pytest.mark.parametrize("extra", [dict(), dict(act=1), dict(act=2, R="sep"), dict(act=4, T=1, R="alias"), dict(act=1, T=1),
                                   dict(K=4, N=12), dict(K=512, M=129)])
def test_checker_passes_the_split_bf16_emulation(extra):
    b = gc.build(_case("gemm_nt", **{**PLAIN, **extra}))
    ratio = _judge("ok", b, emulate_nt(b), expect=None)
    assert ratio <= 1.0


def test_checker_refuses_product_defects():
    b = gc.build(_case("gemm_nt", **PLAIN))
    _judge("term dropped", b, emulate_nt(b, terms=2))
    _judge("k-tail dropped", b, emulate_nt(b, drop_tail=True))
    _judge("row 128 from row 127", b, emulate_nt(b, row_from=(128, 127)))
    _judge("bias per k-tile", b, emulate_nt(b, bias_per_tile=32))
    _judge("one element off by 1e-3", b, emulate_nt(b, one_off=1e-3))
    out = emulate_nt(b)
    out[gc.GUARD - 1] = 0.0
    _judge("sentinel overwritten", b, out, expect="sentinel")
    b = gc.build(_case("gemm_nt", **{**PLAIN, "act": 4, "T": 1, "R": "sep"}))
    _judge("relu derivative >=", b, emulate_nt(b, relu_ge=True), expect="exact")
    missed = {k for k in ("term dropped", "k-tail dropped", "row 128 from row 127", "bias per k-tile",
                          "one element off by 1e-3", "sentinel overwritten", "relu derivative >=") if RESULTS[k] < 4e-5}
    assert missed == {"bias per k-tile", "one element off by 1e-3", "sentinel overwritten"}     # what rel() < 4e-5 lets through


def test_checker_refuses_a_stat_index_off_by_one_group():
    b = gc.build(_case("gemm_nt", mode="f32", M=33, N=12, K=6, norm=1))
    ref = gc.reference(b)["C"]
    sm = b.kw["stat_map"]
    s5 = (5 // sm[0]) * sm[1] + (5 % sm[2]) * sm[3] + sm[4]        # row 5: the first row of stat group 1
    bufs = {k: v.clone() for k, v in b.bufs.items()}
    st = bufs["stats"]
    st[gc.GUARD + 2 * s5: gc.GUARD + 2 * s5 + 2] = st[gc.GUARD + 2 * (s5 - sm[1]): gc.GUARD + 2 * (s5 - sm[1]) + 2]
    wrong = gc.reference(b, bufs)["C"]
    row5 = (torch.arange(ref.idx.numel()) // 12) == 5
    out = _with_ref_values(b, ref._replace(val=torch.where(row5, wrong.val, ref.val)))
    _judge("stat index off by one group", b, out)
    assert RESULTS["stat index off by one group"] > 4e-5
    assert _judge("ok", b, _with_ref_values(b, ref), expect=None) <= 1.0


def _bad_patch_index(defect):
    """gc.patch_index with one planted defect: a border test dropped (the tap reads the nearest pixel instead of
    contributing zero), or mode 1's exactness test dropped."""
    def f(M, conv):
        mode, H, W, C, Ho, Wo, k, sh, sw, p, dil, ldp = gc._conv_fields(conv)
        m = torch.arange(M).unsqueeze(1)
        r, q = m // (Ho * Wo), m % (Ho * Wo)
        ho, wo = q // Wo, q % Wo
        kk = torch.arange(k * k * C).unsqueeze(0)
        tap, c = kk // C, kk % C
        ky, kx = tap // k, tap % k
        if mode == 0:
            hn, wn, dh, dw = ho * sh + ky * dil - p, wo * sw + kx * dil - p, 1, 1
        else:
            hn, wn, dh, dw = ho + p - ky * dil, wo + p - kx * dil, sh, sw
        h, w = torch.div(hn, dh, rounding_mode="floor"), torch.div(wn, dw, rounding_mode="floor")
        tests = {"top": hn >= 0, "left": wn >= 0, "bottom": h < H, "right": w < W,
                 "exact": (hn % dh == 0) & (wn % dw == 0)}
        ok = torch.ones_like(hn + wn, dtype=torch.bool)
        for name, t in tests.items():
            if name != defect:
                ok = ok & t
        idx = ((r * H + h.clamp(0, H - 1)) * W + w.clamp(0, W - 1)) * ldp + c
        return torch.where(ok, idx, torch.zeros_like(idx)), ok
    return f


@pytest.mark.parametrize("mode,defect", [(m, d) for m in ("m0", "m1") for d in ("top", "left", "bottom", "right")] + [("m1", "exact")])
def test_checker_refuses_conv_view_defects(mode, defect, monkeypatch):
    view = dict(conv=mode, M=NA, K=NA, a_rows=NA, k=3, stride=(1, 1) if mode == "m0" else (2, 2), dil=1,
                p="k/2" if mode == "m0" else "0", C=4, ldp="C+4", img="3x5")
    b = gc.build(_case("gemm_nt", mode="bf16x3", vec=3, N=12, **view))
    ref = gc.reference(b)["C"]
    assert _judge("ok", b, _with_ref_values(b, ref), expect=None) <= 1.0
    monkeypatch.setattr(gc, "patch_index", _bad_patch_index(defect))
    wrong = gc.reference(b)["C"]
    monkeypatch.undo()
    _judge(f"{mode} {defect}", b, _with_ref_values(b, wrong))
    assert RESULTS[f"{mode} {defect}"] > 4e-5


@pytest.mark.parametrize("shift", [-1, 1, -10, 10])
def test_checker_refuses_a_shift_that_is_not_zeroed(shift):
    b = gc.build(_case("gemm_tn", mode="bf16x3", M=257, Nn=16, Kk=32, shift=shift))
    ref = gc.reference(b)["slab"]
    kw = b.kwargs(b.bufs)
    assert kw["seq_len"] * kw["seq_div"] < kw["M"], "the case needs more than one sequence"
    wrong = gc.ref_gemm_tn(**{**kw, "seq_len": kw["M"] // kw["seq_div"]})["slab"]    # only the global ends are zeroed
    _judge(f"shift {shift}", b, _with_ref_values(b, wrong, "slab"), key="slab")
    assert RESULTS[f"shift {shift}"] > 4e-5
    assert _judge("ok", b, _with_ref_values(b, ref, "slab"), key="slab", expect=None) <= 1.0


def test_checker_refuses_an_unwritten_empty_split():
    b = gc.build(_case("gemm_tn", mode="bf16x3", M=129, Nn=16, Kk=32, split="empty", bias=1))
    ref = gc.reference(b)
    n = 16 * 32
    assert (ref["slab"].S[-n:] == 0).all() and (ref["slab"].bound[-n:] == 0).all()       # an exact statement: zeros
    for key in ("slab", "bslab"):
        out = _with_ref_values(b, ref[key], key)
        assert _judge("ok", b, out, key=key, expect=None) <= 1.0
        cnt = n if key == "slab" else 16
        out[ref[key].idx[-cnt:] + b.base(key)] = float("nan")
        _judge("empty split unwritten", b, out, key=key, expect="nan")
    out = _with_ref_values(b, ref["slab"], "slab")
    out[ref["slab"].idx[-1] + b.base("slab")] = 1e-30       # "almost zero" is not zero
    _judge("empty split not exactly zero", b, out, key="slab")
