"""One copy of h: the forward recurrences leave h as two fp16 planes (H2P, include/wesep_hip.h: hi = fp16(h), lo = fp16(h - hi))
instead of the bf16 pair plus an fp16 twin; the projection reads both planes (ws_gemm_b2p a_fmt 4), dW_proj the hi plane
(ws_gemm_tnb_h16).

Recurrences (GPU): gates and c bit-identical to the same launch with the pair format; hi is the fp16 nearest to hi + lo.  That
REPLACES the issue's "hi must equal fp16(h)": the kernel's fp32 h is not observable (the pair keeps 16 of its bits, the gates are
stored as unorm16).  With lo = fp16(h - hi) the two say the same up to a tie that lo's own rounding can create at 2^-22 -- but the
replacement alone would pass a kernel whose hi and lo both come from one consistently wrong h; that is what the next two
statements are for.  hi + lo within the bound of
tests/test_cluster2_gpu.py of torch's fp64 LSTM, and within 2^-16 |h| + 2^-24 of the pair-format run (2^-16 is what the pair keeps).

GEMMs (GPU) against a float64 restatement, bound form of profiles/blk_contract.md:  eps_fmt * S + (K + 8) * 2^-24 * S + floors.
  projection: the kernel adds a_hi w_hi + a_hi w_lo + a_lo w_hi of (a_hi + a_lo) * 256 w.  It drops a_lo w_lo: |a_lo| <= 2^-11 |a_hi|
    and |w_lo| <= 2^-11 |w_hi| (half an ulp each), 2^-22 of the product; the pack's own remainder is 2^-22 (the constant
    blk_contract.md keeps for ws_pack_w_f16): eps_fmt = 2^-21; floor 2^-33 * sum |a| where w_lo is an fp16 subnormal (as a_fmt 2).
  dW_proj: G is the hi plane as stored (nothing dropped), both bf16 terms of dout times S_amax go to fp16, round to nearest: exact
    for normal results (8 bits into 11), below that at most 2^-25 / S_amax per term; the floor is stated with the 2^-24 of a
    truncating conversion (the looser of the two): eps_fmt = 0, floor 2^-23 / S_amax * sum |g|.  Beyond fp16's range the lifted
    term is Inf, not clipped: test_dw_proj_overflow_is_loud.
The CPU test shows that losing the lo plane (of h for the projection, of the stored pairs for dW_proj) lies outside these bounds.
The worst err / bound per instantiation goes to profiles/one_h.md by hand from this file's output."""
import math

import pytest
import torch

from wesep_amd import _lib as L

H, N = 256, 128
gpu = pytest.mark.gpu


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int32)


def _weights(g, d):
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    w = dict(wih_f=rnd(4 * H, N, scale=0.08), wih_r=rnd(4 * H, N, scale=0.08), whh_f=rnd(4 * H, H, scale=0.06),
             whh_r=rnd(4 * H, H, scale=0.06), bf=rnd(4 * H, scale=0.2), br=rnd(4 * H, scale=0.2))
    return {k: v.to(d) for k, v in w.items()}


def _torch_lstm(w, x_seqs):
    """h of torch's fp64 BLSTM; x_seqs [nseq][L][N] (cpu, float64)."""
    lstm = torch.nn.LSTM(N, H, batch_first=True, bidirectional=True).double()
    zero = torch.zeros(4 * H, dtype=torch.float64)
    with torch.no_grad():
        for nm, src in (("weight_ih_l0", w["wih_f"]), ("weight_hh_l0", w["whh_f"]), ("bias_ih_l0", w["bf"]), ("bias_hh_l0", zero),
                        ("weight_ih_l0_reverse", w["wih_r"]), ("weight_hh_l0_reverse", w["whh_r"]), ("bias_ih_l0_reverse", w["br"]),
                        ("bias_hh_l0_reverse", zero)):
            getattr(lstm, nm).copy_(src.double().cpu())
        return lstm(x_seqs)[0]


def _nearest_fp16(hi, lo):
    """True where the fp16 value hi is a nearest fp16 to hi + lo: |lo| <= half the spacing of fp16 at hi (a quarter on the side
    where hi is a power of two and the spacing halves)."""
    hi, lo = hi.cpu(), lo.cpu().double()
    code = hi.half().view(torch.int16).to(torch.int32) & 0x7FFF              # (hi holds fp16 values: the conversion is exact)
    E, M = code >> 10, code & 1023
    ulp = torch.ldexp(torch.ones_like(lo), E.clamp_min(1) - 25)             # spacing of fp16 in hi's binade; subnormals: 2^-24
    inward = (lo * torch.sign(hi.double())) < 0
    lim = torch.where(inward & (M == 0) & (E >= 2), ulp / 4, ulp / 2)
    return lo.abs() <= lim


def _check_planes(tag, planes, pairs, gc_planes, gc_pairs, seq, P, nb, want):
    """The three statements of the module docstring for one launch pair; planes / pairs: the hcat buffers."""
    from wesep_amd import dev
    for a, b in zip(gc_planes, gc_pairs):
        assert torch.equal(bits(a), bits(b)), f"{tag}: gates / c differ between the two h formats"
    hi, lo = dev.h2p_unpack(planes, nb)
    assert not torch.isnan(hi).any() and not torch.isnan(lo).any()
    ok = _nearest_fp16(hi, lo)
    assert bool(ok.all()), (tag, int((~ok).sum()), hi.cpu()[~ok][:6].tolist(), lo.cpu()[~ok][:6].tolist())
    h2 = hi.double() + lo.double()
    hp = dev.bls_unpack(pairs).double().view_as(h2)
    gap = (h2 - hp).abs() - (2.0 ** -16 * hp.abs() + 2.0 ** -24)
    err = rel(dev.from_blocked(h2.float().view(nb, 2 * H // 4, 32, 4), seq, P), want)
    err_p = rel(dev.from_blocked(hp.float().view(nb, 2 * H // 4, 32, 4), seq, P), want)
    bad = (gap > 0).nonzero()
    print(f"{tag}: planes vs pair, worst (|diff| - bound) {float(gap.max()):.2e}; worst |diff| / bound "
          f"{float(((h2 - hp).abs() / (2.0 ** -16 * hp.abs() + 2.0 ** -24)).max()):.3f}; hi + lo rel vs torch fp64 {err:.2e} "
          f"(the pair: {err_p:.2e}); {bad.shape[0]} over the bound, first (block, quad, slot, col): {bad[:8].tolist()}")
    if bad.shape[0]:      # the elements themselves, next to fp64's
        w_bl = dev.to_blocked(want.float().to(hi.device), seq)
        for i in bad[:6].tolist():
            print(f"   {i}: hi {float(hi[tuple(i)])!r} lo {float(lo[tuple(i)])!r} pair {float(hp[tuple(i)])!r} fp64 {float(w_bl[tuple(i)])!r}")
    assert float(gap.max()) <= 0.0, (tag, float(gap.max()))
    assert err < 1e-3, (tag, err)


@gpu
@pytest.mark.parametrize("seqs", ["64", "32"])
def test_fused_band_forward_writes_the_planes(seqs, monkeypatch):
    """nseq = 96, L = 3: three tiles, so the 64-sequence kernel's last workgroup has an empty second tile (live1); the 32-sequence
    kernel with WS_FUSED_SEQS=32.  Both the two-term fp16 kernel (hfmt 1) and the default with the FP8 lo term (hfmt 5)."""
    from wesep_amd import dev
    from wesep_amd.functional import _view_maps
    d = _cuda()
    monkeypatch.setenv("WS_FUSED_SEQS", seqs)
    g = torch.Generator().manual_seed(33)
    R, K, Tf = 2, 3, 48
    P = R * K * Tf
    _, _, seq, _ = _view_maps("band", R, K, Tf, N)
    assert seq.nseq == 96 and seq.L == 3
    nb = dev.bl_num_blocks(seq)
    w = _weights(g, d)
    x = torch.randn(P, N, generator=g).to(d)
    bias = torch.cat([w["bf"], w["br"]]).contiguous()
    xn = dev.to_blocked(x, seq, split=True)
    out = _torch_lstm(w, x.double().cpu().view(R, K, Tf, N).permute(0, 2, 1, 3).reshape(R * Tf, K, N))
    want = out.view(R, Tf, K, 2 * H).permute(0, 2, 1, 3).reshape(P, 2 * H)
    for hf in (1, 5):
        fp = torch.empty(L.LSTM_FUSED_PACK_FLOATS, device=d)
        dev.lstm_pack_fused(w["wih_f"], w["wih_r"], w["whh_f"], w["whh_r"], fp, hfmt=hf)
        res = {}
        for h2p in (0, 8):
            gh = torch.zeros(dev.blh_floats(nb, 8 * H), device=d)
            c = torch.full((nb, 2 * H // 4, 32, 4), float("nan"), device=d)
            h = torch.full_like(c, float("nan"))
            dev.lstm_fwd_fused(gh, c, h, xn, fp, bias, seq, gfmt=L.GATES_H2F, hfmt=hf | h2p)
            torch.cuda.synchronize()
            res[h2p] = (gh, c, h)
        _check_planes(f"fused {seqs}-sequence kernel, hfmt {hf}", res[8][2], res[0][2], res[8][:2], res[0][:2], seq, P, nb, want)


def _time_view_case(d):
    """nseq = 64, L = 4 (one cluster per direction, both tag parities): map, weights, input, torch's fp64 h, fresh outputs."""
    from wesep_amd import dev
    from wesep_amd.functional import _view_maps
    g = torch.Generator().manual_seed(34)
    R, K, Tf = 2, 32, 4
    P = R * K * Tf
    _, _, seq, _ = _view_maps("time", R, K, Tf, N)
    assert seq.nseq == 64 and seq.L == 4
    nb = dev.bl_num_blocks(seq)
    w = _weights(g, d)
    x = torch.randn(P, N, generator=g).to(d)
    want = _torch_lstm(w, x.double().cpu().view(R * K, Tf, N)).reshape(P, 2 * H)
    new = lambda: (torch.zeros(dev.blh_floats(nb, 8 * H), device=d), torch.full((nb, 2 * H // 4, 32, 4), float("nan"), device=d),
                   torch.full((nb, 2 * H // 4, 32, 4), float("nan"), device=d))
    return seq, nb, P, w, x, want, new


@gpu
@pytest.mark.parametrize("mode", [L.LSTM_BF16X3_BLK, L.LSTM_BF16X3_BLK16])
def test_streaming_fallback_writes_the_planes(mode):
    """The two predicated streaming kernels behind cluster2 (32- and 16-sequence workgroups), on fp32 pre-activations: a repaired
    layer must leave the same format.  Runs on any device."""
    from wesep_amd import dev
    d = _cuda()
    seq, nb, P, w, x, want, new = _time_view_case(d)
    pre = torch.cat([x @ w["wih_f"].t() + w["bf"], x @ w["wih_r"].t() + w["br"]], 1)
    pre_bl = dev.to_blocked(pre, seq)
    pf, pb = torch.empty(L.LSTM_PACK_FLOATS, device=d), torch.empty(L.LSTM_PACK_FLOATS, device=d)
    dev.lstm_pack(w["whh_f"], w["whh_r"], pf, pb, mode)
    res = {}
    for h2p in (False, True):
        gh, c, h = new()
        dev.lstm_fwd(gh, c, h, pf, seq, mode, gfmt=L.GATES_H2F, gates_in=pre_bl, h2p=h2p)
        torch.cuda.synchronize()
        res[h2p] = (gh, c, h)
    _check_planes(f"streaming forward, mode {mode}", res[True][2], res[False][2], res[True][:2], res[False][:2], seq, P, nb, want)


@gpu
@pytest.mark.parametrize("rf", [0, 1])
def test_cluster2_writes_the_planes(rf):
    """nseq = 64, L = 4, both recurrent formats.  Skipped where the device cannot hold the launch's workgroups co-resident:
    dev.lstm_cluster_resident, the device part of the existing tests' predicate dev.lstm_cluster_ok (whose "L >= 64" says when the
    kernel pays off, not when it can run: the issue sets L = 4)."""
    from wesep_amd import dev
    d = _cuda()
    seq, nb, P, w, x, want, new = _time_view_case(d)
    if not dev.lstm_cluster_resident(seq, d):
        pytest.skip("fewer CUs than the cluster launch needs co-resident workgroups")
    wcat, bcat = torch.empty(2 * 4 * H * N, device=d), torch.empty(2 * 4 * H, device=d)
    zero = torch.zeros(4 * H, device=d)
    dev.lstm_cat_ih(w["wih_f"], w["wih_r"], w["bf"], zero, w["br"], zero, N, wcat, bcat)
    xn = dev.to_blocked(x, seq, split=True)
    res = {}
    for h2p in (False, True):
        gh, c, h = new()
        st = torch.zeros(1, device=d, dtype=torch.int32)
        tw = dev.lstm_fwd_cluster2(gh, c, h, xn, wcat, bcat, w["whh_f"], w["whh_r"], seq, status=st, rfmt=rf, h2p=h2p)
        torch.cuda.synchronize()
        assert int(tw.item()) == 0 and int(st.item()) == 0
        res[h2p] = (gh, c, h)
    _check_planes(f"cluster2 rfmt {rf}", res[True][2], res[False][2], res[True][:2], res[False][:2], seq, P, nb, want)


# ---- the two GEMMs against float64 ----------------------------------------------------------------------------------------
def _planes(hval):
    """fp32 values -> (hi, lo) as fp32 tensors holding fp16 values, the way enc_h2p makes them."""
    hi = hval.half().float()
    return hi, (hval - hi).half().float()


def _proj_bound(hi, lo, Wt, K):
    """eps_fmt * S + (K + 8) 2^-24 S + floor for out = (hi + lo) W^T; hi / lo [rows][K], Wt [N][K], all float64."""
    S = (hi.abs() + lo.abs()) @ Wt.abs().t()
    return (2.0 ** -21 + (K + 8) * 2.0 ** -24) * S + 2.0 ** -33 * (hi.abs() + lo.abs()).sum(1, keepdim=True)


def _tnb_bound(g, a_hi, a_lo, terms, S_amax):
    """(K + 8) 2^-24 S + floor for slab = g^T (a_hi + a_lo); g [rows][G], a [rows][A], float64; `terms` rows were summed."""
    S = g.abs().t() @ (a_hi.abs() + a_lo.abs())
    return (terms + 8) * 2.0 ** -24 * S + 2.0 ** -23 / S_amax * g.abs().sum(0)[:, None]


def test_losing_the_lo_plane_lies_outside_both_bounds():
    """CPU, float64: operands whose lo terms all point the same way (the defect then adds up instead of averaging out)."""
    g = torch.Generator().manual_seed(35)
    K = 512
    hi = (torch.rand(40, K, generator=g) * 0.9 + 0.05).half().double()
    e = torch.frexp(hi)[1]
    lo = torch.ldexp(torch.full_like(hi, 0.4), e - 11).half().double()       # 0.4 ulp of hi, upwards
    Wt = (torch.rand(N, K, generator=g) * 0.06 + 0.01).double()
    full, dropped = (hi + lo) @ Wt.t(), hi @ Wt.t()
    worst = float(((full - dropped).abs() / _proj_bound(hi, lo, Wt, K)).min())
    print(f"projection without the lo plane: smallest err / bound {worst:.1f}")
    assert worst > 4.0
    rows = 5 * 32
    hh = (torch.rand(rows, 2 * H, generator=g) * 0.9 + 0.05).half().double()
    a_hi = (torch.rand(rows, N, generator=g) * 0.9 + 0.05).bfloat16().double()
    a_lo = torch.ldexp(torch.full_like(a_hi, 0.4), torch.frexp(a_hi)[1] - 8).bfloat16().double()   # 0.4 ulp of the bf16 hi term
    full, dropped = hh.t() @ (a_hi + a_lo), hh.t() @ a_hi
    worst = float(((full - dropped).abs() / _tnb_bound(hh, a_hi, a_lo, rows, 256.0)).min())
    print(f"dW_proj without the pairs' lo terms: smallest err / bound {worst:.1f}")
    assert worst > 4.0


def _one_sign(hi16, frac=0.4):
    """lo terms that all point upwards: `frac` of an fp16 ulp of the (positive, normal) fp16 values hi16, as float64."""
    return torch.ldexp(torch.full_like(hi16, frac), torch.frexp(hi16)[1] - 11)


@gpu
@pytest.mark.parametrize("operands", ["random", "one_sign"])
@pytest.mark.parametrize("nseq", [32, 45])
def test_projection_on_the_planes_vs_float64(nseq, operands):
    """K = 512, N = 128; nseq 32: one full 32-slot block per step, 45: a full and a partly padded one (13 live slots).  Nine blocks:
    more than the eight waves of a workgroup.  The bound is mostly its accumulation term, so with random operands a lost term
    averages out to about the bound itself; "one_sign" runs the CPU test's adversarial operands through the kernel -- positive h
    with every lo 0.4 ulp upwards, positive weights whose fp16 remainders 256 w - hi are 0.4 ulp upwards too: any one of the three
    terms missing (a_hi w_lo and a_lo w_hi are each 2^-12.3 of S) is then an error of several bounds (asserted below in float64
    before the kernel's result is looked at)."""
    from wesep_amd import dev
    d = _cuda()
    g = torch.Generator().manual_seed(36 + nseq)
    Ls, K = 9 if nseq == 32 else 5, 2 * H
    P = nseq * Ls
    from wesep_amd.functional import _view_maps
    seq = _view_maps("time", 1, nseq, Ls, N)[2]                      # sequence s, step t at row s * Ls + t
    assert seq.nseq == nseq and seq.L == Ls
    nb = dev.bl_num_blocks(seq)
    if operands == "one_sign":
        h16 = (torch.rand(P, K, generator=g) * 0.9 + 0.05).half().double()
        hi, lo = _planes((h16 + _one_sign(h16)).float())
        assert torch.equal(hi.double(), h16) and bool((lo > 0).all())
    else:
        hval = torch.tanh(torch.randn(P, K, generator=g))
        hval[0, :8] = torch.tensor([0.0, 1e-7, -3e-6, 6e-5, -6.2e-5, 0.99999, -1.0, 2.0 ** -15])     # zeros, fp16 subnormals, the ends
        hi, lo = _planes(hval)
    buf = torch.cat([dev.blh_f16_pack(dev.to_blocked(hi, seq)).reshape(-1), dev.blh_f16_pack(dev.to_blocked(lo, seq)).reshape(-1)]).to(d)
    assert buf.numel() == nb * 32 * K
    if operands == "one_sign":
        w16 = (256.0 * (torch.rand(N, K, generator=g) * 0.06 + 0.01)).half().double()
        Wp = ((w16 + _one_sign(w16)) / 256.0).float()
        bias, res = torch.zeros(N), torch.zeros(P, N)
        for lost in ((lo.double() @ w16.t()) / 256.0, hi.double() @ _one_sign(w16).half().double().t() / 256.0):   # a_lo w_hi, a_hi w_lo
            assert float((lost / _proj_bound(hi.double(), lo.double(), Wp.double(), K)).min()) > 3.0
    else:
        Wp = torch.randn(N, K, generator=g) * 0.06
        bias, res = torch.randn(N, generator=g), torch.randn(P, N, generator=g)
    pack = torch.empty(N * K, device=d)
    dev.pack_w(Wp.to(d), N, K, K, pack, order=1, f16=True)
    out = torch.full((P, N), float("nan"), device=d)
    dev.gemm_b2p(A=buf, K=K, sm=seq, Wpack=pack, C_out=out, ldc=N, bias=bias.to(d), R=res.to(d), a_fmt=4)
    torch.cuda.synchronize()
    hi64, lo64 = hi.double(), lo.double()
    ref = (hi64 + lo64) @ Wp.double().t() + bias.double() + res.double()
    bound = _proj_bound(hi64, lo64, Wp.double(), K) + 2.0 ** -23 * ref.abs()        # (+ the epilogue's two fp32 adds)
    ratio = float(((out.double().cpu() - ref).abs() / bound).max())
    print(f"gemm_b2p a_fmt 4, nseq {nseq}, {operands} operands: worst err / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


@gpu
@pytest.mark.parametrize("split", [(4, 4), (6, 3)])
def test_dw_proj_on_the_hi_plane_vs_float64(split):
    """nblk = 15 (three tiles of L = 5): (4, 4) leaves a short last split of three blocks -- a tail that is no multiple of the
    prefetch depth --, (6, 3) an empty trailing split that must write zeros."""
    from wesep_amd import dev
    d = _cuda()
    ns, bps = split
    g = torch.Generator().manual_seed(37)
    nblk, Ls = 15, 5
    rows = nblk * 32
    hval = torch.tanh(torch.randn(rows, 2 * H, generator=g))
    hi = hval.half().float()
    dout = torch.randn(rows, N, generator=g) * 3e-4 * torch.exp(2 * torch.randn(rows, 1, generator=g))   # five decades of row scales
    dout[3, :4] = torch.tensor([0.0, 1e-12, -2e-10, 4e-9])                                               # below the lifted fp16 range
    pairs = dev.bls_pack(dout)
    a64 = dev.bls_unpack(pairs).double()
    bl = lambda t: t.view(nblk, 32, -1, 4).permute(0, 2, 1, 3).contiguous()      # rows of block b = b * 32 + slot
    G = dev.blh_f16_pack(bl(hi)).reshape(-1).to(d)
    A0 = bl(pairs).to(d)
    amax_f = (dout.abs().max() * 0.5).float()                                    # what max |d(hcat)| could be: within 2^7 of max |dout|
    amax = amax_f.view(torch.int32).clone().to(d)
    S_amax = L.dgates_scale(int(amax.item()))
    assert float(dout.abs().max()) * S_amax <= 65504.0
    slab = torch.full((ns, 2 * H * N), float("nan"), device=d)
    aslab = torch.full((ns, N), float("nan"), device=d)
    dev.gemm_tnb_h16(G=G, g_width=2 * H, g_off=0, g_cols=2 * H, A0=A0, a0_width=N, a0_off=0, nblk=nblk, L_=Ls, slab=slab, nsplit=ns,
                     blocks_per_split=bps, amax=amax, aslab=aslab)
    torch.cuda.synchronize()
    bits32 = pairs.view(torch.int32)
    a_hi, a_lo = (bits32 & -65536).view(torch.float32).double(), (bits32 << 16).view(torch.float32).double()
    worst = worst_a = 0.0
    for s in range(ns):
        r0, r1 = min(s * bps, nblk) * 32, min((s + 1) * bps, nblk) * 32
        got, got_a = slab[s].view(2 * H, N).double().cpu(), aslab[s].double().cpu()
        if r1 == r0:
            assert not got.any() and not got_a.any(), "an empty split must write zeros"
            continue
        g64 = hi[r0:r1].double()
        ref = g64.t() @ a64[r0:r1]
        bound = _tnb_bound(g64, a_hi[r0:r1], a_lo[r0:r1], r1 - r0, S_amax)
        worst = max(worst, float(((got - ref).abs() / bound).max()))
        ref_a = a64[r0:r1].sum(0)
        bound_a = (r1 - r0 + 8) * 2.0 ** -24 * a64[r0:r1].abs().sum(0) + 2.0 ** -23 / S_amax * (r1 - r0)
        worst_a = max(worst_a, float(((got_a - ref_a).abs() / bound_a).max()))
    print(f"gemm_tnb_h16 {split}: worst err / bound slab {worst:.3f}, aslab {worst_a:.3f}")
    assert worst <= 1.0 and worst_a <= 1.0, (worst, worst_a)


@gpu
def test_dw_proj_overflow_is_loud():
    """The magnitude precondition broken on purpose (max |dout| = 100 against an amax word of 1e-6: S = 2^28): the lifted term must
    become Inf and every product sum it enters (its column of dW_proj^T) non-finite -- what the optimizer's guard looks for --,
    never a gradient clipped to 65504 / S; the other columns stay finite, and so do the column sums (db_proj), which are right."""
    from wesep_amd import dev
    d = _cuda()
    g = torch.Generator().manual_seed(38)
    nblk, Ls, col = 2, 2, 37
    rows = nblk * 32
    hi = (torch.rand(rows, 2 * H, generator=g) * 0.9 + 0.05).half().float()
    dout = torch.randn(rows, N, generator=g) * 1e-7
    dout[5, col] = 100.0
    bl = lambda t: t.view(nblk, 32, -1, 4).permute(0, 2, 1, 3).contiguous()
    G, A0 = dev.blh_f16_pack(bl(hi)).reshape(-1).to(d), bl(dev.bls_pack(dout)).to(d)
    amax = torch.tensor(1e-6).view(torch.int32).clone().to(d)
    assert 100.0 * L.dgates_scale(int(amax.item())) > 65504.0
    slab, aslab = torch.zeros(1, 2 * H * N, device=d), torch.zeros(1, N, device=d)
    dev.gemm_tnb_h16(G=G, g_width=2 * H, g_off=0, g_cols=2 * H, A0=A0, a0_width=N, a0_off=0, nblk=nblk, L_=Ls, slab=slab, nsplit=1,
                     blocks_per_split=nblk, amax=amax, aslab=aslab)
    torch.cuda.synchronize()
    fin = torch.isfinite(slab.view(2 * H, N)).cpu()
    assert not fin[:, col].any()
    fin[:, col] = True
    assert bool(fin.all())
    # the column sums never pass through fp16 (fp32 sums of the scaled pairs): db_proj stays right
    want_a = dev.bls_unpack(dev.bls_pack(dout)).double().sum(0)
    assert float((aslab[0].double().cpu() - want_a).abs().max()) <= 2.0 ** -20 * 100.0
