"""The saved LSTM cell state as fp16 (C16, include/wesep_hip.h): cbuf holds fp16(c), round to nearest even, in BLH(2H) -- the forward
recurrences write 2 bytes per cell instead of 4, the BPTT kernels (its only readers) read 2.

The format changes ONE rounding -- what is stored -- and no arithmetic, so every kernel-level statement is exact:
  writers: the same launch with fp32 c and with C16 leaves bit-identical gates and h planes, and the C16 buffer holds c32.half()
    element for element (padded slots included: zero where the fp32 format has zero);
  readers: a BPTT on a C16 buffer and on an fp32 buffer holding c.half().float() leaves bit-identical d(gates), clean status words;
  fall-backs: the predicated streaming launches behind a (forced) time-out of cluster2 / the pair kernel repair C16 buffers to the
    streaming kernels' own bits.
Model level (4 rows x 1 s, 2 repeats, FiLM, multi_fuse), WESEP_C16=1 against =0: the forward is unchanged (waveforms and loss
bit-identical); every gradient moves by at most 2e-4 relative L2 -- the CPU emulation of this rounding (tools/r04_h2_numerics.py,
probe bit 4, everything else fp32) moved the worst tensor by 4.7e-5 at the fixture size and 2.2e-5 at 251 frames; the bound is
that with a margin of 4, between the prediction and the 1e-3 the full-size steps are held to.  Peak memory of the step falls by
half of the cell buffers."""
import gc

import pytest
import torch

from wesep_amd import _lib as L

pytestmark = pytest.mark.gpu

H, N = 256, 128


def _cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def bits(t):
    return t.contiguous().view(torch.int32)


def _seq(view, R, K, Tf):
    from wesep_amd.functional import _view_maps
    return _view_maps(view, R, K, Tf, N)[2]


def _weights(g, d):
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    w = dict(wih_f=rnd(4 * H, N, scale=0.08), wih_r=rnd(4 * H, N, scale=0.08), whh_f=rnd(4 * H, H, scale=0.06),
             whh_r=rnd(4 * H, H, scale=0.06))
    return {k: v.to(d) for k, v in w.items()}


def _extreme_bias(g, zero=False):
    """b_ih + b_hh of both directions [2 * 4H] (column = dir * 4H + gate * H + unit).  Units 5 and 6: i, f, g saturated, so |c_t|
    grows by one per step (above 2 from the third step); units 9 and 10: i and f shut (sigmoid(-12) = 6e-6), so 0 < |c| < 6e-5:
    fp16 subnormals.  The recurrent part moves a pre-activation by about +-1: neither leaves its range."""
    b = torch.zeros(2, 4, H) if zero else torch.randn(2, 4, H, generator=g) * 0.2
    if not zero:
        b[:, 0:3, 5:7] = 8.0
        b[:, 2, 6] = -8.0             # (a negative run as well)
        b[:, 0:2, 9:11] = -12.0
        b[:, 2, 9], b[:, 2, 10] = 1.0, -1.0
    return b.reshape(-1).contiguous()


def _new(nb, d, c16):
    """gates (unorm16 BLH), cbuf (fp32 BL, NaN-filled / C16 BLH(2H), filled with an fp16 NaN pattern), hcat (two planes)."""
    from wesep_amd import dev
    gh = torch.zeros(dev.blh_floats(nb, 8 * H), device=d)
    if c16:
        c = torch.full((dev.blh_floats(nb, 2 * H),), float("nan"), device=d)        # (0x7fc00000: the upper half is an fp16 NaN ...
        c.view(torch.int32).fill_(0x7E007E00)                                        #  ... both halves now)
    else:
        c = torch.full((nb, 2 * H // 4, 32, 4), float("nan"), device=d)
    h = torch.full((nb, 2 * H // 4, 32, 4), float("nan"), device=d)
    return gh, c, h


def _check_writer(tag, r32, r16, seq, nb, want_extremes=True, padding_zero=True):
    """r32 / r16: (gates, c, h planes) of the same launch with fp32 c / with C16."""
    from wesep_amd import dev
    g32, c32, h32 = r32
    g16, c16, h16 = r16
    assert not torch.isnan(c32).any(), tag
    assert torch.equal(bits(g32), bits(g16)), f"{tag}: gates differ between the two cell formats"
    assert torch.equal(bits(h32), bits(h16)), f"{tag}: the planes of h differ between the two cell formats"
    got = c16.reshape(-1)[: nb * 32 * H].view(torch.float16).view(nb, 2 * H // 4, 32, 4)
    want = c32.half()
    same = got.view(torch.int16) == want.view(torch.int16)
    assert bool(same.all()), (tag, int((~same).sum()), got[~same][:6].tolist(), c32[~same][:6].tolist())
    assert torch.equal(dev.blh_f16_unpack(c16, nb, 2 * H), want.float()), tag
    # padded slots (sequence tile * 32 + slot >= nseq): block = tile * L + step
    tile = torch.arange(nb, device=c32.device) // seq.L
    pad = (tile[:, None] * 32 + torch.arange(32, device=c32.device)[None, :]) >= seq.nseq             # [nb][32]
    padm = pad[:, None, :, None].expand_as(got)
    if bool(pad.any()) and padding_zero:
        assert not bool(got[padm].view(torch.int16).any()), f"{tag}: a padded slot is not zero"
    live = c32[~padm].abs()
    big, tiny = int((live > 2.0).sum()), int(((live < 6e-5) & (live > 0)).sum())
    print(f"{tag}: {got.numel()} cells identical to c32.half(); {int(pad.sum())} padded (block, slot) pairs; |c| > 2: {big}, "
          f"0 < |c| < 6e-5: {tiny}, max |c| {float(live.max()):.3f}")
    if want_extremes:
        assert big > 0 and tiny > 0, (tag, big, tiny)


# ---- 1. writers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seqs", ["64", "32"])
@pytest.mark.parametrize("dims", [(2, 3, 48), (2, 5, 22)], ids=["nseq96_L3", "nseq44_L5"])
def test_fused_forward_writes_fp16_cells(seqs, dims, monkeypatch):
    """nseq 96, L 3: three tiles -- the 64-sequence kernel's last workgroup has a dead second tile; nseq 44, L 5: a second tile with
    12 live slots (zero bias there, so that the padded slots -- zero input -- hold exact zeros in either format).  Both fp16-h
    arithmetics (hfmt 1, 5), 64- and 32-sequence kernels."""
    from wesep_amd import dev
    d = _cuda()
    monkeypatch.setenv("WS_FUSED_SEQS", seqs)
    R, K, Tf = dims
    seq = _seq("band", R, K, Tf)
    assert (seq.nseq, seq.L) in ((96, 3), (44, 5))
    nb = dev.bl_num_blocks(seq)
    g = torch.Generator().manual_seed(51)
    w = _weights(g, d)
    padded = seq.nseq % 32 != 0
    bias = _extreme_bias(g, zero=padded).to(d)
    xn = dev.to_blocked(torch.randn(R * K * Tf, N, generator=g).to(d), seq, split=True)
    for hf in (1, 5):
        fp = torch.empty(L.LSTM_FUSED_PACK_FLOATS, device=d)
        dev.lstm_pack_fused(w["wih_f"], w["wih_r"], w["whh_f"], w["whh_r"], fp, hfmt=hf)
        res = {}
        for c16 in (False, True):
            gh, c, h = _new(nb, d, c16)
            dev.lstm_fwd_fused(gh, c, h, xn, fp, bias, seq, gfmt=L.GATES_H2F, hfmt=hf | 8, c16=c16)
            torch.cuda.synchronize()
            res[c16] = (gh, c, h)
        _check_writer(f"fused {seqs}-sequence kernel, hfmt {hf}, nseq {seq.nseq}", res[False], res[True], seq, nb,
                      want_extremes=not padded)


def _stream_case(dims, d, seed=52):
    """Time view: weights, fp32 pre-activations in BL with the extreme units, the normalised input and its bias for cluster2."""
    from wesep_amd import dev
    R, K, Tf = dims
    seq = _seq("time", R, K, Tf)
    nb = dev.bl_num_blocks(seq)
    g = torch.Generator().manual_seed(seed)
    w = _weights(g, d)
    bias = _extreme_bias(g).to(d)
    x = torch.randn(R * K * Tf, N, generator=g).to(d)
    pre = torch.cat([x @ w["wih_f"].t() + bias[:4 * H], x @ w["wih_r"].t() + bias[4 * H:]], 1)
    return seq, nb, w, bias, x, dev.to_blocked(pre, seq)


@pytest.mark.parametrize("mode", [L.LSTM_BF16X3_BLK, L.LSTM_BF16X3_BLK16], ids=["stream32", "s16"])
@pytest.mark.parametrize("dims", [(1, 12, 5), (2, 32, 4)], ids=["nseq12_L5", "nseq64_L4"])
def test_streaming_forward_writes_fp16_cells(mode, dims):
    """The streaming forwards (also the predicated fall-back behind cluster2): nseq 12 has 20 padded slots, whose pre-activations
    are zero -- c = 0 in either format."""
    from wesep_amd import dev
    d = _cuda()
    seq, nb, w, bias, x, pre_bl = _stream_case(dims, d)
    assert (seq.nseq, seq.L) in ((12, 5), (64, 4))
    pf, pb = torch.empty(L.LSTM_PACK_FLOATS, device=d), torch.empty(L.LSTM_PACK_FLOATS, device=d)
    dev.lstm_pack(w["whh_f"], w["whh_r"], pf, pb, mode)
    res = {}
    for c16 in (False, True):
        gh, c, h = _new(nb, d, c16)
        dev.lstm_fwd(gh, c, h, pf, seq, mode, gfmt=L.GATES_H2F, gates_in=pre_bl, h2p=True, c16=c16)
        torch.cuda.synchronize()
        res[c16] = (gh, c, h)
    _check_writer(f"streaming forward, mode {mode}, nseq {seq.nseq}", res[False], res[True], seq, nb)


def _cluster2(seq, nb, w, bias, x, d, c16, rf, dbg=0):
    from wesep_amd import dev
    wcat, bcat = torch.empty(2 * 4 * H * N, device=d), torch.empty(2 * 4 * H, device=d)
    zero = torch.zeros(4 * H, device=d)
    dev.lstm_cat_ih(w["wih_f"], w["wih_r"], bias[:4 * H].contiguous(), zero, bias[4 * H:].contiguous(), zero, N, wcat, bcat)
    xn = dev.to_blocked(x, seq, split=True)
    gh, c, h = _new(nb, d, c16)
    st = torch.zeros(1, device=d, dtype=torch.int32)
    tw = dev.lstm_fwd_cluster2(gh, c, h, xn, wcat, bcat, w["whh_f"], w["whh_r"], seq, status=st, rfmt=rf, h2p=True, c16=c16, dbg=dbg)
    torch.cuda.synchronize()
    return (gh, c, h), tw, st


@pytest.mark.parametrize("rf", [0, 1])
def test_cluster2_writes_fp16_cells(rf):
    """nseq 64, L 4 (one cluster per direction, both tag parities), both recurrent formats.  Skipped where the device cannot hold
    the launch's workgroups co-resident (dev.lstm_cluster_resident, as tests/test_one_h_gpu.py)."""
    from wesep_amd import dev
    d = _cuda()
    seq, nb, w, bias, x, _ = _stream_case((2, 32, 4), d)
    if not dev.lstm_cluster_resident(seq, d):
        pytest.skip("fewer CUs than the cluster launch needs co-resident workgroups")
    res = {}
    for c16 in (False, True):
        res[c16], tw, st = _cluster2(seq, nb, w, bias, x, d, c16, rf)
        assert int(tw.item()) == 0 and int(st.item()) == 0
    _check_writer(f"cluster2 rfmt {rf}", res[False], res[True], seq, nb)


# ---- 2. readers ------------------------------------------------------------------------------------------------------------
def _bptt_case(dims, d):
    """Saved state of a streaming forward (fp32 c), the same cells as a C16 buffer packed on the HOST and as fp32 holding
    c.half().float(), d(hcat) and its amax word."""
    from wesep_amd import dev
    seq, nb, w, bias, x, pre_bl = _stream_case(dims, d, seed=53)
    pf, pb = torch.empty(L.LSTM_PACK_FLOATS, device=d), torch.empty(L.LSTM_PACK_FLOATS, device=d)
    dev.lstm_pack(w["whh_f"], w["whh_r"], pf, pb, L.LSTM_BF16X3_BLK)
    gh, c32, h = _new(nb, d, False)
    dev.lstm_fwd(gh, c32, h, pf, seq, L.LSTM_BF16X3_BLK, gfmt=L.GATES_H2F, gates_in=pre_bl, h2p=True)
    torch.cuda.synchronize()
    c16 = dev.blh_f16_pack(c32).reshape(-1).contiguous()
    assert c16.numel() == dev.blh_floats(nb, 2 * H)
    cr = c32.half().float()
    g = torch.Generator().manual_seed(54)
    dh = dev.to_blocked(torch.randn(seq.nseq * seq.L, 2 * H, generator=g).to(d), seq)
    amax = dh.abs().max().reshape(1).view(torch.int32).clone()
    live = c32.abs()
    assert bool((live > 2.0).any()) and bool(((live < 6e-5) & (live > 0)).any())
    return seq, nb, w, gh, c16, cr, h, dh, amax


READERS = ["pair2", "pair3", "stream0", "stream2", "stream3", "s16"]


def _run_reader(kind, seq, w, gh, cbuf, h, dh, amax, d, c16, dbg=0, run_if=None):
    """One BPTT launch, d(gates) out of place; returns (d(gates), time-out word or None, status word or None)."""
    from wesep_amd import dev
    dg = torch.zeros_like(gh)
    if kind.startswith("pair"):
        rf = int(kind[-1])
        pp = torch.empty(L.LSTM_PACK_FLOATS, device=d)
        dev.lstm_pack_pair(w["whh_f"], w["whh_r"], pp, f16=rf)
        st = torch.zeros(1, device=d, dtype=torch.int32)
        tw = dev.lstm_bwd_pair(gh, cbuf, dh, pp, seq, status=st, gfmt=L.GATES_H2F, dgates=dg, amax=amax, rfmt=rf, c16=c16, dbg=dbg)
        torch.cuda.synchronize()
        return dg, tw, st
    mode = L.LSTM_BF16X3_BLK16 if kind == "s16" else L.LSTM_BF16X3_BLK
    rf = 0 if kind == "s16" else int(kind[-1])
    pack = torch.zeros(L.LSTM_PACK_FLOATS, device=d)
    if rf:
        dev.lstm_pack_bwd_f8(w["whh_f"], w["whh_r"], pack)
    else:
        dev.lstm_pack(w["whh_f"], w["whh_r"], torch.empty(L.LSTM_PACK_FLOATS, device=d), pack, mode)
    dev.lstm_bwd(gh, cbuf, h, dh, pack, seq, mode, gfmt=L.GATES_H2F, dgates=dg, amax=amax, rfmt=rf, c16=c16, run_if=run_if)
    torch.cuda.synchronize()
    return dg, None, None


@pytest.mark.parametrize("kind", READERS)
@pytest.mark.parametrize("dims", [(2, 32, 4), (1, 12, 5)], ids=["nseq64_L4", "nseq12_L5"])
def test_bptt_reads_fp16_cells(kind, dims):
    from wesep_amd import dev
    d = _cuda()
    seq, nb, w, gh, c16, cr, h, dh, amax = _bptt_case(dims, d)
    if kind.startswith("pair") and 4 * (-(-seq.nseq // 32)) > dev.cu_count(d):
        pytest.skip("fewer CUs than the pair launch needs co-resident workgroups")
    gh0 = gh.clone()
    dg16, tw16, st16 = _run_reader(kind, seq, w, gh, c16, h, dh, amax, d, True)
    dg32, tw32, st32 = _run_reader(kind, seq, w, gh, cr, h, dh, amax, d, False)
    for word in (tw16, st16, tw32, st32):
        assert word is None or int(word.item()) == 0, (kind, "time-out / status word")
    assert torch.equal(bits(gh), bits(gh0))                                       # out of place: the saved gates stay
    got = dg16.reshape(-1)[: nb * 32 * 4 * H].view(torch.float16)
    assert bool(torch.isfinite(got).all()) and float(got.float().abs().max()) > 0.0
    assert torch.equal(bits(dg16), bits(dg32)), f"{kind}: d(gates) differ between a C16 buffer and fp32 cells holding c.half().float()"


# ---- 3. the fall-back chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rf", [0, 1])
def test_fallback_behind_cluster2_repairs_fp16_cells(rf):
    """The forced time-out of cluster2 (dbg 8) on C16 buffers, then the predicated streaming forward on the launch's word: gates, c
    and h must be the streaming kernel's own."""
    from wesep_amd import dev
    d = _cuda()
    seq, nb, w, bias, x, pre_bl = _stream_case((2, 32, 4), d)
    if not dev.lstm_cluster_resident(seq, d):
        pytest.skip("fewer CUs than the cluster launch needs co-resident workgroups")
    (gh, c, h), tw, st = _cluster2(seq, nb, w, bias, x, d, True, rf, dbg=8)
    assert int(tw.item()) == 1 and int(st.item()) == 1
    pf, pb = torch.empty(L.LSTM_PACK_FLOATS, device=d), torch.empty(L.LSTM_PACK_FLOATS, device=d)
    dev.lstm_pack(w["whh_f"], w["whh_r"], pf, pb, L.LSTM_BF16X3_BLK)
    dev.lstm_fwd(gh, c, h, pf, seq, L.LSTM_BF16X3_BLK, run_if=tw, gfmt=L.GATES_H2F, gates_in=pre_bl, h2p=True, c16=True)
    gh1, c1, h1 = _new(nb, d, True)
    dev.lstm_fwd(gh1, c1, h1, pf, seq, L.LSTM_BF16X3_BLK, gfmt=L.GATES_H2F, gates_in=pre_bl, h2p=True, c16=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(gh), bits(gh1)) and torch.equal(bits(c), bits(c1)) and torch.equal(bits(h), bits(h1))
    # a clean launch leaves the predicated one empty: nothing is rewritten
    (gh2, c2, h2), tw2, st2 = _cluster2(seq, nb, w, bias, x, d, True, rf)
    assert int(tw2.item()) == 0
    keep = c2.clone()
    dev.lstm_fwd(gh2, c2, h2, pf, seq, L.LSTM_BF16X3_BLK, run_if=tw2, gfmt=L.GATES_H2F, gates_in=pre_bl, h2p=True, c16=True)
    torch.cuda.synchronize()
    assert torch.equal(bits(c2), bits(keep))


@pytest.mark.parametrize("rf", [2, 3])
def test_fallback_behind_the_pair_bptt_repairs_on_fp16_cells(rf):
    """The forced time-out of the pair BPTT (dbg 8) on a C16 buffer, then the predicated streaming BPTT (rfmt 0, as
    blstm_core.blstm_bptt launches it) on the launch's word into the same d(gates): the streaming kernel's own bits."""
    from wesep_amd import dev
    d = _cuda()
    seq, nb, w, gh, c16, cr, h, dh, amax = _bptt_case((2, 32, 4), d)
    if 4 * (-(-seq.nseq // 32)) > dev.cu_count(d):
        pytest.skip("fewer CUs than the pair launch needs co-resident workgroups")
    pp = torch.empty(L.LSTM_PACK_FLOATS, device=d)
    dev.lstm_pack_pair(w["whh_f"], w["whh_r"], pp, f16=rf)
    pb = torch.empty(L.LSTM_PACK_FLOATS, device=d)
    dev.lstm_pack(w["whh_f"], w["whh_r"], torch.empty(L.LSTM_PACK_FLOATS, device=d), pb, L.LSTM_BF16X3_BLK)
    st = torch.zeros(1, device=d, dtype=torch.int32)
    dg = torch.zeros_like(gh)
    tw = dev.lstm_bwd_pair(gh, c16, dh, pp, seq, status=st, gfmt=L.GATES_H2F, dgates=dg, amax=amax, rfmt=rf, c16=True, dbg=8)
    dev.lstm_bwd(gh, c16, h, dh, pb, seq, L.LSTM_BF16X3_BLK, gfmt=L.GATES_H2F, dgates=dg, amax=amax, run_if=tw, c16=True)
    torch.cuda.synchronize()
    assert int(tw.item()) == 1 and int(st.item()) == 1
    own, _, _ = _run_reader("stream0", seq, w, gh, c16, h, dh, amax, d, True)
    assert torch.equal(bits(dg), bits(own))
    assert bool(torch.isfinite(dg.reshape(-1)[: nb * 32 * 4 * H].view(torch.float16)).all())


# ---- 4. / 5. model level and the plan -------------------------------------------------------------------------------------
C16_GRAD_MOVE = 2e-4      # 4 x the CPU probe's worst tensor (4.7e-5, module docstring); measured worst on the MI355X: 5.84e-5


def test_training_step_fp16_cells_vs_fp32_cells(monkeypatch):
    """4 rows x 1 s, 2 repeats, FiLM, multi_fuse; WESEP_C16=1 against =0 from the same seed."""
    from oracle import bsrnn_oracle as O
    import wesep_amd.functional as F_
    from wesep_amd.functional import SISDRFn
    from tests.test_bsrnn_gpu import _build, _oracle_run
    d = _cuda()
    kw = dict(num_repeat=2, spk_fuse_type="FiLM", multi_fuse=True, use_spk_transform=False)
    wav, tgt, emb = O.synth_batch(4, 16000, 11)
    real = F_.blstm_forward
    seen = []

    def spy(plan, *a, **k):
        out, saved = real(plan, *a, **k)
        seen.append((plan, saved[1].numel()))
        return out, saved

    monkeypatch.setattr(F_, "blstm_forward", spy)
    res = {}
    wav_d, tgt_d, emb_d = wav.to(d), tgt.to(d), emb.to(d)
    # (peak of an arm = its high-water mark above what is allocated when it starts; an unmeasured step first, so that what the
    #  process keeps for good exists before either measured arm -- as tests/test_film_fold_gpu.py)
    for label, on in (("warm", "1"), ("1", "1"), ("0", "0")):
        monkeypatch.setenv("WESEP_C16", on)
        seen.clear()
        cfg, params, model = _build(kw, 8, d)
        model.train()
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        est, _ = model(wav_d, emb_d)
        loss = SISDRFn.apply(est, tgt_d, 1e-8)
        loss.backward()
        torch.cuda.synchronize()
        res[label] = dict(est=est.detach().cpu(), loss=loss.detach().cpu(), peak=torch.cuda.max_memory_allocated() - base,
                          grads={n: p.grad.detach().cpu() for n, p in model.named_parameters()}, plans=list(seen))
        del model, est, loss
    on, off = res["1"], res["0"]
    assert len(on["plans"]) == 4 and len(off["plans"]) == 4                      # 2 repeats x (time, band)
    for plan, numel in on["plans"]:
        assert plan.c16 and numel == plan.nb * 32 * H, (plan, numel)              # BLH(2H): half the floats
    for plan, numel in off["plans"]:
        assert not plan.c16 and numel == plan.nb * 32 * 2 * H, (plan, numel)      # WESEP_C16=0: fp32 cells
    assert torch.equal(on["est"], off["est"]) and torch.equal(on["loss"], off["loss"])          # the forward is unchanged
    _, _, grads_o = _oracle_run(cfg, params, wav, tgt, emb)
    worst = worst_on = worst_off = 0.0
    for n in on["grads"]:
        move, e_on, e_off = rel(on["grads"][n], off["grads"][n]), rel(on["grads"][n], grads_o[n]), rel(off["grads"][n], grads_o[n])
        print(f"  {n}: C16 vs fp32 cells {move:.2e}; vs the oracle {e_on:.2e} (fp32 cells: {e_off:.2e})")
        worst, worst_on, worst_off = max(worst, move), max(worst_on, e_on), max(worst_off, e_off)
    half = sum(plan.nb * 32 * 2 * H * 2 for plan, _ in on["plans"])
    print(f"C16 model step: worst gradient move {worst:.2e} (bound {C16_GRAD_MOVE:.0e}); worst vs the oracle {worst_on:.2e} with "
          f"fp16 cells, {worst_off:.2e} with fp32 cells; peak above the arm's start {on['peak'] / 1e6:.2f} MB against "
          f"{off['peak'] / 1e6:.2f} MB (difference {(off['peak'] - on['peak']) / 1e6:.2f} MB; half of the cell buffers is {half / 1e6:.2f} MB)")
    assert worst <= C16_GRAD_MOVE, worst           # measured on the MI355X: 5.84e-5 (worst vs the oracle 9.96e-4 against 9.89e-4 with fp32 cells)
    assert abs((off["peak"] - on["peak"]) - half) <= 0.1 * half, (on["peak"], off["peak"], half)


def test_plans_that_keep_fp32_cells(monkeypatch):
    """Longer than 32768 steps (|c_t| <= t must stay inside fp16), ragged batches and WESEP_C16=0 keep fp32 cells; the plan is what
    blstm_forward allocates by (test_training_step_fp16_cells_vs_fp32_cells checks the buffers of both kinds)."""
    from wesep_amd import dev
    from wesep_amd.blstm_core import make_plan
    d = _cuda()
    monkeypatch.delenv("WESEP_C16", raising=False)
    band, time = _seq("band", 4, 32, 126), _seq("time", 4, 32, 126)
    for seq in (band, time):
        plan = make_plan(seq, d, True)
        assert plan.c16 and plan.h2p, plan
        assert not make_plan(seq, d, False).c16                                   # no backward: no saved cells to narrow
        assert not make_plan(seq, d, True, ragged=True).c16
    long_ = dev.SeqMap(64, dev.BIG, 0, 32769, 1, 32769)
    assert make_plan(long_._replace(L=32768, s2=32768), d, True).c16
    assert not make_plan(long_, d, True).c16
    monkeypatch.setenv("WESEP_C16", "0")
    for seq in (band, time):
        assert not make_plan(seq, d, True).c16
