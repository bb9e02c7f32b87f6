"""Autograd boundary of the pBSRNN hot path: torch.autograd.Function shims whose forward and
backward are sequences of C-ABI launches (wesep_amd/dev.py).  PyTorch supplies device memory,
the stream, and the autograd graph between these coarse ops (so DistributedDataParallel's
bucket hooks fire on the registered Parameters); every FLOP runs in libwesep_hip.so.

Activation layout everywhere: Z = [R, K, Tf, N] fp32 (see include/wesep_hip.h)."""
import os

import numpy as np
import torch

from . import _lib as L
from . import dev
from .dev import BIG, Geom, Rows, SeqMap, StatMap, flat
# the blocked BLSTM core (plan, packs, steps) and the side-stream hand-over of its weight gradients live in blstm_core; the
# names below stay importable from here
from .blstm_core import (G4, H, PAIR_STAMPS, PackCache, WeightPacks, WGradBox, WGradCarrierFn, _NO_CACHE,  # noqa: F401
                         _PROBE_SAT, _cluster_dbg, _empty, _h2_probe, _pair_dbg, _pending, _probe_round, _reduce_new,
                         _side_stream, amax_word, band_dx, band_rfmt, blstm_bptt, blstm_dxn, blstm_forward,
                         blstm_weight_grads, consume_once, defer_wgrad, dxn_fmt, flush_deferred_wgrads, keep_for_side,
                         make_plan, mark_wgrads_ready, pair_rfmt, tnb_a16, weight_grads, wgrad_hold, zero_words)

NBIN = 257
HOP = 128


def _need_cuda(t, who):
    if not t.is_cuda:
        raise L.WesepHipError(f"{who}: wesep_amd has no CPU path; move the model and inputs to the GPU")


# ---------------------------------------------------------------------------------------------
# ResRNN: GroupNorm -> BLSTM -> Linear -> +residual   (wesep/models/bsrnn.py:38-46)
# ---------------------------------------------------------------------------------------------
def _view_maps(view, R, K, Tf, N):
    if view == "time":      # band_rnn: sequences (r,k), steps over t  (bsrnn.py:73-75)
        geo = Geom(R * K, 1, Tf * N, 0, N, Tf, N)
        smap = StatMap(Tf, 1, 1, 0, 0)
        seq = SeqMap(R * K, BIG, 0, Tf, 1, Tf)
        shift = (1, Tf)                     # (seq_div, seq_len) of the h_{t-1} row shift
    elif view == "band":    # band_comm: sequences (r,t), steps over k  (bsrnn.py:78-81)
        geo = Geom(R * Tf, Tf, K * Tf * N, N, Tf * N, K, N)
        smap = StatMap(K * Tf, Tf, Tf, 1, 0)
        seq = SeqMap(R * Tf, Tf, K * Tf, 1, Tf, K)
        shift = (Tf, K)
    else:
        raise ValueError(view)
    return geo, smap, seq, shift


class ResRNNFn(torch.autograd.Function):
    """inputs: z, view, norm.weight, norm.bias, weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0,
    the four *_reverse tensors, proj.weight, proj.bias."""

    @staticmethod
    def forward(ctx, z, view, norm_w, norm_b, wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r,
                bhh_r, proj_w, proj_b):
        _need_cuda(z, "ResRNN")
        z = z.contiguous()
        R, K, Tf, N = z.shape
        if tuple(whh_f.shape) != (G4, H) or tuple(wih_f.shape) != (G4, N):
            raise L.WesepHipError(f"ResRNN kernels are built for hidden {H}; got {tuple(whh_f.shape)}")
        P = R * K * Tf
        d = z.device
        geo, smap, seq, _ = _view_maps(view, R, K, Tf, N)
        stats = _empty(d, geo.ngroups, 2)
        dev.group_stats(z, geo, stats)
        wcat, bcat = _empty(d, 2 * G4, N), _empty(d, 2 * G4)
        dev.lstm_cat_ih(wih_f.contiguous(), wih_r.contiguous(), bih_f, bhh_f, bih_r, bhh_r, N, wcat, bcat)
        pack_f, pack_b = _empty(d, L.LSTM_PACK_FLOATS), _empty(d, L.LSTM_PACK_FLOATS)
        mt = dev.lstm_mode(seq.nseq)
        dev.lstm_pack(whh_f.contiguous(), whh_r.contiguous(), pack_f, pack_b, mt)
        gates = _empty(d, P, 2 * G4)
        dev.gemm_nt(A=z, a_rows=flat(N), M=P, N=2 * G4, K=N, W=wcat, ldw=N, bias=bcat, C_out=gates,
                    c_rows=flat(2 * G4), stats=stats, gamma=norm_w, beta=norm_b, stat_map=smap)
        cbuf, hcat = _empty(d, P, 2 * H), _empty(d, P, 2 * H)
        dev.lstm_fwd(gates, cbuf, hcat, pack_f, seq, mt)
        out = torch.empty_like(z)
        pw = proj_w.contiguous()
        dev.gemm_nt(A=hcat, a_rows=flat(2 * H), M=P, N=N, K=2 * H, W=pw, ldw=2 * H, bias=proj_b,
                    R=z, C_out=out, c_rows=flat(N))
        ctx.save_for_backward(z, stats, gates, cbuf, hcat, wcat, pack_b, norm_w, norm_b, pw)
        ctx.view, ctx.mt = view, mt
        return out

    @staticmethod
    def backward(ctx, dout):
        z, stats, gates, cbuf, hcat, wcat, pack_b, norm_w, norm_b, pw = ctx.saved_tensors
        dout = dout.contiguous()
        R, K, Tf, N = z.shape
        P = R * K * Tf
        d = z.device
        geo, smap, seq, (seq_div, seq_len) = _view_maps(ctx.view, R, K, Tf, N)
        nsplit, rps = dev.tn_splits(P)
        # projection: data + weight gradients
        projT = _empty(d, 2 * H, N)
        dev.transpose(pw, N, 2 * H, 2 * H, projT)
        dhcat = _empty(d, P, 2 * H)
        dev.gemm_nt(A=dout, a_rows=flat(N), M=P, N=2 * H, K=N, W=projT, ldw=N, C_out=dhcat,
                    c_rows=flat(2 * H))
        slab, bslab = _empty(d, nsplit, N * 2 * H), _empty(d, nsplit, N)
        dev.gemm_tn(G=dout, g_rows=flat(N), A=hcat, a_rows=flat(2 * H), M=P, Nn=N, Kk=2 * H, slab=slab,
                    slab_stride=N * 2 * H, bslab=bslab, bslab_stride=N, nsplit=nsplit, rows_per_split=rps)
        dproj_w = _reduce_new(slab, nsplit, N * 2 * H, (N, 2 * H))
        dproj_b = _reduce_new(bslab, nsplit, N, (N,))
        # BPTT: gates (activated) -> d(pre-activation gates), in place
        dev.lstm_bwd(gates, cbuf, hcat, dhcat, pack_b, seq, ctx.mt)
        del dhcat
        # recurrent weight gradients: dW_hh[d] = dgates_d^T h_{t-1}
        dwhh = []
        slab = _empty(d, nsplit, G4 * H)
        for di in (0, 1):
            dev.gemm_tn(G=gates, g_rows=flat(2 * G4), g_off=di * G4, A=hcat, a_rows=flat(2 * H),
                        a_off=di * H, M=P, Nn=G4, Kk=H, slab=slab, slab_stride=G4 * H, nsplit=nsplit,
                        rows_per_split=rps, shift_rows=(-seq.step_rows if di == 0 else seq.step_rows),
                        seq_div=seq_div, seq_len=seq_len)
            dwhh.append(_reduce_new(slab, nsplit, G4 * H, (G4, H)))
        # input weight / bias gradients against the re-normalised input
        slab, bslab = _empty(d, nsplit, 2 * G4 * N), _empty(d, nsplit, 2 * G4)
        dev.gemm_tn(G=gates, g_rows=flat(2 * G4), A=z, a_rows=flat(N), M=P, Nn=2 * G4, Kk=N, slab=slab,
                    slab_stride=2 * G4 * N, bslab=bslab, bslab_stride=2 * G4, nsplit=nsplit,
                    rows_per_split=rps, stats=stats, gamma=norm_w, beta=norm_b, stat_map=smap)
        dwcat = _reduce_new(slab, nsplit, 2 * G4 * N, (2 * G4, N))
        dbcat = _reduce_new(bslab, nsplit, 2 * G4, (2 * G4,))
        del slab, bslab
        # d(normalised input) -> GroupNorm backward (+ residual path)
        wcatT = _empty(d, N, 2 * G4)
        dev.transpose(wcat, 2 * G4, N, N, wcatT)
        dxn = _empty(d, P, N)
        dev.gemm_nt(A=gates, a_rows=flat(2 * G4), M=P, N=N, K=2 * G4, W=wcatT, ldw=2 * G4, C_out=dxn,
                    c_rows=flat(N))
        ab = _empty(d, geo.ngroups, 2)
        dev.gn_bwd_reduce(z, dxn, stats, geo, ab, gamma=norm_w)
        ns2 = min(256, geo.ngroups)
        pslab = _empty(d, ns2, 2, N)
        dev.gn_param_grad(z, dxn, stats, geo, ns2, pslab)
        dgb = _reduce_new(pslab, ns2, 2 * N, (2, N))
        dz = torch.empty_like(z)
        dev.gn_bwd_apply(z, dxn, stats, ab, geo, dz, gamma=norm_w, res=dout)
        # b_ih and b_hh receive the same gradient; clone so their .grad never alias
        return (dz, None, dgb[0], dgb[1],
                dwcat[:G4], dwhh[0], dbcat[:G4], dbcat[:G4].clone(),
                dwcat[G4:], dwhh[1], dbcat[G4:], dbcat[G4:].clone(),
                dproj_w, dproj_b)


def resrnn_mode() -> str:
    """'blocked' (default): split-bf16 path on the blocked layout BL (gemm_blk.hip, lstm_bf16.hip);
    'plain': the generic row-addressed GEMMs + plain-layout recurrence (honours WESEP_GEMM /
    WESEP_LSTM, e.g. both f32 for the exact-fp32 reference path)."""
    return os.environ.get("WESEP_RESRNN", "blocked")


def wgrad_overlap() -> bool:
    """Weight-gradient GEMMs of the blocked ResRNN on a side stream (default on; WESEP_WGRAD_OVERLAP=0
    keeps everything on the current stream)."""
    return os.environ.get("WESEP_WGRAD_OVERLAP", "1") != "0"


_TIME_LEFT = {}   # device key -> time-view ResRNNs of the current graph whose backward (with a carrier) has not run yet


def reset_deferred_wgrads(device):
    """Drop deferred jobs (start of a step: a failed backward may have left some behind)."""
    _pending(device).clear()
    _TIME_LEFT[(device.type, device.index)] = 0


def tail_flush() -> bool:
    """Release the LAST time-view layer's own weight-gradient jobs right behind its BPTT instead of leaving them to the carriers
    (default on; WESEP_TAIL_FLUSH=0): no further pair BPTT follows to hide them under, and the main stream used to sit out their
    1.4 ms at the end of every backward (profiles/r06_bsrnn_trace_gaps.txt: 'idle between gemm_tn_bf16 -> fill')."""
    return os.environ.get("WESEP_TAIL_FLUSH", "1") != "0"


def film_fold(z) -> bool:
    """The speaker-fusion affine in front of a time-view ResRNN is FOLDED into that ResRNN (default on; WESEP_FILM_FOLD=0
    restores the affine_fwd / affine_bwd launches): its five consumers -- statistics, relay, the projection's residual, the two
    GroupNorm backward passes -- form z' = z * (a0 + a[r]) + b[r] in registers from z (dev.Film), the backward apply pass
    multiplies d(z') by a0 + a on the way out and sums (da, db) beside (dgamma, dbeta): two passes over Z per fuse layer and
    one saved copy of Z are gone.  z: the [R, K, Tf, N] input of the fuse layer.  Blocked path on a real device only (the host
    emulation and the ABI dry run keep the unfolded launches), and only where the time view's GroupNorm backward is the
    reduce + apply pair that carries the fold (dev.gn_bwd_apply_pg_ok, not the one-wave kernel of short groups)."""
    if os.environ.get("WESEP_FILM_FOLD", "1") == "0" or not (z.is_cuda and torch.cuda.is_available()):
        return False
    if resrnn_mode() != "blocked" or z.dim() != 4 or z.shape[3] != 128:
        return False
    geo = _view_maps("time", *z.shape)[0]
    return dev.gn_bwd_apply_pg_ok(geo) and not dev.gn_bwd_fused_ok(geo)


def _resrnn_blk_fwd(z, view, norm_w, norm_b, wparams, cache, grad, frames=None, film=None):
    """The launches of ResRNNBlkFn.forward: statistics, plan, packs, the blocked BLSTM.  z contiguous [R, K, Tf, N].
    frames (ragged batches, inference): int32 device table [R] of the rows' valid frames -- the time view's statistics
    cover them only and its pre-activations behind them are zeros (blstm_forward's `steps`); the band view is per frame
    and ignores it.  film (dev.Film, time view): z is the input of a folded speaker-fusion affine -- every consumer below reads
    film(z), `out` is film(z) + Linear(BLSTM(GroupNorm(film(z)))).  Returns (out, stats, plan, W, saved)."""
    _need_cuda(z, "ResRNN")
    wih_f, whh_f, proj_b = wparams[0], wparams[1], wparams[9]
    R, K, Tf, N = z.shape
    if tuple(whh_f.shape) != (G4, H) or tuple(wih_f.shape) != (G4, N) or N != 128:
        raise L.WesepHipError(f"blocked ResRNN kernels are built for input 128 / hidden {H}; got "
                              f"{tuple(wih_f.shape)}, {tuple(whh_f.shape)}")
    d = z.device
    geo, smap, seq, _ = _view_maps(view, R, K, Tf, N)
    ragged = frames is not None and view == "time"
    if film is not None and (view != "time" or frames is not None):
        raise L.WesepHipError("ResRNN: the folded speaker-fusion affine belongs to the time view of rectangular batches")
    fk = dict(film=film) if film is not None else {}
    stats = _empty(d, geo.ngroups, 2)
    if ragged:
        dev.group_stats(z, geo, stats, glen=frames, glen_div=K)
    else:
        dev.group_stats(z, geo, stats, **fk)
    cache = cache if cache is not None else _NO_CACHE
    sig = cache.begin(wparams)
    plan = make_plan(seq, d, grad, gn_geo=geo, ragged=ragged) if ragged else make_plan(seq, d, grad, gn_geo=geo)
    W = WeightPacks(cache, sig, plan.lmode, plan.pair_rfmt, *wparams[:9])
    steps = dict(steps=(frames, K)) if ragged else {}
    out, saved = blstm_forward(plan, W, z, seq, res=z, bias=proj_b,
                               norm=dict(stats=stats, gamma=norm_w, beta=norm_b, stat_map=smap), **steps, **fk)
    return out, stats, plan, W, saved


class ResRNNBlkFn(torch.autograd.Function):
    """ResRNN on the blocked layout: gates / c / h / d(h) never exist in row-major form; every
    activation byte of the recurrence moves as part of a 512-byte contiguous run (include/wesep_hip.h,
    "blocked layout BL").  Same inputs as ResRNNFn.  The BLSTM + projection are blstm_core's steps; this node owns the view's
    maps, the GroupNorm (statistics in front, its backward behind) and the time view's bookkeeping of deferred jobs."""

    @staticmethod
    def forward(ctx, z, dummy, box, cache, view, norm_w, norm_b, wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r,
                bhh_r, proj_w, proj_b, film_a=None, film_b=None, film_a0=1.0):
        """dummy/box: None, or the output and the box of this ResRNN's WGradCarrierFn -- then the ten
        LSTM / proj tensors are passed detached and their gradients travel through the box.  cache: the owning
        module's PackCache or None.  film_a / film_b [R, N] (either may be None), film_a0: a folded speaker-fusion affine in front
        (film_fold): z is ITS input, saved as it is -- no z' exists --, and the backward returns d(z), d(film_a), d(film_b)."""
        z = z.contiguous()
        d = z.device
        film = None
        if film_a is not None or film_b is not None:
            film_a = film_a.contiguous() if film_a is not None else None
            film_b = film_b.contiguous() if film_b is not None else None
            film = dev.Film(film_a, film_b, float(film_a0), z.shape[1] * z.shape[2])
        out, stats, plan, W, saved = _resrnn_blk_fwd(
            z, view, norm_w, norm_b, (wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r, bhh_r, proj_w, proj_b), cache,
            any(ctx.needs_input_grad), film=film)
        ctx.save_for_backward(z, stats, norm_w, *saved, film_a, film_b)
        ctx.film_a0 = float(film_a0)
        if view == "time" and box is not None and plan.grad:
            key = (d.type, d.index)
            _TIME_LEFT[key] = _TIME_LEFT.get(key, 0) + 1
        ctx.view, ctx.box, ctx.plan, ctx.packs = view, box, plan, W
        ctx.consumed = False
        return out

    @staticmethod
    def backward(ctx, dout):
        consume_once(ctx, "ResRNN")
        z, stats, norm_w, gates, cbuf, hcat, xn, hcat16, film_a, film_b = ctx.saved_tensors   # (xn: fp16 copy if hcat16)
        plan, W, box = ctx.plan, ctx.packs, ctx.box
        dout = dout.contiguous()
        R, K, Tf, N = z.shape
        P = R * K * Tf
        d = z.device
        geo, smap, seq, _ = _view_maps(ctx.view, R, K, Tf, N)
        # a time-view recurrence leaves half of the chip idle: the weight-gradient jobs deferred by the previous layers are
        # released right after it is launched
        dg, dout_bl, amax, dxn2 = blstm_bptt(plan, W, gates, cbuf, hcat, dout, seq, release=ctx.view == "time")
        wg = blstm_weight_grads(plan, dg, xn, hcat, dout_bl, amax, hcat16, seq, box)
        del dout_bl
        if box is not None and ctx.view == "time":
            key = (d.type, d.index)
            _TIME_LEFT[key] = _TIME_LEFT.get(key, 1) - 1
            if _TIME_LEFT[key] <= 0 and tail_flush():
                flush_deferred_wgrads(d)     # the graph's last time-view layer: nothing left to hide its jobs under
        # d(normalised input) = dgates Wcat -> GroupNorm backward (+ residual path)
        dxn, dxn_r = blstm_dxn(plan, W, dg, amax, dxn2, seq, P)
        dz = torch.empty_like(z)
        # (dgamma, dbeta): summed by the LAST workgroup of the kernel that produced the partials (wesep_hip.h, ABI v15) --
        # a separate ws_reduce_slabs launch on this stream can sit out a whole weight-gradient GEMM of the side stream
        # before its four workgroups get a CU (round 3: 7 ms per step in 62 such launches)
        dgb = _empty(d, 2, N)
        da = db = None
        if film_a is not None or film_b is not None:
            # folded speaker-fusion affine (film_fold: time view, the reduce + apply pair): xhat from film(z) in both passes; the
            # apply pass writes d(z) = d(z') * (a0 + a) and sums (da, db) per row beside (dgamma, dbeta) -- affine_bwd's pass over
            # d(z') and z does not exist
            film = dev.Film(film_a, film_b, ctx.film_a0, K * Tf)
            ab = _empty(d, geo.ngroups, 2)
            dev.gn_bwd_reduce(z, dxn, stats, geo, ab, gamma=norm_w, film=film)
            pslab = _empty(d, geo.ngroups + dev.tree_groups(geo.ngroups), 2, N)
            da = _empty(d, R, N) if film_a is not None else None
            db = _empty(d, R, N) if film_b is not None else None
            dev.gn_bwd_apply_pg(z, dxn, stats, ab, geo, dz, norm_w, pslab, dgb, zero_words(d, 1 + dev.tree_groups(geo.ngroups)),
                                res=dout, film=film, fslab=_empty(d, geo.ngroups, 2, N), da=da, db=db, fcounter=zero_words(d, R))
        elif dev.gn_bwd_fused_ok(geo):
            # band view: 16 032 groups of 16 KB -- one wave per group, x / dxn / dout cross HBM once (norm.hip)
            ns2 = min(1024, -(-geo.ngroups // 4))
            pslab = _empty(d, ns2 + dev.tree_groups(ns2), 2, N)
            dev.gn_bwd_fused(z, dxn, stats, geo, norm_w, dz, ns2, pslab, res=dout, pout=dgb,
                             counter=zero_words(d, 1 + dev.tree_groups(ns2)), dxn2=dxn_r)
        elif dev.gn_bwd_apply_pg_ok(geo):
            # time view: 1 024 groups of 256 KB: the group means first, then apply + parameter sums in ONE pass over x / dxn
            ab = _empty(d, geo.ngroups, 2)
            dev.gn_bwd_reduce(z, dxn, stats, geo, ab, gamma=norm_w)
            pslab = _empty(d, geo.ngroups + dev.tree_groups(geo.ngroups), 2, N)
            dev.gn_bwd_apply_pg(z, dxn, stats, ab, geo, dz, norm_w, pslab, dgb, zero_words(d, 1 + dev.tree_groups(geo.ngroups)),
                                res=dout)
        else:
            ab = _empty(d, geo.ngroups, 2)
            dev.gn_bwd_reduce(z, dxn, stats, geo, ab, gamma=norm_w)
            ns2 = min(1024, geo.ngroups)
            pslab = _empty(d, ns2, 2, N)
            dev.gn_param_grad(z, dxn, stats, geo, ns2, pslab)
            dev.gn_bwd_apply(z, dxn, stats, ab, geo, dz, gamma=norm_w, res=dout)
            dgb = _reduce_new(pslab, ns2, 2 * N, (2, N))
        gd = torch.zeros((), device=d) if box is not None else None
        return (dz, gd, None, None, None, dgb[0], dgb[1]) + tuple(wg) + (da, db, None)


def pack_prefetch() -> bool:
    """Derived weight forms of every ResRNN built AHEAD on the side stream at the start of a training forward (opt-in:
    WESEP_PACK_PREFETCH=1; default: each is built on the main stream when it is first asked for).  The weights change every
    step, so every step rebuilds ~90 packs -- launches of 5 us, each with the 6 us gap of a dependent launch in front of it:
    about 1 ms per step of the main queue on paper, in the forward, where the side stream has nothing to do.  Measured
    (profiles/r06_summary.md): -0.27 ms in one alternating A/B, 0.0 in the next -- the main queue loses 84 launches per step and
    the forward recurrences run 0.2 ms longer beside the pack kernels: overlap on this chip is close to zero-sum once more.
    Bit-identical either way (tests/test_bsrnn_gpu.py); off by default because it buys nothing measurable."""
    return os.environ.get("WESEP_PACK_PREFETCH", "0") == "1"


def prefetch_packs(layers):
    """layers: (PackCache, the ten LSTM / proj tensors in ResRNNFn order) of every ResRNN, in forward order.  Builds, on the side
    stream and behind everything enqueued so far on the current one (the optimizer's update of these weights), the packs each
    cache was asked for under its previous signature.  The consumer waits for the layer's event when it first asks (PackCache.get).
    Allocation: the packs come from the side stream's pool and go back to it when the signature moves -- at the next prefetch,
    which again stands behind an event of the consumer stream recorded after the consumer's last use."""
    layers = [(c, p) for c, p in layers if c is not None and c.lmode is not None and p[0].is_cuda]
    if not layers or not pack_prefetch() or not torch.cuda.is_available():
        return
    d = layers[0][1][0].device
    todo = []
    for cache, params in layers:
        sig = cache.begin(params)
        if cache.kinds_prev and not cache.items:
            todo.append((cache, sig, params))
    if not todo:
        return
    side = _side_stream(d)
    gate = torch.cuda.Event()
    gate.record(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(side):
        side.wait_event(gate)
        for cache, sig, params in todo:
            W = WeightPacks(cache, sig, cache.lmode, cache.pair_rf, *(p.detach() for p in params[:9]))
            for kind in list(cache.kinds_prev):
                W(kind)
            ready = torch.cuda.Event()
            ready.record(side)
            cache.ready, cache.waited = ready, {side.cuda_stream}


def make_wgrad_carrier(params, blocked=None):
    """(dummy, box) for one ResRNN, or None when the side-stream hand-over does not apply.  `params`:
    the ten LSTM / proj tensors in ResRNNFn order (TF-GridNet's BlstmLinearBlkFn: its eight padded weight tensors, in
    the order of its own arguments; blocked=True there -- the caller has checked its own path).  Must be called BEFORE
    the forward of every ResRNN of the step (see WGradCarrierFn)."""
    if blocked is None:
        blocked = resrnn_mode() == "blocked"
    if not (wgrad_overlap() and blocked and torch.is_grad_enabled()
            and params[0].is_cuda and all(p.requires_grad for p in params)):
        return None
    box = WGradBox()
    return WGradCarrierFn.apply(box, *params), box


def resrnn(z, view, norm_w, norm_b, *params, carrier=None, cache=None, frames=None, film=None):
    """ResRNN forward (autograd-aware) on the path selected by WESEP_RESRNN.  cache: the owning module's PackCache.
    frames (ragged batches): int32 device table [R] of the rows' valid frames; inference on the blocked path only.
    film: (a, b, a0) of a speaker-fusion affine folded into this (time-view, blocked) ResRNN -- the caller asked film_fold()."""
    if film is not None and (frames is not None or resrnn_mode() != "blocked" or view != "time"):
        raise L.WesepHipError("resrnn: film= goes with the time view of the blocked path (functional.film_fold)")
    fa, fb, fa0 = film if film is not None else (None, None, 1.0)
    if frames is not None:
        if torch.is_grad_enabled() or resrnn_mode() != "blocked":
            raise L.WesepHipError("ResRNN: per-row lengths are an inference feature of the blocked path "
                                  "(torch.no_grad(), WESEP_RESRNN=blocked); training batches are cropped by the collate function")
        return _resrnn_blk_fwd(z.contiguous(), view, norm_w, norm_b, tuple(p.detach() for p in params), cache, False,
                               frames=frames)[0]
    if resrnn_mode() != "blocked":
        return ResRNNFn.apply(z, view, norm_w, norm_b, *params)
    if carrier is None:
        return ResRNNBlkFn.apply(z, None, None, cache, view, norm_w, norm_b, *params, fa, fb, fa0)
    dummy, box = carrier
    return ResRNNBlkFn.apply(z, dummy, box, cache, view, norm_w, norm_b, *(p.detach() for p in params), fa, fb, fa0)


# ---------------------------------------------------------------------------------------------
# small dense layers on [R, *] (speaker embedding side): y = x W^T + b
# ---------------------------------------------------------------------------------------------
def _w2d(w):
    return w.reshape(w.shape[0], -1).contiguous()


def _lin_fwd(x, W, b, act=0, w_off=0, ldw=None, K=None):
    M = x.shape[0]
    Nout = W.shape[0]
    K = K if K is not None else W.shape[1]
    ldw = ldw if ldw is not None else W.shape[1]
    y = _empty(x.device, M, Nout)
    vec = 3 if (K % 4 == 0 and ldw % 4 == 0 and w_off % 4 == 0 and x.shape[1] % 4 == 0) else 0
    dev.gemm_nt(A=x, a_rows=flat(x.shape[1]), M=M, N=Nout, K=K, W=W, ldw=ldw, bias=b, C_out=y,
                c_rows=flat(Nout), act=act, vec=vec, w_off=w_off)
    return y


def _lin_bwd_w(dy, x, with_bias=True):
    """dW [Nout, K] = dy^T x, db = colsum(dy); single split (M = R is tiny)."""
    M, Nout = dy.shape
    K = x.shape[1]
    pad = (-Nout) % 4                      # the kernel wants 16-byte G rows (e.g. 251 speaker classes)
    if pad:
        dyp = torch.zeros(M, Nout + pad, device=dy.device, dtype=torch.float32)
        dyp[:, :Nout] = dy
        dy = dyp
    Np = Nout + pad
    rps = -(-M // 32) * 32
    dW = _empty(dy.device, Np, K)
    db = _empty(dy.device, Np) if with_bias else None
    dev.gemm_tn(G=dy, g_rows=flat(Np), A=x, a_rows=flat(K), M=M, Nn=Np, Kk=K, slab=dW,
                slab_stride=Np * K, bslab=db, bslab_stride=Np, nsplit=1, rows_per_split=rps,
                vec=1 if K % 4 == 0 else 0)
    if pad:
        dW = dW[:Nout].contiguous()
        db = db[:Nout].contiguous() if with_bias else None
    return dW, db


def _lin_bwd_x(dy, W, T=None, src_off=0, rows=None, cols=None, lds=None):
    """dx = dy W (optionally * (1 - T^2)); W [rows, cols] with leading dim lds."""
    rows = rows if rows is not None else W.shape[0]
    cols = cols if cols is not None else W.shape[1]
    lds = lds if lds is not None else W.shape[1]
    WT = _empty(dy.device, cols, rows)
    dev.transpose(W, rows, cols, lds, WT, src_off=src_off)
    dx = _empty(dy.device, dy.shape[0], cols)
    vec = 3 if rows % 4 == 0 else 0
    dev.gemm_nt(A=dy, a_rows=flat(rows), M=dy.shape[0], N=cols, K=rows, W=WT, ldw=rows, C_out=dx,
                c_rows=flat(cols), T=T, vec=vec)
    return dx


class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b):
        _need_cuda(x, "Linear")
        x, W2 = x.contiguous(), _w2d(W)
        ctx.save_for_backward(x, W2)
        ctx.wshape = W.shape
        return _lin_fwd(x, W2, b)

    @staticmethod
    def backward(ctx, dy):
        x, W2 = ctx.saved_tensors
        dy = dy.contiguous()
        dW, db = _lin_bwd_w(dy, x)
        dx = _lin_bwd_x(dy, W2) if ctx.needs_input_grad[0] else None
        return dx, dW.view(ctx.wshape), db


class SpkTransformFn(torch.autograd.Function):
    """SpeakerTransform (speaker.py:26-49): Conv1d(k=1) 256->128, 128->128 + Tanh, 128->256."""

    @staticmethod
    def forward(ctx, e, w0, b0, w1, b1, w3, b3):
        _need_cuda(e, "SpeakerTransform")
        e = e.contiguous()
        W0, W1, W3 = _w2d(w0), _w2d(w1), _w2d(w3)
        h0 = _lin_fwd(e, W0, b0)
        h1 = _lin_fwd(h0, W1, b1, act=1)
        y = _lin_fwd(h1, W3, b3)
        ctx.save_for_backward(e, h0, h1, W0, W1, W3)
        ctx.shapes = (w0.shape, w1.shape, w3.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        e, h0, h1, W0, W1, W3 = ctx.saved_tensors
        dy = dy.contiguous()
        dW3, db3 = _lin_bwd_w(dy, h1)
        dp1 = _lin_bwd_x(dy, W3, T=h1)           # d(pre-tanh) of layer 1
        dW1, db1 = _lin_bwd_w(dp1, h0)
        dh0 = _lin_bwd_x(dp1, W1)
        dW0, db0 = _lin_bwd_w(dh0, e)
        de = _lin_bwd_x(dh0, W0) if ctx.needs_input_grad[0] else None
        s0, s1, s3 = ctx.shapes
        return de, dW0.view(s0), db0, dW1.view(s1), db1, dW3.view(s3), db3


# ---------------------------------------------------------------------------------------------
# speaker fusion on Z: out = z * (a0 + a[r]) + b[r]      (speaker.py:81-125, norm.py:118-139)
# ---------------------------------------------------------------------------------------------
def _affine_splits(rows_per_r):
    return max(1, min(64, rows_per_r // 256))


class AffineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, a, b, a0):
        _need_cuda(z, "SpeakerFuse")
        z = z.contiguous()
        R, K, Tf, N = z.shape
        a = a.contiguous() if a is not None else None
        b = b.contiguous() if b is not None else None
        out = torch.empty_like(z)
        dev.affine_fwd(z, a, b, a0, R * K * Tf, K * Tf, N, out)
        ctx.save_for_backward(z, a)
        ctx.a0, ctx.has_b = a0, b is not None
        return out

    @staticmethod
    def backward(ctx, dout):
        z, a = ctx.saved_tensors
        dout = dout.contiguous()
        R, K, Tf, N = z.shape
        ns = _affine_splits(K * Tf)
        da_slab = _empty(z.device, ns, R, N) if a is not None else None
        db_slab = _empty(z.device, ns, R, N) if ctx.has_b else None
        dz = torch.empty_like(z)
        # the splits are summed by the last workgroup of the launch (no ws_reduce_slabs launches: see ResRNNBlkFn.backward)
        da = _empty(z.device, R, N) if a is not None else None
        db = _empty(z.device, R, N) if ctx.has_b else None
        dev.affine_bwd(dout, z, a, ctx.a0, R * K * Tf, K * Tf, N, ns, dz, da_slab, db_slab, da=da, db=db,
                       counter=zero_words(z.device, R) if (da is not None or db is not None) else None)
        return dz, da, db, None


class ConcatFuseFn(torch.autograd.Function):
    """SpeakerFuseLayer 'concat' (speaker.py:90-102): Linear(cat[x, e]) = x Wx^T + (e We^T + b)."""

    @staticmethod
    def forward(ctx, z, e, W, b):
        _need_cuda(z, "SpeakerFuse(concat)")
        z, e, W = z.contiguous(), e.contiguous(), W.contiguous()
        R, K, Tf, N = z.shape
        E = e.shape[1]
        P = R * K * Tf
        c = _lin_fwd(e, W, b, w_off=N, ldw=N + E, K=E)                     # [R, N]
        out = torch.empty_like(z)
        dev.gemm_nt(A=z, a_rows=flat(N), M=P, N=N, K=N, W=W, ldw=N + E, C_out=out, c_rows=flat(N))
        dev.affine_fwd(out, None, c, 1.0, P, K * Tf, N, out)
        ctx.save_for_backward(z, e, W)
        return out

    @staticmethod
    def backward(ctx, dout):
        z, e, W = ctx.saved_tensors
        dout = dout.contiguous()
        R, K, Tf, N = z.shape
        E = e.shape[1]
        P = R * K * Tf
        d = z.device
        ns = _affine_splits(K * Tf)
        dc_slab = _empty(d, ns, R, N)
        dev.affine_bwd(dout, None, None, 1.0, P, K * Tf, N, ns, None, None, dc_slab)
        dc = _reduce_new(dc_slab, ns, R * N, (R, N))
        dW = _empty(d, N, N + E)
        # dWx = dout^T z  -> columns [0, N)
        nsplit, rps = dev.tn_splits(P)
        slab = _empty(d, nsplit, N * N)
        dev.gemm_tn(G=dout, g_rows=flat(N), A=z, a_rows=flat(N), M=P, Nn=N, Kk=N, slab=slab,
                    slab_stride=N * N, nsplit=nsplit, rows_per_split=rps)
        dev.reduce_slabs(slab, nsplit, N * N, N * N, dW, w=N, ldo=N + E)
        # dWe = dc^T e -> columns [N, N+E);  db = colsum(dc)
        dWe, db = _lin_bwd_w(dc, e)
        dev.reduce_slabs(dWe, 1, N * E, N * E, dW, w=E, ldo=N + E, out_off=N)
        dz = _empty(d, R, K, Tf, N)
        WxT = _empty(d, N, N)
        dev.transpose(W, N, N, N + E, WxT)
        dev.gemm_nt(A=dout, a_rows=flat(N), M=P, N=N, K=N, W=WxT, ldw=N, C_out=dz, c_rows=flat(N))
        de = _lin_bwd_x(dc, W, src_off=N, rows=N, cols=E, lds=N + E) if ctx.needs_input_grad[1] else None
        return dz, de, dW, db


# ---------------------------------------------------------------------------------------------
# per-band plans: device descriptor tables for the grouped (32-band) launches
# ---------------------------------------------------------------------------------------------
def mask_nn() -> bool:
    """The mask MLP's data-gradient GEMMs read the weights as they lie (ws_gemm_nt_args.vec bit 3, split-bf16 kernel) instead of
    transposed copies made every step; WESEP_GEMM_NN=0 restores the copies."""
    return dev.gemm_mode() == "bf16x3" and os.environ.get("WESEP_GEMM_NN", "1") != "0"


class BandPlan:
    """Band tables + cached group descriptors for BN[i] (bsrnn.py:252-258) and mask[i]
    (bsrnn.py:271-282).  Descriptors hold parameter pointers, so they are rebuilt only when a
    parameter's storage moves (e.g. .cuda(), load of a new module) or the batch geometry changes."""

    def __init__(self, band_width, feature_dim, device):
        self.dev = device
        self.bands = dev.BandTables(band_width, device)
        self.bw = [int(b) for b in band_width]
        self.f0 = [int(f) for f in self.bands.f0_host]
        self.K = len(self.bw)
        self.N = feature_dim
        N = feature_dim
        H1 = 4 * N
        # flat-gradient offsets
        self.bn_woff = np.concatenate([[0], np.cumsum([N * 2 * b for b in self.bw])]).astype(np.int64)
        self.m_w3off = np.concatenate([[0], np.cumsum([4 * b * H1 for b in self.bw])]).astype(np.int64)
        self.m_b3off = np.concatenate([[0], np.cumsum([4 * b for b in self.bw])]).astype(np.int64)
        # persistent transposed-weight workspaces (descriptors point into them)
        self.bn_wT = _empty(device, int(self.bn_woff[-1]))
        self.m_w1T = _empty(device, self.K * N * H1)
        self.m_w2T = _empty(device, self.K * H1 * H1)
        self.m_w3T = _empty(device, int(self.m_w3off[-1]))
        self._cache = {}

    def _up(self, arr):
        return L.upload_struct_array(arr, self.dev)

    def _key(self, params, R, Tf):
        return (R, Tf) + tuple(p.data_ptr() for p in params)

    # ---- BN ------------------------------------------------------------------------------
    def bn_desc(self, params, R, Tf):
        key = ("bn",) + self._key(params, R, Tf)
        if key not in self._cache:
            K, N = self.K, self.N
            nt = np.zeros(K, dtype=L.GROUP_NT_DTYPE)
            tn = np.zeros(K, dtype=L.GROUP_TN_DTYPE)
            dx = np.zeros(K, dtype=L.GROUP_NT_DTYPE)
            for g in range(K):
                gw, gb, cw, cb = params[4 * g:4 * g + 4]
                bw2 = 2 * self.bw[g]
                nt[g] = (cw.data_ptr(), cb.data_ptr(), gw.data_ptr(), gb.data_ptr(),
                         2 * self.f0[g], g * Tf * N, g, bw2, N, bw2, 0)
                tn[g] = (gw.data_ptr(), gb.data_ptr(), g * Tf * N, 2 * self.f0[g], g,
                         int(self.bn_woff[g]), g * N, N, bw2, 0, 0)
                dx[g] = (self.bn_wT.data_ptr() + 4 * int(self.bn_woff[g]), 0, 0, 0,
                         g * Tf * N, 2 * self.f0[g], 0, N, bw2, N, 0)
            self._cache = {k: v for k, v in self._cache.items() if k[0] != "bn"}
            self._cache[key] = (self._up(nt), self._up(tn), self._up(dx))
        return self._cache[key]

    # ---- mask ----------------------------------------------------------------------------
    def mask_desc(self, params, R, Tf):
        nn = mask_nn()
        key = ("mask", nn) + self._key(params, R, Tf)
        if key not in self._cache:
            K, N = self.K, self.N
            H1 = 4 * N
            M = R * Tf
            d = {n: np.zeros(K, dtype=L.GROUP_NT_DTYPE) for n in ("l1", "l2", "l3", "dh2", "dh1", "dxn")}
            t = {n: np.zeros(K, dtype=L.GROUP_TN_DTYPE) for n in ("w3", "w2", "w1")}
            gtab = np.zeros(K, dtype=np.uint64)
            for g in range(K):
                gw, gb, w1, b1, w2, b2, w3, b3 = params[8 * g:8 * g + 8]
                bw4 = 4 * self.bw[g]
                hoff = g * M * H1
                zoff = g * Tf * N
                gtab[g] = gw.data_ptr()
                d["l1"][g] = (w1.data_ptr(), b1.data_ptr(), gw.data_ptr(), gb.data_ptr(), zoff, hoff, g, N, H1, N, 0)
                d["l2"][g] = (w2.data_ptr(), b2.data_ptr(), 0, 0, hoff, hoff, 0, H1, H1, H1, 0)
                d["l3"][g] = (w3.data_ptr(), b3.data_ptr(), 0, 0, hoff, 4 * self.f0[g], 0, H1, bw4, H1, 0)
                if nn:    # the data-gradient GEMMs take the weights AS THEY LIE (ws_gemm_nt_args.vec bit 3: W'[n][k] = W[k * ldw + n])
                    d["dh2"][g] = (w3.data_ptr(), 0, 0, 0, 4 * self.f0[g], hoff, 0, bw4, H1, H1, 0)
                    d["dh1"][g] = (w2.data_ptr(), 0, 0, 0, hoff, hoff, 0, H1, H1, H1, 0)
                    d["dxn"][g] = (w1.data_ptr(), 0, 0, 0, hoff, zoff, 0, H1, N, N, 0)
                else:
                    d["dh2"][g] = (self.m_w3T.data_ptr() + 4 * int(self.m_w3off[g]), 0, 0, 0,
                                   4 * self.f0[g], hoff, 0, bw4, H1, bw4, 0)
                    d["dh1"][g] = (self.m_w2T.data_ptr() + 4 * g * H1 * H1, 0, 0, 0, hoff, hoff, 0, H1, H1, H1, 0)
                    d["dxn"][g] = (self.m_w1T.data_ptr() + 4 * g * N * H1, 0, 0, 0, hoff, zoff, 0, H1, N, H1, 0)
                t["w3"][g] = (0, 0, 4 * self.f0[g], hoff, 0, int(self.m_w3off[g]), int(self.m_b3off[g]), bw4, H1, 0, 0)
                t["w2"][g] = (0, 0, hoff, hoff, 0, g * H1 * H1, g * H1, H1, H1, 0, 0)
                t["w1"][g] = (gw.data_ptr(), gb.data_ptr(), hoff, zoff, g, g * H1 * N, g * H1, H1, N, 0, 0)
            self._cache = {k: v for k, v in self._cache.items() if k[0] != "mask"}
            out = {k: self._up(v) for k, v in d.items()}
            out.update({"t" + k: self._up(v) for k, v in t.items()})
            out["gamma_tab"] = torch.from_numpy(gtab.view(np.int64)).to(self.dev)
            self._cache[key] = out
        return self._cache[key]


# ---------------------------------------------------------------------------------------------
# STFT + band split + per-band GroupNorm + 1x1 conv     (bsrnn.py:309-336)
# ---------------------------------------------------------------------------------------------
def _band_split_fwd(wav, plan, params, lengths=None, frames=None):
    """The launches of BandSplitFn.forward; wav contiguous [R, T].  lengths / frames (ragged batches, inference: both or
    neither, dev.ragged_tables): the reflect padding turns at a row's own end, the frames behind it are zeros and the
    per-band statistics cover its valid frames.  Returns (z0, xbs, stats)."""
    R, T = wav.shape
    K, N = plan.K, plan.N
    Tf = 1 + T // HOP
    M = R * Tf
    d = wav.device
    xbs = _empty(d, M, 2 * NBIN)
    geo = Geom(R * K, K, Tf * 2 * NBIN, 0, 2 * NBIN, Tf, 128, K, plan.bands.bw2, plan.bands.off2)
    stats = _empty(d, R * K, 2)
    if lengths is None:
        dev.stft_bandsplit(wav, plan.bands, xbs)
        dev.group_stats(xbs, geo, stats)
    else:
        dev.stft_bandsplit(wav, plan.bands, xbs, lengths=lengths)
        dev.group_stats(xbs, geo, stats, glen=frames, glen_div=K)
    nt, _, _ = plan.bn_desc(params, R, Tf)
    z0 = _empty(d, R, K, Tf, N)
    dev.gemm_nt(A=xbs, a_rows=flat(2 * NBIN), M=M, C_out=z0, c_rows=Rows(Tf, K * Tf * N, N),
                stats=stats, stat_map=StatMap(Tf, K, 1, 0, 0), groups=nt, ngroups=K, max_n=N, vec=0)
    return z0, xbs, stats


def _mask_decode_fwd(z, xbs, plan, T, params, lengths=None, frames=None):
    """The launches of MaskDecodeFn.forward; z contiguous [R, K, Tf, N].  lengths / frames as in _band_split_fwd: the
    statistics of mask[i]'s norm cover a row's valid frames, the overlap-add and its envelope end at the row's own end and
    the samples behind it are zeros.  Returns (est, stats, h1, h2, m3)."""
    R, K, Tf, N = z.shape
    H1 = 4 * N
    M = R * Tf
    d = z.device
    D = plan.mask_desc(params, R, Tf)
    geo = Geom(R * K, 1, Tf * N, 0, N, Tf, N, K)
    stats = _empty(d, R * K, 2)
    if lengths is None:
        dev.group_stats(z, geo, stats)
    else:
        dev.group_stats(z, geo, stats, glen=frames, glen_div=K)
    h1, h2 = _empty(d, K, M, H1), _empty(d, K, M, H1)
    dev.gemm_nt(A=z, a_rows=Rows(Tf, K * Tf * N, N), M=M, C_out=h1, c_rows=flat(H1), stats=stats,
                stat_map=StatMap(Tf, K, 1, 0, 0), act=1, groups=D["l1"], ngroups=K, max_n=H1)
    dev.gemm_nt(A=h1, a_rows=flat(H1), M=M, C_out=h2, c_rows=flat(H1), act=1, groups=D["l2"],
                ngroups=K, max_n=H1)
    m3 = _empty(d, M, 4 * NBIN)
    dev.gemm_nt(A=h2, a_rows=flat(H1), M=M, C_out=m3, c_rows=flat(4 * NBIN), groups=D["l3"],
                ngroups=K, max_n=4 * max(plan.bw))
    fr = _empty(d, M, 512)
    dev.mask_istft_frames(xbs, m3, R, Tf, plan.bands, fr)
    est = _empty(d, R, T)
    if lengths is None:
        dev.istft_ola(fr, R, Tf, T, est)
    else:
        dev.istft_ola(fr, R, Tf, T, est, lengths=lengths)
    return est, stats, h1, h2, m3


def band_split_ragged(wav, plan, params, lengths, frames):
    """BandSplitFn for a ragged batch (inference): (z0, xbs)."""
    _need_cuda(wav, "BSRNN")
    return _band_split_fwd(wav.contiguous(), plan, [p.detach() for p in params], lengths, frames)[:2]


def mask_decode_ragged(z, xbs, plan, T, params, lengths, frames):
    """MaskDecodeFn for a ragged batch (inference): est [R, T], zeros behind every row's length."""
    _need_cuda(z, "BSRNN")
    return _mask_decode_fwd(z.contiguous(), xbs, plan, T, [p.detach() for p in params], lengths, frames)[0]


class BandSplitFn(torch.autograd.Function):
    """inputs: wav [R, T], plan, then per band (gn.weight, gn.bias, conv.weight, conv.bias).
    outputs: z0 [R, K, Tf, N], xbs [R*Tf, 2F] (band-split mixture spectrogram, no grad)."""

    @staticmethod
    def forward(ctx, wav, plan, *params):
        _need_cuda(wav, "BSRNN")
        wav = wav.contiguous()
        R, T = wav.shape
        Tf = 1 + T // HOP
        z0, xbs, stats = _band_split_fwd(wav, plan, params)
        ctx.save_for_backward(xbs, stats, *params)
        ctx.plan, ctx.dims = plan, (R, T, Tf)
        ctx.mark_non_differentiable(xbs)
        return z0, xbs

    @staticmethod
    def backward(ctx, dz0, _dxbs):
        xbs, stats = ctx.saved_tensors[:2]
        params = ctx.saved_tensors[2:]
        plan = ctx.plan
        R, T, Tf = ctx.dims
        K, N = plan.K, plan.N
        M = R * Tf
        d = xbs.device
        dz0 = dz0.contiguous()
        _, tn, dxd = plan.bn_desc(params, R, Tf)
        geo = Geom(R * K, K, Tf * 2 * NBIN, 0, 2 * NBIN, Tf, 128, K, plan.bands.bw2, plan.bands.off2)
        smap = StatMap(Tf, K, 1, 0, 0)
        # conv weight / bias gradients (A = re-normalised band spectrogram)
        nsplit, rps = dev.tn_splits(M)
        wtot = int(plan.bn_woff[-1])
        slab, bslab = _empty(d, nsplit, wtot), _empty(d, nsplit, K * N)
        dev.gemm_tn(G=dz0, g_rows=Rows(Tf, K * Tf * N, N), A=xbs, a_rows=flat(2 * NBIN), M=M, slab=slab,
                    slab_stride=wtot, bslab=bslab, bslab_stride=K * N, nsplit=nsplit, rows_per_split=rps,
                    stats=stats, stat_map=smap, groups=tn, ngroups=K, max_n=N, max_k=128, vec=0)
        dW = _reduce_new(slab, nsplit, wtot, (wtot,))
        dB = _reduce_new(bslab, nsplit, K * N, (K * N,))
        # d(normalised spectrogram) -> GroupNorm affine gradients (dX itself is never needed)
        for g in range(K):
            bw2 = 2 * plan.bw[g]
            dev.transpose(params[4 * g + 2].reshape(N, bw2), N, bw2, bw2, plan.bn_wT,
                          dst_off=int(plan.bn_woff[g]))
        dxn = _empty(d, M, 2 * NBIN)
        dev.gemm_nt(A=dz0, a_rows=Rows(Tf, K * Tf * N, N), M=M, C_out=dxn, c_rows=flat(2 * NBIN),
                    groups=dxd, ngroups=K, max_n=128, vec=3)
        ns2 = min(64, R)
        pslab = _empty(d, ns2, K, 2, 128)
        dev.gn_param_grad(xbs, dxn, stats, geo, ns2, pslab)
        dgb = _reduce_new(pslab, ns2, K * 2 * 128, (K, 2, 128))
        grads = []
        for g in range(K):
            bw2 = 2 * plan.bw[g]
            o = int(plan.bn_woff[g])
            grads += [dgb[g, 0, :bw2], dgb[g, 1, :bw2], dW[o:o + N * bw2].view(N, bw2, 1), dB[g * N:(g + 1) * N]]
        return (None, None) + tuple(grads)


# ---------------------------------------------------------------------------------------------
# mask MLP + GLU complex mask + iSTFT     (bsrnn.py:366-389)
# ---------------------------------------------------------------------------------------------
class MaskDecodeFn(torch.autograd.Function):
    """inputs: z [R,K,Tf,N], xbs, plan, T, then per band (gn.w, gn.b, w1, b1, w2, b2, w3, b3).
    output: est [R, T]."""

    @staticmethod
    def forward(ctx, z, xbs, plan, T, *params):
        _need_cuda(z, "BSRNN")
        z = z.contiguous()
        est, stats, h1, h2, m3 = _mask_decode_fwd(z, xbs, plan, T, params)
        ctx.save_for_backward(z, xbs, stats, h1, h2, m3, *params)
        ctx.plan, ctx.T = plan, T
        return est

    @staticmethod
    def backward(ctx, dest):
        z, xbs, stats, h1, h2, m3 = ctx.saved_tensors[:6]
        params = ctx.saved_tensors[6:]
        plan, T = ctx.plan, ctx.T
        R, K, Tf, N = z.shape
        H1 = 4 * N
        M = R * Tf
        d = z.device
        D = plan.mask_desc(params, R, Tf)
        dest = dest.contiguous()
        dm3 = _empty(d, M, 4 * NBIN)
        dev.mask_istft_bwd(dest, xbs, m3, R, Tf, T, plan.bands, dm3)
        nsplit, rps = dev.tn_splits(M)
        maxb4 = 4 * max(plan.bw)
        # layer 3
        w3tot, b3tot = int(plan.m_w3off[-1]), int(plan.m_b3off[-1])
        slab, bslab = _empty(d, nsplit, w3tot), _empty(d, nsplit, b3tot)
        dev.gemm_tn(G=dm3, g_rows=flat(4 * NBIN), A=h2, a_rows=flat(H1), M=M, slab=slab, slab_stride=w3tot,
                    bslab=bslab, bslab_stride=b3tot, nsplit=nsplit, rows_per_split=rps, groups=D["tw3"],
                    ngroups=K, max_n=maxb4, max_k=H1)
        dW3 = _reduce_new(slab, nsplit, w3tot, (w3tot,))
        dB3 = _reduce_new(bslab, nsplit, b3tot, (b3tot,))
        nn = mask_nn()
        vnn = 3 | (8 if nn else 0)
        if not nn:      # (rounds 1-5: 3 K transposes of the weights per step -- 93 launches of 6 us, each with its launch gap, at the
            for g in range(K):                     # head of the backward; the GEMMs stage W as it lies now, round 6)
                bw4 = 4 * plan.bw[g]
                dev.transpose(params[8 * g + 6].reshape(bw4, H1), bw4, H1, H1, plan.m_w3T,
                              dst_off=int(plan.m_w3off[g]))
                dev.transpose(params[8 * g + 4].reshape(H1, H1), H1, H1, H1, plan.m_w2T, dst_off=g * H1 * H1)
                dev.transpose(params[8 * g + 2].reshape(H1, N), H1, N, N, plan.m_w1T, dst_off=g * N * H1)
        dh2 = _empty(d, K, M, H1)
        dev.gemm_nt(A=dm3, a_rows=flat(4 * NBIN), M=M, C_out=dh2, c_rows=flat(H1), T=h2, groups=D["dh2"],
                    ngroups=K, max_n=H1, vec=vnn)
        # layer 2
        slab, bslab = _empty(d, nsplit, K * H1 * H1), _empty(d, nsplit, K * H1)
        dev.gemm_tn(G=dh2, g_rows=flat(H1), A=h1, a_rows=flat(H1), M=M, slab=slab, slab_stride=K * H1 * H1,
                    bslab=bslab, bslab_stride=K * H1, nsplit=nsplit, rows_per_split=rps, groups=D["tw2"],
                    ngroups=K, max_n=H1, max_k=H1)
        dW2 = _reduce_new(slab, nsplit, K * H1 * H1, (K, H1, H1, 1))
        dB2 = _reduce_new(bslab, nsplit, K * H1, (K, H1))
        dh1 = _empty(d, K, M, H1)
        dev.gemm_nt(A=dh2, a_rows=flat(H1), M=M, C_out=dh1, c_rows=flat(H1), T=h1, groups=D["dh1"],
                    ngroups=K, max_n=H1, vec=vnn)
        del dh2
        # layer 1 (A = re-normalised z band rows)
        slab, bslab = _empty(d, nsplit, K * H1 * N), _empty(d, nsplit, K * H1)
        dev.gemm_tn(G=dh1, g_rows=flat(H1), A=z, a_rows=Rows(Tf, K * Tf * N, N), M=M, slab=slab,
                    slab_stride=K * H1 * N, bslab=bslab, bslab_stride=K * H1, nsplit=nsplit,
                    rows_per_split=rps, stats=stats, stat_map=StatMap(Tf, K, 1, 0, 0), groups=D["tw1"],
                    ngroups=K, max_n=H1, max_k=N)
        dW1 = _reduce_new(slab, nsplit, K * H1 * N, (K, H1, N, 1))
        dB1 = _reduce_new(bslab, nsplit, K * H1, (K, H1))
        del slab, bslab
        dxn = _empty(d, R, K, Tf, N)
        dev.gemm_nt(A=dh1, a_rows=flat(H1), M=M, C_out=dxn, c_rows=Rows(Tf, K * Tf * N, N), groups=D["dxn"],
                    ngroups=K, max_n=N, vec=vnn)
        del dh1
        # GroupNorm backward with per-band gamma
        geo = Geom(R * K, 1, Tf * N, 0, N, Tf, N, K)
        ab = _empty(d, R * K, 2)
        dev.gn_bwd_reduce(z, dxn, stats, geo, ab, gamma_tab=D["gamma_tab"])
        ns2 = min(64, R)
        pslab = _empty(d, ns2, K, 2, N)
        dev.gn_param_grad(z, dxn, stats, geo, ns2, pslab)
        dgb = _reduce_new(pslab, ns2, K * 2 * N, (K, 2, N))
        dz = torch.empty_like(z)
        dev.gn_bwd_apply(z, dxn, stats, ab, geo, dz, gamma_tab=D["gamma_tab"])
        grads = []
        for g in range(K):
            bw4 = 4 * plan.bw[g]
            o3, ob3 = int(plan.m_w3off[g]), int(plan.m_b3off[g])
            grads += [dgb[g, 0], dgb[g, 1], dW1[g], dB1[g], dW2[g], dB2[g],
                      dW3[o3:o3 + bw4 * H1].view(bw4, H1, 1), dB3[ob3:ob3 + bw4]]
        return (dz, None, None, None) + tuple(grads)


# ---------------------------------------------------------------------------------------------
# SI-SDR loss (auraloss.time.SISDRLoss, losses.py:24-25)
# ---------------------------------------------------------------------------------------------
class SISDRFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, est, tgt, eps):
        _need_cuda(est, "SISDRLoss")
        est, tgt = est.contiguous().float(), tgt.contiguous().float()
        R = est.shape[0]
        rowstat = _empty(est.device, R, 8)
        loss = _empty(est.device, 1)
        dev.sisdr_fwd(est, tgt, rowstat, loss, eps)
        ctx.save_for_backward(est, tgt, rowstat)
        return loss.view(())

    @staticmethod
    def backward(ctx, gout):
        est, tgt, rowstat = ctx.saved_tensors
        dest = torch.empty_like(est)
        dev.sisdr_bwd(est, tgt, rowstat, gout.contiguous().view(1).float(), dest)
        return dest, None, None
