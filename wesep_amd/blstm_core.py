"""Blocked BLSTM + projection, forward and backward: the training hot path that pBSRNN's ResRNN (functional.ResRNNBlkFn) and
TF-GridNet's intra / inter BLSTMs (functional_tfgridnet.BlstmLinearBlkFn) share.  One plan decided in the forward (BlstmPlan),
one provider of the derived weight forms (PackCache + WeightPacks), one weight-gradient routine with its side-stream
hand-over (WGradBox / WGradCarrierFn), and the launches as four steps over the plan -- blstm_forward, blstm_bptt,
blstm_weight_grads, blstm_dxn -- called in the order they are issued, so that each caller keeps what is its own between them
(GroupNorm and the tail flush there, padding and the strided sequence map here).  Imports nothing from the functional_*
modules; functional.py re-exports the names that lived there.

Layout: every activation of the recurrence lives in the blocked layout BL (include/wesep_hip.h): gates / c / h / d(h) never
exist in row-major form."""
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from . import _lib as L
from . import dev

H = L.LSTM_H          # LSTM hidden size the recurrent kernels are built for
G4 = 4 * H
N = 128               # input / output features the blocked kernels are built for


def _empty(dev_, *shape):
    return torch.empty(*shape, device=dev_, dtype=torch.float32)


def _reduce_new(slab, nsplit, stride, shape):
    out = _empty(slab.device, *shape)
    dev.reduce_slabs(slab, nsplit, stride, int(np.prod(shape)), out)
    return out


# ---------------------------------------------------------------------------------------------
# numerics probes (off by default)
# ---------------------------------------------------------------------------------------------
def _h2_probe() -> int:
    """NUMERICS PROBE (tools/r04_h2_numerics.py; off by default): emulate narrower storage of the saved recurrence state
    by rounding the fp32 buffers in place between kernels.  Bits: 1 = activated gates to fp16, 2 = d(gates) to bf16
    (the hi term of the split pair only), 4 = cell state to fp16, 8 = activated gates to unorm16, 16 = d(hcat) to bf16,
    64 / 128 = the A operand [xn | h] of the weight-gradient GEMMs to fp16 / bf16, 256 / 512 = the pre-activations of the
    unfused (time-view) forward to fp16 / bf16, 1024 = the proj weight gradient on fp16 operands (CPU emulation)."""
    return int(os.environ.get("WESEP_H2_PROBE", "0"))


_PROBE_SAT = [0, 0.0]     # (probe bit 32) saturated d(gates) elements, largest |scaled d(gates)| / 65504 seen


def _probe_round(t, kind, packed=False):
    """In-place rounding of an fp32 buffer.  packed: the buffer holds BLS pairs on the device (hi << 16 | lo): keeping the
    hi term only IS bf16(x); on the CPU emulation it holds plain fp32."""
    if kind == "f16":
        t.copy_(t.half().float())
    elif kind == "u16":      # BL(2048) activated gates: quad q = column >> 2, gate = (q >> 6) & 3; i, f, o in (0, 1), g in (-1, 1)
        v = t.view(-1, 2, 4, 64 * 128)
        v[:, :, 2].mul_(0.5).add_(0.5)
        v.copy_(torch.floor(v * 65535.0 + 0.5) / 65535.0)
        v[:, :, 2].mul_(2.0).sub_(1.0)
    elif packed and torch.cuda.is_available():
        t.view(torch.int32).bitwise_and_(-65536)
    else:
        t.copy_(t.bfloat16().float())


# ---------------------------------------------------------------------------------------------
# selectors: the environment's say in the plan, with the measurements behind each default
# ---------------------------------------------------------------------------------------------
def tnb_a16() -> bool:
    """fp16 copies of [xn | h] for the weight-gradient GEMMs (ws_gemm_tnb a_fmt = 1, ABI v16; with the default WS_GATES_H2F
    only).  WESEP_TNB_A16=0 keeps the split-pair A operand of round 3."""
    return os.environ.get("WESEP_TNB_A16", "1") != "0"


def pair_rfmt(gfmt) -> int:
    """Arithmetic of the pair BPTT's recurrent product (ws_lstm_pair_args.rfmt): 3 (default with WS_GATES_H2F, ABI v20) = the
    stored scaled-fp16 d(gates) x W_hh as fp16 hi + block-scaled FP8 lo, all of W_hh resident on the compute unit, the lo term on
    the block-scaled FP8 matrix instruction (K = 64 at twice the fp16 rate; 0.4 ms per step: profiles/r06_ab/r06_c23_*);
    WESEP_PAIR_RF=2: the same weights, both terms on the fp16 MFMA (ABI v18, the default of round 5); 1: fp16 hi / lo, the lo
    plane streamed (ABI v17); 0: the three-term split-bf16 product of rounds 3-4."""
    rf = int(os.environ.get("WESEP_PAIR_RF", "3"))
    if rf not in (0, 1, 2, 3):
        raise ValueError(f"WESEP_PAIR_RF={rf}: 0, 1, 2 or 3")
    return rf if gfmt == L.GATES_H2F else 0


def dxn_fmt(g_fmt) -> int:
    """a_fmt of the d(xn) GEMM over the 2-byte d(gates) (ws_gemm_b2p): with scaled-fp16 d(gates) (g_fmt 2) 3 = the lo term of the
    product on the block-scaled FP8 matrix instruction (ABI v20, the default: 0.57 -> 0.53 ms per launch alone, 1 ms per step --
    profiles/r06_c30_band_probe.txt, r06_ab/r06_c30_*); WESEP_DXN_F8=0: the format itself (2: both terms on the fp16 MFMA)."""
    return 3 if g_fmt == 2 and os.environ.get("WESEP_DXN_F8", "1") != "0" else g_fmt


def band_rfmt(gfmt, lmode) -> int:
    """Arithmetic of the streaming BPTT's recurrent product (ws_lstm_args.rfmt): 2 (ABI v18, with WS_GATES_H2F on the 32-sequence
    blocked kernels) = the stored scaled-fp16 d(gates) x W_hh as fp16 hi + scaled-FP8 lo, two MFMAs per product and three
    quarters of the weight stream -- the pair BPTT's arithmetic (pair_rfmt); config 2's parity and the 60-step trajectory with
    it: profiles/r06_c1_parity_brf2.log, r05_c23_band_rf2_trajectory.log.  3 (ABI v20, the default): the same pack with the lo
    term on the block-scaled FP8 matrix instruction (2.07 -> 1.88 ms per launch alone, 0.6 ms per step:
    profiles/r06_c26_band_probe.txt, r06_ab/r06_c26_*).  WESEP_BAND_RF=0: the three-term split-bf16 product of rounds 1-5."""
    rf = int(os.environ.get("WESEP_BAND_RF", "3"))
    if rf not in (0, 2, 3):
        raise ValueError(f"WESEP_BAND_RF={rf}: 0, 2 or 3")
    if rf == 3 and os.environ.get("WESEP_BAND_DX", "0") == "1":
        rf = 2                                          # (d(xn) inside the BPTT rides on the fp16 lo term's fragments)
    return rf if gfmt == L.GATES_H2F and lmode == L.LSTM_BF16X3_BLK else 0


def band_dx(brf, seq, geo) -> bool:
    """d(xn) = d(gates) W_ih computed INSIDE the streaming BPTT (ws_lstm_args.dxn, ABI v19; OPT-IN: WESEP_BAND_DX=1, with
    band_rfmt 2): the kernel holds d(gates) in LDS when it produces them, so ws_gemm_b2p's second pass over that 2.1 GB buffer
    (per band-view layer at R = 32) and its launch disappear; the fused GroupNorm backward adds the two directions' shares.
    Measured (profiles/r06_c4_band_probe.txt, r06_ab/r06_c4_bench_{new,nodx}.json): correct to 4.9e-6 and 12.6 GB of HBM reads
    per step less, but NOT faster -- the BPTT is bound by its per-step weight stream from L2 (19 us per MB per workgroup:
    1.98 ms at 0.75 MB, 2.60 ms with W_ih^T's 0.4 MB beside it) and the 0.62 ms it gains equal the 0.70 ms the GEMM takes:
    step 101.8 vs 101.2 ms.  Kept for the traffic figure and for hosts where HBM is the scarcer resource; not the default."""
    return (brf == 2 and os.environ.get("WESEP_BAND_DX", "0") == "1" and not seq.nvalid and dev.gn_bwd_fused_ok(geo))


# ---------------------------------------------------------------------------------------------
# weight gradients on the side stream: deferred jobs, their boxes and the carrier node that delivers them
# ---------------------------------------------------------------------------------------------
_SIDE_STREAMS = {}


def _side_stream(device):
    key = (device.type, device.index)
    if key not in _SIDE_STREAMS:
        # WESEP_SIDE_PRIORITY: HIP stream priority of the weight-gradient side stream (torch convention: lower = more
        # urgent; unset = the default priority)
        pr = os.environ.get("WESEP_SIDE_PRIORITY")
        _SIDE_STREAMS[key] = torch.cuda.Stream(device=device, priority=int(pr)) if pr else torch.cuda.Stream(device=device)
    return _SIDE_STREAMS[key]


_PENDING = {}   # device key -> deferred weight-gradient jobs (closures), oldest first


def _pending(device):
    return _PENDING.setdefault((device.type, device.index), [])


_AMAX = {}   # (device, stream) -> [int32 words, cursor]: scale words of WS_GATES_H2F, handed out one per BPTT launch


def zero_words(device, n=1):
    """`n` consecutive zeroed int32 device words: ws_gemm_p2b's running max |d(hcat)| (the scale source of WS_GATES_H2F,
    wesep_hip.h) and the counters of the "the workgroups add their partials up themselves" epilogues (ws_last_block /
    ws_tree_sum256, which leave them at zero).  Words come from a block that is zero-filled ONCE per 8192 words instead of
    once per use: a small fill is a launch of its own, and every tiny main-stream launch can sit out a whole
    weight-gradient GEMM of the side stream before it gets a CU (profiles/r04_summary.md).  A block is never re-zeroed
    while words of it may still be read (the side stream's deferred jobs): a fresh block is allocated instead and the old
    one dies with its last reference."""
    key = (device.type, device.index, L.stream_ptr().value if device.type == "cuda" and torch.cuda.is_available() else 0)
    ent = _AMAX.get(key)
    if ent is None or ent[1] + n > ent[0].numel():
        ent = _AMAX[key] = [torch.zeros(max(8192, n), device=device, dtype=torch.int32), 0]
    ent[1] += n
    return ent[0][ent[1] - n:ent[1]]


def amax_word(device):
    return zero_words(device, 1)


def mark_wgrads_ready(device):
    """Event on the current stream after which every deferred job's operands are complete (None when
    nothing is pending)."""
    if not _pending(device):
        return None
    ready = torch.cuda.Event()
    ready.record(torch.cuda.current_stream())
    return ready


def flush_deferred_wgrads(device, ready=None):
    """Launch every deferred weight-gradient job on the side stream, ordered after `ready` (default:
    everything enqueued so far on the current stream).  A TIME-VIEW recurrence keeps 128 of 256 CUs
    busy for ~5 ms: its backward marks `ready`, launches the recurrence FIRST -- so its workgroups
    take their CUs at once instead of queueing behind a full-chip GEMM wave -- and then releases the
    jobs into the other half of the chip.  The carriers flush the leftovers."""
    jobs = _pending(device)
    if not jobs:
        return
    side = _side_stream(device)
    if ready is None:
        ready = mark_wgrads_ready(device)
    with torch.cuda.stream(side):
        # `ready` is a GATE, not only a dependency: it holds the jobs back until the kernels in front of the recurrence that
        # was just launched have finished, so that the recurrence's workgroups and the jobs become runnable together and the
        # recurrence (launched first) takes its CUs first.  Without it the jobs -- whose own operands were complete long ago
        # -- fill the chip at once and the recurrence waits for a whole gemm_tnb wave: measured, step 127 -> 135.6 ms (pBSRNN),
        # 305 -> 326 ms (TF-GridNet), profiles/r04_ab_runs.md
        side.wait_event(ready)
        for job, done in jobs:
            side.wait_event(done)        # the job's own producer stream (defer_wgrad); precedes `ready` on one stream
            job(side)
    jobs.clear()


def defer_wgrad(device, job):
    """Queue a weight-gradient job (a closure that takes the side stream).  The job carries an event of its PRODUCER stream,
    recorded now: its operands are complete once everything enqueued so far on the current stream is.  With several producer
    streams (the row streams of models.tfgridnet) a flush issued from one stream must not release another stream's job before
    that stream has produced its operands."""
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream())
    _pending(device).append((job, done))


class WGradBox:
    """Hand-over slot between a ResRNN's backward (producer, side stream) and its carrier node."""
    __slots__ = ("event", "grads", "keep")

    def __init__(self):
        self.event, self.grads, self.keep = None, None, None

    def __del__(self):
        # A carrier that never ran (torch.autograd.grad over a subset of the inputs, an exception inside backward) leaves the
        # operands of an already launched job in `keep`: no stream has waited for the job, so they go back to the allocator
        # the way rounds 3-5 returned every operand -- marked as in use by the side stream
        keep = self.keep
        if keep is not None:
            try:
                for t in keep[0]:
                    t.record_stream(keep[1])
            except Exception:       # interpreter shutdown
                pass


def wgrad_hold() -> bool:
    """How the operands of a deferred weight-gradient job (d(gates), xn, hcat, d(out): 4 GB per ResRNN, 49 GB per step) stay
    valid while the side stream reads them.  Rounds 3-5 marked them `record_stream(side)`: the caching allocator then takes a
    block back only once the GPU has PASSED the side stream's job, so every allocation the host makes ahead of the GPU misses
    the cache -- 49 GB of hipMalloc per step of run-ahead, calls of 1.6-3.7 s each now and then, and a block pattern that
    depends on timing (profiles/r06_c52_diag.txt).  Default now: the job's box keeps the operands until the carrier node has
    made the consumer stream wait for the job's event and drops them there -- an ordinary stream-ordered free on the stream
    that allocated them, no event bookkeeping, the same blocks every step.  WESEP_WGRAD_HOLD=0 restores record_stream."""
    return os.environ.get("WESEP_WGRAD_HOLD", "1") != "0"


def keep_for_side(box, tensors, side, prod):
    """Called by a deferred job once its launches are on `side`: keeps `tensors` -- allocated on the stream `prod`, the one
    the ResRNN's forward and backward ran on -- valid for them (wgrad_hold)."""
    tensors = tuple(t for t in tensors if t is not None)
    if wgrad_hold():
        box.keep = (tensors, side, prod)
    else:
        for t in tensors:
            t.record_stream(side)


class WGradCarrierFn(torch.autograd.Function):
    """Delivers the LSTM / proj weight gradients of one ResRNN to autograd.

    The time-view recurrences occupy 64 of the 256 CUs for ~7 ms each; the weight-gradient GEMMs are
    a side branch of the backward graph (nothing downstream reads them), so ResRNNBlkFn.backward
    launches them on a side HIP stream where they fill the idle CUs under the NEXT layers'
    recurrences.  Autograd, however, wants a node's gradients when its backward returns.  This node
    is the way out: it is created BEFORE every ResRNN of the step (lowest sequence numbers, so the
    engine runs it after all of them), takes the weights as inputs and hands their gradients over
    once the current stream has waited for the side stream's event."""

    @staticmethod
    def forward(ctx, box, *params):
        ctx.box = box
        return params[0].new_zeros(())

    @staticmethod
    def backward(ctx, _g):
        box = ctx.box
        if box.grads is None:
            flush_deferred_wgrads(_g.device)   # leftovers of the last layers
        if box.grads is None:
            raise L.WesepHipError("weight-gradient carrier ran before its ResRNN backward")
        cur = torch.cuda.current_stream()
        cur.wait_event(box.event)
        keep, box.keep = box.keep, None
        if keep is not None:
            # `cur` is ordered behind the job now: operands allocated on `cur` are simply dropped (stream-ordered reuse is
            # safe); an operand of another stream's pool (TF-GridNet's row streams) is not ordered by this wait
            if keep[2] != cur:
                for t in keep[0]:
                    t.record_stream(keep[1])
            del keep
        grads, box.grads = box.grads, None
        for g in grads:
            g.record_stream(cur)
        return (None,) + tuple(grads)


# ---------------------------------------------------------------------------------------------
# derived weight forms: the cache and the one provider
# ---------------------------------------------------------------------------------------------
class PackCache:
    """Derived forms of one ResRNN's LSTM / proj weights -- concatenated W_ih, MFMA-fragment packs of W_hh (per
    recurrence kernel family), W_ih, W_proj and their transposes -- built once per weight VALUE instead of once per
    forward and once more per backward (round 1: 294 pack_w launches / 3.6 ms per step).  Owned by the module that
    owns the parameters (models.bsrnn.ResRNN), so entries die with it.  Signature of the source weights: storage
    addresses + torch version counters + dev.weight_epoch() (FusedClipAdam writes parameters through raw pointers
    and bumps the epoch instead)."""

    def __init__(self):
        self.sig = None
        self.items = {}
        # round 6, prefetch_packs: the kinds asked for under the current / the previous signature (a training step asks for
        # the same ones every step), the recurrence mode they were built for, and the side stream's event behind a prefetch
        self.kinds, self.kinds_prev, self.lmode, self.pair_rf, self.ready, self.waited = [], [], None, 0, None, set()

    @staticmethod
    def signature(params):
        return (dev.weight_epoch(),) + tuple((p.data_ptr(), p._version) for p in params)

    def begin(self, params):
        """Signature of `params` now; drops the cached packs when it moved."""
        sig = self.signature(params)
        if sig != self.sig:
            if self.kinds:
                self.kinds_prev = self.kinds
            self.sig, self.items, self.kinds, self.ready, self.waited = sig, {}, [], None, set()
        return sig

    def note(self, kind):
        if kind not in self.kinds:
            self.kinds.append(kind)

    def get(self, sig, kind, build):
        """The pack `kind` for the weights of signature `sig`; built uncached when the cache has moved on (a
        backward through a graph whose forward predates a weight update)."""
        if sig != self.sig:
            return build()
        if self.ready is not None:       # built ahead on the side stream (prefetch_packs): every consumer stream waits once
            cur = torch.cuda.current_stream()
            if cur.cuda_stream not in self.waited:
                cur.wait_event(self.ready)
                self.waited.add(cur.cuda_stream)
        if kind not in self.items:
            self.items[kind] = build()
        return self.items[kind]


class _NoCache(PackCache):
    def begin(self, params):
        return None

    def note(self, kind):
        pass

    def get(self, sig, kind, build):
        return build()


_NO_CACHE = _NoCache()


# ---------------------------------------------------------------------------------------------
# BPTT kind and the per-launch debug words
# ---------------------------------------------------------------------------------------------
def _bptt_kind(seq, device, cluster) -> str:
    """Which BPTT kernel a blocked-layout ResRNN runs: 'cluster' (opt-in), 'pair' (views with few long sequences: the
    time view), 'stream' (lstm_bf16*.hip)."""
    if cluster and os.environ.get("WESEP_LSTM_CLUSTER_BWD", "0") == "1":
        return "cluster"
    return "pair" if dev.lstm_pair_ok(seq, device) else "stream"


def _pair_dbg() -> int:
    """WESEP_PAIR_FORCE_TIMEOUT=1 (tests): every pair BPTT launch times out in pair 0 at step 2, so the predicated
    streaming fall-back produces the layer's d(gates).  WESEP_PAIR_STAMP=1 (measurement, tools/r06_instep_stamps.py): the
    cycle-stamped build of the kernel (dbg 2048) inside a whole training step."""
    return (8 if os.environ.get("WESEP_PAIR_FORCE_TIMEOUT", "0") == "1" else 0) | (2048 if _pair_stamp_on() else 0)


PAIR_STAMPS = []     # (stamp buffer, steps) of every pair BPTT launched with WESEP_PAIR_STAMP=1, oldest first


def _pair_stamp_on() -> bool:
    return os.environ.get("WESEP_PAIR_STAMP", "0") == "1"


def _pair_stamp_buf(device, steps):
    if not _pair_stamp_on():
        return None
    buf = torch.zeros(steps * 2 * 8 * 2 + 256 * 4 * 2, device=device)   # step stamps of pair 0 + every workgroup's wall-clock row
    PAIR_STAMPS.append((buf, steps))
    return buf


def _cluster_dbg() -> int:
    """WESEP_CLUSTER_FORCE_TIMEOUT=1 (tests): every forward cluster launch times out in workgroup 0 at step 2, so the
    predicated streaming fall-back produces the layer's result."""
    return 8 if os.environ.get("WESEP_CLUSTER_FORCE_TIMEOUT", "0") == "1" else 0


class WeightPacks:
    """W(kind): the derived weight forms of one BLSTM + projection through a PackCache (built on first use, kept until the
    weights change).  kinds: cat (wcat, bcat) | whh (contiguous W_hh pair) | hh (fwd, bwd recurrence packs of mode
    `lmode`) | hh8 / wx8 (streaming BPTT's FP8 packs) | hhp / hhp16 (pair-BPTT pack; hhp16 in the plan's `pair_rf` format) |
    fused* ([W_ih | W_hh] stream of lstm_fused.hip) | wih / wihT* (p2b x-projection, b2p d(xn)) | pw (contiguous proj.weight) |
    proj / proj16 / projT (b2p projection, the same as fp16 hi / lo for h in fp16 planes, p2b d(hcat)).  An object, not a pair
    of closures that name each other: a caller whose cache lives for one forward / backward pair (TF-GridNet) gets its packs
    back when ctx dies, not when the cycle collector runs."""

    def __init__(self, cache, sig, lmode, pair_rf, wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r, bhh_r, proj_w):
        self.cache, self.sig, self.lmode, self.pair_rf = cache, sig, lmode, pair_rf
        self.weights = (wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r, bhh_r, proj_w)
        cache.lmode, cache.pair_rf = lmode, pair_rf

    def __call__(self, kind):
        # (the plan's arithmetic is part of the key: toggling WESEP_PAIR_RF in one process -- A/B benches, tests -- must not
        #  hand an fp16-lo pack to the FP8 kernel; one cache can hold both)
        key = (kind, self.lmode) if kind == "hh" else (kind, self.pair_rf) if kind == "hhp16" else kind
        self.cache.note(kind)
        return self.cache.get(self.sig, key, lambda: self._build(kind))

    def _build(self, kind):
        W, lmode, pair_rf = self, self.lmode, self.pair_rf
        wih_f, whh_f, bih_f, bhh_f, wih_r, whh_r, bih_r, bhh_r, proj_w = self.weights
        d = wih_f.device
        N = wih_f.shape[1]
        if kind == "cat":
            wcat, bcat = _empty(d, 2 * G4, N), _empty(d, 2 * G4)
            dev.lstm_cat_ih(wih_f.contiguous(), wih_r.contiguous(), bih_f, bhh_f, bih_r, bhh_r, N, wcat, bcat)
            return wcat, bcat
        if kind == "whh":
            return whh_f.contiguous(), whh_r.contiguous()
        if kind == "hh":
            pack_f, pack_b = _empty(d, L.LSTM_PACK_FLOATS), _empty(d, L.LSTM_PACK_FLOATS)
            dev.lstm_pack(*W("whh"), pack_f, pack_b, lmode)
            return pack_f, pack_b
        if kind == "hh8":                 # BPTT pack of the streaming kernel's rfmt 2 (fp16 hi + scaled-FP8 lo of 256 w)
            pack = _empty(d, L.LSTM_PACK_FLOATS)
            dev.lstm_pack_bwd_f8(*W("whh"), pack)
            return pack
        if kind == "wx8":                 # W_ih^T stream of the BPTT's own d(xn) (ws_lstm_args.dxn): fp16 hi + scaled-FP8 lo
            pack = _empty(d, L.LSTM_DX_PACK_FLOATS)
            dev.lstm_pack_dx_f8(W("cat")[0], pack)
            return pack
        if kind in ("hhp", "hhp16"):      # hhp16: fp16 hi + fp16 / FP8 lo of 256 w (the rfmt = 1 / 2 pair BPTT)
            pack = _empty(d, L.LSTM_PACK_FLOATS)
            dev.lstm_pack_pair(*W("whh"), pack, f16=pair_rf if kind == "hhp16" else 0)
            return pack
        if kind in ("fused", "fused16", "fused8"):  # fused16: the hfmt 1 pack (256 w; W_hh part as fp16 hi / lo); fused8: hfmt 5
            fpack = _empty(d, L.LSTM_FUSED_PACK_FLOATS)        # (fp16 hi + one FP8 fragment per k-step, ABI v20)
            dev.lstm_pack_fused(wih_f.contiguous(), wih_r.contiguous(), *W("whh"), fpack,
                                hfmt={"fused": 0, "fused16": 1, "fused8": 5}[kind])
            return fpack
        if kind == "wih":
            out = _empty(d, 2 * G4 * N)
            dev.pack_w(W("cat")[0], 2 * G4, N, N, out, order=0)
            return out
        if kind in ("wihT", "wihT16", "wihT8"):   # wihT16: fp16 hi / lo (ws_pack_w_f16): d(xn) from scaled-fp16 d(gates), WS_GATES_H2F
            out = _empty(d, N * 2 * G4)              # wihT8: fp16 hi + FP8 lo fragments (ws_pack_w_f16f8, a_fmt 3)
            dev.pack_w(W("cat")[0], N, 2 * G4, N, out, trans=True, order=1, f16={"wihT": 0, "wihT16": 1, "wihT8": 2}[kind])
            return out
        if kind == "pw":
            return proj_w.contiguous()
        if kind in ("proj", "proj16"):      # proj16: fp16 hi / lo of 256 w (ws_pack_w_f16): the projection over h as fp16 planes
            out = _empty(d, N * 2 * H)
            dev.pack_w(W("pw"), N, 2 * H, 2 * H, out, order=1, f16=kind == "proj16")
            return out
        if kind == "projT":
            out = _empty(d, 2 * H * N)
            dev.pack_w(W("pw"), 2 * H, N, 2 * H, out, trans=True, order=0)
            return out
        raise KeyError(kind)


# ---------------------------------------------------------------------------------------------
# the plan: every choice of one blocked BLSTM, made once
# ---------------------------------------------------------------------------------------------
class BlstmPlan(NamedTuple):
    """Decided in the forward (make_plan) from the sequence map, the device, needs_input_grad and the environment, and kept on
    ctx.  The backward reads this record and nothing from os.environ except the debug words that are per-launch by design
    (_pair_dbg, _cluster_dbg, WESEP_PROBE_SKIP_WGRAD): a variable changed between a forward and its backward neither gets a
    pack built late -- on the stream where the forward's pre-build exists to avoid it -- nor names a format the forward's
    packs do not have."""
    nb: int             # blocks of 32 positions of the sequence map (dev.bl_num_blocks)
    lmode: int          # mode of the streaming recurrence kernels (dev.lstm_blk_mode)
    cluster: bool       # the weight-stationary cluster kernels apply (dev.lstm_cluster_ok)
    fwd: str            # forward branch: 'fused' (projection inside the recurrence) | 'cluster2' | 'cluster' | 'stream'
    bptt: str           # BPTT kernel: 'cluster' | 'pair' | 'stream' (_bptt_kind)
    grad: bool          # a backward will follow: the fp16 copies are written and the backward's packs built in the forward
    gfmt: int           # storage of the saved gates / d(gates) (dev.gates_fmt, wesep_hip.h WS_GATES_*)
    g_fmt: int          # ... as the consumers of d(gates) name it: 0 split pairs, 1 bf16, 2 scaled fp16
    a16: bool           # fp16 copies of [xn | h] for the weight-gradient GEMMs (tnb_a16)
    pair_rfmt: int      # pair BPTT's recurrent product (pair_rfmt); 0 when another kernel runs
    band_rfmt: int      # streaming BPTT's recurrent product (band_rfmt); 0 when another kernel runs
    band_dx: bool       # the streaming BPTT writes d(xn) itself (band_dx)
    a_fmt: int          # a_fmt of the d(xn) GEMM over d(gates) (dxn_fmt)
    h2p: bool = False   # h leaves the recurrence as two fp16 planes: one buffer serves projection and weight gradients (dev.h2p_on)
    c16: bool = False   # the saved cell state is fp16 in BLH(2H): half the bytes written by the forward and read by the BPTT (dev.c16_on)


_WIHT_KIND = {0: "wihT", 1: "wihT", 2: "wihT16", 3: "wihT8"}     # BlstmPlan.a_fmt -> pack of W_ih^T for the d(xn) GEMM


def make_plan(seq, device, grad, gn_geo=None, ragged=False) -> BlstmPlan:
    """gn_geo: geometry of a GroupNorm in front of the BLSTM whose fused backward can add the two directions' d(xn) (band_dx);
    None: the caller has no such consumer and d(xn) always comes from the GEMM.
    ragged: the sequences have their own step counts (blstm_forward's `steps`): the forward takes a branch over precomputed
    gates ('cluster' / 'stream'), where ws_gemm_p2b_len zeroes the tails -- 'fused' and 'cluster2' project inside the
    recurrence and have no length operand."""
    lmode = dev.lstm_blk_mode(seq.nseq)
    cluster = dev.lstm_cluster_ok(seq, device)
    bptt = _bptt_kind(seq, device, cluster)
    # storage of the saved gates / d(gates): unorm16 gates in a BLH buffer of half the bytes by default (TF-GridNet's twelve
    # BLSTMs' saved gates were 77 of the step's 155 GB in round 3); the opt-in cluster BPTT knows the fp32 format only
    gfmt = L.GATES_F32 if bptt == "cluster" else dev.gates_fmt()
    h2 = gfmt != L.GATES_F32
    if ragged:
        fwd = "cluster" if cluster else "stream"
    elif dev.lstm_fuse_ok(seq.nseq, cluster):
        fwd = "fused"
    elif cluster:
        fwd = "cluster2" if h2 and dev.lstm_cluster2_on() else "cluster"
    else:
        fwd = "stream"
    g_fmt = {L.GATES_H2: 1, L.GATES_H2F: 2}.get(gfmt, 0)
    brf = band_rfmt(gfmt, lmode) if grad and bptt == "stream" else 0
    a16 = gfmt == L.GATES_H2F and grad and tnb_a16()
    # the planes replace the pair wherever the fp16 copies exist (a backward follows: inference and the ragged branches keep the
    # pair); the fused forward writes them from its fp16-h kernels only
    h2p = (a16 and dev.h2p_on(device) and not ragged and fwd in ("fused", "cluster2", "stream")
           and (fwd != "fused" or bool(dev.lstm_fused_hfmt(gfmt) & 1)))
    prf = pair_rfmt(gfmt) if grad and bptt == "pair" else 0
    bdx = bool(brf) and gn_geo is not None and band_dx(brf, seq, gn_geo)
    # the cell state in fp16 (C16, wesep_hip.h): every writer of the plan's forward branch -- the fall-back behind cluster2
    # included -- and every reader of its BPTT -- the fall-back behind the pair kernel included -- know the format; the writers
    # have it next to the fp16 planes of h (h2p: a backward follows, WS_GATES_H2F, device buffers, no ragged batch, forward
    # 'fused' on the fp16-h kernels / 'cluster2' / 'stream'), the readers are the pair kernel with all of W_hh resident (rfmt 2 /
    # 3) and the streaming kernels without their own d(xn).  |c_t| <= t: fp16 cannot overflow below 65 504 steps
    c16 = (h2p and grad and gfmt == L.GATES_H2F and dev.c16_on(device) and not ragged and seq.L <= dev.C16_MAX_STEPS
           and ((bptt == "pair" and prf in (2, 3) and not _pair_stamp_on()) or (bptt == "stream" and not bdx)))
    return BlstmPlan(
        nb=dev.bl_num_blocks(seq), lmode=lmode, cluster=cluster, fwd=fwd, bptt=bptt, grad=grad, gfmt=gfmt, g_fmt=g_fmt,
        a16=a16, pair_rfmt=prf, band_rfmt=brf, band_dx=bdx, a_fmt=dxn_fmt(g_fmt), h2p=h2p, c16=c16)


def consume_once(ctx, who):
    """BPTT turns the saved activated gates into d(gates) IN PLACE (and the deferred side-stream job reads them later): a
    second backward through the node would silently differentiate garbage."""
    if ctx.consumed:
        raise L.WesepHipError(f"{who}: second backward through the same graph (retain_graph / multi-loss loops): "
                              "the blocked path consumes its saved gates in place; run the forward again")
    ctx.consumed = True


# ---------------------------------------------------------------------------------------------
# the steps, in launch order
# ---------------------------------------------------------------------------------------------
def blstm_forward(plan, W, x, seq, res, bias, norm=None, steps=None, film=None):
    """out = res + Linear(BLSTM(x')) over the rows of the sequence map `seq`; x [rows, 128] plain, x' = x, or GroupNorm(x) with
    norm = dict(stats=, gamma=, beta=, stat_map=) (applied by ws_gemm_p2b on the way into BL).  W: the pack provider
    (WeightPacks).  Returns (out, saved): saved = (gates, cbuf, hcat, xn, hcat16) for ctx.save_for_backward -- xn is its
    fp16 copy when plan.a16 (the backward never reads the split-pair xn again), hcat16 is None without it and with plan.h2p
    (hcat then holds h as two fp16 planes and the copy is its first half: one tensor for h).
    steps (ragged batches, inference): (int32 device table, div) -- sequence s has table[s // div] valid steps; the
    pre-activations behind them are exact zeros, so the reverse direction reaches a sequence's last valid step with zero
    state (plan from make_plan(ragged=True); a branch that was not taught lengths refuses them).
    film (dev.Film; res is x): x and the residual are read through a folded speaker-fusion affine -- the relay / x-projection
    normalises film(x), the projection adds film(res); nothing else reads x."""
    d = x.device
    norm = dict(norm or {})
    if film is not None:
        if res is not x or steps is not None:
            raise L.WesepHipError("blstm_forward: film= folds ONE affine into operand and residual (res is x), no step counts")
        norm["film"] = film
    rk = dict(film=film) if film is not None else {}
    if steps is not None and (plan.fwd in ("fused", "cluster2") or plan.grad):
        raise L.WesepHipError(f"blstm_forward: per-sequence step counts with forward branch '{plan.fwd}', grad={plan.grad}: "
                              "only the branches over precomputed gates know them, and only the forward")
    lens = dict(steps=steps[0], steps_div=steps[1]) if steps is not None else {}
    nb, gfmt, lmode = plan.nb, plan.gfmt, plan.lmode
    h2 = gfmt != L.GATES_F32
    wcat, bcat = W("cat")
    whf, whr = W("whh")
    xn = _empty(d, nb, 32 * N)
    hcat = _empty(d, nb, 32 * 2 * H)
    cells = dict(c16=True) if plan.c16 else {}      # (the recurrences' keyword for the fp16 cell state)
    cbuf = _empty(d, dev.blh_floats(nb, 2 * H)) if plan.c16 else _empty(d, nb, 32 * 2 * H)
    gates = _empty(d, dev.blh_floats(nb, 2 * G4)) if h2 else _empty(d, nb, 32 * 2 * G4)
    # fp16 copies of the weight-gradient GEMM's A operand [xn | h] (ABI v16; written by the two GEMMs that touch these
    # operands anyway): ws_gemm_tnb then loads 32 instead of 56 KB per block and runs ONE MFMA per product.  TF-GridNet's
    # default too since round 6.  Round 5 left it opt-in there -- "these GEMMs already hide under the inter-frame BPTTs":
    # 304.3 vs 310.0 ms for 8 GB more saved state -- but hidden work is not free work on this chip
    # (profiles/r06_side_stream_tax.md: the clock follows the load): one MFMA per product instead of three on the side stream
    # is 263.6 -> 248.7 ms per step at config 5's per-GPU shape (two runs each, one box), 123 -> 131 GB
    xn16 = _empty(d, dev.blh_floats(nb, N)) if plan.a16 else None
    # plan.h2p: no twin -- `hcat` itself holds h as two fp16 planes (wesep_hip.h, H2P) and its first half IS that copy; the
    # projection then reads 4 bytes per element and writes none, where it read 4 and wrote 2, and dW_proj reads 2 instead of 4
    h2p = plan.h2p
    planes = dict(h2p=True) if h2p else {}      # (the recurrences' keyword for it)
    hcat16 = _empty(d, dev.blh_floats(nb, 2 * H)) if plan.a16 and not h2p else None
    if plan.fwd == "fused":
        # many short sequences (pBSRNN's band view, TF-GridNet's intra-frame path): the recurrence computes x W_ih^T itself
        # from the normalised input (BL(128)): the 16E-byte pre-activation buffer is never written and read back
        # (lstm_fused.hip)
        dev.gemm_p2b(A=x, lda=N, sm=seq, Wpack=None, N=0, C_out=None, A_bl=xn, A_bl16=xn16, **norm)
        hf = dev.lstm_fused_hfmt(gfmt)
        dev.lstm_fwd_fused(gates, cbuf, hcat, xn, W("fused8" if hf & 4 else "fused16" if hf else "fused"), bcat, seq, gfmt=gfmt,
                           hfmt=hf | (8 if h2p else 0), **cells)
    elif plan.fwd == "cluster2":
        # few long sequences (time view, inter-frame path), 2-byte formats (round 5): the cluster kernel computes x W_ih^T
        # itself from the normalised input (lstm_cluster2.hip) -- ws_gemm_p2b only normalises / relays (reads E, writes E
        # (+ E / 2 for the fp16 copy) instead of 17 E), the fp32 pre-activations exist only inside the predicated fall-back
        # behind the launch (the streaming pair, the whole layer again after a time-out: never NaN, no host round trip).
        # Measured for TF-GridNet at BASELINE config 5's geometry: 301.0 -> 277.7 ms/step (same box, together with the fp16
        # pair BPTT: profiles/r05_ab/r05_c11_tfg_*.json), every parity figure of the recipe-geometry test unchanged (waveform
        # 1.27e-5 -> 1.33e-5, worst gradient 3.4e-3 -> 3.1e-3, median 4.1e-4 -> 4.2e-4:
        # profiles/r05_tfg_cfg5_cluster2_bls_input.txt).  The kernel's FIRST cut -- fp16 copy of the input, two-term
        # x-projection -- was not: median gradient error 7.0e-4 and two scalar PReLU slopes over that model's 5e-3 bound
        # (profiles/r05_tfg_cfg5_precision_split.txt); the input keeps its split pair since.  WESEP_LSTM_CLUSTER2=0 selects
        # the round-4 cluster kernel on fp32 pre-activations
        dev.gemm_p2b(A=x, lda=N, sm=seq, Wpack=None, N=0, C_out=None, A_bl=xn, A_bl16=xn16, **norm)
        tw = dev.lstm_fwd_cluster2(gates, cbuf, hcat, xn, wcat, bcat, whf, whr, seq, dbg=_cluster_dbg(), **planes, **cells)
        pre = dev.fallback_scratch(d, nb * 32 * 2 * G4)       # (untouched after a clean launch; one buffer per stream)
        dev.gemm_p2b(A=x, lda=N, sm=seq, Wpack=W("wih"), N=2 * G4, C_out=pre, bias=bcat, run_if=tw, **norm)
        dev.lstm_fwd(gates, cbuf, hcat, W("hh")[0], seq, lmode, run_if=tw, gfmt=gfmt, gates_in=pre, **planes, **cells)
        del pre
    else:
        # pre-activations: in `gates` itself with the fp32 format (one buffer, three lives); with the 2-byte formats a
        # scratch buffer that dies with this forward (the recurrences read it and write the unorm16 gates next to it)
        pre = _empty(d, nb, 32 * 2 * G4) if h2 else gates
        xproj = dict(A=x, lda=N, sm=seq, Wpack=W("wih"), N=2 * G4, C_out=pre, bias=bcat, A_bl=xn, A_bl16=xn16, **norm, **lens)
        rec = dict(gfmt=gfmt, gates_in=pre) if h2 else {}
        # (the round-4 cluster kernel writes pairs only: make_plan never sets h2p for it)
        dev.gemm_p2b(**xproj)
        if _h2_probe() & 768 and not torch.cuda.is_available():
            # NUMERICS PROBE (CPU emulation only): the time view's pre-activations in 2 bytes -- fp16 (bit 256) / bf16 (512)
            pre.copy_(pre.half().float() if _h2_probe() & 256 else pre.bfloat16().float())
        if plan.fwd == "cluster":
            # weight-stationary cluster kernel; behind it the streaming pair predicated on the launch's timeout
            # word: two empty launches after a clean run, the whole layer again if the cluster's workgroups
            # were not co-resident (another stream / process on the GPU) -- never NaN (wesep_hip.h).  The 2-byte
            # formats leave the pre-activations intact: only the recurrence is repeated
            tw = dev.lstm_fwd_cluster(gates, cbuf, hcat, whf, whr, seq, dbg=_cluster_dbg(), **rec)
            if not h2:
                dev.gemm_p2b(run_if=tw, **xproj)
            dev.lstm_fwd(gates, cbuf, hcat, W("hh")[0], seq, lmode, run_if=tw, **rec)
        else:
            dev.lstm_fwd(gates, cbuf, hcat, W("hh")[0], seq, lmode, **planes, **cells, **rec)
        del pre
    out = torch.empty_like(res)
    if h2p:     # both planes against the fp16 hi / lo pack of 256 w: three fp16 MFMAs per product, no copy written
        dev.gemm_b2p(A=hcat, K=2 * H, sm=seq, Wpack=W("proj16"), C_out=out, ldc=N, bias=bias, R=res, a_fmt=4, **rk)
    else:
        dev.gemm_b2p(A=hcat, K=2 * H, sm=seq, Wpack=W("proj"), C_out=out, ldc=N, bias=bias, R=res, a16_out=hcat16, **rk)
    if _h2_probe() and not h2:
        if _h2_probe() & 1:
            _probe_round(gates, "f16")
        if _h2_probe() & 8:
            _probe_round(gates, "u16")
        if _h2_probe() & 4:
            _probe_round(cbuf, "f16")
    if plan.grad:     # (grad mode itself is always off inside a Function's forward)
        # the backward's packs (transposed projections, BPTT weight stream) are built here, where the GPU has a
        # single stream to serve: built lazily in the backward, these 5-10 us launches queue behind the side stream's
        # chip-filling weight-gradient GEMMs for up to a millisecond each (round 2 profile: 4 ms per step)
        W("projT")
        if not plan.band_dx:
            W(_WIHT_KIND[plan.a_fmt])
        if plan.bptt == "pair":
            W("hhp16" if plan.pair_rfmt else "hhp")
        if (plan.bptt == "stream" and not plan.band_rfmt) or (plan.bptt == "pair" and h2):
            W("hh")     # (the pair BPTT's predicated streaming fall-back of the 2-byte formats)
        if plan.bptt == "stream" and plan.band_rfmt:
            W("hh8")
            if plan.band_dx:
                W("wx8")
    return out, (gates, cbuf, hcat, xn16 if plan.a16 else xn, hcat16)


def blstm_bptt(plan, W, gates, cbuf, hcat, dout, seq, release):
    """Backward step 1: d(hcat) = dout Wp (+ dout itself in BL for the weight gradient), then the BPTT of the plan's kind
    with its fall-back: gates (activated) -> d(pre-activation gates).  release: this BPTT leaves part of the chip idle for
    milliseconds (pBSRNN's time view: the pair kernel on half of the CUs; TF-GridNet's inter-frame path: pair / cluster
    kernels, latency-bound on a fraction of the CUs for ~10 ms) -- the weight-gradient jobs deferred by the layers before it
    are released right after it is launched (flush_deferred_wgrads)."""
    d = dout.device
    nb, gfmt = plan.nb, plan.gfmt
    dh, dout_bl = _empty(d, nb, 32 * 2 * H), _empty(d, nb, 32 * N)
    dxn2 = None
    # WS_GATES_H2F: the d(hcat) GEMM raises max |d(hcat)| of this launch in a device word; the BPTT scales its fp16 d(gates)
    # by the power of two it defines, the two consumers of d(gates) undo it (wesep_hip.h)
    amax = amax_word(d) if gfmt == L.GATES_H2F else None
    cells = dict(c16=True) if plan.c16 else {}      # (cbuf holds fp16 cells: blstm_forward)
    dev.gemm_p2b(A=dout, lda=N, sm=seq, Wpack=W("projT"), N=2 * H, C_out=dh, A_bl=dout_bl, amax=amax)
    if _h2_probe() & 16:
        _probe_round(dh, "bf16")
    ready = mark_wgrads_ready(d) if release else None
    # few long sequences: the pair kernel (lstm_pair.hip) -- W_hh's hi plane resident across two workgroups per tile, on HALF
    # of the CUs, so the side stream keeps the other half.  The cluster BPTT (all 256 CUs: it evicts the
    # side-stream weight-gradient GEMMs) stays opt-in (WESEP_LSTM_CLUSTER_BWD=1).  Both work in place without a
    # device-side fall-back: FusedClipAdam.step looks at their status word (asynchronously for the pair kernel).
    # In place on the saved gates also because a clone is not free: 6.4 GB per BLSTM at TF-GridNet's 8 rows x 6 s, 12 copies
    # = 38 ms of a 490 ms step and the largest transient allocation of the backward
    if plan.bptt == "cluster":
        dg = gates
        dev.lstm_bwd_cluster(gates, cbuf, dh, *W("whh"), seq)
    elif gfmt == L.GATES_F32:
        # ABI <= 14 format: split-pair d(gates) in place over the fp32 gates; a pair time-out has no device-side repair
        # (FusedClipAdam skips the update on the device and raises)
        dg = gates
        if plan.bptt == "pair":
            dev.lstm_bwd_pair(gates, cbuf, dh, W("hhp"), seq, dbg=_pair_dbg())
        else:
            dev.lstm_bwd(gates, cbuf, hcat, dh, W("hh")[1], seq, plan.lmode)
    elif plan.bptt == "pair":
        # 2-byte formats: d(gates) go to a buffer of their own (bf16 in BLH for H2: the same bytes written as in place),
        # so the saved gates survive the launch and the streaming BPTT can stand behind it, predicated on the launch's
        # time-out word: an empty launch after a clean run, the whole BPTT again if the pair's workgroups were not
        # co-resident (a resident RCCL kernel, another process) -- no NaN reaches a consumer (wesep_hip.h)
        dg = _empty(d, nb, 32 * 2 * G4) if gfmt == L.GATES_H2S else _empty(d, dev.blh_floats(nb, 2 * G4))
        rf = plan.pair_rfmt
        tw = dev.lstm_bwd_pair(gates, cbuf, dh, W("hhp16" if rf else "hhp"), seq, gfmt=gfmt, dgates=dg, repairable=True,
                               dbg=_pair_dbg(), amax=amax, rfmt=rf, dbg_buf=_pair_stamp_buf(d, seq.L), **cells)
        dev.lstm_bwd(gates, cbuf, hcat, dh, W("hh")[1], seq, plan.lmode, gfmt=gfmt, dgates=dg, run_if=tw, amax=amax, **cells)
    else:
        # streaming BPTT (many short sequences): bf16 d(gates) in place over the unorm16 gates (H2) / split pairs to their own
        # buffer (H2S)
        dg = _empty(d, nb, 32 * 2 * G4) if gfmt == L.GATES_H2S else gates
        brf = plan.band_rfmt
        if plan.band_dx:
            dxn2 = _empty(d, 2, dout.numel() // N, N)        # d(xn) of each direction, written by the BPTT itself
        dev.lstm_bwd(gates, cbuf, hcat, dh, W("hh8") if brf else W("hh")[1], seq, plan.lmode, gfmt=gfmt,
                     dgates=dg if gfmt == L.GATES_H2S else None, amax=amax, rfmt=brf, dxn=dxn2,
                     wxpack=W("wx8") if dxn2 is not None else None, **cells)
    if _h2_probe() & 2 and gfmt == L.GATES_F32:
        _probe_round(gates, "bf16", packed=True)
    if _h2_probe() & 32 and gfmt == L.GATES_F32 and not torch.cuda.is_available():
        # fp16 d(gates) scaled by a power of two taken from max |d(hcat)| of this launch (CPU emulation only: plain fp32)
        amax = float(dh.abs().max())
        S = 2.0 ** (10 - math.floor(math.log2(amax))) if amax > 0 and math.isfinite(amax) else 1.0
        sc = gates * S
        _PROBE_SAT[0] += int((sc.abs() > 65504.0).sum())
        _PROBE_SAT[1] = max(_PROBE_SAT[1], float(sc.abs().max()) / 65504.0)
        gates.copy_(sc.clamp(-65504.0, 65504.0).half().float() / S)
    if ready is not None:
        flush_deferred_wgrads(d, ready)
    return dg, dout_bl, amax, dxn2


def weight_grads(gates, xn, hcat, dout_bl, seq, nb, g_fmt=0, amax=None, hcat16=None, h2p=False):
    """[dW_ih | dW_hh | db] of both directions in one pass over each direction's dgates, and
    dW_proj / db_proj; launched on the current stream.  Returns them in nn.LSTM parameter order: [dW_ih_f, dW_hh_f, db_f,
    db_f (clone), dW_ih_r, dW_hh_r, db_r, db_r (clone), dW_proj, db_proj].  hcat16 given: `xn` and it are the fp16 copies in
    BLH (ws_gemm_tnb a_fmt = 1; g_fmt 2 only).  h2p: `hcat` holds h as two fp16 planes; its hi plane is that copy and the
    operand of dW_proj too (ws_gemm_tnb_h16)."""
    d = gates.device
    if h2p:
        hcat16 = dev.h2p_hi(hcat, nb)
    a_fmt = 1 if hcat16 is not None else 0
    if _h2_probe() & 192 and not torch.cuda.is_available() and not a_fmt:
        # NUMERICS PROBE (CPU emulation only: plain fp32 buffers): the A operand [xn | h] of the weight-gradient GEMMs at
        # fp16 (bit 64) / bf16 (bit 128) -- what a 2-byte A operand of ws_gemm_tnb would cost
        rnd = (lambda t: t.half().float()) if _h2_probe() & 64 else (lambda t: t.bfloat16().float())
        xn, hcat = rnd(xn), rnd(hcat)
    if os.environ.get("WESEP_PROBE_SKIP_WGRAD") == "1":   # measurement only: how much of this is exposed?
        z_ = lambda *s_: torch.zeros(*s_, device=d)
        return [z_(G4, N), z_(G4, H), z_(G4), z_(G4), z_(G4, N), z_(G4, H), z_(G4), z_(G4), z_(N, 2 * H), z_(N)]
    if _h2_probe() & 1024 and not torch.cuda.is_available() and amax is not None:
        # NUMERICS PROBE (CPU emulation only): the proj weight gradient on fp16 operands -- h as fp16, the incoming
        # gradient as fp16 scaled by the d(gates) scale of this backward (L.dgates_scale)
        S = L.dgates_scale(int(amax.reshape(-1)[0]))
        hcat = hcat.half().float()
        dout_bl = (dout_bl * S).half().float() / S
    # dW_proj^T [2H][N] = hcat^T dout (hcat as the streamed-once operand), db_proj = colsum(dout)
    ns, bps = dev.tnb_splits(nb, (2 * H) // 128)
    slab, aslab = _empty(d, ns, 2 * H * N), _empty(d, ns, N)
    if h2p:     # fp16(h) against the stored pairs of dout lifted into fp16 by this backward's scale: two fp16 MFMAs per product
        dev.gemm_tnb_h16(G=hcat16, g_width=2 * H, g_off=0, g_cols=2 * H, A0=dout_bl, a0_width=N, a0_off=0, nblk=nb, L_=seq.L,
                         slab=slab, nsplit=ns, blocks_per_split=bps, amax=amax, aslab=aslab)
    else:
        dev.gemm_tnb(G=hcat, g_width=2 * H, g_off=0, g_cols=2 * H, A0=dout_bl, a0_width=N, a0_off=0, a0_cols=N,
                     nblk=nb, L_=seq.L, slab=slab, nsplit=ns, blocks_per_split=bps, aslab=aslab)
    dproj_w = _reduce_new(slab, ns, 2 * H * N, (2 * H, N)).t().contiguous()
    dproj_b = _reduce_new(aslab, ns, N, (N,))
    ns, bps = dev.tnb_splits(nb, G4 // 128)
    slab, bslab = _empty(d, ns, G4 * (N + H)), _empty(d, ns, G4)
    dwih, dwhh, db = [], [], []
    for di in (0, 1):
        dev.gemm_tnb(G=gates, g_width=2 * G4, g_off=di * G4, g_cols=G4, A0=xn, a0_width=N, a0_off=0,
                     a0_cols=N, A1=hcat16 if a_fmt else hcat, a1_width=2 * H, a1_off=di * H, a1_cols=H,
                     a1_shift=(-1 if di == 0 else 1), nblk=nb, L_=seq.L, slab=slab, nsplit=ns,
                     blocks_per_split=bps, bslab=bslab, g_fmt=g_fmt, amax=amax, a_fmt=a_fmt)
        dw = _reduce_new(slab, ns, G4 * (N + H), (G4, N + H))
        dwih.append(dw[:, :N].contiguous())
        dwhh.append(dw[:, N:].contiguous())
        db.append(_reduce_new(bslab, ns, G4, (G4,)))
    # b_ih and b_hh receive the same gradient; clone so their .grad never alias
    return [dwih[0], dwhh[0], db[0], db[0].clone(), dwih[1], dwhh[1], db[1], db[1].clone(),
            dproj_w, dproj_b]


def blstm_weight_grads(plan, dg, xn, hcat, dout_bl, amax, hcat16, seq, box, order=tuple(range(10))):
    """Backward step 2: the weight gradients -- a side branch of the graph (nothing downstream reads them).  box None: in
    line, returned.  box given (the WGradBox of this BLSTM's carrier): deferred to the side stream as a job that fills the
    box, records its event and keeps its operands valid (keep_for_side); Nones are returned and the carrier delivers.
    order: which of weight_grads' ten the caller's weight arguments take, in the order of those arguments."""
    if box is None:
        wg = weight_grads(dg, xn, hcat, dout_bl, seq, plan.nb, plan.g_fmt, amax, hcat16, h2p=plan.h2p)
        return [wg[i] for i in order]
    prod = torch.cuda.current_stream()

    def job(side):
        wg = weight_grads(dg, xn, hcat, dout_bl, seq, plan.nb, plan.g_fmt, amax, hcat16, h2p=plan.h2p)
        box.grads = [wg[i] for i in order]
        box.event = torch.cuda.Event()
        box.event.record(side)
        keep_for_side(box, (dg, xn, hcat, dout_bl, amax, hcat16), side, prod)
    defer_wgrad(dg.device, job)
    return [None] * len(order)


def blstm_dxn(plan, W, dg, amax, dxn2, seq, rows):
    """Backward step 3: d(x') = d(gates) Wcat as (dxn, None) from ws_gemm_b2p over the `rows` plain rows of the sequence map,
    or the two directions' halves (dxn_f, dxn_r) the streaming BPTT wrote itself."""
    if dxn2 is not None:
        return dxn2[0], dxn2[1]
    dxn = _empty(dg.device, rows, N)
    dev.gemm_b2p(A=dg, K=2 * G4, sm=seq, Wpack=W(_WIHT_KIND[plan.a_fmt]), C_out=dxn, ldc=N, a_fmt=plan.a_fmt, amax=amax)
    return dxn, None
