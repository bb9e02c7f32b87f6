"""Streaming inference for causal Conv-TasNet / SpEx+ with the carried state on the device.

`ConvTasNetStreamer(model, rows)` is a chunked forward of a `ConvTasNet(causal=True)` in eval mode: audio is pushed as it
arrives, in chunks of any size, and the concatenation of what `push` and `flush` return is the estimate
`model(x, emb)[0]` on the concatenated input ([R, T_out]; the plain ends' forward returns the same rows as [R, 1, T_out]).
Every encoder frame, block frame and output sample is computed once.  Only two kernels of a causal model look across time:
the depthwise dilated convolution and the decoder's overlap-add.  Their chunked forms (csrc/stream.hip) carry a ring of
normalised past frames per block and the not-yet-final samples of the overlap-add; everything else is per frame and runs
through the model's own launches on the chunk.

Emission rule, with s = L / 2 and N samples pushed so far: frame k is computed once k * s + Lmax <= N (Lmax: the longest
encoder window, 160 for the Multi ends, L for the plain ones); after K frames, samples [0, K * s) are final and have been
returned.  `flush` zero-extends the pending samples as the whole-utterance encoder does at its end, runs the remaining
frames up to T' = (N - L) // s + 1 and returns the rest: (T' - 1) * s + L samples in all, the length of `model(x, emb)[0]`.

Not built (refused by name at construction): non-causal blocks, gLN (its statistics span the utterance), the Deep ends
(their dilated convolutions look ahead) and training mode.  All rows advance in lockstep.

`fused=True` (cLN models) runs the five launches between a block's two GEMMs as one, `dev.tcn_mid_stream_fwd`: three C-ABI
calls per block in place of seven.  `block=True` (cLN blocks without skip connections) runs the whole block as one,
`dev.tcn_block_stream_fwd`: one call per block, and the estimate's bits no longer depend on how the audio was cut into
packets.  The default issues the unfused launches."""
import torch

from . import _lib as L
from . import dev
from . import functional_tasnet as FT
from .dev import Rows, StatMap
from .functional import LinearFn, _empty
from .modules.tasnet import Conv1DBlock, Conv1DBlock4Fuse, Separation, _FuseLayer, apply_norm


class ConvTasNetStreamer:
    def __init__(self, model, rows, max_chunk_frames=256, fused=False, block=False):
        from .models.convtasnet import ConvTasNet
        if not isinstance(model, ConvTasNet):
            raise TypeError(f"ConvTasNetStreamer: a ConvTasNet is needed, got {type(model).__name__}")
        if model.training:
            raise L.WesepHipError("ConvTasNetStreamer: the model is in training mode; streaming is inference (call model.eval())")
        if "Deep" in (model.encoder_type, model.decoder_type):
            raise NotImplementedError("ConvTasNetStreamer: the Deep encoder / decoder look ahead (dilated convolutions centred "
                                      "on the frame); Deep ends cannot be streamed")
        if model.norm_type == "gLN":
            raise NotImplementedError("ConvTasNetStreamer: norm='gLN' takes its statistics over the whole utterance; "
                                      "stream a cLN or BN model")
        blocks = [m for m in model.separation.modules() if isinstance(m, (Conv1DBlock, Conv1DBlock4Fuse))]
        if not all(b.causal for b in blocks):
            raise NotImplementedError("ConvTasNetStreamer: non-causal blocks look ahead; build the model with causal=True")
        if fused and model.norm_type != "cLN":
            raise NotImplementedError(f"ConvTasNetStreamer: fused=True is built for cLN blocks; this model's norm is "
                                      f"{model.norm_type!r} (BN runs the unfused launches: fused=False)")
        self.fused = bool(fused)
        if block and model.norm_type != "cLN":
            raise NotImplementedError(f"ConvTasNetStreamer: block=True is built for cLN blocks; this model's norm is "
                                      f"{model.norm_type!r} (BN runs the unfused launches: block=False)")
        if block and any(getattr(b, "skip_con", False) for b in blocks):
            raise NotImplementedError("ConvTasNetStreamer: block=True has no skip-connection branch; this model's blocks "
                                      "have skip connections (skip_con=True): stream it with fused=True or the default")
        self.block = bool(block)
        if int(rows) < 1 or int(max_chunk_frames) < 1:
            raise ValueError(f"ConvTasNetStreamer: rows={rows}, max_chunk_frames={max_chunk_frames} must be positive")
        self.model, self.rows, self.max_chunk_frames = model, int(rows), int(max_chunk_frames)
        self.multi = model.encoder_type == "Multi"
        self.stride = model.stride
        enc = model.encoder
        self.L = enc.L1 if self.multi else enc[0].kernel_size[0]
        self.Lmax = max(enc.L1, enc.L2, enc.L3) if self.multi else self.L
        if self.L % self.stride:
            raise NotImplementedError(f"ConvTasNetStreamer: the encoder window L={self.L} must be even (hop = L / 2)")
        self._blocks = blocks
        self._dev = next(model.parameters()).device
        dec = model.decoder.decoder_1d_1 if self.multi else model.decoder
        self._dec = dec
        N = dec.weight.shape[0]
        with torch.no_grad():      # the synthesis matrix [L, N], laid out once (the weights are read at construction)
            self._WT = FT._transposed(dec.weight.reshape(N, self.L).contiguous(), N, self.L)
        self._rings = {}
        for b in blocks:
            conv = b.dconv if isinstance(b, Conv1DBlock4Fuse) else b.dwconv
            H, P = conv.weight.shape[0], conv.weight.shape[-1]
            self._rings[id(b)] = torch.empty(self.rows, (P - 1) * b.dilation + self.max_chunk_frames, H, device=self._dev,
                                             dtype=torch.float32)
        self._carry = torch.empty(self.rows, self.L - self.stride, device=self._dev, dtype=torch.float32)
        self._emb = None
        self._rb = {}
        self.reset()

    # ---- state -------------------------------------------------------------------------------------------------------
    def reset(self):
        """Back to sample 0; the enrollment is kept.  The rings need no clearing: frames before the start are never read."""
        self._pend = torch.empty(self.rows, 0, device=self._dev, dtype=torch.float32)
        self._n, self._k, self._done = 0, 0, False
        with torch.no_grad():
            if self._dec.bias is not None:
                self._carry.copy_(self._dec.bias.detach().reshape(1, 1).expand_as(self._carry))
            else:
                self._carry.zero_()

    @property
    def latency_samples(self):
        """The longest encoder window: a frame is computed once that many samples from its start have arrived."""
        return self.Lmax

    @property
    def state_bytes(self):
        """Carried device state: the blocks' rings, the overlap-add carry and the pending samples (fewer than Lmax a row)."""
        return 4 * (sum(r.numel() for r in self._rings.values()) + self._carry.numel() + self.rows * self.Lmax)

    @property
    def frames_emitted(self):
        return self._k

    @property
    def samples_pushed(self):
        return self._n

    # ---- enrollment --------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def enroll(self, enrollment):
        """The speaker embedding, once, by the model's own code: a fixed embedding [rows, E], an enrollment waveform
        [rows, Tw] through the shared encoder and the SpEx+ speaker encoder, or fbank features [rows, Te, F] through a
        wespeaker encoder; then `spk_transform`, and for concatConv the per-stack rows W_e e + b."""
        m = self.model
        self._check_eval()
        e = enrollment.contiguous().float()
        if e.shape[0] != self.rows:
            raise ValueError(f"ConvTasNetStreamer.enroll: {e.shape[0]} rows, the streamer has {self.rows}")
        if m.joint_training and m.spk_feat:
            e, _ = m._wespeaker_embedding(e)
        elif m.joint_training:
            _, cat_aux, Tpa = m.encoder(e)
            e = m.spk_model(cat_aux, (self.rows, Tpa))
        self._emb = m.spk_transform(e).contiguous()
        self._rb = {}
        for b in self._blocks:
            if isinstance(b, Conv1DBlock4Fuse):
                w = b.conv1x1.weight
                self._rb[id(b)] = LinearFn.apply(self._emb, w[:, b.in_channels:, 0], b.conv1x1.bias).contiguous()
        return self._emb

    def _check_eval(self):
        if self.model.training:
            raise L.WesepHipError("ConvTasNetStreamer: the model is in training mode; streaming is inference (call model.eval())")

    # ---- the chunked forward --------------------------------------------------------------------------------------------
    @torch.no_grad()
    def push(self, chunk):
        """chunk [rows, n], n >= 1 -> the samples that became final, [rows, m] (m = 0 while no new frame is complete)."""
        self._check_eval()
        if self._emb is None:
            raise L.WesepHipError("ConvTasNetStreamer.push: no enrollment yet (call enroll first)")
        if self._done:
            raise L.WesepHipError("ConvTasNetStreamer.push: the stream was flushed (call reset to start another)")
        if chunk.dim() != 2 or chunk.shape[0] != self.rows or chunk.shape[1] < 1:
            raise ValueError(f"ConvTasNetStreamer.push: chunk is {tuple(chunk.shape)}, expected [{self.rows}, n >= 1]")
        self._pend = torch.cat([self._pend, chunk.to(self._dev).float()], 1)
        self._n += chunk.shape[1]
        target = (self._n - self.Lmax) // self.stride + 1 if self._n >= self.Lmax else 0
        return self._advance(target, [])

    @torch.no_grad()
    def flush(self):
        """The end of the stream: the remaining frames on the zero-extended pending samples, then the carry."""
        self._check_eval()
        if self._done:
            raise L.WesepHipError("ConvTasNetStreamer.flush: the stream was flushed already (call reset)")
        if self._n < self.L:
            raise RuntimeError(f"ConvTasNet: input of {self._n} samples is shorter than the encoder window {self.L}")
        if self._emb is None:
            raise L.WesepHipError("ConvTasNetStreamer.flush: no enrollment yet (call enroll first)")
        out = self._advance((self._n - self.L) // self.stride + 1, [])
        self._done = True
        return torch.cat([out, self._carry], 1)

    def _advance(self, target, outs):
        while self._k < target:
            outs.append(self._run(min(target - self._k, self.max_chunk_frames)))
        if not outs:
            return torch.empty(self.rows, 0, device=self._dev, dtype=torch.float32)
        return outs[0] if len(outs) == 1 else torch.cat(outs, 1)

    def _run(self, Tc):
        """Frames [k, k + Tc): encoder, separation, mask, synthesis frames, overlap-add.  Returns est [rows, Tc * s]."""
        R, s, m = self.rows, self.stride, self.model
        need = (Tc - 1) * s + self.Lmax
        xp = torch.zeros(R, -(-need // 4) * 4, device=self._dev, dtype=torch.float32)
        have = min(need, self._pend.shape[1])
        xp[:, :have] = self._pend[:, :have]
        geo = (R, Tc)
        if self.multi:
            e, cat = self._multi_encoder(xp, Tc)
        else:
            w = self._frames_gemm(xp, Tc, m.encoder[0], None, 0)
            e = apply_norm(m.LayerN_S, m.norm_type, w, geo, False)
            from . import functional_campplus as FP
            e = FP.Conv1dFn.apply(e, (R, Tc, 1, 1), m.BottleN_S.weight, m.BottleN_S.bias)
        e = self._separation(e, geo)
        M = R * Tc
        if self.multi:
            dec = m.decoder
            N, B = dec.mask1.weight.shape[0], dec.mask1.weight.shape[1]
            mask = FT._gemm(e.contiguous(), M, B, dec.mask1.weight.reshape(N, B).contiguous(), N, bias=dec.mask1.bias, act=2)
            sm = _empty(self._dev, M, N)
            dev.maskmul_fwd(cat, 0, 3 * N, mask, M, N, sm)
        else:
            from . import functional_ecapa as FE
            gw = m.gen_masks.weight.view(m.gen_masks.weight.shape[0], -1)
            N = gw.shape[0]
            if m.activate == "relu":
                mask = FE.LinearReluFn.apply(e, gw, m.gen_masks.bias)
            else:
                mask = FE.RowBiasActFn.apply(LinearFn.apply(e, gw, m.gen_masks.bias), None, 1, 3)
            sm = FT.MulFn.apply(w, mask)
        fr = FT._gemm(sm, M, N, self._WT, self.L)
        est = _empty(self._dev, R, Tc * s)
        dev.ola_stream_fwd(fr, self._dec.bias, R, Tc, self.L, s, self._carry, est)
        self._pend = self._pend[:, Tc * s:]
        self._k += Tc
        return est

    def _frames_gemm(self, xp, Tc, conv, out, c_off):
        """ReLU(conv1d) of Tc overlapping frames of xp [rows, Tpad] as one GEMM on the frame view (PlainEncoderFn)."""
        N, _, Lk = conv.weight.shape
        return FT._gemm(xp, self.rows * Tc, Lk, conv.weight.reshape(N, Lk).contiguous(), N, bias=conv.bias, act=2,
                        a_rows=Rows(Tc, xp.shape[1], self.stride), out=out, c_ld=None if out is None else out.shape[1],
                        c_off=c_off, vec=2 if Lk % 4 == 0 else 0)

    def _multi_encoder(self, xp, Tc):
        """MultiEncoderFn.forward on Tc frames of the padded buffer: (e [rows*Tc, B], cat [rows*Tc, 3N])."""
        enc = self.model.encoder
        N = enc.encoder_1d_short.weight.shape[0]
        M = self.rows * Tc
        cat = _empty(self._dev, M, 3 * N)
        for i, conv in enumerate((enc.encoder_1d_short, enc.encoder_1d_middle, enc.encoder_1d_long)):
            self._frames_gemm(xp, Tc, conv, cat, i * N)
        st = _empty(self._dev, M, 2)
        dev.group_stats(cat, FT._cln_geom(M, 3 * N), st, FT.LN_EPS)
        B = enc.proj.weight.shape[0]
        e = FT._gemm(cat, M, 3 * N, enc.proj.weight.reshape(B, 3 * N).contiguous(), B, bias=enc.proj.bias,
                     norm=(st, enc.ln.weight, enc.ln.bias, StatMap(1, 1, 1, 0, 0)))
        return e, cat

    def _separation(self, x, geo):
        """FuseSeparation.forward with every conv block replaced by its chunked form."""
        sep = self.model.separation
        for mod in sep.separation:
            if isinstance(mod, Conv1DBlock4Fuse):
                x = self._block(mod, x, geo)
            elif isinstance(mod, Separation):
                if mod.skip_con:
                    total = None
                    for blk in mod.separation:
                        x, skip = self._block(blk, x, geo)
                        total = skip if total is None else total + skip
                    x = total
                else:
                    for blk in mod.separation:
                        x = self._block(blk, x, geo)
            elif isinstance(mod, _FuseLayer):
                x = mod(x, self._emb, geo)
            elif isinstance(mod, torch.nn.PReLU):
                x = mod(x)
            else:                                   # the select_norm module between the fusion layer and the stack
                x = apply_norm(mod, sep.norm_type, x, geo, False)
        return x

    def _block(self, b, x, geo):
        R, Tc = geo
        fuse = isinstance(b, Conv1DBlock4Fuse)
        n1, n2 = (b.lnorm1, b.lnorm2) if fuse else (b.norm_1, b.norm_2)
        bn = (n1.running_mean, n1.running_var, n2.running_mean, n2.running_var) if b.norm_type == "BN" else None
        g = (R, Tc, b.norm_type, b.dilation, bn)
        ring = self._rings[id(b)]
        if fuse:
            return FT.conv_block_stream(x, self._rb[id(b)], g, ring, self._k, b.conv1x1.weight, b.conv1x1.bias,
                                        b.prelu1.weight, n1.weight, n1.bias, b.dconv.weight, b.dconv.bias, b.prelu2.weight,
                                        n2.weight, n2.bias, b.sconv.weight, b.sconv.bias, fused=self.fused,
                                        block=self.block)
        skip = (b.Sc_conv.weight, b.Sc_conv.bias) if b.skip_con else ()
        return FT.conv_block_stream(x, None, g, ring, self._k, b.conv1x1.weight, b.conv1x1.bias, b.PReLU_1.weight,
                                    n1.weight, n1.bias, b.dwconv.weight, b.dwconv.bias, b.PReLU_2.weight, n2.weight,
                                    n2.bias, b.Output.weight, b.Output.bias, *skip, fused=self.fused, block=self.block)
