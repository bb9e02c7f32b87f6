"""Autograd shims of the TF-GridNet path over the C ABI.

Channels-last grids [B*T*Q, C] (T frames, Q frequency bins).  Everything is composed from entry points that other rows
already use, plus one row-softmax kernel:
  * the BLSTMs (hidden 192, input emb_dim * emb_ks) run on the split-bf16 recurrence kernels built for hidden 256:
    the weights are ZERO-PADDED to 256 units -- a padded unit has pre-activations 0, so i = f = o = 1/2, g = 0, c = h = 0
    for ever, and its outgoing weights are zero: the padded network computes exactly the same function;
  * `F.unfold(..., (emb_ks, 1), stride (emb_hs, 1))` in front of a BLSTM is an overlapping ROW VIEW of the layer-normed
    sequence (window of emb_ks consecutive positions = emb_ks * C contiguous floats) fed to the input-projection GEMM; its
    adjoint and the ConvTranspose1d behind the BLSTM are GEMM + the generic overlap-add kernel (hop = emb_hs * C floats);
  * LayerNorm over C, LayerNormalization4DCF over (C, F) and AllHeadPReLULayerNormalization4DCF over (E, F) are all
    "one mean/variance per row, affine per column" on a suitably flattened [rows, width] view -> the cLN kernels;
  * the full-band self-attention is two GEMMs per (batch row, head) around the row softmax.
Reference lines: wesep/models/tfgridnet.py:197-302, wesep/modules/tfgridnet/gridnet_block.py:118-284."""
import numpy as np
import os

import torch

from . import _lib as L
from . import dev
from .dev import BIG, Rows, SeqMap, flat
from .blstm_core import PackCache, WeightPacks, blstm_bptt, blstm_dxn, blstm_forward, blstm_weight_grads, consume_once, make_plan
from .functional import _empty, _need_cuda, _reduce_new
from .functional_tasnet import _cln_geom, _gemm, _transposed, _wgrad, norm_backward

HP = L.LSTM_H          # 256: hidden size the recurrence kernels are built for
G4P = 4 * HP


def pad_lstm(w_ih, w_hh, b_ih, b_hh, col_perm=None):
    """nn.LSTM tensors of hidden size h <= 256 -> (w_ih [1024, K], w_hh [1024, 256], b [1024]) zero-padded to 256 units
    (gate-major rows g*256 + u).  torch index ops on small weight tensors: gradients flow back through them."""
    h = w_hh.shape[1]
    if h > HP:
        raise NotImplementedError(f"TF-GridNet lstm_hidden_units={h} > {HP}")
    d = w_ih.device
    rows = (torch.arange(4, device=d).unsqueeze(1) * HP + torch.arange(h, device=d).unsqueeze(0)).reshape(-1)
    wi = w_ih if col_perm is None else w_ih[:, col_perm]
    wi_p = torch.zeros(G4P, wi.shape[1], device=d, dtype=torch.float32).index_copy(0, rows, wi)
    wh_c = torch.zeros(4 * h, HP, device=d, dtype=torch.float32)
    wh_c = torch.cat([w_hh, wh_c[:, h:]], 1)
    wh_p = torch.zeros(G4P, HP, device=d, dtype=torch.float32).index_copy(0, rows, wh_c)
    b_p = torch.zeros(G4P, device=d, dtype=torch.float32).index_copy(0, rows, b_ih + b_hh)
    return wi_p, wh_p, b_p


def pad_hidden_cols(w, h):
    """[N, 2h] (forward | reverse hidden) -> [N, 512] with each half zero-padded to 256 columns."""
    N = w.shape[0]
    z = torch.zeros(N, HP - h, device=w.device, dtype=torch.float32)
    return torch.cat([w[:, :h], z, w[:, h:], z], 1)


class BlstmFn(torch.autograd.Function):
    """src [nseq*Lr, C] (layer-normed) -> hcat [nseq*n, 512]: windows of ks positions (hop hs) -> input projection ->
    bidirectional recurrence.  Weights are the padded tensors of pad_lstm (both directions stacked)."""

    @staticmethod
    def forward(ctx, src, geo, wcat, bcat, whf, whr):
        _need_cuda(src, "TF-GridNet")
        nseq, Lr, C, ks, hs = geo
        n = (Lr - ks) // hs + 1
        P, K = nseq * n, ks * C
        src = src.contiguous()
        d = src.device
        rows = Rows(n, Lr * C, hs * C)
        gates = _empty(d, P, 2 * G4P)
        dev.gemm_nt(A=src, a_rows=rows, M=P, N=2 * G4P, K=K, W=wcat, ldw=K, bias=bcat, C_out=gates, c_rows=flat(2 * G4P),
                    vec=3 if (C % 4 == 0) else 0)
        pack_f, pack_b = _empty(d, L.LSTM_PACK_FLOATS), _empty(d, L.LSTM_PACK_FLOATS)
        mode = dev.lstm_mode(nseq)
        dev.lstm_pack(whf.contiguous(), whr.contiguous(), pack_f, pack_b, mode)
        cbuf, hcat = _empty(d, P, 2 * HP), _empty(d, P, 2 * HP)
        seq = SeqMap(nseq, BIG, 0, n, 1, n)
        dev.lstm_fwd(gates, cbuf, hcat, pack_f, seq, mode)
        ctx.save_for_backward(src, gates, cbuf, hcat, wcat, pack_b)
        ctx.geo = (nseq, Lr, C, ks, hs, n, mode)
        return hcat

    @staticmethod
    def backward(ctx, dhcat):
        src, gates, cbuf, hcat, wcat, pack_b = ctx.saved_tensors
        nseq, Lr, C, ks, hs, n, mode = ctx.geo
        P, K = nseq * n, ks * C
        d = src.device
        seq = SeqMap(nseq, BIG, 0, n, 1, n)
        gates = gates.clone()                                    # BPTT works in place; keep the saved tensor intact
        dev.lstm_bwd(gates, cbuf, hcat, dhcat.contiguous(), pack_b, seq, mode)
        nsplit, rps = dev.tn_splits(P)
        dwhh = []
        slab = _empty(d, nsplit, G4P * HP)
        for di in (0, 1):
            dev.gemm_tn(G=gates, g_rows=flat(2 * G4P), g_off=di * G4P, A=hcat, a_rows=flat(2 * HP), a_off=di * HP, M=P,
                        Nn=G4P, Kk=HP, slab=slab, slab_stride=G4P * HP, nsplit=nsplit, rows_per_split=rps,
                        shift_rows=(-1 if di == 0 else 1), seq_div=1, seq_len=n)
            dwhh.append(_reduce_new(slab, nsplit, G4P * HP, (G4P, HP)))
        rows = Rows(n, Lr * C, hs * C)
        dwcat, dbcat = _wgrad(gates, P, 2 * G4P, src, K, a_rows=rows, vec=1 if C % 4 == 0 else 0)
        dxu = _gemm(gates, P, 2 * G4P, _transposed(wcat, 2 * G4P, K), K)
        dsrc = _empty(d, nseq, Lr * C)
        dev.ola_fwd(dxu, None, nseq, n, K, hs * C, Lr * C, dsrc)          # adjoint of the window view: overlap-add
        return dsrc.view(nseq * Lr, C), None, dwcat, dbcat, dwhh[0], dwhh[1]


class Deconv1dFn(torch.autograd.Function):
    """hcat [nseq*n, 512] -> [nseq*Lr, C]: ConvTranspose1d(2h -> C, ks, stride hs) along the sequence
    (gridnet_block.py:47-51): GEMM to frames (column i*C + c) + overlap-add with hop hs*C floats."""

    @staticmethod
    def forward(ctx, hcat, geo, Wt):
        nseq, Lr, C, ks, hs, n = geo
        hcat = hcat.contiguous()
        fr = _gemm(hcat, nseq * n, 2 * HP, Wt, ks * C)
        y = _empty(hcat.device, nseq, Lr * C)
        dev.ola_fwd(fr, None, nseq, n, ks * C, hs * C, Lr * C, y)
        ctx.save_for_backward(hcat, Wt)
        ctx.geo = geo
        return y.view(nseq * Lr, C)

    @staticmethod
    def backward(ctx, dy):
        hcat, Wt = ctx.saved_tensors
        nseq, Lr, C, ks, hs, n = ctx.geo
        P = nseq * n
        dfr = _empty(dy.device, P, ks * C)
        dev.ola_bwd(dy.contiguous().view(nseq, Lr * C), nseq, n, ks * C, hs * C, Lr * C, dfr)
        dWt, _ = _wgrad(dfr, P, ks * C, hcat, 2 * HP, with_bias=False)
        dh = _gemm(dfr, P, ks * C, _transposed(Wt, ks * C, 2 * HP), 2 * HP)
        return dh, None, dWt


class AddRowVecFn(torch.autograd.Function):
    """x [M, C] + b [C]."""

    @staticmethod
    def forward(ctx, x, b):
        x = x.contiguous()
        y = torch.empty_like(x)
        M, C = x.shape
        dev.affine_fwd(x, None, b.contiguous().view(1, C), 1.0, M, M, C, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = dy.contiguous()
        M, C = dy.shape
        db = dev.chan_sums(dy, None, None, 1, M, 1, C)[0, 0].contiguous()
        return dy, db


class RowLNFn(torch.autograd.Function):
    """y = gamma * (x - mean_row) * rstd_row + beta over the width of each row (eps 1e-5).  Rows of up to 256 floats
    (the per-position LayerNorm over emb_dim in front of every BLSTM) take the one-pass kernels of norm.hip."""

    @staticmethod
    def forward(ctx, x, gamma, beta):
        _need_cuda(x, "TF-GridNet")
        x = x.contiguous()
        M, Wd = x.shape
        d = x.device
        st = _empty(d, M, 2)
        y = torch.empty_like(x)
        g, b = gamma.contiguous().view(-1), beta.contiguous().view(-1)
        ctx.short = dev.rowln_ok(Wd)
        if ctx.short:
            dev.rowln_fwd(x, g, b, M, Wd, y, st)
        else:
            dev.group_stats(x, _cln_geom(M, Wd), st, dev.LN_EPS)
            dev.dwconv_fwd(x, st, g, b, torch.ones(Wd, 1, device=d), torch.zeros(Wd, device=d), M, 1, Wd, 1, 1, 1, y)
        ctx.save_for_backward(x, st, g)
        ctx.shapes = (gamma.shape, beta.shape)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, st, g = ctx.saved_tensors
        M, Wd = x.shape
        if ctx.short:
            dy = dy.contiguous()
            dx = torch.empty_like(dy)
            tot = dev.rowln_bwd(x, dy, st, g, M, Wd, dx)
            return dx, tot[1].contiguous().view(ctx.shapes[0]), tot[0].contiguous().view(ctx.shapes[1])
        dx, dg, db = norm_backward(x, dy.contiguous().clone(), st, g, "cLN", M, 1, Wd)
        return dx, dg.view(ctx.shapes[0]), db.view(ctx.shapes[1])


class QKVHeadsFn(torch.autograd.Function):
    """The attention heads of a block from the ONE projection GEMM's output qkv [B*T*Q, nh*(2E + cp)] (columns: the Q
    heads, the K heads, the V heads): per projection PReLU(head slope) + LayerNorm over (Q, ch) with the head's affine,
    written head-major as [nh*B, T', Q*ch] (T' = T for the queries, Tp >= T with zero rows for keys / values) by one
    kernel each (dev.heads_fwd / heads_bwd, heads.hip; gridnet_block.py:176-199).  Parameters per projection:
    slope [nh], gamma / beta [nh, Q*ch] (index q*ch + e)."""

    @staticmethod
    def forward(ctx, qkv, geo, sq, gq, bq, sk, gk, bk, sv, gv, bv):
        _need_cuda(qkv, "TF-GridNet")
        B, T, Tp, Q, nh, E, cp = geo
        qkv = qkv.contiguous()
        ld, d = qkv.shape[1], qkv.device
        if ld != nh * (2 * E + cp) or qkv.shape[0] != B * T * Q:
            raise dev.L.WesepHipError(f"QKVHeadsFn: projection output {tuple(qkv.shape)} is not [{B * T * Q}, {nh * (2 * E + cp)}]")
        outs, keep, off = [], [], 0
        for s, g, b, ch, tp in ((sq, gq, bq, E, T), (sk, gk, bk, E, Tp), (sv, gv, bv, cp, Tp)):
            s, g, b = s.contiguous(), g.contiguous(), b.contiguous()
            y = _empty(d, nh * B, tp, Q * ch)
            st = _empty(d, nh, B * T, 2)
            dev.heads_fwd(qkv, ld, off, s, g, b, B, T, tp, Q, nh, ch, y, st)
            outs.append(y)
            keep += [s, g, st]
            off += nh * ch
        ctx.save_for_backward(qkv, *keep)
        ctx.geo = geo
        return tuple(outs)

    @staticmethod
    def backward(ctx, dq, dk, dv):
        qkv = ctx.saved_tensors[0]
        keep = ctx.saved_tensors[1:]
        B, T, Tp, Q, nh, E, cp = ctx.geo
        ld = qkv.shape[1]
        dqkv = torch.empty_like(qkv)                      # the three launches cover every column
        grads, off = [], 0
        for i, (dy, ch, tp) in enumerate(((dq, E, T), (dk, E, Tp), (dv, cp, Tp))):
            s, g, st = keep[3 * i:3 * i + 3]
            dg, db, ds = dev.heads_bwd(qkv, ld, off, dy.contiguous(), s, g, st, B, T, tp, Q, nh, ch, dqkv, ld, off)
            grads += [ds, dg, db]
            off += nh * ch
        return (dqkv, None) + tuple(grads)


class GroupLNFn(torch.autograd.Function):
    """nn.GroupNorm(1, C) on [B*P, C]: one mean/variance per batch row over (P, C), affine per channel."""

    @staticmethod
    def forward(ctx, x, gamma, beta, geo):
        _need_cuda(x, "TF-GridNet")
        B, P = geo
        x = x.contiguous()
        C = x.shape[1]
        d = x.device
        st = _empty(d, B, 2)
        dev.flat_stats(x, B, P * C, st, dev.LN_EPS)
        y = torch.empty_like(x)
        dev.dwconv_fwd(x, st, gamma.contiguous(), beta.contiguous(), torch.ones(C, 1, device=d),
                       torch.zeros(C, device=d), B, P, C, 1, 1, P, y)
        ctx.save_for_backward(x, st, gamma.contiguous())
        ctx.geo = (B, P, C)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, st, g = ctx.saved_tensors
        B, P, C = ctx.geo
        dx, dg, db = norm_backward(x, dy.contiguous().clone(), st, g, "gLN", B, P, C)
        return dx, dg, db, None


class PReluFn(torch.autograd.Function):
    """nn.PReLU with one slope a [1]."""

    @staticmethod
    def forward(ctx, x, a):
        x = x.contiguous()
        if x.numel() % 4:
            raise L.WesepHipError("PReLU: the element count must be a multiple of 4")
        y = torch.empty_like(x)
        dev.prelu_fwd(x.view(-1, 4), None, a, x.numel() // 4, 4, x.numel() // 4, y.view(-1, 4))   # elementwise: any 16-byte view
        ctx.save_for_backward(x, a)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, a = ctx.saved_tensors
        dx = torch.empty_like(x)
        da = dev.prelu_bwd(x.view(-1), dy.contiguous().view(-1), a, dx.view(-1))
        return dx, da.view(a.shape)


class SoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        x = x.contiguous()
        y = torch.empty_like(x)
        dev.softmax_rows_fwd(x, x.shape[0], x.shape[1], scale, y)
        ctx.save_for_backward(y)
        ctx.scale = scale
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dx = torch.empty_like(y)
        dev.softmax_rows_bwd(y, dy.contiguous(), y.shape[0], y.shape[1], ctx.scale, dx)
        return dx, None


class MatmulNTFn(torch.autograd.Function):
    """A [M, K] x B [N, K]^T -> [M, N] (both operands differentiable): the attention products."""

    @staticmethod
    def forward(ctx, A, B):
        A, B = A.contiguous(), B.contiguous()
        M, K = A.shape
        N = B.shape[0]
        ctx.save_for_backward(A, B)
        return _gemm(A, M, K, B, N)

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        dC = dC.contiguous()
        M, K = A.shape
        N = B.shape[0]
        dA = _gemm(dC, M, N, _transposed(B, N, K), K)
        if N % 4 == 0:
            dB, _ = _wgrad(dC, M, N, A, K, with_bias=False)                     # dC^T A
        else:                                                                  # (A^T dC)^T: the TN kernel wants Nn % 4 == 0
            dBt, _ = _wgrad(A, M, K, dC, N, with_bias=False, vec=0)
            dB = _transposed(dBt, K, N)
        return dA, dB


class BatchedMatmulNTFn(torch.autograd.Function):
    """A [G, M, K] x B [G, N, K]^T (+ bias [N]) -> C [G, M, N], both operands differentiable: ONE grouped launch over
    the G = heads x batch rows attention problems of a block (gridnet_block.py:176-206) instead of a host loop of G
    launches, forward and backward (ws_gemm_nt / ws_gemm_tn with per-group descriptors).  bias carries no gradient (it
    is the -inf mask of zero-padded key columns)."""

    @staticmethod
    def _nt(A, W, bias, G, M, K, N, w_kn=False):
        """C[g] = A[g] W'[g]^T, W'[n][k] = W[g][n][k] -- or, w_kn (ws_gemm_nt_args.vec bit 3, round 6), = W[g][k][n]: the
        operand as it lies in memory, where rounds 2-5 copied it into the other orientation first."""
        d = A.device
        C_ = _empty(d, G, M, N)
        tab = np.zeros(G, dtype=L.GROUP_NT_DTYPE)
        wp, bp = W.data_ptr(), (bias.data_ptr() if bias is not None else 0)
        for g in range(G):
            tab[g] = (wp + 4 * g * N * K, bp, 0, 0, g * M * K, g * M * N, 0, K, N, N if w_kn else K, 0)
        desc = L.upload_struct_array(tab, d)
        dev.gemm_nt(A=A, a_rows=flat(K), M=M, C_out=C_, c_rows=flat(N), groups=desc, ngroups=G, max_n=N,
                    vec=(3 if (K % 4 == 0 and (M * K) % 4 == 0) else 0) | (8 if w_kn else 0))
        return C_

    @staticmethod
    def nn_ok(K, N, M):
        """The transposed-W staging takes this product (16-byte pieces of A and of W's rows; the split-bf16 kernel)."""
        return (K % 4 == 0 and N % 4 == 0 and (M * K) % 4 == 0 and dev.gemm_mode() == "bf16x3"
                and os.environ.get("WESEP_GEMM_NN", "1") != "0")

    @staticmethod
    def forward(ctx, A, B, bias):
        _need_cuda(A, "TF-GridNet attention")
        A, B = A.contiguous(), B.contiguous()
        G, M, K = A.shape
        N = B.shape[1]
        ctx.save_for_backward(A, B)
        return BatchedMatmulNTFn._nt(A, B, bias, G, M, K, N)

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        dC = dC.contiguous()
        G, M, K = A.shape
        N = B.shape[1]
        d = A.device
        dA = dB = None
        if ctx.needs_input_grad[0]:
            if BatchedMatmulNTFn.nn_ok(N, K, M):                                # dA = dC B with B [N, K] as it lies
                dA = BatchedMatmulNTFn._nt(dC, B, None, G, M, N, K, w_kn=True)
            else:
                Bt = B.transpose(1, 2).contiguous()                             # [G, K, N]: W'[k][n] of dA = dC B
                dA = BatchedMatmulNTFn._nt(dC, Bt, None, G, M, N, K)
        if ctx.needs_input_grad[1]:
            # dB[g] = dC[g]^T A[g]: the TN kernel, one split (M rows), the slab IS the result
            dB = _empty(d, G, N, K)
            tab = np.zeros(G, dtype=L.GROUP_TN_DTYPE)
            for g in range(G):
                tab[g] = (0, 0, g * M * N, g * M * K, 0, g * N * K, 0, N, K, 0, 0)
            desc = L.upload_struct_array(tab, d)
            rps = -(-M // 32) * 32
            dev.gemm_tn(G=dC, g_rows=flat(N), A=A, a_rows=flat(K), M=M, slab=dB, slab_stride=G * N * K, nsplit=1,
                        rows_per_split=rps, groups=desc, ngroups=G, max_n=N, max_k=K,
                        vec=1 if (K % 4 == 0 and (M * K) % 4 == 0) else 0)
        return dA, dB, None


class BatchedMatmulNNFn(torch.autograd.Function):
    """A [G, M, K] x B [G, K, N] -> C [G, M, N], both operands differentiable: att x V of the attention (gridnet_block.py:203-206)
    with V as the head kernel wrote it -- ws_gemm_nt stages the transposed operand itself (vec bit 3).  Backward: dA = dC B^T is
    the NT product with B's rows as W' rows; dB = A^T dC is the TN kernel.  No operand is copied."""

    @staticmethod
    def forward(ctx, A, B):
        _need_cuda(A, "TF-GridNet attention")
        A, B = A.contiguous(), B.contiguous()
        G, M, K = A.shape
        N = B.shape[2]
        ctx.save_for_backward(A, B)
        return BatchedMatmulNTFn._nt(A, B, None, G, M, K, N, w_kn=True)

    @staticmethod
    def backward(ctx, dC):
        A, B = ctx.saved_tensors
        dC = dC.contiguous()
        G, M, K = A.shape
        N = B.shape[2]
        d = A.device
        dA = dB = None
        if ctx.needs_input_grad[0]:
            dA = BatchedMatmulNTFn._nt(dC, B, None, G, M, N, K)                 # W'[k][n] = B[k][n]: B's rows ARE the W' rows
        if ctx.needs_input_grad[1]:
            dB = _empty(d, G, K, N)                                             # dB[g] = A[g]^T dC[g]
            tab = np.zeros(G, dtype=L.GROUP_TN_DTYPE)
            for g in range(G):
                tab[g] = (0, 0, g * M * K, g * M * N, 0, g * K * N, 0, K, N, 0, 0)
            desc = L.upload_struct_array(tab, d)
            rps = -(-M // 32) * 32
            dev.gemm_tn(G=A, g_rows=flat(K), A=dC, a_rows=flat(N), M=M, slab=dB, slab_stride=G * K * N, nsplit=1,
                        rows_per_split=rps, groups=desc, ngroups=G, max_n=K, max_k=N,
                        vec=1 if (N % 4 == 0 and (M * N) % 4 == 0) else 0)
        return dA, dB


def blocked_path_ok(C, ks, hs):
    """The blocked-layout recurrence machinery shared with the pBSRNN path (blstm_core: plain -> BL input
    projection, 16-sequence / cluster / fused-projection recurrences, BL -> plain output projection with bias and
    residual, BL x BL weight gradients) is built for 128 input features and one position per step -- which is the
    shipped TF-GridNet recipe (emb_dim 128, emb_ks = emb_hs = 1; tfgridnet.yaml).  Default for that geometry since its
    first hardware run (round 2: every stage within 1e-5 of an fp64 statement, tools/diag_tfgrid_blk.py);
    WESEP_TFGRID_BLOCKED=0 selects the row-major path."""
    return os.environ.get("WESEP_TFGRID_BLOCKED", "1") != "0" and C == 128 and ks == 1 and hs == 1


class BlstmLinearBlkFn(torch.autograd.Function):
    """y [nseq*Lr, 128] (layer-normed), res [nseq*Lr, 128] -> res + Linear(BLSTM(y)) on the blocked layout.

    gridnet_block.py:139-160 for emb_ks = emb_hs = 1.  The BLSTM + projection are blstm_core's steps, the ones
    functional.ResRNNBlkFn runs, without a GroupNorm (the LayerNorm over C happens before, per row); this node owns the
    sequence map and its padding.  Sequences are the contiguous runs of Lr rows; when the cluster recurrence applies apart
    from the sequence count (long sequences, few of them: the inter-frame path), the sequences are zero-padded to a
    multiple of 64 -- padded sequences cost no latency and their rows are dropped.  Weights: pad_lstm / pad_hidden_cols
    outputs (hidden zero-padded to 256).

    geo = (nseq, Lr): sequences are contiguous runs of Lr rows; geo = (nseq, Lr, div, s1, s2, step_rows): a STRIDED
    sequence map over the rows of y / res (sequence s, step t -> row (s // div) * s1 + (s % div) * s2 + t * step_rows) --
    the inter-frame path run in place on the [B, T, Q, C] map (round 4; the runtime's plan has done so since round 3): no
    transposed copy of the map before and after the BLSTM, forward or backward; the padding to a multiple of 64 is then
    the map's `nvalid` (wesep_hip.h ws_seqmap), not appended rows."""

    @staticmethod
    def forward(ctx, y, res, geo, dummy, box, wih_f, wih_r, b_f, b_r, whf, whr, lin_w, lin_b):
        """dummy / box: None, or the output and the box of this BLSTM's functional.WGradCarrierFn (created over the eight
        weight tensors, in this order, before the first block of the step) -- then the weight gradients are computed on the
        side stream, released under the NEXT inter-frame BPTT (a latency-bound launch on a quarter of the CUs), and reach
        autograd through the carrier; this node returns None for them (round 4: the twelve BLSTMs' weight-gradient GEMMs,
        48 ms of a 336 ms step, ran in line on the main stream before)."""
        _need_cuda(y, "TF-GridNet")
        nseq, Lr = geo[:2]
        strided = geo[2:] if len(geo) > 2 else None
        d = y.device
        pad = 0
        if Lr >= 64 and nseq % 64 and (-(-nseq // 64) * 64 // 32) * 8 <= dev.cu_count(d):
            pad = -(-nseq // 64) * 64 - nseq
        ns = nseq + pad
        if pad and strided is None:
            z = torch.zeros(pad * Lr, 128, device=d, dtype=torch.float32)
            y, res = torch.cat([y, z], 0), torch.cat([res, z], 0)
        y, res = y.contiguous(), res.contiguous()
        seq = SeqMap(ns, BIG, 0, Lr, 1, Lr) if strided is None else SeqMap(ns, *strided, Lr, nvalid=nseq)
        plan = make_plan(seq, d, any(ctx.needs_input_grad))
        # the weights are fresh autograd outputs of pad_lstm every step: a memo for this forward / backward pair, not a
        # module-owned cache (across calls a key on data_ptr could hit a recycled address).  b_ih = the summed bias, b_hh = 0
        zero = torch.zeros(G4P, device=d, dtype=torch.float32)
        cache = PackCache()
        sig = cache.begin((wih_f, whf, b_f, wih_r, whr, b_r, lin_w))
        W = WeightPacks(cache, sig, plan.lmode, plan.pair_rfmt, wih_f, whf, b_f.contiguous(), zero, wih_r, whr,
                          b_r.contiguous(), zero, lin_w)
        out, saved = blstm_forward(plan, W, y, seq, res=res, bias=lin_b.contiguous())
        ctx.save_for_backward(*saved)
        ctx.geo, ctx.seq, ctx.plan, ctx.packs, ctx.box = (nseq, Lr, ns), seq, plan, W, box
        ctx.consumed = False
        return out[:nseq * Lr] if (pad and strided is None) else out

    @staticmethod
    def backward(ctx, dout):
        consume_once(ctx, "TF-GridNet BLSTM")
        gates, cbuf, hcat, xn, hcat16 = ctx.saved_tensors     # (xn: its fp16 copy if hcat16)
        nseq, Lr, ns = ctx.geo
        seq, plan, W, box = ctx.seq, ctx.plan, ctx.packs, ctx.box
        d = dout.device
        dout = dout.contiguous()
        dres = dout
        appended = ns != nseq and not seq.nvalid      # contiguous runs: the padding sequences are rows behind the data
        if appended:
            dout = torch.cat([dout, torch.zeros((ns - nseq) * Lr, 128, device=d, dtype=torch.float32)], 0)
        # the inter-frame BPTT (few long sequences: pair / cluster kernels on a fraction of the CUs for ~10 ms) is where the
        # weight-gradient jobs deferred by the BLSTMs before it are released
        dg, dout_bl, amax, dxn2 = blstm_bptt(plan, W, gates, cbuf, hcat, dout, seq, release=plan.bptt in ("pair", "cluster"))
        # weight_grads' list -> this node's weight arguments (wih_f, wih_r, b_f, b_r, whf, whr, lin_w, lin_b)
        wg = blstm_weight_grads(plan, dg, xn, hcat, dout_bl, amax, hcat16, seq, box, order=(0, 4, 2, 6, 1, 5, 8, 9))
        del dout_bl
        dy, _ = blstm_dxn(plan, W, dg, amax, dxn2, seq, (ns if appended else nseq) * Lr)
        if appended:
            dy = dy[:nseq * Lr]
        gd = torch.zeros((), device=d) if box is not None else None     # keeps the carrier node in the graph walk
        return (dy, dres, None, gd, None) + tuple(wg)
