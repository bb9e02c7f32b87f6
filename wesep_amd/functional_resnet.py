"""Autograd shims of the wespeaker ResNet speaker encoder over the C ABI.

Channels-last activations [R*H*W, C] (H = mel bin, W = frame).  conv2d = im2col + one split-bf16 MFMA GEMM
(K = k*k*Cin); BatchNorm2d / ReLU / residual are the channels-last BatchNorm kernels of tasnet.hip (a ReLU is a
PReLU of slope 0, "no activation" one of slope 1); the input gradient is GEMM + col2im (gather), the weight
gradient the TN GEMM on the recomputed patch matrix (patches are never kept for the backward)."""
import torch

from . import _lib as L
from . import dev
from . import functional_conv as FC
from .functional import _empty, _need_cuda
from .functional_tasnet import _gemm, _transposed, _wgrad


class ConvBnActFn(torch.autograd.Function):
    """x [R*H*W, Cin] -> act(BN(conv2d(x, w)) (+ res)) [R*Ho*Wo, Cout]; act = ReLU or identity.  `stride` of geo: an int,
    or (sh, sw) for the mel-axis-only strides of CAM++'s FCM head (implicit-patch path, Cin % 4 == 0).  A seventh entry of
    geo (inference only): the int32 device table of the rows' valid OUTPUT widths -- the masked epilogue writes zeros behind
    them (ragged batches)."""

    @staticmethod
    def forward(ctx, x, res, geo, w, gamma, beta, rm, rv):
        _need_cuda(x, "ResNet speaker encoder")
        R, H, W, stride, relu, training = geo[:6]
        wlen = geo[6] if len(geo) > 6 else None
        Cout, Cin, k, _ = w.shape
        pad = k // 2
        sh, sw = stride if isinstance(stride, tuple) else (stride, stride)
        if sh != sw and not (FC.implicit_ok(Cin) and FC.implicit_ok(Cout) and max(sh, sw) <= 2):
            raise L.WesepHipError("ConvBnActFn: unequal strides need channel counts that are multiples of 4, strides <= 2")
        Ho, Wo = dev.conv_out(H, k, sh, pad), dev.conv_out(W, k, sw, pad)
        M = R * Ho * Wo
        x = x.contiguous()
        d = x.device
        Kk = k * k * Cin
        ldp = -(-Kk // 4) * 4                                   # first layer: 9 taps padded to 12 columns
        W2 = torch.zeros(Cout, ldp, device=d, dtype=torch.float32)
        W2[:, :Kk] = w.permute(0, 2, 3, 1).reshape(Cout, Kk)     # column (ky*k + kx)*Cin + c, like the patches
        if FC.implicit_ok(Cin):
            # the patch matrix stays implicit in the GEMM's operand loader (functional_conv): nothing is unfolded
            c = FC.conv2d_fwd(x, R, H, W, Cin, W2, Cout, k, sh, sw, pad)
        else:                                                   # single-channel first layer: 12-column patch rows
            patches = ConvBnActFn._patches(x, R, H, W, Cin, k, sh, pad, M, ldp)
            c = _gemm(patches, M, ldp, W2, Cout)
            del patches
        st = _empty(d, 2, Cout)
        if training:
            dev.bn_stats(c, M, Cout, rm, rv, st)
        else:
            st[0].copy_(rm)
            st[1].copy_(torch.rsqrt(rv + dev.BN_EPS))
        slope = torch.full((1,), 0.0 if relu else 1.0, device=d, dtype=torch.float32)
        u, y = _empty(d, M, Cout), _empty(d, M, Cout)
        res = res.contiguous() if res is not None else None
        if wlen is not None:
            dev.bn_prelu_fwd_len(c, st, gamma, beta, res, slope, M, Cout, Ho * Wo, Wo, wlen, u, y)
        else:
            dev.bn_prelu_fwd(c, st, gamma, beta, res, slope, M, Cout, u, y)
        ctx.save_for_backward(x, c, st, u, W2, gamma, slope)
        ctx.geo = (R, H, W, Cin, Cout, k, (sh, sw), pad, Ho, Wo, ldp, res is not None, training, w.shape)
        return y

    @staticmethod
    def _patches(x, R, H, W, Cin, k, stride, pad, M, ldp):
        if ldp != k * k * Cin:
            patches = torch.zeros(M, ldp, device=x.device, dtype=torch.float32)
        else:
            patches = _empty(x.device, M, ldp)
        dev.im2col(x, R, H, W, Cin, k, stride, pad, patches, ldp)
        return patches

    @staticmethod
    def backward(ctx, dy):
        x, c, st, u, W2, gamma, slope = ctx.saved_tensors
        R, H, W, Cin, Cout, k, (sh, sw), pad, Ho, Wo, ldp, has_res, training, wshape = ctx.geo
        stride = sh
        M = R * Ho * Wo
        d = x.device
        du = dy.contiguous().clone()
        dev.prelu_bwd(u, du, slope, du)                          # ReLU' (slope 0) or identity (slope 1), in place
        dres = du if has_res else None
        dc = _empty(d, M, Cout)
        sums = dev.bn_bwd_any(c, du, st, gamma, M, Cout, dc, training)
        Kk = k * k * Cin
        if FC.implicit_ok(Cin):
            dW2, _ = FC.conv2d_wgrad(dc, x, R, H, W, Cin, Cout, k, sh, sw, pad, with_bias=False)
        else:
            patches = ConvBnActFn._patches(x, R, H, W, Cin, k, stride, pad, M, ldp)
            dW2, _ = _wgrad(dc, M, Cout, patches, ldp, with_bias=False)
            del patches
        dw = dW2[:, :Kk].reshape(Cout, k, k, Cin).permute(0, 3, 1, 2).contiguous()
        dx = None
        if ctx.needs_input_grad[0]:
            if FC.implicit_ok(Cin) and FC.implicit_ok(Cout) and max(sh, sw) <= 2:
                # transposed view of dc, one row per input pixel: Wd[ci][(tap)*Cout + co] = w[co, ci, ky, kx]
                Wd = W2.view(Cout, k * k, Cin).permute(2, 1, 0).reshape(Cin, k * k * Cout).contiguous()
                dx = FC.conv2d_dx(dc, R, H, W, Cin, Wd, Cout, k, sh, sw, pad)
            else:
                dpatches = _gemm(dc, M, Cout, _transposed(W2, Cout, ldp), ldp)
                dx = _empty(d, R * H * W, Cin)
                dev.col2im(dpatches, R, H, W, Cin, k, stride, pad, dx)
        return dx, dres, None, dw.view(wshape), sums[1].contiguous(), sums[0].contiguous(), None, None


class TstpFn(torch.autograd.Function):
    """x [R*F*T, C] -> [R, 2*C*F]: mean || sqrt(unbiased var + 1e-7) over T, feature index c*F + f.  A fourth entry of
    geo (inference only): the int32 device table of the rows' valid frames."""

    @staticmethod
    def forward(ctx, x, geo):
        R, Fq, T = geo[:3]
        tlen = geo[3] if len(geo) > 3 else None
        x = x.contiguous()
        Cc = x.shape[1]
        stats = _empty(x.device, R, 2 * Cc * Fq)
        if tlen is not None:
            dev.tstp_fwd_len(x, R, Fq, T, Cc, tlen, stats)
        else:
            dev.tstp_fwd(x, R, Fq, T, Cc, stats)
        ctx.save_for_backward(x, stats)
        ctx.geo = (R, Fq, T, Cc)
        return stats

    @staticmethod
    def backward(ctx, dstats):
        x, stats = ctx.saved_tensors
        R, Fq, T, Cc = ctx.geo
        dx = torch.empty_like(x)
        dev.tstp_bwd(x, stats, dstats.contiguous(), R, Fq, T, Cc, dx)
        return dx, None


class MhastpFn(torch.autograd.Function):
    """MHASTP / MQMHASTP pooling (models/resnet.py) of x [R*F*T, C] -> [R, Q*H*2*dm]: per query and head, mean || std
    under the head's attention (csrc/mhastp.hip).  geo = (R, F, T, Q, H, layers, ds[, split]) -- split True: the grid
    split over T (ws_mhastp_fwd_split / _bwd_split; the 1-D encoders); params = per query, per head:
    att_0.weight, att_0.bias (, att_1.weight, att_1.bias); cache: the pooling module's PackCache, which keeps the weight
    pack (W1's columns in the kernel order) for one weight version."""

    @staticmethod
    def forward(ctx, x, geo, cache, *params):
        _need_cuda(x, "MHASTP pooling")
        R, Fq, T, Q, Hh, layers, ds = geo[:7]
        split = len(geo) > 7 and bool(geo[7])
        x = x.contiguous()
        Cc = x.shape[1]
        Ch = Cc // Hh
        dm = Ch * Fq
        P1 = dev.mhastp_block_floats(layers, ds, dm)
        sig = cache.begin(params)
        pack = cache.get(sig, "mhastp", lambda: _mhastp_pack(params, Q * Hh, layers, ds, Fq, Ch, P1, x.device))
        out = _empty(x.device, R, Q * Hh * 2 * dm)
        aux = _empty(x.device, R * Q * Hh * 4, dm)
        if split:
            dev.mhastp_fwd_split(x, pack, R, Fq, T, Cc, Q, Hh, layers, ds, out, aux)
        else:
            dev.mhastp_fwd(x, pack, R, Fq, T, Cc, Q, Hh, layers, ds, out, aux)
        ctx.save_for_backward(x, pack, aux)
        ctx.geo = (R, Fq, T, Cc, Q, Hh, layers, ds, Ch, dm, P1)
        ctx.split = split
        return out

    @staticmethod
    def backward(ctx, dout):
        x, pack, aux = ctx.saved_tensors
        R, Fq, T, Cc, Q, Hh, layers, ds, Ch, dm, P1 = ctx.geo
        wgrad = any(ctx.needs_input_grad[3:])
        dx = torch.empty_like(x)
        dpack = torch.empty(Q * Hh * P1, device=x.device, dtype=torch.float32) if wgrad else None
        bwd = dev.mhastp_bwd_split if ctx.split else dev.mhastp_bwd
        bwd(x, pack, aux, dout.contiguous(), R, Fq, T, Cc, Q, Hh, layers, ds, dx, dpack)
        if not wgrad:
            return (dx, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)
        n1 = 64 if layers == 2 else ds
        grads = []
        for qh in range(Q * Hh):
            blk = dpack[qh * P1:(qh + 1) * P1]
            grads.append(blk[:n1 * dm].view(n1, dm, 1))          # views of dpack: no copies
            grads.append(blk[n1 * dm:n1 * dm + n1])
            if layers == 2:
                off2 = n1 * dm + n1
                grads.append(blk[off2:off2 + 64 * ds].view(ds, 64, 1))
                grads.append(blk[off2 + 64 * ds:])
        return (dx, None, None) + tuple(grads)


def _mhastp_pack(params, nqh, layers, ds, Fq, Ch, P1, device):
    pack = torch.empty(nqh * P1, device=device, dtype=torch.float32)
    per = len(params) // nqh
    for qh in range(nqh):
        p = [t.detach().contiguous() for t in params[qh * per:(qh + 1) * per]]
        w2, b2 = (p[2], p[3]) if layers == 2 else (None, None)
        dev.mhastp_pack(p[0], p[1], w2, b2, Fq, Ch, layers, ds, pack[qh * P1:(qh + 1) * P1])
    return pack
