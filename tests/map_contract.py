"""TEST INFRASTRUCTURE ONLY -- contract suite of the feature-map kernels of wesep_amd/csrc/conv2d.hip: ws_im2col_hw /
ws_col2im_hw (and the square wrappers), ws_elu_fwd / bwd, ws_inorm_finalize / apply / bwd_apply, ws_in_act_sums / apply /
bwd_apply, ws_avgpool_fwd / bwd, ws_bilinear_fwd / bwd, ws_scale_bf_fwd / bwd, ws_freq_linear_fwd, ws_softmax_rows_fwd / bwd,
ws_rowbias_act_fwd and ws_act_bwd.  Same shape as tests/norm_contract.py and tests/stft_contract.py: Ref, check, eps_for, the
guards and the pairwise generator with its registries come from tests/gemm_contract.py, Partial / check_partial / sum32 from
tests/norm_contract.py.  No GPU code here: test_map_contract_host_cpu.py checks this module, test_map_contract_gpu.py runs
every case through wesep_amd.dev.  Out of scope: TSTP, ASTP, seg_sums / seg_scale, pre-emphasis, power spectrum and log of
the same file (under contract in tests/pool_contract.py) and the modes of ws_chan_sums dev.inorm_fwd / bwd do not use:
all three modes of ws_chan_sums, with every split count, are under contract in tests/tasnet_contract.py.

1. REFERENCE.  compute(entry, spec, tensors, dtype) restates include/wesep_hip.h as explicit index arithmetic (gathers over
   index tensors; no F.unfold / F.fold / F.interpolate / F.avg_pool2d / torch.softmax: those are the host test's second
   opinion at 1e-12).  Run in float64 it is the reference, run in float32 (sums sequential or pairwise) the emulation of a
   correct kernel, run with `defect` a planted defect.  Channels-last maps [B][H][W][C]:
     im2col   patches[m][(ky k + kx) C + c] = x[r][ho sh + ky - p][wo sw + kx - p][c], 0 outside the image,
              m = (r Ho + ho) Wo + wo, Ho = (H + 2p - k) / sh + 1; C == 1: row stride ldp >= k k, columns [k k, ldp) NOT written
     col2im   dx[r][hi][wi][c] = sum of dpatches[m(ho, wo)][(ky k + kx) C + c] over the taps with ho sh + ky - p == hi,
              wo sw + kx - p == wi, ho < Ho, wo < Wo; a pixel no patch covers (stride above k, the ragged tail) is exactly 0
     elu      y = x > 0 ? x : expm1(x);  dx = dy (x > 0 ? 1 : exp(x))
     inorm    stats = (mean, 1 / sqrt(max(E[u^2] - mean^2, 0) + eps)) from sums = (sum u, sum u^2) over P positions;
              y = (x - mean) rstd;  dx = rstd (dy - S0 / P - y S1 / P)
     in_act   u = flags & 1 ? ELU(x) : x;  n = (u - mean) rstd;  y = flags & 2 ? ELU(n) : n;  d = dy (flags & 2 ? ELU'(n) : 1);
              slab[s][g] = sums over rows [s per, min(P, (s + 1) per)), per = ceil(P / nsplit), of (u, u^2) or (d, d n);
              dx = (flags & 1 ? ELU'(x) : 1) rstd (d - S0 / P - n S1 / P)
     avgpool  y = mean of the sz x sz window (stride sz, floor);  dx = dy / sz^2, exactly 0 on the rows / columns the floor drops
     bilinear src = max((dst + 1/2) h / H - 1/2, 0), i0 = floor(src), i1 = min(i0 + 1, h - 1), l = src - i0 per axis; the
              adjoint is the transposed weights.  The reference takes src as the EXACT rational ((2 dst + 1) h - H) / (2 H).
     scale_bf y = x s[b][f] (mode 0) or x + s[b][f];  dx = dy s or dy;  ds[b][f] = sum over (t, c) of dy x or dy
     freq_lin y[b][t][f'][c] = sum_f W[f' ldw + f] x[b][t][f][c] + rb[b][f']
     softmax  y = exp(scale x - max) / sum;  dx = scale y (dy - sum dy y)
     rowbias  y = act(x + rb[row / rows_per_r][c]) (1 tanh, 3 sigmoid);  act_bwd dx = dy (1 - y^2) or dy y (1 - y)
   Backward entries TAKE their forward quantities: stats, sums and y are uploaded as the fp32 rounding of the float64 values
   and the reference computes from exactly those fp32 numbers, so every entry is judged on its own.  The composed chains
   (test_map_contract_gpu.py) feed each stage the device output of the one before and evaluate the reference there.

2. BOUNDS.  Per element, derived; u = 2^-24, e(n) = eps_for(False, n) = (n + 8) u applied to the same expression over
   absolute values (S).  The build has no fast-math flag (wesep_amd/build.py), so +, *, /, sqrtf round correctly.
     im2col              bit-exact (a copy); padding taps are exact zeros
     col2im              e(n) S, n = ceil(k / sh) ceil(k / sw) >= the addends of a pixel; pixels with at most one addend bit-exact
     avgpool_fwd         e(sz^2 + 1) S (the window sum and the product with fl(1 / sz^2))
     avgpool_bwd         2 u |dy| / sz^2 (fl(1 / sz^2) and one product); the dropped tail exactly 0
     library functions   ULP_EXP = 3 (expf, as tests/stft_contract.py), ULP_EXPM1 = 3, ULP_TANH = 5: the OpenCL full-profile
                         requirement the device library implements.  No header or document under the ROCm installation
                         states other figures (the device library ships as bitcode only), so these stand; one ulp is at
                         most 2 u relative: D_EXP = D_EXPM1 = 6 u, D_TANH = 10 u, D_SIG = 8 u (stft_contract).
     elu_fwd / bwd       x > 0: bit-exact; else D_EXPM1 |y|, (D_EXP + u) |dx| + 2^-125 (expf may underflow to a flushed denormal)
     rowbias_act         dv = u |x + rb|; tanh (Lipschitz 1): dv + D_TANH |y|; sigmoid (Lipschitz 1/4): dv / 4 + D_SIG |y|
     act_bwd             e(0) |dy| (y^2 + |1 - y^2|), e(0) |dy| |y| (|y| + |1 - y|): three roundings
     rstd                an INTERVAL, the one-pass form.  mean is off by d_m, E[u^2] by e(n) E|u^2|, mean^2 by 2 |mean| d_m + d_m^2
                         (+ its rounding, inside e(n) mean^2):  d_v = e(n) (E|u^2| + mean^2) + 2 |mean| d_m + d_m^2.  The
                         kernel's rstd lies in [(1 - 4u) / sqrt(var + d_v + eps), (1 + 4u) / sqrt(max(var - d_v, 0) + eps)]:
                         where the interval reaches 0 it is clamped as the kernel's fmaxf clamps.  ws_inorm_finalize alone takes
                         GIVEN sums: n = 0, d_m = e(0) |mean| (fl(1 / P) and the product); the chain dev.inorm_fwd /
                         dev.in_act_fwd has n = P and d_m = e(P) E|u| (+ D_EXPM1 E|u| with flags & 1).  Ref carries val = the
                         midpoint, bound = the half width, S = the exact rstd.
     inorm_apply         e(0) |x - mean| rstd from given stats; the chain adds d_m rstd_hi + |x - mean| d_r (d_r: the larger
                         distance of rstd from the ends of its interval)
     inorm_bwd_apply     e(0) S, S = |rstd| (|dy| + |S0 / P| + |y S1 / P|)
     in_act              du = D_EXPM1 |u| (flags & 1, x <= 0), dn = du |rstd| + 2 u |n|, ELU and ELU' are Lipschitz 1 and
                         continuous, so a kernel on the other side of the x > 0 test stays inside:
                         y: dn + D_EXPM1 |y| (flags & 2) or dn;  de = dn + D_EXP ELU'(n);  dd = |dy| (de + u ELU'(n))
                         sums fwd: (e(P) + D_EXPM1) S0, (e(P) + 2 D_EXPM1 + u) S1;  bwd: e(P) sum|d| + sum dd,
                         e(P) sum|d n| + sum(dd |n| + |d| dn + u |d n|)
                         dx: (|rstd| (dd + |S1 / P| dn) + e(0) |rstd| (|d| + |S0 / P| + |n S1 / P|)) ELU'(x) + (D_EXP + u) |dx|
     bilinear_fwd        bl_src takes three roundings: fl(h / H), the product, the subtraction: the fp32 coordinate is off by at
                         most d_l = 3 u (src + 1).  l = s - i0 is exact (Sterbenz).  A weight error d moves d from one tap of
                         an axis to the other: d_l |v(i1) - v(i0)| per axis (interpolated over the other axis), on top of
                         e(8) S.  WHERE fp32 AND EXACT ARITHMETIC FLOOR TO DIFFERENT i0 (src within d_l of an integer r) the
                         kernel evaluates the neighbouring cell at its end: the interpolant is continuous and piecewise
                         linear, so it is off by at most (distance inside the own cell) * |own slope| + (distance inside the
                         neighbour) * |neighbour's slope| with the two distances summing to at most d_l; the reference adds
                         the neighbouring cell's slope for exactly those destinations.  The host test confirms it with the
                         fp32 emulation of bl_src on every case.
     bilinear_bwd        the same weight error d_l(X) on both taps (and the neighbouring cell's, as above) of every destination
                         in the support, at most 2 / scale + 3 taps per pass: pass 1 |dy| DW + e(taps) |dy| W, pass 2 the same
                         over tmp plus the propagated error of tmp
     scale_bf_fwd / dx   e(0) |y|; mode 1 dx bit-exact;  ds: e(T C) S
     freq_linear         e(F + 1) (sum |W x| + |rb|)
     softmax_fwd         max-subtracted.  t = scale x (u |t|), z = t - max (dz = u (|t| + |max| + |z|)), rho = D_EXP + expm1(dz);
                         y_j (rho_j + sum_k y_k rho_k + e(n) + 2 u) + 2^-125: the absolute floor covers expf underflowing to 0
                         (or a flushed denormal) where float64 does not, against a sum of at least 1
     softmax_bwd         |scale y| e(n) sum|dy y| + e(0) |scale y| (|dy| + |sum dy y|) + 2^-125 (1 + |scale| (|dy| + |sum dy y|)):
                         the floor covers a denormal y (flushed or not) and a denormal product
   Slabs (in_act_sums) are judged as sums over the splits (norm_contract.Partial): every slab element is written, splits
   that own no row are exact zeros.

3. CONDITION OF THE SUITE.  Such bounds see a dropped or misplaced element only while it weighs enough in its sum: a dropped
   element x shifts a sum by |x| ~ 1 while the bound is e(n) S ~ (n + 8) 2^-24 * 0.8 n.  Gauss and offset data stay at sums of
   at most CAP = 2048 leaves (bound about 0.2): test_map_contract_host_cpu.py confirms on the CPU that every planted defect
   below is refused by the reference alone at these sizes.  Larger sums exist only to cross a loop seam (scale_bf with
   T C > CAP) and carry a structural spike: the last element x1e3.

4. CASES.  cases(entry): gemm_contract's pairwise generator over the *_DIMS tables, topped up so that every dispatch target
   of INST gets MIN_PER_TARGET cases, plus the hand-written seam cases of EXTRA (avgpool sz = 32 on a 32 x 33 map).  The
   grid-stride seam (n = 4 (65536 * 256 + 3) floats through ws_elu_fwd) is a test of its own in test_map_contract_gpu.py.

BUFFERS.  GUARD floats on both sides of every operand and output.  Outputs: the write set starts as NaN (dx aliasing dy: as
that operand), everything else holds SENT and must be bit-identical afterwards -- ldp padding, the columns outside
[off, off + C) of a strided output, guards.  Inputs: everything the contract does not read is NaN (columns outside a strided
dy, W beyond column F, guards); build(case, garbage=True) puts a large finite value there.  Every f32x4 entry keeps every
pointer and row stride 16-byte aligned; only the softmax cases start one float into their allocation, which selects the scalar
kernels; no misaligned pointer goes to an entry that cannot take one."""
import math

import numpy as np
import torch

from tests import gemm_contract as gc
from tests import norm_contract as nc
from tests.gemm_contract import (GUARD, SENT, U, Buf, Built, Case, ContractViolation, Ref, check, eps_for)  # noqa: F401
from tests.norm_contract import Partial, check_partial, sum32  # noqa: F401

GARBAGE = 3.0e30
NAN = float("nan")
IN_EPS = 1e-5
CAP = 2048
F64 = torch.float64
F32 = torch.float32
ULP_EXP, ULP_EXPM1, ULP_TANH = 3, 3, 5
D_EXP, D_EXPM1, D_TANH = 2 * ULP_EXP * U, 2 * ULP_EXPM1 * U, 2 * ULP_TANH * U
D_SIG = (2 * ULP_EXP + 2) * U
TINY = 2.0 ** -125
IMG = gc.IMG
ENTRIES = ("im2col", "col2im", "elu_fwd", "elu_bwd", "inorm_finalize", "inorm_apply", "inorm_bwd_apply", "in_act_sums",
           "in_act_apply", "in_act_bwd_apply", "avgpool_fwd", "avgpool_bwd", "bilinear_fwd", "bilinear_bwd", "scale_bf_fwd",
           "scale_bf_bwd", "freq_linear", "softmax_fwd", "softmax_bwd", "rowbias_act", "act_bwd")
ORDERS = ("seq", "pairwise")


# ------------------------------------------------------------------------------------------------------------
# small helpers
# ------------------------------------------------------------------------------------------------------------
def _sum(v, order):
    """Sum over the last axis: float64 exactly as torch sums, float32 in `order`."""
    return v.sum(-1) if v.dtype == F64 else sum32(v, order)


def _elu(v):
    return torch.where(v > 0, v, torch.expm1(v))


def _elud(v):
    return torch.where(v > 0, torch.ones_like(v), torch.exp(v))


def _ar(n):
    return torch.arange(n)


def _ref(idx, val, S, bound, exact=None):
    idx = idx.reshape(-1)
    ex = torch.zeros(idx.numel(), dtype=torch.bool) if exact is None else exact.reshape(-1)
    return Ref(idx, val.reshape(-1).double(), S.reshape(-1).double(), bound.reshape(-1).double(), ex)


def conv_geom(sp, defect=None):
    H, W, k, sh, sw, p = sp["H"], sp["W"], sp["k"], sp["sh"], sp["sw"], sp["p"]
    return (H + 2 * p - k) // sh + 1, (W + 2 * p - k) // sw + 1


def _patch_src(sp, defect=None):
    """(src [M, kk] pixel index r*H*W + hi*W + wi, ok [M, kk]) of every patch row and tap."""
    R, H, W, k, sh, sw, p = sp["R"], sp["H"], sp["W"], sp["k"], sp["sh"], sp["sw"], sp["p"]
    Ho, Wo = conv_geom(sp)
    m = _ar(R * Ho * Wo)
    r, ho, wo = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    tap = _ar(k * k)
    ky, kx = tap // k, tap % k
    if defect == "taps_transposed":
        ky, kx = kx, ky
    if defect == "stride_swapped":
        sh, sw = sw, sh
    if defect == "pad_off_by_one":
        p = p + 1
    hi = ho[:, None] * sh + ky[None, :] - p
    wi = wo[:, None] * sw + kx[None, :] - p
    ok = (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
    return (r[:, None] * H + hi.clamp(0, H - 1)) * W + wi.clamp(0, W - 1), ok


def bl_axis(n, N, defect=None):
    """One axis of the bilinear map n -> N in exact arithmetic: (Wm [N, n] weights, DW [N, n] the weight error d_l on every tap
    the fp32 kernel may touch, SW list of [N, n] signed tap differences (own cell, neighbouring cells where the floor may
    differ), d_l [N])."""
    X = _ar(N)
    if defect == "align_corners":
        num, den = X * (n - 1), max(N - 1, 1)
    else:
        num, den = (2 * X + 1) * n - N, 2 * N
    if defect != "no_clamp":
        num = num.clamp_min(0)
    i0 = torch.div(num, den, rounding_mode="trunc").clamp_max(n - 1)
    i1 = (i0 + 1).clamp_max(n - 1)
    l = (num - i0 * den).double() / den
    src = num.double() / den
    Wm = torch.zeros(N, n, dtype=F64)
    Wm[X, i0] += 1 - l
    Wm[X, i1] += l
    d_l = 3 * U * (src.abs() + 1) * (1 + 8 * U)
    own = torch.zeros(N, n, dtype=F64)
    own[X, i1] += 1
    own[X, i0] -= 1
    SW, DW = [own], torch.zeros(N, n, dtype=F64)
    # a coordinate clamped by more than d_l (below 0, above n - 1) is clamped in fp32 as well: its weights are exactly 1 and 0
    raw = ((2 * X + 1) * n - N).double() / (2 * N)
    free = d_l * ((raw >= -d_l) & (raw <= n - 1 + d_l))
    DW[X, i0] = free
    DW[X, i1] = free
    fl = torch.div(num, den, rounding_mode="floor")
    below = ((src - fl) <= d_l) & (fl >= 1) & (fl <= n - 1)          # fp32 may floor to fl - 1: the cell [fl - 1, fl]
    above = ((fl + 1 - src) <= d_l) & (fl + 2 <= n - 1) & (fl >= 0)   # fp32 may floor to fl + 1: the cell [fl + 1, fl + 2]
    for mask, a in ((below, -1), (above, 1)):
        if bool(mask.any()):
            alt = torch.zeros(N, n, dtype=F64)
            xs = X[mask]
            alt[xs, fl[mask] + a + 1] += 1
            alt[xs, fl[mask] + a] -= 1
            SW.append(alt)
            DW[xs, fl[mask] + a] = torch.maximum(DW[xs, fl[mask] + a], d_l[mask])
            DW[xs, fl[mask] + a + 1] = torch.maximum(DW[xs, fl[mask] + a + 1], d_l[mask])
    return Wm, DW, SW, d_l


def bl_axis32(n, N, defect=None):
    """bl_src / bl_window of conv2d.hip in fp32: (i0, i1, l) per destination and the [lo, hi] gather window per source."""
    f = np.float32
    sc = f(n) / f(N)
    X = np.arange(N)
    s = (X.astype(f) + f(0.5)) * sc - f(0.5)
    if defect == "align_corners":
        s = X.astype(f) * (f(n - 1) / f(max(N - 1, 1)))
    if defect != "no_clamp":
        s = np.maximum(s, f(0))
    i0 = np.minimum(s.astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l = (s - i0.astype(f)).astype(f)
    sidx = np.arange(n).astype(f)
    lo = np.floor((sidx - f(0.5)) / sc - f(0.5)).astype(np.int64) - 1
    hi = np.ceil((sidx + f(1.5)) / sc - f(0.5)).astype(np.int64) + 1
    if defect == "window_narrow":
        lo = lo + 3          # one tap inside the tight window [floor + 1, ceil - 1]
    return i0, i1, l, np.maximum(lo, 0), np.minimum(hi, N - 1)


def _bl_w32(n, N, defect):
    """[N, n] fp32 weights as the adjoint kernels see them (window applied)."""
    i0, i1, l, lo, hi = bl_axis32(n, N, defect)
    Wm = np.zeros((N, n), dtype=np.float32)
    X = np.arange(N)
    np.add.at(Wm, (X, i0), (np.float32(1) - l))
    np.add.at(Wm, (X, i1), l)
    inside = (X[:, None] >= lo[None, :]) & (X[:, None] <= hi[None, :])
    return torch.from_numpy(Wm * inside)


# ------------------------------------------------------------------------------------------------------------
# compute: the header's formulas, in `dt` (float64: the reference; float32: the emulation), with planted defects
# ------------------------------------------------------------------------------------------------------------
def _rows(t, rows, ld, off, C):
    return t[(_ar(rows)[:, None] * ld + off + _ar(C)[None, :])]


def _in_act_terms(sp, t, dt, defect=None):
    """(x, u, n, d, mean, rstd) [G, P, C] of the fused kernels from the given statistics."""
    G, P, C, flags = sp["G"], sp["P"], sp["C"], sp["flags"]
    if defect == "flags_swapped":
        flags = ((flags & 1) << 1) | (flags >> 1)
    x = t["x"][:G * P * C].reshape(G, P, C).to(dt)
    u = _elu(x) if flags & 1 else x
    st = t["stats"][:G * 2 * C].reshape(G, 2, C).to(dt)
    mean, rstd = st[:, 0:1], st[:, 1:2]
    n = (u - mean) * rstd
    d = None
    if "dy" in t:
        d = _rows(t["dy"], G * P, sp["ldd"], sp["dy_off"], C).reshape(G, P, C).to(dt)
        if flags & 2:
            d = d * _elud(x if defect == "elud_of_x" else n)
    return x, u, n, d, mean, rstd, flags


def compute(entry, sp, t, dt=F64, order="seq", defect=None):
    """name -> values of the write set (in the order of reference()'s idx) of `entry`."""
    e = entry
    if e == "im2col":
        C = sp["C"]
        src, ok = _patch_src(sp, defect)
        v = t["x"][src[:, :, None] * C + _ar(C)].to(dt)
        return {"patches": torch.where(ok[:, :, None], v, torch.zeros((), dtype=dt))}
    if e == "col2im":
        if defect in (None, "no_ho_test"):      # without `ho >= Ho` pixels of the ragged tail read the next rows' patches
            return {"dx": _col2im_gather(sp, t, dt, order, ho_test=defect is None)}
        C, k = sp["C"], sp["k"]      # the other defects: the adjoint of the defective im2col, as a scatter
        src, ok = _patch_src(sp, defect)
        dx = torch.zeros(sp["R"] * sp["H"] * sp["W"], C, dtype=dt)
        dp = t["dpatches"][:src.numel() * C].reshape(-1, C).to(dt)
        dx.index_add_(0, src.reshape(-1)[ok.reshape(-1)], dp[ok.reshape(-1)])
        return {"dx": dx}
    if e == "elu_fwd":
        return {"y": _elu(t["x"][:sp["n"]].to(dt))}
    if e == "elu_bwd":
        x, dy = t["x"][:sp["n"]].to(dt), t["dy"][:sp["n"]].to(dt)
        return {"dx": torch.where(x > 0, dy, dy * torch.exp(x))}
    if e == "inorm_finalize":
        G, P, C = sp["G"], sp["P"], sp["C"]
        s = t["sums"][:G * 2 * C].reshape(G, 2, C).to(dt)
        inv = torch.tensor(1.0, dtype=dt) / P
        mean = s[:, 0] * inv
        var = (s[:, 1] * inv - mean * mean).clamp_min(0)
        if defect == "unbiased" and P > 1:
            var = var * P / (P - 1)
        eps = torch.tensor(sp["eps"], dtype=dt)
        rstd = 1 / (torch.sqrt(var) + eps) if defect == "eps_outside" else 1 / torch.sqrt(var + eps)
        return {"stats": torch.stack([mean, rstd], 1)}
    if e == "inorm_apply":
        G, P, C = sp["G"], sp["P"], sp["C"]
        x = t["x"][:G * P * C].reshape(G, P, C).to(dt)
        st = t["stats"][:G * 2 * C].reshape(G, 2, C).to(dt)
        return {"y": (x - st[:, 0:1]) * st[:, 1:2]}
    if e == "inorm_bwd_apply":
        G, P, C = sp["G"], sp["P"], sp["C"]
        y, dy = t["y"][:G * P * C].reshape(G, P, C).to(dt), t["dy"][:G * P * C].reshape(G, P, C).to(dt)
        st, sm = t["stats"][:G * 2 * C].reshape(G, 2, C).to(dt), t["sums"][:G * 2 * C].reshape(G, 2, C).to(dt)
        inv = torch.tensor(1.0, dtype=dt) / P
        return {"dx": st[:, 1:2] * (dy - sm[:, 0:1] * inv - y * (sm[:, 1:2] * inv))}
    if e == "in_act_sums":
        G, P, C, ns = sp["G"], sp["P"], sp["C"], sp["nsplit"]
        if sp["bwd"]:
            x, u, n, d, _, _, _ = _in_act_terms(sp, t, dt, defect)
            a, b = d, d * n
        else:
            flags = sp["flags"] if defect != "flags_swapped" else ((sp["flags"] & 1) << 1) | (sp["flags"] >> 1)
            x = t["x"][:G * P * C].reshape(G, P, C).to(dt)
            u = _elu(x) if flags & 1 else x
            a, b = u, u * u
        slab = torch.zeros(ns, G, 2, C, dtype=dt)
        per = -(-P // ns)
        for s in range(ns):
            lo, hi = s * per, min(P, (s + 1) * per)
            if defect == "ragged_last_row_dropped" and lo < hi < lo + per:
                hi -= 1
            if hi > lo:
                slab[s, :, 0] = _sum(a[:, lo:hi].transpose(1, 2), order)
                slab[s, :, 1] = _sum(b[:, lo:hi].transpose(1, 2), order)
        return {"slab": slab}
    if e == "in_act_apply":
        x, u, n, _, _, _, flags = _in_act_terms(sp, t, dt, defect)
        return {"y": _elu(n) if flags & 2 else n}
    if e == "in_act_bwd_apply":
        G, P, C = sp["G"], sp["P"], sp["C"]
        x, u, n, d, mean, rstd, flags = _in_act_terms(sp, t, dt, defect)
        sm = t["sums"][:G * 2 * C].reshape(G, 2, C).to(dt)
        inv = torch.tensor(1.0, dtype=dt) / P
        r = rstd * (d - sm[:, 0:1] * inv - n * (sm[:, 1:2] * inv))
        return {"dx": r * _elud(x) if flags & 1 else r}
    if e in ("avgpool_fwd", "avgpool_bwd"):
        B, H, W, C, sz = sp["B"], sp["H"], sp["W"], sp["C"], sp["sz"]
        Ho, Wo = H // sz, W // sz
        inv = torch.tensor(1.0, dtype=dt) / (sz * sz)
        if e == "avgpool_fwd":
            x = t["x"][:B * H * W * C].reshape(B, H, W, C).to(dt)
            win = torch.stack([x[:, dy:Ho * sz:sz, dx:Wo * sz:sz] for dy in range(sz) for dx in range(sz)], -1)
            return {"y": _sum(win, order) * inv}
        dy = t["dy"][:B * Ho * Wo * C].reshape(B, Ho, Wo, C).to(dt)
        h, w = _ar(H) // sz, _ar(W) // sz
        v = dy[:, h.clamp_max(Ho - 1)][:, :, w.clamp_max(Wo - 1)] * inv
        if defect != "tail_not_zero":
            v = v * ((h < Ho)[None, :, None, None] & (w < Wo)[None, None, :, None])
        return {"dx": v}
    if e == "bilinear_fwd":
        B, h, w, H, W, C = sp["B"], sp["h"], sp["w"], sp["H"], sp["W"], sp["C"]
        x = t["x"][:B * h * w * C].reshape(B, h, w, C).to(dt)
        if dt == F64:
            Wy, Wx = bl_axis(h, H, defect)[0], bl_axis(w, W, defect)[0]
            return {"y": torch.einsum("Yy,byxc,Xx->bYXc", Wy, x, Wx)}
        y0, y1, ly, _, _ = bl_axis32(h, H, defect)
        x0, x1, lx, _, _ = bl_axis32(w, W, defect)
        ly, lx = torch.from_numpy(ly)[None, :, None, None], torch.from_numpy(lx)[None, None, :, None]
        g = lambda a, b: x[:, torch.from_numpy(a)][:, :, torch.from_numpy(b)]        # noqa: E731
        return {"y": (g(y0, x0) * (1 - lx) + g(y0, x1) * lx) * (1 - ly) + (g(y1, x0) * (1 - lx) + g(y1, x1) * lx) * ly}
    if e == "bilinear_bwd":
        B, h, w, H, W, C = sp["B"], sp["h"], sp["w"], sp["H"], sp["W"], sp["C"]
        dy = t["dy"][:B * H * W * C].reshape(B, H, W, C).to(dt)
        if dt == F64:
            Wy, Wx = bl_axis(h, H, defect)[0], bl_axis(w, W, defect)[0]
        else:
            Wy, Wx = _bl_w32(h, H, defect), _bl_w32(w, W, defect)
        return {"dx": torch.einsum("Yy,bYXc,Xx->byxc", Wy, dy, Wx)}
    if e in ("scale_bf_fwd", "scale_bf_bwd"):
        B, T, Fq, C, mode = sp["B"], sp["T"], sp["F"], sp["C"], sp["mode"]
        x = t["x"][:B * T * Fq * C].reshape(B, T, Fq, C).to(dt)
        s = t["s"][:B * Fq].reshape(B, Fq).to(dt)
        if defect == "s_indexed_bt":      # s[b][t] instead of s[b][f]
            sv = s.reshape(-1)[(_ar(B)[:, None] * Fq + _ar(T)[None, :]) % (B * Fq)][:, :, None, None]
        else:
            sv = s[:, None, :, None]
        if e == "scale_bf_fwd":
            return {"y": x * sv if mode == 0 else x + sv}
        dy = t["dy"][:B * T * Fq * C].reshape(B, T, Fq, C).to(dt)
        prod = dy * x if mode == 0 else dy
        if defect == "second_row_missing":      # the second row in flight (t + nrl) never reaches ds
            nrl = max(256 // max(C // 4, 1), 1)
            keep = ((_ar(T) // nrl) % 2 == 0).to(dt)
            prod = prod * keep[None, :, None, None]
        return {"dx": dy * sv if mode == 0 else dy.clone(), "ds": _sum(prod.permute(0, 2, 1, 3).reshape(B, Fq, T * C), order)}
    if e == "freq_linear":
        B, T, Fq, C, ldw = sp["B"], sp["T"], sp["F"], sp["C"], sp["ldw"]
        x = t["x"][:B * T * Fq * C].reshape(B, T, Fq, C).to(dt)
        Wm = t["W"][(_ar(Fq)[:, None] * ldw + _ar(Fq)[None, :])].to(dt)
        if defect == "W_transposed":
            Wm = Wm.t()
        rb = t["rb"][:B * Fq].reshape(B, Fq).to(dt)
        rbv = rb[:, None, :, None]
        if defect == "rb_indexed_t":
            rbv = rb.reshape(-1)[(_ar(T)[:, None] % B) * Fq + _ar(Fq)[None, :]][None, :, :, None].expand(B, T, Fq, 1)
        prod = Wm[None, None, :, None, :] * x.permute(0, 1, 3, 2)[:, :, None, :, :]      # [B, T, F', C, F]
        return {"y": _sum(prod, order) + rbv}
    if e == "softmax_fwd":
        rows, n = sp["rows"], sp["n"]
        sc = torch.tensor(sp["scale"], dtype=F32).to(dt)          # the scale the kernel receives is a float
        x = t["x"][:rows * n].reshape(rows, n).to(dt)
        if defect == "no_max":
            ex = torch.exp(x * sc)
        elif defect == "scale_after_max":
            ex = torch.exp((x - x.max(1, keepdim=True).values) * sc)
        else:
            z = x * sc
            ex = torch.exp(z - z.max(1, keepdim=True).values)
        return {"y": ex / _sum(ex, order).unsqueeze(1)}
    if e == "softmax_bwd":
        rows, n = sp["rows"], sp["n"]
        sc = torch.tensor(sp["scale"], dtype=F32).to(dt)
        y, dy = t["y"][:rows * n].reshape(rows, n).to(dt), t["dy"][:rows * n].reshape(rows, n).to(dt)
        r = y * (dy - _sum(dy * y, order).unsqueeze(1))
        return {"dx": r if defect == "bwd_no_scale" else sc * r}
    if e == "rowbias_act":
        rows, C, rpr = sp["rows"], sp["C"], sp["rpr"]
        v = t["x"][:rows * C].reshape(rows, C).to(dt)
        if sp["rb"]:
            v = v + t["rb"][((_ar(rows) // rpr)[:, None] * C + _ar(C)[None, :])].to(dt)
        return {"y": torch.tanh(v) if sp["act"] == 1 else 1 / (1 + torch.exp(-v))}
    if e == "act_bwd":
        y, dy = t["y"][:sp["n"]].to(dt), t["dy"][:sp["n"]].to(dt)
        return {"dx": dy * (1 - y * y) if sp["act"] == 1 else dy * (y * (1 - y))}
    raise ValueError(e)


def _col2im_taps(sp, ho_test=True):
    """For every pixel and tap: (index of the patch row, valid) -- the gather of the header, pixel-major."""
    R, H, W, k, sh, sw, p = sp["R"], sp["H"], sp["W"], sp["k"], sp["sh"], sp["sw"], sp["p"]
    Ho, Wo = conv_geom(sp)
    pix = _ar(R * H * W)
    r, hi, wi = pix // (H * W), (pix // W) % H, pix % W
    tap = _ar(k * k)
    ky, kx = tap // k, tap % k
    hn, wn = hi[:, None] + p - ky[None, :], wi[:, None] + p - kx[None, :]
    ok = (hn >= 0) & (hn % sh == 0) & (wn >= 0) & (wn % sw == 0)
    ho, wo = torch.div(hn.clamp_min(0), sh, rounding_mode="floor"), torch.div(wn.clamp_min(0), sw, rounding_mode="floor")
    if ho_test:
        ok = ok & (ho < Ho)
    ok = ok & (wo < Wo)
    m = (r[:, None] * Ho + ho) * Wo + wo
    return m, ok & (m < R * Ho * Wo), tap


def _col2im_gather(sp, t, dt, order, ho_test=True, absval=False):
    C, k = sp["C"], sp["k"]
    m, ok, tap = _col2im_taps(sp, ho_test)
    src = (m.clamp(0) * (k * k) + tap[None, :])[:, :, None] * C + _ar(C)          # [pix, kk, C]
    n_p = sp["R"] * conv_geom(sp)[0] * conv_geom(sp)[1] * k * k * C
    v = t["dpatches"][src.clamp_max(n_p - 1)].to(dt)
    if absval:
        v = v.abs()
    v = torch.where(ok[:, :, None], v, torch.zeros((), dtype=dt))
    return _sum(v.transpose(1, 2), order)          # [pix, C]


# ------------------------------------------------------------------------------------------------------------
# reference = compute in float64 + the bounds of the module docstring
# ------------------------------------------------------------------------------------------------------------
def rstd_interval(mean, var, e2abs, d_m, n, eps):
    """(lo, hi) of the kernel's rstd: the one-pass variance is off by at most d_v (module docstring)."""
    d_v = eps_for(False, n) * (e2abs + mean ** 2) + 2 * mean.abs() * d_m + d_m ** 2
    lo = (1 - 4 * U) / torch.sqrt(var + d_v + eps)
    hi = (1 + 4 * U) / torch.sqrt((var - d_v).clamp_min(0) + eps)
    return lo, hi


def _stats_ref(G, C, mean, d_m, ma, rstd, lo, hi):
    """Ref over stats [G][2][C]: the mean with its bound, rstd as (midpoint, half width), S = the exact values."""
    val = torch.stack([mean, (lo + hi) / 2], 1)
    bound = torch.stack([d_m, (hi - lo) / 2], 1)
    S = torch.stack([ma, rstd], 1)
    return _ref(_ar(G * 2 * C), val, S, bound)


def _in_act_errs(sp, t):
    """(x, u, n, d, rstd, du, dn, dd, e1) in float64: the propagated errors of the fused kernels' element-wise chain."""
    x, u, n, d, mean, rstd, flags = _in_act_terms(sp, t, F64)
    du = D_EXPM1 * u.abs() * (x <= 0) if flags & 1 else torch.zeros_like(u)
    dn = du * rstd.abs() + 2 * U * n.abs()
    dd = None
    if d is not None:
        if flags & 2:
            e1 = _elud(n)
            dyv = _rows(t["dy"], sp["G"] * sp["P"], sp["ldd"], sp["dy_off"], sp["C"]).reshape(x.shape).double().abs()
            dd = dyv * (dn + D_EXP * e1 + U * e1)
        else:
            dd = torch.zeros_like(d)
    return x, u, n, d, rstd, du, dn, dd, flags


def reference(b, tensors=None, entry=None):
    """name -> Ref | Partial of every output of the built case over `tensors` (default: the case's own buffers)."""
    e, sp = entry or b.case.entry, b.spec
    t = b.views(tensors or b.bufs)
    v = compute(e, sp, t, F64)
    if e == "im2col":
        R, C, k, ldp = sp["R"], sp["C"], sp["k"], sp["ldp"]
        Ho, Wo = conv_geom(sp)
        idx = (_ar(R * Ho * Wo)[:, None, None] * ldp + _ar(k * k)[None, :, None] * C + _ar(C)[None, None, :])
        val = v["patches"]
        return {"patches": _ref(idx, val, val.abs(), torch.zeros_like(val), torch.ones(val.shape, dtype=torch.bool))}
    if e == "col2im":
        R, H, W, C, k, sh, sw = sp["R"], sp["H"], sp["W"], sp["C"], sp["k"], sp["sh"], sp["sw"]
        S = _col2im_gather(sp, t, F64, "seq", absval=True)
        cnt = _col2im_taps(sp)[1].sum(1)
        n = -(-k // sh) * -(-k // sw)
        assert int(cnt.max()) <= n
        ex = (cnt <= 1)[:, None].expand(-1, C)
        return {"dx": _ref(_ar(R * H * W * C), v["dx"], S, eps_for(False, n) * S, ex)}
    if e == "elu_fwd":
        y, x = v["y"], t["x"][:sp["n"]].double()
        return {"y": _ref(_ar(sp["n"]), y, y.abs(), D_EXPM1 * y.abs(), x > 0)}
    if e == "elu_bwd":
        dx, x = v["dx"], t["x"][:sp["n"]].double()
        return {"dx": _ref(_ar(sp["n"]), dx, dx.abs(), (D_EXP + U) * dx.abs() + TINY, x > 0)}
    if e == "inorm_finalize":
        G, P, C = sp["G"], sp["P"], sp["C"]
        s = t["sums"][:G * 2 * C].reshape(G, 2, C).double()
        mean, rstd = v["stats"][:, 0], v["stats"][:, 1]
        var = (s[:, 1] / P - mean * mean).clamp_min(0)
        d_m = eps_for(False, 0) * mean.abs()
        lo, hi = rstd_interval(mean, var, s[:, 1].abs() / P, d_m, 0, sp["eps"])
        return {"stats": _stats_ref(G, C, mean, d_m, mean.abs(), rstd, lo, hi)}
    if e == "inorm_apply":
        y = v["y"]
        return {"y": _ref(_ar(y.numel()), y, y.abs(), eps_for(False, 0) * y.abs())}
    if e == "inorm_bwd_apply":
        G, P, C = sp["G"], sp["P"], sp["C"]
        y, dy = t["y"][:G * P * C].reshape(G, P, C).double(), t["dy"][:G * P * C].reshape(G, P, C).double()
        st, sm = t["stats"][:G * 2 * C].reshape(G, 2, C).double(), t["sums"][:G * 2 * C].reshape(G, 2, C).double()
        S = st[:, 1:2].abs() * (dy.abs() + sm[:, 0:1].abs() / P + (y * sm[:, 1:2]).abs() / P)
        return {"dx": _ref(_ar(G * P * C), v["dx"], S, eps_for(False, 0) * S)}
    if e == "in_act_sums":
        G, P, C, ns = sp["G"], sp["P"], sp["C"], sp["nsplit"]
        eP = eps_for(False, P)
        if sp["bwd"]:
            x, u, n, d, rstd, du, dn, dd, flags = _in_act_errs(sp, t)
            S0, S1 = d.abs().sum(1), (d * n).abs().sum(1)
            b0 = eP * S0 + dd.sum(1)
            b1 = eP * S1 + (dd * n.abs() + d.abs() * dn + U * (d * n).abs()).sum(1)
        else:
            x = t["x"][:G * P * C].reshape(G, P, C).double()
            u = _elu(x) if sp["flags"] & 1 else x
            k = 1 if sp["flags"] & 1 else 0
            S0, S1 = u.abs().sum(1), (u * u).sum(1)
            b0, b1 = (eP + k * D_EXPM1) * S0, (eP + k * (2 * D_EXPM1 + U)) * S1
        per = -(-P // ns)
        zero = torch.zeros(ns, G * 2 * C, dtype=torch.bool)
        zero[[s for s in range(ns) if s * per >= P]] = True
        return {"slab": Partial(_ar(ns * G * 2 * C).reshape(ns, G * 2 * C), v["slab"].sum(0).reshape(-1),
                                torch.stack([S0, S1], 1).reshape(-1), torch.stack([b0, b1], 1).reshape(-1), zero)}
    if e == "in_act_apply":
        G, P, C = sp["G"], sp["P"], sp["C"]
        x, u, n, _, rstd, du, dn, _, flags = _in_act_errs(sp, t)
        y = v["y"]
        bound = dn + D_EXPM1 * y.abs() * (n <= 0) if flags & 2 else dn
        idx = _ar(G * P)[:, None] * sp["ldy"] + sp["y_off"] + _ar(C)[None, :]
        return {"y": _ref(idx, y, y.abs(), bound + U * y.abs())}
    if e == "in_act_bwd_apply":
        G, P, C = sp["G"], sp["P"], sp["C"]
        x, u, n, d, rstd, du, dn, dd, flags = _in_act_errs(sp, t)
        sm = t["sums"][:G * 2 * C].reshape(G, 2, C).double()
        a, bb = sm[:, 0:1] / P, sm[:, 1:2] / P
        S = rstd.abs() * (d.abs() + a.abs() + (n * bb).abs())
        bound = rstd.abs() * (dd + bb.abs() * dn) + eps_for(False, 0) * S
        dx = v["dx"]
        if flags & 1:
            e1 = _elud(x)
            bound, S = bound * e1 + (D_EXP + U) * dx.abs(), S * e1
        idx = _ar(G * P)[:, None] * sp["lddx"] + sp["dx_off"] + _ar(C)[None, :]
        return {"dx": _ref(idx, dx, S, bound)}
    if e == "avgpool_fwd":
        B, H, W, C, sz = sp["B"], sp["H"], sp["W"], sp["C"], sp["sz"]
        S = compute(e, sp, {"x": t["x"][:B * H * W * C].abs()}, F64)["y"]
        return {"y": _ref(_ar(S.numel()), v["y"], S, eps_for(False, sz * sz + 1) * S)}
    if e == "avgpool_bwd":
        dx = v["dx"]
        return {"dx": _ref(_ar(dx.numel()), dx, dx.abs(), 2 * U * dx.abs(), dx == 0)}
    if e == "bilinear_fwd":
        B, h, w, H, W, C = sp["B"], sp["h"], sp["w"], sp["H"], sp["W"], sp["C"]
        x = t["x"][:B * h * w * C].reshape(B, h, w, C).double()
        Wy, _, SWy, dly = bl_axis(h, H)
        Wx, _, SWx, dlx = bl_axis(w, W)
        S = torch.einsum("Yy,byxc,Xx->bYXc", Wy, x.abs(), Wx)
        Gx = sum(torch.einsum("Yy,byxc,Xx->bYXc", Wy, x, sw_).abs() for sw_ in SWx)
        Gy = sum(torch.einsum("Yy,byxc,Xx->bYXc", sw_, x, Wx).abs() for sw_ in SWy)
        Gxy = sum(torch.einsum("Yy,byxc,Xx->bYXc", a, x, c).abs() for a in SWy for c in SWx)
        dY, dX = dly[None, :, None, None], dlx[None, None, :, None]
        bound = dX * Gx + dY * Gy + dX * dY * Gxy + eps_for(False, 8) * S
        return {"y": _ref(_ar(S.numel()), v["y"], S, bound)}
    if e == "bilinear_bwd":
        B, h, w, H, W, C = sp["B"], sp["h"], sp["w"], sp["H"], sp["W"], sp["C"]
        dy = t["dy"][:B * H * W * C].reshape(B, H, W, C).double().abs()
        Wy, DWy, _, _ = bl_axis(h, H)
        Wx, DWx, _, _ = bl_axis(w, W)
        nx, ny = int(((DWx > 0) | (Wx > 0)).sum(0).max()), int(((DWy > 0) | (Wy > 0)).sum(0).max())
        assert nx <= 2 * W / w + 3 + 2 and ny <= 2 * H / h + 3 + 2, (nx, ny)          # bl_window's 2 / scale + 3 (+ the neighbouring cells)
        tabs = torch.einsum("bYXc,Xx->bYxc", dy, Wx)
        dtmp = torch.einsum("bYXc,Xx->bYxc", dy, DWx) + eps_for(False, nx) * tabs
        S = torch.einsum("Yy,bYxc->byxc", Wy, tabs)
        bound = (torch.einsum("Yy,bYxc->byxc", Wy + DWy, dtmp) + torch.einsum("Yy,bYxc->byxc", DWy, tabs)
                 + eps_for(False, ny) * S)
        return {"dx": _ref(_ar(S.numel()), v["dx"], S, bound)}
    if e == "scale_bf_fwd":
        y = v["y"]
        return {"y": _ref(_ar(y.numel()), y, y.abs(), eps_for(False, 0) * y.abs())}
    if e == "scale_bf_bwd":
        B, T, Fq, C, mode = sp["B"], sp["T"], sp["F"], sp["C"], sp["mode"]
        dx = v["dx"]
        ta = {k: (t[k][:B * T * Fq * C].abs() if k in ("x", "dy") else t[k]) for k in ("x", "dy", "s")}
        S = compute(e, sp, ta, F64)["ds"]
        return {"dx": _ref(_ar(dx.numel()), dx, dx.abs(), eps_for(False, 0) * dx.abs(),
                           torch.full(dx.shape, mode == 1, dtype=torch.bool)),
                "ds": _ref(_ar(B * Fq), v["ds"], S, eps_for(False, T * C) * S)}
    if e == "freq_linear":
        B, T, Fq, C = sp["B"], sp["T"], sp["F"], sp["C"]
        ta = {"x": t["x"][:B * T * Fq * C].abs(), "W": t["W"].abs(), "rb": t["rb"][:B * Fq].abs()}
        S = compute(e, sp, ta, F64)["y"]
        return {"y": _ref(_ar(S.numel()), v["y"], S, eps_for(False, Fq + 1) * S)}
    if e == "softmax_fwd":
        rows, n = sp["rows"], sp["n"]
        sc = float(torch.tensor(sp["scale"], dtype=F32))
        z = t["x"][:rows * n].reshape(rows, n).double() * sc
        mx = z.max(1, keepdim=True).values
        dz = U * (z.abs() + mx.abs() + (z - mx).abs())
        rho = D_EXP + torch.expm1(dz)
        y = v["y"]
        bound = y * (rho + (y * rho).sum(1, keepdim=True) + eps_for(False, n) + 2 * U) + TINY
        return {"y": _ref(_ar(rows * n), y, y, bound)}
    if e == "softmax_bwd":
        rows, n = sp["rows"], sp["n"]
        sc = abs(float(torch.tensor(sp["scale"], dtype=F32)))
        y, dy = t["y"][:rows * n].reshape(rows, n).double(), t["dy"][:rows * n].reshape(rows, n).double()
        sa, s = (dy * y).abs().sum(1, keepdim=True), (dy * y).sum(1, keepdim=True)
        S = sc * y.abs() * (dy.abs() + s.abs())
        return {"dx": _ref(_ar(rows * n), v["dx"], S, sc * y.abs() * eps_for(False, n) * sa + eps_for(False, 0) * S
                           + TINY * (1 + sc * (dy.abs() + s.abs())))}
    if e == "rowbias_act":
        rows, C = sp["rows"], sp["C"]
        y = v["y"]
        pre = t["x"][:rows * C].reshape(rows, C).double()
        if sp["rb"]:
            pre = pre + t["rb"][((_ar(rows) // sp["rpr"])[:, None] * C + _ar(C)[None, :])].double()
        dv = U * pre.abs()
        bound = dv + D_TANH * y.abs() if sp["act"] == 1 else dv / 4 + D_SIG * y.abs()
        return {"y": _ref(_ar(rows * C), y, y.abs(), bound)}
    if e == "act_bwd":
        y, dy = t["y"][:sp["n"]].double(), t["dy"][:sp["n"]].double()
        S = dy.abs() * (y * y + (1 - y * y).abs()) if sp["act"] == 1 else dy.abs() * y.abs() * (y.abs() + (1 - y).abs())
        return {"dx": _ref(_ar(sp["n"]), v["dx"], S, eps_for(False, 0) * S)}
    raise ValueError(e)


def chain_stats_ref(u, eps, elu_pre=False):
    """Ref of the statistics [G][2][C] a chain (sums + finalize) leaves for u [G, P, C] float64 (the exact pre-activation):
    d_m = e(P) E|u| (+ D_EXPM1 E|u| when u = ELU(x) was computed by the kernel), n = P."""
    G, P, C = u.shape
    mean, ma = u.mean(1), u.abs().mean(1)
    e2 = (u * u).mean(1)
    var = (e2 - mean * mean).clamp_min(0)
    k = 1 if elu_pre else 0
    d_m = (eps_for(False, P) + k * D_EXPM1) * ma
    lo, hi = rstd_interval(mean, var, e2 * (1 + k * (2 * D_EXPM1 + U)), d_m, P, eps)
    return _stats_ref(G, C, mean, d_m, ma, 1 / torch.sqrt(var + eps), lo, hi), (mean, d_m, lo, hi)


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, targets
# ------------------------------------------------------------------------------------------------------------
NORM_C = [4, 12, 16, 256, 1024, 1028]
NORM_P = [1, 2, 31, 32, 33, 257]
NORM_DATA = ["gauss", "offset", "const", "spike"]
LDS = ["0", "C", "C+4", "2C"]
STRIDES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 3)]
BL = [(1, 1), (1, 7), (4, 9), (2, 64), (3, 96), (7, 7), (9, 4), (64, 2)]
SM_N = [1, 3, 4, 255, 256, 257, 1020, 1024, 1025, 1028, 2049]
PT_N = [4, 1020, 1024, 1028, 4100]
POOL_HW = ["sz", "sz+1", "2sz+1", "9"]
SB_T = ["1", "nrl-1", "nrl", "nrl+1", "2nrl", "2nrl+1"]

DIMS = {
    "im2col": dict(img=list(IMG), k=[1, 3, 5], stride=STRIDES, p=["0", "k/2", "k"], C=[1, 4, 12, 16], ldp=["kk", "kk+3"], R=[1, 2]),
    "col2im": dict(img=list(IMG), k=[1, 3, 5], stride=STRIDES, p=["0", "k/2", "k"], C=[4, 12, 16], R=[1, 2]),
    "elu_fwd": dict(n=PT_N, data=["gauss", "wide"]),
    "elu_bwd": dict(n=PT_N, data=["gauss", "wide"], alias=[0, 1]),
    "inorm_finalize": dict(C=NORM_C, P=NORM_P, G=[1, 3], data=NORM_DATA),
    "inorm_apply": dict(C=NORM_C, P=NORM_P, G=[1, 3], data=NORM_DATA),
    "inorm_bwd_apply": dict(C=NORM_C, P=NORM_P, G=[1, 3], data=NORM_DATA, alias=[0, 1]),
    "in_act_sums": dict(C=NORM_C, P=NORM_P, G=[1, 3], nsplit=["1", "2", "3", "7", "P", "P+1"], flags=[0, 1, 2, 3],
                        mode=["fwd", "bwd"], ldd=LDS, data=NORM_DATA),
    "in_act_apply": dict(C=NORM_C, P=NORM_P, G=[1, 3], flags=[0, 1, 2, 3], ldy=LDS, data=NORM_DATA),
    "in_act_bwd_apply": dict(C=NORM_C, P=NORM_P, G=[1, 3], flags=[0, 1, 2, 3], ldd=LDS, lddx=LDS, alias=[0, 1], data=NORM_DATA),
    "avgpool_fwd": dict(sz=[1, 2, 3], H=POOL_HW, W=POOL_HW, C=[4, 12], B=[1, 2]),
    "avgpool_bwd": dict(sz=[1, 2, 3], H=POOL_HW, W=POOL_HW, C=[4, 12], B=[1, 2]),
    "bilinear_fwd": dict(hH=BL, wW=BL, C=[4, 8], B=[1, 2], data=["gauss", "offset"]),
    "bilinear_bwd": dict(hH=BL, wW=BL, C=[4, 8], B=[1, 2]),
    "scale_bf_fwd": dict(C=[4, 8, 12, 64, 1024, 1028], T=[1, 3, 9], F=[1, 5], B=[1, 2], mode=[0, 1]),
    "scale_bf_bwd": dict(C=[4, 8, 12, 64, 1024, 6, 1028], T=SB_T, F=[1, 5], B=[1, 2], mode=[0, 1]),
    "freq_linear": dict(FC=[(1, 4), (5, 12), (33, 32), (64, 256)], ldw=["F", "F+3"], T=[1, 3], B=[1, 2]),
    "softmax_fwd": dict(n=SM_N, rows=[1, 3], scale=[1.0, 0.37, -2.0], data=["gauss", "equal", "dominant", "spread60"], align=[0, 1]),
    "softmax_bwd": dict(n=SM_N, rows=[1, 3], scale=[1.0, 0.37, -2.0], data=["gauss", "equal", "dominant", "spread60"], align=[0, 1]),
    "rowbias_act": dict(act=[1, 3], rb=[0, 1], C=[1, 5, 64], rows=[1, 7, 300], rpr=[1, 3, 7], data=["gauss", "wide"]),
    "act_bwd": dict(act=[1, 3], n=[1, 5, 1024, 4099]),
}


def _pad(k, p):
    return {"0": 0, "k/2": k // 2, "k": k}[p]


def _conv_empty(img, k, p):
    H, W = IMG[img]
    return H + 2 * _pad(k, p) - k < 0 or W + 2 * _pad(k, p) - k < 0


_CONV_RULES = [
    ("the output is not empty", ("img", "k", "p"), _conv_empty),
    ("a stride of 3 runs with k = 1 and k = 3", ("stride", "k"), lambda s, k: s == (3, 3) and k == 5),
]
RULES = {e: [] for e in ENTRIES}
RULES["im2col"] = _CONV_RULES + [("ldp == k*k*C for C > 1", ("C", "ldp"), lambda C, ldp: C > 1 and ldp != "kk")]
RULES["col2im"] = _CONV_RULES
RULES["in_act_sums"] = [("the forward sums take no dy", ("mode", "ldd"), lambda m, ld: m == "fwd" and ld != "0")]
RULES["in_act_bwd_apply"] = [("dx aliases dy only when both strides agree", ("alias", "ldd", "lddx"),
                             lambda a, l1, l2: a == 1 and ({"0": "C"}.get(l1, l1) != {"0": "C"}.get(l2, l2)))]


def sb_vec(C):
    return C % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0


def sb_nrl(C):
    """Rows per pass of the kernel ws_scale_bf_bwd selects: 256 / (C / 4) row lanes (bwd4), 256 / C rows (scalar)."""
    return 256 // (C // 4) if sb_vec(C) else max(256 // C, 1)


def sb_T(d):
    n = sb_nrl(d["C"])
    return max({"1": 1, "nrl-1": n - 1, "nrl": n, "nrl+1": n + 1, "2nrl": 2 * n, "2nrl+1": 2 * n + 1}[d["T"]], 1)


def _ld(C, v):
    return {"0": C, "C": C, "C+4": C + 4, "2C": 2 * C}[v]


def in_act_ns(d):
    P = d["P"]
    return {"P": P, "P+1": P + 1}.get(d["nsplit"]) or int(d["nsplit"])


def softmax_vec(d):
    return d["n"] <= 1024 and d["n"] % 4 == 0 and not d["align"]


def _targets(entry, d, seed=0):
    e = entry
    if e == "im2col":
        if d["C"] > 1:
            return ("im2col_kernel",)
        return ("im2col_c1_kernel",) + (("im2col_c1[ldp > k*k]",) if d["ldp"] != "kk" else ())
    if e == "col2im":
        k, (sh, sw) = d["k"], d["stride"]
        H, W = IMG[d["img"]]
        p = _pad(k, d["p"])
        t = ("col2im_kernel",)
        if sh > k or sw > k:
            t += ("col2im[uncovered pixels]",)
        if (H + 2 * p - k) % sh or (W + 2 * p - k) % sw:
            t += ("col2im[ragged tail]",)
        return t
    if e in ("elu_fwd", "inorm_finalize", "inorm_apply", "avgpool_fwd", "avgpool_bwd", "bilinear_fwd", "bilinear_bwd",
             "scale_bf_fwd", "freq_linear", "act_bwd"):
        return (f"{e}_kernel",)
    if e in ("elu_bwd", "inorm_bwd_apply"):
        return (f"{e}_kernel",) + ((f"{e}[dx aliases dy]",) if d["alias"] else ())
    if e == "in_act_sums":
        c4 = d["C"] // 4
        t = (f"in_act_sums[{d['mode']}]", f"in_act_sums[flags {d['flags']}]")
        t += ("in_act_sums[idle lanes]",) if 256 % min(c4, 256) else ()
        t += ("in_act_sums[second z block]",) if c4 > 256 else ()
        ns, P = in_act_ns(d), d["P"]
        per = -(-P // ns)
        t += ("in_act_sums[empty split]",) if (ns - 1) * per >= P else ()
        t += ("in_act_sums[ragged split]",) if P % per else ()
        return t
    if e == "in_act_apply":
        return ("in_act_apply_kernel", f"in_act_apply[flags {d['flags']}]") + (("in_act_apply[strided y]",) if _ld(d["C"], d["ldy"]) > d["C"] else ())
    if e == "in_act_bwd_apply":
        return (("in_act_bwd_apply_kernel", f"in_act_bwd_apply[flags {d['flags']}]")
                + (("in_act_bwd_apply[dx aliases dy]",) if d["alias"] else ())
                + (("in_act_bwd_apply[strided]",) if max(_ld(d["C"], d["ldd"]), _ld(d["C"], d["lddx"])) > d["C"] else ()))
    if e == "scale_bf_bwd":
        return (("scale_bf_bwd4_kernel" if sb_vec(d["C"]) else "scale_bf_bwd_kernel"), f"scale_bf_bwd[mode {d['mode']}]")
    if e in ("softmax_fwd", "softmax_bwd"):
        return (f"softmax_rows_{e[-3:]}{'4' if softmax_vec(d) else ''}_kernel",)
    if e == "rowbias_act":
        return ("rowbias_act_fwd_kernel", f"rowbias_act[act {d['act']}]", f"rowbias_act[rb {'on' if d['rb'] else 'NULL'}]")
    raise ValueError(e)


_M = gc.MIN_PER_TARGET
INST = {
    "im2col": ["im2col_kernel", "im2col_c1_kernel", "im2col_c1[ldp > k*k]"],
    "col2im": ["col2im_kernel", "col2im[uncovered pixels]", "col2im[ragged tail]"],
    "elu_bwd": ["elu_bwd_kernel", "elu_bwd[dx aliases dy]"],
    "inorm_bwd_apply": ["inorm_bwd_apply_kernel", "inorm_bwd_apply[dx aliases dy]"],
    "in_act_sums": ["in_act_sums[fwd]", "in_act_sums[bwd]"] + [f"in_act_sums[flags {f}]" for f in range(4)] + [
        "in_act_sums[idle lanes]", "in_act_sums[second z block]", "in_act_sums[empty split]", "in_act_sums[ragged split]"],
    "in_act_apply": ["in_act_apply_kernel", "in_act_apply[strided y]"] + [f"in_act_apply[flags {f}]" for f in range(4)],
    "in_act_bwd_apply": ["in_act_bwd_apply_kernel", "in_act_bwd_apply[dx aliases dy]", "in_act_bwd_apply[strided]"] + [
        f"in_act_bwd_apply[flags {f}]" for f in range(4)],
    "scale_bf_bwd": ["scale_bf_bwd4_kernel", "scale_bf_bwd_kernel", "scale_bf_bwd[mode 0]", "scale_bf_bwd[mode 1]"],
    "softmax_fwd": ["softmax_rows_fwd4_kernel", "softmax_rows_fwd_kernel"],
    "softmax_bwd": ["softmax_rows_bwd4_kernel", "softmax_rows_bwd_kernel"],
    "rowbias_act": ["rowbias_act_fwd_kernel", "rowbias_act[act 1]", "rowbias_act[act 3]", "rowbias_act[rb on]", "rowbias_act[rb NULL]"],
}
for _e in ENTRIES:
    INST.setdefault(_e, [f"{_e}_kernel"])
TOPUP = {e: [({}, INST[e][0], _M)] for e in ENTRIES}
TOPUP["im2col"] = [({"C": 4}, "im2col_kernel", _M), ({"C": 1}, "im2col_c1_kernel", _M), ({"C": 1, "ldp": "kk+3"}, "im2col_c1[ldp > k*k]", _M)]
TOPUP["col2im"] += [({"stride": (3, 3), "k": 1}, "col2im[uncovered pixels]", _M), ({"stride": (3, 3)}, "col2im[ragged tail]", _M)]
TOPUP["elu_bwd"] += [({"alias": 1}, "elu_bwd[dx aliases dy]", _M)]
TOPUP["inorm_bwd_apply"] += [({"alias": 1}, "inorm_bwd_apply[dx aliases dy]", _M)]
TOPUP["in_act_sums"] = ([({"mode": m}, f"in_act_sums[{m}]", _M) for m in ("fwd", "bwd")] + [({"flags": f}, f"in_act_sums[flags {f}]", _M) for f in range(4)]
                        + [({"C": 12}, "in_act_sums[idle lanes]", _M), ({"C": 1028}, "in_act_sums[second z block]", _M),
                           ({"nsplit": "P+1"}, "in_act_sums[empty split]", _M), ({"nsplit": "7", "P": 33}, "in_act_sums[ragged split]", _M)])
TOPUP["in_act_apply"] += [({"ldy": "2C"}, "in_act_apply[strided y]", _M)] + [({"flags": f}, f"in_act_apply[flags {f}]", _M) for f in range(4)]
TOPUP["in_act_bwd_apply"] += ([({"alias": 1}, "in_act_bwd_apply[dx aliases dy]", _M), ({"ldd": "2C"}, "in_act_bwd_apply[strided]", _M)]
                              + [({"flags": f}, f"in_act_bwd_apply[flags {f}]", _M) for f in range(4)])
TOPUP["scale_bf_bwd"] = [({"C": 8}, "scale_bf_bwd4_kernel", _M), ({"C": 6}, "scale_bf_bwd_kernel", _M), ({"C": 12}, "scale_bf_bwd_kernel", _M),
                         ({"mode": 0}, "scale_bf_bwd[mode 0]", _M), ({"mode": 1}, "scale_bf_bwd[mode 1]", _M)]
for _k in ("fwd", "bwd"):
    TOPUP[f"softmax_{_k}"] = [({"n": 1020, "align": 0}, f"softmax_rows_{_k}4_kernel", _M), ({"n": 1024, "align": 1}, f"softmax_rows_{_k}_kernel", _M)]
TOPUP["rowbias_act"] += [({"act": a}, f"rowbias_act[act {a}]", _M) for a in (1, 3)] + [({"rb": 1}, "rowbias_act[rb on]", _M),
                                                                                       ({"rb": 0}, "rowbias_act[rb NULL]", _M)]
EXTRA = {
    "avgpool_fwd": [dict(sz=32, H="sz", W="sz+1", C=4, B=1)],
    "avgpool_bwd": [dict(sz=32, H="sz", W="sz+1", C=4, B=1)],
}
_KEY = {e: "map_" + e for e in ENTRIES}          # the registries of gemm_contract are shared by every suite
for _i, _e in enumerate(ENTRIES):
    gc.DIMS[_KEY[_e]], gc.RULES[_KEY[_e]], gc.INST[_KEY[_e]], gc.TOPUP[_KEY[_e]] = DIMS[_e], RULES[_e], INST[_e], TOPUP[_e]
    gc.SEEDS[_KEY[_e]] = 61 + _i
    gc.PLANNERS[_KEY[_e]] = (lambda e: lambda d, seed: _targets(e, d, seed))(_e)
_CASES = {}


def cases(entry):
    if entry not in _CASES:
        out = [c._replace(entry=entry) for c in gc.cases(_KEY[entry])]
        for i, d in enumerate(EXTRA.get(entry, [])):
            out.append(Case(entry, f"x{i:02d}-" + "-".join(str(v) for v in d.values()), d, _targets(entry, d), 8000 + i))
        _CASES[entry] = out
    return _CASES[entry]


def invalid_pairs(entry):
    return gc.invalid_pairs(_KEY[entry])


def all_pairs(entry):
    return gc.all_pairs(_KEY[entry])


def pairs_of(entry, dims):
    return gc.pairs_of(_KEY[entry], dims)


# ------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------
class MBuilt(nc.NBuilt):
    """norm_contract.NBuilt (bufs / start / spec / alias / outs / wset) + size: name -> the floats of the tensor the call
    receives, so that views() hands over tensors of exactly the contract's extent."""
    def __init__(self, case):
        super().__init__(case)
        self.size = {}

    def views(self, tensors):
        t = {k: v[self.start[k]:self.start[k] + self.size[k]] for k, v in tensors.items()}
        for a, k in self.alias.items():
            t[a] = t[k]
        return t


def _input(b, name, data, fill, read=None, off=0):
    """An operand: `data` (flat) where `read` (bool, default all) is set, `fill` elsewhere, `off` floats into the allocation."""
    data = data.reshape(-1).float()
    t = gc.alloc(data.numel() + off, fill)
    v = data if read is None else torch.where(read.reshape(-1), data, torch.tensor(fill))
    t[GUARD + off:GUARD + off + data.numel()] = v
    b.bufs[name], b.start[name], b.size[name] = t, GUARD + off, data.numel()
    return t


def _output(b, name, n, widx=None, off=0):
    t = gc.alloc(n + off, SENT)
    t[GUARD + off + (_ar(n) if widx is None else widx.reshape(-1))] = NAN
    b.bufs[name], b.start[name], b.size[name] = t, GUARD + off, n
    b.outs.append(name)


def _alias(b, out, name, widx):
    b.alias[out] = name
    b.outs.append(name)
    b.wset = b.start[name] + widx.reshape(-1)


def _norm_data(g, G, P, C, kind):
    x = torch.randn(G, P, C, generator=g)
    if kind == "offset":
        x = x + 100.0
    if kind == "const":
        x = (torch.randint(-8, 9, (G, 1, C), generator=g).float() * 0.25).expand(G, P, C).clone()
    if kind == "spike":
        x[:, P - 1, C - 1] = x[:, P - 1, C - 1].abs().clamp_min(0.5) * 1e3
    return x


def _strided(g, rows, C, ld, off, fill):
    """(data [rows * ld], read mask) of a [rows, C] gauss block in columns [off, off + C) of rows of stride ld."""
    d = torch.randn(rows, ld, generator=g)
    m = torch.zeros(rows, ld, dtype=torch.bool)
    m[:, off:off + C] = True
    return d, m


def _exact_stats(x, flags, eps):
    u = _elu(x.double()) if flags & 1 else x.double()
    mean = u.mean(1)
    var = ((u * u).mean(1) - mean * mean).clamp_min(0)
    return torch.stack([mean, 1 / torch.sqrt(var + eps)], 1)


def build(case, garbage=False):
    e, d, g = case.entry, case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    b = MBuilt(case)
    sp = b.spec
    if e in ("im2col", "col2im"):
        H, W = IMG[d["img"]]
        k, (sh, sw), C, R = d["k"], d["stride"], d["C"], d["R"]
        sp.update(R=R, H=H, W=W, C=C, k=k, sh=sh, sw=sw, p=_pad(k, d["p"]))
        Ho, Wo = conv_geom(sp)
        M = R * Ho * Wo
        if e == "im2col":
            sp["ldp"] = k * k * C + (3 if d["ldp"] == "kk+3" else 0)
            _input(b, "x", torch.randn(R * H * W * C, generator=g), fill)
            widx = _ar(M)[:, None] * sp["ldp"] + _ar(k * k * C)[None, :]
            _output(b, "patches", M * sp["ldp"], widx)
        else:
            _input(b, "dpatches", torch.randn(M * k * k * C, generator=g), fill)
            _output(b, "dx", R * H * W * C)
        return b
    if e in ("elu_fwd", "elu_bwd"):
        n = d["n"]
        x = torch.randn(n, generator=g) * (30.0 if d["data"] == "wide" else 1.0)
        x[::7] = 0.0
        sp.update(n=n)
        _input(b, "x", x, fill)
        if e == "elu_fwd":
            _output(b, "y", n)
            return b
        _input(b, "dy", torch.randn(n, generator=g), fill)
        if d["alias"]:
            _alias(b, "dx", "dy", _ar(n))
        else:
            _output(b, "dx", n)
        return b
    if e in ("inorm_finalize", "inorm_apply", "inorm_bwd_apply", "in_act_sums", "in_act_apply", "in_act_bwd_apply"):
        G, P, C = d["G"], d["P"], d["C"]
        flags = d.get("flags", 0)
        sp.update(G=G, P=P, C=C, flags=flags, eps=IN_EPS)
        x = _norm_data(g, G, P, C, d["data"])
        stats = _exact_stats(x, flags, IN_EPS)
        if e == "inorm_finalize":
            xd = x.double()
            _input(b, "sums", torch.stack([xd.sum(1), (xd * xd).sum(1)], 1), fill)
            _output(b, "stats", G * 2 * C)
            return b
        if e == "inorm_apply":
            _input(b, "x", x, fill)
            _input(b, "stats", stats, fill)
            _output(b, "y", G * P * C)
            return b
        dyv = torch.randn(G, P, C, generator=g)
        if e == "inorm_bwd_apply":
            y = ((x.double() - stats[:, 0:1]) * stats[:, 1:2]).float()
            _input(b, "y", y, fill)
            _input(b, "dy", dyv, fill)
            _input(b, "stats", stats, fill)
            _input(b, "sums", torch.stack([dyv.double().sum(1), (dyv.double() * y.double()).sum(1)], 1), fill)
            if d["alias"]:
                _alias(b, "dx", "dy", _ar(G * P * C))
            else:
                _output(b, "dx", G * P * C)
            return b
        _input(b, "x", x, fill)
        if e == "in_act_apply":
            ld = _ld(C, d["ldy"])
            sp.update(ldy=ld, ldy_arg=0 if d["ldy"] == "0" else ld, y_off=(ld - C) if case.seed % 2 else 0)
            _input(b, "stats", stats, fill)
            _output(b, "y", G * P * ld, _ar(G * P)[:, None] * ld + sp["y_off"] + _ar(C)[None, :])
            return b
        bwd = e == "in_act_bwd_apply" or d["mode"] == "bwd"
        sp["bwd"] = bwd
        if e == "in_act_sums":
            sp["nsplit"] = in_act_ns(d)
            _output(b, "slab", sp["nsplit"] * G * 2 * C)
        if bwd:
            ld = _ld(C, d["ldd"])
            sp.update(ldd=ld, ldd_arg=0 if d["ldd"] == "0" else ld, dy_off=(ld - C) if case.seed % 2 else 0)
            dd, m = _strided(g, G * P, C, ld, sp["dy_off"], fill)
            _input(b, "dy", dd, fill, m)
            _input(b, "stats", stats, fill)
        if e == "in_act_bwd_apply":
            t = b.views(b.bufs)
            _, _, n, dv, _, _, _ = _in_act_terms(sp, t, F64)
            _input(b, "sums", torch.stack([dv.sum(1), (dv * n).sum(1)], 1), fill)
            ldx = _ld(C, d["lddx"])
            sp.update(lddx=ldx, lddx_arg=0 if d["lddx"] == "0" else ldx, dx_off=sp["dy_off"] if d["alias"] else ((ldx - C) if case.seed % 3 else 0))
            widx = _ar(G * P)[:, None] * ldx + sp["dx_off"] + _ar(C)[None, :]
            if d["alias"]:
                _alias(b, "dx", "dy", widx)
            else:
                _output(b, "dx", G * P * ldx, widx)
        return b
    if e in ("avgpool_fwd", "avgpool_bwd"):
        sz = d["sz"]
        hw = lambda v: {"sz": sz, "sz+1": sz + 1, "2sz+1": 2 * sz + 1, "9": max(9, sz)}[v]      # noqa: E731
        B, H, W, C = d["B"], hw(d["H"]), hw(d["W"]), d["C"]
        sp.update(B=B, H=H, W=W, C=C, sz=sz)
        small, big = B * (H // sz) * (W // sz) * C, B * H * W * C
        if e == "avgpool_fwd":
            _input(b, "x", torch.randn(big, generator=g), fill)
            _output(b, "y", small)
        else:
            _input(b, "dy", torch.randn(small, generator=g), fill)
            _output(b, "dx", big)
        return b
    if e in ("bilinear_fwd", "bilinear_bwd"):
        (h, H), (w, W), C, B = d["hH"], d["wW"], d["C"], d["B"]
        sp.update(B=B, h=h, w=w, H=H, W=W, C=C)
        if e == "bilinear_fwd":
            _input(b, "x", torch.randn(B * h * w * C, generator=g) + (100.0 if d["data"] == "offset" else 0.0), fill)
            _output(b, "y", B * H * W * C)
        else:
            _input(b, "dy", torch.randn(B * H * W * C, generator=g), fill)
            _output(b, "dx", B * h * w * C)
            _output(b, "tmp", B * H * w * C)
        return b
    if e in ("scale_bf_fwd", "scale_bf_bwd"):
        C, Fq, B, mode = d["C"], d["F"], d["B"], d["mode"]
        T = sb_T(d) if e == "scale_bf_bwd" else d["T"]
        sp.update(B=B, T=T, F=Fq, C=C, mode=mode)
        n = B * T * Fq * C
        x, dy = torch.randn(B, T, Fq, C, generator=g), torch.randn(B, T, Fq, C, generator=g)
        if T * C > CAP:          # suite condition: a sum above CAP leaves carries a spike on its last element
            x[:, T - 1, :, C - 1] = x[:, T - 1, :, C - 1].abs().clamp_min(0.5) * 1e3
            dy[:, T - 1, :, C - 1] = dy[:, T - 1, :, C - 1].abs().clamp_min(0.5) * 1e3
        _input(b, "x", x, fill)
        _input(b, "s", torch.randn(B * Fq, generator=g), fill)
        if e == "scale_bf_fwd":
            _output(b, "y", n)
        else:
            _input(b, "dy", dy, fill)
            _output(b, "dx", n)
            _output(b, "ds", B * Fq)
        return b
    if e == "freq_linear":
        (Fq, C), T, B = d["FC"], d["T"], d["B"]
        ldw = Fq + (3 if d["ldw"] == "F+3" else 0)
        sp.update(B=B, T=T, F=Fq, C=C, ldw=ldw)
        _input(b, "x", torch.randn(B * T * Fq * C, generator=g), fill)
        m = torch.zeros(Fq, ldw, dtype=torch.bool)
        m[:, :Fq] = True
        _input(b, "W", torch.randn(Fq, ldw, generator=g) / math.sqrt(Fq), fill, m)
        _input(b, "rb", torch.randn(B * Fq, generator=g), fill)
        _output(b, "y", B * T * Fq * C)
        return b
    if e in ("softmax_fwd", "softmax_bwd"):
        rows, n, al = d["rows"], d["n"], d["align"]
        sp.update(rows=rows, n=n, scale=d["scale"])
        x = torch.randn(rows, n, generator=g)
        if d["data"] == "equal":
            x = torch.full((rows, n), 0.75)
        if d["data"] == "dominant":
            x[:, n // 2] += 40.0
        if d["data"] == "spread60":
            x = (torch.rand(rows, n, generator=g) * 120.0 - 60.0)
        if e == "softmax_fwd":
            _input(b, "x", x, fill, off=al)
            _output(b, "y", rows * n, off=al)
        else:
            y = compute("softmax_fwd", sp, {"x": x.reshape(-1)}, F64)["y"]
            _input(b, "y", y.float(), fill, off=al)
            _input(b, "dy", torch.randn(rows * n, generator=g), fill, off=al)
            _output(b, "dx", rows * n, off=al)
        return b
    if e == "rowbias_act":
        rows, C, rpr = d["rows"], d["C"], d["rpr"]
        sp.update(rows=rows, C=C, rpr=rpr, act=d["act"], rb=d["rb"])
        sc = 8.0 if d["data"] == "wide" else 1.0
        _input(b, "x", torch.randn(rows * C, generator=g) * sc, fill)
        if d["rb"]:
            _input(b, "rb", torch.randn(-(-rows // rpr) * C, generator=g), fill)
        _output(b, "y", rows * C)
        return b
    if e == "act_bwd":
        n = d["n"]
        sp.update(n=n, act=d["act"])
        v = torch.randn(n, generator=g).double() * 2
        _input(b, "y", (torch.tanh(v) if d["act"] == 1 else torch.sigmoid(v)).float(), fill)
        _input(b, "dy", torch.randn(n, generator=g), fill)
        _output(b, "dx", n)
        return b
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------
def run(mod, b, tensors, entry=None):
    """The case's call on `mod` (wesep_amd.dev) over `tensors` (the allocations on the device)."""
    e, sp, v = entry or b.case.entry, b.spec, b.views(tensors)
    if e == "im2col":
        mod.im2col_hw(v["x"], sp["R"], sp["H"], sp["W"], sp["C"], sp["k"], sp["sh"], sp["sw"], sp["p"], v["patches"], sp["ldp"])
    elif e == "col2im":
        mod.col2im_hw(v["dpatches"], sp["R"], sp["H"], sp["W"], sp["C"], sp["k"], sp["sh"], sp["sw"], sp["p"], v["dx"])
    elif e == "elu_fwd":
        mod.elu_fwd(v["x"][:sp["n"]], v["y"])
    elif e == "elu_bwd":
        mod.elu_bwd(v["x"][:sp["n"]], v["dy"], v["dx"])
    elif e == "inorm_finalize":
        mod.inorm_finalize(v["sums"], sp["G"], sp["C"], sp["P"], v["stats"], sp["eps"])
    elif e == "inorm_apply":
        mod.inorm_apply(v["x"], v["stats"], sp["G"] * sp["P"], sp["P"], sp["C"], v["y"])
    elif e == "inorm_bwd_apply":
        mod.inorm_bwd_apply(v["y"], v["dy"], v["stats"], v["sums"], sp["G"] * sp["P"], sp["P"], sp["C"], v["dx"])
    elif e == "in_act_sums":
        mod.in_act_sums(v["x"], v.get("dy"), v.get("stats"), sp["G"], sp["P"], sp["C"], sp["flags"], sp["nsplit"], v["slab"],
                        sp.get("ldd_arg", 0), sp.get("dy_off", 0))
    elif e == "in_act_apply":
        mod.in_act_apply(v["x"], v["stats"], sp["G"] * sp["P"], sp["P"], sp["C"], sp["flags"], v["y"], sp["ldy_arg"], sp["y_off"])
    elif e == "in_act_bwd_apply":
        mod.in_act_bwd_apply(v["x"], v["dy"], v["stats"], v["sums"], sp["G"] * sp["P"], sp["P"], sp["C"], sp["flags"], v["dx"],
                             sp["ldd_arg"], sp["dy_off"], sp["lddx_arg"], sp["dx_off"])
    elif e == "avgpool_fwd":
        mod.avgpool_fwd(v["x"], sp["B"], sp["H"], sp["W"], sp["C"], sp["sz"], v["y"])
    elif e == "avgpool_bwd":
        mod.avgpool_bwd(v["dy"], sp["B"], sp["H"], sp["W"], sp["C"], sp["sz"], v["dx"])
    elif e == "bilinear_fwd":
        mod.bilinear_fwd(v["x"], sp["B"], sp["h"], sp["w"], sp["H"], sp["W"], sp["C"], v["y"])
    elif e == "bilinear_bwd":
        mod.bilinear_bwd(v["dy"], sp["B"], sp["h"], sp["w"], sp["H"], sp["W"], sp["C"], v["dx"], tmp=v["tmp"])
    elif e == "scale_bf_fwd":
        mod.scale_bf_fwd(v["x"], v["s"], sp["B"], sp["T"], sp["F"], sp["C"], sp["mode"], v["y"])
    elif e == "scale_bf_bwd":
        mod.scale_bf_bwd(v["x"], v["dy"], v["s"], sp["B"], sp["T"], sp["F"], sp["C"], sp["mode"], v["dx"], v["ds"])
    elif e == "freq_linear":
        mod.freq_linear_fwd(v["x"], v["W"], sp["ldw"], v["rb"], sp["B"], sp["T"], sp["F"], sp["C"], v["y"])
    elif e == "softmax_fwd":
        mod.softmax_rows_fwd(v["x"], sp["rows"], sp["n"], sp["scale"], v["y"])
    elif e == "softmax_bwd":
        mod.softmax_rows_bwd(v["y"], v["dy"], sp["rows"], sp["n"], sp["scale"], v["dx"])
    elif e == "rowbias_act":
        mod.rowbias_act_fwd(v["x"], v.get("rb"), sp["rows"], sp["C"], sp["rpr"], sp["act"], v["y"])
    elif e == "act_bwd":
        mod.act_bwd(v["y"][:sp["n"]], v["dy"], sp["act"], v["dx"])
    else:
        raise ValueError(e)
    return {}


def refusals(dev, t):
    """(name, call): argument sets the library refuses; every call has to come back WS_ERR_INVALID without launching."""
    return [
        ("im2col C % 4", lambda: dev.im2col_hw(t, 1, 5, 5, 6, 3, 1, 1, 1, t, 54)),
        ("im2col ldp < k*k", lambda: dev.im2col_hw(t, 1, 5, 5, 1, 3, 1, 1, 1, t, 8)),
        ("im2col ldp != k*k*C", lambda: dev.im2col_hw(t, 1, 5, 5, 4, 3, 1, 1, 1, t, 40)),
        ("im2col empty output", lambda: dev.im2col_hw(t, 1, 2, 5, 4, 5, 1, 1, 0, t, 100)),
        ("col2im C = 1", lambda: dev.col2im_hw(t, 1, 5, 5, 1, 3, 1, 1, 1, t)),
        ("col2im C % 4", lambda: dev.col2im_hw(t, 1, 5, 5, 6, 3, 1, 1, 1, t)),
        ("elu_fwd n % 4", lambda: dev.elu_fwd(t[:6], t)),
        ("inorm_apply C % 4", lambda: dev.inorm_apply(t, t, 8, 4, 6, t)),
        ("inorm_apply rows % P", lambda: dev.inorm_apply(t, t, 9, 4, 8, t)),
        ("inorm_bwd_apply rows % P", lambda: dev.inorm_bwd_apply(t, t, t, t, 9, 4, 8, t)),
        ("in_act_sums flags = 4", lambda: dev.in_act_sums(t, None, None, 2, 4, 8, 4, 1, t)),
        ("in_act_sums C % 4", lambda: dev.in_act_sums(t, None, None, 2, 4, 6, 0, 1, t)),
        ("in_act_sums backward without stats", lambda: dev.in_act_sums(t, t, None, 2, 4, 8, 0, 1, t)),
        ("in_act_sums ldd < C", lambda: dev.in_act_sums(t, t, t, 2, 4, 8, 0, 1, t, 4)),
        ("in_act_sums ldd % 4", lambda: dev.in_act_sums(t, t, t, 2, 4, 8, 0, 1, t, 10)),
        ("in_act_apply flags = -1", lambda: dev.in_act_apply(t, t, 8, 4, 8, -1, t)),
        ("in_act_apply ldy < C", lambda: dev.in_act_apply(t, t, 8, 4, 8, 0, t, 4)),
        ("in_act_apply ldy % 4", lambda: dev.in_act_apply(t, t, 8, 4, 8, 0, t, 10)),
        ("in_act_apply rows % P", lambda: dev.in_act_apply(t, t, 9, 4, 8, 0, t)),
        ("in_act_bwd_apply lddx % 4", lambda: dev.in_act_bwd_apply(t, t, t, t, 8, 4, 8, 0, t, 0, 0, 10)),
        ("in_act_bwd_apply ldd < C", lambda: dev.in_act_bwd_apply(t, t, t, t, 8, 4, 8, 0, t, 4)),
        ("in_act_bwd_apply flags = 7", lambda: dev.in_act_bwd_apply(t, t, t, t, 8, 4, 8, 7, t)),
        ("avgpool_fwd H < sz", lambda: dev.avgpool_fwd(t, 1, 2, 5, 4, 3, t)),
        ("avgpool_bwd W < sz", lambda: dev.avgpool_bwd(t, 1, 5, 2, 4, 3, t)),
        ("avgpool_fwd C % 4", lambda: dev.avgpool_fwd(t, 1, 4, 4, 6, 2, t)),
        ("bilinear_fwd C % 4", lambda: dev.bilinear_fwd(t, 1, 2, 2, 4, 4, 6, t)),
        ("bilinear_bwd C % 4", lambda: dev.bilinear_bwd(t, 1, 2, 2, 4, 4, 6, t, tmp=t)),
        ("scale_bf_fwd C % 4", lambda: dev.scale_bf_fwd(t, t, 1, 2, 2, 6, 0, t)),
        ("scale_bf_fwd mode = 2", lambda: dev.scale_bf_fwd(t, t, 1, 2, 2, 8, 2, t)),
        ("scale_bf_bwd mode = 2", lambda: dev.scale_bf_bwd(t, t, t, 1, 2, 2, 8, 2, t, t)),
        ("freq_linear F*C > 16384", lambda: dev.freq_linear_fwd(t, t, 65, t, 1, 1, 65, 256, t)),
        ("freq_linear ldw < F", lambda: dev.freq_linear_fwd(t, t, 4, t, 1, 1, 5, 8, t)),
        ("freq_linear C % 4", lambda: dev.freq_linear_fwd(t, t, 5, t, 1, 1, 5, 6, t)),
        ("softmax_rows_fwd n = 0", lambda: dev.softmax_rows_fwd(t, 2, 0, 1.0, t)),
        ("rowbias_act act = 2", lambda: dev.rowbias_act_fwd(t, None, 4, 4, 1, 2, t)),
        ("act_bwd act = 0", lambda: dev.act_bwd(t[:8], t, 0, t)),
    ]


# ------------------------------------------------------------------------------------------------------------
# checker, emulation
# ------------------------------------------------------------------------------------------------------------
SCRATCH = ("tmp",)          # outputs the contract calls scratch: written inside their extent, never outside


def verify(b, ref, after, what=None):
    """Every output of a built case (`after`: name -> whole CPU allocation after the launch) against `ref`; scratch buffers
    keep their guards.  Returns the worst err / bound.  Raises ContractViolation: nan | exact | bound | sentinel."""
    what = what or f"{b.case.entry} {b.case.name}"
    worst = 0.0
    for key, r in ref.items():
        name = b.alias.get(key, key)
        if isinstance(r, Partial):
            worst = max(worst, check_partial(after[name], b.bufs[name], r, f"{what} {key}", b.start[name]))
        else:
            worst = max(worst, check(after[name], b.bufs[name], r, f"{what} {key}", b.start[name]))
    for name in b.outs:
        if name in SCRATCH:
            a, o = after[name], b.bufs[name]
            w = torch.isnan(o)
            if not torch.equal(a[~w].view(torch.int32), o[~w].view(torch.int32)):
                raise ContractViolation("sentinel", f"{what}: the scratch {name} was written outside its extent")
    return worst


def output_bits(b, after):
    """The bits of every output (scratch excepted)."""
    parts = []
    for n in b.outs:
        if n in SCRATCH:
            continue
        t = after[n]
        if n in b.alias.values():
            t = t[b.wset]
        parts.append(t.contiguous().view(torch.int32).reshape(-1))
    return torch.cat(parts)


def _place(b, ref, vals):
    """(after) the allocations with `vals` (name -> values in the order of the reference's idx) written."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    for key, r in ref.items():
        name = b.alias.get(key, key)
        if isinstance(r, Partial):
            after[name][r.rows.reshape(-1) + b.start[name]] = vals[key].reshape(-1).float()
        else:
            after[name][r.idx + b.start[name]] = vals[key].reshape(-1).float()
    for name in b.outs:
        if name in SCRATCH:
            after[name][torch.isnan(after[name])] = 0.0
    return after


def perfect(b, ref):
    """What a correctly rounding kernel leaves: the fp32 rounding of the float64 values."""
    return _place(b, ref, compute(b.case.entry, b.spec, b.views(b.bufs), F64))


def emulate(b, ref, order="seq", defect=None):
    """What a correct fp32 kernel (sums in `order`) leaves -- or one with the planted `defect`."""
    return _place(b, ref, compute(b.case.entry, b.spec, b.views(b.bufs), F32, order, defect))


DEFECTS = {
    "im2col": ["taps_transposed", "stride_swapped", "pad_off_by_one"],
    "col2im": ["taps_transposed", "stride_swapped", "pad_off_by_one", "no_ho_test"],
    "avgpool_bwd": ["tail_not_zero"],
    "bilinear_fwd": ["align_corners", "no_clamp"],
    "bilinear_bwd": ["align_corners", "no_clamp", "window_narrow"],
    "inorm_finalize": ["unbiased", "eps_outside"],
    "in_act_sums": ["flags_swapped", "elud_of_x", "ragged_last_row_dropped"],
    "in_act_apply": ["flags_swapped"],
    "in_act_bwd_apply": ["flags_swapped", "elud_of_x"],
    "scale_bf_fwd": ["s_indexed_bt"],
    "scale_bf_bwd": ["s_indexed_bt", "second_row_missing"],
    "freq_linear": ["W_transposed", "rb_indexed_t"],
    "softmax_fwd": ["no_max", "scale_after_max"],
    "softmax_bwd": ["bwd_no_scale"],
}
