"""TEST INFRASTRUCTURE ONLY -- contract suite of the kernels that make the loss, the first gradient and the weights of a training
step (wesep_amd/csrc/elementwise.hip: ws_affine_fwd / bwd, ws_sisdr_fwd / bwd, ws_grad_norms, ws_clip_adam_step,
ws_guard_commit), of the TF-GridNet attention heads (heads.hip: ws_heads_fwd / bwd) and of ws_tstp_bwd (conv2d.hip).  Same shape
as tests/tasnet_contract.py: Ref, check, eps_for, the guards and the pairwise generator with its registries come from
tests/gemm_contract.py, Partial / check_partial / sum32 from tests/norm_contract.py, the builders of guarded operands from
tests/map_contract.py.  No GPU code here: test_step_contract_host_cpu.py checks this module, test_step_contract_gpu.py runs every
case through wesep_amd.dev.

1. REFERENCE.  compute(entry, spec, tensors, dtype, order, defect) restates include/wesep_hip.h as explicit index arithmetic.  In
   float64 it is the reference, in float32 (sums sequential or pairwise) the emulation of a correct kernel, with `defect` a
   planted defect.  m = r rows_per_r + j:
     affine_fwd   out[m][n] = fma(z[m][n], a0 + a[r][n], b[r][n]) (a / b NULL: 0)
     affine_bwd   dz_in = dz (a0 + a);  da_slab[s][r][n] = sum over the rows j in [s chunk, min(rows_per_r, (s + 1) chunk)) of
                  dz z_in, chunk = ceil(rows_per_r / nsplit); db_slab likewise of dz;  da / db = the slabs summed over s
     sisdr_fwd    three passes per row: means; sxt = sum xc tc, stt = sum tc tc around them, alpha = sxt / (stt + eps); srr = sum
                  res res, srt = sum res tc, res = xc - alpha tc.  A = alpha^2 stt, ratio = A / (srr + eps), sisdr_dB = 10 log10(ratio
                  + eps), k = 10 / ln 10 / (ratio + eps), dLdA = -k / (srr + eps), dLdB = k A / (srr + eps)^2, dalpha = 1 / (stt + eps),
                  c1 = 2 dLdA alpha stt dalpha - 2 dLdB srt dalpha, c2 = 2 dLdB;  rowstat = (mean_x, mean_t, alpha, c1, c2,
                  sisdr_dB, 0, 0);  loss = -sum_r sisdr_dB / R
     sisdr_bwd    dest = gout / R (c1 tc + c2 (xc - alpha tc)) from the uploaded rowstat
     grad_norms   norms[i] = sqrt(sum g^2) (grad NULL: exactly 0); guard[0] = 1 when a norm is not finite
     clip_adam    coef = clip / (norm + 1e-6) when clip > 0 and that is < 1, else 1 (in fp32, from the uploaded fp32 norm);
                  g = grad coef (stored when coef != 1); unless clip_only: g += wd p, m = b1 m + (1 - b1) g, v = b2 v + (1 - b2) g g,
                  p -= lr / bc1 (m / (sqrt(v) / bc2_sqrt + eps)), bc1 = 1 - b1^s, bc2_sqrt = sqrt(1 - b2^s), s = step, or
                  max(step - *step_lag, 1) when a lag word is given.  Nothing is written when a skip word is non-zero
     guard_commit skipped := guard[0] != 0 || (skip1 && *skip1 != 0): ++guard[1], ++guard[2], ++guard[3]; else guard[2] = 0
     heads_fwd    u = PReLU(x[(b T + t) Q + q][off + h ch + e]; slope[h]); mean / biased variance over the Q ch elements of
                  (b, t, h), two passes; y[(h B + b) Tp + t][q ch + e] = gamma[h] ((u - mean) rstd) + beta[h]; rows t in [T, Tp): 0
     heads_bwd    d = dy gamma, n = (u - mean) rstd, dl = rstd (d - mean(d) - n mean(d n)), dx = x > 0 ? dl : slope dl; slab row
                  of workgroup i = sums over its rows i, i + nwg, .. of (dy n | dy | per head: dl x where x <= 0 | zeros)
     tstp_bwd     dx[r][f][t][c] = dmean / T + dstd (x - mean) / ((T - 1) std), T = 1: dmean;  feature index c F + f
   Backward entries TAKE their forward quantities (rowstat, stats, norms): uploaded as the fp32 rounding of the float64 values,
   and the reference computes from exactly those fp32 numbers, so every entry is judged on its own.  The composed chains
   (test_step_contract_gpu.py) feed a stage the device output of the one before.

2. BOUNDS.  Per element, derived; u = 2^-24, e(n) = eps_for(False, n) = (n + 8) u applied to the same expression over absolute
   values (S).  The build has no fast-math flag, so +, *, /, sqrtf round correctly; the compiler may contract a * b + c into one
   fma, which removes a rounding and never adds one, so every count below is an upper count.  A path of r <= 7 roundings is
   inside e(0) = 8 u.
     bit-exact    affine_fwd (ONE fma: the float64 product is exact, the sum is rounded once -- _fma32 resolves the double
                  rounding); guard_commit and every guard / counter word (integers); everything a skipped launch, a clip_only
                  launch (param, moments), a NULL-grad entry or coef == 1 (grad) must leave untouched; the rows t in [T, Tp) of
                  heads_fwd; slab rows of workgroups and splits that own nothing, the pad words of a heads slab row; the columns of
                  dx outside [off, off + nh ch) (sentinels); tstp_bwd at T = 1 (dmean / 1)
     affine_bwd   dz_in: u |dz_in| + u |dz| |a0 + a| (the product; the rounding of a0 + a, absent without a).  Slabs as Partial
                  sums over the splits: da e(rows_per_r + 1) sum |dz z|, db e(rows_per_r) sum |dz|;  da / db: + e(nsplit) S
     sisdr_fwd    carried through the three passes the way norm_contract carries rstd, every quantity an interval (Iv):
                  (1) means: d_m = e(T) E|.|;  (2) the centred sums are taken around the kernel's own means, and exactly
                  sum (x - mx')(t - mt') = sxt + T (mx - mx')(mt - mt'): d_sxt = e(T + 3) sum (|xc| + d_mx)(|tc| + d_mt) + T d_mx
                  d_mt, d_stt likewise;  (3) alpha = sxt / (stt + eps) as the interval of the four corners, two roundings;
                  (4) with c = (mx - mx') + alpha' (mt' - mt) and da = alpha' - alpha the kernel's residual is res + c - da tc, and
                  since sum res = sum tc = 0: sum res'^2 = srr - 2 da srt + T c^2 + da^2 stt and sum res' tc' = srt - da stt - T c
                  (mt' - mt), exactly; the roundings of res' (four, relative to |xc| + |alpha tc|) and of the sums (e(T + 1)) on top;
                  (5) A, ratio, sisdr_dB, k, dLdA, dLdB, dalpha, c1, c2 in interval arithmetic, one relative u per operation.
                  log10f / logf: ULP_LOG = 3 ulp, the log / log10 row of the OpenCL full-profile table tests/map_contract.py
                  names for expf (ULP_EXP); one ulp is at most 2 u relative: D_LOG = 6 u of |log|.  val = the interval's midpoint,
                  bound = its half width.  loss: sum_r d_r / R + e(R + 1) sum |sisdr_dB| / R
     sisdr_bwd    e(0) S, S = |go| (|c1 tc| + |c2| (|xc| + |alpha tc|)): seven roundings on the longest path (go, tc, alpha tc, res,
                  c2 res, the sum, the product)
     grad_norms   s' = s (1 +- e(numel + 1)), n' = sqrtf(s') (1 +- u): n (1 - sqrt(1 - e)) + u n.  The guard word is 1 exactly when
                  the norm cannot be finite (a NaN or Inf planted, squares that overflow fp32 one by one); a word that was 0 stays 0
                  on finite input; a preset non-zero word is never reset
     clip_adam    grad (coef != 1): u |g|.  d_g2 = d_g + u |wd p| + u |g2| (wd = 0: d_g);  exp_avg: (1 - b1) d_g2 + 4 u (|b1 m| +
                  |(1 - b1) g2|) (b1 m, 1 - b1, its product, the sum);  exp_avg_sq: (1 - b2)(2 |g2| d_g2 + d_g2^2) + 5 u (|b2 v| +
                  (1 - b2) g2^2);  sqrtf(v): the interval sqrt(v +- d_v) + u;  denom = sqrt / bc2_sqrt + eps: two roundings;  m /
                  denom: (d_m + |q| d_den) / (den - d_den) + u |q|;  step_size = lr / bc1: one rounding;  param: step_size d_q +
                  |step_size q| (2 u + rho1) + u |p'|.  bc1 / bc2_sqrt are the float rounding of a double expression: the host's
                  (exact here); with step_lag given they come from the device's double pow: one fp32 ulp (rho = 2 u) on each
     heads_fwd    statistics as norm_contract.stats_interval (two-pass, the variance around the kernel's mean), with PReLU's
                  product on top: the data are off by u |u| each, which moves the mean by at most u E|u| and the standard deviation
                  by at most u rms(u) (triangle inequality on the centred vectors);  y as rowln_fwd: |gamma| (d_m hi + |u - m| d_r +
                  hi u |u|) + e(0) (|gamma (u - m)| rstd + |beta|)
     heads_bwd    dl as rowln_bwd: e(0) S + |rstd| e(D) (E|d| + |n| E|d n|), S = |rstd| (|d| + |E d| + |n E(d n)|); dx = slope dl: |slope|
                  times that + u |dx|.  dgamma (e(B T + 1) + 3 u) sum |dy n|, dbeta e(B T) sum |dy|, dslope e(B T D + 1) sum |dl x| +
                  sum d_dl |x|, each a Partial over the nwg slab rows; the wrapper's sums + e(nwg) S
     tstp_bwd     e(0) S, S = |dmean| / T + |dstd (x - mean)| / ((T - 1) std)

3. CONDITION OF THE SUITE.  Such bounds see a dropped or misplaced addend only while it weighs enough in its sum.  Gauss and
   offset data stay at sums of at most CAP = 2048 leaves.  Longer rows exist only to cross a loop seam (T = 2049 and 4100 for the
   1024-thread passes, numel 4097 and 9000 for Adam's stride, numel 5000 for the norm loop) and carry a structural spike: the last
   element x1e3.  For the ordinary SI-SDR regimes (-5, 10, 30 dB at T <= 2048) the derived bound on sisdr_dB stays below 1e-2 dB,
   the tolerance tests/test_kernels_gpu.py names: test_step_contract_host_cpu.py asserts it, so the bound cannot become vacuous.
   The ill-conditioned regimes (estimate within 60 dB of alpha t, constant target, constant estimate, DC offset 10 x the signal,
   eps = 1e-3) are judged for finiteness and the bound only: no planted defect relies on them.

4. CASES.  cases(entry): gemm_contract's pairwise generator over DIMS, topped up so that every dispatch target of INST gets
   MIN_PER_TARGET cases, plus EXTRA: one affine_fwd case of just over 4 194 304 quads (the 16384-block grid cap).

BUFFERS.  GUARD floats on both sides of every operand and output.  Write sets start as NaN, an output that aliases an operand (out
over z, the optimizer's four tensors) starts as that operand; everything else in an output allocation holds SENT and must be
bit-identical afterwards.  Inputs: everything the contract does not read is NaN (the columns outside a strided x, a NULL-grad
entry's gradient); build(case, garbage=True) puts a large finite value there.  Guard, skip, lag and counter words are int32
tensors that run() makes and hands back (as floats: small integers); the heads slab belongs to the wrapper, which hands it back."""
import math

import torch

from tests import gemm_contract as gc
from tests import map_contract as mc
from tests import norm_contract as nc  # noqa: F401
from tests import tasnet_contract as tc
from tests.gemm_contract import (GUARD, SENT, U, Buf, Built, Case, ContractViolation, Ref, check, eps_for)  # noqa: F401
from tests.norm_contract import Partial, check_partial, stats_interval, sum32  # noqa: F401
from tests.tasnet_contract import TBuilt, _ew, _f32, _ones, _red_ref, _slab_ref, _split_sums, _spiked

GARBAGE, NAN, CAP, TINY = mc.GARBAGE, mc.NAN, 2048, mc.TINY
F64, F32 = torch.float64, torch.float32
ULP_EXP, ULP_LOG = mc.ULP_EXP, 3
D_LOG = 2 * ULP_LOG * U
LN_EPS, TSTP_EPS = 1e-5, 1e-7
ORDERS = ("seq", "pairwise")
E0 = eps_for(False, 0)
HD_PAD = 8
ENTRIES = ("affine_fwd", "affine_bwd", "sisdr_fwd", "sisdr_bwd", "grad_norms", "clip_adam_step", "guard_commit", "heads_fwd",
           "heads_bwd", "tstp_bwd")
_ar, _ref, _sum = mc._ar, mc._ref, mc._sum
ORDINARY = ("-5dB", "10dB", "30dB")
ILL = ("near", "const_t", "const_x", "dc10", "eps1e-3")
SISDR_TOL_DB = 1e-2


def _fma32(z, s, b):
    """fp32 fma(z, s, b) of fp32 values held in float64: the product is exact in float64; where the float64 sum lands on an fp32
    tie although the real sum does not, the discarded part decides."""
    p = z * s
    s64 = p + b
    bb = s64 - p
    err = (p - (s64 - bb)) + (b - bb)          # TwoSum: p + b = s64 + err exactly
    r = s64.float()
    rd = r.double()
    other = torch.where(s64 > rd, torch.nextafter(r, torch.full_like(r, math.inf)), torch.nextafter(r, torch.full_like(r, -math.inf))).double()
    tie = (s64 != rd) & ((s64 - rd).abs() == (other - s64).abs()) & (err != 0) & torch.isfinite(other)
    up = torch.maximum(rd, other)
    dn = torch.minimum(rd, other)
    return torch.where(tie, torch.where(err > 0, up, dn), rd)


class Iv:
    """Elementwise interval [lo, hi] of float64 tensors; rnd(n): n roundings of relative u each."""
    def __init__(self, lo, hi):
        lo, hi = torch.as_tensor(lo, dtype=F64), torch.as_tensor(hi, dtype=F64)
        self.lo, self.hi = torch.minimum(lo, hi), torch.maximum(lo, hi)

    @staticmethod
    def pt(v, d=0.0):
        v = torch.as_tensor(v, dtype=F64)
        return Iv(v - d, v + d)

    def mag(self):
        return torch.maximum(self.lo.abs(), self.hi.abs())

    def rnd(self, n=1):
        w = n * U * self.mag() + TINY
        return Iv(self.lo - w, self.hi + w)

    def rel(self, r):
        w = r * self.mag()
        return Iv(self.lo - w, self.hi + w)

    def pos(self):
        return Iv(self.lo.clamp_min(0), self.hi.clamp_min(0))

    def __neg__(self):
        return Iv(-self.hi, -self.lo)

    def __add__(self, o):
        o = o if isinstance(o, Iv) else Iv.pt(o)
        return Iv(self.lo + o.lo, self.hi + o.hi)

    def __sub__(self, o):
        o = o if isinstance(o, Iv) else Iv.pt(o)
        return Iv(self.lo - o.hi, self.hi - o.lo)

    def _corners(self, o, fn):
        c = torch.stack([fn(self.lo, o.lo), fn(self.lo, o.hi), fn(self.hi, o.lo), fn(self.hi, o.hi)])
        return Iv(c.min(0).values, c.max(0).values)

    def __mul__(self, o):
        o = o if isinstance(o, Iv) else Iv.pt(o)
        return self._corners(o, lambda a, b: a * b)

    def __truediv__(self, o):
        o = o if isinstance(o, Iv) else Iv.pt(o)
        assert bool((o.lo > 0).all()), "interval division: the denominator is not positive"
        return self._corners(o, lambda a, b: a / b)

    def mid(self):
        return (self.lo + self.hi) / 2

    def rad(self):
        return (self.hi - self.lo) / 2


# ------------------------------------------------------------------------------------------------------------
# index arithmetic and pieces shared by compute and reference
# ------------------------------------------------------------------------------------------------------------
def ab_chunk(sp):
    return -(-sp["rpr"] // sp["nsplit"])


def _ab_rows(sp, defect=None):
    """(slab row s R + r of every row m [M], weight [M]) of affine_bwd's splits, with the planted split defects."""
    R, rpr, ns = sp["R"], sp["rpr"], sp["nsplit"]
    chunk = ab_chunk(sp)
    m = _ar(R * rpr)
    r, j = m // rpr, m % rpr
    s = j // chunk
    wgt = torch.ones(R * rpr, dtype=F64)
    if defect == "last_row_dropped":
        wgt[(j % chunk == chunk - 1) | (j == rpr - 1)] = 0.0
    if defect == "two_row_twice" and sp["N"] % 4 == 0:
        wgt[((j - s * chunk) % 16) >= 8] = 2.0
    return s * R + r, wgt


def _hd(sp):
    B, T, Tp, Q, nh, ch = (sp[k] for k in ("B", "T", "Tp", "Q", "nh", "ch"))
    return B, T, Tp, Q, nh, ch, nh * ch, Q * nh * ch, Q * ch


def _hd_x(sp, t, dt):
    """x as [B, T, Q, nh, ch] from the columns [x_off, x_off + nh ch) of rows of stride ldx."""
    B, T, _, Q, nh, ch, HC, _, _ = _hd(sp)
    rows = B * T * Q
    idx = _ar(rows)[:, None] * sp["ldx"] + sp["x_off"] + _ar(HC)[None, :]
    return t["x"][idx].to(dt).reshape(B, T, Q, nh, ch)


def _hd_par(sp, t, key, dt):
    """gamma / beta [nh, Q ch] as [1, 1, Q, nh, ch]."""
    _, _, _, Q, nh, ch, _, _, D = _hd(sp)
    return t[key][:nh * D].to(dt).reshape(nh, Q, ch).permute(1, 0, 2)[None, None]


def _hd_slope(sp, t, dt, defect=None):
    nh = sp["nh"]
    a = t["slope"][:nh].to(dt)
    if defect == "slope_of_head0":
        a = a[:1].expand(nh)
    return a.reshape(1, 1, 1, nh, 1)


def _hd_groups(v, sp):
    """[B, T, Q, nh, ch] -> [(b, t, h), Q ch]"""
    B, T, _, Q, nh, ch, _, _, D = _hd(sp)
    return v.permute(0, 1, 3, 2, 4).reshape(B * T * nh, D)


def _hd_ungroup(s, sp):
    """[(b, t, h)] -> [B, T, 1, nh, 1]"""
    B, T, _, _, nh, _, _, _, _ = _hd(sp)
    return s.reshape(B, T, 1, nh, 1)


def _hd_stats_in(sp, t, dt):
    """The uploaded stats[h][b T + t][2] as (mean, rstd) [B, T, 1, nh, 1]."""
    B, T, _, _, nh, _, _, _, _ = _hd(sp)
    st = t["stats"][:nh * B * T * 2].to(dt).reshape(nh, B, T, 2).permute(1, 2, 0, 3)
    return st[..., 0][:, :, None, :, None], st[..., 1][:, :, None, :, None]


def _adam_scalars(sp, defect=None):
    """(bc1, bc2_sqrt) as the fp32 values the kernel divides by, and whether they come from the device's pow."""
    b1, b2 = float(_f32(sp["beta1"])), float(_f32(sp["beta2"]))
    lag = sp["lag"]
    dev_pow = lag is not None and not sp["clip_only"]
    step = sp["step"]
    if dev_pow and defect != "lag_ignored":
        step = step - lag if defect == "lag_not_clamped" else max(step - lag, 1)
    bc1 = 1.0 - b1 ** step if step > 0 else 0.0
    bc2 = 1.0 - b2 ** step if step > 0 else 0.0
    bc2s = bc2 if defect == "bc2_not_sqrt" else math.sqrt(bc2)
    return float(_f32(bc1)), float(_f32(bc2s)), dev_pow


def _skipped(sp, defect=None):
    return (sp["skip0"] not in (None, 0)) or (sp["skip1"] not in (None, 0) and defect != "skip1_ignored")


def _coef32(sp, i, t, defect=None):
    """The clip coefficient of tensor i in fp32 arithmetic, from the uploaded norm."""
    if not sp["clip"] > 0:
        return 1.0
    c = torch.tensor(sp["clip"], dtype=F32) / (t["norms"][i].float() + torch.tensor(1e-6, dtype=F32))
    return float(c) if (float(c) < 1.0 or defect == "clip_when_coef_ge_1") else 1.0


def _tstp_idx(sp, defect=None):
    """The stats index c F + f of every element of x [R][F][T][C]."""
    R, Fq, T, C = sp["R"], sp["F"], sp["T"], sp["C"]
    i = _ar(R * Fq * T * C)
    c, q = i % C, i // C // T
    f, r = q % Fq, q // Fq
    o = r * 2 * C * Fq + (f * C + c if defect == "feature_f_major" else c * Fq + f)
    return o, o + C * Fq


# ------------------------------------------------------------------------------------------------------------
# compute: the header's formulas, in `dt` (float64: the reference; float32: the emulation), with planted defects
# ------------------------------------------------------------------------------------------------------------
def _sisdr_rows(sp, t, dt, order, defect=None):
    R, T = sp["R"], sp["T"]
    x, tg = t["est"][:R * T].reshape(R, T).to(dt), t["tgt"][:R * T].reshape(R, T).to(dt)
    eps = _f32(sp["eps"], dt)
    keep = torch.ones(T, dtype=dt)
    if defect == "last_lane_dropped" and T % 1024:
        keep[T - 1] = 0
    mx, mt = _sum(x * keep, order) / T, _sum(tg * keep, order) / T
    if defect == "mean_not_subtracted":
        mx, mt = torch.zeros_like(mx), torch.zeros_like(mt)
    xc, tcn = x - mx[:, None], tg - mt[:, None]
    sxt, stt = _sum(xc * tcn * keep, order), _sum(tcn * tcn * keep, order)
    alpha = sxt / (stt + eps)
    res = xc - alpha[:, None] * tcn
    srr, srt = _sum(res * res * keep, order), _sum(res * tcn * keep, order)
    A = alpha * alpha * stt
    ratio = A / (srr + eps)
    val = 10 * torch.log10(ratio + eps)
    k = torch.tensor(10.0, dtype=dt) / torch.log(torch.tensor(10.0, dtype=dt)) / (ratio + eps)
    dLdA = -k / (srr + eps)
    dLdB = k * A / ((srr + eps) * (srr + eps))
    dalpha = 1 / (stt + eps)
    c1 = dLdA * 2 * alpha * stt * dalpha - dLdB * 2 * srt * dalpha
    c2 = dLdB if defect == "c2_not_doubled" else dLdB * 2
    z = torch.zeros_like(mx)
    return torch.stack([mx, mt, alpha, c1, c2, val, z, z], 1)


def compute(entry, sp, t, dt=F64, order="seq", defect=None):
    """name -> values of every output of `entry` (slabs as [nsplit, columns], word outputs as floats)."""
    e = entry
    zero = torch.zeros((), dtype=dt)
    if e == "affine_fwd":
        rows, N, rpr = sp["R"] * sp["rpr"], sp["N"], sp["rpr"]
        R = sp["R"]
        z = t["z"][:rows * N].reshape(rows, N).to(dt)
        r = _ar(rows) % R if defect == "r_by_mod" else _ar(rows) // rpr
        a = t["a"][:R * N].reshape(R, N).to(dt)[r] if sp["a"] else torch.zeros(rows, N, dtype=dt)
        bb = t["b"][:R * N].reshape(R, N).to(dt)[r] if sp["b"] else torch.zeros(rows, N, dtype=dt)
        a0 = zero if defect == "a0_dropped" else _f32(sp["a0"], dt)
        if dt == F64:
            return {"out": _fma32(z, (a0 + a).float().double(), bb)}
        return {"out": (z.double() * (a0 + a).double() + bb.double()).float()}
    if e == "affine_bwd":
        R, rpr, N, ns = sp["R"], sp["rpr"], sp["N"], sp["nsplit"]
        M = R * rpr
        dz = t["dz"][:M * N].reshape(M, N).to(dt)
        out = {}
        if sp["dz_in"]:
            a0 = zero if defect == "scale_without_a0" else _f32(sp["a0"], dt)
            scale = (a0 + t["a"][:R * N].reshape(R, N).to(dt))[_ar(M) // rpr] if sp["a"] else a0
            out["dz_in"] = dz * scale
        sid, wgt = _ab_rows(sp, defect)
        w = wgt.to(dt)[:, None]
        if sp["zin"]:
            out["da_slab"] = _split_sums(dz * t["z_in"][:M * N].reshape(M, N).to(dt) * w, sid, ns * R, dt, order).reshape(ns, R * N)
        out["db_slab"] = _split_sums(dz * w, sid, ns * R, dt, order).reshape(ns, R * N)
        if sp["dadb"]:
            lo = 1 if defect == "da_skips_split0" and ns > 1 else 0
            if sp["zin"]:
                out["da"] = _sum(out["da_slab"][lo:].t(), order)
            out["db"] = _sum(out["db_slab"][lo:].t(), order)
            out["counter"] = torch.zeros(R, dtype=dt)
        return out
    if e == "sisdr_fwd":
        R = sp["R"]
        rs = _sisdr_rows(sp, t, dt, order, defect)
        v = rs[:, 5]
        if defect == "mean_first_64_rows":
            v = v[:64]
        return {"rowstat": rs, "loss": (-_sum(v[None, :], order) / R).reshape(1)}
    if e == "sisdr_bwd":
        R, T = sp["R"], sp["T"]
        x, tg = t["est"][:R * T].reshape(R, T).to(dt), t["tgt"][:R * T].reshape(R, T).to(dt)
        rs = t["rowstat"][:R * 8].reshape(R, 8).to(dt)
        if defect == "rowstat_of_row0":
            rs = rs[:1].expand(R, 8)
        go = t["gout"][0].to(dt) if defect == "gout_not_divided" else t["gout"][0].to(dt) / R
        tcn = tg - rs[:, 1:2]
        res = (x - rs[:, 0:1]) - (tcn if defect == "alpha_dropped" else rs[:, 2:3] * tcn)
        return {"dest": go * (rs[:, 3:4] * tcn + rs[:, 4:5] * res)}
    if e == "grad_norms":
        out = []
        for i, n in enumerate(sp["numel"]):
            if i == sp["null"]:
                out.append(zero)
                continue
            g = t[f"g{i}"][:n].to(dt)
            if defect == "one_trip_of_1024":
                g = g[:1024]
            if defect == "last_dropped" and n > 1:
                g = g[:n - 1]
            out.append(torch.sqrt(_sum((g * g)[None, :], order))[0])
        bad = any(not math.isfinite(float(v)) for v in out) or sp["poison"] != "none"
        g0 = sp["guard"]
        res = {"norms": torch.stack(out)}
        if g0 is not None:
            res["guard"] = torch.tensor([1 if (bad and defect != "guard_never_set") else g0, 3, 2, 1], dtype=dt)
        return res
    if e == "clip_adam_step":
        out = {}
        skipped = _skipped(sp, defect)
        bc1, bc2s, _ = _adam_scalars(sp, defect)
        lr, b1, b2, eps, wd = (_f32(sp[k], dt) for k in ("lr", "beta1", "beta2", "eps", "wd"))
        for i, n in enumerate(sp["numel"]):
            p, m, v = (t[f"{k}{i}"][:n].to(dt) for k in "pmv")
            if i == sp["null"]:
                out.update({f"p{i}": p, f"m{i}": m, f"v{i}": v})
                continue
            g = t[f"g{i}"][:n].to(dt)
            if skipped:
                out.update({f"p{i}": p, f"g{i}": g, f"m{i}": m, f"v{i}": v})
                continue
            coef = _coef32(sp, i, t, defect)
            g = g * torch.tensor(coef, dtype=F32).to(dt)
            out[f"g{i}"] = g
            if sp["clip_only"]:
                out.update({f"p{i}": p, f"m{i}": m, f"v{i}": v})
                continue
            g2 = g if defect == "wd_after_moments" else g + wd * p
            m2 = b1 * m + (1 - b1) * g2
            v2 = b2 * v + (1 - b2) * g2 * g2
            denom = torch.sqrt(v2) / torch.tensor(bc2s, dtype=dt) + eps
            p2 = p - (lr / torch.tensor(bc1, dtype=dt)) * (m2 / denom)
            if defect == "wd_after_moments":
                p2 = p2 - lr * wd * p
            out.update({f"p{i}": p2, f"m{i}": m2, f"v{i}": v2})
        for k in ("skip0", "skip1", "lag"):
            if sp[k] is not None:
                out[k] = torch.tensor([sp[k]], dtype=dt)
        return out
    if e == "guard_commit":
        g = list(sp["guard"])
        out = {}
        for it in (1, 2):
            skipped = g[0] != 0 or (sp["skip1"] not in (None, 0) and defect != "skip1_ignored")
            if skipped:
                g = [g[0], g[1] + 1, g[2] + 1, g[3] + 1]
            elif defect != "consecutive_not_reset":
                g = [g[0], g[1], 0, g[3]]
            out[f"guard{it}"] = torch.tensor(g, dtype=dt)
        return out
    if e in ("heads_fwd", "heads_bwd"):
        B, T, Tp, Q, nh, ch, HC, W, D = _hd(sp)
        xx = _hd_x(sp, t, dt)
        a = _hd_slope(sp, t, dt, defect)
        u = torch.where(xx > 0, xx, a * xx)
        g = _hd_par(sp, t, "gamma", dt)
        if e == "heads_fwd":
            if defect == "stats_over_W":
                uu = u.reshape(B * T, W)
                mean = (_sum(uu, order) / W).reshape(B, T, 1, 1, 1).expand(B, T, 1, nh, 1)
                var = (_sum((uu - mean.reshape(B * T, nh)[:, :1]) ** 2, order) / W).reshape(B, T, 1, 1, 1).expand(B, T, 1, nh, 1)
            else:
                ug = _hd_groups(u, sp)
                mg = _sum(ug, order) / D
                mean = _hd_ungroup(mg, sp)
                var = _hd_ungroup(_sum((ug - mg[:, None]) ** 2, order) / D, sp)
            rstd = 1 / torch.sqrt(var + _f32(LN_EPS, dt))
            yy = g * ((u - mean) * rstd) + _hd_par(sp, t, "beta", dt)
            y = torch.full((nh, B, Tp, Q, ch), float("nan") if defect == "pad_unwritten" else 0.0, dtype=dt)
            y[:, :, :T] = yy.permute(3, 0, 1, 2, 4)
            st = torch.stack([mean.reshape(B * T, nh).t(), rstd.reshape(B * T, nh).t()], 2)
            return {"y": y, "stats": st}
        nwg = sp["nwg"]
        mean, rstd = _hd_stats_in(sp, t, dt)
        n = (u - mean) * rstd
        dd = t["dy"][:nh * B * Tp * D].to(dt).reshape(nh, B, Tp, Q, ch)[:, :, :T].permute(1, 2, 3, 0, 4)
        d = dd * g
        if defect == "mean_over_W":
            md = (_sum(d.reshape(B * T, W), order) / W).reshape(B, T, 1, 1, 1)
            mdn = (_sum((d * n).reshape(B * T, W), order) / W).reshape(B, T, 1, 1, 1)
        else:
            md = _hd_ungroup(_sum(_hd_groups(d, sp), order) / D, sp)
            mdn = _hd_ungroup(_sum(_hd_groups(d * n, sp), order) / D, sp)
        dl = rstd * (d - md - n * mdn)
        dx = torch.where(xx > 0, dl, a * dl)
        neg = (xx > 0) if defect == "dslope_over_pos" else ~(xx > 0)
        sl = _sum(_hd_groups(torch.where(neg, dl * xx, zero), sp), order).reshape(B * T, nh)          # the block sum of a row
        terms = torch.cat([(dd * n).reshape(B * T, W), dd.reshape(B * T, W), sl, torch.zeros(B * T, HD_PAD - nh, dtype=dt)], 1)
        if defect == "last_row_dropped":
            terms = terms.clone()
            terms[B * T - 1] = 0
        slab = _split_sums(terms, _ar(B * T) % nwg, nwg, dt, order)
        tot = _sum(slab.t(), order)
        perm = lambda v: v.reshape(Q, nh, ch).permute(1, 0, 2).reshape(nh, D)          # noqa: E731
        return {"dx": dx.reshape(B * T * Q, HC), "slab": slab, "dgamma": perm(tot[:W]), "dbeta": perm(tot[W:2 * W]), "dslope": tot[2 * W:2 * W + nh]}
    if e == "tstp_bwd":
        T = sp["T"]
        n = sp["R"] * sp["F"] * T * sp["C"]
        o0, o1 = _tstp_idx(sp, defect)
        x = t["x"][:n].to(dt)
        st, ds = t["stats"].to(dt), t["dstats"].to(dt)
        if T == 1:
            return {"dx": ds[o0] / 1}
        div = T if defect == "div_by_T" else T - 1
        return {"dx": ds[o0] / T + ds[o1] * (x - st[o0]) / (div * st[o1])}
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# reference = compute in float64 + the bounds of the module docstring
# ------------------------------------------------------------------------------------------------------------
def _exact(val, idx=None):
    return _ref(_ar(val.numel()) if idx is None else idx, val, val.abs(), torch.zeros_like(val), _ones(val))


def sisdr_intervals(sp, t):
    """name -> Iv [R] of the eight rowstat columns (the docstring's five steps)."""
    R, T = sp["R"], sp["T"]
    x, tg = t["est"][:R * T].reshape(R, T).double(), t["tgt"][:R * T].reshape(R, T).double()
    eps = float(_f32(sp["eps"]))
    mx, mt = x.mean(1), tg.mean(1)
    d_mx, d_mt = eps_for(False, T) * x.abs().mean(1), eps_for(False, T) * tg.abs().mean(1)
    xc, tcn = x - mx[:, None], tg - mt[:, None]
    axc, atc = xc.abs() + d_mx[:, None], tcn.abs() + d_mt[:, None]
    sxt, stt = (xc * tcn).sum(1), (tcn * tcn).sum(1)
    eT = eps_for(False, T + 3)
    sxt_i = Iv.pt(sxt, eT * (axc * atc).sum(1) + T * d_mx * d_mt)
    stt_i = Iv.pt(stt, eT * (atc * atc).sum(1) + T * d_mt * d_mt).pos()
    den = (stt_i + eps).rnd()
    alpha_i = (sxt_i / den).rnd()
    alpha = sxt / (stt + eps)
    d_a = torch.maximum((alpha_i.hi - alpha).abs(), (alpha_i.lo - alpha).abs())
    res = xc - alpha[:, None] * tcn
    srr, srt = (res * res).sum(1), (res * tcn).sum(1)
    am = alpha.abs() + d_a
    c = d_mx + am * d_mt
    # the roundings of one res' (x - mx', t - mt', alpha' tc', the difference) and the widest |res'|, |tc'|
    r_i = 4 * U * (axc + am[:, None] * atc)
    ares = res.abs() + c[:, None] + d_a[:, None] * tcn.abs()
    e1 = eps_for(False, T + 1)
    d_srr = 2 * d_a * srt.abs() + T * c * c + d_a * d_a * stt + (2 * ares * r_i + r_i * r_i).sum(1) + e1 * ((ares + r_i) ** 2).sum(1)
    d_srt = d_a * stt + T * c * d_mt + (r_i * atc + (ares + r_i) * U * atc).sum(1) + e1 * ((ares + r_i) * atc).sum(1)
    srr_i, srt_i = Iv.pt(srr, d_srr).pos(), Iv.pt(srt, d_srt)
    A = ((alpha_i * alpha_i).rnd() * stt_i).rnd().pos()
    Be = (srr_i + eps).rnd()
    ratio = (A / Be).rnd()
    re = (ratio + eps).rnd()
    lg = Iv(10 * torch.log10(re.lo), 10 * torch.log10(re.hi))
    val = lg.rel(D_LOG + U).rnd()
    kc = 10.0 / math.log(10.0)
    k = (Iv.pt(torch.full((R,), kc, dtype=F64), kc * (D_LOG + 2 * U)) / re).rnd()
    dLdA = (-(k / Be)).rnd()
    dLdB = ((k * A).rnd() / (Be * Be).rnd()).rnd()
    dal = (Iv.pt(torch.ones(R, dtype=F64)) / den).rnd()
    t1 = (((dLdA * alpha_i).rnd() * stt_i).rnd() * dal).rnd() * 2.0
    t2 = (((dLdB * srt_i).rnd()) * dal).rnd() * 2.0
    z = Iv.pt(torch.zeros(R, dtype=F64))
    return [Iv.pt(mx, d_mx), Iv.pt(mt, d_mt), alpha_i, (t1 - t2).rnd(), dLdB * 2.0, val, z, z]


def _ln_interval(v, eps, pert):
    """stats_interval for data that are themselves off by `pert` [G, n] each: (mean, rstd, d_m, lo, hi)."""
    n = v.shape[1]
    m = v.mean(1)
    var = ((v - m[:, None]) ** 2).mean(1)
    e = eps_for(False, n)
    d_m = e * v.abs().mean(1) + pert.mean(1)
    d_v = e * (var + d_m ** 2) + d_m ** 2
    rms = torch.sqrt((pert ** 2).mean(1))
    s_hi = torch.sqrt(var + d_v) + rms
    s_lo = (torch.sqrt((var - d_v).clamp_min(0)) - rms).clamp_min(0)
    return m, 1 / torch.sqrt(var + eps), d_m, (1 - 4 * U) / torch.sqrt(s_hi ** 2 + eps), (1 + 4 * U) / torch.sqrt(s_lo ** 2 + eps)


def reference(b, tensors=None, entry=None):
    """name -> Ref | Partial of every output of the built case over `tensors` (default: the case's own buffers)."""
    e, sp = entry or b.case.entry, b.spec
    t = b.views(tensors or b.bufs)
    v = compute(e, sp, t, F64)
    if e == "affine_fwd":
        return {"out": _exact(v["out"])}
    if e == "affine_bwd":
        R, rpr, N, ns = sp["R"], sp["rpr"], sp["N"], sp["nsplit"]
        M = R * rpr
        dz = t["dz"][:M * N].reshape(M, N).double()
        out = {}
        if sp["dz_in"]:
            sc = torch.zeros(M, N, dtype=F64)
            if sp["a"]:
                sc = (float(_f32(sp["a0"])) + t["a"][:R * N].reshape(R, N).double())[_ar(M) // rpr].abs()
            out["dz_in"] = _ew(v["dz_in"], U * v["dz_in"].abs() * (1 + U) + U * dz.abs() * sc)
        chunk = ab_chunk(sp)
        empty = lambda s: s * chunk >= rpr          # noqa: E731
        Sb = dz.abs().reshape(R, rpr, N).sum(1)
        bb = eps_for(False, rpr) * Sb
        out["db_slab"] = _slab_ref(v["db_slab"], Sb, bb, ns, empty)
        if sp["zin"]:
            Sa = (dz * t["z_in"][:M * N].reshape(M, N).double()).abs().reshape(R, rpr, N).sum(1)
            ba = eps_for(False, rpr + 1) * Sa
            out["da_slab"] = _slab_ref(v["da_slab"], Sa, ba, ns, empty)
        if sp["dadb"]:
            if sp["zin"]:
                out["da"] = _red_ref(v["da"], Sa, ba, ns)
            out["db"] = _red_ref(v["db"], Sb, bb, ns)
            out["counter"] = _exact(v["counter"])
        return out
    if e == "sisdr_fwd":
        R = sp["R"]
        iv = sisdr_intervals(sp, t)
        val = torch.stack([i.mid() for i in iv], 1)
        bd = torch.stack([i.rad() for i in iv], 1)
        ex = torch.zeros(R, 8, dtype=torch.bool)
        ex[:, 6:] = True
        db = v["rowstat"][:, 5]
        Sl = db.abs().sum().reshape(1) / R
        return {"rowstat": _ref(_ar(R * 8), val, v["rowstat"].abs(), bd, ex),
                "loss": _ref(_ar(1), -iv[5].mid().sum().reshape(1) / R, Sl, iv[5].rad().sum().reshape(1) / R + eps_for(False, R + 1) * Sl)}
    if e == "sisdr_bwd":
        R, T = sp["R"], sp["T"]
        x, tg = t["est"][:R * T].reshape(R, T).double(), t["tgt"][:R * T].reshape(R, T).double()
        rs = t["rowstat"][:R * 8].reshape(R, 8).double()
        go = abs(float(t["gout"][0])) / R
        tcn = tg - rs[:, 1:2]
        S = go * ((rs[:, 3:4] * tcn).abs() + rs[:, 4:5].abs() * ((x - rs[:, 0:1]).abs() + (rs[:, 2:3] * tcn).abs()))
        return {"dest": _ref(_ar(R * T), v["dest"], S, E0 * S)}
    if e == "grad_norms":
        nt = len(sp["numel"])
        val, bd, ex = torch.zeros(nt, dtype=F64), torch.zeros(nt, dtype=F64), torch.zeros(nt, dtype=torch.bool)
        for i, n in enumerate(sp["numel"]):
            if i == sp["null"] or i in sp["nonfinite"]:
                ex[i] = True          # (a non-finite norm: verify() checks that it is not finite and judges it as 0)
                continue
            en = eps_for(False, n + 1)
            val[i] = v["norms"][i]
            bd[i] = val[i] * ((1 - math.sqrt(1 - en)) + U * (1 + en))
        out = {"norms": _ref(_ar(nt), val, val, bd, ex)}
        if sp["guard"] is not None:
            out["guard"] = _exact(v["guard"])
        return out
    if e == "clip_adam_step":
        out = {}
        skipped = _skipped(sp)
        bc1, bc2s, dev_pow = _adam_scalars(sp)
        rho = 2 * U if dev_pow else 0.0
        lr, b1, b2, eps, wd = (float(_f32(sp[k])) for k in ("lr", "beta1", "beta2", "eps", "wd"))
        for i, n in enumerate(sp["numel"]):
            names = [f"{k}{i}" for k in ("pmv" if i == sp["null"] else "pgmv")]
            if i == sp["null"] or skipped:
                out.update({k: _exact(v[k]) for k in names})
                continue
            coef = _coef32(sp, i, t)
            g = v[f"g{i}"]
            d_g = U * g.abs() if coef != 1.0 else torch.zeros_like(g)
            out[f"g{i}"] = _ew(g, d_g, torch.full(g.shape, coef == 1.0))
            if sp["clip_only"]:
                out.update({k: _exact(v[k]) for k in (f"p{i}", f"m{i}", f"v{i}")})
                continue
            p, m, vv = (t[f"{k}{i}"][:n].double() for k in "pmv")
            g2 = g + wd * p
            d_g2 = d_g + (U * (wd * p).abs() + U * g2.abs() if wd != 0 else 0.0)
            m2, v2 = v[f"m{i}"], v[f"v{i}"]
            d_m = (1 - b1) * d_g2 + 4 * U * ((b1 * m).abs() + ((1 - b1) * g2).abs())
            d_v = (1 - b2) * (2 * g2.abs() * d_g2 + d_g2 ** 2) + 5 * U * ((b2 * vv).abs() + (1 - b2) * g2 * g2)
            sq = torch.sqrt(v2)
            d_sq = torch.maximum(torch.sqrt(v2 + d_v) - sq, sq - torch.sqrt((v2 - d_v).clamp_min(0))) + U * torch.sqrt(v2 + d_v)
            den = sq / bc2s + eps
            d_den = (d_sq + sq * (rho + U)) / bc2s * (1 + 4 * U) + U * den
            q = m2 / den
            d_q = (d_m + q.abs() * d_den) / (den - d_den).clamp_min(TINY) + U * q.abs()
            ss = lr / bc1
            p2 = v[f"p{i}"]
            d_p = ss * d_q * (1 + 4 * U) + (ss * q).abs() * (2 * U + rho) + U * p2.abs() + TINY
            out.update({f"p{i}": _ew(p2, d_p), f"m{i}": _ew(m2, d_m + TINY), f"v{i}": _ew(v2, d_v + TINY)})
        for k in ("skip0", "skip1", "lag"):
            if sp[k] is not None:
                out[k] = _exact(v[k])
        return out
    if e == "guard_commit":
        return {k: _exact(x) for k, x in v.items()}
    if e == "heads_fwd":
        B, T, Tp, Q, nh, ch, HC, W, D = _hd(sp)
        xx = _hd_x(sp, t, F64)
        a = _hd_slope(sp, t, F64)
        u = torch.where(xx > 0, xx, a * xx)
        pert = torch.where(xx > 0, torch.zeros_like(u), U * u.abs())
        m, rstd, d_m, lo, hi = _ln_interval(_hd_groups(u, sp), float(_f32(LN_EPS)), _hd_groups(pert, sp))
        ung = lambda s: _hd_ungroup(s, sp)          # noqa: E731
        g, bt = _hd_par(sp, t, "gamma", F64), _hd_par(sp, t, "beta", F64)
        um = u - ung(m)
        d_r = ung(torch.maximum(hi - rstd, rstd - lo))
        Sy = (g * um).abs() * ung(rstd) + bt.abs()
        by = g.abs() * (ung(d_m) * ung(hi) + um.abs() * d_r + ung(hi) * pert) + E0 * Sy
        S = torch.zeros(nh, B, Tp, Q, ch, dtype=F64)
        bd = torch.zeros(nh, B, Tp, Q, ch, dtype=F64)
        S[:, :, :T], bd[:, :, :T] = Sy.permute(3, 0, 1, 2, 4), by.permute(3, 0, 1, 2, 4)
        ex = torch.zeros(nh, B, Tp, Q, ch, dtype=torch.bool)
        ex[:, :, T:] = True
        tr = lambda s: s.reshape(B * T, nh).t()          # noqa: E731
        sval = torch.stack([tr(m), tr((lo + hi) / 2)], 2)
        sbd = torch.stack([tr(d_m), tr((hi - lo) / 2)], 2)
        return {"y": _ref(_ar(S.numel()), v["y"], S, bd, ex), "stats": _ref(_ar(sval.numel()), sval, v["stats"].abs(), sbd)}
    if e == "heads_bwd":
        B, T, Tp, Q, nh, ch, HC, W, D = _hd(sp)
        nwg, BT = sp["nwg"], B * T
        xx = _hd_x(sp, t, F64)
        a = _hd_slope(sp, t, F64)
        u = torch.where(xx > 0, xx, a * xx)
        mean, rstd = _hd_stats_in(sp, t, F64)
        n = (u - mean) * rstd
        an = (u - mean).abs() * rstd.abs()
        dd = t["dy"][:nh * B * Tp * D].double().reshape(nh, B, Tp, Q, ch)[:, :, :T].permute(1, 2, 3, 0, 4)
        d = dd * _hd_par(sp, t, "gamma", F64)
        gm = lambda q: _hd_ungroup(_hd_groups(q, sp).mean(1), sp)          # noqa: E731
        md, mdn = gm(d), gm(d * n)
        Sl = rstd.abs() * (d.abs() + md.abs() + (n * mdn).abs())
        b_dl = E0 * Sl + rstd.abs() * eps_for(False, D) * (gm(d.abs()) + an * gm(d.abs() * an))
        dl = rstd * (d - md - n * mdn)
        pos = xx > 0
        b_dx = torch.where(pos, b_dl, a.abs() * b_dl + U * (a * dl).abs())
        idx = _ar(BT * Q)[:, None] * sp["lddx"] + sp["dx_off"] + _ar(HC)[None, :]
        S_dx = torch.where(pos, Sl, a.abs() * Sl)
        sl_S = _hd_groups(torch.where(pos, torch.zeros_like(dl), (dl * xx).abs()), sp).sum(1).reshape(BT, nh).sum(0)
        sl_b = eps_for(False, BT * D + 1) * sl_S + _hd_groups(torch.where(pos, torch.zeros_like(dl), b_dl * xx.abs()), sp).sum(1).reshape(BT, nh).sum(0)
        Sg, Sb = (dd.abs() * an).reshape(BT, W).sum(0), dd.abs().reshape(BT, W).sum(0)
        pad = torch.zeros(HD_PAD - nh, dtype=F64)
        S = torch.cat([Sg, Sb, sl_S, pad])
        bd = torch.cat([(eps_for(False, BT + 1) + 3 * U) * Sg, eps_for(False, BT) * Sb, sl_b, pad])
        p = _slab_ref(v["slab"], S, bd, nwg, lambda s: s >= BT)
        p.zero[:, 2 * W + nh:] = True
        perm = lambda q: q.reshape(Q, nh, ch).permute(1, 0, 2).reshape(nh, D)          # noqa: E731
        en = eps_for(False, nwg)
        return {"dx": _ref(idx, v["dx"], S_dx, b_dx), "slab": p,
                "dgamma": _ref(_ar(W), v["dgamma"], perm(Sg), perm(bd[:W] + en * Sg)),
                "dbeta": _ref(_ar(W), v["dbeta"], perm(Sb), perm(bd[W:2 * W] + en * Sb)),
                "dslope": _ref(_ar(nh), v["dslope"], sl_S, sl_b + en * sl_S)}
    if e == "tstp_bwd":
        T = sp["T"]
        n = sp["R"] * sp["F"] * T * sp["C"]
        if T == 1:
            return {"dx": _exact(v["dx"])}
        o0, o1 = _tstp_idx(sp)
        x, st, ds = t["x"][:n].double(), t["stats"].double(), t["dstats"].double()
        S = ds[o0].abs() / T + (ds[o1] * (x - st[o0])).abs() / ((T - 1) * st[o1].abs())
        return {"dx": _ref(_ar(n), v["dx"], S, E0 * S)}
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, targets
# ------------------------------------------------------------------------------------------------------------
SISDR = dict(T=[1, 2, 63, 1023, 1024, 1025, 2049, 4100], R=[1, 3, 64, 65, 130], regime=list(ORDINARY + ILL))
HEADS = dict(Q=[1, 7, 65, 16, 36, 205], nh=[1, 3, 8, 5], ch=[4, 12, 32], B=[1, 2], T=[1, 3], pad=[0, 3], off=[0, 8])
DIMS = {
    "affine_fwd": dict(N=[4, 100, 128], a=[0, 1], b=[0, 1], alias=[0, 1], R=[1, 3], rpr=[1, 7, 33]),
    "affine_bwd": dict(N=[4, 100, 128, 1, 3, 126, 127], rpr=[1, 7, 8, 9, 15, 16, 17, 33], nsplit=["1", "2", "3", "rpr", "rpr+3"], a=[0, 1],
                       dz_in=[1, 0], zin=[1, 0], dadb=[0, 1], R=[1, 3]),
    "sisdr_fwd": dict(SISDR),
    "sisdr_bwd": dict(SISDR, gout=[1.0, -2.5]),
    "grad_norms": dict(numel=[1, 1023, 1024, 1025, 5000], nt=[1, 3], null=[0, 1], guard=["null", "zero", "preset"],
                       poison=["none", "nan", "inf", "overflow"]),
    "clip_adam_step": dict(nt=[1, 2, 3, 4, 5], numel=[1, 255, 4096, 4097, 9000], clip=["0", "mid"], wd=[0.0, 1e-4], step=[1, 2, 1000, 100000],
                           lag=["null", "0", "2", "ge"], clip_only=[0, 1], skip0=["null", "zero", "set"], skip1=["null", "zero", "set"],
                           null=[0, 1]),
    "guard_commit": dict(g0=[0, 1, 9], skip1=["null", "zero", "set"]),
    "heads_fwd": dict(HEADS),
    "heads_bwd": dict(HEADS, lddx=["ldx", "ldx+8"], nwg=["1", "BT", "BT+5"]),
    "tstp_bwd": dict(T=[1, 2, 9], F=[1, 3, 5], C=[1, 3, 7], R=[1, 2]),
}
_HD_RULES = [("W = Q nh ch above 9216", ("Q", "nh", "ch"), lambda Q, nh, ch: Q * nh * ch > 9216),
             ("suite condition: statistics over at most CAP elements", ("Q", "ch"), lambda Q, ch: Q * ch > CAP)]
RULES = {e: [] for e in ENTRIES}
RULES["heads_fwd"] = RULES["heads_bwd"] = _HD_RULES
RULES["grad_norms"] = [("a NULL-grad entry next to a real one", ("nt", "null"), lambda nt, null: null and nt < 2)]
RULES["clip_adam_step"] = [("a NULL-grad entry next to a real one", ("nt", "null"), lambda nt, null: null and nt < 2)]


def ab_nsplit(d):
    return {"rpr": d["rpr"], "rpr+3": d["rpr"] + 3}.get(d["nsplit"]) or int(d["nsplit"])


def hd_nwg(d):
    BT = d["B"] * d["T"]
    return {"1": 1, "BT": BT, "BT+5": BT + 5}[d["nwg"]]


def _targets(entry, d, seed=0):
    e = entry
    if e == "affine_fwd":
        t = ("affine_fwd_kernel",) + (("affine_fwd[a NULL]",) if not d["a"] else ()) + (("affine_fwd[b NULL]",) if not d["b"] else ())
        t += ("affine_fwd[out aliases z]",) if d["alias"] else ()
        return t + (("affine_fwd[grid cap]",) if d["R"] * d["rpr"] * d["N"] // 4 > 16384 * 256 else ())
    if e == "affine_bwd":
        ns, rpr = ab_nsplit(d), d["rpr"]
        chunk = -(-rpr // ns)
        vec = d["N"] % 4 == 0
        t = ("affine_bwd4_kernel" if vec else "affine_bwd_kernel",)
        t += ("affine_bwd[empty split]",) if (ns - 1) * chunk >= rpr else ()
        t += ("affine_bwd[dz_in NULL]",) if not d["dz_in"] else ()
        t += ("affine_bwd[no da slab]",) if not d["zin"] else ()
        t += ("affine_bwd[da / db by the last workgroup]",) if d["dadb"] else ()
        t += ("affine_bwd[rows below the row lanes]",) if chunk < (16 if vec else 2) else ()
        t += ("affine_bwd[second trip]",) if chunk > (16 if vec else 2) else ()
        return t
    if e in ("sisdr_fwd", "sisdr_bwd"):
        T, R = d["T"], d["R"]
        if e == "sisdr_bwd":
            return ("sisdr_bwd_kernel",) + (("sisdr_bwd[gout != 1]",) if d["gout"] != 1.0 else ())
        return (("sisdr_fwd_kernel[idle threads]",) if T < 1024 else ("sisdr_fwd_kernel[second trip]",) if T > 1024 else ("sisdr_fwd_kernel[T = 1024]",)) + (
            ("sisdr_mean_kernel[second trip]",) if R > 64 else ("sisdr_mean_kernel[one trip]",))
    if e == "grad_norms":
        t = ("grad_norms_kernel",) + (("grad_norms_kernel[second trip]",) if d["numel"] > 1024 else ())
        t += ("grad_norms[NULL grad]",) if d["null"] else ()
        t += ("grad_norms[guard NULL]",) if d["guard"] == "null" else ()
        return t + (("grad_norms[guard raised]",) if d["guard"] != "null" and d["poison"] != "none" else ())
    if e == "clip_adam_step":
        skipped = "set" in (d["skip0"], d["skip1"])
        t = ("clip_adam_kernel",) + (("clip_adam_kernel[skipped]",) if skipped else ())
        t += ("clip_adam_kernel[clip_only]",) if d["clip_only"] and not skipped else ()
        t += ("clip_adam_kernel[step_lag]",) if d["lag"] != "null" and not d["clip_only"] and not skipped else ()
        t += ("clip_adam_kernel[second trip]",) if d["numel"] > 4096 and not skipped else ()
        t += ("clip_adam_kernel[NULL grad]",) if d["null"] else ()
        return t + (("clip_adam_kernel[norms NULL]",) if d["clip"] == "0" else ())
    if e in ("heads_fwd", "heads_bwd"):
        W = d["Q"] * d["nh"] * d["ch"]
        k = (f"{e}_kernel<4,4>" if W <= 4096 else f"{e}_kernel<12,3>",) + ((f"{e}[W = {W}]",) if W in (4096, 4100, 9216) else ())
        if e == "heads_fwd":
            return k + (("heads_fwd[padded frames]",) if d["pad"] else ())
        nwg, BT = hd_nwg(d), d["B"] * d["T"]
        t = k + (("heads_bwd[idle workgroups]",) if nwg > BT else ())
        t += ("heads_bwd[several rows per workgroup]",) if nwg < BT else ()
        return t + (("heads_bwd[lddx != ldx]",) if d["lddx"] != "ldx" else ())
    if e == "tstp_bwd":
        return ("tstp_bwd_kernel",) + (("tstp_bwd[T = 1]",) if d["T"] == 1 else ())
    return (f"{e}_kernel",)


_M = gc.MIN_PER_TARGET
TOPUP = {
    "affine_fwd": [({}, "affine_fwd_kernel", _M), ({"a": 0}, "affine_fwd[a NULL]", _M), ({"b": 0}, "affine_fwd[b NULL]", _M),
                   ({"alias": 1}, "affine_fwd[out aliases z]", _M)],
    "affine_bwd": [({"N": 100}, "affine_bwd4_kernel", _M), ({"N": 127}, "affine_bwd_kernel", _M), ({"N": 3}, "affine_bwd_kernel", 2 * _M),
                   ({"nsplit": "rpr+3"}, "affine_bwd[empty split]", _M), ({"dz_in": 0}, "affine_bwd[dz_in NULL]", _M),
                   ({"zin": 0}, "affine_bwd[no da slab]", _M), ({"dadb": 1}, "affine_bwd[da / db by the last workgroup]", _M),
                   ({"rpr": 7}, "affine_bwd[rows below the row lanes]", _M), ({"rpr": 33, "nsplit": "1"}, "affine_bwd[second trip]", _M)],
    "sisdr_fwd": [({"T": 63}, "sisdr_fwd_kernel[idle threads]", _M), ({"T": 2049}, "sisdr_fwd_kernel[second trip]", _M),
                  ({"T": 1024}, "sisdr_fwd_kernel[T = 1024]", _M), ({"R": 130}, "sisdr_mean_kernel[second trip]", _M),
                  ({"R": 3}, "sisdr_mean_kernel[one trip]", _M)],
    "sisdr_bwd": [({}, "sisdr_bwd_kernel", _M), ({"gout": -2.5}, "sisdr_bwd[gout != 1]", _M)],
    "grad_norms": [({}, "grad_norms_kernel", _M), ({"numel": 5000}, "grad_norms_kernel[second trip]", _M), ({"null": 1}, "grad_norms[NULL grad]", _M),
                   ({"guard": "null"}, "grad_norms[guard NULL]", _M), ({"guard": "zero", "poison": "overflow"}, "grad_norms[guard raised]", _M)],
    "clip_adam_step": [({}, "clip_adam_kernel", _M), ({"skip1": "set"}, "clip_adam_kernel[skipped]", _M),
                       ({"clip_only": 1, "skip0": "zero", "skip1": "null"}, "clip_adam_kernel[clip_only]", _M),
                       ({"lag": "2", "clip_only": 0, "skip0": "zero", "skip1": "null"}, "clip_adam_kernel[step_lag]", _M),
                       ({"lag": "ge", "clip_only": 0, "skip0": "null", "skip1": "zero"}, "clip_adam_kernel[step_lag]", 2 * _M),
                       ({"numel": 9000, "skip0": "null", "skip1": "null"}, "clip_adam_kernel[second trip]", _M),
                       ({"null": 1}, "clip_adam_kernel[NULL grad]", _M), ({"clip": "0"}, "clip_adam_kernel[norms NULL]", _M)],
    "guard_commit": [({}, "guard_commit_kernel", _M)],
    "tstp_bwd": [({}, "tstp_bwd_kernel", _M), ({"T": 1}, "tstp_bwd[T = 1]", _M)],
}
for _e in ("heads_fwd", "heads_bwd"):
    TOPUP[_e] = [({"Q": 7, "nh": 1, "ch": 4}, f"{_e}_kernel<4,4>", 1), ({}, f"{_e}_kernel<4,4>", _M), ({"Q": 36}, f"{_e}_kernel<12,3>", _M),
                 ({"Q": 16, "nh": 8, "ch": 32}, f"{_e}[W = 4096]", _M), ({"Q": 205, "nh": 5, "ch": 4}, f"{_e}[W = 4100]", _M),
                 ({"Q": 36, "nh": 8, "ch": 32}, f"{_e}[W = 9216]", _M)]
TOPUP["heads_fwd"] += [({"pad": 3}, "heads_fwd[padded frames]", _M)]
TOPUP["heads_bwd"] += [({"nwg": "BT+5"}, "heads_bwd[idle workgroups]", _M), ({"nwg": "1", "B": 2, "T": 3}, "heads_bwd[several rows per workgroup]", _M),
                       ({"lddx": "ldx+8"}, "heads_bwd[lddx != ldx]", _M)]
INST = {e: list(dict.fromkeys(tag for _, tag, _ in TOPUP[e])) for e in ENTRIES}
INST["affine_fwd"].append("affine_fwd[grid cap]")
EXACT_COUNT = {"affine_fwd[grid cap]": 1}
EXTRA = {"affine_fwd": [dict(N=128, a=1, b=1, alias=0, R=5, rpr=26216)]}          # 4 194 560 quads
_KEY = {e: "st_" + e for e in ENTRIES}          # the registries of gemm_contract are shared by every suite
for _i, _e in enumerate(ENTRIES):
    gc.DIMS[_KEY[_e]], gc.RULES[_KEY[_e]], gc.INST[_KEY[_e]], gc.TOPUP[_KEY[_e]] = DIMS[_e], RULES[_e], INST[_e], TOPUP[_e]
    gc.SEEDS[_KEY[_e]] = 201 + _i
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
def sisdr_data(g, R, T, regime):
    """(est, tgt, eps) of a regime: the estimate is 0.8 x the centred target + noise at the regime's level + its own offset."""
    t0 = torch.randn(R, T, generator=g)
    noise = torch.randn(R, T, generator=g)
    snr = {"-5dB": -5.0, "10dB": 10.0, "30dB": 30.0, "near": 60.0, "eps1e-3": 10.0}.get(regime, 10.0)
    x = 0.8 * t0 + 0.8 * 10 ** (-snr / 20) * noise
    dc = 10.0 if regime == "dc10" else 0.3
    tg, x = t0 + dc, x + dc - 0.1
    if regime == "const_t":
        tg = torch.full((R, T), 0.7)
    if regime == "const_x":
        x = torch.full((R, T), -0.4)
    if T > CAP:
        x, tg = torch.stack([_spiked(r) for r in x]), torch.stack([_spiked(r) for r in tg])
    return x.float(), tg.float(), (1e-3 if regime == "eps1e-3" else 1e-8)


def _opt_numels(d):
    """The tensors of an optimizer case: the case's numel first, small ones behind it."""
    return ([d["numel"]] + [7, 300, 130, 5])[:d["nt"]]


def _word(v, preset):
    return {"null": None, "zero": 0, "set": preset, "preset": preset}[v]


def build(case, garbage=False):
    e, d, g = case.entry, case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    b = TBuilt(case)
    sp = b.spec
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731

    def inp(name, data, read=None):
        mc._input(b, name, data, fill, read)

    def out(name, n, widx=None, alias=None):
        if alias:
            mc._alias(b, name, alias, _ar(n) if widx is None else widx)
        else:
            mc._output(b, name, n, widx)

    if e == "affine_fwd":
        R, rpr, N = d["R"], d["rpr"], d["N"]
        rows = R * rpr
        sp.update(R=R, rpr=rpr, N=N, a=d["a"], b=d["b"], a0=1.0 if d["a"] else 0.75, alias=d["alias"])
        inp("z", rn(rows, N))
        if d["a"]:
            inp("a", rn(R, N) * 0.5)
        if d["b"]:
            inp("b", rn(R, N))
        out("out", rows * N, alias="z" if d["alias"] else None)
        return b
    if e == "affine_bwd":
        R, rpr, N = d["R"], d["rpr"], d["N"]
        ns = ab_nsplit(d)
        M = R * rpr
        sp.update(R=R, rpr=rpr, N=N, nsplit=ns, a=d["a"], a0=1.0 if d["a"] else 0.75, dz_in=d["dz_in"], zin=d["zin"], dadb=d["dadb"])
        inp("dz", rn(M, N))
        if d["zin"]:
            inp("z_in", rn(M, N) + 0.25)
        if d["a"]:
            inp("a", rn(R, N) * 0.5)
        if d["dz_in"]:
            out("dz_in", M * N)
        if d["zin"]:
            out("da_slab", ns * R * N)
        out("db_slab", ns * R * N)
        if d["dadb"]:
            if d["zin"]:
                out("da", R * N)
            out("db", R * N)
            b.extras += ["counter"]
        return b
    if e in ("sisdr_fwd", "sisdr_bwd"):
        R, T = d["R"], d["T"]
        x, tg, eps = sisdr_data(g, R, T, d["regime"])
        sp.update(R=R, T=T, eps=eps, regime=d["regime"])
        inp("est", x)
        inp("tgt", tg)
        if e == "sisdr_fwd":
            out("rowstat", R * 8)
            out("loss", 1)
            return b
        inp("rowstat", _sisdr_rows(sp, b.views(b.bufs), F64, "seq"))
        inp("gout", torch.tensor([d["gout"]]))
        out("dest", R * T)
        return b
    if e == "grad_norms":
        numel = ([d["numel"]] + [7, 300])[:d["nt"]]
        null = 1 if d["null"] else -1
        sp.update(numel=numel, null=null, guard=_word(d["guard"], 7), poison=d["poison"], nonfinite=[])
        for i, n in enumerate(numel):
            if i == null:
                continue
            gr = rn(n) * (0.1 * 3 ** i)
            if n > CAP:
                gr = _spiked(gr)
            if i == 0 and d["poison"] != "none":
                sp["nonfinite"] = [0]
                if d["poison"] == "overflow":
                    gr = torch.full((n,), 3.0e19) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
                else:
                    gr[n // 2] = {"nan": float("nan"), "inf": -float("inf")}[d["poison"]]
            inp(f"g{i}", gr)
        out("norms", len(numel))
        if sp["guard"] is not None:
            b.extras += ["guard"]
        return b
    if e == "clip_adam_step":
        numel = _opt_numels(d)
        null = 1 if d["null"] else -1
        step = d["step"]
        lag = {"null": None, "0": 0, "2": 2, "ge": step + 3}[d["lag"]]
        sp.update(numel=numel, null=null, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=d["wd"], step=step, lag=lag, clip_only=d["clip_only"],
                  skip0=_word(d["skip0"], 1), skip1=_word(d["skip1"], 5), clip=0.0)
        norms = []
        for i, n in enumerate(numel):
            sc = 0.1 * 3 ** i
            inp(f"p{i}", rn(n))
            gr = rn(n) * sc
            if i == null:
                norms.append(0.0)
            else:
                inp(f"g{i}", gr)
                norms.append(float(gr.double().norm()))
            inp(f"m{i}", rn(n) * sc * 0.1)
            inp(f"v{i}", (rn(n) * sc) ** 2 * 1e-3)
        live = sorted(v for i, v in enumerate(norms) if i != null)
        if d["clip"] == "mid":
            sp["clip"] = float(_f32(math.sqrt(live[0] * live[-1]) if len(live) > 1 else 0.5 * live[0]))
            inp("norms", torch.tensor(norms))
        for i, n in enumerate(numel):
            for k in ("pmv" if i == null else "pgmv"):
                out(f"{k}{i}", n, alias=f"{k}{i}")
        b.extras += [k for k in ("skip0", "skip1", "lag") if sp[k] is not None]
        return b
    if e == "guard_commit":
        sp.update(guard=[d["g0"], 3, 2, 1], skip1=_word(d["skip1"], 5))
        b.extras += ["guard1", "guard2"]
        return b
    if e in ("heads_fwd", "heads_bwd"):
        B, T, Q, nh, ch = d["B"], d["T"], d["Q"], d["nh"], d["ch"]
        Tp, HC, D = T + d["pad"], nh * ch, Q * ch
        ldx = HC + (12 if d["off"] else 0)
        sp.update(B=B, T=T, Tp=Tp, Q=Q, nh=nh, ch=ch, ldx=ldx, x_off=d["off"])
        rows = B * T * Q
        rd = torch.zeros(rows, ldx, dtype=torch.bool)
        rd[:, d["off"]:d["off"] + HC] = True
        x = rn(rows, ldx) + 0.25
        x.reshape(-1)[::11] = 0.0          # values exactly 0: PReLU's x > 0 test
        inp("x", x, rd)
        inp("slope", torch.tensor([0.25, -0.5, 0.0, 1.0, 0.1, 0.3, 2.0, 0.7][:nh]))
        inp("gamma", rn(nh, D) + 1.0)
        if e == "heads_fwd":
            inp("beta", rn(nh, D))
            out("y", nh * B * Tp * D)
            out("stats", nh * B * T * 2)
            return b
        lddx = ldx if d["lddx"] == "ldx" else ldx + 8
        sp.update(lddx=lddx, dx_off=4 if d["lddx"] != "ldx" else d["off"], nwg=hd_nwg(d))
        dyr = torch.ones(nh, B, Tp, D, dtype=torch.bool)
        dyr[:, :, T:] = False
        inp("dy", rn(nh, B, Tp, D), dyr)
        st = compute("heads_fwd", sp, dict(b.views(b.bufs), beta=torch.zeros(nh * D)), F64)["stats"]
        inp("stats", st)
        out("dx", rows * lddx, _ar(rows)[:, None] * lddx + sp["dx_off"] + _ar(HC)[None, :])
        b.extras += ["slab", "dgamma", "dbeta", "dslope"]
        return b
    if e == "tstp_bwd":
        R, Fq, T, C = d["R"], d["F"], d["T"], d["C"]
        sp.update(R=R, F=Fq, T=T, C=C)
        x = rn(R, Fq, T, C) + 0.5
        xd = x.double()
        mean = xd.mean(2)
        sd = torch.sqrt((((xd - mean[:, :, None]) ** 2).sum(2) / (T - 1) if T > 1 else torch.zeros_like(mean)) + TSTP_EPS)
        inp("x", x)
        inp("stats", torch.stack([mean.permute(0, 2, 1), sd.permute(0, 2, 1)], 1))
        inp("dstats", rn(R, 2, C * Fq))
        out("dx", R * Fq * T * C)
        return b
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------
def _words(vals, device):
    return None if vals is None else torch.tensor(vals if isinstance(vals, list) else [vals], dtype=torch.int32, device=device)


def _table(rows, device):
    import numpy as np
    from wesep_amd import _lib as L
    arr = np.zeros(len(rows), dtype=L.TENSOR_REF_DTYPE)
    for i, (ptrs, n) in enumerate(rows):
        arr[i] = tuple(0 if p is None else p.data_ptr() for p in ptrs) + (n,)
    return L.upload_struct_array(arr, device, blocking=True)


def run(mod, b, tensors, device="cpu", entry=None):
    """The case's call on `mod` (wesep_amd.dev) over `tensors` (the allocations on the device); returns the extras."""
    e, sp, v = entry or b.case.entry, b.spec, b.views(tensors)
    fl = lambda w: w.float()          # noqa: E731
    if e == "affine_fwd":
        mod.affine_fwd(v["z"], v.get("a"), v.get("b"), sp["a0"], sp["R"] * sp["rpr"], sp["rpr"], sp["N"], v["out"])
    elif e == "affine_bwd":
        cnt = _words([0] * sp["R"], device) if sp["dadb"] else None
        mod.affine_bwd(v["dz"], v.get("z_in"), v.get("a"), sp["a0"], sp["R"] * sp["rpr"], sp["rpr"], sp["N"], sp["nsplit"], v.get("dz_in"),
                       v.get("da_slab"), v["db_slab"], v.get("da"), v.get("db"), cnt)
        return {"counter": fl(cnt)} if sp["dadb"] else {}
    elif e == "sisdr_fwd":
        mod.sisdr_fwd(v["est"].reshape(sp["R"], sp["T"]), v["tgt"].reshape(sp["R"], sp["T"]), v["rowstat"], v["loss"], eps=sp["eps"])
    elif e == "sisdr_bwd":
        mod.sisdr_bwd(v["est"].reshape(sp["R"], sp["T"]), v["tgt"].reshape(sp["R"], sp["T"]), v["rowstat"], v["gout"], v["dest"])
    elif e == "grad_norms":
        rows = [((v["norms"], v.get(f"g{i}"), None, None), n) for i, n in enumerate(sp["numel"])]
        guard = _words([sp["guard"], 3, 2, 1], device) if sp["guard"] is not None else None
        mod.grad_norms(_table(rows, device), len(rows), v["norms"], guard)
        return {"guard": fl(guard)} if guard is not None else {}
    elif e == "clip_adam_step":
        rows = [((v[f"p{i}"], v.get(f"g{i}"), v[f"m{i}"], v[f"v{i}"]), n) for i, n in enumerate(sp["numel"])]
        w = {k: _words(sp[k], device) for k in ("skip0", "skip1", "lag")}
        mod.clip_adam_step(_table(rows, device), len(rows), v.get("norms"), sp["clip"], sp["lr"], sp["beta1"], sp["beta2"], sp["eps"], sp["wd"],
                           sp["step"], clip_only=bool(sp["clip_only"]), skip=(w["skip0"], w["skip1"]), step_lag=w["lag"])
        return {k: fl(x) for k, x in w.items() if x is not None}
    elif e == "guard_commit":
        guard, s1 = _words(sp["guard"], device), _words(sp["skip1"], device)
        mod.guard_commit(guard, s1)
        g1 = fl(guard)
        mod.guard_commit(guard, s1)
        return {"guard1": g1, "guard2": fl(guard)}
    elif e == "heads_fwd":
        mod.heads_fwd(v["x"], sp["ldx"], sp["x_off"], v["slope"], v["gamma"], v["beta"], sp["B"], sp["T"], sp["Tp"], sp["Q"], sp["nh"], sp["ch"],
                      v["y"], v["stats"])
    elif e == "heads_bwd":
        dg, db, ds, slab = mod.heads_bwd(v["x"], sp["ldx"], sp["x_off"], v["dy"], v["slope"], v["gamma"], v["stats"], sp["B"], sp["T"], sp["Tp"],
                                         sp["Q"], sp["nh"], sp["ch"], v["dx"], sp["lddx"], sp["dx_off"], nwg=sp["nwg"], with_slab=True)
        return {"slab": slab, "dgamma": dg, "dbeta": db, "dslope": ds}
    elif e == "tstp_bwd":
        mod.tstp_bwd(v["x"], v["stats"], v["dstats"], sp["R"], sp["F"], sp["T"], sp["C"], v["dx"])
    else:
        raise ValueError(e)
    return {}


def refusals(dev, t, device="cpu"):
    """(name, call): one argument set per WS_REQUIRE clause; every call has to come back WS_ERR_INVALID without launching."""
    w = torch.zeros(4, dtype=torch.int32, device=device)
    tab = _table([((t, t, t, t), 8)], device)
    t2 = t[:64].reshape(2, 32)
    ab = lambda **k: (lambda a: dev.affine_bwd(t, a["z"], t, 1.0, a["rows"], a["rpr"], a["N"], a["ns"], t, a["das"], t, a["da"], a["db"], a["cnt"]))(          # noqa: E731
        dict(dict(z=t, rows=8, rpr=4, N=8, ns=2, das=t, da=None, db=None, cnt=None), **k))
    hd = lambda **k: dict(dict(B=1, T=2, Tp=2, Q=2, nh=2, ch=4, ld=8), **k)          # noqa: E731
    hf = lambda **k: (lambda a: dev.heads_fwd(t, a["ld"], 0, t, t, t, a["B"], a["T"], a["Tp"], a["Q"], a["nh"], a["ch"], t, t))(hd(**k))          # noqa: E731
    hb = lambda nwg=None, ldd=8, **k: (lambda a: dev.heads_bwd(t, a["ld"], 0, t, t, t, t, a["B"], a["T"], a["Tp"], a["Q"], a["nh"], a["ch"], t, ldd, 0, nwg=nwg))(hd(**k))          # noqa: E731
    return [
        ("affine_fwd N % 4", lambda: dev.affine_fwd(t, t, t, 1.0, 8, 4, 6, t)),
        ("affine_fwd rows_per_r = 0", lambda: dev.affine_fwd(t, t, t, 1.0, 8, 0, 8, t)),
        ("affine_bwd N above 128", lambda: ab(N=132)),
        ("affine_bwd nsplit = 0", lambda: ab(ns=0)),
        ("affine_bwd rows % rows_per_r", lambda: ab(rows=9)),
        ("affine_bwd da_slab without z_in", lambda: ab(z=None)),
        ("affine_bwd da without a counter", lambda: ab(da=t)),
        ("affine_bwd da without its slab", lambda: ab(da=t, das=None, cnt=w)),
        ("sisdr_fwd T = 0", lambda: dev.sisdr_fwd(t[:0].reshape(2, 0), t[:0].reshape(2, 0), t, t)),
        ("sisdr_bwd T = 0", lambda: dev.sisdr_bwd(t[:0].reshape(2, 0), t[:0].reshape(2, 0), t, t, t)),
        ("sisdr_bwd rowstat NULL", lambda: dev.sisdr_bwd(t2, t2, None, t, t)),
        ("grad_norms ntensors = 0", lambda: dev.grad_norms(tab, 0, t, None)),
        ("clip_adam_step ntensors = 0", lambda: dev.clip_adam_step(tab, 0, t, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)),
        ("clip_adam_step clip without norms", lambda: dev.clip_adam_step(tab, 1, None, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)),
        ("clip_adam_step step = 0", lambda: dev.clip_adam_step(tab, 1, t, 1.0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0)),
        ("guard_commit guard NULL", lambda: dev.guard_commit(None, w)),
        ("heads_fwd ch % 4", lambda: hf(ch=6, ld=12)),
        ("heads_fwd nh = 9", lambda: hf(nh=9, ld=36)),
        ("heads_fwd Tp below T", lambda: hf(Tp=1)),
        ("heads_fwd W above 9216", lambda: hf(Q=289, nh=8, ch=4, ld=32)),
        ("heads_bwd nwg = 0", lambda: hb(nwg=0)),
        ("heads_bwd W above 9216", lambda: hb(Q=289, nh=8, ch=4, ld=32, ldd=32)),
        ("tstp_bwd T = 0", lambda: dev.tstp_bwd(t, t, t, 2, 3, 0, 4, t)),
        ("tstp_bwd C = 0", lambda: dev.tstp_bwd(t, t, t, 2, 3, 4, 0, t)),
    ]


# ------------------------------------------------------------------------------------------------------------
# checker, emulation
# ------------------------------------------------------------------------------------------------------------
def verify(b, ref, after, extra=None, what=None):
    """Every output of a built case against `ref`: `after` = name -> whole CPU allocation after the launch, `extra` = what
    run() returned, on the CPU.  Returns the worst err / bound.  Raises ContractViolation: nan | exact | bound | sentinel."""
    what = what or f"{b.case.entry} {b.case.name}"
    worst = 0.0
    if b.spec.get("nonfinite"):          # grad_norms: a poisoned tensor's norm must not be finite; it is judged as an exact 0 below
        after = dict(after, norms=after["norms"].clone())
        for i in b.spec["nonfinite"]:
            j = b.start["norms"] + i
            if math.isfinite(float(after["norms"][j])):
                raise ContractViolation("exact", f"{what} norms: the norm of the poisoned tensor {i} is {float(after['norms'][j])!r}")
            after["norms"][j] = 0.0
    for key, r in ref.items():
        fn = check_partial if isinstance(r, Partial) else check
        if key in b.extras:
            o = extra[key].reshape(-1).float()
            worst = max(worst, fn(o, torch.full((o.numel(),), NAN), r, f"{what} {key}", 0))
            continue
        name = b.alias.get(key, key)
        worst = max(worst, fn(after[name], b.bufs[name], r, f"{what} {key}", b.start[name]))
    return worst


output_bits = tc.output_bits


def _place(b, ref, vals):
    """(after, extra) with `vals` (name -> values in the order of the reference's idx / rows) written."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    extra = {}
    for key, r in ref.items():
        if key in b.extras:
            extra[key] = vals[key].reshape(-1).float()
            continue
        name = b.alias.get(key, key)
        idx = r.rows.reshape(-1) if isinstance(r, Partial) else r.idx
        after[name][idx + b.start[name]] = vals[key].reshape(-1).float()
    if b.spec.get("nonfinite"):
        for i in b.spec["nonfinite"]:
            after["norms"][b.start["norms"] + i] = float("inf")
    return after, extra


def perfect(b, ref):
    """What a correctly rounding kernel leaves: the fp32 rounding of the float64 values."""
    return _place(b, ref, compute(b.case.entry, b.spec, b.views(b.bufs), F64))


def emulate(b, ref, order="seq", defect=None):
    """What a correct fp32 kernel (sums in `order`) leaves -- or one with the planted `defect`."""
    return _place(b, ref, compute(b.case.entry, b.spec, b.views(b.bufs), F32, order, defect))


DEFECTS = {
    "affine_fwd": ["r_by_mod", "a0_dropped"],
    "affine_bwd": ["last_row_dropped", "two_row_twice", "da_skips_split0", "scale_without_a0"],
    "sisdr_fwd": ["mean_not_subtracted", "last_lane_dropped", "c2_not_doubled", "mean_first_64_rows"],
    "sisdr_bwd": ["gout_not_divided", "alpha_dropped", "rowstat_of_row0"],
    "grad_norms": ["one_trip_of_1024", "last_dropped", "guard_never_set"],
    "clip_adam_step": ["bc2_not_sqrt", "wd_after_moments", "clip_when_coef_ge_1", "lag_not_clamped", "lag_ignored", "skip1_ignored"],
    "guard_commit": ["skip1_ignored", "consecutive_not_reset"],
    "heads_fwd": ["stats_over_W", "pad_unwritten", "slope_of_head0"],
    "heads_bwd": ["dslope_over_pos", "last_row_dropped", "mean_over_W"],
    "tstp_bwd": ["div_by_T", "feature_f_major"],
}
# the defects that may only be caught on the ordinary SI-SDR regimes (the docstring's condition 3)
ORDINARY_ONLY = ("sisdr_fwd", "sisdr_bwd")
