"""TEST INFRASTRUCTURE ONLY -- contract suite of the Conv-TasNet / SpEx+ kernels of wesep_amd/csrc/tasnet.hip: ws_prelu_fwd / bwd,
ws_dwconv_ex_fwd / bwd (and the plain wrappers), ws_chan_sums (all three modes), ws_norm_ab, ws_norm_bwd_apply_cl,
ws_maskmul_fwd / bwd, ws_relu_mask, ws_ola_fwd / bwd, ws_sum_partial, ws_bn_stats, ws_bn_prelu_fwd, ws_bn_bwd, ws_maxpool3_fwd /
bwd, ws_bcast_rows and ws_cross_entropy.  Same shape as tests/map_contract.py: Ref, check, eps_for, the guards and the pairwise
generator with its registries come from tests/gemm_contract.py, Partial / check_partial / sum32 from tests/norm_contract.py,
the builders of guarded operands from tests/map_contract.py.  No GPU code here: test_tasnet_contract_host_cpu.py checks this
module, test_tasnet_contract_gpu.py runs every case through wesep_amd.dev.  Out of scope: ws_flat_stats (tests/norm_contract.py),
the _len and _stream relatives in other files, ws_reduce_slabs (tests/gemm_contract.py).

1. REFERENCE.  compute(entry, spec, tensors, dtype) restates include/wesep_hip.h as explicit index arithmetic (gathers over
   index tensors, sums over explicit tap lists; no F.conv1d / F.conv_transpose1d / F.max_pool1d / F.batch_norm /
   F.cross_entropy / F.prelu / unfold: those are the host test's second opinion at 1e-12).  Run in float64 it is the reference,
   in float32 (sums sequential or pairwise) the emulation of a correct kernel, with `defect` a planted defect.  Channels-last
   rows [R*T'][C], m = r T' + t:
     prelu     pre = x + rb[m / rows_per_r] (written over x; rb NULL: x is not written), y = pre > 0 ? pre : a pre;
               dx = pre > 0 ? dy : a dy, slab = partial sums of dy min(pre, 0) (block s owns the quads i with (i / 256) % nslab == s)
     dwconv    xn = (x - mean_s) rstd_s gamma + beta, s = m / st_div;  y[m] = b + sum_p w[c][p] xn[m + (p - ctr) dil], the taps
               with 0 <= t + (p - ctr) dil < T' only, ctr = causal ? P - 1 : (P - 1) / 2;  dxn[m] = sum_p w[c][p] dy[m - (p - ctr) dil];
               slab[s][p][c] = sum over the rows [s rps, min(M, (s + 1) rps)) of dy[m] xn[m + (p - ctr) dil], slab[s][P][c] = sum dy
     chan_sums slab[s ngroups + grp][0] = sum g, [1] = sum g xhat over the rows j in [s per, min(rpg, (s + 1) per)) of the group,
               per = ceil(rpg / nsplit); xhat = (x - mean_s) rstd_s (stats NULL: x; x NULL: the second row is exactly 0)
     norm_ab   ab[grp] = (sum_c gamma S0, sum_c gamma S1) / n_per_group
     norm_bwd  dx = rstd_s (dxn gamma - ab0_s - xhat ab1_s) (+ res): stats AND ab are indexed by s = m / st_div
     maskmul   s = w m;  dw = ds m (row stride ld_dw, the other columns untouched), dm = m > 0 ? ds w : 0
     relu_mask d = y > 0 ? d : 0, in place
     ola       est[r][j] = bias + sum over t with 0 <= j - hop t < L of frames[r T' + t][j - hop t], j < Tout;
               dframes[m][k] = hop t + k < Tout ? dest[r][hop t + k] : 0
     sum       slab = partial sums of x (block s owns the i with (i / 256) % nslab == s)
     bn_stats  mean, 1 / sqrt(biased var + eps) over the M rows, two passes; running = (1 - mom) old + mom (mean | M / (M - 1) var)
     bn_prelu  u = gamma (x - mean) rstd + beta (+ res), y = PReLU(u)
     bn_bwd    sums = (sum du, sum du xhat); dx = gamma rstd (du - sums0 / M - xhat sums1 / M); slab rows as dwconv's splits
     maxpool3  y[r][t'] = max of the rows 3 t' .. 3 t' + 2; dx goes to the FIRST maximal row, 0 elsewhere and on the T % 3 tail rows
     bcast     out[m] = scale src[m / rows_per_r]
     ce        loss = mean_r (logsumexp_r - z_r[label_r]);  dlogits = (softmax - onehot) / R
   Backward entries TAKE their forward quantities (stats, pre, sums, ab): uploaded as the fp32 rounding of the float64 values,
   and the reference computes from exactly those fp32 numbers, so every entry is judged on its own.  The composed chains
   (test_tasnet_contract_gpu.py) feed each stage the device output of the one before and evaluate the reference there.

2. BOUNDS.  Per element, derived; u = 2^-24, e(n) = eps_for(False, n) = (n + 8) u applied to the same expression over absolute
   values (S).  The build has no fast-math flag (wesep_amd/build.py), so +, *, /, sqrtf round correctly; a path of r <= 7
   roundings is inside e(0) = 8 u.
     bit-exact           relu_mask; ola_bwd (a gather, zeros past Tout); maxpool3_fwd / bwd (a selection; values are compared, not
                         bits, where signed zeros can differ); bcast_rows with scale = 1; prelu y and dx where pre > 0 (rb NULL);
                         maskmul_bwd's zeros; ola_fwd where at most one addend meets the 0 the sum starts from; every exact zero of
                         the header: the second row of chan_sums with x NULL, slabs of splits / blocks that own nothing,
                         maxpool3_bwd's tail rows
     prelu_fwd           pre: u |pre| (one addition).  PReLU is Lipschitz max(1, |a|) and continuous, so a kernel whose rounded
                         pre sits on the other side of 0 stays inside:  y: max(1, |a|) u |pre| + u |y| (rb given), u |y| (pre <= 0)
     prelu_bwd           dx: u |dx|;  slab: e(n + 1) sum |dy min(pre, 0)| (n addends, one product each)
     dwconv              xn takes four roundings: d_xn = 4 u A, A = |(x - mean) rstd gamma| + |beta|.
                         y: (e(P + 1) + 4 u) S, S = |b| + sum_p |w| A;  dxn: e(P + 1) sum_p |w dy|;
                         slab rows p < P: (e(M + 1) + 4 u) sum |dy| A, row P: e(M) sum |dy|, M = R T' (every split together)
     chan_sums           row 0: e(rpg) sum |g|;  row 1: (e(rpg + 1) + 2 u) sum |g xhat| (xhat: two roundings; 0 without stats)
     norm_ab             (e(C + 1) + 2 u) sum_c |gamma S| / n (the products, fl(1 / n) and the last product)
     norm_bwd_apply      e(0) S, S = |rstd| (|dxn gamma| + |ab0| + |xhat ab1|) + |res|: seven roundings on the longest path
     maskmul             u |s|, u |dw|, u |dm|
     ola_fwd             e(ceil(L / hop) + 1) (|bias| + sum |frames|)
     sum_partial         e(n) sum |x|
     wrapper sums        da, dw / db, chan_sums' and bn_bwd's sums, total_sum: the slab's bound + e(nsplit) S (ws_reduce_slabs)
     bn_stats            mean: d_m = e(M) E|x|.  rstd is an INTERVAL, the two-pass form, carried as norm_contract carries it
                         (stats_interval): the variance is taken around the kernel's mean, sum (x - mean')^2 / M = var +
                         (mean - mean')^2 exactly, so d_v = e(M) (var + d_m^2) + d_m^2 and rstd lies in
                         [(1 - 4u) / sqrt(var + d_v + eps), (1 + 4u) / sqrt(max(var - d_v, 0) + eps)]: val = the midpoint, bound
                         = the half width, S = the exact rstd.  The running statistics are read-modify-write, expected from the
                         uploaded old value: running_mean: mom d_m + e(0) (|(1 - mom) old| + |mom mean|);  running_var: the
                         unbiased M / (M - 1) var inside the same interval: mom d_v M / (M - 1) + e(0) (|(1 - mom) old| + mom var M / (M - 1))
     bn_prelu_fwd        u: d_u = e(0) (|(x - mean) rstd gamma| + |beta| + |res|);  y: max(1, |a|) d_u + u |y|
     bn_bwd              slab as chan_sums over M rows; dx: e(0) S + |gamma rstd| (b0 + |xhat| b1) / M, S = |gamma rstd| (|du| +
                         |sums0| / M + |xhat sums1| / M): the entry computes its own sums (b0, b1: their bounds with the reduce)
     bcast_rows          u |out| (scale != 1)
     library functions   ULP_EXP = 3 (map_contract) and ULP_LOG = 3: the OpenCL full-profile requirement the device library
                         implements, the source tests/map_contract.py names for expf / expm1f / tanhf; that table gives log 3 ulp.
                         One ulp is at most 2 u relative: D_EXP = D_LOG = 6 u.
     cross_entropy       max-subtracted.  z = x - max (d_z = u |z|), rho = D_EXP + expm1(d_z); with y = softmax the sum se is
                         off by the relative d_se = sum_k y_k rho_k + e(S); lse = max + logf(se): d_lse = d_se + D_LOG |log se| +
                         u |lse|.  dlogits: the argument x - lse is off by d_a = d_lse + u |x - lse|:
                         (y (D_EXP + expm1(d_a)) + 2^-125) / R + 2 u |dlogits| -- the absolute floor covers expf underflowing to 0
                         or a flushed denormal where float64 does not.  loss: (sum_r (d_lse + u |lse - x_label|)) / R +
                         e(R + 1) sum_r |lse - x_label| / R
   Slabs are judged as float64 sums over the splits (norm_contract.Partial): every slab element is written, splits that own no
   row are exact zeros, and the assignment of rows to the other splits stays open wherever the header leaves it open.

3. CONDITION OF THE SUITE.  Such bounds see a dropped or misplaced addend only while it weighs enough in its sum.  Gauss and
   offset data stay at sums of at most CAP = 2048 leaves: test_tasnet_contract_host_cpu.py confirms on the CPU that every
   planted defect of DEFECTS is refused by the reference alone at these sizes.  Longer sums exist only to cross a loop seam
   (prelu_bwd with n = 4120, sum_partial with n = 5000) and carry a structural spike: the last element x1e3.

4. CASES.  cases(entry): gemm_contract's pairwise generator over DIMS, topped up so that every dispatch target of INST gets
   MIN_PER_TARGET cases, plus the hand-written cases of EXTRA: the three geometries at which dwconv_bwd_w_kernel takes more
   than 64 KB of dynamic LDS (C = 768 with P = 7, C = 776 with P = 5 and P = 7, each at T' = 7, R = 2), once each -- the
   generated cases stay below 64 KB -- and one case each for the plain wrappers ws_dwconv_fwd / ws_dwconv_bwd.

BUFFERS.  GUARD floats on both sides of every operand and output.  Write sets start as NaN, an output that aliases an operand
starts as that operand; everything else in an output allocation holds SENT and must be bit-identical afterwards (the columns
outside the N written of maskmul_bwd's dw, guards).  Inputs: everything the contract does not read is NaN (the columns outside a
strided w, guards); build(case, garbage=True) puts a large finite value there.  The slabs belong to the wrappers of
wesep_amd.dev, which hand them back on request (run() returns them): they are judged as written, without guards."""
import math

import torch

from tests import gemm_contract as gc
from tests import map_contract as mc
from tests import norm_contract as nc
from tests.gemm_contract import (GUARD, SENT, U, Buf, Built, Case, ContractViolation, Ref, check, eps_for)  # noqa: F401
from tests.norm_contract import Partial, check_partial, sum32  # noqa: F401

GARBAGE, NAN, CAP, TINY = mc.GARBAGE, mc.NAN, 2048, mc.TINY
F64, F32 = torch.float64, torch.float32
LN_EPS, BN_EPS, BN_MOM = 1e-5, 1e-5, 0.1
ULP_EXP, ULP_LOG = mc.ULP_EXP, 3
D_EXP, D_LOG = 2 * ULP_EXP * U, 2 * ULP_LOG * U
ORDERS = ("seq", "pairwise")
E0 = eps_for(False, 0)
ENTRIES = ("prelu_fwd", "prelu_bwd", "dwconv_fwd", "dwconv_bwd", "chan_sums", "norm_ab", "norm_bwd_apply", "maskmul_fwd",
           "maskmul_bwd", "relu_mask", "ola_fwd", "ola_bwd", "sum_partial", "bn_stats", "bn_prelu_fwd", "bn_bwd", "maxpool3_fwd",
           "maxpool3_bwd", "bcast_rows", "cross_entropy")
_ar, _ref, _sum = mc._ar, mc._ref, mc._sum


def _f32(v, dt=F64):
    """A scalar the library receives as a C float, in `dt`."""
    return torch.tensor(v, dtype=F32).to(dt)


def _ones(v):
    return torch.ones(v.shape, dtype=torch.bool)


def _zeros(v):
    return torch.zeros(v.shape, dtype=torch.bool)


# ------------------------------------------------------------------------------------------------------------
# index arithmetic shared by compute and reference
# ------------------------------------------------------------------------------------------------------------
def _stat_rows(sp, t, dt, rows, defect=None, key="stats"):
    """(first, second) [rows, 1] of the [n, 2] table `key` at s = m / st_div."""
    m = _ar(rows)
    nst = -(-rows // sp["st_div"])
    s = m % nst if defect == "stats_by_m" else m // sp["st_div"]
    st = t[key][:2 * nst].reshape(nst, 2).to(dt)
    return st[s, 0:1], st[s, 1:2]


def dw_taps(sp, sign=1, defect=None):
    """(src [M, P] row every tap reads, ok [M, P]): row m + sign (p - ctr) dil inside the sequence of m."""
    R, Tp, P, dil = sp["R"], sp["Tp"], sp["P"], sp["dil"]
    causal = sp["causal"] if defect != "causal_centre" else not sp["causal"]
    ctr = P - 1 if causal else (P - 1) // 2
    m = _ar(R * Tp)
    tq = (m % Tp)[:, None]
    p = _ar(P)[None, :]
    tt = tq + sign * (p - ctr) * dil
    ok = (tt >= 0) & (tt < Tp)
    if defect == "boundary_tap_dropped":
        ok = ok & ~(((tt == 0) | (tt == Tp - 1)) & (p != ctr))
    return (m[:, None] + (tt - tq)).clamp(0, R * Tp - 1), ok


def _xn(sp, t, dt, defect=None):
    """(xn, A) [M, C]: the normalised depthwise operand and the absolute values its four roundings scale with."""
    M, C = sp["R"] * sp["Tp"], sp["C"]
    x = t["x"][:M * C].reshape(M, C).to(dt)
    mean, rstd = _stat_rows(sp, t, dt, M, defect)
    gm, bt = t["gamma"][:C].to(dt), t["beta"][:C].to(dt)
    q = (x - mean) * rstd * gm
    return q + bt, q.abs() + bt.abs()


def _split_sums(terms, sid, n, dt, order):
    """out[s] = sum of the rows of `terms` [M, K] with sid == s, s < n; splits that own no row stay exactly 0."""
    out = torch.zeros(n, terms.shape[1], dtype=dt)
    if dt == F64:
        return out.index_add_(0, sid, terms)
    for s in torch.unique(sid).tolist():
        out[s] = _sum(terms[sid == s].t(), order)
    return out


def _row_split(M, rps, defect=None, lane=0):
    """(split of every row [M], weight [M]) of consecutive splits of rps rows, with the planted split defects."""
    m = _ar(M)
    wgt = torch.ones(M, dtype=F64)
    last = ((m % rps == rps - 1) | (m == M - 1))
    if defect == "split_last_row_skipped":
        wgt[last] = 0.0
    if defect == "lane_twice" and lane:
        wgt[(m % rps == lane)] = 2.0
    return m // rps, wgt


def cs_layout(C):
    """(quads, row lanes) of chan_sums_kernel per z-slice: nq = min(256, C / 4 - 256 z), 256 / nq."""
    out = []
    for z in range(-(-(C // 4) // 256)):
        nq = min(256, C // 4 - 256 * z)
        out.append((nq, 256 // nq))
    return out


def bn_lx(C):
    lx = 1
    while lx < C // 4:
        lx <<= 1
    return min(lx, 256)


def dw_lanes(C):
    return 256 if C // 4 >= 256 else -(-(C // 4) // 64) * 64


def dw_lds(C, P):
    return 3 * (P + 1) * dw_lanes(C) * 16


def _last_quads(C):
    """bool [C]: the channels of the last quad of every z-slice of chan_sums_kernel."""
    keep = torch.zeros(C, dtype=torch.bool)
    for z, (nq, _) in enumerate(cs_layout(C)):
        q = 256 * z + nq - 1
        keep[4 * q:4 * q + 4] = True
    return keep


def ola_taps(sp, defect=None):
    """(src [R Tout, n] index into frames, ok) of every output sample: the frames t with 0 <= j - hop t < L."""
    R, Tp, L, hop, Tout = sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"]
    n = -(-L // hop)
    i = _ar(R * Tout)
    r, j = (i // Tout)[:, None], (i % Tout)[:, None]
    t_hi = torch.div(j, hop, rounding_mode="floor")
    tq = t_hi - _ar(n)[None, :]
    k = j - hop * tq
    ok = (tq >= 0) & (tq < Tp) & (k < L) & (k >= 0)
    if defect == "t_lo_off_by_one":
        ok = ok & (tq > torch.div(L - 1 - j, hop, rounding_mode="floor").neg().clamp_min(0))
    return ((r * Tp + tq.clamp(0, Tp - 1)) * L + k.clamp(0, L - 1)), ok


# ------------------------------------------------------------------------------------------------------------
# compute: the header's formulas, in `dt` (float64: the reference; float32: the emulation), with planted defects
# ------------------------------------------------------------------------------------------------------------
def compute(entry, sp, t, dt=F64, order="seq", defect=None):
    """name -> values of every output of `entry` (slabs as [nsplit, columns])."""
    e = entry
    zero = torch.zeros((), dtype=dt)
    if e == "prelu_fwd":
        rows, C, rpr = sp["rows"], sp["C"], sp["rpr"]
        a = t["a"][0].to(dt)
        pre = t["x"][:rows * C].reshape(rows, C).to(dt)
        if sp["rb"]:
            nrb = -(-rows // rpr)
            idx = _ar(rows) % nrb if defect == "rb_by_m" else _ar(rows) // rpr
            pre = pre + t["rb"][:nrb * C].reshape(nrb, C).to(dt)[idx]
        out = {"y": torch.where(pre > 0, pre, a * pre)}
        if sp["rb"]:
            out["x"] = pre
        return out
    if e == "prelu_bwd":
        n, ns = sp["n"], sp["nslab"]
        a = t["a"][0].to(dt)
        pre, dy = t["pre"][:n].to(dt), t["dy"][:n].to(dt)
        terms = torch.where(pre > 0, zero, dy * pre)
        if defect == "last_quad_skipped":
            terms = terms.clone()
            terms[n - 4:] = 0
        sid = (_ar(n) // 1024) % ns
        slab = _split_sums(terms[:, None], sid, ns, dt, order)
        return {"dx": torch.where(pre > 0, dy, a * dy), "slab": slab, "da": _sum(slab.t(), order)}
    if e in ("dwconv_fwd", "dwconv_bwd"):
        M, C, P = sp["R"] * sp["Tp"], sp["C"], sp["P"]
        w = t["w"][:C * P].reshape(C, P).to(dt)
        xn, _ = _xn(sp, t, dt, defect)
        src, ok = dw_taps(sp, 1, defect)
        if e == "dwconv_fwd":
            terms = torch.where(ok[:, :, None], w.t()[None] * xn[src], zero)          # [M, P, C]
            terms = torch.cat([t["b"][:C].to(dt).expand(M, 1, C), terms], 1)
            return {"y": _sum(terms.permute(0, 2, 1), order)}
        dy = t["dy"][:M * C].reshape(M, C).to(dt)
        srcb, okb = dw_taps(sp, -1, defect)
        dxn = _sum(torch.where(okb[:, :, None], w.t()[None] * dy[srcb], zero).permute(0, 2, 1), order)
        sid, wgt = _row_split(M, sp["rps"], defect)
        terms = torch.cat([torch.where(ok[:, :, None], dy[:, None, :] * xn[src], zero), dy[:, None, :]], 1)
        slab = _split_sums((terms * wgt.to(dt)[:, None, None]).reshape(M, (P + 1) * C), sid, sp["nsplit"], dt, order)
        red = _sum(slab.t(), order).reshape(P + 1, C)
        return {"dxn": dxn, "slab": slab, "dw": red[:P].t(), "db": red[P]}
    if e == "chan_sums":
        C, rpg, ng, ns = sp["C"], sp["rpg"], sp["ng"], sp["nsplit"]
        M = ng * rpg
        g = t["g"][:M * C].reshape(M, C).to(dt)
        s1 = torch.zeros_like(g)
        if sp["mode"] != "g":
            xh = t["x"][:M * C].reshape(M, C).to(dt)
            if sp["mode"] == "gxs":
                mean, rstd = _stat_rows(sp, t, dt, M, defect)
                xh = (xh - mean) * rstd
            s1 = g * xh
        per = -(-rpg // ns)
        m = _ar(M)
        sid, wgt = _row_split(rpg, per, defect)
        sid, wgt = sid.repeat(ng) * ng + m // rpg, wgt.repeat(ng)
        slab = _split_sums((torch.cat([g, s1], 1) * wgt.to(dt)[:, None]), sid, ns * ng, dt, order).reshape(ns, ng, 2, C)
        if defect == "last_quad_skipped":
            slab = slab * (~_last_quads(C)).to(dt)
        return {"slab": slab.reshape(ns, ng * 2 * C), "sums": _sum(slab.reshape(ns, -1).t(), order)}
    if e == "norm_ab":
        C, ng = sp["C"], sp["ng"]
        s = t["sums"][:ng * 2 * C].reshape(ng, 2, C).to(dt)
        prod = s * t["gamma"][:C].to(dt)
        if defect == "one_pass_of_256":
            prod = prod[:, :, :256]
        return {"ab": _sum(prod, order) * (torch.tensor(1.0, dtype=dt) / _f32(float(sp["npg"]), dt))}
    if e == "norm_bwd_apply":
        rows, C = sp["rows"], sp["C"]
        x, dxn = t["x"][:rows * C].reshape(rows, C).to(dt), t["dxn"][:rows * C].reshape(rows, C).to(dt)
        mean, rstd = _stat_rows(sp, t, dt, rows, defect)
        a0, a1 = _stat_rows(sp, t, dt, rows, defect, "ab")
        r = (dxn * t["gamma"][:C].to(dt) - a0 - (x - mean) * rstd * a1) * rstd
        return {"dx": r + t["res"][:rows * C].reshape(rows, C).to(dt) if sp["res"] else r}
    if e in ("maskmul_fwd", "maskmul_bwd"):
        rows, N, ldw, off = sp["rows"], sp["N"], sp["ldw"], sp["w_off"]
        widx = _ar(rows)[:, None] * (N if defect == "ldw_ignored" else ldw) + off + _ar(N)[None, :]
        w = t["w"][widx].to(dt)
        m = t["m"][:rows * N].reshape(rows, N).to(dt)
        if e == "maskmul_fwd":
            return {"s": w * m}
        ds = t["ds"][:rows * N].reshape(rows, N).to(dt)
        return {"dw": ds * m, "dm": torch.where((m >= 0) if defect == "mask_ge" else (m > 0), ds * w, zero)}
    if e == "relu_mask":
        d, y = t["d"][:sp["n"]].to(dt), t["y"][:sp["n"]].to(dt)
        return {"d": torch.where((y >= 0) if defect == "mask_ge" else (y > 0), d, zero)}
    if e == "ola_fwd":
        src, ok = ola_taps(sp, defect)
        terms = torch.where(ok, t["frames"][src].to(dt), zero).flip(1)          # ascending t, as the kernel adds
        bias = t["bias"][0].to(dt) if sp["bias"] else zero
        return {"est": _sum(torch.cat([bias.expand(terms.shape[0], 1), terms], 1), order)}
    if e == "ola_bwd":
        R, Tp, L, hop, Tout = sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"]
        i = _ar(R * Tp * L)
        mrow, k = i // L, i % L
        r, tq = mrow // Tp, mrow % Tp
        j = hop * tq + k
        v = t["dest"][(r * Tout + j).clamp_max(R * Tout - 1)].to(dt)
        return {"dframes": v if defect == "no_tout_test" else torch.where(j < Tout, v, zero)}
    if e == "sum_partial":
        n, ns = sp["n"], sp["nslab"]
        x = t["x"][:n].to(dt)
        if defect == "tail_dropped":
            x = torch.where(_ar(n) < (n // 256) * 256, x, zero)
        slab = _split_sums(x[:, None], (_ar(n) // 256) % ns, ns, dt, order)
        return {"slab": slab, "tot": _sum(slab.t(), order)}
    if e == "bn_stats":
        M, C = sp["M"], sp["C"]
        x = t["x"][:M * C].reshape(M, C).to(dt)
        _, wgt = _row_split(M, -(-M // sp["nsplit"]), defect, 256 // bn_lx(C))
        mean = _sum((x * wgt.to(dt)[:, None]).t(), order) / M
        q = _sum(((x - mean) ** 2).t(), order)
        var = q / M
        out = {"stats": torch.stack([mean, 1 / torch.sqrt(var + _f32(BN_EPS, dt))])}
        if sp["run"]:
            mom = _f32(BN_MOM, dt)
            unb = var if defect == "biased_running_var" else q / (M - 1)
            out["running_mean"] = (1 - mom) * t["running_mean"][:C].to(dt) + mom * mean
            out["running_var"] = (1 - mom) * t["running_var"][:C].to(dt) + mom * unb
        return out
    if e == "bn_prelu_fwd":
        M, C = sp["M"], sp["C"]
        x = t["x"][:M * C].reshape(M, C).to(dt)
        st = t["stats"][:2 * C].reshape(2, C).to(dt)
        a = t["a"][0].to(dt)
        u = (x - st[0]) * st[1] * t["gamma"][:C].to(dt) + t["beta"][:C].to(dt)
        res = t["res"][:M * C].reshape(M, C).to(dt) if sp["res"] else None
        if res is not None and defect != "res_after_prelu":
            u = u + res
        y = torch.where(u > 0, u, a * u)
        if res is not None and defect == "res_after_prelu":
            y, u = y + res, u + res
        return {"u": u, "y": y}
    if e == "bn_bwd":
        M, C, ns = sp["M"], sp["C"], sp["nsplit"]
        x, du = t["x"][:M * C].reshape(M, C).to(dt), t["du"][:M * C].reshape(M, C).to(dt)
        st = t["stats"][:2 * C].reshape(2, C).to(dt)
        xh = (x - st[0]) * st[1]
        sid, wgt = _row_split(M, -(-M // ns), defect, 256 // bn_lx(C))
        slab = _split_sums(torch.cat([du, du * xh], 1) * wgt.to(dt)[:, None], sid, ns, dt, order)
        sums = _sum(slab.t(), order).reshape(2, C)
        inv = torch.tensor(1.0, dtype=dt) / _f32(float(M), dt)
        return {"slab": slab, "sums": sums, "dx": t["gamma"][:C].to(dt) * st[1] * (du - sums[0] * inv - xh * (sums[1] * inv))}
    if e in ("maxpool3_fwd", "maxpool3_bwd"):
        R, T, C = sp["R"], sp["T"], sp["C"]
        To = T // 3
        x = t["x"][:R * T * C].reshape(R, T, C).to(dt)
        win = x[:, :3 * To].reshape(R, To, 3, C)
        if e == "maxpool3_fwd":
            return {"y": (win[:, :, :2] if defect == "window_of_two" else win).max(2).values}
        ge = win == win.max(2, keepdim=True).values
        first = ge & (ge.cumsum(2) == 1)
        if defect == "tie_to_last":
            first = ge & (ge.flip(2).cumsum(2).flip(2) == 1)
        dy = t["dy"][:R * To * C].reshape(R, To, 1, C).to(dt)
        dx = torch.zeros(R, T, C, dtype=dt)
        dx[:, :3 * To] = torch.where(first, dy, zero).reshape(R, 3 * To, C)
        return {"dx": dx}
    if e == "bcast_rows":
        M, C, rpr = sp["M"], sp["C"], sp["rpr"]
        nsrc = -(-M // rpr)
        idx = _ar(M) % nsrc if defect == "row_mod" else _ar(M) // rpr
        return {"out": t["src"][:nsrc * C].reshape(nsrc, C).to(dt)[idx] * _f32(sp["scale"], dt)}
    if e == "cross_entropy":
        R, S = sp["R"], sp["S"]
        z = t["logits"][:R * S].reshape(R, S).to(dt)
        lb = torch.tensor(sp["label"])
        if defect == "label_plus_one":
            lb = (lb + 1) % S
        mx = zero if defect == "no_max" else z.max(1, keepdim=True).values
        lse = mx + torch.log(_sum(torch.exp(z - mx), order)).unsqueeze(1)
        onehot = (_ar(S)[None, :] == lb[:, None]).to(dt)
        per = lse[:, 0] - z[_ar(R), torch.tensor(sp["label"])]
        return {"loss": (_sum(per[None, :], order) / R).reshape(1), "dlogits": (torch.exp(z - lse) - onehot) / R}
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# reference = compute in float64 + the bounds of the module docstring
# ------------------------------------------------------------------------------------------------------------
def _slab_ref(v, S, bound, nsplit, empty):
    """Partial over a slab [nsplit, n]: the float64 sum over the splits against (val, bound); `empty` splits are exact zeros."""
    n = S.numel()
    zero = torch.zeros(nsplit, n, dtype=torch.bool)
    zero[[s for s in range(nsplit) if empty(s)]] = True
    return Partial(_ar(nsplit * n).reshape(nsplit, n), v.reshape(nsplit, n).sum(0), S.reshape(-1), bound.reshape(-1), zero)


def _red_ref(val, S, bound, nsplit):
    """The wrapper's ws_reduce_slabs over the splits on top of the slab's bound."""
    return _ref(_ar(val.numel()), val, S, bound + eps_for(False, nsplit) * S)


def _ew(val, bound, exact=None, idx=None):
    return _ref(_ar(val.numel()) if idx is None else idx, val, val.abs(), bound, exact)


def reference(b, tensors=None, entry=None):
    """name -> Ref | Partial of every output of the built case over `tensors` (default: the case's own buffers)."""
    e, sp = entry or b.case.entry, b.spec
    t = b.views(tensors or b.bufs)
    v = compute(e, sp, t, F64)
    if e == "prelu_fwd":
        a = abs(float(t["a"][0]))
        pre = v["x"] if sp["rb"] else t["x"][:sp["rows"] * sp["C"]].reshape(sp["rows"], sp["C"]).double()
        y = v["y"]
        dpre = U * pre.abs() if sp["rb"] else torch.zeros_like(pre)
        out = {"y": _ew(y, max(1.0, a) * dpre + U * y.abs() * (pre <= 0), (pre > 0) if not sp["rb"] else None)}
        if sp["rb"]:
            out["x"] = _ew(pre, dpre)
        return out
    if e == "prelu_bwd":
        n, ns = sp["n"], sp["nslab"]
        pre, dy = t["pre"][:n].double(), t["dy"][:n].double()
        S = torch.where(pre > 0, torch.zeros_like(dy), (dy * pre).abs()).sum().reshape(1)
        bd = eps_for(False, n + 1) * S
        dx = v["dx"]
        return {"dx": _ew(dx, U * dx.abs(), pre > 0), "slab": _slab_ref(v["slab"], S, bd, ns, lambda s: s * 256 >= n // 4),
                "da": _red_ref(v["da"], S, bd, ns)}
    if e in ("dwconv_fwd", "dwconv_bwd"):
        M, C, P = sp["R"] * sp["Tp"], sp["C"], sp["P"]
        wa = t["w"][:C * P].reshape(C, P).double().abs()
        _, A = _xn(sp, t, F64)
        src, ok = dw_taps(sp, 1)
        if e == "dwconv_fwd":
            S = t["b"][:C].double().abs() + (wa.t()[None] * A[src] * ok[:, :, None]).sum(1)
            return {"y": _ref(_ar(M * C), v["y"], S, (eps_for(False, P + 1) + 4 * U) * S)}
        dya = t["dy"][:M * C].reshape(M, C).double().abs()
        srcb, okb = dw_taps(sp, -1)
        Sx = (wa.t()[None] * dya[srcb] * okb[:, :, None]).sum(1)
        Ss = torch.cat([(dya[:, None, :] * A[src] * ok[:, :, None]).sum(0), dya.sum(0, keepdim=True)], 0)
        bd = torch.cat([(eps_for(False, M + 1) + 4 * U) * Ss[:P], eps_for(False, M) * Ss[P:]], 0)
        ns = sp["nsplit"]
        return {"dxn": _ref(_ar(M * C), v["dxn"], Sx, eps_for(False, P + 1) * Sx),
                "slab": _slab_ref(v["slab"], Ss, bd, ns, lambda s: s * sp["rps"] >= M),
                "dw": _red_ref(v["dw"], Ss[:P].t(), bd[:P].t(), ns), "db": _red_ref(v["db"], Ss[P], bd[P], ns)}
    if e == "chan_sums":
        C, rpg, ng, ns = sp["C"], sp["rpg"], sp["ng"], sp["nsplit"]
        ta = dict(t, g=t["g"].abs())
        if sp["mode"] == "gx":
            ta["x"] = t["x"].abs()
        va = compute(e, sp, ta, F64)["slab"].reshape(ns, ng, 2, C).sum(0)
        if sp["mode"] == "gxs":
            M = ng * rpg
            mean, rstd = _stat_rows(sp, t, F64, M)
            xh = (t["x"][:M * C].reshape(M, C).double() - mean) * rstd
            va[:, 1] = (t["g"][:M * C].reshape(M, C).double() * xh).abs().reshape(ng, rpg, C).sum(1)
        bd = torch.stack([eps_for(False, rpg) * va[:, 0], (eps_for(False, rpg + 1) + (2 * U if sp["mode"] == "gxs" else 0)) * va[:, 1]], 1)
        per = -(-rpg // ns)
        p = _slab_ref(v["slab"], va, bd, ns, lambda s: s * per >= rpg)
        if sp["mode"] == "g":
            p.zero.reshape(ns, ng, 2, C)[:, :, 1] = True
        r = _red_ref(v["sums"], va.reshape(-1), bd.reshape(-1), ns)
        if sp["mode"] == "g":
            ex = torch.zeros(ng, 2, C, dtype=torch.bool)
            ex[:, 1] = True
            r = r._replace(exact=ex.reshape(-1))
        return {"slab": p, "sums": r}
    if e == "norm_ab":
        C, ng = sp["C"], sp["ng"]
        S = (t["sums"][:ng * 2 * C].reshape(ng, 2, C).double() * t["gamma"][:C].double()).abs().sum(2) / sp["npg"]
        return {"ab": _ref(_ar(ng * 2), v["ab"], S, (eps_for(False, C + 1) + 2 * U) * S)}
    if e == "norm_bwd_apply":
        rows, C = sp["rows"], sp["C"]
        x, dxn = t["x"][:rows * C].reshape(rows, C).double(), t["dxn"][:rows * C].reshape(rows, C).double()
        mean, rstd = _stat_rows(sp, t, F64, rows)
        a0, a1 = _stat_rows(sp, t, F64, rows, key="ab")
        S = rstd.abs() * ((dxn * t["gamma"][:C].double()).abs() + a0.abs() + ((x - mean) * rstd * a1).abs())
        if sp["res"]:
            S = S + t["res"][:rows * C].reshape(rows, C).double().abs()
        return {"dx": _ref(_ar(rows * C), v["dx"], S, E0 * S)}
    if e == "maskmul_fwd":
        return {"s": _ew(v["s"], U * v["s"].abs())}
    if e == "maskmul_bwd":
        rows, N = sp["rows"], sp["N"]
        m = t["m"][:rows * N].reshape(rows, N)
        idx = _ar(rows)[:, None] * sp["ld_dw"] + sp["dw_off"] + _ar(N)[None, :]
        return {"dw": _ew(v["dw"], U * v["dw"].abs(), idx=idx), "dm": _ew(v["dm"], U * v["dm"].abs(), ~(m > 0))}
    if e == "relu_mask":
        return {"d": _ew(v["d"], torch.zeros_like(v["d"]), _ones(v["d"]))}
    if e == "ola_fwd":
        src, ok = ola_taps(sp)
        ba = float(t["bias"][0].abs()) if sp["bias"] else 0.0
        S = ba + (t["frames"][src].double().abs() * ok).sum(1)
        cnt = ok.sum(1) + (1 if sp["bias"] else 0)
        return {"est": _ref(_ar(S.numel()), v["est"], S, eps_for(False, -(-sp["L"] // sp["hop"]) + 1) * S, cnt <= 1)}
    if e == "ola_bwd":
        return {"dframes": _ew(v["dframes"], torch.zeros_like(v["dframes"]), _ones(v["dframes"]))}
    if e == "sum_partial":
        n, ns = sp["n"], sp["nslab"]
        S = t["x"][:n].double().abs().sum().reshape(1)
        bd = eps_for(False, n) * S
        return {"slab": _slab_ref(v["slab"], S, bd, ns, lambda s: s * 256 >= n), "tot": _red_ref(v["tot"], S, bd, ns)}
    if e == "bn_stats":
        M, C = sp["M"], sp["C"]
        x = t["x"][:M * C].reshape(M, C).double()
        eps = float(_f32(BN_EPS))
        m, rstd, d_m, lo, hi, ma = nc.stats_interval(x.t(), eps)
        val = torch.stack([m, (lo + hi) / 2])
        out = {"stats": _ref(_ar(2 * C), val, torch.stack([ma, rstd]), torch.stack([d_m, (hi - lo) / 2]))}
        if sp["run"]:
            mom = float(_f32(BN_MOM))
            var = ((x - m) ** 2).mean(0)
            d_v = eps_for(False, M) * (var + d_m ** 2) + d_m ** 2
            k = M / (M - 1)
            om, ov = (1 - mom) * t["running_mean"][:C].double(), (1 - mom) * t["running_var"][:C].double()
            Sm, Sv = om.abs() + mom * m.abs(), ov.abs() + mom * var * k
            out["running_mean"] = _ref(_ar(C), v["running_mean"], Sm, mom * d_m + E0 * Sm)
            out["running_var"] = _ref(_ar(C), v["running_var"], Sv, mom * d_v * k + E0 * Sv)
        return out
    if e == "bn_prelu_fwd":
        M, C = sp["M"], sp["C"]
        x = t["x"][:M * C].reshape(M, C).double()
        st = t["stats"][:2 * C].reshape(2, C).double()
        a = abs(float(t["a"][0]))
        S = ((x - st[0]) * st[1] * t["gamma"][:C].double()).abs() + t["beta"][:C].double().abs()
        if sp["res"]:
            S = S + t["res"][:M * C].reshape(M, C).double().abs()
        return {"u": _ref(_ar(M * C), v["u"], S, E0 * S), "y": _ref(_ar(M * C), v["y"], S, max(1.0, a) * E0 * S + U * v["y"].abs())}
    if e == "bn_bwd":
        M, C, ns = sp["M"], sp["C"], sp["nsplit"]
        x, du = t["x"][:M * C].reshape(M, C).double(), t["du"][:M * C].reshape(M, C).double()
        st = t["stats"][:2 * C].reshape(2, C).double()
        xh = (x - st[0]) * st[1]
        Ss = torch.stack([du.abs().sum(0), (du * xh).abs().sum(0)])
        bd = torch.stack([eps_for(False, M) * Ss[0], (eps_for(False, M + 1) + 2 * U) * Ss[1]])
        red = _red_ref(v["sums"], Ss, bd, ns)
        rb = red.bound.reshape(2, C)
        gr = (t["gamma"][:C].double() * st[1]).abs()
        S = gr * (du.abs() + v["sums"][0].abs() / M + (xh * v["sums"][1]).abs() / M)
        rps = -(-M // ns)
        return {"slab": _slab_ref(v["slab"], Ss, bd, ns, lambda s: s * rps >= M), "sums": red,
                "dx": _ref(_ar(M * C), v["dx"], S, E0 * S + gr * (rb[0] + xh.abs() * rb[1]) / M)}
    if e == "maxpool3_fwd":
        return {"y": _ew(v["y"], torch.zeros_like(v["y"]), _ones(v["y"]))}
    if e == "maxpool3_bwd":
        return {"dx": _ew(v["dx"], torch.zeros_like(v["dx"]), _ones(v["dx"]))}
    if e == "bcast_rows":
        o = v["out"]
        return {"out": _ew(o, U * o.abs(), torch.full(o.shape, float(_f32(sp["scale"])) == 1.0))}
    if e == "cross_entropy":
        R, S = sp["R"], sp["S"]
        x = t["logits"][:R * S].reshape(R, S).double()
        mx = x.max(1, keepdim=True).values
        z = x - mx
        rho = D_EXP + torch.expm1(U * z.abs())
        se = torch.exp(z).sum(1, keepdim=True)
        y = torch.exp(z) / se
        lse = mx + torch.log(se)
        d_lse = (y * rho).sum(1, keepdim=True) + eps_for(False, S) + D_LOG * torch.log(se).abs() + U * lse.abs()
        d_a = d_lse + U * (x - lse).abs()
        dl = v["dlogits"]
        per = (lse[:, 0] - x[_ar(R), torch.tensor(sp["label"])])
        Sl = per.abs().sum().reshape(1) / R
        bl = (d_lse[:, 0] + U * per.abs()).sum().reshape(1) / R + eps_for(False, R + 1) * Sl
        return {"loss": _ref(_ar(1), v["loss"], Sl, bl),
                "dlogits": _ref(_ar(R * S), dl, y / R, (y * (D_EXP + torch.expm1(d_a)) + TINY) / R + 2 * U * dl.abs())}
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, targets
# ------------------------------------------------------------------------------------------------------------
SLOPES = [0.0, 0.25, 1.0, -0.5]
DW = dict(C=[4, 24, 260, 768, 776, 1028], P=[1, 3, 5, 7], dil=[1, 2, 8], Tp=[1, 2, 7, 53], R=[1, 3], st=["Tp", "1"], causal=[0, 1])
OLA = dict(Lh=[(1, 1), (4, 2), (5, 2), (7, 7), (80, 10), (3, 5)], Tp=[1, 2, 41], Tout=["1", "Tp*hop", "mid", "full"], R=[1, 2])
BN = dict(C=[4, 12, 20, 32, 256, 1028], M=[2, 3, 257], nsplit=["1", "3", "5", "M+1"], data=["gauss", "offset"])
DIMS = {
    "prelu_fwd": dict(C=[4, 12, 40, 1028], rows=[1, 5, 33], rpr=["1", "5", "rows"], rb=[0, 1], slope=SLOPES),
    "prelu_bwd": dict(n4=[1, 255, 257, 1030], nslab=[1, 3, 7], slope=SLOPES, alias=[0, 1]),
    "dwconv_fwd": dict(DW),
    "dwconv_bwd": dict(DW, rps=["1", "3", "5", "M"], over=[0, 2]),
    "chan_sums": dict(C=[4, 12, 16, 40, 512, 1028], rpg=[1, 5, 257], ng=[1, 3], nsplit=["1", "3", "rpg+2"], mode=["g", "gx", "gxs"],
                      st=["1", "rpg"]),
    "norm_ab": dict(C=[1, 3, 255, 256, 257, 600], ng=[1, 3]),
    "norm_bwd_apply": dict(C=[4, 12, 1028], Tp=[1, 7], R=[1, 3], res=[0, 1], alias=[0, 1], st=["1", "Tp"]),
    "maskmul_fwd": dict(N=[4, 12, 256], ldw=["N", "3N", "N+4"], rows=[1, 5, 33]),
    "maskmul_bwd": dict(N=[4, 12, 256], ldw=["N", "3N", "N+4"], ld_dw=["N", "3N", "N+4"], rows=[1, 5, 33]),
    "relu_mask": dict(n=[4, 1020, 1028, 4100]),
    "ola_fwd": dict(OLA, bias=[0, 1]),
    "ola_bwd": dict(OLA),
    "sum_partial": dict(n=[1, 255, 1027, 5000], nslab=[1, 5, 40]),
    "bn_stats": dict(BN, run=[0, 1]),
    "bn_prelu_fwd": dict(C=[4, 12, 1028], M=[1, 3, 33], res=[0, 1], slope=SLOPES),
    "bn_bwd": dict(BN, alias=[0, 1]),
    "maxpool3_fwd": dict(T=[3, 4, 5, 7, 9], R=[1, 2], C=[4, 40]),
    "maxpool3_bwd": dict(T=[3, 4, 5, 7, 9], R=[1, 2], C=[4, 40]),
    "bcast_rows": dict(M=[1, 7, 20], rpr=["1", "7", "M"], scale=[1.0, 1 / 7], C=[4, 12]),
    "cross_entropy": dict(S=[1, 2, 63, 64, 255, 256, 257, 1000], R=[1, 3], label=["0", "S-1", "rand"], data=["gauss", "+80", "-80", "equal"]),
}
RULES = {e: [] for e in ENTRIES}
RULES["dwconv_bwd"] = [("more than 64 KB of dynamic LDS only in the three hand-written cases", ("C", "P"), lambda C, P: dw_lds(C, P) > 65536)]
RULES["chan_sums"] = [("st_div exists only with stats", ("mode", "st"), lambda m, st: m != "gxs" and st != "1")]
RULES["maskmul_bwd"] = [("ld_dw differs from ldw", ("ldw", "ld_dw"), lambda a, b_: a == b_)]


def _rpr(d, rows):
    return {"1": 1, "5": 5, "7": 7, "rows": rows, "M": rows}[d["rpr"]]


def dw_split(d):
    """(nsplit, rows_per_split) of a dwconv_bwd case."""
    M = d["R"] * d["Tp"]
    rps = M if d["rps"] == "M" else int(d["rps"])
    return -(-M // rps) + d["over"], rps


def _ns(d, key, n):
    return {"rpg+2": n + 2, "M+1": n + 1}.get(d[key]) or int(d[key])


def ola_tout(d):
    (L, hop), Tp = d["Lh"], d["Tp"]
    full = (Tp - 1) * hop + L
    return {"1": 1, "Tp*hop": min(Tp * hop, full), "mid": (Tp - 1) * hop + (L + 1) // 2, "full": full}[d["Tout"]]


def _targets(entry, d, seed=0):
    e = entry
    if e == "prelu_fwd":
        return ("prelu_fwd_kernel", f"prelu_fwd[rb {'on' if d['rb'] else 'NULL'}]")
    if e == "prelu_bwd":
        n4, ns = d["n4"], d["nslab"]
        return (("prelu_bwd_kernel",) + (("prelu_bwd[dx aliases dy]",) if d["alias"] else ()) + (("prelu_bwd[empty block]",) if (ns - 1) * 256 >= n4 else ())
                + (("prelu_bwd[second trip]",) if n4 > ns * 256 else ()))
    if e in ("dwconv_fwd", "dwconv_bwd"):
        P, dil, Tp = d["P"], d["dil"], d["Tp"]
        k = "fwd" if e == "dwconv_fwd" else "bwd"
        t = (f"dwconv_{k}[causal {d['causal']}]",)
        if P > 1 and dil * (1 if d["causal"] else (P - 1) // 2) >= Tp:
            t += (f"dwconv_{k}[every off-centre tap outside]",)
        if e == "dwconv_fwd":
            return ("dwconv_fwd_kernel",) + t
        ns, rps = dw_split(d)
        M = d["R"] * Tp
        t += (f"dwconv_bwd_w_kernel[{dw_lanes(d['C'])} lanes]",)
        t += ("dwconv_bwd_w_kernel[two y slices]",) if d["C"] // 4 > 256 else ()
        t += ("dwconv_bwd_w_kernel[empty split]",) if (ns - 1) * rps >= M else ()
        t += ("dwconv_bwd_w_kernel[split straddles a sequence]",) if d["R"] > 1 and rps < M and Tp % rps and rps > 1 else ()
        t += ("dwconv_bwd_w_kernel[LDS above 64 KB]",) if dw_lds(d["C"], P) > 65536 else ()
        return ("dwconv_bwd_dx_kernel",) + t
    if e == "chan_sums":
        lay = cs_layout(d["C"])
        ns, rpg = _ns(d, "nsplit", d["rpg"]), d["rpg"]
        per = -(-rpg // ns)
        t = (f"chan_sums[{ {'g': 'x NULL', 'gx': 'x without stats', 'gxs': 'x with stats'}[d['mode']] }]",)
        t += ("chan_sums[idle threads]",) if any(256 % nq for nq, _ in lay) else ()
        t += ("chan_sums[second z slice]",) if len(lay) > 1 else ()
        t += ("chan_sums[empty split]",) if (ns - 1) * per >= rpg else ()
        t += ("chan_sums[rows beyond the row lanes]",) if per > min(n for _, n in lay) else ()
        return t
    if e == "norm_ab":
        return ("norm_ab_kernel",) + (("norm_ab[C above 256]",) if d["C"] > 256 else ())
    if e == "norm_bwd_apply":
        return ("norm_bwd_apply_cl_kernel", f"norm_bwd_apply[res {'on' if d['res'] else 'NULL'}]") + (("norm_bwd_apply[dx aliases dxn]",) if d["alias"] else ())
    if e == "maskmul_fwd":
        return ("maskmul_fwd_kernel",) + (("maskmul_fwd[strided w]",) if d["ldw"] != "N" else ())
    if e == "maskmul_bwd":
        return ("maskmul_bwd_kernel",) + (("maskmul_bwd[strided dw]",) if d["ld_dw"] != "N" else ())
    if e == "ola_fwd":
        (L, hop) = d["Lh"]
        return ("ola_fwd_kernel", f"ola_fwd[bias {'on' if d['bias'] else 'NULL'}]") + (("ola_fwd[gaps]",) if hop > L and d["Tp"] > 1 and ola_tout(d) > hop else ()) + (
            ("ola_fwd[cropped]",) if ola_tout(d) < (d["Tp"] - 1) * hop + L else ())
    if e == "ola_bwd":
        (L, hop) = d["Lh"]
        return ("ola_bwd_kernel",) + (("ola_bwd[zeros past Tout]",) if ola_tout(d) < (d["Tp"] - 1) * hop + L else ())
    if e == "sum_partial":
        return ("sum_partial_kernel",) + (("sum_partial[empty block]",) if (d["nslab"] - 1) * 256 >= d["n"] else ()) + (
            ("sum_partial[second trip]",) if d["n"] > d["nslab"] * 256 else ())
    if e in ("bn_stats", "bn_bwd"):
        C, M = d["C"], d["M"]
        ns = _ns(d, "nsplit", M)
        k = "bn_partial_kernel" if e == "bn_stats" else "bn_bwd_sums_kernel"
        t = (k,)
        t += (f"{k}[dead quads]",) if (C // 4) % bn_lx(C) else ()
        t += (f"{k}[two y slices]",) if C // 4 > 256 else ()
        t += (f"{k}[empty split]",) if (ns - 1) * -(-M // ns) >= M else ()
        t += (f"{k}[rows beyond the row lanes]",) if -(-M // ns) > 256 // bn_lx(C) else ()
        if e == "bn_stats":
            t += (f"bn_final_kernel[running {'on' if d['run'] else 'NULL'}]",) + (("bn_final_kernel[splits folded over 4 lanes]",) if ns > 4 else ())
        else:
            t += ("bn_bwd_apply_kernel",) + (("bn_bwd_apply[dx aliases du]",) if d["alias"] else ())
        return t
    if e == "bn_prelu_fwd":
        return ("bn_prelu_fwd_kernel", f"bn_prelu_fwd[res {'on' if d['res'] else 'NULL'}]")
    if e in ("maxpool3_fwd", "maxpool3_bwd"):
        return (f"{e}_kernel",) + ((f"{e}[tail rows]",) if d["T"] % 3 else ())
    if e == "bcast_rows":
        return ("bcast_rows_kernel", "bcast_rows[scale 1]" if d["scale"] == 1.0 else "bcast_rows[scaled]") + (
            ("bcast_rows[ragged last group]",) if d["M"] % _rpr(d, d["M"]) else ())
    if e == "cross_entropy":
        return ("ce_kernel", "ce_kernel[S above 256]" if d["S"] > 256 else "ce_kernel[one trip]")
    return (f"{e}_kernel",)


_M = gc.MIN_PER_TARGET
_BNK = {"bn_stats": "bn_partial_kernel", "bn_bwd": "bn_bwd_sums_kernel"}
TOPUP = {e: [({}, _targets(e, {k: v[0] for k, v in DIMS[e].items()})[0], _M)] for e in ENTRIES}
TOPUP["prelu_fwd"] += [({"rb": r}, f"prelu_fwd[rb {'on' if r else 'NULL'}]", _M) for r in (0, 1)]
TOPUP["prelu_fwd"] += [({"rows": 33, "rpr": "5", "rb": 1}, "prelu_fwd[rb on]", 1)]          # rows_per_r that divides nothing, with rb
TOPUP["prelu_bwd"] += [({"alias": 1}, "prelu_bwd[dx aliases dy]", _M), ({"n4": 255, "nslab": 3}, "prelu_bwd[empty block]", _M),
                       ({"n4": 1030, "nslab": 3}, "prelu_bwd[second trip]", _M)]
for _k in ("fwd", "bwd"):
    TOPUP[f"dwconv_{_k}"] += [({"causal": c}, f"dwconv_{_k}[causal {c}]", _M) for c in (0, 1)] + [
        ({"dil": 8, "Tp": 7, "P": 3}, f"dwconv_{_k}[every off-centre tap outside]", _M)]
TOPUP["dwconv_bwd"] += [({"C": c}, f"dwconv_bwd_w_kernel[{n} lanes]", _M) for c, n in ((24, 64), (260, 128), (768, 192), (776, 256))] + [
    ({"C": 1028}, "dwconv_bwd_w_kernel[two y slices]", _M), ({"over": 2}, "dwconv_bwd_w_kernel[empty split]", _M),
    ({"R": 3, "Tp": 7, "rps": "5"}, "dwconv_bwd_w_kernel[split straddles a sequence]", _M)]
TOPUP["chan_sums"] = [({"mode": m}, f"chan_sums[{n}]", _M) for m, n in (("g", "x NULL"), ("gx", "x without stats"), ("gxs", "x with stats"))] + [
    ({"C": 12}, "chan_sums[idle threads]", _M), ({"C": 1028}, "chan_sums[second z slice]", _M), ({"nsplit": "rpg+2"}, "chan_sums[empty split]", _M),
    ({"rpg": 257, "nsplit": "1"}, "chan_sums[rows beyond the row lanes]", _M)]
TOPUP["relu_mask"] += [({"n": n}, "relu_mask_kernel", 1) for n in DIMS["relu_mask"]["n"]]
TOPUP["norm_ab"] += [({"C": 600}, "norm_ab[C above 256]", _M)]
TOPUP["norm_bwd_apply"] += [({"res": r}, f"norm_bwd_apply[res {'on' if r else 'NULL'}]", _M) for r in (0, 1)] + [({"alias": 1}, "norm_bwd_apply[dx aliases dxn]", _M)]
TOPUP["maskmul_fwd"] += [({"ldw": "3N"}, "maskmul_fwd[strided w]", _M)]
TOPUP["maskmul_bwd"] += [({"ld_dw": "3N"}, "maskmul_bwd[strided dw]", _M)]
TOPUP["ola_fwd"] += [({"bias": r}, f"ola_fwd[bias {'on' if r else 'NULL'}]", _M) for r in (0, 1)] + [
    ({"Lh": (3, 5), "Tp": 41}, "ola_fwd[gaps]", _M), ({"Tout": "mid", "Tp": 2}, "ola_fwd[cropped]", _M)]
TOPUP["ola_bwd"] += [({"Tout": "mid", "Tp": 2}, "ola_bwd[zeros past Tout]", _M)]
TOPUP["sum_partial"] += [({"n": 255, "nslab": 5}, "sum_partial[empty block]", _M), ({"n": 5000, "nslab": 5}, "sum_partial[second trip]", _M)]
for _e, _k in _BNK.items():
    TOPUP[_e] += [({"C": 12}, f"{_k}[dead quads]", _M), ({"C": 1028}, f"{_k}[two y slices]", _M), ({"nsplit": "M+1"}, f"{_k}[empty split]", _M),
                  ({"M": 257, "nsplit": "1"}, f"{_k}[rows beyond the row lanes]", _M)]
TOPUP["bn_stats"] += [({"run": r}, f"bn_final_kernel[running {'on' if r else 'NULL'}]", _M) for r in (0, 1)] + [
    ({"nsplit": "5"}, "bn_final_kernel[splits folded over 4 lanes]", _M)]
TOPUP["bn_bwd"] += [({}, "bn_bwd_apply_kernel", _M), ({"alias": 1}, "bn_bwd_apply[dx aliases du]", _M)]
TOPUP["bn_prelu_fwd"] += [({"res": r}, f"bn_prelu_fwd[res {'on' if r else 'NULL'}]", _M) for r in (0, 1)]
for _e in ("maxpool3_fwd", "maxpool3_bwd"):
    TOPUP[_e] += [({"T": 7}, f"{_e}[tail rows]", _M)]
TOPUP["bcast_rows"] += [({"scale": 1.0}, "bcast_rows[scale 1]", _M), ({"scale": 1 / 7}, "bcast_rows[scaled]", _M),
                        ({"M": 20, "rpr": "7"}, "bcast_rows[ragged last group]", _M)]
TOPUP["cross_entropy"] += [({"S": 1000}, "ce_kernel[S above 256]", _M), ({"S": 255}, "ce_kernel[one trip]", _M)]
INST = {e: list(dict.fromkeys(tag for _, tag, _ in TOPUP[e])) for e in ENTRIES}
INST["dwconv_bwd"].append("dwconv_bwd_w_kernel[LDS above 64 KB]")
EXACT_COUNT = {"dwconv_bwd_w_kernel[LDS above 64 KB]": 3}          # the hand-written cases of EXTRA, once each
_BIG = dict(dil=1, Tp=7, R=2, st="Tp", causal=0, rps="5", over=0)
EXTRA = {
    "dwconv_bwd": [dict(C=768, P=7, **_BIG), dict(C=776, P=5, **_BIG), dict(C=776, P=7, **dict(_BIG, causal=1, st="1"))],
}
PLAIN = {"dwconv_fwd": dict(C=24, P=3, dil=2, Tp=7, R=3, st="Tp", causal=0),
         "dwconv_bwd": dict(C=24, P=3, dil=2, Tp=7, R=3, st="Tp", causal=0, rps="5", over=0)}
_KEY = {e: "tn_" + e for e in ENTRIES}          # the registries of gemm_contract are shared by every suite
for _i, _e in enumerate(ENTRIES):
    gc.DIMS[_KEY[_e]], gc.RULES[_KEY[_e]], gc.INST[_KEY[_e]], gc.TOPUP[_KEY[_e]] = DIMS[_e], RULES[_e], INST[_e], TOPUP[_e]
    gc.SEEDS[_KEY[_e]] = 101 + _i
    gc.PLANNERS[_KEY[_e]] = (lambda e: lambda d, seed: _targets(e, d, seed))(_e)
_CASES = {}


def cases(entry):
    if entry not in _CASES:
        out = [c._replace(entry=entry) for c in gc.cases(_KEY[entry])]
        for i, d in enumerate(EXTRA.get(entry, [])):
            out.append(Case(entry, f"x{i:02d}-" + "-".join(str(v) for v in d.values()), d, _targets(entry, d), 8000 + i))
        _CASES[entry] = out
    return _CASES[entry]


def plain_case(entry):
    """The one case of a plain wrapper (ws_dwconv_fwd / ws_dwconv_bwd): the _ex entry with causal = 0."""
    d = PLAIN[entry]
    return Case(entry, "plain-" + "-".join(str(v) for v in d.values()), d, (f"ws_{entry}[plain wrapper]",), 8100)


def invalid_pairs(entry):
    return gc.invalid_pairs(_KEY[entry])


def all_pairs(entry):
    return gc.all_pairs(_KEY[entry])


def pairs_of(entry, dims):
    return gc.pairs_of(_KEY[entry], dims)


# ------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------
class TBuilt(mc.MBuilt):
    """map_contract.MBuilt + extras: the outputs the wrappers of wesep_amd.dev allocate and hand back (slabs, reduced sums)."""
    def __init__(self, case):
        super().__init__(case)
        self.extras = []


def _stats_of(x, groups, eps=LN_EPS):
    """[groups, 2] float64 (mean, rstd) of x split into `groups` contiguous groups."""
    v = x.double().reshape(groups, -1)
    m = v.mean(1)
    return torch.stack([m, 1 / torch.sqrt(((v - m[:, None]) ** 2).mean(1) + eps)], 1)


def _spiked(v):
    v = v.clone()
    v.reshape(-1)[-1] = math.copysign(max(abs(float(v.reshape(-1)[-1])), 0.5), float(v.reshape(-1)[-1])) * 1e3
    return v


def _zeroed(g, v, every=7):
    v = v.clone()
    v.reshape(-1)[::every] = 0.0
    return v


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

    if e == "prelu_fwd":
        rows, C = d["rows"], d["C"]
        rpr = _rpr(d, rows)
        sp.update(rows=rows, C=C, rpr=rpr, rb=d["rb"])
        x = _zeroed(g, rn(rows, C))
        if d["rb"]:
            rb = rn(-(-rows // rpr), C)
            x[:, 1::4] = -rb[_ar(rows) // rpr][:, 1::4]          # pre exactly 0
            inp("rb", rb)
        inp("x", x)
        inp("a", torch.tensor([d["slope"]]))
        if d["rb"]:
            out("x", rows * C, alias="x")
        out("y", rows * C)
        return b
    if e == "prelu_bwd":
        n = 4 * d["n4"]
        sp.update(n=n, nslab=d["nslab"])
        pre, dy = _zeroed(g, rn(n)), rn(n)
        if n > CAP:
            pre, dy = _spiked(pre), _spiked(dy)
            pre[-1] = -pre[-1].abs()
        inp("pre", pre)
        inp("dy", dy)
        inp("a", torch.tensor([d["slope"]]))
        out("dx", n, alias="dy" if d["alias"] else None)
        b.extras += ["slab", "da"]
        return b
    if e in ("dwconv_fwd", "dwconv_bwd"):
        C, P, Tp, R = d["C"], d["P"], d["Tp"], d["R"]
        M = R * Tp
        st_div = Tp if d["st"] == "Tp" else 1
        sp.update(R=R, Tp=Tp, C=C, P=P, dil=d["dil"], st_div=st_div, causal=bool(d["causal"]))
        x = rn(M, C) + 0.5
        if e == "dwconv_bwd":
            sp["nsplit"], sp["rps"] = dw_split(d)
            inp("dy", rn(M, C))
        inp("x", x)
        inp("stats", _stats_of(x, M // st_div))
        inp("gamma", rn(C) + 1.0)
        inp("beta", rn(C))
        inp("w", rn(C, P))
        if e == "dwconv_fwd":
            inp("b", rn(C))
            out("y", M * C)
        else:
            out("dxn", M * C)
            b.extras += ["slab", "dw", "db"]
        return b
    if e == "chan_sums":
        C, rpg, ng = d["C"], d["rpg"], d["ng"]
        M = ng * rpg
        sp.update(C=C, rpg=rpg, ng=ng, nsplit=_ns(d, "nsplit", rpg), mode=d["mode"], st_div=rpg if d["st"] == "rpg" else 1)
        x = rn(M, C) + 0.5
        inp("g", rn(M, C))
        if d["mode"] != "g":
            inp("x", x)
        if d["mode"] == "gxs":
            inp("stats", _stats_of(x, M // sp["st_div"]))
        b.extras += ["slab", "sums"]
        return b
    if e == "norm_ab":
        C, ng = d["C"], d["ng"]
        sp.update(C=C, ng=ng, npg=7 * C)
        inp("sums", rn(ng, 2, C) * 3)
        inp("gamma", rn(C) + 1.0)
        out("ab", ng * 2)
        return b
    if e == "norm_bwd_apply":
        C, Tp, R = d["C"], d["Tp"], d["R"]
        rows = R * Tp
        st_div = Tp if d["st"] == "Tp" else 1
        sp.update(rows=rows, C=C, st_div=st_div, res=d["res"])
        x = rn(rows, C) + 0.5
        inp("x", x)
        inp("dxn", rn(rows, C))
        inp("stats", _stats_of(x, rows // st_div))
        inp("ab", rn(rows // st_div, 2) * 0.3)
        inp("gamma", rn(C) + 1.0)
        if d["res"]:
            inp("res", rn(rows, C))
        out("dx", rows * C, alias="dxn" if d["alias"] else None)
        return b
    if e in ("maskmul_fwd", "maskmul_bwd"):
        N, rows = d["N"], d["rows"]
        ld = lambda v: {"N": N, "3N": 3 * N, "N+4": N + 4}[v]          # noqa: E731
        ldw = ld(d["ldw"])
        sp.update(rows=rows, N=N, ldw=ldw, w_off={"N": 0, "3N": N, "N+4": 4}[d["ldw"]])
        rd = torch.zeros(rows, ldw, dtype=torch.bool)
        rd[:, sp["w_off"]:sp["w_off"] + N] = True
        m = torch.relu(rn(rows, N))          # the ReLU output of the mask GEMM: exact zeros
        m[:, 2::5] = -m[:, 2::5] - 0.25          # and negative values a ReLU would not leave: the backward tests m > 0
        if e == "maskmul_bwd":
            inp("ds", rn(rows, N))
        inp("w", rn(rows, ldw), rd)
        inp("m", m)
        if e == "maskmul_fwd":
            out("s", rows * N)
        else:
            ldd = ld(d["ld_dw"])
            sp.update(ld_dw=ldd, dw_off={"N": 0, "3N": N, "N+4": 4}[d["ld_dw"]])
            out("dw", rows * ldd, _ar(rows)[:, None] * ldd + sp["dw_off"] + _ar(N)[None, :])
            out("dm", rows * N)
        return b
    if e == "relu_mask":
        n = d["n"]
        sp.update(n=n)
        inp("y", torch.relu(rn(n)))
        inp("d", rn(n))
        out("d", n, alias="d")
        return b
    if e in ("ola_fwd", "ola_bwd"):
        (L, hop), Tp, R = d["Lh"], d["Tp"], d["R"]
        Tout = ola_tout(d)
        sp.update(R=R, Tp=Tp, L=L, hop=hop, Tout=Tout, bias=d.get("bias", 0))
        if e == "ola_fwd":
            inp("frames", rn(R * Tp, L))
            if d["bias"]:
                inp("bias", torch.tensor([0.375]))
            out("est", R * Tout)
        else:
            inp("dest", rn(R, Tout))
            out("dframes", R * Tp * L)
        return b
    if e == "sum_partial":
        n = d["n"]
        sp.update(n=n, nslab=d["nslab"])
        x = rn(n)
        inp("x", _spiked(x) if n > CAP else x)
        b.extras += ["slab", "tot"]
        return b
    if e in ("bn_stats", "bn_bwd", "bn_prelu_fwd"):
        C, M = d["C"], d["M"]
        sp.update(M=M, C=C)
        x = rn(M, C) * 0.01 + 5.0 if d.get("data") == "offset" else rn(M, C)
        inp("x", x)
        if e == "bn_stats":
            sp.update(nsplit=_ns(d, "nsplit", M), run=d["run"])
            if d["run"]:
                inp("running_mean", rn(C))
                inp("running_var", rn(C).abs() + 0.5)
                out("running_mean", C, alias="running_mean")
                b.alias["running_var"] = "running_var"
                b.outs.append("running_var")
            out("stats", 2 * C)
            return b
        xd = x.double()
        mean = xd.mean(0)
        inp("stats", torch.stack([mean, 1 / torch.sqrt(((xd - mean) ** 2).mean(0) + BN_EPS)]))
        inp("gamma", rn(C) + 1.0)
        if e == "bn_prelu_fwd":
            sp.update(res=d["res"])
            inp("beta", rn(C))
            inp("a", torch.tensor([d["slope"]]))
            if d["res"]:
                inp("res", rn(M, C))
            out("u", M * C)
            out("y", M * C)
            return b
        sp.update(nsplit=_ns(d, "nsplit", M))
        inp("du", rn(M, C))
        out("dx", M * C, alias="du" if d["alias"] else None)
        b.extras += ["slab", "sums"]
        return b
    if e in ("maxpool3_fwd", "maxpool3_bwd"):
        R, T, C = d["R"], d["T"], d["C"]
        sp.update(R=R, T=T, C=C)
        inp("x", torch.randint(-1, 2, (R, T, C), generator=g).float() * 0.5)          # three levels: windows with two and three equal maxima
        if e == "maxpool3_fwd":
            out("y", R * (T // 3) * C)
        else:
            inp("dy", rn(R, T // 3, C))
            out("dx", R * T * C)
        return b
    if e == "bcast_rows":
        M, C = d["M"], d["C"]
        rpr = _rpr(d, M)
        sp.update(M=M, C=C, rpr=rpr, scale=d["scale"])
        inp("src", rn(-(-M // rpr), C))
        out("out", M * C)
        return b
    if e == "cross_entropy":
        R, S = d["R"], d["S"]
        z = {"gauss": rn(R, S) * 3, "+80": rn(R, S) * 3 + 80.0, "-80": rn(R, S) * 3 - 80.0, "equal": torch.full((R, S), 1.25)}[d["data"]]
        lb = {"0": [0] * R, "S-1": [S - 1] * R, "rand": torch.randint(0, S, (R,), generator=g).tolist()}[d["label"]]
        sp.update(R=R, S=S, label=lb)
        inp("logits", z)
        out("loss", 1)
        out("dlogits", R * S)
        return b
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------
def run(mod, b, tensors, device="cpu", entry=None, plain=False):
    """The case's call on `mod` (wesep_amd.dev) over `tensors` (the allocations on the device); returns the extras."""
    e, sp, v = entry or b.case.entry, b.spec, b.views(tensors)
    if e == "prelu_fwd":
        mod.prelu_fwd(v["x"], v.get("rb"), v["a"], sp["rows"], sp["C"], sp["rpr"], v["y"])
    elif e == "prelu_bwd":
        da, slab = mod.prelu_bwd(v["pre"], v["dy"], v["a"], v["dx"], nslab=sp["nslab"], with_slab=True)
        return {"slab": slab, "da": da}
    elif e == "dwconv_fwd":
        a = (v["x"], v["stats"], v["gamma"], v["beta"], v["w"], v["b"], sp["R"], sp["Tp"], sp["C"], sp["P"], sp["dil"], sp["st_div"])
        if plain:
            mod._call("ws_dwconv_fwd", *[mod._p(x) if torch.is_tensor(x) else x for x in a], mod._p(v["y"]))
        else:
            mod.dwconv_fwd(*a, v["y"], causal=sp["causal"])
    elif e == "dwconv_bwd":
        a = (v["dy"], v["x"], v["stats"], v["gamma"], v["beta"], v["w"], sp["R"], sp["Tp"], sp["C"], sp["P"], sp["dil"], sp["st_div"])
        if plain:
            slab = torch.empty(sp["nsplit"], sp["P"] + 1, sp["C"], device=device, dtype=F32)
            mod._call("ws_dwconv_bwd", *[mod._p(x) if torch.is_tensor(x) else x for x in a], mod._p(v["dxn"]), sp["nsplit"], sp["rps"], mod._p(slab))
            return {"slab": slab}
        dw, db, slab = mod.dwconv_bwd(*a, v["dxn"], causal=sp["causal"], splits=(sp["nsplit"], sp["rps"]), with_slab=True)
        return {"slab": slab, "dw": dw, "db": db}
    elif e == "chan_sums":
        sums, slab = mod.chan_sums(v["g"], v.get("x"), v.get("stats"), sp["st_div"], sp["rpg"], sp["ng"], sp["C"], nsplit=sp["nsplit"], with_slab=True)
        return {"slab": slab, "sums": sums}
    elif e == "norm_ab":
        mod.norm_ab(v["sums"], v["gamma"], sp["ng"], sp["C"], sp["npg"], v["ab"])
    elif e == "norm_bwd_apply":
        mod.norm_bwd_apply_cl(v["x"], v["dxn"], v["stats"], v["ab"], v["gamma"], v.get("res"), sp["rows"], sp["C"], sp["st_div"], v["dx"])
    elif e == "maskmul_fwd":
        mod.maskmul_fwd(v["w"], sp["w_off"], sp["ldw"], v["m"], sp["rows"], sp["N"], v["s"])
    elif e == "maskmul_bwd":
        mod.maskmul_bwd(v["ds"], v["w"], sp["w_off"], sp["ldw"], v["m"], sp["rows"], sp["N"], v["dw"], sp["dw_off"], sp["ld_dw"], v["dm"])
    elif e == "relu_mask":
        mod.relu_mask(v["d"], v["y"])
    elif e == "ola_fwd":
        mod.ola_fwd(v["frames"], v.get("bias"), sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"], v["est"])
    elif e == "ola_bwd":
        mod.ola_bwd(v["dest"], sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"], v["dframes"])
    elif e == "sum_partial":
        tot, slab = mod.total_sum(v["x"], nslab=sp["nslab"], with_slab=True)
        return {"slab": slab, "tot": tot}
    elif e == "bn_stats":
        mod.bn_stats(v["x"], sp["M"], sp["C"], v.get("running_mean"), v.get("running_var"), v["stats"], nsplit=sp["nsplit"])
    elif e == "bn_prelu_fwd":
        mod.bn_prelu_fwd(v["x"], v["stats"], v["gamma"], v["beta"], v.get("res"), v["a"], sp["M"], sp["C"], v["u"], v["y"])
    elif e == "bn_bwd":
        sums, slab = mod.bn_bwd(v["x"], v["du"], v["stats"], v["gamma"], sp["M"], sp["C"], v["dx"], nsplit=sp["nsplit"], with_slab=True)
        return {"slab": slab, "sums": sums}
    elif e == "maxpool3_fwd":
        mod.maxpool3_fwd(v["x"], sp["R"], sp["T"], sp["C"], v["y"])
    elif e == "maxpool3_bwd":
        mod.maxpool3_bwd(v["x"], v["dy"], sp["R"], sp["T"], sp["C"], v["dx"])
    elif e == "bcast_rows":
        mod.bcast_rows(v["src"], sp["scale"], sp["rpr"], sp["M"], sp["C"], v["out"])
    elif e == "cross_entropy":
        mod.cross_entropy(v["logits"].reshape(sp["R"], sp["S"]), torch.tensor(sp["label"], dtype=torch.int64, device=device), v["loss"], v["dlogits"])
    else:
        raise ValueError(e)
    return {}


def refusals(dev, t, device="cpu"):
    """(name, call): one argument set per WS_REQUIRE clause; every call has to come back WS_ERR_INVALID without launching."""
    lb = torch.zeros(4, dtype=torch.int64, device=device)
    dw = lambda **k: dict(dict(R=2, Tp=4, C=8, P=3, dil=1, st=4), **k)          # noqa: E731
    dwf = lambda **k: (lambda a: dev.dwconv_fwd(t, t, t, t, t, t, a["R"], a["Tp"], a["C"], a["P"], a["dil"], a["st"], t))(dw(**k))          # noqa: E731
    dwb = lambda sp_, **k: (lambda a: dev.dwconv_bwd(t, t, t, t, t, t, a["R"], a["Tp"], a["C"], a["P"], a["dil"], a["st"], t, splits=sp_))(dw(**k))          # noqa: E731
    return [
        ("prelu_fwd C % 4", lambda: dev.prelu_fwd(t, None, t, 4, 6, 1, t)),
        ("prelu_fwd rows_per_r = 0 with rb", lambda: dev.prelu_fwd(t, t, t, 4, 8, 0, t)),
        ("prelu_bwd n % 4", lambda: dev.prelu_bwd(t[:6], t, t, t, nslab=1)),
        ("prelu_bwd nslab = 0", lambda: dev.prelu_bwd(t[:8], t, t, t, nslab=0)),
        ("dwconv_fwd C % 4", lambda: dwf(C=6)),
        ("dwconv_fwd even P", lambda: dwf(P=4)),
        ("dwconv_fwd P = 9", lambda: dwf(P=9)),
        ("dwconv_fwd dil = 0", lambda: dwf(dil=0)),
        ("dwconv_fwd st_div = 0", lambda: dwf(st=0)),
        ("dwconv_fwd Tp = 0", lambda: dwf(Tp=0)),
        ("dwconv_bwd P = 9", lambda: dwb((8, 1), P=9)),
        ("dwconv_bwd splits do not cover the rows", lambda: dwb((3, 2))),
        ("dwconv_bwd nsplit = 0", lambda: dwb((0, 8))),
        ("dwconv_bwd rows_per_split = 0", lambda: dwb((8, 0))),
        ("chan_sums C % 4", lambda: dev.chan_sums(t, None, None, 1, 4, 2, 6, nsplit=1)),
        ("chan_sums stats without x", lambda: dev.chan_sums(t, None, t, 1, 4, 2, 8, nsplit=1)),
        ("chan_sums st_div = 0 with stats", lambda: dev.chan_sums(t, t, t, 0, 4, 2, 8, nsplit=1)),
        ("chan_sums nsplit = 0", lambda: dev.chan_sums(t, None, None, 1, 4, 2, 8, nsplit=0)),
        ("norm_ab n_per_group = 0", lambda: dev.norm_ab(t, t, 2, 8, 0, t)),
        ("norm_ab C = 0", lambda: dev.norm_ab(t, t, 2, 0, 8, t)),
        ("norm_bwd_apply_cl C % 4", lambda: dev.norm_bwd_apply_cl(t, t, t, t, t, None, 4, 6, 1, t)),
        ("norm_bwd_apply_cl st_div = 0", lambda: dev.norm_bwd_apply_cl(t, t, t, t, t, None, 4, 8, 0, t)),
        ("maskmul_fwd N % 4", lambda: dev.maskmul_fwd(t, 0, 8, t, 4, 6, t)),
        ("maskmul_fwd ldw % 4", lambda: dev.maskmul_fwd(t, 0, 10, t, 4, 8, t)),
        ("maskmul_bwd ld_dw % 4", lambda: dev.maskmul_bwd(t, t, 0, 8, t, 4, 8, t, 0, 10, t)),
        ("maskmul_bwd ldw % 4", lambda: dev.maskmul_bwd(t, t, 0, 10, t, 4, 8, t, 0, 8, t)),
        ("relu_mask n % 4", lambda: dev.relu_mask(t[:6], t)),
        ("ola_fwd Tout > (Tp - 1) * hop + L", lambda: dev.ola_fwd(t, None, 2, 4, 6, 3, 16, t)),
        ("ola_fwd Tout = 0", lambda: dev.ola_fwd(t, None, 2, 4, 6, 3, 0, t)),
        ("ola_fwd hop = 0", lambda: dev.ola_fwd(t, None, 2, 4, 6, 0, 6, t)),
        ("ola_bwd L = 0", lambda: dev.ola_bwd(t, 2, 4, 0, 3, 8, t)),
        ("ola_bwd Tout = 0", lambda: dev.ola_bwd(t, 2, 4, 6, 3, 0, t)),
        ("total_sum nslab = 0", lambda: dev.total_sum(t[:8], nslab=0)),
        ("bn_stats C % 4", lambda: dev.bn_stats(t, 4, 6, None, None, t, nsplit=1)),
        ("bn_stats running_mean without running_var", lambda: dev.bn_stats(t, 4, 8, t, None, t, nsplit=1)),
        ("bn_stats nsplit = 0", lambda: dev.bn_stats(t, 4, 8, None, None, t, nsplit=0)),
        ("bn_prelu_fwd C % 4", lambda: dev.bn_prelu_fwd(t, t, t, t, None, t, 4, 6, t, t)),
        ("bn_prelu_fwd M = 0", lambda: dev.bn_prelu_fwd(t, t, t, t, None, t, 0, 8, t, t)),
        ("bn_bwd C % 4", lambda: dev.bn_bwd(t, t, t, t, 4, 6, t, nsplit=1)),
        ("bn_bwd nsplit = 0", lambda: dev.bn_bwd(t, t, t, t, 4, 8, t, nsplit=0)),
        ("maxpool3_fwd T < 3", lambda: dev.maxpool3_fwd(t, 2, 2, 8, t)),
        ("maxpool3_fwd C % 4", lambda: dev.maxpool3_fwd(t, 2, 6, 6, t)),
        ("maxpool3_bwd T < 3", lambda: dev.maxpool3_bwd(t, t, 2, 2, 8, t)),
        ("maxpool3_bwd C % 4", lambda: dev.maxpool3_bwd(t, t, 2, 6, 6, t)),
        ("bcast_rows rows_per_r = 0", lambda: dev.bcast_rows(t, 1.0, 0, 4, 8, t)),
        ("bcast_rows C % 4", lambda: dev.bcast_rows(t, 1.0, 2, 4, 6, t)),
        ("cross_entropy S = 0", lambda: dev.cross_entropy(t[:0].reshape(4, 0), lb, t, t)),
    ]


# ------------------------------------------------------------------------------------------------------------
# checker, emulation
# ------------------------------------------------------------------------------------------------------------
def _extra_before(x):
    return torch.full((x.numel(),), NAN)


def verify(b, ref, after, extra=None, what=None):
    """Every output of a built case against `ref`: `after` = name -> whole CPU allocation after the launch, `extra` = what
    run() returned, on the CPU.  Returns the worst err / bound.  Raises ContractViolation: nan | exact | bound | sentinel."""
    what = what or f"{b.case.entry} {b.case.name}"
    worst = 0.0
    for key, r in ref.items():
        if key in b.extras:
            o = extra[key].reshape(-1).float()
            fn = check_partial if isinstance(r, Partial) else check
            worst = max(worst, fn(o, _extra_before(o), r, f"{what} {key}", 0))
            continue
        name = b.alias.get(key, key)
        worst = max(worst, check(after[name], b.bufs[name], r, f"{what} {key}", b.start[name]))
    return worst


def output_bits(b, after, extra=None):
    """The bits of every output: the write sets of the operands written in place, the other allocations whole, the extras."""
    parts = []
    for n in dict.fromkeys(b.outs):
        t = after[n]
        if n in b.alias.values():
            t = t[b.start[n]:b.start[n] + b.size[n]]
        parts.append(t.contiguous().view(torch.int32).reshape(-1))
    for n in b.extras:
        parts.append(extra[n].contiguous().reshape(-1).view(torch.int32))
    return torch.cat(parts)


def _place(b, ref, vals):
    """(after, extra) with `vals` (name -> values in the order of the reference's idx) written."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    extra = {}
    for key, r in ref.items():
        if key in b.extras:
            extra[key] = vals[key].reshape(-1).float()
            continue
        name = b.alias.get(key, key)
        after[name][r.idx + b.start[name]] = vals[key].reshape(-1).float()
    return after, extra


def perfect(b, ref):
    """What a correctly rounding kernel leaves: the fp32 rounding of the float64 values (rstd: the interval's midpoint)."""
    vals = compute(b.case.entry, b.spec, b.views(b.bufs), F64)
    vals = {k: (ref[k].val if k == "stats" and b.case.entry == "bn_stats" else v) for k, v in vals.items()}
    return _place(b, ref, vals)


def emulate(b, ref, order="seq", defect=None):
    """What a correct fp32 kernel (sums in `order`) leaves -- or one with the planted `defect`."""
    return _place(b, ref, compute(b.case.entry, b.spec, b.views(b.bufs), F32, order, defect))


DEFECTS = {
    "prelu_fwd": ["rb_by_m"],
    "prelu_bwd": ["last_quad_skipped"],
    "dwconv_fwd": ["boundary_tap_dropped", "causal_centre", "stats_by_m"],
    "dwconv_bwd": ["boundary_tap_dropped", "causal_centre", "stats_by_m", "split_last_row_skipped"],
    "chan_sums": ["last_quad_skipped", "split_last_row_skipped", "stats_by_m"],
    "norm_ab": ["one_pass_of_256"],
    "norm_bwd_apply": ["stats_by_m"],
    "maskmul_fwd": ["ldw_ignored"],
    "maskmul_bwd": ["ldw_ignored", "mask_ge"],
    "relu_mask": ["mask_ge"],
    "ola_fwd": ["t_lo_off_by_one"],
    "ola_bwd": ["no_tout_test"],
    "sum_partial": ["tail_dropped"],
    "bn_stats": ["biased_running_var", "lane_twice"],
    "bn_prelu_fwd": ["res_after_prelu"],
    "bn_bwd": ["lane_twice", "split_last_row_skipped"],
    "maxpool3_fwd": ["window_of_two"],
    "maxpool3_bwd": ["tie_to_last"],
    "bcast_rows": ["row_mod"],
    "cross_entropy": ["label_plus_one", "no_max"],
}
