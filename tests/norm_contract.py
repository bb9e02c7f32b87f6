"""TEST INFRASTRUCTURE ONLY -- contract suite of the normalisation kernels: wesep_amd/csrc/norm.hip (ws_group_stats,
ws_group_stats_len, ws_gn_bwd_reduce, ws_gn_bwd_apply, ws_gn_param_grad, ws_gn_bwd_apply_pg, ws_gn_bwd_fused2, ws_rowln_fwd,
ws_rowln_bwd) and the two chunked-statistics pairs (ws_flat_stats of tasnet.hip, ws_flat_stats_len of ragged_grid.hip).  Same
shape as tests/gemm_contract.py, tests/blk_contract.py and tests/conv3x3_contract.py: Ref, check, eps_for, the guards and the
pairwise generator with its registries are imported from gemm_contract.  No GPU code here: the CPU test
(test_norm_contract_host_cpu.py) checks this module, the GPU test (test_norm_contract_gpu.py) runs every case through
wesep_amd.dev.

1. REFERENCE (float64, explicit gathers; F.group_norm / F.layer_norm are the host test's independent second opinion).
   Group g of a ws_groups_geom covers rows l < L and columns c < W_g at base(g) + l * rs + c,
     base(g) = (g / gdiv) * gs1 + (g % gdiv) * gs2 + band_off[g % nbands],  W_g = band_w ? band_w[g % nbands] : W
   (group_index).  stats[g] = (mean, 1 / sqrt(biased var + eps)) over that set; with glen over its first glen[g / glen_div] rows;
   flat_stats_len over the first glen[g] * per_step floats.  The backward entries TAKE stats (and ab): the builder uploads
   the fp32 rounding of the float64 values and the reference computes xhat = (x - mean) * rstd from exactly those fp32
   numbers, so every entry is judged on its own.
     ab[g]  = (mean_g(dxn gamma), mean_g(dxn gamma xhat))
     dx     = rstd (dxn gamma - ab0 - xhat ab1) (+ res)
     dgamma[band][c] = sum dxn xhat,  dbeta[band][c] = sum dxn   over the rows of the groups of the band
     rowln  y = gamma (x - mean) rstd + beta;  dx = rstd (gamma dy - mean(gamma dy) - xhat mean(gamma dy xhat)) (+ res);
            d(beta)[c] = sum_rows dy, d(gamma)[c] = sum_rows dy xhat
   Outputs whose split assignment the header does not fix (the ws_gn_param_grad slabs, pslab, the rowln_bwd slab) are
   judged as sums: every element of the write set is written (NaN before, finite after), the float64 sum over the splits /
   workgroups meets the reference sum, slabs of splits that own no group and the columns [band_w[b], W) are exact zeros.
   pout (and the [2, W] sum dev.rowln_bwd returns) is also held against the float64 sum of the rows the kernel left,
   eps_for(False, rows).  The ceil(nwg / 32)
   extra rows of pslab are scratch (may be written); the counter words are zero afterwards.

2. BOUNDS.  Derived, no tuned constant; eps_for(False, n) = (n + 8) * 2^-24 is gemm_contract's fp32 any-order bound.
     sums, means   eps_for(False, n) * S, S = the same expression over absolute values (|dxn| |gamma| |x - mean| |rstd| ...),
                   n = the number of addends (the leaves: a tree over partial sums adds no new ones)
     dx, y         eps_for(False, 0) * S + 2^-24 |res|,  S = |rstd| (|dxn gamma| + |a0| + |xhat a1|); where the kernel takes
                   the two means itself (gn_bwd_fused, rowln_bwd) plus their propagated bound |rstd| (b_a0 + |xhat| b_a1)
     rstd          an INTERVAL.  d_m = eps_for(False, n) * mean|x| bounds the mean.  The two-pass sum satisfies
                   sum (x - m')^2 = sum (x - m)^2 + n (m - m')^2, so the variance is off by at most
                   d_v = eps_for(False, n) * (var + d_m^2) + d_m^2, and the kernel's rstd must lie in
                   [1 / sqrt(var + d_v + eps), 1 / sqrt(max(var - d_v, 0) + eps)], widened by 4 * 2^-24 relative for the add,
                   sqrtf and the division.  Ref carries it as val = the midpoint, bound = the half width, S = the exact rstd.
     rowln_fwd y   |gamma| (d_m rstd_hi + |x - mean| d_r) + eps_for(False, 0) (|gamma (x - mean)| rstd + |beta|),
                   d_r = the larger distance of rstd from the ends of its interval.
   CONDITION OF THE SUITE: these bounds see a dropped element only while it weighs enough in its group, so no case with
   gauss / row-x1e3 data has a group above 2048 elements (CAP) and offset data (x = 1000 + N(0, 1)) stays at n <= 1024; the
   cases that exist to cross a loop seam with a larger group carry a `spike` (one structurally chosen element x1e3: the
   group's last element, the first element of the last row, the last column of the first row, the first row behind glen).

3. CASES.  cases(entry): gemm_contract's pairwise generator over *_DIMS, topped up per kernel instantiation, plus the few
   hand-written seam cases of EXTRA (255 / 256 / 257 / 513 quads per group for the 256-thread loops; M = 2048 * RPB + 1 for
   the grid-stride loop of every rowln instantiation).  `targets` mirrors geom_vec4, ws_gn_param_grad's dispatch and rowln_lpr.

BUFFERS.  GUARD floats on both sides of every operand and output.  Outputs: the write set starts as NaN (dx aliasing dxn /
dy: as that operand), everything else holds SENT and must be bit-identical afterwards.  Inputs: everything the contract
does not read is NaN -- gaps between bands, row tails up to rs, rows of other groups, rows behind glen, gamma beyond the
band's width, guards; build(case, garbage=True) puts a large finite value there instead.  Vectorised cases keep every
pointer 16-byte aligned; scalar cases also run with the operands starting one float into their allocation."""
import math

import numpy as np
import torch

from tests import gemm_contract as gc
from tests.gemm_contract import (GUARD, SENT, U, Buf, Built, Case, ContractViolation, Ref, check, eps_for)  # noqa: F401

GARBAGE = 3.0e30
NAN = float("nan")
GN_EPS = float(np.finfo(np.float32).eps)
LN_EPS = 1e-5
CAP = 2048
GROUP_ENTRIES = ("group_stats", "gn_bwd_reduce", "gn_bwd_apply", "gn_param_grad", "gn_bwd_apply_pg", "gn_bwd_fused")
ENTRIES = GROUP_ENTRIES + ("rowln_fwd", "rowln_bwd", "flat_stats", "flat_stats_len")
COMPOSED = "norm_composed"
BAND_W = [2, 6, 10, 32, 128]
F64 = torch.float64


# ------------------------------------------------------------------------------------------------------------
# geometry
# ------------------------------------------------------------------------------------------------------------
def make_geom(kind, W, L, ng):
    """The ws_groups_geom fields (+ span: the floats of the tensor) of a geometry kind."""
    g = dict(L=L, nbands=1, band_w=None, band_off=None, kind=kind)
    if kind in ("time", "mask", "cln"):
        g.update(ngroups=ng, gdiv=1, gs1=L * W, gs2=0, rs=W, W=W, nbands=3 if kind == "mask" else 1, span=ng * L * W)
    elif kind == "odd-stride":
        rs = W + 1
        g.update(ngroups=ng, gdiv=1, gs1=L * rs + 2, gs2=0, rs=rs, W=W, span=ng * (L * rs + 2))
    elif kind == "band":            # x [R][K = L][Tf][N = W]; group = (r, frame)
        Tf = 3
        g.update(ngroups=ng, gdiv=Tf, gs1=L * Tf * W, gs2=W, rs=Tf * W, W=W, span=-(-ng // Tf) * L * Tf * W)
    elif kind == "bandsplit":       # x [R][Tf = L][rs]; group = (r, band); gaps between the bands, a tail behind the last
        off, p = [], 0
        for w, gap in zip(BAND_W, (3, 1, 2, 5, 3)):
            p += gap
            off.append(p)
            p += w
        rs = p + 7
        g.update(ngroups=ng * 5, gdiv=5, gs1=L * rs, gs2=0, rs=rs, W=128, nbands=5, band_w=list(BAND_W), band_off=off,
                 span=ng * L * rs)
    elif kind == "bandsplit2":      # gdiv = 2 != nbands = 4: blocks of L rows hold bands (0, 1), (2, 3), (0, 1), ...
        g.update(ngroups=ng * 4, gdiv=2, gs1=L * 190, gs2=5, rs=190, W=128, nbands=4, band_w=[6, 10, 32, 128],
                 band_off=[3, 20, 1, 50], span=ng * 2 * L * 190)
    else:
        raise ValueError(kind)
    return g


def geom_vec4(geo):
    return (geo["band_w"] is None and geo["band_off"] is None
            and all(v % 4 == 0 for v in (geo["W"], geo["rs"], geo["gs1"], geo["gs2"])))


def group_index(geo, g, rows=None, defect=None):
    """(idx [rows, W_g], band, W_g): the header's formula."""
    band = g % geo["nbands"]
    Wg = geo["band_w"][band] if geo["band_w"] else geo["W"]
    ob = g % geo["gdiv"] if defect == "off_gdiv" else band
    base = (g // geo["gdiv"]) * geo["gs1"] + (g % geo["gdiv"]) * geo["gs2"] + (geo["band_off"][ob] if geo["band_off"] else 0)
    rows = geo["L"] if rows is None else rows
    return base + torch.arange(rows).unsqueeze(1) * geo["rs"] + torch.arange(Wg).unsqueeze(0), band, Wg


def rowln_lpr(W):
    return 64 if W > 128 else 32 if W > 64 else 16 if W > 32 else 8


def rowln_grid(M, W):
    rpb = 256 // rowln_lpr(W)
    return min(-(-M // rpb), 2048)


# ------------------------------------------------------------------------------------------------------------
# bounds
# ------------------------------------------------------------------------------------------------------------
def stats_interval(v, eps):
    """v [G, n] float64 -> (mean, rstd, d_m, lo, hi, mean|x|) per row: the module docstring's interval."""
    n = v.shape[1]
    m = v.mean(1)
    var = ((v - m.unsqueeze(1)) ** 2).mean(1)
    ma = v.abs().mean(1)
    e = eps_for(False, n)
    d_m = e * ma
    d_v = e * (var + d_m ** 2) + d_m ** 2
    lo = (1 - 4 * U) / torch.sqrt(var + d_v + eps)
    hi = (1 + 4 * U) / torch.sqrt((var - d_v).clamp_min(0) + eps)
    return m, 1 / torch.sqrt(var + eps), d_m, lo, hi, ma


def _stats_ref(m, rstd, d_m, lo, hi, ma, first=0):
    G = m.numel()
    idx = 2 * (first + torch.arange(G)).unsqueeze(1) + torch.arange(2).unsqueeze(0)
    val = torch.stack([m, (lo + hi) / 2], 1)
    bound = torch.stack([d_m, (hi - lo) / 2], 1)
    S = torch.stack([ma, rstd], 1)
    return Ref(idx.reshape(-1), val.reshape(-1), S.reshape(-1), bound.reshape(-1), torch.zeros(2 * G, dtype=torch.bool))


def _ref(idx, val, S, bound):
    idx = idx.reshape(-1)
    return Ref(idx, val.reshape(-1), S.reshape(-1), bound.reshape(-1), torch.zeros(idx.numel(), dtype=torch.bool))


def _cat(refs):
    return Ref(*[torch.cat([r[i] for r in refs]) for i in range(5)])


class Partial:
    """A partial-sum output: `rows` [nrows, ncols] = the write set (flat indices), summed over the rows against (val, bound);
    zero = mask [nrows, ncols] of exact zeros; scratch = indices that may be written."""
    def __init__(self, rows, val, S, bound, zero=None, scratch=None):
        self.rows, self.val, self.S, self.bound = rows, val, S, bound
        self.zero = torch.zeros(rows.shape, dtype=torch.bool) if zero is None else zero
        self.scratch = torch.zeros(0, dtype=torch.long) if scratch is None else scratch


# ------------------------------------------------------------------------------------------------------------
# references.  `sp` = the case's spec (build), `t` = name -> float32 tensor the call receives (allocation minus base)
# ------------------------------------------------------------------------------------------------------------
def _defective_stats(v, eps, defect, n_other):
    n = v.numel()
    if defect == "one_pass":
        f = v.float()
        m = f.sum() / n
        var = ((f * f).sum() / n - m * m).clamp_min(0)
        return m.double(), 1 / torch.sqrt(var.double() + eps)
    if defect == "drop_last_quad" and n > 4:
        v = v[:-4]
    if defect == "n_geoW":
        m = v.sum() / n_other
        return m, 1 / torch.sqrt(((v - m) ** 2).sum() / n_other + eps)
    m = v.mean()
    var = ((v - m) ** 2).mean()
    if defect == "unbiased" and n > 1:
        var = var * n / (n - 1)
    return m, 1 / torch.sqrt(var + eps)


def _glen_rows(sp, g, defect=None):
    geo = sp["geo"]
    if sp.get("glen") is None or defect == "glen_ignored":
        return geo["L"]
    gl = sp["glen"]
    gi = g if defect == "glen_g" else g // sp["glen_div"]
    return min(max(int(gl[min(gi, len(gl) - 1)]), 1), geo["L"])


def ref_group_stats(sp, t, defect=None):
    geo, x = sp["geo"], t["x"]
    refs = []
    for g in range(geo["ngroups"]):
        rows = _glen_rows(sp, g, defect)
        idx, _, Wg = group_index(geo, g, rows, defect)
        v = x[idx.reshape(-1)].double()
        r = _stats_ref(*stats_interval(v.unsqueeze(0), sp["eps"]), first=g)
        if defect:
            m, rs = _defective_stats(v, sp["eps"], defect, rows * geo["W"])
            r = r._replace(val=torch.stack([m, rs]).double())
        refs.append(r)
    return {"stats": _cat(refs)}


def _gamma(sp, t, band, Wg, defect=None):
    if sp["gamma"] == "tab":
        o = sp["gamma_off"][0 if defect == "gamma_tab0" else band]
        return t["gamma"][o:o + Wg].double()
    return t["gamma"][:Wg].double()


def _group_terms(sp, t, g, defect=None):
    """(idx, xhat, |x - mean| |rstd|, dxn (+ dxn2), gamma or None, rstd) of group g from the UPLOADED fp32 statistics."""
    geo = sp["geo"]
    idx, band, Wg = group_index(geo, g, None, defect)
    mean, rstd = t["stats"][2 * g].double(), t["stats"][2 * g + 1].double()
    x = t["x"][idx].double()
    d = t["dxn"][idx].double()
    if "dxn2" in t:
        d = d + t["dxn2"][idx].double()
    return idx, (x - mean) * rstd, (x - mean).abs() * rstd.abs(), d, _gamma(sp, t, band, Wg, defect) if "gamma" in t else None, rstd


def _dabs(sp, t, idx):
    d = t["dxn"][idx].double().abs()
    return d + t["dxn2"][idx].double().abs() if "dxn2" in t else d


def ref_gn_bwd_reduce(sp, t, defect=None):
    geo = sp["geo"]
    val, S, bd = [], [], []
    for g in range(geo["ngroups"]):
        idx, xh, axh, d, gm, _ = _group_terms(sp, t, g, defect)
        n = idx.numel() if defect != "n_geoW" else geo["L"] * geo["W"]
        dg, adg = d * gm, _dabs(sp, t, idx) * gm.abs()
        val += [dg.sum() / n, (dg * xh).sum() / n]
        S += [adg.sum() / idx.numel(), (adg * axh).sum() / idx.numel()]
        bd += [eps_for(False, idx.numel()) * s for s in S[-2:]]
    return {"ab": _ref(torch.arange(2 * geo["ngroups"]), torch.stack(val), torch.stack(S), torch.stack(bd))}


def _dx_ref(sp, t, own_means, defect=None):
    """dx of every group; own_means: the kernel takes ab itself from the given stats (fused) instead of reading t['ab']."""
    geo = sp["geo"]
    I, V, SS, B = [], [], [], []
    for g in range(geo["ngroups"]):
        idx, xh, axh, d, gm, rstd = _group_terms(sp, t, g, defect)
        dg, adg = d * gm, _dabs(sp, t, idx) * gm.abs()
        extra = 0.0
        if own_means:
            n = idx.numel()
            a0, a1 = dg.mean(), (dg * xh).mean()
            extra = rstd.abs() * eps_for(False, n) * (adg.mean() + xh.abs() * (adg * axh).mean())
        else:
            a0, a1 = t["ab"][2 * g].double(), t["ab"][2 * g + 1].double()
            if defect == "ab_swapped":
                a0, a1 = a1, a0
        v = rstd * (dg - a0 - xh * a1)
        S = rstd.abs() * (adg + a0.abs() + (xh * a1).abs())
        bound = eps_for(False, 0) * S + extra
        if "res" in t:
            r = t["res"][idx].double()
            bound = bound + U * r.abs()
            if defect != "res_skipped":
                v = v + r
        I.append(idx.reshape(-1)), V.append(v.reshape(-1)), SS.append(S.reshape(-1)), B.append(bound.reshape(-1))
    return _ref(torch.cat(I), torch.cat(V), torch.cat(SS), torch.cat(B))


def ref_gn_bwd_apply(sp, t, defect=None):
    return {"dx": _dx_ref(sp, t, False, defect)}


def _param_sums(sp, t, defect=None):
    """(val, S) [nbands, 2, W]: row 0 dgamma, row 1 dbeta; n addends per element = groups of the band * L."""
    geo = sp["geo"]
    nb, W = geo["nbands"], geo["W"]
    val, S = torch.zeros(nb, 2, W, dtype=F64), torch.zeros(nb, 2, W, dtype=F64)
    for g in range(geo["ngroups"]):
        idx, xh, axh, d, _, _ = _group_terms(sp, t, g, defect)
        ad = _dabs(sp, t, idx)
        if defect == "odd_rows_dropped":
            xh, axh, d, ad = xh[0::2], axh[0::2], d[0::2], ad[0::2]
        b, Wg = g % nb, idx.shape[1]
        val[b, 0, :Wg] += (d * xh).sum(0)
        val[b, 1, :Wg] += d.sum(0)
        S[b, 0, :Wg] += (ad * axh).sum(0)
        S[b, 1, :Wg] += ad.sum(0)
    return val, S


def ref_gn_param_grad(sp, t, defect=None):
    geo, ns = sp["geo"], sp["nsplit"]
    nb, W = geo["nbands"], geo["W"]
    val, S = _param_sums(sp, t, defect)
    per_band = geo["ngroups"] // nb
    rows = torch.arange(ns * nb * 2 * W).reshape(ns, nb * 2 * W)
    zero = torch.zeros(ns, nb, 2, W, dtype=torch.bool)
    zero[per_band:] = True
    if geo["band_w"]:
        for b in range(nb):
            zero[:, b, :, geo["band_w"][b]:] = True
    return {"slab": Partial(rows, val.reshape(-1), S.reshape(-1), eps_for(False, per_band * geo["L"]) * S.reshape(-1),
                            zero.reshape(ns, -1))}


def _pslab(sp, t, nrows, with_pout, defect=None):
    geo = sp["geo"]
    val, S = _param_sums(sp, t, defect)
    bound = eps_for(False, geo["ngroups"] * geo["L"]) * S.reshape(-1)
    extra = -(-nrows // 32) if with_pout else 0
    out = {"pslab": Partial(torch.arange(nrows * 256).reshape(nrows, 256), val.reshape(-1), S.reshape(-1), bound,
                            scratch=nrows * 256 + torch.arange(extra * 256))}
    if with_pout:
        out["pout"] = _ref(torch.arange(256), val.reshape(-1), S.reshape(-1), bound)
    return out


def ref_gn_bwd_apply_pg(sp, t, defect=None):
    return dict(dx=_dx_ref(sp, t, False, defect), **_pslab(sp, t, sp["geo"]["ngroups"], True, defect))


def ref_gn_bwd_fused(sp, t, defect=None):
    return dict(dx=_dx_ref(sp, t, True, defect), **_pslab(sp, t, sp["nwg"], sp["pout"], defect))


def ref_rowln_fwd(sp, t, defect=None):
    M, W = sp["M"], sp["W"]
    x = t["x"][:M * W].reshape(M, W).double()
    g, b = t["gamma"][:W].double(), t["beta"][:W].double()
    m, rstd, d_m, lo, hi, ma = stats_interval(x, sp["eps"])
    xm = x - m.unsqueeze(1)
    y = g * xm * rstd.unsqueeze(1) + b
    d_r = torch.maximum(hi - rstd, rstd - lo).unsqueeze(1)
    bound = g.abs() * (d_m.unsqueeze(1) * hi.unsqueeze(1) + xm.abs() * d_r) + eps_for(False, 0) * ((g * xm).abs() * rstd.unsqueeze(1) + b.abs())
    return {"y": _ref(torch.arange(M * W), y, (g * xm).abs() * rstd.unsqueeze(1) + b.abs(), bound),
            "stats": _stats_ref(m, rstd, d_m, lo, hi, ma)}


def ref_rowln_bwd(sp, t, defect=None):
    M, W = sp["M"], sp["W"]
    x, dy = t["x"][:M * W].reshape(M, W).double(), t["dy"][:M * W].reshape(M, W).double()
    g = t["gamma"][:W].double()
    st = t["stats"][:2 * M].reshape(M, 2).double()
    mean, rstd = st[:, :1], st[:, 1:]
    xh, axh = (x - mean) * rstd, (x - mean).abs() * rstd.abs()
    gd = g * dy
    s1, s2 = gd.mean(1, keepdim=True), (gd * xh).mean(1, keepdim=True)
    v = rstd * (gd - s1 - xh * s2)
    S = rstd.abs() * (gd.abs() + s1.abs() + (xh * s2).abs())
    e = eps_for(False, W)
    bound = eps_for(False, 0) * S + rstd.abs() * e * (gd.abs().mean(1, keepdim=True) + xh.abs() * (gd.abs() * axh).mean(1, keepdim=True))
    if "res" in t:
        r = t["res"][:M * W].reshape(M, W).double()
        v, bound = v + r, bound + U * r.abs()
    tv = torch.stack([dy.sum(0), (dy * xh).sum(0)])
    tS = torch.stack([dy.abs().sum(0), (dy.abs() * axh).sum(0)])
    grid = rowln_grid(M, W)
    return {"dx": _ref(torch.arange(M * W), v, S, bound),
            "slab": Partial(torch.arange(grid * 2 * W).reshape(grid, 2 * W), tv.reshape(-1), tS.reshape(-1), eps_for(False, M) * tS.reshape(-1)),
            "tot": _ref(torch.arange(2 * W), tv, tS, eps_for(False, M) * tS)}


def flat_counts(sp):
    """floats of every group that the statistics cover"""
    if sp.get("glen") is None:
        return [sp["n"]] * sp["ng"]
    return [min(max(int(v), 1), sp["n"] // sp["per_step"]) * sp["per_step"] for v in sp["glen"]]


def ref_flat_stats(sp, t, defect=None):
    refs = []
    for g, cnt in enumerate(flat_counts(sp)):
        v = t["x"][g * sp["n"]: g * sp["n"] + cnt].double()
        r = _stats_ref(*stats_interval(v.unsqueeze(0), sp["eps"]), first=g)
        n4, nch = cnt // 4, sp["nchunk"]
        per = -(-n4 // nch)
        if defect == "stale_empty_chunk" and per * (nch - 1) >= n4:
            # an empty chunk merged as if it held `per` quads of its (zero) mean and no spread
            k = 4 * per
            m2 = ((v - v.mean()) ** 2).sum() + v.mean() ** 2 * cnt * k / (cnt + k)
            r = r._replace(val=torch.stack([v.mean() * cnt / (cnt + k), 1 / torch.sqrt(m2 / (cnt + k) + sp["eps"])]))
        refs.append(r)
    return {"stats": _cat(refs)}


REFS = {"group_stats": ref_group_stats, "gn_bwd_reduce": ref_gn_bwd_reduce, "gn_bwd_apply": ref_gn_bwd_apply,
        "gn_param_grad": ref_gn_param_grad, "gn_bwd_apply_pg": ref_gn_bwd_apply_pg, "gn_bwd_fused": ref_gn_bwd_fused,
        "rowln_fwd": ref_rowln_fwd, "rowln_bwd": ref_rowln_bwd, "flat_stats": ref_flat_stats, "flat_stats_len": ref_flat_stats}


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, targets
# ------------------------------------------------------------------------------------------------------------
SPIKES = ["spike-last", "spike-lastrow0", "spike-row0last", "spike-behind"]
DATA = ["gauss", "row-x1e3", "offset"] + SPIKES
DATA_NOLEN = DATA[:-1]
GEOMS = ["time", "band", "bandsplit", "bandsplit2", "mask", "cln", "odd-stride"]
WIDTHS = [4, 12, 128, 132, 384, 1, 3, 37, 771, "tab"]
LS = [1, 2, 7, 8, 9, 33]
NGS = [1, 3, 4, 6]
_GEO = {"geom": GEOMS, "W": WIDTHS, "L": LS, "ng": NGS}

GS_DIMS = dict(_GEO, glen=["off", "full", "ones", "mixed"], glen_div=["1", "K"], align=[0, 1], data=DATA)
RD_DIMS = dict(_GEO, gamma=["vec", "tab"], align=[0, 1], data=DATA_NOLEN)
AP_DIMS = dict(_GEO, gamma=["vec", "tab"], res=["off", "sep"], alias=[0, 1], align=[0, 1], data=DATA_NOLEN)
PG_DIMS = dict(geom=GEOMS, W=[4, 12, 128, 1, 3, 37, "tab"], L=LS, ng=[1, 3, 6], nsplit=["1", "2", "3", "over"], align=[0, 1],
               data=DATA_NOLEN)
APG_DIMS = dict(geom=["time", "band"], ng=[1, 2, 31, 32, 33, 65], L=[1, 7, 8, 9, 17], res=["off", "sep"], alias=[0, 1],
                data=DATA_NOLEN)
FU_DIMS = dict(geom=["time", "band"], L=[2, 4, 30, 32], ng=[1, 3, 4, 5, 9], nwg=["1", "2", "ceil", "over", "33", "65"],
               dxn2=[0, 1], pout=[0, 1], res=["off", "sep"], data=DATA_NOLEN)
RL_W = [4, 28, 32, 36, 64, 68, 128, 132, 200, 256]
RL_M = ["1", "RPB-1", "RPB", "RPB+1"]
RL_DATA = ["gauss", "row-x1e3", "offset", "spike-last", "spike-lastrow0"]
RF_DIMS = dict(W=RL_W, M=RL_M, data=RL_DATA)
RB_DIMS = dict(W=RL_W, M=RL_M, res=["off", "sep"], alias=[0, 1], data=RL_DATA)
FS_N = [4, 1020, 1024, 1028, 4100]
FS_CH = ["1", "2", "3", "64", "65", "over"]
FS_DIMS = dict(n=FS_N, nchunk=FS_CH, ng=[1, 3], data=["gauss", "offset", "spike-last"])
FL_DIMS = dict(n=FS_N, nchunk=FS_CH, per_step=[4, 128], glen=["1", "max", "mixed"], ng=[1, 3],
               data=["gauss", "offset", "spike-last", "spike-behind"])


def _wmax(W):
    return 128 if W == "tab" else W


def _is_spike(data):
    return data in SPIKES


def _vec_kind(geom, W):
    return geom in ("time", "band", "mask", "cln") and W != "tab" and W % 4 == 0


_GEO_RULES = [
    ("a band_w table carries its own widths", ("geom", "W"), lambda g, W: (g in ("bandsplit", "bandsplit2")) != (W == "tab")),
    ("cln is L = 1", ("geom", "L"), lambda g, L: g == "cln" and L != 1),
    ("odd-stride is W % 4 == 0 with rs % 4 != 0", ("geom", "W"), lambda g, W: g == "odd-stride" and (W == "tab" or W % 4 != 0)),
    ("suite condition: a group above 2048 elements carries a spike", ("W", "L", "data"),
     lambda W, L, data: _wmax(W) * L > CAP and not _is_spike(data)),
    ("offset data stays at n <= 1024", ("W", "L", "data"), lambda W, L, data: data == "offset" and _wmax(W) * L > 1024),
]
_ALIGN_RULE = ("a start one float into the allocation needs the scalar path", ("align", "geom", "W"),
               lambda a, g, W: a == 1 and _vec_kind(g, W))
GS_RULES = _GEO_RULES + [
    _ALIGN_RULE,
    ("glen_div = K needs a glen table", ("glen", "glen_div"), lambda gl, dv: gl == "off" and dv == "K"),
    ("spike-behind needs a row behind glen", ("data", "glen"), lambda data, gl: data == "spike-behind" and gl in ("off", "full")),
    ("spike-behind needs a row behind glen", ("data", "L"), lambda data, L: data == "spike-behind" and L == 1),
]
RD_RULES = _GEO_RULES + [_ALIGN_RULE]
PG_RULES = _GEO_RULES + [
    _ALIGN_RULE,
    ("ws_gn_param_grad: ngroups % nbands == 0", ("geom", "ng"), lambda g, ng: g == "mask" and ng % 3 != 0),
]
_SIZE128 = [("suite condition: a group above 2048 elements carries a spike", ("L", "data"),
             lambda L, data: 128 * L > CAP and not _is_spike(data)),
            ("offset data stays at n <= 1024", ("L", "data"), lambda L, data: data == "offset" and 128 * L > 1024)]
FS_RULES = [("suite condition: a group above 2048 elements carries a spike", ("n", "data"),
             lambda n, data: n > CAP and not _is_spike(data)),
            ("offset data stays at n <= 1024", ("n", "data"), lambda n, data: data == "offset" and n > 1024)]
FL_RULES = FS_RULES + [
    ("per_step divides n_per_group", ("n", "per_step"), lambda n, ps: n % ps != 0),
    ("spike-behind needs floats behind the count", ("data", "glen"), lambda data, gl: data == "spike-behind" and gl == "max"),
    ("spike-behind needs floats behind the count", ("data", "n", "per_step"), lambda data, n, ps: data == "spike-behind" and n == ps),
]


def _v(b):
    return "true" if b else "false"


def _geo_of(d):
    W = d.get("W", 128)
    return make_geom(d["geom"], 128 if W == "tab" else W, d["L"], d["ng"])


def _targets(entry, d, seed=0):
    if entry in ("group_stats", "gn_bwd_reduce", "gn_bwd_apply"):
        v4 = geom_vec4(_geo_of(d)) and not d.get("align", 0)
        k = f"{entry}_kernel<{_v(v4)}>"
        if entry == "group_stats":
            return (k,) + ((k + "[glen]",) if d["glen"] != "off" else ())
        t = (k, f"{entry}[{'gamma_tab' if d['gamma'] == 'tab' else 'gamma'}]")
        if entry == "gn_bwd_apply":
            t += (f"gn_bwd_apply[res {d['res']}]",) + (("gn_bwd_apply[dx aliases dxn]",) if d["alias"] else ())
        return t
    if entry == "gn_param_grad":
        geo = _geo_of(d)
        return ("gn_param_grad128_kernel" if geo["nbands"] == 1 and geo["W"] == 128 and geom_vec4(geo) and not d["align"]
                else "gn_param_grad_kernel",)
    if entry == "gn_bwd_apply_pg":
        return ("gn_bwd_apply_pg_kernel", f"gn_bwd_apply_pg[res {d['res']}]")
    if entry == "gn_bwd_fused":
        return ("gn_bwd_fused_kernel", f"gn_bwd_fused[dxn2 {'on' if d['dxn2'] else 'off'}]",
                f"gn_bwd_fused[pout {'on' if d['pout'] else 'off'}]", f"gn_bwd_fused[res {d['res']}]")
    if entry in ("rowln_fwd", "rowln_bwd"):
        t = (f"{entry}_kernel<{rowln_lpr(d['W'])}>",)
        if entry == "rowln_bwd":
            t += (f"rowln_bwd[res {d['res']}]",) + (("rowln_bwd[dx aliases dy]",) if d["alias"] else ())
        return t
    nch = flat_nchunk(d)
    return (f"{entry}_chunk_kernel", f"{entry}_final_kernel[{'serial' if nch > 64 else 'butterfly'}]")


def flat_nchunk(d):
    return d["n"] // 4 + 1 if d["nchunk"] == "over" else int(d["nchunk"])


def _kv(name):
    return [f"{name}_kernel<true>", f"{name}_kernel<false>"]


INST = {
    "group_stats": _kv("group_stats") + [k + "[glen]" for k in _kv("group_stats")],
    "gn_bwd_reduce": _kv("gn_bwd_reduce") + ["gn_bwd_reduce[gamma]", "gn_bwd_reduce[gamma_tab]"],
    "gn_bwd_apply": _kv("gn_bwd_apply") + ["gn_bwd_apply[gamma]", "gn_bwd_apply[gamma_tab]", "gn_bwd_apply[res off]",
                                           "gn_bwd_apply[res sep]", "gn_bwd_apply[dx aliases dxn]"],
    "gn_param_grad": ["gn_param_grad128_kernel", "gn_param_grad_kernel"],
    "gn_bwd_apply_pg": ["gn_bwd_apply_pg_kernel", "gn_bwd_apply_pg[res off]", "gn_bwd_apply_pg[res sep]"],
    "gn_bwd_fused": ["gn_bwd_fused_kernel"] + [f"gn_bwd_fused[{k} {v}]" for k, vs in (("dxn2", ("off", "on")), ("pout", ("off", "on")),
                                                                                     ("res", ("off", "sep"))) for v in vs],
    "rowln_fwd": [f"rowln_fwd_kernel<{l}>" for l in (8, 16, 32, 64)],
    "rowln_bwd": [f"rowln_bwd_kernel<{l}>" for l in (8, 16, 32, 64)] + ["rowln_bwd[res off]", "rowln_bwd[res sep]",
                                                                        "rowln_bwd[dx aliases dy]"],
    "flat_stats": ["flat_stats_chunk_kernel", "flat_stats_final_kernel[butterfly]", "flat_stats_final_kernel[serial]"],
    "flat_stats_len": ["flat_stats_len_chunk_kernel", "flat_stats_len_final_kernel[butterfly]", "flat_stats_len_final_kernel[serial]"],
}
_M = gc.MIN_PER_TARGET
_VEC, _SCL = {"geom": "time", "W": 128}, {"geom": "bandsplit", "W": "tab"}
TOPUP = {
    "group_stats": [(dict(_VEC, glen="off", align=0), INST["group_stats"][0], _M), (dict(_SCL, glen="off"), INST["group_stats"][1], _M),
                    (dict(_VEC, glen="mixed", align=0), INST["group_stats"][2], _M), (dict(_SCL, glen="mixed"), INST["group_stats"][3], _M)],
    "gn_bwd_reduce": [(dict(_VEC, align=0), INST["gn_bwd_reduce"][0], _M), (_SCL, INST["gn_bwd_reduce"][1], _M),
                      ({"gamma": "vec"}, INST["gn_bwd_reduce"][2], _M), ({"gamma": "tab"}, INST["gn_bwd_reduce"][3], _M)],
    "gn_bwd_apply": [(dict(_VEC, align=0), INST["gn_bwd_apply"][0], _M), (_SCL, INST["gn_bwd_apply"][1], _M),
                     ({"gamma": "vec"}, INST["gn_bwd_apply"][2], _M), ({"gamma": "tab"}, INST["gn_bwd_apply"][3], _M),
                     ({"res": "off"}, INST["gn_bwd_apply"][4], _M), ({"res": "sep"}, INST["gn_bwd_apply"][5], _M),
                     ({"alias": 1}, INST["gn_bwd_apply"][6], _M)],
    "gn_param_grad": [({"geom": "time", "W": 128, "align": 0}, "gn_param_grad128_kernel", _M),
                      ({"geom": "band", "W": 128, "align": 0}, "gn_param_grad128_kernel", _M), (_SCL, "gn_param_grad_kernel", _M)],
    "gn_bwd_apply_pg": [({}, "gn_bwd_apply_pg_kernel", _M)] + [({"res": r}, f"gn_bwd_apply_pg[res {r}]", _M) for r in ("off", "sep")],
    "gn_bwd_fused": [({}, "gn_bwd_fused_kernel", _M)] + [({k: v}, f"gn_bwd_fused[{k} {n}]", _M) for k, v, n in (
        ("dxn2", 0, "off"), ("dxn2", 1, "on"), ("pout", 0, "off"), ("pout", 1, "on"), ("res", "off", "off"), ("res", "sep", "sep"))],
    "rowln_fwd": [({"W": w}, f"rowln_fwd_kernel<{rowln_lpr(w)}>", _M) for w in (28, 36, 68, 200)],
    "rowln_bwd": [({"W": w}, f"rowln_bwd_kernel<{rowln_lpr(w)}>", _M) for w in (28, 36, 68, 200)] + [
        ({"res": "off"}, "rowln_bwd[res off]", _M), ({"res": "sep"}, "rowln_bwd[res sep]", _M), ({"alias": 1}, "rowln_bwd[dx aliases dy]", _M)],
    "flat_stats": [({"nchunk": "2"}, INST["flat_stats"][1], _M), ({"nchunk": "65"}, INST["flat_stats"][2], _M)],
    "flat_stats_len": [({"nchunk": "2"}, INST["flat_stats_len"][1], _M), ({"nchunk": "65"}, INST["flat_stats_len"][2], _M)],
}
DIMS = {"group_stats": GS_DIMS, "gn_bwd_reduce": RD_DIMS, "gn_bwd_apply": AP_DIMS, "gn_param_grad": PG_DIMS,
        "gn_bwd_apply_pg": APG_DIMS, "gn_bwd_fused": FU_DIMS, "rowln_fwd": RF_DIMS, "rowln_bwd": RB_DIMS, "flat_stats": FS_DIMS,
        "flat_stats_len": FL_DIMS}
RULES = {"group_stats": GS_RULES, "gn_bwd_reduce": RD_RULES, "gn_bwd_apply": RD_RULES, "gn_param_grad": PG_RULES,
         "gn_bwd_apply_pg": _SIZE128, "gn_bwd_fused": _SIZE128, "rowln_fwd": [], "rowln_bwd": [], "flat_stats": FS_RULES,
         "flat_stats_len": FL_RULES}
gc.DIMS.update(DIMS)
gc.RULES.update(RULES)
gc.SEEDS.update({e: 31 + i for i, e in enumerate(ENTRIES)})
gc.INST.update(INST)
gc.TOPUP.update(TOPUP)
for _e in ENTRIES:
    gc.PLANNERS[_e] = (lambda e: lambda d, seed: _targets(e, d, seed))(_e)

# hand-written seam cases (values outside the lists): quads per group around the 256-thread stride, and the grid-stride
# loop of every rowln instantiation (M = 2048 * RPB + 1, at most 8 MB, the spike on the last row)
_QUADS = [dict(geom="time", W=4, L=L, ng=2, data="spike-last" if 4 * L > CAP else "gauss") for L in (255, 256, 257, 513)]
EXTRA = {
    "group_stats": [dict(q, glen="off", glen_div="1", align=0) for q in _QUADS],
    "gn_bwd_reduce": [dict(q, gamma="vec", align=0) for q in _QUADS],
    "gn_bwd_apply": [dict(q, gamma="vec", res="sep", alias=0, align=0) for q in _QUADS],
    "rowln_fwd": [dict(W=w, M="grid+1", data="spike-last") for w in (28, 36, 68, 200)],
    "rowln_bwd": [dict(W=w, M="grid+1", res="off", alias=0, data="spike-last") for w in (28, 36, 68, 200)],
}
_COMPOSED = [("time-W128-L8", dict(geom="time", W=128, L=8, ng=3, gamma="vec")),
             ("band-W128-L8", dict(geom="band", W=128, L=8, ng=6, gamma="vec")),
             ("bandsplit", dict(geom="bandsplit", W="tab", L=7, ng=3, gamma="tab")),
             ("bandsplit-gdiv2", dict(geom="bandsplit2", W="tab", L=7, ng=3, gamma="tab")),
             ("mask-W12", dict(geom="mask", W=12, L=9, ng=6, gamma="tab"))]


def cases(entry):
    if entry == COMPOSED:
        return [Case(COMPOSED, n, dict(d, res="sep", alias=0, align=0, data="gauss"), ("composed",), 9000 + i)
                for i, (n, d) in enumerate(_COMPOSED)]
    out = list(gc.cases(entry))
    for i, d in enumerate(EXTRA.get(entry, [])):
        out.append(Case(entry, f"x{i:02d}-" + "-".join(str(v) for v in d.values()), d, _targets(entry, d), 8000 + i))
    return out


def invalid_pairs(entry):
    return gc.invalid_pairs(entry)


# ------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------
class NBuilt(Built):
    """bufs: name -> whole allocation; start: name -> where the tensor the call receives begins; spec: geometry, tables and
    scalars of the call; alias: output name -> the operand it is written over (wset: that write set inside the allocation)."""
    def __init__(self, case):
        super().__init__(case)
        self.start, self.spec, self.alias = {}, {}, {}

    def views(self, tensors):
        """name -> the tensor the call receives (also under the alias names: dx -> dxn)."""
        t = {k: v[self.start[k]:] for k, v in tensors.items()}
        for a, k in self.alias.items():
            t[a] = t[k]
        return t


def _spike(v):
    return math.copysign(max(abs(float(v)), 0.5), float(v)) * 1e3


def _group_data(g, L, Wg, kind, rows):
    x, d = torch.randn(L, Wg, generator=g), torch.randn(L, Wg, generator=g)
    if kind == "row-x1e3":
        x[L // 2] *= 1e3
        d[L // 2] *= 1e3
    pos = {"spike-last": (L - 1, Wg - 1), "spike-lastrow0": (L - 1, 0), "spike-row0last": (0, Wg - 1)}.get(kind)
    if kind == "spike-behind" and rows < L:
        pos = (rows, 0)
    if pos:
        x[pos], d[pos] = _spike(x[pos]), _spike(d[pos])
    if kind == "offset":
        x += 1000.0
    return x, d


def _glen_table(kind, L, n, seed):
    if kind == "full":
        return [L] * n
    if kind == "ones":
        return [1] * n
    gl = [1 + (3 * i + seed) % L for i in range(n)]
    if L > 1 and all(v == L for v in gl):
        gl[0] = L - 1
    return gl


def _out(b, name, n, widx, st):
    """An output allocation of n floats (+ 1 when it starts one float in): SENT, NaN on the write set."""
    t = gc.alloc(n + 1, SENT)
    t[st + widx] = NAN
    b.bufs[name], b.start[name] = t, st
    b.outs.append(name)
    return t


def _small_out(b, name, n):
    return _out(b, name, n, torch.arange(n), GUARD)


def _build_group(case, garbage):
    e, d, g = case.entry, case.dims, gc.gen(case.seed)
    if e == COMPOSED:
        e = "gn_bwd_apply"
    fill = GARBAGE if garbage else NAN
    if e in ("gn_bwd_apply_pg", "gn_bwd_fused"):
        d = dict(d, W=128, align=0, gamma="vec")
    geo = _geo_of(d)
    assert not (d["align"] and geom_vec4(geo)), "a vectorised case must keep its pointers 16-byte aligned"
    b = NBuilt(case)
    sp = b.spec
    sp.update(geo=geo, eps=GN_EPS, gamma=d.get("gamma", "vec"))
    st = GUARD + d["align"]
    ng, L, span = geo["ngroups"], geo["L"], geo["span"]
    if e == "group_stats" and d["glen"] != "off":
        sp["glen_div"] = geo["nbands"] if d["glen_div"] == "K" and geo["nbands"] > 1 else 3 if d["glen_div"] == "K" else 1
        sp["glen"] = _glen_table(d["glen"], L, -(-ng // sp["glen_div"]), case.seed)
    X, D = gc.alloc(span + 1, fill), gc.alloc(span + 1, fill)
    widx = []
    for gi in range(ng):
        idx, band, Wg = group_index(geo, gi)
        rows = _glen_rows(sp, gi)
        xv, dv = _group_data(g, L, Wg, d["data"], rows)
        if rows < L and d["data"] != "spike-behind":
            xv[rows:] = fill            # rows behind glen: not read, not counted
        X[st + idx], D[st + idx] = xv, dv
        widx.append(idx.reshape(-1))
    widx = torch.cat(widx)
    b.bufs["x"], b.start["x"] = X, st
    if e == "group_stats":
        _small_out(b, "stats", 2 * ng)
        return b
    b.bufs["dxn"], b.start["dxn"] = D, st
    # statistics as the forward leaves them: the fp32 rounding of the float64 values
    sref = ref_group_stats(sp, {"x": X[st:]})["stats"]
    S = gc.alloc(2 * ng, fill)
    S[GUARD:GUARD + 2 * ng] = sref.S.reshape(ng, 2).float().reshape(-1)     # S of the rstd slot = the exact rstd
    S[GUARD:GUARD + 2 * ng:2] = sref.val[0::2].float()
    b.bufs["stats"], b.start["stats"] = S, GUARD
    # gamma: per column, or one 16-byte aligned piece per band between unread gaps
    nb = geo["nbands"]
    if e != "gn_param_grad":
        if sp["gamma"] == "tab":
            ws = [geo["band_w"][k] if geo["band_w"] else geo["W"] for k in range(nb)]
            sp["gamma_off"], p = [], 0
            for w in ws:
                sp["gamma_off"].append(p)
                p += (w + 7) // 4 * 4
            Gm = gc.alloc(p + 1, fill)
            for o, w in zip(sp["gamma_off"], ws):
                Gm[st + o: st + o + w] = 1 + 0.5 * torch.randn(w, generator=g)
        else:
            Gm = gc.alloc(geo["W"] + 1, fill)
            Gm[st: st + geo["W"]] = 1 + 0.5 * torch.randn(geo["W"], generator=g)
        b.bufs["gamma"], b.start["gamma"] = Gm, st
    if e == "gn_bwd_fused" and d["dxn2"]:
        D2 = gc.alloc(span + 1, fill)
        D2[st + widx] = torch.randn(widx.numel(), generator=g)
        b.bufs["dxn2"], b.start["dxn2"] = D2, st
    if e == "gn_bwd_reduce":
        _small_out(b, "ab", 2 * ng)
        return b
    if e == "gn_param_grad":
        per_band = ng // nb
        sp["nsplit"] = per_band + 2 if d["nsplit"] == "over" else int(d["nsplit"])
        _small_out(b, "slab", sp["nsplit"] * nb * 2 * geo["W"])
        return b
    if e == "gn_bwd_apply" or e == "gn_bwd_apply_pg":
        ab = ref_gn_bwd_reduce(sp, b.views(b.bufs))["ab"].val.float()
        A = gc.alloc(2 * ng, fill)
        A[GUARD:GUARD + 2 * ng] = ab
        b.bufs["ab"], b.start["ab"] = A, GUARD
    if d["res"] == "sep":
        Rb = gc.alloc(span + 1, fill)
        Rb[st + widx] = torch.randn(widx.numel(), generator=g)
        b.bufs["res"], b.start["res"] = Rb, st
    if d.get("alias"):
        b.alias["dx"] = "dxn"
        b.outs.append("dxn")
        b.wset = st + widx
    else:
        _out(b, "dx", span, widx, st)
    if e == "gn_bwd_apply":
        return b
    if e == "gn_bwd_apply_pg":
        nrows, sp["pout"] = ng, 1
    else:
        sp["nwg"] = nrows = {"1": 1, "2": 2, "ceil": -(-ng // 4), "over": ng // 4 + 2, "33": 33, "65": 65}[d["nwg"]]
        sp["pout"] = d["pout"]
    extra = -(-nrows // 32) if sp["pout"] else 0
    _out(b, "pslab", (nrows + extra) * 256 + 64, torch.arange(nrows * 256), GUARD)
    if sp["pout"]:
        _small_out(b, "pout", 256)
    sp["counter"] = 1 + extra
    return b


def rowln_M(d):
    rpb = 256 // rowln_lpr(d["W"])
    return {"1": 1, "RPB-1": max(rpb - 1, 1), "RPB": rpb, "RPB+1": rpb + 1, "grid+1": 2048 * rpb + 1}[d["M"]]


def _rows_data(g, M, W, kind):
    x, d = torch.randn(M, W, generator=g), torch.randn(M, W, generator=g)
    if kind == "row-x1e3":
        x[M // 2] *= 1e3
        d[M // 2] *= 1e3
    pos = {"spike-last": (M - 1, W - 1), "spike-lastrow0": (M - 1, 0)}.get(kind)
    if pos:
        x[pos], d[pos] = _spike(x[pos]), _spike(d[pos])
    if kind == "offset":
        x += 1000.0
    return x.reshape(-1), d.reshape(-1)


def _input(b, name, data, fill):
    t = gc.alloc(data.numel(), fill)
    t[GUARD:GUARD + data.numel()] = data
    b.bufs[name], b.start[name] = t, GUARD


def _build_rowln(case, garbage):
    e, d, g = case.entry, case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    M, W = rowln_M(d), d["W"]
    b = NBuilt(case)
    b.spec.update(M=M, W=W, eps=LN_EPS)
    xv, dv = _rows_data(g, M, W, d["data"])
    _input(b, "x", xv, fill)
    _input(b, "gamma", 1 + 0.5 * torch.randn(W, generator=g), fill)
    if e == "rowln_fwd":
        _input(b, "beta", torch.randn(W, generator=g), fill)
        _small_out(b, "y", M * W)
        _small_out(b, "stats", 2 * M)
        return b
    _input(b, "dy", dv, fill)
    fw = ref_rowln_fwd(b.spec, dict(b.views(b.bufs), beta=torch.zeros(W)))["stats"]
    st = fw.S.reshape(M, 2).clone()
    st[:, 0] = fw.val.reshape(M, 2)[:, 0]
    _input(b, "stats", st.float().reshape(-1), fill)
    if d["res"] == "sep":
        _input(b, "res", torch.randn(M * W, generator=g), fill)
    if d["alias"]:
        b.alias["dx"] = "dy"
        b.outs.append("dy")
        b.wset = GUARD + torch.arange(M * W)
    else:
        _small_out(b, "dx", M * W)
    _small_out(b, "slab", rowln_grid(M, W) * 2 * W)
    b.bufs["tot"], b.start["tot"] = torch.full((2 * W,), NAN), 0       # returned by the wrapper: no guards of its own
    b.outs.append("tot")
    return b


def _build_flat(case, garbage):
    e, d, g = case.entry, case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    n, ng = d["n"], d["ng"]
    b = NBuilt(case)
    sp = b.spec
    sp.update(n=n, ng=ng, nchunk=flat_nchunk(d), eps=LN_EPS)
    if e == "flat_stats_len":
        ps = sp["per_step"] = d["per_step"]
        mx = n // ps
        sp["glen"] = {"1": [1] * ng, "max": [mx] * ng, "mixed": [1 + (5 * i + case.seed) % mx for i in range(ng)]}[d["glen"]]
        if d["glen"] == "mixed" and mx > 1 and all(v == mx for v in sp["glen"]):
            sp["glen"][0] = mx - 1
    x = torch.full((ng, n), fill)
    for gi, cnt in enumerate(flat_counts(sp)):
        v = torch.randn(n, generator=g)
        if d["data"] == "offset":
            v += 1000.0
        if d["data"] == "spike-last":
            v[cnt - 1] = _spike(v[cnt - 1])
        if d["data"] == "spike-behind":
            if cnt < n:
                v[cnt] = _spike(v[cnt])
            x[gi] = v                   # finite data behind the count: counting it changes the result, reading it must not
        else:
            x[gi, :cnt] = v[:cnt]
    _input(b, "x", x.reshape(-1), fill)
    _small_out(b, "stats", 2 * ng)
    return b


def build(case, garbage=False):
    if case.entry in GROUP_ENTRIES or case.entry == COMPOSED:
        return _build_group(case, garbage)
    if case.entry in ("rowln_fwd", "rowln_bwd"):
        return _build_rowln(case, garbage)
    return _build_flat(case, garbage)


def reference(b, tensors=None, defect=None, entry=None):
    e = entry or ("gn_bwd_apply" if b.case.entry == COMPOSED else b.case.entry)
    return REFS[e](b.spec, b.views(tensors or b.bufs), defect)


# ------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------
def dev_geom(mod, geo, device):
    def tab(v):
        return None if v is None else torch.tensor(v, dtype=torch.int32, device=device)
    return mod.Geom(geo["ngroups"], geo["gdiv"], geo["gs1"], geo["gs2"], geo["rs"], geo["L"], geo["W"], geo["nbands"],
                    tab(geo["band_w"]), tab(geo["band_off"]))


def _gamma_args(sp, v, device):
    if sp["gamma"] != "tab":
        return dict(gamma=v["gamma"])
    ptrs = torch.tensor([v["gamma"].data_ptr() + 4 * o for o in sp["gamma_off"]], dtype=torch.int64, device=device)
    return dict(gamma_tab=ptrs)


def run(mod, b, tensors, device, entry=None):
    """The case's call on `mod` (wesep_amd.dev) over `tensors` (the allocations on `device`).  Returns what the call leaves
    outside them: {'tot': ..., 'counter': ...}."""
    e, sp, v = entry or b.case.entry, b.spec, b.views(tensors)
    out = {}
    if e in GROUP_ENTRIES:
        geo = dev_geom(mod, sp["geo"], device)
    if e == "group_stats":
        gl = None if sp.get("glen") is None else torch.tensor(sp["glen"], dtype=torch.int32, device=device)
        mod.group_stats(v["x"], geo, v["stats"], sp["eps"], glen=gl, glen_div=sp.get("glen_div", 1))
    elif e == "gn_bwd_reduce":
        mod.gn_bwd_reduce(v["x"], v["dxn"], v["stats"], geo, v["ab"], **_gamma_args(sp, v, device))
    elif e == "gn_bwd_apply":
        mod.gn_bwd_apply(v["x"], v["dxn"], v["stats"], v["ab"], geo, v["dx"], res=v.get("res"), **_gamma_args(sp, v, device))
    elif e == "gn_param_grad":
        mod.gn_param_grad(v["x"], v["dxn"], v["stats"], geo, sp["nsplit"], v["slab"])
    elif e == "gn_bwd_apply_pg":
        out["counter"] = torch.zeros(sp["counter"], dtype=torch.int32, device=device)
        mod.gn_bwd_apply_pg(v["x"], v["dxn"], v["stats"], v["ab"], geo, v["dx"], v["gamma"], v["pslab"], v["pout"], out["counter"],
                            res=v.get("res"))
    elif e == "gn_bwd_fused":
        out["counter"] = torch.zeros(sp["counter"], dtype=torch.int32, device=device)
        mod.gn_bwd_fused(v["x"], v["dxn"], v["stats"], geo, v["gamma"], v["dx"], sp["nwg"], v["pslab"], res=v.get("res"),
                         pout=v.get("pout"), counter=out["counter"] if sp["pout"] else None, dxn2=v.get("dxn2"))
    elif e == "rowln_fwd":
        mod.rowln_fwd(v["x"], v["gamma"], v["beta"], sp["M"], sp["W"], v["y"], v["stats"], sp["eps"])
    elif e == "rowln_bwd":
        out["tot"] = mod.rowln_bwd(v["x"], v["dy"], v["stats"], v["gamma"], sp["M"], sp["W"], v["dx"], res=v.get("res"),
                                   slab=v["slab"])
    elif e == "flat_stats":
        mod.flat_stats(v["x"], sp["ng"], sp["n"], v["stats"], sp["eps"], nchunk=sp["nchunk"])
    else:
        gl = torch.tensor(sp["glen"], dtype=torch.int32, device=device)
        mod.flat_stats_len(v["x"], sp["ng"], sp["n"], gl, sp["per_step"], v["stats"], sp["eps"], nchunk=sp["nchunk"])
    return out


def refusals(dev, t, device):
    """(name, call): argument sets the header refuses; every call has to raise without launching."""
    G = dev.Geom
    i32 = torch.zeros(64, dtype=torch.int32, device=device)

    def fused(L, W):
        geo = G(4, 1, L * W, 0, W, L, W)
        return lambda: dev.gn_bwd_fused(t, t, t, geo, t, t, 1, t)
    g128 = G(4, 1, 8 * 128, 0, 128, 8, 128, 2)
    return [
        ("gn_bwd_fused odd L", fused(3, 128)), ("gn_bwd_fused L = 34", fused(34, 128)), ("gn_bwd_fused W = 64", fused(4, 64)),
        ("gn_bwd_apply_pg nbands = 2", lambda: dev.gn_bwd_apply_pg(t, t, t, t, g128, t, t, t, t, i32)),
        ("gn_param_grad W = 132", lambda: dev.gn_param_grad(t, t, t, G(4, 1, 8 * 132, 0, 132, 8, 132), 1, t)),
        ("gn_param_grad ngroups % nbands", lambda: dev.gn_param_grad(t, t, t, G(5, 1, 8 * 128, 0, 128, 8, 128, 2), 1, t)),
        ("rowln_fwd W = 260", lambda: dev.rowln_fwd(t, t, t, 4, 260, t, t)), ("rowln_fwd W = 6", lambda: dev.rowln_fwd(t, t, t, 4, 6, t, t)),
        ("rowln_bwd W = 260", lambda: dev.rowln_bwd(t, t, t, t, 4, 260, t)), ("rowln_bwd W = 6", lambda: dev.rowln_bwd(t, t, t, t, 4, 6, t)),
        ("flat_stats n % 4", lambda: dev.flat_stats(t, 2, 1022, t, nchunk=2)),
    ]


# ------------------------------------------------------------------------------------------------------------
# checker
# ------------------------------------------------------------------------------------------------------------
def check_partial(out, before, p: Partial, what, base):
    """A partial-sum output: written everywhere, exact zeros where the contract says zero, the float64 sum over the rows
    inside the bound, nothing outside the write set (and the scratch) changed.  Returns the worst err / bound."""
    o = out.detach().cpu().reshape(-1)
    got = o[p.rows + base]
    seen = Ref(torch.cat([p.rows.reshape(-1), p.scratch]), torch.cat([got.reshape(-1).double(), torch.zeros(p.scratch.numel(), dtype=F64)]),
               torch.zeros(p.rows.numel() + p.scratch.numel(), dtype=F64), torch.zeros(p.rows.numel() + p.scratch.numel(), dtype=F64),
               torch.cat([p.zero.reshape(-1), torch.zeros(p.scratch.numel(), dtype=torch.bool)]))
    seen.val[:p.rows.numel()][p.zero.reshape(-1)] = 0.0
    o2 = o.clone()
    o2[p.scratch + base] = 0.0      # scratch may hold anything, NaN included
    check(o2, before, seen, what, base)     # nan | exact | sentinel
    err = (got.double().sum(0) - p.val).abs()
    bad = err > p.bound
    if bad.any():
        j = int((err / p.bound.clamp_min(1e-300) * bad).argmax())
        raise ContractViolation("bound", f"{what}: {int(bad.sum())} sums outside the bound; worst at column {j}: got "
                                         f"{float(got.double().sum(0)[j])!r} ref {float(p.val[j])!r} err {float(err[j]):.3e} "
                                         f"bound {float(p.bound[j]):.3e}")
    pos = p.bound > 0
    return float((err[pos] / p.bound[pos]).max()) if pos.any() else 0.0


def verify(b, ref, after, extra=None, what=None):
    """Every output of a built case (`after`: name -> whole CPU allocation after the launch; `extra`: what run() returned,
    on the CPU) against `ref`.  Returns the worst err / bound.  Raises ContractViolation: nan | exact | bound | sentinel."""
    what = what or b.case.name
    worst = 0.0
    for key, r in ref.items():
        name = b.alias.get(key, key)
        if key == "tot":
            worst = max(worst, check(extra["tot"].reshape(-1), b.bufs["tot"], r, f"{what} tot", 0))
        elif isinstance(r, Partial):
            worst = max(worst, check_partial(after[name], b.bufs[name], r, f"{what} {key}", b.start[name]))
        else:
            worst = max(worst, check(after[name], b.bufs[name], r, f"{what} {key}", b.start[name]))
    if "pout" in ref and "pslab" in ref:     # pout against the rows the kernel left
        p = ref["pslab"]
        rows = after["pslab"][p.rows + b.start["pslab"]].double()
        left = _ref(torch.arange(256), rows.sum(0), rows.abs().sum(0), eps_for(False, rows.shape[0]) * rows.abs().sum(0))
        keep = torch.full_like(after["pout"], SENT)
        keep[b.start["pout"]: b.start["pout"] + 256] = after["pout"][b.start["pout"]: b.start["pout"] + 256]
        worst = max(worst, check(keep, keep, left, f"{what} pout against the pslab rows", b.start["pout"]))
    if "tot" in ref and "slab" in ref:       # the wrapper's sum against the slab rows the kernel left
        p = ref["slab"]
        rows = after["slab"][p.rows + b.start["slab"]].double()
        n = rows.shape[1]
        left = _ref(torch.arange(n), rows.sum(0), rows.abs().sum(0), eps_for(False, rows.shape[0]) * rows.abs().sum(0))
        worst = max(worst, check(extra["tot"].reshape(-1), extra["tot"].reshape(-1), left, f"{what} tot against the slab rows", 0))
    if extra is not None and "counter" in extra and bool((extra["counter"] != 0).any()):
        raise ContractViolation("exact", f"{what}: the counter words are {extra['counter'].tolist()}, the contract says 0")
    return worst


def output_bits(b, after, extra=None):
    """The bits of every output (the pslab scratch rows excepted)."""
    parts = []
    for n in b.outs:
        if n == "tot":
            parts.append(extra["tot"].contiguous().view(torch.int32).reshape(-1))
            continue
        t = after[n]
        if n in b.alias.values():       # an operand written in place: what surrounds the write set is input poison
            t = t[b.wset]
        if n == "pslab":
            t = t[:b.start[n] + (b.spec.get("nwg") or b.spec["geo"]["ngroups"]) * 256]
        parts.append(t.contiguous().view(torch.int32).reshape(-1))
    return torch.cat(parts)


def perfect(b, ref):
    """(after, extra) a correctly rounding kernel leaves for `ref`: a partial sum whole in row 0, zeros in the other rows."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    extra = {}
    for key, r in ref.items():
        name = b.alias.get(key, key)
        if key == "tot":
            extra["tot"] = r.val.float()
        elif isinstance(r, Partial):
            v = torch.zeros(r.rows.shape, dtype=torch.float32)
            v[0] = r.val.float()
            v[r.zero] = 0.0
            after[name][r.rows + b.start[name]] = v
        else:
            after[name][r.idx + b.start[name]] = r.val.float()
    if "counter" in b.spec:
        extra["counter"] = torch.zeros(b.spec["counter"], dtype=torch.int32)
    return after, extra


# ------------------------------------------------------------------------------------------------------------
# fp32 emulations (host test): every sum in one of three orders
# ------------------------------------------------------------------------------------------------------------
ORDERS = ("seq", "pairwise", "lanes256")


def sum32(v, order):
    """float32 sum over the last axis: sequential, pairwise, or 256 strided lanes (sequential inside a lane) + a tree."""
    v = v.float()
    if order == "seq":
        return torch.from_numpy(np.add.accumulate(v.numpy(), axis=-1, dtype=np.float32)[..., -1].copy())
    if order == "pairwise":
        while v.shape[-1] > 1:
            if v.shape[-1] % 2:
                v = torch.cat([v, torch.zeros(v.shape[:-1] + (1,))], -1)
            v = v[..., 0::2] + v[..., 1::2]
        return v[..., 0]
    pad = (-v.shape[-1]) % 256
    v = torch.cat([v, torch.zeros(v.shape[:-1] + (pad,))], -1)
    return sum32(sum32(v.reshape(v.shape[:-1] + (-1, 256)).transpose(-1, -2), "seq"), "pairwise")


def _stats32(v, eps, order):
    n = v.shape[-1]
    m = sum32(v, order) / n
    q = sum32((v.float() - m.unsqueeze(-1)) ** 2, order) / n
    return m, 1.0 / torch.sqrt(q + torch.tensor(eps, dtype=torch.float32))


def emulate(b, order):
    """(after, extra) of a correct fp32 kernel that sums in `order`."""
    e, sp = b.case.entry, b.spec
    after = {k: v.clone() for k, v in b.bufs.items()}
    t = b.views(after)
    src = b.views(b.bufs)
    extra = {}
    if "counter" in sp:
        extra["counter"] = torch.zeros(sp["counter"], dtype=torch.int32)
    if e in ("flat_stats", "flat_stats_len"):
        for g, cnt in enumerate(flat_counts(sp)):
            v = src["x"][g * sp["n"]: g * sp["n"] + cnt]
            n4 = cnt // 4
            per = -(-n4 // sp["nchunk"])
            N, mean, m2 = 0.0, 0.0, 0.0
            for c in range(sp["nchunk"]):
                lo, hi = 4 * c * per, min(cnt, 4 * (c + 1) * per)
                if hi <= lo:
                    continue
                m = sum32(v[lo:hi], order) / (hi - lo)
                q = float(sum32((v[lo:hi] - m) ** 2, order))
                nt, dl = N + (hi - lo), float(m) - mean
                mean, m2, N = mean + dl * (hi - lo) / nt, m2 + q + dl * dl * N * (hi - lo) / nt, nt
            t["stats"][2 * g] = mean
            t["stats"][2 * g + 1] = 1.0 / torch.sqrt(torch.tensor(m2 / N, dtype=torch.float32) + torch.tensor(sp["eps"], dtype=torch.float32))
        return after, extra
    if e in ("rowln_fwd", "rowln_bwd"):
        M, W = sp["M"], sp["W"]
        x, g = src["x"][:M * W].reshape(M, W), src["gamma"][:W]
        if e == "rowln_fwd":
            m, r = _stats32(x, sp["eps"], order)
            t["y"][:M * W] = ((x - m.unsqueeze(1)) * r.unsqueeze(1) * g + src["beta"][:W]).reshape(-1)
            t["stats"][:2 * M] = torch.stack([m, r], 1).reshape(-1)
            return after, extra
        dy, st = src["dy"][:M * W].reshape(M, W), src["stats"][:2 * M].reshape(M, 2)
        xh = (x - st[:, :1]) * st[:, 1:]
        gd = g * dy
        s1, s2 = sum32(gd, order) / W, sum32(gd * xh, order) / W
        o = (gd - s1.unsqueeze(1) - xh * s2.unsqueeze(1)) * st[:, 1:]
        if "res" in src:
            o = o + src["res"][:M * W].reshape(M, W)
        extra["tot"] = torch.stack([sum32(dy.t(), order), sum32((dy * xh).t(), order)]).reshape(-1)
        t["slab"][:rowln_grid(M, W) * 2 * W] = 0.0
        t["slab"][:2 * W] = extra["tot"]
        t["dx"][:M * W] = o.reshape(-1)
        return after, extra
    geo = sp["geo"]
    nb, W = geo["nbands"], geo["W"]
    psum = torch.zeros(nb, 2, W)
    for g in range(geo["ngroups"]):
        rows = _glen_rows(sp, g)
        idx, band, Wg = group_index(geo, g, rows)
        x = src["x"][idx]
        if e == "group_stats":
            m, r = _stats32(x.reshape(-1), sp["eps"], order)
            t["stats"][2 * g], t["stats"][2 * g + 1] = m, r
            continue
        mean, rstd = src["stats"][2 * g], src["stats"][2 * g + 1]
        d = src["dxn"][idx] + src["dxn2"][idx] if "dxn2" in src else src["dxn"][idx]
        xh = (x - mean) * rstd
        psum[band, 0, :Wg] += sum32((d * xh).t(), order)
        psum[band, 1, :Wg] += sum32(d.t(), order)
        if e == "gn_param_grad":
            continue
        gm = (src["gamma"][sp["gamma_off"][band]:][:Wg] if sp["gamma"] == "tab" else src["gamma"][:Wg])
        dg = d * gm
        n = idx.numel()
        if e == "gn_bwd_reduce" or e == "gn_bwd_fused":
            a0, a1 = sum32(dg.reshape(-1), order) / n, sum32((dg * xh).reshape(-1), order) / n
        if e == "gn_bwd_reduce":
            t["ab"][2 * g], t["ab"][2 * g + 1] = a0, a1
            continue
        if e != "gn_bwd_fused":
            a0, a1 = src["ab"][2 * g], src["ab"][2 * g + 1]
        o = (dg - a0 - xh * a1) * rstd
        if "res" in src:
            o = o + src["res"][idx]
        t["dx"][idx] = o
    if e == "gn_param_grad":
        t["slab"][:nb * 2 * W] = psum.reshape(-1)
        t["slab"][nb * 2 * W: sp["nsplit"] * nb * 2 * W] = 0.0
    if e in ("gn_bwd_apply_pg", "gn_bwd_fused"):
        nrows = sp.get("nwg") or geo["ngroups"]
        t["pslab"][:nrows * 256] = 0.0
        t["pslab"][:256] = psum.reshape(-1)
        if sp["pout"]:
            t["pout"][:256] = psum.reshape(-1)
    return after, extra
