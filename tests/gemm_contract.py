"""TEST INFRASTRUCTURE ONLY -- contract suite of the generic GEMM family (ws_gemm_nt, ws_gemm_tn, ws_conv_wgrad,
ws_reduce_slabs; include/wesep_hip.h).  No GPU code here: the CPU test (test_gemm_contract_host_cpu.py) checks this
module, the GPU test (test_gemm_contract_gpu.py) runs every case through the C ABI.

Three parts.

1. REFERENCE.  ref_gemm_nt / ref_gemm_tn / ref_conv_wgrad / ref_reduce_slabs take the keyword arguments of
   wesep_amd.dev.gemm_nt / gemm_tn / conv_wgrad / reduce_slabs on CPU tensors and restate the header comment in float64:
   row offset (m / div) * s1 + (m % div) * s2, stat index (m / st_div1) * st_m1 + (m % st_div2) * st_m2 + st_base,
   per-group overrides, the conv view of both modes as an explicit gather over (r, ho, wo, ky, kx, c), the shift rule
   on the step index, the split ranges, out_off / bout_off.  Each returns, per output buffer, a `Ref`:
     idx    the WRITE SET: flat indices of the buffer the contract says are written
     val    the float64 value of every written element
     S      the magnitude: the same computation with every operand replaced by its absolute value
            (|a'| @ |w|^T + |bias|; with norm-on-load |a'| = (|a| + |mean|) |rstd| |gamma| + |beta|; TN: |G|^T @ |a'| per split)
     bound  eps * S' + 2^-24 |R|   (S' = S carried through the epilogue, below)
     exact  elements that are exact statements (a mask said zero): the output is exactly the residual or exactly 0
     tanh   None, or the factor f of the extra 4 * 2^-24 * |out| * f the bound gets for tanhf (act 1)

2. BOUND.  An output passes when |out - ref| <= bound for every element of the write set.
     eps = (K + 8) * 2^-24                 exact-fp32 kernels
     eps = 2^-15 + (K + 8) * 2^-24         split-bf16 kernels
   K = the length of the sum (TN / conv_wgrad: the rows of the split; reduce_slabs: the number of slabs).
   Derivation: bf16 keeps 8 significant bits, so round-to-nearest leaves |x - hi| <= 2^-8 |x| (half an ulp of 2^-7),
   and lo = bf16(x - hi) leaves |x - hi - lo| <= 2^-17 |x|.  A split product a_hi w_hi + a_hi w_lo + a_lo w_hi misses
   a w by the dropped a_lo w_lo <= 2^-8 |a| * 2^-8 |w| = 2^-16 |a||w| plus the two representation errors
   2 * 2^-17 |a||w|: 2^-15 |a||w| in all (second-order terms are below 2^-24 and sit in the + 8).  The rest is
   worst-case fp32 accumulation of K terms (K * 2^-24 * S) plus the roundings of the prologue (four for the norm), the
   bias add and the epilogue's own operations (the + 8).
   (The issue this suite was written for stated 2^-16, taking 2^-9 for bf16's rounding error: that is the error of a
   9-bit format.  The first run on an MI355X showed correct kernels at up to 2.72e-5 * S = 0.89 * 2^-15 on single-product
   elements (K = 4, or one row x1e3 dominating a sum) -- 1.8 * 2^-16; test_gemm_contract_host_cpu.py constructs operands
   whose correctly rounded three-term product is off by more than 2^-16 and never by more than 2^-15.  The constant
   follows the arithmetic; a dropped term (2^-8 relative) still lies 100x outside.)
   tanh and ReLU are 1-Lipschitz, so S' = S behind them; the factor (1 - T^2)
   or the ReLU mask multiplies S'; the residual adds its own rounding 2^-24 |R|; tanhf adds 4 * 2^-24 |out|.
   (1 - T^2) is evaluated in fp32 with an absolute error of 2^-25, which reaches the output as 2^-25 |v| <= 2^-25 S:
   that stays inside eps * S * |1 - T^2| only while (K + 8) * |1 - T^2| >= 1/2.  The generator therefore draws the
   saved tanh outputs as 0.9 * tanh(.), |1 - T^2| >= 0.19: (K + 8) * 0.19 >= 1.7 for every K >= 1.
   These constants are derived, not tuned.

3. CASES.  cases(entry) is a fixed list (seeded RNG, identical on every call) in which EVERY PAIR of values of the
   dimensions in NT_DIMS / TN_DIMS / WG_DIMS occurs in at least one valid case, except the pairs that a named rule of
   *_RULES forbids under every completion (invalid_pairs(entry) lists them with the rule's name).  Validity = the
   WS_REQUIRE rules of the entry points plus what the kernels' vector loads need (vec bits).  Every case carries the
   kernel instantiation the dispatcher is expected to pick (`targets`), computed by mirroring ws_gemm_nt /
   ws_gemm_nt_bf16_nb / ws_launch_gemm_tn_bf16 / ws_conv_wgrad / ws_reduce_slabs and the vec_epi test of the bf16 NT kernel.

BUFFERS (build(case)).  Every operand and output lives inside a larger allocation with GUARD floats on both sides.
Outputs: the write set starts as NaN (with R aliasing C it necessarily starts as the residual), everything else holds
the finite sentinel SENT and must be bit-identical after the launch.  Inputs: everything the contract does not read is
NaN (guards, lda - K tails, channels C .. ldp of a pixel, padding rows, unused stat slots)."""
import ctypes
import itertools
from typing import NamedTuple, Optional

import numpy as np
import torch

GUARD = 4096
SENT = 24601.0
U = 2.0 ** -24
BIG = 1 << 30
NA = "n/a"
MAX_CASES = 400


class ContractViolation(AssertionError):
    def __init__(self, kind, msg):
        super().__init__(f"[{kind}] {msg}")
        self.kind = kind


class Ref(NamedTuple):
    idx: torch.Tensor
    val: torch.Tensor
    S: torch.Tensor
    bound: torch.Tensor
    exact: torch.Tensor
    tanh: Optional[torch.Tensor] = None


def eps_for(bf16: bool, K: int) -> float:
    return (2.0 ** -15 if bf16 else 0.0) + (K + 8) * U


def _is_bf16(mode):
    assert mode in ("f32", "bf16x3"), "the contract cases always name the product mode"
    return mode == "bf16x3"


def _row_off(m, rows):
    div, s1, s2 = rows
    return (m // div) * s1 + (m % div) * s2


def _host(ptr, n):
    """n floats at a raw host address (group tables carry pointers)."""
    return torch.from_numpy(np.ctypeslib.as_array((ctypes.c_float * int(n)).from_address(int(ptr))))


def _table(groups, ngroups, dtype):
    return np.frombuffer(groups.cpu().numpy().tobytes(), dtype=dtype)[:ngroups]


def _conv_fields(conv):
    mode, H, W, C, Ho, Wo, k, sh, sw, p = [int(v) for v in conv[:10]]
    dil = int(conv[10]) if len(conv) > 10 and conv[10] else 1
    ldp = int(conv[11]) if len(conv) > 11 and conv[11] else C
    return mode, H, W, C, Ho, Wo, k, sh, sw, p, dil, ldp


def patch_index(M, conv):
    """The implicit patch matrix as a gather: (idx [M, k*k*C] element offsets into the image, ok [M, k*k*C])."""
    mode, H, W, C, Ho, Wo, k, sh, sw, p, dil, ldp = _conv_fields(conv)
    m = torch.arange(M).unsqueeze(1)
    r, q = m // (Ho * Wo), m % (Ho * Wo)
    ho, wo = q // Wo, q % Wo
    kk = torch.arange(k * k * C).unsqueeze(0)
    tap, c = kk // C, kk % C
    ky, kx = tap // k, tap % k
    if mode == 0:
        h, w = ho * sh + ky * dil - p, wo * sw + kx * dil - p
        ok = (h >= 0) & (h < H) & (w >= 0) & (w < W)
    else:
        hn, wn = ho + p - ky * dil, wo + p - kx * dil
        h, w = torch.div(hn, sh, rounding_mode="floor"), torch.div(wn, sw, rounding_mode="floor")
        ok = (hn >= 0) & (wn >= 0) & (hn % sh == 0) & (wn % sw == 0) & (h < H) & (w < W)
    idx = ((r * H + h) * W + w) * ldp + c
    return torch.where(ok, idx, torch.zeros_like(idx)), ok


def _norm(a, absa, m, stats, stat_map, st_base, gamma, beta, K):
    d1, m1, d2, m2 = [int(v) for v in stat_map[:4]]
    s = (m // d1) * m1 + (m % d2) * m2 + int(st_base)
    st = stats.reshape(-1).double()
    mean, rstd = st[2 * s].unsqueeze(1), st[2 * s + 1].unsqueeze(1)
    gm, bt = gamma.reshape(-1)[:K].double(), beta.reshape(-1)[:K].double()
    return (a - mean) * rstd * gm + bt, (absa + mean.abs()) * rstd.abs() * gm.abs() + bt.abs()


def ref_gemm_nt(*, A, a_rows, M, C_out, c_rows, N=0, K=0, W=None, ldw=0, bias=None, R=None, T=None, stats=None,
                gamma=None, beta=None, stat_map=None, act=0, groups=None, ngroups=0, max_n=0, vec=3, a_off=0, c_off=0,
                w_off=0, mode=None, conv=None):
    from wesep_amd import _lib as L
    bf16 = _is_bf16(mode) and (vec & 3) == 3        # ws_gemm_nt: the split kernel needs both vector bits
    wt = bool(vec & 8)
    Af = A.reshape(-1)
    m = torch.arange(M)
    if groups is None:
        sm = stat_map or (1, 0, 1, 0, 0)
        gl = [dict(W=W.reshape(-1)[w_off:], bias=bias, gamma=gamma, beta=beta, a_off=0, c_off=0, st_base=sm[4], K=K, N=N,
                   ldw=ldw)]
    else:
        gl = []
        for gd in _table(groups, ngroups, L.GROUP_NT_DTYPE):
            Kg, Ng, lg = int(gd["K"]), int(gd["N"]), int(gd["ldw"])
            gl.append(dict(W=_host(gd["W"], (Kg if wt else Ng) * lg), bias=_host(gd["bias"], Ng) if gd["bias"] else None,
                           gamma=_host(gd["gamma"], Kg) if gd["gamma"] else None,
                           beta=_host(gd["beta"], Kg) if gd["beta"] else None, a_off=int(gd["a_off"]),
                           c_off=int(gd["c_off"]), st_base=int(gd["st_base"]), K=Kg, N=Ng, ldw=lg))
    out = []
    for g in gl:
        Kg, Ng, lg = g["K"], g["N"], g["ldw"]
        if conv is not None:
            idx, ok = patch_index(M, conv)
            a = torch.where(ok, Af[a_off + g["a_off"] + idx].double(), torch.zeros((), dtype=torch.float64))
        else:
            a = Af[(a_off + g["a_off"] + _row_off(m, a_rows)).unsqueeze(1) + torch.arange(Kg).unsqueeze(0)].double()
        absa = a.abs()
        if stats is not None:
            a, absa = _norm(a, absa, m, stats, stat_map, g["st_base"], g["gamma"], g["beta"], Kg)
        n_, k_ = torch.arange(Ng).unsqueeze(1), torch.arange(Kg).unsqueeze(0)
        w = g["W"].reshape(-1)[k_ * lg + n_ if wt else n_ * lg + k_].double()
        v, S = a @ w.t(), absa @ w.abs().t()
        if g["bias"] is not None:
            b = g["bias"].reshape(-1)[:Ng].double()
            v, S = v + b, S + b.abs()
        eps = eps_for(bf16, Kg)
        exact = torch.zeros(M, Ng, dtype=torch.bool)
        tanh = None
        if act == 1:
            v, tanh = torch.tanh(v), torch.ones(M, Ng, dtype=torch.float64)
        if act == 2:
            exact = v + eps * S < 0          # clearly negative pre-activation: exactly 0 behind the ReLU
            v = torch.relu(v)
        cidx = (c_off + g["c_off"] + _row_off(m, c_rows)).unsqueeze(1) + torch.arange(Ng).unsqueeze(0)
        Sp = S.clone()
        if T is not None:
            t = T.reshape(-1)[cidx].double()
            f = (t > 0).double() if act == 4 else 1 - t * t
            if act == 4:
                exact = exact | (t <= 0)
            v, Sp = v * f, Sp * f.abs()
            if tanh is not None:
                tanh = tanh * f.abs()
        bound = eps * Sp
        if R is not None:
            r = R.reshape(-1)[cidx].double()
            v, bound = v + r, bound + U * r.abs()
        v = torch.where(exact, (R.reshape(-1)[cidx].double() if R is not None else torch.zeros_like(v)), v)
        out.append(Ref(cidx.reshape(-1), v.reshape(-1), S.reshape(-1), bound.reshape(-1), exact.reshape(-1),
                       None if tanh is None else tanh.reshape(-1)))
    return {"C": _cat(out)}


def _cat(refs):
    if len(refs) == 1:
        return refs[0]
    th = None if refs[0].tanh is None else torch.cat([r.tanh for r in refs])
    return Ref(*[torch.cat([r[i] for r in refs]) for i in range(5)], th)


def _split_sums(g, a, absa, nsplit, rows, M, bf16):
    """Per split: (G^T a, |G|^T |a'|, eps * S) of the rows [s * rows, min(M, (s + 1) * rows))."""
    Nn, Kk = g.shape[1], a.shape[1]
    vals, Ss, bs = [], [], []
    for sp in range(nsplit):
        lo, hi = sp * rows, min(M, (sp + 1) * rows)
        if hi > lo:
            v, S = g[lo:hi].t() @ a[lo:hi], g[lo:hi].abs().t() @ absa[lo:hi]
        else:
            v = S = torch.zeros(Nn, Kk, dtype=torch.float64)
        vals.append(v.reshape(-1))
        Ss.append(S.reshape(-1))
        bs.append(eps_for(bf16, max(hi - lo, 0)) * S.reshape(-1))
    return vals, Ss, bs


def _tn_refs(g, a, absa, nsplit, rows, M, bf16, slab_stride, out_off, bslab, bslab_stride, bout_off):
    Nn, Kk = g.shape[1], a.shape[1]
    vals, Ss, bs = _split_sums(g, a, absa, nsplit, rows, M, bf16)
    idx = torch.cat([sp * slab_stride + out_off + torch.arange(Nn * Kk) for sp in range(nsplit)])
    z = torch.zeros(idx.numel(), dtype=torch.bool)
    res = {"slab": Ref(idx, torch.cat(vals), torch.cat(Ss), torch.cat(bs), z)}
    if bslab is not None:
        one = torch.ones(M, 1, dtype=torch.float64)
        vals, Ss, bs = _split_sums(g, one, one, nsplit, rows, M, bf16)
        idx = torch.cat([sp * bslab_stride + bout_off + torch.arange(Nn) for sp in range(nsplit)])
        res["bslab"] = Ref(idx, torch.cat(vals), torch.cat(Ss), torch.cat(bs), torch.zeros(idx.numel(), dtype=torch.bool))
    return res


def ref_gemm_tn(*, G, g_rows, A, a_rows, M, slab, slab_stride, nsplit, rows_per_split, Nn=0, Kk=0, bslab=None,
                bslab_stride=0, out_off=0, bout_off=0, stats=None, gamma=None, beta=None, stat_map=None, shift_rows=0,
                seq_div=1, seq_len=1, groups=None, ngroups=0, max_n=0, max_k=0, vec=1, g_off=0, a_off=0, mode=None,
                conv=None):
    from wesep_amd import _lib as L
    bf16 = _is_bf16(mode)
    Gf, Af = G.reshape(-1), A.reshape(-1)
    m = torch.arange(M)
    if groups is None:
        sm = stat_map or (1, 0, 1, 0, 0)
        gl = [dict(gamma=gamma, beta=beta, g_off=0, a_off=0, st_base=sm[4], out_off=out_off, bout_off=bout_off, Nn=Nn, Kk=Kk)]
    else:
        gl = []
        for gd in _table(groups, ngroups, L.GROUP_TN_DTYPE):
            kg = int(gd["Kk"])
            gl.append(dict(gamma=_host(gd["gamma"], kg) if gd["gamma"] else None,
                           beta=_host(gd["beta"], kg) if gd["beta"] else None, g_off=int(gd["g_off"]),
                           a_off=int(gd["a_off"]), st_base=int(gd["st_base"]), out_off=int(gd["out_off"]),
                           bout_off=int(gd["bout_off"]), Nn=int(gd["Nn"]), Kk=kg))
    res = []
    for g_ in gl:
        ng, kg = g_["Nn"], g_["Kk"]
        g = Gf[(g_off + g_["g_off"] + _row_off(m, g_rows)).unsqueeze(1) + torch.arange(ng).unsqueeze(0)].double()
        if conv is not None:
            idx, ok = patch_index(M, conv)
            a = torch.where(ok, Af[a_off + g_["a_off"] + idx].double(), torch.zeros((), dtype=torch.float64))
        else:
            mm, ok = m, torch.ones(M, dtype=torch.bool)
            if shift_rows != 0:     # m' = m + shift_rows; the row is zero when the step index +/- 1 leaves [0, seq_len)
                t2 = (m // seq_div) % seq_len + (1 if shift_rows > 0 else -1)
                ok = (t2 >= 0) & (t2 < seq_len)
                mm = torch.where(ok, m + shift_rows, m)
            a = Af[(a_off + g_["a_off"] + _row_off(mm, a_rows)).unsqueeze(1) + torch.arange(kg).unsqueeze(0)].double()
            a = torch.where(ok.unsqueeze(1), a, torch.zeros((), dtype=torch.float64))
        absa = a.abs()
        if stats is not None:
            a, absa = _norm(a, absa, m, stats, stat_map, g_["st_base"], g_["gamma"], g_["beta"], kg)
            if shift_rows != 0:     # the zeroed row stays zero: it is the operand that is replaced, not the raw load
                a, absa = a * ok.unsqueeze(1), absa * ok.unsqueeze(1)
        res.append(_tn_refs(g, a, absa, nsplit, rows_per_split, M, bf16, slab_stride, g_["out_off"], bslab, bslab_stride,
                            g_["bout_off"]))
    out = {"slab": _cat([r["slab"] for r in res])}
    if bslab is not None:
        out["bslab"] = _cat([r["bslab"] for r in res])
    return out


def ref_conv_wgrad(*, G, ldg, X, M, Nn, conv, slab, nsplit, tiles_per_split, bslab=None):
    Kk = int(conv[6]) ** 2 * int(conv[3])
    m = torch.arange(M)
    g = G.reshape(-1)[(m * ldg).unsqueeze(1) + torch.arange(Nn).unsqueeze(0)].double()
    idx, ok = patch_index(M, conv)
    a = torch.where(ok, X.reshape(-1)[idx].double(), torch.zeros((), dtype=torch.float64))
    return _tn_refs(g, a, a.abs(), nsplit, 32 * tiles_per_split, M, True, Nn * Kk, 0, bslab, Nn, 0)


def ref_reduce_slabs(slab, nsplit, stride, count, out, w=0, ldo=0, out_off=0):
    s = slab.reshape(-1).double()
    i = torch.arange(count)
    rows = torch.stack([s[k * stride + i] for k in range(nsplit)])
    o = out_off + ((i // w) * ldo + (i % w) if w > 0 else i)
    S = rows.abs().sum(0)
    return {"out": Ref(o, rows.sum(0), S, eps_for(False, nsplit) * S, torch.zeros(count, dtype=torch.bool))}


# ------------------------------------------------------------------------------------------------------------
# checker
# ------------------------------------------------------------------------------------------------------------
def check(out, before, ref: Ref, what="", base=0):
    """`out` (the whole allocation) against `ref`; `before` = the allocation as it was uploaded; `base` = where the tensor
    the call received starts inside it.  Returns the worst err / bound (0 when every bound is 0 and met).  Raises
    ContractViolation(kind): nan | exact | bound | sentinel."""
    o = out.detach().cpu().reshape(-1)
    if base:
        ref = ref._replace(idx=ref.idx + base)
    got = o[ref.idx]
    if torch.isnan(got).any():
        j = int(torch.isnan(got).nonzero()[0])
        raise ContractViolation("nan", f"{what}: element {int(ref.idx[j])} of the write set is NaN (unwritten?)")
    gd = got.double()
    ex = ref.exact
    if ex.any() and not torch.equal(got[ex], ref.val[ex].float()):
        j = int((got[ex] != ref.val[ex].float()).nonzero()[0])
        raise ContractViolation("exact", f"{what}: masked element {int(ref.idx[ex][j])} is {float(got[ex][j])!r}, "
                                         f"the contract says exactly {float(ref.val[ex][j])!r}")
    err = (gd - ref.val).abs()
    bound = ref.bound if ref.tanh is None else ref.bound + 4 * U * gd.abs() * ref.tanh
    bad = (err > bound) & ~ex
    if bad.any():
        j = int((err / bound.clamp_min(1e-300) * bad).argmax())
        raise ContractViolation("bound", f"{what}: {int(bad.sum())} elements outside the bound; worst at {int(ref.idx[j])}: "
                                         f"got {float(gd[j])!r} ref {float(ref.val[j])!r} err {float(err[j]):.3e} "
                                         f"bound {float(bound[j]):.3e} S {float(ref.S[j]):.3e}")
    keep = torch.ones(o.numel(), dtype=torch.bool)
    keep[ref.idx] = False
    a, b = o.view(torch.int32)[keep], before.detach().cpu().reshape(-1).view(torch.int32)[keep]
    if not torch.equal(a, b):
        j = int(keep.nonzero().reshape(-1)[(a != b).nonzero()[0]])
        raise ContractViolation("sentinel", f"{what}: element {j} outside the write set changed "
                                            f"({float(before.reshape(-1)[j])!r} -> {float(o[j])!r})")
    pos = (bound > 0) & ~ex
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def bound_of_plain_product(A, W, bf16=True):
    """(ref, bound) of A @ W^T for the blocked-layout tests: S from plain |A| @ |W|^T."""
    A, W = A.detach().double().cpu(), W.detach().double().cpu()
    return A @ W.t(), eps_for(bf16, A.shape[1]) * (A.abs() @ W.abs().t())


def assert_elementwise(out, ref, bound, what=""):
    err = (out.detach().double().cpu() - ref).abs()
    bad = err > bound
    assert not bad.any(), (f"{what}: {int(bad.sum())} elements outside eps * S; worst err / bound "
                           f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
    return float((err / bound.clamp_min(1e-300)).max())


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, pairwise generator
# ------------------------------------------------------------------------------------------------------------
CONV_SUB = ("k", "stride", "dil", "p", "C", "ldp", "img")
CONV_DIMS = {"k": [1, 3, 5], "stride": [(1, 1), (1, 2), (2, 1), (2, 2)], "dil": [1, 2, 3], "p": ["0", "k/2", "dil*k/2"],
             "C": [4, 12, 16, 80], "ldp": ["0", "C+4", "5C"], "img": ["1xT", "Tx1", "3x5", "13x37"]}
IMG = {"1xT": (1, 23), "Tx1": (23, 1), "3x5": (3, 5), "13x37": (13, 37)}

NT_DIMS = {"mode": ["f32", "bf16x3"], "M": [1, 31, 32, 33, 127, 128, 129, 257, 1001],
           "N": [1, 4, 12, 30, 32, 36, 60, 64, 68, 96, 124, 128, 132, 260],
           "K": [1, 3, 4, 6, 28, 32, 36, 70, 100, 132, 512], "vec": [0, 1, 2, 3],
           "a_rows": ["flat", "padded", "two"], "c_rows": ["flat", "padded", "two"], "c_align": [0, 1], "bias": [0, 1],
           "act": [0, 1, 2, 4], "T": [0, 1], "R": ["off", "sep", "alias"], "norm": [0, 1], "groups": [0, 1],
           "wt": ["off", "N", "N+4"], "conv": ["off", "m0", "m1"], **CONV_DIMS}
TN_DIMS = {"mode": ["f32", "bf16x3"], "M": NT_DIMS["M"], "Nn": [4, 12, 16, 32, 36, 128, 200],
           "Kk": [1, 6, 32, 100, 128, 132, 512], "vec": [0, 1], "g_rows": ["flat", "padded", "two"],
           "a_rows": ["flat", "padded", "two"], "split": ["one", "exact", "partial", "empty", "odd"], "bias": [0, 1],
           "out_off": [0, 1], "norm": [0, 1], "shift": [0, -1, 1, -10, 10], "groups": [0, 1], "conv": ["off", "m0"],
           **CONV_DIMS}
WG_DIMS = {"Nn": [4, 8, 16, 32], "ldg": ["Nn", "Nn+4", "80"], "split": ["one", "exact", "ragged"], "bias": [0, 1],
           **CONV_DIMS}


def geometry(conv, img, k, stride, dil, p):
    """(H, W, Ho, Wo, p) of a view, or None when it has no output pixel."""
    H, W = IMG[img]
    sh, sw = stride
    pp = {"0": 0, "k/2": k // 2, "dil*k/2": dil * (k // 2)}[p]
    if conv == "m0":
        nh, nw = H + 2 * pp - dil * (k - 1) - 1, W + 2 * pp - dil * (k - 1) - 1
        if nh < 0 or nw < 0:
            return None
        return H, W, nh // sh + 1, nw // sw + 1, pp
    Ho, Wo = (H - 1) * sh - 2 * pp + dil * (k - 1) + 1, (W - 1) * sw - 2 * pp + dil * (k - 1) + 1
    return (H, W, Ho, Wo, pp) if Ho >= 1 and Wo >= 1 else None


def _on(c):
    return c not in ("off", NA)


# (name, dims, violated(values...)).  A rule is evaluated only when all its dims are assigned.
_CONV_RULES = [
    ("the view has no output pixel (window larger than the padded image)", ("conv", "img", "k", "stride", "dil", "p"),
     lambda conv, img, k, stride, dil, p: _on(conv) and geometry(conv, img, k, stride, dil, p) is None),
]


def _sub_rules(conv_key="conv"):
    rules = []
    for d in CONV_SUB:
        rules.append((f"{d} exists only with a conv view", (conv_key, d), lambda conv, v: _on(conv) != (v != NA)))
    rules.append(_CONV_RULES[0])
    return rules


NT_RULES = [
    ("split-bf16 NT needs vec bits 0 and 1 (otherwise ws_gemm_nt runs an fp32 kernel)", ("mode", "vec"),
     lambda mode, vec: mode == "bf16x3" and vec != 3),
    ("split-bf16 NT loads float4: K % 4 == 0", ("mode", "K"), lambda mode, K: mode == "bf16x3" and K != NA and K % 4 != 0),
    ("vec bit 0/1 needs K % 4 == 0", ("vec", "K"), lambda vec, K: vec != 0 and K != NA and K % 4 != 0),
    ("act 4 reads the saved output T", ("act", "T"), lambda act, T: act == 4 and not T),
    ("transposed W needs the split-bf16 kernel", ("wt", "mode"), lambda wt, mode: wt != "off" and mode != "bf16x3"),
    ("transposed W needs vec 15", ("wt", "vec"), lambda wt, vec: wt != "off" and vec != 3),
    ("transposed W needs N % 4 == 0", ("wt", "N"), lambda wt, N: wt != "off" and N % 4 != 0),
    ("transposed W needs K % 4 == 0 (A is float4-loaded)", ("wt", "K"), lambda wt, K: wt != "off" and K != NA and K % 4 != 0),
    ("transposed W excludes norm-on-load", ("wt", "norm"), lambda wt, norm: wt != "off" and norm),
    ("transposed W excludes the conv view", ("wt", "conv"), lambda wt, conv: wt != "off" and conv != "off"),
    ("the conv view needs the split-bf16 kernel", ("conv", "mode"), lambda conv, mode: conv != "off" and mode != "bf16x3"),
    ("the conv view needs vec 7", ("conv", "vec"), lambda conv, vec: conv != "off" and vec != 3),
    ("the conv view excludes groups", ("conv", "groups"), lambda conv, groups: conv != "off" and groups),
    ("the conv view excludes norm-on-load", ("conv", "norm"), lambda conv, norm: conv != "off" and norm),
    ("M is derived from the view (R * Ho * Wo)", ("conv", "M"), lambda conv, M: (conv != "off") != (M == NA)),
    ("K is derived from the view (k * k * C)", ("conv", "K"), lambda conv, K: (conv != "off") != (K == NA)),
    ("the view ignores a_div / a_s1 / a_s2", ("conv", "a_rows"), lambda conv, a: (conv != "off") != (a == NA)),
] + _sub_rules()

TN_RULES = [
    ("vec bit 0 needs Kk % 4 == 0", ("vec", "Kk"), lambda vec, Kk: vec == 1 and Kk != NA and Kk % 4 != 0),
    ("the conv view needs the split-bf16 kernel", ("conv", "mode"), lambda conv, mode: conv != "off" and mode != "bf16x3"),
    ("the conv view excludes groups", ("conv", "groups"), lambda conv, groups: conv != "off" and groups),
    ("the conv view excludes norm-on-load", ("conv", "norm"), lambda conv, norm: conv != "off" and norm),
    ("the conv view excludes the shift", ("conv", "shift"), lambda conv, shift: conv != "off" and shift != 0),
    ("M is derived from the view (R * Ho * Wo)", ("conv", "M"), lambda conv, M: (conv != "off") != (M == NA)),
    ("Kk is derived from the view (k * k * C)", ("conv", "Kk"), lambda conv, K: (conv != "off") != (K == NA)),
    ("the view ignores a_div / a_s1 / a_s2", ("conv", "a_rows"), lambda conv, a: (conv != "off") != (a == NA)),
] + _sub_rules()

WG_RULES = [
    ("the view has no output pixel (window larger than the padded image)", ("img", "k", "stride", "dil", "p"),
     lambda img, k, stride, dil, p: geometry("m0", img, k, stride, dil, p) is None),
]

DIMS = {"gemm_nt": NT_DIMS, "gemm_tn": TN_DIMS, "conv_wgrad": WG_DIMS}
RULES = {"gemm_nt": NT_RULES, "gemm_tn": TN_RULES, "conv_wgrad": WG_RULES}


def _values(entry, d):
    v = list(DIMS[entry][d])
    if entry in ("gemm_nt", "gemm_tn") and (d in CONV_SUB or d in ("M", "K", "Kk", "a_rows")):
        v = v + [NA]
    return v


def violated(entry, assign):
    """Name of the first rule a (partial) assignment violates, or None."""
    for name, dims, fn in RULES[entry]:
        if all(d in assign for d in dims) and fn(*[assign[d] for d in dims]):
            return name
    return None


def pair_rule(entry, d1, v1, d2, v2):
    """Why the pair (d1 = v1, d2 = v2) occurs in no valid case: the name of a rule over both dimensions that is violated
    under every completion of its other dimensions, or the rules that every value of one third dimension runs into."""
    if NA in (v1, v2):
        return "n/a is not a value: the dimension does not exist in that case"
    base = {d1: v1, d2: v2}
    for name, dims, fn in RULES[entry]:
        if d1 in dims and d2 in dims:
            rest = [d for d in dims if d not in (d1, d2)]
            if all(fn(*[{**base, **dict(zip(rest, c))}[d] for d in dims])
                   for c in itertools.product(*[_values(entry, d) for d in rest])):
                return name
    for h in DIMS[entry]:
        if h in base:
            continue
        names = []
        for c in _values(entry, h):
            n = violated(entry, {**base, h: c})
            if n is None:
                break
            names.append(n)
        else:
            return f"every value of {h} is ruled out: " + "; ".join(sorted(set(names)))
    return None


class Case(NamedTuple):
    entry: str
    name: str
    dims: dict
    targets: tuple
    seed: int


def _complete(entry, fixed, rng):
    """A random valid assignment containing `fixed`, or None: dimensions are drawn one after the other (the conv view
    first), each from the values no rule refuses so far; a dead end starts over."""
    dims = DIMS[entry]
    order = [d for d in ("conv", "mode") if d in dims] + [d for d in dims if d not in ("conv", "mode")]
    for _ in range(200):
        a = dict(fixed)
        for d in order:
            if d in a:
                continue
            vals = _values(entry, d)
            for j in rng.permutation(len(vals)):
                a[d] = vals[int(j)]
                if violated(entry, a) is None:
                    break
            else:
                break
        else:
            if violated(entry, a) is None:
                return {d: a[d] for d in dims}
    return None


def _pairs_of(entry, a):
    ks = list(DIMS[entry])
    return {(ks[i], a[ks[i]], ks[j], a[ks[j]]) for i in range(len(ks)) for j in range(i + 1, len(ks))
            if a[ks[i]] != NA and a[ks[j]] != NA}


def all_pairs(entry):
    ks = list(DIMS[entry])
    return [(ks[i], v1, ks[j], v2) for i in range(len(ks)) for j in range(i + 1, len(ks))
            for v1 in DIMS[entry][ks[i]] for v2 in DIMS[entry][ks[j]]]


_CACHE = {}
# Other contract suites (tests/blk_contract.py) add their entry points to DIMS / RULES / TOPUP / INST / SEEDS and name, in
# PLANNERS, the function (dims, seed) -> targets that mirrors their dispatcher; cases(entry) then serves them as well.
SEEDS = {"gemm_nt": 1, "gemm_tn": 2, "conv_wgrad": 3}
PLANNERS = {}


def invalid_pairs(entry):
    cases(entry)
    return _CACHE[entry][1]


# every instantiation / branch has to be the expected target of at least this many cases
MIN_PER_TARGET = 8
NT_INST = [f"gemm_nt_kernel<{a},{w}>" for a in (0, 1) for w in (0, 1)] + ["gemm_nt_bf16_kernel<NORM,NB4>"] + [
    f"gemm_nt_bf16_kernel<{k},NB{nb}>" for k in ("PLAIN", "CONV", "WT") for nb in (1, 2, 4)]
TN_INST = ["gemm_tn_kernel<0>", "gemm_tn_kernel<1>"] + [f"gemm_tn_bf16_kernel<CONV{c},NARROW{n}>" for c in (0, 1)
                                                        for n in (0, 1)]
WG_INST = ["conv_wgrad_kernel[1 chunk]", "conv_wgrad_kernel[multi chunk]"]
RS_INST = ["reduce_slabs_few_kernel", "reduce_slabs_2d_kernel<16>", "reduce_slabs_2d_kernel<4>", "reduce_slabs_kernel"]
INST = {"gemm_nt": NT_INST, "gemm_tn": TN_INST, "conv_wgrad": WG_INST, "reduce_slabs": RS_INST}
EPI = ("epilogue:vec", "epilogue:scalar")

# partial assignments the generator tops up with random completions until MIN_PER_TARGET cases reach the target;
# the last block: both epilogues of the bf16 NT kernel with every act, with T, with R and with R aliasing C
_NT_TOPUP = ([({"mode": "f32", "vec": v}, f"gemm_nt_kernel<{v & 1},{v >> 1}>", MIN_PER_TARGET) for v in range(4)] +
             [({"mode": "bf16x3", "norm": 1}, "gemm_nt_bf16_kernel<NORM,NB4>", MIN_PER_TARGET)] +
             [({"mode": "bf16x3", "norm": 0, "groups": 0, "N": n, **extra}, f"gemm_nt_bf16_kernel<{k},NB{nb}>", MIN_PER_TARGET)
              for k, extra in (("PLAIN", {"wt": "off", "conv": "off"}), ("CONV", {"conv": "m0", "wt": "off"}),
                               ("CONV", {"conv": "m1", "wt": "off"}), ("WT", {"wt": "N+4", "conv": "off"}))
              for nb, n in ((1, 12), (1, 32), (2, 36), (2, 64), (4, 68), (4, 132)) if not (k == "WT" and n % 4)] +
             [({"mode": "bf16x3", "c_align": al, "N": 36 if al else 64, "act": act, **extra}, tag, 1)
              for al, tag in ((0, EPI[0]), (1, EPI[1])) for act in (0, 1, 2, 4)
              for extra in ({"T": 1, "R": "off"}, {"R": "sep"}, {"R": "alias"})])
_TN_TOPUP = ([({"mode": "f32", "vec": v}, f"gemm_tn_kernel<{v}>", MIN_PER_TARGET) for v in (0, 1)] +
             [({"mode": "bf16x3", "conv": c, "Nn": n, "norm": 0, "groups": 0}, f"gemm_tn_bf16_kernel<CONV{int(c != 'off')},NARROW{nr}>",
               MIN_PER_TARGET) for c in ("off", "m0") for nr, n in ((1, 16), (1, 32), (0, 36), (0, 200))])
_WG_TOPUP = [({"k": 5, "C": 80}, WG_INST[1], MIN_PER_TARGET), ({"k": 3}, WG_INST[0], MIN_PER_TARGET)]
TOPUP = {"gemm_nt": _NT_TOPUP, "gemm_tn": _TN_TOPUP, "conv_wgrad": _WG_TOPUP}


def cases(entry):
    """The fixed case list of an entry point (gemm_nt | gemm_tn | conv_wgrad | reduce_slabs)."""
    if entry in _CACHE:
        return _CACHE[entry][0]
    if entry == "reduce_slabs":
        out = _reduce_cases()
        _CACHE[entry] = (out, {})
        return out
    rng = np.random.default_rng(SEEDS[entry])
    todo = all_pairs(entry)
    covered, invalid, chosen = set(), {}, []
    for pr in todo:
        if pr in covered or pr in invalid:
            continue
        why = pair_rule(entry, *pr)
        if why:
            invalid[pr] = why
            continue
        best = None
        for _ in range(40):     # a few completions; keep the one that covers the most new pairs
            a = _complete(entry, {pr[0]: pr[1], pr[2]: pr[3]}, rng)
            if a is None:
                continue
            gain = len(_pairs_of(entry, a) - covered)
            if best is None or gain > best[0]:
                best = (gain, a)
        if best is None:
            invalid[pr] = "UNNAMED: no valid completion found"     # the CPU test refuses these
            continue
        chosen.append(best[1])
        covered |= _pairs_of(entry, best[1])
    out = [_mk_case(entry, a, i) for i, a in enumerate(chosen)]
    for fixed, tag, need in TOPUP[entry]:
        # (need 1: a case with exactly these values; otherwise the target's count over the whole list)
        have = sum(1 for c in out if tag in c.targets and (need > 1 or all(c.dims[d] == v for d, v in fixed.items())))
        tries = 0
        while have < need and tries < 50:
            tries += 1
            a = _complete(entry, fixed, rng)
            if a is None:
                continue
            c = _mk_case(entry, a, len(out))
            if tag in c.targets:
                out.append(c)
                have += 1
    assert len(out) <= MAX_CASES, (entry, len(out))
    _CACHE[entry] = (out, invalid)
    return out


def _mk_case(entry, a, i):
    b = PLANNERS[entry](a, 1000 + i) if entry in PLANNERS else build(Case(entry, "", a, (), 1000 + i), plan_only=True)
    name = f"{i:03d}-" + "-".join(f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v) for v in a.values() if v != NA)
    return Case(entry, name, a, b, 1000 + i)


def _reduce_cases():
    out = []
    i = 0
    for count in (1, 8, 9, 64, 100, 4097, 16384, 16385, 65536, 65537):
        for nsplit in (1, 15, 16, 17, 63, 64, 65, 130):
            if count > 20000 and nsplit > 65:
                continue
            for w, oo in (((0, 0), (1, 1)) if (count + nsplit) % 2 else ((1, 0), (0, 1))):
                a = {"count": count, "nsplit": nsplit, "w": w, "out_off": oo}
                if count <= 8 and nsplit >= 64:
                    t = RS_INST[0]
                elif count <= 65536 and nsplit >= 64:
                    t = RS_INST[1]
                elif count <= 16384 and nsplit >= 16:
                    t = RS_INST[2]
                else:
                    t = RS_INST[3]
                out.append(Case("reduce_slabs", f"{i:03d}-count{count}-nsplit{nsplit}-w{w}-off{oo}", a, (t,), 5000 + i))
                i += 1
    return out


# ------------------------------------------------------------------------------------------------------------
# builders: a case -> CPU buffers + the keyword arguments of the wesep_amd.dev call
# ------------------------------------------------------------------------------------------------------------
class Buf(NamedTuple):
    """Placeholder of a tensor argument: buffer `name`, optionally the slice [lo, hi) of it."""
    name: str
    lo: int = -1
    hi: int = -1


class Built:
    def __init__(self, case):
        self.case = case
        self.bufs = {}          # name -> CPU float32 tensor (the whole allocation)
        self.kw = {}            # dev keyword arguments; tensors as Buf placeholders
        self.groups = None      # list of dicts (pointer fields as (buffer name, offset)) or None
        self.group_dtype = None
        self.outs = []          # output buffer names, in the order of the reference's dict
        self.out_keys = {}      # reference key -> buffer name
        self.blocks = []        # TN / conv_wgrad: per group (out_off, Nn * Kk, bout_off, Nn) inside a split's slab

    def base(self, name):
        """Where the tensor the call receives starts inside the allocation `name`."""
        v = next(v for v in self.kw.values() if isinstance(v, Buf) and v.name == name)
        return max(v.lo, 0)

    def kwargs(self, tensors, device="cpu"):
        """The dev.* keyword arguments over `tensors` (the buffers on some device)."""
        from wesep_amd import _lib as L
        kw = {}
        for k, v in self.kw.items():
            if isinstance(v, Buf):
                t = tensors[v.name]
                kw[k] = t if v.lo < 0 else t[v.lo:v.hi]
            else:
                kw[k] = v
        if self.groups is not None:
            desc = np.zeros(len(self.groups), dtype=self.group_dtype)
            for i, g in enumerate(self.groups):
                for f, v in g.items():
                    desc[i][f] = (tensors[v[0]].data_ptr() + 4 * v[1]) if isinstance(v, tuple) else v
            kw["groups"] = L.upload_struct_array(desc, device)
        return kw


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def draw(g, rows, cols):
    """Mixed scales: some rows x1e3, some columns x1e-3, some exact zeros, both signs."""
    x = torch.randn(rows, cols, generator=g)
    x = x * torch.where(torch.rand(rows, 1, generator=g) < 0.1, 1e3, 1.0)
    x = x * torch.where(torch.rand(1, cols, generator=g) < 0.1, 1e-3, 1.0)
    return torch.where(torch.rand(rows, cols, generator=g) < 0.05, torch.zeros(()), x).float()


def _alloc(n, fill):
    return torch.full((int(n) + 2 * GUARD,), fill, dtype=torch.float32)


alloc, gen, pairs_of = _alloc, _gen, _pairs_of      # public names of the helpers other contract suites share


def _rows_layout(kind, M, width, vec4):
    """(Rows, span): where the M rows of `width` floats go; padded / two-level layouts leave holes."""
    pad = 4 if vec4 or width % 4 == 0 else 3
    if kind in ("flat", NA):
        return (BIG, 0, width), M * width
    ld = width + pad
    if kind == "padded":
        return (BIG, 0, ld), M * ld
    div = 7 if M >= 7 else 1
    s1 = (div + 2) * ld
    return (div, s1, ld), ((M - 1) // div) * s1 + ((M - 1) % div) * ld + width


def _fill_rows(buf, off, rows, M, data):
    idx = (off + _row_off(torch.arange(M), rows)).unsqueeze(1) + torch.arange(data.shape[1]).unsqueeze(0)
    buf[idx] = data
    return idx


def _view(d, seed):
    """ConvView fields + image size of the conv dims of a case; R images."""
    conv = d.get("conv", "m0")
    k, (sh, sw), dil, C = d["k"], d["stride"], d["dil"], d["C"]
    H, W, Ho, Wo, p = geometry(conv, d["img"], k, d["stride"], dil, d["p"])
    ldp = {"0": 0, "C+4": C + 4, "5C": 5 * C}[d["ldp"]]
    R = 1 if Ho * Wo > 400 else 2 + seed % 2
    from wesep_amd.dev import ConvView
    return ConvView(0 if conv == "m0" else 1, H, W, C, Ho, Wo, k, sh, sw, p, dil, ldp), R


def _image(g, view, R):
    _, H, W, C, _, _, _, _, _, _, _, ldp = view
    ld = ldp or C
    X = _alloc(R * H * W * ld, float("nan"))
    img = X[GUARD:GUARD + R * H * W * ld].view(R * H * W, ld)
    img[:, :C] = draw(g, R * H * W, C)
    return X


def _stats(g, M, base):
    """StatMap with st_div1 != st_div2 and a base; only the slots the map reaches are finite."""
    d1, m1, d2, m2 = 5, 3, 3, 1
    m = torch.arange(M)
    s = (m // d1) * m1 + (m % d2) * m2
    n = int(s.max()) + 1
    return (d1, m1, d2, m2, base), s, n


def build(case, plan_only=False):
    if case.entry == "gemm_nt":
        return _build_nt(case, plan_only)
    if case.entry == "gemm_tn":
        return _build_tn(case, plan_only)
    if case.entry == "conv_wgrad":
        return _build_wg(case, plan_only)
    return _build_rs(case)


def _nt_targets(mode, vec, N_list, K, groups, norm, wt, conv, c_rows, c_offs, R_on, T_on):
    if mode == "bf16x3" and vec == 3:
        nb = 4 if (groups or norm) else (1 if N_list[0] <= 32 else 2 if N_list[0] <= 64 else 4)
        kind = "WT" if wt else "CONV" if conv else "NORM" if norm else "PLAIN"
        t = [f"gemm_nt_bf16_kernel<{kind},NB{nb}>"]
        for N, co in zip(N_list, c_offs):   # vec_epi: N % 4, c_s1 % 4, c_s2 % 4, 16-byte aligned C (and R, T: same offset)
            al = N % 4 == 0 and c_rows[1] % 4 == 0 and c_rows[2] % 4 == 0 and co % 4 == 0
            tag = EPI[0] if al else EPI[1]
            if tag not in t:
                t.append(tag)
        return tuple(t)
    return (f"gemm_nt_kernel<{vec & 1},{(vec >> 1) & 1}>",)


def _build_nt(case, plan_only):
    d, seed = case.dims, case.seed
    g = _gen(seed)
    conv_on, groups, norm, wt = d["conv"] != "off", bool(d["groups"]), bool(d["norm"]), d["wt"] != "off"
    vec, mode = d["vec"], d["mode"]
    view = None
    if conv_on:
        view, Rn = _view(d, seed)
        M, K = Rn * view[4] * view[5], view[6] ** 2 * view[3]
    else:
        M, K = d["M"], d["K"]
    N = d["N"]
    ng = 3 if groups else 1
    q = 4 if (vec or mode == "bf16x3") and K % 4 == 0 else 1
    Ks = [K, max(q, (K // 2) // q * q), max(q, K - q)][:ng]
    nq = 4 if wt else 1
    Ns = [N, max(nq, (N * 2 // 3) // nq * nq), max(nq, (N // 3) // nq * nq)][:ng]
    a_rows, a_span = _rows_layout(d["a_rows"], M, K, vec & 1)
    c_rows, c_span = _rows_layout(d["c_rows"], M, N, N % 4 == 0)
    if d["c_rows"] == "padded":     # a column block of a wider matrix: ldc = 2N + 8, the block starts at column N + 4
        c_rows, c_span = (BIG, 0, 2 * N + 8), M * (2 * N + 8)
    c0 = GUARD + (N + 4 if d["c_rows"] == "padded" else 0) + (2 if d["c_align"] else 0)
    a_reg, c_reg = (a_span + 15) // 4 * 4 + 8, (c_span + 15) // 4 * 4 + 8
    a_offs = [i * a_reg for i in range(ng)]
    c_offs = [i * c_reg for i in range(ng)]
    targets = _nt_targets(mode, vec, Ns, K, groups, norm, wt, conv_on, c_rows, [c0 + o for o in c_offs], d["R"] != "off",
                          d["T"])
    if plan_only:
        return targets
    b = Built(case)
    # A
    if conv_on:
        b.bufs["A"] = _image(g, view, Rn)
    else:
        A = _alloc(ng * a_reg, float("nan"))
        for i in range(ng):
            _fill_rows(A, GUARD + a_offs[i], a_rows, M, draw(g, M, Ks[i]))
        b.bufs["A"] = A
    # parameters: W, bias, gamma, beta of every group in one allocation, 16-byte aligned pieces between NaN gaps
    pieces, pos = {}, GUARD
    par = []
    for i in range(ng):
        Kg, Ng = Ks[i], Ns[i]
        if wt:
            ldw = Ng + (4 if d["wt"] == "N+4" else 0)
            Wm = torch.full((Kg, ldw), float("nan"))
            Wm[:, :Ng] = draw(g, Ng, Kg).t() * 0.1
        else:
            ldw = Kg + (4 if (i + seed) % 2 and Kg % 4 == 0 else 0)
            Wm = torch.full((Ng, ldw), float("nan"))
            Wm[:, :Kg] = draw(g, Ng, Kg) * 0.1
        for nm, t in (("W", Wm.reshape(-1)), ("bias", draw(g, 1, Ng).reshape(-1)), ("gamma", draw(g, 1, Kg).reshape(-1)),
                      ("beta", draw(g, 1, Kg).reshape(-1))):
            pieces[(nm, i)] = (pos, t)
            pos += (t.numel() + 19) // 4 * 4
        par.append(ldw)
    P = _alloc(pos - GUARD, float("nan"))
    for (nm, i), (o, t) in pieces.items():
        P[o:o + t.numel()] = t
    b.bufs["P"] = P

    def piece(nm, i):
        o, t = pieces[(nm, i)]
        return Buf("P", o, o + t.numel())
    # C (+ R, T with the same geometry)
    Cb = _alloc(ng * c_reg + 8 + N, SENT)
    widx = torch.cat([_fill_rows(Cb, c0 + c_offs[i], c_rows, M, torch.full((M, Ns[i]), float("nan"))).reshape(-1)
                      for i in range(ng)])
    b.bufs["C"] = Cb
    kw = dict(A=Buf("A"), a_rows=a_rows, M=M, C_out=Buf("C"), c_rows=c_rows, act=d["act"], vec=vec | (8 if wt else 0),
              a_off=GUARD, c_off=c0, mode=mode)
    if d["R"] != "off":
        rv = draw(g, 1, widx.numel()).reshape(-1)
        if d["R"] == "alias":
            Cb[widx] = rv
            kw["R"] = Buf("C")
        else:
            Rb = torch.full_like(Cb, float("nan"))
            Rb[widx] = rv
            b.bufs["R"] = Rb
            kw["R"] = Buf("R")
    if d["T"]:
        Tb = torch.full_like(Cb, float("nan"))
        t = torch.randn(widx.numel(), generator=g)
        if d["act"] == 4:           # saved ReLU outputs: exact zeros, negatives, nothing else within 1e-3 of 0
            t = torch.where(t.abs() < 1e-3, torch.full_like(t, 0.5), t)
            t = torch.where(torch.rand(widx.numel(), generator=g) < 0.15, torch.zeros(()), t)
        else:                       # saved tanh outputs, |T| <= 0.9 (module docstring)
            t = 0.9 * torch.tanh(t)
        Tb[widx] = t.float()
        b.bufs["T"] = Tb
        kw["T"] = Buf("T")
    if norm:
        sm, s, n = _stats(g, M, 2)
        St = _alloc(2 * (n + 2) * ng, float("nan"))
        bases = [2 + i * (n + 2) for i in range(ng)]
        for i in range(ng):
            St[GUARD + 2 * (s + bases[i])] = torch.randn(n, generator=g)[s]
            St[GUARD + 2 * (s + bases[i]) + 1] = (0.5 + 1.5 * torch.rand(n, generator=g))[s]
        b.bufs["stats"] = St
        kw["stats"] = Buf("stats", GUARD, St.numel() - GUARD)
        kw["stat_map"] = sm[:4] + (bases[0],)
    if groups:
        b.group_dtype = __import__("wesep_amd._lib", fromlist=["x"]).GROUP_NT_DTYPE
        b.groups = []
        for i in range(ng):
            gd = dict(W=("P", pieces[("W", i)][0]), bias=("P", pieces[("bias", i)][0]) if d["bias"] else 0,
                      gamma=("P", pieces[("gamma", i)][0]) if norm else 0, beta=("P", pieces[("beta", i)][0]) if norm else 0,
                      a_off=a_offs[i], c_off=c_offs[i], st_base=bases[i] if norm else 0, K=Ks[i], N=Ns[i], ldw=par[i])
            b.groups.append(gd)
        kw.update(ngroups=ng, max_n=max(Ns))
    else:
        kw.update(N=N, K=K, W=Buf("P"), w_off=pieces[("W", 0)][0], ldw=par[0])
        if d["bias"]:
            kw["bias"] = piece("bias", 0)
        if norm:
            kw["gamma"], kw["beta"] = piece("gamma", 0), piece("beta", 0)
    if conv_on:
        kw["conv"] = view
    b.kw, b.outs, b.out_keys = kw, ["C"], {"C": "C"}
    return b


def _tn_split(kind, M, unit=1):
    """(nsplit, rows_per_split) in units of `unit` rows."""
    n = -(-M // unit)
    if kind == "one":
        return 1, n
    if kind == "exact":
        dv = next((x for x in range(2, n + 1) if n % x == 0), 1)
        return dv, n // dv
    if kind in ("partial", "ragged"):
        rows = max(1, (n * 2 + 4) // 5)
        if n % rows == 0:
            rows += 1
        return -(-n // rows), rows
    if kind == "empty":
        ns, rows = _tn_split("partial", M, unit)
        return ns + 1, rows
    rows = 37 if n > 37 else max(1, n - 1)      # "odd": not a multiple of 32
    return -(-n // rows), rows


tn_split = _tn_split      # (public: tests/blk_contract.py splits block ranges with the same kinds)


def _build_tn(case, plan_only):
    d, seed = case.dims, case.seed
    g = _gen(seed)
    conv_on, groups, norm = d["conv"] != "off", bool(d["groups"]), bool(d["norm"])
    mode, vec, shift = d["mode"], d["vec"], d["shift"]
    view = None
    if conv_on:
        view, Rn = _view(d, seed)
        M, Kk = Rn * view[4] * view[5], view[6] ** 2 * view[3]
    else:
        M, Kk = d["M"], d["Kk"]
    seq_div, seq_len = 1, 1
    if shift:
        seq_div, seq_len = abs(shift), (3, 4, 5, 7)[seed % 4]
        M = -(-M // (seq_div * seq_len)) * seq_div * seq_len      # whole sequences: M % (seq_div * seq_len) == 0
    Nn = d["Nn"]
    ng = 3 if groups else 1
    q = 4 if vec and Kk % 4 == 0 else 1
    Ks = [Kk, max(q, (Kk // 2) // q * q), max(q, Kk - q)][:ng]
    Ns = [Nn, max(4, (Nn // 2) // 4 * 4), max(4, Nn - 4)][:ng]
    narrow = not groups and not norm and Nn <= 32
    targets = ((f"gemm_tn_bf16_kernel<CONV{int(conv_on)},NARROW{int(narrow)}>",) if mode == "bf16x3"
               else (f"gemm_tn_kernel<{vec}>",))
    if plan_only:
        return targets
    b = Built(case)
    g_rows, g_span = _rows_layout(d["g_rows"], M, Nn, True)
    a_rows, a_span = _rows_layout(d["a_rows"], M, Kk, vec)
    g_reg, a_reg = (g_span + 15) // 4 * 4 + 8, (a_span + 15) // 4 * 4 + 8
    Gb = _alloc(ng * g_reg, float("nan"))
    for i in range(ng):
        _fill_rows(Gb, GUARD + i * g_reg, g_rows, M, draw(g, M, Ns[i]))
    b.bufs["G"] = Gb
    if conv_on:
        b.bufs["A"] = _image(g, view, Rn)
    else:
        Ab = _alloc(ng * a_reg, float("nan"))
        for i in range(ng):
            _fill_rows(Ab, GUARD + i * a_reg, a_rows, M, draw(g, M, Ks[i]))
        b.bufs["A"] = Ab
    nsplit, rows = _tn_split(d["split"], M)
    oo = 12 if d["out_off"] else 0
    blk = [n * k for n, k in zip(Ns, Ks)]
    out_offs = [oo + sum(blk[:i]) + 5 * i for i in range(ng)]
    bout_offs = [(3 if d["out_off"] else 0) + sum(Ns[:i]) + 2 * i for i in range(ng)]
    slab_stride = out_offs[-1] + blk[-1] + 7
    bslab_stride = bout_offs[-1] + Ns[-1] + 3
    Sb = _alloc(nsplit * slab_stride, SENT)
    for sp in range(nsplit):
        for i in range(ng):
            o = GUARD + sp * slab_stride + out_offs[i]
            Sb[o:o + blk[i]] = float("nan")
    b.bufs["slab"] = Sb
    kw = dict(G=Buf("G"), g_rows=g_rows, A=Buf("A"), a_rows=a_rows, M=M, slab=Buf("slab", GUARD, Sb.numel()),
              slab_stride=slab_stride, nsplit=nsplit, rows_per_split=rows, vec=vec, g_off=GUARD, a_off=GUARD, mode=mode,
              shift_rows=shift, seq_div=seq_div, seq_len=seq_len)
    b.outs, b.out_keys = ["slab"], {"slab": "slab"}
    if d["bias"]:
        Bb = _alloc(nsplit * bslab_stride, SENT)
        for sp in range(nsplit):
            for i in range(ng):
                o = GUARD + sp * bslab_stride + bout_offs[i]
                Bb[o:o + Ns[i]] = float("nan")
        b.bufs["bslab"] = Bb
        kw.update(bslab=Buf("bslab", GUARD, Bb.numel()), bslab_stride=bslab_stride)
        b.outs.append("bslab")
        b.out_keys["bslab"] = "bslab"
    pieces, pos = {}, GUARD
    for i in range(ng):
        for nm in ("gamma", "beta"):
            pieces[(nm, i)] = pos
            pos += (Ks[i] + 19) // 4 * 4
    P = _alloc(pos - GUARD, float("nan"))
    for (nm, i), o in pieces.items():
        P[o:o + Ks[i]] = draw(g, 1, Ks[i]).reshape(-1)
    b.bufs["P"] = P
    bases = [0] * ng
    if norm:
        sm, s, n = _stats(g, M, 2)
        St = _alloc(2 * (n + 2) * ng, float("nan"))
        bases = [2 + i * (n + 2) for i in range(ng)]
        for i in range(ng):
            St[GUARD + 2 * (s + bases[i])] = torch.randn(n, generator=g)[s]
            St[GUARD + 2 * (s + bases[i]) + 1] = (0.5 + 1.5 * torch.rand(n, generator=g))[s]
        b.bufs["stats"] = St
        kw["stats"] = Buf("stats", GUARD, St.numel() - GUARD)
        kw["stat_map"] = sm[:4] + (bases[0],)
    if groups:
        b.group_dtype = __import__("wesep_amd._lib", fromlist=["x"]).GROUP_TN_DTYPE
        b.groups = [dict(gamma=("P", pieces[("gamma", i)]) if norm else 0, beta=("P", pieces[("beta", i)]) if norm else 0,
                         g_off=i * g_reg, a_off=i * a_reg, st_base=bases[i], out_off=out_offs[i], bout_off=bout_offs[i],
                         Nn=Ns[i], Kk=Ks[i]) for i in range(ng)]
        kw.update(ngroups=ng, max_n=max(Ns), max_k=max(Ks))
    else:
        kw.update(Nn=Nn, Kk=Kk, out_off=out_offs[0], bout_off=bout_offs[0])
        if norm:
            kw["gamma"] = Buf("P", pieces[("gamma", 0)], pieces[("gamma", 0)] + Kk)
            kw["beta"] = Buf("P", pieces[("beta", 0)], pieces[("beta", 0)] + Kk)
    if conv_on:
        kw["conv"] = view
    b.kw = kw
    b.blocks = [(out_offs[i], blk[i], bout_offs[i], Ns[i]) for i in range(ng)]
    return b


def _build_wg(case, plan_only):
    d, seed = case.dims, case.seed
    view, Rn = _view({**d, "conv": "m0"}, seed)
    M, Kk, Nn = Rn * view[4] * view[5], view[6] ** 2 * view[3], d["Nn"]
    if plan_only:
        return (WG_INST[1] if Kk > 768 else WG_INST[0],)
    g = _gen(seed)
    b = Built(case)
    ldg = {"Nn": Nn, "Nn+4": Nn + 4, "80": 80}[d["ldg"]]
    Gb = _alloc(M * ldg, float("nan"))
    Gb[GUARD:GUARD + M * ldg].view(M, ldg)[:, :Nn] = draw(g, M, Nn)
    b.bufs["G"], b.bufs["X"] = Gb, _image(g, view, Rn)
    nsplit, tiles = _tn_split(d["split"], M, 32)
    Sb = _alloc(nsplit * Nn * Kk, SENT)
    Sb[GUARD:GUARD + nsplit * Nn * Kk] = float("nan")
    b.bufs["slab"] = Sb
    kw = dict(G=Buf("G", GUARD, Gb.numel()), ldg=ldg, X=Buf("X", GUARD, b.bufs["X"].numel()), M=M, Nn=Nn, conv=view,
              slab=Buf("slab", GUARD, Sb.numel()), nsplit=nsplit, tiles_per_split=tiles)
    b.outs, b.out_keys = ["slab"], {"slab": "slab"}
    if d["bias"]:
        Bb = _alloc(nsplit * Nn, SENT)
        Bb[GUARD:GUARD + nsplit * Nn] = float("nan")
        b.bufs["bslab"] = Bb
        kw["bslab"] = Buf("bslab", GUARD, Bb.numel())
        b.outs.append("bslab")
        b.out_keys["bslab"] = "bslab"
    b.kw = kw
    b.blocks = [(0, Nn * Kk, 0, Nn)]
    return b


def wgrad_as_gemm_tn(kw):
    """The gemm_tn (conv.on) keyword arguments that state the same weight gradient as conv_wgrad's `kw`."""
    Nn, view = kw["Nn"], kw["conv"]
    Kk = view[6] ** 2 * view[3]
    out = dict(G=kw["G"], g_rows=(BIG, 0, kw["ldg"]), A=kw["X"], a_rows=(BIG, 0, Kk), M=kw["M"], slab=kw["slab"],
               slab_stride=Nn * Kk, nsplit=kw["nsplit"], rows_per_split=32 * kw["tiles_per_split"], Nn=Nn, Kk=Kk, vec=0,
               mode="bf16x3", conv=view)
    if "bslab" in kw:
        out.update(bslab=kw["bslab"], bslab_stride=Nn)
    return out


def _build_rs(case):
    d = case.dims
    g = _gen(case.seed)
    count, nsplit = d["count"], d["nsplit"]
    stride = count + 5
    b = Built(case)
    Sb = _alloc(nsplit * stride, float("nan"))
    Sb[GUARD:GUARD + nsplit * stride].view(nsplit, stride)[:, :count] = draw(g, nsplit, count)
    b.bufs["slab"] = Sb
    w = 7 if d["w"] and count >= 7 else (1 if d["w"] else 0)
    ldo = w + 3 if w else 0
    n_out = ((count - 1) // w) * ldo + w if w else count
    oo = GUARD + (5 if d["out_off"] else 0)
    Ob = _alloc(n_out + 8, SENT)
    i = torch.arange(count)
    Ob[oo + ((i // w) * ldo + (i % w) if w else i)] = float("nan")
    b.bufs["out"] = Ob
    b.kw = dict(slab=Buf("slab", GUARD, Sb.numel()), nsplit=nsplit, stride=stride, count=count, out=Buf("out"), w=w,
                ldo=ldo, out_off=oo)
    b.outs, b.out_keys = ["out"], {"out": "out"}
    return b


def reduced(ref: Ref, nsplit):
    """The reference of one group's block after ws_reduce_slabs over its splits (ref = that block, split-major):
    bound = sum of the splits' bounds + the fp32 sum of nsplit numbers of magnitude |val| + bound."""
    v, bd, S = ref.val.reshape(nsplit, -1), ref.bound.reshape(nsplit, -1), ref.S.reshape(nsplit, -1)
    n = v.shape[1]
    return Ref(torch.arange(n), v.sum(0), S.sum(0), bd.sum(0) + eps_for(False, nsplit) * (v.abs() + bd).sum(0),
               torch.zeros(n, dtype=torch.bool))


REFS = {"gemm_nt": ref_gemm_nt, "gemm_tn": ref_gemm_tn, "conv_wgrad": ref_conv_wgrad, "reduce_slabs": ref_reduce_slabs}


def reference(b: Built, tensors=None):
    """The reference of a built case, from its CPU buffers (before any launch)."""
    kw = b.kwargs(tensors or b.bufs, "cpu")
    if b.case.entry == "reduce_slabs":
        return ref_reduce_slabs(**kw)
    return REFS[b.case.entry](**kw)
