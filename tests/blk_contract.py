"""TEST INFRASTRUCTURE ONLY -- contract suite of the blocked-layout GEMM family of wesep_amd/csrc/gemm_blk.hip (ws_pack_w,
ws_pack_w_f16, ws_pack_w_f16f8, ws_gemm_p2b, ws_gemm_p2b_len, ws_gemm_b2p, ws_gemm_tnb; include/wesep_hip.h).  Same shape as
tests/gemm_contract.py, whose Ref / check / pairwise generator / guards it imports.  No GPU code here: the CPU test
(test_blk_contract_host_cpu.py) checks this module, the GPU test (test_blk_contract_gpu.py) runs every case through the C ABI.

1. REFERENCE.  ref_pack_w / ref_gemm_p2b / ref_gemm_b2p / ref_gemm_tnb take the keyword arguments of the wesep_amd.dev
   wrappers on CPU tensors (the opaque Wpack replaced by the logical weight W'[N][K] it was packed from) and restate the header
   in float64.  Activation operands are what is STORED: BLS pairs decode to hi + lo, BLH elements to their bf16 / fp16 value,
   scaled fp16 to value / S with S = ws_dgates_scale(*amax) -- all exact in float64, so the quantisation of an input format is
   not an error of the kernel.  Index formulas are written out from the header text (positions(), bl_index()), not taken from
   dev.to_blocked; the host test shows the two agree.

2. BOUNDS.  |out - ref| <= eps_fmt * S + (K + 8) * 2^-24 * S + floors, S = the same sum over the magnitudes of the terms the
   kernel adds (|hi| + |lo| of every split operand), K = the length of the sum (tnb: 32 * blocks of the split).
   u8 = 2^-8 is bf16's rounding error (8 significant bits), u11 = 2^-11 fp16's.  A STORED pair x = hi + lo has |lo| <= u8 |x|
   (first order); a pair the kernel SPLITS itself from an fp32 x leaves x - hi - lo <= u8 * u8 / 2 |x| = 2^-17 |x|.
     p2b          fp32 A split in the kernel against a split-bf16 pack, three terms: the dropped lo * lo (2^-16) + both
                  representation errors (2 * 2^-17) = 2^-15, the constant of the generic sweep.  GroupNorm-on-load uses
                  gemm_contract's |a'| magnitude; its four fp32 roundings sit in the + 8.
     b2p a_fmt 0  stored pairs (exact) against a split-bf16 pack: dropped lo * lo 2^-16 + the weight's 2^-17 = 1.5 * 2^-16.
     b2p a_fmt 1  bf16 A (exact), hi / lo weights, two terms, nothing dropped: the weight's representation error 2^-17.
     b2p a_fmt 2  scaled fp16 A (exact) against fp16 hi / lo of 256 w: hi leaves a remainder <= u11 |256 w|, lo = fp16(remainder)
                  misses it by u11 of that: 2^-22 relative; where the remainder is an fp16 subnormal (< 2^-14) the error is
                  half the subnormal spacing, 2^-25 of 256 w = 2^-33 of w: floor 2^-33 * sum_k |a|.
     b2p a_fmt 3  hi term exact; lo term = e4m3(a / 256) * 256 times e4m3(r / 2^E) * 2^E for the remainder r = 256 w - hi, E the
                  fragment's exponent (largest code in [128, 256)).  e4m3 keeps 4 significant bits: |q(x) - x| <= 2^-4 |x| for
                  normals, <= 2^-10 (half the subnormal spacing 2^-9) below 2^-6, so with da = 2^-4 |a| + 2^-2 (256 * 2^-10)
                  and dr = 2^-4 |r| + 2^(E - 10):  err <= sum_k |a| dr + da |r| + da dr, everything over 256 S.  The floor
                  2^-2 |r| is stated with the fragment's maximum 2^(E + 8) >= |r|, not per element.  |r| <= 2^-11 |256 w|, so
                  the term is about 2^-14 of the product.
     tnb g_fmt 0  stored pairs on both sides, three terms: the dropped lo * lo, 2^-16.
     tnb g_fmt 1  bf16 G (exact) times stored pairs, two terms: nothing dropped, accumulation only.
     tnb g_fmt 2  WS_TNB_F16=0: the fp16 G splits exactly into bf16 hi + lo (11 = 8 + 3 bits) and runs the three-term product:
                  2^-16.  Default (fp16 instruction): G as it is, the A pair's terms lifted by 2^6 and converted to fp16 with
                  round-toward-zero: both are 8-bit numbers, exact while 2^-14 <= |64 t| <= 65504 (PRECONDITION |a| <= 1020,
                  now in the header); below, the fp16 subnormal spacing 2^-24 truncates each term by < 2^-30 of a: floor
                  2^-29 * sum |g|.  No relative term.
     tnb a_fmt 1  one fp16 x fp16 MFMA on exact operands: accumulation only.
     bslab / aslab  column sums of exact operands (v_dot2 of both terms with (1, 1)): accumulation only.
   A_bl of p2b is bit-exact BLS of the fp32 operand (split8: two round-to-nearest-even conversions, hi = bf16(x),
   lo = bf16(x - hi)) where that operand is reproducible -- without GroupNorm it is the loaded A.  With GroupNorm the compiler
   may contract (v - mean) * rstd * gamma + beta into fmas, so the fp32 operand is known to 5 * 2^-24 of its magnitude (four
   roundings, (1 + u)^4 - 1 <= 5 u) and A_bl is held to that + the header's 2^-17; A_bl16 = fp16(operand) likewise: bit-exact
   without GroupNorm, else within fp16's 2^-11 (+ 2^-25 where the result is an fp16 subnormal) of the perturbed operand --
   one fp16 ulp.  Padded slots and the slots steps[] cuts off are exact zeros in C, A_bl and A_bl16.
   a16_out of b2p is bit-exact fp16(hi + lo) of every stored cell, padded slots included (they relay what A holds).
   amax: max(before, lo) <= after <= max(before, hi) with [lo, hi] = [max(|ref| - bound), max(|ref| + bound)] over C.
   These constants are derived, not tuned.

3. CASES.  cases(entry) through gemm_contract's pairwise generator: every pair of values of P2B_DIMS / B2P_DIMS / TNB_DIMS /
   PACK_DIMS occurs in a valid case or is excluded by a named rule (invalid_pairs(entry)); the rules mirror the WS_REQUIREs.
   `targets` mirrors gemm_p2b_launch / ws_gemm_b2p / ws_gemm_tnb.  The WS_TNB_GDEPTH=2 variants are read once per process and
   are diagnostics: not covered.

BUFFERS.  As gemm_contract.build: GUARD floats on both sides of every allocation; outputs: write set NaN, everything else SENT
(ldc tails, rows of C no slot maps to, eight blocks behind the last block of every BL / BLH buffer, one slab behind nsplit);
inputs: everything the contract does not read is NaN (lda tails, unmapped rows, unused stat slots, the rows of the steps a
steps[] table cuts off, columns of G / A outside their range).  Padded slots of BL operands hold zeros; build(case, garbage=True)
puts large finite values into everything the kernels must select away instead."""
import os

import torch

from tests import gemm_contract as gc
from tests.gemm_contract import (GUARD, SENT, U, Buf, Built, Case, ContractViolation, Ref, assert_elementwise,  # noqa: F401
                                 check, draw, eps_for)

BIG = gc.BIG
NANBITS16 = 0x7E00          # a NaN in fp16 and in bf16
TAIL_BLOCKS = 8             # sentinel blocks behind the last block of a BL buffer: the grid rounds nblk up to 8 waves
GARBAGE = 3.0e30


# ------------------------------------------------------------------------------------------------------------
# formats and index formulas, from the header text
# ------------------------------------------------------------------------------------------------------------
def bls_decode(x):
    """BLS words (float32 storage) -> (hi + lo, |hi| + |lo|) in float64."""
    bits = x.contiguous().view(torch.int32)
    hi, lo = (bits & -65536).view(torch.float32).double(), (bits << 16).view(torch.float32).double()
    return hi + lo, hi.abs() + lo.abs()


def bls_encode(x):
    """fp32 -> BLS words: hi = bf16(x), lo = bf16(x - hi), both round to nearest even (split8 of gemm_blk.hip)."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    bits = (hi.view(torch.int16).to(torch.int32) << 16) | (lo.view(torch.int16).to(torch.int32) & 0xFFFF)
    return bits.view(torch.float32)


def h2(buf, dtype):
    """float32 storage -> its 2-byte elements."""
    return buf.contiguous().view(dtype)


def bl_index(nblk, C):
    """[nblk, 32, C] element offsets: (b, slot i, column c) at b*32*C + ((c >> 2)*32 + i)*4 + (c & 3)."""
    b = torch.arange(nblk).view(-1, 1, 1)
    i = torch.arange(32).view(1, -1, 1)
    c = torch.arange(C).view(1, 1, -1)
    return b * 32 * C + ((c >> 2) * 32 + i) * 4 + (c & 3)


def to_bl(x):
    """[nblk, 32, C] -> memory order of BL(C) (the index formula as a view: [nblk][C/4][32][4])."""
    n, _, C = x.shape
    return x.reshape(n, 32, C // 4, 4).permute(0, 2, 1, 3).reshape(-1)


def from_bl(buf, nblk, C):
    return buf.reshape(-1)[: nblk * 32 * C].reshape(nblk, C // 4, 32, 4).permute(0, 2, 1, 3).reshape(nblk, 32, C)


def positions(sm):
    """ws_seqmap: (pos [nblk, 32], valid [nblk, 32], seq [nblk, 32], step [nblk, 32]); padded slots carry the position of the
    last valid sequence (what the kernels clamp to: an address that exists)."""
    nt = -(-sm.nseq // 32)
    nv = sm.nvalid if sm.nvalid > 0 else sm.nseq
    seq = (torch.arange(nt).view(-1, 1, 1) * 32 + torch.arange(32).view(1, 1, -1)).expand(nt, sm.L, 32)
    step = torch.arange(sm.L).view(1, -1, 1).expand(nt, sm.L, 32)
    valid = seq < nv
    s = seq.clamp(max=nv - 1)
    pos = (s // sm.div) * sm.s1 + (s % sm.div) * sm.s2 + step * sm.step_rows
    n = nt * sm.L
    return pos.reshape(n, 32), valid.reshape(n, 32), s.reshape(n, 32), step.reshape(n, 32)


def dgates_scale(amax):
    from wesep_amd import _lib as L
    return L.dgates_scale(int(amax.reshape(-1)[0]))


def split_bf16(w):
    w = w.float()
    hi = w.to(torch.bfloat16).float()
    return hi, (w - hi).to(torch.bfloat16).float()


def split_f16(w):
    """(hi, remainder, lo) of 256 w in fp32: hi = fp16(256 w), remainder = 256 w - hi (exact), lo = fp16(remainder)."""
    s = 256.0 * w.float()
    hi = s.half().float()
    rem = s - hi
    return hi, rem, rem.half().float()


def frag_exponents(rem):
    """E [N/32, K/64] of ws_pack_w_f16f8: the largest |remainder| of a [32 n][64 k] fragment becomes a code in [128, 256)."""
    N, K = rem.shape
    mx = rem.abs().reshape(N // 32, 32, K // 64, 64).amax(dim=(1, 3))
    e = torch.floor(torch.log2(mx.double().clamp_min(1e-300))) - 7
    return torch.where(mx > 0, e, torch.zeros_like(e)).clamp_min(-126)


def logical_w(W, N, K, ldw, trans=False, w_off=0):
    """W'[n][k] = trans ? W[k*ldw + n] : W[n*ldw + k]."""
    n, k = torch.arange(N).view(-1, 1), torch.arange(K).view(1, -1)
    return W.reshape(-1)[w_off + (k * ldw + n if trans else n * ldw + k)]


# ------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------
def _units(x, N, K, order):
    """[N, K] -> [unit r, lane, j]: element j of unit (r, lane) = x[32 nt + (lane & 31)][16 ks + 8 (lane >> 5) + j];
    r = nt * (K/16) + ks (order 0, p2b) or ks * (N/32) + nt (order 1, b2p)."""
    v = x.reshape(N // 32, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).reshape(N // 32, K // 16, 64, 8)
    if order == 1:
        v = v.permute(1, 0, 2, 3)
    return v.reshape(-1, 64, 8)


def ref_pack_w(W, N, K, ldw, trans=False, order=0, w_off=0, f16=False):
    """The pack as int16 [N*K*2] (bf16 / fp16 bit patterns) -- bit-exact for f16 in (0, 1); for f16 = 2 a dict with the
    hi plane (int16 [K/64, 4, 4, 64, 8]), the remainders in fragment order and the exponents."""
    w = logical_w(W, N, K, ldw, trans, w_off).float()
    if int(f16) == 2:
        hi, rem, _ = split_f16(w)
        nst = K // 64
        # stage st: hi fragments [ks 4][nt 4][lane][j]; codes [nt][piece][lane][16 bytes], byte 8 i + j of a lane <-> k-step i
        def frag(x):
            return x.reshape(4, 32, nst, 4, 2, 8).permute(2, 3, 0, 4, 1, 5).reshape(nst, 4, 4, 64, 8)    # [st][i][nt][lane][j]
        E = frag_exponents(rem)                                                      # [nt, st]
        r = frag(rem).permute(0, 2, 3, 1, 4).reshape(nst, 4, 64, 2, 16).permute(0, 1, 3, 2, 4)    # [st][nt][piece][lane][16]
        return {"hi": frag(hi).half().view(torch.int16), "rem": r, "E": E.t().contiguous()}
    if f16:
        hi, _, lo = split_f16(w)
        parts = [t.half().view(torch.int16) for t in (hi, lo)]
    else:
        hi, lo = split_bf16(w)
        parts = [t.to(torch.bfloat16).view(torch.int16) for t in (hi, lo)]
    return torch.stack([_units(p, N, K, order) for p in parts], 1).reshape(-1)


def _zero_ref(n):
    z = torch.zeros(n, dtype=torch.float64)
    return z, z.clone(), z.clone()


def ref_gemm_p2b(*, A, lda, sm, W, N, K=128, bias=None, A_bl=None, stats=None, gamma=None, beta=None, stat_map=None,
                 run_if=None, amax=None, A_bl16=None, steps=None, steps_div=1, **_):
    """W: the logical W'[N][K] (None when N = 0).  Returns {"C", "A_bl", "A_bl16": Ref, "A_bl:bits" / "A_bl16:bits": the
    expected bit patterns where they are reproducible, "amax": (lo, hi)}; {} when run_if points at 0."""
    if run_if is not None and int(run_if.reshape(-1)[0]) == 0:
        return {}
    pos, valid, seq, step = positions(sm)
    if steps is not None:
        valid = valid & (step < steps.reshape(-1)[seq // steps_div].long())
    nblk = pos.shape[0]
    a32 = A.reshape(-1)[(pos * lda).unsqueeze(-1) + torch.arange(K)]
    a, mag, repro = a32.double(), a32.double().abs(), stats is None
    if stats is not None:
        d1, m1, d2, m2, base = [int(v) for v in stat_map]
        s = (pos // d1) * m1 + (pos % d2) * m2 + base
        st = stats.reshape(-1).double()
        mean, rstd = st[2 * s].unsqueeze(-1), st[2 * s + 1].unsqueeze(-1)
        gm, bt = gamma.reshape(-1)[:K].double(), beta.reshape(-1)[:K].double()
        a, mag = (a - mean) * rstd * gm + bt, (mag + mean.abs()) * rstd.abs() * gm.abs() + bt.abs()
    z = torch.zeros((), dtype=torch.float64)
    v3 = valid.unsqueeze(-1)
    a, mag = torch.where(v3, a, z), torch.where(v3, mag, z)
    out = {}
    pad = (~valid).unsqueeze(-1)
    if A_bl is not None or A_bl16 is not None:
        ex = pad.expand(nblk, 32, K)
        d = 5 * U * mag                                     # what is known of the fp32 operand behind the norm
        if A_bl is not None:
            if repro:
                bits = bls_encode(torch.where(v3, a32, torch.zeros(())))
                val = bls_decode(bits)[0]
                out["A_bl:bits"] = to_bl(bits).view(torch.int32)
                out["A_bl"] = Ref(torch.arange(val.numel()), to_bl(val), to_bl(mag), to_bl(torch.zeros_like(val)),
                                  torch.ones(val.numel(), dtype=torch.bool))
            else:
                out["A_bl"] = Ref(torch.arange(a.numel()), to_bl(a), to_bl(mag), to_bl(2.0 ** -17 * (a.abs() + d) + d), to_bl(ex))
        if A_bl16 is not None:
            if repro:
                h = torch.where(v3, a32, torch.zeros(())).half()
                out["A_bl16:bits"] = to_bl(h).view(torch.int16)
                val = h.double()
                out["A_bl16"] = Ref(torch.arange(val.numel()), to_bl(val), to_bl(mag), to_bl(torch.zeros_like(val)),
                                    torch.ones(val.numel(), dtype=torch.bool))
            else:
                out["A_bl16"] = Ref(torch.arange(a.numel()), to_bl(a), to_bl(mag),
                                    to_bl(2.0 ** -11 * (a.abs() + d) + d + 2.0 ** -25), to_bl(ex))
    if N:
        w = W.double()
        v, S = a @ w.t(), mag @ w.abs().t()
        if bias is not None:
            bv = bias.reshape(-1)[:N].double()
            v, S = v + bv, S + bv.abs()
        v, S = torch.where(v3, v, z), torch.where(v3, S, z)
        bound = eps_for(True, K) * S
        out["C"] = Ref(torch.arange(v.numel()), to_bl(v), to_bl(S), to_bl(bound), to_bl(pad.expand(nblk, 32, N)))
        if amax is not None:
            out["amax"] = (float((v.abs() - bound).max().clamp_min(0)), float((v.abs() + bound).max()))
    return out


def b2p_eps(a_fmt, K):
    return {0: 2.0 ** -16 + 2.0 ** -17, 1: 2.0 ** -17, 2: 2.0 ** -22, 3: 0.0}[a_fmt] + (K + 8) * U


def ref_gemm_b2p(*, A, K, sm, W, ldc, N=128, bias=None, R=None, a_fmt=0, amax=None, a16_out=None, drop_lo=False, **_):
    """W: the logical W'[128][K].  drop_lo: the reference of a kernel that forgot the lo term of the weights (host test)."""
    pos, valid, _, _ = positions(sm)
    nblk = pos.shape[0]
    out = {}
    Sc = 1.0
    if a_fmt == 0:
        a, mag = bls_decode(from_bl(A, nblk, K))
    elif a_fmt == 1:
        a = from_bl(h2(A, torch.bfloat16), nblk, K).double()
        mag = a.abs()
    else:
        Sc = dgates_scale(amax)
        a = from_bl(h2(A, torch.float16), nblk, K).double() / Sc
        mag = a.abs()
    w32 = W.float()
    floor = 0.0
    if a_fmt < 2:
        hi, lo = split_bf16(w32)
        wmag = hi.double().abs() + lo.double().abs()
        wd = hi.double() if drop_lo else w32.double()
    else:
        hi, rem, lo = split_f16(w32)
        wmag = (hi.double().abs() + rem.double().abs()) / 256.0
        wd = hi.double() / 256.0 if drop_lo else w32.double()
        if a_fmt == 2:
            floor = 2.0 ** -33 * mag.sum(-1, keepdim=True)
        else:
            E = frag_exponents(rem)                                          # [N/32, K/64]
            ef = torch.exp2(E - 10).repeat_interleave(32, 0).repeat_interleave(64, 1)
            mx = torch.exp2(E + 8).repeat_interleave(32, 0).repeat_interleave(64, 1)
            As, r = mag * Sc, rem.double().abs()
            dr, da = 2.0 ** -4 * r + ef, 2.0 ** -4 * As
            floor = (As @ dr.t() + da @ r.t() + 0.25 * mx.sum(1) + da @ dr.t() + 0.25 * dr.sum(1)) / (256.0 * Sc)
    v, S = a @ wd.t(), mag @ wmag.t()
    if bias is not None:
        bv = bias.reshape(-1)[:N].double()
        v, S = v + bv, S + bv.abs()
    bound = b2p_eps(a_fmt, K) * S + floor
    vm = valid.reshape(-1)
    cidx = (pos.reshape(-1)[vm] * ldc).unsqueeze(1) + torch.arange(N).unsqueeze(0)
    v, S, bound = v.reshape(-1, N)[vm], S.reshape(-1, N)[vm], bound.reshape(-1, N)[vm]
    if R is not None:
        r = R.reshape(-1)[cidx].double()
        v, bound = v + r, bound + U * r.abs()
    out["C"] = Ref(cidx.reshape(-1), v.reshape(-1), S.reshape(-1), bound.reshape(-1), torch.zeros(cidx.numel(), dtype=torch.bool))
    if a16_out is not None:
        cells = A.reshape(-1)[: nblk * 32 * K]
        h = bls_decode(cells)[0].float().half()              # hi + lo is an fp32 number; one rounding to fp16
        out["a16_out:bits"] = h.view(torch.int16)
        out["a16_out"] = Ref(torch.arange(h.numel()), h.double(), h.double().abs(), torch.zeros(h.numel(), dtype=torch.float64),
                             torch.ones(h.numel(), dtype=torch.bool))
    return out


def tnb_kernel(g_fmt, a_fmt, ta, aslab, f16env):
    """The instantiation ws_gemm_tnb picks (WS_TNB_GDEPTH unset: depth 4)."""
    if a_fmt == 1:
        return "gemm_tnb16_kernel<false,3,4,1>"
    a = "true" if aslab else "false"
    if g_fmt == 2:
        return f"gemm_tnb16_kernel<{a},{3 if f16env != '0' else 2},4>"
    if g_fmt == 1:
        return f"gemm_tnb16_kernel<{a},1,4>"
    if ta == 3:
        return f"gemm_tnb_kernel<3,{a}>"
    return "gemm_tnb_kernel<1,true>"


def tnb_eps(kernel):
    """(relative eps of the product, floor factor on sum |g|)."""
    if kernel.startswith("gemm_tnb_kernel") or kernel in ("gemm_tnb16_kernel<true,2,4>", "gemm_tnb16_kernel<false,2,4>"):
        return 2.0 ** -16, 0.0
    if kernel in ("gemm_tnb16_kernel<true,3,4>", "gemm_tnb16_kernel<false,3,4>"):
        return 0.0, 2.0 ** -29
    return 0.0, 0.0


def ref_gemm_tnb(*, G, g_width, g_off, g_cols, A0, a0_width, a0_off, a0_cols, nblk, L_, nsplit, blocks_per_split, a0_shift=0,
                 A1=None, a1_width=0, a1_off=0, a1_cols=0, a1_shift=0, bslab=None, aslab=None, g_fmt=0, amax=None, a_fmt=0,
                 f16env="unset", drop_lo=False, defect=None, **_):
    """drop_lo / defect: the output of a kernel with a planted defect (host test): "unmasked" = the shifted operand read
    unshifted instead of zeroed at a tile's end, "neighbour" = the shift crossing into the next tile's block, "split" = the
    boundary between the first two splits one block late."""
    def dec(buf, width, two_byte, scale=1.0):
        if two_byte is None:
            v, m = bls_decode(from_bl(buf, nblk, width))
            if drop_lo:
                v = (from_bl(buf, nblk, width).contiguous().view(torch.int32) & -65536).view(torch.float32).double()
            return v, m
        v = from_bl(h2(buf, two_byte), nblk, width).double() / scale
        return v, v.abs()

    def shifted(x, shift):                       # Acat(b) = A(b + shift) inside the tile, zero outside [0, L)
        if shift == 0:
            return x
        st = torch.arange(nblk) % L_ + shift
        ok = (st >= 0) & (st < L_)
        if defect == "neighbour":
            ok = (torch.arange(nblk) + shift >= 0) & (torch.arange(nblk) + shift < nblk)
        src = torch.where(ok, torch.arange(nblk) + shift, torch.arange(nblk))
        if defect == "unmasked":
            return x[src]
        return torch.where(ok.view(-1, 1, 1), x[src], torch.zeros((), dtype=torch.float64))
    Sc = dgates_scale(amax) if g_fmt == 2 else 1.0
    g, gm = dec(G, g_width, {0: None, 1: torch.bfloat16, 2: torch.float16}[g_fmt], Sc)
    g, gm = g[:, :, g_off:g_off + g_cols], gm[:, :, g_off:g_off + g_cols]
    parts = [(A0, a0_width, a0_off, a0_cols, a0_shift)] + ([(A1, a1_width, a1_off, a1_cols, a1_shift)] if a1_cols else [])
    av, am = [], []
    for buf, width, off, cols, shift in parts:
        v, m = dec(buf, width, torch.float16 if a_fmt else None)
        av.append(shifted(v[:, :, off:off + cols], shift))
        am.append(shifted(m[:, :, off:off + cols], shift))
    a, amg = torch.cat(av, 2), torch.cat(am, 2)
    acols = a.shape[2]
    epsr, fl = tnb_eps(tnb_kernel(g_fmt, a_fmt, acols // 128, aslab is not None, f16env))
    res = {k: [] for k in ("slab", "bslab", "aslab")}
    for sp in range(nsplit):
        lo, hi = sp * blocks_per_split, min(nblk, (sp + 1) * blocks_per_split)
        if defect == "split":
            lo, hi = lo + (sp == 1), min(nblk, hi + (sp == 0))
        n = max(hi - lo, 0) * 32
        if n:
            gs, gms = g[lo:hi].reshape(n, g_cols), gm[lo:hi].reshape(n, g_cols)
            as_, ams = a[lo:hi].reshape(n, acols), amg[lo:hi].reshape(n, acols)
            v, S = gs.t() @ as_, gms.t() @ ams
            bnd = (epsr + (n + 8) * U) * S + fl * gms.sum(0).unsqueeze(1)
            res["slab"].append((v.reshape(-1), S.reshape(-1), bnd.reshape(-1)))
            res["bslab"].append((gs.sum(0), gms.sum(0), (n + 8) * U * gms.sum(0)))
            res["aslab"].append((as_.sum(0), ams.sum(0), (n + 8) * U * ams.sum(0)))
        else:
            res["slab"].append(_zero_ref(g_cols * acols))
            res["bslab"].append(_zero_ref(g_cols))
            res["aslab"].append(_zero_ref(acols))
    out = {}
    for key, on, cnt in (("slab", True, g_cols * acols), ("bslab", bslab is not None, g_cols), ("aslab", aslab is not None, acols)):
        if on:
            v, S, b = [torch.cat([r[i] for r in res[key]]) for i in range(3)]
            out[key] = Ref(torch.arange(nsplit * cnt), v, S, b, torch.zeros(nsplit * cnt, dtype=torch.bool))
    return out


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, targets
# ------------------------------------------------------------------------------------------------------------
SEQ_DIMS = {"nseq": [1, 31, 32, 33, 63, 64, 65, 100], "L": [1, 2, 3, 7, 37],
            "map": ["time", "band", "gaps1", "gaps3"],           # sq_div: BIG, one that does not divide nseq, 1, 3
            "nvalid": ["0", "n-1", "n-31", "1"]}
P2B_DIMS = {**SEQ_DIMS, "N": [0, 64, 128, 192, 1024, 2048], "lda": [128, 132, 160], "norm": ["off", "time", "band"],
            "bias": [0, 1], "A_bl": [0, 1], "A_bl16": [0, 1], "amax": ["none", "zero", "above"], "run_if": ["none", 0, 1],
            "steps": ["none", "all", "mixed"], "steps_div": [1, "bands"]}
B2P_DIMS = {**SEQ_DIMS, "K": [64, 128, 512, 1024, 2048], "a_fmt": [0, 1, 2, 3], "bias": [0, 1], "R": ["off", "sep", "alias"],
            "ldc": [128, 132, 256], "a16_out": [0, 1], "trans": [0, 1], "headroom": ["top", "mid", "low"]}
TNB_DIMS = {"g_fmt": [0, 1, 2], "a_fmt": [0, 1], "f16env": ["unset", "0"], "ta": [1, 3], "aslab": [0, 1], "bslab": [0, 1],
            "g_geom": [(128, 0, 128), (512, 256, 256), (2048, 1024, 1024)], "a0": [(128, 0), (256, 128)],
            "a1": [(512, 0), (512, 256)], "a1_shift": [0, 1, -1, 3, -3], "ntile": [1, 2, 4], "L": [1, 2, 3, 7, 37],
            "split": ["one", "exact", "partial", "empty", "auto"]}
PACK_DIMS = {"kind": ["bf16", "f16", "f16f8"], "N": [32, 64, 128, 192, 1024], "K": [16, 64, 128, 2048], "ldw": ["=", "+4"],
             "trans": [0, 1], "order": [0, 1], "w_off": [0, 12]}

_SEQ_RULES = [
    ("nvalid names a proper prefix: nvalid = nseq - 1 needs nseq >= 2", ("nvalid", "nseq"), lambda nv, n: nv == "n-1" and n < 2),
    ("nvalid names a proper prefix: nvalid = nseq - 31 needs nseq >= 32", ("nvalid", "nseq"), lambda nv, n: nv == "n-31" and n < 32),
    ("nvalid names a proper prefix: nvalid = 1 needs nseq >= 2", ("nvalid", "nseq"), lambda nv, n: nv == "1" and n < 2),
]
P2B_RULES = _SEQ_RULES + [
    ("N = 0 relays the operand: it needs A_bl or A_bl16 (null pointer)", ("N", "A_bl", "A_bl16"),
     lambda N, a, b: N == 0 and not a and not b),
    ("N = 0 has no C: no bias", ("N", "bias"), lambda N, b: N == 0 and b),
    ("N = 0 has no C: amax is not touched", ("N", "amax"), lambda N, a: N == 0 and a != "none"),
    ("steps_div exists only with a steps table", ("steps", "steps_div"), lambda s, d: s == "none" and d != 1),
]
B2P_RULES = _SEQ_RULES + [
    ("a16_out goes with a_fmt 0", ("a16_out", "a_fmt"), lambda o, f: o and f != 0),
]
TNB_RULES = [
    ("g_fmt 1 / 2 (2-byte G) are built for 384 A columns", ("g_fmt", "ta"), lambda g, ta: g != 0 and ta != 3),
    ("a_fmt = 1 is built for g_fmt = 2", ("a_fmt", "g_fmt"), lambda a, g: a == 1 and g != 2),
    ("a_fmt = 1 is built for 384 A columns", ("a_fmt", "ta"), lambda a, ta: a == 1 and ta != 3),
    ("a_fmt = 1 has no aslab", ("a_fmt", "aslab"), lambda a, s: a == 1 and s),
    ("WS_TNB_F16 chooses among the g_fmt 2 kernels only", ("f16env", "g_fmt"), lambda e, g: e == "0" and g != 2),
    ("WS_TNB_F16 is not read with a_fmt = 1", ("f16env", "a_fmt"), lambda e, a: e == "0" and a == 1),
    ("128 A columns leave no A1: nothing to shift", ("ta", "a1_shift"), lambda ta, s: ta == 1 and s != 0),
]
PACK_RULES = [
    ("ws_pack_w_f16f8: N = 128", ("kind", "N"), lambda k, N: k == "f16f8" and N != 128),
    ("ws_pack_w_f16f8: K % 64", ("kind", "K"), lambda k, K: k == "f16f8" and K % 64 != 0),
    ("the fp16 + FP8 pack exists in the b2p order only", ("kind", "order"), lambda k, o: k == "f16f8" and o != 1),
]

P2B_INST = ["gemm_p2b_kernel<false>", "gemm_p2b_kernel<true>"]
B2P_INST = [f"gemm_b2p_kernel<{i}>" for i in range(4)]
TNB_INST = ["gemm_tnb_kernel<1,true>", "gemm_tnb_kernel<3,true>", "gemm_tnb_kernel<3,false>"] + [
    f"gemm_tnb16_kernel<{a},{g},4>" for a in ("true", "false") for g in (1, 2, 3)] + ["gemm_tnb16_kernel<false,3,4,1>"]
PACK_INST = ["pack_w_kernel", "pack_w16_kernel", "pack_w16f8_kernel"]
ENTRIES = ("pack_w", "gemm_p2b", "gemm_b2p", "gemm_tnb")
INST = {"pack_w": PACK_INST, "gemm_p2b": P2B_INST, "gemm_b2p": B2P_INST, "gemm_tnb": TNB_INST}


def _tnb_fixed(kernel):
    for g in (0, 1, 2):
        for a in (0, 1):
            for ta in (1, 3):
                for s in (0, 1):
                    for e in ("unset", "0"):
                        f = {"g_fmt": g, "a_fmt": a, "ta": ta, "aslab": s, "f16env": e}
                        if gc.violated("gemm_tnb", f) is None and tnb_kernel(g, a, ta, s, e) == kernel:
                            return f
    raise AssertionError(kernel)


def _targets(entry, d, seed):
    if entry == "gemm_p2b":
        return (P2B_INST[d["steps"] != "none"],)
    if entry == "gemm_b2p":
        return (B2P_INST[d["a_fmt"]],)
    if entry == "gemm_tnb":
        return (tnb_kernel(d["g_fmt"], d["a_fmt"], d["ta"], d["aslab"], d["f16env"]),)
    return (PACK_INST[("bf16", "f16", "f16f8").index(d["kind"])],)


gc.DIMS.update({"pack_w": PACK_DIMS, "gemm_p2b": P2B_DIMS, "gemm_b2p": B2P_DIMS, "gemm_tnb": TNB_DIMS})
gc.RULES.update({"pack_w": PACK_RULES, "gemm_p2b": P2B_RULES, "gemm_b2p": B2P_RULES, "gemm_tnb": TNB_RULES})
gc.SEEDS.update({"pack_w": 11, "gemm_p2b": 12, "gemm_b2p": 13, "gemm_tnb": 14})
gc.INST.update(INST)
for _e in ENTRIES:
    gc.PLANNERS[_e] = (lambda e: lambda d, seed: _targets(e, d, seed))(_e)
gc.TOPUP.update({
    "pack_w": [({"kind": k}, t, gc.MIN_PER_TARGET) for k, t in zip(("bf16", "f16", "f16f8"), PACK_INST)],
    "gemm_p2b": [({"steps": "none"}, P2B_INST[0], gc.MIN_PER_TARGET), ({"steps": "mixed"}, P2B_INST[1], gc.MIN_PER_TARGET)],
    "gemm_b2p": [({"a_fmt": i}, B2P_INST[i], gc.MIN_PER_TARGET) for i in range(4)],
    "gemm_tnb": [(_tnb_fixed(k), k, gc.MIN_PER_TARGET) for k in TNB_INST],
})


def cases(entry):
    return gc.cases(entry)


def invalid_pairs(entry):
    return gc.invalid_pairs(entry)


# ------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------
def seq_map(kind, nseq, L, nvalid):
    """(SeqMap, P): the map shapes of the sweep and the rows of the plain tensor they address."""
    from wesep_amd.dev import SeqMap
    nv = {"0": 0, "n-1": nseq - 1, "n-31": nseq - 31, "1": 1}[nvalid]
    if kind == "time":          # functional._view_maps("time"): sequence (r, k), steps over t
        sm = SeqMap(nseq, BIG, 0, L, 1, L, nv)
    elif kind == "band":        # functional._view_maps("band"): sequence (r, t), steps over k; Tf does not divide nseq
        Tf = next(t for t in (5, 7, 3) if nseq % t)
        sm = SeqMap(nseq, Tf, L * Tf, 1, Tf, L, nv)
    elif kind == "gaps1":       # sq_div = 1, every other row unmapped, two rows between sequences
        sm = SeqMap(nseq, 1, 2 * L + 2, 0, 2, L, nv)
    else:                       # sq_div = 3 (33, 64, 65, 100, 31, 32, 1 are no multiples), a hole row per step, two per group
        sm = SeqMap(nseq, 3, 4 * L + 2, 1, 4, L, nv)
    pos, valid, _, _ = positions(sm)
    return sm, int(pos[valid].max()) + 1


def _alloc_bl(nblk, C, fill, two_byte=False):
    """A BL(C) / BLH(C) output: the blocks are the write set, TAIL_BLOCKS more blocks and the guards hold SENT."""
    per = 32 * C // (2 if two_byte else 1)
    t = gc.alloc((nblk + TAIL_BLOCKS) * per, SENT)
    w = t[GUARD:GUARD + nblk * per]
    if two_byte:
        w.view(torch.int16).fill_(NANBITS16)
    else:
        w.fill_(float("nan"))
    return t, Buf("", GUARD, GUARD + (nblk + TAIL_BLOCKS) * per)


def _word(value):
    """A guarded int32 word: 33 words, the one in the middle is the argument."""
    t = torch.full((33,), 0x5A5A5A5A, dtype=torch.int32)
    t[16] = value
    return t


def _fbits(x):
    return int(torch.tensor(float(x), dtype=torch.float32).view(torch.int32))


def _weights(b, g, N, K, trans, kind, order, ldw_extra=0, w_off=0, scale=0.1):
    """The weight matrix (buffer "W"), its logical view (b.W) and an empty pack buffer "Wpack"."""
    rows, cols = (K, N) if trans else (N, K)
    ldw = cols + ldw_extra
    if kind:                    # fp16 of 256 w: |w| < 255 (header); the draw's rows x1e3 reach 5e3 * scale
        scale = min(scale, 0.01)
    Wb = gc.alloc(w_off + rows * ldw, float("nan"))
    m = Wb[GUARD + w_off:GUARD + w_off + rows * ldw].view(rows, ldw)
    w = draw(g, N, K) * scale
    m[:, :cols] = w.t() if trans else w
    b.bufs["W"] = Wb
    b.bufs["Wpack"] = gc.alloc(N * K + (4 * (K // 64) if kind == 2 else 0), SENT)
    b.pack = dict(W=Buf("W", GUARD, Wb.numel()), N=N, K=K, ldw=ldw, out=Buf("Wpack", GUARD, b.bufs["Wpack"].numel() - GUARD),
                  trans=bool(trans), order=order, w_off=w_off, f16=kind)
    b.W = w


def _scaled_f16(x, headroom):
    """fp16(x * S) and the amax word that defines S: values first, then amax, so every stored value is finite."""
    from wesep_amd import _lib as L
    m = float(x.abs().max()) or 1.0
    am = {"top": m * 2.0 ** -6.5, "mid": m, "low": m * 2.0 ** 12}[headroom]      # max |x| S in [2^14, 2^15.5), [2^8, 2^9), [2^-4, 2^-3)
    bits = _fbits(am)
    return (x * L.dgates_scale(bits)).half(), bits


def _p2b_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    b = Built(case)
    b.kinds = {}
    sm, P = seq_map(d["map"], d["nseq"], d["L"], d["nvalid"])
    pos, valid, seq, step = positions(sm)
    nblk, N, K, lda = pos.shape[0], d["N"], 128, d["lda"]
    nv = sm.nvalid or sm.nseq
    fill = GARBAGE if garbage else float("nan")
    kw = dict(lda=lda, sm=sm, N=N, K=K)
    if d["steps"] != "none":
        sdiv = 1 if d["steps_div"] == 1 else 5
        n = -(-nv // sdiv)
        tab = torch.full((n,), d["L"], dtype=torch.int32)
        if d["steps"] == "mixed":
            tab = ((torch.arange(n) * 7) % d["L"] + 1).to(torch.int32)
            tab[0], tab[-1] = 1, d["L"]
        b.bufs["steps"] = tab
        kw.update(steps=Buf("steps"), steps_div=sdiv)
        live = valid & (step < tab[seq // sdiv].long())
    else:
        live = valid
    Ab = gc.alloc(P * lda, fill)
    rows = pos[live]
    # (with A_bl16 the operand has to fit fp16: |a| <= 500 or so, |gamma| <= 4, rstd <= 2)
    Ab[GUARD:GUARD + P * lda].view(P, lda)[rows, :K] = draw(g, rows.numel(), K) * (0.1 if d["A_bl16"] else 1.0)
    b.bufs["A"] = Ab
    kw["A"] = Buf("A", GUARD, GUARD + P * lda)
    if N:
        _weights(b, g, N, K, False, 0, 0)
        kw["Wpack"] = Buf("Wpack", GUARD, GUARD + N * K)
        Cb, sl = _alloc_bl(nblk, N, None)
        b.bufs["C"], kw["C_out"] = Cb, sl._replace(name="C")
        b.out_keys["C"], b.kinds["C"] = "C", "f32"
    else:
        kw.update(Wpack=None, C_out=None)
        b.pack, b.W = None, None
    pieces = gc.alloc(N + 2 * K + 64, float("nan"))
    o_bias, o_gm, o_bt = GUARD, GUARD + (N + 19) // 4 * 4, GUARD + (N + 19) // 4 * 4 + K + 16
    pieces[o_bias:o_bias + N] = draw(g, 1, max(N, 1)).reshape(-1)[:N]
    pieces[o_gm:o_gm + K], pieces[o_bt:o_bt + K] = draw(g, 1, K).reshape(-1).clamp(-4, 4), draw(g, 1, K).reshape(-1)
    b.bufs["P"] = pieces
    if d["bias"]:
        kw["bias"] = Buf("P", o_bias, o_bias + N)
    if d["norm"] != "off":
        from wesep_amd.dev import StatMap
        smap = StatMap(7, 1, 1, 0, 2) if d["norm"] == "time" else StatMap(11, 3, 3, 1, 2)      # pos // 7;  (pos // 11) * 3 + pos % 3
        allpos = torch.arange(P)
        s_all = (allpos // smap[0]) * smap[1] + (allpos % smap[2]) * smap[3] + smap[4]
        St = gc.alloc(2 * (int(s_all.max()) + 1), fill)
        s = s_all[rows]
        St[GUARD + 2 * s] = torch.randn(s.numel(), generator=g)
        St[GUARD + 2 * s + 1] = 0.5 + 1.5 * torch.rand(s.numel(), generator=g)
        b.bufs["stats"] = St
        kw.update(stats=Buf("stats", GUARD, St.numel() - GUARD), stat_map=smap, gamma=Buf("P", o_gm, o_gm + K),
                  beta=Buf("P", o_bt, o_bt + K))
    if d["A_bl"]:
        t, sl = _alloc_bl(nblk, K, None)
        b.bufs["A_bl"], kw["A_bl"] = t, sl._replace(name="A_bl")
        b.out_keys["A_bl"], b.kinds["A_bl"] = "A_bl", "bls"
    if d["A_bl16"]:
        t, sl = _alloc_bl(nblk, K, None, two_byte=True)
        b.bufs["A_bl16"], kw["A_bl16"] = t, sl._replace(name="A_bl16")
        b.out_keys["A_bl16"], b.kinds["A_bl16"] = "A_bl16", torch.float16
    if d["amax"] != "none":
        b.bufs["amax"] = _word(0 if d["amax"] == "zero" else _fbits(1e30))
        kw["amax"] = Buf("amax", 16, 17)
        b.out_keys["amax"], b.kinds["amax"] = "amax", "amax"
    if d["run_if"] != "none":
        b.bufs["run_if"] = _word(d["run_if"])
        kw["run_if"] = Buf("run_if", 16, 17)
    b.kw, b.outs = kw, list(b.out_keys.values())
    return b


def _blocked_operand(g, nblk, width, fmt, lo, hi, headroom="mid", scale=1.0, valid=None, garbage=False):
    """A BL / BLH operand: columns [lo, hi) hold drawn values (fmt: "bls" | "bf16" | "f16" | "f16s" = scaled fp16), everything
    else NaN; padded slots (valid False) hold zeros, or GARBAGE.  Returns (allocation, amax bits or None)."""
    x = draw(g, nblk * 32, hi - lo).view(nblk, 32, hi - lo) * scale
    junk = None
    if valid is not None:
        x = torch.where(valid.unsqueeze(-1), x, torch.zeros(()))
        junk = (~valid).unsqueeze(-1).expand_as(x) if garbage else None
    bits = None
    if fmt == "bls":
        full = torch.full((nblk, 32, width), float("nan"))
        full[:, :, lo:hi] = bls_encode(torch.where(junk, torch.full((), 1.0e4), x) if junk is not None else x)
        t = gc.alloc(nblk * 32 * width, float("nan"))
        t[GUARD:GUARD + nblk * 32 * width] = to_bl(full)
        return t, bits
    if fmt == "f16s":
        x, bits = _scaled_f16(x, headroom)
    full = torch.full((nblk, 32, width), NANBITS16, dtype=torch.int16)
    if junk is not None:       # (after the scale was chosen: the stored garbage is finite whatever S is)
        x = torch.where(junk, torch.full((), 1.0e4, dtype=x.dtype), x)
    full[:, :, lo:hi] = (x.to(torch.bfloat16) if fmt == "bf16" else x.half()).view(torch.int16)
    t = gc.alloc(nblk * 32 * width // 2, float("nan"))
    t[GUARD:GUARD + nblk * 32 * width // 2] = to_bl(full).view(torch.float32)
    return t, bits


def _b2p_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    b = Built(case)
    b.kinds = {}
    sm, P = seq_map(d["map"], d["nseq"], d["L"], d["nvalid"])
    pos, valid, _, _ = positions(sm)
    nblk, N, K, ldc, fmt = pos.shape[0], 128, d["K"], d["ldc"], d["a_fmt"]
    Ab, bits = _blocked_operand(g, nblk, K, ("bls", "bf16", "f16s", "f16s")[fmt], 0, K, d["headroom"], valid=valid, garbage=garbage)
    b.bufs["A"] = Ab
    kw = dict(A=Buf("A", GUARD, Ab.numel() - GUARD), K=K, sm=sm, ldc=ldc, N=N, a_fmt=fmt)
    if bits is not None:
        b.bufs["amax"] = _word(bits)
        kw["amax"] = Buf("amax", 16, 17)
    _weights(b, g, N, K, d["trans"], (0, 0, 1, 2)[fmt], 1, ldw_extra=4 * (case.seed % 2), w_off=12 * (case.seed // 2 % 2))
    kw["Wpack"] = Buf("Wpack", GUARD, b.bufs["Wpack"].numel() - GUARD)
    Cb = gc.alloc(P * ldc, SENT)
    rows = pos[valid]
    cidx = GUARD + (rows * ldc).unsqueeze(1) + torch.arange(N).unsqueeze(0)
    Cb[cidx] = float("nan")
    pieces = gc.alloc(N, float("nan"))
    pieces[GUARD:GUARD + N] = draw(g, 1, N).reshape(-1)
    b.bufs["P"] = pieces
    if d["bias"]:
        kw["bias"] = Buf("P", GUARD, GUARD + N)
    if d["R"] != "off":
        rv = draw(g, rows.numel(), N)
        if d["R"] == "alias":
            Cb[cidx] = rv
            kw["R"] = Buf("C", GUARD, GUARD + P * ldc)
        else:
            Rb = gc.alloc(P * ldc, GARBAGE if garbage else float("nan"))
            Rb[cidx] = rv
            b.bufs["R"] = Rb
            kw["R"] = Buf("R", GUARD, GUARD + P * ldc)
    b.bufs["C"] = Cb
    kw["C_out"] = Buf("C", GUARD, GUARD + P * ldc)
    b.out_keys["C"], b.kinds["C"] = "C", "f32"
    if d["a16_out"]:
        t, sl = _alloc_bl(nblk, K, None, two_byte=True)
        b.bufs["a16_out"], kw["a16_out"] = t, sl._replace(name="a16_out")
        b.out_keys["a16_out"], b.kinds["a16_out"] = "a16_out", torch.float16
    b.kw, b.outs = kw, list(b.out_keys.values())
    return b


def tnb_split(kind, nblk, gtiles):
    if kind == "auto":
        from wesep_amd import dev
        return dev.tnb_splits(nblk, gtiles)
    return gc.tn_split(kind, nblk)


def _tnb_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    b = Built(case)
    b.kinds = {}
    nblk, L_ = d["ntile"] * d["L"], d["L"]
    gw, goff, gcols = d["g_geom"]
    gfmt, afmt = d["g_fmt"], d["a_fmt"]
    f16path = gfmt == 2 and afmt == 0 and d["f16env"] != "0"
    Gb, bits = _blocked_operand(g, nblk, gw, ("bls", "bf16", "f16s")[gfmt], goff, goff + gcols, ("mid", "top")[case.seed % 2])
    b.bufs["G"] = Gb
    a_kind = "f16" if afmt else "bls"
    a_scale = 0.1 if (f16path or afmt) else 1.0         # the fp16 instruction's precondition |a| < 1023 (header)
    a0w, a0off = d["a0"]
    b.bufs["A0"], _ = _blocked_operand(g, nblk, a0w, a_kind, a0off, a0off + 128, scale=a_scale)
    kw = dict(G=Buf("G", GUARD, Gb.numel() - GUARD), g_width=gw, g_off=goff, g_cols=gcols,
              A0=Buf("A0", GUARD, b.bufs["A0"].numel() - GUARD), a0_width=a0w, a0_off=a0off, a0_cols=128, nblk=nblk, L_=L_,
              g_fmt=gfmt, a_fmt=afmt)
    acols = 128
    if d["ta"] == 3:
        a1w, a1off = d["a1"]
        b.bufs["A1"], _ = _blocked_operand(g, nblk, a1w, a_kind, a1off, a1off + 256, scale=a_scale)
        kw.update(A1=Buf("A1", GUARD, b.bufs["A1"].numel() - GUARD), a1_width=a1w, a1_off=a1off, a1_cols=256,
                  a1_shift=d["a1_shift"])
        acols = 384
    if bits is not None:
        b.bufs["amax"] = _word(bits)
        kw["amax"] = Buf("amax", 16, 17)
    nsplit, bps = tnb_split(d["split"], nblk, gcols // 128)
    kw.update(nsplit=nsplit, blocks_per_split=bps)
    for key, on, cnt in (("slab", True, gcols * acols), ("bslab", d["bslab"], gcols), ("aslab", d["aslab"], acols)):
        if on:
            t = gc.alloc((nsplit + 1) * cnt, SENT)          # one more slab behind nsplit: sentinel
            t[GUARD:GUARD + nsplit * cnt] = float("nan")
            b.bufs[key] = t
            kw[key] = Buf(key, GUARD, t.numel() - GUARD)
            b.out_keys[key], b.kinds[key] = key, "f32"
    b.blocks = [(0, gcols * acols, 0, gcols)]
    b.env = {"WS_TNB_F16": "0"} if d["f16env"] == "0" else {}
    b.f16env = d["f16env"]
    b.kw, b.outs = kw, list(b.out_keys.values())
    return b


def _pack_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    b = Built(case)
    kind = ("bf16", "f16", "f16f8").index(d["kind"])
    scale = (0.1, 3.0e-3, 1.0)[case.seed % 3] * (1.0e-2 if kind else 1.0)
    _weights(b, g, d["N"], d["K"], d["trans"], kind, d["order"], ldw_extra=4 if d["ldw"] == "+4" else 0, w_off=d["w_off"],
             scale=scale)
    n = (d["K"] // 64) * 6145 if kind == 2 else d["N"] * d["K"]    # (f16f8: 24 KB per stage + one dword of E8M0 bytes per stage)
    b.bufs["Wpack"][GUARD:GUARD + n] = float("nan")
    b.kw = dict(b.pack)
    b.out_keys, b.outs, b.kinds = {"pack": "Wpack"}, ["Wpack"], {"Wpack": "pack"}
    return b


_BUILD = {"pack_w": _pack_build, "gemm_p2b": _p2b_build, "gemm_b2p": _b2p_build, "gemm_tnb": _tnb_build}


def build(case, garbage=False):
    b = _BUILD[case.entry](case, garbage)
    for attr, v in (("pack", None), ("W", None), ("env", {}), ("f16env", "unset")):
        if not hasattr(b, attr):
            setattr(b, attr, v)
    return b


def reference(b, tensors=None):
    t = tensors or b.bufs
    kw = b.kwargs(t, "cpu")
    e = b.case.entry
    if e == "pack_w":
        return {"pack": ref_pack_w(**{k: v for k, v in kw.items() if k != "out"})}
    if e == "gemm_p2b":
        return ref_gemm_p2b(W=b.W, **kw)
    if e == "gemm_b2p":
        return ref_gemm_b2p(W=b.W, **kw)
    return ref_gemm_tnb(f16env=b.f16env, **kw)


def run(mod, b, tensors, device="cpu"):
    """The case's calls on the namespace `mod` (wesep_amd.dev, or an emulation of it): the weight pack, then the entry."""
    old = {k: os.environ.get(k) for k in b.env}
    os.environ.update(b.env)
    try:
        if b.pack is not None:
            pk = {k: (tensors[v.name][v.lo:v.hi] if isinstance(v, Buf) else v) for k, v in b.pack.items()}
            mod.pack_w(pk.pop("W"), pk.pop("N"), pk.pop("K"), pk.pop("ldw"), pk.pop("out"), **pk)
        if b.case.entry != "pack_w":
            getattr(mod, b.case.entry)(**b.kwargs(tensors, device))
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ------------------------------------------------------------------------------------------------------------
# checker
# ------------------------------------------------------------------------------------------------------------
def _same(a, b, what, kind="sentinel"):
    a, b = a.contiguous().view(torch.int32).reshape(-1), b.contiguous().view(torch.int32).reshape(-1)
    if not torch.equal(a, b):
        j = int((a != b).nonzero()[0])
        raise ContractViolation(kind, f"{what}: word {j} changed ({int(b[j]):#x} -> {int(a[j]):#x})")


def _check_pack(out, before, ref, kw, what):
    N, K, kind = kw["N"], kw["K"], int(kw["f16"])
    o = out[GUARD:]
    if kind != 2:
        got = o[: N * K].view(torch.int16)
        if not torch.equal(got, ref):
            j = int((got != ref).nonzero()[0])
            raise ContractViolation("exact", f"{what}: 2-byte element {j} is {int(got[j]) & 0xFFFF:#06x}, the unit formula "
                                             f"says {int(ref[j]) & 0xFFFF:#06x}")
        n = N * K
        worst = 0.0
    else:
        nst = K // 64
        by = o[: nst * 6144 + nst].contiguous().view(torch.uint8)
        st = by[: nst * 24576].reshape(nst, 24576)
        hi = st[:, :16384].contiguous().view(torch.int16).reshape(nst, 4, 4, 64, 8)
        if not torch.equal(hi, ref["hi"]):
            raise ContractViolation("exact", f"{what}: the hi plane is not fp16(256 w) in the fragment order")
        E = by[nst * 24576: nst * 24576 + 4 * nst].reshape(nst, 4).double() - 127
        if not torch.equal(E, ref["E"]):
            raise ContractViolation("exact", f"{what}: fragment exponents {E.tolist()} != {ref['E'].tolist()}")
        codes = st[:, 16384:].contiguous().view(torch.float8_e4m3fn).float().double().reshape(nst, 4, 2, 64, 16)
        if not bool(torch.isfinite(codes).all()):
            raise ContractViolation("nan", f"{what}: a code is NaN")
        sc = torch.exp2(E).view(nst, 4, 1, 1, 1)
        r = ref["rem"].double()
        x = r.abs() / sc                                   # |remainder| in code units: < 256
        ulp = torch.exp2(torch.floor(torch.log2(x.clamp_min(2.0 ** -6))) - 3)          # e4m3: 3 mantissa bits, subnormals below 2^-6
        err, bound = (codes * sc - r).abs(), 0.5 * ulp * sc
        if bool((err > bound).any()):
            raise ContractViolation("bound", f"{what}: a code misses the remainder by {float((err / bound).max()):.3f} half ulps")
        worst = float((err / bound).max())
        n = nst * 6144 + nst
    _same(out[:GUARD], before[:GUARD], what + " front guard")
    _same(out[GUARD + n:], before[GUARD + n:], what + " behind the pack")
    return worst


def _decoded(t, kind, idx=None):
    """The allocation as float32 values the generic checker can compare: BLS words of the write set -> hi + lo; 2-byte
    elements -> their values."""
    if kind == "bls":
        o = t.clone()
        o[idx] = bls_decode(t[idx])[0].float()
        return o
    if kind in (torch.float16, torch.bfloat16):
        return h2(t, kind).float()
    return t


def verify(b, ref, after, what=None):
    """Every output allocation of a built case (`after`: name -> CPU tensor after the launch) against `ref`.  Returns the
    worst err / bound.  Raises ContractViolation: nan | exact | bound | sentinel | amax."""
    what = what or b.case.name
    if b.case.entry == "pack_w":
        return _check_pack(after["Wpack"], b.bufs["Wpack"], ref["pack"], b.kw, what)
    worst = 0.0
    for key, name in b.out_keys.items():
        kind, before, out = b.kinds[name], b.bufs[name], after[name]
        if key not in ref:                     # run_if pointed at 0: nothing may change, amax included
            _same(out, before, f"{what} {key} (launch predicated off)")
            continue
        if kind == "amax":
            lo, hi = ref[key]
            _same(torch.cat([out[:16], out[17:]]), torch.cat([before[:16], before[17:]]), f"{what} amax guard words")
            b0, a1 = float(before[16:17].view(torch.float32)), float(out[16:17].view(torch.float32))
            if not (max(b0, lo) <= a1 <= max(b0, hi)):
                raise ContractViolation("amax", f"{what}: amax {b0!r} -> {a1!r}, the contract says max(before, [{lo!r}, {hi!r}])")
            continue
        r = ref[key]
        base = b.base(name)
        if kind == "bls":
            worst = max(worst, check(_decoded(out, kind, r.idx + base), before, r, f"{what} {key}", base))
        elif kind in (torch.float16, torch.bfloat16):
            worst = max(worst, check(_decoded(out, kind), _decoded(before, kind), r, f"{what} {key}", 2 * base))
        else:
            worst = max(worst, check(out, before, r, f"{what} {key}", base))
        if key + ":bits" in ref:
            want = ref[key + ":bits"]
            got = (out[base:].view(want.dtype))[: want.numel()]
            if not torch.equal(got, want):
                j = int((got != want).nonzero()[0])
                raise ContractViolation("exact", f"{what} {key}: element {j} holds {int(got[j]):#x}, bit-exact is {int(want[j]):#x}")
    return worst


def output_bits(b, after):
    """The output allocations as one int32 vector (two launches, or a launch with garbage in what it must not read)."""
    return torch.cat([after[n].contiguous().view(torch.int32).reshape(-1) for n in b.outs])


def perfect(b, ref):
    """The buffers a correctly rounding kernel leaves for `ref` (the host test plants its defects into copies of these)."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    for key, name in b.out_keys.items():
        if key not in ref:
            continue
        kind, base = b.kinds[name], b.base(name)
        if kind == "amax":
            before = float(after[name][16:17].view(torch.float32))
            after[name][16] = _fbits(max(before, 0.5 * (ref[key][0] + ref[key][1])))
            continue
        r = ref[key]
        if key + ":bits" in ref:              # (re-encoding hi + lo need not give the same pair)
            want = ref[key + ":bits"]
            after[name][base:].view(want.dtype)[: want.numel()] = want
        elif kind == "bls":
            after[name][r.idx + base] = bls_encode(r.val.float())
        elif kind in (torch.float16, torch.bfloat16):
            after[name].view(torch.int16)[r.idx + 2 * base] = r.val.float().to(kind).view(torch.int16)
        else:
            after[name][r.idx + base] = r.val.float()
    return after


def emulate(b, tensors=None):
    """The case on tests/emu_blk.py.  The emulation keeps BL buffers as plain fp32 (it does not model the split pair), so
    BLS operands are decoded on the way in and A_bl is encoded on the way out.  Returns the buffers after the call."""
    from tests import emu_blk
    t = {k: v.clone() for k, v in (tensors or b.bufs).items()}
    d, e = b.case.dims, b.case.entry
    bls_in = {"gemm_b2p": ["A"] if d.get("a_fmt") == 0 else [],
              "gemm_tnb": (["G"] if d.get("g_fmt") == 0 else []) + (["A0", "A1"] if d.get("a_fmt") == 0 else [])}.get(e, [])
    for n in bls_in:
        if n in t:
            t[n] = bls_decode(t[n])[0].float()
    run(emu_blk, b, t)
    if "A_bl" in b.out_keys and not (b.kw.get("run_if") is not None and int(t["run_if"][16]) == 0):
        n = b.kw["sm"].L * -(-b.kw["sm"].nseq // 32) * 32 * 128
        t["A_bl"][GUARD:GUARD + n] = bls_encode(t["A_bl"][GUARD:GUARD + n])
    return t
