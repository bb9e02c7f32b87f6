"""TEST INFRASTRUCTURE ONLY -- contract suite of the speaker pooling and the ragged speaker stage: conv2d.hip (ws_tstp_fwd, ws_astp_fwd /
bwd, ws_seg_sums / scale, ws_preemph_pad, ws_power_spec, ws_log_eps), mhastp.hip (ws_mhastp_pack / fwd / bwd / fwd_split / bwd_split)
and ragged_spk.hip (ws_bn_prelu_fwd_len, ws_tstp_fwd_len, ws_astp_fwd_len, ws_time_mean_len, ws_cmn_len, ws_tail_select_len,
ws_preemph_pad_len).  Same shape as tests/step_contract.py: Ref, check, eps_for, the guards and the pairwise generator with its
registries come from tests/gemm_contract.py, Partial / check_partial / sum32 from tests/norm_contract.py, the builders of guarded
operands from tests/map_contract.py.  No GPU code here: test_pool_contract_host_cpu.py checks this module, test_pool_contract_gpu.py
runs every case through wesep_amd.dev.

1. REFERENCE.  compute(entry, sp, tensors, dtype, order, defect, tiles) restates include/wesep_hip.h as explicit index arithmetic.
   In float64 it is the reference, in float32 (sums over time sequential or pairwise; the softmax of MHASTP in one pass or online in
   the tiles and T splits of the kernel) the emulation of a correct kernel, with `defect` a planted defect.  n_r = the row's table
   entry clamped as the header says ([1, T]; tail_select [0, T]; bn_prelu [0, W]; preemph_pad_len [max(pad + 1, 2), T]); without a
   table n_r = T.  Everything behind n_r is selected to zero, never multiplied.
     tstp_fwd[_len]    mean = sum_{t < n} x / n;  var = sum (x - mean)^2 / (n - 1) (n = 1: 0);  stats[r][0 | 1][c F + f] = mean | sqrt(var + eps)
     astp_fwd[_len]    m = max_t lg, e = exp(lg - m), z = sum e, mean = sum e x / z, ex2 = sum e x^2 / z over t < n;  out[r] = mean ||
                       sqrt(max(ex2 - mean^2, floor));  aux[r] = (m, z, mean, ex2)
     astp_bwd          gv = gstd / (2 std) where ex2 - mean^2 > floor (STRICT), else 0;  gm = gmean - 2 mean gv;  al = exp(lg - m) / z;
                       dx = al (gm + 2 gv x);  dlogits = al (gm x + gv x^2 - gm mean - gv ex2)
     seg_sums          out[r][s][c] = sum over t in [s seg_len, min(T, (s + 1) seg_len)) of a (b)
     seg_scale         out[r][t][c] = (x ? x : 1) m[r][t / seg_len][c]
     preemph_pad[_len] y[k] = x[k] - coef x[k - 1], y[0] = x[0] - coef x[1];  out[r][j] = y[reflect_n(j - pad)] for j < n + 2 pad, 0 up to
                       T + 2 pad (the turn of the reflection is the row's own n)
     power_spec        p[m][f] = re^2 + im^2 (f < nf), 0 for f in [nf, ldp)
     log_eps           x = log(x + eps)
     bn_prelu_fwd_len  row m: r = m / rows_per_r, w = m % W;  u = ((x - mean) rstd) gamma + beta (+ res), y = u > 0 ? u : slope u where
                       w < n_r, both 0 elsewhere
     time_mean_len     mean[r][c] = sum_{t < n} x / n;   cmn_len  y = t < n ? x - mean : 0;   tail_select_len  y = t < n ? x : 0
     MHASTP            head h = channels [h Ch, (h + 1) Ch) x F rows, dm = Ch F.  Kernel feature order k = f Ch + c, upstream order
                       nat(k) = c F + f.  pack block (q H + h) = W1 [n1][dm] with its columns in KERNEL order, b1 [n1], then (layers 2) W2
                       [ds][64], b2 [ds];  n1 = 64 (layers 2) | ds (layers 1).  logits[t][i] = W2 tanh(W1 x_t + b1) + b2 | W1 x_t + b1, row
                       i = 0 (ds = 1) or nat(k) (ds = dm) serves feature k.  m, s = max / sum exp over T, mean = sum e x / s, var = sum e
                       x^2 / s - mean^2.  aux [R][Q][H][4][dm] = (m, s, mean, var) in KERNEL order (var raw, unclamped);  out [R][Q][H][2]
                       [dm] = mean || sqrt(max(var, 1e-7)) in UPSTREAM order.
     mhastp_fwd_split  the same from tsplit partial states over frames [s ceil(T / tsplit), ...); a split without a frame leaves
                       (-inf, 0, 0, 0) in part and is skipped by the merge
     mhastp_bwd[_split] dvar = dstd / (2 sqrt(var)) where var >= 1e-7 (NOT strict), else 0;  c = dmean mean + dvar (var - mean^2);  al =
                       exp(logit - m) / s;  g = x (dmean + dvar (x - 2 mean));  dlogit[t][nat(k)] = al (g - c) (ds = dm) | dlogit[t] = al
                       sum_k (g - c) (ds = 1);  dz = (W2^T dlogit)(1 - h^2);  dx = sum_q (al (dmean + 2 dvar (x - mean)) + W1^T dz);
                       work = dz [M][QH][n1], (layers 2) h [M][QH][64], dlogit [M][QH][ds], M = R T;  slab[s] = the blocks (dW1 with its
                       columns back in UPSTREAM order, db1, dW2, db2) summed over the rows of split s = [s ceil(M / nsplit), ...);
                       dpack = the slabs summed (nsplit = 1: written directly)
   Backward entries TAKE their forward quantities (aux, out) as the fp32 rounding of the float64 values and the reference computes
   from exactly those fp32 numbers, the clamp branch included.  astp_bwd's branch is an fp32 expression (ex2 - mean mean) the
   compiler may contract into one fma: where the two evaluations disagree the element is judged against the hull of both branches.

2. BOUNDS.  Per element, derived; u = 2^-24, e(n) = eps_for(False, n) = (n + 8) u over the same expression in absolute values.
     bit-exact    seg_scale with x NULL, tail_select_len, mhastp_pack, every zero behind a length, the columns [nf, ldp) of power_spec,
                  preemph_pad at coef = 0, a one-frame segment of seg_sums without b, the slab rows of a split that owns no row, the
                  state of a T split that owns no frame
     elementwise  a path of r <= 7 roundings is inside e(0) S: bn_prelu_fwd_len (bit for bit against ws_bn_prelu_fwd is a device
                  identity of test_pool_contract_gpu.py), preemph_pad, power_spec, seg_scale (u |out|)
     log_eps      u (the rounding of x + eps moves the log by at most u) + D_LOG |log|, D_LOG = 2 ULP_LOG u, ULP_LOG = 3 (OpenCL full profile)
     sums         mean, seg_sums: e(n) sum |.| (any order); cmn: d_mean + u |y|
     TSTP         d_m = e(n) E|x|; the kernel's second pass runs around its own mean: sum (x - mean')^2 = m2 + n (mean - mean')^2, so
                  m2' in [m2 (1 - e(n + 3)), (m2 + n d_m^2)(1 + e(n + 3))]; std = the image of that interval under sqrt(. / (n - 1) + eps),
                  three more roundings
     softmax      a logit error dz gives the weight exp(lg - m) a relative error w = D_EXP + expm1(dz).  ASTP: dz = u |lg - m| (the
                  max of inputs is exact).  z: sum e w + e(n) z.  One weight error serves z, s1 and s2 alike, so with alpha' = e (1 +
                  d) / sum e (1 + d), wbar = sum alpha w and ww = (w + wbar) / (1 - wbar): |alpha' - alpha| <= alpha ww, and exactly
                  sum alpha' (x - mean')^2 = sum alpha' (x - mean)^2 - (mean' - mean)^2.  The sums' own roundings (rho = 2 e(n) + 3 u:
                  two sums, the products, the division) are relative to E|x| and E[x^2]: d_mean = sum alpha |x - mean| ww + rho E|x|;
                  d_ex2 = sum alpha x^2 ww + rho ex2; var = ex2 - mean^2 as the interval [var - d_var, var + d_var], d_var = sum alpha
                  (x - mean)^2 ww + (sum alpha |x - mean| ww)^2 + rho ex2 + 2 |mean| rho E|x| + 2 u (ex2 + mean^2): the cancellation
                  costs roundings, not weight errors; std = the image of that interval under sqrt(max(., floor)) (1 +- 2 u): a case
                  that straddles the floor is judged against the interval, never a point.
     MHASTP       dz through the attention: d_z1 = e(dm + 1)(|x| |W1| + |b1|); tanh is 1-Lipschitz: d_h = d_z1 + D_TANH |h|; d_logit = |W2|
                  d_h + e(65)(|W2| |h| + |b2|) (layers 1: d_z1).  aux[0], a max of computed logits: max_t d_logit.  The exponent's
                  error: d_logit + d_max + u |logit - m|.  Online evaluation rescales the running sums once per tile and once per
                  split: w += (tiles + tsplit)(D_EXP + 3 u) + u |m - logit| (the rescale exponents telescope to m - logit), sums e(T +
                  tiles + tsplit); a weight below 2^-100 may flush to zero (absolute term).
     astp_bwd     al: D_EXP + expm1(u |lg - m|) + u.  dx: (w + e(0)) al (|gmean| + 2 |mean gv| + 2 |gv x|); dlogits: (w + e(4)) al ((|gmean|
                  + 2 |mean gv|)(|x| + |mean|) + |gv| (x^2 + ex2))
     mhastp_bwd   al as above with d_logit of the recomputed attention.  dlogit: al S_g (w + e(4)), S_g = |x| (|dmean| + |dvar| (|x| + 2
                  |mean|)) + |dmean mean| + |dvar| (|var| + mean^2) (ds = 1: sum_k S_g, e(dm + 4)).  dz: |W2| d_dlogit |1 - h^2| + e(ds + 1)
                  |W2| |dlogit| + |acc| (2 |h| d_h + d_h^2 + 2 u).  dx: sum_q (al S_A (w + e(0)) + |W1| d_dz + e(n1 + 1) |W1| |dz|) + e(2 Q) S.
                  Weight gradients: sum_m (d_G |A| + |G| d_A) + e(M + 1) sum |G| |A| as Partial sums over the splits; dpack + e(nsplit) S.

3. CONDITION OF THE SUITE.  No sum is longer than CAP = 2048 leaves, but for the two cases that cross the one-frame tiles (dm =
   2720, 4080: the inner product of the attention over dm), which no planted defect relies on.  test_pool_contract_host_cpu.py
   shows every planted defect refused by the reference alone, and computes the worst derived bound on mean and std of MHASTP
   relative to the feature's rms over the ordinary regimes (gauss, dm <= CAP, T > 1: at T = 1 the variance is the floor);
   profiles/pool_contract.md records it.  It is looser than the global 1e-5 of test_mhastp_gpu.py, by design: e(dm) is a worst
   case over the signs of dm roundings and goes through the exponential; that test stays, and this one sees what it cannot.

4. CASES.  cases(entry): gemm_contract's pairwise generator over DIMS, topped up to MIN_PER_TARGET per dispatch target of INST,
   plus EXTRA (every lane-split factor of mh_stage1, the one-frame tiles of dm = 2720 / 4080, the row splits of the weight
   gradients, the empty T split).  GRID_CAP_CASE (tail_select_len over the 32768-block cap) is run once by the GPU file alone.

BUFFERS.  As step_contract: GUARD floats around every operand and output, write sets NaN, the rest SENT; everything a contract does
not read (behind a length, between ld and width) is NaN, build(case, garbage=True) puts a large finite value there.  part (the T
split workspace) is scratch: judged only for the empty-split states and for staying inside its extent."""
import math

import torch

from tests import gemm_contract as gc
from tests import map_contract as mc
from tests import tasnet_contract as tc
from tests.gemm_contract import (GUARD, SENT, U, Buf, Built, Case, ContractViolation, Ref, check, eps_for)  # noqa: F401
from tests.norm_contract import Partial, check_partial, sum32  # noqa: F401
from tests.tasnet_contract import TBuilt, _f32, _red_ref

GARBAGE, NAN, CAP, TINY = mc.GARBAGE, mc.NAN, 2048, mc.TINY
F64, F32 = torch.float64, torch.float32
ULP_EXP, ULP_TANH, ULP_LOG = mc.ULP_EXP, mc.ULP_TANH, 3
D_EXP, D_TANH, D_LOG = mc.D_EXP, mc.D_TANH, 2 * 3 * U
E0 = eps_for(False, 0)
FLOOR = 1e-7
FLOOR32 = float(_f32(FLOOR))
FLUSH = 2.0 ** -100
ORDERS = ("seq", "pairwise")
TILES = ("online", "onepass")
MH_THREADS, MH_TT, MH_LDS_FLOATS = 256, 16, 16384
_ar, _ref, _sum = mc._ar, mc._ref, mc._sum
CONV_ENTRIES = ("tstp_fwd", "astp_fwd", "astp_bwd", "seg_sums", "seg_scale", "preemph_pad", "power_spec", "log_eps")
MH_ENTRIES = ("mhastp_pack", "mhastp_fwd", "mhastp_bwd", "mhastp_fwd_split", "mhastp_bwd_split")
LEN_ENTRIES = ("bn_prelu_fwd_len", "tstp_fwd_len", "astp_fwd_len", "time_mean_len", "cmn_len", "tail_select_len", "preemph_pad_len")
ENTRIES = CONV_ENTRIES + MH_ENTRIES + LEN_ENTRIES
SCRATCH = ("part",)


def _en(n):
    """e(n) for a tensor (or number) of term counts."""
    return (n + 8) * U


# ------------------------------------------------------------------------------------------------------------
# index arithmetic shared by compute and reference
# ------------------------------------------------------------------------------------------------------------
def len_lo(entry, sp):
    """The lower end of the clamp range the header states for the entry's table."""
    if entry == "tail_select_len" or entry == "bn_prelu_fwd_len":
        return 0
    if entry == "preemph_pad_len":
        return max(sp["pad"] + 1, 2)
    return 1


def lens(entry, sp, defect=None):
    """[R] frames of every row: the table clamped as the header says (no table: T; bn_prelu: W)."""
    hi = sp["W"] if entry == "bn_prelu_fwd_len" else sp["T"]
    tab = sp.get("tab")
    if tab is None:
        return torch.full((sp["R"],), hi, dtype=torch.long)
    v = torch.tensor(tab, dtype=torch.long)
    if defect == "tlen_unclamped":
        return v
    if defect == "clamp_pad_plus_1":
        return v.clamp(sp["pad"] + 1, hi)
    if defect == "clamp_lo_1":
        return v.clamp(1, hi)
    return v.clamp(len_lo(entry, sp), hi)


def _tmask(T, n, defect=None):
    """[R, T]: t < n_r (the planted tlen + 1 reads one frame more)."""
    return _ar(T)[None, :] < (n + (1 if defect == "tlen_plus_1" else 0))[:, None]


def mh_n1(layers, ds):
    return 64 if layers == 2 else ds


def mh_block_floats(layers, ds, dm):
    n1 = mh_n1(layers, ds)
    return n1 * dm + n1 + (64 * ds + ds if layers == 2 else 0)


def mh_tt(dm, layers, ds, bwd):
    """Frames per tile (mh_geom): MH_TT, or what the 64 KiB of LDS hold; below 1 the geometry is refused."""
    per_tt = (2 if bwd else 1) * dm + mh_n1(layers, ds) + (ds if layers == 2 else 0)
    return min(MH_TT, (MH_LDS_FLOATS - (4 * MH_TT if bwd else 0)) // per_tt)


def mh_ks(n1):
    """Lanes that share one output row of mh_stage1."""
    ks = 1
    while ks * 2 <= 64 and ks * 2 * n1 <= MH_THREADS:
        ks *= 2
    return ks


def mh_split_sizes(R, T, H, cus):
    """ws_mhastp_split_sizes' tsplit (mh_tsplit)."""
    rh, want = R * H, 2 * max(cus, 1)
    tiles = -(-T // MH_TT)
    n = max(1, min(tiles, -(-want // rh)))
    per = -(-tiles // n)
    return -(-tiles // per)


def mh_nat(F_, Ch):
    """nat[k] = c F + f of the kernel index k = f Ch + c."""
    k = _ar(F_ * Ch)
    return (k % Ch) * F_ + k // Ch


def _mh(sp):
    R, F_, T, Ch, Q, H, layers, ds = (sp[k] for k in ("R", "F", "T", "Ch", "Q", "H", "layers", "ds"))
    dm = F_ * Ch
    n1 = mh_n1(layers, ds)
    return R, F_, T, Ch, Q, H, layers, ds, dm, n1, mh_block_floats(layers, ds, dm), n1 * dm + n1


def _mh_blocks(sp, t, dt, defect=None):
    """(W1 [Q, H, n1, dm] in kernel order, b1 [Q, H, n1], W2 [Q, H, ds, 64] | None, b2 [Q, H, ds] | None) of the pack."""
    R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
    pk = t["pack"][:Q * H * P1].to(dt)
    pk = pk.reshape(H, Q, P1).permute(1, 0, 2) if defect == "block_h_major" and Q > 1 and H > 1 else pk.reshape(Q, H, P1)
    W1, b1 = pk[..., :n1 * dm].reshape(Q, H, n1, dm), pk[..., n1 * dm:off2]
    if layers == 1:
        return W1, b1, None, None
    return W1, b1, pk[..., off2:off2 + 64 * ds].reshape(Q, H, ds, 64), pk[..., off2 + 64 * ds:off2 + 64 * ds + ds]


def _mh_x(sp, t, dt, defect=None):
    """x [R][F][T][C] as [R, H, T, dm] in kernel order."""
    R, F_, T, Ch, Q, H = (sp[k] for k in ("R", "F", "T", "Ch", "Q", "H"))
    X = t["x"][:R * F_ * T * Ch * H].to(dt).reshape(R, F_, T, H, Ch).permute(0, 3, 2, 1, 4).reshape(R, H, T, F_ * Ch)
    if defect == "head0_for_all" and H > 1:
        X = X[:, :1].expand(R, H, T, F_ * Ch)
    return X


def _mh_unx(sp, v):
    """[R, H, T, dm] kernel order -> flat [R][F][T][C]."""
    R, F_, T, Ch, H = (sp[k] for k in ("R", "F", "T", "Ch", "H"))
    return v.reshape(R, H, T, F_, Ch).permute(0, 3, 2, 1, 4).reshape(-1)


def _mh_attention(sp, t, dt, defect=None):
    """X [R, H, T, dm], hidden [R, Q, H, T, n1] (tanh output | logits), logits by row [R, Q, H, T, ds], by feature [.., dm]."""
    R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
    X = _mh_x(sp, t, dt, defect)
    W1, b1, W2, b2 = _mh_blocks(sp, t, dt, defect)
    z1 = torch.einsum("rhtk,qhuk->rqhtu", X, W1) + b1[None, :, :, None, :]
    if layers == 2:
        hid = z1 if defect == "tanh_skipped" else torch.tanh(z1)
        Lr = torch.einsum("rqhtu,qhiu->rqhti", hid, W2) + b2[None, :, :, None, :]
    else:
        hid, Lr = z1, z1
    Lk = Lr.expand(R, Q, H, T, dm) if ds == 1 else Lr[..., mh_nat(F_, Ch)]
    return X, hid, Lr, Lk


def _mh_tiles(sp, tsplit):
    """[(split, [(t0, nt), ...])] of the forward's tiles."""
    T, TT = sp["T"], sp["TTf"]
    chunk = -(-T // tsplit)
    out = []
    for s in range(tsplit):
        lo = min(T, s * chunk)
        hi = min(T, lo + chunk)
        out.append((s, [(t0, min(TT, hi - t0)) for t0 in range(lo, hi, TT)]))
    return out


def _mh_moments(sp, Lk, X, dt, order, tiles, tsplit, merge, defect=None):
    """(m, s, sx, sxx) [R, Q, H, dm] and the states of empty splits.  float64 / onepass: max and sums over T at once; online:
    the kernel's tiles, T splits and merge."""
    xv = X[:, None]
    if dt == F64 or tiles == "onepass":
        m = Lk.max(3).values
        e = torch.exp(Lk - m[:, :, :, None])
        tl = lambda v: v.permute(0, 1, 2, 4, 3)          # noqa: E731
        return m, _sum(tl(e), order), _sum(tl(e * xv), order), _sum(tl((e * xv) * xv), order)
    ninf = torch.full(Lk.shape[:3] + Lk.shape[4:], -math.inf, dtype=dt)
    states = []
    for s, tl in _mh_tiles(sp, tsplit):
        m, se, sx, sxx = ninf.clone(), torch.zeros_like(ninf), torch.zeros_like(ninf), torch.zeros_like(ninf)
        for t0, nt in tl:
            if defect == "partial_tile_dropped" and nt < sp["TTf"]:
                continue
            L = Lk[:, :, :, t0:t0 + nt]
            mt = torch.maximum(m, L.max(3).values)
            sc = torch.exp(m - mt)
            if defect == "no_rescale":
                sc = torch.where(torch.isinf(m), sc, torch.ones_like(sc))
            se, sx = se * sc, sx * sc
            if defect != "rescale_not_sxx":
                sxx = sxx * sc
            e = torch.exp(L - mt[:, :, :, None])
            x_ = xv[:, :, :, t0:t0 + nt]
            if order == "seq":
                for tt in range(nt):
                    se, sx, sxx = se + e[:, :, :, tt], sx + e[:, :, :, tt] * x_[:, :, :, tt], sxx + (e[:, :, :, tt] * x_[:, :, :, tt]) * x_[:, :, :, tt]
            else:
                pm = lambda v: v.permute(0, 1, 2, 4, 3)          # noqa: E731
                se, sx, sxx = se + _sum(pm(e), order), sx + _sum(pm(e * x_), order), sxx + _sum(pm((e * x_) * x_), order)
            m = mt
        states.append((m, se, sx, sxx))
    if not merge:
        return states[0]
    first = 1 if defect == "merge_skips_split0" and tsplit > 1 else 0
    m = ninf.clone()
    for st in states:
        m = torch.maximum(m, st[0])
    se, sx, sxx = torch.zeros_like(ninf), torch.zeros_like(ninf), torch.zeros_like(ninf)
    for st in states[first:]:
        empty = st[1] == 0
        sc = torch.exp(st[0] - m)
        if defect == "empty_split_nan":
            sc = torch.where(empty, torch.full_like(sc, NAN), sc)
            empty = torch.zeros_like(empty)
        se, sx, sxx = (torch.where(empty, a, a + p * sc) for a, p in ((se, st[1]), (sx, st[2]), (sxx, st[3])))
    return m, se, sx, sxx


def _mh_empty_part(sp, tsplit):
    """(flat indices into part, values) of the states of T splits that own no frame."""
    R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
    per = R * Q * H * 4 * dm
    idx, val = [], []
    for s, tl in _mh_tiles(sp, tsplit):
        if not tl:
            idx.append(s * per + _ar(per))
            v = torch.zeros(R * Q * H, 4, dm, dtype=F64)
            v[:, 0] = -math.inf
            val.append(v.reshape(-1))
    return (torch.cat(idx), torch.cat(val)) if idx else (torch.zeros(0, dtype=torch.long), torch.zeros(0, dtype=F64))


def mh_rps(sp):
    return -(-(sp["R"] * sp["T"]) // sp["nsplit"])


def _row_weights(sp, defect=None):
    """(split [M], weight [M]) of the rows m = r T + t of the weight gradients."""
    M = sp["R"] * sp["T"]
    rps = mh_rps(sp)
    m = _ar(M)
    w = torch.ones(M, dtype=F64)
    if defect == "split_last_block_dropped":
        j = m % rps
        last = torch.minimum((m // rps + 1) * rps, torch.tensor(M)) - (m // rps) * rps          # rows of the split
        w[(j // 16 == (last - 1) // 16) & (last % 16 != 0)] = 0.0
    if defect == "wgrad_skips_split0" and sp["nsplit"] > 1:
        w[m // rps == 0] = 0.0
    return m // rps, w


# ------------------------------------------------------------------------------------------------------------
# compute: the header's formulas, in `dt` (float64: the reference; float32: the emulation), with planted defects
# ------------------------------------------------------------------------------------------------------------
def _tstp_parts(e, sp, t, dt, order, defect=None):
    R, Fq, T, C = sp["R"], sp["F"], sp["T"], sp["C"]
    n = lens(e, sp, defect)
    mask = _tmask(T, n, defect)[:, None, None, :]          # [R, 1, 1, T]
    x = t["x"][:R * Fq * T * C].reshape(R, Fq, T, C).to(dt).permute(0, 1, 3, 2)          # [R, F, C, T]
    zero = torch.zeros((), dtype=dt)
    xs = torch.where(mask, x, zero)
    cnt = n.to(dt)[:, None, None]
    mean = _sum(xs, order) / (T if defect == "mean_div_T" else cnt)
    dv = torch.where(mask, xs - mean[..., None], zero)
    m2 = _sum(dv * dv, order)
    den = cnt if defect == "div_by_T" else cnt - 1
    var = torch.where(cnt > 1, m2 / torch.where(den > 0, den, torch.ones_like(den)), zero)
    return dict(mean=mean, m2=m2, var=var, cnt=cnt, absmean=_sum(xs.abs(), order) / cnt.clamp_min(1))


def _astp_parts(e, sp, t, dt, order, defect=None):
    R, T, C = sp["R"], sp["T"], sp["C"]
    n = lens(e, sp, defect)
    mask = _tmask(T, n, defect)[:, None, :]          # [R, 1, T]
    zero = torch.zeros((), dtype=dt)
    x = torch.where(mask, t["x"][:R * T * C].reshape(R, T, C).to(dt).permute(0, 2, 1), zero)
    lg = torch.where(mask, t["lg"][:R * T * C].reshape(R, T, C).to(dt).permute(0, 2, 1), torch.full((), -math.inf, dtype=dt))
    m = lg.max(2).values
    ex = torch.where(mask, torch.exp(lg - m[..., None]), zero)
    z, s1, s2 = _sum(ex, order), _sum(ex * x, order), _sum(ex * x * x, order)
    return dict(x=x, lg=lg, m=m, e=ex, z=z, s1=s1, s2=s2, cnt=n.to(dt)[:, None], mask=mask)


def _preemph(e, sp, t, dt, defect=None):
    R, T, pad, ldo = sp["R"], sp["T"], sp["pad"], sp["ldo"]
    coef = _f32(sp["coef"], dt)
    x = t["x"][:R * T].reshape(R, T).to(dt)
    L = lens(e, sp, defect)[:, None]
    turn = torch.full_like(L, T) if defect == "reflect_at_T" else L
    j = _ar(T + 2 * pad)[None, :].expand(R, -1)
    k = (j - pad).abs()
    k = torch.where(k >= turn, 2 * (turn - 1) - k, k).clamp(0, T - 1)
    prev = torch.where(k > 0, k - 1, torch.zeros_like(k) if defect == "y0_from_x0" else torch.ones_like(k)).clamp(0, T - 1)
    val = torch.gather(x, 1, k) - coef * torch.gather(x, 1, prev)
    tail = torch.full((), NAN if defect == "tail_unwritten" else 0.0, dtype=dt)
    return torch.where(j < L + 2 * pad, val, tail), j < L + 2 * pad, torch.gather(x, 1, k), coef * torch.gather(x, 1, prev)


def _astp_branch(aux):
    """astp_bwd's test ex2 - mean mean > floor in fp32, as two roundings and as one fma: (taken, ambiguous) [R, C]."""
    mean, ex2 = aux[:, 2].double(), aux[:, 3].double()
    two = (ex2 - (mean * mean).float().double()).float().double() > FLOOR32
    one = (ex2 - mean * mean).float().double() > FLOOR32
    return two, two != one


def compute(entry, sp, t, dt=F64, order="seq", defect=None, tiles="online"):
    """name -> values of every output of `entry` (slabs as [nsplit, columns])."""
    e = entry
    zero = torch.zeros((), dtype=dt)
    if e in ("tstp_fwd", "tstp_fwd_len"):
        R, Fq, C = sp["R"], sp["F"], sp["C"]
        p = _tstp_parts(e, sp, t, dt, order, defect)
        sd = torch.sqrt(p["var"] + _f32(sp["eps"], dt))
        if defect == "feature_f_major":
            return {"stats": torch.stack([p["mean"].reshape(R, -1), sd.reshape(R, -1)], 1)}
        return {"stats": torch.stack([p["mean"].permute(0, 2, 1).reshape(R, -1), sd.permute(0, 2, 1).reshape(R, -1)], 1)}
    if e in ("astp_fwd", "astp_fwd_len"):
        p = _astp_parts(e, sp, t, dt, order, defect)
        mean, ex2 = p["s1"] / p["z"], p["s2"] / p["z"]
        var = ex2 - mean * mean
        sd = torch.sqrt(var if defect == "var_unclamped" else torch.maximum(var, _f32(FLOOR, dt)))
        return {"out": torch.cat([mean, sd], 1), "aux": torch.stack([p["m"], p["z"], mean, var if defect == "aux3_is_var" else ex2], 1)}
    if e == "astp_bwd":
        R, T, C = sp["R"], sp["T"], sp["C"]
        x, lg = (t[k][:R * T * C].reshape(R, T, C).to(dt) for k in ("x", "lg"))
        aux, out, do = t["aux"][:R * 4 * C].reshape(R, 4, C), t["out"][:R * 2 * C].reshape(R, 2, C).to(dt), t["dout"][:R * 2 * C].reshape(R, 2, C).to(dt)
        m, z, mean, ex2 = (aux[:, i].to(dt)[:, None] for i in range(4))
        taken, _ = _astp_branch(aux)
        if defect == "floor_not_strict":
            taken = (aux[:, 3].double() - aux[:, 2].double() ** 2).float().double() >= FLOOR32
        if sp.get("branch") is not None:
            taken = sp["branch"]
        gv = torch.where(taken, do[:, 1] / (2 * out[:, 1]), zero)[:, None]
        gm = do[:, 0][:, None] - 2 * mean * gv
        al = torch.exp(lg - m) / z
        dbar = gm * mean + gv * (ex2 - mean * mean if defect == "dbar_with_var" else ex2)
        return {"dx": al * (gm + 2 * gv * x), "dlg": al * (gm * x + gv * x * x - dbar)}
    if e == "seg_sums":
        R, T, C, sl = sp["R"], sp["T"], sp["C"], sp["seg_len"]
        nseg = -(-T // sl)
        v = t["a"][:R * T * C].reshape(R, T, C).to(dt)
        if sp["b"] and defect != "b_ignored":
            v = v * t["b"][:R * T * C].reshape(R, T, C).to(dt)
        if defect == "odd_frame_dropped":
            tt = _ar(T)
            cnt = torch.minimum(torch.tensor(T), (tt // sl + 1) * sl) - (tt // sl) * sl
            v = torch.where(((cnt % 2 == 1) & (tt % sl == cnt - 1))[None, :, None], zero, v)
        vp = torch.zeros(R, nseg * sl, C, dtype=dt)
        vp[:, :T] = v
        return {"out": _sum(vp.reshape(R, nseg, sl, C).permute(0, 1, 3, 2), order)}
    if e == "seg_scale":
        R, T, C, sl = sp["R"], sp["T"], sp["C"], sp["seg_len"]
        nseg = -(-T // sl)
        idx = (_ar(T) % sl).clamp(max=nseg - 1) if defect == "t_mod_seg_len" else _ar(T) // sl
        v = t["m"][:R * nseg * C].reshape(R, nseg, C).to(dt)[:, idx]
        if sp["x"] and defect != "x_ignored":
            v = v * t["x"][:R * T * C].reshape(R, T, C).to(dt)
        return {"out": v}
    if e in ("preemph_pad", "preemph_pad_len"):
        return {"out": _preemph(e, sp, t, dt, defect)[0]}
    if e == "power_spec":
        M, nf, lds, ldp = sp["M"], sp["nf"], sp["lds"], sp["ldp"]
        s = t["spec"][:M * lds].to(dt)
        s = s[:M * 2 * nf].reshape(M, 2 * nf) if defect == "stride_2nf" else s.reshape(M, lds)[:, :2 * nf]
        re, im = s[:, 0::2], s[:, 1::2]
        p = torch.full((M, ldp), NAN if defect == "pad_unwritten" else 0.0, dtype=dt)
        p[:, :nf] = re * re + (re * re if defect == "re_twice" else im * im)
        return {"p": p}
    if e == "log_eps":
        x = t["x"][:sp["n"]].to(dt)
        if defect == "log10":
            return {"x": torch.log10(x + _f32(sp["eps"], dt))}
        return {"x": torch.log(x if defect == "eps_dropped" else x + _f32(sp["eps"], dt))}
    if e == "bn_prelu_fwd_len":
        R, rpr, W, C = sp["R"], sp["rpr"], sp["W"], sp["C"]
        M = R * rpr
        m = _ar(M)
        r = (m // W) % R if defect == "r_from_W" else m // rpr
        valid = ((m % W) < lens(e, sp, defect)[r])[:, None]
        x = t["x"][:M * C].reshape(M, C).to(dt)
        st = t["stats"][:2 * C].reshape(2, C).to(dt)
        v = ((x - st[0]) * st[1]) * t["gamma"][:C].to(dt) + t["beta"][:C].to(dt)
        if sp["res"]:
            v = v + t["res"][:M * C].reshape(M, C).to(dt)
        slope = t["a"][0].to(dt)
        y = v if defect == "y_is_u" else torch.where(v > 0, v, slope * v)
        if defect == "tail_multiplied":
            return {"u": v * valid.to(dt), "y": y * valid.to(dt)}
        return {"u": torch.where(valid, v, zero), "y": torch.where(valid, y, zero)}
    if e in ("time_mean_len", "cmn_len", "tail_select_len"):
        R, T, C = sp["R"], sp["T"], sp["C"]
        n = lens(e, sp, defect)
        mask = _tmask(T, n, defect)[:, :, None]
        x = t["x"][:R * T * C].reshape(R, T, C).to(dt)
        if e == "tail_select_len":
            return {"y": x * mask.to(dt) if defect == "tail_multiplied" else torch.where(mask, x, zero)}
        mean = _sum(torch.where(mask, x, zero).permute(0, 2, 1), order) / (T if defect == "mean_div_T" else n.to(dt)[:, None])
        if e == "time_mean_len":
            return {"mean": mean}
        return {"y": (x - mean[:, None]) * mask.to(dt) if defect == "tail_multiplied" else torch.where(mask, x - mean[:, None], zero)}
    if e == "mhastp_pack":
        F_, Ch, layers, ds = sp["F"], sp["Ch"], sp["layers"], sp["ds"]
        dm, n1 = F_ * Ch, mh_n1(layers, ds)
        w1 = t["w1"][:n1 * dm].reshape(n1, dm).to(dt)
        parts = [(w1 if defect == "columns_not_permuted" else w1[:, mh_nat(F_, Ch)]).reshape(-1), t["b1"][:n1].to(dt)]
        if layers == 2:
            parts += [t["w2"][:64 * ds].to(dt), t["b2"][:ds].to(dt)]
            if defect == "b2_before_w2":
                parts[2], parts[3] = parts[3], parts[2]
        return {"blk": torch.cat(parts)}
    if e in ("mhastp_fwd", "mhastp_fwd_split"):
        R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
        X, _, _, Lk = _mh_attention(sp, t, dt, defect)
        split = e == "mhastp_fwd_split"
        m, s, sx, sxx = _mh_moments(sp, Lk, X, dt, order, tiles, sp["tsplit"] if split else 1, split, defect)
        mean = sx / s
        var = sxx / s - mean * mean
        sd = torch.sqrt(var if defect == "var_unclamped" else torch.maximum(var, _f32(FLOOR, dt)))
        nat = mh_nat(F_, Ch)
        o = torch.zeros(R, Q, H, 2, dm, dtype=dt)
        if defect == "out_kernel_order":
            o[..., 0, :], o[..., 1, :] = mean, sd
        else:
            o[..., 0, nat], o[..., 1, nat] = mean, sd
        aux = torch.stack([m, s, mean, var], 3)
        if defect == "aux_native_order":
            a2 = torch.zeros_like(aux)
            a2[..., nat] = aux
            aux = a2
        out = {"out": o, "aux": aux}
        if split:
            out["part"] = _mh_empty_part(sp, sp["tsplit"])[1].to(dt)
        return out
    if e in ("mhastp_bwd", "mhastp_bwd_split"):
        R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
        nat = mh_nat(F_, Ch)
        X, hid, Lr, Lk = _mh_attention(sp, t, dt)
        W1, b1, W2, b2 = _mh_blocks(sp, t, dt)
        aux = t["aux"][:R * Q * H * 4 * dm].reshape(R, Q, H, 4, dm).to(dt)
        m, s, mean, var = (aux[:, :, :, i][:, :, :, None] for i in range(4))          # [R, Q, H, 1, dm]
        go = t["dout"][:R * Q * H * 2 * dm].reshape(R, Q, H, 2, dm).to(dt)
        if defect == "dout_kernel_order":
            dmean, dstd = go[:, :, :, 0][:, :, :, None], go[:, :, :, 1][:, :, :, None]
        else:
            dmean, dstd = go[:, :, :, 0][..., nat][:, :, :, None], go[:, :, :, 1][..., nat][:, :, :, None]
        fl = _f32(FLOOR, dt)
        keep = (var > fl) if defect == "floor_strict" else (var >= fl)
        if defect == "dvar_unclamped":
            keep = torch.ones_like(keep)
        dvar = torch.where(keep, 0.5 * dstd / torch.sqrt(torch.where(keep & (var > 0), var, torch.ones_like(var))), zero)
        if defect == "dvar_unclamped":
            dvar = 0.5 * dstd / torch.sqrt(var)
        c = dmean * mean + (zero if defect == "c_without_var" else dvar * (var - mean * mean))
        al = torch.exp(Lk - m) * (1 / s)
        xv = X[:, None]
        direct = al * (dmean + 2 * dvar * (xv - mean))
        gt = xv * (dmean + dvar * (xv - 2 * mean))
        if ds == 1:
            tot = _sum(gt - c, order)
            dl = (torch.exp(Lr[..., 0] - m[..., 0, 0:1]) / s[..., 0, 0:1] * tot)[..., None]
        else:
            dl = torch.zeros_like(Lk)
            dl[..., nat] = al * (gt - c)
        if layers == 2:
            wz = torch.einsum("rqhti,qhiu->rqhtu", dl, W2) * (1 - hid * hid)
        else:
            wz = dl
        back = torch.einsum("rqhtu,qhuk->rqhtk", wz, W1)
        dxk = torch.zeros_like(X)
        for q in (range(Q - 1, Q) if defect == "last_query_only" else range(Q)):
            dxk = (dxk + direct[:, q]) + back[:, q]
        out = {"dx": _mh_unx(sp, dxk)}
        if not sp["wgrad"]:
            return out
        rows = lambda v: v.permute(0, 3, 1, 2, 4).reshape(R * T, Q, H, -1)          # noqa: E731
        gz, work = rows(wz), [rows(wz).reshape(-1)]
        if layers == 2:
            gh, gl = rows(hid), rows(dl)
            work += [gh.reshape(-1), gl.reshape(-1)]
        out["work"] = torch.cat(work)
        sid, wgt = _row_weights(sp, defect)
        ns = sp["nsplit"]
        Xm = X.permute(0, 2, 1, 3).reshape(R * T, H, dm)
        slab = torch.zeros(ns, Q, H, P1, dtype=dt)
        for sidx in range(ns):
            sel = (sid == sidx).nonzero().reshape(-1)
            if sel.numel() == 0:
                continue
            w = wgt[sel].to(dt)[:, None, None, None]
            g_, x_ = gz[sel] * w, Xm[sel]
            dW1 = torch.einsum("mqhu,mhk->qhuk", g_, x_)
            db1 = g_.sum(0) if dt == F64 else _sum(g_.permute(1, 2, 3, 0), order)
            blk = torch.zeros(Q, H, n1, dm, dtype=dt)
            if defect == "dpack_kernel_order":
                blk = dW1
            else:
                blk[..., nat] = dW1
            if defect == "bias_column_at_nb_minus_1":
                kk = int(nat[dm - 1])
                db1, blk = blk[..., kk].clone(), blk.clone()
                blk[..., kk] = g_.sum(0)
            slab[sidx, :, :, :n1 * dm] = blk.reshape(Q, H, -1)
            slab[sidx, :, :, n1 * dm:off2] = db1
            if layers == 2:
                l_ = gl[sel] * w
                slab[sidx, :, :, off2:off2 + 64 * ds] = torch.einsum("mqhi,mqhu->qhiu", l_, gh[sel]).reshape(Q, H, -1)
                slab[sidx, :, :, off2 + 64 * ds:] = l_.sum(0) if dt == F64 else _sum(l_.permute(1, 2, 3, 0), order)
        slab = slab.reshape(ns, Q * H * P1)
        if ns > 1:
            out["slab"] = slab
        out["dpack"] = slab[0] if ns == 1 else _sum(slab.t(), order)
        return out
    raise ValueError(e)


# ------------------------------------------------------------------------------------------------------------
# reference = compute in float64 + the bounds of the module docstring
# ------------------------------------------------------------------------------------------------------------
def _R(val, bound, exact=None, S=None, idx=None):
    return _ref(_ar(val.numel()) if idx is None else idx, val, val.abs() if S is None else S, bound, exact)


def _exact(val, idx=None):
    return _R(val, torch.zeros_like(val), torch.ones(val.shape, dtype=torch.bool), idx=idx)


def _iv(lo, hi):
    """(val, bound) of an interval."""
    return (lo + hi) / 2, (hi - lo) / 2 * (1 + 1e-12) + TINY


def _moment_bounds(ex, x, w, n, nsum):
    """Softmax moments over the last axis: weights `ex` (float64, masked to 0), data x, relative weight errors w, n terms,
    nsum = the roundings of the sums.  -> dict(z, mean, ex2, var, d_z, d_mean, d_ex2, d_var)."""
    z = ex.sum(-1)
    al = ex / z[..., None]
    mean, ex2, Eabs = (al * x).sum(-1), (al * x * x).sum(-1), (al * x.abs()).sum(-1)
    xc = x - mean[..., None]
    var = (al * xc * xc).sum(-1)
    # one weight error serves z, s1 and s2 alike: alpha' <= alpha (1 + w) / (1 - wbar), |alpha' - alpha| <= alpha ww
    wbar = (al * w).sum(-1)
    ww = (w + wbar[..., None]) / (1 - wbar).clamp_min(TINY)[..., None]
    rho = (2 * _en(nsum) + 3 * U) * 1.001          # the sums' own roundings, the products, the division
    fl = n * FLUSH
    d_z = (ex * w).sum(-1) + _en(nsum) * z + fl
    dmw = (al * xc.abs() * ww).sum(-1)
    d_mean = dmw + rho * Eabs + fl * x.abs().amax(-1) + TINY
    d_ex2 = (al * x * x * ww).sum(-1) + rho * ex2 + fl * (x * x).amax(-1) + TINY
    am = mean.abs() + dmw
    d_var = (al * xc * xc * ww).sum(-1) + dmw ** 2 + rho * ex2 + 2 * am * rho * Eabs + (rho * Eabs) ** 2 + 2 * U * (ex2 + am * am) + fl * (x * x).amax(-1) + TINY
    return dict(z=z, mean=mean, ex2=ex2, var=var, d_z=d_z, d_mean=d_mean, d_ex2=d_ex2, d_var=d_var)


def _std_iv(var, d_var, floor=FLOOR32):
    lo = torch.sqrt((var - d_var).clamp_min(floor)) * (1 - 2 * U)
    hi = torch.sqrt((var + d_var).clamp_min(floor)) * (1 + 2 * U)
    return _iv(lo, hi)


def _mh_errs(sp, t, ntiles):
    """float64 attention of the case and the docstring's error terms: dict(X, hid, Lr, Lk, d_h, d_Lr, d_Lk)."""
    R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
    X, hid, Lr, Lk = _mh_attention(sp, t, F64)
    W1, b1, W2, b2 = _mh_blocks(sp, t, F64)
    d_z1 = eps_for(False, dm + 1) * (torch.einsum("rhtk,qhuk->rqhtu", X.abs(), W1.abs()) + b1.abs()[None, :, :, None, :])
    if layers == 2:
        d_h = d_z1 + D_TANH * hid.abs() + TINY
        d_Lr = torch.einsum("rqhtu,qhiu->rqhti", d_h, W2.abs()) + eps_for(False, 65) * (
            torch.einsum("rqhtu,qhiu->rqhti", hid.abs(), W2.abs()) + b2.abs()[None, :, :, None, :])
    else:
        d_h, d_Lr = d_z1, d_z1
    d_Lk = d_Lr.expand(R, Q, H, T, dm) if ds == 1 else d_Lr[..., mh_nat(F_, Ch)]
    return dict(X=X, hid=hid, Lr=Lr, Lk=Lk, d_h=d_h, d_Lr=d_Lr, d_Lk=d_Lk, W1=W1, W2=W2)


def reference(b, tensors=None, entry=None):
    """name -> Ref | Partial of every output of the built case over `tensors` (default: the case's own buffers)."""
    e, sp = entry or b.case.entry, b.spec
    t = b.views(tensors or b.bufs)
    v = compute(e, sp, t, F64)
    if e in ("tstp_fwd", "tstp_fwd_len"):
        R = sp["R"]
        p = _tstp_parts(e, sp, t, F64, "seq")
        n = p["cnt"]
        d_m = _en(n) * p["absmean"] + TINY
        e2 = _en(n + 3)
        den = (n - 1).clamp_min(1)
        eps = float(_f32(sp["eps"]))
        lo = torch.sqrt((p["m2"] * (1 - e2)).clamp_min(0) / den + eps) * (1 - 3 * U)
        hi = torch.sqrt((p["m2"] + n * d_m ** 2) * (1 + e2) / den + eps) * (1 + 3 * U)
        sv, sb = _iv(lo, hi)
        fl = lambda q: q.permute(0, 2, 1).reshape(R, -1)          # noqa: E731
        return {"stats": _R(torch.stack([fl(p["mean"]), fl(sv)], 1), torch.stack([fl(d_m.expand_as(p["mean"])), fl(sb)], 1))}
    if e in ("astp_fwd", "astp_fwd_len"):
        p = _astp_parts(e, sp, t, F64, "seq")
        dz = U * torch.where(p["mask"], (p["lg"] - p["m"][..., None]).abs(), torch.zeros((), dtype=F64))
        mb = _moment_bounds(p["e"], p["x"], D_EXP + torch.expm1(dz) + U, p["cnt"], p["cnt"] + 1)
        sv, sb = _std_iv(mb["var"], mb["d_var"])
        zero = torch.zeros_like(mb["z"])
        return {"out": _R(torch.cat([mb["mean"], sv], 1), torch.cat([mb["d_mean"], sb], 1)),
                "aux": _R(v["aux"], torch.stack([zero, mb["d_z"], mb["d_mean"], mb["d_ex2"]], 1),
                          torch.stack([torch.ones_like(zero, dtype=torch.bool)] + [torch.zeros_like(zero, dtype=torch.bool)] * 3, 1))}
    if e == "astp_bwd":
        R, T, C = sp["R"], sp["T"], sp["C"]
        x, lg = (t[k][:R * T * C].reshape(R, T, C).double() for k in ("x", "lg"))
        aux, out, do = (t[k].double() for k in ("aux", "out", "dout"))
        aux, out, do = aux[:R * 4 * C].reshape(R, 4, C), out[:R * 2 * C].reshape(R, 2, C), do[:R * 2 * C].reshape(R, 2, C)
        m, z, mean, ex2 = (aux[:, i][:, None] for i in range(4))
        taken, amb = _astp_branch(t["aux"][:R * 4 * C].reshape(R, 4, C))
        res = {}
        for key in ("dx", "dlg"):
            val, bd = None, None
            for br in (taken, ~taken):
                vv = compute(e, dict(sp, branch=br), t, F64)[key]
                gv = torch.where(br, do[:, 1] / (2 * out[:, 1]), torch.zeros((), dtype=F64))[:, None].abs()
                al = torch.exp(lg - m) / z
                w = D_EXP + torch.expm1(U * (lg - m).abs()) + U
                G = do[:, 0][:, None].abs() + 2 * mean.abs() * gv
                if key == "dx":
                    bb = (w + E0) * al * (G + 2 * gv * x.abs())
                else:
                    bb = (w + eps_for(False, 4)) * al * (G * (x.abs() + mean.abs()) + gv * (x * x + ex2))
                bb = bb + TINY
                if val is None:
                    val, bd = vv, bb
                else:          # the hull of both branches where the fp32 test is ambiguous
                    a2 = amb[:, None].expand_as(vv)
                    lo, hi = torch.minimum(val - bd, vv - bb), torch.maximum(val + bd, vv + bb)
                    val, bd = torch.where(a2, (lo + hi) / 2, val), torch.where(a2, (hi - lo) / 2, bd)
            res[key] = _R(val, bd)
        return res
    if e == "seg_sums":
        R, T, C, sl = sp["R"], sp["T"], sp["C"], sp["seg_len"]
        nseg = -(-T // sl)
        S = compute(e, sp, {k: x.abs() for k, x in t.items()}, F64)["out"]
        cnt = torch.tensor([min(T, (s + 1) * sl) - s * sl for s in range(nseg)], dtype=F64)[None, :, None].expand(R, nseg, C)
        ex = (cnt == 1) & (not sp["b"])
        return {"out": _R(v["out"], _en(cnt + 1) * S, ex, S)}
    if e == "seg_scale":
        if not sp["x"]:
            return {"out": _exact(v["out"])}
        return {"out": _R(v["out"], U * v["out"].abs() * (1 + U) + TINY)}
    if e in ("preemph_pad", "preemph_pad_len"):
        R, T, pad, ldo = sp["R"], sp["T"], sp["pad"], sp["ldo"]
        val, live, a, cb = _preemph(e, sp, t, F64)
        idx = _ar(R)[:, None] * ldo + _ar(T + 2 * pad)[None, :]
        bd = torch.where(live, 2 * U * (a.abs() + cb.abs()) + TINY, torch.zeros((), dtype=F64))
        ex = ~live | torch.full(live.shape, float(_f32(sp["coef"])) == 0.0)
        return {"out": _R(val, bd, ex, idx=idx)}
    if e == "power_spec":
        M, nf, ldp = sp["M"], sp["nf"], sp["ldp"]
        ex = torch.zeros(M, ldp, dtype=torch.bool)
        ex[:, nf:] = True
        return {"p": _R(v["p"], 4 * U * v["p"] + TINY, ex)}
    if e == "log_eps":
        return {"x": _R(v["x"], U * (1 + 4 * U) + D_LOG * v["x"].abs())}
    if e == "bn_prelu_fwd_len":
        R, rpr, W, C = sp["R"], sp["rpr"], sp["W"], sp["C"]
        M = R * rpr
        x = t["x"][:M * C].reshape(M, C).double()
        st = t["stats"][:2 * C].reshape(2, C).double()
        S = ((x - st[0]) * st[1] * t["gamma"][:C].double()).abs() + t["beta"][:C].double().abs()
        if sp["res"]:
            S = S + t["res"][:M * C].reshape(M, C).double().abs()
        m = _ar(M)
        valid = ((m % W) < lens(e, sp)[m // rpr])[:, None].expand(M, C)
        S = torch.where(valid, S, torch.zeros((), dtype=F64))
        return {"u": _R(v["u"], E0 * S + TINY, ~valid, S), "y": _R(v["y"], E0 * S * max(1.0, abs(float(t["a"][0]))) + TINY, ~valid, S)}
    if e in ("time_mean_len", "cmn_len", "tail_select_len"):
        R, T, C = sp["R"], sp["T"], sp["C"]
        if e == "tail_select_len":
            return {"y": _exact(v["y"])}
        n = lens(e, sp)
        mask = _tmask(T, n)[:, :, None]
        x = t["x"][:R * T * C].reshape(R, T, C).double()
        nn = n.double()[:, None]
        d_m = _en(nn) * torch.where(mask, x.abs(), torch.zeros((), dtype=F64)).sum(1) / nn + TINY
        if e == "time_mean_len":
            return {"mean": _R(v["mean"], d_m)}
        live = mask.expand(R, T, C)
        return {"y": _R(v["y"], torch.where(live, d_m[:, None] + U * v["y"].abs(), torch.zeros((), dtype=F64)), ~live)}
    if e == "mhastp_pack":
        return {"blk": _exact(v["blk"])}
    if e in ("mhastp_fwd", "mhastp_fwd_split"):
        R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
        split = e == "mhastp_fwd_split"
        ntl = -(-T // sp["TTf"]) + (sp["tsplit"] if split else 1)
        a = _mh_errs(sp, t, ntl)
        Lk, X = a["Lk"].permute(0, 1, 2, 4, 3), a["X"][:, None].permute(0, 1, 2, 4, 3)          # [R, Q, H, dm, T]
        d_L = a["d_Lk"].permute(0, 1, 2, 4, 3)
        m = Lk.amax(-1, keepdim=True)
        d_max = d_L.amax(-1, keepdim=True)
        w = D_EXP + torch.expm1(d_L + d_max + U * (Lk - m).abs()) + ntl * (D_EXP + 3 * U) + U * (m - Lk).abs() + U
        mb = _moment_bounds(torch.exp(Lk - m), X.expand_as(Lk), w, T, T + ntl)
        sv, sb = _std_iv(mb["var"], mb["d_var"])
        nat = mh_nat(F_, Ch)
        oval, obd = torch.zeros(R, Q, H, 2, dm, dtype=F64), torch.zeros(R, Q, H, 2, dm, dtype=F64)
        oval[..., 0, nat], oval[..., 1, nat], obd[..., 0, nat], obd[..., 1, nat] = mb["mean"], sv, mb["d_mean"], sb
        aval = torch.stack([m[..., 0], mb["z"], mb["mean"], mb["var"]], 3)
        abd = torch.stack([d_max[..., 0] + TINY, mb["d_z"], mb["d_mean"], mb["d_var"]], 3)
        out = {"out": _R(oval, obd), "aux": _R(aval, abd)}
        if split:
            idx, val = _mh_empty_part(sp, sp["tsplit"])
            out["part"] = _exact(val, idx)
        return out
    if e in ("mhastp_bwd", "mhastp_bwd_split"):
        return _ref_mh_bwd(sp, t, v)
    raise ValueError(e)


def _ref_mh_bwd(sp, t, v):
    R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
    nat = mh_nat(F_, Ch)
    a = _mh_errs(sp, t, 0)
    X, hid, Lr, Lk, W1, W2 = a["X"], a["hid"], a["Lr"], a["Lk"], a["W1"].abs(), (a["W2"].abs() if layers == 2 else None)
    aux = t["aux"][:R * Q * H * 4 * dm].reshape(R, Q, H, 4, dm).double()
    m, s, mean, var = (aux[:, :, :, i][:, :, :, None] for i in range(4))
    go = t["dout"][:R * Q * H * 2 * dm].reshape(R, Q, H, 2, dm).double()
    dmean, dstd = go[:, :, :, 0][..., nat][:, :, :, None].abs(), go[:, :, :, 1][..., nat][:, :, :, None]
    keep = var >= FLOOR32
    dvar = torch.where(keep, 0.5 * dstd / torch.sqrt(torch.where(keep, var, torch.ones_like(var))), torch.zeros((), dtype=F64)).abs()
    xv = X[:, None]
    al = torch.exp(Lk - m) / s
    w = D_EXP + torch.expm1(a["d_Lk"] + U * (Lk - m).abs()) + 3 * U
    S_A = dmean + 2 * dvar * (xv - mean).abs()
    d_direct = al * S_A * (w + E0) + TINY
    S_g = xv.abs() * (dmean + dvar * (xv.abs() + 2 * mean.abs())) + dmean * mean.abs() + dvar * (var.abs() + mean * mean)
    e4 = eps_for(False, 4)
    # the values of the float64 run, in the layouts of compute
    rows = lambda q: q.permute(0, 3, 1, 2, 4).reshape(R * T, Q, H, -1)          # noqa: E731
    if ds == 1:
        al0 = torch.exp(Lr[..., 0] - m[..., 0, 0:1]) / s[..., 0, 0:1]
        w0 = D_EXP + torch.expm1(a["d_Lr"][..., 0] + U * (Lr[..., 0] - m[..., 0, 0:1]).abs()) + 3 * U
        S_dl = (al0 * S_g.sum(-1))[..., None]
        d_dl = S_dl * (w0[..., None] + eps_for(False, dm + 4)) + TINY
    else:
        S_dl, d_dl = torch.zeros_like(Lk), torch.zeros_like(Lk)
        S_dl[..., nat], d_dl[..., nat] = al * S_g, al * S_g * (w + e4) + TINY
    # dl, dz of the float64 run (recomputed: compute() hands them over only with wgrad)
    full = compute("mhastp_bwd", dict(sp, wgrad=1, nsplit=1), t, F64)
    wz = full["work"][:R * T * Q * H * n1].reshape(R, T, Q, H, n1).permute(0, 2, 3, 1, 4)
    if layers == 2:
        o = R * T * Q * H * n1
        dl = full["work"][o + R * T * Q * H * 64:].reshape(R, T, Q, H, ds).permute(0, 2, 3, 1, 4)
        S_acc = torch.einsum("rqhti,qhiu->rqhtu", S_dl, W2)
        d_acc = torch.einsum("rqhti,qhiu->rqhtu", d_dl, W2) + eps_for(False, ds + 1) * S_acc
        g = (1 - hid * hid).abs()
        d_g = 2 * hid.abs() * a["d_h"] + a["d_h"] ** 2 + 2 * U
        d_wz = d_acc * (g + d_g) + S_acc * d_g + U * S_acc * g + TINY
        S_wz = S_acc * g
    else:
        dl, d_wz, S_wz = wz, d_dl, S_dl
    S_back = torch.einsum("rqhtu,qhuk->rqhtk", S_wz, W1)
    d_back = torch.einsum("rqhtu,qhuk->rqhtk", d_wz, W1) + eps_for(False, n1 + 1) * S_back
    S_dx = (al * S_A + S_back).sum(1)
    d_dx = (d_direct + d_back).sum(1) + eps_for(False, 2 * Q) * S_dx + TINY
    out = {"dx": _R(v["dx"], _mh_unx(sp, d_dx), S=_mh_unx(sp, S_dx))}
    if not sp["wgrad"]:
        return out
    wparts, wb = [rows(wz).reshape(-1)], [rows(d_wz.expand_as(wz)).reshape(-1)]
    if layers == 2:
        wparts += [rows(hid).reshape(-1), rows(dl).reshape(-1)]
        wb += [rows(a["d_h"]).reshape(-1), rows(d_dl.expand_as(dl)).reshape(-1)]
    out["work"] = _R(v["work"], torch.cat(wb) + U * torch.cat(wparts).abs())
    M, ns = R * T, sp["nsplit"]
    eM = eps_for(False, M + 1)
    Xm = X.permute(0, 2, 1, 3).reshape(M, H, dm).abs()
    dgz, gza = rows(d_wz.expand_as(wz)), rows(wz).abs()
    S = torch.zeros(Q, H, P1, dtype=F64)
    bd = torch.zeros(Q, H, P1, dtype=F64)
    sW1 = torch.einsum("mqhu,mhk->qhuk", gza, Xm)
    bW1 = torch.einsum("mqhu,mhk->qhuk", dgz, Xm) + eM * sW1
    blkS, blkB = torch.zeros(Q, H, n1, dm, dtype=F64), torch.zeros(Q, H, n1, dm, dtype=F64)
    blkS[..., nat], blkB[..., nat] = sW1, bW1
    S[..., :n1 * dm], bd[..., :n1 * dm] = blkS.reshape(Q, H, -1), blkB.reshape(Q, H, -1)
    S[..., n1 * dm:off2], bd[..., n1 * dm:off2] = gza.sum(0), dgz.sum(0) + eM * gza.sum(0)
    if layers == 2:
        ha, dh = rows(hid).abs(), rows(a["d_h"])
        la, dla = rows(dl).abs(), rows(d_dl.expand_as(dl))
        sW2 = torch.einsum("mqhi,mqhu->qhiu", la, ha)
        bW2 = torch.einsum("mqhi,mqhu->qhiu", dla, ha + dh) + torch.einsum("mqhi,mqhu->qhiu", la, dh) + eM * sW2
        S[..., off2:off2 + 64 * ds], bd[..., off2:off2 + 64 * ds] = sW2.reshape(Q, H, -1), bW2.reshape(Q, H, -1)
        S[..., off2 + 64 * ds:], bd[..., off2 + 64 * ds:] = la.sum(0), dla.sum(0) + eM * la.sum(0)
    S, bd = S.reshape(-1), bd.reshape(-1) + TINY
    rps = mh_rps(sp)
    if ns > 1:
        out["slab"] = tc._slab_ref(v["slab"], S, bd, ns, lambda s_: s_ * rps >= M)
        out["dpack"] = _red_ref(v["dpack"], S, bd, ns)
    else:
        out["dpack"] = _R(v["dpack"], bd, S=S)
    return out


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, targets
# ------------------------------------------------------------------------------------------------------------
POOL_C, POOL_T = [1, 3, 64, 65, 257], [1, 2, 3, 64, 257]
REG_STATS = ["gauss", "offset", "const"]
REG_LOGIT = REG_STATS + ["rising", "peak_last", "peak_first"]
REG_FLOOR = ["floor_above", "floor_below"]
TABS = ["full", "mixed", "clamped"]
MH_GEO = [(1, 1), (3, 1), (7, 9), (8, 8), (5, 13), (10, 8), (5, 51), (16, 16), (1, 257), (10, 32), (8, 64)]          # dm 1 .. 512
MH_GEO_SPLIT = [(3, 1), (5, 13), (16, 16)]
MH_TS = ["1", "2", "TT-1", "TT", "TT+1", "2TT+1"]
# every lane-split factor of mh_stage1 at layers 1, ds = dm: n1 = dm
KS_GEO = [(1, 1), (1, 2), (2, 2), (5, 1), (2, 4), (3, 3), (4, 4), (17, 1), (4, 8), (3, 11), (8, 8), (5, 13), (8, 16), (3, 43), (16, 16), (1, 257)]
_MH = dict(geo=MH_GEO, T=MH_TS, layers=[1, 2], dsk=["1", "dm"], Q=[1, 2, 3], H=[1, 2, 4], R=[1, 2], regime=REG_LOGIT)
_MHS = dict(geo=MH_GEO_SPLIT, T=[2, 9, 17, 33], tsplit=["1", "2", "T"], layers=[1, 2], dsk=["1", "dm"], Q=[1, 2], H=[1, 2], R=[1, 2],
            regime=["gauss", "rising", "peak_last", "peak_first"])
DIMS = {
    "tstp_fwd": dict(C=POOL_C, T=POOL_T, F=[1, 2, 5], R=[1, 3], regime=REG_STATS),
    "astp_fwd": dict(C=POOL_C, T=POOL_T, R=[1, 3], regime=REG_LOGIT),
    "astp_bwd": dict(C=POOL_C, T=POOL_T, R=[1, 3], regime=REG_LOGIT),
    "seg_sums": dict(seg_len=[1, 2, 3, 100], T=[1, 7, 100, 101, 199], b=[0, 1], C=[4, 12, 260], R=[1, 2]),
    "seg_scale": dict(seg_len=[1, 2, 3, 100], T=[1, 7, 100, 101, 199], x=[0, 1], alias=[0, 1], C=[4, 12, 260], R=[1, 2]),
    "preemph_pad": dict(pad=[0, 1, 3, 256], T=["2", "pad+1", "pad+2", "700"], ldo=["tight", "+5"], coef=[0.0, 0.97], R=[1, 3]),
    "power_spec": dict(nf=[1, 257], lds=["2nf", "2nf+2"], ldp=["nf", "nf+3"], M=[1, 5]),
    "log_eps": dict(n=[8, 257, 5000], eps=[1e-6]),
    "mhastp_pack": dict(geo=[(1, 1), (3, 1), (5, 13), (16, 16), (8, 64)], layers=[1, 2], dsk=["1", "dm"]),
    "mhastp_fwd": dict(_MH),
    "mhastp_bwd": dict(_MH, wg=["none", "1", "2", "3"]),
    "mhastp_fwd_split": dict(_MHS),
    "mhastp_bwd_split": dict(_MHS, wg=["none", "1", "3"]),
    "bn_prelu_fwd_len": dict(C=[4, 12, 64], W=[1, 5, 8], rpr=["2W", "4W"], R=[1, 3], res=[0, 1], slope=[0.0, 0.25, 1.0], tab=TABS),
    "tstp_fwd_len": dict(C=POOL_C, T=POOL_T, F=[1, 2, 5], R=[1, 3], regime=REG_STATS, tab=TABS),
    "astp_fwd_len": dict(C=POOL_C, T=POOL_T, R=[1, 3], regime=REG_LOGIT, tab=TABS),
    "time_mean_len": dict(C=[1, 63, 64, 65, 130], T=[1, 2, 5, 9], R=[1, 3], tab=TABS),
    "cmn_len": dict(C=[1, 63, 64, 65, 130], T=[1, 2, 5, 9], R=[1, 3], tab=TABS, alias=[0, 1]),
    "tail_select_len": dict(C=[4, 8, 260], T=[1, 3, 9], R=[1, 3], tab=TABS, alias=[0, 1]),
    "preemph_pad_len": dict(pad=[0, 1, 3, 256], T=["2", "pad+1", "pad+2", "700"], ldo=["tight", "+5"], coef=[0.0, 0.97], R=[1, 3], tab=TABS),
}
_PRE_RULES = [("T > 1 and T > pad", ("pad", "T"), lambda pad, T: pre_T({"pad": pad, "T": T}) < max(2, pad + 1))]
RULES = {e: [] for e in ENTRIES}
RULES["preemph_pad"] = RULES["preemph_pad_len"] = _PRE_RULES
RULES["seg_scale"] = [("out may alias x only where x is given", ("x", "alias"), lambda x, alias: alias and not x)]


def pre_T(d):
    return d["T"] if isinstance(d["T"], int) else {"2": 2, "pad+1": d["pad"] + 1, "pad+2": d["pad"] + 2, "700": 700}[d["T"]]


def mh_dims(entry, d):
    """(F, Ch, H, Q, R, layers, ds, dm, TT forward, TT backward, T, tsplit) of a MHASTP case."""
    F_, Ch = d["geo"]
    dm = F_ * Ch
    ds = 1 if d["dsk"] == "1" else dm
    L = d["layers"]
    ttf, ttb = mh_tt(dm, L, ds, False), mh_tt(dm, L, ds, True)
    tt = ttb if "bwd" in entry else ttf
    T = d["T"] if isinstance(d["T"], int) else {"1": 1, "2": 2, "TT-1": max(tt - 1, 1), "TT": tt, "TT+1": tt + 1, "2TT+1": 2 * tt + 1}[d["T"]]
    ts = d.get("tsplit")
    ts = None if ts is None else (ts if isinstance(ts, int) else {"1": 1, "2": min(2, T), "T": T}[ts])
    return F_, Ch, d["H"], d["Q"], d["R"], L, ds, dm, ttf, ttb, T, ts


def mh_nsplit(d, M):
    """Row splits of the weight gradients (0: none asked for)."""
    wg = d.get("wg", "none")
    return {"none": 0, "M+1": M + 1}[wg] if wg in ("none", "M+1") else int(wg)


def _targets(entry, d, seed=0):
    e = entry
    t = ({"time_mean_len": "row_mean_len_kernel<false>", "cmn_len": "row_mean_len_kernel<true>"}.get(e, e + "_kernel"),)
    if e in ("tstp_fwd", "tstp_fwd_len"):
        t += ("%s[T = 1]" % e,) if d["T"] == 1 else ()
        t += ("%s[second block]" % e,) if d["R"] * d["F"] * d["C"] > 256 else ()
    elif e in ("astp_fwd", "astp_fwd_len", "astp_bwd"):
        t += ("%s[T = 1]" % e,) if d["T"] == 1 else ()
        t += ("%s[clamp]" % e,) if d["regime"] in ("const", "floor_below", "floor_eq") or d["T"] == 1 else ()
        t += ("%s[second block]" % e,) if d["R"] * d["C"] * (d["T"] if e == "astp_bwd" else 1) > 256 else ()
    elif e == "seg_sums":
        T, sl = d["T"], d["seg_len"]
        t += ("seg_sums[b NULL]",) if not d["b"] else ()
        t += ("seg_sums[short last segment]",) if T % sl and T > sl else ()
        t += ("seg_sums[seg_len > T]",) if sl > T else ()
        t += ("seg_sums[odd frame]",) if min(sl, T) % 2 or (T % sl) % 2 else ()
    elif e == "seg_scale":
        t += ("seg_scale[x NULL]",) if not d["x"] else ()
        t += ("seg_scale[in place]",) if d["alias"] else ()
    elif e in ("preemph_pad", "preemph_pad_len"):
        t += ("%s[pad = 0]" % e,) if d["pad"] == 0 else ()
        t += ("%s[T = pad + 1]" % e,) if pre_T(d) == d["pad"] + 1 else ()
        t += ("%s[ldo above T + 2 pad]" % e,) if d["ldo"] != "tight" else ()
        t += ("%s[coef = 0]" % e,) if d["coef"] == 0.0 else ()
    elif e == "power_spec":
        t += ("power_spec[zeroed columns]",) if d["ldp"] != "nf" else ()
        t += ("power_spec[lds above 2 nf]",) if d["lds"] != "2nf" else ()
    elif e == "bn_prelu_fwd_len":
        t += ("bn_prelu_fwd_len[res]",) if d["res"] else ()
        t += ("bn_prelu_fwd_len[rows_per_r = 4 W]",) if d["rpr"] == "4W" else ()
    elif e in ("time_mean_len", "cmn_len"):
        t += ("%s[second channel block]" % e,) if d["C"] > 64 else ()
        t += ("%s[in place]" % e,) if d.get("alias") else ()
    elif e == "tail_select_len":
        t += ("tail_select_len[in place]",) if d["alias"] else ()
        t += ("tail_select_len[grid cap]",) if d["R"] * d["T"] * d["C"] // 4 > 32768 * 256 else ()
    elif e in MH_ENTRIES and e != "mhastp_pack":
        F_, Ch, H, Q, R, L, ds, dm, ttf, ttb, T, ts = mh_dims(e, d)
        tt = ttb if "bwd" in e else ttf
        n1 = mh_n1(L, ds)
        t += ("%s[layers %d]" % (e, L), "%s[ds = %s]" % (e, "1" if ds == 1 and d["dsk"] == "1" else "dm"))
        t += ("%s[partial tile]" % e,) if T % tt else ()
        t += ("%s[several tiles]" % e,) if T > tt else ()
        t += ("%s[second feature pass]" % e,) if dm > MH_THREADS else ()
        t += ("%s[second u0 pass]" % e,) if n1 > MH_THREADS // mh_ks(n1) else ()
        t += ("%s[several queries]" % e,) if Q > 1 else ()
        if ts is not None:
            t += ("%s[empty T split]" % e,) if (ts - 1) * -(-T // ts) >= T else ()
            t += ("%s[tsplit = 1]" % e,) if ts == 1 else ()
        if "bwd" in e:
            M = R * T
            ns = mh_nsplit(d, M)
            t += ("%s[no weight gradients]" % e,) if not ns else ()
            t += ("%s[one row split]" % e,) if ns == 1 else ()
            t += ("%s[slab]" % e,) if ns > 1 else ()
            t += ("%s[empty row split]" % e,) if ns > 1 and (ns - 1) * -(-M // ns) >= M else ()
            t += ("%s[bias column in a tile of its own]" % e,) if ns and dm % 64 == 0 else ()
    return t


_M = gc.MIN_PER_TARGET


def _topups(e):
    d0 = {k: v[0] for k, v in DIMS[e].items()}
    t = [({}, _targets(e, d0)[0], _M)]
    add = lambda fixed, tag, n=_M: t.append((fixed, f"{e}[{tag}]", n))          # noqa: E731
    if e in ("tstp_fwd", "tstp_fwd_len"):
        add({"T": 1}, "T = 1"), add({"C": 257, "R": 3}, "second block")
    if e in ("astp_fwd", "astp_fwd_len", "astp_bwd"):
        add({"T": 1}, "T = 1"), add({"regime": "const"}, "clamp"), add({"C": 257, "R": 3}, "second block")
    if e == "seg_sums":
        add({"b": 0}, "b NULL"), add({"T": 101, "seg_len": 3}, "short last segment", 1), add({"T": 199}, "short last segment")
        add({"seg_len": 100, "T": 7}, "seg_len > T", 1), add({"seg_len": 100}, "seg_len > T"), add({"seg_len": 3}, "odd frame")
    if e == "seg_scale":
        add({"x": 0, "alias": 0}, "x NULL"), add({"x": 1, "alias": 1}, "in place")
    if e in ("preemph_pad", "preemph_pad_len"):
        add({"pad": 0}, "pad = 0"), add({"T": "pad+1"}, "T = pad + 1"), add({"ldo": "+5"}, "ldo above T + 2 pad"), add({"coef": 0.0}, "coef = 0")
    if e == "power_spec":
        add({"ldp": "nf+3"}, "zeroed columns"), add({"lds": "2nf+2"}, "lds above 2 nf")
    if e == "bn_prelu_fwd_len":
        add({"res": 1}, "res"), add({"rpr": "4W"}, "rows_per_r = 4 W")
    if e in ("time_mean_len", "cmn_len"):
        add({"C": 130}, "second channel block")
    if e in ("cmn_len", "tail_select_len"):
        add({"alias": 1}, "in place")
    if e in MH_ENTRIES and e != "mhastp_pack":
        add({"layers": 1}, "layers 1"), add({"layers": 2}, "layers 2"), add({"dsk": "1", "geo": (5, 13)}, "ds = 1"), add({"dsk": "dm", "geo": (8, 8)}, "ds = dm")
        big = MH_GEO[-1] if e in ("mhastp_fwd", "mhastp_bwd") else (16, 16)
        if e in ("mhastp_fwd", "mhastp_bwd"):
            add({"T": "TT+1"}, "partial tile"), add({"T": "2TT+1"}, "several tiles")
            add({"geo": big}, "second feature pass"), add({"geo": big, "layers": 1, "dsk": "dm"}, "second u0 pass", 2)
        else:
            add({"T": 17}, "partial tile"), add({"T": 33, "tsplit": "1"}, "several tiles"), add({"tsplit": "1"}, "tsplit = 1")
        add({"Q": 2}, "several queries")
        if "bwd" in e:
            add({"wg": "none"}, "no weight gradients"), add({"wg": "1"}, "one row split"), add({"wg": "3"}, "slab")
            add({"wg": "3", "geo": (8, 8) if e == "mhastp_bwd" else (16, 16)}, "bias column in a tile of its own", 2)
    return t


TOPUP = {e: _topups(e) for e in ENTRIES}
INST = {e: list(dict.fromkeys(tag for _, tag, _ in TOPUP[e])) for e in ENTRIES}
for _e in ("mhastp_fwd_split", "mhastp_bwd_split"):
    INST[_e].append(f"{_e}[empty T split]")
for _e in ("mhastp_bwd", "mhastp_bwd_split"):
    INST[_e].append(f"{_e}[empty row split]")
for _e in ("mhastp_fwd", "mhastp_bwd"):
    INST[_e] += [f"{_e}[second u0 pass]"] if f"{_e}[second u0 pass]" not in INST[_e] else []
# targets that hand-written cases of EXTRA reach (counted, not topped up)
MIN_COUNT = {f"{e}[{k}]": 1 for e in MH_ENTRIES for k in ("empty T split", "empty row split", "second u0 pass", "bias column in a tile of its own")}
_X = dict(layers=1, dsk="dm", Q=1, H=2, R=1, regime="gauss")
_BIG = dict(layers=2, dsk="dm", Q=1, H=1, R=1, regime="gauss", T=3)
_SPL = dict(geo=(5, 13), layers=2, dsk="dm", Q=2, H=2, regime="gauss")
_FLR = dict(geo=(3, 1), T="2TT+1", Q=2, H=2, R=1)
EXTRA = {
    "mhastp_fwd": [dict(_X, geo=g, T="TT+1") for g in KS_GEO] + [dict(_BIG, geo=(10, 272)), dict(_BIG, geo=(10, 408))],
    # (the lane-split sweep carries the row splits of the weight gradients: M = R T in {5, 17, 33} x nsplit in {1, 2, 3, M + 1})
    "mhastp_bwd": [dict(_X, geo=g, T=(5, 17, 33)[i % 3], wg=("1", "2", "3", "M+1")[i % 4]) for i, g in enumerate(KS_GEO)] + [
        dict(_BIG, geo=(10, 272), wg="1"), dict(_BIG, geo=(10, 408), wg="none")] + [
        dict(_FLR, regime=r, layers=L, dsk=k, wg=w) for r in REG_FLOOR + ["floor_eq"] for L, k, w in ((1, "dm", "none"), (2, "1", "2"))],
    "astp_bwd": [dict(C=C, T=T, R=R, regime=r) for r in REG_FLOOR + ["floor_eq"] for C, T, R in ((3, 4, 1), (65, 64, 3))],
    "astp_fwd": [dict(C=3, T=4, R=1, regime=r) for r in REG_FLOOR],
    "mhastp_fwd_split": [dict(_SPL, R=1, T=9, tsplit=4), dict(_SPL, R=2, T=9, tsplit=4, layers=1, dsk="1", regime="peak_last")],
    "mhastp_bwd_split": [dict(_SPL, R=1, T=9, tsplit=4, wg="M+1"), dict(_SPL, R=2, T=9, tsplit=4, layers=1, dsk="1", wg="2")],
    # lengths below two samples at pad = 0 with a live coefficient: L = 2, x[r][2:] is never read (tabv: the table itself)
    "preemph_pad_len": [dict(pad=0, T=T, ldo=ldo, coef=0.97, R=3, tab="clamped", tabv=(1, 0, -5)) for T, ldo in ((5, "tight"), (700, "+5"))],
}
GRID_CAP_CASE = Case("tail_select_len", "grid-cap", dict(C=4, T=1198373, R=7, tab="mixed", alias=0), ("tail_select_len_kernel", "tail_select_len[grid cap]"), 9100)
_KEY = {e: "pool_" + e for e in ENTRIES}          # the registries of gemm_contract are shared by every suite
for _i, _e in enumerate(ENTRIES):
    gc.DIMS[_KEY[_e]], gc.RULES[_KEY[_e]], gc.INST[_KEY[_e]], gc.TOPUP[_KEY[_e]] = DIMS[_e], RULES[_e], INST[_e], TOPUP[_e]
    gc.SEEDS[_KEY[_e]] = 301 + _i
    gc.PLANNERS[_KEY[_e]] = (lambda e: lambda d, seed: _targets(e, d, seed))(_e)
_CASES = {}


def cases(entry):
    if entry not in _CASES:
        out = [c._replace(entry=entry) for c in gc.cases(_KEY[entry])]
        for i, d in enumerate(EXTRA.get(entry, [])):
            out.append(Case(entry, f"x{i:02d}-" + "-".join("x".join(str(q) for q in v) if isinstance(v, tuple) else str(v) for v in d.values()), d,
                            _targets(entry, d), 9000 + i))
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
def make_table(kind, R, lo, hi, seed=0):
    """The raw table of a case: full = hi everywhere; mixed = the short and the long rows in range; clamped = entries the
    header says are clamped (0, -5, hi + 7) next to ordinary ones."""
    if kind == "full":
        return [hi] * R
    pool = [lo, lo + 1, lo + 2, lo + 3, lo + 4, hi - 1, hi]
    pool = [min(max(v, lo), hi) for v in pool]
    tab = [pool[(seed + 3 * r) % len(pool)] for r in range(R)]
    if kind == "clamped":
        bad = [0, -5, hi + 7, 1]
        tab = [bad[(seed + r) % 4] if r % 2 == 0 else tab[r] for r in range(R)]
    return tab


def _floor_pattern(T, target):
    """x over t with mean 0 exactly and E[x^2] = target under uniform weights: (a, -a, b, -b, 0, ...)."""
    x = torch.zeros(T, dtype=F64)
    if T >= 4:
        b2 = T * target / 4
        x[2], x[3] = math.sqrt(b2), -math.sqrt(b2)
        x[2:4] = x[2:4].float().double()
        a2 = T * target / 2 - float(x[2]) ** 2
    else:
        a2 = T * target / 2
    if T >= 2:
        x[0], x[1] = math.sqrt(max(a2, 0.0)), -math.sqrt(max(a2, 0.0))
    return x.float()


def _floor_eq_pattern(T):
    """The pattern whose E[x^2], rounded to fp32, IS the floor: scan a's neighbours."""
    x = _floor_pattern(T, FLOOR32).double()
    a = x[0].float()
    for _ in range(2):
        for cand in [a] + [torch.nextafter(a, torch.tensor(s * math.inf)) for s in (1.0, -1.0)]:
            c = cand
            for _step in range(200):
                xx = x.clone()
                xx[0], xx[1] = c.double(), -c.double()
                if float(((xx * xx).sum() / T).float()) == FLOOR32:
                    return xx.float()
                c = torch.nextafter(c, torch.tensor(math.inf if float(cand) >= float(a) else -math.inf))
    raise AssertionError("no fp32 amplitude gives E[x^2] == the floor")


def _floor_x(T, regime):
    if regime == "floor_eq":
        return _floor_eq_pattern(T)
    return _floor_pattern(T, FLOOR * (1.02 if regime == "floor_above" else 0.98))


def _profile(T, regime, saturating):
    """g_t of the logit regimes (the logit moves by gain * g_t)."""
    t = _ar(T).double()
    if regime == "rising":
        return ((-2 + 4 * t / max(T - 1, 1)), 20.0) if saturating else (t / T, 0.5 * T)
    peak = T - 1 if regime == "peak_last" else 0
    if saturating:
        return torch.where(t == peak, 3.0, -3.0).double(), 60.0
    return (t == peak).double(), 120.0


def _stats_x(g, shape, taxis, regime):
    x = torch.randn(*shape, generator=g)
    if regime == "offset":
        x = x + 30.0
    if regime == "const":
        x = x.narrow(taxis, 0, 1).expand(*shape).contiguous()
    return x


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

    def table(lo, hi, R):
        if "tab" in d:
            sp["tab"] = list(d["tabv"]) if "tabv" in d else make_table(d["tab"], R, lo, hi, case.seed)

    if e in ("tstp_fwd", "tstp_fwd_len"):
        R, Fq, T, C = d["R"], d["F"], d["T"], d["C"]
        sp.update(R=R, F=Fq, T=T, C=C, eps=1e-7)
        table(1, T, R)
        x = _stats_x(g, (R, Fq, T, C), 2, d["regime"])
        inp("x", x, _tmask(T, lens(e, sp))[:, None, :, None].expand(R, Fq, T, C))
        out("stats", R * 2 * C * Fq)
        return b
    if e in ("astp_fwd", "astp_fwd_len", "astp_bwd"):
        R, T, C, reg = d["R"], d["T"], d["C"], d["regime"]
        sp.update(R=R, T=T, C=C, regime=reg)
        table(1, T, R)
        x = _stats_x(g, (R, T, C), 1, reg if reg in REG_STATS else "gauss")
        lg = rn(R, T, C)
        if reg in ("rising", "peak_last", "peak_first"):
            pr, gain = _profile(T, reg, False)
            lg = lg + (gain * pr).float()[None, :, None]
        if reg.startswith("floor"):
            x = (_floor_x(T, reg)[None, :, None] * torch.ones(R, T, C)).contiguous()
            lg = torch.zeros(R, T, C) + rn(R, 1, C)
        live = _tmask(T, lens(e, sp))[:, :, None].expand(R, T, C)
        inp("x", x, live)
        inp("lg", lg, live)
        if e != "astp_bwd":
            out("out", R * 2 * C)
            out("aux", R * 4 * C)
            return b
        f = compute("astp_fwd", sp, b.views(b.bufs), F64)
        inp("out", f["out"])
        inp("aux", f["aux"])
        inp("dout", rn(R, 2 * C))
        out("dx", R * T * C)
        out("dlg", R * T * C)
        return b
    if e in ("seg_sums", "seg_scale"):
        R, T, C, sl = d["R"], d["T"], d["C"], d["seg_len"]
        nseg = -(-T // sl)
        sp.update(R=R, T=T, C=C, seg_len=sl)
        if e == "seg_sums":
            sp["b"] = d["b"]
            inp("a", rn(R, T, C))
            if d["b"]:
                inp("b", rn(R, T, C) + 0.5)
            out("out", R * nseg * C)
            return b
        sp.update(x=d["x"], alias=d["alias"])
        inp("m", rn(R, nseg, C))
        if d["x"]:
            inp("x", rn(R, T, C))
        out("out", R * T * C, alias="x" if d["alias"] else None)
        return b
    if e in ("preemph_pad", "preemph_pad_len"):
        R, pad, T = d["R"], d["pad"], pre_T(d)
        ldo = T + 2 * pad + (5 if d["ldo"] == "+5" else 0)
        sp.update(R=R, T=T, pad=pad, ldo=ldo, coef=d["coef"])
        table(max(pad + 1, 2), T, R)
        inp("x", rn(R, T), _tmask(T, lens(e, sp)))
        out("out", R * ldo, _ar(R)[:, None] * ldo + _ar(T + 2 * pad)[None, :])
        return b
    if e == "power_spec":
        M, nf = d["M"], d["nf"]
        lds, ldp = 2 * nf + (2 if d["lds"] != "2nf" else 0), nf + (3 if d["ldp"] != "nf" else 0)
        sp.update(M=M, nf=nf, lds=lds, ldp=ldp)
        rd = torch.zeros(M, lds, dtype=torch.bool)
        rd[:, :2 * nf] = True
        inp("spec", rn(M, lds) * 3, rd)
        out("p", M * ldp)
        return b
    if e == "log_eps":
        n = d["n"]
        sp.update(n=n, eps=d["eps"])
        x = rn(n).abs() * torch.where(torch.rand(n, generator=g) < 0.3, 1e-4, 10.0)
        x[:5] = torch.tensor([0.0, 1e-41, 1e-30, 1.0, 1e30])
        inp("x", x)
        out("x", n, alias="x")
        return b
    if e == "bn_prelu_fwd_len":
        R, W, C = d["R"], d["W"], d["C"]
        rpr = W * (2 if d["rpr"] == "2W" else 4)
        sp.update(R=R, W=W, C=C, rpr=rpr, res=d["res"])
        table(0, W, R)
        M = R * rpr
        m = _ar(M)
        valid = ((m % W) < lens(e, sp)[m // rpr])[:, None].expand(M, C)
        inp("x", rn(M, C), valid)
        inp("stats", torch.stack([0.3 * rn(C), 0.5 + torch.rand(C, generator=g)]))
        inp("gamma", 1 + 0.2 * rn(C))
        inp("beta", 0.3 * rn(C))
        if d["res"]:
            inp("res", rn(M, C), valid)
        inp("a", torch.tensor([d["slope"]]))
        out("u", M * C)
        out("y", M * C)
        return b
    if e in ("time_mean_len", "cmn_len", "tail_select_len"):
        R, T, C = d["R"], d["T"], d["C"]
        sp.update(R=R, T=T, C=C)
        table(0 if e == "tail_select_len" else 1, T, R)
        x = rn(R, T, C) + 0.5 if T * C < (1 << 22) else torch.rand(R, T, C, generator=g)
        inp("x", x, _tmask(T, lens(e, sp))[:, :, None].expand(R, T, C))
        if e == "time_mean_len":
            out("mean", R * C)
        else:
            out("y", R * T * C, alias="x" if d["alias"] else None)
        return b
    if e == "mhastp_pack":
        F_, Ch = d["geo"]
        dm = F_ * Ch
        ds = 1 if d["dsk"] == "1" else dm
        n1 = mh_n1(d["layers"], ds)
        sp.update(F=F_, Ch=Ch, layers=d["layers"], ds=ds)
        inp("w1", rn(n1, dm))
        inp("b1", rn(n1))
        if d["layers"] == 2:
            inp("w2", rn(ds, 64))
            inp("b2", rn(ds))
        out("blk", mh_block_floats(d["layers"], ds, dm))
        return b
    if e in MH_ENTRIES:
        return _build_mh(b, e, d, g, inp, out)
    raise ValueError(e)


def mh_weights(g, sp, regime, vdir):
    """The parameters of every (query, head) as wespeaker shapes them: [(W1 [n1, dm] upstream column order, b1, W2, b2)]."""
    R, F_, T, Ch, Q, H, layers, ds, dm, n1, P1, off2 = _mh(sp)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    out = []
    for q in range(Q):
        for h in range(H):
            W1, b1 = rn(n1, dm) / math.sqrt(dm), 0.05 * rn(n1)
            # (dm above CAP exists to cross the one-frame tiles: a flat second layer keeps e(dm) away from the exponent)
            W2, b2 = (rn(ds, 64) / (8 if dm <= CAP else 64), 0.05 * rn(ds)) if layers == 2 else (None, None)
            if regime in ("rising", "peak_last", "peak_first"):
                vh = vdir[:, h * Ch:(h + 1) * Ch].t().reshape(-1)          # upstream order c F + f
                unit = vh / (vh * vh).sum().clamp_min(1e-6)
                _, gain = _profile(T, regime, layers == 2)
                if layers == 2:
                    W1[0], b1[0] = unit, 0.0
                    W2[:, 0] = gain
                else:
                    W1 = W1 + gain * unit[None, :]
            if regime.startswith("floor"):
                W1 = torch.zeros(n1, dm)
            out.append((W1, b1, W2, b2))
    return out


def mh_pack(sp, weights):
    """The pack of ws_mhastp_pack from upstream-shaped parameters."""
    nat = mh_nat(sp["F"], sp["Ch"])
    blocks = []
    for W1, b1, W2, b2 in weights:
        blocks += [W1[:, nat].reshape(-1), b1] + ([W2.reshape(-1), b2] if W2 is not None else [])
    return torch.cat(blocks)


def _build_mh(b, e, d, g, inp, out):
    sp = b.spec
    F_, Ch, H, Q, R, L, ds, dm, ttf, ttb, T, ts = mh_dims(e, d)
    reg = d["regime"]
    C = Ch * H
    sp.update(R=R, F=F_, T=T, Ch=Ch, C=C, Q=Q, H=H, layers=L, ds=ds, TTf=ttf, TTb=ttb, regime=reg)
    if ts is not None:
        sp["tsplit"] = ts
    x = _stats_x(g, (R, F_, T, C), 2, reg if reg in REG_STATS else "gauss")
    vdir = torch.randn(F_, C, generator=g)
    if reg in ("rising", "peak_last", "peak_first"):
        pr, _ = _profile(T, reg, L == 2)
        x = x + pr.float()[None, None, :, None] * vdir[None, :, None, :]
    if reg.startswith("floor"):
        x = (_floor_x(T, reg)[None, None, :, None] * torch.ones(R, F_, T, C)).contiguous()
    weights = mh_weights(g, sp, reg, vdir)
    sp["weights"] = weights
    inp("x", x)
    inp("pack", mh_pack(sp, weights))
    n_aux, n_out = R * Q * H * 4 * dm, R * Q * H * 2 * dm
    if e in ("mhastp_fwd", "mhastp_fwd_split"):
        out("out", n_out)
        out("aux", n_aux)
        if ts is not None:
            out("part", ts * n_aux)
        return b
    M = R * T
    ns = mh_nsplit(d, M)
    sp.update(wgrad=1 if ns else 0, nsplit=max(ns, 1))
    f = compute("mhastp_fwd", sp, b.views(b.bufs), F64)
    inp("aux", f["aux"])
    inp("dout", torch.randn(R, Q, H, 2, dm, generator=g))
    out("dx", R * F_ * T * C)
    if ns:
        P = Q * H * mh_block_floats(L, ds, dm)
        out("work", M * Q * H * (mh_n1(L, ds) + (64 + ds if L == 2 else 0)))
        if ns > 1:
            out("slab", ns * P)
        out("dpack", P)
    return b


# ------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------
def _tab(sp, device):
    return torch.tensor(sp["tab"], dtype=torch.int32, device=device)


def run(mod, b, tensors, device="cpu", entry=None, plain=False):
    """The case's call on `mod` (wesep_amd.dev) over `tensors` (the allocations on the device).  plain: the entry point
    without a table / without T splits (the bit-for-bit identities of the GPU file)."""
    e, sp, v = entry or b.case.entry, b.spec, b.views(tensors)
    if plain:
        e = e.replace("_len", "").replace("_split", "")
    if e == "tstp_fwd":
        mod.tstp_fwd(v["x"], sp["R"], sp["F"], sp["T"], sp["C"], v["stats"], eps=sp["eps"])
    elif e == "tstp_fwd_len":
        mod.tstp_fwd_len(v["x"], sp["R"], sp["F"], sp["T"], sp["C"], _tab(sp, device), v["stats"], eps=sp["eps"])
    elif e == "astp_fwd":
        mod.astp_fwd(v["x"], v["lg"], sp["R"], sp["T"], sp["C"], v["out"], v["aux"])
    elif e == "astp_fwd_len":
        mod.astp_fwd_len(v["x"], v["lg"], sp["R"], sp["T"], sp["C"], _tab(sp, device), v["out"], v["aux"])
    elif e == "astp_bwd":
        mod.astp_bwd(v["x"], v["lg"], v["out"], v["aux"], v["dout"], sp["R"], sp["T"], sp["C"], v["dx"], v["dlg"])
    elif e == "seg_sums":
        mod.seg_sums(v["a"], v.get("b"), sp["R"], sp["T"], sp["C"], sp["seg_len"], v["out"])
    elif e == "seg_scale":
        mod.seg_scale(v.get("x"), v["m"], sp["R"], sp["T"], sp["C"], sp["seg_len"], v["out"])
    elif e == "preemph_pad":
        mod.preemph_pad(v["x"], sp["R"], sp["T"], sp["pad"], sp["ldo"], sp["coef"], v["out"])
    elif e == "preemph_pad_len":
        mod.preemph_pad_len(v["x"], sp["R"], sp["T"], sp["pad"], sp["ldo"], sp["coef"], _tab(sp, device), v["out"])
    elif e == "power_spec":
        mod.power_spec(v["spec"], sp["M"], sp["nf"], sp["lds"], sp["ldp"], v["p"])
    elif e == "log_eps":
        mod.log_eps(v["x"], sp["eps"])
    elif e == "bn_prelu_fwd_len":
        mod.bn_prelu_fwd_len(v["x"], v["stats"], v["gamma"], v["beta"], v.get("res"), v["a"], sp["R"] * sp["rpr"], sp["C"], sp["rpr"], sp["W"],
                             _tab(sp, device), v["u"], v["y"])
    elif e == "bn_prelu_fwd":
        mod.bn_prelu_fwd(v["x"], v["stats"], v["gamma"], v["beta"], v.get("res"), v["a"], sp["R"] * sp["rpr"], sp["C"], v["u"], v["y"])
    elif e == "time_mean_len":
        mod.time_mean_len(v["x"], sp["R"], sp["T"], sp["C"], _tab(sp, device), v["mean"])
    elif e == "cmn_len":
        mod.cmn_len(v["x"], sp["R"], sp["T"], sp["C"], _tab(sp, device), v["y"])
    elif e == "tail_select_len":
        mod.tail_select_len(v["x"], sp["R"], sp["T"], sp["C"], _tab(sp, device), v["y"])
    elif e == "mhastp_pack":
        mod.mhastp_pack(v["w1"], v["b1"], v.get("w2"), v.get("b2"), sp["F"], sp["Ch"], sp["layers"], sp["ds"], v["blk"])
    elif e in ("mhastp_fwd", "mhastp_fwd_split"):
        a = (v["x"], v["pack"], sp["R"], sp["F"], sp["T"], sp["C"], sp["Q"], sp["H"], sp["layers"], sp["ds"], v["out"], v["aux"])
        if e == "mhastp_fwd":
            mod.mhastp_fwd(*a)
        else:
            mod.mhastp_fwd_split(*a, tsplit=sp["tsplit"], part=v["part"])
    elif e in ("mhastp_bwd", "mhastp_bwd_split"):
        a = (v["x"], v["pack"], v["aux"], v["dout"], sp["R"], sp["F"], sp["T"], sp["C"], sp["Q"], sp["H"], sp["layers"], sp["ds"], v["dx"])
        kw = dict(dpack=v["dpack"], nsplit=sp["nsplit"], work=v["work"], slab=v.get("slab")) if sp["wgrad"] else {}
        if e == "mhastp_bwd":
            mod.mhastp_bwd(*a, **kw)
        else:
            mod.mhastp_bwd_split(*a, tsplit=sp["tsplit"], **kw)
    else:
        raise ValueError(e)
    return {}


def refusals(dev, t, device="cpu"):
    """(name, call): argument sets the library refuses; every call has to come back WS_ERR_INVALID without launching."""
    from wesep_amd import _lib as L
    import ctypes as C
    tab = torch.ones(8, dtype=torch.int32, device=device)
    p = lambda x: None if x is None else C.c_void_p(x.data_ptr())          # noqa: E731
    raw = lambda name, *a: (lambda: L.check(getattr(L.lib(), name)(*a, L.stream_ptr()), name))          # noqa: E731
    fw = lambda **k: (lambda a: dev.mhastp_fwd(t, t, a["R"], a["F"], a["T"], a["C"], 1, a["H"], a["layers"], a["ds"], t, t))(          # noqa: E731
        dict(dict(R=1, F=2, T=3, C=4, H=2, layers=2, ds=4), **k))
    bw = lambda **k: (lambda a: dev.mhastp_bwd(t, t, t, t, 1, a["F"], 3, a["C"], 1, 1, 2, a["ds"], t))(dict(dict(F=2, C=4, ds=8), **k))          # noqa: E731
    return [
        ("mhastp_bwd dm = 5420: no frame fits the LDS budget", lambda: bw(F=10, C=542, ds=5420)),
        ("mhastp_fwd ds neither 1 nor dm", lambda: fw(ds=3)),
        ("mhastp_fwd C % H", lambda: fw(C=5, ds=1)),
        ("mhastp_fwd layers 3", lambda: fw(layers=3)),
        ("mhastp_fwd_split tsplit above T", lambda: dev.mhastp_fwd_split(t, t, 1, 2, 3, 4, 1, 2, 2, 4, t, t, tsplit=4, part=t)),
        ("mhastp_bwd_split tsplit above T", lambda: dev.mhastp_bwd_split(t, t, t, t, 1, 2, 3, 4, 1, 2, 2, 4, t, tsplit=4)),
        ("mhastp_bwd dpack without work", raw("ws_mhastp_bwd", p(t), p(t), p(t), p(t), 1, 2, 3, 4, 1, 2, 2, 4, p(t), None, None, 1, p(t))),
        ("mhastp_bwd slabs without a slab", raw("ws_mhastp_bwd", p(t), p(t), p(t), p(t), 1, 2, 3, 4, 1, 2, 2, 4, p(t), p(t), None, 2, p(t))),
        ("mhastp_pack layers 2 without W2", lambda: dev.mhastp_pack(t, t, None, None, 2, 2, 2, 1, t)),
        ("preemph_pad T = 1, pad = 0", lambda: dev.preemph_pad(t, 2, 1, 0, 1, 0.97, t)),
        ("preemph_pad T = pad", lambda: dev.preemph_pad(t, 2, 3, 3, 9, 0.97, t)),
        ("preemph_pad ldo below T + 2 pad", lambda: dev.preemph_pad(t, 2, 8, 3, 13, 0.97, t)),
        ("preemph_pad_len T = 1", lambda: dev.preemph_pad_len(t, 2, 1, 0, 1, 0.97, tab, t)),
        ("preemph_pad_len NULL table", raw("ws_preemph_pad_len", p(t), 2, 8, 3, 14, C.c_float(0.97), None, p(t))),
        ("tstp_fwd_len NULL table", raw("ws_tstp_fwd_len", p(t), 2, 3, 4, 4, None, C.c_float(1e-7), p(t))),
        ("astp_fwd_len NULL table", raw("ws_astp_fwd_len", p(t), p(t), 2, 3, 4, None, C.c_float(1e-7), p(t), p(t))),
        ("time_mean_len NULL table", raw("ws_time_mean_len", p(t), 2, 3, 4, None, p(t))),
        ("cmn_len NULL table", raw("ws_cmn_len", p(t), 2, 3, 4, None, p(t))),
        ("tail_select_len NULL table", raw("ws_tail_select_len", p(t), 2, 3, 4, None, p(t))),
        ("tail_select_len C % 4", lambda: dev.tail_select_len(t, 2, 3, 6, tab, t)),
        ("bn_prelu_fwd_len NULL table", raw("ws_bn_prelu_fwd_len", p(t), p(t), p(t), p(t), None, p(t), C.c_longlong(8), 4, 4, 2, None, p(t), p(t))),
        ("bn_prelu_fwd_len W does not divide rows_per_r", lambda: dev.bn_prelu_fwd_len(t, t, t, t, None, t, 12, 4, 4, 3, tab, t, t)),
        ("seg_sums C % 4", lambda: dev.seg_sums(t, None, 2, 5, 6, 2, t)),
        ("seg_scale seg_len = 0", lambda: dev.seg_scale(None, t, 2, 5, 4, 0, t)),
        ("power_spec lds below 2 nf", lambda: dev.power_spec(t, 2, 5, 9, 5, t)),
        ("power_spec ldp below nf", lambda: dev.power_spec(t, 2, 5, 10, 4, t)),
        ("astp_fwd T = 0", lambda: dev.astp_fwd(t, t, 2, 0, 4, t, t)),
        ("tstp_fwd C = 0", lambda: dev.tstp_fwd(t, 2, 3, 4, 0, t)),
    ]


# ------------------------------------------------------------------------------------------------------------
# checker, emulation
# ------------------------------------------------------------------------------------------------------------
def verify(b, ref, after, extra=None, what=None):
    """Every output of a built case against `ref`: `after` = name -> whole CPU allocation after the launch.  Returns the worst
    err / bound.  Raises ContractViolation: nan | exact | bound | sentinel."""
    what = what or f"{b.case.entry} {b.case.name}"
    worst = 0.0
    for key, r in ref.items():
        name = b.alias.get(key, key)
        before = b.bufs[name]
        if key in SCRATCH:          # scratch: anything inside its extent, nothing outside; the listed states exact
            before = before.clone()
            lo = b.start[name]
            before[lo:lo + b.size[name]] = after[name][lo:lo + b.size[name]]
        fn = check_partial if isinstance(r, Partial) else check
        worst = max(worst, fn(after[name], before, r, f"{what} {key}", b.start[name]))
    return worst


output_bits = tc.output_bits


def _place(b, ref, vals):
    """(after, extra) with `vals` (name -> values in the order of the reference's idx / rows) written."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    for key, r in ref.items():
        name = b.alias.get(key, key)
        if key in SCRATCH:
            after[name][b.start[name]:b.start[name] + b.size[name]] = 0.0
        idx = r.rows.reshape(-1) if isinstance(r, Partial) else r.idx
        after[name][idx + b.start[name]] = vals[key].reshape(-1).float()
    return after, {}


def perfect(b, ref):
    """What a correctly rounding kernel leaves: the fp32 rounding of the float64 values."""
    return _place(b, ref, compute(b.case.entry, b.spec, b.views(b.bufs), F64))


def emulate(b, ref, order="seq", defect=None, tiles="online"):
    """What a correct fp32 kernel (sums in `order`, softmax in `tiles`) leaves -- or one with the planted `defect`."""
    return _place(b, ref, compute(b.case.entry, b.spec, b.views(b.bufs), F32, order, defect, tiles))


_LEN = ["tlen_unclamped", "tlen_plus_1"]
DEFECTS = {
    "tstp_fwd": ["div_by_T", "feature_f_major"],
    "astp_fwd": ["var_unclamped", "aux3_is_var"],
    "astp_bwd": ["floor_not_strict", "dbar_with_var"],
    "seg_sums": ["odd_frame_dropped", "b_ignored"],
    "seg_scale": ["t_mod_seg_len", "x_ignored"],
    "preemph_pad": ["y0_from_x0"],
    "power_spec": ["re_twice", "pad_unwritten", "stride_2nf"],
    "log_eps": ["eps_dropped", "log10"],
    "mhastp_pack": ["columns_not_permuted", "b2_before_w2"],
    "mhastp_fwd": ["partial_tile_dropped", "no_rescale", "rescale_not_sxx", "var_unclamped", "out_kernel_order", "aux_native_order", "head0_for_all",
                   "block_h_major", "tanh_skipped"],
    "mhastp_bwd": ["floor_strict", "dvar_unclamped", "c_without_var", "dout_kernel_order", "last_query_only", "dpack_kernel_order",
                   "bias_column_at_nb_minus_1", "split_last_block_dropped", "wgrad_skips_split0"],
    "mhastp_fwd_split": ["merge_skips_split0", "empty_split_nan", "partial_tile_dropped"],
    "mhastp_bwd_split": ["split_last_block_dropped", "dout_kernel_order"],
    "bn_prelu_fwd_len": ["tail_multiplied", "r_from_W", "y_is_u"],
    "tstp_fwd_len": _LEN + ["mean_div_T", "div_by_T"],
    "astp_fwd_len": _LEN + ["var_unclamped"],
    "time_mean_len": _LEN + ["mean_div_T"],
    "cmn_len": _LEN + ["mean_div_T", "tail_multiplied"],
    "tail_select_len": ["tail_multiplied", "tlen_plus_1", "clamp_lo_1"],
    "preemph_pad_len": ["reflect_at_T", "clamp_pad_plus_1", "tail_unwritten", "tlen_unclamped", "y0_from_x0"],
}
