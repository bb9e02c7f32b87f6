"""TEST INFRASTRUCTURE ONLY -- contract suite of the transform pair of pBSRNN (wesep_amd/csrc/stft.hip: ws_stft_bandsplit,
ws_stft_bandsplit_len, ws_mask_istft_frames, ws_istft_ola, ws_istft_ola_len, ws_mask_istft_bwd) and of its hop / window
relatives (ws_ola_norm_len of ragged_grid.hip, ws_ola_fwd / ws_ola_bwd of tasnet.hip).  No GPU code here: the CPU test
(test_stft_contract_host_cpu.py) checks this module, the GPU test (test_stft_contract_gpu.py) runs every case through
wesep_amd.dev.  Ref, check, eps_for, the guards and the pairwise generator with its registries come from
tests/gemm_contract.py; the generator is used as it is.

REFERENCE.  float64 index arithmetic that restates include/wesep_hip.h, not a call of torch.stft:
  padded[q] = x[reflect(q - 256)], reflect turning at 0 and at Tr - 1 (Tr = lengths[r], or T); frame t = padded[128 t :
  128 t + 512] times w[n] = 0.5 - 0.5 cos(2 pi n / 512); numpy.fft.rfft / irfft in float64 as the transform; bin k of band g
  (first bin f0, width bw) at column 2 f0 + (k - f0) (re) and 2 f0 + bw + (k - f0) (im) of xbs, mask channel c at
  4 f0 + c bw + (k - f0); Im of DC and Nyquist dropped in the inverse; overlap-add over the frames t <= Tr / 128 that
  contain the padded coordinate, divided by the sum of w^2 over the same frames, centre trim; exact zeros from lengths[r]
  on and in the frames from 1 + lengths[r] / 128 on; the backward as the explicit adjoint (below, ref_bwd); ola_fwd /
  ola_bwd / ola_norm_len as their header lines say.  torch.stft / torch.istft in float64 (autograd for the backward, per
  row for ragged tables) are the second opinion of the CPU test: 1e-12 relative on every case.

BOUNDS.  Every output element: |out - ref| <= bound, bound = eps * S + named extra terms, S = the same computation on
absolute values.  u = 2^-24.  All constants are computed below from these counts; none is tuned to a run.

  Complex arithmetic is counted on the modulus: a rounded complex add misses by <= u |a + b|, a rounded complex product
  by <= sqrt(5) u |a||b| (Brent, Percival, Zimmermann 2007; an FMA contraction only removes roundings).  A value of the
  FFT at any stage is a sum of inputs with coefficients of modulus 1, so the moduli of the values one output depends on
  sum to at most S = sum_n |x_n| at every stage, and an error made at one stage reaches an output with coefficient 1:
  every rounding level costs (its constant) * u * S.
    dft8: three add levels (3), one product with a W8 constant (sqrt 5) whose fp32 representation is off by <= u (1):
          4 + sqrt(5) per pass, three passes.
    two twiddle products: sqrt(5) u each plus the table error TW_ERR each.
    TW_ERR: no accuracy statement for sincospif was found on the build machine (the headers under the ROCm tree only
          declare __ocml_sincospi_f32; no document or header there gives an ulp figure).  As the fallback the issue names:
          the largest |fp32 - fp64| of the 512-entry table computed on the CPU (TABLE_DIFF, 2^-25 at most: correct
          rounding) plus one ulp of a value below 1 (2^-24) per component, times sqrt(2) for the modulus.  The argument
          j / 256 is exact in fp32.
    DEPTH_FFT = 3 (4 + sqrt 5) u + 2 (sqrt(5) u + TW_ERR)           ~ 27.4 u
    EPS_FFT   = ceil(DEPTH_FFT / u + 1) u  (the + 1: the product with the window; rounding up to a whole u also covers
                the second-order terms, (1 + 32 u)^2 - 1 - 64 u < 2^-38)
  Window term: the kernel's window is 0.5f - 0.5f * tw[n].x.  0.5f * c is exact, c is off by TW_COMP = TABLE_DIFF + 2^-24,
    the subtraction rounds a value <= 1 (2^-25): D_W = TW_COMP / 2 + 2^-25 ~ 1.25 u ABSOLUTE, which at n = 1 (w = 3.8e-5)
    is a relative error of 2e-3.  It enters as D_W * sum_n |x_n|, not through eps.

  stft_bandsplit   every bin of frame t: EPS_FFT * sum_n |x_n| w_n + D_W * sum_n |x_n|.  Tail frames exact zeros.
  mask_istft_frames  A_k = (|Xr| + |Xi|)(|mre| + |mim|) bounds the modulus of the masked bin and, times the relative
    error of its inputs, the modulus of its error: mre = o * sigmoid(.) carries D_SIG + u, the complex product three more
    roundings.  D_SIG: 1 / (1 + expf(-x)) = expf (3 ulp, the OpenCL full-profile requirement the device library
    implements; 1 ulp <= 2 u relative) + the add + a correctly rounded division (hipcc's default) = 8 u.
    S = w_n / 512 * sum_k c_k A_k (c = 1 at DC / Nyquist, 2 elsewhere: the Hermitian extension);
    bound = (EPS_FFT + D_SIG + 4 u) * S + D_W / 512 * sum_k c_k A_k   (1 / 512 is a power of two).
  istft_ola   y / e with y a sum of `terms` <= 4 frames values, e the fp32 sum of fp32 w^2:
    (terms + 2) u * sum |frames| / e   (terms - 1 adds, the division, slack of two)
    + sum |frames| / e * d_e / (e - d_e),  d_e = sum_t (2 w D_W + D_W^2 + u w^2) + terms u e.
    e is bounded below: sample pos lies in frame t0 = pos / 128 at n0 = 256 + pos % 128 in [256, 383]; t0 <= (T - 1) / 128
    <= Tf - 1 (and t0 <= lengths[r] / 128 for pos < lengths[r]), so that frame always counts and e >= w(383)^2 =
    sin^4(pi 383 / 512) > 0.256.  With T >= 257 (the reflect pad's own condition) every row has Tf >= 3 frames, so a
    second frame (t0 + 1 or t0 - 1, n0 -+ 128) counts as well and e >= w(383)^2 + w(255)^2 > 1.24 except on the last 128
    samples of a row whose length is a multiple of 128, where e >= 0.256 stands.  d_e <= 4 (2.5 u + u) + 4 u * 1.5 =
    20 u, so e - d_e > 0.2559.
  mask_istft_bwd  dv = dwav * w / e: |dv| (2 u + d_e / (e - d_e)) + |dwav| D_W / e on the input of the forward FFT bound:
    E_V = EPS_FFT * sum_n |dv_n| + sum_n (that input error), per frame, for every bin.  g = V * c_k / 512 exactly
    (powers of two).  dmr = gre Xr + gim Xi (three roundings): E_dm = (E_V + 3 u S_V) c_k / 512 (|Xr| + |Xi|),
    S_dm = S_V c_k / 512 (|Xr| + |Xi|).  d[0], d[bw]: s (E_dm + (D_SIG + u) S_dm).  d[2 bw], d[3 bw] = dm o s (1 - s):
    |o| s ((1 - s)(E_dm + (D_SIG + 3 u) S_dm) + S_dm (D_SIG s + u)): the last term is the ABSOLUTE error of 1 - s in fp32
    (at a gate of +30 the fp32 sigmoid is exactly 1 and the output exactly 0 where float64 has 9e-14).
    Where the bound is 0 (a zero dwav row, a zero mask value) the output has to be exactly the reference.
  ola_fwd   eps_for(False, terms) * S, terms = the frames of the sum + the bias.
  ola_bwd   exact: a copy or zero.
  ola_norm_len  (a + b) * fl(1 / env): the add, the rounding of 1 / env (taken in double, rounded once), the product:
    ((1 + u)^3 - 1) * (|a| + |b|) / env.

The worst-case FFT bound is loose on dense data (32 u * sum |x_n| w_n against a typical error of u * sqrt(sum x^2)):
Gaussian frames sit near 1e-2 of it.  The sweep stays sharp through STRUCTURED data: an impulse reduces every output to
one twiddle product times one window value, a bin-centred tone and DC make S large against every other bin's value.

DIMENSIONS / RULES / CASES: *_DIMS, *_RULES below, registered with the generator of gemm_contract; cases(entry) adds the
grid-stride extras.  BUFFERS as in gemm_contract: operands and outputs inside GUARD floats, write sets NaN, the rest of
an output allocation SENT; inputs the contract does not read NaN (build(case)) or 3e30 (build(case, garbage=True)):
guards, samples from lengths[r] on, frames from 1 + lengths[r] / hop on for the overlap-add entries."""
import math

import numpy as np
import torch

from tests import gemm_contract as gc
from tests.gemm_contract import (GUARD, SENT, U, Built, Case, ContractViolation, Ref, check, eps_for)  # noqa: F401

NFFT, HOP, NBIN = 512, 128, 257
GARBAGE = 3.0e30
NAN = float("nan")
F64 = torch.float64
ENTRIES = ("stft_bandsplit", "mask_istft_frames", "istft_ola", "mask_istft_bwd", "ola_norm_len", "ola_fwd", "ola_bwd")
COMPOSED = "stft_composed"

_ANG = 2.0 * np.pi * np.arange(NFFT) / NFFT
WIN = 0.5 - 0.5 * np.cos(_ANG)
TW64 = np.cos(_ANG) - 1j * np.sin(_ANG)
TW32 = TW64.astype(np.complex64)
WIN32 = (np.float32(0.5) - np.float32(0.5) * TW32.real).astype(np.float32)
TABLE_DIFF = float(max(np.abs(TW32.real.astype(np.float64) - TW64.real).max(), np.abs(TW32.imag.astype(np.float64) - TW64.imag).max()))
TW_COMP = TABLE_DIFF + U
TW_ERR = math.sqrt(2.0) * TW_COMP
D_W = TW_COMP / 2 + U / 2
DEPTH_FFT = 3 * (4 + math.sqrt(5.0)) * U + 2 * (math.sqrt(5.0) * U + TW_ERR)
EPS_FFT = math.ceil(DEPTH_FFT / U + 1) * U
ULP_EXP = 3
D_SIG = (2 * ULP_EXP + 2) * U
EPS_FRAMES = EPS_FFT + D_SIG + 4 * U
EPS_NORM = (1 + U) ** 3 - 1
E_MIN = math.sin(math.pi * 383 / 512) ** 4      # the lower bound of the envelope (docstring)
CONSTANTS = {"TABLE_DIFF/u": TABLE_DIFF / U, "TW_ERR/u": TW_ERR / U, "D_W/u": D_W / U, "DEPTH_FFT/u": DEPTH_FFT / U,
             "EPS_FFT/u": EPS_FFT / U, "D_SIG/u": D_SIG / U, "EPS_FRAMES/u": EPS_FRAMES / U, "E_MIN": E_MIN}


# ------------------------------------------------------------------------------------------------------------
# band tables and layouts
# ------------------------------------------------------------------------------------------------------------
def band_table(name):
    if name == "bsrnn16k":
        from oracle.bsrnn_oracle import band_widths
        return [int(v) for v in band_widths(16000, 512)]
    return {"one": [257], "ones": [1] * 257, "uneven": [1, 3, 64, 128, 61]}[name]


def band_cols(widths, defect=None):
    """(re, im, mc): column of Re / Im of every bin in an xbs row, and of the four mask channels in a mask row."""
    bw = np.asarray(widths, dtype=np.int64)
    f0 = np.concatenate([[0], np.cumsum(bw)[:-1]])
    g = np.repeat(np.arange(len(bw)), bw)
    fl = np.arange(NBIN) - f0[g]
    b = bw[g]
    if defect == "neighbour-bw":        # the scatter offset takes the next band's width (the previous one's in the last band)
        b = bw[np.where(g + 1 < len(bw), g + 1, np.maximum(g - 1, 0))]
    re, im = 2 * f0[g] + fl, 2 * f0[g] + b + fl
    if defect == "re-im-swapped":
        re, im = im, re
    mc = np.stack([4 * f0[g] + c * bw[g] + fl for c in range(4)])
    return re, im, mc


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def _ref(idx, val, S, bound, exact=None):
    idx = np.asarray(idx).reshape(-1)
    n = idx.size
    ex = np.zeros(n, dtype=bool) if exact is None else np.asarray(exact).reshape(-1)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)))
    return Ref(torch.from_numpy(idx.astype(np.int64)), t(val), t(S), t(bound), torch.from_numpy(ex.copy()))


def _lens(sp):
    return list(sp["lens"]) if sp.get("lens") is not None else [sp["T"]] * sp["R"]


def frame_index(Tr, T, ntf, defect=None):
    """[ntf][512] sample index of every frame element of a row with Tr valid samples."""
    p = HOP * np.arange(ntf)[:, None] + np.arange(NFFT)[None, :] - NFFT // 2
    p = np.where(p < 0, -p - (1 if defect == "left-reflect" else 0), p)
    turn = T if defect == "reflect-T-len" else Tr
    last = turn if defect == "reflect-T" else turn - 1
    return np.where(p >= turn, 2 * last - p, p)


def ref_stft(sp, v, defect=None):
    R, T, Tf = sp["R"], sp["T"], sp["Tf"]
    re, im, _ = band_cols(sp["widths"], defect)
    win = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / (NFFT - 1)) if defect == "symmetric-hann" else WIN
    Tfd = -(-T // HOP) if defect == "tf-ceil" else Tf
    cols = np.concatenate([re, im])
    idx = ((np.arange(R)[:, None, None] * Tfd + np.arange(Tfd)[None, :, None]) * (2 * NBIN) + cols[None, None, :])
    val = np.zeros((R, Tfd, 2 * NBIN))
    S, bound = np.zeros_like(val), np.zeros_like(val)
    exact = np.zeros(val.shape, dtype=bool)
    tw = None
    if defect == "twiddle":             # table entry 1 off by 2^-20 relative, in both of its roles: twiddle and window
        tw = TW64.copy()
        tw[1] *= 1 + 2.0 ** -20
        win = 0.5 - 0.5 * tw.real
        tw = tw[(np.arange(NFFT)[:, None] * np.arange(NBIN)[None, :]) % NFFT]
    for r, Tr in enumerate(_lens(sp)):
        ntf = min(1 + Tr // HOP, Tfd)
        fr = v["wav"][r * T:][frame_index(Tr, T, ntf, defect)]
        X = (fr * win) @ tw if tw is not None else np.fft.rfft(fr * win, axis=1)
        val[r, :ntf] = np.concatenate([X.real, X.imag], axis=1)
        S[r, :ntf] = (np.abs(fr) * WIN).sum(1)[:, None]
        bound[r, :ntf] = EPS_FFT * S[r, :ntf] + D_W * np.abs(fr).sum(1)[:, None]
        exact[r, ntf:] = True
        if defect == "tail-not-zero" and ntf < Tfd:
            val[r, ntf:] = val[r, 0] + 1.0
    if defect is None:
        o = np.argsort(idx.reshape(-1))
        return {"xbs": _ref(idx.reshape(-1)[o], val.reshape(-1)[o], S.reshape(-1)[o], bound.reshape(-1)[o], exact.reshape(-1)[o])}
    return {"xbs": _ref(idx, val, S, bound, exact)}


def _masked(sp, v, NF):
    re, im, mc = band_cols(sp["widths"])
    xbs = v["xbs"][:NF * 2 * NBIN].reshape(NF, 2 * NBIN)
    m3 = v["m3"][:NF * 4 * NBIN].reshape(NF, 4 * NBIN)
    Xr, Xi = xbs[:, re], xbs[:, im]
    o0, o1, s0, s1 = m3[:, mc[0]], m3[:, mc[1]], _sig(m3[:, mc[2]]), _sig(m3[:, mc[3]])
    return Xr, Xi, o0, o1, s0, s1


_CK = np.full(NBIN, 2.0)
_CK[0] = _CK[NBIN - 1] = 1.0


def ref_frames(sp, v, defect=None):
    NF = sp["R"] * sp["Tf"]
    Xr, Xi, o0, o1, s0, s1 = _masked(sp, v, NF)
    mre, mim = o0 * s0, o1 * s1
    er, ei = Xr * mre - Xi * mim, Xr * mim + Xi * mre
    ei[:, 0] = 0.0
    if defect != "nyquist-im-kept":
        ei[:, NBIN - 1] = 0.0
        fr = np.fft.irfft(er + 1j * ei, n=NFFT, axis=1)
    else:       # the full inverse over the Hermitian extension, Im of Nyquist carried along
        Y = np.concatenate([er + 1j * ei, (er - 1j * ei)[:, NBIN - 2:0:-1]], axis=1)
        fr = np.fft.ifft(Y, axis=1).real
    fr = fr * WIN[None, :]
    A = (_CK[None, :] * (np.abs(Xr) + np.abs(Xi)) * (np.abs(mre) + np.abs(mim))).sum(1)[:, None] / NFFT
    S = A * WIN[None, :]
    return {"frames": _ref(np.arange(NF * NFFT), fr, S, EPS_FRAMES * S + D_W * A)}


def _ola_terms(frames_r, T, tmax, env_tmax=None):
    """Row: (y, |y| sum, e, d_e, terms) of the overlap-add at every sample; frames t <= tmax count (t <= env_tmax in e)."""
    q = np.arange(T) + NFFT // 2
    y, ya, e, de = np.zeros(T), np.zeros(T), np.zeros(T), np.zeros(T)
    terms = np.zeros(T)
    env_tmax = tmax if env_tmax is None else env_tmax
    for j in range(4):
        t = q // HOP - j
        n = q - HOP * t
        ok = (t >= 0) & (t <= tmax)
        if frames_r is not None:
            f = np.where(ok, frames_r[np.clip(t, 0, frames_r.shape[0] - 1), n], 0.0)
            y, ya = y + f, ya + np.abs(f)
        oke = (t >= 0) & (t <= env_tmax)
        w = WIN[n]
        e = e + np.where(oke, w * w, 0.0)
        de = de + np.where(oke, 2 * w * D_W + D_W * D_W + U * w * w, 0.0)
        terms = terms + ok
    return y, ya, e, de + terms * U * e, terms


def ref_ola(sp, v, defect=None):
    R, T, Tf = sp["R"], sp["T"], sp["Tf"]
    fr = v["frames"][:R * Tf * NFFT].reshape(R, Tf, NFFT)
    val, S, bound = np.zeros((R, T)), np.zeros((R, T)), np.zeros((R, T))
    exact = np.zeros((R, T), dtype=bool)
    for r, Tr in enumerate(_lens(sp)):
        tmax = Tr // HOP
        et = {"env-last-missing": tmax - 1, "env-all-frames": Tf - 1}.get(defect)
        y, ya, e, de, terms = (a[:Tr] for a in _ola_terms(fr[r], T, tmax, et))
        _, _, e0, de0, _ = (a[:Tr] for a in _ola_terms(None, T, tmax))
        with np.errstate(divide="ignore", invalid="ignore"):    # (a planted envelope may be 0)
            val[r, :Tr] = y / e
        S[r, :Tr] = ya / e0
        bound[r, :Tr] = (terms + 2) * U * ya / e0 + ya / e0 * de0 / (e0 - de0)
        exact[r, Tr:] = True
        if defect == "tail-not-zero":
            val[r, Tr:] = 1.0
    return {"wav": _ref(np.arange(R * T), val, S, bound, exact)}


def ref_bwd(sp, v, defect=None):
    """dmask3 = the adjoint of (frames -> overlap-add / envelope) through the GLU mask.  With dv[t][n] = dwav[128 t + n - 256]
    w[n] / e (0 outside the row) and V = rfft(dv): frames[n] = (1 / 512) sum_k c_k Re(Y_k e^{+i theta}), so dL / dRe Y_k =
    c_k / 512 Re V_k, dL / dIm Y_k = c_k / 512 Im V_k (0 at DC / Nyquist, whose Im the inverse drops); Y = (Xr + i Xi)(mre +
    i mim) gives dmre = gre Xr + gim Xi, dmim = -gre Xi + gim Xr; mre = o s(gate): d o = dm s, d gate = dm o s (1 - s)."""
    R, T, Tf = sp["R"], sp["T"], sp["Tf"]
    NF = R * Tf
    Xr, Xi, o0, o1, s0, s1 = _masked(sp, v, NF)
    _, _, mc = band_cols(sp["widths"])
    dw = v["dwav"][:R * T].reshape(R, T)
    _, _, e, de, _ = _ola_terms(None, T, T // HOP)
    p = HOP * np.arange(Tf)[:, None] + np.arange(NFFT)[None, :] - NFFT // 2
    ok = (p >= 0) & (p < T)
    pc = np.clip(p, 0, T - 1)
    sc = (np.full(NBIN, 2.0) if defect == "edge-x2" else _CK) / NFFT
    val, S, bound = (np.zeros((NF, 4 * NBIN)) for _ in range(3))
    for r in range(R):
        d = np.where(ok, dw[r][pc], 0.0)
        dv = d * WIN[None, :] / e[pc]
        V = np.fft.rfft(dv, axis=1)
        SV = np.abs(dv).sum(1)[:, None]
        EV = EPS_FFT * SV + (np.abs(dv) * (2 * U + (de / (e - de))[pc]) + np.abs(d) * D_W / e[pc]).sum(1)[:, None]
        gre, gim = V.real * sc, V.imag * sc
        gim[:, 0] = gim[:, NBIN - 1] = 0.0
        rows = slice(r * Tf, (r + 1) * Tf)
        xr, xi = Xr[rows], Xi[rows]
        XA = np.abs(xr) + np.abs(xi)
        Sdm = SV * sc * XA
        Edm = (EV + 3 * U * SV) * sc * XA
        for c, dm, o, s in ((0, gre * xr + gim * xi, o0[rows], s0[rows]), (1, -gre * xi + gim * xr, o1[rows], s1[rows])):
            val[rows, mc[c]] = dm * s
            S[rows, mc[c]] = Sdm * s
            bound[rows, mc[c]] = s * (Edm + (D_SIG + U) * Sdm)
            val[rows, mc[2 + c]] = dm * o * s * (1 - s)
            S[rows, mc[2 + c]] = Sdm * np.abs(o) * s * (1 - s)
            bound[rows, mc[2 + c]] = np.abs(o) * s * ((1 - s) * (Edm + (D_SIG + 3 * U) * Sdm) + Sdm * (D_SIG * s + U))
    return {"dm3": _ref(np.arange(NF * 4 * NBIN), val, S, bound)}


def ref_ola_fwd(sp, v, defect=None):
    R, Tp, L, hop, Tout = sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"]
    fr = v["frames"][:R * Tp * L].reshape(R, Tp, L)
    bias = float(v["bias"][0]) if sp["bias"] else 0.0
    j = np.arange(Tout)
    val, S, terms = np.zeros((R, Tout)), np.zeros((R, Tout)), np.zeros(Tout)
    for k in range(-(-L // hop)):
        t = j // hop - k
        n = j - hop * t
        ok = (t >= 0) & (t < Tp) & (n < L)
        if defect == "t_lo":
            ok &= t >= j // hop - L // hop + 1
        f = np.where(ok[None, :], fr[:, np.clip(t, 0, Tp - 1), np.clip(n, 0, L - 1)], 0.0)
        val, S, terms = val + f, S + np.abs(f), terms + ok
    val = val + bias * (terms if defect == "bias-per-frame" else 1.0)
    S = S + abs(bias)
    eps = (terms + 1 + 8) * U       # eps_for(False, terms + 1), element by element
    assert eps_for(False, 3) == (3 + 8) * U
    return {"est": _ref(np.arange(R * Tout), val, S, eps[None, :] * S)}


def ref_ola_bwd(sp, v, defect=None):
    R, Tp, L, hop, Tout = sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"]
    j = (hop * np.arange(Tp)[:, None] + np.arange(L)[None, :])
    flat = np.arange(R)[:, None, None] * Tout + j[None]
    inside = np.broadcast_to(j[None] < Tout, flat.shape)
    val = np.where(inside | (defect == "no-zero-past-Tout"), v["dest"][flat], 0.0)
    z = np.zeros(val.shape)
    return {"dframes": _ref(np.arange(R * Tp * L), val, z, z, np.ones(val.shape, dtype=bool))}


def ref_ola_norm_len(sp, v, defect=None):
    R, T, Tf, n = sp["R"], sp["T"], sp["Tf"], sp["n"]
    hop = n // 2
    fr = v["frames"][:R * Tf * n].reshape(R, Tf, n)
    win = v["win"][:n]
    i = np.arange(T)
    t1 = (i + hop) // hop
    k = i + hop - t1 * hop
    val, S, bound = np.zeros((R, T)), np.zeros((R, T)), np.zeros((R, T))
    exact = np.zeros((R, T), dtype=bool)
    for r, ln in enumerate(_lens(sp)):
        ln = min(max(ln, 0), T)
        two = t1 < 1 + ln // hop
        a = fr[r, t1 - 1, hop + k]
        b = np.where(two, fr[r, np.minimum(t1, Tf - 1), k], 0.0)
        env = win[hop + k] ** 2 + np.where(two, win[k] ** 2, 0.0)
        val[r, :ln] = ((a + b) / env)[:ln]
        S[r, :ln] = ((np.abs(a) + np.abs(b)) / env)[:ln]
        exact[r, ln:] = True
    return {"est": _ref(np.arange(R * T), val, S, EPS_NORM * S, exact)}


REFS = {"stft_bandsplit": ref_stft, "mask_istft_frames": ref_frames, "istft_ola": ref_ola, "mask_istft_bwd": ref_bwd,
        "ola_norm_len": ref_ola_norm_len, "ola_fwd": ref_ola_fwd, "ola_bwd": ref_ola_bwd}

# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, cases
# ------------------------------------------------------------------------------------------------------------
TS = [257, 383, 384, 385, 511, 512, 513, 640, 1000, 1280, 1920, 2049]
RS = [1, 2, 3, 4, 5]
BANDS = ["bsrnn16k", "one", "ones", "uneven"]
LENS = ["off", "full", "min", "k128", "mixed"]
WAV_DATA = ["gauss", "impulse-0", "impulse-last", "impulse-255", "impulse-256", "impulse-257", "dc", "tone-bin64", "row-x1e3", "offset"]
SPEC_DATA = ["gauss", "row-x1e3", "offset", "bin-0", "bin-64", "bin-256"]
MASK_DATA = ["gauss", "sat", "zero-gate"]
OLA_LH = [(20, 10), (80, 10), (160, 10), (16, 8), (7, 3), (4, 4), (5, 1)]
OLA_TOUT = ["full", "full-1", "last+1", "hop"]
ON_T = ["4h", "4h+1", "3h+2", "5h-1", "6h+3"]

ST_DIMS = dict(T=TS, R=RS, bands=BANDS, lengths=LENS, data=WAV_DATA)
FR_DIMS = dict(T=TS, R=RS, bands=BANDS, data=SPEC_DATA, mask=MASK_DATA)
OL_DIMS = dict(T=TS, R=RS, lengths=LENS, data=["gauss", "row-x1e3", "offset"])
BW_DIMS = dict(T=TS, R=RS, bands=BANDS, data=["gauss", "impulse-0", "impulse-last", "dc", "row-x1e3", "offset"], spec=["gauss", "offset"],
               mask=MASK_DATA)
ON_DIMS = dict(n=[8, 16, 128, 256], T=ON_T, R=[1, 3, 4], lengths=LENS[1:], data=["gauss", "row-x1e3", "offset"])
OF_DIMS = dict(Lhop=OLA_LH, Tp=[1, 2, 9, 33], Tout=OLA_TOUT, bias=[0, 1], R=[1, 3])
OB_DIMS = dict(Lhop=OLA_LH, Tp=[1, 2, 9, 33], Tout=OLA_TOUT, R=[1, 3])

_LEN_RULES = [
    ("k128: a multiple of 128 below T that is a valid length (>= 257) needs T >= 385", ("lengths", "T"),
     lambda ln, T: ln == "k128" and T < 385),
    ("mixed: rows of 257, T - 1, T and one with lengths % 128 == 127 (383 at least) need T >= 383", ("lengths", "T"),
     lambda ln, T: ln == "mixed" and T < 383),
    ("mixed holds four different rows", ("lengths", "R"), lambda ln, R: ln == "mixed" and R < 4),
]
ST_RULES = _LEN_RULES + [
    ("an impulse at sample 257 lies inside every row's valid samples", ("data", "T"), lambda d, T: d == "impulse-257" and T < 258),
    ("an impulse at sample 257 lies inside every row's valid samples", ("data", "lengths"),
     lambda d, ln: d == "impulse-257" and ln in ("min", "mixed")),
]
RULES = {"stft_bandsplit": ST_RULES, "mask_istft_frames": [], "istft_ola": _LEN_RULES, "mask_istft_bwd": [],
         "ola_norm_len": [("mixed holds four different rows", ("lengths", "R"), lambda ln, R: ln == "mixed" and R < 4)],
         "ola_fwd": [], "ola_bwd": []}
DIMS = {"stft_bandsplit": ST_DIMS, "mask_istft_frames": FR_DIMS, "istft_ola": OL_DIMS, "mask_istft_bwd": BW_DIMS,
        "ola_norm_len": ON_DIMS, "ola_fwd": OF_DIMS, "ola_bwd": OB_DIMS}
NFRAMES = (3, 15, 16, 17, 32, 33)


def on_T(d):
    h = d["n"] // 2
    return {"4h": 4 * h, "4h+1": 4 * h + 1, "3h+2": 3 * h + 2, "5h-1": 5 * h - 1, "6h+3": 6 * h + 3}.get(d["T"], d["T"])


def ola_Tout(d):
    (L, hop), Tp = d["Lhop"], d["Tp"]
    full = (Tp - 1) * hop + L
    v = {"full": full, "full-1": full - 1, "last+1": (Tp - 1) * hop + 1, "hop": hop}.get(d["Tout"], d["Tout"])
    return min(max(v, 1), full)


def _targets(entry, d, seed=0):
    if entry in ("stft_bandsplit", "mask_istft_frames", "mask_istft_bwd"):
        nf = d["R"] * (1 + d["T"] // HOP)
        k = {"stft_bandsplit": "stft_bandsplit_kernel", "mask_istft_frames": "mask_istft_frames_kernel",
             "mask_istft_bwd": "mask_istft_bwd_kernel"}[entry]
        t = (k, f"{k}[bands {d['bands']}]", f"{k}[last workgroup {'full' if nf % 16 == 0 else 'with idle waves'}]")
        if entry == "stft_bandsplit":
            t += (f"{k}[lengths {'off' if d['lengths'] == 'off' else 'on'}]",)
        return t + ((f"{entry}[nframes {nf}]",) if nf in NFRAMES else ())
    if entry == "istft_ola":
        return ("istft_ola_kernel", f"istft_ola_kernel[lengths {'off' if d['lengths'] == 'off' else 'on'}]") + (
            ("istft_ola_kernel[grid-stride]",) if d["R"] * d["T"] > 8192 * 256 else ())
    if entry == "ola_norm_len":
        return ("ola_norm_len_kernel", f"ola_norm_len_kernel[{'vector' if on_T(d) % 4 == 0 else 'scalar'} stores]")
    total = d["R"] * (ola_Tout(d) if entry == "ola_fwd" else d["Tp"] * d["Lhop"][0])
    return (f"{entry}_kernel",) + ((f"{entry}_kernel[bias {'on' if d['bias'] else 'NULL'}]",) if entry == "ola_fwd" else ()) + (
        (f"{entry}_kernel[grid-stride]",) if total > 32768 * 256 else ())


def _inst(entry):
    k = {"stft_bandsplit": "stft_bandsplit_kernel", "mask_istft_frames": "mask_istft_frames_kernel",
         "mask_istft_bwd": "mask_istft_bwd_kernel"}.get(entry)
    if k:
        return [k] + [f"{k}[bands {b}]" for b in BANDS] + [f"{k}[last workgroup full]", f"{k}[last workgroup with idle waves]"] + (
            [f"{k}[lengths off]", f"{k}[lengths on]"] if entry == "stft_bandsplit" else []) + [f"{entry}[nframes {n}]" for n in NFRAMES]
    if entry == "istft_ola":
        return ["istft_ola_kernel", "istft_ola_kernel[lengths off]", "istft_ola_kernel[lengths on]", "istft_ola_kernel[grid-stride]"]
    if entry == "ola_norm_len":
        return ["ola_norm_len_kernel", "ola_norm_len_kernel[vector stores]", "ola_norm_len_kernel[scalar stores]"]
    return [f"{entry}_kernel", f"{entry}_kernel[grid-stride]"] + ([f"{entry}_kernel[bias on]", f"{entry}_kernel[bias NULL]"] if entry == "ola_fwd" else [])


INST = {e: _inst(e) for e in ENTRIES}
# R * Tf = 3, 15, 16, 17, 32, 33 (Tf = 1 + T / 128): the last workgroup full, and with 13, 1, 15, 16, 15 idle frames
_NF_FIX = [dict(R=1, T=257), dict(R=3, T=513), dict(R=5, T=383), dict(R=1, T=1920), dict(R=4, T=384), dict(R=1, T=2049),
           dict(R=2, T=1920), dict(R=4, T=1000), dict(R=3, T=1280)]
_M = gc.MIN_PER_TARGET


def _nf_topup(entry):
    return [(f, f"{entry}[nframes {f['R'] * (1 + f['T'] // HOP)}]", 1) for f in _NF_FIX]


TOPUP = {
    "stft_bandsplit": _nf_topup("stft_bandsplit") + [({"bands": b}, f"stft_bandsplit_kernel[bands {b}]", _M) for b in BANDS] + [
        ({"lengths": "mixed", "bands": b}, "stft_bandsplit_kernel[lengths on]", 1) for b in BANDS],
    "mask_istft_frames": _nf_topup("mask_istft_frames"),
    "mask_istft_bwd": _nf_topup("mask_istft_bwd"),
    "istft_ola": [({"lengths": "mixed"}, "istft_ola_kernel[lengths on]", _M)],
    "ola_norm_len": [({"T": t}, f"ola_norm_len_kernel[{'vector' if t == '4h' else 'scalar'} stores]", _M) for t in ("4h", "4h+1")],
    "ola_fwd": [({"Lhop": (7, 3)}, "ola_fwd_kernel", 1)], "ola_bwd": [],
}
gc.DIMS.update(DIMS)
gc.RULES.update(RULES)
gc.SEEDS.update({e: 71 + i for i, e in enumerate(ENTRIES)})
gc.INST.update(INST)
gc.TOPUP.update(TOPUP)
for _e in ENTRIES:
    gc.PLANNERS[_e] = (lambda e: lambda d, seed: _targets(e, d, seed))(_e)

# grid-stride extras, just past the cap of each capped launcher (ws_istft_ola: 8192 blocks of 256; ws_ola_fwd / ws_ola_bwd:
# 32768 blocks of 256).  ws_ola_norm_len caps at 32768 blocks of 256 threads of 4 samples: 33.5 M samples and twice that in
# frames, which no test of a few hundred milliseconds can hold -- recorded in profiles/stft_contract.md as not seen.
EXTRA = {
    "istft_ola": [dict(T=8192 * 256 + 77, R=1, lengths="off", data="gauss")],
    "ola_fwd": [dict(Lhop=(4, 4), Tp=32768 * 64 + 3, Tout="full-1", bias=1, R=1)],
    "ola_bwd": [dict(Lhop=(4, 4), Tp=32768 * 64 + 3, Tout="full-1", R=1)],
}
_COMPOSED = [dict(T=1000, R=3, bands=b, lengths="off", data="gauss") for b in BANDS] + [
    dict(T=513, R=2, bands="bsrnn16k", lengths="off", data="tone-bin64"), dict(T=257, R=1, bands="uneven", lengths="off", data="impulse-255")]


def _name(d):
    return "-".join(f"{v[0]}x{v[1]}" if isinstance(v, tuple) else str(v) for v in d.values())


def cases(entry):
    if entry == COMPOSED:
        return [Case(COMPOSED, f"c{i}-" + _name(d), d, ("composed",), 9000 + i) for i, d in enumerate(_COMPOSED)]
    out = list(gc.cases(entry))
    for i, d in enumerate(EXTRA.get(entry, [])):
        out.append(Case(entry, f"x{i:02d}-" + _name(d), d, _targets(entry, d), 8000 + i))
    return out


def invalid_pairs(entry):
    return gc.invalid_pairs(entry)


# ------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------
class SBuilt(Built):
    def __init__(self, case):
        super().__init__(case)
        self.spec, self.sizes = {}, {}

    def views(self, tensors):
        """name -> float64 numpy view from where the call's tensor starts to the end of the allocation."""
        return {k: v[GUARD:].double().numpy() for k, v in tensors.items()}


def length_table(kind, T, R, seed, unit=HOP):
    """Per-row valid samples: None (off), or R values of the pattern; `unit` = the hop (min = 2 * unit + 1)."""
    lo = 2 * unit + 1
    if kind == "off":
        return None
    if kind == "full":
        return [T] * R
    if kind == "min":
        return [lo] * R
    if kind == "k128":
        return [max((T - 1) // unit * unit, 2 * unit if unit != HOP else 3 * unit)] * R
    rows = [lo, T - 1, T, max((T + 1) // unit * unit - 1, 3 * unit - 1)]
    return [rows[(i + seed) % 4] for i in range(R)]


def _input(b, name, data, fill):
    data = np.asarray(data, dtype=np.float32).reshape(-1)
    t = gc.alloc(data.size, fill)
    t[GUARD:GUARD + data.size] = torch.from_numpy(data)
    b.bufs[name], b.sizes[name] = t, data.size


def _output(b, name, n):
    t = gc.alloc(n, SENT)
    t[GUARD:GUARD + n] = NAN
    b.bufs[name], b.sizes[name] = t, n
    b.outs.append(name)


def wav_rows(rng, kind, lens, T, fill):
    R = len(lens)
    x = np.full((R, T), fill, dtype=np.float64)
    for r, Tr in enumerate(lens):
        n = np.arange(Tr)
        if kind.startswith("impulse"):
            row = np.zeros(Tr)
            row[Tr - 1 if kind == "impulse-last" else int(kind.split("-")[1])] = 1.5 * (-1) ** r
        elif kind == "dc":
            row = np.full(Tr, 0.75)
        elif kind == "tone-bin64":
            row = np.cos(2 * np.pi * 64 * n / NFFT + 0.3 * r)
        else:
            row = rng.standard_normal(Tr) * (1e3 if kind == "row-x1e3" and r == R // 2 else 1.0) + (1000.0 if kind == "offset" else 0.0)
        x[r, :Tr] = row
    return x


def _dense(rng, shape, kind):
    x = rng.standard_normal(shape)
    if kind == "row-x1e3":
        x[shape[0] // 2] *= 1e3
    if kind == "offset":
        x += 1000.0
    return x


def _spec_data(rng, NF, widths, kind):
    if not kind.startswith("bin-"):
        return _dense(rng, (NF, 2 * NBIN), kind)
    re, im, _ = band_cols(widths)
    k = int(kind.split("-")[1])
    x = np.zeros((NF, 2 * NBIN))
    x[:, re[k]], x[:, im[k]] = rng.standard_normal(NF), rng.standard_normal(NF)
    return x


def _mask_data(rng, NF, widths, kind):
    _, _, mc = band_cols(widths)
    m = rng.standard_normal((NF, 4 * NBIN))
    if kind == "sat":
        m[:, np.concatenate([mc[2], mc[3]])] = np.where(rng.random((NF, 2 * NBIN)) < 0.5, -30.0, 30.0)
    if kind == "zero-gate":     # gate logits exactly 0: both sigmoids exactly 0.5, s (1 - s) exactly 0.25
        m[:, np.concatenate([mc[2], mc[3]])] = 0.0
    return m


def build(case, garbage=False):
    e, d = case.entry, case.dims
    if e == COMPOSED:
        e = "stft_bandsplit"
    fill = GARBAGE if garbage else NAN
    rng = np.random.default_rng(case.seed)
    b = SBuilt(case)
    sp = b.spec
    if e in ("stft_bandsplit", "mask_istft_frames", "istft_ola", "mask_istft_bwd"):
        R, T = d["R"], d["T"]
        Tf = 1 + T // HOP
        sp.update(R=R, T=T, Tf=Tf, lens=length_table(d.get("lengths", "off"), T, R, case.seed))
        if "bands" in d:
            sp.update(bands=d["bands"], widths=band_table(d["bands"]))
    if e == "stft_bandsplit":
        _input(b, "wav", wav_rows(rng, d["data"], _lens(sp), T, fill), fill)
        _output(b, "xbs", R * Tf * 2 * NBIN)
    elif e == "mask_istft_frames":
        _input(b, "xbs", _spec_data(rng, R * Tf, sp["widths"], d["data"]), fill)
        _input(b, "m3", _mask_data(rng, R * Tf, sp["widths"], d["mask"]), fill)
        _output(b, "frames", R * Tf * NFFT)
    elif e == "istft_ola":
        fr = _dense(rng, (R, Tf, NFFT), d["data"])
        for r, Tr in enumerate(_lens(sp)):
            fr[r, 1 + Tr // HOP:] = fill
        _input(b, "frames", fr, fill)
        _output(b, "wav", R * T)
    elif e == "mask_istft_bwd":
        _input(b, "dwav", wav_rows(rng, d["data"], [T] * R, T, fill), fill)
        _input(b, "xbs", _dense(rng, (R * Tf, 2 * NBIN), d["spec"]), fill)
        _input(b, "m3", _mask_data(rng, R * Tf, sp["widths"], d["mask"]), fill)
        _output(b, "dm3", R * Tf * 4 * NBIN)
    elif e == "ola_norm_len":
        n, R, T = d["n"], d["R"], on_T(d)
        hop = n // 2
        Tf = 1 + T // hop
        sp.update(n=n, R=R, T=T, Tf=Tf, lens=length_table(d["lengths"], T, R, case.seed, hop))
        fr = _dense(rng, (R, Tf, n), d["data"])
        for r, ln in enumerate(sp["lens"]):
            fr[r, 1 + ln // hop:] = fill
        _input(b, "frames", fr, fill)
        _input(b, "win", np.sin(np.pi * (np.arange(n) + 0.5) / n), fill)
        _output(b, "est", R * T)
    else:
        (L, hop), Tp, R = d["Lhop"], d["Tp"], d["R"]
        Tout = ola_Tout(d)
        sp.update(L=L, hop=hop, Tp=Tp, R=R, Tout=Tout, bias=d.get("bias", 0))
        if e == "ola_fwd":
            _input(b, "frames", rng.standard_normal((R, Tp, L), dtype=np.float32), fill)
            _input(b, "bias", [0.625], fill)
            _output(b, "est", R * Tout)
        else:
            _input(b, "dest", rng.standard_normal((R, Tout), dtype=np.float32), fill)
            _output(b, "dframes", R * Tp * L)
    return b


def reference(b, tensors=None, defect=None, entry=None):
    e = entry or ("stft_bandsplit" if b.case.entry == COMPOSED else b.case.entry)
    return REFS[e](b.spec, b.views(tensors or b.bufs), defect)


# ------------------------------------------------------------------------------------------------------------
# the calls
# ------------------------------------------------------------------------------------------------------------
_BT = {}


def bands_on(mod, name, device):
    key = (name, str(device))
    if key not in _BT:
        _BT[key] = mod.BandTables(band_table(name), device)
    return _BT[key]


def _len_tensor(lens, device):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=device)


def run(mod, b, tensors, device, entry=None, lens="spec"):
    """The case's call on `mod` (wesep_amd.dev) over `tensors` (the allocations on `device`)."""
    e, sp = entry or b.case.entry, b.spec
    v = {k: t[GUARD:GUARD + b.sizes[k]] for k, t in tensors.items()}
    lt = _len_tensor(sp.get("lens") if lens == "spec" else lens, device)
    if e == "stft_bandsplit":
        mod.stft_bandsplit(v["wav"].view(sp["R"], sp["T"]), bands_on(mod, sp["bands"], device), v["xbs"], lengths=lt)
    elif e == "mask_istft_frames":
        mod.mask_istft_frames(v["xbs"], v["m3"], sp["R"], sp["Tf"], bands_on(mod, sp["bands"], device), v["frames"])
    elif e == "istft_ola":
        mod.istft_ola(v["frames"], sp["R"], sp["Tf"], sp["T"], v["wav"], lengths=lt)
    elif e == "mask_istft_bwd":
        mod.mask_istft_bwd(v["dwav"], v["xbs"], v["m3"], sp["R"], sp["Tf"], sp["T"], bands_on(mod, sp["bands"], device), v["dm3"])
    elif e == "ola_norm_len":
        mod.ola_norm_len(v["frames"], v["win"], sp["R"], sp["Tf"], sp["n"], sp["T"], lt, v["est"])
    elif e == "ola_fwd":
        mod.ola_fwd(v["frames"], v["bias"] if sp["bias"] else None, sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"], v["est"])
    else:
        mod.ola_bwd(v["dest"], sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"], v["dframes"])
    return {}


def refusals(dev, t, device):
    """(name, call): argument sets the WS_REQUIRE rules refuse; every call has to raise without launching."""
    bt = bands_on(dev, "one", device)
    bad = dev.BandTables([256], device)
    i32 = torch.full((8,), 300, dtype=torch.int32, device=device)
    w = lambda T: t[:2 * T].view(2, T)
    return [
        ("stft_bandsplit T = 256", lambda: dev.stft_bandsplit(w(256), bt, t)),
        ("stft_bandsplit_len T = 256", lambda: dev.stft_bandsplit(w(256), bt, t, lengths=i32)),
        ("stft_bandsplit nbins = 256", lambda: dev.stft_bandsplit(w(512), bad, t)),
        ("mask_istft_frames Tf = 0", lambda: dev.mask_istft_frames(t, t, 2, 0, bt, t)),
        ("mask_istft_frames nbins = 256", lambda: dev.mask_istft_frames(t, t, 2, 4, bad, t)),
        ("istft_ola Tf != 1 + T / 128", lambda: dev.istft_ola(t, 2, 4, 512, t)),
        ("istft_ola_len Tf != 1 + T / 128", lambda: dev.istft_ola(t, 2, 6, 512, t, lengths=i32)),
        ("istft_ola R = 0", lambda: dev.istft_ola(t, 0, 5, 512, t)),
        ("mask_istft_bwd Tf != 1 + T / 128", lambda: dev.mask_istft_bwd(t, t, t, 2, 4, 512, bt, t)),
        ("mask_istft_bwd nbins = 256", lambda: dev.mask_istft_bwd(t, t, t, 2, 5, 512, bad, t)),
        ("ola_norm_len n = 12", lambda: dev.ola_norm_len(t, t, 2, 1 + 100 // 6, 12, 100, i32, t)),
        ("ola_norm_len Tf != 1 + T / hop", lambda: dev.ola_norm_len(t, t, 2, 7, 16, 100, i32, t)),
        ("ola_fwd Tout > (Tp - 1) * hop + L", lambda: dev.ola_fwd(t, None, 2, 3, 20, 10, 41, t)),
        ("ola_fwd hop = 0", lambda: dev.ola_fwd(t, None, 2, 3, 20, 0, 20, t)),
        ("ola_bwd Tout = 0", lambda: dev.ola_bwd(t, 2, 3, 20, 10, 0, t)),
    ]


# ------------------------------------------------------------------------------------------------------------
# checker
# ------------------------------------------------------------------------------------------------------------
def verify(b, ref, after, extra=None, what=None):
    """Every output of a built case (`after`: name -> whole CPU allocation after the launch) against `ref`.  Returns the
    worst err / bound.  Raises ContractViolation: nan | exact | bound | sentinel."""
    what = what or b.case.name
    return max(check(after[k], b.bufs[k], r, f"{what} {k}", GUARD) for k, r in ref.items())


def output_bits(b, after, extra=None):
    return torch.cat([after[n].contiguous().view(torch.int32).reshape(-1) for n in b.outs])


def planted(b, ref):
    """The allocations a kernel leaves that writes exactly (idx, fp32(val)) of `ref` -- the reference itself, or a defective
    reference: an index outside the write set lands in the sentinels or the guard."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    for k, r in ref.items():
        after[k][r.idx + GUARD] = r.val.float()
    return after


# ------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' own arithmetic (host test)
# ------------------------------------------------------------------------------------------------------------
_H = np.float32(0.70710678118654752440)
_W81, _W83 = np.complex64(complex(_H, -_H)), np.complex64(complex(-_H, -_H))


def _mi(a):
    return (a.imag - 1j * a.real).astype(np.complex64)


def dft8_32(v):
    """stft.hip's dft8 over axis 0 of a complex64 array [8, ...]."""
    a0, a4, a1, a5 = v[0] + v[4], v[0] - v[4], v[1] + v[5], v[1] - v[5]
    a2, a6, a3, a7 = v[2] + v[6], v[2] - v[6], v[3] + v[7], v[3] - v[7]
    a5, a6, a7 = a5 * _W81, _mi(a6), a7 * _W83
    b0, b2, b1, b3 = a0 + a2, a0 - a2, a1 + a3, _mi(a1 - a3)
    c0, c2, c1, c3 = a4 + a6, a4 - a6, a5 + a7, _mi(a5 - a7)
    return np.stack([b0 + b1, c0 + c1, b2 + b3, c2 + c3, b0 - b1, c0 - c1, b2 - b3, c2 - c3]).astype(np.complex64)


def fft512_32(x, tw=TW32):
    """stft.hip's fft512 in complex64: x [F, 512] -> X [F, 512]; 512 = 8 * 8 * 8, n = 64 n1 + 8 n2 + n3, k = k1 + 8 k2 + 64 k3."""
    F = x.shape[0]
    a = np.moveaxis(x.astype(np.complex64).reshape(F, 8, 8, 8), 0, -1)          # [n1, n2, n3, F]
    i8 = np.arange(8)
    a = dft8_32(a)                                                                # [k1, n2, n3, F]
    a = a * tw[((8 * i8[None, :, None] + i8[None, None, :]) * i8[:, None, None]) % NFFT][..., None]
    a = np.moveaxis(dft8_32(np.moveaxis(a, 1, 0)), 0, 1)                          # [k1, k2, n3, F]
    a = a * tw[(8 * i8[None, None, :] * i8[None, :, None]) % NFFT][..., None]
    a = np.moveaxis(dft8_32(np.moveaxis(a, 2, 0)), 0, 2)                          # [k1, k2, k3, F]
    return np.moveaxis(a, -1, 0).transpose(0, 3, 2, 1).reshape(F, NFFT)


def _sig32(x):
    one = np.float32(1)
    with np.errstate(over="ignore"):
        return (one / (one + np.exp(-x, dtype=np.float32))).astype(np.float32)


def _env32(T, tmax):
    q = np.arange(T) + NFFT // 2
    e = np.zeros(T, dtype=np.float32)
    for j in range(3, -1, -1):      # ascending t
        t = q // HOP - j
        ok = (t >= 0) & (t <= tmax)
        w = WIN32[q - HOP * t]
        e = np.where(ok, e + w * w, e).astype(np.float32)
    return e


def emulate(b):
    """name -> the output (natural layout, float32) of correct fp32 arithmetic in the kernel's own order."""
    e, sp = b.case.entry, b.spec
    v = {k: t[GUARD:GUARD + b.sizes[k]].numpy() for k, t in b.bufs.items() if k not in b.outs}
    f32 = np.float32
    if e == "stft_bandsplit":
        R, T, Tf = sp["R"], sp["T"], sp["Tf"]
        re, im, _ = band_cols(sp["widths"])
        out = np.zeros((R, Tf, 2 * NBIN), dtype=f32)
        for r, Tr in enumerate(_lens(sp)):
            ntf = 1 + Tr // HOP
            X = fft512_32(v["wav"][r * T:(r + 1) * T][frame_index(Tr, T, ntf)] * WIN32[None, :])
            out[r, :ntf, re], out[r, :ntf, im] = X.real[:, :NBIN].T, X.imag[:, :NBIN].T
        return {"xbs": out}
    if e in ("mask_istft_frames", "mask_istft_bwd"):
        NF = sp["R"] * sp["Tf"]
        re, im, mc = band_cols(sp["widths"])
        xbs, m3 = v["xbs"].reshape(NF, -1), v["m3"].reshape(NF, -1)
        Xr, Xi, o0, o1, s0, s1 = xbs[:, re], xbs[:, im], m3[:, mc[0]], m3[:, mc[1]], _sig32(m3[:, mc[2]]), _sig32(m3[:, mc[3]])
    if e == "mask_istft_frames":
        mre, mim = o0 * s0, o1 * s1
        er, ei = Xr * mre - Xi * mim, Xr * mim + Xi * mre
        ei[:, 0] = ei[:, NBIN - 1] = 0
        Y = np.concatenate([er - 1j * ei, (er + 1j * ei)[:, NBIN - 2:0:-1]], axis=1).astype(np.complex64)
        return {"frames": (fft512_32(Y).real * f32(1.0 / NFFT) * WIN32[None, :]).astype(f32)}
    if e == "istft_ola":
        R, T, Tf = sp["R"], sp["T"], sp["Tf"]
        fr = v["frames"].reshape(R, Tf, NFFT)
        out = np.zeros((R, T), dtype=f32)
        q = np.arange(T) + NFFT // 2
        for r, Tr in enumerate(_lens(sp)):
            y = np.zeros(T, dtype=f32)
            for j in range(3, -1, -1):
                t = q // HOP - j
                ok = (t >= 0) & (t <= Tr // HOP)
                y = np.where(ok, y + np.where(ok, fr[r, np.clip(t, 0, Tf - 1), q - HOP * t], 0), y).astype(f32)
            out[r, :Tr] = y[:Tr] / _env32(T, Tr // HOP)[:Tr]
        return {"wav": out}
    if e == "mask_istft_bwd":
        R, T, Tf = sp["R"], sp["T"], sp["Tf"]
        dw = v["dwav"].reshape(R, T)
        env = _env32(T, Tf - 1)
        p = HOP * np.arange(Tf)[:, None] + np.arange(NFFT)[None, :] - NFFT // 2
        ok, pc = (p >= 0) & (p < T), np.clip(p, 0, T - 1)
        out = np.zeros((NF, 4 * NBIN), dtype=f32)
        sc = (_CK / NFFT).astype(f32)
        for r in range(R):
            dv = np.where(ok, dw[r][pc] * WIN32[None, :] / env[pc], 0).astype(f32)
            V = fft512_32(dv)[:, :NBIN]
            gre, gim = V.real * sc, V.imag * sc
            gim[:, 0] = gim[:, NBIN - 1] = 0
            rows = slice(r * Tf, (r + 1) * Tf)
            for c, dm, o, s in ((0, gre * Xr[rows] + gim * Xi[rows], o0[rows], s0[rows]),
                                (1, -gre * Xi[rows] + gim * Xr[rows], o1[rows], s1[rows])):
                out[rows, mc[c]] = dm * s
                out[rows, mc[2 + c]] = dm * o * s * (f32(1) - s)
        return {"dm3": out}
    if e == "ola_norm_len":
        R, T, Tf, n = sp["R"], sp["T"], sp["Tf"], sp["n"]
        hop, fr, win = n // 2, v["frames"].reshape(R, Tf, n), v["win"]
        i = np.arange(T)
        t1 = (i + hop) // hop
        k = i + hop - t1 * hop
        out = np.zeros((R, T), dtype=f32)
        for r, ln in enumerate(sp["lens"]):
            two = t1 < 1 + ln // hop
            env = win[hop + k].astype(np.float64) ** 2 + np.where(two, win[k].astype(np.float64) ** 2, 0.0)
            s = np.where(two, fr[r, t1 - 1, hop + k] + np.where(two, fr[r, np.minimum(t1, Tf - 1), k], 0), fr[r, t1 - 1, hop + k]).astype(f32)
            out[r, :ln] = (s * (1.0 / env).astype(f32))[:ln]
        return {"est": out}
    R, Tp, L, hop, Tout = sp["R"], sp["Tp"], sp["L"], sp["hop"], sp["Tout"]
    if e == "ola_fwd":
        fr = v["frames"].reshape(R, Tp, L)
        j = np.arange(Tout)
        acc = np.full((R, Tout), v["bias"][0] if sp["bias"] else 0, dtype=f32)
        for k in range(-(-L // hop) - 1, -1, -1):
            t = j // hop - k
            nn = j - hop * t
            ok = (t >= 0) & (t < Tp) & (nn < L)
            acc = np.where(ok[None], acc + np.where(ok[None], fr[:, np.clip(t, 0, Tp - 1), np.clip(nn, 0, L - 1)], 0), acc).astype(f32)
        return {"est": acc}
    j = hop * np.arange(Tp)[:, None] + np.arange(L)[None, :]
    d = v["dest"].reshape(R, Tout)
    return {"dframes": np.where((j < Tout)[None], d[:, np.minimum(j, Tout - 1)], 0).astype(f32)}


def emulated(b):
    after = {k: t.clone() for k, t in b.bufs.items()}
    for k, o in emulate(b).items():
        after[k][GUARD:GUARD + o.size] = torch.from_numpy(np.ascontiguousarray(o, dtype=np.float32).reshape(-1))
    return after


# ------------------------------------------------------------------------------------------------------------
# planted defects: (name, entry, the cases it can show on, what it is)
# ------------------------------------------------------------------------------------------------------------
def _has_tail(c):
    return c.dims.get("lengths", "off") in ("min", "k128", "mixed")


DEFECTS = [
    ("reflect-T", "stft_bandsplit", None, "reflect turning at T instead of T - 1"),
    ("left-reflect", "stft_bandsplit", None, "left reflect off by one"),
    ("symmetric-hann", "stft_bandsplit", None, "symmetric (N - 1) instead of periodic Hann"),
    ("tf-ceil", "stft_bandsplit", lambda c: c.dims["T"] % HOP == 0, "Tf = ceil(T / 128)"),
    ("re-im-swapped", "stft_bandsplit", None, "re and im halves of a band swapped"),
    ("neighbour-bw", "stft_bandsplit", lambda c: c.dims["bands"] in ("bsrnn16k", "uneven"), "bw of the neighbouring band in the scatter offset"),
    ("reflect-T-len", "stft_bandsplit", _has_tail, "reflect at T under lengths"),
    ("tail-not-zero", "stft_bandsplit", _has_tail, "tail frames not zero"),
    ("twiddle", "stft_bandsplit", lambda c: c.dims["data"] in ("impulse-255", "impulse-257"), "table entry 1 perturbed by 2^-20 relative"),
    ("nyquist-im-kept", "mask_istft_frames", None, "Im of Nyquist not dropped in the inverse"),
    ("edge-x2", "mask_istft_bwd", None, "DC / Nyquist scaled by 2 in the backward"),
    ("env-last-missing", "istft_ola", None, "the last frame missing from the envelope"),
    ("env-all-frames", "istft_ola", _has_tail, "the envelope counting all Tf frames under lengths"),
    ("tail-not-zero", "istft_ola", _has_tail, "tail samples not zero"),
    ("t_lo", "ola_fwd", lambda c: c.dims["Lhop"] == (7, 3) and c.dims["Tp"] > 1, "t_lo off by one where hop does not divide L"),
    ("bias-per-frame", "ola_fwd", lambda c: c.dims["bias"] == 1 and c.dims["Tp"] > 1, "bias added per frame"),
    ("no-zero-past-Tout", "ola_bwd", lambda c: c.dims["Tout"] != "full", "ola_bwd not zero past Tout"),
]
# "Im of Nyquist not dropped" cannot be refused: the real part of the inverse transform does not depend on it (its basis
# function is sin(pi n) = 0), so the planted output EQUALS the reference; the host test asserts that identity instead.
INVISIBLE = ("nyquist-im-kept",)
