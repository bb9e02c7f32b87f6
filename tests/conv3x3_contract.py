"""TEST INFRASTRUCTURE ONLY -- contract suite of the 3 x 3 halo convolutions of wesep_amd/csrc/conv3x3.hip (ws_conv3x3,
ws_conv3x3_pack, ws_conv3x3_wgrad; include/wesep_hip.h).  Same shape as tests/gemm_contract.py and tests/blk_contract.py; Ref,
check, eps_for, the guards, draw and the pairwise generator with its registries are imported from gemm_contract.  No GPU code
here: the CPU test (test_conv3x3_contract_host_cpu.py) checks this module, the GPU test (test_conv3x3_contract_gpu.py) runs every
case through the C ABI.

1. REFERENCE.  ref_conv3x3 / ref_conv3x3_pack / ref_conv3x3_wgrad take the keyword arguments of the wesep_amd.dev wrappers on CPU
   tensors and restate the header in float64 as explicit gathers over (b, h, w, ky, kx, c) -- no F.conv2d, no
   torch.nn.grad.conv2d_weight: tests/emu_dev.py is built on those and serves as the independent second opinion.
     conv3x3        Y[m][y_off + n] = bias[n] + R[m][y_off + n] + sum X[pixel(m) + (ky - 1, kx - 1)][x_off + c] W[n][(ky*3 + kx)*Cin + c],
                    zero outside the image; write set = columns [y_off, y_off + Cout) of the B*H*Wd rows of stride ldy.  W is the
                    fp32 matrix the pack was made from: the pack's representation error is the kernel's to answer for.
     conv3x3_wgrad  one Ref per buffer, split-major.  Split s sums the pixels of tiles [s * tps, min(ntiles, (s + 1) * tps));
                    tile t = (b, rt, cg), cg = t % ceil(Wd / 4), rt = (t / ceil(Wd / 4)) % ceil(H / 30), 30 rows x 4 columns;
                    image column sw * w + kx - 1.  A split with no tile is an EXACT statement: every element 0.0.
     conv3x3_pack   the unit formula in numpy, element by element: unit (((chunk*9 + tap)*NTP + t)*2 + part)*64 + lane, element j
                    = W[t*32 + (lane & 31)][tap][16 chunk + 8 (lane >> 5) + j], W gathered from the sources by
                    w_k[n*s_row + (c - col_off)*s_col + (flip ? 8 - tap : tap)*s_tap]; part 0 = round-to-nearest-even bf16 (on the
                    bit pattern, not through torch), part 1 = bf16 of the remainder; zero beyond Cout / Cin and in columns no source
                    covers.  Exact: the whole buffer is compared as bits.  Weights are zero or normal fp32 in [2^-20, 2^4] -- no
                    subnormals: the header does not say how the conversion treats them.
   The two composed cases (entry "conv3x3_composed") run the pair the way the dense block does: a layer's forward through
   conv3x3_pack_srcs with one [co][ci][3][3] source, and the input gradient of a channel block -- several layers' weights side by
   side, flip = 1, X = dY, Y = R -- against the float64 gather of the ADJOINT of the layers' forward (ref_dense_dx), which knows
   nothing of flipped taps or swapped strides.

2. BOUND.  No new constants: |out - ref| <= eps_for(True, K) * S + 2^-24 |R| (gemm_contract's docstring: split-bf16, three
   products, fp32 accumulation), S = the same sum over absolute values.  Forward: K = 9 * Cin.  Weight-gradient slab: K = the
   grid pixels of the split.  bslab: eps_for(False, K), a plain fp32 sum.  Derived, not tuned.

3. CASES.  cases(entry) through gemm_contract's pairwise generator over C3_DIMS / WG3_DIMS / PK3_DIMS: the smallest values at
   which each tile seam (32 rows, 8 / 16 columns; 30 rows, 4 columns), chunk seam (16 / 32 channels), channel-tile seam (32, 64
   and the padded third tile) and dispatcher switch (Wd >= 100, Cout <= 32, Cin > 16, Nn <= 16, sw) is crossed.  `targets`
   mirrors ws_conv3x3 / ws_conv3x3_wgrad with WS_CONV3X3_VARIANT and WS_CONV3X3_WGRAD16 unset.

BUFFERS (build(case)).  GUARD floats on both sides of every operand and output.  Outputs: the write set starts as NaN (with R
aliasing Y as the residual), everything else holds SENT and must be bit-identical afterwards: ldy tails, columns outside
[y_off, y_off + Cout), slab rows behind Nn*9*Cin up to slab_stride, bslab behind Nn, pack floats behind conv3x3_pack_floats.
Inputs: everything the contract does not read is NaN -- X columns outside [x_off, x_off + Cin), G columns outside
[g_off, g_off + Nn), R outside the write set, the guards, every pack-source element the gather does not name.
build(case, garbage=True) puts a large finite value there instead."""
import numpy as np
import torch

from tests import gemm_contract as gc
from tests.gemm_contract import (GUARD, SENT, U, Buf, Built, Case, ContractViolation, Ref, check, draw, eps_for)  # noqa: F401

GARBAGE = 3.0e30
NAN = float("nan")
ENTRIES = ("conv3x3", "conv3x3_wgrad", "conv3x3_pack")
COMPOSED = "conv3x3_composed"


def pack_geometry(Cin, Cout):
    """(NTP, chunks, floats of the pack): NTP = ceil(Cout / 32) rounded up to even when above 2."""
    ntt, nch = -(-Cout // 32), -(-Cin // 16)
    ntp = ntt if ntt <= 2 else ntt + (ntt & 1)
    return ntp, nch, nch * 9 * ntp * 2 * 64 * 8 // 2


def bf16_bits(x):
    """Round-to-nearest-even bf16 of a finite float32 array, on the bit pattern."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


# ------------------------------------------------------------------------------------------------------------
# references
# ------------------------------------------------------------------------------------------------------------
def _pixels(B, H, Wd):
    m = torch.arange(B * H * Wd)
    return m, m // (H * Wd), (m // Wd) % H, m % Wd


def _gather(Xf, pix, ok, ld, off, Cc):
    """[M, 9 * Cc] float64: channel c of the tap pixels, zero where the tap leaves the image."""
    idx = (pix * ld + off).unsqueeze(-1) + torch.arange(Cc)
    a = torch.where(ok.unsqueeze(-1), Xf[idx].double(), torch.zeros((), dtype=torch.float64))
    return a.reshape(pix.shape[0], -1)


def _hi(x):
    return x.float().bfloat16().double()


def ref_conv3x3(*, X, ldx, W, ldw, B, H, Wd, Cin, Cout, Y, ldy, bias=None, R=None, x_off=0, y_off=0, defect=None):
    """W: the fp32 matrix [Cout][ldw >= 9 * Cin] the pack was made from.  defect: the output of a kernel with a planted defect
    (host test)."""
    M = B * H * Wd
    m, b, h, w = _pixels(B, H, Wd)
    tap = torch.arange(9)
    ky, kx = tap // 3, tap % 3
    hh, ww = h.unsqueeze(1) + ky - 1, w.unsqueeze(1) + kx - 1
    okh, okw = (hh >= 0) & (hh < H), (ww >= 0) & (ww < Wd)
    if defect == "wrap_w":          # the tap right of the last column reads the next row's first pixel
        okw = ww >= 0
    if defect == "wrap_h":          # the tap above the first row reads the previous image's last row
        okh = hh < H
    pix = (b.unsqueeze(1) * H + hh) * Wd + ww
    ok = okh & okw & (pix >= 0) & (pix < M)
    pix = torch.where(ok, pix, torch.zeros_like(pix))
    Xf = X.reshape(-1)
    a = _gather(Xf, pix, ok, ldx, x_off, Cin)
    wm = W.reshape(-1)[:Cout * ldw].reshape(Cout, ldw)[:, :9 * Cin].double()
    if defect == "kykx":
        wm = wm.reshape(Cout, 3, 3, Cin).transpose(1, 2).reshape(Cout, 9 * Cin)
    av, wv = (a, wm) if defect != "drop_lo" else (_hi(a), _hi(wm))
    v, S = av @ wv.t(), a.abs() @ wm.abs().t()
    if defect == "no_cin_select":   # channels Cin .. 16 ceil(Cin / 16) of every tap pixel meet the pack's zero weights
        pad = -(-Cin // 16) * 16 - Cin
        idx = ((pix * ldx + x_off + Cin).unsqueeze(-1) + torch.arange(pad)).clamp_max(Xf.numel() - 1)
        junk = torch.where(ok.unsqueeze(-1), Xf[idx].double(), torch.zeros((), dtype=torch.float64))
        v = v + (0.0 * junk).sum((1, 2)).unsqueeze(1)
    if bias is not None:
        bv = bias.reshape(-1)[:Cout].double()
        S = S + bv.abs()
        if defect == "bias_last_quad":
            bv = bv.clone()
            bv[-4:] = 0
        v = v + bv
    bound = eps_for(True, 9 * Cin) * S
    n = torch.arange(Cout)
    cidx = (m * ldy + y_off).unsqueeze(1) + n
    if R is not None:
        r = R.reshape(-1)[cidx].double()
        bound = bound + U * r.abs()
        if defect == "R_stride":    # R read with stride Cout instead of ldy
            r = R.reshape(-1)[(m * Cout + y_off).unsqueeze(1) + n].double()
        v = v + r
    z = torch.zeros(M * Cout, dtype=torch.bool)
    return {"Y": Ref(cidx.reshape(-1), v.reshape(-1), S.reshape(-1), bound.reshape(-1), z)}


def wgrad_tiles(B, H, Wd):
    return B * (-(-H // 30)) * (-(-Wd // 4))


def ref_conv3x3_wgrad(*, G, ldg, X, ldx, B, H, Wd, Cin, Nn, slab, nsplit, tiles_per_split, bslab=None, sw=1, Wx=0, g_off=0,
                      slab_stride=0, bslab_stride=0, x_off=0, defect=None):
    Wx = Wx or Wd
    slab_stride, bslab_stride = slab_stride or Nn * 9 * Cin, bslab_stride or Nn
    m, b, h, w = _pixels(B, H, Wd)
    ncg, nrt = -(-Wd // 4), -(-H // 30)
    ntiles = B * nrt * ncg
    tile = (b * nrt + h // 30) * ncg + w // 4
    if defect == "row_fastest":
        tile = (b * ncg + w // 4) * nrt + h // 30
    tap = torch.arange(9)
    ky, kx = tap // 3, tap % 3
    hh = h.unsqueeze(1) + ky - 1
    ww = (w if defect == "sw_ignored" else sw * w).unsqueeze(1) + kx - 1
    ok = (hh >= 0) & (hh < H) & (ww >= 0) & (ww < Wx)
    pix = torch.where(ok, (b.unsqueeze(1) * H + hh) * Wx + ww, torch.zeros_like(hh))
    a = _gather(X.reshape(-1), pix, ok, ldx, x_off, Cin)
    g = G.reshape(-1)[(m * ldg + g_off).unsqueeze(1) + torch.arange(Nn)].double()
    if defect == "drop_lo":
        a, g = _hi(a), _hi(g)
    res = {"slab": [], "bslab": []}
    for s in range(nsplit):
        lo, hi = s * tiles_per_split, min(ntiles, (s + 1) * tiles_per_split)
        if defect == "plus_one":
            hi = min(ntiles, hi + 1)
        cnt = ((tile >= lo) & (tile < hi)).double()
        if defect == "seam_twice":   # the first row of a 30-row tile is counted by the tile above as well
            up = tile - ncg
            cnt = cnt + ((h % 30 == 0) & (h > 0) & (up >= lo) & (up < hi)).double()
        sel = cnt.nonzero().reshape(-1)
        k = sel.numel()
        if k:
            gs, as_ = g[sel] * cnt[sel].unsqueeze(1), a[sel]
            S = gs.abs().t() @ as_.abs()
            res["slab"].append(((gs.t() @ as_).reshape(-1), S.reshape(-1), eps_for(True, k) * S.reshape(-1), False))
            bv = gs.sum(0) * (-(-Cin // 32) if defect == "bias_per_chunk" else 1)
            res["bslab"].append((bv, gs.abs().sum(0), eps_for(False, k) * gs.abs().sum(0), False))
        else:
            for key, n in (("slab", Nn * 9 * Cin), ("bslab", Nn)):
                zz = torch.zeros(n, dtype=torch.float64)
                res[key].append((zz, zz.clone(), zz.clone(), True))
    out = {}
    for key, on, n, stride in (("slab", True, Nn * 9 * Cin, slab_stride), ("bslab", bslab is not None, Nn, bslab_stride)):
        if on:
            idx = torch.cat([s * stride + torch.arange(n) for s in range(nsplit)])
            v, S, bd = [torch.cat([r[i] for r in res[key]]) for i in range(3)]
            ex = torch.cat([torch.full((n,), r[3], dtype=torch.bool) for r in res[key]])
            out[key] = Ref(idx, v, S, bd, ex)
    return out


def logical_w(srcs, Cin, Cout, flip):
    """W[n][tap][c] (float32 numpy [Cout, 9, Cin]) as the header gathers it from the sources; zero where no source covers c."""
    Wl = np.zeros((Cout, 9, Cin), np.float32)
    n, tap = np.arange(Cout).reshape(-1, 1, 1), np.arange(9).reshape(1, -1, 1)
    for w, off, s_row, s_col, s_tap, col_off, cols in srcs:
        c = np.arange(cols).reshape(1, 1, -1)
        Wl[:, :, col_off:col_off + cols] = w.reshape(-1).numpy()[off + n * s_row + c * s_col + ((8 - tap) if flip else tap) * s_tap]
    return Wl


def ref_conv3x3_pack(srcs, Cin, Cout, flip=False, out=None, defect=None):
    """The pack as int16 bit patterns [2 * conv3x3_pack_floats]."""
    ntp, nch, nfl = pack_geometry(Cin, Cout)
    Wp = np.zeros((ntp * 32, 9, nch * 16), np.float32)
    Wp[:Cout, :, :Cin] = logical_w(srcs, Cin, Cout, flip and defect != "flip_ignored")
    hi = bf16_bits(Wp)
    lo = bf16_bits(Wp - bf16_value(hi))
    parts = np.stack([lo, hi] if defect == "swap_parts" else [hi, lo])
    chunk, tap, t, part, lane, j = np.meshgrid(np.arange(nch), np.arange(9), np.arange(ntp), np.arange(2), np.arange(64),
                                               np.arange(8), indexing="ij")
    unit = (((chunk * 9 + tap) * ntp + t) * 2 + part) * 64 + lane
    bits = np.zeros(2 * nfl, np.uint16)
    bits[unit * 8 + j] = parts[part, t * 32 + (lane & 31), tap, 16 * chunk + 8 * (lane >> 5) + j]
    return torch.from_numpy(bits.view(np.int16).copy())


def pack_decode(bits, Cin, Cout):
    """hi + lo of a pack (int16 bits) as float64 [Cout, 9, Cin]: the unit formula read backwards."""
    ntp, nch, _ = pack_geometry(Cin, Cout)
    v = bf16_value(bits.numpy().view(np.uint16)).astype(np.float64).reshape(nch, 9, ntp, 2, 2, 32, 8)   # chunk tap t part half l31 j
    v = v[:, :, :, 0] + v[:, :, :, 1]                                                                    # chunk tap t half l31 j
    return torch.from_numpy(v.transpose(2, 4, 1, 0, 3, 5).reshape(ntp * 32, 9, nch * 16)[:Cout, :, :Cin].copy())


def ref_dense_dx(*, dY, ldg, layers, lo, Cb, B, H, Wd, R, ldy, y_off=0):
    """The input gradient of channels [lo, lo + Cb) of a dense block, as the adjoint of the layers' forward
    y_k[b][h][w][co] = sum x[b][h + ky - 1][w + kx - 1][ci] w_k[co][ci][ky][kx]:
      dx[b][h][w][n] = R + sum_k sum_{co, ky, kx} dy[b][h - ky + 1][w - kx + 1][col_k + co] w_k[co][lo + n][ky][kx].
    layers: (w_k [Co][Ci][3][3], col_k) -- dy of layer k is columns [col_k, col_k + Co) of dY."""
    M = B * H * Wd
    m, b, h, w = _pixels(B, H, Wd)
    dyf = dY.reshape(-1)
    v, S = torch.zeros(M, Cb, dtype=torch.float64), torch.zeros(M, Cb, dtype=torch.float64)
    K = 0
    for wk, col in layers:
        Co = wk.shape[0]
        K += 9 * Co
        for ky in range(3):
            for kx in range(3):
                hh, ww = h - ky + 1, w - kx + 1
                ok = (hh >= 0) & (hh < H) & (ww >= 0) & (ww < Wd)
                pix = torch.where(ok, (b * H + hh) * Wd + ww, torch.zeros_like(hh))
                g = torch.where(ok.unsqueeze(1), dyf[(pix * ldg + col).unsqueeze(1) + torch.arange(Co)].double(),
                                torch.zeros((), dtype=torch.float64))
                wt = wk[:, lo:lo + Cb, ky, kx].double()              # [Co, Cb]
                v, S = v + g @ wt, S + g.abs() @ wt.abs()
    cidx = (m * ldy + y_off).unsqueeze(1) + torch.arange(Cb)
    r = R.reshape(-1)[cidx].double()
    bound = eps_for(True, K) * S + U * r.abs()
    return {"Y": Ref(cidx.reshape(-1), (v + r).reshape(-1), S.reshape(-1), bound.reshape(-1), torch.zeros(M * Cb, dtype=torch.bool))}


# ------------------------------------------------------------------------------------------------------------
# dimensions, rules, targets
# ------------------------------------------------------------------------------------------------------------
DATA = ["gauss", "pixel-x1e3", "channel-x1e-3"]
C3_DIMS = {"H": [1, 2, 31, 32, 33, 65], "Wd": [1, 7, 8, 9, 17, 99, 100, 113, 129], "B": [1, 3], "Cin": [4, 12, 16, 20, 32, 36],
           "Cout": [4, 28, 32, 36, 64, 68, 100, 132], "ldx": ["Cin", "Cin+4", "80"], "x_off": ["0", "4", "end"],
           "ldy": ["Cout", "Cout+4", "160"], "y_off": ["0", "4", "end"], "bias": [0, 1], "R": ["off", "alias", "sep"], "data": DATA}
WG3_DIMS = {"H": [1, 29, 30, 31, 61], "Wd": [1, 3, 4, 5, 9, 33], "sw": ["1", "2-Wx-odd", "2-Wx-even"], "B": [1, 3],
            "Cin": [4, 20, 32, 36, 68], "Nn": [4, 12, 16, 20, 32, 36, 68], "ldg": ["Nn", "Nn+4", "80"], "g_off": ["0", "4", "end"],
            "ldx": ["Cin", "Cin+4", "80"], "x_off": ["0", "4", "end"], "split": ["one", "exact", "ragged", "over"], "bslab": [0, 1],
            "strides": ["exact", "padded"], "data": DATA}
PK3_DIMS = {"Cin": [4, 12, 16, 20, 36], "Cout": [4, 32, 36, 64, 68, 132], "nsrc": [1, 2, 5], "flip": [0, 1],
            "layout": ["oihw", "tap-major", "padded"], "cover": ["all", "gap"]}


def _off_rule(ld, off, what):
    return (f"{off} != 0 needs columns beside the range: {ld} > {what}", (ld, off), lambda l, o: l == what and o != "0")


C3_RULES = [_off_rule("ldx", "x_off", "Cin"), _off_rule("ldy", "y_off", "Cout")]
WG3_RULES = [_off_rule("ldg", "g_off", "Nn"), _off_rule("ldx", "x_off", "Cin"),
             ("a ragged split needs three tiles (30 rows x 4 columns)", ("split", "H", "Wd", "B"),
              lambda s, H, Wd, B: s == "ragged" and wgrad_tiles(B, H, Wd) < 3)]
PK3_RULES = [("disjoint non-empty ranges (and a gap) need that many columns", ("nsrc", "Cin", "cover"),
              lambda n, Cin, cover: n + (cover == "gap") > Cin)]


def c3_target(Cin, Cout, Wd):
    """ws_conv3x3's choice with WS_CONV3X3_VARIANT unset."""
    wide, pf = Wd >= 100, Cin > 16
    if Cout <= 32:
        return f"conv3x3_kernel<1,{4 if wide else 2},{'true' if pf else 'false'}>"
    if wide:
        return "conv3x3_kernel<2,4,false>"
    return f"conv3x3_kernel<2,2,{'true' if pf else 'false'}>"


def wg3_target(Nn, sw):
    return f"conv3x3_wgrad{'16' if Nn <= 16 else ''}_kernel<{sw}>"


C3_INST = ["conv3x3_kernel<1,4,true>", "conv3x3_kernel<1,4,false>", "conv3x3_kernel<1,2,true>", "conv3x3_kernel<1,2,false>",
           "conv3x3_kernel<2,4,false>", "conv3x3_kernel<2,2,true>", "conv3x3_kernel<2,2,false>"]
WG3_INST = ["conv3x3_wgrad16_kernel<1>", "conv3x3_wgrad16_kernel<2>", "conv3x3_wgrad_kernel<1>", "conv3x3_wgrad_kernel<2>"]
PK3_INST = ["conv3x3_pack_kernel"]
INST = {"conv3x3": C3_INST, "conv3x3_wgrad": WG3_INST, "conv3x3_pack": PK3_INST}


def _sw(d):
    return 1 if d["sw"] == "1" else 2


def _targets(entry, d, seed):
    if entry == "conv3x3":
        return (c3_target(d["Cin"], d["Cout"], d["Wd"]),)
    if entry == "conv3x3_wgrad":
        return (wg3_target(d["Nn"], _sw(d)),)
    return tuple(PK3_INST)


def _c3_topup():
    out = []
    for nt, couts in ((1, (4, 28, 32)), (2, (36, 68, 132))):
        for p, wds in ((4, (100, 113, 129)), (2, (7, 9, 99))):
            for pf, cins in ((True, (20, 32, 36)), (False, (4, 12, 16))):
                tag = c3_target(cins[0], couts[0], wds[0])
                for i, need in enumerate((3, 6, gc.MIN_PER_TARGET)):
                    out.append(({"Cout": couts[i], "Wd": wds[i], "Cin": cins[i]}, tag, need))
    return out


gc.DIMS.update({"conv3x3": C3_DIMS, "conv3x3_wgrad": WG3_DIMS, "conv3x3_pack": PK3_DIMS})
gc.RULES.update({"conv3x3": C3_RULES, "conv3x3_wgrad": WG3_RULES, "conv3x3_pack": PK3_RULES})
gc.SEEDS.update({"conv3x3": 21, "conv3x3_wgrad": 22, "conv3x3_pack": 23})
gc.INST.update(INST)
for _e in ENTRIES:
    gc.PLANNERS[_e] = (lambda e: lambda d, seed: _targets(e, d, seed))(_e)
gc.TOPUP.update({
    "conv3x3": _c3_topup(),
    "conv3x3_wgrad": [({"Nn": n, "sw": s}, wg3_target(n, 1 if s == "1" else 2), need)
                      for s in WG3_DIMS["sw"] for n, need in ((4, 3), (16, gc.MIN_PER_TARGET), (20, 3), (68, gc.MIN_PER_TARGET))],
    "conv3x3_pack": [({}, PK3_INST[0], gc.MIN_PER_TARGET)],
})

# the pair as the dense block uses it: (name, kind, dims)
_COMPOSED = [
    ("layer-Ci20-Co16", "layer", dict(Ci=20, Co=16, B=2, H=33, Wd=9)),
    ("layer-Ci36-Co32-wide", "layer", dict(Ci=36, Co=32, B=1, H=3, Wd=101)),
    ("dx-Cin16-Cb80", "dx", dict(Cin=16, Cb=80, B=2, H=33, Wd=9)),
    ("dx-Cin32-Cb80", "dx", dict(Cin=32, Cb=80, B=1, H=34, Wd=7)),
    ("dx-Cin16-Cb160", "dx", dict(Cin=16, Cb=160, B=1, H=5, Wd=17)),
    ("dx-Cin32-Cb160-wide", "dx", dict(Cin=32, Cb=160, B=1, H=3, Wd=101)),
]


def cases(entry):
    if entry == COMPOSED:
        out = []
        for i, (name, kind, d) in enumerate(_COMPOSED):
            t = c3_target(d["Ci"], d["Co"], d["Wd"]) if kind == "layer" else c3_target(d["Cin"], d["Cb"], d["Wd"])
            out.append(Case(COMPOSED, name, dict(d, kind=kind), (t, PK3_INST[0]), 7000 + i))
        return out
    return gc.cases(entry)


def invalid_pairs(entry):
    return gc.invalid_pairs(entry)


# ------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------
def _data(g, rows, cols, kind):
    x = torch.randn(rows, cols, generator=g)
    if kind == DATA[1]:
        x[rows // 2] *= 1e3
    if kind == DATA[2]:
        x[:, cols // 2] *= 1e-3
    return x


def _ld_off(d, ld_key, off_key, Cc, name):
    ld = {name: Cc, name + "+4": Cc + 4, "80": 80, "160": 160}[d[ld_key]]
    return ld, {"0": 0, "4": 4, "end": ld - Cc}[d[off_key]]


def _columns(rows, ld, off, data, fill):
    """A guarded allocation of `rows` rows of stride ld whose columns [off, off + data.shape[1]) hold `data`."""
    t = gc.alloc(rows * ld, fill)
    t[GUARD:GUARD + rows * ld].view(rows, ld)[:, off:off + data.shape[1]] = data
    return t


def _output(b, name, rows, ld, off, Cc, key=None):
    """An output of `rows` rows: SENT everywhere, NaN in columns [off, off + Cc)."""
    b.bufs[name] = _columns(rows, ld, off, torch.full((rows, Cc), NAN), SENT)
    b.out_keys[key or name] = name
    return Buf(name, GUARD, GUARD + rows * ld)


def _forward_buffers(b, g, fill, M, Cout, ldy, y_off, bias, R):
    """Y (+ bias, R) of a forward call; returns the keyword arguments."""
    kw = dict(Y=_output(b, "Y", M, ldy, y_off, Cout), ldy=ldy, y_off=y_off)
    if bias:
        P = gc.alloc(Cout, fill)
        P[GUARD:GUARD + Cout] = draw(g, 1, Cout).reshape(-1)
        b.bufs["P"] = P
        kw["bias"] = Buf("P", GUARD, GUARD + Cout)
    if R != "off":
        rv = draw(g, M, Cout)
        if R == "alias":
            b.bufs["Y"][GUARD:GUARD + M * ldy].view(M, ldy)[:, y_off:y_off + Cout] = rv
            kw["R"] = Buf("Y", GUARD, GUARD + M * ldy)
        else:
            b.bufs["R"] = _columns(M, ldy, y_off, rv, fill)
            kw["R"] = Buf("R", GUARD, GUARD + M * ldy)
    return kw


def _c3_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    B, H, Wd, Cin, Cout = d["B"], d["H"], d["Wd"], d["Cin"], d["Cout"]
    ldx, x_off = _ld_off(d, "ldx", "x_off", Cin, "Cin")
    ldy, y_off = _ld_off(d, "ldy", "y_off", Cout, "Cout")
    M = B * H * Wd
    b = Built(case)
    b.bufs["X"] = _columns(M, ldx, x_off, _data(g, M, Cin, d["data"]), fill)
    b.bufs["Wm"] = _columns(Cout, 9 * Cin, 0, draw(g, Cout, 9 * Cin) * 0.1, fill)
    nfl = pack_geometry(Cin, Cout)[2]
    b.bufs["Wpack"] = gc.alloc(nfl, fill)
    b.packs = [dict(srcs=[(Buf("Wm"), GUARD, 9 * Cin, 1, Cin, 0, Cin)], Cin=Cin, Cout=Cout, flip=False,
                    out=Buf("Wpack", GUARD, GUARD + nfl))]
    kw = dict(X=Buf("X", GUARD, GUARD + M * ldx), ldx=ldx, x_off=x_off, W=Buf("Wpack", GUARD, GUARD + nfl), ldw=9 * Cin, B=B, H=H,
              Wd=Wd, Cin=Cin, Cout=Cout)
    kw.update(_forward_buffers(b, g, fill, M, Cout, ldy, y_off, d["bias"], d["R"]))
    b.kw, b.outs = kw, ["Y"]
    return b


def wg3_split(kind, ntiles):
    """(nsplit, tiles_per_split)."""
    if kind == "one":
        return 1, ntiles
    if kind == "exact":
        return ntiles, 1
    if kind == "ragged":
        return gc.tn_split("partial", ntiles)
    ns, tps = gc.tn_split("partial", ntiles) if ntiles >= 3 else (1, ntiles)
    return ns + 2, tps                           # "over": two trailing splits own no tile


def _wg3_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    B, H, Wd, Cin, Nn, sw = d["B"], d["H"], d["Wd"], d["Cin"], d["Nn"], _sw(d)
    Wx = Wd if sw == 1 else (2 * Wd - 1 if d["sw"] == "2-Wx-odd" else 2 * Wd)
    ldg, g_off = _ld_off(d, "ldg", "g_off", Nn, "Nn")
    ldx, x_off = _ld_off(d, "ldx", "x_off", Cin, "Cin")
    M, Mx = B * H * Wd, B * H * Wx
    b = Built(case)
    b.bufs["G"] = _columns(M, ldg, g_off, _data(g, M, Nn, d["data"]), fill)
    b.bufs["X"] = _columns(Mx, ldx, x_off, _data(g, Mx, Cin, d["data"]), fill)
    nsplit, tps = wg3_split(d["split"], wgrad_tiles(B, H, Wd))
    pad = d["strides"] == "padded"
    n, ss, bs = Nn * 9 * Cin, Nn * 9 * Cin + (12 if pad else 0), Nn + (4 if pad else 0)
    kw = dict(G=Buf("G", GUARD, GUARD + M * ldg), ldg=ldg, g_off=g_off, X=Buf("X", GUARD, GUARD + Mx * ldx), ldx=ldx, x_off=x_off,
              B=B, H=H, Wd=Wd, Cin=Cin, Nn=Nn, slab=_output(b, "slab", nsplit, ss, 0, n), nsplit=nsplit, tiles_per_split=tps, sw=sw,
              Wx=Wx, slab_stride=ss if pad else 0)
    if d["bslab"]:
        kw.update(bslab=_output(b, "bslab", nsplit, bs, 0, Nn), bslab_stride=bs if pad else 0)
    b.kw, b.outs, b.packs = kw, list(b.out_keys.values()), []
    return b


def _weights(g, *shape):
    """Zero or normal fp32 with magnitudes in [2^-20, 2^4], both signs."""
    n = int(np.prod(shape))
    mag = torch.exp2(24 * torch.rand(n, generator=g, dtype=torch.float64) - 20).float()
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return torch.where(torch.rand(n, generator=g) < 0.1, torch.zeros(()), mag * sign).reshape(shape)


def _ranges(g, Cin, nsrc, gap):
    """nsrc disjoint non-empty column ranges of [0, Cin), in shuffled order; with `gap` one column between two of them (or
    the last one) stays uncovered."""
    cuts = sorted((torch.randperm(Cin - 1, generator=g)[:nsrc + int(gap) - 1] + 1).tolist())
    edges = [0] + cuts + [Cin]
    parts = [(edges[i], edges[i + 1] - edges[i]) for i in range(len(edges) - 1)]
    if gap:
        del parts[int(torch.randint(len(parts), (1,), generator=g))]
    return [parts[int(i)] for i in torch.randperm(len(parts), generator=g)]


def _source(g, Cout, cols, layout, fill, off):
    """(guarded allocation, s_row, s_col, s_tap): the elements the gather names hold weights, the others `fill`."""
    if layout == "oihw":
        s_row, s_col, s_tap = 9 * cols, 9, 1
    elif layout == "tap-major":
        s_row, s_col, s_tap = 9 * cols, 1, cols
    else:
        s_tap, s_col = 2, 21
        s_row = s_col * cols + 5
    n, c, tap = torch.arange(Cout).view(-1, 1, 1), torch.arange(cols).view(1, -1, 1), torch.arange(9).view(1, 1, -1)
    idx = off + n * s_row + c * s_col + tap * s_tap
    t = gc.alloc(int(idx.max()) + 1, fill)
    t[GUARD + idx] = _weights(g, Cout, cols, 9)
    return t, s_row, s_col, s_tap


def _pk3_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    Cin, Cout = d["Cin"], d["Cout"]
    b = Built(case)
    srcs = []
    for k, (col_off, cols) in enumerate(_ranges(g, Cin, d["nsrc"], d["cover"] == "gap")):
        off = 8 * (k % 2) if d["layout"] == "padded" else 0
        b.bufs[f"S{k}"], s_row, s_col, s_tap = _source(g, Cout, cols, d["layout"], fill, off)
        srcs.append((Buf(f"S{k}"), GUARD + off, s_row, s_col, s_tap, col_off, cols))
    nfl = pack_geometry(Cin, Cout)[2]
    b.bufs["Wpack"] = gc.alloc(nfl + 64, SENT)
    b.bufs["Wpack"][GUARD:GUARD + nfl] = NAN
    b.packs = [dict(srcs=srcs, Cin=Cin, Cout=Cout, flip=bool(d["flip"]), out=Buf("Wpack", GUARD, GUARD + nfl + 64))]
    b.kw, b.outs, b.out_keys = {}, ["Wpack"], {"pack": "Wpack"}
    return b


def _composed_build(case, garbage):
    d, g = case.dims, gc.gen(case.seed)
    fill = GARBAGE if garbage else NAN
    B, H, Wd = d["B"], d["H"], d["Wd"]
    M = B * H * Wd
    b = Built(case)
    if d["kind"] == "layer":        # columns [0, Ci) of the wide feature map -> a buffer of the layer's own, with bias
        Ci, Co, ldx = d["Ci"], d["Co"], 80
        b.bufs["X"] = _columns(M, ldx, 0, _data(g, M, Ci, DATA[0]), fill)
        b.bufs["S0"] = _columns(Co, 9 * Ci, 0, draw(g, Co, 9 * Ci) * 0.1, fill)      # nn.Conv2d weight [co][ci][3][3]
        srcs = [(Buf("S0"), GUARD, 9 * Ci, 9, 1, 0, Ci)]
        Cin, Cout, flip, ldy, y_off = Ci, Co, False, Co, 0
        kw = _forward_buffers(b, g, fill, M, Cout, ldy, y_off, 1, "off")
        b.layers = None
    else:                           # dY of two layers side by side -> accumulated into columns [lo, lo + Cb) of the gradient map
        Cin, Cb, lo = d["Cin"], d["Cb"], 4
        Co = Cin // 2
        ldx, ldy, y_off = Cin, Cb + 8, lo
        b.bufs["X"] = _columns(M, ldx, 0, _data(g, M, Cin, DATA[0]), fill)
        srcs, b.layers = [], []
        for k in range(2):
            Ci = lo + Cb + 4 * (k + 1)                                                # the layer reads channels [0, Ci) of the map
            b.bufs[f"S{k}"] = _columns(Co, 9 * Ci, 0, draw(g, Co, 9 * Ci) * 0.1, fill)
            # pointer advanced to input channel lo, rows = the block's channels, columns = the layer's output channels
            srcs.append((Buf(f"S{k}"), GUARD + 9 * lo, 9, 9 * Ci, 1, k * Co, Co))
            b.layers.append((f"S{k}", Co, Ci, k * Co))
        Cout, flip = Cb, True
        kw = _forward_buffers(b, g, fill, M, Cout, ldy, y_off, 0, "alias")
        b.lo = lo
    nfl = pack_geometry(Cin, Cout)[2]
    b.bufs["Wpack"] = gc.alloc(nfl, fill)
    b.packs = [dict(srcs=srcs, Cin=Cin, Cout=Cout, flip=flip, out=Buf("Wpack", GUARD, GUARD + nfl))]
    kw.update(X=Buf("X", GUARD, GUARD + M * ldx), ldx=ldx, x_off=0, W=Buf("Wpack", GUARD, GUARD + nfl), ldw=9 * Cin, B=B, H=H, Wd=Wd,
              Cin=Cin, Cout=Cout)
    b.kw, b.outs = kw, ["Y"]
    return b


_BUILD = {"conv3x3": _c3_build, "conv3x3_wgrad": _wg3_build, "conv3x3_pack": _pk3_build, COMPOSED: _composed_build}


def build(case, garbage=False):
    return _BUILD[case.entry](case, garbage)


def _pack_kwargs(p, tensors):
    def t(v):
        return tensors[v.name] if v.lo < 0 else tensors[v.name][v.lo:v.hi]
    return dict(srcs=[(t(s[0]),) + tuple(s[1:]) for s in p["srcs"]], Cin=p["Cin"], Cout=p["Cout"], flip=p["flip"], out=t(p["out"]))


def reference(b, tensors=None, defect=None):
    t = tensors or b.bufs
    e = b.case.entry
    if e == "conv3x3_pack":
        return {"pack": ref_conv3x3_pack(defect=defect, **_pack_kwargs(b.packs[0], t))}
    kw = b.kwargs(t, "cpu")
    if e == "conv3x3_wgrad":
        return ref_conv3x3_wgrad(defect=defect, **kw)
    if e == COMPOSED and b.layers is not None:
        layers = [(t[n][GUARD:GUARD + Co * 9 * Ci].reshape(Co, Ci, 3, 3), col) for n, Co, Ci, col in b.layers]
        return ref_dense_dx(dY=kw["X"], ldg=kw["ldx"], layers=layers, lo=b.lo, Cb=kw["Cout"], B=kw["B"], H=kw["H"], Wd=kw["Wd"],
                            R=kw["R"], ldy=kw["ldy"], y_off=kw["y_off"])
    Cin, Cout = kw["Cin"], kw["Cout"]
    if e == COMPOSED:               # [co][ci][3][3] -> the tap-major rows of the header's formula
        Wm = t["S0"][GUARD:GUARD + Cout * 9 * Cin].reshape(Cout, Cin, 9).transpose(1, 2).reshape(Cout, 9 * Cin)
    else:
        Wm = t["Wm"][GUARD:GUARD + Cout * 9 * Cin]
    return ref_conv3x3(defect=defect, **dict(kw, W=Wm))


def run(mod, b, tensors, device="cpu"):
    """The case's calls on the namespace `mod` (wesep_amd.dev, or tests.emu_dev): the weight pack, then the entry."""
    for p in b.packs:
        mod.conv3x3_pack_srcs(**_pack_kwargs(p, tensors))
    if b.case.entry != "conv3x3_pack":
        getattr(mod, "conv3x3" if b.case.entry == COMPOSED else b.case.entry)(**b.kwargs(tensors, device))


# ------------------------------------------------------------------------------------------------------------
# checker
# ------------------------------------------------------------------------------------------------------------
def _same(a, b, what):
    a, b = a.contiguous().view(torch.int32).reshape(-1), b.contiguous().view(torch.int32).reshape(-1)
    if not torch.equal(a, b):
        j = int((a != b).nonzero()[0])
        raise ContractViolation("sentinel", f"{what}: word {j} changed ({int(b[j]):#x} -> {int(a[j]):#x})")


def check_pack(out, before, bits, what):
    """The whole pack as bits; everything around it bit-identical to what it held."""
    n = bits.numel() // 2
    got = out[GUARD:GUARD + n].contiguous().view(torch.int16)
    if not torch.equal(got, bits):
        j = int((got != bits).nonzero()[0])
        raise ContractViolation("exact", f"{what}: bf16 element {j} (unit {j // 8}, j {j % 8}) is {int(got[j]) & 0xFFFF:#06x}, "
                                         f"the unit formula says {int(bits[j]) & 0xFFFF:#06x}")
    _same(out[:GUARD], before[:GUARD], what + " front guard")
    _same(out[GUARD + n:], before[GUARD + n:], what + " behind the pack")
    return 0.0


def verify(b, ref, after, what=None):
    """Every output allocation of a built case (`after`: name -> CPU tensor after the launch) against `ref`.  Returns the
    worst err / bound.  Raises ContractViolation: nan | exact | bound | sentinel."""
    what = what or b.case.name
    if b.case.entry == "conv3x3_pack":
        return check_pack(after["Wpack"], b.bufs["Wpack"], ref["pack"], what)
    return max(check(after[name], b.bufs[name], ref[key], f"{what} {key}", GUARD) for key, name in b.out_keys.items())


def output_bits(b, after):
    return torch.cat([after[n].contiguous().view(torch.int32).reshape(-1) for n in b.outs])


def perfect(b, ref):
    """The buffers a correctly rounding kernel leaves for `ref` (the host test plants its defects into copies of these)."""
    after = {k: v.clone() for k, v in b.bufs.items()}
    if b.case.entry == "conv3x3_pack":
        bits = ref["pack"]
        after["Wpack"][GUARD:GUARD + bits.numel() // 2] = bits.view(torch.float32)
        return after
    for key, name in b.out_keys.items():
        after[name][ref[key].idx + GUARD] = ref[key].val.float()
    return after


def emulate(b, tensors=None):
    """The case on tests/emu_dev.py (which keeps the plain weight rows instead of the pack)."""
    from tests import emu_dev
    t = {k: v.clone() for k, v in (tensors or b.bufs).items()}
    run(emu_dev, b, t)
    return t
