"""Host-side emulation of the rows forms (include/wesep_hip.h: ws_resample_stream_rows_fwd, ws_rows_copy_fwd) on torch
arenas: the descriptor table, the refusals with the row index, and the per-row body -- which is, as in the kernel, the ONE
function the solo emulation runs (tests/emu_resample.py kernel_values), here on a row's slice of the arenas.  Plus the table
of seven rows that the CPU and the GPU tests share.

Arenas are 1-D torch tensors (float64 for the emulation: the float-rounded taps and samples, products exact).  buf and hist
may be the same tensor (a stream's two history buffers inside one allocation); ranges are compared by address."""
import numpy as np
import torch

from tests import emu_resample as EMU
from tests import resample_contract as RC

MAX_UD, MAX_K, LDS_TAPS = 1024, 4096, 2048
FIELDS = ("in_off", "taps_off", "out_off", "hist_off", "U", "D", "K", "lead", "n_valid", "final", "g_first", "n_out", "hist_from",
          "hist_len")
IDENTITY = (1, 1, 0, 1)          # U, D, w, K of the container's own rate: the one tap 1.0


def row(**kw):
    r = dict.fromkeys(FIELDS, 0)
    assert set(kw) <= set(FIELDS), set(kw) - set(FIELDS)
    r.update(kw)
    return r


def _addr(t, off):
    return t.data_ptr() + off * t.element_size()


def _disjoint(spans):
    """a written range meets no other range of the call; (lo, hi, row, write, name), as the entry point's sweep"""
    far = {False: None, True: None}
    for x in sorted(spans, key=lambda s: s[0]):
        hit = far[True] if far[True] and x[0] < far[True][1] else (far[False] if x[3] and far[False] and x[0] < far[False][1] else None)
        EMU._require(hit is None, f"row {x[2]}: its {x[4]} range overlaps the {hit[4] if hit else ''} range of row {hit[2] if hit else ''}")
        if far[x[3]] is None or x[1] > far[x[3]][1]:
            far[x[3]] = x


def check_table(rows, buf, taps, y, hist):
    """the refusals of ws_resample_stream_rows_fwd, each with the row index"""
    EMU._require(1 <= len(rows) <= 65535, "A outside [1, 65535]")
    n = lambda t: 0 if t is None else t.numel()
    spans = []
    for i, r in enumerate(rows):
        U, D, K = r["U"], r["D"], r["K"]
        EMU._require(1 <= U <= MAX_UD and 1 <= D <= MAX_UD, f"row {i}: U and D lie in [1, {MAX_UD}]")
        EMU._require(1 <= K <= MAX_K, f"row {i}: K lies in [1, {MAX_K}]")
        EMU._require(K >= D, f"row {i}: K is below D")
        EMU._require((K - D) % 2 == 0, f"row {i}: K - D is odd")
        try:
            EMU.check_call((U, D, (K - D) // 2, K), r["lead"], r["n_valid"], r["final"], r["g_first"], r["n_out"], r["hist_from"], r["hist_len"])
        except EMU.Refused as e:
            raise EMU.Refused(f"row {i}: {e}") from None
        q_end = r["g_first"] * U + r["n_out"]
        EMU._require(q_end + U + 256 < 2 ** 31 and (q_end // U + 2) * D + K < 2 ** 31 and r["n_valid"] + K + 256 < 2 ** 31,
                     f"row {i}: offsets reach 2^31")
        EMU._require(0 <= r["in_off"] <= n(buf) - r["n_valid"], f"row {i}: buf leaves the arena")
        EMU._require(0 <= r["taps_off"] <= n(taps) - U * K, f"row {i}: taps leaves the arena")
        EMU._require(r["n_out"] == 0 or 0 <= r["out_off"] <= n(y) - r["n_out"], f"row {i}: y leaves the arena")
        EMU._require(r["hist_len"] == 0 or 0 <= r["hist_off"] <= n(hist) - r["hist_len"], f"row {i}: hist leaves the arena")
        spans.append((_addr(buf, r["in_off"]), _addr(buf, r["in_off"] + r["n_valid"]), i, False, "buf"))
        spans.append((_addr(taps, r["taps_off"]), _addr(taps, r["taps_off"] + U * K), i, False, "taps"))
        if r["n_out"]:
            spans.append((_addr(y, r["out_off"]), _addr(y, r["out_off"] + r["n_out"]), i, True, "y"))
        if r["hist_len"]:
            spans.append((_addr(hist, r["hist_off"]), _addr(hist, r["hist_off"] + r["hist_len"]), i, True, "hist"))
    _disjoint(spans)


def grid(rows):
    """(workgroups along x, A, bytes of dynamic LDS): what the host table sizes"""
    nb = max(-(-r["n_out"] // 256) - (-r["hist_len"] // 256) for r in rows)
    return nb, len(rows), 4 * LDS_TAPS if any(r["U"] * r["K"] <= LDS_TAPS for r in rows) else 0


def rows_fwd(rows, buf, taps, y, hist):
    """The launch: every row's outputs to y and its history to hist.  All reads happen before any write, as in a launch whose
    written ranges meet no other range."""
    check_table(rows, buf, taps, y, hist)
    outs = []
    for r in rows:
        U, D, K = r["U"], r["D"], r["K"]
        b = buf[r["in_off"]:r["in_off"] + r["n_valid"]].numpy()
        t = taps[r["taps_off"]:r["taps_off"] + U * K].numpy().reshape(U, K)
        val = EMU.kernel_values((U, D, (K - D) // 2, K), t, b, r["lead"], r["n_valid"], r["final"], r["g_first"], r["n_out"])
        outs.append((torch.from_numpy(val), buf[r["in_off"] + r["hist_from"]:r["in_off"] + r["hist_from"] + r["hist_len"]].clone()))
    for r, (val, h) in zip(rows, outs):
        y[r["out_off"]:r["out_off"] + r["n_out"]] = val
        hist[r["hist_off"]:r["hist_off"] + r["hist_len"]] = h


def rows_copy(rows, src, dst):
    """ws_rows_copy_fwd: per row len floats from src_off to dst_off, then `fill` zeros"""
    EMU._require(1 <= len(rows) <= 65535, "A outside [1, 65535]")
    spans = []
    for i, r in enumerate(rows):
        ln, fill = r["len"], r["fill"]
        EMU._require(ln >= 0 and fill >= 0 and ln + fill > 0, f"row {i}: bad sizes")
        EMU._require(ln == 0 or 0 <= r["src_off"] <= src.numel() - ln, f"row {i}: src leaves the arena")
        EMU._require(0 <= r["dst_off"] <= dst.numel() - ln - fill, f"row {i}: dst leaves the arena")
        if ln:
            spans.append((_addr(src, r["src_off"]), _addr(src, r["src_off"] + ln), i, False, "src"))
        spans.append((_addr(dst, r["dst_off"]), _addr(dst, r["dst_off"] + ln + fill), i, True, "dst"))
    _disjoint(spans)
    got = [src[r["src_off"]:r["src_off"] + r["len"]].clone() for r in rows]
    for r, g in zip(rows, got):
        dst[r["dst_off"]:r["dst_off"] + r["len"]] = g
        dst[r["dst_off"] + r["len"]:r["dst_off"] + r["len"] + r["fill"]] = 0


# ---- the table of seven rows ---------------------------------------------------------------------------------------------
# pair, lead ("w": the stream's start), n_valid, final, g_first, n_out, (hist_from, hist_len); what the row is there for
SEVEN_SPEC = [
    ((8000, 16000), "w", 300, 0, 0, 586, (286, 14)),       # LDS table, stream start, 586 outputs: three workgroups
    ((48000, 16000), 0, 400, 0, 5, 115, (360, 40)),        # LDS table, mid-stream (lead 0), a first group above 0
    ((44100, 16000), "w", 900, 0, 0, 320, (865, 35)),      # global table, stream start
    ((16000, 44100), 0, 200, 1, 0, 532, (0, 0)),           # global table, final: taps behind the end skipped, no history
    ((16000, 16000), 0, 3, 0, 0, 3, (0, 0)),               # the container's rate: identity table; 3 outputs beside 586
    ((8000, 16000), "w", 5, 0, 0, 0, (0, 5)),              # fewer than w samples so far: no output, the history moves
    ((48000, 16000), "w", 50, 1, 0, 17, (0, 0)),           # a whole short signal: start and end in one row
]
GAP = 3          # floats between the ranges of consecutive rows in every arena (sentinels in the GPU test)


def seven_rows(seed=11):
    """-> (rows, arenas, meta): rows as dicts; arenas: numpy float32 buf and taps and the lengths n_y, n_hist; meta per row:
    (pair, z, q0) -- the row's outputs are samples [q0, q0 + n_out) of the whole-signal result of z (resample_contract), or
    z itself for the identity row (pair None)."""
    rng = np.random.default_rng(seed)
    rows, meta, bufs, tables, taps_off = [], [], [], [], {}
    n_buf = n_y = n_hist = GAP
    for pair, lead, n_valid, final, g_first, n_out, (hist_from, hist_len) in SEVEN_SPEC:
        ident = pair[0] == pair[1]
        U, D, w, K = IDENTITY if ident else RC.GEOM[pair]
        key = "identity" if ident else pair
        if key not in taps_off:
            taps_off[key] = sum(t.size for t in tables)
            tables.append(np.ones(1, dtype=np.float32) if ident else RC.taps32(*pair).reshape(-1))
        lead = w if lead == "w" else lead
        x = rng.uniform(-1.0, 1.0, size=n_valid).astype(np.float32)
        rows.append(row(in_off=n_buf, taps_off=taps_off[key], out_off=n_y, hist_off=n_hist, U=U, D=D, K=K, lead=lead, n_valid=n_valid,
                        final=final, g_first=g_first, n_out=n_out, hist_from=hist_from, hist_len=hist_len))
        bufs.append((n_buf, x))
        n_buf, n_y, n_hist = n_buf + n_valid + GAP, n_y + n_out + GAP, n_hist + hist_len + GAP
        if ident:
            meta.append((None, x, g_first))
        else:
            # buf[0] is sample P of a signal z whose groups line up with the buffer's: P + w - lead a multiple of D
            P = 0 if lead == w else (-(w - lead)) % D
            z = np.concatenate([rng.uniform(-1.0, 1.0, size=P).astype(np.float32), x])
            meta.append((pair, z, (g_first + (P + w - lead) // D) * U))
    buf = np.full(n_buf, np.nan, dtype=np.float32)          # NaN between the rows: nothing outside a row's range is read
    for off, x in bufs:
        buf[off:off + len(x)] = x
    return rows, dict(buf=buf, taps=np.concatenate(tables), n_y=n_y, n_hist=n_hist), meta
