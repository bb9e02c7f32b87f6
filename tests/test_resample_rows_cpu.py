"""CPU: the rows forms of the resampler without a GPU -- the new symbols and descriptors in the header, the binding and the built
library (neither ABI number moves), the emulation of the rows kernel (tests/emu_resample_rows.py) against the fp64 restatement
and against the solo emulation on one table of seven rows, every refusal of the two entry points by name and with the row
index (tables made by wesep_amd.dev, the calls refused before any launch), and the per-row bookkeeping of
wesep_amd.resample.StreamResamplerRows (step_plan) against the solo emulation's."""
import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from tests import emu_resample as EMU
from tests import emu_resample_rows as ROWS
from tests import resample_contract as RC
from wesep_amd import _lib as L
from wesep_amd import dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ws_resample_stream_rows_fwd", "ws_rows_copy_fwd")
err = lambda: L.lib().ws_last_error().decode()


def test_rows_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    lib = L.lib()
    for name in NAMES:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        assert name in L.EXPORTED_SYMBOLS and getattr(lib, name) is not None
    assert lib.ws_abi_version() == 20 == L.ABI_VERSION
    from wesep_amd import engine as E
    from wesep_amd import resample as RS
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2
    assert callable(RS.StreamResamplerRows) and callable(dev.resample_stream_rows_fwd) and callable(dev.rows_copy_fwd)


def test_descriptor_dtypes_match_the_c_layout():
    fields = lambda dt: ", ".join(f"offsetof({{0}}, {n})" for n in dt.names)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "wesep_hip.h"\nint main(void) {\n'
            '  size_t v[] = {sizeof(ws_resample_row), ' + fields(L.RESAMPLE_ROW).format("ws_resample_row") +
            ', sizeof(ws_rows_copy_row), ' + fields(L.ROWS_COPY_ROW).format("ws_rows_copy_row") + '};\n'
            '  for (size_t i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%zu ", v[i]);\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write(prog)
        subprocess.run(["cc", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = []
    for dt in (L.RESAMPLE_ROW, L.ROWS_COPY_ROW):
        want += [dt.itemsize] + [dt.fields[n][1] for n in dt.names]
    assert got == want and L.RESAMPLE_ROW.itemsize == 72 and L.ROWS_COPY_ROW.itemsize == 24
    assert tuple(L.RESAMPLE_ROW.names) == ROWS.FIELDS


def test_table_is_one_array_for_host_and_device():
    rows, _, _ = ROWS.seven_rows()
    tab = dev.resample_rows_table(rows)
    assert tab.dtype == L.RESAMPLE_ROW and len(tab) == 7 and dev.resample_rows_table(tab) is tab
    for i, r in enumerate(rows):
        assert all(int(tab[i][k]) == r[k] for k in ROWS.FIELDS)
    # the device copy is made from the same array's bytes
    assert bytes(L.upload_struct_array(tab, "cpu").numpy()) == tab.tobytes()
    with pytest.raises(L.WesepHipError, match="row 0 has unknown fields"):
        dev.resample_rows_table([dict(n_valdi=3)])


# ---- the emulation of the rows kernel on the seven rows ------------------------------------------------------------------
@pytest.fixture(scope="module")
def seven():
    rows, arenas, meta = ROWS.seven_rows()
    buf = torch.from_numpy(arenas["buf"].astype(np.float64))
    taps = torch.from_numpy(arenas["taps"].astype(np.float64))
    y = torch.full((arenas["n_y"],), 12345.0, dtype=torch.float64)
    hist = torch.full((arenas["n_hist"],), 12345.0, dtype=torch.float64)
    ROWS.rows_fwd(rows, buf, taps, y, hist)
    return rows, arenas, meta, y, hist


def test_seven_rows_cover_what_they_should():
    rows, arenas, _ = ROWS.seven_rows()
    lds = [r["U"] * r["K"] <= ROWS.LDS_TAPS for r in rows]
    assert any(lds) and not all(lds)                                    # staged and global tables in one launch
    assert any(r["lead"] == (r["K"] - r["D"]) // 2 > 0 and not r["final"] for r in rows)      # a stream's start
    assert any(r["lead"] == 0 and r["K"] > 1 and r["g_first"] > 0 for r in rows)              # mid-stream
    assert any(r["final"] and r["hist_len"] == 0 for r in rows)
    assert any(r["n_out"] == 0 and r["hist_len"] > 0 for r in rows)
    assert any(r["K"] == 1 for r in rows)                               # the container's rate
    assert max(r["n_out"] for r in rows) > 256 and any(r["n_out"] == 3 for r in rows)
    assert ROWS.grid(rows) == (4, 7, 8192)                              # row 0: three workgroups of outputs, one of history
    assert np.isnan(arenas["buf"]).sum() == ROWS.GAP * 8


def test_emulated_rows_against_the_restatement(seven):
    rows, arenas, meta, y, _ = seven
    for i, (r, (pair, z, q0)) in enumerate(zip(rows, meta)):
        got = y[r["out_off"]:r["out_off"] + r["n_out"]].numpy()
        if pair is None:
            assert np.array_equal(got, z.astype(np.float64)), i          # the identity table: the samples themselves
            continue
        ref = RC.reference(z, *pair)[q0:q0 + r["n_out"]]
        bnd = RC.bound(z, *pair)[q0:q0 + r["n_out"]]
        assert ref.shape == got.shape and np.all(np.abs(got - ref) <= bnd), (i, float(np.abs(got - ref).max()))


def test_emulated_rows_equal_the_solo_emulation(seven):
    rows, arenas, meta, y, hist = seven
    buf64, taps64 = arenas["buf"].astype(np.float64), arenas["taps"].astype(np.float64)
    claimed_y, claimed_h = np.zeros(arenas["n_y"], bool), np.zeros(arenas["n_hist"], bool)
    for i, r in enumerate(rows):
        U, D, K = r["U"], r["D"], r["K"]
        geom = (U, D, (K - D) // 2, K)
        b = buf64[r["in_off"]:r["in_off"] + r["n_valid"]]
        EMU.check_call(geom, r["lead"], r["n_valid"], r["final"], r["g_first"], r["n_out"], r["hist_from"], r["hist_len"])
        solo = EMU.kernel_values(geom, taps64[r["taps_off"]:r["taps_off"] + U * K].reshape(U, K), b, r["lead"], r["n_valid"], r["final"],
                                 r["g_first"], r["n_out"])
        assert torch.equal(y[r["out_off"]:r["out_off"] + r["n_out"]], torch.from_numpy(solo)), i
        assert torch.equal(hist[r["hist_off"]:r["hist_off"] + r["hist_len"]],
                           torch.from_numpy(b[r["hist_from"]:r["hist_from"] + r["hist_len"]])), i
        claimed_y[r["out_off"]:r["out_off"] + r["n_out"]] = True
        claimed_h[r["hist_off"]:r["hist_off"] + r["hist_len"]] = True
    assert torch.all(y[torch.from_numpy(~claimed_y)] == 12345.0) and torch.all(hist[torch.from_numpy(~claimed_h)] == 12345.0)
    assert torch.all(torch.isfinite(y[torch.from_numpy(claimed_y)]))


def test_emulated_rows_copy_gathers_and_scatters():
    src = torch.arange(100, dtype=torch.float64)
    rect = torch.full((3 * 20,), -1.0, dtype=torch.float64)
    gather = [dict(src_off=5, dst_off=0, len=20, fill=0), dict(src_off=40, dst_off=20, len=7, fill=13), dict(src_off=0, dst_off=40, len=0, fill=20)]
    ROWS.rows_copy(gather, src, rect)
    assert torch.equal(rect[:20], src[5:25]) and torch.equal(rect[20:27], src[40:47]) and torch.all(rect[27:] == 0)
    with pytest.raises(EMU.Refused, match="row 1: its dst range overlaps the dst range of row 0"):
        ROWS.rows_copy([dict(src_off=0, dst_off=0, len=10, fill=0), dict(src_off=50, dst_off=9, len=5, fill=0)], src, rect)


# ---- the entry points' refusals: before any launch, by name, with the row index -------------------------------------------
N_BUF, N_TAPS, N_Y, N_HIST = 1000, 200, 600, 100
OK0 = dict(in_off=0, taps_off=0, out_off=0, hist_off=0, U=2, D=1, K=15, lead=7, n_valid=100, final=0, g_first=0, n_out=172, hist_from=86,
           hist_len=14)
OK1 = dict(in_off=100, taps_off=30, out_off=200, hist_off=50, U=1, D=3, K=41, lead=0, n_valid=400, final=0, g_first=0, n_out=120,
           hist_from=360, hist_len=40)


def _rows_call(rows, which=None, n=(N_BUF, N_TAPS, N_Y, N_HIST), null=()):
    """the entry point on host memory that no launch will ever see: every call here is refused"""
    tab = dev.resample_rows_table(rows)
    mem = [(ctypes.c_float * 1024)() for _ in range(4)]
    ptr = [None if nm in null else ctypes.cast(m, ctypes.c_void_p) for nm, m in zip(("buf", "taps", "y", "hist"), mem)]
    host = None if "rows" in null else ctypes.c_void_p(tab.ctypes.data)
    devp = None if "d_rows" in null else ctypes.c_void_p(tab.ctypes.data)
    rc = L.lib().ws_resample_stream_rows_fwd(host, devp, len(tab), ptr[0], n[0], ptr[1], n[1], ptr[2], n[2], ptr[3], n[3], None)
    return rc, err()


def _bad(**kw):
    """row 1 of a table of two with some fields changed"""
    return [OK0, dict(OK1, **kw)]


ROW_REFUSALS = {
    "U above the limit": (_bad(U=1025), "row 1: U=1025, D=3; U and D lie in [1, 1024]"),
    "D below 1": (_bad(D=0), "row 1: U=1, D=0; U and D lie in [1, 1024]"),
    "K above the limit": (_bad(K=4097), "row 1: K=4097 taps per output sample; K lies in [1, 4096]"),
    "K below D": (_bad(K=1, D=3), "row 1: K=1 is below D=3"),
    "K - D odd": (_bad(K=42), "row 1: K - D = 39 is odd"),
    "bad sizes": (_bad(n_valid=0), "row 1: bad sizes (n_valid=0 >= 1"),
    "nothing to do": (_bad(n_out=0, hist_len=0), "row 1: bad sizes"),
    "lead above w": (_bad(lead=20), "row 1: lead=20 outside [0, w=19]"),
    "g_first negative": (_bad(g_first=-1), "row 1: lead=0 outside [0, w=19] or g_first=-1 negative"),
    "buf leaves its arena": (_bad(in_off=601), "row 1: buf [601, 601 + 400) leaves the arena of 1000 floats"),
    "buf offset negative": (_bad(in_off=-1), "row 1: buf [-1, -1 + 400) leaves the arena"),
    "taps leave their arena": (_bad(taps_off=160), "row 1: taps [160, 160 + 1 * 41) leaves the arena of 200 floats"),
    "y leaves its arena": (_bad(out_off=481), "row 1: y [481, 481 + 120) leaves the arena of 600 floats"),
    "hist leaves its arena": (_bad(hist_off=61), "row 1: hist [61, 61 + 40) leaves the arena of 100 floats"),
    "history outside the valid samples": (_bad(hist_from=361), "row 1: history [361, 361 + 40) leaves the 400 valid samples"),
    "a non-final row short of samples": (_bad(n_out=121), "row 1: outputs up to 121 need 401 valid samples, 400 are given and the end is not final"),
    "a final row past the end": (_bad(final=1, n_out=128), "row 1: outputs up to 128 asked, the 400 valid samples end the signal at output 127"),
    "offsets reaching 2^31": (_bad(g_first=2 ** 31 - 200, n_out=0), "row 1: offsets reach 2^31"),
    "overlapping outputs": (_bad(out_off=171), "row 1: its y range overlaps the y range of row 0"),
    "overlapping histories": (_bad(hist_off=13), "row 1: its hist range overlaps the hist range of row 0"),
}


@pytest.mark.parametrize("name", list(ROW_REFUSALS))
def test_rows_entry_point_refuses(name):
    rows, msg = ROW_REFUSALS[name]
    rc, text = _rows_call(rows)
    assert rc == -1 and text.startswith("ws_resample_stream_rows_fwd: ") and msg in text, text
    # the emulation refuses the same table, naming the same row
    a = lambda n: torch.zeros(n, dtype=torch.float64)
    with pytest.raises(EMU.Refused, match="row 1"):
        ROWS.check_table(rows, a(N_BUF), a(N_TAPS), a(N_Y), a(N_HIST))


def test_rows_entry_point_refuses_the_first_row_by_its_index_and_the_call_itself():
    rc, text = _rows_call([dict(OK0, K=14), OK1])
    assert rc == -1 and "row 0: K - D = 13 is odd" in text
    for null in ("rows", "d_rows", "buf", "taps"):
        rc, text = _rows_call([OK0, OK1], null=(null,))
        assert rc == -1 and "ws_resample_stream_rows_fwd: rows, d_rows, buf or taps is NULL" in text
    rc, text = _rows_call([OK0, OK1], null=("y",))
    assert rc == -1 and "row 0: y is NULL with n_out=172" in text
    rc, text = _rows_call([OK0, OK1], null=("hist",))
    assert rc == -1 and "row 0: hist is NULL with hist_len=14" in text
    rc, text = _rows_call([])
    assert rc == -1 and "A=0 is outside [1, 65535]" in text
    rc, text = _rows_call([OK0, OK1], n=(N_BUF, -1, N_Y, N_HIST))
    assert rc == -1 and "an arena length is negative" in text


def test_rows_entry_point_compares_ranges_by_address():
    """buf and hist as parts of ONE allocation (a stream's two history buffers): a history that lands on a buffer some row
    of the launch reads is refused, whatever the arenas are called"""
    tab = dev.resample_rows_table([dict(OK0, hist_off=0), dict(OK1, hist_off=200)])       # relative to hist = buf + 500
    mem = (ctypes.c_float * 4096)()
    base = ctypes.cast(mem, ctypes.c_void_p).value
    p = lambda off: ctypes.c_void_p(base + 4 * off)
    call = lambda hist_at: L.lib().ws_resample_stream_rows_fwd(ctypes.c_void_p(tab.ctypes.data), ctypes.c_void_p(tab.ctypes.data), 2, p(0), 1000,
                                                               p(2000), 200, p(3000), 600, p(hist_at), 300, None)
    assert call(480) == -1 and "row 0: its hist range overlaps the buf range of row 1" in err()
    assert call(90) == -1 and "its hist range overlaps the buf range of row 0" in err()


COPY_OK = [dict(src_off=0, dst_off=0, len=10, fill=2), dict(src_off=20, dst_off=12, len=5, fill=0)]
COPY_REFUSALS = {
    "negative length": ([COPY_OK[0], dict(COPY_OK[1], len=-1)], "row 1: bad sizes (len=-1"),
    "nothing to do": ([COPY_OK[0], dict(COPY_OK[1], len=0)], "row 1: bad sizes (len=0 >= 0, fill=0"),
    "src leaves its arena": ([COPY_OK[0], dict(COPY_OK[1], src_off=96)], "row 1: src [96, 96 + 5) leaves the arena of 100 floats"),
    "dst leaves its arena": ([COPY_OK[0], dict(COPY_OK[1], dst_off=46, fill=1)], "row 1: dst [46, 46 + 5 + 1) leaves the arena of 50 floats"),
    "overlapping destinations": ([COPY_OK[0], dict(COPY_OK[1], dst_off=11)], "row 1: its dst range overlaps the dst range of row 0"),
}


@pytest.mark.parametrize("name", list(COPY_REFUSALS))
def test_rows_copy_entry_point_refuses(name):
    rows, msg = COPY_REFUSALS[name]
    tab = dev.rows_copy_table(rows)
    a, b = (ctypes.c_float * 128)(), (ctypes.c_float * 128)()
    t = ctypes.c_void_p(tab.ctypes.data)
    rc = L.lib().ws_rows_copy_fwd(t, t, len(tab), ctypes.cast(a, ctypes.c_void_p), 100, ctypes.cast(b, ctypes.c_void_p), 50, None)
    assert rc == -1 and err().startswith("ws_rows_copy_fwd: ") and msg in err(), err()
    with pytest.raises(EMU.Refused, match="row 1"):
        ROWS.rows_copy(rows, torch.zeros(100, dtype=torch.float64), torch.zeros(50, dtype=torch.float64))


def test_rows_copy_entry_point_refuses_a_copy_onto_its_source_and_null():
    tab = dev.rows_copy_table([dict(src_off=0, dst_off=5, len=10, fill=0)])
    a = (ctypes.c_float * 128)()
    t, p = ctypes.c_void_p(tab.ctypes.data), ctypes.cast(a, ctypes.c_void_p)
    assert L.lib().ws_rows_copy_fwd(t, t, 1, p, 100, p, 100, None) == -1 and "row 0: its dst range overlaps the src range of row 0" in err()
    assert L.lib().ws_rows_copy_fwd(t, None, 1, p, 100, p, 100, None) == -1 and "rows, d_rows, src or dst is NULL" in err()
    assert L.lib().ws_rows_copy_fwd(t, t, 0, p, 100, p, 100, None) == -1 and "A=0 is outside [1, 65535]" in err()


# ---- the bookkeeping of StreamResamplerRows ------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [(8000, 16000), (48000, 16000), (44100, 16000), (16000, 44100)])
def test_step_plan_is_the_solo_streams_bookkeeping(pair):
    """step_plan, driven as StreamResamplerRows drives it, on the rows emulation: per push the solo emulation's outputs and
    history, exactly, for packets of 1 .. 2 K samples, then the flush"""
    from wesep_amd.resample import step_plan
    geom = RC.GEOM[pair]
    U, D, w, K = geom
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, size=6 * K).astype(np.float32).astype(np.float64)
    max_push = 2 * K
    solo = EMU.EmuStream(*pair, max_push=max_push)
    ld = K - 1 + max_push
    buf = torch.zeros(2 * ld, dtype=torch.float64)
    taps = torch.from_numpy(RC.taps32(*pair).astype(np.float64).reshape(-1))
    cur = h = n_in = groups = seen = 0
    while seen <= len(x):
        n = int(min(len(x) - seen, rng.integers(1, max_push + 1)))
        final = n == 0
        buf[cur * ld + h:cur * ld + h + n] = torch.from_numpy(x[seen:seen + n])
        lead, n_valid, n_out, hist_from, hist_len, g_new = step_plan(geom, n_in, groups, h, n, final)
        y = torch.zeros(n_out, dtype=torch.float64)
        if n_out or hist_len:
            ROWS.rows_fwd([ROWS.row(in_off=cur * ld, hist_off=(1 - cur) * ld, U=U, D=D, K=K, lead=lead, n_valid=n_valid, final=int(final),
                                    n_out=n_out, hist_from=hist_from, hist_len=hist_len)], buf, taps, y, buf)
        want = solo.flush() if final else solo.push(x[seen:seen + n])
        assert np.array_equal(y.numpy(), want), (pair, seen, n)
        if final:
            break
        cur, h, groups, n_in, seen = 1 - cur, hist_len, g_new, n_in + n, seen + n
        assert (cur, h, groups, n_in) == (solo.cur, solo.h, solo.groups, solo.n_in)
        assert np.array_equal(buf[cur * ld:cur * ld + h].numpy(), solo.history())
