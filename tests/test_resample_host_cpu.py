"""CPU: the resampler without a GPU -- the new symbols in the header, the binding and the built library (neither ABI number
moves), ws_resample_geom / ws_resample_taps against the restatement (tests/resample_contract.py), the formula's own
properties (phase sums, a 1 kHz sine), every refusal by name, and the streaming bookkeeping (tests/emu_resample.py): emitted
counts follow the rule and the concatenation is the whole-signal result, for every split of N in 0..3K into two pushes.

For (44100, 16000), K = 475, that is a million splits; both emulations run every one of them for all three pairs: the index
emulation (EmuStream(values=False): counts, the range of outputs of every call, and that every call reads exactly what the
whole-signal form reads for those outputs) and the arithmetic one (values=True: the concatenation equals the whole-signal
result exactly).  The arithmetic kernel keeps the groups it has evaluated (a group's outputs are a function of the samples
under its taps and of the taps skipped at either end) and reuses one only after comparing the samples themselves."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import emu_resample as EMU
from tests import resample_contract as RC
from wesep_amd import _lib as L
from wesep_amd import dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ws_resample_geom", "ws_resample_taps", "ws_resample_fwd", "ws_resample_stream_fwd")
STREAM_PAIRS = [(8000, 16000), (48000, 16000), (44100, 16000)]
err = lambda: L.lib().ws_last_error().decode()


def test_resample_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "wesep_hip.h")).read()
    lib = L.lib()
    for name in NAMES:
        m = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M)
        assert m, f"{name} is not declared in wesep_hip.h"
        res, args = L._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(m.group(1).split(",")), name
        assert getattr(lib, name) is not None
    assert lib.ws_abi_version() == 20 == L.ABI_VERSION
    from wesep_amd import engine as E
    from wesep_amd import resample as RS
    assert E.lib().ws_engine_abi_version() == E.ENGINE_ABI_VERSION == 2
    assert callable(RS.resample) and callable(RS.StreamResampler) and callable(dev.resample_fwd) and callable(dev.resample_stream_fwd)


@pytest.mark.parametrize("pair", RC.PAIRS)
def test_geom_and_taps_equal_the_restatement(pair):
    assert RC.geometry(*pair) == RC.GEOM[pair]
    assert dev.resample_geom(*pair) == RC.GEOM[pair]
    taps = dev.resample_taps(*pair)
    assert taps.dtype == np.float32 and taps.shape == RC.GEOM[pair][::3]
    assert np.array_equal(taps, RC.taps32(*pair))


@pytest.mark.parametrize("pair", RC.PAIRS)
def test_formula_phase_sums_and_sine(pair):
    sums = RC.taps64(*pair).sum(axis=1)
    print(f"{pair}: phase sums in [{sums.min():.6f}, {sums.max():.6f}]")
    assert np.all(np.abs(sums - 1.0) <= 1e-3)
    e = RC.sine_error(*pair, RC.reference(RC.sine(pair[0]), *pair, taps=RC.taps64(*pair)))
    print(f"{pair}: 1 kHz sine, max error over the middle three quarters {e:.2e}")
    assert e <= 2e-3


def test_refusals_are_by_name():
    lib = L.lib()
    v = [ctypes.c_int(0) for _ in range(4)]
    r = [ctypes.byref(x) for x in v]
    buf, buf2 = (ctypes.c_float * 4096)(), (ctypes.c_float * 4096)()
    p, p2 = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(buf2, ctypes.c_void_p)
    assert lib.ws_resample_geom(0, 16000, *r) == -1 and "ws_resample_geom: rate_in=0 and rate_out=16000 must be positive" in err()
    assert lib.ws_resample_geom(16000, -1, *r) == -1 and "must be positive" in err()
    assert lib.ws_resample_geom(16000, 16001, *r) == -1 and "U=16001, D=16000; U and D may not exceed 1024" in err()
    assert lib.ws_resample_geom(1025, 1, *r) == -1 and "ws_resample_geom: 1025 -> 1 reduces to U=1, D=1025" in err()
    assert lib.ws_resample_geom(1000, 1, *r) == -1 and "K=13122 taps per output sample; K may not exceed 4096" in err()
    assert lib.ws_resample_geom(8000, 16000, None, r[1], r[2], r[3]) == -1 and "ws_resample_geom: U, D, w or K is NULL" in err()
    assert lib.ws_resample_geom(1024, 1023, *r) == 0 and v[0].value == 1023 and v[1].value == 1024
    assert lib.ws_resample_taps(8000, 16000, None) == -1 and "ws_resample_taps: taps is NULL" in err()
    assert lib.ws_resample_taps(0, 16000, p) == -1 and "ws_resample_taps: rate_in=0" in err()
    assert lib.ws_resample_taps(44100, 16001, p) == -1 and "ws_resample_taps: 44100 -> 16001 reduces to" in err()
    # ws_resample_fwd(x, ldx, R, n_in, rate_in, rate_out, taps, y, ldy, stream)
    fwd = lambda *a: lib.ws_resample_fwd(*a, None)
    assert fwd(None, 100, 1, 100, 8000, 16000, p, p2, 200) == -1 and "ws_resample_fwd: x, taps or y is NULL" in err()
    assert fwd(p, 100, 1, 100, 8000, 16000, None, p2, 200) == -1 and "ws_resample_fwd: x, taps or y is NULL" in err()
    assert fwd(p, 100, 1, 100, 8000, 16000, p, None, 200) == -1 and "ws_resample_fwd: x, taps or y is NULL" in err()
    assert fwd(p, 100, 1, 100, -8000, 16000, p, p2, 200) == -1 and "ws_resample_fwd: rate_in=-8000" in err()
    assert fwd(p, 100, 1, 100, 16000, 16001, p, p2, 200) == -1 and "ws_resample_fwd: 16000 -> 16001 reduces to" in err()
    assert fwd(p, 100, 1, 0, 8000, 16000, p, p2, 200) == -1 and "ws_resample_fwd: bad sizes" in err()
    assert fwd(p, 100, 0, 100, 8000, 16000, p, p2, 200) == -1 and "ws_resample_fwd: bad sizes" in err()
    assert fwd(p, 99, 1, 100, 8000, 16000, p, p2, 200) == -1 and "ws_resample_fwd: row pitch ldx=99 below n_in=100" in err()
    assert fwd(p, 100, 1, 100, 8000, 16000, p, p2, 199) == -1 and "ldy=199 below n_out=200" in err()
    # ws_resample_stream_fwd(buf, ldb, R, rate_in, rate_out, taps, lead, n_valid, final, g_first, n_out, y, ldy, hist_from, hist_len, hist, ldh)
    sf = lambda *a: lib.ws_resample_stream_fwd(*a, None)
    ok = [p, 200, 1, 8000, 16000, p, 7, 100, 0, 0, 2 * 86, p2, 400, 86, 14, ctypes.c_void_p(p2.value + 2048), 14]
    bad = lambda i, val: sf(*[val if j == i else a for j, a in enumerate(ok)])
    assert bad(0, None) == -1 and "ws_resample_stream_fwd: buf or taps is NULL" in err()
    assert bad(5, None) == -1 and "ws_resample_stream_fwd: buf or taps is NULL" in err()
    assert bad(11, None) == -1 and "ws_resample_stream_fwd: y is NULL with n_out=172" in err()
    assert bad(15, None) == -1 and "ws_resample_stream_fwd: hist is NULL with hist_len=14" in err()
    assert bad(3, 0) == -1 and "ws_resample_stream_fwd: rate_in=0" in err()
    assert bad(4, 16001) == -1 and "ws_resample_stream_fwd: 8000 -> 16001 reduces to" in err()
    assert bad(2, 0) == -1 and "ws_resample_stream_fwd: bad sizes" in err()
    assert bad(7, 0) == -1 and "ws_resample_stream_fwd: bad sizes" in err()
    assert bad(6, 8) == -1 and "ws_resample_stream_fwd: lead=8 outside [0, w=7]" in err()
    assert bad(6, -1) == -1 and "ws_resample_stream_fwd: lead=-1 outside" in err()
    assert bad(1, 99) == -1 and "ws_resample_stream_fwd: a row pitch is below its row" in err()
    assert bad(13, 87) == -1 and "ws_resample_stream_fwd: history [87, 87 + 14) leaves the 100 valid samples" in err()
    assert bad(15, ctypes.c_void_p(p.value + 4 * 50)) == -1 and "ws_resample_stream_fwd: hist overlaps buf" in err()
    # 100 valid samples with 7 leading taps skipped: group g needs g + 8 samples -> 93 groups, 186 outputs
    assert bad(10, 2 * 94) == -1 and "need 101 valid samples, 100 are given and the end is not final" in err()
    final = list(ok)
    final[8], final[10] = 1, 201
    assert sf(*final) == -1 and "outputs up to 201 asked, the 100 valid samples end the signal at output 200" in err()


def test_emulated_kernel_whole_signal_is_the_restatement():
    rng = np.random.default_rng(0)
    for pair in RC.PAIRS:
        for n in (1, RC.GEOM[pair][2], RC.GEOM[pair][3], 257):
            x = rng.standard_normal(n)
            a, b = EMU.whole(x, *pair), RC.reference(x, *pair)
            assert a.shape == b.shape and np.allclose(a, b, rtol=0, atol=1e-12 * max(1.0, np.abs(x).max()) * 8)


def _splits(pair, values, x):
    """Every N in 0..3K and every split N = a + b into two pushes (a zero-length push is no push), then the flush.  The first
    push of a samples runs once per a; every b continues from a copy of the state it left."""
    U, D, w, K = RC.GEOM[pair]
    n_max = 3 * K
    memo = {} if values else None
    whole = [EMU.whole(x[:N], *pair, memo=memo) if values and N else np.zeros(0) for N in range(n_max + 1)]
    st = EMU.EmuStream(*pair, max_push=n_max, values=values, memo=memo)
    size = (lambda y: len(y)) if values else (lambda y: y[1] - y[0])
    empty = np.zeros(0) if values else (0, 0)
    checked = 0
    for a in range(n_max + 1):
        st.reset()
        y1 = st.push(x[:a]) if a else empty
        assert size(y1) == RC.emitted(a, *pair), (pair, a)
        assert st.h < K and np.array_equal(st.history(), x[a - st.h:a]), (pair, a)
        snap = st.snapshot()
        for b in range(n_max - a + 1):
            N = a + b
            st.restore(snap)
            y2 = st.push(x[a:N]) if b else empty
            assert size(y2) == RC.emitted(N, *pair) - RC.emitted(a, *pair), (pair, a, b)
            assert st.h < K and np.array_equal(st.history(), x[N - st.h:N]), (pair, a, b)
            y3 = st.flush()
            if values:
                assert np.array_equal(np.concatenate([y1, y2, y3]), whole[N]), (pair, a, b)
            else:
                pos = 0
                for lo, hi in (y1, y2, y3):
                    if hi > lo:
                        assert lo == pos, (pair, a, b)
                        pos = hi
                assert pos == RC.out_len(N, *pair), (pair, a, b)
            checked += 1
    return checked


@pytest.mark.parametrize("pair", STREAM_PAIRS)
def test_emission_counts_and_indices_for_every_split(pair):
    K = RC.GEOM[pair][3]
    assert _splits(pair, False, np.arange(3 * K, dtype=np.int64)) == (3 * K + 1) * (3 * K + 2) // 2


@pytest.mark.parametrize("pair", STREAM_PAIRS)
def test_streamed_values_equal_the_whole_signal_exactly(pair):
    K = RC.GEOM[pair][3]
    x = np.random.default_rng(1).standard_normal(3 * K)
    assert _splits(pair, True, x) == (3 * K + 1) * (3 * K + 2) // 2


def test_memoised_kernel_emulation_is_the_plain_one_and_checks_its_samples():
    pair = (44100, 16000)
    x = np.random.default_rng(2).standard_normal(1500)
    memo = {}
    a = EMU.whole(x, *pair, memo=memo)
    assert memo and np.array_equal(a, EMU.whole(x, *pair)) and np.array_equal(a, EMU.whole(x, *pair, memo=memo))
    y = x.copy()
    y[700] += 1.0                                   # other samples under the same entry names: recomputed, not reused
    b = EMU.whole(y, *pair, memo=memo)
    assert np.array_equal(b, EMU.whole(y, *pair)) and not np.array_equal(a, b)


def test_emulation_refuses_what_the_kernel_refuses():
    g = RC.GEOM[(8000, 16000)]
    with pytest.raises(EMU.Refused, match="not final"):
        EMU.check_call(g, 7, 100, False, 0, 2 * 94, 0, 0)
    with pytest.raises(EMU.Refused, match="past the end"):
        EMU.check_call(g, 7, 100, True, 0, 201, 0, 0)
    EMU.check_call(g, 7, 100, False, 0, 2 * 93, 86, 14)
    EMU.check_call(g, 7, 100, True, 0, 200, 0, 0)
    with pytest.raises(EMU.Refused, match="not sample 0"):
        EMU.kernel_ranges(g, 5, 7, 100, False, 0, 2, 200)
