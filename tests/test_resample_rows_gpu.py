"""GPU: the rows forms of the resampler through the C ABI (wesep_amd.dev / wesep_amd.resample).  One launch over the table of
seven rows of tests/emu_resample_rows.py (tables in LDS and in global memory, the identity table, a stream's start, middle
and end, a row that only moves its history, 586 outputs beside 3): outputs and histories bit for bit those of seven
ws_resample_stream_fwd calls with R = 1, within the fp64 bound of tests/resample_contract.py, nothing written outside the
rows' ranges.  The rows copy against indexing.  StreamResamplerRows against one StreamResampler a row."""
import numpy as np
import pytest
import torch

from tests import emu_resample_rows as ROWS
from tests import resample_contract as RC

pytestmark = pytest.mark.gpu
GUARD = 12345.0


@pytest.fixture(scope="module")
def seven():
    """the launch, once: (rows, meta, buf, taps, y, hist) with y and hist sentinel-filled before it"""
    from wesep_amd import dev
    d = torch.device("cuda:0")
    rows, arenas, meta = ROWS.seven_rows()
    buf, taps = torch.from_numpy(arenas["buf"]).to(d), torch.from_numpy(arenas["taps"]).to(d)
    y = torch.full((arenas["n_y"],), GUARD, device=d)
    hist = torch.full((arenas["n_hist"],), GUARD, device=d)
    dev.resample_stream_rows_fwd(rows, buf, taps, y, hist)
    torch.cuda.synchronize()
    return rows, meta, buf, taps, y, hist


def test_seven_rows_equal_seven_solo_calls(seven):
    from wesep_amd import dev
    from wesep_amd.resample import taps_on
    rows, meta, buf, taps, y, hist = seven
    for i, (r, (pair, z, _)) in enumerate(zip(rows, meta)):
        got = y[r["out_off"]:r["out_off"] + r["n_out"]]
        got_h = hist[r["hist_off"]:r["hist_off"] + r["hist_len"]]
        b = buf[r["in_off"]:r["in_off"] + r["n_valid"]].clone()[None]
        if pair is None:                    # the identity table: no solo call has this geometry; the samples themselves
            assert torch.equal(got, b[0, r["g_first"]:r["g_first"] + r["n_out"]]), i
            continue
        ys = torch.full((1, r["n_out"] + 2), GUARD, device=buf.device) if r["n_out"] else None
        hs = torch.full((1, r["hist_len"] + 2), GUARD, device=buf.device) if r["hist_len"] else None
        dev.resample_stream_fwd(b, *pair, taps_on(*pair, buf.device), r["lead"], r["n_valid"], bool(r["final"]), r["g_first"], r["n_out"], ys,
                                r["hist_from"], r["hist_len"], hs)
        if ys is not None:
            assert torch.equal(got, ys[0, :r["n_out"]]), (i, pair)
        if hs is not None:
            assert torch.equal(got_h, hs[0, :r["hist_len"]]) and torch.equal(got_h, b[0, r["hist_from"]:r["hist_from"] + r["hist_len"]]), (i, pair)


def test_seven_rows_against_fp64_and_sentinels(seven):
    rows, meta, buf, taps, y, hist = seven
    yh, hh = y.cpu().numpy().astype(np.float64), hist.cpu().numpy()
    free_y, free_h = np.ones(len(yh), bool), np.ones(len(hh), bool)
    for i, (r, (pair, z, q0)) in enumerate(zip(rows, meta)):
        got = yh[r["out_off"]:r["out_off"] + r["n_out"]]
        free_y[r["out_off"]:r["out_off"] + r["n_out"]] = False
        free_h[r["hist_off"]:r["hist_off"] + r["hist_len"]] = False
        assert np.all(np.isfinite(got)), i
        if pair is None:
            continue
        ref, bnd = RC.reference(z, *pair)[q0:q0 + r["n_out"]], RC.bound(z, *pair)[q0:q0 + r["n_out"]]
        e = np.abs(got - ref)
        if r["n_out"]:
            print(f"row {i} {pair}: worst error / bound {float(np.max(e / np.maximum(bnd, 1e-300))):.3f}")
        assert np.all(e <= bnd), (i, pair, float(e.max()))
    assert free_y.sum() == ROWS.GAP * 8 and np.all(yh[free_y] == GUARD), "wrote outside the rows' y ranges"
    assert free_h.sum() == ROWS.GAP * 8 and np.all(hh[free_h] == GUARD), "wrote outside the rows' hist ranges"


def test_rows_copy_gathers_and_scatters():
    from wesep_amd import dev
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    state = torch.randn(5000, generator=g).to(d)             # per-slot pending samples at slot offsets
    off, have, pitch = [7, 1500, 3001], [700, 3, 257], 700
    rect = torch.full((3 * pitch + 4,), GUARD, device=d)
    dev.rows_copy_fwd([dict(src_off=o, dst_off=2 + i * pitch, len=n, fill=pitch - n) for i, (o, n) in enumerate(zip(off, have))], state, rect)
    want = torch.full_like(rect, GUARD)
    for i, (o, n) in enumerate(zip(off, have)):
        want[2 + i * pitch:2 + (i + 1) * pitch] = 0
        want[2 + i * pitch:2 + i * pitch + n] = state[o:o + n]
    assert torch.equal(rect, want)
    back = torch.full((5000,), GUARD, device=d)               # the scatter: each row's samples behind another offset
    dst = [4000, 10, 2000]
    dev.rows_copy_fwd([dict(src_off=2 + i * pitch, dst_off=o, len=n, fill=0) for i, (o, n) in enumerate(zip(dst, have))], rect, back)
    want = torch.full_like(back, GUARD)
    for i, (o, n) in enumerate(zip(dst, have)):
        want[o:o + n] = state[off[i]:off[i] + n]
    assert torch.equal(back, want)
    only_fill = torch.full((300,), GUARD, device=d)
    dev.rows_copy_fwd([dict(src_off=0, dst_off=1, len=0, fill=298)], state, only_fill)
    assert only_fill[0] == GUARD and only_fill[299] == GUARD and torch.all(only_fill[1:299] == 0)


PAIRS = [(8000, 16000), (48000, 16000), (16000, 16000), (44100, 16000), (16000, 48000), (16000, 44100)]


def _packets(rng, n, rate):
    """10 ms packets, one of 250 ms among them, a random tail"""
    out, left, i = [], n, 0
    while left:
        c = min(left, rate // 4 if i == 3 else (rate // 100 if i < 8 else int(rng.integers(1, 700))))
        out.append(c)
        left -= c
        i += 1
    return out


def test_stream_rows_equal_one_solo_stream_a_row():
    """rows at six pairs of rates, each with its own packet sizes, a late start and an early end: every push and the flush
    bit for bit a StreamResampler of one row, also when the other rows carry other data, inf and NaN; one launch a round"""
    from wesep_amd.resample import StreamResampler, StreamResamplerRows
    d = torch.device("cuda:0")
    rng = np.random.default_rng(9)
    n = [int(0.3 * p[0]) + 7 * i for i, p in enumerate(PAIRS)]
    x = [torch.from_numpy(rng.uniform(-1, 1, size=m).astype(np.float32)).to(d) for m in n]
    packets = [_packets(rng, m, p[0]) for m, p in zip(n, PAIRS)]
    start = [0, 2, 0, 1, 3, 0]                      # the round in which a row's first packet arrives

    def run(signals, max_push=1000):
        pool = StreamResamplerRows(PAIRS, max_push=max_push, device=d)
        outs, pos, nxt = [[] for _ in PAIRS], [0] * len(PAIRS), [0] * len(PAIRS)
        rnd = 0
        while any(nxt[i] <= len(packets[i]) for i in range(len(PAIRS))):
            chunks, ending = {}, []
            for i in range(len(PAIRS)):
                if rnd < start[i] or nxt[i] > len(packets[i]):
                    continue
                if nxt[i] == len(packets[i]):
                    ending.append(i)
                else:
                    c = packets[i][nxt[i]]
                    chunks[i] = signals[i][pos[i]:pos[i] + c]
                    pos[i] += c
                nxt[i] += 1
            before = pool.launches
            if chunks:
                for i, y in pool.push(chunks).items():
                    outs[i].append(y)
                pieces = max(-(-c.shape[0] // max_push) for c in chunks.values())
                assert pool.launches - before == pieces, "one launch a round, whatever the rows and rates"
            for i, y in pool.flush(ending).items():
                outs[i].append(y)
            rnd += 1
        return [torch.cat(o) for o in outs]

    got = run(x)
    for i, pair in enumerate(PAIRS):
        if pair[0] == pair[1]:
            assert torch.equal(got[i], x[i]), pair
            continue
        solo = StreamResampler(1, *pair, max_push=1000, device=d)
        seen, ys = 0, []
        for c in packets[i]:
            ys.append(solo.push(x[i][None, seen:seen + c])[0])
            seen += c
        ys.append(solo.flush()[0])
        want = torch.cat(ys)
        assert got[i].shape == want.shape == (RC.out_len(n[i], *pair),) and torch.equal(got[i], want), pair
    # isolation: row 1 and row 3 keep their bits when every other row carries other data, inf and NaN
    other = [torch.full_like(s, float("nan")) if i % 2 == 0 else s for i, s in enumerate(x)]
    other[4] = torch.full_like(x[4], float("inf"))
    other[5] = -x[5]
    again = run(other)
    assert torch.equal(again[1], got[1]) and torch.equal(again[3], got[3])
