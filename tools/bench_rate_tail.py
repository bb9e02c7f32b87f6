"""Rate tail pool (ws_engine_rate_tail_pool_*): a steady tick of 4 staggered live recordings at 8 / 16 / 48 / 48 kHz against the
plain tail pool at 16 kHz on the same feed, in the same run; and the three launches a rate tick adds, alone.

    python tools/bench_rate_tail.py --out profiles/rate_tail.json --md profiles/rate_tail.md

pBSRNN (6 repeats), Conv-TasNet / SpEx+ (N 256) and DPCCN as their constructors build them (tools/bench_live.py MODELS), fixed
embeddings, K = 2 targets, container rate 16 kHz, window S = 4 s, fade 20 ms, warm S / 2, max_rows 8.  Four recordings of the
same duration in packets of 100 ms AT THEIR OWN RATE, a tick every 500 ms; recording i starts 3 i packets late, so no two are
aligned.  Arm "rate": one rate tail pool, the recordings at 8, 16, 48 and 48 kHz.  Arm "plain": one tail pool, four recordings at
16 kHz of the same duration, the same packets in time.  A tick's time is the host clock around it (it synchronises itself).
*steady* ticks: every recording in flight has more than a window of audio, so all 8 rows share one forward in both arms.  After
one warm-up run per arm, `--repeats` runs per arm, alternating: median and min - max.  "added launches alone": the gather, the
emission and resampler B with the tables of such a steady tick (8 rows), through the Python bindings on one stream, 5 warm-up
rounds, then `--trio_iters` rounds timed back to back with one synchronisation at the end.  The --md file is rewritten up to
the line `<!-- notes -->`; what follows it is kept.  Needs a GPU.  Nothing here is a gate."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_live import MODELS, SR  # noqa: E402

RATES = (8000, 16000, 48000, 48000)
ARCHS = ("pBSRNN", "ConvTasNet", "DPCCN")


def run(eng, E, mixes, rates, embs, S, C, warm, max_rows, packet_ms, every, stagger, rate_arm):
    """-> dict(steady [ms], other [ms], total ms, shapes {(forwards, rows, launches)}, state bytes)"""
    N, K = len(mixes), embs[0].shape[0]
    if rate_arm:
        pool = eng.rate_tail_pool(N, K, S, C, sorted(set(rates)), warm, max_rows)
        slots = [pool.attach(embs[i], E.ENROLL_EMBEDDING, rates[i]) for i in range(N)]
        keys = ("rate_tail_pool_state_bytes", "rate_tail_pool_forwards", "rate_tail_pool_rows")
    else:
        pool = eng.tail_pool(N, K, S, C, warm, max_rows)
        slots = [pool.attach(embs[i], E.ENROLL_EMBEDDING) for i in range(N)]
        keys = ("tail_pool_state_bytes", "tail_pool_forwards", "tail_pool_rows")
    state = eng.info(keys[0])
    packet = [r * packet_ms // 1000 for r in rates]
    pos, steady, other, shapes = [0] * N, [], [], set()
    t_all, t = time.perf_counter(), 0
    while any(p < len(m) for p, m in zip(pos, mixes)):
        live = [i for i in range(N) if t >= stagger * i and pos[i] < len(mixes[i])]
        if live:
            pool.push({slots[i]: mixes[i][pos[i]:pos[i] + packet[i]] for i in live})
        for i in live:
            pos[i] = min(len(mixes[i]), pos[i] + packet[i])
        if live and (t + 1) % every == 0:
            # more than a window of audio everywhere (a packet to spare for the filters' look-ahead): every row is a full window
            full = all(pos[i] * SR // rates[i] >= S + SR * packet_ms // 1000 for i in live)
            t0 = time.perf_counter()
            pool.tick([slots[i] for i in live])
            dt = (time.perf_counter() - t0) * 1e3
            if eng.info(keys[2]):
                (steady if full and len(live) == N else other).append(dt)
                if full and len(live) == N:
                    shapes.add((eng.info(keys[1]), eng.info(keys[2]), eng.info("n_launches")))
        for i in live:
            if pos[i] >= len(mixes[i]):
                pool.flush(slots[i])
        t += 1
    total = (time.perf_counter() - t_all) * 1e3
    pool.close()
    return dict(steady=steady, other=other, total=total, shapes=sorted(shapes), state=state)


def trio_alone(S, C, m, K, iters):
    """The gather, the emission and resampler B on the tables of a steady tick of RATES (K rows each), alone -> ms per round"""
    from wesep_amd import dev
    from wesep_amd.resample import step_plan
    d = torch.device("cuda:0")
    geom = lambda a, b: (1, 1, 0, 1) if a == b else dev.resample_geom(a, b)
    taps, taps_at, at = [], {}, 0
    for r in sorted(set(RATES)):
        for pair in ((r, SR), (SR, r)):
            t = np.ones(1, np.float32) if r == SR else dev.resample_taps(*pair).reshape(-1)
            taps_at[pair], at = at, at + len(t)
            taps.append(t)
    taps = torch.from_numpy(np.concatenate(taps)).to(d)
    gather, emit, brows = [], [], []
    span_at, row_at, hold_at, b_at, out_at = 0, 0, 0, 0, 0
    N0 = 3 * S + 17                                                  # a window that starts at no group boundary
    for r in RATES:
        U, D, w, Kt = geom(r, SR)
        a0 = N0 - S
        g_a, g_last = a0 // U, (N0 - 1) // U
        lo, hi = g_a * D - w, g_last * D - w + Kt
        bg = geom(SR, r)
        n_in = 10 * m
        groups = max(0, (n_in - bg[2]) // bg[1])
        h = n_in - max(0, groups * bg[1] - bg[2])
        lead, n_valid, n_out, hist_from, hist_len, _ = step_plan(bg, n_in, groups, h, m, False)
        b_ld = (bg[3] - 1 + S + 3) // 4 * 4
        for _k in range(K):
            gather.append(dict(in_off=span_at, taps_off=taps_at[(r, SR)], out_off=row_at, U=U, D=D, K=Kt, lead=0, n_valid=hi - lo, final=0,
                               g_first=0, p_first=a0 % U, L=S, fill=0))
            emit.append(dict(y_off=row_at, hold_in_off=hold_at, hold_out_off=hold_at + C, out_off=b_at + h, L=S, p=S - C - m, h=C, m=m,
                             c_new=C, scale=1.0))
            brows.append(dict(in_off=b_at, taps_off=taps_at[(SR, r)], out_off=out_at, hist_off=b_at + b_ld, U=bg[0], D=bg[1], K=bg[3],
                              lead=lead, n_valid=n_valid, final=0, n_out=n_out, hist_from=hist_from, hist_len=hist_len))
            row_at, hold_at, b_at, out_at = row_at + S, hold_at + 2 * C, b_at + 2 * b_ld, out_at + n_out
        span_at += hi - lo
    g = torch.Generator(device="cpu").manual_seed(0)
    spans, rows = torch.randn(span_at, generator=g).to(d), torch.zeros(row_at, device=d)
    hold, bbuf, out = torch.zeros(hold_at, device=d), torch.zeros(b_at, device=d), torch.zeros(out_at, device=d)
    ramp = ((torch.arange(C, dtype=torch.float32) + 1) / (C + 1)).to(d)
    tabs = dev.window_resample_rows_table(gather), dev.tail_emit_rows_table(emit), dev.resample_rows_table(brows)

    def trio():
        return (dev.window_resample_rows(tabs[0], spans, taps, rows), dev.tail_emit_rows(tabs[1], C, ramp, rows, hold, bbuf),
                dev.resample_stream_rows_fwd(tabs[2], bbuf, taps, out, bbuf))

    for _ in range(5):
        trio()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    keep = [trio() for _ in range(iters)]
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / iters
    del keep
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--archs", default=",".join(ARCHS))
    ap.add_argument("--packet_ms", type=int, default=100)
    ap.add_argument("--tick_ms", type=int, default=500)
    ap.add_argument("--fade_ms", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=12.0, help="every recording")
    ap.add_argument("--window", type=float, default=4.0)
    ap.add_argument("--max_rows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--trio_iters", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rate_tail: needs a GPU (no CPU measurement exists)")
    if a.tick_ms % a.packet_ms:
        raise SystemExit("bench_rate_tail: the tick period is a whole number of packets")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    S, C, K, every = int(a.window * SR), SR * a.fade_ms // 1000, 2, a.tick_ms // a.packet_ms
    rng = np.random.default_rng(0)
    feed = {True: RATES, False: (SR,) * len(RATES)}
    mixes = {arm: [(0.1 * rng.standard_normal(int(a.seconds * r))).astype(np.float32) for r in rates] for arm, rates in feed.items()}
    embs = [rng.standard_normal((K, 256)).astype(np.float32) for _ in RATES]
    trio_ms = trio_alone(S, C, SR * a.tick_ms // 1000, K, a.trio_iters)
    print(json.dumps(dict(added_launches_alone_ms=trio_ms)), flush=True)
    tmp = tempfile.mkdtemp()
    cases = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for arch in a.archs.split(","):
        name, kw = MODELS[arch]
        torch.manual_seed(0)
        path = os.path.join(tmp, f"{arch}.wsw")
        export_engine(get_model(name)(joint_training=False, **kw), path)
        eng = E.Engine(path)
        args = (S, C, S // 2, a.max_rows, a.packet_ms, every, 3)
        short_s = a.window + (2 * every + 3 * len(RATES) + 2) * a.packet_ms / 1000.0      # every shape of the timed runs
        for arm in (True, False):
            run(eng, E, [x[:int(short_s * r)] for x, r in zip(mixes[arm], feed[arm])], feed[arm], embs, *args, arm)
        runs = {True: [], False: []}
        for _ in range(a.repeats):                                            # the arms alternate: drift hits them alike
            for arm in (True, False):
                runs[arm].append(run(eng, E, mixes[arm], feed[arm], embs, *args, arm))
        for arm, rs in runs.items():
            med = [statistics.median(r["steady"]) for r in rs]
            c = dict(arch=arch, path="rate tail pool, 8 / 16 / 48 / 48 kHz" if arm else "tail pool, 16 kHz", steady_ticks=len(rs[0]["steady"]),
                     tick_ms=statistics.median(med), tick_ms_runs=med, tick_worst_ms=max(max(r["steady"]) for r in rs),
                     total_ms=statistics.median(r["total"] for r in rs), state_bytes=rs[0]["state"], shapes=rs[0]["shapes"])
            cases.append(c)
            print(json.dumps(c), flush=True)
        cases[-2]["over_plain_ms"] = cases[-2]["tick_ms"] - cases[-1]["tick_ms"]
        with open(a.out, "w") as f:                                           # what is measured so far
            json.dump(dict(partial=True, added_launches_alone_ms=trio_ms, cases=cases), f, indent=1)
        eng.close()
        os.remove(path)
    os.rmdir(tmp)
    dev_name = torch.cuda.get_device_name(0)
    lines = ["# Rate tail pool: a tick of 4 staggered recordings at 8 / 16 / 48 / 48 kHz against the plain tail pool at 16 kHz", "",
             f"Written by `tools/bench_rate_tail.py` on {dev_name}; JSON beside this file.  Recipe geometries, fixed embeddings, K = 2 "
             f"targets, container rate 16 kHz, window {a.window:g} s, fade {a.fade_ms} ms, warm {a.window / 2:g} s, max_rows {a.max_rows}, 4 "
             f"recordings of {a.seconds:g} s in packets of {a.packet_ms} ms at their own rate, a tick every {a.tick_ms} ms, recording i started "
             f"3 i packets late, {a.repeats} runs per arm after a warm-up run per arm (median; min – max), the arms alternating in the same "
             f"run.  wall = host clock around the tick; it synchronises itself.  *steady*: every recording has more than a window of audio: "
             f"8 rows, one forward, in both arms.  Nothing here is a gate.", "",
             "| model | path | steady ticks | ms / steady tick (median; min – max; worst) | rate − plain, ms | forwards, rows, launches / steady "
             "tick | total ms | state bytes |", "|---|---|---|---|---|---|---|---|"]
    for c in cases:
        shapes = "—" if not c["shapes"] else "; ".join(f"{f}, {r}, {l}" for f, r, l in c["shapes"])
        over = f"{c['over_plain_ms']:+.3f}" if "over_plain_ms" in c else "—"
        lines.append(f"| {c['arch']} | {c['path']} | {c['steady_ticks']} | {c['tick_ms']:.2f} ({min(c['tick_ms_runs']):.2f} – "
                     f"{max(c['tick_ms_runs']):.2f}; {c['tick_worst_ms']:.2f}) | {over} | {shapes} | {c['total_ms']:.1f} | {c['state_bytes']} |")
    lines += ["", f"The three added launches alone (gather of 8 windows of {S} samples, emission of 8 x {SR * a.tick_ms // 1000} samples, resampler B "
              f"over the 8 rows; Python bindings, table uploads included, {a.trio_iters} rounds back to back, one synchronisation): "
              f"**{trio_ms:.3f} ms** per round.", "", "<!-- notes -->"]
    with open(a.out, "w") as f:
        json.dump(dict(sample_rate=SR, rates=RATES, window_s=a.window, fade_ms=a.fade_ms, tick_ms=a.tick_ms, seconds=a.seconds, max_rows=a.max_rows,
                       packet_ms=a.packet_ms, repeats=a.repeats, device=dev_name, added_launches_alone_ms=trio_ms, trio_iters=a.trio_iters,
                       cases=cases), f, indent=1)
    if a.md:
        keep = ""
        if os.path.exists(a.md):
            old = open(a.md).read()
            if "<!-- notes -->" in old:
                keep = old.split("<!-- notes -->", 1)[1]
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + keep)
    print("\n".join(lines))


if __name__ == "__main__":
    main()
