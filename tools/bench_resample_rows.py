"""The rows form of the streaming resampler: one launch for N streams at mixed rates against N solo launches.

    python tools/bench_resample_rows.py --out profiles/resample_rows.json --md profiles/resample_rows.md

N = 1, 4, 8 and 16 streams with their rates cycled over 8 / 16 / 48 kHz, every stream in mid-stream with one 10 ms packet
behind its history -- the step of resampler A of a rate stream (caller -> 16 kHz; the 16 kHz rows run the identity table).
Three arms in ONE run, alternating, `--repeats` runs each, HIP events around `--iters` back-to-back rounds:
  rows    one ws_resample_stream_rows_fwd over all N rows: the table's upload (N * 72 bytes, pinned, on the stream) and the
          launch, through dev.resample_stream_rows_fwd with a table made once
  solo    N ws_resample_stream_fwd calls with R = 1, the 16 kHz rows as a device copy -- what N solo streams issue
  copy    one ws_rows_copy_fwd that gathers N rows of 170 pending samples into a rectangle of pitch 310, zeros behind them
Time is per ROUND through the Python binding: for kernels this short it is the host's issue rate (ctypes calls, the upload's
enqueue), not the kernels' duration.  Before timing, the rows arm's outputs are compared with the solo arm's (torch.equal).
The --md file is rewritten up to the line `<!-- notes -->`; what follows it is kept.  Needs a GPU.  Nothing here is a gate."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RATES, MODEL_RATE, MS = (8000, 16000, 48000), 16000, 10


def make_round(N, d):
    """N mid-stream rows: history of K - 1 samples, one packet behind it; arenas, the table, and the solo calls' arguments"""
    from wesep_amd import dev
    from wesep_amd.resample import geometry, step_plan
    tables, t_off, rows, solo = [], {}, [], []
    n_buf = n_y = n_hist = 0
    for i in range(N):
        rate = RATES[i % len(RATES)]
        ident = rate == MODEL_RATE
        U, D, w, K = (1, 1, 0, 1) if ident else geometry(rate, MODEL_RATE)
        if rate not in t_off:
            t_off[rate] = sum(t.size for t in tables)
            tables.append(np.ones(1, np.float32) if ident else dev.resample_taps(rate, MODEL_RATE).reshape(-1))
        n = rate * MS // 1000
        # a stream that has taken 50 packets: its counters, then one more packet
        n_in = 50 * n
        groups = max(0, (n_in - w) // D)
        h = n_in - max(0, groups * D - w)
        lead, n_valid, n_out, hist_from, hist_len, _ = step_plan((U, D, w, K), n_in, groups, h, n, False)
        rows.append(dict(in_off=n_buf, taps_off=t_off[rate], out_off=n_y, hist_off=n_hist, U=U, D=D, K=K, lead=lead, n_valid=n_valid,
                         n_out=n_out, hist_from=hist_from, hist_len=hist_len))
        solo.append((rate, ident, n_buf, n_valid, lead, n_y, n_out, n_hist, hist_from, hist_len))
        n_buf, n_y, n_hist = n_buf + n_valid, n_y + n_out, n_hist + max(hist_len, 1)
    g = torch.Generator().manual_seed(N)
    return dict(tab=dev.resample_rows_table(rows), solo=solo, buf=torch.randn(n_buf, generator=g).to(d),
                taps=torch.from_numpy(np.concatenate(tables)).to(d), y=torch.zeros(n_y, device=d), hist=torch.zeros(n_hist, device=d))


def arm_rows(r):
    from wesep_amd import dev
    dev.resample_stream_rows_fwd(r["tab"], r["buf"], r["taps"], r["y"], r["hist"])


def arm_solo(r, y, hist):
    from wesep_amd import dev
    from wesep_amd.resample import taps_on
    for rate, ident, in_off, n_valid, lead, out_off, n_out, hist_off, hist_from, hist_len in r["solo"]:
        if ident:
            y[out_off:out_off + n_out].copy_(r["buf"][in_off:in_off + n_out])
            continue
        dev.resample_stream_fwd(r["buf"][in_off:in_off + n_valid][None], rate, MODEL_RATE, taps_on(rate, MODEL_RATE, y.device), lead, n_valid, False, 0,
                                n_out, y[out_off:out_off + n_out][None], hist_from, hist_len, hist[hist_off:hist_off + hist_len][None])


def arm_copy(c):
    from wesep_amd import dev
    dev.rows_copy_fwd(c["tab"], c["src"], c["dst"])


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--streams", default="1,4,8,16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample_rows: needs a GPU (no CPU measurement exists)")
    from wesep_amd import dev
    d = torch.device("cuda:0")
    cases = []
    for N in map(int, a.streams.split(",")):
        r = make_round(N, d)
        y2, h2 = torch.zeros_like(r["y"]), torch.zeros_like(r["hist"])
        have, pitch = 170, 310
        c = dict(tab=dev.rows_copy_table([dict(src_off=i * 512, dst_off=i * pitch, len=have, fill=pitch - have) for i in range(N)]),
                 src=torch.randn(N * 512, device=d), dst=torch.empty(N * pitch, device=d))
        arms = {"rows": lambda: arm_rows(r), "solo": lambda: arm_solo(r, y2, h2), "copy": lambda: arm_copy(c)}
        for _ in range(20):
            for fn in arms.values():
                fn()
        torch.cuda.synchronize()
        if not (torch.equal(r["y"], y2) and torch.equal(r["hist"], h2)):
            raise SystemExit(f"bench_resample_rows: N={N}: the rows launch and the solo calls differ")
        runs = {k: [] for k in arms}
        for _ in range(a.repeats):                       # the arms alternate: drift hits them alike
            for k, fn in arms.items():
                runs[k].append(timed(fn, a.iters))
        case = dict(streams=N, rates=[RATES[i % len(RATES)] for i in range(N)], outputs=int(r["y"].numel()),
                    launches=dict(rows=1, solo=N, copy=1), us_runs=runs,
                    us_median={k: statistics.median(v) for k, v in runs.items()}, us_min={k: min(v) for k, v in runs.items()},
                    us_max={k: max(v) for k, v in runs.items()})
        cases.append(case)
        print(json.dumps(case), flush=True)
    name = torch.cuda.get_device_name(0)
    lines = ["# Rows forms of the resampler: one launch for N streams at mixed rates", "",
             f"Written by `tools/bench_resample_rows.py` on {name}; JSON beside this file.  Nothing here is a gate.", "",
             f"## One round of resampler A for N streams (rates cycled over 8 / 16 / 48 kHz, one {MS} ms packet each, mid-stream): µs per "
             f"round through the Python binding, HIP events around {a.iters} back-to-back rounds, {a.repeats} runs per arm, alternating "
             "(median, min – max)", "",
             "rows: the table's upload and ONE `ws_resample_stream_rows_fwd`.  solo: N `ws_resample_stream_fwd` calls with R = 1 (a 16 kHz "
             "row: a device copy).  copy: ONE `ws_rows_copy_fwd` gathering N rows of 170 samples into pitch 310.  The rows launch's outputs "
             "and histories were compared with the solo calls' before timing (`torch.equal`).", "",
             "| N | outputs | rows: launches | rows µs | min – max | solo: launches | solo µs | min – max | solo / rows | copy µs | min – max |",
             "|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in cases:
        m, lo, hi = c["us_median"], c["us_min"], c["us_max"]
        lines.append(f"| {c['streams']} | {c['outputs']} | 1 | {m['rows']:.1f} | {lo['rows']:.1f} – {hi['rows']:.1f} | {c['streams']} | {m['solo']:.1f} | "
                     f"{lo['solo']:.1f} – {hi['solo']:.1f} | {m['solo'] / m['rows']:.2f} | {m['copy']:.1f} | {lo['copy']:.1f} – {hi['copy']:.1f} |")
    lines += ["", "<!-- notes -->"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=name, model_rate=MODEL_RATE, packet_ms=MS, iters=a.iters, cases=cases), f, indent=1)
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
