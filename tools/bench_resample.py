"""The device resampler: kernel time per call, and a rate-stream push against a plain push.

    python tools/bench_resample.py --out profiles/resample.json --md profiles/resample.md

Part 1, kernel: ws_resample_fwd for the seven rate pairs of include/wesep_hip.h ("sample rates") at 10 ms and 4 s of audio,
one row.  HIP events around `--iters` back-to-back calls, three runs, median and min - max: time per CALL through the
Python binding (a geometry call and the launch call through ctypes, then the launch), which for a short kernel is the
host's issue rate, not the kernel's duration.  For the kernel's own duration run the kernel part alone under a kernel
trace -- `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_resample.py --kernels_only --iters 20
--repeats 1 --out k.json`: every case then is 25 dispatches of `resample_kernel` (5 warm-up), in the order of the JSON.
Next to the time: the bytes a call must move at least (input once, output once, the tap table once) and the GB/s that
makes; for the 44.1 kHz and 22.05 kHz pairs the table (300 - 575 KB, read through the caches) is most of the traffic of a 10 ms call.  No roofline
target is set.
Part 2, streams: on the SpEx+ shape of profiles/engine_stream.md, rows 1 and 8, 10 ms packets -- the plain stream's push
(160 samples at 16 kHz) and the rate stream's push at 8 kHz (80 samples) and 48 kHz (480 samples), default path and
WS_STREAM_BLOCK_KERNEL, wall ms per push (the push synchronises itself, once), three runs per arm, alternating.
The --md file is rewritten up to the line `<!-- notes -->`; what follows it is kept.  Needs a GPU.  Nothing here is a gate."""
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

PAIRS = [(8000, 16000), (48000, 16000), (44100, 16000), (16000, 8000), (16000, 48000), (16000, 44100), (22050, 16000)]
SHAPE = dict(N=256, L=20, B=256, H=512, P=3, X=8, R=4, norm="cLN", causal=True, spk_emb_dim=256, joint_training=False)
G, WARMUP = 256, 20


def kernel_case(pair, seconds, iters, repeats):
    from wesep_amd import dev
    from wesep_amd.resample import geometry, out_len, taps_on
    d = torch.device("cuda:0")
    U, D, w, K = geometry(*pair)
    n_in = max(1, int(round(pair[0] * seconds)))
    n_out = out_len(n_in, *pair)
    x = torch.randn(1, n_in, device=d)
    y = torch.empty(1, n_out, device=d)
    taps = taps_on(*pair, d)
    for _ in range(5):
        dev.resample_fwd(x, n_in, *pair, taps, y)
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            dev.resample_fwd(x, n_in, *pair, taps, y)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) * 1e3 / iters)
    nbytes = 4 * (n_in + n_out + U * K)
    med = statistics.median(runs)
    return dict(rate_in=pair[0], rate_out=pair[1], U=U, D=D, w=w, K=K, taps_bytes=4 * U * K, staging="LDS" if U * K <= 2048 else "global",
                seconds=seconds, n_in=n_in, n_out=n_out, us_runs=runs, us_median=med, us_min=min(runs), us_max=max(runs),
                bytes_min=nbytes, gb_per_s=nbytes / med / 1e3, mac_per_call=n_out * K)


def stream_arm(eng, rows, rate, ms, pushes, block_kernel):
    from wesep_amd import engine as E
    n = rate * ms // 1000
    rng = np.random.default_rng(rows * 1000 + n)
    x = (0.1 * rng.standard_normal((rows, (WARMUP + pushes) * n))).astype(np.float32)
    emb = rng.standard_normal((rows, 256)).astype(np.float32)
    if rate == 16000:
        st = eng.stream(rows, emb, E.ENROLL_EMBEDDING, max_chunk_frames=G, block_kernel=block_kernel)
    else:
        st = eng.rate_stream(rows, emb, E.ENROLL_EMBEDDING, rate, max_chunk_frames=G, max_push=n, block_kernel=block_kernel)
    chunks = [np.ascontiguousarray(x[:, i * n:(i + 1) * n]) for i in range(WARMUP + pushes)]
    for c in chunks[:WARMUP]:
        st.push(c)
    launches = set()
    t0 = time.perf_counter()
    for c in chunks[WARMUP:]:
        st.push(c)
        launches.add(eng.info("n_launches"))
    wall_ms = (time.perf_counter() - t0) * 1e3 / pushes
    state = eng.info("stream_state_bytes")
    st.close()
    return dict(wall_ms=wall_ms, launches=max(launches), state_bytes=state)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--seconds", type=float, default=4.0, help="audio per stream run")
    ap.add_argument("--kernels_only", action="store_true", help="part 1 only, JSON only (for a run under a kernel trace)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_resample: needs a GPU (no CPU measurement exists)")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    kernels = []
    for pair in PAIRS:
        for seconds in (0.01, 4.0):
            c = kernel_case(pair, seconds, a.iters, a.repeats)
            kernels.append(c)
            print(json.dumps(c), flush=True)
    if a.kernels_only:
        with open(a.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), kernels=kernels), f, indent=1)
        return
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "spex_causal.wsw")
    export_engine(get_model("ConvTasNet")(**SHAPE), path)
    eng = E.Engine(path)
    streams, ms = [], 10
    pushes = max(8, int(a.seconds * 1000 / ms))
    for rows in map(int, a.rows.split(",")):
        for block_kernel in (False, True):
            arms = (16000, 8000, 48000)
            runs = {r: [] for r in arms}
            for _ in range(a.repeats):                                   # the arms alternate: drift hits them alike
                for r in arms:
                    runs[r].append(stream_arm(eng, rows, r, ms, pushes, block_kernel))
            for r in arms:
                wall = [x["wall_ms"] for x in runs[r]]
                c = dict(rows=rows, rate=r, packet_samples=r * ms // 1000, block_kernel=block_kernel, pushes=pushes, wall_ms_runs=wall,
                         wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall),
                         launches_per_push=runs[r][0]["launches"], state_bytes=runs[r][0]["state_bytes"])
                streams.append(c)
                print(json.dumps(c), flush=True)
    eng.close()
    os.remove(path)
    os.rmdir(tmp)
    name = torch.cuda.get_device_name(0)
    lines = ["# The device resampler: kernel time, and a rate-stream push against a plain push", "",
             f"Written by `tools/bench_resample.py` on {name}; JSON beside this file.  Nothing here is a gate.", "",
             f"## `ws_resample_fwd`, one row: time per call through the Python binding, HIP events around {a.iters} back-to-back calls, "
             f"{a.repeats} runs (median, min – max)", "",
             "bytes = input once + output once + the tap table once (what a call must move at least); MAC = n_out K.", "",
             "| pair | U | D | K | taps | table bytes | audio | n_in | n_out | µs / call (median) | min – max | bytes | GB/s | GMAC/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in kernels:
        lines.append(f"| {c['rate_in']} → {c['rate_out']} | {c['U']} | {c['D']} | {c['K']} | {c['staging']} | {c['taps_bytes']} | "
                     f"{c['seconds'] * 1e3:g} ms | {c['n_in']} | {c['n_out']} | {c['us_median']:.2f} | {c['us_min']:.2f} – {c['us_max']:.2f} | "
                     f"{c['bytes_min']} | {c['gb_per_s']:.2f} | {c['mac_per_call'] / c['us_median'] / 1e3:.2f} |")
    lines += ["", f"## A push of 10 ms: the plain stream (16 kHz) and the rate stream (8 kHz, 48 kHz), SpEx+ shape, {a.seconds:g} s of audio "
              f"per run after {WARMUP} warm-up pushes, {a.repeats} runs per arm, alternating", "",
              "| rows | block kernel | rate | packet | wall ms / push (median) | min – max | over the plain push | launches / push | state bytes |",
              "|---|---|---|---|---|---|---|---|---|"]
    by = {(c["rows"], c["block_kernel"], c["rate"]): c for c in streams}
    for c in streams:
        base = by[(c["rows"], c["block_kernel"], 16000)]
        lines.append(f"| {c['rows']} | {'yes' if c['block_kernel'] else 'no'} | {c['rate']} | {c['packet_samples']} | {c['wall_ms_median']:.3f} | "
                     f"{c['wall_ms_min']:.3f} – {c['wall_ms_max']:.3f} | {c['wall_ms_median'] - base['wall_ms_median']:+.3f} ms | "
                     f"{c['launches_per_push']:.0f} | {c['state_bytes']} |")
    lines += ["", "<!-- notes -->"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=name, shape=SHAPE, max_chunk_frames=G, warmup_pushes=WARMUP, kernels=kernels, streams=streams), f, indent=1)
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
