"""Tail pool (ws_engine_tail_pool_*): N staggered live recordings ticked through one pool against N one-slot pools, the four
architectures at their recipe geometries: time per tick, forwards per tick, the GPU share of a tick period, state.

    python tools/bench_tail.py --out profiles/tail.json --md profiles/tail.md

pBSRNN (6 repeats), Conv-TasNet / SpEx+ (N 256), DPCCN and TF-GridNet (6 blocks) as their constructors build them, fixed
embeddings, K = 2 targets, 16 kHz, window S = 4 s, fade 20 ms, warm S / 2, max_rows 8, N in {1, 4, 8} recordings in packets of
100 ms with a tick every 500 ms.  Recording i starts 3 i packets late -- 300 ms, no multiple of the tick -- so no two recordings
are aligned.  A *step* gives every recording in flight its next packet (no launch); every fifth step ticks them all: ONE tick of
the pool, or one tick per one-slot pool, one after another.  A tick's time is the host clock around it (it synchronises
itself).  *steady* ticks are those in which every firing slot ran a full window; the others hold slots in warm-up, whose rows
run in forwards of their own.  After one warm-up run per arm, `--repeats` runs per arm, alternating: median and min - max.  The
--md file is rewritten up to the line `<!-- notes -->`; what follows it is kept.  Needs a GPU.  Nothing here is a gate."""
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


def run(eng, E, mixes, embs, S, C, warm, max_rows, packet, every, stagger, pooled):
    """-> dict(steady [ms], warmup [ms], total ms, shapes {(forwards, rows, launches)}, state bytes)"""
    N, n, K = len(mixes), len(mixes[0]), embs[0].shape[0]
    pools = [eng.tail_pool(N, K, S, C, warm, max_rows)] if pooled else [eng.tail_pool(1, K, S, C, warm, max_rows) for _ in range(N)]
    state = eng.info("tail_pool_state_bytes") * len(pools)
    where = [(pools[0], pools[0].attach(embs[i], E.ENROLL_EMBEDDING)) if pooled else (pools[i], pools[i].attach(embs[i], E.ENROLL_EMBEDDING))
             for i in range(N)]
    pos, steady, warmup, shapes = [0] * N, [], [], set()
    t_all, t = time.perf_counter(), 0
    while any(p < n for p in pos):
        live = [i for i in range(N) if t >= stagger * i and pos[i] < n]
        for pool in pools:
            chunk = {where[i][1]: mixes[i][pos[i]:pos[i] + packet] for i in live if where[i][0] is pool}
            if chunk:
                pool.push(chunk)
        for i in live:
            pos[i] = min(n, pos[i] + packet)
        if live and (t + 1) % every == 0:
            full = all(pos[i] >= S for i in live)
            t0 = time.perf_counter()
            fw = rows = launches = 0
            for pool in pools:
                named = [where[i][1] for i in live if where[i][0] is pool]
                if named:
                    pool.tick(named)
                    fw, rows, launches = fw + eng.info("tail_pool_forwards"), rows + eng.info("tail_pool_rows"), launches + eng.info("n_launches")
            if rows:
                (steady if full else warmup).append((time.perf_counter() - t0) * 1e3)
                if full and len(live) == N:
                    shapes.add((fw, rows, launches))
        for i in live:
            if pos[i] >= n:
                where[i][0].flush(where[i][1])
        t += 1
    total = (time.perf_counter() - t_all) * 1e3
    for pool in pools:
        pool.close()
    return dict(steady=steady, warmup=warmup, total=total, shapes=sorted(shapes), state=state)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--archs", default=",".join(MODELS))
    ap.add_argument("--counts", default="1,4,8", help="recordings in flight")
    ap.add_argument("--packet_ms", type=int, default=100)
    ap.add_argument("--tick_ms", type=int, default=500)
    ap.add_argument("--fade_ms", type=int, default=20)
    ap.add_argument("--seconds", type=float, default=20.0, help="every recording")
    ap.add_argument("--window", type=float, default=4.0)
    ap.add_argument("--max_rows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tail: needs a GPU (no CPU measurement exists)")
    if a.tick_ms % a.packet_ms:
        raise SystemExit("bench_tail: the tick period is a whole number of packets")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    S, C, n, K = int(a.window * SR), SR * a.fade_ms // 1000, int(a.seconds * SR), 2
    packet, every, counts = SR * a.packet_ms // 1000, a.tick_ms // a.packet_ms, [int(c) for c in a.counts.split(",")]
    rng = np.random.default_rng(0)
    mixes = [(0.1 * rng.standard_normal(n)).astype(np.float32) for _ in range(max(counts))]
    embs = [rng.standard_normal((K, 256)).astype(np.float32) for _ in range(max(counts))]
    tmp = tempfile.mkdtemp()
    cases = []
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for arch in a.archs.split(","):
        name, kw = MODELS[arch]
        torch.manual_seed(0)
        path = os.path.join(tmp, f"{arch}.wsw")
        export_engine(get_model(name)(joint_training=False, **kw), path)
        eng = E.Engine(path)
        for N in counts:
            mx, em = mixes[:N], embs[:N]
            args = (S, C, S // 2, a.max_rows, packet, every, 3)
            short = [x[:S + 2 * every * packet + 3 * N * packet] for x in mx]     # every shape of the timed runs
            for pooled in (True, False):
                run(eng, E, short, em, *args, pooled)
            runs = {True: [], False: []}
            for _ in range(a.repeats):                                            # the arms alternate: drift hits them alike
                for pooled in (True, False):
                    runs[pooled].append(run(eng, E, mx, em, *args, pooled))
            for pooled, rs in runs.items():
                med = [statistics.median(r["steady"]) for r in rs]
                c = dict(arch=arch, N=N, path="pool" if pooled else "one-slot pools", steady_ticks=len(rs[0]["steady"]),
                         warmup_ticks=len(rs[0]["warmup"]), tick_ms=statistics.median(med), tick_ms_runs=med,
                         tick_worst_ms=max(max(r["steady"]) for r in rs),
                         warmup_tick_ms=statistics.median(statistics.median(r["warmup"]) for r in rs) if rs[0]["warmup"] else None,
                         gpu_share=statistics.median(med) / a.tick_ms, total_ms=statistics.median(r["total"] for r in rs),
                         state_bytes=rs[0]["state"], shapes=rs[0]["shapes"])
                cases.append(c)
                print(json.dumps(c), flush=True)
            with open(a.out, "w") as f:                                           # what is measured so far
                json.dump(dict(partial=True, cases=cases), f, indent=1)
        eng.close()
        os.remove(path)
    os.rmdir(tmp)
    lines = ["# Tail pool: N staggered live recordings ticked through one pool against N one-slot pools", "",
             f"Written by `tools/bench_tail.py` on {torch.cuda.get_device_name(0)}; JSON beside this file.  Recipe geometries, fixed "
             f"embeddings, K = 2 targets, 16 kHz, window {a.window:g} s, fade {a.fade_ms} ms, warm {a.window / 2:g} s, max_rows "
             f"{a.max_rows}, N recordings of {a.seconds:g} s in packets of {a.packet_ms} ms, a tick every {a.tick_ms} ms, recording i "
             f"started 3 i packets late (no multiple of the tick), {a.repeats} runs per arm after a warm-up run per arm (median; "
             f"min – max).  A tick names every recording in flight: ONE tick of the pool, or one tick per one-slot pool, one after "
             f"another.  wall = host clock around the tick; it synchronises itself.  *steady*: every firing slot ran a full "
             f"window.  GPU share = steady tick time / tick period: the part of real time the device spends on these N "
             f"recordings.  The arms alternate in the same run.  Nothing here is a gate.", "",
             "| model | N | path | steady ticks | ms / steady tick (median; min – max; worst) | GPU share | ms / warm-up tick | "
             "forwards, rows, launches / steady tick of all N | total ms | state bytes |", "|---|---|---|---|---|---|---|---|---|---|"]
    for c in cases:
        wu = "—" if c["warmup_tick_ms"] is None else f"{c['warmup_tick_ms']:.2f}"
        shapes = "—" if not c["shapes"] else "; ".join(f"{f}, {r}, {l}" for f, r, l in c["shapes"])
        lines.append(f"| {c['arch']} | {c['N']} | {c['path']} | {c['steady_ticks']} | {c['tick_ms']:.2f} ({min(c['tick_ms_runs']):.2f} – "
                     f"{max(c['tick_ms_runs']):.2f}; {c['tick_worst_ms']:.2f}) | {c['gpu_share']:.3f} | {wu} | {shapes} | "
                     f"{c['total_ms']:.1f} | {c['state_bytes']} |")
    lines += ["", "<!-- notes -->"]
    with open(a.out, "w") as f:
        json.dump(dict(sample_rate=SR, window_s=a.window, fade_ms=a.fade_ms, tick_ms=a.tick_ms, seconds=a.seconds, max_rows=a.max_rows,
                       packet_ms=a.packet_ms, repeats=a.repeats, device=torch.cuda.get_device_name(0), cases=cases), f, indent=1)
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
