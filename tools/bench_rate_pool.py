"""N live calls at mixed sample rates on one engine: a rate-pool round against N serial rate-stream pushes, and the plain
pool's round as the floor.

    python tools/bench_rate_pool.py --out profiles/rate_pool.json --md profiles/rate_pool.md

Shape of profiles/stream_pool.md (N 256, L 20, B 256, H 512, P 3, X 8, R 4, cLN, causal, Multi ends, concatConv, fixed
embedding), 10 ms packets, max_chunk_frames 256 in every arm (a round is one group of frames).  For N in {1, 4, 8, 16}, three
arms, run alternately in ONE process, --repeats times each (default 3), so that the spread is known:
  * rate pool   one ws_engine_rate_pool_push that carries one packet for each of N slots, the slots' rates cycled over
                8 / 16 / 48 kHz (80 / 160 / 480 samples): one launch chain, one synchronisation;
  * serial      the same packets as N ws_engine_rate_stream_push calls on N solo rate streams of one row -- the path such
                calls take without the rate pool: N launch chains, N synchronisations;
  * plain pool  one ws_engine_pool_push of N calls at 16 kHz: the floor -- the difference to the rate pool is what the
                resampler and copy launches cost.
Per run: wall ms per ROUND (every call gets its next packet), the host clock around the calls, each of which synchronises
itself; launches per round; the carried state in bytes.  The --md file is rewritten up to the line `<!-- notes -->`; what
follows it is kept.  Needs a GPU.  Nothing here is a gate."""
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

SR = 16000
RATES = (8000, 16000, 48000)
SHAPE = dict(N=256, L=20, B=256, H=512, P=3, X=8, R=4, norm="cLN", causal=True, spk_emb_dim=256, joint_training=False)
G = 256
WARMUP = 20


def _data(n_calls, rounds, seed, rates):
    rng = np.random.default_rng(seed)
    x = [(0.1 * rng.standard_normal((WARMUP + rounds) * (r // 100))).astype(np.float32) for r in rates]
    emb = rng.standard_normal((n_calls, 256)).astype(np.float32)
    return x, emb


def _timed_rounds(eng, push, packets, rounds):
    for p in packets[:WARMUP]:
        push(p)
    launches = set()
    t0 = time.perf_counter()
    for p in packets[WARMUP:]:
        launches.add(push(p))
    return (time.perf_counter() - t0) * 1e3 / rounds, max(launches)


def rate_pool_arm(eng, n_calls, rounds):
    from wesep_amd import engine as E
    rates = [RATES[i % len(RATES)] for i in range(n_calls)]
    x, emb = _data(n_calls, rounds, n_calls * 1000, rates)
    pool = eng.rate_pool(n_calls, [8000, 48000], max_chunk_frames=G, max_push=480)
    state = eng.info("stream_state_bytes")
    slots = [pool.attach(emb[i], E.ENROLL_EMBEDDING, rates[i]) for i in range(n_calls)]
    packets = [{s: np.ascontiguousarray(x[i][r * (rates[i] // 100):(r + 1) * (rates[i] // 100)]) for i, s in enumerate(slots)}
               for r in range(WARMUP + rounds)]

    def push(p):
        pool.push(p)
        return eng.info("n_launches")
    wall_ms, launches = _timed_rounds(eng, push, packets, rounds)
    pool.close()
    return dict(wall_ms=wall_ms, launches=launches, state_bytes=state)


def serial_arm(eng, n_calls, rounds):
    from wesep_amd import engine as E
    rates = [RATES[i % len(RATES)] for i in range(n_calls)]
    x, emb = _data(n_calls, rounds, n_calls * 1000, rates)
    streams, state = [], 0
    for i in range(n_calls):
        streams.append(eng.rate_stream(1, emb[i:i + 1], E.ENROLL_EMBEDDING, rates[i], max_chunk_frames=G, max_push=480))
        state += eng.info("stream_state_bytes")
    packets = [[np.ascontiguousarray(x[i][None, r * (rates[i] // 100):(r + 1) * (rates[i] // 100)]) for i in range(n_calls)]
               for r in range(WARMUP + rounds)]

    def push(p):
        k = 0
        for st, c in zip(streams, p):
            st.push(c)
            k += eng.info("n_launches")
        return k
    wall_ms, launches = _timed_rounds(eng, push, packets, rounds)
    for st in streams:
        st.close()
    return dict(wall_ms=wall_ms, launches=launches, state_bytes=state)


def plain_pool_arm(eng, n_calls, rounds):
    from wesep_amd import engine as E
    x, emb = _data(n_calls, rounds, n_calls * 1000, [SR] * n_calls)
    pool = eng.stream_pool(n_calls, max_chunk_frames=G)
    state = eng.info("stream_state_bytes")
    slots = [pool.attach(emb[i], E.ENROLL_EMBEDDING) for i in range(n_calls)]
    packets = [{s: np.ascontiguousarray(x[i][r * 160:(r + 1) * 160]) for i, s in enumerate(slots)} for r in range(WARMUP + rounds)]

    def push(p):
        pool.push(p)
        return eng.info("n_launches")
    wall_ms, launches = _timed_rounds(eng, push, packets, rounds)
    pool.close()
    return dict(wall_ms=wall_ms, launches=launches, state_bytes=state)


ARMS = {"rate pool": rate_pool_arm, "serial": serial_arm, "plain pool": plain_pool_arm}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--calls", default="1,4,8,16")
    ap.add_argument("--seconds", type=float, default=2.0, help="audio per call and run")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rate_pool: needs a GPU (no CPU measurement exists)")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    torch.manual_seed(0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "spex_causal.wsw")
    export_engine(get_model("ConvTasNet")(**SHAPE), path)
    eng = E.Engine(path)
    rounds = max(8, int(a.seconds * 100))
    cases = []
    for n_calls in map(int, a.calls.split(",")):
        runs = {arm: [] for arm in ARMS}
        for _ in range(a.repeats):                                       # the arms alternate: drift hits them alike
            for arm, fn in ARMS.items():
                runs[arm].append(fn(eng, n_calls, rounds))
        for arm in ARMS:
            wall = [r["wall_ms"] for r in runs[arm]]
            c = dict(calls=n_calls, arm=arm, rates=[RATES[i % len(RATES)] if arm != "plain pool" else SR for i in range(n_calls)], rounds=rounds,
                     wall_ms_runs=wall, wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall),
                     launches_per_round=runs[arm][0]["launches"], state_bytes=runs[arm][0]["state_bytes"])
            cases.append(c)
            print(json.dumps(c), flush=True)
    eng.close()
    os.remove(path)
    os.rmdir(tmp)
    by = {(c["calls"], c["arm"]): c for c in cases}
    name = torch.cuda.get_device_name(0)
    lines = ["# Rate pool: one round of N live calls at 8 / 16 / 48 kHz against N serial rate-stream pushes", "",
             f"Written by `tools/bench_rate_pool.py` on {name}; JSON beside this file.  SpEx+ shape (N 256, L 20, B 256, H 512, P 3, X 8, "
             f"R 4, cLN, causal, Multi ends, concatConv), fixed embeddings, 10 ms packets, the calls' rates cycled over 8 / 16 / 48 kHz, "
             f"{rounds} rounds per run after {WARMUP} warm-up rounds, `max_chunk_frames` {G}, `max_push` 480, {a.repeats} runs per arm, "
             f"alternating in one process (median, and min – max as the spread).  `rate pool` is one `ws_engine_rate_pool_push`, `serial` "
             f"is N `ws_engine_rate_stream_push` calls on N solo rate streams of one row, `plain pool` is one `ws_engine_pool_push` of N "
             f"calls at 16 kHz (the floor).  wall = host clock around the calls, each of which synchronises itself.  Nothing here is a "
             f"gate.", "",
             "| calls | arm | wall ms / round (median) | wall min – max | launches / round | state bytes |",
             "|---|---|---|---|---|---|"]
    for c in cases:
        lines.append(f"| {c['calls']} | {c['arm']} | {c['wall_ms_median']:.3f} | {c['wall_ms_min']:.3f} – {c['wall_ms_max']:.3f} | "
                     f"{c['launches_per_round']} | {c['state_bytes']} |")
    lines += ["", "Rate pool against serial (\"separated\": the pool's slowest run is faster than the serial arm's fastest run), and over the "
              "plain pool's round:", ""]
    for n_calls in sorted({c["calls"] for c in cases}):
        p, s, f = by[(n_calls, "rate pool")], by[(n_calls, "serial")], by[(n_calls, "plain pool")]
        verdict = (f"separated, {s['wall_ms_median'] / p['wall_ms_median']:.2f}x" if p["wall_ms_max"] < s["wall_ms_min"] else
                   ("overlap" if s["wall_ms_max"] >= p["wall_ms_min"] else
                    f"the rate pool is SLOWER, {p['wall_ms_median'] / s['wall_ms_median']:.2f}x"))
        lines.append(f"- {n_calls} calls: rate pool {p['wall_ms_median']:.3f} vs serial {s['wall_ms_median']:.3f} ms a round — {verdict}; "
                     f"{p['wall_ms_median'] - f['wall_ms_median']:+.3f} ms over the plain pool's {f['wall_ms_median']:.3f} "
                     f"({p['launches_per_round'] - f['launches_per_round']:+d} launches)")
    lines += ["", "<!-- notes -->"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(shape=SHAPE, sample_rate=SR, rates=RATES, packet_ms=10, max_chunk_frames=G, max_push=480, warmup_rounds=WARMUP,
                       device=name, cases=cases), f, indent=1)
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
