"""N live calls on one engine: a stream-pool round against N serial pushes on N solo streams.

    python tools/bench_stream_pool.py --out profiles/stream_pool.json --md profiles/stream_pool.md

Shape of profiles/engine_stream.md (N 256, L 20, B 256, H 512, P 3, X 8, R 4, cLN, causal, Multi ends, concatConv, fixed
embedding), 10 ms packets at 16 kHz, max_chunk_frames 256 in both arms (a round is one group of frames).  For N in
{1, 2, 4, 8, 16}, two arms, run alternately in one process, --repeats times each (default 3), so that the spread is known:
  * pool    one ws_engine_pool_push that carries one packet for each of N slots: one launch chain, one synchronisation;
  * serial  N ws_engine_stream_push calls on N solo streams of one row, one after another -- the only arrangement there
            was for unsynchronised calls before the pool: N launch chains, N synchronisations.
Per run: wall ms per ROUND (every call gets its next packet), the host clock around the calls, each of which synchronises
itself; launches per round; the carried state in bytes (pool: one allocation; serial: N streams' allocations).  Also one
UNEQUAL round at N = 8: one slot delivers 250 ms while seven deliver 10 ms -- the rectangle is [8][400] for 7 x 16 + 400
valid frames, the price of one rectangle -- against the same packets pushed serially.  The --md file is rewritten up to the
line `<!-- notes -->`; what follows it is kept.  Needs a GPU.  Nothing here is a gate."""
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
SHAPE = dict(N=256, L=20, B=256, H=512, P=3, X=8, R=4, norm="cLN", causal=True, spk_emb_dim=256, joint_training=False)
G = 256
WARMUP = 20


def _data(n_calls, n, rounds, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_calls, (WARMUP + rounds) * n)).astype(np.float32)
    emb = rng.standard_normal((n_calls, 256)).astype(np.float32)
    return x, emb


def pool_arm(eng, n_calls, n, rounds):
    from wesep_amd import engine as E
    x, emb = _data(n_calls, n, rounds, n_calls * 1000 + n)
    pool = eng.stream_pool(n_calls, max_chunk_frames=G)
    state = eng.info("stream_state_bytes")
    slots = [pool.attach(emb[i], E.ENROLL_EMBEDDING) for i in range(n_calls)]
    packets = [{s: np.ascontiguousarray(x[i, r * n:(r + 1) * n]) for i, s in enumerate(slots)} for r in range(WARMUP + rounds)]
    for p in packets[:WARMUP]:
        pool.push(p)
    launches = set()
    t0 = time.perf_counter()
    for p in packets[WARMUP:]:
        pool.push(p)
        launches.add(eng.info("n_launches"))
    wall_ms = (time.perf_counter() - t0) * 1e3 / rounds
    pool.close()
    return dict(wall_ms=wall_ms, launches=max(launches), state_bytes=state)


def serial_arm(eng, n_calls, n, rounds):
    from wesep_amd import engine as E
    x, emb = _data(n_calls, n, rounds, n_calls * 1000 + n)
    streams, state = [], 0
    for i in range(n_calls):
        streams.append(eng.stream(1, emb[i:i + 1], E.ENROLL_EMBEDDING, max_chunk_frames=G))
        state += eng.info("stream_state_bytes")
    packets = [[np.ascontiguousarray(x[i:i + 1, r * n:(r + 1) * n]) for i in range(n_calls)] for r in range(WARMUP + rounds)]
    for p in packets[:WARMUP]:
        for st, c in zip(streams, p):
            st.push(c)
    launches = set()
    t0 = time.perf_counter()
    for p in packets[WARMUP:]:
        k = 0
        for st, c in zip(streams, p):
            st.push(c)
            k += eng.info("n_launches")
        launches.add(k)
    wall_ms = (time.perf_counter() - t0) * 1e3 / rounds
    for st in streams:
        st.close()
    return dict(wall_ms=wall_ms, launches=max(launches), state_bytes=state)


def unequal_round(eng, arm, n_calls, long_n, n, rounds):
    """ms of ONE round in which call 0 delivers long_n samples and the others n, after a warm-up of equal rounds"""
    from wesep_amd import engine as E
    x, emb = _data(n_calls, n, rounds, 77)
    rng = np.random.default_rng(5)
    long_x = rng.standard_normal(long_n).astype(np.float32)
    times, launches = [], 0
    for _ in range(rounds):
        if arm == "pool":
            pool = eng.stream_pool(n_calls, max_chunk_frames=long_n // 10 + 16)
            slots = [pool.attach(emb[i], E.ENROLL_EMBEDDING) for i in range(n_calls)]
            for r in range(WARMUP):
                pool.push({s: np.ascontiguousarray(x[i, r * n:(r + 1) * n]) for i, s in enumerate(slots)})
            p = {s: (long_x if i == 0 else np.ascontiguousarray(x[i, WARMUP * n:(WARMUP + 1) * n])) for i, s in enumerate(slots)}
            t0 = time.perf_counter()
            pool.push(p)
            times.append((time.perf_counter() - t0) * 1e3)
            launches = eng.info("n_launches")
            pool.close()
        else:
            streams = [eng.stream(1, emb[i:i + 1], E.ENROLL_EMBEDDING, max_chunk_frames=long_n // 10 + 16) for i in range(n_calls)]
            for r in range(WARMUP):
                for i, st in enumerate(streams):
                    st.push(np.ascontiguousarray(x[i:i + 1, r * n:(r + 1) * n]))
            p = [long_x[None] if i == 0 else np.ascontiguousarray(x[i:i + 1, WARMUP * n:(WARMUP + 1) * n]) for i in range(n_calls)]
            launches = 0
            t0 = time.perf_counter()
            for st, c in zip(streams, p):
                st.push(c)
                launches += eng.info("n_launches")
            times.append((time.perf_counter() - t0) * 1e3)
            for st in streams:
                st.close()
    return dict(ms_runs=times, ms_median=statistics.median(times), ms_min=min(times), ms_max=max(times), launches=launches)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--calls", default="1,2,4,8,16")
    ap.add_argument("--seconds", type=float, default=2.0, help="audio per call and run")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_pool: needs a GPU (no CPU measurement exists)")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    torch.manual_seed(0)
    model = get_model("ConvTasNet")(**SHAPE)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "spex_causal.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    n = SR * 10 // 1000
    rounds = max(8, int(a.seconds * 100))
    cases = []
    for n_calls in map(int, a.calls.split(",")):
        runs = {"pool": [], "serial": []}
        for _ in range(a.repeats):                                       # the arms alternate: drift hits them alike
            runs["pool"].append(pool_arm(eng, n_calls, n, rounds))
            runs["serial"].append(serial_arm(eng, n_calls, n, rounds))
        for arm in ("pool", "serial"):
            wall = [r["wall_ms"] for r in runs[arm]]
            c = dict(calls=n_calls, arm=arm, rounds=rounds, wall_ms_runs=wall, wall_ms_median=statistics.median(wall),
                     wall_ms_min=min(wall), wall_ms_max=max(wall), launches_per_round=runs[arm][0]["launches"],
                     state_bytes=runs[arm][0]["state_bytes"])
            cases.append(c)
            print(json.dumps(c), flush=True)
    unequal = {arm: unequal_round(eng, arm, 8, 4000, n, max(a.repeats, 3)) for arm in ("pool", "serial")}
    print(json.dumps(unequal), flush=True)
    eng.close()
    os.remove(path)
    os.rmdir(tmp)
    by = {(c["calls"], c["arm"]): c for c in cases}
    lines = ["# Stream pool: one round of N live calls against N serial pushes", "",
             f"Written by `tools/bench_stream_pool.py` on {torch.cuda.get_device_name(0)}; JSON beside this file.  SpEx+ shape "
             f"(N 256, L 20, B 256, H 512, P 3, X 8, R 4, cLN, causal, Multi ends, concatConv), fixed embeddings, 16 kHz, 10 ms "
             f"packets, {rounds} rounds per run after {WARMUP} warm-up rounds, `max_chunk_frames` {G}, {a.repeats} runs per arm, "
             f"alternating in one process (median, and min – max as the spread).  A round gives every call its next packet: "
             f"`pool` is one `ws_engine_pool_push`, `serial` is N `ws_engine_stream_push` calls on N solo streams of one row -- "
             f"the arrangement there was before the pool.  wall = host clock around the calls, each of which synchronises "
             f"itself.  Nothing here is a gate.", "",
             "| calls | arm | wall ms / round (median) | wall min – max | launches / round | round / packet (wall) | state bytes |",
             "|---|---|---|---|---|---|---|"]
    for c in cases:
        lines.append(f"| {c['calls']} | {c['arm']} | {c['wall_ms_median']:.3f} | {c['wall_ms_min']:.3f} – {c['wall_ms_max']:.3f} | "
                     f"{c['launches_per_round']} | {c['wall_ms_median'] / 10:.3f} | {c['state_bytes']} |")
    lines += ["", "Pool against serial (\"separated\": the pool's slowest run is faster than the serial arm's fastest run):", ""]
    for n_calls in sorted({c["calls"] for c in cases}):
        p, s = by[(n_calls, "pool")], by[(n_calls, "serial")]
        verdict = (f"separated, {s['wall_ms_median'] / p['wall_ms_median']:.2f}x" if p["wall_ms_max"] < s["wall_ms_min"] else
                   ("overlap" if s["wall_ms_max"] >= p["wall_ms_min"] else
                    f"the pool is SLOWER, {p['wall_ms_median'] / s['wall_ms_median']:.2f}x"))
        lines.append(f"- {n_calls} calls: pool {p['wall_ms_median']:.3f} vs serial {s['wall_ms_median']:.3f} ms a round — {verdict}; "
                     f"the pool round is {p['wall_ms_median'] / by[(1, 'serial')]['wall_ms_median']:.2f} solo pushes"
                     if (1, "serial") in by else
                     f"- {n_calls} calls: pool {p['wall_ms_median']:.3f} vs serial {s['wall_ms_median']:.3f} ms a round — {verdict}")
    up, us = unequal["pool"], unequal["serial"]
    lines += ["", f"One unequal round, 8 calls, one delivers 250 ms (400 frames) and seven deliver 10 ms (16 frames each): the pool "
              f"runs one rectangle [8][400] -- 3200 frame rows for 512 valid ones -- in {up['ms_median']:.3f} ms ({up['ms_min']:.3f} – "
              f"{up['ms_max']:.3f}, {up['launches']} launches); the same packets as 8 serial pushes take {us['ms_median']:.3f} ms "
              f"({us['ms_min']:.3f} – {us['ms_max']:.3f}, {us['launches']} launches).", "", "<!-- notes -->"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(shape=SHAPE, sample_rate=SR, packet_ms=10, max_chunk_frames=G, warmup_rounds=WARMUP,
                       device=torch.cuda.get_device_name(0), cases=cases, unequal_round=unequal), f, indent=1)
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
