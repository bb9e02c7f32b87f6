"""Live pool (ws_engine_live_pool_*) against N solo live handles (ws_engine_live_*), the four architectures at their recipe
geometries: time per window-completing push, total, rounds and forwards per push, state.

    python tools/bench_live_pool.py --out profiles/live_pool.json --md profiles/live_pool.md

pBSRNN (6 repeats), Conv-TasNet / SpEx+ (N 256), DPCCN and TF-GridNet (6 blocks) as their constructors build them, fixed
embeddings, K = 2 targets, 16 kHz, window S = 4 s, overlap O = 1 s (hop 3 s), max_rows 8, N in {1, 4, 8} recordings of 60 s in
packets of 100 ms.  Two feeds:
  aligned    every recording starts at push 0: every window-completing push carries N windows;
  staggered  recording i starts 2 i pushes late (more than a packet, no multiple of the hop): no two windows complete in one push.
Each feed runs through one pool (one push per step for every recording in flight) and through N solo handles (one push per
recording per step, one after another) in the same run, alternating; a step's time is the host clock around its push or
pushes, which synchronise themselves when a window became complete.  After one warm-up of 12 s per arm (every shape of the
timed runs has then run), `--repeats` runs per arm: median and min - max.  `--hold_ms W` adds a third pool arm, hold /
staggered: the staggered feed through ws_engine_live_pool_store, with ONE ws_engine_live_pool_run of every slot with a complete
window once every recording has one waiting or ws_engine_live_pool_due reports that the oldest has waited W ms of audio;
recordings that end are final in the next run.  A completing step of that arm is a step whose run launched; the added latency
is the largest age met at a run, in samples.  `--skip_solo` leaves the solo handles out (the pool arms are the yardsticks of
the hold arm).  The outputs of the aligned pool are compared with
ws_engine_separate_long per recording.  The --md file is rewritten up to the line `<!-- notes -->`; what follows it is kept.
Needs a GPU.  Nothing here is a gate."""
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


def feed(N, n, packet, stagger, push_step, finish):
    """Drives N recordings of n samples: at step t recording i (started at step stagger * i) gives its next packet.
    push_step({i: (pos, len)}) -> True when a window became complete; finish(i) ends recording i.  -> (ms of the steps that
    completed a window, ms of the others, total ms)"""
    pos = [0] * N
    hit, miss = [], []
    t_all = time.perf_counter()
    t = 0
    while any(p < n for p in pos):
        part = {i: (pos[i], min(packet, n - pos[i])) for i in range(N) if t >= stagger * i and pos[i] < n}
        if part:
            t0 = time.perf_counter()
            done = push_step(part)
            (hit if done else miss).append((time.perf_counter() - t0) * 1e3)
            for i, (p, c) in part.items():
                pos[i] = p + c
                if pos[i] >= n:
                    finish(i)
        t += 1
    return hit, miss, (time.perf_counter() - t_all) * 1e3


def pool_run(eng, E, mixes, embs, S, O, max_rows, packet, stagger, keep=False):
    N, n = len(mixes), len(mixes[0])
    pool = eng.live_pool(N, 2, S, O, max_rows)
    state = eng.info("live_pool_state_bytes")
    slots = [pool.attach(embs[i], E.ENROLL_EMBEDDING) for i in range(N)]
    shape, parts = set(), {i: [] for i in range(N)}

    def push_step(part):
        got = pool.push({slots[i]: mixes[i][p:p + c] for i, (p, c) in part.items()})
        r = eng.info("live_pool_rounds")
        if r:
            shape.add((r, eng.info("live_pool_forwards"), eng.info("n_launches")))
        if keep:
            for i in part:
                parts[i].append(got[slots[i]])
        return r > 0

    def finish(i):
        tail = pool.flush(slots[i])
        if keep:
            parts[i].append(tail)

    hit, miss, total = feed(N, n, packet, stagger, push_step, finish)
    pool.close()
    out = [np.concatenate(parts[i], axis=1) for i in range(N)] if keep else None
    return dict(hit=hit, miss=miss, total=total, shape=sorted(shape), state=state), out


def hold_run(eng, E, mixes, embs, S, O, max_rows, packet, stagger, hold_n):
    """the staggered feed stored, the windows run on a hold of hold_n samples"""
    N, n = len(mixes), len(mixes[0])
    pool = eng.live_pool(N, 2, S, O, max_rows)
    state = eng.info("live_pool_state_bytes")
    slots = [pool.attach(embs[i], E.ENROLL_EMBEDDING) for i in range(N)]
    shape, ending, ages = set(), [], []

    def run():
        final = [slots[i] for i in ending]
        del ending[:]
        pool.run(final=final)
        r = eng.info("live_pool_rounds")
        if r:
            shape.add((r, eng.info("live_pool_forwards"), eng.info("n_launches")))
        return r > 0

    def push_step(part):
        pool.store({slots[i]: mixes[i][p:p + c] for i, (p, c) in part.items()})
        rows, age = pool.due()
        if rows >= 2 * N or (rows > 0 and age >= hold_n):
            ages.append(age)
            return run()
        return False

    hit, miss, total = feed(N, n, packet, stagger, push_step, ending.append)
    if ending:                                                    # the recordings that ended after the last run
        t0 = time.perf_counter()
        run()
        total += (time.perf_counter() - t0) * 1e3
    pool.close()
    return dict(hit=hit, miss=miss, total=total, shape=sorted(shape), state=state, age_max=max(ages) if ages else 0)


def solo_run(eng, E, mixes, embs, S, O, max_rows, packet, stagger):
    N, n = len(mixes), len(mixes[0])
    lvs = [eng.live(embs[i], E.ENROLL_EMBEDDING, S, O, max_rows) for i in range(N)]
    state = eng.info("live_state_bytes")

    def push_step(part):
        done = False
        for i, (p, c) in part.items():
            lvs[i].push(mixes[i][p:p + c])
            done = done or eng.info("live_groups") > 0
        return done

    hit, miss, total = feed(N, n, packet, stagger, push_step, lambda i: lvs[i].flush())
    for lv in lvs:
        lv.close()
    return dict(hit=hit, miss=miss, total=total, state=N * state)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--archs", default=",".join(MODELS))
    ap.add_argument("--counts", default="1,4,8", help="recordings in flight")
    ap.add_argument("--packet_ms", type=int, default=100)
    ap.add_argument("--seconds", type=float, default=60.0, help="every recording")
    ap.add_argument("--window", type=float, default=4.0)
    ap.add_argument("--overlap", type=float, default=1.0)
    ap.add_argument("--max_rows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--hold_ms", type=float, default=None, help="adds the arm hold / staggered: store, then run on a hold of this many ms")
    ap.add_argument("--skip_solo", action="store_true", help="leave the solo handles out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_live_pool: needs a GPU (no CPU measurement exists)")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    S, O, n, K = int(a.window * SR), int(a.overlap * SR), int(a.seconds * SR), 2
    packet, counts = SR * a.packet_ms // 1000, [int(c) for c in a.counts.split(",")]
    hold_n = None if a.hold_ms is None else int(a.hold_ms * SR / 1000 + 0.5)
    windows = 1 + (n - S) // (S - O)                                              # regular windows per recording (the last one ends it)
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
        refs = {}
        for N in counts:
            mx, em = mixes[:N], embs[:N]
            arms = {("pool", "aligned"): 0, ("solo", "aligned"): 0, ("pool", "staggered"): 2, ("solo", "staggered"): 2}
            if a.skip_solo:
                arms = {k: v for k, v in arms.items() if k[0] != "solo"}
            if hold_n is not None:
                arms[("hold", "staggered")] = 2

            def one(kind, data, st):
                if kind == "pool":
                    return pool_run(eng, E, data, em, S, O, a.max_rows, packet, st)[0]
                if kind == "hold":
                    return hold_run(eng, E, data, em, S, O, a.max_rows, packet, st, hold_n)
                return solo_run(eng, E, data, em, S, O, a.max_rows, packet, st)

            warm = [x[:3 * S] for x in mx]                                        # three windows: every shape of the timed runs
            for (kind, _), st in arms.items():
                one(kind, warm, st)
            runs = {k: [] for k in arms}
            for _ in range(a.repeats):                                            # the arms alternate: drift hits them alike
                for (kind, fd), st in arms.items():
                    runs[(kind, fd)].append(one(kind, mx, st))
            # the aligned pool's outputs against ws_engine_separate_long, per recording
            _, got = pool_run(eng, E, mx, em, S, O, a.max_rows, packet, 0, keep=True)
            rel = 0.0
            for i in range(N):
                if i not in refs:
                    refs[i] = eng.separate_long(mx[i], em[i], E.ENROLL_EMBEDDING, S, O, a.max_rows).astype(np.float64)
                rel = max(rel, float(np.linalg.norm(got[i].astype(np.float64) - refs[i]) / np.linalg.norm(refs[i])))
            for (kind, fd), rs in runs.items():
                hits = [statistics.median(r["hit"]) for r in rs]
                c = dict(arch=arch, N=N, feed=fd, path=kind, steps_completing=len(rs[0]["hit"]), steps_other=len(rs[0]["miss"]),
                         hit_ms=statistics.median(hits), hit_ms_runs=hits, hit_worst_ms=max(max(r["hit"]) for r in rs),
                         miss_ms=statistics.median(statistics.median(r["miss"]) for r in rs) if rs[0]["miss"] else None,
                         total_ms=statistics.median(r["total"] for r in rs), total_ms_runs=[r["total"] for r in rs],
                         state_bytes=rs[0]["state"], shapes=rs[0].get("shape"), rel_vs_long=rel if (kind, fd) == ("pool", "aligned") else None,
                         windows_per_step=N * windows / len(rs[0]["hit"]), hold_samples=hold_n if kind == "hold" else None,
                         age_max_samples=max(r["age_max"] for r in rs) if kind == "hold" else None)
                c["hit_ms_per_window"] = c["hit_ms"] / c["windows_per_step"]
                cases.append(c)
                print(json.dumps(c), flush=True)
            with open(a.out, "w") as f:                                           # what is measured so far
                json.dump(dict(partial=True, cases=cases), f, indent=1)
        eng.close()
        os.remove(path)
    os.rmdir(tmp)
    lines = ["# Live pool: N live recordings through one pool against N solo live handles", "",
             f"Written by `tools/bench_live_pool.py` on {torch.cuda.get_device_name(0)}; JSON beside this file.  Recipe geometries, "
             f"fixed embeddings, K = 2 targets, 16 kHz, window {a.window:g} s, overlap {a.overlap:g} s, max_rows {a.max_rows}, N "
             f"recordings of {a.seconds:g} s in packets of {a.packet_ms} ms, {a.repeats} runs per arm after a warm-up of three "
             f"windows per arm (median; min – max).  A *step* gives every recording in flight its next packet: ONE push of the "
             f"pool, or one push per solo handle, one after another -- the parent commit's path.  wall = host clock around the "
             f"step; it synchronises itself when a window became complete.  *aligned*: every recording starts at step 0, so a "
             f"completing step carries N windows; *staggered*: recording i starts 2 i steps late, so no two windows complete in "
             f"one step.  The arms alternate in the same run.  Nothing here is a gate."
             + ("" if hold_n is None else f"  *hold*: the staggered feed through store, one run of every slot with a complete window once "
                f"every recording has one waiting or the oldest has waited {a.hold_ms:g} ms ({hold_n} samples); a completing step "
                f"is one whose run launched.  windows / step: the recordings' regular windows over the completing steps, i.e. the recordings "
                f"that share a step's forwards; added latency: the largest age met at a run."), "",
             "| model | N | feed | path | completing steps | ms / completing step (median; min – max; worst) | windows / step | "
             "ms / window | ms / other step | total ms (min – max) | total / (N x audio) | rounds, forwards, launches / completing step | "
             "added latency (samples) | state bytes | rel L2 vs separate_long (worst recording) |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in cases:
        miss = "—" if c["miss_ms"] is None else f"{c['miss_ms']:.4f}"
        shapes = "—" if not c["shapes"] else "; ".join(f"{r}, {f}, {l}" for r, f, l in c["shapes"])
        rel = "—" if c["rel_vs_long"] is None else f"{c['rel_vs_long']:.1e}"
        lines.append(f"| {c['arch']} | {c['N']} | {c['feed']} | {c['path']} | {c['steps_completing']} | {c['hit_ms']:.2f} "
                     f"({min(c['hit_ms_runs']):.2f} – {max(c['hit_ms_runs']):.2f}; {c['hit_worst_ms']:.2f}) | "
                     f"{c['windows_per_step']:.2f} | {c['hit_ms_per_window']:.2f} | {miss} | "
                     f"{c['total_ms']:.1f} ({min(c['total_ms_runs']):.1f} – {max(c['total_ms_runs']):.1f}) | "
                     f"{c['total_ms'] / (1e3 * a.seconds * c['N']):.4f} | {shapes} | "
                     f"{'—' if c['age_max_samples'] is None else c['age_max_samples']} | {c['state_bytes']} | {rel} |")
    lines += ["", "<!-- notes -->"]
    with open(a.out, "w") as f:
        json.dump(dict(sample_rate=SR, window_s=a.window, overlap_s=a.overlap, seconds=a.seconds, max_rows=a.max_rows,
                       packet_ms=a.packet_ms, repeats=a.repeats, hold_ms=a.hold_ms, device=torch.cuda.get_device_name(0), cases=cases), f, indent=1)
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
