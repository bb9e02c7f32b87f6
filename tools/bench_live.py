"""Live windows (ws_engine_live_*) of the four architectures at their recipe geometries: time per push, total, state.

    python tools/bench_live.py --out profiles/live.json --md profiles/live.md

pBSRNN (6 repeats), Conv-TasNet / SpEx+ (N 256), DPCCN and TF-GridNet (6 blocks) as their constructors build them, fixed
embeddings, K = 2 targets, 16 kHz, window S = 4 s, overlap O = 1 s (hop 3 s), max_rows 8, a 60 s recording in packets of 10
and 100 ms.  Per run, after one warm-up recording through the same handle (every shape the timed run uses has then run):
  * wall ms of every push -- the host clock around the call, which synchronises itself when a window became complete -- split
    into the pushes that completed a window and those that did not (host only: no launch, no synchronisation);
  * the total over the recording, flush included, and the same recording through ws_engine_separate_long in the same run,
    alternating with the live runs;
  * launches of a window-completing push, and "live_state_bytes".
Three runs per arm; median and min - max.  The --md file is rewritten up to the line `<!-- notes -->`; what follows it is
kept.  Needs a GPU.  Nothing here is a gate."""
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
MODELS = {
    "pBSRNN": ("BSRNN", dict(num_repeat=6, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False)),
    "ConvTasNet": ("ConvTasNet", dict(N=256, spk_emb_dim=256)),
    "DPCCN": ("DPCCN", dict()),
    "TFGridNet": ("TFGridNet", dict(n_fft=128, stride=64, n_layers=6, lstm_hidden_units=192, attn_n_head=4, attn_approx_qk_dim=512,
                                    emb_dim=128, emb_ks=1, emb_hs=1, spk_fuse_type="multiply", use_spk_transform=False)),
}


def live_run(lv, eng, mix, packet):
    S, H = lv.window, lv.window - lv.overlap
    emitted = lambda N: max((0 if N < S else 1 + (N - S) // H) - 1, 0) * H        # the rule of include/wesep_engine.h
    hit, miss, launches = [], [], set()
    t_all = time.perf_counter()
    for pos in range(0, len(mix), packet):
        chunk = mix[pos:pos + packet]
        t0 = time.perf_counter()
        got = lv.push(chunk, est_cap=emitted(pos + len(chunk)) - emitted(pos))         # a buffer of what this push emits
        ms = (time.perf_counter() - t0) * 1e3
        if eng.info("live_groups"):
            hit.append(ms)
            launches.add(eng.info("n_launches"))
        else:
            miss.append(ms)
        del got
    t0 = time.perf_counter()
    lv.flush()
    flush_ms = (time.perf_counter() - t0) * 1e3
    total_ms = (time.perf_counter() - t_all) * 1e3
    windows = eng.info("live_windows")
    lv.reset()
    return dict(hit_ms=statistics.median(hit), hit_max_ms=max(hit), miss_ms=statistics.median(miss) if miss else None,
                flush_ms=flush_ms, total_ms=total_ms, pushes=len(hit) + len(miss), hits=len(hit), windows=windows,
                launches=sorted(launches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--archs", default=",".join(MODELS))
    ap.add_argument("--packets_ms", default="10,100")
    ap.add_argument("--seconds", type=float, default=60.0, help="the recording")
    ap.add_argument("--window", type=float, default=4.0)
    ap.add_argument("--overlap", type=float, default=1.0)
    ap.add_argument("--max_rows", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_live: needs a GPU (no CPU measurement exists)")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    S, O, n, K = int(a.window * SR), int(a.overlap * SR), int(a.seconds * SR), 2
    rng = np.random.default_rng(0)
    mix, emb = (0.1 * rng.standard_normal(n)).astype(np.float32), rng.standard_normal((K, 256)).astype(np.float32)
    tmp = tempfile.mkdtemp()
    cases = []
    for arch in a.archs.split(","):
        name, kw = MODELS[arch]
        torch.manual_seed(0)
        path = os.path.join(tmp, f"{arch}.wsw")
        export_engine(get_model(name)(joint_training=False, **kw), path)
        eng = E.Engine(path)
        lv = eng.live(emb, E.ENROLL_EMBEDDING, S, O, a.max_rows)
        state = eng.info("live_state_bytes")
        packets = [SR * int(ms) // 1000 for ms in a.packets_ms.split(",")]
        live_run(lv, eng, mix, packets[-1])                                   # warm-up: every shape of the timed runs
        eng.separate_long(mix, emb, E.ENROLL_EMBEDDING, S, O, a.max_rows)
        runs = {p: [] for p in packets}
        long_ms, ref = [], None
        for _ in range(a.repeats):                                            # the arms alternate: drift hits them alike
            for p in packets:
                runs[p].append(live_run(lv, eng, mix, p))
            t0 = time.perf_counter()
            ref = eng.separate_long(mix, emb, E.ENROLL_EMBEDDING, S, O, a.max_rows)
            long_ms.append((time.perf_counter() - t0) * 1e3)
            long_info = dict(long_windows=eng.info("long_windows"), long_forwards=eng.info("long_forwards"), arena_bytes=eng.info("arena_bytes"))
        # the outputs of the two paths on this recording (groups form differently: rounding of other row counts)
        parts = [lv.push(mix[pos:pos + packets[-1]]) for pos in range(0, n, packets[-1])] + [lv.flush()]
        got = np.concatenate(parts, axis=1)
        rel = float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref.astype(np.float64)))
        lv.close()
        for p in packets:
            med = lambda key: statistics.median(r[key] for r in runs[p] if r[key] is not None) if runs[p][0][key] is not None else None
            c = dict(arch=arch, packet_ms=1000 * p // SR, packet_samples=p, pushes=runs[p][0]["pushes"], hits=runs[p][0]["hits"],
                     windows=runs[p][0]["windows"], hit_ms=med("hit_ms"), hit_ms_runs=[r["hit_ms"] for r in runs[p]],
                     hit_max_ms=max(r["hit_max_ms"] for r in runs[p]), miss_ms=med("miss_ms"), flush_ms=med("flush_ms"),
                     total_ms=med("total_ms"), total_ms_runs=[r["total_ms"] for r in runs[p]], launches_hit=runs[p][0]["launches"],
                     state_bytes=state, long_ms=statistics.median(long_ms), long_ms_runs=long_ms, rel_vs_long=rel, **long_info)
            cases.append(c)
            print(json.dumps(c), flush=True)
        eng.close()
        os.remove(path)
    os.rmdir(tmp)
    lines = ["# Live windows: time per push, total over a recording, state", "",
             f"Written by `tools/bench_live.py` on {torch.cuda.get_device_name(0)}; JSON beside this file.  Recipe geometries, fixed "
             f"embeddings, K = 2 targets, 16 kHz, window {a.window:g} s, overlap {a.overlap:g} s, max_rows {a.max_rows}, a "
             f"{a.seconds:g} s recording, {a.repeats} runs per arm after one warm-up recording (median; min – max of the totals).  "
             f"wall = host clock around the call; a push that completes a window synchronises itself, one that completes none is "
             f"host work only.  `separate_long` is the same recording through `ws_engine_separate_long` in the same run, "
             f"alternating with the live runs.  Latency is S … S + H = {a.window:g} … {2 * a.window - a.overlap:g} s of audio by "
             f"construction; the table is about compute.  Nothing here is a gate.", "",
             "| model | packet | pushes (completing a window) | ms / completing push (median; worst) | ms / other push | flush ms | "
             "total ms (min – max) | separate_long ms (min – max) | total / audio | launches / completing push | state bytes | "
             "separate_long arena bytes | rel L2 vs separate_long |", "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for c in cases:
        miss = "—" if c["miss_ms"] is None else f"{c['miss_ms']:.4f}"
        lines.append(f"| {c['arch']} | {c['packet_ms']} ms | {c['pushes']} ({c['hits']}) | {c['hit_ms']:.2f}; {c['hit_max_ms']:.2f} | {miss} | "
                     f"{c['flush_ms']:.2f} | {c['total_ms']:.1f} ({min(c['total_ms_runs']):.1f} – {max(c['total_ms_runs']):.1f}) | "
                     f"{c['long_ms']:.1f} ({min(c['long_ms_runs']):.1f} – {max(c['long_ms_runs']):.1f}) | "
                     f"{c['total_ms'] / (1e3 * a.seconds):.4f} | {', '.join(map(str, c['launches_hit']))} | {c['state_bytes']} | "
                     f"{c['arena_bytes']} | {c['rel_vs_long']:.1e} |")
    lines += ["", "<!-- notes -->"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(sample_rate=SR, window_s=a.window, overlap_s=a.overlap, seconds=a.seconds, max_rows=a.max_rows,
                       repeats=a.repeats, device=torch.cuda.get_device_name(0), cases=cases), f, indent=1)
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
