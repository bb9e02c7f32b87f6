"""The whole-block kernel in the native runtime: a round of live calls with WS_STREAM_BLOCK_KERNEL against the default path.

    python tools/bench_stream_block.py --out profiles/stream_block.json --md profiles/stream_block.md

The protocol and the arms of tools/bench_stream_pool.py (imported): SpEx+ shape, fixed embeddings, 10 ms packets at 16 kHz,
max_chunk_frames 256, 200 rounds per run after 20 warm-up rounds of the same shape.  Rows: a pool round with 1, 8 and 16
calls (one ws_engine_pool_push), and a solo stream of one row (one ws_engine_stream_push).  Arms: `default` -- GEMM, fused
middle, GEMM per block, the path there was -- and `block` -- one ws_tcn_block_stream(_rows)_fwd per block --, run
alternately in one process, --repeats times each (default 3).  The reference of a row is the default arm of the same run.
"separated" means that the block arm's slowest run is below the default arm's fastest.  The --md file is rewritten up to the
line `<!-- notes -->`; what follows it is kept.  Needs a GPU.  Nothing here is a gate."""
import argparse
import json
import os
import statistics
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_stream_pool import G, SHAPE, SR, WARMUP, pool_arm, serial_arm      # noqa: E402


class Flagged:
    """The engine with block_kernel=True on every stream and pool it opens: the arms of bench_stream_pool run on it as is."""

    def __init__(self, eng):
        self._eng = eng

    def stream(self, *a, **kw):
        return self._eng.stream(*a, block_kernel=True, **kw)

    def stream_pool(self, *a, **kw):
        return self._eng.stream_pool(*a, block_kernel=True, **kw)

    def info(self, key):
        return self._eng.info(key)


def verdict(d, b):
    if b["wall_ms_max"] < d["wall_ms_min"]:
        return f"separated: the block arm is faster, {d['wall_ms_median'] / b['wall_ms_median']:.2f}x"
    if d["wall_ms_max"] < b["wall_ms_min"]:
        return f"the block arm is SLOWER, {b['wall_ms_median'] / d['wall_ms_median']:.2f}x (separated the other way)"
    return "not separated: the runs of the two arms overlap"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--calls", default="1,8,16")
    ap.add_argument("--seconds", type=float, default=2.0, help="audio per call and run")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_block: needs a GPU (no CPU measurement exists)")
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    torch.manual_seed(0)
    model = get_model("ConvTasNet")(**SHAPE)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "spex_causal.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    engs = {"default": eng, "block": Flagged(eng)}
    n = SR * 10 // 1000
    rounds = max(8, int(a.seconds * 100))
    rows = [("pool", k) for k in map(int, a.calls.split(","))] + [("solo stream, 1 row", 1)]
    cases = []
    for kind, n_calls in rows:
        run = pool_arm if kind == "pool" else serial_arm
        runs = {"default": [], "block": []}
        for _ in range(a.repeats):                                       # the arms alternate: drift hits them alike
            for arm in ("default", "block"):
                runs[arm].append(run(engs[arm], n_calls, n, rounds))
        for arm in ("default", "block"):
            wall = [r["wall_ms"] for r in runs[arm]]
            c = dict(row=kind, calls=n_calls, arm=arm, rounds=rounds, wall_ms_runs=wall, wall_ms_median=statistics.median(wall),
                     wall_ms_min=min(wall), wall_ms_max=max(wall), launches_per_round=runs[arm][0]["launches"],
                     state_bytes=runs[arm][0]["state_bytes"])
            cases.append(c)
            print(json.dumps(c), flush=True)
    eng.close()
    os.remove(path)
    os.rmdir(tmp)
    lines = ["# The whole block in one launch: a round with WS_STREAM_BLOCK_KERNEL against the default path", "",
             f"Written by `tools/bench_stream_block.py` on {torch.cuda.get_device_name(0)}; JSON beside this file.  SpEx+ shape "
             f"(N 256, L 20, B 256, H 512, P 3, X 8, R 4, cLN, causal, Multi ends, concatConv), fixed embeddings, 16 kHz, 10 ms "
             f"packets (16 frames a call and round), {rounds} rounds per run after {WARMUP} warm-up rounds of the same shape, "
             f"`max_chunk_frames` {G}, {a.repeats} runs per arm, alternating in one process (median, and min – max as the "
             f"spread).  `default`: GEMM, `ws_tcn_mid_stream(_rows)_fwd`, GEMM per block; `block`: one "
             f"`ws_tcn_block_stream(_rows)_fwd` per block.  The reference of a row is the default arm of the same run.  wall = "
             f"host clock around the calls, each of which synchronises itself.  Nothing here is a gate; the flag is opt-in.", "",
             "| row | calls | arm | wall ms / round (median) | wall min – max | launches / round | state bytes |",
             "|---|---|---|---|---|---|---|"]
    for c in cases:
        lines.append(f"| {c['row']} | {c['calls']} | {c['arm']} | {c['wall_ms_median']:.3f} | {c['wall_ms_min']:.3f} – "
                     f"{c['wall_ms_max']:.3f} | {c['launches_per_round']} | {c['state_bytes']} |")
    lines += ["", "Block against default, per row (\"separated\": the block arm's slowest run is below the default arm's fastest):", ""]
    for kind, n_calls in rows:
        d, b = (next(c for c in cases if (c["row"], c["calls"], c["arm"]) == (kind, n_calls, arm)) for arm in ("default", "block"))
        lines.append(f"- {kind}, {n_calls} call(s): default {d['wall_ms_median']:.3f} ms ({d['launches_per_round']} launches) vs block "
                     f"{b['wall_ms_median']:.3f} ms ({b['launches_per_round']} launches) a round — {verdict(d, b)}")
    lines += ["", "<!-- notes -->"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(shape=SHAPE, sample_rate=SR, packet_ms=10, max_chunk_frames=G, warmup_rounds=WARMUP,
                       device=torch.cuda.get_device_name(0), cases=cases), f, indent=1)
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
