"""Streaming a causal cLN Conv-TasNet at the SpEx+ shape: the native runtime's push against the Python streamer.

    python tools/bench_engine_stream.py --out profiles/engine_stream.json --md profiles/engine_stream.md

Shape of profiles/stream_tasnet.md (N 256, L 20, B 256, H 512, P 3, X 8, R 4, cLN, causal, Multi ends, concatConv, fixed
embedding), rows 1 and 8, chunks of 10 / 40 / 160 ms at 16 kHz, 4 s of audio after 20 warm-up pushes, max_chunk_frames 256 in
every arm (a push is one group of frames).  Three arms, each run three times, alternating, so that the spread is known:
  * native        ws_engine_stream_push through the ctypes binding (one C call per push; host buffers in and out);
  * python-fused  ConvTasNetStreamer(fused=True): GEMM, ws_tcn_mid_stream_fwd, GEMM per block;
  * python-unfused ConvTasNetStreamer(fused=False): the launches of the streamer before the fused kernel existed -- the
    baseline, taken in the same session on the same device.
Per run: wall ms per push with a synchronise per push (the native push synchronises itself, once; the Python arms get a
torch.cuda.synchronize() after every push), and for the Python arms device ms per push (HIP events around a run of pushes
without a synchronise inside; the native push cannot be measured that way -- it waits for its own samples).  Also launches
per push and the carried state in bytes.  The --md file is rewritten up to the line `<!-- notes -->`; what follows it is
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
SHAPE = dict(N=256, L=20, B=256, H=512, P=3, X=8, R=4, norm="cLN", causal=True, spk_emb_dim=256, joint_training=False)
G = 256
WARMUP = 20
# hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage on csrc/stream.hip (no packed FP32)
RESOURCES = [("tcn_mid_stream_kernel", 79, 47, 0, "dynamic, (2 H + 16) * 4 bytes", 8),
             ("dwconv_stream_kernel", 106, 110, 0, "0", 4),
             ("ola_stream_kernel", 38, 12, 0, "dynamic, (L - hop) * 4 bytes", 8)]


def python_arm(model, rows, n, pushes, fused, calls):
    from wesep_amd.streaming import ConvTasNetStreamer
    d = next(model.parameters()).device
    g = torch.Generator().manual_seed(rows * 1000 + n)
    x = torch.randn(rows, (WARMUP + pushes) * n, generator=g).to(d)
    emb = torch.randn(rows, 256, generator=g).to(d)
    st = ConvTasNetStreamer(model, rows, max_chunk_frames=G, fused=fused)
    st.enroll(emb)
    chunks = [x[:, i * n:(i + 1) * n].contiguous() for i in range(WARMUP + pushes)]
    for c in chunks[:WARMUP]:
        st.push(c)
    torch.cuda.synchronize()
    half = pushes // 2
    c0 = calls[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for c in chunks[WARMUP:WARMUP + half]:
        st.push(c)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / half
    launches = (calls[0] - c0) / half
    t0 = time.perf_counter()
    for c in chunks[WARMUP + half:]:
        st.push(c)
        torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3 / (pushes - half)
    return dict(wall_ms=wall_ms, device_ms=dev_ms, launches=launches, state_bytes=st.state_bytes)


def native_arm(eng, rows, n, pushes):
    from wesep_amd import engine as E
    rng = np.random.default_rng(rows * 1000 + n)
    x = rng.standard_normal((rows, (WARMUP + pushes) * n)).astype(np.float32)
    emb = rng.standard_normal((rows, 256)).astype(np.float32)
    st = eng.stream(rows, emb, E.ENROLL_EMBEDDING, max_chunk_frames=G)
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
    return dict(wall_ms=wall_ms, device_ms=None, launches=max(launches), state_bytes=state)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--rows", default="1,8")
    ap.add_argument("--chunks_ms", default="10,40,160")
    ap.add_argument("--seconds", type=float, default=4.0, help="audio per run")
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_engine_stream: needs a GPU (no CPU measurement exists)")
    from wesep_amd import _lib as L
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    calls, check = [0], L.check

    def counting(rc, what=""):
        calls[0] += 1
        return check(rc, what)

    L.check = counting
    torch.manual_seed(0)
    model = get_model("ConvTasNet")(**SHAPE)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "spex_causal.wsw")
    export_engine(model, path)
    eng = E.Engine(path)
    model = model.cuda().eval()
    cases = []
    for rows in map(int, a.rows.split(",")):
        for ms in map(int, a.chunks_ms.split(",")):
            n = SR * ms // 1000
            pushes = max(8, int(a.seconds * 1000 / ms) // 2 * 2)
            arms = ("native", "python-fused", "python-unfused")
            all_runs = {arm: [] for arm in arms}
            for _ in range(a.repeats):                                   # the arms alternate: drift hits them alike
                for arm in arms:
                    if arm == "native":
                        all_runs[arm].append(native_arm(eng, rows, n, pushes))
                    else:
                        all_runs[arm].append(python_arm(model, rows, n, pushes, arm == "python-fused", calls))
            for arm in arms:
                runs = all_runs[arm]
                wall = [r["wall_ms"] for r in runs]
                dev = [r["device_ms"] for r in runs if r["device_ms"] is not None]
                c = dict(rows=rows, chunk_ms=ms, chunk_samples=n, pushes=pushes, arm=arm, wall_ms_runs=wall,
                         wall_ms_median=statistics.median(wall), wall_ms_min=min(wall), wall_ms_max=max(wall),
                         device_ms_runs=dev, device_ms_median=statistics.median(dev) if dev else None,
                         launches_per_push=runs[0]["launches"], state_bytes=runs[0]["state_bytes"])
                cases.append(c)
                print(json.dumps(c), flush=True)
    eng.close()
    os.remove(path)
    os.rmdir(tmp)
    lines = ["# Streaming in the native runtime: time per push against the Python streamer", "",
             f"Written by `tools/bench_engine_stream.py` on {torch.cuda.get_device_name(0)}; JSON beside this file.  SpEx+ shape "
             f"(N 256, L 20, B 256, H 512, P 3, X 8, R 4, cLN, causal, Multi ends, concatConv), fixed embedding, 16 kHz, "
             f"{a.seconds:g} s of audio per run after {WARMUP} warm-up pushes, `max_chunk_frames` {G}, {a.repeats} runs per arm "
             f"(median, and min – max as the spread).  wall = host clock per push with a synchronise per push; device = HIP "
             f"events around a run of pushes without a synchronise inside (Python arms only: the native push waits for its own "
             f"samples).  `python-unfused` issues the launches of the streamer as it was before `ws_tcn_mid_stream_fwd`: the "
             f"baseline, taken in the same session.  Nothing here is a gate.", "",
             "| rows | chunk | arm | wall ms / push (median) | wall min – max | device ms / push (median) | launches / push | "
             "push / chunk (wall) | state bytes |", "|---|---|---|---|---|---|---|---|---|"]
    for c in cases:
        dev = "—" if c["device_ms_median"] is None else f"{c['device_ms_median']:.3f}"
        lines.append(f"| {c['rows']} | {c['chunk_ms']} ms | {c['arm']} | {c['wall_ms_median']:.3f} | {c['wall_ms_min']:.3f} – "
                     f"{c['wall_ms_max']:.3f} | {dev} | {c['launches_per_push']:.0f} | {c['wall_ms_median'] / c['chunk_ms']:.3f} | "
                     f"{c['state_bytes']} |")
    lines += ["", "Separation of neighbouring arms (the slower arm's fastest run against the faster arm's slowest run; "
              "\"overlap\" means the arms do not separate beyond the three-run spread):", ""]
    by = {(c["rows"], c["chunk_ms"], c["arm"]): c for c in cases}
    for rows in sorted({c["rows"] for c in cases}):
        for ms in sorted({c["chunk_ms"] for c in cases}):
            for fast, slow in (("native", "python-fused"), ("python-fused", "python-unfused")):
                f, s = by[(rows, ms, fast)], by[(rows, ms, slow)]
                verdict = (f"separated, {s['wall_ms_median'] / f['wall_ms_median']:.2f}x" if f["wall_ms_max"] < s["wall_ms_min"]
                           else "overlap")
                lines.append(f"- rows {rows}, {ms} ms: {fast} {f['wall_ms_median']:.3f} vs {slow} {s['wall_ms_median']:.3f} ms — {verdict}")
    lines += ["", "Kernel resources (`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage`, no packed FP32):", "",
              "| kernel | SGPRs | VGPRs | scratch | LDS | occupancy (waves / SIMD) |", "|---|---|---|---|---|---|"]
    lines += [f"| `{k}` | {sg} | {vg} | {sc} | {lds} | {occ} |" for k, sg, vg, sc, lds, occ in RESOURCES]
    lines += ["", "<!-- notes -->"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(shape=SHAPE, sample_rate=SR, max_chunk_frames=G, warmup_pushes=WARMUP,
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
