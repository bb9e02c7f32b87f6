"""Streaming Conv-TasNet on the SpEx+ shape: time per push, C-ABI calls per push, push time over chunk duration.

    python tools/bench_stream_tasnet.py --out profiles/stream_tasnet.json [--md profiles/stream_tasnet_table.md]

The model is the SpEx+ configuration (N 256, L 20, B 256, H 512, P 3, X 8, R 4, cLN, causal, Multi ends, concatConv) with
a fixed embedding, so a push is the separator alone.  rows in {1, 8, 32}, chunks of 10 / 40 / 160 ms at 16 kHz.  Per case:
  * device time per push: HIP events around the whole run of pushes, over the number of pushes (no synchronise inside);
  * host wall clock per push with a device synchronise after every push -- what a caller who waits for the samples sees;
  * C-ABI calls per push (every call launches at least one kernel; the torch copies that move pending samples are not
    counted) -- the figure a fused per-block kernel would attack;
  * push time over chunk duration (below 1: faster than real time);
  * for scale, the whole-utterance `forward` of the same model over the same audio, as one call.
Needs a GPU: there is no CPU measurement.  Nothing here is a gate."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SR = 16000
SHAPE = dict(N=256, L=20, B=256, H=512, P=3, X=8, R=4, norm="cLN", causal=True, spk_emb_dim=256, joint_training=False)


def run_case(model, rows, chunk_ms, pushes, warmup, calls):
    from wesep_amd.streaming import ConvTasNetStreamer
    d = next(model.parameters()).device
    n = SR * chunk_ms // 1000
    g = torch.Generator().manual_seed(rows * 1000 + chunk_ms)
    x = torch.randn(rows, (warmup + pushes) * n, generator=g).to(d)
    emb = torch.randn(rows, 256, generator=g).to(d)
    st = ConvTasNetStreamer(model, rows, max_chunk_frames=max(256, n // 10 + 16))
    st.enroll(emb)
    chunks = [x[:, i * n:(i + 1) * n].contiguous() for i in range(warmup + pushes)]

    def go(lo, hi, sync):
        out = 0
        for c in chunks[lo:hi]:
            out += st.push(c).shape[1]
            if sync:
                torch.cuda.synchronize()
        return out

    go(0, warmup, False)                       # the first pushes also fill the 160-sample window
    torch.cuda.synchronize()
    half = pushes // 2
    c0 = calls[0]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    emitted = go(warmup, warmup + half, False)
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / half
    per_push_calls = (calls[0] - c0) / half
    t0 = time.perf_counter()
    emitted += go(warmup + half, warmup + pushes, True)
    wall_ms = (time.perf_counter() - t0) * 1e3 / (pushes - half)
    assert emitted == pushes * n, (emitted, pushes * n)         # steady state: every push emits one chunk's worth
    # the same audio through the whole-utterance forward, one call
    with torch.no_grad():
        model(x[:, :4000], emb)
        torch.cuda.synchronize()
        e0.record()
        model(x[:, warmup * n:], emb)
        e1.record()
        torch.cuda.synchronize()
    whole_ms = e0.elapsed_time(e1)
    return dict(rows=rows, chunk_ms=chunk_ms, chunk_samples=n, pushes=pushes, device_ms_per_push=dev_ms,
                wall_ms_per_push_synced=wall_ms, abi_calls_per_push=per_push_calls, push_over_chunk_device=dev_ms / chunk_ms,
                push_over_chunk_wall=wall_ms / chunk_ms, audio_seconds=pushes * n / SR, whole_forward_ms=whole_ms,
                stream_total_device_ms=dev_ms * pushes, state_bytes=st.state_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--md", default=None)
    ap.add_argument("--rows", default="1,8,32")
    ap.add_argument("--chunks_ms", default="10,40,160")
    ap.add_argument("--seconds", type=float, default=4.0, help="audio per case")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream_tasnet: needs a GPU (no CPU measurement exists)")
    from wesep_amd import _lib as L
    from wesep_amd.models import get_model
    calls, check = [0], L.check

    def counting(rc, what=""):
        calls[0] += 1
        return check(rc, what)

    L.check = counting
    torch.manual_seed(0)
    model = get_model("ConvTasNet")(**SHAPE).cuda().eval()
    res = []
    for rows in map(int, a.rows.split(",")):
        for ms in map(int, a.chunks_ms.split(",")):
            pushes = max(8, int(a.seconds * 1000 / ms) // 2 * 2)
            r = run_case(model, rows, ms, pushes, 20, calls)
            res.append(r)
            print(json.dumps(r), flush=True)
    lines = ["| rows | chunk | device ms / push | wall ms / push (synced) | C-ABI calls / push | push / chunk (device) | "
             "push / chunk (wall) | streamed total ms | whole forward ms | audio s |", "|---|---|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['rows']} | {r['chunk_ms']} ms | {r['device_ms_per_push']:.3f} | {r['wall_ms_per_push_synced']:.3f} | "
                     f"{r['abi_calls_per_push']:.0f} | {r['push_over_chunk_device']:.3f} | {r['push_over_chunk_wall']:.3f} | "
                     f"{r['stream_total_device_ms']:.1f} | {r['whole_forward_ms']:.1f} | {r['audio_seconds']:.2f} |")
    table = "\n".join(lines)
    print(table)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(shape=SHAPE, sample_rate=SR, device=torch.cuda.get_device_name(0), cases=res), f, indent=1)
    if a.md:
        with open(a.md, "w") as f:
            f.write(table + "\n")


if __name__ == "__main__":
    main()
