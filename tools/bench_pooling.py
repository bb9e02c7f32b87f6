"""MHASTP / MQMHASTP pooling on the MI355X: (1) the pooling layer's forward + backward at the `bench.py --joint` shape
(R 32, 398 frames -> the ResNet34 activation [32, 10, 50, 256]) and (2) the joint pBSRNN training step of `bench.py --joint`
with TSTP and with MQMHASTP pooling, timed alternately on one box.  Prints one JSON line.

    python tools/bench_pooling.py [--iters 50] [--steps 5] [--rounds 3]

Work counted for the roof (fp32 VALU FMA, tools/bench_common.py figures): per frame and (query, head) the attention MLP
64*dm + ds*64 products forward; the backward recomputes it and adds dx (W1^T dz), dh (W2^T dl) and the two weight
gradients -- about 3x the forward."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_common import PEAK_HBM_GBS   # noqa: E402

PEAK_FP32_TFLOPS = 157.3       # MI355X_MICROARCH.md: vector FP32


def pool_flops(R, T, Q, H, dm, ds, layers=2):
    n1 = 64 if layers == 2 else ds
    fwd = 2 * R * T * Q * H * (n1 * dm + (64 * ds if layers == 2 else 0))
    return fwd, 4 * fwd          # backward: recompute + dx + dW (and dh, dW2)


def bench_pool(iters, d):
    from wesep_amd.models.resnet import MQMHASTP
    R, Fq, T, C = 32, 10, 50, 256
    pool = MQMHASTP(in_dim=C * Fq).to(d)
    x = torch.randn(R * Fq * T, C, device=d).relu_().requires_grad_(True)
    dout = torch.randn(R, pool.get_out_dim(), device=d)

    def once():
        out = pool.run(x, R, Fq, T)
        out.backward(dout)
    for _ in range(5):
        once()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    f_ms = b_ms = 0.0
    for _ in range(iters):
        ev[0].record()
        out = pool.run(x, R, Fq, T)
        ev[1].record()
        out.backward(dout)
        ev[2].record()
        torch.cuda.synchronize()
        f_ms += ev[0].elapsed_time(ev[1])
        b_ms += ev[1].elapsed_time(ev[2])
    f_ms, b_ms = f_ms / iters, b_ms / iters
    q0 = pool.n_query[0]
    ffl, bfl = pool_flops(R, T, pool.query_num, q0.head_num, q0.d_model, q0.d_s)
    tf = (ffl + bfl) / ((f_ms + b_ms) * 1e-3) / 1e12
    return {"shape": [R, Fq, T, C], "pool": "MQMHASTP", "fwd_ms": f_ms, "bwd_ms": b_ms, "fwd_bwd_ms": f_ms + b_ms,
            "gflop": (ffl + bfl) / 1e9, "tflops": tf, "fp32_roof_frac": tf / PEAK_FP32_TFLOPS,
            "roof_ms": (ffl + bfl) / (PEAK_FP32_TFLOPS * 1e12) * 1e3}


def make_step(pool, d):
    import bench as B
    from wesep_amd.models import get_model
    from wesep_amd.optim import FusedClipAdam
    from wesep_amd.utils.losses import parse_loss
    from wesep_amd.utils.synthetic import synth_batch
    torch.manual_seed(0)
    kw = dict(B.MODEL_KW)
    kw.update(joint_training=True, spk_model="ResNet34", spk_feat=True,
              spk_args=dict(feat_dim=80, embed_dim=256, pooling_func=pool, two_emb_layer=False))
    model = get_model("BSRNN")(**kw).to(d).train()
    opt = FusedClipAdam(model.parameters(), lr=B.LR0, weight_decay=B.WD, clip_grad=B.CLIP)
    crit = parse_loss("SISDR")[0]
    R = B.ROWS
    wav, tgt, _ = (t.to(d) for t in synth_batch(R, B.T, 42))
    fb = torch.randn(R, 398, 80, generator=torch.Generator().manual_seed(43))
    emb = (fb - fb.mean(1, keepdim=True)).to(d)

    def step():
        est, _ = model(wav, emb)
        loss = crit(est, tgt).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def bench_joint(steps, rounds, d):
    runs = {p: make_step(p, d) for p in ("TSTP", "MQMHASTP")}
    for fn in runs.values():
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {p: [] for p in runs}
    for _ in range(rounds):                # alternate: both variants see the same box state
        for p, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                fn()
            torch.cuda.synchronize()
            times[p].append((time.perf_counter() - t0) / steps * 1e3)
    best = {p: min(v) for p, v in times.items()}
    return {"step_ms": best, "all_ms": times, "delta_ms": best["MQMHASTP"] - best["TSTP"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-joint", action="store_true")
    args = ap.parse_args()
    d = torch.device("cuda", 0)
    out = {"pooling": bench_pool(args.iters, d), "hbm_peak_gbs": PEAK_HBM_GBS, "fp32_peak_tflops": PEAK_FP32_TFLOPS}
    if not args.no_joint:
        out["joint_step"] = bench_joint(args.steps, args.rounds, d)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
