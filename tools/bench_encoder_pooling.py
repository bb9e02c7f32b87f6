"""Pooling of the 1-D speaker encoders (ECAPA-TDNN, CAM++) on the MI355X, timed alternately on one box; one JSON line.

    python tools/bench_encoder_pooling.py [--iters 30] [--steps 3] [--rounds 3] [--no-joint] [--no-engine]

(1) MHASTP / MQMHASTP forward + backward at the joint shapes, the per-(row, head) grid (ws_mhastp_fwd / _bwd) against
    the grid split over T (ws_mhastp_fwd_split / _bwd_split): ECAPA c512 (R 32, 398 frames, C 1536) and CAM++ (R 32,
    199 frames, C 512); and an R sweep of ECAPA-MHASTP (R*H from 2 to 256) to show where the split stops paying.
(2) The joint pBSRNN training step of `bench.py --joint` with ECAPA-ASTP against ECAPA-MQMHASTP and with CAM++-TSTP
    against CAM++-ASTP and CAM++-MQMHASTP.
(3) The native runtime's first-call and steady latency for R = 1 with a 10 s enrollment (1001 fbank frames).

Work counted for the roof as in tools/bench_pooling.py (fp32 VALU FMA): the attention MLP forward, about 4x that for
the backward (recompute, dx, dh and the weight gradients)."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.bench_common import PEAK_HBM_GBS          # noqa: E402
from tools.bench_pooling import PEAK_FP32_TFLOPS, pool_flops   # noqa: E402


def _pool_case(name, R, T, C, d):
    from wesep_amd.models.resnet import MHASTP, MQMHASTP
    pool = (MQMHASTP if name == "MQMHASTP" else MHASTP)(in_dim=C).to(d)
    x = torch.randn(R * T, C, device=d).relu_().requires_grad_(True)
    dout = torch.randn(R, pool.get_out_dim(), device=d)
    q0 = pool.n_query[0] if name == "MQMHASTP" else pool
    Q = pool.query_num if name == "MQMHASTP" else 1

    def once(split):
        out = pool.run(x, R, 1, T, split=split)
        out.backward(dout)
    return once, pool_flops(R, T, Q, q0.head_num, q0.d_model, q0.d_s), Q * q0.head_num


def _time_alternating(fns, iters, rounds):
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(iters):
                fn()
            ev1.record()
            torch.cuda.synchronize()
            times[k].append(ev0.elapsed_time(ev1) / iters)
    return {k: min(v) for k, v in times.items()}


def bench_pools(iters, rounds, d):
    from wesep_amd import dev
    cus = dev.cu_count(d)
    out = []
    cases = [("ECAPA_c512", n, 32, 398, 1536) for n in ("MHASTP", "MQMHASTP")] + \
            [("CAMPPlus", n, 32, 199, 512) for n in ("MHASTP", "MQMHASTP")] + \
            [("ECAPA_c512_sweep", "MHASTP", R, 398, 1536) for R in (1, 2, 8, 128)]
    for enc, name, R, T, C in cases:
        once, (ffl, bfl), qh = _pool_case(name, R, T, C, d)
        best = _time_alternating({"per_row_head": lambda: once(False), "split": lambda: once(True)}, iters, rounds)
        H = 2 if name == "MHASTP" else 8
        tsplit = dev.mhastp_split_sizes(R, 1, T, C, qh // H, H, cus)[0]
        row = {"encoder": enc, "pool": name, "R": R, "T": T, "C": C, "RH": R * H,
               "tsplit": tsplit, "gflop": (ffl + bfl) / 1e9, "ms": best,
               "speedup": best["per_row_head"] / best["split"]}
        row["fp32_roof_frac"] = {k: (ffl + bfl) / (v * 1e-3) / 1e12 / PEAK_FP32_TFLOPS for k, v in best.items()}
        out.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    return out


def make_step(spk_model, pool, d):
    import bench as B
    from wesep_amd.models import get_model
    from wesep_amd.optim import FusedClipAdam
    from wesep_amd.utils.losses import parse_loss
    from wesep_amd.utils.synthetic import synth_batch
    torch.manual_seed(0)
    kw = dict(B.MODEL_KW)
    kw.update(joint_training=True, spk_model=spk_model, spk_feat=True,
              spk_args=dict(feat_dim=80, embed_dim=kw["spk_emb_dim"], pooling_func=pool))
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
    out = {}
    for spk_model, pools in (("ECAPA_TDNN_c512", ("ASTP", "MQMHASTP")), ("CAMPPlus", ("TSTP", "ASTP", "MQMHASTP"))):
        runs = {p: make_step(spk_model, p, d) for p in pools}
        for fn in runs.values():
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        times = {p: [] for p in runs}
        for _ in range(rounds):
            for p, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    fn()
                torch.cuda.synchronize()
                times[p].append((time.perf_counter() - t0) / steps * 1e3)
        out[spk_model] = {"step_ms": {p: min(v) for p, v in times.items()}, "all_ms": times}
        print(json.dumps({spk_model: out[spk_model]}), file=sys.stderr, flush=True)
        del runs
        torch.cuda.empty_cache()
    return out


def bench_engine(d, reps=10):
    import numpy as np
    from wesep_amd import engine as E
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    out = {}
    g = torch.Generator().manual_seed(1)
    mix = (0.1 * torch.randn(1, 64000, generator=g)).numpy()
    fb = torch.randn(1, 1001, 80, generator=g)
    fb = (fb - fb.mean(1, keepdim=True)).numpy()
    for spk_model, pool in (("ECAPA_TDNN_c512", "ASTP"), ("ECAPA_TDNN_c512", "MQMHASTP"), ("CAMPPlus", "TSTP"),
                            ("CAMPPlus", "ASTP"), ("CAMPPlus", "MQMHASTP")):
        torch.manual_seed(0)
        model = get_model("BSRNN")(num_repeat=6, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                                   joint_training=True, spk_feat=True, spk_model=spk_model, spk_emb_dim=192,
                                   spk_args=dict(feat_dim=80, embed_dim=192, pooling_func=pool)).eval()
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "m.wsw")
            export_engine(model, path)
            eng = E.Engine(path)
            t0 = time.perf_counter()
            eng.separate(mix, fb, E.ENROLL_FBANK)
            first = (time.perf_counter() - t0) * 1e3
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                eng.separate(mix, fb, E.ENROLL_FBANK)
                ts.append((time.perf_counter() - t0) * 1e3)
            eng.close()
        out[f"{spk_model}-{pool}"] = {"first_ms": first, "steady_ms": float(np.median(ts))}
        print(json.dumps({f"{spk_model}-{pool}": out[f"{spk_model}-{pool}"]}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-joint", action="store_true")
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    d = torch.device("cuda", 0)
    out = {"pooling": bench_pools(args.iters, args.rounds, d), "hbm_peak_gbs": PEAK_HBM_GBS,
           "fp32_peak_tflops": PEAK_FP32_TFLOPS}
    if not args.no_joint:
        out["joint_step"] = bench_joint(args.steps, args.rounds, d)
    if not args.no_engine:
        out["engine_R1_10s"] = bench_engine(d)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
