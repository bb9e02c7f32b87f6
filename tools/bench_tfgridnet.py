"""GPU bench of the TF-GridNet row (default reference configuration, fixed embeddings, 6 s utterances):
fwd + SI-SDR + bwd + per-tensor clip + Adam on `--rows` rows of 4 s, one JSON line.  Not the headline metric."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--recipe", action="store_true",
                    help="model_args of examples/librimix/tse/v2/confs/tfgridnet.yaml (emb_dim 128, emb_ks = emb_hs = 1) "
                         "instead of the constructor defaults (emb_dim 48, emb_ks 4)")
    ap.add_argument("--rowmajor", action="store_true",
                    help="WESEP_TFGRID_BLOCKED=0: the row-major recurrence path instead of the blocked-layout default")
    ap.add_argument("--cpu", action="store_true", help="also time the CPU oracle on a bounded sample (cpu_baseline)")
    args = ap.parse_args()
    os.environ["WESEP_TFGRID_BLOCKED"] = "0" if args.rowmajor else "1"
    from wesep_amd.functional import SISDRFn
    from wesep_amd.models import get_model
    from wesep_amd.optim import FusedClipAdam
    from wesep_amd.utils.synthetic import synth_batch
    d = torch.device("cuda:0")
    torch.manual_seed(0)
    kw = dict(n_fft=128, stride=64, n_layers=6, lstm_hidden_units=192, attn_n_head=4, attn_approx_qk_dim=512,
              emb_dim=128, emb_ks=1, emb_hs=1, use_spk_transform=False, spk_fuse_type="multiply") if args.recipe else {}
    model = get_model("TFGridNet")(joint_training=False, **kw).to(d).train()
    opt = FusedClipAdam(model.parameters(), lr=1e-3, weight_decay=1e-4, clip_grad=5.0)
    wav, tgt, emb = (t.to(d) for t in synth_batch(args.rows, 96000, 42))

    def step():
        est, _ = model(wav, emb)
        loss = SISDRFn.apply(est, tgt, 1e-8)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    from wesep_amd import dev, _lib as L
    import bench_common as BC
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    dev.prof_enable(True)
    # the recurrence launches are priced at the model's REAL hidden size (192 in the recipe), not the 256 the kernels pad to
    hidden = next((m.hidden for m in model.modules() if hasattr(m, "hidden") and isinstance(getattr(m, "hidden"), int)), None)
    dev.alg_reset(True, lstm_units=hidden)
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    dev.prof_enable(False)
    roof = BC.roofline(dev, L, args.steps)
    dev.alg_reset(False)
    cpu = BC.cpu_baseline("tfgridnet") if args.cpu else None
    print(json.dumps({"metric": "utterances/sec (6 s, 16 kHz) fwd+bwd, TF-GridNet (fixed embeddings), 6 s utterances",
                      "value": args.rows * args.steps / el, "unit": "utterances/s",
                      "ms_per_step": el / args.steps * 1e3, "rows": args.rows, "steps": args.steps,
                      "dtype": "bf16x3 (recurrences, projections, attention, convolutions) + fp16x2 (inter-frame pair BPTT, d(xn); the inter-frame "
                               "cluster forward's recurrent product with WESEP_LSTM_CLUSTER2=1) + fp16x1 weight gradients (WESEP_TNB_A16=1), fp32 accumulate",
                      "lstm_units_priced": hidden,
                      "config": "recipe" if args.recipe else "constructor defaults", "blocked_recurrence": bool(args.recipe and not args.rowmajor),
                      "data": "synthetic", "final_loss_dB": float(loss.item()),
                      "params_M": sum(p.numel() for p in model.parameters()) / 1e6,
                      "peak_mem_GB": torch.cuda.max_memory_allocated() / 1e9, "roofline": roof, "cpu_baseline": cpu,
                      "n_gpus": 1, "higher_is_better": True}), flush=True)


if __name__ == "__main__":
    main()
