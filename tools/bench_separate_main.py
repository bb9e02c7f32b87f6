#!/usr/bin/env python
"""Throughput of `separate_main` on a seeded ragged workload: generator and runner (profiles/ragged_speaker.md).

    python tools/bench_separate_main.py --work DIR --gen                      # models + wavs + scp, from the seed alone
    python tools/bench_separate_main.py --work DIR --run \
        --arm tree8=runtime/separate_main:--batch,8 \
        --arm loop8=runtime/separate_main:--batch,8:WS_ENGINE_RAGGED_SPK=0 \
        --arm sort8=runtime/separate_main:--batch,8,--sort_by_length \
        --arm parent8=../parent/runtime/separate_main:--batch,8  --runs 2 --out DIR/result.json
    python tools/bench_separate_main.py --work DIR --run \
        --arm whole=runtime/separate_main --arm parent=../parent/runtime/separate_main       # the path without the new flags
    python tools/bench_separate_main.py --work DIR --gen --long_seconds 600 --utterances 1   # one synthetic 10-minute mixture
    python tools/bench_separate_main.py --work DIR --run --timeout 900 \
        --arm chunk4=runtime/separate_main:--chunk_seconds,4,--chunk_rows,8                  # windows of 4 s (profiles/longform.md)

Workload (the one of profiles/ragged_batch.md, now reproducible): 64 utterances, mixtures uniform in 1-8 s, two
enrollments per utterance uniform in 3-6 s, 16 kHz int16 noise; models with random weights: joint pBSRNN (6 repeats,
multiply fusion, no multi-fuse) + ResNet34 (TSTP) on waveform enrollment ("resnet34"), and the same separator with
ECAPA-TDNN c512 + ASTP ("ecapa"); with --models tfgridnet the recipe's TF-GridNet (6 blocks) + ResNet34.  Everything
is written under --work; nothing outside the tree is read.

An arm is NAME=EXE[:ARG,ARG...[:ENV=VALUE,...]].  The runner warms every arm up once per model, then runs the arms
alternating, --runs times each, and records per run the tool's own total (engine ms: the sum of the forwards' host times,
each of which ends in a device synchronise), the wall time of the process and the peak arena it printed."""
import argparse
import json
import os
import re
import subprocess
import sys
import time
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = {
    "resnet34": dict(spk_model="ResNet34", spk_emb_dim=256,
                     spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False)),
    "ecapa": dict(spk_model="ECAPA_TDNN_c512", spk_emb_dim=192, spk_args=dict(feat_dim=80, embed_dim=192, pooling_func="ASTP")),
    # --models tfgridnet (not in the default set): the recipe's TF-GridNet, 6 blocks, joint ResNet34 (profiles/ragged_gridnet.md)
    "tfgridnet": dict(separator="TFGridNet", spk_model="ResNet34", spk_emb_dim=256,
                      spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False)),
    # --models dpccn,spexplus (long recordings, profiles/longform.md): the constructors' default geometries, DPCCN with a
    # joint ResNet34, Conv-TasNet with its own SpEx+ speaker encoder on the waveform
    "dpccn": dict(separator="DPCCN", spk_model="ResNet34", spk_emb_dim=256, spk_feat=True,
                  spk_args=dict(feat_dim=80, embed_dim=256, pooling_func="TSTP", two_emb_layer=False)),
    "spexplus": dict(separator="ConvTasNet", N=256, spk_emb_dim=256),
}
DEFAULT_MODELS = ("resnet34", "ecapa")
TFGRIDNET = dict(n_fft=128, stride=64, n_layers=6, lstm_hidden_units=192, attn_n_head=4, attn_approx_qk_dim=512, emb_dim=128,
                 emb_ks=1, emb_hs=1, spk_fuse_type="multiply", use_spk_transform=False)


def _write_wav(path, x, sr=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes(np.asarray(x, dtype=np.int16).tobytes())


def workload(seed=2024, n=64, sr=16000, long_seconds=None):
    """(mixture samples [n], enrollment samples [n, 2]) of the seeded workload; long_seconds: every mixture that long."""
    rng = np.random.default_rng(seed)
    mix_n, enr_n = rng.integers(1 * sr, 8 * sr + 1, n), rng.integers(3 * sr, 6 * sr + 1, (n, 2))
    if long_seconds:
        mix_n[:] = int(long_seconds * sr)
    return mix_n, enr_n, rng


def generate(work, seed=2024, n=64, models=DEFAULT_MODELS, long_seconds=None):
    sys.path.insert(0, ROOT)
    import torch
    from wesep_amd.bin.export_engine import export_engine
    from wesep_amd.models import get_model
    os.makedirs(os.path.join(work, "wav"), exist_ok=True)
    mix_n, enr_n, rng = workload(seed, n, long_seconds=long_seconds)
    lines = []
    for i in range(n):
        paths = [os.path.join(work, "wav", f"{kind}{i:02d}.wav") for kind in ("mix", "a", "b")]
        for p, m in zip(paths, (mix_n[i], enr_n[i, 0], enr_n[i, 1])):
            _write_wav(p, rng.integers(-3000, 3000, int(m)))
        lines.append(f"u{i:02d} {paths[0]} {paths[1]} {paths[2]}\n")
    with open(os.path.join(work, "wav.scp"), "w") as f:
        f.writelines(lines)
    for name in models:
        torch.manual_seed(seed)
        kw = dict(MODELS[name])
        separator = kw.pop("separator", "BSRNN")
        if separator == "TFGridNet":
            model = get_model("TFGridNet")(joint_training=True, spk_feat=True, **TFGRIDNET, **kw)
        elif separator in ("DPCCN", "ConvTasNet"):
            model = get_model(separator)(joint_training=True, **kw)
        else:
            model = get_model("BSRNN")(num_repeat=6, spk_fuse_type="multiply", multi_fuse=False, use_spk_transform=False,
                                       joint_training=True, spk_feat=True, **kw)
        with torch.no_grad():
            for key, buf in model.named_buffers():
                if key.endswith("running_var"):
                    buf.uniform_(0.5, 1.5)
        export_engine(model, os.path.join(work, f"{name}.wsw"))
    return dict(seed=seed, utterances=n, audio_s=float(mix_n.sum()) / 16000, models=list(models))


def parse_arm(spec):
    name, rest = spec.split("=", 1)
    parts = rest.split(":")
    args = [a for a in parts[1].split(",") if a] if len(parts) > 1 else []
    env = dict(kv.split("=", 1) for kv in parts[2].split(",") if kv) if len(parts) > 2 else {}
    return name, os.path.abspath(parts[0]), args, env


def run_once(exe, args, env, work, model, timeout):
    out_dir = os.path.join(work, "out")
    os.makedirs(out_dir, exist_ok=True)
    cmd = [exe, "--wav_scp", os.path.join(work, "wav.scp"), "--model", os.path.join(work, f"{model}.wsw"), "--output_dir",
           out_dir] + args
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, **env), timeout=timeout)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(f"{' '.join(cmd)} failed ({r.returncode}): {r.stderr[-2000:]}")
    m = re.search(r"Total: process (\d+)ms audio taken (\d+)ms", r.stdout)
    arena = [int(v) for v in re.findall(r"(\d+) MiB arena", r.stdout)]
    launches = [int(v) for v in re.findall(r"(\d+) launches", r.stdout)]
    return dict(engine_ms=int(m.group(2)), audio_ms=int(m.group(1)), wall_s=round(wall, 3), peak_arena_mib=max(arena),
                launches_per_forward_max=max(launches))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--work", required=True)
    ap.add_argument("--gen", action="store_true")
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--arm", action="append", default=[])
    ap.add_argument("--models", default=",".join(DEFAULT_MODELS))
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per process")
    ap.add_argument("--long_seconds", type=float, default=None, help="--gen: every mixture this long (long recordings)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    models = [m for m in a.models.split(",") if m]
    result = {}
    if a.gen:
        result["workload"] = generate(a.work, a.seed, a.utterances, models, a.long_seconds)
    if a.run:
        arms = [parse_arm(s) for s in a.arm]
        if len(arms) < 1:
            ap.error("--run needs at least one --arm")
        result["arms"] = {}
        for model in models:
            for name, exe, args, env in arms:                       # warm-up of every arm: code objects, file cache
                run_once(exe, args, env, a.work, model, a.timeout)
            runs = {name: [] for name, *_ in arms}
            for _ in range(a.runs):                                 # alternating: neighbours on the host hit every arm alike
                for name, exe, args, env in arms:
                    runs[name].append(run_once(exe, args, env, a.work, model, a.timeout))
                    print(model, name, json.dumps(runs[name][-1]), flush=True)
            result["arms"][model] = runs
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
