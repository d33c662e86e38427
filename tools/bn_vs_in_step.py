"""Median fused-step time of norm='batch' against norm='instance' on one device.

Both trainers live in one process and their timed blocks alternate (instance, batch, instance,
...), so clock / thermal drift and the box-to-box spread hit both alike.  Prints one JSON line
and, with --out, writes it to a file:

    python tools/bn_vs_in_step.py --out profiles/bn_vs_in_step.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "infrared-colorization-with-resnet-generator-and-patchgan_amd"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=9, help="alternating timed blocks per trainer")
    ap.add_argument("--only", default=None, choices=["instance", "batch"],
                    help="run one norm alone (e.g. under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    irc = importlib.import_module(PKG)
    g = torch.Generator().manual_seed(7)
    ir = (torch.rand(a.batch, 1, a.size, a.size, generator=g) * 2 - 1).cuda()
    rgb = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    trainers = {}
    for norm in ([a.only] if a.only else ["instance", "batch"]):
        cfg = irc.Config()
        cfg.device, cfg.compute_dtype, cfg.norm = "cuda:0", a.dtype, norm
        torch.manual_seed(1)
        trainers[norm] = irc.GANTrainer(cfg)
        for _ in range(a.warmup):
            trainers[norm].step(ir, rgb)
    torch.cuda.synchronize()
    times = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for norm, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                L = tr.step(ir, rgb)
            e1.record()
            e1.synchronize()
            times[norm].append(e0.elapsed_time(e1) / a.steps)
    assert all(torch.isfinite(tr.step(ir, rgb)).all() for tr in trainers.values())
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"metric": "median fused step, ms", "size": a.size, "batch": a.batch, "dtype": a.dtype,
           "steps_per_block": a.steps, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           **{k + "_ms": round(v, 4) for k, v in med.items()},
           "blocks_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    if len(med) == 2:
        res["batch_over_instance"] = round(med["batch"] / med["instance"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
