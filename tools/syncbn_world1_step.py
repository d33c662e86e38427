"""What the SyncBN split and its collectives cost on ONE device: the median fused step of
norm='batch' local against Config.sync_bn with the collectives forced on over RCCL at world
size 1.

Two trainers in one process, one RCCL process group of one rank:
  local -- GANTrainer(cfg): no collectives at all (world size 1);
  sync  -- cfg.sync_bn = True, GANTrainer(cfg, force_reduce=True): the bucketed gradient
           all-reduces AND one fp64 all-reduce per BatchNorm forward and backward;
  grads -- (with --grads) force_reduce=True without sync_bn: the gradient all-reduces alone, so
           sync - grads is the share of the BatchNorm split.
Their timed blocks alternate (local, sync, local, ...), so clock / thermal drift and the
box-to-box spread hit all alike.  A collective over one rank moves no data between devices: this
measures launch, stream hand-over and kernel-split cost, NOT multi-rank RCCL latency.  Prints
one JSON line and, with --out, writes it to a file:

    python tools/syncbn_world1_step.py --grads --out profiles/syncbn_world1_step.json
"""
import argparse
import importlib
import json
import os
import statistics
import sys
import tempfile

import torch
import torch.distributed as dist

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
    ap.add_argument("--grads", action="store_true", help="also time the forced gradient collectives without sync_bn")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    store = os.path.join(tempfile.mkdtemp(), "store")
    dist.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    irc = importlib.import_module(PKG)
    g = torch.Generator().manual_seed(7)
    ir = (torch.rand(a.batch, 1, a.size, a.size, generator=g) * 2 - 1).cuda()
    rgb = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    kinds = {"local": (False, False), "sync": (True, True)}
    if a.grads:
        kinds["grads"] = (False, True)
    trainers = {}
    for kind, (sync, force) in kinds.items():
        cfg = irc.Config()
        cfg.device, cfg.compute_dtype, cfg.norm, cfg.sync_bn = "cuda:0", a.dtype, "batch", sync
        torch.manual_seed(1)
        trainers[kind] = irc.GANTrainer(cfg, force_reduce=force)
        assert (trainers[kind].core.gen.bn_sync is not None) == sync
        for _ in range(a.warmup):
            trainers[kind].step(ir, rgb)
    torch.cuda.synchronize()
    times = {k: [] for k in trainers}
    for _ in range(a.rounds):
        for kind, tr in trainers.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                tr.step(ir, rgb)
            e1.record()
            e1.synchronize()
            times[kind].append(e0.elapsed_time(e1) / a.steps)
    assert all(torch.isfinite(tr.step(ir, rgb)).all() for tr in trainers.values())
    torch.cuda.synchronize()
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"metric": "median fused step, ms", "size": a.size, "batch": a.batch, "dtype": a.dtype, "norm": "batch",
           "world_size": 1, "backend": "nccl", "steps_per_block": a.steps, "rounds": a.rounds,
           "device": torch.cuda.get_device_name(0),
           **{k + "_ms": round(v, 4) for k, v in med.items()},
           "sync_over_local": round(med["sync"] / med["local"], 4),
           "blocks_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    if "grads" in med:
        res["sync_over_grads"] = round(med["sync"] / med["grads"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
