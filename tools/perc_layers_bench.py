"""The fused step's time under Config.perc_layers, on one device.

One trainer per configuration in one process, the bf16 step at 256x256, B = 16, their timed blocks
alternating:

    default        the attributes left alone (relu3_3 at weight 1: the reference's launches)
    three          relu1_2, relu2_2, relu3_3 at weights 1, 0.5, 0.25, the pooled taps fused into
                   the max-pool backward (irgan_maxpool_bwd_tap)
    three_unfused  the same with engine.NO_TAP_FUSION: maxpool_bwd, then l1_tap over the whole map

``--configs default`` touches no attribute of this option, so the same file also times a tree
from before it (copy it there): run that tree and this one in turns, the older one twice, and its
own run-to-run spread is the yardstick for the default configuration.

    python tools/perc_layers_bench.py --configs default,three,three_unfused
"""
import argparse
import importlib
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "infrared-colorization-with-resnet-generator-and-patchgan_amd"
THREE = (("relu1_2", "relu2_2", "relu3_3"), (1.0, 0.5, 0.25))


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters   # ms per call


def _trainer(irc, name, dtype):
    cfg = irc.Config()
    cfg.device, cfg.compute_dtype = "cuda:0", dtype
    if name != "default":
        cfg.perc_layers, cfg.perc_weights = THREE
    tr = irc.GANTrainer(cfg)
    tr.netG.store.load(irc.seeded_state(irc.g_param_shapes(), 0), strict=True)
    tr.netD.store.load(irc.seeded_state(irc.d_param_shapes(), 1), strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    return tr


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="default,three,three_unfused")
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--rounds", type=int, default=9, help="timed blocks per configuration")
    ap.add_argument("--label", default="", help="a word for the output's first line (which tree this is)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    irc = importlib.import_module(PKG)
    names = a.configs.split(",")
    assert set(names) <= {"default", "three", "three_unfused"}, names
    g = torch.Generator().manual_seed(7)
    ir = (torch.rand(a.batch, 1, a.size, a.size, generator=g) * 2 - 1).cuda()
    rgb = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    trainers = {n: _trainer(irc, n, a.dtype) for n in names}

    def step(n):
        if n != "default":
            irc.engine.NO_TAP_FUSION = n == "three_unfused"
        return trainers[n].step(ir, rgb)

    for n in names:
        for _ in range(a.warmup):
            step(n)
    torch.cuda.synchronize()
    times = {n: [] for n in names}
    for _ in range(a.rounds):
        for n in names:
            times[n].append(_timed(lambda: step(n), a.steps))
    lines = [f"{a.label + ': ' if a.label else ''}device: {torch.cuda.get_device_name(0)}",
             f"fused {a.dtype} step, {a.size}x{a.size}, B = {a.batch}; median of {a.rounds} interleaved blocks of "
             f"{a.steps} steps"]
    for n in names:
        losses = trainers[n].losses(step(n))
        assert all(torch.isfinite(torch.tensor(v)) for v in losses.values()), (n, losses)
        t = times[n]
        lines.append(f"  {n:<14} {statistics.median(t):8.3f} ms  [min {min(t):.3f}, max {max(t):.3f}]  "
                     f"{a.batch / statistics.median(t) * 1e3:7.1f} img/s   loss_G_perc {losses['loss_G_perc']:.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)


if __name__ == "__main__":
    main()
