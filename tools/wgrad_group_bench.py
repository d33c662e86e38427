"""Per-layer time of the ResnetBlock weight gradient (256 -> 256, 3x3 reflect, 64 x 64 maps, B = 16,
bf16) through ops.conv_wgrad (one layer per launch) and ops.conv_wgrad_group with 1..4 layers
per launch, kernel + reduce, dispatch included.  Interleaved: every round times each variant
once over ``--layers`` distinct layers' operands (the step's 18, so L2 holds no operand from the
previous launch), and the medians over the rounds are printed.

    python tools/wgrad_group_bench.py [--rounds 9] [--batch 16] [--hw 64] [--ch 256] [--only "group 3"]"""
import argparse
import importlib
import statistics
import sys

import torch

sys.path.insert(0, ".")
irc = importlib.import_module("infrared-colorization-with-resnet-generator-and-patchgan_amd")
ops = irc.ops
DEV = "cuda"

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--hw", type=int, default=64)
ap.add_argument("--ch", type=int, default=256)
ap.add_argument("--layers", type=int, default=12)   # a multiple of 1, 2, 3 and 4
ap.add_argument("--only", default=None, help="time this variant alone (a counter pass): per-layer, 'group 3', ...")
args = ap.parse_args()
B, H, C, L = args.batch, args.hw, args.ch, args.layers
spec = ops.ConvSpec(C, C, 3, 1, 1, ops.PAD_REFLECT)
xs = [ops.Feat(torch.randn(B, H, H, C, device=DEV).bfloat16()) for _ in range(L)]
dys = [ops.Feat(torch.randn(B, H, H, C, device=DEV).bfloat16()) for _ in range(L)]
dws = [torch.zeros(C * 9 * C, device=DEV) for _ in range(L)]


def per_layer():
    for x, dy, dw in zip(xs, dys, dws):
        ops.conv_wgrad(spec, x, dy, dw, ops.BF16)


def grouped(g):
    def run():
        for i in range(0, L, g):
            assert ops.conv_wgrad_group(spec, xs[i:i + g], dys[i:i + g], dws[i:i + g], ops.BF16)
    return run


def timeit(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / L * 1e3   # us per layer


variants = {"per-layer": per_layer, **{f"group {g}": grouped(g) for g in (1, 2, 3, 4)}}
if args.only:
    variants = {args.only: variants[args.only]}
for fn in variants.values():   # warm-up
    fn()
torch.cuda.synchronize()
times = {k: [] for k in variants}
for _ in range(args.rounds):
    for k, fn in variants.items():
        times[k].append(timeit(fn))
print(f"wgrad {C}->{C} 3x3 reflect @ b{B}/{H}x{H}, us per layer (kernel + reduce), {args.rounds} interleaved rounds")
for k, v in times.items():
    print(f"  {k:10s} median {statistics.median(v):6.1f}  min {min(v):6.1f}  max {max(v):6.1f}", flush=True)
