"""What gradient-norm clipping (Config.clip_grad_G / clip_grad_D) costs, on one device.

The reduction kernel alone (ops.grad_sumsq) on G's flat gradient size, HIP events around blocks
of launches, over a rotation of buffers larger than the 256 MiB Infinity Cache ("hbm": what the
step sees) and on one buffer over and over ("hot"); then the fused bf16 step at 256x256, B = 16
with both clips off and both on (binding), two trainers in one process, their timed blocks
alternating.

    python tools/grad_clip_bench.py --out profiles/grad_clip_on.txt
    rocprofv3 --kernel-trace --stats ... -- python tools/grad_clip_bench.py --profile-steps 20
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
CLIP = 1.0   # far below either network's gradient norm at initialisation: both clips bind


def _timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        fn(i)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3   # us per call


def kernel_times(irc, n, sets, iters, rounds, warmup):
    ops = irc.ops
    g = torch.Generator().manual_seed(3)
    bufs = [(torch.randn(n, generator=g) * 1e-2).cuda() for _ in range(sets)]
    ws = torch.zeros(ops.grad_sumsq_parts(n), dtype=torch.float64, device="cuda")
    out = {}
    for label, pick in (("hbm", lambda i: bufs[i % sets]), ("hot", lambda i: bufs[0])):
        _timed(lambda i: ops.grad_sumsq(pick(i), ws), warmup)
        t = [_timed(lambda i: ops.grad_sumsq(pick(i), ws), iters) for _ in range(rounds)]
        out[label] = (statistics.median(t), min(t), max(t))
    return out


def _trainer(irc, clip):
    cfg = irc.Config()
    cfg.device, cfg.compute_dtype = "cuda:0", "bf16"
    cfg.clip_grad_G = cfg.clip_grad_D = clip
    torch.manual_seed(1)
    return irc.GANTrainer(cfg)


def _batch(size, batch):
    g = torch.Generator().manual_seed(7)
    return ((torch.rand(batch, 1, size, size, generator=g) * 2 - 1).cuda(),
            (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda())


def step_times(irc, size, batch, warmup, steps, rounds):
    ir, rgb = _batch(size, batch)
    trainers = {c: _trainer(irc, c) for c in (0.0, CLIP)}
    for tr in trainers.values():
        for _ in range(warmup):
            tr.step(ir, rgb)
    torch.cuda.synchronize()
    times = {c: [] for c in trainers}
    for _ in range(rounds):
        for c, tr in trainers.items():
            times[c].append(_timed(lambda i: tr.step(ir, rgb), steps) / 1e3)   # ms per step
    norms = trainers[CLIP].losses(trainers[CLIP].step(ir, rgb))
    assert all(torch.isfinite(tr.step(ir, rgb)).all() for tr in trainers.values())
    return {c: (statistics.median(v), min(v), max(v)) for c, v in times.items()}, norms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=8, help="gradient buffers in the rotation (4n bytes each)")
    ap.add_argument("--iters", type=int, default=24, help="launches per timed block")
    ap.add_argument("--rounds", type=int, default=15, help="timed blocks")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--step-rounds", type=int, default=9)
    ap.add_argument("--profile-steps", type=int, default=0,
                    help="only run this many clipped steps (for a kernel trace) and exit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    irc = importlib.import_module(PKG)
    if a.profile_steps:
        tr, (ir, rgb) = _trainer(irc, CLIP), _batch(a.size, a.batch)
        for _ in range(a.profile_steps):
            L = tr.step(ir, rgb)
        torch.cuda.synchronize()
        print({k: round(v, 4) for k, v in tr.losses(L).items()})
        return
    n = irc.engine.ParamStore(irc.g_param_shapes(), "cpu").numel
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"G flat gradient: n = {n} fp32 ({4 * n / 2 ** 20:.1f} MiB), "
             f"{irc.ops.grad_sumsq_parts(n)} blocks of 256 threads", ""]
    for label, (med, lo, hi) in kernel_times(irc, n, a.sets, a.iters, a.rounds, a.warmup).items():
        note = (f"rotation of {a.sets} buffers, {a.sets * 4 * n / 2 ** 20:.0f} MiB" if label == "hbm"
                else "one buffer, back to back")
        lines.append(f"ops.grad_sumsq, {label} ({note}); median of {a.rounds} blocks of {a.iters} calls: "
                     f"{med:7.1f} us  [min {lo:.1f}, max {hi:.1f}]  {4 * n / med / 1e6:5.2f} TB/s")
    lines.append("")
    st, norms = step_times(irc, a.size, a.batch, a.warmup, a.steps, a.step_rounds)
    lines.append(f"fused bf16 step, {a.size}x{a.size}, B = {a.batch}; median of {a.step_rounds} interleaved "
                 f"blocks of {a.steps} steps")
    for c, (med, lo, hi) in st.items():
        lines.append(f"  clip_grad_G = clip_grad_D = {c:<4g} {med:8.3f} ms  [min {lo:.3f}, max {hi:.3f}]")
    on, off = st[CLIP][0], st[0.0][0]
    lines.append(f"  clips on / off: {on / off:.4f} ({(on - off) * 1e3:+.0f} us per step); "
                 f"norms of the last step: D {norms['grad_norm_D']:.3f}, G {norms['grad_norm_G']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
