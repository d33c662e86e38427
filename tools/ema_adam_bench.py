"""What the generator weight EMA (Config.ema_decay) costs, on one device.

Kernel timing, on G's flat parameter count, HIP events around blocks of launches, the three
forms interleaved block by block and the median block taken:

    (a) ops.adam_dev                         the plain update (7 streams: 4 reads, 3 writes)
    (b) ops.adam_dev(..., ema=e)             Adam + EMA in one pass (9 streams: 5 reads, 4 writes)
    (c) ops.adam_dev + torch.lerp_           the unfused pair (10 streams and two launches)

each over a rotation of buffer sets larger than the 256 MiB Infinity Cache ("hbm": what the
step sees, its other kernels having swept the caches) and on one set over and over ("hot").
Then the fused bf16 step at 256x256, B = 16 with ema_decay 0 and 0.999, two trainers in one
process, their timed blocks alternating.

    python tools/ema_adam_bench.py --out profiles/ema_adam.txt
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
LR, B1, B2, EPS, DECAY = 2e-4, 0.5, 0.999, 1e-8, 0.999


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
    bufs = []
    for _ in range(sets):
        p = torch.randn(n, generator=g).cuda()
        bufs.append(dict(p=p, g=(torch.randn(n, generator=g) * 1e-2).cuda(), m=torch.zeros_like(p),
                         v=torch.zeros_like(p), e=p.clone()))
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    prm2, prm3 = torch.zeros(2, device="cuda"), torch.zeros(3, device="cuda")
    ops.adam_prep(cnt, LR, B1, B2, prm2)
    cnt.zero_()
    ops.adam_prep(cnt, LR, B1, B2, prm3, decay=DECAY)
    w = ops.ema_weight(DECAY, 1)

    def form_a(b):
        ops.adam_dev(b["p"], b["g"], b["m"], b["v"], prm2, B1, B2, EPS)

    def form_b(b):
        ops.adam_dev(b["p"], b["g"], b["m"], b["v"], prm3, B1, B2, EPS, ema=b["e"])

    def form_c(b):
        ops.adam_dev(b["p"], b["g"], b["m"], b["v"], prm2, B1, B2, EPS)
        b["e"].lerp_(b["p"], w)

    forms = {"a adam": form_a, "b adam+ema fused": form_b, "c adam, then lerp_": form_c}
    out = {}
    for label, pick in (("hbm", lambda i: bufs[i % sets]), ("hot", lambda i: bufs[0])):
        times = {k: [] for k in forms}
        for k, f in forms.items():
            _timed(lambda i: f(pick(i)), warmup)
        for _ in range(rounds):
            for k, f in forms.items():
                times[k].append(_timed(lambda i: f(pick(i)), iters))
        out[label] = {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}
    assert all(torch.isfinite(b[k]).all() for b in bufs for k in b)
    return out


def step_times(irc, size, batch, warmup, steps, rounds):
    g = torch.Generator().manual_seed(7)
    ir = (torch.rand(batch, 1, size, size, generator=g) * 2 - 1).cuda()
    rgb = (torch.rand(batch, 3, size, size, generator=g) * 2 - 1).cuda()
    trainers = {}
    for d in (0.0, DECAY):
        cfg = irc.Config()
        cfg.device, cfg.compute_dtype, cfg.ema_decay = "cuda:0", "bf16", d
        torch.manual_seed(1)
        trainers[d] = irc.GANTrainer(cfg)
        for _ in range(warmup):
            trainers[d].step(ir, rgb)
    torch.cuda.synchronize()
    times = {d: [] for d in trainers}
    for _ in range(rounds):
        for d, tr in trainers.items():
            times[d].append(_timed(lambda i: tr.step(ir, rgb), steps) / 1e3)   # ms per step
    assert all(torch.isfinite(tr.step(ir, rgb)).all() for tr in trainers.values())
    return {d: (statistics.median(v), min(v), max(v)) for d, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=4, help="buffer sets in the rotation (5 x 4n bytes each)")
    ap.add_argument("--iters", type=int, default=24, help="launches per timed block")
    ap.add_argument("--rounds", type=int, default=15, help="interleaved timed blocks per form")
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=10, help="steps per timed block")
    ap.add_argument("--step-rounds", type=int, default=9)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    irc = importlib.import_module(PKG)
    n = irc.engine.ParamStore(irc.g_param_shapes(), "cpu").numel
    lines = [f"device: {torch.cuda.get_device_name(0)}",
             f"G flat buffer: n = {n} fp32 ({4 * n / 2 ** 20:.1f} MiB per stream)", ""]
    kt = kernel_times(irc, n, a.sets, a.iters, a.rounds, a.warmup)
    streams = {"a adam": 7, "b adam+ema fused": 9, "c adam, then lerp_": 10}
    for label, res in kt.items():
        note = (f"rotation of {a.sets} buffer sets, {a.sets * 5 * 4 * n / 2 ** 20:.0f} MiB" if label == "hbm"
                else "one buffer set, back to back")
        lines.append(f"kernels, {label} ({note}); median of {a.rounds} interleaved blocks of {a.iters} calls")
        for k, (med, lo, hi) in res.items():
            lines.append(f"  ({k:<20}) {med:8.1f} us  [min {lo:.1f}, max {hi:.1f}]  "
                         f"{streams[k] * 4 * n / med / 1e6:6.2f} TB/s over {streams[k]} streams")
        ta, tb, tc = (res[k][0] for k in streams)
        lines.append(f"  fused / unfused pair (b/c): {tb / tc:.3f}    fused / plain (b/a): {tb / ta:.3f} "
                     f"(bytes: 9/7 = {9 / 7:.3f})")
        lines.append("")
    if not a.no_step:
        st = step_times(irc, a.size, a.batch, a.warmup, a.steps, a.step_rounds)
        lines.append(f"fused bf16 step, {a.size}x{a.size}, B = {a.batch}; median of {a.step_rounds} interleaved "
                     f"blocks of {a.steps} steps")
        for d, (med, lo, hi) in st.items():
            lines.append(f"  ema_decay = {d:<6g} {med:8.3f} ms  [min {lo:.3f}, max {hi:.3f}]")
        lines.append(f"  EMA on / off: {st[DECAY][0] / st[0.0][0]:.4f} "
                     f"({(st[DECAY][0] - st[0.0][0]) * 1e3:+.0f} us per step)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
