"""The fused Downsample-adjoint + InstanceNorm backward (ops.blur_down_bwd_in: two launches + the
finalize) against the launches it replaces (ops.blur_down_bwd + in_backward's reduce, finalize
and apply) at the down1 / down2 shapes of the flagship step and of 512x640, B = 4.

HIP events around blocks of launches, the two variants in interleaved blocks (so a clock or
thermal drift hits both), buffers rotated over sets that together exceed the Infinity Cache, so
every launch reads HBM.  Bytes: the algorithmic counts (small gradient, z and dz once per pass).

    python tools/resample_in_bwd_bench.py            # standalone kernels
    python tools/resample_in_bwd_bench.py --step     # the bf16 step, switch on / off in one process
"""
import importlib
import sys

import torch

sys.path.insert(0, ".")
irc = importlib.import_module("infrared-colorization-with-resnet-generator-and-patchgan_amd")
ops = irc.ops
DEV = "cuda"
Feat = ops.Feat


def block_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def kernels():
    # (name, N, H, W, C) of z: the full-resolution pre-norm map; dy is [N][H/2][W/2][C]
    shapes = [("down1 b16@256", 16, 256, 256, 128), ("down2 b16@256", 16, 128, 128, 256),
              ("down1 b4@512x640", 4, 512, 640, 128), ("down2 b4@512x640", 4, 256, 320, 256)]
    for name, N, H, W, C in shapes:
        E = N * H * W * C
        nset = max(2, -(-(512 << 20) // (int(4.5 * E))) + 1)
        sets = []
        for _ in range(nset):
            z = torch.randn(N, H, W, C, device=DEV).bfloat16()
            dy = (torch.randn(N, H // 2, W // 2, C, device=DEV) * 0.01).bfloat16()
            dz = torch.empty_like(z)
            mr = torch.empty(2 * N * C, device=DEV)
            sets.append((z, dy, dz, mr))
        work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
        red = torch.empty(2 * N * C, device=DEV)
        for z, _, _, mr in sets:
            ops.in_stats(Feat(z), work, mr)
        it = [0]

        def plain():
            z, dy, dz, mr = sets[it[0] % nset]
            it[0] += 1
            ops.blur_down_bwd(Feat(dy), Feat(dz))
            r, a = ops.in_bwd_parts(Feat(dz), Feat(z), ops.ACT_RELU, mr, work, red, Feat(dz))
            r()
            a()

        def fused():
            z, dy, dz, mr = sets[it[0] % nset]
            it[0] += 1
            if not ops.blur_down_bwd_in(Feat(dy), Feat(z), ops.ACT_RELU, mr, work, red, Feat(dz)):
                raise RuntimeError(f"{name}: the library refused the fused launches")

        for fn in (plain, fused):
            block_us(fn, nset)
        tp, tf = [], []
        for _ in range(5):
            tp.append(block_us(plain, 2 * nset))
            tf.append(block_us(fused, 2 * nset))
        tp.sort(), tf.sort()
        bp, bf = 2 * E * (0.25 + 1) + 4 * E + 6 * E, 2 * E * (0.25 + 1) * 2 + 2 * E   # bytes, see the issue's table
        print(f"{name:18s} C={C:3d}  three launches {tp[2]:7.1f} us [{tp[0]:.1f}-{tp[-1]:.1f}] {bp / tp[2] / 1e6:5.2f} TB/s"
              f"   fused {tf[2]:7.1f} us [{tf[0]:.1f}-{tf[-1]:.1f}] {bf / tf[2] / 1e6:5.2f} TB/s   x{tp[2] / tf[2]:.2f}",
              flush=True)
        del sets


def step(B=16, S=256, blocks=6, steps=20):
    """Median step time with the switch on and off, alternating blocks in one process."""
    cfg = irc.Config()
    cfg.device, cfg.compute_dtype, cfg.batch_size, cfg.img_size = "cuda:0", "bf16", B, S
    tr = irc.GANTrainer(cfg)
    tr.netG.store.load(irc.seeded_state(irc.g_param_shapes(), 0), strict=True)
    tr.netD.store.load(irc.seeded_state(irc.d_param_shapes(), 1), strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    g = torch.Generator().manual_seed(7)
    ir = (torch.rand(B, 1, S, S, generator=g) * 2 - 1).cuda()
    rgb = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
    for on in (True, False):
        ops.set_resample_bwd_fused(on)
        for _ in range(5):
            tr.step(ir, rgb)
    torch.cuda.synchronize()
    for blk in range(blocks):
        for on in (True, False):
            ops.set_resample_bwd_fused(on)
            tr.step(ir, rgb)
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
            evs[0].record()
            for i in range(steps):
                tr.step(ir, rgb)
                evs[i + 1].record()
            torch.cuda.synchronize()
            ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
            print(f"block {blk} fused={'on ' if on else 'off'} median {ms[steps // 2]:.3f} ms  min {ms[0]:.3f}", flush=True)
    ops.set_resample_bwd_fused(True)


if __name__ == "__main__":
    step() if "--step" in sys.argv else kernels()
