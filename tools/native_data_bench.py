"""The data path at img_size=None (profiles/native_data_path.txt).  B = 4, 512x640, both
modalities: irgan_u8_native_to_unit against the identity-table pair (irgan_area_resize_u8
+ irgan_u8_to_unit), HIP events, interleaved, medians; then train_kaist at native size on
a synthetic 512x640 tree (decode-bound: it shows the path end to end, not the kernels)."""
import argparse
import ctypes
import importlib
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "native_data_path.txt"))
OUT = ap.parse_args().out
irc = importlib.import_module("infrared-colorization-with-resnet-generator-and-patchgan_amd")
D, P, stream, call = irc.data, irc.ops.P, irc.ops.stream, irc._lib.call
DEV = "cuda"
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


B, H, W = 4, 512, 640
rng = np.random.default_rng(0)
ir = torch.from_numpy(rng.integers(0, 256, size=(B, H, W), dtype=np.uint8)).to(DEV)
rgb = torch.from_numpy(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)).to(DEV)
flip = torch.tensor([1, 0, 1, 0], dtype=torch.uint8, device=DEV)
rs = D.DeviceResizer(None, DEV)
yt, xt = rs._tab(H, H), rs._tab(W, W)
mx = torch.zeros(B, dtype=torch.int32, device=DEV)
o = {C: torch.empty(B, C, H, W, dtype=torch.float32, device=DEV) for C in (1, 3)}
o8 = {C: torch.empty(B, C, H, W, dtype=torch.uint8, device=DEV) for C in (1, 3)}


def native(u8, C, rule):
    mx.zero_()
    call("irgan_u8_native_to_unit", P(u8), B, H, W, C, ctypes.c_int64(H * W * C), P(flip), int(rule), P(mx), P(o[C]),
         None, stream())


def tables(u8, C, rule):
    mx.zero_()
    call("irgan_area_resize_u8", P(u8), B, H, W, C, ctypes.c_int64(H * W * C), P(yt[0]), P(yt[1]), P(yt[2]), H,
         P(xt[0]), P(xt[1]), P(xt[2]), W, P(flip), P(o8[C]), P(mx), stream())
    call("irgan_u8_to_unit", P(o8[C]), B, ctypes.c_int64(C * H * W), P(mx), int(rule), P(o[C]), stream())


forms = {
    "native  ir": lambda: native(ir, 1, True), "tables  ir": lambda: tables(ir, 1, True),
    "native rgb": lambda: native(rgb, 3, False), "tables rgb": lambda: tables(rgb, 3, False),
    "native both": lambda: (native(ir, 1, True), native(rgb, 3, False)),
    "tables both": lambda: (tables(ir, 1, True), tables(rgb, 3, False)),
}
# same results at the timed size
native(ir, 1, True); a1 = o[1].clone(); tables(ir, 1, True); assert torch.equal(a1, o[1])
native(rgb, 3, False); a3 = o[3].clone(); tables(rgb, 3, False); assert torch.equal(a3, o[3])
say(f"B={B} {H}x{W}: native == identity-table pair bit for bit (ir, rgb)")

INNER, SAMPLES = 20, 40
for f in forms.values():
    for _ in range(10):
        f()
torch.cuda.synchronize()
t = {k: [] for k in forms}
for _ in range(SAMPLES):
    for k, f in forms.items():          # interleaved: every sample visits each form
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            f()
        e1.record()
        e1.synchronize()
        t[k].append(e0.elapsed_time(e1) * 1000.0 / INNER)
say(f"us per call (HIP events over {INNER} back-to-back calls incl. the img_max memset; {SAMPLES} interleaved samples)")
for k, v in t.items():
    v.sort()
    say(f"  {k:12s} median {statistics.median(v):8.2f}  min {v[0]:8.2f}  p90 {v[int(0.9 * len(v))]:8.2f}")
byt = B * H * W * (1 + 4) + B * H * W * 3 * (1 + 4)
say(f"  bytes moved by the native form, both modalities: {byt / 1e6:.1f} MB "
    f"-> {byt / statistics.median(t['native both']) / 1e6:.2f} TB/s at its median")

# one train_kaist epoch at native size (decode-bound; shows the path end to end)
tmp = tempfile.mkdtemp()
seq = os.path.join(tmp, "set00", "V000")
os.makedirs(os.path.join(seq, "lwir")); os.makedirs(os.path.join(seq, "visible"))
N = 20
for i in range(N):
    g = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    Image.fromarray(np.repeat(g[:, :, None], 3, 2)).save(os.path.join(seq, "lwir", f"I{i:05d}.png"))
    c = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    Image.fromarray(c).save(os.path.join(seq, "visible", f"I{i:05d}.png"))
cfg = irc.Config()
cfg.device, cfg.train_roots, cfg.img_size = DEV, [os.path.join(tmp, "set00")], None
cfg.batch_size, cfg.epochs, cfg.num_workers, cfg.save_dir = 4, 2, 0, os.path.join(tmp, "ckpt")
stamps = []


def log(s):
    if " DONE " in s:
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
        say("  " + s)


t0 = time.perf_counter()
hist = irc.train_kaist(cfg, log=log)
say(f"train_kaist img_size=None, {N} pairs of {H}x{W} PNG (18 train / 2 val, B=4, bf16, 0 workers): "
    f"epoch 1 (with set-up) {stamps[0] - t0:.2f} s, epoch 2 {stamps[1] - stamps[0]:.2f} s wall")
shutil.rmtree(tmp, ignore_errors=True)
