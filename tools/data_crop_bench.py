"""The load_size crop on the device (profiles/data_crop.txt).  B = 16, 512x640 frames, load
size 286x286, crop 256x256, both modalities: DeviceResizer with load_size (the *_crop
entries compute the window alone) against what a user could do without it -- DeviceResizer
at the load size, then a torch slice of each image's window and .contiguous().  Same
offsets and flips for both; HIP events, interleaved, medians.  The alternative applies the
IR max rule and the flip to the whole load-size image (it cannot do otherwise), so only its
RGB output is compared with the crop path's."""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data_crop.txt"))
OUT = ap.parse_args().out
irc = importlib.import_module("infrared-colorization-with-resnet-generator-and-patchgan_amd")
D = irc.data
DEV = "cuda"
assert torch.cuda.is_available(), "this measurement needs the GPU"
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


B, H, W, L, S = 16, 512, 640, 286, 256
rng = np.random.default_rng(0)
ir = torch.from_numpy(rng.integers(0, 256, size=(B, H, W), dtype=np.uint8)).to(DEV)
rgb = torch.from_numpy(rng.integers(0, 256, size=(B, H, W, 3), dtype=np.uint8)).to(DEV)
flip0 = torch.zeros(B, dtype=torch.uint8, device=DEV)
flip = torch.tensor([i % 2 for i in range(B)], dtype=torch.uint8, device=DEV)
offs = rng.integers(0, L - S + 1, size=(B, 2)).astype(np.int32)
crop = torch.from_numpy(offs).to(DEV)
rs_crop = D.DeviceResizer(S, DEV, load_size=L)
rs_full = D.DeviceResizer(L, DEV)
# per-image windows of a (B, C, L, L) tensor as one gather-free stack of slices
win = [(int(oy), int(ox)) for oy, ox in offs]


def crop_path(fl):
    return (rs_crop._one(ir, 1, fl, True, crop=crop, load=(L, L)),
            rs_crop._one(rgb, 3, fl, False, crop=crop, load=(L, L)))


def slice_path(fl):
    out = []
    for u8, C, rule in ((ir, 1, True), (rgb, 3, False)):
        full = rs_full._one(u8, C, fl, rule)
        out.append(torch.stack([full[b, :, oy:oy + S, ox:ox + S] for b, (oy, ox) in enumerate(win)]).contiguous())
    return out


# without a flip the two agree wherever the alternative is right at all: RGB always, IR
# because these frames' maxima exceed 1 in the window and in the load-size image alike
a, b = crop_path(flip0), slice_path(flip0)
assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
say(f"B={B} {H}x{W} -> load {L}x{L} -> crop {S}x{S}: crop entries == full resize + slice, bit for bit (no flip)")
say(f"  destination pixels computed per image: {S * S} against {L * L} ({100.0 * S * S / (L * L):.1f} %)")

forms = {"crop entries": lambda: crop_path(flip), "resize + slice": lambda: slice_path(flip)}
INNER, SAMPLES = 10, 40
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
say(f"us per batch, IR + RGB (HIP events over {INNER} back-to-back batches, output allocation and the img_max "
    f"memset included; {SAMPLES} interleaved samples)")
for k, v in t.items():
    v.sort()
    say(f"  {k:15s} median {statistics.median(v):8.2f}  min {v[0]:8.2f}  p90 {v[int(0.9 * len(v))]:8.2f}")
m = {k: statistics.median(v) for k, v in t.items()}
say(f"  resize + slice / crop entries at the medians: {m['resize + slice'] / m['crop entries']:.2f}x")
say(f"  (per modality the crop form issues 2 kernel launches and the img_max memset; the slice form the same "
    f"at {L}x{L}, then {B} slice views and one stack copy from Python)")
