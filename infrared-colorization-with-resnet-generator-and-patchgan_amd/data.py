"""KAIST data pipeline: the reference's image I/O and
paired dataset (ir:803-852, 887-942, 1045-1177) with the per-sample pixel work
moved to the device.

Reference behaviour, per sample in CPU DataLoader workers: cv2.imread ->
cv2.resize(INTER_AREA) to img_size^2 -> float32 / 255 -> paired random
horizontal flip -> x * 2 - 1.  At ~1,000 img/s per GPU that is the bottleneck
(ir:107: 4 workers).  Here:

* ``KAISTPairDataset`` keeps the reference's constructor, pairing rules
  (filename intersection of sibling ``lwir`` / ``visible`` folders, os.walk
  order, ``indices`` subset) and ``__getitem__`` contract ({'ir': 1xHxW,
  'rgb': 3xHxW} float32 in [-1, 1]) -- computed on the host exactly as the
  reference does, for code that indexes the dataset directly;
* ``KAISTPairDataset.raw(i)`` returns only the DECODED uint8 images (+ the flip
  draw), and ``kaist_loader`` collates those into pinned uint8 batches that one
  ``irgan_area_resize_u8`` + one ``irgan_u8_to_unit`` launch per modality turn
  into the [-1, 1] device batch (csrc/data.hip).  ``train_kaist`` uses this path.

``img_size`` is read in one place, ``target_hw``: an int S (the reference's S x S), a
(height, width) pair, or None for each image's own size (the reference loaders'
img_size=None, ir:817, 847).  A rectangular target follows cv::resize's own dispatch
per call (copy / area tables per axis / the linear path when either axis upscales);
at the source size the device path is one ``irgan_u8_native_to_unit`` launch.

``load_size`` (read in one place, ``load_hw``: an int, a (height, width) pair, "native", or
None = off, the default) adds the pix2pix crop jitter to TRAINING samples (augment=True): the
image is resized to the load size, a random ``img_size`` window -- the same (oy, ox) for IR and
RGB, drawn with python ``random`` after the flip draw -- is cut out of it, and flip and float
conversion see that window (the IR max rule of ir:1142 included).  "native" cuts the window
out of the decoded frame.  ``__getitem__`` does that on the host; ``raw`` only draws, and the
``irgan_*_crop_*`` entries compute the window alone on the device, bit for bit the host's.
augment=False (validation, the val split of train_kaist, run_test) ignores ``load_size`` and
resizes straight to ``img_size``; with "native" the validation scale therefore differs from
the training crops'.  With ``load_size=None`` no extra draw is made and nothing changes.

Decoding: OpenCV is not available in this image, so files are decoded with PIL
and converted with cv2's rules (IMREAD_GRAYSCALE: 16-bit PNG -> high byte,
colour -> BGR2GRAY fixed-point weights; IMREAD_COLOR + BGR2RGB).  INTER_AREA is
OpenCV's general area-resize recurrence (computeResizeAreaTab + resizeArea_,
float32, round half to even), restated here and in the kernel with the same
float operation order.  Parity with cv2 itself is UNPINNED (cv2 absent; the
reference ships no decoded fixtures): the host and device paths are pinned to
each other bit for bit, and the area tables to the exact area integral.
"""
from __future__ import annotations

import ctypes
import os
import random

import numpy as np
import torch

from . import _lib
from .ops import P, stream

__all__ = ["EXTS", "target_hw", "parse_img_size", "load_hw", "parse_load_size", "area_table", "linear_area_table", "resize_area_u8", "resize_linear_area_u8", "imread_gray", "imread_rgb", "load_ir_image", "load_rgb_image",
           "collect_kaist_ir_files_from_sets", "scan_kaist_pairs", "KAISTPairDataset", "DeviceResizer",
           "collate_raw", "kaist_loader"]

EXTS = ('.png', '.jpg', '.jpeg', '.bmp', '.tif', '.tiff')   # ir:901, 1072


# ----------------------------------------------------------------------------
# INTER_AREA tables (OpenCV computeResizeAreaTab) and the host resize
# ----------------------------------------------------------------------------

def area_table(ssize: int, dsize: int):
    """Per-axis INTER_AREA table as CSR arrays (ptr [dsize+1], src [k], w [k]):
    destination index d takes sum_{e in ptr[d]..ptr[d+1]-1} w[e] * S[src[e]].

    OpenCV's recurrence for scale = ssize / dsize >= 1 (cv::resize computes the
    scale as 1 / (dsize / ssize) in double): the cell [d*scale, d*scale + scale)
    clipped to the image, partial first / last source pixels weighted by their
    covered fraction, every weight divided by the cell width; entries ordered by
    source index."""
    scale = 1.0 / (dsize / ssize)
    if scale < 1.0:
        raise ValueError("area_table is the downscaling table; upscaling uses linear_area_table")
    ptr, src, w = [0], [], []
    for dx in range(dsize):
        fsx1 = dx * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        if sx1 - fsx1 > 1e-3:
            src.append(sx1 - 1)
            w.append(float(np.float32((sx1 - fsx1) / cell)))
        for sx in range(sx1, sx2):
            src.append(sx)
            w.append(float(np.float32(1.0 / cell)))
        if fsx2 - sx2 > 1e-3:
            src.append(sx2)
            w.append(float(np.float32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        ptr.append(len(src))
    return np.array(ptr, np.int32), np.array(src, np.int32), np.array(w, np.float32)


INTER_RESIZE_COEF_BITS = 11
INTER_RESIZE_COEF_SCALE = 1 << INTER_RESIZE_COEF_BITS


def _cv_round(v):
    return int(np.rint(v))   # cvRound: nearest, ties to even


def linear_area_table(ssize: int, dsize: int, columns: bool = True):
    """Per-axis table of cv2.resize(INTER_AREA) when either axis UPscales: OpenCV then
    runs its linear resampler with "area mode" coefficients (resizeGeneric_ with
    area_mode): source index s = floor(d * scale), fraction
    f = (d + 1) - (s + 1) / scale (as float32), f <= 0 -> 0 else f - floor(f); left /
    right border clamps (s < 0 -> s = 0, f = 0; s >= ssize - 1 -> s = ssize - 1, f = 0);
    8-bit fixed-point weights round((1 - f) * 2048), round(f * 2048).  The border
    clamps are the column table's (columns=True); the row table keeps s and f as
    computed (OpenCV clamps the second source ROW index instead).
    Returns (ofs int32 [dsize], coef int16-valued int32 [dsize][2], lim): destinations
    d >= lim take the single tap S[ofs] * 2048 (OpenCV's xmax; rows never do)."""
    inv = dsize / ssize
    scale = 1.0 / inv
    ofs = np.zeros(dsize, np.int32)
    coef = np.zeros((dsize, 2), np.int32)
    lim = dsize
    for d in range(dsize):
        sx = int(np.floor(d * scale))
        f = float(np.float32((d + 1) - (sx + 1) * inv))
        f = 0.0 if f <= 0 else float(np.float32(f - np.floor(f)))
        if columns and sx < 0:
            f, sx = 0.0, 0
        if columns and sx + 1 >= ssize:
            lim = min(lim, d)
            if sx >= ssize - 1:
                f, sx = 0.0, ssize - 1
        ofs[d] = sx
        c0, c1 = np.float32(1.0) - np.float32(f), np.float32(f)
        coef[d] = (_cv_round(np.float32(c0 * np.float32(INTER_RESIZE_COEF_SCALE))),
                   _cv_round(np.float32(c1 * np.float32(INTER_RESIZE_COEF_SCALE))))
    return ofs, coef, lim


def resize_linear_area_u8(img: np.ndarray, width: int, height: int) -> np.ndarray:
    """cv2.resize(img, (width, height), interpolation=INTER_AREA) for uint8 when either axis
    upscales (OpenCV's generic linear path in 8-bit fixed point): horizontal
    D = S[x0] * a0 + S[x0 + C] * a1 (int32; single tap S[x0] * 2048 from the xmax border
    on), vertical dst = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2 with
    the second row clamped to the image (VResizeLinear<uchar, int, short>)."""
    a = np.asarray(img)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    H, W, C = a.shape
    xo, xc, xlim = linear_area_table(W, width)
    yo, yc, _ = linear_area_table(H, height, columns=False)
    S = a.astype(np.int64)
    x1 = np.minimum(xo + 1, W - 1)
    D = S[:, xo, :] * xc[None, :, 0, None] + S[:, x1, :] * xc[None, :, 1, None]
    D[:, xlim:, :] = S[:, xo[xlim:], :] * INTER_RESIZE_COEF_SCALE
    y1 = np.minimum(yo + 1, H - 1)
    D0, D1 = D[yo], D[y1]
    b0, b1 = yc[:, 0, None, None], yc[:, 1, None, None]
    r = (((b0 * (D0 >> 4)) >> 16) + ((b1 * (D1 >> 4)) >> 16) + 2) >> 2
    r = (r & 0xFF).astype(np.uint8)   # uchar(...) cast, no saturation (as OpenCV)
    return r[:, :, 0] if squeeze else r


def _slots(ptr, src, w):
    """Regroup a CSR table by position-within-run: slot t = the t-th entry of every
    destination that has one (so a vectorised pass adds in the table's order)."""
    n = len(ptr) - 1
    cnt = np.diff(ptr)
    out = []
    for t in range(int(cnt.max())):
        d = np.nonzero(cnt > t)[0]
        e = ptr[d] + t
        out.append((d, src[e], w[e]))
    return out


def _whole(v):
    if isinstance(v, (bool, np.bool_)):
        return None
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)) and float(v).is_integer():
        return int(v)
    return None


def target_hw(img_size, src_hw=None):
    """The one reading of ``img_size`` (Config, the loaders, the datasets, DeviceResizer,
    run_test) -> the (h, w) an image of source size ``src_hw`` is brought to:

    * an int S: (S, S), the reference's square resize (ir:818, 1139);
    * a pair (H, W), tuple or list: HEIGHT FIRST, the order of a (B, C, H, W) tensor's
      last two axes -- the opposite of cv2.resize's dsize, which is (width, height);
    * None: ``src_hw`` itself, each image keeps its size (the loaders' img_size=None,
      ir:817, 847); with no source to be native to (src_hw None) that is an error.

    Integral floats count as ints; anything else raises ValueError."""
    if img_size is None:
        if src_hw is None:
            raise ValueError("img_size=None keeps the source size, and there is no source here")
        return int(src_hw[0]), int(src_hw[1])
    s = _whole(img_size)
    if s is not None:
        hw = (s, s)
    elif isinstance(img_size, (tuple, list)) and len(img_size) == 2:
        hw = (_whole(img_size[0]), _whole(img_size[1]))
    else:
        hw = (None, None)
    if hw[0] is None or hw[1] is None or hw[0] < 1 or hw[1] < 1:
        raise ValueError(f"img_size must be a positive int, a (height, width) pair of them or None, got {img_size!r}")
    return hw


def parse_img_size(text: str):
    """The command line's ``--img-size N | HxW | native`` as an ``img_size`` value."""
    t = text.strip().lower()
    if t == "native":
        return None
    try:
        parts = [int(p) for p in t.split("x")]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2):
        raise ValueError(f"--img-size takes N, HxW (height first) or 'native', got {text!r}")
    size = parts[0] if len(parts) == 1 else tuple(parts)
    target_hw(size)
    return size


def load_hw(load_size, src_hw=None):
    """The one reading of ``load_size`` (Config, KAISTPairDataset, DeviceResizer), the size a
    training image is resized to before a random ``img_size`` window is cut out of it -> the
    (height, width) of that load-size image for a source of size ``src_hw``:

    * an int S or a (height, width) pair: target_hw's forms, height first;
    * the string "native": ``src_hw`` itself, nothing is resampled and the window is cut out
      of the decoded frame; with no source given (src_hw None) that is an error.

    None (the option is off) is not a size: callers test for it first.  Anything else raises
    ValueError."""
    if isinstance(load_size, str):
        if load_size.strip().lower() != "native":
            raise ValueError(f"load_size must be a positive int, a (height, width) pair of them or 'native', "
                             f"got {load_size!r}")
        if src_hw is None:
            raise ValueError("load_size='native' keeps the source size, and there is no source here")
        return int(src_hw[0]), int(src_hw[1])
    if load_size is None:
        raise ValueError("load_size=None turns the crop off; there is no load size to read")
    try:
        return target_hw(load_size)
    except ValueError:
        raise ValueError(f"load_size must be a positive int, a (height, width) pair of them or 'native', "
                         f"got {load_size!r}") from None


def parse_load_size(text: str):
    """The command line's ``--load-size N | HxW | native`` as a ``load_size`` value."""
    t = text.strip().lower()
    if t == "native":
        return "native"
    try:
        parts = [int(p) for p in t.split("x")]
    except ValueError:
        parts = []
    if len(parts) not in (1, 2):
        raise ValueError(f"--load-size takes N, HxW (height first) or 'native', got {text!r}")
    size = parts[0] if len(parts) == 1 else tuple(parts)
    load_hw(size)
    return size


def _check_crop(img_size, load_size):
    """``load_size`` against ``img_size`` as far as it can be judged without a source: a
    malformed value, a crop with no size (img_size None) and an int / pair load size below
    the crop on either axis raise ValueError ('native' is judged per batch, _window)."""
    if load_size is None:
        return
    if img_size is None:
        load_hw(load_size, (1, 1))
        raise ValueError("load_size crops a window of img_size out of the load-size image: it needs an img_size, "
                         "not None")
    h, w = target_hw(img_size)
    lh, lw = load_hw(load_size, (h, w))
    if lh < h or lw < w:
        raise ValueError(f"load_size {lh}x{lw} is smaller than img_size {h}x{w}: the crop does not fit")


def _window(img_size, load_size, ir_hw, rgb_hw):
    """((Hl, Wl), (h, w)): the load-size image the IR and RGB sources of sizes ``ir_hw`` /
    ``rgb_hw`` are brought to, and the window cut out of it.  'native' sources that differ
    from each other or are smaller than the window raise RuntimeError."""
    h, w = target_hw(img_size)
    L, Lr = load_hw(load_size, ir_hw), load_hw(load_size, rgb_hw)
    if L != Lr:
        raise RuntimeError(f"load_size='native' crops each frame at its own size, but the IR frames are "
                           f"{L[0]}x{L[1]} and the RGB frames {Lr[0]}x{Lr[1]}: one window cannot serve both -- "
                           "give a load_size")
    if L[0] < h or L[1] < w:
        raise RuntimeError(f"load_size='native': the frames are {L[0]}x{L[1]}, smaller than the "
                           f"{h}x{w} crop (img_size)")
    return L, (h, w)


def resize_area_u8(img: np.ndarray, size) -> np.ndarray:
    """cv2.resize(img, (w, h), interpolation=INTER_AREA) for uint8 HxW or HxWxC input,
    host side, with (h, w) = target_hw(size, img.shape[:2]) -- note the order: ``size``
    is an int or (HEIGHT, WIDTH), cv2's dsize is (width, height).  cv::resize's dispatch:
    a target equal to the source size returns a copy (dsize == ssize); both axes with
    scale >= 1 take OpenCV's area path, each axis with its own table: float32 in
    OpenCV's operation order -- per destination row, each source row of its cell
    reduced horizontally (buf = 0 + a0*S0 + a1*S1 ...), then sum = b0*buf0 + b1*buf1
    ..., rounded half to even and clamped to uint8; either axis upscaling sends the whole
    image through resize_linear_area_u8."""
    a = np.asarray(img)
    h, w = target_hw(size, a.shape[:2])
    if (h, w) == tuple(a.shape[:2]):
        return a.copy()
    if a.shape[0] < h or a.shape[1] < w:
        return resize_linear_area_u8(a, w, h)
    squeeze = a.ndim == 2
    if squeeze:
        a = a[:, :, None]
    H, W, C = a.shape
    yt = _slots(*area_table(H, h))
    xt = _slots(*area_table(W, w))
    S = a.astype(np.float32)
    # horizontal pass for every source row: (H, w, C)
    buf = np.zeros((H, w, C), np.float32)
    for d, s, wt in xt:
        buf[:, d, :] = buf[:, d, :] + S[:, s, :] * wt[None, :, None]
    out = np.zeros((h, w, C), np.float32)
    for t, (d, s, wt) in enumerate(yt):
        term = buf[s, :, :] * wt[:, None, None]
        out[d] = term if t == 0 else out[d] + term
    r = np.clip(np.rint(out), 0, 255).astype(np.uint8)
    return r[:, :, 0] if squeeze else r


# ----------------------------------------------------------------------------
# decoding (cv2.imread semantics through PIL) and the reference loaders
# ----------------------------------------------------------------------------

def imread_gray(path) -> np.ndarray:
    """cv2.imread(path, IMREAD_GRAYSCALE) -> HxW uint8 (ir:812, 1134).  16-bit
    sources keep their high byte (libpng strip-16, as OpenCV's PNG decoder
    without IMREAD_ANYDEPTH).  JPEG: OpenCV asks libjpeg for JCS_GRAYSCALE, i.e. the
    decoded Y plane itself -- PIL's draft('L') mode does the same (no YCbCr -> RGB ->
    gray round trip).  Other colour sources (PNG / BMP / TIFF): cvtColor's BGR2GRAY
    fixed-point weights (4899, 9617, 1868) / 2^14 with rounding."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("I;16", "I;16B", "I;16L", "I"):   # 16-bit source
            return (np.asarray(im).astype(np.uint32) >> 8).astype(np.uint8)
        if im.format == "JPEG" and im.mode != "L":
            im.draft("L", im.size)                        # libjpeg's grayscale output (Y)
        if im.mode == "L":
            return np.asarray(im).copy()
        rgb = np.asarray(im.convert("RGB")).astype(np.uint32)
    g = (rgb[..., 0] * 4899 + rgb[..., 1] * 9617 + rgb[..., 2] * 1868 + (1 << 13)) >> 14
    return g.astype(np.uint8)


def imread_rgb(path) -> np.ndarray:
    """cv2.imread(path, IMREAD_COLOR) + cvtColor(BGR2RGB) -> HxWx3 uint8 (ir:842-845)."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode in ("I;16", "I;16B", "I;16L", "I"):
            g = (np.asarray(im).astype(np.uint32) >> 8).astype(np.uint8)
            return np.repeat(g[:, :, None], 3, axis=2)
        return np.asarray(im.convert("RGB")).copy()


def _unit_ir(img_u8: np.ndarray) -> np.ndarray:
    img = img_u8.astype(np.float32)
    if img.max() > 1.0:          # ir:823-827 (imread GRAYSCALE always yields uint8)
        img /= 255.0
    return np.clip(img, 0.0, 1.0)


def load_ir_image(path, img_size=None):
    """ir:803-830: HxW float32 in [0, 1], INTER_AREA-resized to ``img_size`` (target_hw's
    forms; None, the default, keeps the source size)."""
    return _unit_ir(resize_area_u8(imread_gray(path), img_size))


def load_rgb_image(path, img_size=None):
    """ir:833-852: HxWx3 float32 RGB in [0, 1], INTER_AREA-resized to ``img_size``
    (target_hw's forms; None, the default, keeps the source size)."""
    return np.clip(resize_area_u8(imread_rgb(path), img_size).astype(np.float32) / 255.0, 0.0, 1.0)


def _list_imgs(folder):
    if not os.path.isdir(folder):
        return {}
    return {fn: os.path.join(folder, fn) for fn in os.listdir(folder) if fn.lower().endswith(EXTS)}


def collect_kaist_ir_files_from_sets(set_roots):
    """ir:887-942: [(ir_path, set_name, seq_rel)] for every image of every 'lwir'
    folder that has a sibling 'visible' folder (os.walk order, files sorted)."""
    if isinstance(set_roots, (str, bytes)):
        set_roots = [set_roots]
    entries = []
    for root in set_roots:
        if not os.path.isdir(root):
            print(f"[WARN] set root not found: {root}")
            continue
        set_name = os.path.basename(root.rstrip("\\/"))
        for dirpath, _, _ in os.walk(root):
            if os.path.basename(dirpath).lower() != "lwir":
                continue
            seq_dir = os.path.dirname(dirpath)
            if not os.path.isdir(os.path.join(seq_dir, "visible")):
                continue
            files = sorted(_list_imgs(dirpath).values())
            seq_rel = os.path.relpath(seq_dir, root)
            entries += [(p, set_name, seq_rel) for p in files]
    return entries


def scan_kaist_pairs(roots):
    """KAISTPairDataset's pairing (ir:1067-1117): per 'lwir' folder with a sibling
    'visible' folder, the sorted filename intersection; roots in order."""
    roots = list(roots) if isinstance(roots, (list, tuple)) else [roots]
    ir_paths, rgb_paths = [], []
    for one in roots:
        if not os.path.isdir(one):
            continue
        for dirpath, _, _ in os.walk(one):
            if os.path.basename(dirpath).lower() != "lwir":
                continue
            vis = os.path.join(os.path.dirname(dirpath), "visible")
            if not os.path.isdir(vis):
                continue
            irm, rgbm = _list_imgs(dirpath), _list_imgs(vis)
            for fn in sorted(set(irm) & set(rgbm)):
                ir_paths.append(irm[fn])
                rgb_paths.append(rgbm[fn])
    if not ir_paths:
        raise RuntimeError(f"No IR-RGB pairs found under roots: {roots}")
    return ir_paths, rgb_paths


class KAISTPairDataset(torch.utils.data.Dataset):
    """ir:1045-1177 with the reference's signature and item contract; see the
    module docstring for the device path (``raw`` + ``kaist_loader``).  ``img_size``:
    target_hw's forms -- an int, (height, width), or None for each pair's own size.
    ``load_size`` (load_hw's forms; None, the default: off) is the paired random-crop jitter
    of a training dataset: each image is resized to the load size and a random ``img_size``
    window of it, the same for IR and RGB, is the sample; augment=False ignores it."""

    def __init__(self, root, img_size=256, augment=True, indices=None, verbose=True, load_size=None):
        super().__init__()
        target_hw(img_size, (1, 1))   # reject a malformed size here, not in a worker
        _check_crop(img_size, load_size)
        self.img_size, self.augment, self.load_size = img_size, augment, load_size
        all_ir, all_rgb = scan_kaist_pairs(root)
        if indices is not None:
            self.ir_paths = [all_ir[i] for i in indices]
            self.rgb_paths = [all_rgb[i] for i in indices]
        else:
            self.ir_paths, self.rgb_paths = all_ir, all_rgb
        if verbose:
            print(f"[KAISTPairDataset] total pairs: {len(self.ir_paths)} (augment={self.augment})")

    def __len__(self):
        return len(self.ir_paths)

    def _flip(self):
        return bool(self.augment and random.random() < 0.5)   # ir:1166, python RNG in the worker

    def _crop(self, ir_hw, rgb_hw):
        """The crop draw of a training sample with a load_size: ((Hl, Wl), (h, w), (oy, ox)),
        python RNG in the worker, after the flip draw; None (and no draw) otherwise."""
        if not self.augment or self.load_size is None:
            return None
        L, (h, w) = _window(self.img_size, self.load_size, ir_hw, rgb_hw)
        oy = random.randint(0, L[0] - h)
        ox = random.randint(0, L[1] - w)
        return L, (h, w), (oy, ox)

    def __getitem__(self, idx):
        ir8, rgb8 = imread_gray(self.ir_paths[idx]), imread_rgb(self.rgb_paths[idx])
        flip = self._flip()
        crop = self._crop(ir8.shape[:2], rgb8.shape[:2])
        if crop is None:
            ir8, rgb8 = resize_area_u8(ir8, self.img_size), resize_area_u8(rgb8, self.img_size)
        else:   # resize to the load size, keep the window; the IR max rule sees the window
            L, (h, w), (oy, ox) = crop
            ir8 = resize_area_u8(ir8, L)[oy:oy + h, ox:ox + w]
            rgb8 = resize_area_u8(rgb8, L)[oy:oy + h, ox:ox + w]
        ir = _unit_ir(ir8)
        rgb = np.clip(rgb8.astype(np.float32) / 255.0, 0.0, 1.0)
        if flip:
            ir = np.fliplr(ir).copy()
            rgb = np.fliplr(rgb).copy()
        ir_t = torch.from_numpy(ir).unsqueeze(0)
        rgb_t = torch.from_numpy(np.transpose(rgb, (2, 0, 1)).copy())
        return {"ir": ir_t * 2.0 - 1.0, "rgb": rgb_t * 2.0 - 1.0}

    def raw(self, idx):
        """Decoded full-resolution uint8 images, the flip draw and, for a training sample
        with a load_size, the crop draw ``"crop": (oy, ox)``: the host half of the device
        path (resize / crop / flip / normalisation run in csrc/data.hip)."""
        ir8, rgb8 = imread_gray(self.ir_paths[idx]), imread_rgb(self.rgb_paths[idx])
        item = {"ir_u8": torch.from_numpy(ir8), "rgb_u8": torch.from_numpy(rgb8), "flip": int(self._flip())}
        crop = self._crop(ir8.shape[:2], rgb8.shape[:2])
        if crop is not None:
            item["crop"] = crop[2]
        return item


class _RawView(torch.utils.data.Dataset):
    def __init__(self, ds):
        self.ds = ds

    def __len__(self):
        return len(self.ds)

    def __getitem__(self, i):
        if isinstance(self.ds, torch.utils.data.Subset):
            return self.ds.dataset.raw(self.ds.indices[i])
        return self.ds.raw(i)


def collate_raw(items):
    """Stack decoded items into uint8 batches (pinned by the DataLoader).  Each modality
    needs one source size within the batch (one resize launch per modality); the IR and
    RGB sources may differ (the reference resizes each image on its own, ir:1139, 1156).
    Items that carry a crop draw (KAISTPairDataset.raw with a load_size) add ``"crop"``, the
    draws as an int32 (B, 2) tensor of (oy, ox); without them the key is absent."""
    for key in ("ir_u8", "rgb_u8"):
        shapes = {tuple(it[key].shape[:2]) for it in items}
        if len(shapes) != 1:
            raise RuntimeError(f"a device batch needs one {key[:-3]} source size, got {sorted(shapes)}")
    batch = {"ir_u8": torch.stack([it["ir_u8"] for it in items]),
             "rgb_u8": torch.stack([it["rgb_u8"] for it in items]),
             "flip": torch.tensor([it["flip"] for it in items], dtype=torch.uint8)}
    if any("crop" in it for it in items):
        batch["crop"] = torch.tensor([it["crop"] for it in items], dtype=torch.int32).reshape(len(items), 2)
    return batch


class DeviceResizer:
    """uint8 decoded batch -> {'ir': (B,1,h,w), 'rgb': (B,3,h,w)} float32 [-1, 1] on
    the device, (h, w) = target_hw(img_size, source size): per modality one
    area-resize+flip launch and one normalisation launch (the IR max rule of ir:1142
    included), or, where the target is the source size, the single native pass
    (irgan_u8_native_to_unit).  Tables cached per (source n, target n).

    ``load_size`` (load_hw's forms; None: off): a batch that carries ``"crop"`` (collate_raw:
    the training samples of a dataset with a load_size) is resized to the load size and only
    its (h, w) window at each image's (oy, ox) is computed -- the same dispatch, applied to
    source -> load size, through the *_crop entries; tables per (source n, load n).  A batch
    without ``"crop"`` (validation) goes straight to img_size as above."""

    def __init__(self, img_size, device, load_size=None):
        target_hw(img_size, (1, 1))
        _check_crop(img_size, load_size)
        self.img_size, self.load_size, self.device = img_size, load_size, torch.device(device)
        self._tabs = {}

    def _tab(self, n, d):
        t = self._tabs.get((n, d))
        if t is None:
            t = self._tabs[(n, d)] = tuple(torch.from_numpy(a).to(self.device) for a in area_table(n, d))
        return t

    def _ltab(self, n, d, columns):
        key = ("lin", n, d, columns)
        t = self._tabs.get(key)
        if t is None:
            ofs, coef, lim = linear_area_table(n, d, columns)
            t = self._tabs[key] = (torch.from_numpy(ofs).to(self.device), torch.from_numpy(coef).to(self.device), lim)
        return t

    def resize_u8(self, u8, C, flip=None, img_max=None, hw=None, crop=None, load=None):
        """(B,H,W[,C]) uint8 device batch -> (B,C,h,w) uint8 (cv2.resize INTER_AREA,
        optional per-image horizontal flip).  ``hw`` overrides the resizer's own target
        (run_test: the ground truth goes to its prediction's size).  ``crop`` (int32 (B, 2)
        device tensor of (oy, ox), with ``load`` = (Hl, Wl)): the resize goes to ``load`` and
        the result is its (h, w) window at each image's offset."""
        if u8.dtype != torch.uint8 or not u8.is_cuda:
            raise ValueError("resize_u8 takes a uint8 device tensor")
        u8 = u8.contiguous()
        B, H, W = u8.shape[:3]
        h, w = hw if hw is not None else target_hw(self.img_size, (H, W))
        Hl, Wl = load if crop is not None else (h, w)   # the size the tables resize to
        win = () if crop is None else (P(crop), h, w)
        out8 = torch.empty(B, C, h, w, dtype=torch.uint8, device=self.device)
        if H < Hl or W < Wl:   # an upscaling axis: OpenCV's linear path with area coefficients
            yo, yc, _ = self._ltab(H, Hl, False)
            xo, xc, xlim = self._ltab(W, Wl, True)
            _lib.call("irgan_linear_area_resize_u8" if crop is None else "irgan_linear_area_resize_crop_u8", P(u8), B,
                      H, W, C, ctypes.c_int64(H * W * C), P(yo), P(yc), Hl, P(xo), P(xc), xlim, Wl, *win,
                      P(flip) if flip is not None else None, P(out8),
                      P(img_max) if img_max is not None else None, stream())
            return out8
        yp, ys, yw = self._tab(H, Hl)   # (an axis that keeps its size: the identity table, unit weights)
        xp, xs, xw = self._tab(W, Wl)
        _lib.call("irgan_area_resize_u8" if crop is None else "irgan_area_resize_crop_u8", P(u8), B, H, W, C,
                  ctypes.c_int64(H * W * C), P(yp), P(ys), P(yw), Hl, P(xp), P(xs), P(xw), Wl, *win,
                  P(flip) if flip is not None else None, P(out8),
                  P(img_max) if img_max is not None else None, stream())
        return out8

    def _one(self, u8, C, flip, max_rule, keep_u8=False, crop=None, load=None):
        """(B,C,h,w) float32 [-1, 1]; keep_u8: also the resized uint8 batch (what the
        reference's loaders hold before their float conversion).  ``crop`` / ``load``: as
        resize_u8 (the resized batch is then the window)."""
        B, H, W = u8.shape[:3]
        h, w = target_hw(self.img_size, (H, W))
        Hl, Wl = load if crop is not None else (h, w)
        mx = torch.zeros(B, dtype=torch.int32, device=self.device)
        out = torch.empty(B, C, h, w, dtype=torch.float32, device=self.device)
        if (Hl, Wl) == (H, W):   # nothing to resize: uint8 NHWC -> float NCHW in one pass
            if u8.dtype != torch.uint8 or not u8.is_cuda:
                raise ValueError("the device path takes a uint8 device tensor")
            u8 = u8.contiguous()
            out8 = torch.empty(B, C, h, w, dtype=torch.uint8, device=self.device) if keep_u8 else None
            win = () if crop is None else (P(crop), h, w)
            _lib.call("irgan_u8_native_to_unit" if crop is None else "irgan_u8_native_crop_to_unit", P(u8), B, H, W, C,
                      ctypes.c_int64(H * W * C), *win, P(flip) if flip is not None else None, int(max_rule), P(mx),
                      P(out), P(out8) if keep_u8 else None, stream())
            return (out, out8) if keep_u8 else out
        out8 = self.resize_u8(u8, C, flip, mx, crop=crop, load=load)
        _lib.call("irgan_u8_to_unit", P(out8), B, ctypes.c_int64(C * h * w), P(mx), int(max_rule), P(out), stream())
        return (out, out8) if keep_u8 else out

    def _crop_of(self, batch):
        """The batch's crop draws, checked on the host: ((Hl, Wl), int32 (B, 2) CPU tensor),
        or (None, None) for a batch without them.  Nothing has touched the device yet."""
        if "crop" not in batch:
            return None, None
        if self.load_size is None:
            raise ValueError("this batch carries crop offsets, but the resizer has no load_size to crop from")
        L, (h, w) = _window(self.img_size, self.load_size, batch["ir_u8"].shape[1:3], batch["rgb_u8"].shape[1:3])
        crop = torch.as_tensor(batch["crop"]).to("cpu", torch.int32)
        B = batch["ir_u8"].shape[0]
        if tuple(crop.shape) != (B, 2):
            raise ValueError(f"crop must hold one (oy, ox) per image, shape ({B}, 2), got {tuple(crop.shape)}")
        oy, ox = crop[:, 0], crop[:, 1]
        if int(oy.min()) < 0 or int(oy.max()) > L[0] - h or int(ox.min()) < 0 or int(ox.max()) > L[1] - w:
            raise ValueError(f"crop offsets {crop.tolist()} leave the {L[0]}x{L[1]} load-size image: a {h}x{w} window "
                             f"needs 0 <= oy <= {L[0] - h}, 0 <= ox <= {L[1] - w}")
        return L, crop.contiguous()

    def __call__(self, batch):
        load, crop = self._crop_of(batch)
        hw_ir = target_hw(self.img_size, batch["ir_u8"].shape[1:3])
        hw_rgb = target_hw(self.img_size, batch["rgb_u8"].shape[1:3])
        if hw_ir != hw_rgb:
            raise RuntimeError(f"img_size=None keeps each image's own size, but this batch's IR frames are "
                               f"{hw_ir[0]}x{hw_ir[1]} and its RGB frames {hw_rgb[0]}x{hw_rgb[1]}: such a pair "
                               "cannot be stacked for the loss -- give an img_size")
        ir8 = batch["ir_u8"].to(self.device, non_blocking=True).contiguous()
        rgb8 = batch["rgb_u8"].to(self.device, non_blocking=True).contiguous()
        flip = batch["flip"].to(self.device, non_blocking=True)
        if crop is not None:
            crop = crop.to(self.device, non_blocking=True)
        return {"ir": self._one(ir8, 1, flip, True, crop=crop, load=load),
                "rgb": self._one(rgb8, 3, flip, False, crop=crop, load=load)}


class _DeviceLoader:
    def __init__(self, loader, fn):
        self.loader, self.fn = loader, fn

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for b in self.loader:
            yield self.fn(b)


def kaist_loader(dataset: KAISTPairDataset, batch_size, device, shuffle=False, drop_last=False, num_workers=0,
                 sampler=None):
    """DataLoader over ``dataset.raw`` (workers decode only) whose batches are
    resized / flipped / normalised on ``device`` (DeviceResizer) to ``dataset.img_size``
    (target_hw's forms; None: the batch's own size, one size per batch by collate_raw).
    A training dataset's ``load_size`` comes along: its batches carry the crop draws and the
    device computes only the window (augment=False draws none and resizes as above)."""
    base = dataset.dataset if isinstance(dataset, torch.utils.data.Subset) else dataset
    dl = torch.utils.data.DataLoader(_RawView(dataset), batch_size=batch_size, shuffle=shuffle and sampler is None,
                                     sampler=sampler, num_workers=num_workers, collate_fn=collate_raw,
                                     pin_memory=torch.device(device).type == "cuda", drop_last=drop_last)
    return _DeviceLoader(dl, DeviceResizer(base.img_size, device, load_size=base.load_size))
