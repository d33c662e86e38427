"""``load_size`` on the device: DeviceResizer and the three *_crop entries
(irgan_area_resize_crop_u8, irgan_linear_area_resize_crop_u8, irgan_u8_native_crop_to_unit)
against the host path -- resize_area_u8 to the load size, numpy slice, flip, _unit_ir --
bit for bit (torch.equal / np.array_equal, no tolerance): C = 1 with the IR max rule and
C = 3, batch 3, per-image offsets that include (0, 0) and (Hl - h, Wl - w), flips [0, 1, 1]."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLIP = [0, 1, 1]
EINVAL = 1001


def _host(D, src, load, hw, off, flip, ir):
    """One image: (window bytes as CHW uint8, [-1, 1] float CHW) as the host computes them."""
    (h, w), (oy, ox) = hw, off
    K = D.resize_area_u8(src, load)[oy:oy + h, ox:ox + w]
    K = np.ascontiguousarray(K[:, ::-1] if flip else K)
    f = D._unit_ir(K) if ir else np.clip(K.astype(np.float32) / 255.0, 0.0, 1.0)
    K3, f3 = (K[None], f[None]) if K.ndim == 2 else (np.transpose(K, (2, 0, 1)), np.transpose(f, (2, 0, 1)))
    return torch.from_numpy(K3.copy()), torch.from_numpy(f3.copy()) * 2.0 - 1.0


def _sources(src_hw, seed, dark=False):
    """IR (3, H, W) and RGB (3, H, W, 3) uint8.  dark: IR images 0 and 1 hold bytes <= 1 but
    for one 255 at pixel (0, 0)."""
    rng = np.random.default_rng(seed)
    ir = rng.integers(0, 256, size=(3,) + src_hw, dtype=np.uint8)
    if dark:
        ir[:2] = rng.integers(0, 2, size=(2,) + src_hw, dtype=np.uint8)
        ir[:2, 0, 0] = 255
    rgb = rng.integers(0, 256, size=(3,) + src_hw + (3,), dtype=np.uint8)
    return ir, rgb


def _offsets(load, hw, mid):
    return [(0, 0), (load[0] - hw[0], load[1] - hw[1]), mid]


def _check(D, ir, rgb, load_size, load, hw, offs):
    """__call__ on the batch, and _one per modality with the window's bytes."""
    rs = D.DeviceResizer(hw, DEV, load_size=load_size)
    crop = torch.tensor(offs, dtype=torch.int32)
    flip = torch.tensor(FLIP, dtype=torch.uint8)
    out = rs({"ir_u8": torch.from_numpy(ir), "rgb_u8": torch.from_numpy(rgb), "flip": flip, "crop": crop})
    assert out["ir"].shape == (3, 1) + hw and out["rgb"].shape == (3, 3) + hw
    want = {}
    for key, src, isir in (("ir", ir, True), ("rgb", rgb, False)):
        want[key] = [_host(D, src[b], load, hw, offs[b], FLIP[b], isir) for b in range(3)]
        for b in range(3):
            assert torch.equal(out[key][b].cpu(), want[key][b][1]), (key, b)
    for key, src, C, rule in (("ir", ir, 1, True), ("rgb", rgb, 3, False)):
        got, got8 = rs._one(torch.from_numpy(src).to(DEV), C, flip.to(DEV), rule, keep_u8=True, crop=crop.to(DEV),
                            load=load)
        for b in range(3):
            assert torch.equal(got8[b].cpu(), want[key][b][0]), (key, b)
            assert torch.equal(got[b].cpu(), want[key][b][1]), (key, b)
    return out, want


AREA = [((13, 17), (7, 9), (4, 5), (1, 2)),          # non-integer scales on both axes
        ((13, 17), (13, 9), (6, 5), (3, 1)),         # the rows keep their size: the identity table
        ((40, 50), (30, 40), (20, 30), (4, 7))]      # 600 pixels: three blocks, the last ragged


@pytest.mark.parametrize("src_hw,load,hw,mid", AREA)
def test_area_crop(src_hw, load, hw, mid):
    D = pkg().data
    assert load[0] <= src_hw[0] and load[1] <= src_hw[1] and load != src_hw
    ir, rgb = _sources(src_hw, 1)
    _check(D, ir, rgb, load, load, hw, _offsets(load, hw, mid))


def test_linear_crop_spans_xlim():
    """5x6 -> 8x11 (both axes upscale) -> 5x7.  Columns from xlim on take a single tap: the
    windows at ox = 4 hold columns on both sides of it, the one at ox = 0 only two-tap ones."""
    D = pkg().data
    src_hw, load, hw = (5, 6), (8, 11), (5, 7)
    _, _, xlim = D.linear_area_table(src_hw[1], load[1])
    offs = _offsets(load, hw, (1, 4))
    assert offs[1] == (3, 4)
    for oy, ox in offs[1:]:
        assert ox < xlim <= ox + hw[1] - 1, (ox, xlim)
    assert offs[0][1] + hw[1] - 1 < xlim
    ir, rgb = _sources(src_hw, 2)
    _check(D, ir, rgb, load, load, hw, offs)
    # one axis up, one down still takes the linear path
    _check(D, ir, rgb, (8, 4), (8, 4), (5, 3), _offsets((8, 4), (5, 3), (2, 0)))


@pytest.mark.parametrize("ox", [0, 3, 20])
def test_native_crop(ox):
    """11x70 -> 7x50 window of the frame itself: whole 16-pixel runs, clipped units, and (odd
    ox, C = 3) rows whose first aligned pixel differs from row to row."""
    D = pkg().data
    src_hw, hw = (11, 70), (7, 50)
    ir, rgb = _sources(src_hw, 3)
    offs = _offsets(src_hw, hw, (2, ox))
    assert offs[1] == (4, 20)
    _check(D, ir, rgb, "native", src_hw, hw, offs)
    _check(D, ir, rgb, src_hw, src_hw, hw, offs)          # a load size equal to the source: the same pass


def test_native_crop_short_rows():
    """9x23 -> 6x17: rows of 17 and 51 bytes; the uint8 copy (keep_u8) compared too, and the
    float output alone (no uint8 copy)."""
    D = pkg().data
    src_hw, hw = (9, 23), (6, 17)
    ir, rgb = _sources(src_hw, 4)
    offs = _offsets(src_hw, hw, (1, 5))
    out, want = _check(D, ir, rgb, "native", src_hw, hw, offs)
    rs = D.DeviceResizer(hw, DEV, load_size="native")
    crop = torch.tensor(offs, dtype=torch.int32, device=DEV)
    flip = torch.tensor(FLIP, dtype=torch.uint8, device=DEV)
    got = rs._one(torch.from_numpy(rgb).to(DEV), 3, flip, False, crop=crop, load=src_hw)
    assert torch.equal(got, out["rgb"])


@pytest.mark.parametrize("src_hw,load_size,load,hw", [((13, 17), (7, 9), (7, 9), (4, 5)),        # area
                                                      ((5, 6), (8, 11), (8, 11), (5, 7)),        # linear
                                                      ((11, 70), "native", (11, 70), (7, 50)),   # native
                                                      ((9, 23), "native", (9, 23), (6, 17))])
def test_ir_max_rule_sees_the_window(src_hw, load_size, load, hw):
    """IR images 0 and 1: bytes <= 1 but for a 255 at source pixel (0, 0).  Image 0's window
    sits in the far corner and holds only bytes <= 1 while its load-size image does not: it
    must stay undivided (max over the crop, not over the load-size image).  Image 1's window
    at (0, 0) holds the bright pixel: divided.  Image 2 is an ordinary frame."""
    D = pkg().data
    ir, rgb = _sources(src_hw, 5, dark=True)
    far = (load[0] - hw[0], load[1] - hw[1])
    offs = [far, (0, 0), (1, 1)]
    R0 = D.resize_area_u8(ir[0], load)
    assert R0.max() > 1 and R0[far[0]:, far[1]:].max() <= 1 and R0[far[0]:, far[1]:].max() == 1
    assert D.resize_area_u8(ir[1], load)[:hw[0], :hw[1]].max() > 1
    out, want = _check(D, ir, rgb, load_size, load, hw, offs)
    vals = set(np.unique(out["ir"][0].cpu().numpy()).tolist())
    assert vals == {-1.0, 1.0}                                         # bytes 0 and 1 as they are: x * 2 - 1
    top = np.float32(int(want["ir"][1][0].max())) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)
    assert int(want["ir"][1][0].max()) > 1 and float(out["ir"][1].max()) == float(top)   # divided by 255
    # the bare entry's img_max is the window's
    rs = D.DeviceResizer(hw, DEV, load_size=load_size)
    crop = torch.tensor(offs, dtype=torch.int32, device=DEV)
    u8 = torch.from_numpy(ir).to(DEV)
    mx = torch.zeros(3, dtype=torch.int32, device=DEV)
    if load == src_hw:
        o = torch.empty(3, 1, *hw, dtype=torch.float32, device=DEV)
        irc = pkg()
        irc._lib.call("irgan_u8_native_crop_to_unit", irc.ops.P(u8), 3, src_hw[0], src_hw[1], 1,
                      ctypes.c_int64(src_hw[0] * src_hw[1]), irc.ops.P(crop), hw[0], hw[1], None, 1, irc.ops.P(mx),
                      irc.ops.P(o), None, irc.ops.stream())
        got_mx = mx.cpu().tolist()
        assert got_mx == [int(want["ir"][b][0].max()) for b in range(3)]
    else:
        rs.resize_u8(u8, 1, None, mx, crop=crop, load=load)
        got_mx = mx.cpu().tolist()
        # the resizing kernels only report maxima above 1 (what the rule asks)
        assert got_mx == [m if m > 1 else 0 for m in (int(want["ir"][b][0].max()) for b in range(3))]
    assert got_mx[0] <= 1 < got_mx[1]


@pytest.mark.parametrize("src_hw,hw", [((13, 17), (7, 9)), ((5, 6), (8, 11)), ((9, 23), (9, 23))])
def test_plain_entries_unchanged(src_hw, hw):
    """The existing entries, called as before the crop existed (no load_size, no crop in the
    batch), on one small case of each path -- area, linear, native -- against the host."""
    D = pkg().data
    ir, rgb = _sources(src_hw, 6, dark=True)
    flip = torch.tensor(FLIP, dtype=torch.uint8)
    rs = D.DeviceResizer(hw, DEV)
    out = rs({"ir_u8": torch.from_numpy(ir), "rgb_u8": torch.from_numpy(rgb), "flip": flip})
    for key, src, C, isir in (("ir", ir, 1, True), ("rgb", rgb, 3, False)):
        got, got8 = rs._one(torch.from_numpy(src).to(DEV), C, flip.to(DEV), isir, keep_u8=True)
        for b in range(3):
            w8, wf = _host(D, src[b], hw, hw, (0, 0), FLIP[b], isir)
            assert torch.equal(out[key][b].cpu(), wf) and torch.equal(got[b].cpu(), wf), (key, b)
            assert torch.equal(got8[b].cpu(), w8), (key, b)


def test_off_range_offsets_launch_nothing(monkeypatch):
    irc = pkg()
    D = irc.data
    ir, rgb = _sources((13, 17), 7)
    rs = D.DeviceResizer((4, 5), DEV, load_size=(7, 9))
    calls = []
    monkeypatch.setattr(irc._lib, "call", lambda name, *a: calls.append(name))
    batch = {"ir_u8": torch.from_numpy(ir), "rgb_u8": torch.from_numpy(rgb),
             "flip": torch.tensor(FLIP, dtype=torch.uint8)}
    for bad in ([[0, 0], [4, 4], [0, 0]], [[0, 5], [0, 0], [0, 0]], [[0, 0], [0, 0], [-1, 0]], [[0, 0], [0, -1], [3, 4]]):
        with pytest.raises(ValueError, match="offsets"):
            rs(dict(batch, crop=torch.tensor(bad, dtype=torch.int32)))
    assert calls == []
    rs(dict(batch, crop=torch.tensor([[0, 0], [3, 4], [1, 2]], dtype=torch.int32)))   # in range: both modalities
    assert calls == ["irgan_area_resize_crop_u8", "irgan_u8_to_unit"] * 2


def test_bare_entries_refuse_a_bad_window():
    """A null crop, or an output larger than the load size on either axis: IRGAN_EINVAL, and
    the output is untouched.  Empty work returns 0."""
    irc = pkg()
    D = irc.data
    P, st = irc.ops.P, irc.ops.stream
    lib = irc._lib.load()
    N, H, W, C = 2, 13, 17, 3
    Hl, Wl, h, w = 7, 9, 4, 5
    src = torch.zeros(N, H, W, C, dtype=torch.uint8, device=DEV)
    crop = torch.zeros(N, 2, dtype=torch.int32, device=DEV)
    out8 = torch.full((N, C, Hl + 1, Wl + 1), 9, dtype=torch.uint8, device=DEV)
    out = torch.full((N, C, H + 1, W + 1), 7.0, dtype=torch.float32, device=DEV)
    rs = D.DeviceResizer((h, w), DEV, load_size=(Hl, Wl))
    yt, xt = rs._tab(H, Hl), rs._tab(W, Wl)
    stride = ctypes.c_int64(H * W * C)

    def area(cr, ho, wo, n=N):
        return lib.irgan_area_resize_crop_u8(P(src), n, H, W, C, stride, P(yt[0]), P(yt[1]), P(yt[2]), Hl, P(xt[0]),
                                             P(xt[1]), P(xt[2]), Wl, P(cr), ho, wo, None, P(out8), None, st())

    lsrc = torch.zeros(N, 5, 6, C, dtype=torch.uint8, device=DEV)
    yo, yc, _ = rs._ltab(5, 8, False)
    xo, xc, xlim = rs._ltab(6, 11, True)

    def linear(cr, ho, wo, n=N):
        return lib.irgan_linear_area_resize_crop_u8(P(lsrc), n, 5, 6, C, ctypes.c_int64(5 * 6 * C), P(yo), P(yc), 8,
                                                    P(xo), P(xc), xlim, 11, P(cr), ho, wo, None, P(out8), None, st())

    def native(cr, ho, wo, n=N):
        return lib.irgan_u8_native_crop_to_unit(P(src), n, H, W, C, stride, P(cr), ho, wo, None, 0, None, P(out),
                                                None, st())

    for fn, (hl, wl) in ((area, (Hl, Wl)), (linear, (8, 11)), (native, (H, W))):
        assert fn(None, 2, 2) == EINVAL
        assert fn(crop, hl + 1, 2) == EINVAL
        assert fn(crop, 2, wl + 1) == EINVAL
        assert fn(crop, 2, 2, n=0) == 0 and fn(crop, 0, 2) == 0
    torch.cuda.synchronize()
    assert bool((out8 == 9).all()) and bool((out == 7.0).all())
    assert native(crop, h, w) == 0 and area(crop, h, w) == 0 and linear(crop, 5, 7) == 0
    torch.cuda.synchronize()


def _kaist_tree(root, n_img=5, size=(20, 26)):
    rng = np.random.default_rng(8)
    seq = os.path.join(root, "set00", "V000")
    os.makedirs(os.path.join(seq, "lwir"))
    os.makedirs(os.path.join(seq, "visible"))
    for i in range(n_img):
        Image.fromarray(rng.integers(0, 256, size=size, dtype=np.uint8)).save(os.path.join(seq, "lwir", f"I{i:05d}.png"))
        Image.fromarray(rng.integers(0, 256, size=size + (3,), dtype=np.uint8)).save(
            os.path.join(seq, "visible", f"I{i:05d}.png"))
    return os.path.join(root, "set00")


def test_kaist_loader_equals_host_items(tmp_path):
    """One kaist_loader pass (workers in-process) against __getitem__ under the same seed:
    both draw flip, oy, ox per item in order."""
    D = pkg().data
    root = _kaist_tree(str(tmp_path))
    ds = D.KAISTPairDataset(root, img_size=(8, 10), load_size=(12, 15), verbose=False)
    random.seed(9)
    got = list(D.kaist_loader(ds, 3, DEV, shuffle=False, num_workers=0))
    assert [b["ir"].shape for b in got] == [(3, 1, 8, 10), (2, 1, 8, 10)]
    random.seed(9)
    k = 0
    for b in got:
        for j in range(b["ir"].shape[0]):
            ref = ds[k]
            assert torch.equal(b["ir"][j].cpu(), ref["ir"]) and torch.equal(b["rgb"][j].cpu(), ref["rgb"]), k
            k += 1
    assert k == 5
    # the validation view of the same files draws nothing and resizes straight to img_size
    val = D.KAISTPairDataset(root, img_size=(8, 10), augment=False, load_size=(12, 15), verbose=False)
    vb = next(iter(D.kaist_loader(val, 2, DEV)))
    for j in range(2):
        assert torch.equal(vb["ir"][j].cpu(), val[j]["ir"]) and torch.equal(vb["rgb"][j].cpu(), val[j]["rgb"])
