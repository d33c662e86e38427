"""Rectangular and native-resolution ``img_size``, host side (ir:803-852, 1132-1177):
the one size vocabulary (data.target_hw), cv::resize's dispatch restated for an
(h, w) target -- copy at the source size, per-axis area tables when both scales are
>= 1, the linear path as soon as either axis upscales -- the loaders, the datasets and
the command line.  cv2 is not importable here, so parity with OpenCV itself stays
unpinned; the area path is pinned to the exact fp64 area average."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import PKG_NAME, pkg


@pytest.fixture(scope="module")
def D():
    return pkg().data


# ---------------------------------------------------------------- the size helper

def test_target_hw_three_forms(D):
    assert D.target_hw(256, (512, 640)) == (256, 256)
    assert D.target_hw(256) == (256, 256)
    assert D.target_hw(np.int64(32), (5, 5)) == (32, 32)
    assert D.target_hw(32.0) == (32, 32)                      # an integral float is an int
    assert D.target_hw((512, 640), (100, 100)) == (512, 640)  # height first
    assert D.target_hw([24, 40]) == (24, 40)
    assert D.target_hw((np.int32(24), 40.0)) == (24, 40)
    assert D.target_hw(None, (512, 640)) == (512, 640)
    assert D.target_hw(None, torch.Size([37, 61])) == (37, 61)
    assert all(isinstance(v, int) for v in D.target_hw(None, np.zeros((7, 9, 3)).shape[:2]))


@pytest.mark.parametrize("bad", [0, -3, (0, 4), (4, -1), (1, 2, 3), (5,), (), 2.5, (4, 2.5), "256", "4x5",
                                 (None, 4), True, {4, 5}, np.zeros(2)])
def test_target_hw_rejects(D, bad):
    with pytest.raises(ValueError):
        D.target_hw(bad, (8, 8))


def test_target_hw_native_needs_a_source(D):
    with pytest.raises(ValueError):
        D.target_hw(None)
    irc = pkg()
    with pytest.raises(ValueError):
        irc.SyntheticPairDataset(3, img_size=None)


# ---------------------------------------------------------------- host resize

@pytest.mark.parametrize("shape,s", [((48, 60, 3), 24), ((48, 60), 20),       # both axes down
                                     ((48, 60, 3), 96), ((48, 60), 61),       # both axes up
                                     ((48, 60, 3), 50), ((48, 60), 48), ((48, 60, 3), 60)])   # mixed / one axis kept
def test_square_pair_equals_int(D, shape, s):
    a = np.random.default_rng(2).integers(0, 256, size=shape, dtype=np.uint8)
    assert np.array_equal(D.resize_area_u8(a, (s, s)), D.resize_area_u8(a, s))
    assert np.array_equal(D.resize_area_u8(a, [s, s]), D.resize_area_u8(a, s))


@pytest.mark.parametrize("shape", [(48, 60, 3), (48, 60), (37, 61, 3)])
def test_target_equal_to_source_returns_the_bytes(D, shape):
    a = np.random.default_rng(3).integers(0, 256, size=shape, dtype=np.uint8)
    for size in (shape[:2], list(shape[:2]), None):
        r = D.resize_area_u8(a, size)
        assert r.dtype == np.uint8 and np.array_equal(r, a)
        assert r is not a and not np.shares_memory(r, a)       # a copy, as OpenCV's dsize == ssize
    sq = a[:37, :37]
    assert np.array_equal(D.resize_area_u8(sq, 37), sq)


def overlap_matrix(n_in, n_out):
    """fp64 weights of the exact area average: destination d covers [d*s, (d+1)*s) of the
    source axis, each source pixel weighted by the length of its overlap / s."""
    s = n_in / n_out
    M = np.zeros((n_out, n_in))
    for d in range(n_out):
        lo, hi = d * s, (d + 1) * s
        for k in range(n_in):
            M[d, k] = max(0.0, min(hi, k + 1) - max(lo, k)) / s
    return M


SRC = np.random.default_rng(4).integers(0, 256, size=(48, 60, 3), dtype=np.uint8)


@pytest.mark.parametrize("hw", [(24, 40), (40, 24), (48, 30)])
def test_rect_area_path_vs_exact_area_average(D, hw):
    """Each case has its own scale per axis ((48, 30) keeps the rows: the identity table);
    h != w, so a swap of height and width fails on the shape alone.  Bound: a correctly
    rounded byte is within 0.5 of the exact average, and float32 accumulation of at most
    255 * n terms moves the sum by far less than 2^-10."""
    h, w = hw
    got = D.resize_area_u8(SRC, hw)
    assert got.shape == (h, w, 3) and got.dtype == np.uint8
    ref = np.einsum("yh,hwc,xw->yxc", overlap_matrix(48, h), SRC.astype(np.float64), overlap_matrix(60, w))
    err = np.abs(got.astype(np.float64) - ref).max()
    print(f"rect area {hw}: max |byte - exact| = {err:.6f}")
    assert err <= 0.5 + 2.0 ** -10
    g2 = D.resize_area_u8(SRC[:, :, 1], hw)                    # HxW input: same bytes
    assert g2.shape == (h, w) and np.array_equal(g2, got[:, :, 1])


def test_rect_area_equals_square_function_on_square_crop(D):
    a = SRC[:48, :48]
    assert np.array_equal(D.resize_area_u8(a, (24, 24)), D.resize_area_u8(a, 24))


@pytest.mark.parametrize("hw", [(64, 40), (40, 64), (96, 120), (48, 61)])
def test_either_axis_upscaling_takes_the_linear_path(D, hw):
    """48x60 -> (64, 40): the rows upscale, so the whole image leaves the area path
    (cv::resize does so when either scale is below 1)."""
    h, w = hw
    got = D.resize_area_u8(SRC, hw)
    assert got.shape == (h, w, 3)
    assert np.array_equal(got, D.resize_linear_area_u8(SRC, w, h))


# ---------------------------------------------------------------- loaders and datasets

def _tree(root, size=(40, 56), n=3):
    rng = np.random.default_rng(6)
    seq = os.path.join(root, "set00", "V000")
    os.makedirs(os.path.join(seq, "lwir"))
    os.makedirs(os.path.join(seq, "visible"))
    out = []
    for i in range(n):
        ir = rng.integers(0, 256, size=size, dtype=np.uint8)
        rgb = rng.integers(0, 256, size=size + (3,), dtype=np.uint8)
        Image.fromarray(np.repeat(ir[:, :, None], 3, 2)).save(os.path.join(seq, "lwir", f"I{i:05d}.png"))
        Image.fromarray(rgb).save(os.path.join(seq, "visible", f"I{i:05d}.png"))
        out.append((ir, rgb))
    return os.path.join(root, "set00"), out


def test_dataset_rectangular_and_native(D, tmp_path):
    root, imgs = _tree(str(tmp_path))
    ds = D.KAISTPairDataset(root, img_size=(24, 40), augment=False, verbose=False)
    for i, (ir, rgb) in enumerate(imgs):
        it = ds[i]
        assert it["ir"].shape == (1, 24, 40) and it["rgb"].shape == (3, 24, 40)
        want = D.resize_area_u8(rgb, (24, 40)).astype(np.float32) / 255.0
        assert torch.equal(it["rgb"], torch.from_numpy(np.transpose(want, (2, 0, 1)).copy()) * 2.0 - 1.0)
    nat = D.KAISTPairDataset(root, img_size=None, augment=False, verbose=False)
    for i, (ir, rgb) in enumerate(imgs):
        it = nat[i]
        assert it["ir"].shape == (1, 40, 56) and it["rgb"].shape == (3, 40, 56)
        assert torch.equal(it["ir"][0], torch.from_numpy(ir.astype(np.float32) / 255.0) * 2.0 - 1.0)
        assert torch.equal(it["rgb"], torch.from_numpy(
            np.transpose(rgb.astype(np.float32) / 255.0, (2, 0, 1)).copy()) * 2.0 - 1.0)
    with pytest.raises(ValueError):
        D.KAISTPairDataset(root, img_size=(24, 40, 3), verbose=False)


def test_loaders_take_the_three_forms(D, tmp_path):
    root, imgs = _tree(str(tmp_path), n=1)
    ir_p = os.path.join(root, "V000", "lwir", "I00000.png")
    rgb_p = os.path.join(root, "V000", "visible", "I00000.png")
    ir, rgb = imgs[0]
    assert np.array_equal(D.load_ir_image(ir_p), ir.astype(np.float32) / 255.0)
    assert np.array_equal(D.load_rgb_image(rgb_p, None), rgb.astype(np.float32) / 255.0)
    assert D.load_ir_image(ir_p, (24, 40)).shape == (24, 40)
    assert np.array_equal(D.load_rgb_image(rgb_p, (24, 40)), D.resize_area_u8(rgb, (24, 40)).astype(np.float32) / 255.0)
    assert np.array_equal(D.load_ir_image(ir_p, 20), D.load_ir_image(ir_p, (20, 20)))


def test_synthetic_pairs_rectangular():
    irc = pkg()
    ds = irc.SyntheticPairDataset(3, img_size=(32, 48), seed=5)
    assert ds[0]["ir"].shape == (1, 32, 48) and ds[2]["rgb"].shape == (3, 32, 48)
    sq, pair = irc.SyntheticPairDataset(2, img_size=16, seed=5), irc.SyntheticPairDataset(2, img_size=[16, 16], seed=5)
    assert torch.equal(sq[1]["rgb"], pair[1]["rgb"])


def test_collage_panels_are_h_by_w():
    irc = pkg()
    rng = np.random.default_rng(8)
    ir01 = rng.random((32, 48), dtype=np.float32)
    pred = rng.integers(0, 256, size=(32, 48, 3), dtype=np.uint8)
    gt01 = rng.random((32, 48, 3), dtype=np.float32)
    c = irc.make_comparison_collage(ir01, pred, gt01, add_text=False, pad=8)
    assert c.shape == (32, 3 * 48 + 16, 3)
    assert np.array_equal(c[:, 56:104], pred) and not c[:, 48:56].any()


def test_command_line_img_size(D):
    import importlib
    m = importlib.import_module(PKG_NAME + ".__main__")
    assert m.config_from_argv([]).img_size == 256 and m.config_from_argv([]).mode == "test"
    cfg = m.config_from_argv(["train", "--img-size", "512x640"])
    assert cfg.mode == "train" and cfg.img_size == (512, 640)
    assert m.config_from_argv(["--img-size", "128"]).img_size == 128
    assert m.config_from_argv(["test", "--img-size", "native"]).img_size is None
    for bad in ("0", "4x5x6", "big", "4x", "-2x4"):
        with pytest.raises(ValueError):
            D.parse_img_size(bad)
