"""``load_size``, the paired random-crop jitter, host side: the one reader (data.load_hw),
the errors raised before any GPU work, KAISTPairDataset.__getitem__ against resize -> slice
-> flip -> convert done by hand with the same draws, the untouched flip stream of a dataset
without the option, augment=False, collate_raw, Config and the command line."""
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import PKG_NAME, pkg


@pytest.fixture(scope="module")
def D():
    return pkg().data


# ---------------------------------------------------------------- the reader and its errors

def test_load_hw_forms(D):
    assert D.load_hw(286) == (286, 286)
    assert D.load_hw(286, (512, 640)) == (286, 286)
    assert D.load_hw((300, 360)) == (300, 360)               # height first, as img_size
    assert D.load_hw([np.int32(12), 15.0]) == (12, 15)
    assert D.load_hw("native", (512, 640)) == (512, 640)
    assert D.load_hw(" Native ", torch.Size([37, 61])) == (37, 61)
    assert all(isinstance(v, int) for v in D.load_hw("native", np.zeros((7, 9)).shape))


@pytest.mark.parametrize("bad", [0, -3, (0, 4), (1, 2, 3), 2.5, "286", "4x5", "nativ", True, None, {4, 5}])
def test_load_hw_rejects(D, bad):
    with pytest.raises(ValueError):
        D.load_hw(bad, (8, 8))


def test_load_hw_native_needs_a_source(D):
    with pytest.raises(ValueError):
        D.load_hw("native")


def _tree(root, n_img=6, ir_size=(20, 26), rgb_size=None, dark=()):
    """One sequence of n_img PNG pairs; frames listed in ``dark`` hold IR bytes <= 1."""
    rng = np.random.default_rng(4)
    seq = os.path.join(root, "set00", "V000")
    os.makedirs(os.path.join(seq, "lwir"))
    os.makedirs(os.path.join(seq, "visible"))
    for i in range(n_img):
        g = rng.integers(0, 2 if i in dark else 256, size=ir_size, dtype=np.uint8)
        Image.fromarray(g).save(os.path.join(seq, "lwir", f"I{i:05d}.png"))
        Image.fromarray(rng.integers(0, 256, size=(rgb_size or ir_size) + (3,), dtype=np.uint8)).save(
            os.path.join(seq, "visible", f"I{i:05d}.png"))
    return os.path.join(root, "set00")


def test_constructor_errors(D, tmp_path):
    root = _tree(str(tmp_path), n_img=1)
    mk = lambda **kw: D.KAISTPairDataset(root, verbose=False, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="img_size"):
        mk(img_size=None, load_size=12)                              # a crop needs a size
    with pytest.raises(ValueError, match="img_size"):
        mk(img_size=None, load_size="native")
    with pytest.raises(ValueError, match="smaller"):
        mk(img_size=16, load_size=15)
    with pytest.raises(ValueError, match="smaller"):
        mk(img_size=(8, 10), load_size=(12, 9))                      # one axis is enough
    with pytest.raises(ValueError, match="smaller"):
        mk(img_size=(8, 10), load_size=(7, 15))
    for bad in ("286", 0, (1, 2, 3), 2.5, True):
        with pytest.raises(ValueError, match="load_size"):
            mk(img_size=8, load_size=bad)
    mk(img_size=(8, 10), load_size=(8, 10))                           # equal: offsets are all (0, 0)
    mk(img_size=(8, 10), load_size="native")                          # judged per frame


def test_native_errors_name_both_sizes(D, tmp_path):
    """'native' frames smaller than the crop, or IR / RGB frames of different sizes."""
    small = D.KAISTPairDataset(_tree(str(tmp_path / "a"), n_img=1), img_size=(24, 20), load_size="native",
                               verbose=False)
    for get in (small.__getitem__, small.raw):
        with pytest.raises(RuntimeError, match="20x26.*24x20"):
            get(0)
    differ = D.KAISTPairDataset(_tree(str(tmp_path / "b"), n_img=1, rgb_size=(22, 26)), img_size=(8, 10),
                                load_size="native", verbose=False)
    for get in (differ.__getitem__, differ.raw):
        with pytest.raises(RuntimeError, match="20x26.*22x26"):
            get(0)
    # DeviceResizer meets the same two cases on the batch, before it touches the device
    rs = D.DeviceResizer((24, 20), "cpu", load_size="native")
    batch = {"ir_u8": torch.zeros(1, 20, 26, dtype=torch.uint8), "rgb_u8": torch.zeros(1, 20, 26, 3, dtype=torch.uint8),
             "flip": torch.zeros(1, dtype=torch.uint8), "crop": torch.zeros(1, 2, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="20x26.*24x20"):
        rs(batch)
    batch["rgb_u8"] = torch.zeros(1, 22, 26, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="20x26.*22x26"):
        D.DeviceResizer((8, 10), "cpu", load_size="native")(batch)


def test_device_resizer_constructor_and_offsets(D):
    with pytest.raises(ValueError, match="img_size"):
        D.DeviceResizer(None, "cpu", load_size=12)
    with pytest.raises(ValueError, match="smaller"):
        D.DeviceResizer((8, 10), "cpu", load_size=(12, 9))
    with pytest.raises(ValueError, match="load_size"):
        D.DeviceResizer(8, "cpu", load_size="big")
    rs = D.DeviceResizer((8, 10), "cpu", load_size=(12, 15))
    batch = {"ir_u8": torch.zeros(2, 20, 26, dtype=torch.uint8), "rgb_u8": torch.zeros(2, 20, 26, 3, dtype=torch.uint8),
             "flip": torch.zeros(2, dtype=torch.uint8)}
    for bad in ([[0, 0], [5, 0]], [[0, 6], [0, 0]], [[-1, 0], [0, 0]], [[0, 0], [4, -2]]):
        with pytest.raises(ValueError, match="offsets"):
            rs(dict(batch, crop=torch.tensor(bad, dtype=torch.int32)))
    with pytest.raises(ValueError, match="shape"):
        rs(dict(batch, crop=torch.zeros(3, 2, dtype=torch.int32)))
    with pytest.raises(ValueError, match="load_size"):                # offsets, but nothing to crop from
        D.DeviceResizer((8, 10), "cpu")(dict(batch, crop=torch.zeros(2, 2, dtype=torch.int32)))


# ---------------------------------------------------------------- __getitem__ and raw

def _by_hand(D, ds, i, load, hw, flip, oy, ox):
    h, w = hw
    ir8 = D.resize_area_u8(D.imread_gray(ds.ir_paths[i]), load)[oy:oy + h, ox:ox + w]
    rgb8 = D.resize_area_u8(D.imread_rgb(ds.rgb_paths[i]), load)[oy:oy + h, ox:ox + w]
    if flip:
        ir8, rgb8 = ir8[:, ::-1], rgb8[:, ::-1]
    ir = D._unit_ir(np.ascontiguousarray(ir8))
    rgb = np.ascontiguousarray(rgb8).astype(np.float32) / 255.0
    return (torch.from_numpy(ir)[None] * 2.0 - 1.0,
            torch.from_numpy(np.transpose(rgb, (2, 0, 1)).copy()) * 2.0 - 1.0)


@pytest.mark.parametrize("load_size,load", [((12, 15), (12, 15)),      # area path
                                            (14, (14, 14)),            # an int
                                            ((20, 15), (20, 15)),      # an identity axis
                                            ((24, 30), (24, 30)),      # upscaling: the linear path
                                            ("native", (20, 26))])     # no resampling
def test_getitem_equals_by_hand(D, tmp_path, load_size, load):
    """Seeded python RNG: per item the flip draw, then oy, then ox.  Frame 2 is dark (IR
    bytes <= 1: the max rule skips / 255 on the window)."""
    hw = (8, 10)
    ds = D.KAISTPairDataset(_tree(str(tmp_path), dark=(2,)), img_size=hw, load_size=load_size, verbose=False)
    random.seed(0)
    items = [ds[i] for i in range(len(ds))]
    random.seed(0)
    raws = [ds.raw(i) for i in range(len(ds))]
    rng = random.Random(0)
    flips, offs = [], []
    for i, (it, rw) in enumerate(zip(items, raws)):
        flip = rng.random() < 0.5
        oy = rng.randint(0, load[0] - hw[0])
        ox = rng.randint(0, load[1] - hw[1])
        flips.append(flip)
        offs.append((oy, ox))
        want_ir, want_rgb = _by_hand(D, ds, i, load, hw, flip, oy, ox)
        assert it["ir"].shape == (1,) + hw and it["rgb"].shape == (3,) + hw
        assert it["ir"].dtype == torch.float32 and it["rgb"].dtype == torch.float32
        assert torch.equal(it["ir"], want_ir) and torch.equal(it["rgb"], want_rgb), i
        assert rw["flip"] == int(flip) and tuple(rw["crop"]) == (oy, ox)
        assert tuple(rw["ir_u8"].shape) == (20, 26) and tuple(rw["rgb_u8"].shape) == (20, 26, 3)   # still decoded only
    assert len(set(flips)) == 2 and len(set(offs)) > 1                # the seed exercises both flips, several windows
    assert float(items[2]["ir"].max()) == 1.0                         # byte 1 undivided: 1 * 2 - 1


def test_ir_max_rule_sees_the_window(D, tmp_path):
    """An IR frame that is <= 1 everywhere but one 255 pixel: a window without that pixel is
    not divided by 255, a window with it is."""
    seq = os.path.join(str(tmp_path), "set00", "V000")
    os.makedirs(os.path.join(seq, "lwir"))
    os.makedirs(os.path.join(seq, "visible"))
    g = np.random.default_rng(0).integers(0, 2, size=(12, 16), dtype=np.uint8)
    g[5, 7] = 255
    Image.fromarray(g).save(os.path.join(seq, "lwir", "I0.png"))
    Image.fromarray(np.zeros((12, 16, 3), np.uint8)).save(os.path.join(seq, "visible", "I0.png"))
    ds = D.KAISTPairDataset(os.path.join(str(tmp_path), "set00"), img_size=(6, 8), load_size="native", verbose=False)
    seen = set()
    for seed in range(40):
        random.seed(seed)
        it = ds[0]["ir"][0].numpy()
        rng = random.Random(seed)
        flip = rng.random() < 0.5
        oy, ox = rng.randint(0, 6), rng.randint(0, 8)
        win = g[oy:oy + 6, ox:ox + 8].astype(np.float32)
        inside = oy <= 5 < oy + 6 and ox <= 7 < ox + 8
        want = np.clip(win / np.float32(255.0), 0.0, 1.0) if inside else win      # divided only with the 255 in it
        want = want[:, ::-1] if flip else want
        assert np.array_equal(it, want * np.float32(2.0) - np.float32(1.0)), (seed, oy, ox)
        assert (it == 1.0).sum() == (1 if inside else int((win == 1).sum()))
        seen.add(inside)
    assert seen == {True, False}


def test_flip_stream_without_the_option_is_untouched(D, tmp_path):
    """load_size=None draws exactly one random() per item, as before the option existed; with
    it the flips of the same seed are different draws of the same stream."""
    root = _tree(str(tmp_path))
    plain = D.KAISTPairDataset(root, img_size=(8, 10), verbose=False)
    crop = D.KAISTPairDataset(root, img_size=(8, 10), load_size=(12, 15), verbose=False)
    assert plain.load_size is None
    random.seed(5)
    got = [plain.raw(i) for i in range(len(plain))]
    after = random.random()
    rng = random.Random(5)
    assert [g["flip"] for g in got] == [int(rng.random() < 0.5) for _ in range(len(plain))]
    assert after == rng.random()                                      # nothing else was drawn
    assert all("crop" not in g for g in got)
    random.seed(5)
    items = [plain[i] for i in range(len(plain))]
    assert random.random() == after
    for i, (it, g) in enumerate(zip(items, got)):                     # and the tensors are today's
        ir = D._unit_ir(D.resize_area_u8(D.imread_gray(plain.ir_paths[i]), (8, 10)))
        ir = np.fliplr(ir).copy() if g["flip"] else ir
        assert torch.equal(it["ir"], torch.from_numpy(ir)[None] * 2.0 - 1.0)
    random.seed(5)
    got_c = [crop.raw(i) for i in range(len(crop))]
    rng = random.Random(5)
    for g in got_c:                                                   # three draws per item, flip first
        assert g["flip"] == int(rng.random() < 0.5)
        assert tuple(g["crop"]) == (rng.randint(0, 4), rng.randint(0, 5))


@pytest.mark.parametrize("load_size", [None, (12, 15), 14, "native"])
def test_augment_false_ignores_load_size(D, tmp_path, load_size):
    root = _tree(str(tmp_path), n_img=3)
    ref = D.KAISTPairDataset(root, img_size=(8, 10), augment=False, verbose=False)
    ds = D.KAISTPairDataset(root, img_size=(8, 10), augment=False, load_size=load_size, verbose=False)
    random.seed(1)
    state = random.getstate()
    for i in range(3):
        a, b = ds[i], ref[i]
        assert torch.equal(a["ir"], b["ir"]) and torch.equal(a["rgb"], b["rgb"])
        r = ds.raw(i)
        assert "crop" not in r and r["flip"] == 0
    assert random.getstate() == state                                 # no draw at all


def test_collate_raw_carries_crop_only_when_present(D, tmp_path):
    root = _tree(str(tmp_path), n_img=3)
    plain = D.KAISTPairDataset(root, img_size=(8, 10), verbose=False)
    crop = D.KAISTPairDataset(root, img_size=(8, 10), load_size=(12, 15), verbose=False)
    random.seed(2)
    b = D.collate_raw([plain.raw(i) for i in range(3)])
    assert set(b) == {"ir_u8", "rgb_u8", "flip"}
    random.seed(2)
    items = [crop.raw(i) for i in range(3)]
    b = D.collate_raw(items)
    assert set(b) == {"ir_u8", "rgb_u8", "flip", "crop"}
    assert b["crop"].dtype == torch.int32 and tuple(b["crop"].shape) == (3, 2)
    assert b["crop"].tolist() == [list(it["crop"]) for it in items]
    assert b["flip"].tolist() == [it["flip"] for it in items]


# ---------------------------------------------------------------- Config and the command line

def test_config_default_is_off():
    assert pkg().Config().load_size is None


def test_cli_load_size(D):
    import importlib
    main = importlib.import_module(PKG_NAME + ".__main__")
    assert main.config_from_argv(["train"]).load_size is None
    assert main.config_from_argv(["train", "--load-size", "286"]).load_size == 286
    assert main.config_from_argv(["train", "--load-size", "300x360"]).load_size == (300, 360)
    cfg = main.config_from_argv(["train", "--load-size", "native", "--img-size", "256x320"])
    assert cfg.load_size == "native" and cfg.img_size == (256, 320) and cfg.mode == "train"
    assert D.parse_load_size(" NATIVE ") == "native"
    for bad in ("", "x", "0", "12x", "1x2x3", "2.5", "big", "-4"):
        with pytest.raises(ValueError):
            D.parse_load_size(bad)
    with pytest.raises(SystemExit):
        main.config_from_argv(["train", "--load-size", "big"])
    assert "--load-size" in main.__doc__


def test_train_kaist_passes_load_size_to_the_training_set_only(tmp_path, monkeypatch):
    """train_kaist builds three datasets: the count, the training set (load_size) and the
    validation set (none).  A stub records them and stops the run before any network."""
    irc = pkg()
    root = _tree(str(tmp_path), n_img=4)
    seen = []
    real = irc.data.KAISTPairDataset

    class Stop(Exception):
        pass

    def spy(*a, **kw):
        seen.append((kw.get("augment"), kw.get("load_size")))
        return real(*a, **kw)

    def stop(*a, **kw):
        raise Stop()

    monkeypatch.setattr(irc.data, "KAISTPairDataset", spy)
    monkeypatch.setattr(irc.data, "kaist_loader", stop)
    cfg = irc.Config()
    cfg.device, cfg.train_roots, cfg.img_size, cfg.load_size = "cpu", [root], (8, 10), (12, 15)
    with pytest.raises(Stop):
        irc.train_kaist(cfg, log=lambda *_: None)
    assert seen == [(False, None), (True, (12, 15)), (False, None)]
    cfg.img_size = None                                               # a crop needs a size: before any GPU work
    with pytest.raises(ValueError, match="img_size"):
        irc.train_kaist(cfg, log=lambda *_: None)
