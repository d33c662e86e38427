"""Rectangular and native-resolution ``img_size`` on the device (ir:803-852, 1132-1177,
1333-1514, 1549-1723): DeviceResizer with an (h, w) target and at the source size
(irgan_u8_native_to_unit) bit for bit against the host items, kaist_loader,
train_kaist against the fp64 oracle at 32x48 and on a directory at native size, and
run_test with a rectangular and a native img_size."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch
from PIL import Image

from conftest import pkg
from oracle import infer as OI
from oracle import step as O

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _host_item(D, ir_u8, rgb_u8, flip, size):
    ir = D.resize_area_u8(ir_u8, size).astype(np.float32)
    if ir.max() > 1.0:
        ir /= 255.0
    rgb = D.resize_area_u8(rgb_u8, size).astype(np.float32) / 255.0
    if flip:
        ir, rgb = np.fliplr(ir).copy(), np.fliplr(rgb).copy()
    return (torch.from_numpy(ir)[None] * 2.0 - 1.0,
            torch.from_numpy(np.transpose(rgb, (2, 0, 1)).copy()) * 2.0 - 1.0)


def _batch(H, W, seed):
    rng = np.random.default_rng(seed)
    ir = rng.integers(0, 256, size=(3, H, W), dtype=np.uint8)
    ir[1] = rng.integers(0, 2, size=(H, W), dtype=np.uint8)        # max <= 1: the IR rule skips / 255 (ir:1142)
    rgb = rng.integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    return ir, rgb, torch.tensor([1, 0, 1], dtype=torch.uint8)


@pytest.mark.parametrize("hw", [(24, 40), (40, 24), (48, 30), (64, 40), (96, 120)])
def test_device_rectangular_equals_host(hw):
    """48x60 -> area tables per axis ((48, 30): the rows keep their size), and the linear
    path once either axis upscales ((64, 40), (96, 120))."""
    D = pkg().data
    ir, rgb, flip = _batch(48, 60, 0)
    out = D.DeviceResizer(hw, DEV)({"ir_u8": torch.from_numpy(ir), "rgb_u8": torch.from_numpy(rgb), "flip": flip})
    assert out["ir"].shape == (3, 1) + hw and out["rgb"].shape == (3, 3) + hw
    for b in range(3):
        hi, hr = _host_item(D, ir[b], rgb[b], bool(flip[b]), hw)
        assert torch.equal(out["ir"][b].cpu(), hi), b
        assert torch.equal(out["rgb"][b].cpu(), hr), b


def _identity_table_pair(D, rs, u8, C, flip, max_rule):
    """What the native kernel replaces: irgan_area_resize_u8 with identity tables, then
    irgan_u8_to_unit."""
    irc = pkg()
    B, H, W = u8.shape[:3]
    mx = torch.zeros(B, dtype=torch.int32, device=DEV)
    out8 = rs.resize_u8(u8, C, flip, mx)
    out = torch.empty(B, C, H, W, dtype=torch.float32, device=DEV)
    irc._lib.call("irgan_u8_to_unit", irc.ops.P(out8), B, ctypes.c_int64(C * H * W), irc.ops.P(mx), int(max_rule),
                  irc.ops.P(out), irc.ops.stream())
    return out, out8


@pytest.mark.parametrize("H,W", [(40, 56), (37, 61), (130, 250)])
def test_native_kernel(H, W):
    """37x61: row bytes 61 and 183, no multiple of 16, rows misaligned; 130x250: many
    blocks per image.  C = 1 with the IR max rule, C = 3 without."""
    D = pkg().data
    ir, rgb, flip = _batch(H, W, 3)
    rs = D.DeviceResizer(None, DEV)
    out = rs({"ir_u8": torch.from_numpy(ir), "rgb_u8": torch.from_numpy(rgb), "flip": flip})
    assert out["ir"].shape == (3, 1, H, W) and out["rgb"].shape == (3, 3, H, W)
    for b in range(3):
        hi, hr = _host_item(D, ir[b], rgb[b], bool(flip[b]), None)
        assert torch.equal(out["ir"][b].cpu(), hi), b
        assert torch.equal(out["rgb"][b].cpu(), hr), b
    fl = flip.to(DEV)
    for src, C, rule in ((ir, 1, True), (rgb, 3, False)):
        u8 = torch.from_numpy(src).to(DEV)
        got, got8 = rs._one(u8, C, fl, rule, keep_u8=True)
        want, want8 = _identity_table_pair(D, rs, u8, C, fl, rule)
        assert torch.equal(got, want) and torch.equal(got8, want8)
        s4 = torch.from_numpy(src.reshape(3, H, W, C)).permute(0, 3, 1, 2)
        copy = torch.stack([torch.flip(s4[b], [2]) if flip[b] else s4[b] for b in range(3)])
        assert torch.equal(got8.cpu(), copy)
        assert torch.equal(rs._one(u8, C, fl, rule), got)            # without the uint8 copy
    # an int img_size that equals the source size takes the same pass
    sq = torch.from_numpy(np.ascontiguousarray(rgb[:, :37, :37])).to(DEV)
    a = D.DeviceResizer(37, DEV)._one(sq, 3, fl, False)
    b_, _ = _identity_table_pair(D, D.DeviceResizer(37, DEV), sq, 3, fl, False)
    assert torch.equal(a, b_)


@pytest.mark.parametrize("C,off,pad", [(1, 5, 3), (2, 1, 1), (2, 6, 0), (3, 7, 2), (4, 2, 0), (4, 8, 4)])
def test_native_entry_point_any_base_and_stride(C, off, pad):
    """The entry point itself on a base address `off` bytes past an aligned one and an
    image stride `pad` bytes above H*W*C: every C <= 4 (C = 2, 4 on an address that no
    pixel start can align: the pixel-by-pixel path), against torch's own float32 ops."""
    irc = pkg()
    P = irc.ops.P
    N, H, W = 2, 9, 45
    rng = np.random.default_rng(C * 16 + off)
    stride = H * W * C + pad
    buf = torch.from_numpy(rng.integers(0, 256, size=off + N * stride, dtype=np.uint8))
    dbuf = buf.to(DEV)
    src = torch.stack([buf[off + n * stride: off + n * stride + H * W * C].view(H, W, C) for n in range(N)])
    flip = torch.tensor([0, 1], dtype=torch.uint8)
    out = torch.full((N, C, H, W), 7.0, dtype=torch.float32, device=DEV)
    out8 = torch.zeros(N, C, H, W, dtype=torch.uint8, device=DEV)
    mx = torch.zeros(N, dtype=torch.int32, device=DEV)
    fl = flip.to(DEV)
    irc._lib.call("irgan_u8_native_to_unit", ctypes.c_void_p(dbuf.data_ptr() + off), N, H, W, C,
                  ctypes.c_int64(stride), P(fl), 1, P(mx), P(out), P(out8), irc.ops.stream())
    assert mx.cpu().tolist() == [int(src[n].max()) for n in range(N)]
    want8 = src.permute(0, 3, 1, 2).clone()
    want8[1] = torch.flip(want8[1], [2])
    assert torch.equal(out8.cpu(), want8)
    unit = np.clip(want8.numpy().astype(np.float32) / np.float32(255.0), 0.0, 1.0)
    assert torch.equal(out.cpu(), torch.from_numpy(unit) * 2.0 - 1.0)
    # empty sizes return 0 and touch nothing; a bad channel count is refused
    lib = irc._lib.load()
    assert lib.irgan_u8_native_to_unit(P(dbuf), 0, H, W, C, ctypes.c_int64(stride), None, 0, None, P(out), None,
                                       irc.ops.stream()) == 0
    assert lib.irgan_u8_native_to_unit(P(dbuf), N, H, W, 5, ctypes.c_int64(stride), None, 0, None, P(out), None,
                                       irc.ops.stream()) != 0
    assert lib.irgan_u8_native_to_unit(P(dbuf), N, H, W, C, ctypes.c_int64(stride - pad - 1), None, 0, None, P(out),
                                       None, irc.ops.stream()) != 0
    assert lib.irgan_u8_native_to_unit(P(dbuf), N, H, W, C, ctypes.c_int64(stride), None, 1, None, P(out), None,
                                       irc.ops.stream()) != 0      # the max rule needs img_max


def test_native_size_needs_one_size_per_pair():
    D = pkg().data
    batch = {"ir_u8": torch.zeros(2, 40, 56, dtype=torch.uint8), "rgb_u8": torch.zeros(2, 48, 56, 3, dtype=torch.uint8),
             "flip": torch.zeros(2, dtype=torch.uint8)}
    with pytest.raises(RuntimeError, match="40x56.*48x56"):
        D.DeviceResizer(None, DEV)(batch)
    out = D.DeviceResizer((24, 40), DEV)(batch)                       # a given size: sources may differ
    assert out["ir"].shape == (2, 1, 24, 40) and out["rgb"].shape == (2, 3, 24, 40)


def _kaist_tree(root, n_seq=2, n_img=4, size=(40, 56)):
    rng = np.random.default_rng(1)
    for s in range(n_seq):
        seq = os.path.join(root, "set00", f"V{s:03d}")
        os.makedirs(os.path.join(seq, "lwir"))
        os.makedirs(os.path.join(seq, "visible"))
        for i in range(n_img):
            g = rng.integers(0, 256, size=size, dtype=np.uint8)
            Image.fromarray(np.repeat(g[:, :, None], 3, 2)).save(os.path.join(seq, "lwir", f"I{i:05d}.png"))
            Image.fromarray(rng.integers(0, 256, size=size + (3,), dtype=np.uint8)).save(
                os.path.join(seq, "visible", f"I{i:05d}.png"))
    return os.path.join(root, "set00")


@pytest.mark.parametrize("img_size,hw", [((32, 48), (32, 48)), (None, (40, 56))])
def test_kaist_loader_equals_reference_items(tmp_path, img_size, hw):
    D = pkg().data
    root = _kaist_tree(str(tmp_path))
    ds = D.KAISTPairDataset(root, img_size=img_size, augment=False)
    got = list(D.kaist_loader(ds, 3, DEV, shuffle=False, drop_last=False))
    assert [b["ir"].shape[0] for b in got] == [3, 3, 2]
    k = 0
    for b in got:
        assert b["ir"].shape[1:] == (1,) + hw and b["rgb"].shape[1:] == (3,) + hw
        for j in range(b["ir"].shape[0]):
            ref = ds[k]
            assert torch.equal(b["ir"][j].cpu(), ref["ir"]) and torch.equal(b["rgb"][j].cpu(), ref["rgb"])
            k += 1


def _floats(line, *names):
    out = []
    for n in names:
        m = re.search(re.escape(n) + r"\s*:?\s*(-?\d+\.\d+(?:e[-+]\d+)?)", line)
        out.append(float(m.group(1)))
    return out


def test_train_kaist_rectangular_vs_oracle(tmp_path):
    """test_train_kaist_plumbing_vs_oracle's recipe (fp32, seeded G / D / VGG, N = 7,
    B = 5: one step per epoch) on 32x48 pairs, with its tolerances."""
    irc = pkg()
    cfg = irc.Config()
    cfg.device, cfg.compute_dtype = DEV, "fp32"
    cfg.img_size = (32, 48)
    cfg.epochs, cfg.lr_decay_start_epoch, cfg.save_every = 3, 1, 5
    cfg.val_ratio, cfg.batch_size = 0.3, 5
    cfg.save_dir = str(tmp_path / "ckpt")
    G = O.seeded_params(O.g_param_shapes(), 1, bias_std=0.02)
    Dp = O.seeded_params(O.d_param_shapes(), 2, bias_std=0.02)
    V = O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True)
    cfg.init_G_weights = str(tmp_path / "g0.pth")
    torch.save(G, cfg.init_G_weights)

    def hook(tr):
        tr.netD.store.load(Dp, strict=True)
        tr.vgg.store.load(V, strict=True)
        tr.netD.repack()
        tr.vgg.repack()

    ds = irc.SyntheticPairDataset(7, img_size=(32, 48), seed=5)
    assert ds[0]["ir"].shape == (1, 32, 48)
    logs = []
    hist = irc.train_kaist(cfg, dataset=ds, log=logs.append, trainer_hook=hook)
    assert len(hist) == 3
    idxs = list(range(7))
    random.seed(42)
    random.shuffle(idxs)
    tr_i, va_i = idxs[:5], idxs[5:]
    dd = lambda P: {k: v.double().clone() for k, v in P.items()}   # noqa: E731
    G64, D64, V64 = dd(G), dd(Dp), dd(V)
    ir = torch.stack([ds[i]["ir"] for i in tr_i]).double()
    rgb = torch.stack([ds[i]["rgb"] for i in tr_i]).double()
    ref = O.train_step(G64, D64, V64, ir, rgb, O.AdamState(G64), O.AdamState(D64))
    step1 = next(line for line in logs if line.startswith("Epoch [1/3] Step [1/1]"))
    d_log, g_log = _floats(step1, "D", "G")
    gan, l1 = _floats(step1, "GAN", "L1")
    print(step1, {k: float(ref[k]) for k in ("loss_D", "loss_G", "loss_G_GAN", "loss_G_L1")})
    assert abs(d_log - float(ref["loss_D"])) <= 2e-4 and abs(g_log - float(ref["loss_G"])) <= 2e-4, step1
    assert abs(l1 - float(ref["loss_G_L1"])) <= 2e-4 and abs(gan - float(ref["loss_G_GAN"])) <= 2e-4
    vir = torch.stack([ds[i]["ir"] for i in va_i]).double()
    vrgb = torch.stack([ds[i]["rgb"] for i in va_i]).double()
    with torch.no_grad():
        val_ref = float((O.g_forward(G64, vir) - vrgb).abs().mean())
    done1 = next(line for line in logs if line.startswith("Epoch [1/3] DONE"))
    print(done1, val_ref)
    assert abs(_floats(done1, "val L1")[0] - val_ref) <= 1e-3, (done1, val_ref)


def test_train_kaist_on_directory_at_native_size(tmp_path):
    """cfg.img_size = None: the 40x56 frames train as they are (bf16 step), through the
    native device pass."""
    irc = pkg()
    root = _kaist_tree(str(tmp_path))
    cfg = irc.Config()
    cfg.device = DEV
    cfg.train_roots = [root]
    cfg.img_size, cfg.batch_size, cfg.epochs, cfg.num_workers = None, 2, 1, 0
    cfg.save_dir = str(tmp_path / "ckpt")
    logs = []
    hist = irc.train_kaist(cfg, log=logs.append)
    assert len(hist) == 1 and np.isfinite(hist[0]["loss_G"]) and np.isfinite(hist[0]["loss_D"])
    assert np.isfinite(hist[0]["val_l1"])
    assert "Total pairs: 8, train: 7, val: 1" in logs
    assert os.path.isfile(os.path.join(cfg.save_dir, "netG_epoch_001.pth"))


def _gt_tree(root):
    """As test_run_test_outputs_and_csv builds it: set02/V000 with 3 frames 64x80 + 2 frames
    72x96, frame 4's GT missing; set05/V001 without visible/ (not scanned, ir:929-930)."""
    rng = np.random.default_rng(11)
    sizes = [(64, 80)] * 3 + [(72, 96)] * 2
    seq = os.path.join(root, "set02", "V000")
    os.makedirs(os.path.join(seq, "lwir"))
    os.makedirs(os.path.join(seq, "visible"))
    for i, (h, w) in enumerate(sizes):
        g = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        Image.fromarray(np.repeat(g[:, :, None], 3, 2)).save(os.path.join(seq, "lwir", f"I{i:05d}.png"))
        if i != 4:
            Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(
                os.path.join(seq, "visible", f"I{i:05d}.png"))
    seq2 = os.path.join(root, "set05", "V001", "lwir")
    os.makedirs(seq2)
    Image.fromarray(rng.integers(0, 256, size=(64, 80, 3), dtype=np.uint8)).save(os.path.join(seq2, "I00000.png"))
    return [os.path.join(root, "set02"), os.path.join(root, "set05")], sizes


@pytest.mark.parametrize("img_size", [(32, 48), None])
def test_run_test_rectangular_and_native(tmp_path, img_size):
    irc = pkg()
    D = irc.data
    cfg = irc.Config()
    cfg.device, cfg.compute_dtype = DEV, "fp32"
    cfg.img_size, cfg.test_batch, cfg.topk = img_size, 2, 3
    cfg.test_roots, sizes = _gt_tree(str(tmp_path / "kaist"))
    cfg.output_dir = str(tmp_path / "results")
    cfg.save_comparisons, cfg.comparison_add_text = True, False
    G = O.seeded_params(O.g_param_shapes(), 1, bias_std=0.02)
    cfg.test_G_weights = str(tmp_path / "g.pth")
    torch.save(G, cfg.test_G_weights)
    logs = []
    metrics = irc.run_test(cfg, log=logs.append)
    assert len(metrics) == 4
    m = irc.IRColorizationModel(cfg)
    m.load_weights(cfg.test_G_weights)
    m.eval()
    entries = D.collect_kaist_ir_files_from_sets(cfg.test_roots)
    assert len(entries) == 5
    rows = {}
    for (ir_path, set_name, seq_name), src_hw in zip(entries, sizes):
        hw = img_size if img_size is not None else src_hw
        rel = os.path.join(set_name, seq_name, os.path.basename(ir_path))
        saved = np.asarray(Image.open(os.path.join(cfg.output_dir, rel)))
        assert saved.shape == hw + (3,), (rel, saved.shape)
        ir01 = D.load_ir_image(ir_path, img_size=img_size)
        want = irc.inference.colorize_u8(m, irc.ir_to_tensor(ir01).to(DEV))[0].cpu().numpy()
        d = np.abs(saved.astype(int) - want.astype(int))
        print(rel, "max code diff", d.max(), "share", (d > 0).mean())
        assert d.max() <= 1 and (d > 0).mean() < 0.01, rel      # batch vs single-frame G: fp32 round-off
        gt_path = os.path.join(os.path.dirname(os.path.dirname(ir_path)), "visible", os.path.basename(ir_path))
        if os.path.isfile(gt_path):
            gt01_ = D.load_rgb_image(gt_path, img_size=img_size)
            gt8_ = D.resize_area_u8(D.imread_rgb(gt_path), hw)
            dev = irc.inference.image_metrics_u8(torch.from_numpy(saved.copy())[None].to(DEV),
                                                 torch.from_numpy(gt8_)[None].to(DEV))[0]
            # independent of the device code: compute_metrics' float32 differences (ir:1195-1199)
            # summed in fp64, and the oracle's PSNR / SSIM.  (The oracle's own MAE / MSE are
            # float32 np.mean: at 64x80x3 terms their rounding alone passes the 2e-8 below.)
            diff = (saved.astype(np.float32) / 255.0 - gt01_).astype(np.float64)
            _, _, psnr_o, ssim_o = OI.compute_metrics(saved.astype(np.float32) / 255.0, gt01_, with_ssim=True)
            rows[rel] = (dev, (np.abs(diff).mean(), (diff ** 2).mean(), psnr_o, ssim_o))
            # the collage: [IR | pred | GT], h x w panels, `pad` black columns between them
            stem = os.path.splitext(os.path.basename(ir_path))[0]
            c = np.asarray(Image.open(os.path.join(cfg.output_dir, "Comparisons", set_name, seq_name,
                                                   stem + "_cmp.png")))
            assert c.shape == (hw[0], 3 * hw[1] + 2 * cfg.comparison_pad, 3)
            assert np.array_equal(c[:, hw[1] + 8:2 * hw[1] + 8], saved)
            gt01 = D.resize_area_u8(D.imread_rgb(gt_path), hw).astype(np.float32) / 255.0
            assert np.array_equal(c[:, 2 * hw[1] + 16:], (gt01 * 255.0).astype(np.uint8))   # float01_to_uint8_rgb
            ir_panel = np.repeat((np.clip(ir01, 0.0, 1.0) * 255.0).astype(np.uint8)[:, :, None], 3, axis=2)
            assert np.array_equal(c[:, :hw[1]], ir_panel)
    assert set(rows) == {m_["file"] for m_ in metrics}
    lines = open(os.path.join(cfg.output_dir, "metrics_test.csv")).read().splitlines()
    assert lines[0] == "file,mae,mse,psnr,ssim" and lines[5] == "" and lines[7] == "# count,4"
    for line in lines[1:5]:
        f, mae, mse, psnr, ssim = line.split(",")
        for r in rows[f]:
            print(f, [float(mae) - r[0], float(mse) - r[1], float(psnr) - r[2], float(ssim) - r[3]])
            assert abs(float(mae) - r[0]) < 2e-8 and abs(float(mse) - r[1]) < 2e-8
            assert abs(float(psnr) - r[2]) < 2e-6 and abs(float(ssim) - r[3]) < 2e-6
