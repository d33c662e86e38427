"""Golden vectors for norm='batch' (nn.BatchNorm2d in the generator and the PatchGAN), by
EXECUTING THE REFERENCE on the CPU (same loader and stubs as make_golden.py):

    python tests/golden/make_bn_golden.py

Conv weights come from ``oracle.seeded_params`` on the bias-less layout (the tests rebuild
them from the seeds).  The BatchNorm parameters are stored in the fixtures: gamma = 1 + 0.1 n,
beta = 0.1 n (n standard normal, fixed seed), so the affine part and both signs of
gamma * xhat + beta are exercised, and one gamma entry per network is exactly 0.

* step_s32_bn.npz -- the records make_golden.run_reference makes (two steps of ir:1636-1681,
  fp32 and fp64, err32; 32x32, B = 2) with cfg.norm = 'batch' for G and D, plus the full
  gamma / beta gradients and G's eval-mode output on ``ir`` after step 1; every running_mean /
  running_var / num_batches_tracked after step 1 and after step 2 (fp32 and fp64) goes to
  step_s32_bn_stats.npz.
* modules_bn.npz -- output, input gradient and parameter gradients of one call in train mode
  and in eval mode (seeded non-trivial running statistics) of a small generator (ngf 8,
  2 blocks, 20x28, padding 'zero'), the same with no_antialias / no_antialias_up, and a
  discriminator (ndf 8, n_layers 2, 24x24); fp64.  Also the ordered key list and shapes of the
  reference's BatchNorm state_dict() for G (default flags) and D (n_layers 3).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden import LAMBDA_ORDER, SEED_D, SEED_DATA, SEED_G, SEED_IDX, SEED_V, digest, load_reference  # noqa: E402
from oracle import step as O  # noqa: E402

SEED_BN_G, SEED_BN_D, SEED_RUN = 41, 42, 43
BN_BUFFERS = (".running_mean", ".running_var", ".num_batches_tracked")


def bn_params(keys, shapes, seed):
    """gamma / beta of every BatchNorm module in ``keys`` (state order), one gamma set to 0."""
    g = torch.Generator().manual_seed(seed)
    out, first = {}, True
    for k in keys:
        if k.endswith(BN_BUFFERS):
            continue
        n = torch.randn(shapes[k], generator=g)
        out[k] = (1.0 + 0.1 * n if k.endswith(".weight") else 0.1 * n).double()   # fp32 values: both runs' alike
        if first and k.endswith(".weight"):
            out[k][1] = 0.0
            first = False
    return out


def running_stats(keys, shapes, seed):
    """Non-trivial running statistics for the eval-mode cases."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k in keys:
        if k.endswith(".running_mean"):
            out[k] = 0.05 * torch.randn(shapes[k], generator=g, dtype=torch.float64)
        elif k.endswith(".running_var"):
            out[k] = 0.5 + torch.rand(shapes[k], generator=g, dtype=torch.float64)
    return out


def load_seeded(net, conv_shapes, seed, bn_seed, dtype):
    """Seeded conv weights + stored BatchNorm parameters into a reference module; returns the
    BatchNorm parameter dict (fp64) and the module's BatchNorm keys in state order."""
    sd = net.state_dict()
    conv = O.seeded_params(conv_shapes, seed, bias_std=0.02)
    bn_keys = [k for k in sd if k not in conv]
    assert [k for k in sd if k in conv] == list(conv), "conv layout differs from the oracle's"
    bn = bn_params(bn_keys, {k: tuple(sd[k].shape) for k in bn_keys}, bn_seed)
    net.load_state_dict({**conv, **bn}, strict=False)
    net.to(dtype)
    return bn, bn_keys


def buffers_of(net):
    return {k: v.detach().clone() for k, v in net.state_dict().items() if k.endswith(BN_BUFFERS)}


def run_step_reference(R, dtype, H=32, W=32, B=2):
    cfg = R.Config()
    cfg.device = "cpu"
    cfg.norm = "batch"
    model = R.IRColorizationModel(cfg)
    netG = model.netG
    bnG, _ = load_seeded(netG, O.g_param_shapes(use_bias=False), SEED_G, SEED_BN_G, dtype)
    netD = R.NLayerDiscriminator(input_nc=4, ndf=64, n_layers=3, norm_layer=R.get_norm_layer("batch"))
    bnD, _ = load_seeded(netD, O.d_param_shapes(use_bias=False), SEED_D, SEED_BN_D, dtype)
    netG.train()
    netD.train()
    optG = torch.optim.Adam(netG.parameters(), lr=cfg.lr_G, betas=(cfg.beta1, cfg.beta2))
    optD = torch.optim.Adam(netD.parameters(), lr=cfg.lr_D, betas=(cfg.beta1, cfg.beta2))
    vgg = R.VGGPerceptual("cpu").to(dtype)
    l1 = nn.L1Loss()
    g = torch.Generator().manual_seed(SEED_DATA)
    ir = (torch.rand(B, 1, H, W, generator=g) * 2 - 1).to(dtype)
    rgb = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(dtype)
    rec = {"ir": ir.float().numpy(), "rgb": rgb.float().numpy(),
           "meta": np.array([H, W, B, 0, 0, SEED_G, SEED_D, SEED_V], np.int64),
           "lambdas": np.array([getattr(cfg, k) for k in LAMBDA_ORDER], np.float64)}
    for tag, bn in (("bnG", bnG), ("bnD", bnD)):
        for k, v in bn.items():
            rec[f"{tag}|{k}"] = v.float().numpy()
    full = {}
    for step in (1, 2):
        # ---- body of ir:1636-1681, driving the reference's own objects
        optD.zero_grad()
        with torch.no_grad():
            fake_det = model(ir)
        pred_real = netD(torch.cat([ir, rgb], dim=1))
        pred_fake = netD(torch.cat([ir, fake_det], dim=1))
        loss_D = 0.5 * (F.relu(1.0 - pred_real).mean() + F.relu(1.0 + pred_fake).mean())
        loss_D.backward()
        gradD = {k: p.grad.detach().clone() for k, p in netD.named_parameters()}
        optD.step()
        optG.zero_grad()
        fake = model(ir)
        pred_fake_G = netD(torch.cat([ir, fake], dim=1))
        l_gan = -pred_fake_G.mean()
        l_l1 = l1(fake, rgb) * cfg.lambda_L1
        l_perc = F.l1_loss(vgg(fake), vgg(rgb)) * cfg.lambda_perc
        l_tv = R.tv_loss(fake) * cfg.lambda_tv
        l_ssim = R.ssim_loss_torch((fake + 1.0) / 2.0, (rgb + 1.0) / 2.0) * cfg.lambda_ssim
        loss_G = cfg.lambda_gan * l_gan + l_l1 + l_perc + l_tv + l_ssim
        loss_G.backward()
        gradG = {k: p.grad.detach().clone() for k, p in netG.named_parameters()}
        optG.step()
        p = f"step{step}_"
        for k, v in dict(loss_D=loss_D, loss_G=loss_G, loss_G_GAN=l_gan, loss_G_L1=l_l1, loss_G_perc=l_perc,
                         loss_G_TV=l_tv, loss_G_ssim=l_ssim).items():
            rec[p + k] = np.float64(v.item())
        for tag, net in (("G", netG), ("D", netD)):
            for k, v in buffers_of(net).items():
                rec[f"rs{step}|{tag}|{k}"] = v.numpy()
        if step == 1:
            full = {"gG": gradG, "gD": gradD}
            rec["fake"] = fake.detach().float().numpy()
            rec["pred_real"] = pred_real.detach().float().numpy()
            rec["pred_fake"] = pred_fake.detach().float().numpy()
            rec["pred_fake_G"] = pred_fake_G.detach().float().numpy()
            model.eval()   # running statistics, nothing updated
            with torch.no_grad():
                rec["eval_fake"] = model(ir).double().numpy()
            model.train()
            gen = torch.Generator().manual_seed(SEED_IDX)
            for tag, grads, params in (("gG", gradG, dict(netG.named_parameters())),
                                       ("gD", gradD, dict(netD.named_parameters()))):
                for k in grads:
                    idx, samp, s, a = digest(grads[k], gen)
                    rec[f"{tag}|{k}|idx"] = idx
                    rec[f"{tag}|{k}|val"] = samp
                    rec[f"{tag}|{k}|sum"] = np.float64(s)
                    rec[f"{tag}|{k}|abs"] = np.float64(a)
                    rec[f"{tag}|{k}|post"] = params[k].detach().reshape(-1)[torch.from_numpy(idx)].float().numpy()
                    if grads[k].dim() == 1:   # gamma / beta (and the three conv biases): in full
                        rec[f"{tag}|{k}|full"] = grads[k].double().numpy()
    return rec, full


def make_step():
    R = load_reference()
    rec, g32 = run_step_reference(R, torch.float32)
    rec64, g64 = run_step_reference(R, torch.float64)
    for tag in ("gG", "gD"):
        for k in g32[tag]:
            a, b = g32[tag][k].double(), g64[tag][k].double()
            rec[f"{tag}|{k}|val64"] = rec64[f"{tag}|{k}|val"]
            rec[f"{tag}|{k}|err32"] = np.float64((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
            rec[f"{tag}|{k}|err32l2"] = np.float64((a - b).norm() / b.norm().clamp_min(1e-30))
            if f"{tag}|{k}|full" in rec64:
                rec[f"{tag}|{k}|full"] = rec64[f"{tag}|{k}|full"]
    for k in [k for k in rec64 if k.startswith("step") or (k.startswith("rs") and not k.endswith("tracked"))]:
        rec[k + "_64"] = rec64[k]
    rec["fake64"] = rec64["fake"]
    rec["eval_fake_64"] = rec64["eval_fake"]
    # the running statistics in a file of their own (each file stays below the largest fixture)
    stats = {k: rec.pop(k) for k in [k for k in rec if k.startswith("rs")]}
    out = os.path.join(HERE, "step_s32_bn_stats.npz")
    np.savez_compressed(out, **stats)
    print("wrote", out, os.path.getsize(out), "bytes")
    out = os.path.join(HERE, "step_s32_bn.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes; loss_D", rec["step1_loss_D"], "loss_G", rec["step1_loss_G"],
          "worst err32l2", max((float(rec[k]), k) for k in rec if k.endswith("|err32l2")))
    return R


MODULE_CASES = {
    # name: (kind, kwargs, input shape)
    "bn_g": ("g", dict(no_antialias=False, no_antialias_up=False), (3, 1, 20, 28)),
    "bn_g_noaa": ("g", dict(no_antialias=True, no_antialias_up=True), (3, 1, 20, 28)),
    "bn_d": ("d", {}, (2, 4, 24, 24)),
}


def make_modules(R):
    rec = {}
    for name, (kind, kw, xs) in MODULE_CASES.items():
        if kind == "g":
            net = R.ResnetUNetGenerator(1, 3, 8, norm_layer=R.get_norm_layer("batch"), use_dropout=False, n_blocks=2,
                                        padding_type="zero", **kw)
            shapes = O.g_param_shapes(ngf=8, n_blocks=2, use_bias=False, padding_type="zero", **kw)
            seed, bn_seed = SEED_G, SEED_BN_G
        else:
            net = R.NLayerDiscriminator(4, 8, n_layers=2, norm_layer=R.get_norm_layer("batch"))
            shapes = O.d_param_shapes(4, 8, 2, use_bias=False)
            seed, bn_seed = SEED_D, SEED_BN_D
        bn, bn_keys = load_seeded(net, shapes, seed, bn_seed, torch.float64)
        sd = net.state_dict()
        run = running_stats(bn_keys, {k: tuple(sd[k].shape) for k in bn_keys}, SEED_RUN)
        net.load_state_dict(run, strict=False)
        for k, v in {**bn, **run}.items():
            rec[f"{name}|param|{k}"] = v.numpy()
        x0 = torch.rand(xs, generator=torch.Generator().manual_seed(5), dtype=torch.float64) * 2 - 1
        rec[f"{name}|x"] = x0.numpy()
        for mode in ("train", "eval"):
            net.load_state_dict(run, strict=False)   # the train call updated them
            net.train() if mode == "train" else net.eval()
            net.zero_grad()
            x = x0.clone().requires_grad_(True)
            out = net(x)
            out = out[0] if isinstance(out, tuple) else out
            Rw = torch.randn(out.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64)
            (out * Rw).sum().backward()
            p = f"{name}|{mode}"
            rec[f"{p}|out"] = out.detach().numpy()
            rec[f"{p}|dx"] = x.grad.numpy()
            g = torch.Generator().manual_seed(99)
            for k, prm in net.named_parameters():
                flat = prm.grad.reshape(-1)
                idx = torch.randint(0, flat.numel(), (min(64, flat.numel()),), generator=g)
                rec[f"{p}|{k}|idx"] = idx.numpy().astype(np.int64)
                rec[f"{p}|{k}|val"] = flat[idx].numpy()
                rec[f"{p}|{k}|norm"] = np.float64(flat.norm())
            for k, v in buffers_of(net).items():
                rec[f"{p}|after|{k}"] = v.numpy()
            print(p, "out", float(out.detach().abs().mean()))
    # the reference's BatchNorm state_dict() layout: G with default flags, D with n_layers 3
    for tag, net in (("G", R.ResnetUNetGenerator(1, 3, 64, norm_layer=R.get_norm_layer("batch"))),
                     ("D", R.NLayerDiscriminator(4, 64, n_layers=3, norm_layer=R.get_norm_layer("batch")))):
        sd = net.state_dict()
        rec[f"layout|{tag}|keys"] = np.array(list(sd.keys()))
        rec[f"layout|{tag}|shapes"] = np.array([",".join(str(d) for d in v.shape) for v in sd.values()])
        rec[f"layout|{tag}|dtypes"] = np.array([str(v.dtype) for v in sd.values()])
    out = os.path.join(HERE, "modules_bn.npz")
    np.savez_compressed(out, **rec)
    print("wrote", out, os.path.getsize(out), "bytes")


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 8))
    R = make_step()
    make_modules(R)


if __name__ == "__main__":
    main()
