"""Config.gan_mode in the fused train step: the fp32 parity mode against a CPU reference, the
module API's gan_loss_D against the fused step, and the fast dtypes.

The reference is oracle.step.train_step restated with the objective as a parameter, from the
oracle's own pieces (g_forward, d_forward, vgg_features, tv_loss, ssim_loss, adam_update): the
0.5 on D, D's Adam before G's GAN term and the other four G terms are those of ir:1647-1679.

Shapes, seeds, lambdas and tolerances are those of
test_gpu_step.py::test_step_fp32_vs_oracle_full_tensors (batch 2, 64x64, seed 11, the s64_smooth
golden's lambdas): losses within 1e-4 * max(1, |ref64|); every gradient of G and D but the
pre-InstanceNorm biases in relative L2 <= max(5e-3, 5 * err32), err32 the restated oracle's own
fp32-vs-fp64 distance; and the post-step parameters within 2 * lr + 1e-6 of the fp64 reference's
(Adam's first step moves every element by about lr).

Negative control, inside every case: the same reference under hinge differs from the case's in
gradD["model.8.weight"] by more than 10x that key's limit, so a step that ignored the option
could not pass.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, pkg
from oracle import step as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_KEYS = ("loss_D", "loss_G", "loss_G_GAN", "loss_G_L1", "loss_G_perc", "loss_G_TV", "loss_G_ssim")
LAMBDA_ORDER = ("lambda_L1", "lambda_perc", "lambda_tv", "lambda_ssim", "lambda_gan")
LR = 2e-4
SEED = 11
CONTROL_KEY = "model.8.weight"


def lambdas():
    return dict(zip(LAMBDA_ORDER, (float(v) for v in load_golden("s64_smooth")["lambdas"])))


def seeded():
    return (O.seeded_params(O.g_param_shapes(), 1, bias_std=0.02), O.seeded_params(O.d_param_shapes(), 2, bias_std=0.02),
            O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True))


def batch(seed=SEED, size=64):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, 1, size, size, generator=g) * 2 - 1, torch.rand(2, 3, size, size, generator=g) * 2 - 1


def make_trainer(dtype, mode, label, lam=None):
    irc = pkg()
    cfg = irc.Config()
    cfg.device = DEV
    cfg.compute_dtype = dtype
    for k, v in (lam or lambdas()).items():
        setattr(cfg, k, v)
    cfg.gan_mode, cfg.gan_real_label = mode, label
    tr = irc.GANTrainer(cfg)
    G, D, V = seeded()
    tr.netG.store.load(G, strict=True)
    tr.netD.store.load(D, strict=True)
    tr.vgg.store.load(V, strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    return tr, cfg


# ---- oracle.step.train_step with the objective as a parameter

def _term(x, y, mode):
    if mode == "lsgan":
        return ((x - y) ** 2).mean()
    return F.binary_cross_entropy_with_logits(x, torch.full_like(x, y))


def d_objective(pred_real, pred_fake, mode, t):
    if mode == "hinge":
        return 0.5 * (F.relu(1.0 - pred_real).mean() + F.relu(1.0 + pred_fake).mean())
    return 0.5 * (_term(pred_real, t, mode) + _term(pred_fake, 0.0, mode))


def g_objective(pred_fake, mode):
    return -pred_fake.mean() if mode == "hinge" else _term(pred_fake, 1.0, mode)


def train_step(G, D, V, ir, rgb, optG, optD, lam, mode, t):
    out = {}
    keys = [k for k in G if not k.endswith(".filt")]
    gk = {k: G[k].detach().clone().requires_grad_(k in keys) for k in G}
    fake = O.g_forward(gk, ir)
    # ---- D step (ir:1636-1651)
    dk = {k: D[k].detach().clone().requires_grad_(True) for k in D}
    pred_real = O.d_forward(dk, torch.cat([ir, rgb], 1))
    pred_fake = O.d_forward(dk, torch.cat([ir, fake.detach()], 1))
    loss_D = d_objective(pred_real, pred_fake, mode, t)
    out["gradD"] = dict(zip(D, torch.autograd.grad(loss_D, [dk[k] for k in D])))
    O.adam_update(D, out["gradD"], optD)
    # ---- G step (ir:1656-1681), D frozen at its updated weights
    l_gan = g_objective(O.d_forward(D, torch.cat([ir, fake], 1)), mode)
    l_l1 = (fake - rgb).abs().mean() * lam["lambda_L1"]
    l_perc = (O.vgg_features(V, fake) - O.vgg_features(V, rgb)).abs().mean() * lam["lambda_perc"]
    l_tv = O.tv_loss(fake) * lam["lambda_tv"]
    l_ssim = O.ssim_loss((fake + 1.0) / 2.0, (rgb + 1.0) / 2.0) * lam["lambda_ssim"]
    loss_G = lam["lambda_gan"] * l_gan + l_l1 + l_perc + l_tv + l_ssim
    out["gradG"] = dict(zip(keys, torch.autograd.grad(loss_G, [gk[k] for k in keys])))
    O.adam_update(G, out["gradG"], optG)
    out.update(loss_D=loss_D.item(), loss_G=loss_G.item(), loss_G_GAN=l_gan.item(), loss_G_L1=l_l1.item(),
               loss_G_perc=l_perc.item(), loss_G_TV=l_tv.item(), loss_G_ssim=l_ssim.item(), G=G, D=D)
    return out


@functools.lru_cache(maxsize=None)
def reference(mode, label, dtype):
    """The restated step on the seeded weights and batch.  Cached: computed once (the hinge
    reference serves every case's control), never written."""
    ir, rgb = batch()
    G, D, V = ({k: v.to(dtype).clone() for k, v in P.items()} for P in seeded())
    t = float(np.float32(label))     # the label as the library's float carries it
    return train_step(G, D, V, ir.to(dtype), rgb.to(dtype), O.AdamState(G, lr=LR), O.AdamState(D, lr=LR), lambdas(),
                      mode, t)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("mode,label", [("lsgan", 1.0), ("vanilla", 1.0), ("vanilla", 0.9)])
def test_step_fp32_vs_restated_oracle(mode, label):
    o64, o32 = reference(mode, label, torch.float64), reference(mode, label, torch.float32)
    hinge = reference("hinge", 1.0, torch.float64)
    tr, cfg = make_trainer("fp32", mode, label)
    assert cfg.lr_G == cfg.lr_D == LR
    ir, rgb = batch()
    d = tr.losses(tr.step(ir.to(DEV), rgb.to(DEV)))
    assert tuple(d) == LOSS_KEYS
    for k in LOSS_KEYS:
        print("STEP", mode, label, k, d[k], o64[k])
        assert abs(d[k] - o64[k]) <= 1e-4 * max(1.0, abs(o64[k])), (k, d[k], o64[k])
    pre_in = set(O.pre_in_bias_keys(list(o64["gradG"]) + list(o64["gradD"])))
    limits = {}
    for store, tag, post in ((tr.netG.store, "gradG", "G"), (tr.netD.store, "gradD", "D")):
        for k, g64 in o64[tag].items():
            moved = (store.oihw(k).cpu().double() - o64[post][k]).abs().max().item()
            assert moved <= 2 * LR + 1e-6, (post, k, moved)
            if k in pre_in:
                continue
            err32 = rel_l2(o32[tag][k], g64)
            limits[tag, k] = max(5e-3, 5 * err32)
            err = rel_l2(store.oihw(k, store.grad).cpu(), g64)
            assert err <= limits[tag, k], (tag, k, err, err32)
    # the control: under hinge this gradient is another one, far outside the limit it was held to
    away = rel_l2(hinge["gradD"][CONTROL_KEY], o64["gradD"][CONTROL_KEY])
    print("STEP", mode, label, "control: hinge vs case", away, "limit", limits["gradD", CONTROL_KEY])
    assert away > 10 * limits["gradD", CONTROL_KEY]


def test_module_api_gan_loss_d_matches_fused_trainer():
    """As test_gpu_module_api.py::test_module_api_matches_fused_trainer, with gan_loss_D in the
    torch hinge's place, under lsgan: the D step of a hand-written loop over netD(...) has the
    fused step's loss_D (1e-5 relative) and D gradients (1e-4 * max |ref|)."""
    irc = pkg()
    fx = load_golden("s32")
    lam = dict(zip(LAMBDA_ORDER, (float(v) for v in fx["lambdas"])))
    tr, cfg = make_trainer("fp32", "lsgan", 1.0, lam)
    G, D, _ = seeded()
    model = irc.IRColorizationModel(cfg)
    model.netG.load_state_dict(G)
    netD = irc.NLayerDiscriminator(input_nc=cfg.input_nc + cfg.output_nc, ndf=64, n_layers=3,
                                   norm_layer=irc.get_norm_layer(cfg.norm), device=DEV, compute_dtype="fp32")
    netD.load_state_dict(D)
    ir, rgb = torch.from_numpy(fx["ir"]).to(DEV), torch.from_numpy(fx["rgb"]).to(DEV)
    d = tr.losses(tr.step(ir, rgb))
    with torch.no_grad():
        fk = model(ir)
    ld = irc.gan_loss_D(netD(torch.cat([ir, rgb], 1)), netD(torch.cat([ir, fk], 1)), "lsgan")
    ld.backward()
    assert abs(ld.item() - d["loss_D"]) <= 1e-5 * max(1, abs(d["loss_D"])), (ld.item(), d["loss_D"])
    for k, p in netD.named_parameters():
        ref = tr.netD.store.oihw(k, tr.netD.store.grad)
        err = (p.grad - ref).abs().max().item()
        assert err <= 1e-4 * max(ref.abs().max().item(), 1e-6), (k, err)


@functools.lru_cache(maxsize=None)
def fp32_first_step_losses(mode):
    tr, _ = make_trainer("fp32", mode, 1.0)
    ir, rgb = batch(seed=12)
    return tr.losses(tr.step(ir.to(DEV), rgb.to(DEV)))


@pytest.mark.parametrize("mode", ["lsgan", "vanilla"])
@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_fast_dtypes_two_steps(dtype, mode):
    tr, _ = make_trainer(dtype, mode, 1.0)
    ir, rgb = (t.to(DEV) for t in batch(seed=12))
    g0, d0 = tr.netG.store.flat.clone(), tr.netD.store.flat.clone()
    first = tr.losses(tr.step(ir, rgb))
    second = tr.losses(tr.step(ir, rgb))
    for losses in (first, second):
        assert all(np.isfinite(v) for v in losses.values()), losses
    for store, before in ((tr.netG.store, g0), (tr.netD.store, d0)):
        assert torch.isfinite(store.flat).all() and not torch.equal(store.flat, before)
    if dtype == "bf16":   # the bf16 rule of test_gpu_step.py: 3e-2 relative of the fp32-mode step
        ref = fp32_first_step_losses(mode)
        for k in LOSS_KEYS:
            print("STEP bf16", mode, k, first[k], ref[k])
            assert abs(first[k] - ref[k]) <= 3e-2 * max(1.0, abs(ref[k])), (k, first[k], ref[k])
