"""Config.perc_layers / perc_weights in the fused train step: the fp32 parity mode against a CPU
reference, the default left bit-identical, the module API's perceptual_loss, the fast dtypes
and the unfused composition (engine.NO_TAP_FUSION).

The reference is test_gpu_gan_mode_step.py's restated oracle.step.train_step under hinge with the
perceptual term taken over a list of VGG maps, rebuilt here from the oracle's pieces (VGG_CONVS,
IMAGENET_MEAN / STD, g_forward, d_forward, tv_loss, ssim_loss, adam_update):
loss_G_perc = lambda_perc * sum_l w_l * mean|phi_l(fake) - phi_l(rgb)|.

Batch 2, 64x64, seed 11, the seeded G / D / VGG of that file and Config's own lambdas (30, 30,
1e-4, 2, 0.1: the s64_smooth golden has lambda_perc = 0).  Bounds as there: losses within
1e-4 * max(1, |ref64|); every gradient of G but the pre-InstanceNorm biases in relative L2 <=
max(5e-3, 5 * err32), err32 the restated oracle's own fp32-vs-fp64 distance; the post-step
parameters within 2 * lr + 1e-6 of the fp64 reference's.

Negative control, inside every case: the relu3_3-only reference differs from the case's in
gradG["outc.1.weight"] by more than 10x that key's limit, so a step that ignored the option could
not pass.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC
from conftest import pkg
from oracle import step as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_KEYS = ("loss_D", "loss_G", "loss_G_GAN", "loss_G_L1", "loss_G_perc", "loss_G_TV", "loss_G_ssim")
LAMBDAS = dict(lambda_L1=30.0, lambda_perc=30.0, lambda_tv=1e-4, lambda_ssim=2.0, lambda_gan=0.1)
LAYERS = ("relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3")
LR = 2e-4
SEED = 11
CONTROL_KEY = "outc.1.weight"
THREE = (("relu1_2", "relu2_2", "relu3_3"), (1.0, 0.5, 0.25))
CASES = [THREE, (("relu2_2",), None), (("relu1_1", "relu3_1"), None)]
CASE_IDS = ["three-weighted", "relu2_2-alone", "no-pooled-tap"]


def seeded():
    return (O.seeded_params(O.g_param_shapes(), 1, bias_std=0.02), O.seeded_params(O.d_param_shapes(), 2, bias_std=0.02),
            O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True))


def batch(seed=SEED, size=(64, 64)):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, 1, *size, generator=g) * 2 - 1, torch.rand(2, 3, *size, generator=g) * 2 - 1


def make_trainer(dtype, layers=None, weights=None, deterministic=False):
    irc = pkg()
    cfg = irc.Config()
    cfg.device = DEV
    cfg.compute_dtype = dtype
    cfg.deterministic = deterministic
    for k, v in LAMBDAS.items():
        assert getattr(cfg, k) == v   # Config's defaults
    if layers is not None:
        cfg.perc_layers, cfg.perc_weights = layers, weights
    tr = irc.GANTrainer(cfg)
    G, D, V = seeded()
    tr.netG.store.load(G, strict=True)
    tr.netD.store.load(D, strict=True)
    tr.vgg.store.load(V, strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    return tr, cfg


@pytest.fixture
def restore_deterministic():
    ops = pkg().ops
    old = ops.set_deterministic(False)
    ops.set_deterministic(old)
    yield
    ops.set_deterministic(old)


# ---- the reference: oracle.step's pieces, the perceptual term over a list of maps

def vgg_maps(V, x):
    """The seven ReLU maps of vgg16.features[:16] (oracle.step.vgg_features, every map kept)."""
    mean = torch.tensor(O.IMAGENET_MEAN, dtype=x.dtype).view(1, 3, 1, 1)
    std = torch.tensor(O.IMAGENET_STD, dtype=x.dtype).view(1, 3, 1, 1)
    h = ((x + 1.0) / 2.0 - mean) / std
    maps = {}
    for name, (i, _, _) in zip(LAYERS, O.VGG_CONVS):
        h = F.relu(F.conv2d(h, V[f"{i}.weight"], V[f"{i}.bias"], padding=1))
        maps[name] = h
        if i in (2, 7):
            h = F.max_pool2d(h, 2)
    return maps


def perc_term(V, fake, rgb, layers, weights):
    weights = weights or (1.0,) * len(layers)
    mf, mr = vgg_maps(V, fake), vgg_maps(V, rgb)
    return sum(w * (mf[n] - mr[n]).abs().mean() for n, w in zip(layers, weights))


def train_step(G, D, V, ir, rgb, optG, optD, lam, layers, weights):
    out = {}
    keys = [k for k in G if not k.endswith(".filt")]
    gk = {k: G[k].detach().clone().requires_grad_(k in keys) for k in G}
    fake = O.g_forward(gk, ir)
    # ---- D step (ir:1636-1651)
    dk = {k: D[k].detach().clone().requires_grad_(True) for k in D}
    pred_real = O.d_forward(dk, torch.cat([ir, rgb], 1))
    pred_fake = O.d_forward(dk, torch.cat([ir, fake.detach()], 1))
    loss_D = 0.5 * (F.relu(1.0 - pred_real).mean() + F.relu(1.0 + pred_fake).mean())
    out["gradD"] = dict(zip(D, torch.autograd.grad(loss_D, [dk[k] for k in D])))
    O.adam_update(D, out["gradD"], optD)
    # ---- G step (ir:1656-1681), D frozen at its updated weights
    l_gan = -O.d_forward(D, torch.cat([ir, fake], 1)).mean()
    l_l1 = (fake - rgb).abs().mean() * lam["lambda_L1"]
    l_perc = perc_term(V, fake, rgb, layers, weights) * lam["lambda_perc"]
    l_tv = O.tv_loss(fake) * lam["lambda_tv"]
    l_ssim = O.ssim_loss((fake + 1.0) / 2.0, (rgb + 1.0) / 2.0) * lam["lambda_ssim"]
    loss_G = lam["lambda_gan"] * l_gan + l_l1 + l_perc + l_tv + l_ssim
    out["gradG"] = dict(zip(keys, torch.autograd.grad(loss_G, [gk[k] for k in keys])))
    O.adam_update(G, out["gradG"], optG)
    out.update(loss_D=loss_D.item(), loss_G=loss_G.item(), loss_G_GAN=l_gan.item(), loss_G_L1=l_l1.item(),
               loss_G_perc=l_perc.item(), loss_G_TV=l_tv.item(), loss_G_ssim=l_ssim.item(), G=G, D=D)
    return out


@functools.lru_cache(maxsize=None)
def reference(layers, weights, dtype):
    """The restated step on the seeded weights and batch.  Cached: computed once (the relu3_3
    reference serves every case's control), never written."""
    ir, rgb = batch()
    G, D, V = ({k: v.to(dtype).clone() for k, v in P.items()} for P in seeded())
    return train_step(G, D, V, ir.to(dtype), rgb.to(dtype), O.AdamState(G, lr=LR), O.AdamState(D, lr=LR), LAMBDAS,
                      layers, weights)


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30))


@pytest.mark.parametrize("layers,weights", CASES, ids=CASE_IDS)
def test_step_fp32_vs_restated_oracle(layers, weights):
    o64, o32 = reference(layers, weights, torch.float64), reference(layers, weights, torch.float32)
    plain = reference(("relu3_3",), None, torch.float64)
    tr, cfg = make_trainer("fp32", layers, weights)
    assert cfg.lr_G == cfg.lr_D == LR
    ir, rgb = batch()
    d = tr.losses(tr.step(ir.to(DEV), rgb.to(DEV)))
    assert tuple(d) == LOSS_KEYS
    for k in LOSS_KEYS:
        print("STEP", layers, k, d[k], o64[k])
        assert abs(d[k] - o64[k]) <= 1e-4 * max(1.0, abs(o64[k])), (k, d[k], o64[k])
    pre_in = set(O.pre_in_bias_keys(list(o64["gradG"])))
    limits = {}
    store = tr.netG.store
    for k, g64 in o64["gradG"].items():
        moved = (store.oihw(k).cpu().double() - o64["G"][k]).abs().max().item()
        assert moved <= 2 * LR + 1e-6, (k, moved)
        if k in pre_in:
            continue
        err32 = rel_l2(o32["gradG"][k], g64)
        limits[k] = max(5e-3, 5 * err32)
        err = rel_l2(store.oihw(k, store.grad).cpu(), g64)
        assert err <= limits[k], (k, err, err32)
    # the control: with relu3_3 alone this gradient is another one, far outside the limit it was held to
    away = rel_l2(plain["gradG"][CONTROL_KEY], o64["gradG"][CONTROL_KEY])
    print("STEP", layers, "control: relu3_3 vs case", away, "limit", limits[CONTROL_KEY])
    assert away > 10 * limits[CONTROL_KEY]


def test_default_is_bit_identical_to_explicit_relu3_3(restore_deterministic):
    """The attributes left alone and ("relu3_3",) at (1.0,) are one step: the same loss vector and
    the same G gradients, bit for bit (fp32 mode, deterministic)."""
    ir, rgb = (t.to(DEV) for t in batch())
    got = []
    for layers, weights in ((None, None), (("relu3_3",), (1.0,))):
        tr, _ = make_trainer("fp32", layers, weights, deterministic=True)
        assert tr.core.perc_taps is None   # the reference's launches, not the tap kernels
        L = tr.step(ir, rgb).clone()
        got.append((L, tr.netG.store.grad.clone()))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert got[0][0][3].item() > 0


def test_module_api_value_matches_fused_step():
    irc = pkg()
    layers, weights = THREE
    tr, cfg = make_trainer("fp32", layers, weights)
    ir, rgb = (t.to(DEV) for t in batch())
    with torch.no_grad():
        fake = tr.model(ir)   # before the step moves G
    d = tr.losses(tr.step(ir, rgb))
    got = cfg.lambda_perc * irc.perceptual_loss(tr.vgg, fake, rgb, layers, weights).item()
    print("API value", got, d["loss_G_perc"])
    assert abs(got - d["loss_G_perc"]) <= 1e-5 * abs(d["loss_G_perc"])


def test_module_api_gradient_vs_fp64_with_the_unfused_fallback():
    """38x46: relu1_2 (38x46) takes the fused pool backward, relu2_2 (19x23) is refused and takes
    maxpool_bwd + l1_tap, whose last row and column carry tap gradient only."""
    irc = pkg()
    layers, weights = THREE
    _, _, V = seeded()
    vgg = irc.VGGPerceptual(DEV, compute_dtype="fp32")
    vgg.store.load(V, strict=True)
    vgg.repack()
    fake, real = batch(seed=13, size=(38, 46))[1], batch(seed=14, size=(38, 46))[1]
    refs = {}
    for dt in (torch.float64, torch.float32):
        f = fake.to(dt).clone().requires_grad_(True)
        val = perc_term({k: v.to(dt) for k, v in V.items()}, f, real.to(dt), layers, weights)
        refs[dt] = (val.item(), torch.autograd.grad(val, f)[0])
    f = fake.to(DEV).requires_grad_(True)
    r = real.to(DEV).requires_grad_(True)
    val = irc.perceptual_loss(vgg, f, r, layers, weights)
    val.backward()
    assert r.grad is None
    v64, g64 = refs[torch.float64]
    err32 = rel_l2(refs[torch.float32][1], g64)
    err = rel_l2(f.grad.cpu(), g64)
    print("API grad", err, "err32", err32, "value", val.item(), v64)
    assert abs(val.item() - v64) <= 1e-4 * max(1.0, abs(v64))
    assert err <= max(5e-3, 5 * err32)
    # upstream gradients scale it
    f2 = fake.to(DEV).requires_grad_(True)
    (2.5 * irc.perceptual_loss(vgg, f2, real.to(DEV), layers, weights)).backward()
    assert torch.allclose(f2.grad, 2.5 * f.grad, rtol=1e-6, atol=0)


@functools.lru_cache(maxsize=None)
def fp32_first_step_losses():
    tr, _ = make_trainer("fp32", *THREE)
    ir, rgb = batch(seed=12)
    return tr.losses(tr.step(ir.to(DEV), rgb.to(DEV)))


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_fast_dtypes_two_steps(dtype):
    tr, _ = make_trainer(dtype, *THREE)
    ir, rgb = (t.to(DEV) for t in batch(seed=12))
    g0, d0 = tr.netG.store.flat.clone(), tr.netD.store.flat.clone()
    first = tr.losses(tr.step(ir, rgb))
    second = tr.losses(tr.step(ir, rgb))
    for losses in (first, second):
        assert all(np.isfinite(v) for v in losses.values()), losses
    for store, before in ((tr.netG.store, g0), (tr.netD.store, d0)):
        assert torch.isfinite(store.flat).all() and not torch.equal(store.flat, before)
    if dtype == "bf16":   # the bf16 rule of test_gpu_step.py: 3e-2 relative of the fp32-mode step
        ref = fp32_first_step_losses()
        for k in LOSS_KEYS:
            print("STEP bf16", k, first[k], ref[k])
            assert abs(first[k] - ref[k]) <= 3e-2 * max(1.0, abs(ref[k])), (k, first[k], ref[k])


def test_no_tap_fusion_is_the_same_step(monkeypatch, restore_deterministic):
    """engine.NO_TAP_FUSION (maxpool_bwd, then l1_tap over the whole map) against the fused pool
    backward, bf16, three layers: the same image gradient bit for bit (both round one fp32 sum
    once), the perceptual loss within R_ACC (another summation order)."""
    engine = pkg().engine
    ir, rgb = (t.to(DEV) for t in batch(seed=12))
    got = []
    for off in (False, True):
        monkeypatch.setattr(engine, "NO_TAP_FUSION", off)
        tr, _ = make_trainer("bf16", *THREE, deterministic=True)
        L = tr.step(ir, rgb).clone()
        got.append((L[3].item(), tr.vgg.engine.bufs.d["dvin"].clone(), tr.core.bufs.d["dfake"].clone()))
    (l0, dv0, df0), (l1, dv1, df1) = got
    print("NO_TAP_FUSION perc", l0, l1)
    assert torch.equal(dv0, dv1) and torch.equal(df0, df1)
    assert dv0.abs().max().item() > 0
    assert abs(l0 - l1) <= LC.R_ACC * abs(l0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_backward_input_and_backward_taps_are_one_walk(dtype):
    """VGGEngine's two public backwards are one walk under two seeds: after one forward of a 2+2
    batch (24x40, so the maps 24x40, 12x20 and 6x10 are all even), ops.l1 into dfeat followed by
    backward_input and backward_taps(DEFAULT_TAPS) give the same dvin -- value equality: the seeds
    differ only in the sign of their zeros -- and the same loss within R_ACC."""
    irc = pkg()
    ops, B = irc.ops, 2
    vgg = irc.VGGPerceptual(DEV, compute_dtype=dtype)
    vgg.store.load(seeded()[2], strict=True)
    vgg.repack()
    eng = vgg.engine
    both = torch.cat([batch(seed=13, size=(24, 40))[1], batch(seed=14, size=(24, 40))[1]]).to(DEV)
    feat = eng.forward(irc.ir_colorization._nhwc_input(both, eng.packs[0], eng.tdt, eng.scale, eng.shift))
    assert (feat.N, feat.H, feat.W) == (2 * B, 6, 10)
    loss_a, loss_b = (torch.zeros(1, dtype=torch.float64, device=DEV) for _ in range(2))
    dfeat = torch.empty_like(feat.t[:B])
    ops.l1(feat.t[:B], feat.t[B:], 1.0, dfeat, loss_a)
    dv_a = eng.backward_input(ops.Feat(dfeat), B).t.clone()
    dv_b = eng.backward_taps(irc.engine.DEFAULT_TAPS, B, 1.0, loss_b).t.clone()
    print("ONE WALK", dtype, "loss", loss_a.item(), loss_b.item(), "max|dvin|", dv_a.abs().max().item())
    assert torch.equal(dv_a, dv_b)
    assert dv_a.abs().max().item() > 0
    assert abs(loss_a.item() - loss_b.item()) <= LC.R_ACC * abs(loss_a.item())
