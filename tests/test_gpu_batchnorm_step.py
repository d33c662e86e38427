"""The fused train step with norm='batch' on the MI355X against the reference's golden vectors
(tests/golden/make_bn_golden.py -> step_s32_bn.npz, step_s32_bn_stats.npz: two steps of
ir:1636-1681 executed on the reference with nn.BatchNorm2d in G and D, fp32 and fp64).

Comparison rules: those of tests/test_gpu_step.py for step_s32.npz -- losses, G output and D
logits <= 1e-4 rel; post-step parameters within 2 lr; gradients (gamma / beta included) in
relative L2 against the fp64 run within max(5e-3, 5 err32l2); step-2 losses against fp64 within
max(1e-3, 3 |fp32 - fp64|).  Running buffers after each step against the fp64 record: max
|diff| <= max(10 x the reference's own |fp32 - fp64|, 1e-6 max |fp64|).  bf16: the step's
bf16-vs-fp32 bound of test_gpu_step.py (3e-2 rel).
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden, pkg
from oracle import step as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOSS_KEYS = ("loss_D", "loss_G", "loss_G_GAN", "loss_G_L1", "loss_G_perc", "loss_G_TV", "loss_G_ssim")
LAMBDA_ORDER = ("lambda_L1", "lambda_perc", "lambda_tv", "lambda_ssim", "lambda_gan")


@pytest.fixture(scope="module")
def fx():
    d = load_golden("s32_bn")
    d.update(np.load(os.path.join(GOLDEN, "step_s32_bn_stats.npz")))
    return d


def make_trainer(fx, dtype, seed_shift=0):
    irc = pkg()
    cfg = irc.Config()
    cfg.device = DEV
    cfg.compute_dtype = dtype
    cfg.norm = "batch"
    for k, v in zip(LAMBDA_ORDER, fx["lambdas"]):
        setattr(cfg, k, float(v))
    tr = irc.GANTrainer(cfg)
    G = O.seeded_params(O.g_param_shapes(use_bias=False), 1 + seed_shift, bias_std=0.02)
    D = O.seeded_params(O.d_param_shapes(use_bias=False), 2 + seed_shift, bias_std=0.02)
    for tag, sd in (("bnG|", G), ("bnD|", D)):
        sd.update({k[len(tag):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(tag)})
    assert set(tr.netG.store.shapes) == {k for k in G if not k.endswith(".filt")}
    assert set(tr.netD.store.shapes) == set(D)
    tr.netG.store.load(G)
    tr.netD.store.load(D)
    tr.vgg.store.load(O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True), strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    return tr, cfg


def digest_check(store, fx, tag, tol):
    """test_gpu_step.digest_check (l2 form) over every parameter, gamma / beta included; the
    1-D ones also in full against the fp64 run."""
    worst = 0.0
    for k in store.shapes:
        g = store.oihw(k, store.grad).reshape(-1).double().cpu().numpy()
        idx = fx[f"{tag}|{k}|idx"]
        post = store.oihw(k).reshape(-1).cpu().numpy()[idx]
        assert np.max(np.abs(post - fx[f"{tag}|{k}|post"])) <= 2 * 2e-4 + 1e-6, f"post-step {k}"
        lim = max(tol, 5 * float(fx[f"{tag}|{k}|err32l2"]))
        ref = fx[f"{tag}|{k}|val64"]
        err = np.linalg.norm(g[idx] - ref) / max(np.linalg.norm(ref), 1e-30)
        assert err <= lim, f"grad {k}: {err} > {lim}"
        if f"{tag}|{k}|full" in fx:
            full = fx[f"{tag}|{k}|full"]
            err = np.linalg.norm(g - full) / max(np.linalg.norm(full), 1e-30)
            assert err <= lim, f"full grad {k}: {err} > {lim}"
        worst = max(worst, err / lim)
    return worst


def running_check(tr, fx, step):
    """Running buffers against the fp64 record; returns the worst |diff| / bound."""
    worst = 0.0
    for tag, net, nbt in (("G", tr.netG, 2 * step), ("D", tr.netD, 3 * step)):
        for k, v in net.store.buffers.items():
            if k.endswith("num_batches_tracked"):
                assert v.dtype == torch.int64 and int(v) == nbt == int(fx[f"rs{step}|{tag}|{k}"]), (k, int(v))
                continue
            r32, r64 = fx[f"rs{step}|{tag}|{k}"].astype(np.float64), fx[f"rs{step}|{tag}|{k}_64"]
            bound = max(10 * np.max(np.abs(r32 - r64)), 1e-6 * np.max(np.abs(r64)))
            ratio = float(np.max(np.abs(v.double().cpu().numpy() - r64)) / bound)
            assert ratio <= 1.0, (step, tag, k, ratio)
            worst = max(worst, ratio)
    return worst


def test_batch_norm_step_fp32_matches_reference_golden(fx):
    """Two fp32 steps against the reference.  Measured on an MI355X: worst running-buffer
    |diff| / bound 0.103 after step 1 and 0.109 after step 2 (bound: 10 x the reference's own
    fp32-vs-fp64 difference, floor 1e-6 of the tensor's max); worst gradient error / bound 0.0004
    (D) and 0.20 (G).  G's eval-mode output after step 1: max |diff| 4.0e-6 against the
    reference's fp32 record (the asserted one, as for `fake`); 1.06e-4 against its fp64 record,
    from which the reference's own fp32 run is 1.08e-4 away (the parameters after Adam's first,
    sign-like step differ by up to 2 lr between any two runs)."""
    tr, cfg = make_trainer(fx, "fp32")
    ir, rgb = torch.from_numpy(fx["ir"]).to(DEV), torch.from_numpy(fx["rgb"]).to(DEV)
    d = tr.losses(tr.step(ir, rgb))
    for k in LOSS_KEYS:
        ref = fx["step1_" + k]
        assert abs(d[k] - ref) <= 1e-4 * max(1.0, abs(ref)), (k, d[k], ref)
    fake = tr.netG.engine.bufs.d["fake"].permute(0, 3, 1, 2).cpu().numpy()
    assert np.max(np.abs(fake - fx["fake"])) <= 1e-4
    De = tr.netD.engine   # the D step's logits on [real; fake] (tag "d"): two groups
    pred = De.bufs.d[f"de{len(De.packs) - 1}"].permute(0, 3, 1, 2).cpu().numpy()
    B = fx["ir"].shape[0]
    scale = max(np.max(np.abs(fx["pred_real"])), 1e-6)
    assert np.max(np.abs(pred[:B] - fx["pred_real"])) <= 1e-4 * max(1, scale)
    assert np.max(np.abs(pred[B:] - fx["pred_fake"])) <= 1e-4 * max(1, scale)
    print("grad worst err / bound: D", digest_check(tr.netD.store, fx, "gD", 5e-3),
          "G", digest_check(tr.netG.store, fx, "gG", 5e-3))
    print("running buffers after step 1: worst |diff| / bound", running_check(tr, fx, 1))
    # G in eval mode after step 1: the running statistics, and nothing is updated
    before = {k: v.clone() for k, v in tr.netG.store.buffers.items()}
    ev = tr.netG.engine.forward(ir, training=False).permute(0, 3, 1, 2).double().cpu().numpy()
    # forward outputs are held to the reference's fp32 record (as `fake` above and in
    # test_gpu_step.py); the fp64 record's figure is printed beside it
    e32, e64 = np.max(np.abs(ev - fx["eval_fake"])), np.max(np.abs(ev - fx["eval_fake_64"]))
    print("eval output after step 1: max |diff| vs the fp32 record", e32, "vs the fp64 record", e64,
          "(the reference's own fp32 vs fp64:", np.max(np.abs(fx["eval_fake"] - fx["eval_fake_64"])), ")")
    assert e32 <= 1e-4
    assert all(torch.equal(v, before[k]) for k, v in tr.netG.store.buffers.items())
    assert np.max(np.abs(ev - fx["fake64"])) > 1e-2     # and it is not the train-mode output
    d2 = tr.losses(tr.step(ir, rgb))
    for k in ("loss_D", "loss_G"):
        ref64, ref32 = float(fx["step2_" + k + "_64"]), float(fx["step2_" + k])
        assert abs(d2[k] - ref64) <= max(1e-3 * max(1.0, abs(ref64)), 3 * abs(ref32 - ref64)), (k, d2[k], ref64)
    print("running buffers after step 2: worst |diff| / bound", running_check(tr, fx, 2))


def test_batch_norm_step_bf16_close_to_fp32(fx):
    """The bf16 step at 32x32, B = 2: finite, losses and running buffers within the bf16-vs-fp32
    step bound (3e-2 rel, test_gpu_step.py) of the fp32 run's."""
    ir, rgb = torch.from_numpy(fx["ir"]).to(DEV), torch.from_numpy(fx["rgb"]).to(DEV)
    t16, _ = make_trainer(fx, "bf16")
    t32, _ = make_trainer(fx, "fp32")
    l16, l32 = t16.losses(t16.step(ir, rgb)), t32.losses(t32.step(ir, rgb))
    f16 = t16.netG.engine.bufs.d["fake"]
    assert torch.isfinite(f16).all() and f16.abs().max() <= 1.0
    for st in (t16.netG.store, t16.netD.store):
        assert torch.isfinite(st.grad).all() and torch.isfinite(st.flat).all()
    for k in LOSS_KEYS:
        assert np.isfinite(l16[k]), k
        if k != "loss_G_TV":
            assert abs(l16[k] - l32[k]) <= 3e-2 * max(1.0, abs(l32[k])), (k, l16[k], l32[k])
    for name in ("netG", "netD"):
        b16, b32 = getattr(t16, name).store.buffers, getattr(t32, name).store.buffers
        for k, v in b32.items():
            if k.endswith("num_batches_tracked"):
                assert int(b16[k]) == int(v)
                continue
            assert torch.isfinite(b16[k]).all(), k
            err = float((b16[k] - v).abs().max())
            assert err <= 3e-2 * max(1.0, float(v.abs().max())), (name, k, err)


def test_batch_norm_full_state_resume_is_bit_identical(fx, tmp_path):
    """The full state saved after step 1 and loaded into a fresh trainer (other weights, other
    running statistics): step 2 is bit-identical to the uninterrupted run's -- parameters,
    gradients, Adam moments, running buffers, num_batches_tracked (deterministic mode: no fp32
    atomics anywhere in the step)."""
    ops = pkg().ops
    ir, rgb = torch.from_numpy(fx["ir"]).to(DEV), torch.from_numpy(fx["rgb"]).to(DEV)
    old = ops.set_deterministic(True)
    try:
        a, _ = make_trainer(fx, "fp32")
        a.step(ir, rgb)
        path = tmp_path / "full.pt"
        a.save_checkpoint(path)
        sd = torch.load(path, map_location="cpu", weights_only=True)
        assert sd["netG"]["inc.2.num_batches_tracked"].dtype == torch.int64
        assert int(sd["netG"]["inc.2.num_batches_tracked"]) == 2 and int(sd["netD"]["model.3.num_batches_tracked"]) == 3
        la = a.losses(a.step(ir, rgb))
        b, _ = make_trainer(fx, "fp32", seed_shift=10)
        b.step(ir * 0.5, rgb)            # its own history, overwritten by the load
        b.load_checkpoint(path)
        lb = b.losses(b.step(ir, rgb))
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(old)
    for k in la:
        assert abs(la[k] - lb[k]) <= 1e-12 * max(1.0, abs(la[k])), (k, la[k], lb[k])
    for name in ("netG", "netD"):
        sa, sb = getattr(a, name).store, getattr(b, name).store
        assert torch.equal(sa.flat, sb.flat), f"{name} parameters"
        assert torch.equal(sa.grad, sb.grad), f"{name} gradients"
        assert torch.equal(sa.m, sb.m) and torch.equal(sa.v, sb.v), f"{name} Adam moments"
        for k, v in sa.buffers.items():
            assert torch.equal(v, sb.buffers[k]), (name, k)
        assert sa.step_count == sb.step_count == 2
