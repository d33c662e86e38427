"""Config.clip_grad_G / clip_grad_D without a GPU: the options' defaults, validation before any
device work and command-line flags, the coefficient formula, GANStep.loss_dict's key sets, and
BucketedAllreduce.finish's schedule for a clipped step (one whole-buffer apply after every
bucket) against the unclipped one (per bucket), single-process and over two gloo ranks."""
import importlib
import math
import os
import socket
import types

import pytest
import torch

from conftest import pkg

LOSS_KEYS = ["loss_D", "loss_G", "loss_G_GAN", "loss_G_L1", "loss_G_perc", "loss_G_TV", "loss_G_ssim"]
WORLD = 2


def test_config_defaults_are_off():
    cfg = pkg().Config()
    assert cfg.clip_grad_G == 0.0 and cfg.clip_grad_D == 0.0


def test_command_line_flags():
    main = importlib.import_module(pkg().__name__ + ".__main__")
    cfg = main.config_from_argv(["train", "--clip-grad-G", "5", "--clip-grad-D", "0.25"])
    assert cfg.clip_grad_G == 5.0 and cfg.clip_grad_D == 0.25 and cfg.mode == "train"
    cfg = main.config_from_argv(["train", "--clip-grad-D", "2"])
    assert cfg.clip_grad_G == 0.0 and cfg.clip_grad_D == 2.0
    cfg = main.config_from_argv(["train"])
    assert cfg.clip_grad_G == cfg.clip_grad_D == 0.0


@pytest.mark.parametrize("name", ["clip_grad_G", "clip_grad_D"])
@pytest.mark.parametrize("value", [-1.0, float("nan"), float("inf"), -float("inf")])
def test_trainer_refuses_bad_max_norm_before_any_device_work(name, value, monkeypatch):
    irc = pkg()
    ic = importlib.import_module(irc.__name__ + ".ir_colorization")

    def no_gpu_work(*a, **k):
        raise AssertionError(f"a network was built before {name} was checked")
    monkeypatch.setattr(ic, "IRColorizationModel", no_gpu_work)
    monkeypatch.setattr(ic, "GANStep", no_gpu_work)
    cfg = irc.Config()
    cfg.device = "cpu"
    setattr(cfg, name, value)
    with pytest.raises(ValueError, match=name):
        irc.GANTrainer(cfg)


def test_clip_coef_is_torchs_formula():
    c = pkg().ops.clip_coef
    assert c(0.0, 0.5) == 1.0                       # an all-zero gradient is left alone
    assert c(1.0, 2.0) == 1.0 and c(2.0 - 1e-5, 2.0) == 1.0
    assert c(4.0, 2.0) == 2.0 / (4.0 + 1e-6) < 0.5
    assert c(2.0, 2.0) == 2.0 / (2.0 + 1e-6) < 1.0   # at the threshold the 1e-6 already binds, as in torch
    assert c(float("inf"), 2.0) == 0.0
    assert math.isnan(c(float("nan"), 2.0))          # no special handling (error_if_nonfinite=False)
    g = torch.randn(1000, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    p = torch.nn.Parameter(torch.zeros(1000, dtype=torch.float64))
    p.grad = g.clone()
    norm = float(torch.nn.utils.clip_grad_norm_([p], 3.0))
    assert torch.allclose(p.grad, g * c(norm, 3.0), rtol=1e-14, atol=0)


def test_reduction_grid_is_a_function_of_n_alone():
    parts = pkg().ops.grad_sumsq_parts
    assert [parts(n) for n in (0, 1, 1024, 1025, 5000)] == [0, 1, 1, 2, 5]
    assert parts(1024 * 1024) == 1024 == parts(1024 * 1024 + 1) == parts(45 << 20)


def test_loss_dict_key_sets():
    GANStep = pkg().engine.GANStep
    L = torch.tensor([1.0, 0.2, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], dtype=torch.float64)
    cfg = types.SimpleNamespace(lambda_gan=0.1)      # a config from before the options
    assert list(GANStep.loss_dict(L, cfg)) == LOSS_KEYS
    cfg = pkg().Config()
    off = GANStep.loss_dict(L, cfg)
    assert list(off) == LOSS_KEYS
    cfg.clip_grad_D = 1.0
    d = GANStep.loss_dict(L, cfg)
    assert list(d) == LOSS_KEYS + ["grad_norm_D"] and d["grad_norm_D"] == 7.0
    cfg.clip_grad_G = 2.0
    d = GANStep.loss_dict(L, cfg)
    assert list(d) == LOSS_KEYS + ["grad_norm_D", "grad_norm_G"] and d["grad_norm_G"] == 8.0
    cfg.clip_grad_D = 0.0
    assert list(GANStep.loss_dict(L, cfg)) == LOSS_KEYS + ["grad_norm_G"]
    assert {k: d[k] for k in LOSS_KEYS} == off


def _recorder(store, whole):
    calls = []

    def apply(a, b):
        calls.append((a, b, store.grad.clone() if whole else None))   # what a whole-buffer apply sees
    if whole:
        apply.whole = True
    return calls, apply


def test_finish_without_collectives_applies_once_either_way():
    engine = pkg().engine
    store = engine.ParamStore(engine.d_param_shapes(), "cpu", with_adam=False)
    for whole in (False, True):
        red = engine.BucketedAllreduce(store)
        assert not red.active
        calls, apply = _recorder(store, whole)
        red.ready(next(iter(store.shapes)))
        red.finish(apply)
        assert [(a, b) for a, b, _ in calls] == [(0, store.numel)]
    engine.BucketedAllreduce(store).finish()         # no apply: nothing to call


G_READY = ["up1_conv.0.weight"] + [f"resblocks.{b}.conv_block.1.weight" for b in reversed(range(9))]


def _finish_worker(rank, port, out):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        engine = pkg().engine
        res = {}
        for mode in ("bucketed", "whole"):
            store = engine.ParamStore(engine.g_param_shapes(), "cpu", with_adam=False)
            store.grad.copy_(torch.randn(store.numel, generator=torch.Generator().manual_seed(100 + rank)))
            red = engine.BucketedAllreduce(store, bucket_bytes=4 << 20)
            for k in G_READY:
                red.ready(k)
            issued = len(red.works)
            calls, apply = _recorder(store, mode == "whole")
            red.finish(apply)
            res[mode] = {"spans": [(a, b) for a, b, _ in calls], "issued": issued, "grad": store.grad.clone(),
                         "seen": calls[-1][2] if mode == "whole" else None, "left": (len(red.works), red.end)}
        torch.save(res, os.path.join(out, f"f{rank}.pt"))
    finally:
        dist.destroy_process_group()


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_finish_two_ranks_whole_apply_runs_once_after_every_bucket(tmp_path):
    import torch.multiprocessing as mp
    engine = pkg().engine
    mp.spawn(_finish_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    res = [torch.load(tmp_path / f"f{r}.pt", weights_only=True) for r in range(WORLD)]
    store = engine.ParamStore(engine.g_param_shapes(), "cpu", with_grad=False, with_adam=False)
    want = sum(torch.randn(store.numel, generator=torch.Generator().manual_seed(100 + r))
               for r in range(WORLD)) / WORLD
    for r in res:
        b, w = r["bucketed"], r["whole"]
        assert b["issued"] >= 4 and w["issued"] == b["issued"]     # the same buckets go out either way
        # unclipped: today's per-bucket calls, tail first, covering the buffer once
        spans = b["spans"]
        assert len(spans) == b["issued"] + 1
        assert spans[0][1] == store.numel and spans[-1][0] == 0
        assert all(spans[i][0] == spans[i + 1][1] for i in range(len(spans) - 1))
        # clipped: one call over the whole buffer, and what it saw was the finished mean
        assert w["spans"] == [(0, store.numel)]
        torch.testing.assert_close(w["seen"], want, rtol=1e-6, atol=1e-7)
        assert torch.equal(w["seen"], w["grad"]) and torch.equal(w["grad"], b["grad"])
        assert b["left"] == w["left"] == (0, store.numel)          # ready for the next step
    assert torch.equal(res[0]["whole"]["grad"], res[1]["whole"]["grad"])
