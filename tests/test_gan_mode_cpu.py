"""Config.gan_mode / gan_real_label without a GPU: the options' defaults, command-line flags,
validation before any device work, ops.gan_loss's refusal of an unknown mode before the library
is called, and GANStep.loss_dict's key set under every mode."""
import importlib
import types

import pytest
import torch

from conftest import pkg

LOSS_KEYS = ["loss_D", "loss_G", "loss_G_GAN", "loss_G_L1", "loss_G_perc", "loss_G_TV", "loss_G_ssim"]
SENTINEL = -7.0


def test_config_defaults_are_the_reference_objective():
    cfg = pkg().Config()
    assert cfg.gan_mode == "hinge" and cfg.gan_real_label == 1.0


def test_mode_codes():
    assert pkg().ops.GAN_MODES == {"hinge": 0, "lsgan": 1, "vanilla": 2}


def test_command_line_flags():
    main = importlib.import_module(pkg().__name__ + ".__main__")
    cfg = main.config_from_argv(["train", "--gan-mode", "lsgan", "--gan-real-label", "0.9"])
    assert cfg.gan_mode == "lsgan" and cfg.gan_real_label == 0.9 and cfg.mode == "train"
    cfg = main.config_from_argv(["train", "--gan-mode", "vanilla"])
    assert cfg.gan_mode == "vanilla" and cfg.gan_real_label == 1.0
    cfg = main.config_from_argv(["train", "--gan-mode", "hinge"])
    assert cfg.gan_mode == "hinge"
    cfg = main.config_from_argv(["train"])
    assert cfg.gan_mode == "hinge" and cfg.gan_real_label == 1.0
    with pytest.raises(SystemExit):
        main.config_from_argv(["train", "--gan-mode", "wgan"])


BAD = [("wgan", 1.0, "gan_mode")] + \
      [(mode, t, "gan_real_label") for mode in ("lsgan", "vanilla")
       for t in (0.0, -0.1, 1.5, float("nan"), float("inf"))] + \
      [("hinge", 0.9, "gan_real_label")]


@pytest.mark.parametrize("mode,label,name", BAD)
def test_trainer_refuses_bad_objective_before_any_device_work(mode, label, name, monkeypatch):
    irc = pkg()
    ic = importlib.import_module(irc.__name__ + ".ir_colorization")

    def no_gpu_work(*a, **k):
        raise AssertionError(f"a network was built before {name} was checked")
    monkeypatch.setattr(ic, "IRColorizationModel", no_gpu_work)
    monkeypatch.setattr(ic, "GANStep", no_gpu_work)
    cfg = irc.Config()
    cfg.device = "cpu"
    cfg.gan_mode, cfg.gan_real_label = mode, label
    with pytest.raises(ValueError, match=name):
        irc.GANTrainer(cfg)


@pytest.mark.parametrize("mode,label", [("hinge", 1.0), ("lsgan", 1.0), ("lsgan", 0.9), ("vanilla", 0.5),
                                        ("vanilla", 1e-3)])
def test_check_accepts_every_mode_and_smoothed_labels(mode, label):
    ic = importlib.import_module(pkg().__name__ + ".ir_colorization")
    cfg = pkg().Config()
    cfg.gan_mode, cfg.gan_real_label = mode, label
    assert ic._check_gan(cfg) == (mode, label)
    # a config object from before the options is the reference objective
    assert ic._check_gan(types.SimpleNamespace()) == ("hinge", 1.0)


@pytest.mark.parametrize("mode", ["wgan", "LSGAN", "", None, 1])
def test_ops_gan_loss_refuses_an_unknown_mode_before_the_library(mode):
    ops = pkg().ops
    pred = torch.zeros(8)
    grad = torch.full((8,), SENTINEL)
    loss = torch.full((1,), SENTINEL, dtype=torch.float64)
    with pytest.raises(ValueError, match="gan_mode"):
        ops.gan_loss(pred, 4, 0, mode, 1.0, 1.0, grad, loss)
    assert bool((grad == SENTINEL).all()) and loss.item() == SENTINEL


@pytest.mark.parametrize("mode", ["hinge", "lsgan", "vanilla"])
def test_loss_dict_key_set_is_unchanged_under_every_mode(mode):
    GANStep = pkg().engine.GANStep
    L = torch.tensor([1.0, 0.2, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0], dtype=torch.float64)
    cfg = pkg().Config()
    base = GANStep.loss_dict(L, cfg)
    cfg.gan_mode = mode
    d = GANStep.loss_dict(L, cfg)
    assert list(d) == LOSS_KEYS and d == base
    assert d["loss_G_GAN"] == 0.2 / cfg.lambda_gan
    # a config from before the option
    assert list(GANStep.loss_dict(L, types.SimpleNamespace(lambda_gan=0.1))) == LOSS_KEYS


def test_module_functions_are_public():
    irc = pkg()
    ic = importlib.import_module(irc.__name__ + ".ir_colorization")
    assert "gan_loss_D" in ic.__all__ and "gan_loss_G" in ic.__all__
    # no CPU fallback: a CPU tensor is refused, not computed
    with pytest.raises(RuntimeError, match="HIP device"):
        ic.gan_loss_D(torch.zeros(4), torch.zeros(4), "lsgan")
    with pytest.raises(RuntimeError, match="HIP device"):
        ic.gan_loss_G(torch.zeros(4), "vanilla")
