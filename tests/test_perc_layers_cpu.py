"""Config.perc_layers / perc_weights on the host: the defaults, _check_perc's accepted and refused
settings (the trainer calls it before any GPU work), and the two command-line flags."""
import importlib
import math

import pytest

from conftest import PKG_NAME, pkg

ALL = ("relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3")


def check(layers, weights=None):
    irc = pkg()
    cfg = irc.Config()
    cfg.perc_layers, cfg.perc_weights = layers, weights
    return irc.ir_colorization._check_perc(cfg)


def test_config_defaults():
    cfg = pkg().Config()
    assert cfg.perc_layers == ("relu3_3",)
    assert cfg.perc_weights is None
    assert pkg().ir_colorization._check_perc(cfg) == (("relu3_3", 1.0),)


def test_layer_names_are_torchvisions_relu_positions():
    assert pkg().engine.PERC_LAYERS == ALL


def test_vgg_stack_derives_todays_values():
    """VGG_CONVS, PERC_LAYERS and vgg_param_shapes() are derived from engine.VGG_STACK; pinned
    here to literals (checkpoints, the oracle and torchvision's state_dict depend on them)."""
    eng = pkg().engine
    assert eng.VGG_CONVS == ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256),
                             (14, 256, 256))
    assert eng.PERC_LAYERS == ("relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3")
    assert list(eng.vgg_param_shapes()) == ["0.weight", "0.bias", "2.weight", "2.bias", "5.weight", "5.bias",
                                            "7.weight", "7.bias", "10.weight", "10.bias", "12.weight", "12.bias",
                                            "14.weight", "14.bias"]
    assert [c.relu for c in eng.VGG_STACK if c.pool] == ["relu1_2", "relu2_2"]


def test_exports():
    irc = pkg()
    assert "perceptual_loss" in irc.ir_colorization.__all__
    assert callable(irc.perceptual_loss)


@pytest.mark.parametrize("layers,weights,want", [
    (("relu3_3",), None, (("relu3_3", 1.0),)),
    (ALL, None, tuple((n, 1.0) for n in ALL)),
    (["relu1_2", "relu2_2", "relu3_3"], [1, 0.5, 0.25], (("relu1_2", 1.0), ("relu2_2", 0.5), ("relu3_3", 0.25))),
    (("relu2_2",), (3.0,), (("relu2_2", 3.0),)),
])
def test_check_perc_accepts(layers, weights, want):
    assert check(layers, weights) == want


def test_check_perc_sorts_by_depth_and_drops_zero_weights():
    got = check(("relu3_3", "relu1_1", "relu2_2", "relu1_2"), (0.25, 2.0, 0.0, 1.0))
    assert got == (("relu1_1", 2.0), ("relu1_2", 1.0), ("relu3_3", 0.25))


@pytest.mark.parametrize("layers,weights", [
    (("relu4_1",), None),                               # unknown name
    (("relu3_3", "conv1_1"), None),
    (("relu1_2", "relu1_2"), None),                     # duplicate
    ((), None),                                         # empty
    ([], None),
    (("relu1_2", "relu3_3"), (1.0,)),                   # lengths differ
    (("relu1_2",), (1.0, 2.0)),
    (("relu1_2", "relu3_3"), (1.0, float("nan"))),      # not finite
    (("relu1_2", "relu3_3"), (1.0, math.inf)),
    (("relu1_2", "relu3_3"), (1.0, -0.5)),              # negative
    (("relu1_2", "relu3_3"), (0.0, 0.0)),               # all zero
])
def test_check_perc_refuses(layers, weights):
    with pytest.raises(ValueError, match="perc_"):
        check(layers, weights)


def test_argv_flags():
    main = importlib.import_module(PKG_NAME + ".__main__")
    cfg = main.config_from_argv(["train", "--perc-layers", "relu1_2,relu2_2,relu3_3", "--perc-weights", "1,0.5,0.25"])
    assert cfg.perc_layers == ("relu1_2", "relu2_2", "relu3_3")
    assert cfg.perc_weights == (1.0, 0.5, 0.25)
    assert pkg().ir_colorization._check_perc(cfg) == (("relu1_2", 1.0), ("relu2_2", 0.5), ("relu3_3", 0.25))
    cfg = main.config_from_argv(["train"])
    assert cfg.perc_layers == ("relu3_3",) and cfg.perc_weights is None
