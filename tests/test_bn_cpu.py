"""norm='batch' without a GPU: the BatchNorm parameter layout against the reference's recorded
state_dict() (tests/golden/modules_bn.npz, made by executing the reference), the norm_layer
mapping, the host side of the parameter store, and the multi-rank refusal."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN, pkg


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "modules_bn.npz")))


def _layout(fx, tag):
    keys = [str(k) for k in fx[f"layout|{tag}|keys"]]
    shapes = [tuple(int(d) for d in str(s).split(",") if d) for s in fx[f"layout|{tag}|shapes"]]
    return keys, shapes


@pytest.mark.parametrize("tag", ["G", "D"])
def test_batch_norm_param_shapes_match_reference_state_dict(fx, tag):
    irc = pkg()
    got = irc.g_param_shapes(batch_norm=True) if tag == "G" else irc.d_param_shapes(n_layers=3, batch_norm=True)
    keys, shapes = _layout(fx, tag)
    assert list(got.keys()) == keys
    assert [tuple(v) for v in got.values()] == shapes
    # only outc.1 / model.0 / the last D conv keep a conv bias (use_bias False, ir:452-455, 590-593)
    conv_bias = [k for k in keys if k.endswith(".bias") and k[:-5] + ".running_mean" not in keys]
    assert conv_bias == (["outc.1.bias"] if tag == "G" else ["model.0.bias", "model.11.bias"])


def test_batch_norm_keys_follow_padding_and_dropout():
    """The ResnetBlock's BatchNorm modules sit right after its convs (res_conv_keys + 1)."""
    irc = pkg()
    from importlib import import_module
    eng = import_module(irc.__name__ + ".engine")
    for pad in ("reflect", "replicate", "zero"):
        for drop in (False, True):
            k1, k2 = eng.res_conv_keys(pad, drop)
            s = irc.g_param_shapes(n_blocks=1, padding_type=pad, use_dropout=drop, batch_norm=True)
            blk = [k for k in s if k.startswith("resblocks.0.")]
            want = []
            for c in (k1, k2):
                want += [f"resblocks.0.conv_block.{c}.weight"] + [
                    f"resblocks.0.conv_block.{c + 1}.{n}"
                    for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
            assert blk == want, (pad, drop)


def test_instance_and_none_layouts_unchanged():
    irc = pkg()
    from oracle import step as O
    assert irc.g_param_shapes() == O.g_param_shapes()
    assert irc.g_param_shapes(use_bias=False) == O.g_param_shapes(use_bias=False)
    assert irc.d_param_shapes() == O.d_param_shapes()
    assert irc.d_param_shapes(use_bias=False) == O.d_param_shapes(use_bias=False)


def test_norm_name_maps_batch_norm():
    irc = pkg()
    ic = __import__("importlib").import_module(irc.__name__ + ".ir_colorization")
    assert ic._norm_name(nn.BatchNorm2d) == "batch"
    assert ic._norm_name(functools.partial(nn.BatchNorm2d, affine=True)) == "batch"
    assert ic._norm_name(irc.get_norm_layer("batch")) == "batch"
    assert ic._norm_name(nn.InstanceNorm2d) == "instance"
    assert ic._norm_name(irc.get_norm_layer("none")) == "none"


def test_param_store_keeps_running_buffers_outside_the_flat_range():
    irc = pkg()
    eng = __import__("importlib").import_module(irc.__name__ + ".engine")
    shapes = irc.d_param_shapes(4, 8, 2, batch_norm=True)
    st = eng.ParamStore(shapes, torch.device("cpu"))
    bufs = [k for k in shapes if k.endswith((".running_mean", ".running_var", ".num_batches_tracked"))]
    assert list(st.buffers) == bufs and not set(bufs) & set(st.shapes)
    assert list(st.state()) == list(shapes)                      # state order == the reference's
    assert all(float(st.buffers[k].sum()) == 0 for k in bufs if not k.endswith("var"))
    assert all(bool((st.buffers[k] == 1).all()) for k in bufs if k.endswith("var"))
    assert st.buffers["model.3.num_batches_tracked"].dtype == torch.int64
    # Adam's parameter indices follow parameters() order: conv weight, BN weight, BN bias, ...
    sd = st.adam_state_dict(2e-4)
    assert sd["param_groups"][0]["params"] == list(range(len(st.shapes)))
    assert list(st.shapes)[:5] == ["model.0.weight", "model.0.bias", "model.2.weight", "model.3.weight", "model.3.bias"]
    # load / state round trip, buffers included
    g = torch.Generator().manual_seed(0)
    src = {k: torch.randn(v, generator=g) if len(v) else torch.tensor(7) for k, v in shapes.items()}
    st.load(src, strict=True)
    for k, v in st.state().items():
        assert torch.equal(v.float(), src[k].float()), k
    assert int(st.buffers["model.6.num_batches_tracked"]) == 7
    # a store without BatchNorm allocates no buffers
    assert not eng.ParamStore(irc.d_param_shapes(4, 8, 2), torch.device("cpu")).buffers


def test_multi_rank_batch_norm_is_refused_before_any_device_work(monkeypatch):
    irc = pkg()
    ic = __import__("importlib").import_module(irc.__name__ + ".ir_colorization")
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)

    def no_device_work(*a, **kw):
        raise AssertionError("the trainer built a network before refusing")
    monkeypatch.setattr(ic, "IRColorizationModel", no_device_work)
    monkeypatch.setattr(ic, "NLayerDiscriminator", no_device_work)
    cfg = irc.Config()
    cfg.device = "cuda:0"
    cfg.norm = "batch"
    with pytest.raises(NotImplementedError, match="SyncBN"):
        irc.GANTrainer(cfg)
    # world size 1 (and norm='instance' at any size) passes the check
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    ic._refuse_multi_rank_batch_norm(cfg)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    cfg.norm = "instance"
    ic._refuse_multi_rank_batch_norm(cfg)
