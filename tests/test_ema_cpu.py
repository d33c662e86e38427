"""Config.ema_decay without a GPU: the weight formula (ops.ema_weight), the option's default
and command-line flag, ParamStore's EMA buffer on the CPU, and GANTrainer's refusal of a decay
outside [0, 1) before any GPU work."""
import importlib

import pytest
import torch

from conftest import pkg


def test_ema_weight_first_step_is_warm_up():
    assert pkg().ops.ema_weight(0.999, 1) == 1.0 - 2.0 / 11.0


def test_ema_weight_reaches_one_minus_decay_and_stays():
    w, d = pkg().ops.ema_weight, 0.999
    first = next(t for t in range(1, 100000) if (1 + t) / (10 + t) >= d)
    assert first > 1 and w(d, first - 1) > 1 - d
    for t in (first, first + 1, 10 * first, 10 ** 7):
        assert w(d, t) == 1 - d


def test_ema_weight_is_non_increasing():
    w = pkg().ops.ema_weight
    for d in (0.5, 0.9, 0.999):
        ws = [w(d, t) for t in range(1, 12000)]
        assert all(a >= b for a, b in zip(ws, ws[1:]))
        assert all(0.0 < x < 1.0 for x in ws)


def test_config_default_is_off():
    assert pkg().Config().ema_decay == 0.0


def test_command_line_flag():
    main = importlib.import_module(pkg().__name__ + ".__main__")
    assert main.config_from_argv(["train", "--ema-decay", "0.999"]).ema_decay == 0.999
    assert main.config_from_argv(["train"]).ema_decay == pkg().Config().ema_decay == 0.0


def _store():
    irc = pkg()
    return irc.engine.ParamStore(irc.g_param_shapes(), "cpu")


def test_param_store_ema_buffer():
    S = _store()
    assert S.ema is None
    with pytest.raises(RuntimeError):
        S.swap_ema()
    S.flat.copy_(torch.randn(S.numel, generator=torch.Generator().manual_seed(0)))
    S.enable_ema()
    assert S.ema is not S.flat and S.ema.data_ptr() != S.flat.data_ptr()
    assert torch.equal(S.ema, S.flat)


def test_param_store_swap_twice_restores_both():
    S = _store()
    g = torch.Generator().manual_seed(1)
    S.flat.copy_(torch.randn(S.numel, generator=g))
    S.enable_ema()
    S.flat.add_(torch.randn(S.numel, generator=g))
    flat0, ema0 = S.flat.clone(), S.ema.clone()
    pf, pe = S.flat.data_ptr(), S.ema.data_ptr()
    assert not torch.equal(flat0, ema0)
    S.swap_ema()
    assert torch.equal(S.flat, ema0) and torch.equal(S.ema, flat0)
    assert (S.flat.data_ptr(), S.ema.data_ptr()) == (pf, pe)   # contents move, the tensors stay
    S.swap_ema()
    assert torch.equal(S.flat, flat0) and torch.equal(S.ema, ema0)


def test_param_store_ema_state_has_the_parameter_keys():
    S = _store()
    S.enable_ema()
    st = S.state(buf=S.ema)
    assert list(st) == list(S.shapes)
    assert all(tuple(v.shape) == S.shapes[k] for k, v in st.items())
    bn = pkg().engine.ParamStore(pkg().g_param_shapes(batch_norm=True, use_bias=False), "cpu")
    bn.enable_ema()
    assert bn.buffers and list(bn.state(buf=bn.ema)) == list(bn.shapes)   # no running statistics


@pytest.mark.parametrize("decay", [1.0, -0.1])
def test_trainer_refuses_decay_outside_the_unit_interval(decay, monkeypatch):
    irc = pkg()
    ic = importlib.import_module(irc.__name__ + ".ir_colorization")

    def no_gpu_work(*a, **k):
        raise AssertionError("a network was built before ema_decay was checked")
    monkeypatch.setattr(ic, "IRColorizationModel", no_gpu_work)
    monkeypatch.setattr(ic, "GANStep", no_gpu_work)
    cfg = irc.Config()
    cfg.device = "cpu"
    cfg.ema_decay = decay
    with pytest.raises(ValueError, match="ema_decay"):
        irc.GANTrainer(cfg)
