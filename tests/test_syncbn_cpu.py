"""Config.sync_bn without a GPU: the default, and what it does to the multi-rank refusal of
norm='batch' (tests/test_bn_cpu.py pins the refusal itself)."""
import importlib

import pytest

from conftest import pkg


def _ic():
    return importlib.import_module(pkg().__name__ + ".ir_colorization")


def _world(monkeypatch, n):
    import torch.distributed as dist
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: n)


def test_sync_bn_defaults_to_off():
    assert pkg().Config().sync_bn is False


def test_sync_bn_lifts_the_multi_rank_refusal(monkeypatch):
    ic = _ic()
    _world(monkeypatch, 2)
    cfg = pkg().Config()
    cfg.norm = "batch"
    cfg.sync_bn = True
    assert ic._refuse_multi_rank_batch_norm(cfg) is None


def test_without_sync_bn_the_refusal_stays_and_names_the_option(monkeypatch):
    ic = _ic()
    _world(monkeypatch, 2)
    cfg = pkg().Config()
    cfg.norm = "batch"
    assert cfg.sync_bn is False
    with pytest.raises(NotImplementedError, match="SyncBN") as e:
        ic._refuse_multi_rank_batch_norm(cfg)
    assert "sync_bn" in str(e.value)
    del cfg.sync_bn   # a Config from before the option (read with getattr): still refused
    with pytest.raises(NotImplementedError, match="SyncBN"):
        ic._refuse_multi_rank_batch_norm(cfg)


def test_sync_bn_is_ignored_without_batch_norm(monkeypatch):
    ic = _ic()
    _world(monkeypatch, 2)
    cfg = pkg().Config()
    cfg.sync_bn = True
    for norm in ("instance", "none"):
        cfg.norm = norm
        assert ic._refuse_multi_rank_batch_norm(cfg) is None
