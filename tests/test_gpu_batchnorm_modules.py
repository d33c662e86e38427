"""norm='batch' through the module API on the MI355X, fp32 compute, against goldens made by
executing the reference in fp64 (tests/golden/make_bn_golden.py -> modules_bn.npz): train-mode
and eval-mode forward and gradients of a small generator (anti-aliased and not) and a small
discriminator; the state_dict round trip with the reference's BatchNorm checkpoint layout; and
a guard that the 'instance' / 'none' paths are untouched.

Tolerances: those of tests/test_gpu_module_variants.py for the norm='none' variants (outputs
<= 1e-4 abs, input gradients <= 1e-4 rel, parameter gradients rel-L2 <= 5e-3 on the sampled
entries and on the norm); running buffers after the train call: max-rel 1e-5 (the fp32 forward
bound of tests/test_gpu_kernels.py).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import GOLDEN, pkg
from oracle import step as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
BUFS = ("running_mean", "running_var", "num_batches_tracked")
CASES = {"bn_g": ("g", dict(no_antialias=False, no_antialias_up=False)),
         "bn_g_noaa": ("g", dict(no_antialias=True, no_antialias_up=True)),
         "bn_d": ("d", {})}


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(os.path.join(GOLDEN, "modules_bn.npz")))


def build(irc, fx, name):
    kind, kw = CASES[name]
    if kind == "g":
        net = irc.ResnetUNetGenerator(1, 3, 8, norm_layer=irc.get_norm_layer("batch"), n_blocks=2, padding_type="zero",
                                      device=DEV, compute_dtype="fp32", **kw)
        conv = O.seeded_params(O.g_param_shapes(ngf=8, n_blocks=2, use_bias=False, padding_type="zero", **kw), 1,
                               bias_std=0.02)
    else:
        net = irc.NLayerDiscriminator(4, 8, n_layers=2, norm_layer=irc.get_norm_layer("batch"), device=DEV,
                                      compute_dtype="fp32")
        conv = O.seeded_params(O.d_param_shapes(4, 8, 2, use_bias=False), 2, bias_std=0.02)
    pre = f"{name}|param|"
    stored = {k[len(pre):]: torch.from_numpy(v) for k, v in fx.items() if k.startswith(pre)}
    missing, unexpected = net.load_state_dict({**conv, **stored}, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    return net, stored


def grad_digest_close(fx, prefix, named, tol=5e-3):
    for k, g in named:
        flat = g.detach().reshape(-1).double().cpu().numpy()
        idx, ref = fx[f"{prefix}|{k}|idx"], fx[f"{prefix}|{k}|val"]
        nref = float(fx[f"{prefix}|{k}|norm"])
        err = np.linalg.norm(flat[idx] - ref) / max(np.linalg.norm(ref), 1e-30)
        nerr = abs(np.linalg.norm(flat) - nref) / max(nref, 1e-30)
        assert err <= tol and nerr <= tol, (prefix, k, err, nerr)


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("name", list(CASES))
def test_batch_norm_modules_vs_reference(fx, name, mode):
    irc = pkg()
    net, stored = build(irc, fx, name)
    net.train() if mode == "train" else net.eval()
    before = {k: v.clone() for k, v in net.state_dict().items() if k.endswith(BUFS)}
    x = torch.from_numpy(fx[f"{name}|x"]).float().to(DEV).requires_grad_(CASES[name][0] == "d")
    out = net(x)
    out = out[0] if isinstance(out, tuple) else out
    p = f"{name}|{mode}"
    ref = fx[f"{p}|out"]
    assert out.shape == ref.shape
    err = float(np.max(np.abs(out.detach().double().cpu().numpy() - ref)))
    print(p, "max |out - ref|", err)
    assert err <= 1e-4 * max(1.0, np.abs(ref).max())
    Rw = torch.randn(out.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64).float().to(DEV)
    (out * Rw).sum().backward()
    if x.requires_grad:
        dref = fx[f"{p}|dx"]
        assert float(np.max(np.abs(x.grad.double().cpu().numpy() - dref))) <= 1e-4 * np.abs(dref).max()
    grad_digest_close(fx, p, [(k, q.grad) for k, q in net.named_parameters()])
    after = {k: v for k, v in net.state_dict().items() if k.endswith(BUFS)}
    for k, v in after.items():
        if mode == "eval":   # running statistics used, nothing updated
            assert torch.equal(v, before[k]), k
        elif k.endswith("num_batches_tracked"):
            assert v.dtype == torch.int64 and int(v) == int(before[k]) + 1 == int(fx[f"{p}|after|{k}"]), k
        else:
            want = torch.from_numpy(fx[f"{p}|after|{k}"])
            assert float((v.double().cpu() - want).abs().max() / want.abs().max()) <= 1e-5, k


def test_separate_discriminator_calls_use_their_own_statistics(fx):
    """netD(real), netD(fake), then one backward (ir:1642-1650): each call normalises with its own
    batch's statistics, back-propagates through them, and updates the running buffers once."""
    irc = pkg()
    net, _ = build(irc, fx, "bn_d")
    ref, _ = build(irc, fx, "bn_d")
    x = torch.from_numpy(fx["bn_d|x"]).float().to(DEV)
    a, b = net(x), net(x * 0.5 + 0.1)
    (a.square().mean() + b.square().mean()).backward()
    ga = {k: p.grad.clone() for k, p in net.named_parameters()}
    ra = ref(x)
    ra.square().mean().backward()
    g1 = {k: p.grad.clone() for k, p in ref.named_parameters()}
    rb = ref(x * 0.5 + 0.1)
    rb.square().mean().backward()    # .grad accumulates: g1 + g2
    assert torch.equal(a, ra) and torch.equal(b, rb)
    for k, p in ref.named_parameters():
        assert float((ga[k] - p.grad).norm() / p.grad.norm().clamp_min(1e-30)) <= 1e-5, k
        assert not torch.equal(p.grad, g1[k])
    for k, v in net.state_dict().items():
        if k.endswith(BUFS):
            assert torch.equal(v, ref.state_dict()[k]), k
        if k.endswith("num_batches_tracked"):
            assert int(v) == 2


def plain_stack(sd):
    """A plain torch.nn module tree with the names of ``sd``: Conv2d / BatchNorm2d / a 'filt'
    buffer holder at each dotted path."""
    root = nn.Module()
    mods = list(dict.fromkeys(k.rsplit(".", 1)[0] for k in sd))   # in state order
    for path in mods:
        if path + ".running_mean" in sd:
            leaf = nn.BatchNorm2d(sd[path + ".weight"].shape[0])
        elif path + ".filt" in sd:
            leaf = nn.Module()
            leaf.register_buffer("filt", torch.zeros_like(sd[path + ".filt"]))
        else:
            O_, I, kh, kw = sd[path + ".weight"].shape
            leaf = nn.Conv2d(I, O_, (kh, kw), bias=path + ".bias" in sd)
        node = root
        parts = path.split(".")
        for q in parts[:-1]:
            if not hasattr(node, q):
                node.add_module(q, nn.Module())
            node = getattr(node, q)
        node.add_module(parts[-1], leaf)
    return root


@pytest.mark.parametrize("tag", ["G", "D"])
def test_state_dict_round_trip_with_reference_layout(fx, tag, tmp_path):
    irc = pkg()
    keys = [str(k) for k in fx[f"layout|{tag}|keys"]]
    shapes = [tuple(int(d) for d in str(s).split(",") if d) for s in fx[f"layout|{tag}|shapes"]]
    dtypes = [str(d) for d in fx[f"layout|{tag}|dtypes"]]
    norm = irc.get_norm_layer("batch")
    net = (irc.ResnetUNetGenerator(1, 3, 64, norm_layer=norm, device=DEV, compute_dtype="fp32") if tag == "G" else
           irc.NLayerDiscriminator(4, 64, n_layers=3, norm_layer=norm, device=DEV, compute_dtype="fp32"))
    g = torch.Generator().manual_seed(3)
    ckpt = {}
    for k, shp, dt in zip(keys, shapes, dtypes):   # a "reference checkpoint": its keys, shapes and dtypes
        if dt == "torch.int64":
            ckpt[k] = torch.tensor(5)
        elif k.endswith(".filt"):
            ckpt[k] = net.state_dict()[k].cpu().clone()
        else:
            ckpt[k] = torch.rand(shp, generator=g) + 0.5
    net.load_state_dict(ckpt, strict=True)
    sd = net.state_dict()
    assert list(sd.keys()) == keys
    for k, shp, dt in zip(keys, shapes, dtypes):
        assert tuple(sd[k].shape) == shp and str(sd[k].dtype) == dt, k
        assert torch.equal(sd[k].cpu(), ckpt[k]), k
    # the engine reads what was loaded: the BatchNorm layers' own views
    bn = next(n for n in (net.engine.norms.values() if tag == "G" else net.engine.norms) if n is not None)
    assert torch.equal(bn.running_var.cpu(), ckpt[bn.key + ".running_var"]) and int(bn.num_batches_tracked) == 5
    path = tmp_path / "net.pth"
    torch.save({k: v.detach().contiguous().cpu() for k, v in sd.items()}, path)
    back = torch.load(path, map_location="cpu", weights_only=True)
    plain = plain_stack(back)
    plain.load_state_dict(back, strict=True)
    assert list(plain.state_dict().keys()) == keys
    # init_weights: BatchNorm weight ~ N(1, gain), bias 0, conv weights ~ N(0, gain) from one generator
    irc.init_weights(net, "normal", 0.02, generator=torch.Generator().manual_seed(1))
    gen = torch.Generator().manual_seed(1)
    for k, p in net.named_parameters():
        if k.endswith(".weight"):
            want = torch.empty(p.shape).normal_(1.0 if p.dim() == 1 else 0.0, 0.02, generator=gen)
            assert torch.equal(p.detach().cpu(), want), k
        else:
            assert not p.detach().any(), k


@pytest.mark.parametrize("norm", ["instance", "none"])
def test_instance_and_none_paths_untouched(norm, monkeypatch):
    """An 'instance' / 'none' generator and discriminator built through the new construction
    code (make_norm with the store and key, the norm-module slots) give the same bits as ones
    built with that code switched off, and allocate no BatchNorm buffers."""
    import importlib
    irc = pkg()
    eng = importlib.import_module(irc.__name__ + ".engine")
    ic = importlib.import_module(irc.__name__ + ".ir_colorization")

    def make():
        G = irc.ResnetUNetGenerator(1, 3, 64, norm_layer=irc.get_norm_layer(norm), n_blocks=1, device=DEV)
        D = irc.NLayerDiscriminator(4, 64, n_layers=2, norm_layer=irc.get_norm_layer(norm), device=DEV)
        for net, seed in ((G, 1), (D, 2)):
            assert not net.store.buffers and not any(k.endswith(BUFS) for k in net.state_dict())
            assert not any(k.startswith(("ab_", "bn_")) for k in list(net.engine.bufs.d) + list(net.engine.bufs.state))
            irc.init_weights(net, "normal", 0.02, generator=torch.Generator().manual_seed(seed))
        g = torch.Generator().manual_seed(4)
        x = (torch.rand(2, 1, 24, 20, generator=g) * 2 - 1).to(DEV)
        xd = (torch.rand(2, 4, 24, 20, generator=g) * 2 - 1).to(DEV)
        with torch.no_grad():
            return G(x)[0].clone(), D(xd).clone()
    new = make()
    old_make = {"instance": eng.INLayer, "none": eng.NoNorm}
    monkeypatch.setattr(eng, "make_norm", lambda n, store=None, key=None: old_make[n if n else "none"]())
    monkeypatch.setattr(ic, "_norm_slot", lambda store, key: None)
    old = make()
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])
