"""gan_loss_kernel of csrc/loss.hip (``ops.gan_loss``: the LSGAN and BCE objectives of
Config.gan_mode) against fp64 autograd on the CPU, with the conventions of test_gpu_losses.py:
the fp64 loss word pre-filled with LOSS0 (the kernel adds to it), the gradient buffer pre-filled
with junk that must be overwritten (the kernel writes), scale = 0.37.

Shapes
  side 0, n_half = 70001   2n = 140002 > 512 * 256: a second grid-stride round; the real / fake
                           boundary ``i < n`` falls inside a wave (70001 % 64 = 49)
  side 1, n = 140003
  n_half in {1, 63, 65}    ragged single blocks, the boundary inside / just past the first wave
Planted in every half (40 of each at the large sizes, as many as fit at the small ones): exactly
0, +-1, +-30, +-88, +-100 and t.  exp(88) and exp(100) overflow fp32, so a naive sigmoid or
log(1 + exp(x)) shows as inf / NaN; an element equal to its target t gives an LSGAN gradient of
exactly 0.

Modes x labels: lsgan and vanilla, each with t = 1 and t = fp32(0.9).  The fp64 reference uses
the fp32-rounded label, which is what the ABI receives (a ``float``): with the Python double 0.9
the planted element differs from the target by 2^-26 relative instead of 0.

Bounds, U = 2^-24 (one fp32 rounding, relative):
  LSGAN gradient  |got - g64| <= 4 U |g64| per element (the rule of the hinge tests).  The kernel
                  spends two of them: scale arrives rounded to fp32 and the result is rounded
                  once; the subtraction and the products between run in fp64.
  BCE gradient    |got - g64| <= 8 U c scale / n absolute, c = 0.5 on side 0 and 1 on side 1: the
                  sigmoid is at most 1 and carries expf, an add, a divide, the subtraction of the
                  label and two scalings.  Absolute, because sigmoid(x) - 1 cancels.
  loss word       within LC.R_ACC * ref (every term is non-negative)
  every output finite.
Module functions (gan_loss_D / gan_loss_G, scale 1): the same bounds times the upstream gradient
1.75 -- exact in fp32, so that the product with it adds one rounding, inside the LSGAN rule's
four; the value, returned as fp32, within LC.R_ACC * ref.

The worst err / bound of every case on the MI355X is recorded in profiles/gan_loss_parity.txt.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
LOSS0 = LC.LOSS0
SCALE = 0.37
T09 = float(np.float32(0.9))     # the label as the ABI's float carries it
LABELS = {"t1": 1.0, "t0.9": T09}
PLANT = (0.0, 1.0, -1.0, 30.0, -30.0, 88.0, -88.0, 100.0, -100.0)


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


def loss_word():
    return torch.full((1,), LOSS0, dtype=torch.float64, device=DEV)


def report(what, **figs):
    print("PARITY " + what + ": " + ", ".join(f"{k} = {v:.3g}" for k, v in figs.items()))


def half(n, t, gen):
    """One half's logits: N(0, 1.5^2) with the planted values (and the label t) at random places,
    40 of each, or as many of each as fit; a half shorter than the list takes values from it in turn
    (n = 1: -88, far from every target, so that no objective's loss drowns in the LOSS0 it is added
    to: bce(30, 1) = 9e-14 sits at the fp64 word's own rounding)."""
    p = torch.randn(n, generator=gen) * 1.5
    vals = PLANT + (t,)
    per = min(40, n // len(vals))
    if per:
        at = torch.randperm(n, generator=gen)[:per * len(vals)]
        for j, v in enumerate(vals):
            p[at[j * per:(j + 1) * per]] = v
    else:
        for j in range(n):
            p[j] = vals[(j * 7 + n + 5) % len(vals)]   # n = 1: -88
    return p


@functools.lru_cache(maxsize=None)
def case(side, n, tname):
    """(p fp32, n, t) of a case.  Cached: built once, never written."""
    t = LABELS[tname]
    gen = torch.Generator().manual_seed(1000 * side + n)
    p = torch.cat([half(n, t, gen), half(n, t, gen)]) if side == 0 else half(n, t, gen)
    return p, t


def term(x, y, mode):
    if mode == "lsgan":
        return (x - y) ** 2
    return F.binary_cross_entropy_with_logits(x, torch.full_like(x, y), reduction="none")


def objective(p, n, side, mode, t):
    """The table of INTEGRATION.md s.11 in the dtype of p, unscaled."""
    if side == 0:
        return 0.5 * (term(p[:n], t, mode).mean() + term(p[n:], 0.0, mode).mean())
    return term(p, 1.0, mode).mean()


@functools.lru_cache(maxsize=None)
def reference(side, n, tname, mode, dtype=torch.float64):
    """(loss, grad) of scale * objective by autograd in ``dtype`` on the CPU."""
    p, t = case(side, n, tname)
    x = p.to(dtype, copy=True).requires_grad_(True)
    ref = objective(x, n, side, mode, t) * SCALE
    ref.backward()
    return ref.item(), x.grad.detach()


def grad_bound(g64, side, n, mode, w=SCALE):
    if mode == "lsgan":
        return 4 * U * g64.abs() + 1e-300
    return torch.full_like(g64, 8 * U * (0.5 if side == 0 else 1.0) * w / n)


def run(ops, p, n, side, mode, t):
    pd = p.to(DEV)
    grad = torch.randn(p.numel(), generator=torch.Generator().manual_seed(3)).to(DEV) + 2.0   # overwritten
    loss = loss_word()
    ops.gan_loss(pd, n, side, mode, t, SCALE, grad, loss)
    return loss.item() - LOSS0, grad.cpu()


CASES = [(0, 70001), (1, 140003), (0, 1), (0, 63), (0, 65), (1, 1), (1, 63), (1, 65)]


@pytest.mark.parametrize("tname", list(LABELS))
@pytest.mark.parametrize("mode", ["lsgan", "vanilla"])
@pytest.mark.parametrize("side,n", CASES, ids=lambda v: str(v))
def test_gan_loss_vs_fp64_autograd(ops, side, n, mode, tname):
    p, t = case(side, n, tname)
    if n == 70001:
        assert 2 * n > 512 * 256 and n % 64 != 0
    ref, g64 = reference(side, n, tname, mode)
    loss, grad = run(ops, p, n, side, mode, t)
    ratio = ((grad.double() - g64).abs() / grad_bound(g64, side, n, mode)).max().item()
    lerr = abs(loss - ref)
    report(f"gan_loss {mode} side {side} n {n} {tname}", grad_err_over_bound=ratio,
           loss_err_over_bound=lerr / (LC.R_ACC * ref))
    assert torch.isfinite(grad).all() and math.isfinite(loss)
    if mode == "lsgan":    # an element at its target: exactly no gradient
        target = torch.cat([torch.full((n,), t), torch.zeros(n)]) if side == 0 else torch.ones(n)
        hit = p == target
        assert n < 10 or hit.any()
        assert (grad[hit] == 0).all() and (g64[hit] == 0).all()
    assert ratio <= 1.0
    assert lerr <= LC.R_ACC * ref   # the terms are non-negative: absref == ref


@pytest.mark.parametrize("side,n", [(0, 70001), (1, 140003), (0, 65)], ids=lambda v: str(v))
def test_hinge_through_the_new_entry_is_ops_hinge(ops, side, n):
    p, _ = case(side, n, "t1")
    pd = p.to(DEV)
    junk = torch.randn(p.numel(), generator=torch.Generator().manual_seed(3)).to(DEV) + 2.0
    ga, gb, la, lb = junk.clone(), junk.clone(), loss_word(), loss_word()
    ops.hinge(pd, n, side, SCALE, ga, la)
    ops.gan_loss(pd, n, side, "hinge", 1.0, SCALE, gb, lb)
    a, b = la.item() - LOSS0, lb.item() - LOSS0
    report(f"gan_loss hinge side {side} n {n}", loss_rel_diff=abs(a - b) / abs(a))
    assert torch.equal(ga, gb)
    assert abs(a - b) <= 1e-12 * abs(a)


BAD_CALLS = [("side 2", 2, 1, 1.0), ("side -1", -1, 2, 1.0), ("objective 3", 0, 3, 1.0), ("objective -1", 1, -1, 1.0),
             ("label 0", 0, 1, 0.0), ("label -0.1", 0, 2, -0.1), ("label 1.5", 0, 1, 1.5),
             ("label nan", 0, 2, float("nan")), ("label inf", 1, 1, float("inf")), ("hinge label 0.9", 0, 0, T09)]


@pytest.mark.parametrize("what,side,objective,label", BAD_CALLS, ids=[c[0] for c in BAD_CALLS])
def test_abi_refuses_and_leaves_the_buffers(ops, what, side, objective, label):
    lib = pkg()._lib
    n = 65
    pred = torch.randn(2 * n, generator=torch.Generator().manual_seed(5)).to(DEV)
    g0 = torch.randn(2 * n, generator=torch.Generator().manual_seed(6)).to(DEV) + 2.0
    grad, loss = g0.clone(), loss_word()
    with pytest.raises(lib.IrganError, match="irgan_gan_loss"):
        lib.call("irgan_gan_loss", ops.P(pred), n, side, objective, ctypes.c_float(label), ctypes.c_float(SCALE),
                 ops.P(grad), ops.P(loss), ops.stream())
    torch.cuda.synchronize()
    assert torch.equal(grad, g0) and loss.item() == LOSS0


UP = 1.75     # the upstream gradient: not 1, exact in fp32


@pytest.mark.parametrize("tname", list(LABELS))
@pytest.mark.parametrize("mode", ["lsgan", "vanilla"])
def test_module_functions_value_and_both_gradients(mode, tname):
    irc = pkg()
    t = LABELS[tname]
    gen = torch.Generator().manual_seed(41)
    shape = (3, 1, 7, 5)
    n = 3 * 7 * 5
    r, f = half(n, t, gen).reshape(shape), half(n, t, gen).reshape(shape)
    figs = {}
    # D: both inputs get a gradient
    r64, f64 = r.double().requires_grad_(True), f.double().requires_grad_(True)
    ref = objective(torch.cat([r64.reshape(-1), f64.reshape(-1)]), n, 0, mode, t)
    (ref * UP).backward()
    rd, fd = r.to(DEV).requires_grad_(True), f.to(DEV).requires_grad_(True)
    got = irc.gan_loss_D(rd, fd, mode, t)
    assert got.shape == () and got.dtype == torch.float32
    (got * UP).backward()
    assert rd.grad.shape == shape and fd.grad.shape == shape
    for name, g, g64 in (("real", rd.grad, r64.grad), ("fake", fd.grad, f64.grad)):
        figs[f"D_{name}_grad"] = ((g.cpu().double() - g64).abs() / grad_bound(g64, 0, n, mode, w=UP)).max().item()
    figs["D_value"] = abs(got.item() - ref.item()) / (LC.R_ACC * ref.item())
    # G
    f64 = f.double().requires_grad_(True)
    ref = objective(f64.reshape(-1), n, 1, mode, t)
    (ref * UP).backward()
    fd = f.to(DEV).requires_grad_(True)
    got = irc.gan_loss_G(fd, mode)
    (got * UP).backward()
    figs["G_grad"] = ((fd.grad.cpu().double() - f64.grad).abs() / grad_bound(f64.grad, 1, n, mode, w=UP)).max().item()
    figs["G_value"] = abs(got.item() - ref.item()) / (LC.R_ACC * ref.item())
    report(f"gan_loss_D/G {mode} {tname}", **figs)
    assert all(math.isfinite(v) and v <= 1.0 for v in figs.values()), figs


def test_module_functions_refuse_mismatched_or_foreign_inputs():
    irc = pkg()
    a, b = torch.zeros(3, 1, 7, 5, device=DEV), torch.zeros(3, 1, 7, 4, device=DEV)
    with pytest.raises(ValueError, match="element count"):
        irc.gan_loss_D(a, b, "lsgan")
    with pytest.raises(ValueError, match="fp32"):
        irc.gan_loss_D(a, a.bfloat16(), "lsgan")
    with pytest.raises(ValueError, match="gan_mode"):
        irc.gan_loss_G(a, "wgan")
    with pytest.raises(RuntimeError):
        irc.gan_loss_D(a, a.cpu(), "vanilla")
