"""Config.clip_grad_G / clip_grad_D on the GPU: the deterministic sum-of-squares reduction and
the clip form of the device prep against fp64 formed in the test from the same fp32 inputs, the
clip arm of the Adam kernels against the project's own unclipped entries run on a pre-scaled
gradient (bit for bit: no tolerance), the bad-argument refusals, and the fused step: options
that never bind leave it untouched, options that bind reproduce torch's clip_grad_norm_ +
torch.optim.Adam, with EMA, in bf16 / fp8, and under the forced-collective schedule.

Bounds.  The norm: every square is exact in fp64 and n of them are added, so the relative error
of the sum is at most n * 2^-53 (1.2e-10 at the largest n here), half of that after the root;
the tests allow 1e-9.  The coefficient and the clipped update carry no tolerance.  The step
against torch.optim.Adam (fp64, fed store.grad * coef): the bound of tests/test_gpu_step.py's
own torch-Adam comparison (test_full_state_checkpoint_resume_and_torch_adam, its last
assertion): |p - ref| <= 1e-6 * lr + 1e-7.  The moments of that step, against fp64 formed from the
kernel's own inputs (the fp32 product gc = g * coef, the previous m and v) and its fp32 weights:
m' = m + w1 (gc - m) is two roundings (the difference, the fma), each relative to a quantity
<= |gc| + |m|; v' = b2 v + (w2 gc) gc is four, each relative to a positive term <= v'.  The tests
allow twice that, 4 * 2^-24 (|gc| + |m|) and 8 * 2^-24 v' (as tests/test_gpu_ema.py doubles its
bound)."""
import os

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, B1, B2, EPS, DECAY = 2e-4, 0.5, 0.999, 1e-8, 0.999
EINVAL = 1001
# csrc/loss.hip: the reduction takes one group of four per thread, at most 1024 blocks of 256
# threads: a full round of its grid is SUMSQ_ROUND elements, the rest grid-strides
SUMSQ_ROUND = 1024 * 256 * 4
# ... and adam_launch's rounds (one element / one group of four per thread, at most 8192 blocks)
ADAM_SCALAR_ROUND = 8192 * 256
ADAM_VEC_ROUND = ADAM_SCALAR_ROUND * 4
SIZES = [1, 3, 255, 256, 257, 1027, SUMSQ_ROUND + 1027]   # the last: a full round + an odd remainder
OFFS = [0, 1, 3]   # floats from a 16-byte boundary
PAD = 8
LOSS_KEYS = {"loss_D", "loss_G", "loss_G_GAN", "loss_G_L1", "loss_G_perc", "loss_G_TV", "loss_G_ssim"}


@pytest.fixture(autouse=True)
def _deterministic():
    """The trainers below run with Config.deterministic (process-wide ops state): put it back."""
    ops = pkg().ops
    old = ops.set_deterministic(False)
    try:
        yield
    finally:
        ops.set_deterministic(old)


def _view(n, off, fill):
    """``fill`` (n floats, CPU) as a view ``off`` floats into a zeroed allocation of n + PAD."""
    base = torch.zeros(n + PAD, device=DEV)
    v = base[off:off + n]
    v.copy_(fill.to(DEV))
    assert v.data_ptr() % 16 == 4 * (off % 4)
    return v


def _padding_is_zero(view):
    base, o = view._base, view.storage_offset()
    return not bool(base[:o].any()) and not bool(base[o + view.numel():].any())


def _norm64(g):
    return float(g.detach().cpu().double().pow(2).sum().sqrt())


def _prep(ops, g, max_norm, decay=0.0, count=None, prm=None):
    """Reduction + clip prep on ``g``: (norm fp64 tensor, prm, count, partials)."""
    n = g.numel()
    ws = torch.zeros(ops.grad_sumsq_parts(n), dtype=torch.float64, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV) if count is None else count
    prm = torch.zeros(4, device=DEV) if prm is None else prm
    norm = torch.zeros(1, dtype=torch.float64, device=DEV)
    ops.grad_sumsq(g, ws)
    ops.adam_clip_prep(count, LR, B1, B2, prm, ws, n, max_norm, norm, decay)
    return norm, prm, count, ws


# ---------------------------------------------------------------------------------------------
# 1. the reduction and the coefficient
# ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off", OFFS)
@pytest.mark.parametrize("n", SIZES)
def test_norm_vs_fp64_and_deterministic(n, off):
    ops = pkg().ops
    gen = torch.Generator().manual_seed(n + 31 * off)
    g = _view(n, off, torch.randn(n, generator=gen))
    assert ops.grad_sumsq_parts(n) == max(1, min(-(-n // 1024), 1024))   # a function of n alone
    want = _norm64(g)
    norm, prm, _, ws = _prep(ops, g, 1e30)
    norm2, _, _, ws2 = _prep(ops, g, 1e30)
    host = ops.grad_norm(g)
    torch.cuda.synchronize()
    got = float(norm.item())
    rel = abs(got - want) / want
    print(f"n={n} off={off}: norm={got!r} want={want!r} rel={rel:.3e} parts={ws.numel()}")
    assert rel <= 1e-9
    # two launches on the same data: the same fp64 bits, partial by partial
    assert torch.equal(ws.view(torch.int64), ws2.view(torch.int64))
    assert norm.view(torch.int64).item() == norm2.view(torch.int64).item()
    # the host-side sum of the partials (ops.grad_norm) is the device's
    assert np.float64(host).tobytes() == np.float64(got).tobytes()
    assert float(prm[3].item()) == 1.0
    assert _padding_is_zero(g)


def test_norm_does_not_overflow():
    ops = pkg().ops
    n = 1027
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(n, generator=gen)
    x[::7] = 1e25 * torch.sign(x[::7])
    g = _view(n, 1, x)
    assert torch.isinf(g.pow(2).sum())           # an fp32 accumulator overflows on this buffer
    norm, prm, _, _ = _prep(ops, g, 1.0)
    got, want = float(norm.item()), _norm64(g)
    assert np.isfinite(got) and want > 1e26
    assert abs(got - want) / want <= 1e-9
    assert float(prm[3].item()) == float(np.float32(1.0 / (got + 1e-6)))


def test_coefficient():
    ops = pkg().ops
    n = 1027
    # all-zero gradient: norm 0, coefficient exactly 1
    norm, prm, cnt, _ = _prep(ops, _view(n, 3, torch.zeros(n)), 0.5)
    assert float(norm.item()) == 0.0 and float(prm[3].item()) == 1.0 and int(cnt.item()) == 1
    g = _view(n, 3, torch.randn(n, generator=torch.Generator().manual_seed(9)))
    # below max_norm: exactly 1
    norm, prm, _, _ = _prep(ops, g, 1e3)
    nv = float(norm.item())
    assert 1.0 < nv < 1e3 and float(prm[3].item()) == 1.0
    # above: float32(max_norm / (norm + 1e-6)), the quotient in fp64
    for max_norm in (0.37 * nv, 1.0, 1e-3):
        norm, prm, _, _ = _prep(ops, g, max_norm)
        assert float(norm.item()) == nv
        want = np.float32(np.float64(max_norm) / (np.float64(nv) + np.float64(1e-6)))
        got = prm.cpu().numpy()[3]
        print(f"max_norm={max_norm!r}: prm[3]={got!r} want={want!r}")
        assert got == want and got < 1.0
        assert np.float32(ops.clip_coef(nv, max_norm)) == want
    # the count and prm[0..2] are the EMA prep's, step after step
    cnt, prm = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(4, device=DEV)
    cnt_e, prm_e = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(3, device=DEV)
    for t in (1, 2, 3):
        _prep(ops, g, 1.0, decay=DECAY, count=cnt, prm=prm)
        ops.adam_prep(cnt_e, LR, B1, B2, prm_e, decay=DECAY)
        assert int(cnt.item()) == t == int(cnt_e.item())
        assert torch.equal(prm[:3], prm_e)


# ---------------------------------------------------------------------------------------------
# 2. the clip arm of the Adam kernels
# ---------------------------------------------------------------------------------------------

ADAM_CASES = [(n, (o,) * 5) for n in SIZES for o in OFFS] + [
    (1027, (0, 1, 2, 3, 1)),                        # no common offset: the one-element-per-lane kernel
    (ADAM_SCALAR_ROUND + 1027, (0, 1, 2, 3, 1)),    # ... and a ragged second round of it
    (ADAM_VEC_ROUND + 1027, (1,) * 5),              # a full round of the 16-byte kernel + a ragged one
]


@pytest.mark.parametrize("ema_on", [False, True], ids=["plain", "ema"])
@pytest.mark.parametrize("n,offs", ADAM_CASES, ids=[f"n{n}_off{''.join(map(str, o))}" for n, o in ADAM_CASES])
def test_adam_clip_equals_plain_entries_on_scaled_gradient(n, offs, ema_on):
    """p, m, v (and ema) of the clip entries, coefficient from prm[3] and from the host, equal
    the EXISTING entries run on g * coef formed in fp32 by torch -- bit for bit."""
    ops = pkg().ops
    gen = torch.Generator().manual_seed(n + 7 * sum(offs) + ema_on)
    p, m, v, e, g = (_view(n, o, torch.randn(n, generator=gen)) for o in offs)
    m.zero_()
    v.zero_()
    decay = DECAY if ema_on else 0.0
    ema = (lambda x: x) if ema_on else (lambda x: None)   # noqa: E731
    ph, mh, vh, eh = (_view(n, o, x.cpu()) for o, x in zip(offs, (p, m, v, e)))    # host coefficient
    pr, mr, vr, er = p.clone(), m.clone(), v.clone(), e.clone()                    # the plain entries
    e0 = e.clone()
    cnt, prm = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(4, device=DEV)
    cnt_r, prm_r = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(3, device=DEV)
    ws = torch.zeros(ops.grad_sumsq_parts(n), dtype=torch.float64, device=DEV)
    norm = torch.zeros(1, dtype=torch.float64, device=DEV)
    for t in (1, 2, 3):
        g.copy_(torch.randn(n, generator=gen).to(DEV) * (1.0 + t))
        g0 = g.clone()
        max_norm = 0.37 * _norm64(g)                 # a coefficient with a full mantissa
        ops.grad_sumsq(g, ws)
        ops.adam_clip_prep(cnt, LR, B1, B2, prm, ws, n, max_norm, norm, decay)
        ops.adam_dev(p, g, m, v, prm, B1, B2, EPS, ema=ema(e), clip=True)
        coef = prm[3:4].clone()
        assert 0.3 < float(coef.item()) < 0.4
        gs = g * coef                                # torch: one fp32 product per element
        if ema_on:
            ops.adam_prep(cnt_r, LR, B1, B2, prm_r, decay=DECAY)
        else:
            ops.adam_prep(cnt_r, LR, B1, B2, prm_r)
        ops.adam_dev(pr, gs, mr, vr, prm_r, B1, B2, EPS, ema=ema(er))
        ops.adam(ph, g, mh, vh, t, LR, B1, B2, EPS, ema=ema(eh), decay=decay, coef=float(coef.item()))
        torch.cuda.synchronize()
        for name, dev, host, ref in (("p", p, ph, pr), ("m", m, mh, mr), ("v", v, vh, vr), ("ema", e, eh, er)):
            assert torch.equal(dev, ref), (name, t, "prm form vs the plain entries on g * coef")
            assert torch.equal(host, ref), (name, t, "host-coefficient form vs the plain entries on g * coef")
        assert torch.equal(g, g0), "the gradient buffer is only read"
        assert not torch.equal(gs, g0)
    if ema_on:
        assert not torch.equal(e, e0)
    else:
        assert torch.equal(e, e0) and torch.equal(eh, e0)
    assert bool((m != 0).all())                      # every element was visited, head and tail included
    for name, x in (("p", p), ("m", m), ("v", v), ("e", e), ("g", g), ("ph", ph)):
        assert _padding_is_zero(x), name


def test_bad_arguments_are_refused_and_launch_nothing():
    irc = pkg()
    ops, lib = irc.ops, irc._lib.load()
    n = 5000
    parts = ops.grad_sumsq_parts(n)
    assert parts == 5 and ops.grad_sumsq_parts(0) == 0
    g = torch.ones(n, device=DEV)
    st = ops.stream()
    ws = torch.full((parts + 1,), -7.0, dtype=torch.float64, device=DEV)
    # the reduction: null workspace, null gradient, empty, a partial count that does not match n
    assert lib.irgan_grad_sumsq(ops.P(g), n, None, parts, st) == EINVAL
    assert lib.irgan_grad_sumsq(None, n, ops.P(ws), parts, st) == EINVAL
    assert lib.irgan_grad_sumsq(ops.P(g), 0, ops.P(ws), parts, st) == EINVAL
    for bad in (parts - 1, parts + 1, 0):
        assert lib.irgan_grad_sumsq(ops.P(g), n, ops.P(ws), bad, st) == EINVAL
    with pytest.raises(irc._lib.IrganError, match=str(EINVAL)):
        ops.grad_sumsq(g, ws)                        # parts + 1 doubles
    torch.cuda.synchronize()
    assert bool((ws == -7.0).all())
    # the prep
    ops.grad_sumsq(g, ws[:parts])
    cnt = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    prm = torch.full((4,), -3.0, device=DEV)
    norm = torch.full((1,), -5.0, dtype=torch.float64, device=DEV)
    import ctypes
    d = ctypes.c_double

    def prep(count=cnt, decay=0.0, partials=ws, nparts=parts, nn=n, max_norm=1.0, out=prm):
        return lib.irgan_adam_clip_prep(ops.P(count), d(LR), d(B1), d(B2), d(decay), ops.P(partials), nparts, nn,
                                        d(max_norm), ops.P(norm), ops.P(out), st)
    for kw in (dict(max_norm=0.0), dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(partials=None),
               dict(count=None), dict(out=None), dict(nparts=parts + 1), dict(nparts=parts - 1), dict(nn=0),
               dict(nn=n + 1024), dict(decay=1.0), dict(decay=-0.1)):
        assert prep(**kw) == EINVAL, kw
    with pytest.raises(ValueError):
        ops.adam_clip_prep(cnt, LR, B1, B2, torch.zeros(3, device=DEV), ws[:parts], n, 1.0)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 4 and bool((prm == -3.0).all()) and float(norm.item()) == -5.0
    # ... and the same call with good arguments goes through
    assert prep() == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == 5 and abs(float(norm.item()) - n ** 0.5) <= 1e-9 * n ** 0.5
    # the Adam entries: no prm
    x = [torch.zeros(8, device=DEV) for _ in range(4)]
    f = ctypes.c_float
    assert lib.irgan_adam_clip_dev(*(ops.P(t) for t in x), None, 8, None, f(B1), f(B2), f(EPS), st) == EINVAL
    with pytest.raises(ValueError):
        ops.adam_dev(*x, torch.zeros(3, device=DEV), B1, B2, EPS, clip=True)
    with pytest.raises(ValueError):
        ops.adam(*x, 1, LR, B1, B2, EPS, ema=torch.zeros(7, device=DEV), decay=DECAY, coef=0.5)
    torch.cuda.synchronize()
    assert not any(bool(t.any()) for t in x)


LAYOUT = {"a.weight": (5, 3, 3, 3), "a.bias": (5,), "b.weight": (7, 5, 1, 1)}


@pytest.mark.parametrize("decay", [DECAY, 0.0], ids=["ema", "plain"])
def test_paramstore_clip_device_and_host_count(decay):
    """ParamStore.adam_begin(max_norm=): the step count on the device and on the host give one
    result, the norm lands in norm_out, grad stays unscaled, and apply takes the whole buffer only."""
    ParamStore = pkg().engine.ParamStore
    gen = torch.Generator().manual_seed(5)
    dev, host = ParamStore(LAYOUT, DEV), ParamStore(LAYOUT, DEV)
    dev.dev_adam = True
    n = dev.numel
    init = torch.randn(n, generator=gen).to(DEV)
    for s in (dev, host):
        s.flat.copy_(init)
        s.enable_ema()
    out = torch.zeros(2, dtype=torch.float64, device=DEV)
    for t in (1, 2, 3):
        gr = torch.randn(n, generator=gen).to(DEV)
        dev.grad.copy_(gr)
        host.grad.copy_(gr)
        apply = dev.adam_begin(LR, B1, B2, EPS, ema_decay=decay, max_norm=2.0, norm_out=out[0:1])
        assert apply.whole
        with pytest.raises(ValueError):
            apply(0, 64)
        apply(0, n)
        host.adam_begin(LR, B1, B2, EPS, ema_decay=decay, max_norm=2.0, norm_out=out[1:2])(0, n)
        torch.cuda.synchronize()
        for name in ("flat", "m", "v", "ema", "grad"):
            assert torch.equal(getattr(dev, name), getattr(host, name)), (name, t)
        assert torch.equal(dev.grad, gr)
        assert float(out[0].item()) == float(out[1].item())
        assert abs(float(out[0].item()) - _norm64(gr)) <= 1e-9 * _norm64(gr) and float(out[0].item()) > 2.0
    assert int(dev._count.item()) == 3 and dev.step_count == host.step_count == 3
    # against the unclipped path on the scaled gradient (host count, whole buffer)
    ref = ParamStore(LAYOUT, DEV)
    ref.flat.copy_(init)
    gen = torch.Generator().manual_seed(5)
    torch.randn(n, generator=gen)
    for t in (1, 2, 3):
        gr = torch.randn(n, generator=gen).to(DEV)
        coef = torch.tensor(pkg().ops.clip_coef(pkg().ops.grad_norm(gr), 2.0), dtype=torch.float32, device=DEV)
        ref.grad.copy_(gr * coef)
        ref.adam_step(LR, B1, B2, EPS)
    assert torch.equal(ref.flat, dev.flat) and torch.equal(ref.m, dev.m) and torch.equal(ref.v, dev.v)
    # adam_step(max_norm=) is the host-count form
    a, b = ParamStore(LAYOUT, DEV), ParamStore(LAYOUT, DEV)
    for s in (a, b):
        s.flat.copy_(init)
        s.grad.copy_(gr)
    a.adam_step(LR, B1, B2, EPS, max_norm=2.0)
    b.grad.mul_(coef)
    b.adam_step(LR, B1, B2, EPS)
    assert torch.equal(a.flat, b.flat) and torch.equal(a.grad, gr)


# ---------------------------------------------------------------------------------------------
# 3. the fused step (fp32, 32 x 32, B = 2, seeded like the s32 tests)
# ---------------------------------------------------------------------------------------------

def _trainer(clip_G=0.0, clip_D=0.0, dtype="fp32", decay=0.0, norm="instance", **kw):
    from oracle import step as O
    irc = pkg()
    cfg = irc.Config()
    cfg.device = DEV
    cfg.compute_dtype = dtype
    cfg.deterministic = True
    cfg.norm = norm
    cfg.clip_grad_G, cfg.clip_grad_D, cfg.ema_decay = clip_G, clip_D, decay
    torch.manual_seed(1234)   # init_net draws G and D from the global generator
    tr = irc.GANTrainer(cfg, **kw)
    if norm != "instance":    # another parameter layout: the seeded initialisation stands
        return tr
    tr.netG.store.load(O.seeded_params(O.g_param_shapes(), 1, bias_std=0.02), strict=True)
    tr.netD.store.load(O.seeded_params(O.d_param_shapes(), 2, bias_std=0.02), strict=True)
    tr.vgg.store.load(O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True), strict=True)
    for net in (tr.netG, tr.netD, tr.vgg):
        net.repack()
    if decay:
        tr.netG.store.ema.copy_(tr.netG.store.flat)   # the average starts from the loaded weights
    return tr


def _batches(k, hw=32, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(2, 1, hw, hw, generator=g) * 2 - 1).to(DEV),
             (torch.rand(2, 3, hw, hw, generator=g) * 2 - 1).to(DEV)) for _ in range(k)]


def _snap(tr):
    return {f"{n}.{f}": getattr(getattr(tr, n).store, f).clone() for n in ("netG", "netD") for f in ("flat", "m", "v")}


_MEASURED = {}


def _measured():
    """Computed once: two steps of a plain trainer and of one whose clips (1e30) never bind --
    their states, loss vectors, and the second one's gradient buffers."""
    if not _MEASURED:
        for name, c in (("off", 0.0), ("never", 1e30)):
            tr = _trainer(c, c)
            Ls = [tr.step(ir, rgb).clone() for ir, rgb in _batches(1)]
            first = {"gG": tr.netG.store.grad.clone(), "gD": tr.netD.store.grad.clone()}
            Ls += [tr.step(ir, rgb).clone() for ir, rgb in _batches(2)[1:]]
            torch.cuda.synchronize()
            _MEASURED[name] = {"state": _snap(tr), "L": Ls, "first": first, "gG": tr.netG.store.grad.clone(),
                               "gD": tr.netD.store.grad.clone(), "dict": tr.losses(Ls[-1])}
    return _MEASURED


def test_clips_that_never_bind_leave_the_step_untouched():
    r = _measured()
    off, on = r["off"], r["never"]
    for k, v in off["state"].items():
        assert torch.equal(v, on["state"][k]), k
    for t in range(2):
        assert torch.equal(off["L"][t][:6], on["L"][t][:6]), t
        assert bool((off["L"][t][6:] == 0).all())
    assert set(off["dict"]) == LOSS_KEYS
    assert set(on["dict"]) == LOSS_KEYS | {"grad_norm_D", "grad_norm_G"}
    for slot, key in ((6, "gD"), (7, "gG")):
        got, want = float(on["L"][1][slot].item()), _norm64(on[key])
        print(f"losses[{slot}]={got!r} fp64 norm of the gradient buffer={want!r}")
        assert want > 0 and abs(got - want) <= 1e-9 * want
    assert on["dict"]["grad_norm_D"] == float(on["L"][1][6].item())
    assert on["dict"]["grad_norm_G"] == float(on["L"][1][7].item())
    # one network alone: only its slot and its key
    tr = _trainer(0.0, 1e30)
    L = tr.step(*_batches(1)[0])
    assert float(L[7].item()) == 0.0 and float(L[6].item()) > 0.0
    assert set(tr.losses(L)) == LOSS_KEYS | {"grad_norm_D"}


def _torch_adam(p0, m0, v0, grad, t, lr):
    """torch.optim.Adam in fp64 on one flat parameter with moments (m0, v0) after t - 1 steps."""
    p = torch.nn.Parameter(p0.double().cpu().clone())
    p.grad = grad.double().cpu().clone()
    opt = torch.optim.Adam([p], lr=lr, betas=(B1, B2), eps=EPS)
    if t > 1:
        opt.state[p] = {"step": torch.tensor(float(t - 1)), "exp_avg": m0.double().cpu().clone(),
                        "exp_avg_sq": v0.double().cpu().clone()}
    opt.step()
    return p.detach()


def _check_clipped_update(tr, before, L, clip, t, must_bind):
    lr = tr.current_lr_G
    assert tr.cfg.lr_D == tr.cfg.lr_G
    for name, slot in (("netD", 6), ("netG", 7)):
        S = getattr(tr, name).store
        norm = float(L[slot].item())
        want = _norm64(S.grad)
        # the gradient buffer is unscaled: its norm is the reported one, not max_norm
        assert abs(norm - want) <= 1e-9 * want, (name, norm, want)
        coef = np.float32(pkg().ops.clip_coef(norm, clip[name]))
        print(f"step {t} {name}: norm={norm!r} max_norm={clip[name]!r} coef={coef!r}")
        if must_bind:
            assert coef < 1.0 and norm > 1.5 * clip[name], (name, norm, clip[name])
        gc = S.grad * torch.tensor(coef, device=DEV)            # fp32, as the kernel forms it
        p = _torch_adam(before[name + ".flat"], before[name + ".m"], before[name + ".v"], gc, t, lr)
        dp = (S.flat.double().cpu() - p).abs().max().item()
        assert dp <= 1e-6 * lr + 1e-7, (name, t, dp)            # tests/test_gpu_step.py, the torch-Adam check
        # the moments: fp64 from the kernel's own inputs and its fp32 weights (1 - float32(b))
        m0, v0, g64 = before[name + ".m"].double().cpu(), before[name + ".v"].double().cpu(), gc.double().cpu()
        b2f = np.float32(B2)
        w1, w2 = float(np.float32(1) - np.float32(B1)), float(np.float32(1) - b2f)
        m_ref = m0 + w1 * (g64 - m0)
        v_ref = float(b2f) * v0 + (w2 * g64) * g64
        tiny = 4 * 2.0 ** -126   # below the smallest normal fp32 a result may be flushed
        em = ((S.m.double().cpu() - m_ref).abs() / (4 * 2.0 ** -24 * (g64.abs() + m0.abs()) + tiny)).max().item()
        ev = ((S.v.double().cpu() - v_ref).abs() / (8 * 2.0 ** -24 * v_ref + tiny)).max().item()
        print(f"step {t} {name}: max |p - torch| = {dp:.3e}, m err/bound = {em:.3f}, v err/bound = {ev:.3f}")
        assert em <= 1.0 and ev <= 1.0, (name, t, em, ev)


def _half_norms():
    first = _measured()["never"]["first"]
    return {"netG": 0.5 * _norm64(first["gG"]), "netD": 0.5 * _norm64(first["gD"])}


def test_active_clip_matches_torch_clip_then_adam():
    clip = _half_norms()
    tr = _trainer(clip["netG"], clip["netD"])
    for t, (ir, rgb) in enumerate(_batches(2), start=1):
        before = _snap(tr)
        L = tr.step(ir, rgb).clone()
        torch.cuda.synchronize()
        # step 1 binds by construction (half the norm just measured; G's moves a little with the
        # clipped D); Adam's first step hardly depends on the gradient's scale, the second does
        _check_clipped_update(tr, before, L, clip, t, must_bind=t == 1)
    _MEASURED["clipped"] = {"state": _snap(tr), "L": L}
    # not the unclipped step
    off = _measured()["off"]["state"]
    assert not torch.equal(off["netG.m"], tr.netG.store.m) and not torch.equal(off["netD.flat"], tr.netD.store.flat)


def test_ema_follows_the_clipped_parameters():
    from test_gpu_ema import _bound, _ema_ref, _w32
    clip = _half_norms()
    tr = _trainer(clip["netG"], clip["netD"], decay=DECAY)
    G = tr.netG.store
    for t, (ir, rgb) in enumerate(_batches(2), start=1):
        e_prev, before = G.ema.clone(), _snap(tr)
        L = tr.step(ir, rgb).clone()
        torch.cuda.synchronize()
        _check_clipped_update(tr, before, L, clip, t, must_bind=t == 1)
        err = (G.ema.double() - _ema_ref(e_prev, G.flat, _w32(t))).abs()
        bound = _bound(e_prev, G.flat)
        print(f"t={t}: max err/bound = {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), (t, (err / bound).max().item())
    assert not torch.equal(G.ema, G.flat)
    if "clipped" in _MEASURED:   # the same two steps without the average: p, m, v bit for bit
        for k, v in _MEASURED["clipped"]["state"].items():
            assert torch.equal(v, _snap(tr)[k]), k


@pytest.mark.parametrize("dtype,hw,norm", [("bf16", 32, "instance"), ("fp8", 64, "instance"), ("bf16", 32, "batch")])
def test_reduced_precision_and_batch_norm_steps_clip_and_report(dtype, hw, norm):
    c = 1e-2
    tr = _trainer(c, c, dtype=dtype, norm=norm)
    before = _snap(tr)
    d = tr.losses(tr.step(*_batches(1, hw=hw)[0]))
    torch.cuda.synchronize()
    print(dtype, norm, d)
    assert all(np.isfinite(x) for x in d.values()), d
    assert d["grad_norm_D"] > c and d["grad_norm_G"] > c          # both clips bind
    for k, v in _snap(tr).items():
        assert bool(torch.isfinite(v).all()), k
        assert not torch.equal(v, before[k]), k
    for name, key in (("netD", "grad_norm_D"), ("netG", "grad_norm_G")):
        S = getattr(tr, name).store
        assert abs(d[key] - _norm64(S.grad)) <= 1e-9 * d[key]
        # m after the first step is (1 - b1) * g * coef: its norm is (1 - b1) * max_norm
        mn = _norm64(S.m)
        assert abs(mn - (1 - B1) * c) <= 1e-4 * c, (name, mn)


def _forced_worker(rank, store, out, clip):
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1,
                           device_id=torch.device("cuda", 0))
    tr = _trainer(clip["netG"], clip["netD"], force_reduce=True)
    core = tr.core
    assert core.g_reduce.active and core.d_reduce.active
    spans = []
    finish = core.g_reduce.finish

    def spy(apply=None):
        def rec(a, b):
            spans.append((a, b, len(core.g_reduce.works)))
            apply(a, b)
        rec.whole = getattr(apply, "whole", False)
        finish(rec)
    core.g_reduce.finish = spy
    Ls = [tr.step(ir, rgb).clone() for ir, rgb in _batches(2)]
    torch.cuda.synchronize()
    assert pkg().engine.replicas_identical([core.G.flat, core.D.flat], force=True)
    torch.save({"state": {k: v.cpu() for k, v in _snap(tr).items()}, "L": [x.cpu() for x in Ls], "spans": spans,
                "numel": core.G.numel}, os.path.join(out, "forced.pt"))
    dist.destroy_process_group()


def test_forced_collectives_with_clipping_bit_identical(tmp_path):
    """tests/test_gpu_dp.py's forced-collective pattern with both clips binding: the bucketed
    reduce, then ONE reduction -> prep -> Adam over the whole buffer; parameters, moments and
    norms equal the plain schedule's bit for bit."""
    import torch.multiprocessing as mp
    clip = _half_norms()
    mp.spawn(_forced_worker, args=(str(tmp_path / "store"), str(tmp_path), clip), nprocs=1, join=True)
    r = torch.load(tmp_path / "forced.pt", weights_only=True)
    assert r["spans"] == [(0, r["numel"], r["spans"][0][2])] * 2 and r["spans"][0][2] > 1, r["spans"]
    tr = _trainer(clip["netG"], clip["netD"])
    Ls = [tr.step(ir, rgb).clone() for ir, rgb in _batches(2)]
    torch.cuda.synchronize()
    for k, v in _snap(tr).items():
        assert torch.equal(r["state"][k], v.cpu()), k
    for t in range(2):
        assert torch.equal(r["L"][t][6:], Ls[t][6:].cpu()), t      # the norms: the same bits
        assert float(Ls[t][6].item()) > clip["netD"] and float(Ls[t][7].item()) > 0
        assert torch.allclose(r["L"][t][:6], Ls[t][:6].cpu(), rtol=1e-12, atol=0)
