"""Config.ema_decay on the GPU: the Adam kernels with EMA against those without (bit for bit)
and an fp64 recurrence, the plain entries off 16-byte alignment, ParamStore.adam_begin's one
path, the unchanged step, the bucketed (data-parallel) path, resume, GANTrainer.ema_weights()
and train_kaist's EMA files.

The EMA bound used throughout: e' = e + w (p - e) in fp32 is at most four roundings in either
lerp form, each relative to a quantity <= |e| + |p|, i.e. 4 * 2^-24 = 2^-22 of it; the tests
allow twice that, |e' - ref| <= 2^-21 (|e| + |p|) + 1e-30, with ref formed in fp64 from the
kernel's own new p, its own previous e and the fp32 weight it used."""
import os

import numpy as np
import pytest
import torch

from conftest import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LR, B1, B2, EPS, DECAY = 2e-4, 0.5, 0.999, 1e-8, 0.999
SEED = 1234
# the launch geometry (csrc/loss.hip: adam_launch under nblocks' cap): at most 8192 blocks x 256
# threads per round, x 4 elements in the vector kernel; the rest grid-strides
SCALAR_ROUND = 8192 * 256
FULL_ROUND = SCALAR_ROUND * 4
PAD = 8   # floats each _views allocation holds beyond its view


@pytest.fixture(autouse=True)
def _deterministic():
    """The trainers below run with Config.deterministic (process-wide ops state): put it back."""
    ops = pkg().ops
    old = ops.set_deterministic(False)
    try:
        yield
    finally:
        ops.set_deterministic(old)


def _bound(e_prev, p_new):
    return 2.0 ** -21 * (e_prev.double().abs() + p_new.double().abs()) + 1e-30


def _ema_ref(e_prev, p_new, w):
    return e_prev.double() + float(w) * (p_new.double() - e_prev.double())


def _w32(t, decay=DECAY):
    return np.float32(pkg().ops.ema_weight(decay, t))


# ---------------------------------------------------------------------------------------------
# 1. the kernels
# ---------------------------------------------------------------------------------------------

def _views(n, offs, gen):
    """One randn vector of n elements per offset, each a view starting offs[i] elements into
    its own zeroed allocation of n + PAD (the allocator's blocks are 512-byte aligned, so
    offs[i] % 4 is the pointer's offset from a 16-byte boundary in floats)."""
    out = []
    for o in offs:
        base = torch.zeros(n + PAD, device=DEV)
        v = base[o:o + n]
        v.copy_(torch.randn(n, generator=gen).to(DEV))
        assert v.data_ptr() % 16 == 4 * (o % 4)
        out.append(v)
    return out


def _padding_is_zero(view):
    """The PAD floats of a _views allocation outside the view: nothing was written there."""
    base, o = view._base, view.storage_offset()
    assert base.numel() == view.numel() + PAD
    return not bool(base[:o].any()) and not bool(base[o + view.numel():].any())


TINY = [(1, 1), (5, 3), (6, 2), (10, 1)]   # fallback (nvec == 0); head 1; head 2; head 3 and tail 3
TINY_IDS = ["n1_off1", "n5_off3", "n6_off2", "n10_off1"]


@pytest.mark.parametrize("n,offs", [
    (1, (0,) * 5), (63, (0,) * 5), (1001, (0,) * 5),
    (FULL_ROUND + 1001, (0,) * 5),                       # a full round of the grid + a ragged second one
    (1001, (1,) * 5), (1001, (2,) * 5), (1001, (3,) * 5),  # shared misalignment: scalar head, vector body
    (1001, (0, 1, 2, 3, 1)),                             # no common offset: the one-element-per-lane kernel
] + [(n, (o,) * 5) for n, o in TINY],
    ids=["n1", "n63", "n1001", "full_round_plus_1001", "off1", "off2", "off3", "mixed_offsets"] + TINY_IDS)
def test_adam_ema_kernels_vs_adam_and_fp64(n, offs):
    ops = pkg().ops
    gen = torch.Generator().manual_seed(n + 7 * sum(offs))
    p, m, v, e, g = _views(n, offs, gen)
    m.zero_()
    v.zero_()
    e0 = e.clone()
    # the same update on the plain kernels (host arguments / device count) and on the
    # host-argument EMA entry, each on tensors of its own
    pa, ma, va = p.clone(), m.clone(), v.clone()
    pb, mb, vb = p.clone(), m.clone(), v.clone()
    ph, mh, vh, eh = p.clone(), m.clone(), v.clone(), e.clone()
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    cnt_b = torch.zeros(1, dtype=torch.int32, device=DEV)
    prm = torch.zeros(3, device=DEV)
    prm_b = torch.zeros(2, device=DEV)
    for t in (1, 2, 3):
        g.copy_(torch.randn(n, generator=gen).to(DEV))
        e_prev = e.clone()
        ops.adam_prep(cnt, LR, B1, B2, prm, decay=DECAY)
        ops.adam_dev(p, g, m, v, prm, B1, B2, EPS, ema=e)
        ops.adam(pa, g, ma, va, t, LR, B1, B2, EPS)
        ops.adam_prep(cnt_b, LR, B1, B2, prm_b)
        ops.adam_dev(pb, g, mb, vb, prm_b, B1, B2, EPS)
        ops.adam(ph, g, mh, vh, t, LR, B1, B2, EPS, ema=eh, decay=DECAY)
        torch.cuda.synchronize()
        for name, got, a, b, h in (("p", p, pa, pb, ph), ("m", m, ma, mb, mh), ("v", v, va, vb, vh)):
            assert torch.equal(got, a), (name, t, "vs ops.adam")
            assert torch.equal(got, b), (name, t, "vs ops.adam_prep + ops.adam_dev")
            assert torch.equal(got, h), (name, t, "vs ops.adam with ema")
        # the device-side count and weight
        assert int(cnt.item()) == t and int(cnt_b.item()) == t
        want = _w32(t)
        w = prm.cpu().numpy()[2]
        print(f"n={n} t={t}: prm[2]={w!r} want={want!r}")
        assert abs(np.float64(w) - np.float64(want)) <= np.spacing(want), (t, w, want)
        assert torch.equal(prm[:2], prm_b), "the EMA prep's step_size / bc2_sqrt"
        # fp64 reference from the kernel's own p_new and previous e, with the weight it used
        err = (e.double() - _ema_ref(e_prev, p, w)).abs()
        bound = _bound(e_prev, p)
        print(f"n={n} t={t}: max err/bound = {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), (t, (err / bound).max().item())
        # negative control: next step's weight in the reference must not pass
        err_wrong = (e.double() - _ema_ref(e_prev, p, _w32(t + 1))).abs()
        assert not (err_wrong <= bound).all(), (t, "the check cannot tell w_t from w_t+1")
        # host arguments = device count, bit for bit
        assert torch.equal(e, eh), (t, "ops.adam with ema vs ops.adam_dev with ema")
        if t == 1:
            # every element was visited, tail included.  An element whose exact update is below
            # the rounding bound may legitimately keep its value (p and e are independent
            # normals: about one in 10^7 lies that close), so those are the only ones excused;
            # at n <= 1001 the seeds used here have none.
            movable = (_ema_ref(e0, p, w) - e0.double()).abs() > bound
            assert (e != e0)[movable].all()
            assert int((~movable).sum()) <= max(0, n // 100000), int((~movable).sum())
            if n <= 1001:
                assert (e != e0).all()
    # nothing was written outside [0, n)
    for name, x in (("p", p), ("m", m), ("v", v), ("e", e)):
        assert _padding_is_zero(x), name


def test_adam_ema_binding_refuses_mismatched_sizes():
    ops = pkg().ops
    x = [torch.zeros(8, device=DEV) for _ in range(4)]
    with pytest.raises(ValueError):
        ops.adam(*x, 1, LR, B1, B2, EPS, ema=torch.zeros(7, device=DEV), decay=DECAY)
    with pytest.raises(ValueError):
        ops.adam_prep(torch.zeros(1, dtype=torch.int32, device=DEV), LR, B1, B2, torch.zeros(2, device=DEV),
                      decay=DECAY)


# |p - torch.optim.Adam on the CPU| after three steps: the project's Adam bound
# (tests/test_gpu_losses.py: the same hyper-parameters, randn parameters and gradients)
ADAM_BOUND = 5e-7


@pytest.mark.parametrize("n,offs", [(n, (o,) * 4) for n, o in TINY] + [
    (1001, (1,) * 4), (1001, (2,) * 4), (1001, (3,) * 4),
    (1001, (0, 1, 2, 3)),                   # no common offset: the one-element-per-lane kernel
    (SCALAR_ROUND + 1001, (0, 1, 2, 3)),    # ... and a second, ragged round of it
], ids=TINY_IDS + ["off1", "off2", "off3", "mixed_offsets", "mixed_offsets_second_round"])
def test_plain_adam_offsets(n, offs):
    """The plain entries off alignment (head / 16-byte body / tail, and the fallback): bit-equal
    to the same update on aligned clones and to the EMA entry's p / m / v on the same views."""
    ops = pkg().ops
    gen = torch.Generator().manual_seed(n + 7 * sum(offs))
    p, m, v, g = _views(n, offs, gen)
    m.zero_()
    v.zero_()
    pa, ma, va = p.clone(), m.clone(), v.clone()      # aligned, ops.adam
    pb, mb, vb = p.clone(), m.clone(), v.clone()      # aligned, device count
    # the EMA entry on offset views of its own (e at p's offset)
    pe, me, ve, ee = _views(n, offs[:3] + offs[:1], gen)
    pe.copy_(p)
    me.zero_()
    ve.zero_()
    pt = p.cpu().clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=LR, betas=(B1, B2), eps=EPS)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    prm = torch.zeros(2, device=DEV)
    for t in (1, 2, 3):
        gr = torch.randn(n, generator=gen)
        g.copy_(gr.to(DEV))
        pt.grad = gr
        opt.step()
        ops.adam(p, g, m, v, t, LR, B1, B2, EPS)
        ops.adam(pa, g, ma, va, t, LR, B1, B2, EPS)
        ops.adam_prep(cnt, LR, B1, B2, prm)
        ops.adam_dev(pb, g, mb, vb, prm, B1, B2, EPS)
        ops.adam(pe, g, me, ve, t, LR, B1, B2, EPS, ema=ee, decay=DECAY)
        torch.cuda.synchronize()
        for name, got, a, b, e in (("p", p, pa, pb, pe), ("m", m, ma, mb, me), ("v", v, va, vb, ve)):
            assert torch.equal(got, a), (name, t, "vs ops.adam on aligned clones")
            assert torch.equal(got, b), (name, t, "vs ops.adam_prep + ops.adam_dev on aligned clones")
            assert torch.equal(got, e), (name, t, "vs the EMA entry on the same offsets")
        if t == 1:
            assert bool((m != 0).all())   # every element was visited, head and tail included
    err = float((p.cpu() - pt.detach()).abs().max())
    print(f"n={n} offs={offs}: max |p - torch.optim.Adam| / bound = {err / ADAM_BOUND:.3f}")
    assert err < ADAM_BOUND
    for name, x in (("p", p), ("m", m), ("v", v), ("g", g)):
        assert _padding_is_zero(x), name


LAYOUT = {"a.weight": (5, 3, 3, 3), "a.bias": (5,), "b.weight": (7, 5, 1, 1)}


@pytest.mark.parametrize("decay", [DECAY, 0.0], ids=["ema", "plain"])
def test_paramstore_one_path(decay):
    """ParamStore.adam_begin with the step count on the device and on the host, applied whole
    and in two spans, with and without EMA, across a state load: one result."""
    ParamStore = pkg().engine.ParamStore
    gen = torch.Generator().manual_seed(5)
    dev, host = ParamStore(LAYOUT, DEV), ParamStore(LAYOUT, DEV)
    dev.dev_adam = True
    n = dev.numel
    cut = 192   # a.weight's 135 elements fill slices of 64 up to here
    assert n == host.numel and 0 < cut < n and cut % 64 == 0 and cut == dev.offsets["a.bias"]
    init = torch.randn(n, generator=gen).to(DEV)
    for s in (dev, host):
        s.flat.copy_(init)
        s.enable_ema()
    ema0 = init.clone()

    def step():
        gr = torch.randn(n, generator=gen).to(DEV)
        dev.grad.copy_(gr)
        host.grad.copy_(gr)
        dev.adam_begin(LR, B1, B2, EPS, ema_decay=decay)(0, n)
        apply = host.adam_begin(LR, B1, B2, EPS, ema_decay=decay)
        apply(0, cut)
        apply(cut, n)
        torch.cuda.synchronize()
        for name in ("flat", "m", "v", "ema"):
            assert torch.equal(getattr(dev, name), getattr(host, name)), (name, dev.step_count)

    for _ in range(3):
        step()
    assert int(dev._count.item()) == 3 and dev.step_count == host.step_count == 3
    assert not torch.equal(dev.flat, init)
    dev.step_count = host.step_count = 7   # as load_adam_state_dict leaves it
    step()
    assert int(dev._count.item()) == 8 and dev.step_count == host.step_count == 8
    if decay:
        assert not torch.equal(dev.ema, ema0)
    else:
        assert torch.equal(dev.ema, ema0) and torch.equal(host.ema, ema0)


# ---------------------------------------------------------------------------------------------
# trainers
# ---------------------------------------------------------------------------------------------

def _cfg(dtype, decay):
    cfg = pkg().Config()
    cfg.device = DEV
    cfg.compute_dtype = dtype
    cfg.deterministic = True
    cfg.ema_decay = decay
    return cfg


def _trainer(dtype="bf16", decay=DECAY, seed=SEED, **kw):
    torch.manual_seed(seed)   # init_net draws G and D from the global generator
    return pkg().GANTrainer(_cfg(dtype, decay), **kw)


def _batches(k, hw=32, seed=11):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand(2, 1, hw, hw, generator=g) * 2 - 1).to(DEV),
             (torch.rand(2, 3, hw, hw, generator=g) * 2 - 1).to(DEV)) for _ in range(k)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_step_is_unchanged_and_ema_follows_the_recurrence(dtype):
    off, on = _trainer(dtype, 0.0), _trainer(dtype, DECAY)
    Go, Gn = off.netG.store, on.netG.store
    assert torch.equal(Go.flat, Gn.flat) and torch.equal(off.netD.store.flat, on.netD.store.flat)
    assert Go.ema is None and "ema" not in off.state_dict()
    assert torch.equal(Gn.ema, Gn.flat) and Gn.ema.data_ptr() != Gn.flat.data_ptr()
    for t, (ir, rgb) in enumerate(_batches(3), start=1):
        e_prev = Gn.ema.clone()
        Lo = off.step(ir, rgb).clone()
        Ln = on.step(ir, rgb).clone()
        torch.cuda.synchronize()
        assert torch.equal(Lo, Ln), (t, Lo.tolist(), Ln.tolist())
        for name in ("flat", "m", "v"):
            assert torch.equal(getattr(Go, name), getattr(Gn, name)), (t, "G." + name)
        assert torch.equal(off.netD.store.flat, on.netD.store.flat), (t, "D.flat")
        assert Gn.step_count == t
        err = (Gn.ema.double() - _ema_ref(e_prev, Gn.flat, _w32(t))).abs()
        bound = _bound(e_prev, Gn.flat)
        print(f"{dtype} t={t}: max err/bound = {(err / bound).max().item():.3f}")
        assert (err <= bound).all(), (t, (err / bound).max().item())
    assert Go.ema is None and "ema" not in off.state_dict()
    assert not torch.equal(Gn.ema, Gn.flat)
    sd = on.state_dict()
    assert list(sd["ema"]) == list(Gn.shapes)
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 for v in sd["ema"].values())
    k = next(iter(Gn.shapes))
    assert torch.equal(sd["ema"][k], Gn.oihw(k, Gn.ema).cpu())


def _bucketed_worker(rank, store, out):
    """World size 1 over RCCL with the gradient collectives forced on: G's Adam + EMA runs
    bucket by bucket behind each all-reduce (BucketedAllreduce.finish)."""
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"file://{store}", rank=0, world_size=1,
                           device_id=torch.device("cuda", 0))
    tr = _trainer("bf16", DECAY, force_reduce=True)
    assert tr.core.g_reduce.active
    spans = []
    finish = tr.core.g_reduce.finish

    def spy(apply=None):
        finish((lambda a, b: (spans.append((a, b)), apply(a, b))) if apply is not None else None)
    tr.core.g_reduce.finish = spy
    for ir, rgb in _batches(2):
        tr.step(ir, rgb)
    torch.cuda.synchronize()
    G = tr.netG.store
    torch.save({"ema": G.ema.cpu(), "flat": G.flat.cpu(), "spans": spans}, os.path.join(out, "bucketed.pt"))
    dist.destroy_process_group()


def test_bucketed_path_gives_the_same_ema(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_bucketed_worker, args=(str(tmp_path / "store"), str(tmp_path)), nprocs=1, join=True)
    r = torch.load(tmp_path / "bucketed.pt", weights_only=True)
    assert len(r["spans"]) > 2, "one bucket per step: the bucketed path did not run"
    tr = _trainer("bf16", DECAY)
    for ir, rgb in _batches(2):
        tr.step(ir, rgb)
    torch.cuda.synchronize()
    G = tr.netG.store
    assert torch.equal(r["flat"], G.flat.cpu())
    assert torch.equal(r["ema"], G.ema.cpu())
    assert not torch.equal(r["ema"], r["flat"])


def test_resume(tmp_path):
    b = _batches(3)
    a = _trainer()
    for ir, rgb in b[:2]:
        a.step(ir, rgb)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path)
    a.step(*b[2])
    Ga = a.netG.store
    # resumed in a fresh trainer (other initial weights: everything comes from the file)
    r = _trainer(seed=SEED + 1)
    assert not torch.equal(r.netG.store.flat, Ga.flat)
    r.load_checkpoint(path)
    r.step(*b[2])
    # ... and once more, entering and leaving ema_weights() before the step: the fused step
    # must find the live weights packed again
    c = _trainer(seed=SEED + 2)
    c.load_checkpoint(path)
    with c.ema_weights():
        pass
    c.step(*b[2])
    torch.cuda.synchronize()
    for tr in (r, c):
        G = tr.netG.store
        assert G.step_count == 3
        assert torch.equal(G.flat, Ga.flat)
        assert torch.equal(G.ema, Ga.ema)
    # an older file (no "ema" entry): the average restarts from the loaded parameters
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert "ema" in sd
    ema_saved = sd.pop("ema")
    old = _trainer(seed=SEED + 3)
    old.load_state_dict(sd)
    Gold = old.netG.store
    assert torch.equal(Gold.ema, Gold.flat) and Gold.ema.data_ptr() != Gold.flat.data_ptr()
    k = next(iter(Gold.shapes))
    assert torch.equal(Gold.oihw(k).cpu(), sd["netG"][k]) and not torch.equal(ema_saved[k], sd["netG"][k])
    # an EMA-off trainer takes the EMA file and ignores the entry
    offt = _trainer(decay=0.0, seed=SEED + 4)
    offt.load_checkpoint(path)
    assert offt.netG.store.ema is None and "ema" not in offt.state_dict()
    assert torch.equal(offt.netG.store.oihw(k).cpu(), sd["netG"][k])


def test_ema_weights_context(tmp_path):
    irc = pkg()
    tr = _trainer()
    for ir, rgb in _batches(2):
        tr.step(ir, rgb)
    G = tr.netG.store
    ir = _batches(1, seed=12)[0][0]
    flat0, ema0 = G.flat.clone(), G.ema.clone()
    assert not torch.equal(flat0, ema0)
    with torch.no_grad():
        live = tr.model(ir).clone()
        with tr.ema_weights() as m:
            assert m is tr.model
            assert torch.equal(G.flat, ema0) and torch.equal(G.ema, flat0)
            inside = tr.model(ir).clone()
            esd = tr.ema_state_dict()
    assert torch.equal(G.flat, flat0) and torch.equal(G.ema, ema0)
    assert not torch.equal(inside, live)
    # a fresh model loading ema_state_dict() from a file computes the same image
    assert list(esd) == list(tr.netG.state_dict())
    k = next(iter(G.shapes))
    assert torch.equal(esd[k], G.oihw(k, G.ema).cpu())
    outside = tr.ema_state_dict()
    assert all(torch.equal(v, outside[key]) for key, v in esd.items())   # asked inside or outside the context
    path = str(tmp_path / "netG_ema.pth")
    torch.save(esd, path)
    torch.manual_seed(SEED + 9)
    fresh = irc.IRColorizationModel(_cfg("bf16", 0.0))
    fresh.load_weights(path)
    with torch.no_grad():
        assert torch.equal(fresh(ir), inside)
        assert torch.equal(tr.model(ir), live)
        # an exception inside the context: swapped back all the same
        with pytest.raises(KeyError):
            with tr.ema_weights():
                raise KeyError("boom")
        assert torch.equal(G.flat, flat0) and torch.equal(G.ema, ema0)
        assert torch.equal(tr.model(ir), live)
    # the three refusals
    with pytest.raises(RuntimeError):
        with tr.ema_weights():
            with tr.ema_weights():
                pass
    with pytest.raises(RuntimeError):
        with tr.ema_weights():
            tr.step(*_batches(1)[0])
    assert torch.equal(G.flat, flat0) and torch.equal(G.ema, ema0)
    offt = _trainer(decay=0.0)
    with pytest.raises(RuntimeError):
        with offt.ema_weights():
            pass
    with pytest.raises(RuntimeError):
        offt.ema_state_dict()


@pytest.mark.parametrize("decay", [DECAY, 0.0], ids=["on", "off"])
def test_train_kaist_files_and_log(tmp_path, decay):
    irc = pkg()
    cfg = irc.Config()
    cfg.device = DEV
    cfg.batch_size, cfg.epochs, cfg.save_every, cfg.img_size = 2, 2, 1, 32
    cfg.save_dir = str(tmp_path / "ck")
    cfg.ema_decay = decay
    lines = []
    torch.manual_seed(SEED)
    hist = irc.train_kaist(cfg, dataset=irc.SyntheticPairDataset(8, 32), log=lines.append)
    files = sorted(os.listdir(cfg.save_dir))
    assert {"netG_epoch_001.pth", "netG_epoch_002.pth", "netG_best.pth"} <= set(files)
    done = [s for s in lines if " DONE | " in s]
    assert len(done) == 2 and len(hist) == 2
    if not decay:
        assert not [f for f in files if "ema" in f.lower()], files
        assert not [s for s in lines if "EMA" in s]
        assert all("val_l1_ema" not in h for h in hist)
        return
    load = lambda f: torch.load(os.path.join(cfg.save_dir, f), map_location="cpu", weights_only=True)  # noqa: E731
    best = load("netG_best.pth")
    for f in ("netG_ema_epoch_001.pth", "netG_ema_epoch_002.pth", "netG_ema_best.pth"):
        assert f in files, files
        assert list(load(f)) == list(best), f
    live, ema = load("netG_epoch_002.pth"), load("netG_ema_epoch_002.pth")
    k = next(iter(live))
    assert not torch.equal(live[k], ema[k])
    assert all(np.isfinite(h["val_l1_ema"]) for h in hist)
    for s in done:   # the EMA line follows the epoch's DONE line
        nxt = lines[lines.index(s) + 1]
        assert "EMA" in nxt and "val L1" in nxt, nxt
