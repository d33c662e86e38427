"""Eval mode of the fp8 generator and its scale state as saved state, on the MI355X.

An eval-mode forward (``training=False``: validate_kaist, run_test, colorize_u8 on a model in
eval(), netG.eval()(x)) reads the delayed-scaling slots (ops.Fp8Acts) and writes none of them;
its one possible state change is the calibration pre-pass on unseen slots.  The scale state
travels with GANTrainer.state_dict() (entry "fp8") and beside a generator checkpoint
(``<file>.fp8``), and the de-quantisation factors a forward used belong to that call.

Everything here is bitwise: the eval kernels' e4m3 bytes against the recording kernels', eval
outputs against each other and against the training-mode forward test_gpu_fp8.py holds to the fp8
oracle, trainers against trainers (ops.set_deterministic, restored afterwards).  Shapes: 64x64,
B=2, ngf=64 -- the smallest at which both fp8 groups run (fp8_layers == (True, True), H/4 = 16 is
one fp8 tile); the module-level tests run 2 ResnetBlocks.
"""
import importlib
import os

import pytest
import torch

from conftest import pkg
from trajectory_data import pair

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, S = 2, 64
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


@pytest.fixture()
def deterministic(ops):
    prev = ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(prev)


def _xy(size):
    """x: the smooth field of trajectory_data; y: faint noise with a few saturated impulses --
    after InstanceNorm its maxima are far from x's, so it calibrates other scales."""
    g = torch.Generator().manual_seed(11)
    x = pair(g, B, size)[0]
    y = torch.randn(B, 1, size, size, generator=g) * 0.02
    for n in range(B):
        for k in range(3):
            i, j = torch.randint(0, size, (2,), generator=g).tolist()
            y[n, 0, i, j] = 1.0 if k % 2 == 0 else -1.0
    return x.to(DEV), y.clamp(-1, 1).to(DEV)


@pytest.fixture(scope="module")
def xy():
    return _xy(S)


def u8(t):
    return t.contiguous().view(torch.uint8)


# ---------------------------------------------------------------------------------------------
# 1. kernels
# ---------------------------------------------------------------------------------------------

def _sentinel_acts(ops, qv):
    """One slot whose scale is qv and whose amax partials hold a sentinel: the read-only Fp8Out of
    it is what an eval-mode forward hands a producer."""
    a = ops.Fp8Acts(1, DEV)
    a.q.fill_(qv)
    a.dq.fill_(1.0 / qv)
    a.amax.fill_(SENTINEL)
    return a


def _untouched(a, qv):
    assert (a.amax.cpu() == SENTINEL).all() and a.q.item() == qv and a.dq.item() == 1.0 / qv and a.seen == [False]


@pytest.mark.parametrize("N,H,W,C,relu", [(3, 15, 17, 256, True), (2, 64, 64, 256, True), (2, 16, 16, 8, False)],
                         ids=["ragged-rows", "several-blocks", "narrow"])
def test_in_apply_fp8_eval_forms(ops, N, H, W, C, relu):
    """irgan_in_apply_fp8 with y=NULL, amax=NULL writes the y8 bytes of the full call and
    records nothing; with a residual, amax=NULL alone leaves y and y8 as the full call's, and
    y=NULL is IRGAN_EINVAL with nothing written (so it is together with the amax record)."""
    torch.manual_seed(5)
    Fe = ops.Feat
    act = ops.ACT_RELU if relu else ops.ACT_NONE
    z = (torch.randn(N, H, W, C) * 1.7 + 0.3).bfloat16().to(DEV)
    res = torch.randn(N, H, W, C).bfloat16().to(DEV)
    mr = torch.empty(N * C * 2, device=DEV)
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    ops.in_stats(Fe(z), work, mr)
    qv = 8.0
    qt = torch.tensor([qv], device=DEV)

    def full(r):
        y = torch.empty_like(z)
        y8 = torch.empty(z.shape, dtype=torch.float8_e4m3fn, device=DEV)
        amax = ops.amax_slots(1, DEV)
        ops.in_apply(Fe(z), mr, Fe(y), act=act, res=r, q8=(Fe(y8), ops.Pi(qt, 0), ops.amax_ptr(amax, 0)))
        assert amax.max().item() > 0
        return y, y8

    # y8 alone, nothing recorded
    y, y8 = full(None)
    assert u8(y8).any()
    a = _sentinel_acts(ops, qv)
    got8 = torch.zeros(z.shape, dtype=torch.float8_e4m3fn, device=DEV)
    out = ops.Fp8Out(a, 0, Fe(got8), record=False)
    assert out.side[2] is None
    ops.in_apply(Fe(z), mr, None, act=act, q8=out.side)
    out.finish(None)
    assert torch.equal(u8(got8), u8(y8))
    _untouched(a, qv)
    # y and y8, nothing recorded (no residual, then with one)
    for r in (None, Fe(res)):
        y, y8 = full(r)
        goty, got8 = torch.zeros_like(z), torch.zeros(z.shape, dtype=torch.float8_e4m3fn, device=DEV)
        ops.in_apply(Fe(z), mr, Fe(goty), act=act, res=r, q8=ops.Fp8Out(a, 0, Fe(got8), record=False).side)
        assert torch.equal(goty.view(torch.int16), y.view(torch.int16)) and torch.equal(u8(got8), u8(y8))
        _untouched(a, qv)
    # y == NULL with a residual, or with the amax record: IRGAN_EINVAL, nothing written
    lib = importlib.import_module(pkg().__name__ + "._lib")
    einval = lib.header_enum("IRGAN_EINVAL")
    got8 = torch.full(z.shape, 0x5A, dtype=torch.uint8, device=DEV)
    for rp, ap in ((ops.P(res), None), (ops.P(res), ops.amax_ptr(a.amax, 0)), (None, ops.amax_ptr(a.amax, 0))):
        rc = lib.load().irgan_in_apply_fp8(ops.P(z), N, H * W, C, C, 0, ops.P(mr), act, rp, C, 0, None, 0, 0,
                                           ops.P(got8), C, 0, ops.Pi(qt, 0), ap, ops.stream())
        assert rc == einval
    torch.cuda.synchronize()
    assert (got8 == 0x5A).all()
    _untouched(a, qv)


def test_resamplers_fp8_without_amax(ops):
    """irgan_sep_resample_fp8 with amax=NULL, at the shapes of test_resamplers_emit_fp8_copy
    (down1's Downsample of act(IN(z)) into the x1 slice, the UpsampleAA of h into the other):
    out and y8 bytes as with the record, nothing recorded.  Third case: the same up-sampling from
    an fp32 h, which the row-pipelined kernel does not take -- the one-row-per-block form runs."""
    torch.manual_seed(6)
    Fe = ops.Feat
    N, H, C1, C2 = 2, 20, 128, 256
    z = torch.randn(N, 2 * H, 2 * H, C1).bfloat16().to(DEV)
    mr = torch.empty(N * C1 * 2, device=DEV)
    work = torch.empty(ops.IN_PARTS * N * C1, dtype=torch.float64, device=DEV)
    ops.in_stats(Fe(z), work, mr)
    h = torch.randn(N, H // 2, H // 2, C2).bfloat16().to(DEV)
    qv = 32.0
    qt = torch.tensor([qv], device=DEV)
    for kind in ("down_in", "up", "up_f32"):
        off, c = (C2, C1) if kind == "down_in" else (0, C2)
        src = h.float() if kind == "up_f32" else h
        a = _sentinel_acts(ops, qv)
        outs = []
        for rec in (True, False):
            cat = torch.zeros(N, H, H, C2 + C1, dtype=torch.bfloat16, device=DEV)
            cat8 = torch.zeros(N, H, H, C2 + C1, dtype=torch.float8_e4m3fn, device=DEV)
            amax = ops.amax_slots(1, DEV)
            q8 = (Fe(cat8, off, c), ops.Pi(qt, 0), ops.amax_ptr(amax, 0)) if rec else \
                ops.Fp8Out(a, 0, Fe(cat8, off, c), record=False).side
            if kind == "down_in":
                assert ops.blur_down_in(Fe(z), mr, ops.ACT_RELU, Fe(cat, off, c), q8=q8)
            else:
                yt, xt = ops._up_axis(h.shape[1], H, False), ops._up_axis(h.shape[2], H, False)
                assert ops.sep_resample_fp8(Fe(src), None, ops.ACT_NONE, Fe(cat, off, c), yt, xt, q8)
            assert rec == (amax.max().item() > 0)
            outs.append((cat, cat8))
        (cat, cat8), (ecat, ecat8) = outs
        assert u8(cat8).any()
        assert torch.equal(cat.view(torch.int16), ecat.view(torch.int16)), kind
        assert torch.equal(u8(cat8), u8(ecat8)), kind
        _untouched(a, qv)


# ---------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------

def _netG(n_blocks=2, seed=1):
    """An fp8 generator with seeded weights, in eval() (the tests name the mode per call)."""
    irc = pkg()
    net = irc.ResnetUNetGenerator(1, 3, 64, n_blocks=n_blocks, device=DEV, compute_dtype="fp8")
    net.store.load(irc.seeded_state(irc.g_param_shapes(1, 3, 64, n_blocks), seed, bias_std=0.02), strict=True)
    net.repack()
    assert net.engine.fp8_layers(B, S, S) == (True, True)
    return net.eval()


def _fwd_slots(eng):
    """The slots a forward reads: the ResnetBlock operands and the concat."""
    (f0, fn), (c0, cn) = eng.fp8_slots["fwd"], eng.fp8_slots["cat"]
    return list(range(f0, f0 + fn)) + list(range(c0, c0 + cn))


def _state(eng):
    A = eng.f8a
    return A.q.cpu().clone(), A.dq.cpu().clone(), A.amax.cpu().clone(), list(A.seen)


def _same_state(a, b):
    return all(torch.equal(u, v) for u, v in zip(a[:3], b[:3])) and a[3] == b[3]


def _calibrates_differently(make, eng, y):
    """The precondition of the history tests: a fresh model of the same weights calibrated on y
    alone ends with a q different from ``eng``'s in at least one forward slot."""
    other = make()
    other.engine.forward(y, training=False)
    sl = _fwd_slots(eng)
    assert all(other.engine.f8a.seen[s] for s in sl)
    return not torch.equal(other.engine.f8a.q.cpu()[sl], eng.f8a.q.cpu()[sl])


# 2 ---------------------------------------------------------------------------------------------

def test_eval_forward_leaves_scales_frozen(xy):
    x, _ = xy
    net = _netG()
    eng = net.engine
    eng.forward(x, training=False)   # calibrates
    assert eng.fp8_prepasses == 1 and all(eng.f8a.seen[s] for s in _fwd_slots(eng))
    sl = torch.tensor(_fwd_slots(eng), device=DEV)
    eng.f8a.q[sl] *= 0.5             # a valid scale with one more bit of headroom
    eng.f8a.dq[sl] *= 2.0
    before = _state(eng)
    out = eng.forward(x, training=False)
    assert torch.isfinite(out).all()
    assert _same_state(before, _state(eng)) and eng.fp8_prepasses == 1
    # no bf16 t map: the engine's own set still holds the pre-pass's, so look at a fresh set
    fresh = importlib.import_module(pkg().__name__ + ".engine").Buffers(x.device)
    out2 = eng.forward(x, bufs=fresh, training=False).clone()
    assert torch.equal(out2, out) and _same_state(before, _state(eng))
    assert not any(k.startswith("t") and k[1:].isdigit() for k in fresh.d), sorted(fresh.d)


# 3 ---------------------------------------------------------------------------------------------

def test_eval_is_idempotent_and_history_free(xy):
    irc = pkg()
    x, y = xy
    m = _netG()
    a = irc.inference.colorize_u8(m, x).clone()
    assert _calibrates_differently(_netG, m.engine, y), "y calibrates the same scales as x: choose another y"
    b = irc.inference.colorize_u8(m, x).clone()
    irc.inference.colorize_u8(m, y)
    c = irc.inference.colorize_u8(m, x).clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert m.engine.fp8_prepasses == 1
    # reset_fp8_scales(): every slot unseen, the next eval call calibrates again (now on y)
    m.engine.reset_fp8_scales()
    assert not any(m.engine.f8a.seen)
    irc.inference.colorize_u8(m, y)
    assert m.engine.fp8_prepasses == 2


# 4 ---------------------------------------------------------------------------------------------

def test_eval_equals_second_training_forward(xy):
    """The pre-pass is a first training-mode call, the frozen pass a second one: bitwise the
    output of the forward test_gpu_fp8.py holds to the fp8 oracle (so the e4m3-only apply and
    the record-free producers change no byte downstream)."""
    x, _ = xy
    m1, m2 = _netG(), _netG()
    m1.engine.forward(x, training=True)
    want = m1.engine.forward(x, training=True).clone()
    got = m2.engine.forward(x, training=False).clone()
    assert torch.equal(got, want)
    sl = _fwd_slots(m1.engine)
    print("forward q, training x2:", m1.engine.f8a.q.cpu()[sl].tolist())
    print("forward q, eval       :", m2.engine.f8a.q.cpu()[sl].tolist())
    assert torch.equal(m1.engine.f8a.q.cpu()[sl], m2.engine.f8a.q.cpu()[sl])


# 5, 6 ------------------------------------------------------------------------------------------

def _trainer(dtype="fp8", seed_shift=0):
    from oracle import step as O
    irc = pkg()
    cfg = irc.Config()
    cfg.device = DEV
    cfg.compute_dtype = dtype
    cfg.batch_size = B
    cfg.img_size = S
    tr = irc.GANTrainer(cfg)
    tr.netG.store.load(O.seeded_params(O.g_param_shapes(), 1 + seed_shift, bias_std=0.02), strict=True)
    tr.netD.store.load(O.seeded_params(O.d_param_shapes(), 2 + seed_shift, bias_std=0.02), strict=True)
    tr.vgg.store.load(O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True), strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    return tr


def _batches(n, seed=31):
    g = torch.Generator().manual_seed(seed)
    return [tuple(t.to(DEV) for t in pair(g, B, S)) for _ in range(n)]


def _same_training_state(a, b):
    for name in ("netG", "netD"):
        sa, sb = getattr(a, name).store, getattr(b, name).store
        assert torch.equal(sa.flat, sb.flat), name + " parameters"
        assert torch.equal(sa.m, sb.m) and torch.equal(sa.v, sb.v), name + " Adam state"
        assert sa.step_count == sb.step_count


def test_validation_leaves_training_alone(xy, deterministic):
    irc = pkg()
    _, y = xy
    bt = _batches(3)
    ta, tb = _trainer(), _trainer()
    la = [ta.step(*bt[k]).clone() for k in range(3)]
    lb = [tb.step(*bt[k]).clone() for k in range(2)]
    eng = tb.netG.engine

    def probe():   # a fresh fp8 generator with B's weights of this moment
        net = _netG(n_blocks=9)
        net.store.flat.copy_(tb.netG.store.flat)
        net.repack()
        return net
    assert _calibrates_differently(probe, eng, y), "the validation batch calibrates B's scales: choose another"
    before = _state(eng)
    val = [{"ir": y, "rgb": torch.zeros(B, 3, S, S, device=DEV)}, {"ir": -y, "rgb": torch.zeros(B, 3, S, S, device=DEV)}]
    v = irc.validate_kaist(tb.model, val, DEV)
    assert v == v and _same_state(before, _state(eng)) and eng.fp8_prepasses == 0
    lb.append(tb.step(*bt[2]).clone())
    _same_training_state(ta, tb)
    for u, w in zip(la, lb):
        assert torch.equal(u, w)


def test_resume_restores_fp8_scales(tmp_path, deterministic):
    bt = _batches(4, seed=32)
    a = _trainer()
    for k in range(3):
        a.step(*bt[k])
    path = tmp_path / "full.pt"
    a.save_checkpoint(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert set(sd["fp8"]) == {"q", "dq", "amax", "seen"}
    b = _trainer(seed_shift=10)
    b.load_checkpoint(path)
    sa, sb = _state(a.netG.engine), _state(b.netG.engine)
    assert _same_state(sa, sb)
    assert all(sb[3][s] for s in _fwd_slots(b.netG.engine)) and not (sb[0] == 1).all()
    la, lb = a.step(*bt[3]), b.step(*bt[3])
    assert torch.equal(la, lb)
    _same_training_state(a, b)
    # a file without the entry: every slot unseen again
    del sd["fp8"]
    b.load_state_dict(sd)
    assert not any(b.netG.engine.f8a.seen) and (b.netG.engine.f8a.q == 1).all() and not b.netG.engine.f8a.amax.any()
    # a mismatching entry names both counts
    bad = a.state_dict()["fp8"]
    bad = {k: (v[:-1] if k != "amax" else v[:-pkg().ops.FP8_AMAX_PARTS]) for k, v in bad.items()}
    with pytest.raises(ValueError) as ei:
        b.netG.load_fp8_state_dict(bad)
    n = len(b.netG.engine.f8a.seen)
    assert str(n) in str(ei.value) and str(n - 1) in str(ei.value)


def test_other_dtypes_keep_their_state_dict_keys():
    tr = _trainer("fp32")
    sd = tr.state_dict()
    assert list(sd) == ["netG", "netD", "optimizer_G", "optimizer_D", "epoch_index", "lr_scale"]
    assert tr.netG.fp8_state_dict() is None
    # an fp8 entry in the file is ignored by a trainer of another dtype
    sd["fp8"] = {"q": torch.ones(3), "dq": torch.ones(3), "amax": torch.zeros(3, dtype=torch.int32),
                 "seen": torch.ones(3, dtype=torch.bool)}
    tr.load_state_dict(sd)
    assert list(tr.state_dict()) == list(sd)[:-1]


# 7 ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [S, 256])
def test_module_api_backward_reads_its_own_call(size, deterministic):
    """A forward between an autograd forward and its backward moves the shared scales; the weight
    gradients still de-quantise the first call's e4m3 operands with the first call's factors.
    The recorded forward runs on scales delayed from y, so the factors it used are not the ones
    a later forward finds (after a calibrating first call the two would coincide).
    Besides 64x64, 256x256: irgan_conv_wgrad_fp8 takes output rows of 64 or a multiple of 128
    pixels, so only from W/4 = 64 on do the weight gradients of both groups read the e4m3
    operands at all (below, they fall back to the bf16 operands and the factors are never used)."""
    x, y = _xy(size)
    gout = torch.randn(B, 3, size, size, generator=torch.Generator().manual_seed(3)).to(DEV) * 1e-2

    def grads(middle):
        net = _netG().train()
        sl = _fwd_slots(net.engine)
        with torch.no_grad():
            net(y)   # training mode: the shared forward scales are now y's
        used = net.engine.f8a.dq.cpu()[sl]
        out, _ = net(x)   # quantises with y's scales, rolls the slots on to x's
        assert not torch.equal(used, net.engine.f8a.dq.cpu()[sl]), "the shared scales did not move"
        if middle:
            with torch.no_grad():
                net(y)   # uses x's scales, rolls on to y's
        out.backward(gout)
        return out.detach().clone(), [p.grad.clone() for p in net.parameters()]

    out_a, ga = grads(False)
    out_b, gb = grads(True)
    assert torch.equal(out_a, out_b)
    assert any(g.abs().max() > 0 for g in ga)
    for k, (u, w) in enumerate(zip(ga, gb)):
        assert torch.equal(u, w), f"parameter {k}"


def test_backward_of_an_eval_forward_rolls_its_dy_slots(xy, deterministic):
    """A module in eval() under autograd: the forward is frozen (and keeps the bf16 maps its
    backward reads), the backward treats its dY slots as every backward does -- it calibrates or
    records them, rolls them and clears the maxima -- and never touches a forward slot.
    The eval call is a calibration pre-pass plus the frozen pass, i.e. the second of two
    training-mode forwards, so a train() module after one no_grad forward is the yardstick:
    same output, same parameter gradients, same dY slots, bit for bit.  A second backward with a
    64 times larger dout moves the first dY scale in the chain, up1_conv's, down by exactly 2^6 (the
    later ones see gradients the delayed scale has clamped: not up), and leaves no maximum behind."""
    x, _ = xy
    gout = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(4)).to(DEV) * 1e-2
    ev, tr = _netG(), _netG().train()
    eng = ev.engine
    (d0, dn), (u0, un) = eng.fp8_slots["dy"], eng.fp8_slots["ud_dy"]
    dys = list(range(d0, d0 + dn)) + list(range(u0, u0 + un))
    fw = _fwd_slots(eng)

    def run(net, dout):
        out, _ = net(x)
        out.backward(dout)
        return out.detach().clone(), [p.grad.clone() for p in net.parameters()]

    with torch.no_grad():
        tr(x)
    out_t, g_t = run(tr, gout)
    out_e, g_e = run(ev, gout)
    assert eng.fp8_prepasses == 1 and not ev.training
    assert torch.equal(out_e, out_t)
    for k, (u, w) in enumerate(zip(g_e, g_t)):
        assert torch.equal(u, w), f"parameter {k}"
    se, st_ = _state(eng), _state(tr.engine)
    assert all(se[3][s] for s in dys) and not se[2].any(), "dY slots calibrated, maxima cleared"
    assert torch.equal(se[0][dys], st_[0][dys]) and torch.equal(se[1][dys], st_[1][dys])
    assert not (se[0][dys] == 1).all()
    # a second call with larger gradients: the dY slots roll on, the forward slots stay
    out_e2, _ = run(ev, gout * 64)
    s2 = _state(eng)
    assert torch.equal(out_e2, out_e) and eng.fp8_prepasses == 1
    assert (s2[0][dys] <= se[0][dys]).all() and torch.equal(s2[1][dys], 1.0 / s2[0][dys])
    up1_dy = eng.c_up1.rec.s_dy
    assert s2[0][up1_dy].item() == se[0][up1_dy].item() / 64
    assert not s2[2].any()
    assert torch.equal(s2[0][fw], se[0][fw]) and torch.equal(s2[1][fw], se[1][fw])
    assert [s2[3][s] for s in fw] == [se[3][s] for s in fw]


# 8 ---------------------------------------------------------------------------------------------

def test_sidecar_file_restores_eval_scales(tmp_path, xy):
    irc = pkg()
    x, y = xy

    def model(seed):
        torch.manual_seed(seed)
        cfg = irc.Config()
        cfg.device = DEV
        cfg.compute_dtype = "fp8"
        return irc.IRColorizationModel(cfg).eval()

    m = model(1)
    irc.inference.colorize_u8(m, y)            # calibrated on y ...
    want = irc.inference.colorize_u8(m, x).clone()   # ... so a calibration on x would show
    assert m.netG.engine.fp8_prepasses == 1
    path = str(tmp_path / "netG_best.pth")
    ic = importlib.import_module(pkg().__name__ + ".ir_colorization")
    ic._save_generator(m.netG, path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert len(sd) == 52 and list(sd) == list(m.netG.state_dict())
    side = torch.load(path + ".fp8", map_location="cpu", weights_only=True)
    assert set(side) == {"q", "dq", "amax", "seen"}
    m2 = model(2)
    said = []
    m2.load_weights(path, log=said.append)
    assert len(said) == 1 and path + ".fp8" in said[0]   # never silently
    got = irc.inference.colorize_u8(m2, x)
    assert m2.netG.engine.fp8_prepasses == 0
    assert torch.equal(got, want)
    # without the sidecar file the first batch calibrates through the pre-pass
    os.remove(path + ".fp8")
    m3 = model(3)
    m3.load_weights(path, log=said.append)
    assert len(said) == 1
    assert not any(m3.netG.engine.f8a.seen)
    irc.inference.colorize_u8(m3, x)
    assert m3.netG.engine.fp8_prepasses == 1
