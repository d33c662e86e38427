"""Grouped ResnetBlock weight gradients (irgan_conv_wgrad_group, ops.conv_wgrad_group): up to
four problems of one geometry in one wide-n launch and one ordered reduce, and the generator
backward that defers its ResnetBlock weight gradients into such groups.

Kernel level, against fp64 on the same bf16 operands with the bound of
test_gpu_bf16_parity.test_bf16_conv_family_tight's weight gradient (the tile index and the split
count differ between the two entry points, the arithmetic does not); count 1 bit-identical to
ops.conv_wgrad (in deterministic mode: every count); a problem's result independent of its
neighbours; repeatable; rejected calls leave dw alone.  Step level: one GANTrainer.step with grouping on and off."""
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden, pkg
from oracle import step as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_ACC = 2e-5   # fp32 accumulation (test_gpu_bf16_parity.R_ACC)
N = 2

# (Cin, Cout, pad mode, H, W): one and several tiles, a partial last segment (70), two segments
# per row (130), a row shorter than a segment (the resblock map of a 64^2 image)
CASES = [(128, 128, 0, 5, 64), (256, 256, 1, 4, 70), (256, 128, 0, 3, 130), (128, 256, 1, 16, 16)]


def q(t):
    """bf16-representable copy (fp32 storage)."""
    return t.bfloat16().float()


def nhwc(x, dt=torch.bfloat16):
    return x.permute(0, 2, 3, 1).contiguous().to(DEV, dt)


def ref_dw(x, gy, cout, mode):
    """fp64 weight gradient of the 3x3, stride-1, pad-1 conv (zero or reflect) on the given operands."""
    w = torch.zeros(cout, x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
    xd = x.double()
    if mode == 1:
        y = F.conv2d(F.pad(xd, (1, 1, 1, 1), mode="reflect"), w)
    else:
        y = F.conv2d(xd, w, padding=1)
    y.backward(gy.double())
    return w.grad


def check(got, ref, aref, what):
    bound = R_ACC * aref + 1e-30
    err = (got - ref).abs()
    ratio = (err / bound).max().item()
    print(f"{what}: worst |err|/bound = {ratio:.3g}, max |err| {err.max().item():.3g}")
    assert ratio <= 1.0, f"{what}: worst |err|/bound = {ratio:.3g}, max |err| {err.max().item():.3g}"


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


_PROBLEMS = {}


def problem(case, seed):
    """Seeded operands of one problem of ``case`` and its fp64 references, computed once."""
    key = (case, seed)
    if key not in _PROBLEMS:
        cin, cout, mode, H, W = case
        g = torch.Generator().manual_seed(1000 * CASES.index(case) + seed)
        x = q(torch.randn(N, cin, H, W, generator=g))
        gy = q(torch.randn(N, cout, H, W, generator=g))
        dw0 = torch.randn(cout * 9 * cin, generator=g)
        _PROBLEMS[key] = dict(x=nhwc(x), gy=nhwc(gy), dw0=dw0.to(DEV), ref=ref_dw(x, gy, cout, mode),
                              aref=ref_dw(x.abs(), gy.abs(), cout, mode))
    return _PROBLEMS[key]


def run_group(ops, case, seeds, ws=None):
    """The grouped launch over the problems ``seeds``; (ok, [dw], [problem])."""
    cin, cout, mode, H, W = case
    spec = ops.ConvSpec(cin, cout, 3, 1, 1, mode)
    ps = [problem(case, s) for s in seeds]
    dws = [p["dw0"].clone() for p in ps]
    ok = ops.conv_wgrad_group(spec, [ops.Feat(p["x"]) for p in ps], [ops.Feat(p["gy"]) for p in ps], dws, ops.BF16,
                              ws=ws)
    torch.cuda.synchronize()
    return ok, dws, ps


@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("case", CASES)
def test_group_against_fp64(ops, case, count):
    """(a) every problem's dw - dw0 within the fp32-accumulation bound of fp64; (b) count 1
    bit-identical to ops.conv_wgrad."""
    cin, cout, mode, H, W = case
    ok, dws, ps = run_group(ops, case, list(range(count)))
    assert ok, "the grouped launch refused a wide-n shape"
    for i, (dw, p) in enumerate(zip(dws, ps)):
        got = (dw - p["dw0"]).view(cout, 3, 3, cin).permute(0, 3, 1, 2).double().cpu()
        check(got, p["ref"], p["aref"] + p["dw0"].abs().max().item() * 1e-2, f"{case} count {count} problem {i}")
    if count == 1:
        one = ps[0]["dw0"].clone()
        ops.conv_wgrad(ops.ConvSpec(cin, cout, 3, 1, 1, mode), ops.Feat(ps[0]["x"]), ops.Feat(ps[0]["gy"]), one,
                       ops.BF16)
        assert torch.equal(one, dws[0]), "count 1 differs from ops.conv_wgrad"


@pytest.mark.parametrize("case", CASES)
def test_group_problems_independent(ops, case):
    """(c) dW_A of the group (A, B, C) and of (A, B', C') bit-identical."""
    _, a, _ = run_group(ops, case, [0, 1, 2])
    _, b, _ = run_group(ops, case, [0, 3, 4])
    assert torch.equal(a[0], b[0]), "a problem's gradient depends on its neighbours in the group"
    assert not torch.equal(a[1], b[1])


@pytest.mark.parametrize("case", CASES)
def test_group_repeatable(ops, case):
    """(d) two runs of one group bit-identical, in deterministic mode and out of it (the grouped
    path has no atomics either way).  In deterministic mode every problem also keeps the splits of
    a launch of its own: each dw is ops.conv_wgrad's bit for bit, whatever the count."""
    cin, cout, mode, H, W = case
    spec = ops.ConvSpec(cin, cout, 3, 1, 1, mode)
    for det in (True, False):
        old = ops.set_deterministic(det)
        try:
            (ok, first, ps), (_, second, _) = (run_group(ops, case, [0, 1, 2]) for _ in range(2))
            assert ok
            assert all(torch.equal(x, y) for x, y in zip(first, second)), f"deterministic {det}: not repeatable"
            if det:
                for dw, p in zip(first, ps):
                    one = p["dw0"].clone()
                    ops.conv_wgrad(spec, ops.Feat(p["x"]), ops.Feat(p["gy"]), one, ops.BF16)
                    assert torch.equal(one, dw), "deterministic mode: a grouped dw differs from ops.conv_wgrad"
        finally:
            ops.set_deterministic(old)


def test_group_rejected_calls_touch_nothing(ops):
    """(e) count 5, or a workspace one float too small: False and every dw as it was."""
    case = CASES[1]
    cin, cout, mode, H, W = case
    ok, dws, ps = run_group(ops, case, [0, 1, 2, 3, 4])
    assert not ok
    assert all(torch.equal(dw, p["dw0"]) for dw, p in zip(dws, ps))
    # splits of a 3-problem launch: CUs / (tiles * 3), at most a quarter of the 64-pixel segments
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    tiles, nseg = (cout // 128) * (cin // 128) * 3, N * H * -(-W // 64)
    sk = max(1, min(cus // (tiles * 3), -(-nseg // 4)))
    sk = -(-nseg // -(-nseg // sk))
    need = 3 * sk * cout * 9 * cin
    ok, dws, ps = run_group(ops, case, [0, 1, 2], ws=torch.empty(need - 1, device=DEV))
    assert not ok
    assert all(torch.equal(dw, p["dw0"]) for dw, p in zip(dws, ps))
    ok, dws, ps = run_group(ops, case, [0, 1, 2], ws=torch.empty(need, device=DEV))
    assert ok, "a workspace of exactly count * splits * n floats was refused"
    ref = run_group(ops, case, [0, 1, 2])[1]
    assert all(torch.equal(x, y) for x, y in zip(dws, ref))


# ---------------------------------------------------------------------------- step level

LAMBDA_ORDER = ("lambda_L1", "lambda_perc", "lambda_tv", "lambda_ssim", "lambda_gan")


def make_trainer(fx, n_blocks):
    irc = pkg()
    cfg = irc.Config()
    cfg.device, cfg.compute_dtype = DEV, "bf16"
    for k, v in zip(LAMBDA_ORDER, fx["lambdas"]):
        setattr(cfg, k, float(v))
    model = irc.IRColorizationModel(cfg)
    if n_blocks != 9:
        model.netG = irc.ResnetUNetGenerator(cfg.input_nc, cfg.output_nc, cfg.ngf, n_blocks=n_blocks, device=DEV,
                                             compute_dtype="bf16")
    tr = irc.GANTrainer(cfg, model=model)
    tr.netG.store.load(O.seeded_params(O.g_param_shapes(n_blocks=n_blocks), 1, bias_std=0.02), strict=True)
    tr.netD.store.load(O.seeded_params(O.d_param_shapes(), 2, bias_std=0.02), strict=True)
    tr.vgg.store.load(O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True), strict=True)
    for m in (tr.netG, tr.netD, tr.vgg):
        m.repack()
    return tr


@pytest.mark.parametrize("det", [True, False])
@pytest.mark.parametrize("n_blocks,group", [(9, 3), (2, 3), (9, 4)])
def test_step_grouping_on_and_off(ops, n_blocks, group, det):
    """One step at 64^2, B = 2, bf16, from one seeded state with the ResnetBlock weight gradients
    grouped (3 per launch; n_blocks 2: groups of 3 and 1, the tail flush; 4 per launch, the
    engine's default: 18 layers as 4 x 4 + 2) and per layer.  Deterministic mode: everything but
    the ResnetBlock conv gradients bit-identical, those within relative L2 1e-3 (they keep the
    per-layer splits there, so they are in fact equal too: asserted).  Default mode, where the
    grouped launch splits each layer count times fewer ways and other layers reduce with fp32
    atomics: the ResnetBlock conv gradients within relative L2 1e-3 (only the number of fp32
    partials per element differs; the activations of one step do not depend on any dW), and
    each network's whole gradient within the same bound (the atomics' order)."""
    fx = load_golden("s64")
    g = torch.Generator().manual_seed(77)
    ir = (torch.rand(2, 1, 64, 64, generator=g) * 2 - 1).to(DEV)
    rgb = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    old_det = ops.set_deterministic(det)
    old_grp = ops.set_wgrad_group(3)
    try:
        grads = {}
        for grp in (group, 0):
            ops.set_wgrad_group(grp)
            tr = make_trainer(fx, n_blocks)
            tr.step(ir, rgb)
            torch.cuda.synchronize()
            grads[grp] = (tr.netG.store, tr.netD.store.grad.clone())
    finally:
        ops.set_wgrad_group(old_grp)
        ops.set_deterministic(old_det)

    def rel_l2(a, b):
        return ((a - b).double().norm() / b.double().norm()).item()

    sa, sb = grads[group][0], grads[0][0]
    if det:
        assert torch.equal(grads[group][1], grads[0][1]), "D gradients differ"
    else:
        assert rel_l2(grads[group][1], grads[0][1]) <= 1e-3
        assert rel_l2(sa.grad, sb.grad) <= 1e-3
    res = {f"{c.key}.weight" for pair in tr.netG.engine.blocks for c in pair}
    assert len(res) == 2 * n_blocks
    for key in sa.shapes:
        a, b = sa.krsc(key, sa.grad), sb.krsc(key, sb.grad)
        if key in res:
            rel = rel_l2(a, b)
            print(f"{key}: deterministic {det}, relative L2 {rel:.3g}")
            assert b.abs().max() > 0 and rel <= 1e-3, (key, rel)
            assert not det or torch.equal(a, b), f"{key}: deterministic mode depends on the group size"
        elif det:
            assert torch.equal(a, b), f"{key}: gradient differs outside the ResnetBlock convs"
