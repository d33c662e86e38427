"""csrc/batchnorm.hip on the MI355X against fp64 ``F.batch_norm`` + autograd on the SAME
operands (fp32, and bf16-representable values for the bf16 runs): forward y, {mean, rstd},
the running buffers, dx, dgamma, dbeta; the group semantics; eval mode; the {shift, scale}
table of the fused resample consumers.

Bounds (the ones the InstanceNorm kernels are held to):
  fp32 -- tests/test_gpu_kernels.py::test_instance_norm_fwd_bwd: max-rel 1e-5 on the forward
          (here also on the statistics and running buffers), 1e-4 on the backward (dx, and the
          dgamma / dbeta sums);
  bf16 -- tests/test_gpu_bf16_elementwise.py: |got - ref| <= 2^-8 |ref| + r_acc * absref per
          element, r_acc 1e-5 for the apply expressions and 2e-5 for the fp32 sums; the
          statistics are fp32 outputs in either mode and keep the fp32 bound.
"""
import pytest
import torch
import torch.nn.functional as F

from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
R_BF16 = 2.0 ** -8
TDT = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


def relerr(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def bound_ratio(got, ref, aref, r_out, r_acc):
    err = (got.double() - ref).abs()
    return float((err / (r_out * ref.abs() + r_acc * aref + 1e-30)).max())


def to_slice(x, dt, ld, off, fill=7.0):
    """NCHW CPU -> NHWC device tensor of width ld, x in channels [off, off + C) (junk around)."""
    N, C, H, W = x.shape
    t = torch.full((N, H, W, ld), fill, device=DEV, dtype=dt)
    t[..., off:off + C] = x.permute(0, 2, 3, 1).to(DEV, dt)
    return t


def from_slice(t, off, C):
    return t[..., off:off + C].double().cpu().permute(0, 3, 1, 2).contiguous()


def act64(h, act):
    return {0: h, 1: F.relu(h), 2: F.leaky_relu(h, 0.2)}[act]


# name: (N, H, W, C, groups, ld, off, act, residual + dy2, data mean, data std)
CASES = {
    "c8": (3, 5, 7, 8, 1, 8, 0, 1, False, 0.7, 2.0),
    "c24_g1": (4, 9, 11, 24, 1, 24, 0, 2, False, -0.3, 1.5),
    "c24_g2": (4, 9, 11, 24, 2, 24, 0, 2, False, -0.3, 1.5),
    "c64_wide": (2, 16, 16, 64, 1, 96, 16, 1, False, 0.2, 1.0),
    "c12_scalar": (2, 6, 5, 12, 1, 12, 0, 2, False, 0.5, 2.0),
    "c16_res_dy2": (2, 7, 9, 16, 1, 16, 0, 0, True, 0.1, 1.0),
    "c8_mean100": (3, 5, 7, 8, 1, 8, 0, 1, False, 100.0, 0.1),
}


def make_case(name, dtype, seed=0):
    N, H, W, C, G, ld, off, act, extra, mu, sd = CASES[name]
    g = torch.Generator().manual_seed(seed + 17)
    dt = TDT[dtype]
    rnd = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    q = (lambda t: t.to(dt).float()) if dtype == "bf16" else (lambda t: t)  # noqa: E731
    x = q(rnd(N, C, H, W) * sd + mu)
    gamma, beta = 1 + 0.5 * rnd(C), 0.3 * rnd(C)
    gamma[1] = 0.0                       # an exactly-zero scale
    gamma[2] = -gamma[2].abs() - 0.1     # and a negative one
    if mu == 100.0:
        beta[:] = 0.02 * rnd(C)          # both signs of gamma * xhat + beta stay populated
    c = dict(name=name, N=N, H=H, W=W, C=C, G=G, ld=ld, off=off, act=act, dtype=dtype, dt=dt, x=x, gamma=gamma,
             beta=beta, dy=q(rnd(N, C, H, W)), res=q(rnd(N, C, H, W)) if extra else None,
             dy2=q(rnd(N, C, H, W) * 0.5) if extra else None,
             rm0=0.1 * rnd(C), rv0=0.5 + torch.rand(C, generator=g))
    return c


def reference(c, repeat=1, mask_on_xhat=False, biased_running_var=False, x=None, dy=None, dy2=None, res=None):
    """fp64 F.batch_norm per group (training), the running buffers updated group after group,
    each ``repeat`` times; autograd for dx / dgamma / dbeta."""
    x = (c["x"] if x is None else x).double().requires_grad_(True)
    dy = c["dy"] if dy is None else dy
    dy2, res = c["dy2"] if dy2 is None else dy2, c["res"] if res is None else res
    gamma, beta = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    rm, rv = c["rm0"].double().clone(), c["rv0"].double().clone()
    N, G = x.shape[0], c["G"]
    ng = N // G
    outs, means, rstds = [], [], []
    for gi in range(G):
        xg = x[gi * ng:(gi + 1) * ng]
        for _ in range(repeat):
            if biased_running_var:
                rm.mul_(0.9).add_(0.1 * xg.detach().mean(dim=(0, 2, 3)))
                rv.mul_(0.9).add_(0.1 * xg.detach().var(dim=(0, 2, 3), unbiased=False))
                h = F.batch_norm(xg, None, None, gamma, beta, True, 0.1, 1e-5)
            else:
                h = F.batch_norm(xg, rm, rv, gamma, beta, True, 0.1, 1e-5)
        if mask_on_xhat:   # the WRONG activation mask (a negative control): on xhat, not on the affine output
            xh = F.batch_norm(xg, None, None, None, None, True, 0.1, 1e-5)
            d = {0: torch.ones_like(xh), 1: (xh > 0).double(), 2: torch.where(xh > 0, 1.0, 0.2).double()}[c["act"]]
            outs.append(h * d.detach())
        else:
            outs.append(act64(h, c["act"]))
        m = xg.detach().mean(dim=(0, 2, 3))
        means.append(m)
        rstds.append((xg.detach().var(dim=(0, 2, 3), unbiased=False) + 1e-5).rsqrt())
    y = torch.cat(outs)
    if res is not None:
        y = y + res.double()
    gy = dy.double() + (dy2.double() if dy2 is not None else 0.0)
    y.backward(gy)
    return dict(y=y.detach(), dx=x.grad, dgamma=gamma.grad, dbeta=beta.grad, rm=rm, rv=rv,
                mean=torch.stack(means), rstd=torch.stack(rstds))


def run_kernels(ops, c, repeat=1, G=None, x=None, dy=None, dy2=None, res=None, update=True):
    """stats -> apply -> backward through the ops wrappers; everything back on the CPU."""
    G = c["G"] if G is None else G
    x = c["x"] if x is None else x
    dy = c["dy"] if dy is None else dy
    dy2, res = c["dy2"] if dy2 is None else dy2, c["res"] if res is None else res
    N, C, H, W = x.shape
    dt, ld, off = c["dt"], c["ld"], c["off"]
    xd = to_slice(x, dt, ld, off)
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    rm, rv = c["rm0"].to(DEV), c["rv0"].to(DEV)
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    mr = torch.zeros(N * C * ops.BN_TABLE, device=DEV)
    ab = torch.zeros(N * C * 2, device=DEV)
    X = ops.Feat(xd, off, C)
    ops.bn_stats(X, work, mr, G, gamma, beta, rm if update else None, rv if update else None, repeat, ab=ab)
    yd = torch.full((N, H, W, ld), 3.0, device=DEV, dtype=dt)
    rd = to_slice(res, dt, ld, off) if res is not None else None
    ops.bn_apply(X, mr, gamma, beta, ops.Feat(yd, off, C), act=c["act"], res=ops.Feat(rd, off, C) if res is not None else None)
    dyd = to_slice(dy, dt, ld, off)
    d2d = to_slice(dy2, dt, ld, off) if dy2 is not None else None
    dxd = torch.full((N, H, W, ld), 5.0, device=DEV, dtype=dt)
    red = torch.empty(2 * N * C, device=DEV)
    dgamma, dbeta = torch.full((C,), 0.25, device=DEV), torch.full((C,), -0.5, device=DEV)   # accumulated into
    ops.bn_backward(ops.Feat(dyd, off, C), X, c["act"], mr, gamma, beta, work, red, ops.Feat(dxd, off, C),
                    dgamma=dgamma, dbeta=dbeta, groups=G, dy2=ops.Feat(d2d, off, C) if dy2 is not None else None)
    torch.cuda.synchronize()
    t = mr.view(N, C, ops.BN_TABLE).double().cpu()
    outside = torch.cat([yd[..., :off].flatten(), yd[..., off + C:].flatten()])
    assert bool((outside == 3.0).all()), "apply wrote outside its channel slice"
    outside = torch.cat([dxd[..., :off].flatten(), dxd[..., off + C:].flatten()])
    assert bool((outside == 5.0).all()), "backward wrote outside its channel slice"
    return dict(y=from_slice(yd, off, C), dx=from_slice(dxd, off, C), y_raw=yd, dx_raw=dxd, mr_raw=mr.clone(),
                mean=t[..., 0] + t[..., 2], rstd=t[..., 1], rm=rm.double().cpu(), rv=rv.double().cpu(),
                dgamma=(dgamma - 0.25).double().cpu(), dbeta=(dbeta + 0.5).double().cpu(), ab=ab.view(N, C, 2).cpu())


def errors(c, got, ref):
    """Every figure as a fraction of its bound (<= 1 passes)."""
    N, G = c["N"], c["G"]
    ng = N // G
    mean_n, rstd_n = ref["mean"].repeat_interleave(ng, 0), ref["rstd"].repeat_interleave(ng, 0)
    out = {"mean": relerr(got["mean"], mean_n) / 1e-5, "rstd": relerr(got["rstd"], rstd_n) / 1e-5,
           "running_mean": relerr(got["rm"], ref["rm"]) / 1e-5, "running_var": relerr(got["rv"], ref["rv"]) / 1e-5}
    if c["dtype"] == "fp32":
        out.update(y=relerr(got["y"], ref["y"]) / 1e-5, dx=relerr(got["dx"], ref["dx"]) / 1e-4,
                   dgamma=relerr(got["dgamma"], ref["dgamma"]) / 1e-4, dbeta=relerr(got["dbeta"], ref["dbeta"]) / 1e-4)
        return out
    x, ga, be = c["x"].double(), c["gamma"].double()[None, :, None, None], c["beta"].double()[None, :, None, None]
    xh = (x - mean_n[..., None, None]) * rstd_n[..., None, None]
    res = c["res"].double().abs() if c["res"] is not None else 0.0
    out["y"] = bound_ratio(got["y"], ref["y"], (ga * xh).abs() + be.abs() + res, R_BF16, 1e-5)
    gy = c["dy"].double() + (c["dy2"].double() if c["dy2"] is not None else 0.0)
    h = ga * xh + be
    g = gy * {0: torch.ones_like(h), 1: (h > 0).double(), 2: torch.where(h > 0, 1.0, 0.2).double()}[c["act"]]
    gs = [g[i * ng:(i + 1) * ng] for i in range(G)]
    xs = [xh[i * ng:(i + 1) * ng] for i in range(G)]
    mg = torch.stack([a.mean(dim=(0, 2, 3)) for a in gs]).repeat_interleave(ng, 0)[..., None, None]
    mgx = torch.stack([(a * b).mean(dim=(0, 2, 3)) for a, b in zip(gs, xs)]).repeat_interleave(ng, 0)[..., None, None]
    aref = (ga.abs() * rstd_n[..., None, None]) * (g.abs() + mg.abs() + (xh * mgx).abs())
    out["dx"] = bound_ratio(got["dx"], ref["dx"], aref, R_BF16, 1e-5)
    out["dbeta"] = bound_ratio(got["dbeta"], ref["dbeta"], g.abs().sum(dim=(0, 2, 3)), 0.0, 2e-5)
    out["dgamma"] = bound_ratio(got["dgamma"], ref["dgamma"], (g * xh).abs().sum(dim=(0, 2, 3)), 0.0, 2e-5)
    return out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_batch_norm_kernels_vs_fp64(ops, name, dtype):
    """y, {mean, rstd}, running buffers (repeat 1), dx, dgamma, dbeta of every case; then the
    two negative controls: the same dx check against a reference whose activation mask sits on
    xhat, and the same running_var check against a biased-variance reference, must FAIL."""
    c = make_case(name, dtype)
    got, ref = run_kernels(ops, c), reference(c)
    e = errors(c, got, ref)
    print(name, dtype, {k: round(v, 4) for k, v in e.items()})
    assert all(v <= 1.0 for v in e.values()), e
    if c["act"] != 0:
        wrong = errors(c, got, {**ref, **{k: reference(c, mask_on_xhat=True)[k] for k in ("dx", "dgamma", "dbeta")}})
        assert wrong["dx"] > 1.0, ("mask-on-xhat control passed", wrong)
    if CASES[name][-1] >= 1.0:   # (std 0.1: the variance term is too small a share of running_var to tell)
        biased = errors(c, got, {**ref, "rv": reference(c, biased_running_var=True)["rv"]})
        assert biased["running_var"] > 1.0, ("biased running_var control passed", biased)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("repeat", [1, 2])
def test_running_buffers_repeat(ops, dtype, repeat):
    """repeat = k applies one forward's running update k times (group after group, each k
    times); y and the statistics do not depend on it; update switched off leaves the buffers."""
    c = make_case("c24_g2", dtype)
    got, ref = run_kernels(ops, c, repeat=repeat), reference(c, repeat=repeat)
    assert relerr(got["rm"], ref["rm"]) <= 1e-5 and relerr(got["rv"], ref["rv"]) <= 1e-5
    once = run_kernels(ops, c, repeat=1)
    assert torch.equal(got["y_raw"], once["y_raw"]) and torch.equal(got["mr_raw"], once["mr_raw"])
    if repeat == 2:
        assert relerr(once["rm"], ref["rm"]) > 1e-5     # and it is not the single update
    off = run_kernels(ops, c, update=False)
    assert torch.equal(off["rm"], c["rm0"].double()) and torch.equal(off["rv"], c["rv0"].double())
    assert torch.equal(off["y_raw"], once["y_raw"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_group_property(ops, dtype):
    """G = 2 on [a; b] is two G = 1 calls on a and on b: y, the tables and dx bit for bit, the
    running buffers as the two calls in order, dgamma / dbeta their sum within fp32 rounding."""
    c = make_case("c24_g2", dtype)
    both = run_kernels(ops, c, G=2)
    h = c["N"] // 2
    sl = lambda t, i: t[i * h:(i + 1) * h]  # noqa: E731
    halves = []
    for i in (0, 1):
        ci = dict(c)
        if i == 1:   # the second call starts from the first call's running buffers
            ci["rm0"], ci["rv0"] = halves[0]["rm"].float(), halves[0]["rv"].float()
        halves.append(run_kernels(ops, ci, G=1, x=sl(c["x"], i), dy=sl(c["dy"], i)))
    for k in ("y_raw", "dx_raw"):
        assert torch.equal(both[k], torch.cat([halves[0][k], halves[1][k]])), k
    assert torch.equal(both["mr_raw"], torch.cat([halves[0]["mr_raw"], halves[1]["mr_raw"]]))
    assert torch.equal(both["rm"], halves[1]["rm"]) and torch.equal(both["rv"], halves[1]["rv"])
    for k in ("dgamma", "dbeta"):
        a, b = halves[0][k], halves[1][k]
        assert bool(((both[k] - (a + b)).abs() <= 2.0 ** -22 * (a.abs() + b.abs() + 0.75)).all()), k
    # and G = 1 on the whole batch is something else
    assert not torch.equal(run_kernels(ops, c, G=1)["y_raw"], both["y_raw"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["c24_g1", "c12_scalar", "c64_wide"])
def test_eval_mode_apply_and_backward(ops, name, dtype):
    """Eval mode: the same apply kernel fed from the running statistics reproduces
    batch_norm(training=False) and leaves the buffers bit for bit; its backward is
    dx = gamma * rstd * g with the dgamma / dbeta sums."""
    c = make_case(name, dtype)
    N, C, H, W, dt, ld, off = c["N"], c["C"], c["H"], c["W"], c["dt"], c["ld"], c["off"]
    gamma, beta, rm, rv = (c[k].to(DEV) for k in ("gamma", "beta", "rm0", "rv0"))
    rm0, rv0 = rm.clone(), rv.clone()
    mr = torch.zeros(N * C * ops.BN_TABLE, device=DEV)
    ops.bn_eval_table(rm, rv, gamma, beta, N, mr)
    X = ops.Feat(to_slice(c["x"], dt, ld, off), off, C)
    yd = torch.zeros(N, H, W, ld, device=DEV, dtype=dt)
    ops.bn_apply(X, mr, gamma, beta, ops.Feat(yd, off, C), act=c["act"])
    dxd = torch.zeros(N, H, W, ld, device=DEV, dtype=dt)
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    red = torch.empty(2 * N * C, device=DEV)
    dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    ops.bn_backward(ops.Feat(to_slice(c["dy"], dt, ld, off), off, C), X, c["act"], mr, gamma, beta, work, red,
                    ops.Feat(dxd, off, C), dgamma=dgamma, dbeta=dbeta, eval_mode=True)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    x = c["x"].double().requires_grad_(True)
    g64, b64 = c["gamma"].double().requires_grad_(True), c["beta"].double().requires_grad_(True)
    y = act64(F.batch_norm(x, c["rm0"].double(), c["rv0"].double(), g64, b64, False, 0.1, 1e-5), c["act"])
    y.backward(c["dy"].double())
    gy, gdx = from_slice(yd, off, C), from_slice(dxd, off, C)
    if dtype == "fp32":
        assert relerr(gy, y.detach()) <= 1e-5 and relerr(gdx, x.grad) <= 1e-4
        assert relerr(dgamma.cpu(), g64.grad) <= 1e-4 and relerr(dbeta.cpu(), b64.grad) <= 1e-4
    else:
        ga, rstd = c["gamma"].double()[None, :, None, None], (c["rv0"].double() + 1e-5).rsqrt()[None, :, None, None]
        xh = (c["x"].double() - c["rm0"].double()[None, :, None, None]) * rstd
        assert bound_ratio(gy, y.detach(), (ga * xh).abs() + c["beta"].double().abs()[None, :, None, None], R_BF16,
                           1e-5) <= 1.0
        assert bound_ratio(gdx, x.grad, x.grad.abs(), R_BF16, 1e-5) <= 1.0
        assert relerr(dgamma.cpu(), g64.grad) <= 1e-4 and relerr(dbeta.cpu(), b64.grad) <= 1e-4


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("kind", ["down", "up"])
def test_fused_resample_consumers_read_the_shift_scale_table(ops, kind, dtype):
    """ops.blur_down_in / ops.upsample_in with the {shift, scale} table (ops.NORM_AFFINE) against
    the resampled fp64 activations, to the bound the InstanceNorm fused form is held to
    (test_gpu_bf16_elementwise.py::test_resample_in_bf16: r_out |ref| + 1e-5 absref, absref from
    the terms |x * scale| + |shift| the kernel forms).  The channel whose gamma is exactly 0 does
    not depend on x at all: act(beta) resampled, the same bits for another input."""
    c = make_case("c64_wide", dtype)
    c.update(ld=64, off=0)
    N, C, H, W, dt = c["N"], c["C"], c["H"], c["W"], c["dt"]
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    xd = to_slice(c["x"], dt, C, 0)
    X = ops.Feat(xd)
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    mr, ab = torch.zeros(N * C * ops.BN_TABLE, device=DEV), torch.zeros(N * C * 2, device=DEV)
    ops.bn_stats(X, work, mr, 1, gamma, beta, ab=ab)
    Ho, Wo = (H // 2, W // 2) if kind == "down" else (2 * H, 2 * W)
    fused = torch.zeros(N, Ho, Wo, C, device=DEV, dtype=dt)
    fn, plain = (ops.blur_down_in, ops.blur_down) if kind == "down" else (ops.upsample_in, ops.upsample)
    assert fn(X, ab, c["act"] | ops.NORM_AFFINE, ops.Feat(fused)), "the fused consumer refused the shape"
    # the plain resample kernel is linear with non-negative taps: run it on fp32 copies of the
    # exact fp64 activations and of the absolute terms
    r = reference(c)
    sc = c["gamma"].double()[None, :, None, None] * r["rstd"][0][None, :, None, None]
    sh = c["beta"].double()[None, :, None, None] - r["mean"][0][None, :, None, None] * sc
    habs = (c["x"].double() * sc).abs() + sh.abs()
    out, aout = torch.zeros(N, Ho, Wo, C, device=DEV), torch.zeros(N, Ho, Wo, C, device=DEV)
    plain(ops.Feat(to_slice(r["y"].float(), torch.float32, C, 0)), ops.Feat(out))
    plain(ops.Feat(to_slice(habs.float(), torch.float32, C, 0)), ops.Feat(aout))
    r_out = R_BF16 if dtype == "bf16" else 2.0 ** -23
    ratio = bound_ratio(from_slice(fused, 0, C), from_slice(out, 0, C), from_slice(aout, 0, C), r_out, 1e-5)
    print(kind, dtype, "worst |err| / bound", round(ratio, 4))
    assert ratio <= 1.0
    # gamma[1] == 0: another input (other statistics), the same beta -> the same bits in channel 1
    x2 = to_slice((c["x"] * 3 + 1).to(dt).float(), dt, C, 0)
    ops.bn_stats(ops.Feat(x2), work, mr, 1, gamma, beta, ab=ab)
    fused2 = torch.zeros_like(fused)
    assert fn(ops.Feat(x2), ab, c["act"] | ops.NORM_AFFINE, ops.Feat(fused2))
    assert torch.equal(fused[..., 1], fused2[..., 1]) and not torch.equal(fused[..., 0], fused2[..., 0])
    want = act64(c["beta"][1].double(), c["act"])
    assert float((fused[..., 1].double() - want).abs().max()) <= (r_out + 1e-5) * abs(float(want))
