"""The InstanceNorm backward taken from the Downsample adjoint (irgan_sep_resample_in_bwd_reduce /
_apply, sep_pipe_kernel's output-side epilogue; ops.blur_down_bwd_in): the backward of down1 /
down2 without the up-sampled gradient in memory.

Reference of every case, on the same device tensors: today's ``ops.blur_down_bwd`` gives the
bf16 ``da`` (the fused kernels round the adjoint to the same bits before they use it); the rest
is fp64 torch from da, z and the {mean, rstd} table mr:

    xhat = (z - mean) * rstd,  g = da * act'(xhat),  red64 = {mean g, mean g*xhat},
    dz64 = rstd * (g - mg64 - xhat * mgx64)

Bounds (derived from the formats, not measured):

    |red - red64| <= 2^-20 * {mean|g|, mean|g*xhat|}                          per (n, c)
    |dz - dz64|  <= 2^-8 |dz64| + rstd * (dg + |xhat| * dgx)
                    + 2^-22 * rstd * (|g| + |mg64| + |xhat| |mgx64|)              per element

dg / dgx are the red bounds: the bf16 half-ulp of the result, the allowed red error carried
through the formula, and the fp32 evaluation of the three-term expression.  fp32 chains of a
few dozen terms and an fp64 finalize stay far inside 2^-20.  The three launches the fused pair
replaces (blur_down_bwd + in_backward) are held to the same two bounds on the same inputs -- and the
fused pair to their bits (test_fused_equals_three_launches): the reduce sums in the reduce pass's order.

Cases: the smallest shapes that reach each arm of sep_pipe_launch (the table in CASES).
"""
import functools

import pytest
import torch

from conftest import pkg
from oracle import step as O

gpu = pytest.mark.gpu
DEV = "cuda"
SENT = -3.0   # bf16-exact filler of everything a launch must not write
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


# name: (N, Hin, Win, C, (ld - C, off), act)
CASES = {
    # output 68x48: R = 8 with a ragged last row block (68 = 8*8 + 4); CB = 128, ipt 1, opt 2
    "a_ragged_slice": (2, 34, 24, 128, (64, 64), ACT_RELU),
    # output 64x256, the flagship arm: CB = 64 (two channel groups), ipt 2, opt 4
    "b_flagship_arm": (1, 32, 128, 128, (0, 0), ACT_RELU),
    # output 16x32: R = 4, CB = 16, opt 1
    "c_small_lrelu": (2, 8, 16, 16, (0, 0), ACT_LRELU),
    # three images, output 80x48: nb = 10 partials per image
    "d_three_images": (3, 40, 24, 64, (0, 0), ACT_RELU),
}


def nhwc(N, H, W, C, extra, off, gen, scale, shift=0.0, dtype=torch.bfloat16):
    """A [N][H][W][C + extra] tensor filled with SENT whose channels off .. off + C are random."""
    t = torch.full((N, H, W, C + extra), SENT, dtype=dtype)
    t[..., off:off + C] = (torch.randn(N, H, W, C, generator=gen) * scale + shift).to(dtype)
    return t.to(DEV)


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and the fp64 reference of a case, computed once and shared (never modified)."""
    ops = pkg().ops
    N, Hin, Win, C, (extra, off), act = CASES[name]
    H, W = 2 * Hin, 2 * Win
    gen = torch.Generator().manual_seed(11)
    zt = nhwc(N, H, W, C, extra, off, gen, 2.0, 0.5)
    dyt = nhwc(N, Hin, Win, C, extra, off, gen, 0.01)
    z, dy = ops.Feat(zt, off, C), ops.Feat(dyt, off, C)
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    mr = torch.empty(2 * N * C, device=DEV)
    ops.in_stats(z, work, mr)
    da = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=DEV)
    ops.blur_down_bwd(dy, ops.Feat(da))
    m = mr.view(N, 1, 1, C, 2).double()
    mean, rstd = m[..., 0], m[..., 1]
    xh = (zt[..., off:off + C].double() - mean) * rstd
    slope = {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: 0.2}[act]
    g = da.double() * torch.where(xh > 0, 1.0, slope)
    mg, mgx = g.mean(dim=(1, 2), keepdim=True), (g * xh).mean(dim=(1, 2), keepdim=True)
    dg = 2.0 ** -20 * g.abs().mean(dim=(1, 2), keepdim=True)
    dgx = 2.0 ** -20 * (g * xh).abs().mean(dim=(1, 2), keepdim=True)
    dz64 = rstd * (g - mg - xh * mgx)
    bound = (2.0 ** -8 * dz64.abs() + rstd * (dg + xh.abs() * dgx)
             + 2.0 ** -22 * rstd * (g.abs() + mg.abs() + xh.abs() * mgx.abs()))
    torch.cuda.synchronize()
    return dict(z=z, dy=dy, mr=mr, act=act, shape=(N, H, W, C), sl=(extra, off), mg=mg, mgx=mgx, dg=dg, dgx=dgx,
                dz64=dz64, bound=bound)


def check(c, red, dz, what):
    N, H, W, C = c["shape"]
    r = red.view(N, 1, 1, C, 2).double()
    for got, ref, lim, nm in ((r[..., 0], c["mg"], c["dg"], "mean g"), (r[..., 1], c["mgx"], c["dgx"], "mean g*xhat")):
        ratio = ((got - ref).abs() / (lim + 1e-300)).max().item()
        print(f"{what}: {nm}: worst |err| / bound = {ratio:.3g}")
        assert ratio <= 1.0, f"{what}: {nm}: worst |err| / bound = {ratio:.3g}"
    err = (dz.double() - c["dz64"]).abs()
    ratio = (err / (c["bound"] + 1e-300)).max().item()
    print(f"{what}: dz: worst |err| / bound = {ratio:.3g}, max |err| = {err.max().item():.3g}")
    assert ratio <= 1.0, f"{what}: dz: worst |err| / bound = {ratio:.3g}"


def outputs(ops, c):
    N, H, W, C = c["shape"]
    extra, off = c["sl"]
    work = torch.zeros(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    red = torch.full((2 * N * C,), SENT, device=DEV)
    dzt = torch.full((N, H, W, C + extra), SENT, dtype=torch.bfloat16, device=DEV)
    return work, red, dzt, ops.Feat(dzt, off, C)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_matches_fp64(ops, name):
    c = case(name)
    N, H, W, C = c["shape"]
    extra, off = c["sl"]
    work, red, dzt, dz = outputs(ops, c)
    assert ops.blur_down_bwd_in(c["dy"], c["z"], c["act"], c["mr"], work, red, dz), "the library refused the case"
    torch.cuda.synchronize()
    check(c, red, dzt[..., off:off + C], f"fused {name}")
    assert bool((dzt[..., :off] == SENT).all()) and bool((dzt[..., off + C:] == SENT).all()), "wrote outside the slice"
    # run to run: the same bits (no atomics, fixed combine order)
    work2, red2, dzt2, dz2 = outputs(ops, c)
    assert ops.blur_down_bwd_in(c["dy"], c["z"], c["act"], c["mr"], work2, red2, dz2)
    torch.cuda.synchronize()
    assert torch.equal(red, red2) and torch.equal(dzt, dzt2)


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_three_launch_path_meets_the_same_bounds(ops, name):
    """The yardstick is fair: blur_down_bwd + in_backward pass it on the same inputs."""
    c = case(name)
    N, H, W, C = c["shape"]
    extra, off = c["sl"]
    work, red, dzt, dz = outputs(ops, c)
    ops.blur_down_bwd(c["dy"], dz)
    ops.in_backward(dz, c["z"], c["act"], c["mr"], work, red, dz)
    torch.cuda.synchronize()
    check(c, red, dzt[..., off:off + C], f"three launches {name}")


@gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_equals_three_launches(ops, name):
    """By construction, not by tolerance: the reduce forms the adjoint's bf16 values per pixel in
    the plain launch's operation order and sums them in the reduce pass's chains, blocks and
    finalize, the apply evaluates irgan_in_bwd_apply's expression -- so red and dz are the bits
    of blur_down_bwd + in_backward, and a step computes what it computed before."""
    c = case(name)
    work, red, dzt, dz = outputs(ops, c)
    assert ops.blur_down_bwd_in(c["dy"], c["z"], c["act"], c["mr"], work, red, dz)
    work2, red2, dzt2, dz2 = outputs(ops, c)
    ops.blur_down_bwd(c["dy"], dz2)
    r, a = ops.in_bwd_parts(dz2, c["z"], c["act"], c["mr"], work2, red2, dz2)
    r()
    a()
    torch.cuda.synchronize()
    assert torch.equal(red, red2), f"red differs: max {float((red - red2).abs().max()):.3g}"
    assert torch.equal(dzt, dzt2), "dz differs"


@gpu
def test_no_activation(ops):
    """act = none on the smallest case's inputs (the derivative is 1 everywhere)."""
    c = dict(case("c_small_lrelu"))
    N, H, W, C = c["shape"]
    m = c["mr"].view(N, 1, 1, C, 2).double()
    rstd = m[..., 1]
    xh = (c["z"].t.double() - m[..., 0]) * rstd
    da = torch.empty(N, H, W, C, dtype=torch.bfloat16, device=DEV)
    ops.blur_down_bwd(c["dy"], ops.Feat(da))
    g = da.double()
    c["mg"], c["mgx"] = g.mean(dim=(1, 2), keepdim=True), (g * xh).mean(dim=(1, 2), keepdim=True)
    c["dg"] = 2.0 ** -20 * g.abs().mean(dim=(1, 2), keepdim=True)
    c["dgx"] = 2.0 ** -20 * (g * xh).abs().mean(dim=(1, 2), keepdim=True)
    c["dz64"] = rstd * (g - c["mg"] - xh * c["mgx"])
    c["bound"] = (2.0 ** -8 * c["dz64"].abs() + rstd * (c["dg"] + xh.abs() * c["dgx"])
                  + 2.0 ** -22 * rstd * (g.abs() + c["mg"].abs() + xh.abs() * c["mgx"].abs()))
    work, red, dzt, dz = outputs(ops, c)
    assert ops.blur_down_bwd_in(c["dy"], c["z"], ACT_NONE, c["mr"], work, red, dz)
    torch.cuda.synchronize()
    check(c, red, dzt, "fused, no activation")


def _refusal_args(ops, N, Hin, Win, C, extra, off, dtype):
    gen = torch.Generator().manual_seed(5)
    zt = nhwc(N, 2 * Hin, 2 * Win, C, extra, off, gen, 2.0, 0.5, dtype)
    dyt = nhwc(N, Hin, Win, C, extra, off, gen, 0.01, dtype=dtype)
    z, dy = ops.Feat(zt, off, C), ops.Feat(dyt, off, C)
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    mr = torch.empty(2 * N * C, device=DEV)
    ops.in_stats(z, work, mr)
    red = torch.full((2 * N * C,), SENT, device=DEV)
    dzt = torch.full((N, 2 * Hin, 2 * Win, C + extra), SENT, dtype=dtype, device=DEV)
    return dy, z, mr, work, red, dzt


@gpu
@pytest.mark.parametrize("what", ["fp32", "c12", "ld_not_8"])
def test_refusals_write_nothing(ops, what):
    C, extra, dtype = {"fp32": (16, 0, torch.float32), "c12": (12, 0, torch.bfloat16),
                       "ld_not_8": (16, 4, torch.bfloat16)}[what]
    dy, z, mr, work, red, dzt = _refusal_args(ops, 2, 8, 16, C, extra, 0, dtype)
    work.fill_(SENT)
    assert ops.blur_down_bwd_in(dy, z, ACT_RELU, mr, work, red, ops.Feat(dzt, 0, C)) is False
    torch.cuda.synchronize()
    assert bool((dzt == SENT).all()) and bool((red == SENT).all()) and bool((work == SENT).all())


@gpu
def test_refuses_dz_aliasing_z(ops):
    dy, z, mr, work, red, _ = _refusal_args(ops, 2, 8, 16, 16, 0, 0, torch.bfloat16)
    before = z.t.clone()
    work.fill_(SENT)
    assert ops.blur_down_bwd_in(dy, z, ACT_RELU, mr, work, red, ops.Feat(z.t, 0, 16)) is False
    torch.cuda.synchronize()
    assert torch.equal(z.t, before) and bool((red == SENT).all()) and bool((work == SENT).all())


# ---- engine level -------------------------------------------------------------------------

def _one_step(fused):
    """G's gradient after one bf16 GANStep at 64x64, B = 2, from the seeded state."""
    irc = pkg()
    old = irc.ops.set_resample_bwd_fused(fused)
    try:
        cfg = irc.Config()
        cfg.device = DEV
        cfg.compute_dtype = "bf16"
        tr = irc.GANTrainer(cfg)
        tr.netG.store.load(O.seeded_params(O.g_param_shapes(), 1, bias_std=0.02), strict=True)
        tr.netD.store.load(O.seeded_params(O.d_param_shapes(), 2, bias_std=0.02), strict=True)
        tr.vgg.store.load(O.seeded_params(O.vgg_param_shapes(), 3, kaiming=True), strict=True)
        for m in (tr.netG, tr.netD, tr.vgg):
            m.repack()
        g = torch.Generator().manual_seed(23)
        ir = (torch.rand(2, 1, 64, 64, generator=g) * 2 - 1).to(DEV)
        rgb = (torch.rand(2, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
        tr.step(ir, rgb)
        torch.cuda.synchronize()
        st = tr.netG.store
        return st.grad.clone(), {k: st.oihw(k, st.grad).double().clone() for k in ("inc.1.weight", "down1.0.weight")}
    finally:
        irc.ops.set_resample_bwd_fused(old)


@gpu
def test_step_gradients_switch_on_off():
    """inc.1 and down1.0 sit behind both fused layers: their gradients with the fused backward
    and with the three launches, from the same state, within rel-L2 1e-3 (bf16 gradients carry
    about 2^-9 per element) -- and, the kernels being bit-equal, the same bits; the fused step
    twice in deterministic mode: bit-equal store.grad."""
    ops = pkg().ops
    old = ops.set_deterministic(True)
    try:
        flat_a, on = _one_step(True)
        flat_b, _ = _one_step(True)
        _, off = _one_step(False)
    finally:
        ops.set_deterministic(old)
    assert torch.equal(flat_a, flat_b), "the fused backward is not reproducible run to run"
    for k in on:
        assert torch.equal(on[k], off[k]), f"{k}: the fused backward changes the gradient's bits"
        d = ((on[k] - off[k]).norm() / off[k].norm()).item()
        print(f"{k}: rel-L2(fused, three launches) = {d:.3g}")
        assert d <= 1e-3, (k, d)
