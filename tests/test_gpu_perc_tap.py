"""The two kernels of Config.perc_layers against fp64 from the same operands.

``ops.l1_tap`` (irgan_l1_tap): dz = (accumulate ? dz : 0) + (a > 0 ? sgn(a - b) * w / count : 0),
loss += w * mean|a - b|.  Operands bf16 and fp32, dz bf16 and fp32, accumulate 0 and 1; the 16-byte
kernel on aligned tensors and the scalar one on views one element into their storage.  count =
512 * 256 * 8 + 296 gives both kernels' grid-stride loops (512 blocks) a second, ragged round.
Every 97th element is an exact tie (a == b) and about half are a == 0: there dz must be exactly
what it held (or 0 without accumulate).

``ops.maxpool_bwd_tap`` (irgan_maxpool_bwd_tap): dx[q] = (argmax == q && max > 0 ? dy : 0) +
(x[q] > 0 ? sgn(x[q] - xr[q]) * w / count : 0), loss += w * mean|x - xr|.  One case per arm, N = 2,
H = 4, W/2 one more than the pooled pixels a block covers (a ragged last block):
  bf16 C = 64 / 128 / 256   the whole-row kernel, 16 / 8 / 4 pooled pixels per block
  bf16 C = 24, fp32 C = 16  the 8-channel kernel, 85 1/3 / 128 pooled pixels per block
  fp32 C = 3                the one-channel kernel, 85 1/3 pooled pixels per block
Three more cases at H = 2052 (one per kernel) make the blocks stride over the pooled rows.
x is a ReLU output (about half zeros, so all-zero windows occur) with planted tied maxima, windows
forced non-positive (zeros and negatives) and x == xr elements.

Bounds: an fp32 dz / dx within 1e-6 * max|ref| of fp64 (one fp32 division and one add); a bf16 one
within one bf16 ulp of the fp64 value per element (the fp32 sum is rounded once); the loss within
loss_cases.R_ACC relative, the bound ops.l1 is held to.
"""
import pytest
import torch

import loss_cases as LC
from conftest import pkg

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = {"f32": torch.float32, "bf16": torch.bfloat16}
LOSS0 = LC.LOSS0
W_TAP = 15.0
L1_COUNT = 512 * 256 * 8 + 296


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


def loss_word():
    return torch.full((1,), LOSS0, dtype=torch.float64, device=DEV)


def rounded(t, dt):
    return t.to(T[dt]).float()


def bf16_ulp(ref):
    """One bf16 ulp at each fp64 value (8 significant bits); tiny at 0, where the result is exact."""
    mag = ref.abs().clamp_min(1e-300)
    return torch.where(ref == 0, torch.full_like(ref, 1e-30), torch.exp2(torch.floor(torch.log2(mag)) - 7))


def check_grad(got, want, gdt, what):
    got = got.double().cpu()
    err = (got - want).abs()
    if gdt == "f32":
        bound = 1e-6 * want.abs().max().item()
        print(f"TAP {what}: max err {err.max().item():.3g}, bound {bound:.3g}")
        assert err.max().item() <= bound
    else:
        ratio = (err / bf16_ulp(want)).max().item()
        print(f"TAP {what}: max err / bf16 ulp {ratio:.3g}")
        assert ratio <= 1.0


def check_loss(loss, ref, what):
    lerr = abs(loss.item() - LOSS0 - ref)
    print(f"TAP {what}: loss err / bound {lerr / (LC.R_ACC * ref):.3g}")
    assert lerr <= LC.R_ACC * ref


def tap_term(a, b, w):
    """(a > 0 ? sgn(a - b) * w / count : 0) in fp64."""
    a, b = a.double(), b.double()
    return torch.where(a > 0, torch.sign(a - b), torch.zeros_like(a)) * (w / a.numel())


# ----------------------------------------------------------------------------
# l1_tap
# ----------------------------------------------------------------------------

def placed(t, dtype, aligned):
    """t on the device as ``dtype``: a fresh tensor, or a view one element into its storage."""
    if aligned:
        v = t.to(DEV, dtype).contiguous()
        assert v.data_ptr() % 16 == 0
        return v
    buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)
    buf[1:] = t.to(DEV, dtype)
    v = buf[1:]
    assert v.data_ptr() % 16 != 0 and v.numel() % 8 == 0
    return v


@pytest.mark.parametrize("aligned", [True, False], ids=["vec", "scalar"])
@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "acc"])
@pytest.mark.parametrize("gdt", ["f32", "bf16"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_l1_tap_vs_fp64(ops, dt, gdt, accumulate, aligned):
    gen = torch.Generator().manual_seed(41)
    a = rounded(torch.relu(torch.randn(L1_COUNT, generator=gen)), dt)
    b = rounded(torch.relu(torch.randn(L1_COUNT, generator=gen)), dt)
    b[::97] = a[::97]   # exact ties
    tie = (a == b) | (a == 0)
    assert (a == 0).sum() > L1_COUNT // 4 and ((a == b) & (a > 0)).sum() > 1000
    dz0 = rounded(torch.randn(L1_COUNT, generator=gen) * (W_TAP / L1_COUNT), gdt)
    dz = placed(dz0, T[gdt], aligned)
    loss = loss_word()
    ops.l1_tap(placed(a, T[dt], aligned), placed(b, T[dt], aligned), W_TAP, dz, loss, accumulate=accumulate)
    want = tap_term(a, b, W_TAP) + (dz0.double() if accumulate else 0.0)
    what = f"l1_tap {dt}->{gdt} acc={int(accumulate)} {'vec' if aligned else 'scalar'}"
    check_grad(dz, want, gdt, what)
    held = dz0 if accumulate else torch.zeros_like(dz0)
    assert torch.equal(dz.float().cpu()[tie], held[tie])   # no tap at a tie or at a == 0: exactly what it held
    check_loss(loss, (a.double() - b.double()).abs().mean().item() * W_TAP, what)


# ----------------------------------------------------------------------------
# maxpool_bwd_tap
# ----------------------------------------------------------------------------

# (dtype, C, W/2): W/2 = pooled pixels per block + 1 (rounded up where a block ends inside a pixel)
POOL_CASES = [("bf16", 64, 17), ("bf16", 128, 9), ("bf16", 256, 5), ("bf16", 24, 86), ("f32", 16, 129),
              ("f32", 3, 86)]
POOL_IDS = [f"{dt}-C{C}" for dt, C, _ in POOL_CASES]
N, H = 2, 4


def pool_inputs(dt, C, Wo, seed=43, H=H):
    """x, xr, dy (NHWC, CPU fp32 holding dtype-exact values)."""
    gen = torch.Generator().manual_seed(seed)
    Wd = 2 * Wo
    x = torch.relu(torch.randn(N, H, Wd, C, generator=gen))
    xr = torch.relu(torch.randn(N, H, Wd, C, generator=gen))
    x, xr = rounded(x, dt), rounded(xr, dt)
    win = x.view(N, H // 2, 2, Wo, 2, C)   # [n][i][a][j][b][c], a view
    # tied maxima: pooled columns j % 3 == 0 hold one positive value at (0, 1) and (1, 0)
    win[:, :, 0, 0::3, 1, :] = 3.0
    win[:, :, 1, 0::3, 0, :] = 3.0
    # non-positive windows: pooled columns j % 5 == 1 are zeros with one negative value
    win[:, :, :, 1::5, :, :] = 0.0
    win[:, :, 1, 1::5, 1, :] = -1.0
    flat = x.view(-1)
    xr.view(-1)[::7] = flat[::7]           # x == xr elements
    dy = rounded(torch.randn(N, H // 2, Wo, C, generator=gen) * (W_TAP / x.numel()), dt)
    return x, xr, dy


def pool_reference(x, xr, dy, w):
    """fp64: the gradient routed to the first maximum of each window where it is positive, plus
    the tap."""
    n, h, wd, c = x.shape
    v = x.double().view(n, h // 2, 2, wd // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, wd // 2, c, 4)
    m = v.max(-1, keepdim=True).values
    eq = v == m
    first = eq & (eq.cumsum(-1) == 1)
    routed = torch.where(first & (m > 0), dy.double().unsqueeze(-1), torch.zeros_like(v))
    routed = routed.view(n, h // 2, wd // 2, c, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(n, h, wd, c)
    return routed + tap_term(x, xr, w)


def dev(t, dt):
    return pkg().ops.Feat(t.to(DEV, T[dt]).contiguous())


def run_fused(ops, x, xr, dy, dt):
    dx = dev(torch.full_like(x, float("nan")), dt)
    loss = loss_word()
    assert ops.maxpool_bwd_tap(dev(x, dt), dev(xr, dt), dev(dy, dt), dx, W_TAP, loss)
    return dx.t, loss


@pytest.mark.parametrize("dt,C,Wo", POOL_CASES, ids=POOL_IDS)
def test_maxpool_bwd_tap_vs_fp64(ops, dt, C, Wo):
    x, xr, dy = pool_inputs(dt, C, Wo)
    dx, loss = run_fused(ops, x, xr, dy, dt)
    what = f"maxpool_bwd_tap {dt} C={C} W={2 * Wo}"
    check_grad(dx, pool_reference(x, xr, dy, W_TAP), dt, what)
    check_loss(loss, (x.double() - xr.double()).abs().mean().item() * W_TAP, what)


@pytest.mark.parametrize("dt,C,Wo", POOL_CASES, ids=POOL_IDS)
def test_fused_equals_maxpool_bwd_then_l1_tap(ops, dt, C, Wo):
    x, xr, dy = pool_inputs(dt, C, Wo)
    dx, loss = run_fused(ops, x, xr, dy, dt)
    xd, rd = dev(x, dt), dev(xr, dt)
    dx2 = dev(torch.full_like(x, float("nan")), dt)
    loss2 = loss_word()
    ops.maxpool_bwd(xd, dev(dy, dt), dx2, relu_mask=True)
    ops.l1_tap(xd.t, rd.t, W_TAP, dx2.t, loss2, accumulate=True)
    assert torch.equal(dx.view(torch.int16 if dt == "bf16" else torch.int32),
                       dx2.t.view(torch.int16 if dt == "bf16" else torch.int32))
    ref = (x.double() - xr.double()).abs().mean().item() * W_TAP
    assert abs(loss.item() - loss2.item()) <= LC.R_ACC * ref


@pytest.mark.parametrize("dt,C,Wo", [POOL_CASES[0], POOL_CASES[4], POOL_CASES[5]],
                         ids=[POOL_IDS[0], POOL_IDS[4], POOL_IDS[5]])
def test_tall_map_blocks_stride_over_the_pooled_rows(ops, dt, C, Wo):
    """H = 2052: N * H / 2 = 2052 pooled rows against the 1024 block rows the launcher gives a
    two-block-wide grid, so every block takes a second row and four of them a third.  One case per
    kernel; dx against the unfused pair bit for bit (held to fp64 above), the loss against fp64."""
    x, xr, dy = pool_inputs(dt, C, Wo, H=2052)
    xd, rd, gd = dev(x, dt), dev(xr, dt), dev(dy, dt)
    dx, dx2 = dev(torch.full_like(x, float("nan")), dt), dev(torch.full_like(x, float("nan")), dt)
    loss, loss2 = loss_word(), loss_word()
    assert ops.maxpool_bwd_tap(xd, rd, gd, dx, W_TAP, loss)
    ops.maxpool_bwd(xd, gd, dx2, relu_mask=True)
    ops.l1_tap(xd.t, rd.t, W_TAP, dx2.t, loss2, accumulate=True)
    assert torch.equal(dx.t, dx2.t) and torch.isfinite(dx.t).all()
    check_loss(loss, (x.double() - xr.double()).abs().mean().item() * W_TAP, f"tall {dt} C={C}")


@pytest.mark.parametrize("dt,C,Wo", POOL_CASES, ids=POOL_IDS)
def test_without_a_difference_the_tap_vanishes(ops, dt, C, Wo):
    """Negative control: xr = x leaves irgan_maxpool_bwd's result, bit for bit, and no loss; the
    tapped result is another one."""
    x, xr, dy = pool_inputs(dt, C, Wo)
    tapped, _ = run_fused(ops, x, xr, dy, dt)
    plain, loss = run_fused(ops, x, x, dy, dt)
    dx2 = dev(torch.full_like(x, float("nan")), dt)
    ops.maxpool_bwd(dev(x, dt), dev(dy, dt), dx2, relu_mask=True)
    assert torch.equal(plain, dx2.t)
    assert loss.item() == LOSS0
    assert not torch.equal(plain, tapped)
    assert (plain != tapped).float().mean().item() > 0.2   # most x > 0 elements carry a tap


@pytest.mark.parametrize("hw", [(5, 34), (4, 35)], ids=["odd-H", "odd-W"])
def test_odd_sides_are_refused_and_nothing_runs(ops, hw):
    h, wd = hw
    gen = torch.Generator().manual_seed(5)
    x = torch.relu(torch.randn(N, h, wd, 64, generator=gen))
    xr = torch.relu(torch.randn(N, h, wd, 64, generator=gen))
    dy = torch.randn(N, h // 2, wd // 2, 64, generator=gen)
    for dt in ("bf16", "f32"):
        dx = dev(torch.full_like(x, 7.0), dt)
        loss = loss_word()
        assert ops.maxpool_bwd_tap(dev(x, dt), dev(xr, dt), dev(dy, dt), dx, W_TAP, loss) is False
        torch.cuda.synchronize()
        assert (dx.t == 7.0).all() and loss.item() == LOSS0
