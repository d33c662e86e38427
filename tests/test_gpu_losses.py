"""Tight parity for the kernels of csrc/loss.hip beyond one block: ragged, wide, non-square.

Companion of test_gpu_bf16_parity.py / test_gpu_bf16_elementwise.py for the loss and Adam
kernels.  Every case runs the HIP kernel through ``ops`` on fp32 NHWC operands and compares
with an fp64 CPU reference of the same operation on the same values (oracle.step with
autograd for TV and SSIM).  Every loss case pre-fills g with non-zero values (the kernels do
``g +=``) and the fp64 loss word with LOSS0 (they add to it atomically), and uses a weight
that is not 1.  SSIM work buffers start as NaN, so a read of a map element that no kernel
wrote shows.

What each case reaches (names as in csrc/loss.hip):

SSIM, ``ops.ssim`` vs ``O.ssim_loss((x + 1) / 2)``; shapes are (N, H, W, C), window
  two_xblocks_ragged_rows (2, 21, 100, 3), 11   W*C = 300: blockIdx.x = 1 of ssim_vfused_kernel
                                   and the second ``e += TPB`` pass of both ssim_hrow_kernel loops;
                                   H % VR = 5: the ragged row block and ``if (y0 + r >= H) break``.
                                   Planted: a == b == const (s11 + s22 + C2 at its minimum) across
                                   e = 256 and into the ragged rows, and a patch where only a is const
  two_xblocks_plain    same shape, no patches: the same paths at the E32 of random images
  widest_lds_row       (1, 9, 1820, 3), 11      W*C = 5460, the widest row ssim_hrow_kernel takes
                                   (65,520 B of dynamic LDS, 22 passes of its loops)
  global_fallback      (1, 12, 1824, 3), 11     W*C = 5472: ssim_h5_kernel / ssim_h_kernel, x-grid
                                   of 8 blocks with a ragged last one (``if (xw >= W) return``)
  all_border_w15/_w13  (2, 5, 40, 3), 15 / 13   H < K/2 and H < VR: every row is border in the
                                   vertical pass, one ragged row block per image
  window1 / window9    (2, 9, 40, 3), 1 / 9     the remaining ssim_launch<K> instances
  c1_odd_batch         (3, 17, 300, 1), 11      C = 1 (``e / C``), hb = 3 row blocks per image with
                                   a ragged last: ``blockIdx.y / hb`` at odd N
  batch split          the N = 2 launch at w == two N = 1 launches at w / 2, bit for bit in g
                       (-w / (float)S and all after it are the same bits), loss words sum to 1e-12
  refusal              N*H = 65536 > 65535 (the y-grid limit): raises, g and loss untouched
  Bound: |got - g64| <= 4 * E32 per element, E32 = max |g32 - g64| of the fp32 oracle
  (tests/loss_cases.py; self-checked without a device in test_losses_bound_cpu.py);
  loss word within 2e-5 * l64.

TV, ``ops.tv`` vs ``O.tv_loss``
  (3, 200, 37, 3)   N*H = 600 > 512: rows 512..599 are the second ``row += gridDim.x`` round of
                    tv_kernel, in another image (``row % H``) than the same blocks' first rows
  (1, 4, 300, 3)    W > 256: the second ``xw += TPB`` pass
  (2, 1, 50, 3)     H = 1: inv_v = 0, neither vertical branch is taken
  (2, 50, 1, 3)     W = 1: inv_h = 0, neither horizontal branch is taken
  (2, 33, 20, 1)    C = 1
  Constant patches give exact ties d == 0 (sgn(0) = 0 == torch's abs'(0)).
  Bound per element: 8 * 2^-24 * (w * (2 inv_v + 2 inv_h) + |g0|), eight fp32 roundings (two
  reciprocals, three adds, w, the scale by w, the add into g); loss within 2e-5 * ref.

Hinge, ``ops.hinge`` vs fp64 autograd
  mode 0, n_half = 70001   2n = 140002 > 512 * 256: a second grid-stride round of hinge_kernel;
                           the real / fake boundary ``i < n`` falls inside a wave (70001 % 64 = 49)
  mode 1, n = 140003
  scale = 0.37, values planted at exactly +1 and -1 (relu'(0) = 0).  Gradient: a constant per
  branch, within 4 * 2^-24 relative; loss within 2e-5 * absref.

L1, ``ops.l1`` on views one element into their storage, count % 8 == 0: the alignment test of
  irgan_l1 alone selects l1_kernel<..., false>; count = 512 * 256 + 296 gives its grid-stride loop
  a second, ragged round.  fp32 and bf16 operands, fp32 and bf16 ga, accumulate into a bf16 ga.
  Bounds of test_l1_bf16_features_tight.

Adam, n = 8192 * 256 * 4 + 1001: a second, ragged round of the grid-stride loop of the 16-byte kernel
  these aligned tensors take (the one-element-per-lane kernel's: tests/test_gpu_ema.py).  Three steps
  of ``ops.adam`` and of ``ops.adam_prep`` + ``ops.adam_dev`` vs torch.optim.Adam on the CPU (5e-7 on
  p); m and v equal between the variants; the device step count is 3; prm within one fp32 ulp of the
  host's fp64 formula.

The worst err / bound of every case on the MI355X is recorded in profiles/loss_parity.txt.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC
from conftest import pkg
from oracle import step as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24      # one fp32 rounding (half an ulp, relative)
R_BF16 = 2.0 ** -8
LOSS0 = LC.LOSS0


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


def loss_word():
    return torch.full((1,), LOSS0, dtype=torch.float64, device=DEV)


def report(what, **figs):
    print("PARITY " + what + ": " + ", ".join(f"{k} = {v:.3g}" for k, v in figs.items()))


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound (fp64 on the CPU)."""
    err = (got.double().cpu() - ref).abs()
    return (err / bound).max().item()


# ----------------------------------------------------------------------------
# SSIM
# ----------------------------------------------------------------------------

def run_ssim(ops, a, b, g0, window, w):
    """ops.ssim on CPU NHWC tensors -> (loss word, g), both on the CPU."""
    ad, bd, g = a.to(DEV), b.to(DEV), g0.clone().to(DEV)
    loss = loss_word()
    work = torch.full((10 * a.numel(),), float("nan"), device=DEV)
    ops.ssim(ops.Feat(ad), ops.Feat(bd), w, g, loss, work, window)
    return loss.item(), g.cpu()


@pytest.mark.parametrize("name", list(LC.SSIM_CASES))
def test_ssim_vs_fp64_oracle(ops, name):
    a, b, g0 = LC.ssim_inputs(name)
    _, window = LC.SSIM_CASES[name]
    l64, g64, e32 = LC.ssim_reference(name)
    loss, g = run_ssim(ops, a, b, g0, window, LC.SSIM_W)
    ratio = LC.worst_ratio(g, name)
    lerr = abs(loss - LOSS0 - l64)
    report(f"ssim {name}", err_over_E32=ratio, margin=LC.MARGIN, E32_over_max_g=e32 / g64.abs().max().item(),
           loss_err_over_bound=lerr / (LC.R_ACC * l64))
    assert torch.isfinite(g).all()
    assert ratio <= LC.MARGIN
    assert lerr <= LC.R_ACC * l64


def test_ssim_batch_launch_equals_per_image_launches(ops):
    name = "two_xblocks_ragged_rows"
    a, b, g0 = LC.ssim_inputs(name)
    _, window = LC.SSIM_CASES[name]
    w = LC.SSIM_W
    lb, gb = run_ssim(ops, a, b, g0, window, w)
    per = [run_ssim(ops, a[i:i + 1].contiguous(), b[i:i + 1].contiguous(), g0[i:i + 1].contiguous(), window, w / 2)
           for i in range(2)]
    assert torch.equal(gb, torch.cat([g for _, g in per]))
    split, batch = sum(l - LOSS0 for l, _ in per), lb - LOSS0
    report("ssim batch split", loss_rel_diff=abs(split - batch) / batch)
    assert abs(split - batch) <= 1e-12 * batch


def test_ssim_refuses_more_rows_than_the_y_grid(ops):
    N, H, W, C = 1, 65536, 1, 1
    gen = torch.Generator().manual_seed(77)
    a = (torch.rand(N, H, W, C, generator=gen) * 2 - 1).to(DEV)
    b = (torch.rand(N, H, W, C, generator=gen) * 2 - 1).to(DEV)
    g0 = torch.randn(N, H, W, C, generator=gen).to(DEV)
    g, loss = g0.clone(), loss_word()
    work = torch.zeros(10 * a.numel(), device=DEV)
    with pytest.raises(Exception):
        ops.ssim(ops.Feat(a), ops.Feat(b), LC.SSIM_W, g, loss, work)
    torch.cuda.synchronize()
    assert torch.equal(g, g0) and loss.item() == LOSS0


# ----------------------------------------------------------------------------
# TV
# ----------------------------------------------------------------------------

TV_W = 0.3
TV_CASES = [(3, 200, 37, 3), (1, 4, 300, 3), (2, 1, 50, 3), (2, 50, 1, 3), (2, 33, 20, 1)]


def tv_reference(x):
    """O.tv_loss; where an axis has one sample its term has no elements (the oracle's mean over
    nothing is NaN) and the loss is the other term of the same expression."""
    H, W = x.shape[2:]
    if H > 1 and W > 1:
        return O.tv_loss(x)
    if H > 1:
        return (x[:, :, 1:, :] - x[:, :, :-1, :]).abs().mean()
    return (x[:, :, :, 1:] - x[:, :, :, :-1]).abs().mean()


@pytest.mark.parametrize("shape", TV_CASES, ids=lambda s: "x".join(map(str, s)))
def test_tv_vs_fp64_oracle(ops, shape):
    N, H, W, C = shape
    gen = torch.Generator().manual_seed(N * 1000 + H + W)
    x = torch.rand(N, H, W, C, generator=gen) * 2 - 1
    # constant patches: exact ties d == 0 in both directions, one of them across the last rows
    # of image 0 / the last columns
    x[0, H // 4:H // 4 + 5, W // 4:W // 4 + 6, :] = 0.25
    x[N - 1, max(H - 3, 0):, max(W - 4, 0):, :] = -0.5
    inv_v = 1.0 / (N * C * (H - 1) * W) if H > 1 else 0.0
    inv_h = 1.0 / (N * C * H * (W - 1)) if W > 1 else 0.0
    g0 = torch.randn(N, H, W, C, generator=gen) * (TV_W * (inv_v + inv_h))
    g0[g0 == 0] = TV_W * (inv_v + inv_h)

    x64 = x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    ref = tv_reference(x64) * TV_W
    ref.backward()
    gref = x64.grad.permute(0, 2, 3, 1) + g0.double()
    assert H == 1 or (x[:, 1:] == x[:, :-1]).any(), "no exact vertical tie planted"
    assert W == 1 or (x[:, :, 1:] == x[:, :, :-1]).any(), "no exact horizontal tie planted"

    g, loss = g0.clone().to(DEV), loss_word()
    ops.tv(ops.Feat(x.to(DEV)), TV_W, g, loss)
    bound = 8 * U * (TV_W * (2 * inv_v + 2 * inv_h) + g0.double().abs())
    ratio = worst(g, gref, bound)
    lerr = abs(loss.item() - LOSS0 - ref.item())
    report(f"tv {shape}", grad_err_over_bound=ratio, loss_err_over_bound=lerr / (LC.R_ACC * ref.item()))
    assert ratio <= 1.0
    assert lerr <= LC.R_ACC * ref.item()


# ----------------------------------------------------------------------------
# hinge
# ----------------------------------------------------------------------------

HINGE_SCALE = 0.37


def hinge_pred(n, gen):
    p = torch.randn(n, generator=gen) * 1.5
    at = torch.randperm(n, generator=gen)[:200]
    p[at[:100]] = 1.0
    p[at[100:]] = -1.0
    p[0], p[n - 1] = 1.0, -1.0
    return p


def run_hinge(ops, p, n_half, mode):
    pd = p.to(DEV)
    grad = torch.randn(p.numel(), generator=torch.Generator().manual_seed(3)).to(DEV) + 2.0   # overwritten
    loss = loss_word()
    ops.hinge(pd, n_half, mode, HINGE_SCALE, grad, loss)
    return loss.item() - LOSS0, grad


def test_hinge_d_loss_second_round_and_boundary_inside_a_wave(ops):
    n = 70001
    assert 2 * n > 512 * 256 and n % 64 != 0
    gen = torch.Generator().manual_seed(21)
    p = torch.cat([hinge_pred(n, gen), hinge_pred(n, gen)])
    p64 = p.double().requires_grad_(True)
    ref = 0.5 * (F.relu(1 - p64[:n]).mean() + F.relu(1 + p64[n:]).mean()) * HINGE_SCALE
    ref.backward()
    loss, grad = run_hinge(ops, p, n, 0)
    gref = p64.grad
    assert (gref[:n][p[:n] == 1.0] == 0).all() and (gref[n:][p[n:] == -1.0] == 0).all()
    ratio = worst(grad, gref, 4 * U * gref.abs() + 1e-300)
    lerr = abs(loss - ref.item())
    report("hinge mode 0", grad_err_over_bound=ratio, loss_err_over_bound=lerr / (LC.R_ACC * ref.item()))
    assert ratio <= 1.0
    assert lerr <= LC.R_ACC * ref.item()   # the terms are non-negative: absref == ref


def test_hinge_g_loss_second_round(ops):
    n = 140003
    p = hinge_pred(n, torch.Generator().manual_seed(22))
    p64 = p.double().requires_grad_(True)
    ref = -p64.mean() * HINGE_SCALE
    ref.backward()
    absref = HINGE_SCALE * p.double().abs().mean().item()
    loss, grad = run_hinge(ops, p, n, 1)
    ratio = worst(grad, p64.grad, 4 * U * p64.grad.abs())
    lerr = abs(loss - ref.item())
    report("hinge mode 1", grad_err_over_bound=ratio, loss_err_over_bound=lerr / (LC.R_ACC * absref))
    assert ratio <= 1.0
    assert lerr <= LC.R_ACC * absref


# ----------------------------------------------------------------------------
# L1: the scalar path chosen by alignment
# ----------------------------------------------------------------------------

L1_COUNT = 512 * 256 + 296
L1_W = 30.0


def shifted(t, dtype):
    """A device view of t that starts one element into its storage."""
    buf = torch.zeros(t.numel() + 1, dtype=dtype, device=DEV)
    buf[1:] = t.to(DEV, dtype)
    v = buf[1:]
    assert v.data_ptr() % 16 != 0 and v.numel() % 8 == 0
    return v


@pytest.mark.parametrize("dt,gdt,accumulate", [("f32", "f32", False), ("bf16", "bf16", True), ("bf16", "bf16", False),
                                               ("f32", "bf16", True), ("bf16", "f32", False)])
def test_l1_misaligned_views_take_the_scalar_kernel(ops, dt, gdt, accumulate):
    T = {"f32": torch.float32, "bf16": torch.bfloat16}
    gen = torch.Generator().manual_seed(31)
    rnd = lambda: torch.randn(L1_COUNT, generator=gen)   # noqa: E731
    a, b = rnd(), rnd()
    if dt == "bf16":
        a, b = a.bfloat16().float(), b.bfloat16().float()
    b[::97] = a[::97]   # exact ties
    ga0 = (rnd() * (L1_W / L1_COUNT)).to(T[gdt]).float()
    ga = shifted(ga0, T[gdt])
    loss = loss_word()
    ops.l1(shifted(a, T[dt]), shifted(b, T[dt]), L1_W, ga, loss, accumulate=accumulate)
    d = a.double() - b.double()
    ref = d.abs().mean() * L1_W
    term = torch.sign(d) * L1_W / L1_COUNT
    want = term + ga0.double() if accumulate else term
    aref = term.abs() + ga0.double().abs() if accumulate else term.abs()
    r_out = R_BF16 if gdt == "bf16" else 0.0
    ratio = worst(ga, want, r_out * want.abs() + 1e-7 * aref + 1e-30)
    lerr = abs(loss.item() - LOSS0 - ref.item())
    report(f"l1 scalar {dt}->{gdt} acc={int(accumulate)}", grad_err_over_bound=ratio,
           loss_err_over_bound=lerr / (LC.R_ACC * ref.item()))
    assert ratio <= 1.0
    assert lerr <= LC.R_ACC * ref.item()


# ----------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------

def test_adam_second_round_host_and_device_step_count(ops):
    n = 8192 * 256 * 4 + 1001
    lr, b1, b2, eps = 2e-4, 0.5, 0.999, 1e-8
    gen = torch.Generator().manual_seed(41)
    p = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) for _ in range(3)]
    pt = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=lr, betas=(b1, b2), eps=eps)
    z = lambda: torch.zeros(n, device=DEV)   # noqa: E731
    ph, mh, vh = p.to(DEV), z(), z()
    pd, md, vd = p.to(DEV), z(), z()
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    prm = torch.zeros(2, device=DEV)
    worst_ulp = 0.0
    for i, gr in enumerate(grads):
        t = i + 1
        pt.grad = gr.clone()
        opt.step()
        gd = gr.to(DEV)
        ops.adam(ph, gd, mh, vh, t, lr, b1, b2, eps)
        ops.adam_prep(count, lr, b1, b2, prm)
        ops.adam_dev(pd, gd, md, vd, prm, b1, b2, eps)
        want = np.array([lr / (1 - b1 ** t), math.sqrt(1 - b2 ** t)], dtype=np.float64).astype(np.float32)
        got = prm.cpu().numpy()
        ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        worst_ulp = max(worst_ulp, float(ulps.max()))
        assert ulps.max() <= 1.0, (t, got, want)
    assert count.item() == 3
    ref = pt.detach()
    eh, ed = float((ph.cpu() - ref).abs().max()), float((pd.cpu() - ref).abs().max())
    report("adam", host_err_over_bound=eh / 5e-7, dev_err_over_bound=ed / 5e-7, prm_ulps=worst_ulp)
    assert eh < 5e-7 and ed < 5e-7
    assert torch.equal(mh, md) and torch.equal(vh, vd)
    # every element was visited, the ragged tail included.  m alone cannot tell at this n: it
    # cancels to an exact zero where g_3 == -m_2 (element 1621412 of this seed, in the CPU's fp32
    # arithmetic as well), so such an element shows its visit by v, which only three zero
    # gradients would leave at zero
    assert bool(((mh != 0) | (vh != 0)).all())
    assert int((mh == 0).sum()) <= n // 10 ** 6
