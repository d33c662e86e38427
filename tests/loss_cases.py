"""Shared data, references and the error yardstick of the SSIM parity tests
(test_gpu_losses.py on the device, test_losses_bound_cpu.py without one).  Torch on the CPU
only: nothing here loads the library or touches a GPU.

The yardstick: the oracle's ssim_loss run in fp32 differs from the same oracle in fp64 by
E32 = max |g32 - g64| over the gradient; a kernel passes when every element of its gradient
is within MARGIN * E32 of g64.  Kernel and oracle sum the same terms in another order (two
separable K-tap passes with an fp32 window against one K*K-tap convolution), so neither is
a priori the more accurate and the margin is 4, not 1.
"""
import functools

import torch
import torch.nn.functional as F

from oracle import step as O

MARGIN = 4.0
R_ACC = 2e-5        # long fp32 sums of non-negative terms (test_gpu_bf16_elementwise.py)
SSIM_W = 0.85       # loss weight of every SSIM case (not 1, halves exactly)
LOSS0 = 0.123       # pre-fill of the fp64 loss word

# name -> (N, H, W, C), window
SSIM_CASES = {
    "two_xblocks_ragged_rows": ((2, 21, 100, 3), 11),   # with planted zero-variance patches
    "two_xblocks_plain": ((2, 21, 100, 3), 11),         # the same shape at the E32 of random images
    "widest_lds_row": ((1, 9, 1820, 3), 11),
    "global_fallback": ((1, 12, 1824, 3), 11),
    "all_border_w15": ((2, 5, 40, 3), 15),
    "all_border_w13": ((2, 5, 40, 3), 13),
    "window1": ((2, 9, 40, 3), 1),
    "window9": ((2, 9, 40, 3), 9),
    "c1_odd_batch": ((3, 17, 300, 1), 11),
}


def ssim_inputs(name):
    """(a, b, g0): fp32 NHWC images in [-1, 1] and the non-zero pre-fill of g, at the scale
    w / S of the gradient itself so that it perturbs the sum without drowning it."""
    (N, H, W, C), _ = SSIM_CASES[name]
    gen = torch.Generator().manual_seed(1000 + sorted(SSIM_CASES).index(name))
    a = torch.rand(N, H, W, C, generator=gen) * 2 - 1
    b = (a + 0.4 * torch.randn(N, H, W, C, generator=gen)).clamp(-1, 1)
    if name == "two_xblocks_ragged_rows":
        # zero variance in both images (s11 + s22 + C2 at its minimum), across the x-block
        # boundary e = 256 (x = 85.3), up to the right border and into the ragged row block
        a[0, 4:19, 70:100, :] = 0.3
        b[0, 4:19, 70:100, :] = 0.3
        # zero variance in a alone
        a[1, 2:16, 5:35, :] = -0.6
    g0 = torch.randn(N, H, W, C, generator=gen) * (SSIM_W / a.numel())
    g0[g0 == 0] = SSIM_W / a.numel()
    return a, b, g0


def _oracle(a, b, g0, window, w, dtype):
    x = a.to(dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = b.to(dtype).permute(0, 3, 1, 2).contiguous()
    loss = O.ssim_loss((x + 1) / 2, (y + 1) / 2, window_size=window) * w
    loss.backward()
    return loss.detach(), x.grad.permute(0, 2, 3, 1).contiguous() + g0.to(dtype)


@functools.lru_cache(maxsize=None)
def ssim_reference(name, w=SSIM_W):
    """(l64, g64, E32) of a case: the fp64 oracle's weighted loss and gradient (g0 added) and
    the fp32 oracle's worst gradient error against it.  Cached: computed once, never written."""
    a, b, g0 = ssim_inputs(name)
    _, window = SSIM_CASES[name]
    l64, g64 = _oracle(a, b, g0, window, w, torch.float64)
    _, g32 = _oracle(a, b, g0, window, w, torch.float32)
    e32 = (g32.double() - g64).abs().max().item()
    assert e32 > 0
    return l64.item(), g64, e32


def worst_ratio(got, name, w=SSIM_W):
    """max |got - g64| / E32 of a gradient for a case; the check is ratio <= MARGIN."""
    _, g64, e32 = ssim_reference(name, w)
    return ((got.double() - g64).abs().max() / e32).item()


def gauss_win32(K):
    """gauss_win<K>() of csrc/loss.hip: fp32 taps, sequential fp32 sum, fp32 divide."""
    taps = []
    for k in range(K):
        c = torch.tensor(float(k), dtype=torch.float32) - torch.tensor((K - 1) / 2.0, dtype=torch.float32)
        taps.append(torch.exp(-(c * c) / torch.tensor(2.0 * 1.5 * 1.5, dtype=torch.float32)))
    s = torch.zeros((), dtype=torch.float32)
    for t in taps:
        s = s + t
    return [t / s for t in taps]


def _hpass(maps, win, drop_outer_from=None):
    """Horizontal K-tap pass over NHWC maps, taps added in the kernel's order k = 0..K-1 with
    zeros outside the row.  drop_outer_from = e0: the mutation -- elements e = x*C + c >= e0
    of every row lose their outermost tap (k = K-1)."""
    K, HK = len(win), len(win) // 2
    N, H, W, C = maps[0].shape
    out = []
    keep = None
    if drop_outer_from is not None:
        e = torch.arange(W * C).reshape(W, C)
        keep = (e < drop_outer_from).float()
    for m in maps:
        mp = F.pad(m, (0, 0, HK, HK))
        acc = torch.zeros_like(m)
        for k in range(K):
            term = win[k] * mp[:, :, k:k + W, :]
            if keep is not None and k == K - 1:
                term = term * keep
            acc = acc + term
        out.append(acc)
    return out


def _vpass(maps, win):
    K, HK = len(win), len(win) // 2
    H = maps[0].shape[1]
    out = []
    for m in maps:
        mp = F.pad(m, (0, 0, 0, 0, HK, HK))
        acc = torch.zeros_like(m)
        for k in range(K):
            acc = acc + win[k] * mp[:, k:k + H]
        out.append(acc)
    return out


def separable_fp32(a, b, g0, window, w, drop_outer_from=None):
    """A torch fp32 restatement of the kernels' arithmetic (ssim_hrow / ssim_vfused in
    csrc/loss.hip): (a+1)/2, horizontal then vertical pass of the five moments, the SSIM map
    and its three adjoint maps, horizontal then vertical pass of those, the input gradient
    added into g0.  Returns (loss, g).  drop_outer_from: see _hpass (first horizontal pass)."""
    f = torch.float32
    win = gauss_win32(window)
    S = a.numel()
    p, q = (a.to(f) + 1.0) * 0.5, (b.to(f) + 1.0) * 0.5
    mom = _vpass(_hpass([p, q, p * p, q * q, p * q], win, drop_outer_from), win)
    mu1, mu2, e11, e22, e12 = mom
    C1 = torch.tensor(0.01, dtype=f) * torch.tensor(0.01, dtype=f)
    C2 = torch.tensor(0.03, dtype=f) * torch.tensor(0.03, dtype=f)
    dLdS = -torch.tensor(w, dtype=f) / torch.tensor(float(S), dtype=f)
    m11, m22, m12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11, s22, s12 = e11 - m11, e22 - m22, e12 - m12
    A1, A2 = 2.0 * m12 + C1, 2.0 * s12 + C2
    B1, B2 = m11 + m22 + C1, s11 + s22 + C2
    den = B1 * B2
    Sv = (A1 * A2) / den
    dmu1 = (2.0 * mu2 * (A2 - A1)) / den - Sv * 2.0 * mu1 / B1 + Sv * 2.0 * mu1 / B2
    de11 = -Sv / B2
    de12 = 2.0 * A1 / den
    adj = _vpass(_hpass([dLdS * dmu1, dLdS * de11, dLdS * de12], win), win)
    gp = adj[0] + 2.0 * p * adj[1] + q * adj[2]
    loss = torch.tensor(w, dtype=f) * (1.0 - Sv).sum() / torch.tensor(float(S), dtype=f)
    return loss.item(), g0.to(f) + 0.5 * gp
