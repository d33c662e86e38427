"""Self-check of the SSIM bound of test_gpu_losses.py, on the CPU with torch alone (no GPU, no
library load).

The GPU test accepts a gradient whose every element is within 4 * E32 of the fp64 oracle,
E32 being the fp32 oracle's own worst error (tests/loss_cases.py).  Two things have to hold
for that to be a test:

* a correct implementation of the kernels' arithmetic passes: loss_cases.separable_fp32, a
  torch fp32 restatement of csrc/loss.hip (fp32 gauss_win, horizontal then vertical pass,
  the kernel's formulas in the kernel's order), stays inside the margin on the case with
  planted zero-variance patches and on the all-border cases;
* a subtly wrong one fails: the same restatement with ONE mutation -- elements e >= 256 of a
  row (the second x-block / second LDS pass) lose their outermost tap, weight 1e-3 -- is
  outside the margin, so the margin does not hide a one-tap error in the second block.
"""
import pytest
import torch

import loss_cases as LC


def _run(name, **kw):
    a, b, g0 = LC.ssim_inputs(name)
    _, window = LC.SSIM_CASES[name]
    loss, g = LC.separable_fp32(a, b, g0, window, LC.SSIM_W, **kw)
    l64, _, _ = LC.ssim_reference(name)
    return loss, l64, LC.worst_ratio(g, name)


@pytest.mark.parametrize("name", ["two_xblocks_ragged_rows", "all_border_w15", "all_border_w13"])
def test_separable_fp32_restatement_is_inside_the_margin(name):
    loss, l64, ratio = _run(name)
    print(f"{name}: restatement err/E32 = {ratio:.3f}")
    assert ratio <= LC.MARGIN
    assert abs(loss - l64) <= LC.R_ACC * l64


def test_e32_is_a_rounding_sized_fraction_of_the_gradient():
    """The yardstick is no loose tolerance: E32 is a few fp32 roundings of max |g| (<= 1e-5)
    on random images.  The planted zero-variance patches cost more -- there s11 + s22 + C2
    is C2 = 9e-4 plus the fp32 noise of e11 - mu1^2, and 1 / B2-sized adjoints cancel -- but
    4 * E32 still stays below the 1e-3 weight of the window's outermost tap."""
    rels = {}
    for name in LC.SSIM_CASES:
        _, g64, e32 = LC.ssim_reference(name)
        rels[name] = e32 / g64.abs().max().item()
        print(f"{name}: E32 = {e32:.3e} = {rels[name]:.2e} of max|g|")
    planted = rels.pop("two_xblocks_ragged_rows")
    assert max(rels.values()) <= 1e-5
    assert LC.MARGIN * planted <= 1e-3


def test_one_dropped_tap_in_the_second_block_fails_the_margin():
    name = "two_xblocks_ragged_rows"
    (N, H, W, C), window = LC.SSIM_CASES[name]
    assert W * C > 256
    _, _, ok = _run(name)
    _, _, bad = _run(name, drop_outer_from=256)
    print(f"{name}: err/E32 = {ok:.3f} as written, {bad:.1f} with the outermost tap dropped for e >= 256")
    assert ok <= LC.MARGIN < bad
    # the mutation touches the second block only: below e = 256 - (window // 2) * C the two agree
    a, b, g0 = LC.ssim_inputs(name)
    _, g_ok = LC.separable_fp32(a, b, g0, window, LC.SSIM_W)
    _, g_bad = LC.separable_fp32(a, b, g0, window, LC.SSIM_W, drop_outer_from=256)
    cut = (256 - (window // 2) * C) // C
    assert torch.equal(g_ok[:, :, :cut], g_bad[:, :, :cut])
    assert not torch.equal(g_ok[:, :, cut:], g_bad[:, :, cut:])
