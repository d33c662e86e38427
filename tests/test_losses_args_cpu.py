"""ops.tv and ops.ssim pass only (ptr, N, H, W, C) to the library, which reads the image as
contiguous NHWC.  A Feat that is a channel slice (ld != C, or off != 0) would be read as if
it were whole, silently; both wrappers refuse it before anything is launched or written, so
the check needs no device."""
import pytest
import torch

from conftest import pkg

SENTINEL = -7.0


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


def _bufs(C):
    g = torch.full((1, 4, 5, C), SENTINEL)
    loss = torch.full((1,), SENTINEL, dtype=torch.float64)
    work = torch.full((10 * g.numel(),), SENTINEL)
    return g, loss, work


# (ld, off, C) of the slice: narrower than the row, offset into it, both
SLICES = [(8, 0, 3), (4, 1, 3), (8, 2, 3)]


@pytest.mark.parametrize("ld,off,C", SLICES)
def test_tv_refuses_a_channel_slice(ops, ld, off, C):
    x = ops.Feat(torch.zeros(1, 4, 5, ld), off, C)
    g, loss, _ = _bufs(C)
    with pytest.raises(ValueError, match="channel slice"):
        ops.tv(x, 0.5, g, loss)
    assert bool((g == SENTINEL).all()) and loss.item() == SENTINEL


@pytest.mark.parametrize("which", ["a", "b"])
@pytest.mark.parametrize("ld,off,C", SLICES)
def test_ssim_refuses_a_channel_slice(ops, ld, off, C, which):
    whole = ops.Feat(torch.zeros(1, 4, 5, C))
    sl = ops.Feat(torch.zeros(1, 4, 5, ld), off, C)
    g, loss, work = _bufs(C)
    with pytest.raises(ValueError, match="channel slice"):
        ops.ssim(sl if which == "a" else whole, whole if which == "a" else sl, 0.5, g, loss, work)
    assert bool((g == SENTINEL).all()) and loss.item() == SENTINEL and bool((work == SENTINEL).all())
