"""engine.fp8_plan without a GPU or the library: the numbering of the e4m3 weight images and of
the activation scale slots.  The Fp8Weights job order and every Fp8Acts.snapshot() / update()
range depend on it; a wrong index would not fail, it would read another layer's valid scale."""
import pytest

from conftest import pkg


def _plan(n_blocks, fp8_ud):
    return pkg().engine.fp8_plan(n_blocks, fp8_ud)


@pytest.mark.parametrize("fp8_ud", [False, True])
@pytest.mark.parametrize("n", [1, 2, 9])
def test_fp8_plan_numbers_every_image_and_slot_once(n, fp8_ud):
    convs, slots = _plan(n, fp8_ud)
    assert len(convs) == 2 * n + (2 if fp8_ud else 0)
    assert len({c.key for c in convs}) == len(convs)
    # weight images: exactly range(4n) / range(4n + 4), each once
    images = [i for c in convs for i in (c.w_fwd, c.w_flip)]
    assert sorted(images) == list(range(4 * n + (4 if fp8_ud else 0)))
    # the named ranges are contiguous (start, count) pairs that tile range(4n + 4), each slot once
    assert set(slots) == {"fwd", "dy", "cat", "ud_dy", "x1"}
    covered = [s for start, count in slots.values() for s in range(start, start + count)]
    assert sorted(covered) == list(range(4 * n + 4))

    def inside(slot, name):
        return slots[name][0] <= slot < slots[name][0] + slots[name][1]
    # every record's slots lie in the range that rolls them; with the calibration-only x1 slot, which
    # no record names, the records' slots and the ranges cover range(4n + 4)
    res, ud = convs[:2 * n], convs[2 * n:]
    assert all(inside(c.s_x, "fwd") and inside(c.s_dy, "dy") for c in res)
    assert all(inside(c.s_x, "cat") and inside(c.s_dy, "ud_dy") for c in ud)
    assert sorted(c.s_x for c in res) == list(range(2 * n))
    assert sorted(c.s_dy for c in res) == list(range(2 * n, 4 * n))
    used = {s for c in convs for s in (c.s_x, c.s_dy)} | {slots["x1"][0]}
    if fp8_ud:   # down2 reads the x1 slice of up1_conv's concat: one operand slot for both
        assert [c.s_x for c in ud] == [4 * n, 4 * n] and sorted(c.s_dy for c in ud) == [4 * n + 1, 4 * n + 2]
        assert used == set(range(4 * n + 4))
    else:
        assert used == set(range(4 * n)) | {4 * n + 3}


def test_fp8_plan_layout_two_blocks():
    """The full table for n_blocks = 2 with down2 / up1_conv, written out."""
    convs, slots = _plan(2, True)
    #        key                        w_fwd w_flip s_x s_dy
    want = [("resblocks.0.conv_block.1", 0, 1, 0, 5),
            ("resblocks.0.conv_block.5", 2, 3, 1, 4),
            ("resblocks.1.conv_block.1", 4, 5, 2, 7),
            ("resblocks.1.conv_block.5", 6, 7, 3, 6),
            ("down2.0", 8, 9, 8, 10),
            ("up1_conv.0", 10, 11, 8, 9)]
    assert [tuple(c) for c in convs] == want
    assert slots == {"fwd": (0, 4), "dy": (4, 4), "cat": (8, 1), "ud_dy": (9, 2), "x1": (11, 1)}


def test_fp8_plan_is_what_the_engine_builds_from():
    """The record fields by name (the engine reads them by name, never by position)."""
    c = _plan(1, False)[0][0]
    assert (c.key, c.w_fwd, c.w_flip, c.s_x, c.s_dy) == ("resblocks.0.conv_block.1", 0, 1, 0, 3)
