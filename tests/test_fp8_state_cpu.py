"""The fp8 delayed-scaling state (ops.Fp8Acts) as saved state, without a GPU: it round-trips
through state_dict() / torch.save / torch.load(weights_only=True) / load_state_dict() on CPU
tensors, loading copies IN PLACE (the ctypes pointers the engine hands to kernels, ops.Pi, point
into the same storage afterwards), a slot-count mismatch is a ValueError that names both counts,
and the slot layout (engine.fp8_plan) is what the saved state is numbered by."""
import importlib
import io

import pytest
import torch

from conftest import pkg


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


def _filled(ops, n, seed):
    g = torch.Generator().manual_seed(seed)
    a = ops.Fp8Acts(n, "cpu")
    e = torch.randint(-6, 12, (n,), generator=g).float()
    a.q.copy_(2.0 ** e)
    a.dq.copy_(2.0 ** -e)
    a.amax.copy_((torch.rand(a.amax.numel(), generator=g) * 50).view(torch.int32))
    a.seen[:] = [bool(v) for v in torch.randint(0, 2, (n,), generator=g).tolist()]
    return a


def test_state_round_trip_in_place(ops):
    n = 11
    a = _filled(ops, n, 1)
    assert any(a.seen) and not all(a.seen)
    sd = a.state_dict()
    assert set(sd) == {"q", "dq", "amax", "seen"}
    assert all(isinstance(v, torch.Tensor) and v.device.type == "cpu" for v in sd.values())
    f = io.BytesIO()
    torch.save(sd, f)
    f.seek(0)
    sd = torch.load(f, map_location="cpu", weights_only=True)
    b = ops.Fp8Acts(n, "cpu")
    assert b.seen == [False] * n and (b.q == 1).all() and not b.amax.any()
    ptrs = (b.q.data_ptr(), b.dq.data_ptr(), b.amax.data_ptr())
    pi = [ops.Pi(b.q, 3).value, ops.Pi(b.dq, 7).value, ops.amax_ptr(b.amax, 2).value]
    seen_list = b.seen
    b.load_state_dict(sd)
    assert torch.equal(b.q, a.q) and torch.equal(b.dq, a.dq) and torch.equal(b.amax, a.amax) and b.seen == a.seen
    # in place: the tensors (and so every pointer into them) are the ones from before the load
    assert ptrs == (b.q.data_ptr(), b.dq.data_ptr(), b.amax.data_ptr())
    assert pi == [ops.Pi(b.q, 3).value, ops.Pi(b.dq, 7).value, ops.amax_ptr(b.amax, 2).value]
    assert b.seen is seen_list
    # the saved state is a copy: changing the source afterwards does not reach it
    a.q.mul_(2)
    assert not torch.equal(a.state_dict()["q"], sd["q"])
    # reset(): every slot unseen again, same storage
    b.reset()
    assert b.seen == [False] * n and (b.q == 1).all() and (b.dq == 1).all() and not b.amax.any()
    assert ptrs == (b.q.data_ptr(), b.dq.data_ptr(), b.amax.data_ptr()) and b.seen is seen_list


def test_slot_count_mismatch_raises(ops):
    a = _filled(ops, 40, 2)
    b = ops.Fp8Acts(12, "cpu")
    before = (b.q.clone(), b.dq.clone(), b.amax.clone(), list(b.seen))
    with pytest.raises(ValueError) as ei:
        b.load_state_dict(a.state_dict())
    assert "40" in str(ei.value) and "12" in str(ei.value)
    assert torch.equal(b.q, before[0]) and torch.equal(b.dq, before[1]) and torch.equal(b.amax, before[2])
    assert b.seen == before[3]


def test_fp8_plan_unchanged():
    """The numbering the saved state depends on: two operand slots and two dY slots per block,
    then the concat, the two dY of up1_conv / down2 and down2's calibration copy of x1."""
    engine = importlib.import_module(pkg().__name__ + ".engine")
    for n in (2, 9):
        for ud in (False, True):
            convs, slots = engine.fp8_plan(n, ud)
            assert slots == {"fwd": (0, 2 * n), "dy": (2 * n, 2 * n), "cat": (4 * n, 1), "ud_dy": (4 * n + 1, 2),
                             "x1": (4 * n + 3, 1)}
            assert sum(c for _, c in slots.values()) == 4 * n + 4
            assert len(convs) == 2 * n + (2 if ud else 0)
            k1, k2 = engine.res_conv_keys()
            for b in range(n):
                assert convs[2 * b] == (f"resblocks.{b}.conv_block.{k1}", 4 * b, 4 * b + 1, 2 * b, 2 * n + 2 * b + 1)
                assert convs[2 * b + 1] == (f"resblocks.{b}.conv_block.{k2}", 4 * b + 2, 4 * b + 3, 2 * b + 1,
                                            2 * n + 2 * b)
            if ud:
                assert convs[2 * n] == ("down2.0", 4 * n, 4 * n + 1, 4 * n, 4 * n + 2)
                assert convs[2 * n + 1] == ("up1_conv.0", 4 * n + 2, 4 * n + 3, 4 * n, 4 * n + 1)
