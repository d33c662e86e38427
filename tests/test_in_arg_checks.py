"""The InstanceNorm entry points reject bad arguments as the BatchNorm ones do: IRGAN_EINVAL,
nothing launched, nothing written.  Every checked call returns before it touches HIP, so the
test needs no device; where one is present the buffers live on it, and they are large enough
that even an unchecked launch of these arguments would stay inside them."""
import pytest
import torch

from conftest import gpu_available, pkg

N, HW, C = 1, 16, 8
F32, BAD_DT, BAD_ACT = 0, 7, 7
SENTINEL = -7.0


@pytest.fixture(scope="module")
def env():
    irc = pkg()
    lib = irc._lib.load()
    assert irc._lib.F32 == F32
    dev = "cuda" if gpu_available() else "cpu"
    f = lambda n, dt=torch.float32: torch.full((n,), SENTINEL, dtype=dt, device=dev)
    # rows of ld = 8 at off = 8 end at element 15 * 8 + 8 + 7 = 135 < 1024
    bufs = dict(x=f(1024), dy=f(1024), dy2=f(1024), res=f(1024), y=f(1024), dx=f(1024), mr=f(2 * N * C),
                red=f(2 * N * C), db=f(C), work=f(16 * irc._lib.IN_PARTS * C, torch.float64))
    return lib, bufs, irc._lib.header_enum("IRGAN_EINVAL")


GOOD = (F32, C, 0)       # (dtype, ld, off) of a valid slice
BAD_SLICE = (F32, C, C)  # off + C > ld
BAD_DTYPE = (BAD_DT, C, 0)
# the slices each entry takes; those of in_apply share one dtype argument (x's)
SLICES = {
    "irgan_in_stats": ["x"],
    "irgan_in_apply": ["x", "res", "y"],
    "irgan_in_bwd_reduce": ["dy", "dy2", "x"],
    "irgan_in_bwd_apply": ["dy", "dy2", "x", "dx"],
    "irgan_channel_sum": ["x"],
}
TAKES_ACT = {"irgan_in_apply", "irgan_in_bwd_reduce", "irgan_in_bwd_apply"}


def _call(lib, b, entry, act=0, **bad):
    """entry with every argument valid but act and the slices named in ``bad`` (name -> (dtype, ld, off))"""
    p = {k: t.data_ptr() for k, t in b.items()}
    s = {k: bad.get(k, GOOD) for k in ("x", "dy", "dy2", "res", "y", "dx")}
    sl = lambda k: (p[k], *s[k])                # noqa: E731  pointer, dtype, ld, off
    nd = lambda k: (p[k], *s[k][1:])            # noqa: E731  pointer, ld, off
    bwd = (*sl("dy"), *sl("dy2"), *sl("x"), act, N, HW, C, p["mr"])
    if entry == "irgan_in_stats":
        return lib.irgan_in_stats(p["x"], s["x"][0], N, HW, C, *s["x"][1:], p["work"], p["mr"], None)
    if entry == "irgan_in_apply":
        return lib.irgan_in_apply(p["x"], s["x"][0], N, HW, C, *s["x"][1:], p["mr"], act, *nd("res"), *nd("y"), None,
                                  None)
    if entry == "irgan_in_bwd_reduce":
        return lib.irgan_in_bwd_reduce(*bwd, p["work"], p["red"], None)
    if entry == "irgan_in_bwd_apply":
        return lib.irgan_in_bwd_apply(*bwd, p["red"], *sl("dx"), p["db"], None)
    return lib.irgan_channel_sum(p["x"], s["x"][0], N * HW, C, *s["x"][1:], p["db"], p["work"], None)


# one bad argument per case: each slice's offset, each dtype argument, the activation
CASES = [(e, "slice", k) for e, ks in SLICES.items() for k in ks]
CASES += [(e, "dtype", k) for e, ks in SLICES.items() for k in (ks if e != "irgan_in_apply" else ["x"])]
CASES += [(e, "act", "") for e in SLICES if e in TAKES_ACT]


@pytest.mark.parametrize("entry,bad,which", CASES)
def test_in_entry_points_reject_bad_arguments(env, entry, bad, which):
    lib, bufs, einval = env
    kw = {"slice": {which: BAD_SLICE}, "dtype": {which: BAD_DTYPE}, "act": {"act": BAD_ACT}}[bad]
    assert _call(lib, bufs, entry, **kw) == einval
    for name, t in bufs.items():
        assert bool((t == SENTINEL).all()), f"{entry} wrote {name}"
