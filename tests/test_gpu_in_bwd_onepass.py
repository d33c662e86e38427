"""The one-pass InstanceNorm backward (irgan_in_bwd_onepass[_fp8], in_bwd_onepass_kernel):
one workgroup per (image, 16 channels) loads dy and z once, reduces and writes dx.

The entry point is called directly through ``ops.in_bwd_onepass`` (independent of
in_backward's policy) and held to the fp64 reference and bounds of
test_gpu_bf16_elementwise.py::test_in_backward_bf16:

    red = {mean g, mean g*xhat}:  |got - ref64| <= 2e-5 * mean|terms|
    dx:  |got - ref64| <= 2^-8 |ref64| + 1e-5 * absref,  ref64 from the RETURNED red

and to the three launches it replaces, bit for bit (red, dx, the fp8 copy).

Shapes: the full register capacity (4096 px) with two channel groups per image, 4095 px,
a tail that ends inside the chains, one pixel, and a PatchGAN shape.  The policy of
``ops.in_backward`` is plain Python and is tested without a GPU.
"""
import functools
import importlib.util
import os

import pytest
import torch

from conftest import PKG_NAME, ROOT, pkg

gpu = pytest.mark.gpu
DEV = "cuda"
R_BF16 = 2.0 ** -8
SENT = -3.0   # bf16-exact filler of everything a launch must not write


@pytest.fixture(scope="module")
def ops():
    return pkg().ops


def q(t):
    return t.bfloat16().float()


def to_slice(x, ld_extra, off, fill=SENT, dtype=torch.bfloat16):
    N, C, H, W = x.shape
    t = torch.full((N, H, W, C + ld_extra), fill, device=DEV, dtype=dtype)
    t[..., off:off + C] = x.permute(0, 2, 3, 1).to(DEV, dtype)
    return t


def from_slice(t, off, C):
    return t[..., off:off + C].double().cpu().permute(0, 3, 1, 2).contiguous()


def outside_untouched(t, off, C, fill=SENT):
    return bool((t[..., :off] == fill).all()) and bool((t[..., off + C:] == fill).all())


def check(got, ref, aref, r_out, r_acc, what):
    err = (got.double() - ref).abs()
    bound = r_out * ref.abs() + r_acc * aref + 1e-30
    ratio = (err / bound).max().item()
    assert ratio <= 1.0, f"{what}: worst |err|/bound = {ratio:.3g}, max |err| {err.max().item():.3g}"


def act_grad32(xh32, act):
    if act == 1:
        return (xh32 > 0).double()
    if act == 2:
        return torch.where(xh32 > 0, 1.0, 0.2).double()
    return torch.ones_like(xh32, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def inputs(shape, seed=3):
    """(z, dy) on the CPU, bf16-representable; shared by every case of a shape."""
    g = torch.Generator().manual_seed(seed)
    return q(torch.randn(shape, generator=g) * 2 + 0.5), q(torch.randn(shape, generator=g))


def stats(ops, zd, off, C):
    N = zd.shape[0]
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    mr = torch.empty(2 * N * C, device=DEV)
    ops.in_stats(ops.Feat(zd, off, C), work, mr)
    return mr


def check_backward(z, dy, act, mr, red, dx64, what, d2=None):
    """red and dx against fp64 on the same bf16 values (test_in_backward_bf16's reference)."""
    N, C, H, W = z.shape
    m = mr.view(N, C, 2).cpu()
    m32, r32 = m[..., 0, None, None], m[..., 1, None, None]
    xh32 = (z - m32) * r32                                  # the kernels' fp32 xhat (mask decisions)
    mean, rstd = m32.double(), r32.double()
    xh = (z.double() - mean) * rstd
    g = (dy.double() + (d2.double() if d2 is not None else 0.0)) * act_grad32(xh32, act)
    mg, mgx = g.mean(dim=(2, 3)), (g * xh).mean(dim=(2, 3))
    got_red = red.view(N, C, 2).double().cpu()
    check(got_red[..., 0], mg, g.abs().mean(dim=(2, 3)), 0.0, 2e-5, f"{what}: mean g")
    check(got_red[..., 1], mgx, (g * xh).abs().mean(dim=(2, 3)), 0.0, 2e-5, f"{what}: mean g*xhat")
    kg, kgx = got_red[..., 0, None, None], got_red[..., 1, None, None]
    ref = rstd * (g - kg - xh * kgx)
    aref = rstd * (g.abs() + kg.abs() + (xh * kgx).abs())
    check(dx64, ref, aref, R_BF16, 1e-5, f"{what}: dx")


SHAPES = [(2, 32, 64, 64),    # full capacity, two groups per image
          (1, 16, 63, 65),    # 4095 px, one short of capacity
          (3, 48, 45, 38),    # masked tail inside the chains, in-order block combine
          (1, 16, 1, 1),      # a single pixel
          (2, 512, 31, 31)]   # a D shape
# (ld - C, off) of z / of dy and dx: ld = C + 16 at off = 8; then z in rows of 2C + 48 bytes
# at byte offset 48 and dy, dx in rows of 2C + 16 bytes at byte offset 16 -- every access
# 16-byte aligned, every other pixel's not 32-byte aligned
SLICES = {"c16o8": ((16, 8), (16, 8)), "c24o24": ((24, 24), (8, 8))}


@gpu
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("sl", sorted(SLICES))
@pytest.mark.parametrize("inplace", [True, False])
@pytest.mark.parametrize("act", [0, 1, 2])
def test_onepass_fp64(ops, shape, sl, inplace, act):
    N, C, H, W = shape
    z, dy = inputs(shape)
    (zx, zo), (gx, go) = SLICES[sl]
    zd, dyd = to_slice(z, zx, zo), to_slice(dy, gx, go)
    mr = stats(ops, zd, zo, C)
    red = torch.empty(2 * N * C, device=DEV)
    dxd, do = (dyd, go) if inplace else (torch.full((N, H, W, C + gx), SENT, device=DEV, dtype=torch.bfloat16), go)
    zd0 = zd.clone()
    assert ops.in_bwd_onepass(ops.Feat(dyd, go, C), ops.Feat(zd, zo, C), act, mr, red, ops.Feat(dxd, do, C))
    check_backward(z, dy, act, mr, red, from_slice(dxd, do, C), f"onepass {shape} {sl} act={act} inplace={inplace}")
    assert outside_untouched(dxd, do, C), "one-pass wrote outside its channel slice"
    assert torch.equal(zd, zd0)
    if not inplace:
        assert torch.equal(from_slice(dyd, go, C), dy.double()) and outside_untouched(dyd, go, C)


def _illegal(name):
    """(shape, z dtype, dy2?, ld_extra of dx) of each argument set the kernel must refuse."""
    return {"hw4097": ((1, 16, 17, 241), torch.bfloat16, False, 0),
            "c24": ((2, 24, 8, 8), torch.bfloat16, False, 0),
            "fp32z": ((2, 16, 8, 8), torch.float32, False, 0),
            "dy2": ((2, 16, 8, 8), torch.bfloat16, True, 0),
            "ldc4": ((2, 16, 8, 8), torch.bfloat16, False, 4)}[name]


@gpu
@pytest.mark.parametrize("name", ["hw4097", "c24", "fp32z", "dy2", "ldc4"])
def test_onepass_refuses(ops, name):
    """IRGAN_EUNSUPPORTED: nothing launched, dx and red untouched; ops.in_backward at the same
    arguments still answers through reduce + finalize + apply."""
    shape, zdt, with2, ldx_extra = _illegal(name)
    N, C, H, W = shape
    z, dy = inputs(shape)
    d2 = q(inputs(shape, seed=4)[1] * 0.5) if with2 else None
    zd = to_slice(z, 0, 0, dtype=zdt)
    dyd = to_slice(dy, 0, 0)
    d2d = to_slice(d2, 0, 0) if with2 else None
    mr = stats(ops, zd, 0, C)
    red = torch.full((2 * N * C,), 77.0, device=DEV)
    dxd = torch.full((N, H, W, C + ldx_extra), SENT, device=DEV, dtype=torch.bfloat16)
    F = ops.Feat
    args = (F(dyd), F(zd), 1, mr)
    kw = dict(dy2=F(d2d) if with2 else None)
    assert not ops.in_bwd_onepass(*args, red, F(dxd, 0, C), **kw)
    torch.cuda.synchronize()
    assert bool((dxd == SENT).all()) and bool((red == 77.0).all()), "a refused call wrote its outputs"
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    ops.in_backward(*args, work, red, F(dxd, 0, C), **kw)
    check_backward(z, dy, 1, mr, red, from_slice(dxd, 0, C), f"in_backward {name}", d2=d2)


@gpu
@pytest.mark.parametrize("shape", SHAPES + [(16, 256, 16, 16), (4, 128, 32, 24), (32, 64, 7, 9)])
@pytest.mark.parametrize("act", [1, 2])
def test_onepass_equals_three_launches(ops, shape, act):
    """red and dx are bit for bit those of reduce + finalize + apply: the one-pass kernel groups
    its sums as rows8_kernel<1> and finalize_kernel do (tree and in-order block combines, one
    and several partials per finalize lane), so a step computes what it computed before."""
    N, C, H, W = shape
    z, dy = inputs(shape)
    zd, dyd = to_slice(z, 0, 0), to_slice(dy, 16, 8)
    mr = stats(ops, zd, 0, C)
    F = ops.Feat
    red1, red3 = torch.zeros(2 * N * C, device=DEV), torch.zeros(2 * N * C, device=DEV)
    dx1, dx3 = torch.zeros_like(zd), torch.zeros_like(zd)
    assert ops.in_bwd_onepass(F(dyd, 8, C), F(zd), act, mr, red1, F(dx1))
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    reduce, apply = ops.in_bwd_parts(F(dyd, 8, C), F(zd), act, mr, work, red3, F(dx3))
    reduce()
    apply()
    assert torch.equal(red1, red3), (red1 - red3).abs().max().item()
    assert torch.equal(dx1, dx3)


@gpu
def test_onepass_deterministic(ops):
    shape = SHAPES[0]
    N, C, H, W = shape
    z, dy = inputs(shape)
    zd, dyd = to_slice(z, 0, 0), to_slice(dy, 0, 0)
    mr = stats(ops, zd, 0, C)
    out = []
    for _ in range(2):
        red = torch.zeros(2 * N * C, device=DEV)
        dx = torch.zeros_like(zd)
        assert ops.in_bwd_onepass(ops.Feat(dyd), ops.Feat(zd), 1, mr, red, ops.Feat(dx))
        out.append((dx, red))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@gpu
def test_onepass_fp8_copy(ops):
    """irgan_in_bwd_onepass_fp8: the same bf16 dx and red as the plain kernel, and the fp8
    bytes and amax irgan_fp8_quant makes from that dx (test_gpu_fp8.py's pattern)."""
    shape = SHAPES[0]
    N, C, H, W = shape
    Fe = ops.Feat
    z, dy = inputs(shape)
    zd, dyd = to_slice(z, 0, 0), to_slice(dy, 0, 0)
    mr = stats(ops, zd, 0, C)
    qt = torch.tensor([8.0], device=DEV)
    red, red2 = torch.empty(2 * N * C, device=DEV), torch.empty(2 * N * C, device=DEV)
    dx, dx2 = torch.empty_like(zd), torch.empty_like(zd)
    y8 = torch.empty(zd.shape, dtype=torch.float8_e4m3fn, device=DEV)
    amax = ops.amax_slots(1, DEV)
    assert ops.in_bwd_onepass(Fe(dyd), Fe(zd), ops.ACT_RELU, mr, red, Fe(dx),
                              q8=(Fe(y8), ops.Pi(qt, 0), ops.amax_ptr(amax, 0)))
    assert ops.in_bwd_onepass(Fe(dyd), Fe(zd), ops.ACT_RELU, mr, red2, Fe(dx2))
    assert torch.equal(dx, dx2) and torch.equal(red, red2)
    ref8 = torch.empty_like(y8)
    ra = ops.amax_slots(1, DEV)
    ops.fp8_quant(Fe(dx), Fe(ref8), ops.Pi(qt, 0), ops.amax_ptr(ra, 0))
    assert torch.equal(y8.view(torch.uint8), ref8.view(torch.uint8))
    assert amax.max().item() == ra.max().item() > 0
    # and the three launches with the fp8 side output give the same bytes
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    red3, dx3, y83 = torch.empty_like(red), torch.empty_like(zd), torch.empty_like(y8)
    a3 = ops.amax_slots(1, DEV)
    reduce, apply = ops.in_bwd_parts(Fe(dyd), Fe(zd), ops.ACT_RELU, mr, work, red3, Fe(dx3),
                                     q8=(Fe(y83), ops.Pi(qt, 0), ops.amax_ptr(a3, 0)))
    reduce()
    apply()
    assert torch.equal(red, red3) and torch.equal(dx, dx3) and torch.equal(y8.view(torch.uint8), y83.view(torch.uint8))
    assert amax.max().item() == a3.max().item()


@gpu
def test_in_backward_takes_onepass(ops, monkeypatch):
    """At N * C / 16 >= half the CUs ops.in_backward is the one-pass launch, with and without
    the fp8 side output; with the switch off it is not."""
    shape = (16, 256, 4, 4)
    N, C, H, W = shape
    Fe = ops.Feat
    z, dy = inputs(shape)
    zd, dyd = to_slice(z, 0, 0), to_slice(dy, 0, 0)
    mr = stats(ops, zd, 0, C)
    work = torch.empty(ops.IN_PARTS * N * C, dtype=torch.float64, device=DEV)
    calls = []
    real = ops.in_bwd_onepass
    monkeypatch.setattr(ops, "in_bwd_onepass", lambda *a, **k: calls.append(1) or real(*a, **k))
    red, dx = torch.empty(2 * N * C, device=DEV), torch.empty_like(zd)
    ops.in_backward(Fe(dyd), Fe(zd), 2, mr, work, red, Fe(dx))
    assert len(calls) == 1
    check_backward(z, dy, 2, mr, red, from_slice(dx, 0, C), "in_backward (one-pass)")
    y8 = torch.empty(zd.shape, dtype=torch.float8_e4m3fn, device=DEV)
    qt, amax = torch.tensor([8.0], device=DEV), ops.amax_slots(1, DEV)
    dx8 = torch.empty_like(zd)
    ops.in_backward(Fe(dyd), Fe(zd), 2, mr, work, red, Fe(dx8), q8=(Fe(y8), ops.Pi(qt, 0), ops.amax_ptr(amax, 0)))
    assert len(calls) == 2 and torch.equal(dx8, dx)
    monkeypatch.setattr(ops, "IN_BWD_ONEPASS", [False])
    dx3 = torch.empty_like(zd)
    ops.in_backward(Fe(dyd), Fe(zd), 2, mr, work, red, Fe(dx3))
    assert len(calls) == 2
    check_backward(z, dy, 2, mr, red, from_slice(dx3, 0, C), "in_backward (switch off)")


# ---- the policy (no GPU) ----------------------------------------------------------------

BF, F32 = 1, 0
OKDT, OKLD = (BF, BF, BF), (256, 0, 256, 0, 256, 0)


def test_policy_threshold_and_legality(ops):
    use = ops.in_bwd_use_onepass
    assert use(16, 4096, 256, OKDT, OKLD, 256)            # the resblock shape: 256 workgroups
    assert use(8, 4096, 256, OKDT, OKLD, 256)             # exactly half the CUs
    assert not use(7, 4096, 256, OKDT, OKLD, 256)         # 112 workgroups: the row-split passes
    assert use(32, 961, 512, OKDT, OKLD, 256)
    assert not use(16, 4097, 256, OKDT, OKLD, 256)        # does not fit the registers
    assert not use(16, 4096, 264, OKDT, OKLD, 256)        # C % 16
    assert not use(16, 4096, 256, (BF, F32, BF), OKLD, 256)
    assert not use(16, 4096, 256, OKDT, (260, 0, 256, 0, 256, 0), 256)
    assert not use(16, 4096, 256, OKDT, (256, 4, 256, 0, 256, 0), 256)
    assert not use(16, 4096, 256, OKDT, OKLD, 256, has_db=True)
    assert not use(16, 4096, 256, OKDT, OKLD, 256, has_dy2=True)


def test_policy_ignores_q8(ops):
    """The fp8 side output never changes the path: the same bf16 dx plus its copy."""
    for N, HW, C in [(16, 4096, 256), (4, 4096, 256), (32, 1024, 256), (16, 16384, 128), (2, 100, 24)]:
        for db in (False, True):
            a = ops.in_bwd_use_onepass(N, HW, C, OKDT, OKLD, 256, has_db=db)
            assert a == ops.in_bwd_use_onepass(N, HW, C, OKDT, OKLD, 256, has_db=db, q8=object())


def test_policy_env_switch(ops, monkeypatch):
    """IRGAN_IN_BWD_ONEPASS=0 selects reduce + finalize + apply; unset or 1 leaves the policy
    on.  The switch is read when ops is imported: a second copy of the module is executed
    under each setting (the package's own ops stays as it is)."""
    got = []
    for v in (None, "1", "0"):
        monkeypatch.delenv("IRGAN_IN_BWD_ONEPASS", raising=False)
        if v is not None:
            monkeypatch.setenv("IRGAN_IN_BWD_ONEPASS", v)
        spec = importlib.util.spec_from_file_location(f"{PKG_NAME}._ops_env_probe", os.path.join(ROOT, PKG_NAME, "ops.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        got.append(mod.in_bwd_use_onepass(16, 4096, 256, OKDT, OKLD, 256))
    assert got == [True, True, False]
