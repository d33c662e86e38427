"""Thin typed wrappers over the C ABI (include/irgan.h) on device tensors.

Activations are NHWC ``Feat`` slices (tensor, channel offset, channel count);
torch is used for device memory and the current HIP stream only.  Every
function here launches hand-written HIP kernels from libirgan.so.
"""
from __future__ import annotations

import ctypes
import math
import os

import torch

from . import _lib
from ._lib import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, BF16, F32, FP8, IN_PARTS, PAD_REFLECT,  # noqa: F401
                   PAD_ZERO)

TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, FP8: torch.float8_e4m3fn}


def dt_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float8_e4m3fn:
        return FP8
    raise TypeError(f"unsupported dtype {t.dtype}")


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return ctypes.c_void_p(0 if t is None else t.data_ptr())


def Pi(t, i):
    """Pointer to element i of a contiguous device tensor (a scale / amax slot)."""
    return ctypes.c_void_p(t.data_ptr() + i * t.element_size())


_DET = [False]
CONV_DETERMINISTIC = _lib.header_enum("IRGAN_CONV_DETERMINISTIC")


def set_deterministic(on: bool) -> bool:
    """Deterministic mode for the launches this module makes: every split-K weight gradient
    carries IRGAN_CONV_DETERMINISTIC in its descriptor (ordered slab reduction, never fp32
    atomics), so the step is bitwise reproducible under any stream schedule.  Host-side
    state of this module (the library keeps none).  Returns the previous setting."""
    old, _DET[0] = _DET[0], bool(on)
    return old


_RING_WS = {}


def _ring_ws(dev, floats):
    """Per-(device, stream) fp32 workspace of the ring's line GEMM (irgan_reflect_dgrad_ring_ws)."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    w = _RING_WS.get(key)
    if w is None or w.numel() < floats:
        w = _RING_WS[key] = torch.empty(floats, dtype=torch.float32, device=dev)
    return w


RING_LINE = [True]


def set_ring_line(on: bool) -> bool:
    """The line-GEMM ring launches (default) or the general reflect_ring_kernel for the
    ResnetBlock shapes (the A/B reference of the line form).  Returns the previous setting."""
    old, RING_LINE[0] = RING_LINE[0], bool(on)
    return old


RING_EPI = [True]


def set_ring_epi(on: bool) -> bool:
    """The ResnetBlock ring folded into the interior launch's store pass
    (irgan_conv_dgrad_reflect_line, default) or the separate fold launch after it -- the
    same dx bit for bit (tests/test_gpu_ring_epi.py).  Returns the previous setting."""
    old, RING_EPI[0] = RING_EPI[0], bool(on)
    return old


def _ring(d, dy: "Feat", buf, p, dx: "Feat"):
    """The reflect-pad ring of a bf16 backward-data onto dx (after its interior): the line
    GEMM + fold on ResnetBlock shapes, else the general ring launch (the library decides)."""
    ws = _ring_ws(dx.t.device, dx.N * 4 * 68 * dx.C)
    _lib.call("irgan_reflect_dgrad_ring_ws", ctypes.byref(d), dy.ptr, P(buf), p, dx.ptr, P(ws),
              ws.numel() if RING_LINE[0] else 0, 1 << 20, stream())


class LaunchTimer:
    """Optional HIP-event timing of tagged conv launches (bench.py's live
    roofline).  Events are recorded on the launching stream around each launch."""

    def __init__(self, tags):
        self.tags = set(tags)   # None: every tagged launch (tools/layer_times.py)
        self.pending = []
        self.enabled = False

    def wrap(self, tag, fn, count=0):
        """count > 0: the launch does the work of that many launches of ``tag`` (a grouped weight
        gradient): it is recorded as ``count`` launches of elapsed / count each, and not at all
        when fn returns False (nothing ran)."""
        if not self.enabled or (self.tags is not None and tag not in self.tags):
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        if count and out is False:
            return out
        b.record()
        self.pending.append((tag, a, b, count or 1))
        return out

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for tag, a, b, count in self.pending:
            n, t = agg.get(tag, (0, 0.0))
            agg[tag] = (n + count, t + a.elapsed_time(b))
        return {k: (n, t / n) for k, (n, t) in agg.items()}  # (launches, mean ms)


TIMER = LaunchTimer(())


def hbm_tag(kind, x: "Feat"):
    """Tag of an HBM-bound pass over the NHWC tensor x (bench.py's GB/s lines)."""
    return f"{kind}:b{x.N}@{x.H}x{x.W}x{x.C}"


def _timed(kind, x, fn):
    return TIMER.wrap(hbm_tag(kind, x), fn) if TIMER.enabled else fn()


def conv_tag(kind, spec, x_hw, n=None):
    pad = "r" if spec.mode == PAD_REFLECT else "z"
    nb = f"b{n}/" if n is not None else ""
    return f"{kind}:{spec.cin}x{spec.cout}k{spec.k}s{spec.stride}{pad}@{nb}{x_hw[0]}x{x_hw[1]}"


class Feat:
    """NHWC channel slice: element (p, c) at t.view(-1)[p*ld + off + c]."""
    __slots__ = ("t", "off", "C")

    def __init__(self, t: torch.Tensor, off: int = 0, C: int | None = None):
        assert t.dim() == 4 and t.is_contiguous()
        self.t, self.off = t, off
        self.C = t.shape[3] - off if C is None else C

    N = property(lambda s: s.t.shape[0])
    H = property(lambda s: s.t.shape[1])
    W = property(lambda s: s.t.shape[2])
    ld = property(lambda s: s.t.shape[3])
    dt = property(lambda s: dt_code(s.t))
    P = property(lambda s: s.t.shape[0] * s.t.shape[1] * s.t.shape[2])

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def sl(self, off, C):
        return Feat(self.t, self.off + off, C)

    def batch(self, b0, nb):
        return Feat(self.t[b0:b0 + nb], self.off, self.C)


# ----------------------------------------------------------------------------
# convolution
# ----------------------------------------------------------------------------

class ConvSpec:
    """A conv layer's geometry.  For nn.ConvTranspose2d the spec describes the
    conv it transposes (cout = ConvT in-channels, cin = ConvT out-channels)."""

    def __init__(self, cin, cout, k, stride=1, pad=0, mode=PAD_ZERO):
        self.cin, self.cout, self.k, self.stride, self.pad, self.mode = cin, cout, k, stride, pad, mode

    def out_hw(self, H, W):
        p, k, s = self.pad, self.k, self.stride
        return (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1

    def phases(self, reflect_padded=False):
        """backward-data phase decomposition per axis: (phase, tap residue, taps, c0)."""
        k, s = self.k, self.stride
        p = 0 if reflect_padded else self.pad
        out = []
        for ph in range(s):
            tr = (ph + p) % s
            A = max(0, -(-(k - tr) // s))
            base = (ph + p - tr) // s
            out.append((ph, tr, A, base - A + 1))
        return out


def _desc(**kw):
    """irgan_conv_desc from keyword fields.  Built by the Structure's own keyword
    constructor (~2 us on the host, half the setattr loop: ~150 conv launches per step);
    values that are not plain ints (numpy / torch scalars) take the converting path."""
    try:
        return _lib.ConvDesc(**kw)
    except TypeError:
        d = _lib.ConvDesc()
        for k, v in kw.items():
            setattr(d, k, int(v))
        return d


def _fwd_desc(s: "ConvSpec", x: "Feat", y: "Feat", cin, dtype, out_dtype, act=ACT_NONE, accumulate=0, y_sized=True,
              **extra):
    """The forward-style descriptor of conv ``s`` over x (``cin`` channels as stored) with y at the
    conv's output size (checked, unless y only lends its ld / off: ``y_sized`` False) -- the output
    of a forward, the dY a weight gradient reads.  ``extra``: the fields that are 0 elsewhere
    (mask_act / ldm / moff, cin_real, flags)."""
    N, H, W, ldx = x.t.shape   # one shape read: ~150 conv launches per step go through here
    Ho, Wo = s.out_hw(H, W)
    assert not y_sized or y.t.shape[:3] == (N, Ho, Wo), "conv shape mismatch"
    return _desc(N=N, H=H, W=W, Cin=cin, ldx=ldx, xoff=x.off, Ho=Ho, Wo=Wo, Cout=s.cout, ldy=y.t.shape[3],
                 yoff=y.off, OH=Ho, OW=Wo, omy=1, ooy=0, omx=1, oox=0, KH=s.k, KW=s.k, sy=s.stride, sx=s.stride,
                 c0y=-s.pad, c0x=-s.pad, pad_mode=s.mode, act=act, accumulate=int(accumulate), dtype=dtype,
                 out_dtype=out_dtype, **extra)


def _dgrad_desc(pc: "PackedConv", phase, dy: "Feat", dx: "Feat", accumulate, dtype=None, mask: "Feat" = None,
                mask_act=0, shift=0, **ring):
    """The backward-data descriptor of one phase (an entry of pc.dg): the stride-1 conv of dy with
    the phase's flipped image into dx's pixels (py + st * i, px + st * j).  ``shift`` = p: the
    interior of a reflect-padded layer (the image is packed for the padded domain).  ``dtype``:
    dy's, when it is not pc's (the e4m3 copy).  ``ring``: fields replaced afterwards -- the
    split-K ring descriptors of the fp32 path, off the hot path."""
    (py, _, ay, c0y), (px, _, ax, c0x), _ = phase
    s, st = pc.spec, pc.spec.stride
    (N, H, W, ldx), (_, OH, OW, ldy) = dy.t.shape, dx.t.shape
    d = _desc(N=N, H=H, W=W, Cin=pc.cout_eff, ldx=ldx, xoff=dy.off, Ho=-(-(OH - py) // st),
              Wo=-(-(OW - px) // st), Cout=s.cin, ldy=ldy, yoff=dx.off, OH=OH, OW=OW, omy=st, ooy=py, omx=st,
              oox=px, KH=ay, KW=ax, sy=1, sx=1, c0y=c0y + shift, c0x=c0x + shift, pad_mode=PAD_ZERO, act=0,
              accumulate=int(accumulate), dtype=pc.dtype if dtype is None else dtype, out_dtype=dx.dt,
              mask_act=mask_act, ldm=mask.ld if mask else 0, moff=mask.off if mask else 0,
              cin_real=s.cout if s.cout < pc.cout_eff else 0)
    for k, v in ring.items():
        setattr(d, k, v)
    return d


IRGAN_EUNSUPPORTED = 1002   # include/irgan.h


def _try(name, *args) -> bool:
    """Call entry point ``name``.  IRGAN_EUNSUPPORTED means the library does not take the
    arguments and NOTHING ran: False, and the caller takes its other path.  Any other non-zero
    code raises IrganError naming the entry point."""
    rc = getattr(_lib.load(), name)(*args)
    if rc == IRGAN_EUNSUPPORTED:
        return False
    if rc != 0:
        raise _lib.IrganError(f"{name} failed with code {rc}")
    return True


def _rup(a, b):
    return (a + b - 1) // b * b


def weight_pack(master: torch.Tensor, dst: torch.Tensor, cout, kh, kw, cin, transpose=0, s=1, tyr=0, ay=0,
                txr=0, ax=0, cpad=0, kalign=1):
    _lib.call("irgan_weight_pack", P(master), P(dst), dt_code(dst), cout, kh, kw, cin, transpose, s, tyr, ay, txr,
              ax, cpad, kalign, stream())


def eff_channels(c, dtype):
    """Channel count a conv input is stored with: bf16 narrow inputs (1/3/4 ch)
    are zero-padded to 8 so the LDS-DMA kernel reads 16-byte chunks."""
    return 8 if (dtype == BF16 and c < 8) else c


class PackedConv:
    """Per-layer packed weights: forward (cast) and backward-data (flipped /
    per-phase) images in the compute dtype, refreshed after each optimizer step.
    bf16 rows are [taps][channels] zero-padded to a multiple of 64 (the K-tile)."""

    def __init__(self, spec: ConvSpec, master: torch.Tensor, bias: torch.Tensor | None, dtype: int,
                 need_dgrad=True, reflect_dgrad=None):
        self.spec, self.master, self.bias, self.dtype = spec, master, bias, dtype
        dev = master.device
        tdt = TORCH_DT[dtype]
        k = spec.k
        self.cin_eff = eff_channels(spec.cin, dtype)     # forward input channels as stored
        self.cout_eff = eff_channels(spec.cout, dtype)   # backward-data input (dY) channels as stored
        self.kalign = 64 if dtype == BF16 else 1
        kf = _rup(k * k * self.cin_eff, self.kalign)
        self.fwd = master if dtype == F32 else torch.empty(spec.cout * kf, dtype=tdt, device=dev)
        self.reflect = spec.mode == PAD_REFLECT if reflect_dgrad is None else reflect_dgrad
        self.dg = []
        if need_dgrad:
            for (py, tyr, ay, c0y) in spec.phases(self.reflect):
                for (px, txr, ax, c0x) in spec.phases(self.reflect):
                    kd = _rup(ay * ax * self.cout_eff, self.kalign)
                    buf = torch.empty(spec.cin * kd, dtype=tdt, device=dev)
                    self.dg.append(((py, tyr, ay, c0y), (px, txr, ax, c0x), buf))

    def jobs(self):
        """The weight_pack jobs of this layer as irgan_pack_desc records."""
        s, out = self.spec, []
        if self.dtype != F32:
            out.append(PackDesc(self.master.data_ptr(), self.fwd.data_ptr(), dt_code(self.fwd), s.cout, s.k, s.k,
                                s.cin, 0, 1, 0, 0, 0, 0, self.cin_eff, self.kalign, 0))
        for (py, tyr, ay, _), (px, txr, ax, _), buf in self.dg:
            out.append(PackDesc(self.master.data_ptr(), buf.data_ptr(), dt_code(buf), s.cout, s.k, s.k, s.cin, 1,
                                s.stride, tyr, ay, txr, ax, self.cout_eff, self.kalign, 0))
        return out

    def pack(self):
        s = self.spec
        if self.dtype != F32:
            weight_pack(self.master, self.fwd, s.cout, s.k, s.k, s.cin, cpad=self.cin_eff, kalign=self.kalign)
        for (py, tyr, ay, _), (px, txr, ax, _), buf in self.dg:
            weight_pack(self.master, buf, s.cout, s.k, s.k, s.cin, 1, s.stride, tyr, ay, txr, ax,
                        cpad=self.cout_eff, kalign=self.kalign)


class PackDesc(ctypes.Structure):
    """irgan_pack_desc (include/irgan.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p)] + [
        (n, ctypes.c_int32) for n in "dtype Cout KH KW Cin transpose s tyr Ay txr Ax cpad kalign reserved".split()]


class PackBatch:
    """All re-pack jobs of a set of layers as ONE irgan_weight_pack_batch launch.
    The descriptor table lives on the device; it is rebuilt only if a packed
    buffer moved (buffers are allocated once, so normally never)."""

    def __init__(self, packs):
        self.packs = list(packs)
        self.key, self.table, self.n = None, None, 0

    def run(self):
        jobs = [j for p in self.packs for j in p.jobs()]
        key = tuple((j.src, j.dst) for j in jobs)
        if key != self.key:
            arr = (PackDesc * len(jobs))(*jobs)
            raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
            self.table = raw.to(self.packs[0].master.device)
            self.key, self.n = key, len(jobs)
        if self.n:
            _lib.call("irgan_weight_pack_batch", P(self.table), self.n, stream())


def conv_fwd(pc: PackedConv, x: Feat, y: Feat, act=ACT_NONE, bias=True, accumulate=False, mask: Feat = None,
             mask_act=0):
    s = pc.spec
    assert y.C == s.cout and x.C == pc.cin_eff, "conv_fwd shape mismatch"
    d = _fwd_desc(s, x, y, pc.cin_eff, pc.dtype, y.dt, act, accumulate, mask_act=mask_act,
                  ldm=mask.ld if mask else 0, moff=mask.off if mask else 0,
                  cin_real=s.cin if s.cin < pc.cin_eff else 0)
    assert x.dt == pc.dtype
    TIMER.wrap(conv_tag("fwd", s, (x.H, x.W), x.N), lambda: _lib.call(
        "irgan_conv_fwd", ctypes.byref(d), x.ptr, P(pc.fwd), P(pc.bias if bias else None), y.ptr,
        mask.ptr if mask else None, stream()))


def conv_fwd_pool(pc: PackedConv, x: Feat, y, yp: Feat, act=ACT_RELU) -> bool:
    """y = act(conv(x)) (y: a Feat, or None when only the pooled map is needed) and yp = its
    2x2 max-pool, in one launch (irgan_conv_fwd_pool: the VGG conv1_2 -> MaxPool2d(2),
    ir:664).  False when the layer has no fused kernel -- then NOTHING ran."""
    s = pc.spec
    Ho, Wo = s.out_hw(x.H, x.W)
    if pc.dtype != BF16 or yp.dt != BF16 or yp.off or yp.ld != s.cout or Ho % 2 or Wo % 2:
        return False
    assert (yp.N, yp.H, yp.W, yp.C) == (x.N, Ho // 2, Wo // 2, s.cout) and x.C == pc.cin_eff
    if y is not None:
        assert (y.H, y.W, y.C, y.N, y.dt) == (Ho, Wo, s.cout, x.N, BF16)
    # no full-size y: the descriptor carries a dense one's ld / off, which are yp's (checked above)
    d = _fwd_desc(s, x, y if y is not None else yp, pc.cin_eff, pc.dtype, BF16, act, y_sized=y is not None)
    return TIMER.wrap(conv_tag("fwdpool", s, (x.H, x.W), x.N), lambda: _try(
        "irgan_conv_fwd_pool", ctypes.byref(d), x.ptr, P(pc.fwd), P(pc.bias), y.ptr if y is not None else None,
        yp.ptr, stream()))


def conv_fwd_stats(pc: PackedConv, x: Feat, y: Feat, part: torch.Tensor) -> int:
    """conv_fwd (no activation) that also writes y's InstanceNorm partials into
    ``part`` (irgan_conv_fwd_stats).  Returns the partials per image, or 0 when the
    layer has no fused kernel -- then NOTHING ran and the caller does conv_fwd +
    in_stats."""
    s = pc.spec
    if pc.dtype != BF16 or y.dt != BF16 or s.cout % 64 or s.cout == 192 or (s.stride != 1 and s.k != 4):
        return 0
    assert y.C == s.cout and x.C == pc.cin_eff, "conv_fwd shape mismatch"
    d = _fwd_desc(s, x, y, pc.cin_eff, pc.dtype, y.dt, cin_real=s.cin if s.cin < pc.cin_eff else 0)
    nb = ctypes.c_int32(0)
    ran = TIMER.wrap(conv_tag("fwd", s, (x.H, x.W), x.N), lambda: _try(
        "irgan_conv_fwd_stats", ctypes.byref(d), x.ptr, P(pc.fwd), P(pc.bias), y.ptr, P(part), ctypes.byref(nb),
        stream()))
    return int(nb.value) if ran else 0


# D's last layer (4x4, stride 1, pad 1, one output channel) on the dedicated VALU kernels
# (csrc/head.hip); IRGAN_NO_PATCH_HEAD=1 runs it on the generic conv kernels
PATCH_HEAD = [os.environ.get("IRGAN_NO_PATCH_HEAD") != "1"]


def is_patch_head(pc: PackedConv, x: Feat) -> bool:
    s = pc.spec
    return (PATCH_HEAD[0] and pc.dtype == BF16 and x.dt == BF16 and s.cout == 1 and s.k == 4 and s.stride == 1
            and s.pad == 1 and s.mode == PAD_ZERO and s.cin == x.C == 512)


def patch_head_fwd(pc: PackedConv, x: Feat, y: torch.Tensor) -> bool:
    """y (fp32 [N][H-1][W-1][1]) = the PatchGAN head conv of x + bias (irgan_patch_head_fwd);
    False (nothing launched) where the dedicated kernel does not take the layer."""
    if not is_patch_head(pc, x):
        return False
    assert y.dtype == torch.float32 and tuple(y.shape) == (x.N, x.H - 1, x.W - 1, 1) and y.is_contiguous()

    ws = _wgrad_ws(y.device)   # the per-pixel tap products; consumed by the same stream's next launch

    return TIMER.wrap(conv_tag("fwd", pc.spec, (x.H, x.W), x.N), lambda: _try(
        "irgan_patch_head_fwd", x.ptr, x.N, x.H, x.W, x.C, x.ld, x.off, P(pc.fwd),
        P(pc.bias) if pc.bias is not None else None, P(y), P(ws), ws.numel(), stream()))


def patch_head_dgrad(pc: PackedConv, g: torch.Tensor, dx: Feat) -> bool:
    """dx (bf16, written) = the PatchGAN head's backward-data of g = dL/dy (fp32 [N][H-1][W-1][1])
    (irgan_patch_head_dgrad); False (nothing launched) where the kernel does not take the layer."""
    if not is_patch_head(pc, dx):
        return False
    assert g.dtype == torch.float32 and tuple(g.shape[:3]) == (dx.N, dx.H - 1, dx.W - 1) and g.is_contiguous()
    return TIMER.wrap(conv_tag("dgrad", pc.spec, (dx.H, dx.W), dx.N), lambda: _try(
        "irgan_patch_head_dgrad", P(g), g.shape[3], P(pc.fwd), dx.ptr, dx.N, dx.H, dx.W, dx.C, dx.ld, dx.off,
        stream()))


def patch_head_wgrad(pc: PackedConv, x: Feat, g: torch.Tensor, dw: torch.Tensor) -> bool:
    """dw (fp32 KRSC view, accumulated) += the PatchGAN head's weight gradient from x and
    g = dL/dy (fp32 [N][H-1][W-1][1]) (irgan_patch_head_wgrad: block partials in the wgrad
    workspace, ordered reduce); False (nothing launched) where the kernel does not take it."""
    if not is_patch_head(pc, x):
        return False
    assert g.dtype == torch.float32 and tuple(g.shape[:3]) == (x.N, x.H - 1, x.W - 1) and g.is_contiguous()
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == 16 * x.C
    ws = _wgrad_ws(dw.device)
    return TIMER.wrap(conv_tag("wgrad", pc.spec, (x.H, x.W), x.N), lambda: _try(
        "irgan_patch_head_wgrad", x.ptr, x.N, x.H, x.W, x.C, x.ld, x.off, P(g), g.shape[3], P(dw), P(ws),
        ws.numel(), stream()))


def conv_dgrad(pc: PackedConv, dy: Feat, dx: Feat, accumulate=False, mask: Feat = None, mask_act=0,
               pad_buf: torch.Tensor = None, bias=False):
    """dx = d(conv)/dx^T dy.  Reflect-padded layers: _dgrad_reflect; stride-2 layers launch per
    phase (or all four phases in one irgan_conv_dgrad_s2 launch)."""
    s = pc.spec
    assert dy.C == pc.cout_eff and dx.C == s.cin and dy.dt == pc.dtype
    if pc.reflect:
        assert mask is None
        _dgrad_reflect(pc, dy, dx, accumulate, pad_buf)
        return

    def phases():
        if s.stride == 2 and len(pc.dg) == 4 and pc.dtype == BF16 and not bias and _dgrad_s2(pc, dy, dx, accumulate,
                                                                                              mask, mask_act):
            return   # all four phases in one launch (irgan_conv_dgrad_s2)
        for ph in pc.dg:
            d = _dgrad_desc(pc, ph, dy, dx, accumulate, mask=mask, mask_act=mask_act)
            if d.Ho <= 0 or d.Wo <= 0:
                continue
            assert d.KH > 0 and d.KW > 0
            _lib.call("irgan_conv_fwd", ctypes.byref(d), dy.ptr, P(ph[2]), P(pc.bias if bias else None), dx.ptr,
                      mask.ptr if mask else None, stream())
    TIMER.wrap(conv_tag("dgrad", s, (dx.H, dx.W), dx.N), phases)


def _dgrad_reflect(pc: PackedConv, dy: Feat, dx: Feat, accumulate, pad_buf=None, f8=None):
    """Backward-data of a reflect-padded layer over the padded domain (Hp x Wp) folded back: the
    interior u in [p, H+p) maps 1:1 onto dx and is written there directly; only the ring of width
    p is computed separately and folded onto dx's border band.  bf16 ResnetBlock shapes: the
    ring's line GEMM, then the interior launch whose store pass adds the ring terms
    (irgan_conv_dgrad_reflect_line[_fp8]); other bf16 shapes: the interior launch, then the ring
    (irgan_reflect_dgrad_ring_ws); fp32: split-K ring partials in pad_buf (fp32 scratch) folded
    by irgan_reflect_ring_fold.  f8 = (wd8, dqw, dy8, dqx): the interior on the e4m3 copies of
    the flipped image and of dy (conv_dgrad_fp8); the ring stays on the bf16 dy."""
    s, p, H, W = pc.spec, pc.spec.pad, dx.H, dx.W
    ph = pc.dg[0]
    (_, _, ay, c0y), (_, _, ax, c0x), buf = ph
    d = _dgrad_desc(pc, ph, dy, dx, accumulate, shift=p)
    if f8 is not None:
        wd8, dqw, dy8, dqx = f8
        d8 = _dgrad_desc(pc, ph, dy8, dx, accumulate, dtype=FP8, shift=p)
        ring_mfma = p > 0
    else:
        ring_mfma = (p > 0 and pc.dtype == BF16 and pc.cout_eff % 32 == 0 and H >= 2 * p + 2
                     and W >= 2 * p + 2 and dy.ld % 8 == 0 and dy.off % 8 == 0)

    def launch():
        if ring_mfma and RING_LINE[0] and RING_EPI[0] and (f8 is not None or dx.dt == BF16):
            # line GEMM, then the interior with the ring folded into its store pass
            ws = _ring_ws(dx.t.device, dx.N * 4 * 68 * dx.C)
            if f8 is None:
                ran = _try("irgan_conv_dgrad_reflect_line", ctypes.byref(d), dy.ptr, P(buf), p, dx.ptr, P(ws),
                           ws.numel(), stream())
            else:
                ran = _try("irgan_conv_dgrad_reflect_line_fp8", ctypes.byref(d), dy.ptr, P(buf), ctypes.byref(d8),
                           dy8.ptr, P(wd8), dqx, dqw, p, dx.ptr, P(ws), ws.numel(), stream())
            if ran:
                return
        if f8 is None:
            _lib.call("irgan_conv_fwd", ctypes.byref(d), dy.ptr, P(buf), None, dx.ptr, None, stream())
        else:
            _lib.call("irgan_conv_fwd_fp8", ctypes.byref(d8), dy8.ptr, P(wd8), dqx, dqw, None, dx.ptr, None,
                      ctypes.byref(ctypes.c_int32(0)), stream())
        if ring_mfma:
            _ring(d, dy, buf, p, dx)

    TIMER.wrap(conv_tag("dgrad" if f8 is None else "dgrad8", s, (H, W), dx.N), launch)
    if p == 0 or ring_mfma:
        return
    # ring in split-K partials: rows[ks][N][2p][Wp][C], cols[ks][N][H][2p][C]
    Wp = W + 2 * p
    rsz, csz = dx.N * 2 * p * Wp * s.cin, dx.N * H * 2 * p * s.cin
    nk = -(-(ay * ax * pc.cout_eff) // 64)
    ksplit = 1 if pc.dtype == F32 else max(1, min(nk // 2, 16))
    assert pad_buf is not None
    ksplit = max(1, min(ksplit, pad_buf.numel() // (rsz + csz)))
    rows_b = pad_buf[:ksplit * rsz]
    cols_b = pad_buf[ksplit * rsz:ksplit * (rsz + csz)]
    ring = dict(ldy=s.cin, yoff=0, out_dtype=F32)
    for k in range(p):
        # padded rows k and H+p+k (full width) -> compact rows k, p+k
        dr = _dgrad_desc(pc, ph, dy, dx, 0, **ring, Ho=2, Wo=Wp, OH=2 * p, OW=Wp, omy=p, ooy=k, omx=1, oox=0,
                         sy=H + p, sx=1, c0y=c0y + k, c0x=c0x)
        _lib.call("irgan_conv_fwd_splitk", ctypes.byref(dr), dy.ptr, P(buf), P(rows_b), ksplit, rsz, stream())
        # padded columns k and W+p+k of the interior rows -> compact columns k, p+k
        dcl = _dgrad_desc(pc, ph, dy, dx, 0, **ring, Ho=H, Wo=2, OH=H, OW=2 * p, omy=1, ooy=0, omx=p, oox=k, sy=1,
                          sx=W + p, c0y=c0y + p, c0x=c0x + k)
        _lib.call("irgan_conv_fwd_splitk", ctypes.byref(dcl), dy.ptr, P(buf), P(cols_b), ksplit, csz, stream())
    _lib.call("irgan_reflect_ring_fold", P(rows_b), P(cols_b), ksplit, dx.N, H, W, s.cin, p, dx.ptr, dx.dt,
              dx.ld, dx.off, stream())


def _dgrad_s2(pc: PackedConv, dy: Feat, dx: Feat, accumulate, mask, mask_act) -> bool:
    """The four phase launches of a 4x4 stride-2 backward-data as one irgan_conv_dgrad_s2
    launch; False (nothing ran) when the library does not take the shapes."""
    descs, ws = (_lib.ConvDesc * 4)(), (ctypes.c_void_p * 4)()
    for k, ph in enumerate(pc.dg):
        descs[k] = _dgrad_desc(pc, ph, dy, dx, accumulate, mask=mask, mask_act=mask_act)
        ws[k] = ph[2].data_ptr()
    return _try("irgan_conv_dgrad_s2", descs, dy.ptr, ws, dx.ptr, mask.ptr if mask else None, stream())


def conv_wgrad(spec: ConvSpec, x: Feat, dy: Feat, dw: torch.Tensor, dtype: int, splitk=0):
    """dw (fp32 KRSC view, accumulated) += weight gradient of conv(x) given dy."""
    assert dy.C == spec.cout and x.C >= spec.cin
    assert x.dt == dtype and dy.dt == dtype and dw.dtype == torch.float32
    d = _fwd_desc(spec, x, dy, spec.cin, dtype, F32, accumulate=1, flags=CONV_DETERMINISTIC if _DET[0] else 0)
    ws = _wgrad_ws(dw.device) if dtype == BF16 else None
    TIMER.wrap(conv_tag("wgrad", spec, (x.H, x.W), x.N), lambda: _lib.call(
        "irgan_conv_wgrad_ws", ctypes.byref(d), x.ptr, dy.ptr, P(dw), splitk, P(ws), 0 if ws is None else ws.numel(),
        stream()))


WGRAD_GROUP_MAX = 4   # W2_GROUP_MAX (csrc/conv_wgrad_pc.hip)
# ResnetBlock weight gradients per grouped launch in GeneratorEngine.backward; 0: per-layer
# launches (IRGAN_NO_WGRAD_GROUP=1, the A/B switch).  4: the fastest of 2, 3, 4 in the 256^2
# B = 16 step and per layer (profiles/wgrad_group.txt)
WGRAD_GROUP = [0 if os.environ.get("IRGAN_NO_WGRAD_GROUP") else 4]


def set_wgrad_group(n: int) -> int:
    """Group size of the deferred ResnetBlock weight gradients (0: per-layer launches).
    Returns the previous setting."""
    assert 0 <= n <= WGRAD_GROUP_MAX
    old, WGRAD_GROUP[0] = WGRAD_GROUP[0], int(n)
    return old


def conv_wgrad_group(spec: ConvSpec, xs, dys, dws, dtype: int, ws: torch.Tensor = None) -> bool:
    """dws[i] += weight gradient of conv(xs[i]) given dys[i], all of one shape and slicing, in
    one launch and one ordered reduce (irgan_conv_wgrad_group).  False: the library does not
    take the group (shape, dtype, count, workspace) and NOTHING ran.  ``ws``: the split-K slab
    (default: the stream's wgrad workspace).  Out of deterministic mode each problem is split
    1 / n as many ways as alone (fewer fp32 partials per element); in it every problem keeps its
    own splits, so each dw is conv_wgrad's bit for bit whatever n."""
    n = len(xs)
    assert n == len(dys) == len(dws) and n >= 1
    x, dy = xs[0], dys[0]
    for a, b, dw in zip(xs, dys, dws):
        assert a.t.shape == x.t.shape and a.off == x.off and b.t.shape == dy.t.shape and b.off == dy.off
        assert b.C == spec.cout and a.C >= spec.cin and a.dt == dtype and b.dt == dtype and dw.dtype == torch.float32
    d = _fwd_desc(spec, x, dy, spec.cin, dtype, F32, accumulate=1, flags=CONV_DETERMINISTIC if _DET[0] else 0)
    if ws is None:
        ws = _wgrad_ws(dws[0].device)
    arr = ctypes.c_void_p * n
    px, pdy, pdw = arr(*(a.t.data_ptr() for a in xs)), arr(*(b.t.data_ptr() for b in dys)), \
        arr(*(w.data_ptr() for w in dws))
    return TIMER.wrap(conv_tag("wgrad", spec, (x.H, x.W), x.N), lambda: _try(
        "irgan_conv_wgrad_group", ctypes.byref(d), n, px, pdy, pdw, P(ws), ws.numel(), stream()), count=n)


WGRAD_WS_FLOATS = 24 << 20  # split-K slab workspace (96 MB): >= slots x tile for every layer of the step
_WGRAD_WS = {}


def _wgrad_ws(dev):
    """Per-(device, stream) fp32 workspace for the wgrad split-K partials
    (irgan_conv_wgrad_ws): plain-store slabs + an ordered reduce instead of fp32
    atomics into dw.  One per stream, so concurrent streams never share it."""
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    w = _WGRAD_WS.get(key)
    if w is None:
        w = _WGRAD_WS[key] = torch.empty(WGRAD_WS_FLOATS, dtype=torch.float32, device=dev)
    return w


# ----------------------------------------------------------------------------
# instance norm / reductions
# ----------------------------------------------------------------------------

def in_stats(x: Feat, work: torch.Tensor, mr: torch.Tensor):
    """{mean, rstd} of x: partial-sum launch + fixed-order finalize launch."""
    _lib.call("irgan_in_stats", x.ptr, x.dt, x.N, x.H * x.W, x.C, x.ld, x.off, P(work), P(mr), stream())


def in_finalize(x: Feat, part: torch.Tensor, nb: int, mr: torch.Tensor):
    """{mean, rstd} of x from the nb per-image partials irgan_conv_fwd_stats wrote."""
    _lib.call("irgan_in_finalize", P(part), x.N, x.H * x.W, x.C, nb, P(mr), stream())


def in_apply(x: Feat, mr, y: Feat, act=ACT_NONE, res: Feat = None, xhat: torch.Tensor = None, q8=None):
    """y = act(IN(x)) [+ res].  q8 = (y8 Feat, q ptr, amax ptr): also the fp8 copy of y
    (irgan_in_apply_fp8; bf16, no xhat).  The amax pointer may be None (nothing recorded), and
    then, without a residual, so may y: the e4m3 copy alone, for a forward whose bf16 y nobody
    reads."""
    assert y is not None or (q8 is not None and q8[2] is None and res is None)
    assert y is None or x.dt == y.dt
    if q8 is not None:
        y8, qp, ap = q8
        assert xhat is None and x.dt == BF16 and y8.dt == FP8 and (y8.N, y8.H, y8.W, y8.C) == (x.N, x.H, x.W, x.C)
        assert y is None or (y.N, y.H, y.W, y.C) == (x.N, x.H, x.W, x.C)
        kind = "in_apply8_res" if res is not None else ("in_apply8" if y is not None else "in_apply8_only")
        _timed(kind, x, lambda: _lib.call(
            "irgan_in_apply_fp8", x.ptr, x.N, x.H * x.W, x.C, x.ld, x.off, P(mr), act,
            res.ptr if res else None, res.ld if res else 0, res.off if res else 0,
            y.ptr if y is not None else None, y.ld if y is not None else 0, y.off if y is not None else 0,
            y8.ptr, y8.ld, y8.off, qp, ap, stream()))
        return
    _timed("in_apply_res" if res is not None else "in_apply", x, lambda: _lib.call(
        "irgan_in_apply", x.ptr, x.dt, x.N, x.H * x.W, x.C, x.ld, x.off, P(mr), act, res.ptr if res else None,
        res.ld if res else 0, res.off if res else 0, y.ptr, y.ld, y.off, P(xhat), stream()))


def in_bwd_parts(dy: Feat, x: Feat, act: int, mr, work, red, dx: Feat, db=None, dy2: Feat = None, q8=None):
    """(reduce, apply) launch closures of in_backward (also used for per-pass timing).
    q8 = (y8 Feat, q ptr, amax ptr): the apply also writes the fp8 copy of dx."""
    N, HW, C = x.N, x.H * x.W, x.C
    d2 = (dy2.ptr, dy2.dt, dy2.ld, dy2.off) if dy2 is not None else (None, 0, 0, 0)

    def reduce():
        _lib.call("irgan_in_bwd_reduce", dy.ptr, dy.dt, dy.ld, dy.off, *d2, x.ptr, x.dt, x.ld, x.off, act, N, HW, C,
                  P(mr), P(work), P(red), stream())

    def apply():
        if q8 is not None:
            y8, qp, ap = q8
            assert db is None and y8.dt == FP8 and dx.dt == BF16 and (y8.N, y8.H, y8.W, y8.C) == (dx.N, dx.H, dx.W, C)
            _lib.call("irgan_in_bwd_apply_fp8", dy.ptr, dy.ld, dy.off, d2[0], d2[2], d2[3], x.ptr, x.ld, x.off, act,
                      N, HW, C, P(mr), P(red), dx.ptr, dx.ld, dx.off, y8.ptr, y8.ld, y8.off, qp, ap, stream())
            return
        _lib.call("irgan_in_bwd_apply", dy.ptr, dy.dt, dy.ld, dy.off, *d2, x.ptr, x.dt, x.ld, x.off, act, N, HW, C,
                  P(mr), P(red), dx.ptr, dx.dt, dx.ld, dx.off, P(db), stream())
    return reduce, apply


IN_ONEPASS_CG = _lib.header_enum("IRGAN_IN_ONEPASS_CG")        # channels per workgroup
IN_ONEPASS_ELEMS = _lib.header_enum("IRGAN_IN_ONEPASS_ELEMS")  # elements of one workgroup's slice
# the one-pass InstanceNorm backward where it is legal and fills the chip;
# IRGAN_IN_BWD_ONEPASS=0: always reduce + finalize + apply (the A/B switch)
IN_BWD_ONEPASS = [os.environ.get("IRGAN_IN_BWD_ONEPASS") != "0"]
_CUS = {}


def _cu_count(dev) -> int:
    c = _CUS.get(dev)
    if c is None:
        c = _CUS[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return c


def in_bwd_onepass_legal(N, HW, C, dts, lds, has_db=False, has_dy2=False) -> bool:
    """What irgan_in_bwd_onepass accepts: dts the dtype codes of dy, x and dx, lds every
    ld and off of theirs."""
    return (all(d == BF16 for d in dts) and not has_db and not has_dy2 and C % IN_ONEPASS_CG == 0
            and HW * IN_ONEPASS_CG <= IN_ONEPASS_ELEMS and all(v % 8 == 0 for v in lds))


def in_bwd_use_onepass(N, HW, C, dts, lds, cus, has_db=False, has_dy2=False, q8=None) -> bool:
    """in_backward's choice between the one-pass kernel and the three row-split launches:
    one-pass when it is legal and its N * C / CG workgroups are at least half the CUs (below
    that the row-split passes fill the chip better).  q8 has no say: the fp8 side output
    stays the same bf16 dx plus its copy."""
    del q8
    return (IN_BWD_ONEPASS[0] and in_bwd_onepass_legal(N, HW, C, dts, lds, has_db, has_dy2)
            and 2 * N * (C // IN_ONEPASS_CG) >= cus)


def in_bwd_onepass(dy: Feat, x: Feat, act: int, mr, red, dx: Feat, dy2: Feat = None, q8=None) -> bool:
    """in_backward in one launch (irgan_in_bwd_onepass[_fp8]): red is an output.  False when
    the library does not support the arguments -- then NOTHING ran and nothing was written."""
    N, HW, C = x.N, x.H * x.W, x.C
    d2 = (dy2.ptr, dy2.dt, dy2.ld, dy2.off) if dy2 is not None else (None, 0, 0, 0)
    if q8 is None:
        return _try("irgan_in_bwd_onepass", dy.ptr, dy.dt, dy.ld, dy.off, *d2, x.ptr, x.dt, x.ld, x.off, act, N, HW,
                    C, P(mr), P(red), dx.ptr, dx.dt, dx.ld, dx.off, stream())
    y8, qp, ap = q8
    if not (dy.dt == x.dt == dx.dt == BF16 and (dy2 is None or dy2.dt == BF16)):
        return False
    assert y8.dt == FP8 and (y8.N, y8.H, y8.W, y8.C) == (dx.N, dx.H, dx.W, C)
    return _try("irgan_in_bwd_onepass_fp8", dy.ptr, dy.ld, dy.off, d2[0], d2[2], d2[3], x.ptr, x.ld, x.off, act, N,
                HW, C, P(mr), P(red), dx.ptr, dx.ld, dx.off, y8.ptr, y8.ld, y8.off, qp, ap, stream())


def in_backward(dy: Feat, x: Feat, act: int, mr, work, red, dx: Feat, db=None, dy2: Feat = None, q8=None):
    """dx = backward of act(IN(x)) applied to (dy [+ dy2]); x = PRE-norm input."""
    if in_bwd_use_onepass(x.N, x.H * x.W, x.C, (dy.dt, x.dt, dx.dt), (dy.ld, dy.off, x.ld, x.off, dx.ld, dx.off),
                          _cu_count(x.t.device), db is not None, dy2 is not None, q8):
        # 6 B per element: the in_bwd_apply roofline line.  The library still refuses where the
        # reduce pass's row partition does not fit its threads (batches of several hundred
        # images, C >= 2048): nothing ran, and the three launches below take over
        if _timed("in_bwd_apply", x, lambda: in_bwd_onepass(dy, x, act, mr, red, dx, q8=q8)):
            return
    reduce, apply = in_bwd_parts(dy, x, act, mr, work, red, dx, db, dy2, q8)
    _timed("in_bwd_reduce", x, reduce)
    _timed("in_bwd_apply", x, apply)


_CS_WORK = {}


def channel_sum(g: Feat, db: torch.Tensor):
    key = (db.device, g.C, torch.cuda.current_stream(db.device).cuda_stream)
    w = _CS_WORK.get(key)
    if w is None:
        w = _CS_WORK[key] = torch.empty(16 * IN_PARTS * g.C, dtype=torch.float64, device=db.device)
    _lib.call("irgan_channel_sum", g.ptr, g.dt, g.P, g.C, g.ld, g.off, P(db), P(w), stream())


# ----------------------------------------------------------------------------
# batch norm (csrc/batchnorm.hip): per-channel statistics over groups of samples
# ----------------------------------------------------------------------------

NORM_AFFINE = _lib.header_enum("IRGAN_NORM_AFFINE")   # OR-ed into act: the table is BatchNorm's {shift, scale}
BN_TABLE = _lib.header_enum("IRGAN_BN_TABLE")         # floats per (n, c) of the statistics table
BN_EPS, BN_MOMENTUM = 1e-5, 0.1                       # nn.BatchNorm2d's defaults (ir:158-159)


def bn_stats(x: Feat, work: torch.Tensor, mr: torch.Tensor, groups=1, gamma=None, beta=None, running_mean=None,
             running_var=None, repeat=1, ab=None, nb=0):
    """Training-mode statistics of x per (group, channel): mr[n][c] = {mean, rstd, mean_lo, 0}
    (BN_TABLE floats; each sample carries its group's entry) and, with ``ab``, the {shift, scale} table of the fused resample
    consumers.  nb > 0: ``work`` already holds nb {sum, sum of squares} partials per image
    (conv_fwd_stats); else a statistics pass over x runs first.  running_mean / running_var
    (optional) are updated in place, group after group, each ``repeat`` times."""
    assert x.N % groups == 0 and repeat >= 1
    if nb:
        _lib.call("irgan_bn_finalize", P(work), x.N, x.H * x.W, x.C, nb, groups, P(gamma), P(beta), P(running_mean),
                  P(running_var), BN_MOMENTUM, BN_EPS, repeat, P(mr), P(ab), stream())
    else:
        _lib.call("irgan_bn_stats", x.ptr, x.dt, x.N, x.H * x.W, x.C, x.ld, x.off, groups, P(gamma), P(beta),
                  P(running_mean), P(running_var), BN_MOMENTUM, BN_EPS, repeat, P(work), P(mr), P(ab), stream())


def bn_eval_table(running_mean, running_var, gamma, beta, N: int, mr: torch.Tensor, ab=None):
    """Eval mode: the mr (and ab) tables of N samples from the running statistics."""
    _lib.call("irgan_bn_eval_table", P(running_mean), P(running_var), P(gamma), P(beta), N, running_mean.numel(),
              BN_EPS, P(mr), P(ab), stream())


def bn_apply(x: Feat, mr, gamma, beta, y: Feat, act=ACT_NONE, res: Feat = None):
    """y = act(gamma * (x - mean) * rstd + beta) [+ res]."""
    assert x.dt == y.dt and (res is None or res.dt == x.dt)
    _lib.call("irgan_bn_apply", x.ptr, x.dt, x.N, x.H * x.W, x.C, x.ld, x.off, P(mr), P(gamma), P(beta), act,
              res.ptr if res else None, res.ld if res else 0, res.off if res else 0, y.ptr, y.ld, y.off, stream())


def bn_backward(dy: Feat, x: Feat, act: int, mr, gamma, beta, work, red, dx: Feat, dgamma=None, dbeta=None, groups=1,
                eval_mode=False, dy2: Feat = None):
    """dx = backward of act(BN(x)) applied to (dy [+ dy2]); x = PRE-norm input; dgamma / dbeta
    (fp32, optional) are accumulated.  eval_mode: mr holds the running statistics."""
    d2 = (dy2.ptr, dy2.dt, dy2.ld, dy2.off) if dy2 is not None else (None, 0, 0, 0)
    _lib.call("irgan_bn_backward", dy.ptr, dy.dt, dy.ld, dy.off, *d2, x.ptr, x.dt, x.ld, x.off, act, x.N, x.H * x.W,
              x.C, groups, int(eval_mode), P(mr), P(gamma), P(beta), P(work), P(red), dx.ptr, dx.dt, dx.ld, dx.off,
              P(dgamma), P(dbeta), stream())


# SyncBN: the passes above cut into a local half (fp64 sums) and a finishing half (from the sums
# the caller has all-reduced).  One buffer per pass: sums[G][C][2] then cnt[G] doubles.

def bn_sync_numel(groups: int, C: int) -> int:
    """Doubles of a SyncBN sums buffer: {sum, sum} per (group, channel) + the count per group."""
    return groups * (2 * C + 1)


def bn_sync_sums(x: Feat, work: torch.Tensor, sums: torch.Tensor, groups=1, nb=0):
    """Forward, local half: sums[g][c] = {sum x, sum x^2} over the local samples of group g and
    cnt[g] = their element count.  nb > 0: ``work`` holds nb conv-epilogue partials per image."""
    assert x.N % groups == 0 and sums.dtype == torch.float64 and sums.numel() >= bn_sync_numel(groups, x.C)
    _lib.call("irgan_bn_sync_sums", x.ptr, x.dt, x.N, x.H * x.W, x.C, x.ld, x.off, groups, nb, P(work), P(sums),
              stream())


def bn_sync_finalize(sums: torch.Tensor, N: int, C: int, mr: torch.Tensor, groups=1, gamma=None, beta=None,
                     running_mean=None, running_var=None, repeat=1, ab=None):
    """Forward, finishing half, from the REDUCED sums: the tables of the N local samples and the
    running update with the global mean / unbiased variance (bn_stats' arguments)."""
    assert N % groups == 0 and repeat >= 1 and sums.dtype == torch.float64 and sums.numel() >= bn_sync_numel(groups, C)
    _lib.call("irgan_bn_sync_finalize", P(sums), N, C, groups, P(gamma), P(beta), P(running_mean), P(running_var),
              BN_MOMENTUM, BN_EPS, repeat, P(mr), P(ab), stream())


def bn_sync_backward_sums(dy: Feat, x: Feat, act: int, mr, gamma, beta, work, bsums: torch.Tensor, dgamma=None,
                          dbeta=None, groups=1, dy2: Feat = None):
    """Backward, local half: bsums[g][c] = {sum g, sum g * xhat} and the counts; dgamma / dbeta
    (optional) take the LOCAL sums -- the gradient all-reduce averages them like any weight's."""
    assert x.N % groups == 0 and bsums.dtype == torch.float64 and bsums.numel() >= bn_sync_numel(groups, x.C)
    d2 = (dy2.ptr, dy2.dt, dy2.ld, dy2.off) if dy2 is not None else (None, 0, 0, 0)
    _lib.call("irgan_bn_sync_backward_sums", dy.ptr, dy.dt, dy.ld, dy.off, *d2, x.ptr, x.dt, x.ld, x.off, act, x.N,
              x.H * x.W, x.C, groups, P(mr), P(gamma), P(beta), P(work), P(bsums), P(dgamma), P(dbeta), stream())


def bn_sync_backward_dx(dy: Feat, x: Feat, act: int, mr, gamma, beta, bsums: torch.Tensor, dx: Feat, groups=1,
                        dy2: Feat = None):
    """Backward, finishing half: dx from the REDUCED bsums (the means over the reduced count)."""
    assert x.N % groups == 0 and bsums.dtype == torch.float64 and bsums.numel() >= bn_sync_numel(groups, x.C)
    d2 = (dy2.ptr, dy2.dt, dy2.ld, dy2.off) if dy2 is not None else (None, 0, 0, 0)
    _lib.call("irgan_bn_sync_backward_dx", dy.ptr, dy.dt, dy.ld, dy.off, *d2, x.ptr, x.dt, x.ld, x.off, act, x.N,
              x.H * x.W, x.C, groups, P(mr), P(gamma), P(beta), P(bsums), dx.ptr, dx.dt, dx.ld, dx.off, stream())


# ----------------------------------------------------------------------------
# resampling / elementwise
# ----------------------------------------------------------------------------

RS_DOWN, RS_UP, RS_PAD = 0, 1, 2
TMAX = 8
_TABLES = {}


def _host_table(kind, n_in, p=0, transpose=False):
    """Host (idx [rows][TMAX], w [rows][TMAX], rows) of a per-axis resampling map,
    built by the C ABI (irgan_resample_table)."""
    import numpy as np
    cap = 2 * n_in + 2 * p + 8
    idx = np.zeros(cap * TMAX, np.int32)
    w = np.zeros(cap * TMAX, np.float32)
    rows = _lib.load().irgan_resample_table(kind, n_in, p, int(transpose), idx.ctypes.data_as(ctypes.c_void_p),
                                              w.ctypes.data_as(ctypes.c_void_p), TMAX, cap)
    if rows < 0:
        raise _lib.IrganError(f"irgan_resample_table({kind}, {n_in}, {p}) failed: {rows}")
    return idx[:rows * TMAX].reshape(rows, TMAX), w[:rows * TMAX].reshape(rows, TMAX), rows


def _device_table(idx, w, rows, dev):
    """Device copy of a table; each row's taps start at slot 0, so keep only the
    widest row's tap count."""
    import numpy as np
    T = max(1, int((w != 0).sum(axis=1).max()))
    return (torch.from_numpy(np.ascontiguousarray(idx[:, :T])).to(dev),
            torch.from_numpy(np.ascontiguousarray(w[:, :T])).to(dev), rows, T)


def _dev(device):
    return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)


def resample_table(kind, n_in, p=0, transpose=False, device=None):
    """Device (idx, w, rows, T) per-axis table of a separable resampling map, cached."""
    dev = _dev(device)
    key = (kind, n_in, p, bool(transpose), dev)
    t = _TABLES.get(key)
    if t is None:
        t = _TABLES[key] = _device_table(*_host_table(kind, n_in, p, transpose), dev)
    return t


def bilinear_matrix(n_in, n_out):
    """Dense (n_out x n_in) map of F.interpolate(mode='bilinear', align_corners=True)
    along one axis (ir:555-556, 562-563): source coordinate o*(n_in-1)/(n_out-1),
    linear weights between its two neighbours (ATen's upsample_bilinear2d)."""
    import numpy as np
    M = np.zeros((n_out, n_in), np.float64)
    scale = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    for o in range(n_out):
        src = np.float32(np.float32(scale) * o) if n_out > 1 else 0.0
        i0 = min(int(src), n_in - 1)
        i1 = i0 + (1 if i0 < n_in - 1 else 0)
        lam = float(src) - i0
        M[o, i0] += 1.0 - lam
        M[o, i1] += lam
    return M


def _dense(idx, w, rows, n_in):
    import numpy as np
    M = np.zeros((rows, n_in), np.float64)
    for r in range(rows):
        for t in range(idx.shape[1]):
            if w[r, t] != 0:
                M[r, idx[r, t]] += w[r, t]
    return M


def _table_from_dense(M):
    """(idx, w, rows) table of a dense map (rows x n_in), taps packed from slot 0."""
    import numpy as np
    rows = M.shape[0]
    nz = [np.nonzero(M[r])[0] for r in range(rows)]
    T = max(1, max(len(z) for z in nz))
    if T > TMAX:
        raise _lib.IrganError(f"resampling map needs {T} taps per row (> {TMAX})")
    idx = np.zeros((rows, TMAX), np.int32)
    w = np.zeros((rows, TMAX), np.float32)
    for r, z in enumerate(nz):
        idx[r, :len(z)] = z
        w[r, :len(z)] = M[r, z]
    return idx, w, rows


def resize_table(n_in, n_out, after_up=False, transpose=False, device=None):
    """Per-axis table of the odd-size decoder fallback (ir:555-556, 562-563): the
    bilinear align_corners resize from the up-sampled length to the skip's length.
    after_up=True composes it with UpsampleAA (n_in -> 2*n_in -> n_out) into ONE
    map, so the up-sample + resize is a single sep_resample launch."""
    import numpy as np
    dev = _dev(device)
    key = ("resize", n_in, n_out, bool(after_up), bool(transpose), dev)
    t = _TABLES.get(key)
    if t is None:
        if after_up:
            M = bilinear_matrix(2 * n_in, n_out) @ _dense(*_host_table(RS_UP, n_in), n_in)
        else:
            M = bilinear_matrix(n_in, n_out)
        M[np.abs(M) < 1e-12] = 0.0
        t = _TABLES[key] = _device_table(*_table_from_dense(M.T.copy() if transpose else M), dev)
    return t


def sep_resample(x: Feat, y: Feat, ytab, xtab, accumulate=False):
    (ty, wy, ry, Ty), (tx, wx, rx, Tx) = ytab, xtab
    assert (ry, rx) == (y.H, y.W) and x.C == y.C and x.N == y.N, "sep_resample shape mismatch"
    _lib.call("irgan_sep_resample", x.ptr, x.dt, x.N, x.H, x.W, x.C, x.ld, x.off, y.ptr, y.dt, y.H, y.W, y.ld, y.off,
              P(ty), P(wy), Ty, P(tx), P(wx), Tx, int(accumulate), stream())


def sep_resample_in(z: Feat, mr: torch.Tensor, act, y: Feat, ytab, xtab) -> bool:
    """y = resample(act(InstanceNorm(z))) with z's {mean, rstd} table ``mr``
    (irgan_sep_resample_in: the IN apply fused into the resample's loads).  False when
    the kernel does not take the shapes -- then NOTHING ran."""
    (ty, wy, ry, Ty), (tx, wx, rx, Tx) = ytab, xtab
    assert (ry, rx) == (y.H, y.W) and z.C == y.C and z.N == y.N, "sep_resample_in shape mismatch"
    return _try("irgan_sep_resample_in", z.ptr, z.dt, z.N, z.H, z.W, z.C, z.ld, z.off, P(mr), act, y.ptr, y.dt, y.H,
                y.W, y.ld, y.off, P(ty), P(wy), Ty, P(tx), P(wx), Tx, stream())


def sep_resample_fp8(x: Feat, mr, act, y: Feat, ytab, xtab, q8) -> bool:
    """sep_resample (mr None) / sep_resample_in (mr: act(IN(x)) on load) into bf16 y that
    also writes y's e4m3 copy: q8 = (y8 Feat, q pointer, amax pointer or None: nothing
    recorded), an Fp8Out's ``side`` (irgan_sep_resample_fp8).  False when the kernel does not take the shapes --
    then NOTHING ran."""
    (ty, wy, ry, Ty), (tx, wx, rx, Tx) = ytab, xtab
    y8, qp, ap = q8
    assert (ry, rx) == (y.H, y.W) and x.C == y.C and x.N == y.N, "sep_resample_fp8 shape mismatch"
    assert y8.dt == FP8 and (y8.N, y8.H, y8.W, y8.C) == (y.N, y.H, y.W, y.C)
    return _try("irgan_sep_resample_fp8", x.ptr, x.dt, x.N, x.H, x.W, x.C, x.ld, x.off, P(mr), act, y.ptr, y.dt, y.H,
                y.W, y.ld, y.off, P(ty), P(wy), Ty, P(tx), P(wx), Tx, y8.ptr, y8.ld, y8.off, qp, ap, stream())


def blur_down(x: Feat, y: Feat):
    """Downsample (ir:269-310)."""
    sep_resample(x, y, resample_table(RS_DOWN, x.H), resample_table(RS_DOWN, x.W))


def blur_down_in(z: Feat, mr: torch.Tensor, act, y: Feat, q8=None) -> bool:
    """Downsample of act(IN(z)) (ir:469-482) without storing the normalised tensor;
    q8: also y's e4m3 copy (sep_resample_fp8)."""
    if q8 is not None:
        return sep_resample_fp8(z, mr, act, y, resample_table(RS_DOWN, z.H), resample_table(RS_DOWN, z.W), q8)
    return sep_resample_in(z, mr, act, y, resample_table(RS_DOWN, z.H), resample_table(RS_DOWN, z.W))


def blur_down_bwd(dy: Feat, dx: Feat, accumulate=False):
    sep_resample(dy, dx, resample_table(RS_DOWN, dx.H, transpose=True), resample_table(RS_DOWN, dx.W, transpose=True),
                 accumulate)


# The InstanceNorm backward of down1 / down2 taken from the Downsample adjoint without storing
# the up-sampled gradient (blur_down_bwd_in); IRGAN_RESAMPLE_BWD_FUSED=0: the adjoint launch
# followed by reduce + finalize + apply (the A/B switch)
RESAMPLE_BWD_FUSED = [os.environ.get("IRGAN_RESAMPLE_BWD_FUSED") != "0"]


def set_resample_bwd_fused(on: bool) -> bool:
    """blur_down_bwd_in (default) or blur_down_bwd + in_backward for the layers that can take
    either (INLayer.resample_bwd).  Returns the previous setting."""
    old, RESAMPLE_BWD_FUSED[0] = RESAMPLE_BWD_FUSED[0], bool(on)
    return old


def _shares_bytes(a: Feat, b: Feat) -> bool:
    """False only when the two slices share no byte: disjoint channels of one tensor, or
    disjoint storage ranges."""
    if a.t.data_ptr() == b.t.data_ptr() and a.ld == b.ld:
        return a.off < b.off + b.C and b.off < a.off + a.C
    a0, b0 = a.t.data_ptr(), b.t.data_ptr()
    return a0 < b0 + b.t.numel() * b.t.element_size() and b0 < a0 + a.t.numel() * a.t.element_size()


def sep_resample_in_bwd(dy: Feat, ytab, xtab, z: Feat, act, mr, work, red, dz: Feat) -> bool:
    """dz = backward of act(InstanceNorm(z)) applied to resample(dy), the resampled gradient
    never stored (irgan_sep_resample_in_bwd_reduce + _apply; red is an output).  False when the
    library does not take the arguments -- then NOTHING ran and nothing was written."""
    (ty, wy, ry, Ty), (tx, wx, rx, Tx) = ytab, xtab
    assert (ry, rx) == (z.H, z.W) == (dz.H, dz.W) and dy.C == z.C == dz.C and dy.N == z.N == dz.N, \
        "sep_resample_in_bwd shape mismatch"
    if dz.dt != BF16 or dz.ld % 8 or dz.off % 8 or _shares_bytes(z, dz):
        return False   # what the apply refuses, asked before the reduce runs
    head = (dy.ptr, dy.dt, dy.N, dy.H, dy.W, dy.C, dy.ld, dy.off, z.H, z.W, P(ty), P(wy), Ty, P(tx), P(wx), Tx,
            z.ptr, z.dt, z.ld, z.off, P(mr), act)
    if not _timed("resample_in_bwd_reduce", z,
                  lambda: _try("irgan_sep_resample_in_bwd_reduce", *head, P(work), P(red), stream())):
        return False
    _timed("resample_in_bwd_apply", z,
           lambda: _lib.call("irgan_sep_resample_in_bwd_apply", *head, P(red), dz.ptr, dz.dt, dz.ld, dz.off, None,
                             None, stream()))
    return True


def blur_down_bwd_in(dy: Feat, z: Feat, act, mr, work, red, dz: Feat) -> bool:
    """The backward of Downsample(act(IN(z))) down to z's gradient: blur_down_bwd + in_backward
    without the full-resolution gradient in between (sep_resample_in_bwd)."""
    return sep_resample_in_bwd(dy, resample_table(RS_DOWN, z.H, transpose=True),
                               resample_table(RS_DOWN, z.W, transpose=True), z, act, mr, work, red, dz)


def _up_axis(n_in, n_out, transpose):
    if n_out == 2 * n_in:
        return resample_table(RS_UP, n_in, transpose=transpose)
    return resize_table(n_in, n_out, after_up=True, transpose=transpose)   # odd-size fallback folded in


def upsample(x: Feat, y: Feat, q8=None):
    """UpsampleAA (ir:313-355); when y is not 2x (odd skip sizes) the reference's
    bilinear resize to the skip's size (ir:555-556, 562-563) is folded into the map.
    q8: also y's e4m3 copy (sep_resample_fp8; the plain launch + fp8_quant if the LDS
    form does not take the shapes)."""
    yt, xt = _up_axis(x.H, y.H, False), _up_axis(x.W, y.W, False)
    if q8 is not None and sep_resample_fp8(x, None, ACT_NONE, y, yt, xt, q8):
        return
    sep_resample(x, y, yt, xt)
    if q8 is not None:
        fp8_quant(y, *q8)


def upsample_in(z: Feat, mr: torch.Tensor, act, y: Feat) -> bool:
    """UpsampleAA of act(IN(z)) (ir:557-561) without storing the normalised tensor."""
    return sep_resample_in(z, mr, act, y, _up_axis(z.H, y.H, False), _up_axis(z.W, y.W, False))


def upsample_bwd(dy: Feat, dx: Feat, work=None, accumulate=False):
    sep_resample(dy, dx, _up_axis(dx.H, dy.H, True), _up_axis(dx.W, dy.W, True), accumulate)


def resize(x: Feat, y: Feat, accumulate=False):
    """F.interpolate(x, size=(y.H, y.W), mode='bilinear', align_corners=True)."""
    sep_resample(x, y, resize_table(x.H, y.H), resize_table(x.W, y.W), accumulate)


def resize_bwd(dy: Feat, dx: Feat, accumulate=False):
    sep_resample(dy, dx, resize_table(dx.H, dy.H, transpose=True), resize_table(dx.W, dy.W, transpose=True),
                 accumulate)


def pad_table(n_in, p, mode, transpose=False, device=None):
    """Per-axis (idx, w, rows, T) table of nn.ReflectionPad2d(p) (mode "reflect") or
    nn.ReplicationPad2d(p) ("replicate", ir:383, 404): padded coordinate u reads
    reflect(u - p) / clamp(u - p, 0, n_in - 1); transpose: the fold (its adjoint)."""
    if mode == "reflect":
        return resample_table(RS_PAD, n_in, p, transpose, device)
    import numpy as np
    dev = _dev(device)
    key = ("replicate", n_in, p, bool(transpose), dev)
    t = _TABLES.get(key)
    if t is None:
        M = np.zeros((n_in + 2 * p, n_in), np.float64)
        for u in range(n_in + 2 * p):
            M[u, min(max(u - p, 0), n_in - 1)] = 1.0
        t = _TABLES[key] = _device_table(*_table_from_dense(M.T.copy() if transpose else M), dev)
    return t


def pad(x: Feat, y: Feat, p: int, mode):
    """y = ReflectionPad2d(p) / ReplicationPad2d(p) of x (y is (H + 2p) x (W + 2p))."""
    sep_resample(x, y, pad_table(x.H, p, mode, device=x.t.device), pad_table(x.W, p, mode, device=x.t.device))


def pad_fold(dxp: Feat, dx: Feat, p: int, mode, accumulate=False):
    """Backward of pad(): every padded position's gradient added onto the pixel it copied."""
    sep_resample(dxp, dx, pad_table(dx.H, p, mode, True, dx.t.device), pad_table(dx.W, p, mode, True, dx.t.device),
                 accumulate)


def dropout(x: Feat, y: Feat, seed: int, p: float = 0.5):
    """nn.Dropout(p) in training mode (ir:394-395): y = x * keep / (1 - p), keep ~ Bernoulli(1 - p)
    from a counter-based hash of (seed, element index) -- the backward applies the same
    call to the gradient (same seed -> same mask, same scale)."""
    assert (x.N, x.H, x.W, x.C) == (y.N, y.H, y.W, y.C)
    _lib.call("irgan_dropout", x.ptr, x.dt, x.P, x.C, x.ld, x.off, y.ptr, y.dt, y.ld, y.off,
              ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), ctypes.c_float(p), stream())


def reflect_fold(dxpad: Feat, dx: Feat, p: int, accumulate=False):
    """Backward of nn.ReflectionPad2d(p): dx[q] = sum over padded u with reflect(u-p) = q."""
    sep_resample(dxpad, dx, resample_table(RS_PAD, dx.H, p, transpose=True),
                 resample_table(RS_PAD, dx.W, p, transpose=True), accumulate)


def maxpool(x: Feat, y: Feat):
    assert x.off == 0 and x.C == x.ld and y.off == 0
    _lib.call("irgan_maxpool_fwd", x.ptr, x.dt, x.N, x.H, x.W, x.C, y.ptr, stream())


def maxpool_bwd(x: Feat, dy: Feat, dx: Feat, relu_mask=True):
    _lib.call("irgan_maxpool_bwd", x.ptr, dy.ptr, x.dt, x.N, x.H, x.W, x.C, dx.ptr, int(relu_mask), stream())


def maxpool_bwd_tap(x: Feat, xr: Feat, dy: Feat, dx: Feat, w: float, loss: torch.Tensor) -> bool:
    """maxpool_bwd(relu_mask=True) of a pool input that is a perceptual tap: dx also receives the
    tap's gradient (x > 0 ? sgn(x - xr) * w / count : 0) and ``loss`` += w * mean|x - xr|, in the
    one launch (irgan_maxpool_bwd_tap).  False when the library refuses the shape (an odd side)
    -- then NOTHING ran and the caller does maxpool_bwd + l1_tap(accumulate=True)."""
    for f in (x, xr, dy, dx):
        assert f.off == 0 and f.C == f.ld and f.dt == x.dt
    assert (xr.N, xr.H, xr.W, xr.C) == (x.N, x.H, x.W, x.C) == (dx.N, dx.H, dx.W, dx.C)
    assert (dy.N, dy.H, dy.W, dy.C) == (x.N, x.H // 2, x.W // 2, x.C)
    return _try("irgan_maxpool_bwd_tap", x.ptr, xr.ptr, dy.ptr, x.dt, x.N, x.H, x.W, x.C, dx.ptr,
                ctypes.c_float(w), P(loss), stream())


def nchw_to_nhwc(x: torch.Tensor, y: Feat, scale=None, shift=None):
    N, C, H, W = x.shape
    _lib.call("irgan_nchw_to_nhwc", P(x), N, C, H, W, y.ptr, y.dt, y.ld, y.off, P(scale), P(shift), stream())


def nhwc_to_nchw(x: Feat, y: torch.Tensor, scale=1.0, accumulate=False):
    _lib.call("irgan_nhwc_to_nchw", x.ptr, x.dt, x.ld, x.off, x.N, x.C, x.H, x.W, P(y), ctypes.c_float(scale),
              int(accumulate), stream())


def axpby(x: Feat, a: float, y: Feat, b: float = 0.0):
    _lib.call("irgan_axpby", x.ptr, x.dt, x.ld, x.off, ctypes.c_float(a), y.ptr, y.dt, y.ld, y.off,
              ctypes.c_float(b), x.P, x.C, stream())


def affine(x: Feat, scale, shift, y: Feat, accumulate=False):
    _lib.call("irgan_affine", x.ptr, x.dt, x.ld, x.off, P(scale), P(shift), y.ptr, y.dt, y.ld, y.off,
              int(accumulate), x.P, x.C, stream())


def act_bwd(dy: Feat, a: Feat, act: int, dx: Feat):
    _lib.call("irgan_act_bwd", dy.ptr, dy.dt, dy.ld, dy.off, a.ptr, a.dt, a.ld, a.off, act, dx.ptr, dx.dt, dx.ld,
              dx.off, dy.P, dy.C, stream())


# ----------------------------------------------------------------------------
# losses / optimizer
# ----------------------------------------------------------------------------

def hinge(pred: torch.Tensor, n_half: int, mode: int, scale: float, grad: torch.Tensor, loss: torch.Tensor):
    _lib.call("irgan_hinge", P(pred), n_half, mode, ctypes.c_float(scale), P(grad), P(loss), stream())


GAN_MODES = {"hinge": 0, "lsgan": 1, "vanilla": 2}   # Config.gan_mode -> irgan_gan_loss's objective


def gan_loss(pred: torch.Tensor, n_half: int, side: int, mode: str, real_label: float, scale: float,
             grad: torch.Tensor, loss: torch.Tensor):
    """The GAN objective ``mode`` (a key of GAN_MODES) on the patch logits: side 0 is D's loss on
    [real (n_half); fake (n_half)] with the real target ``real_label``, side 1 G's term on fake
    (n_half).  ``loss`` += scale * value, ``grad`` written.  "hinge" is ops.hinge's launch."""
    if mode not in GAN_MODES:
        raise ValueError(f"gan_mode must be one of {sorted(GAN_MODES)}, got {mode!r}")
    _lib.call("irgan_gan_loss", P(pred), n_half, side, GAN_MODES[mode], ctypes.c_float(real_label),
              ctypes.c_float(scale), P(grad), P(loss), stream())


def l1(a: torch.Tensor, b: torch.Tensor, w: float, ga: torch.Tensor, loss: torch.Tensor, accumulate=False):
    _lib.call("irgan_l1", P(a), P(b), dt_code(a), a.numel(), ctypes.c_float(w), P(ga),
              dt_code(ga) if ga is not None else 0, int(accumulate), P(loss), stream())


def l1_tap(a: torch.Tensor, b: torch.Tensor, w: float, dz: torch.Tensor, loss: torch.Tensor, accumulate=False):
    """One perceptual tap (irgan_l1_tap): a / b the fake / real post-ReLU features, dz the gradient
    w.r.t. the layer's pre-activation.  ``loss`` += w * mean|a - b|;
    dz = (accumulate ? dz : 0) + (a > 0 ? sgn(a - b) * w / count : 0)."""
    assert a.numel() == b.numel() == dz.numel() and a.dtype == b.dtype
    _lib.call("irgan_l1_tap", P(a), P(b), dt_code(a), a.numel(), ctypes.c_float(w), P(dz), dt_code(dz),
              int(accumulate), P(loss), stream())


def _whole(x: Feat, what: str):
    """irgan_tv / irgan_ssim_ws take (ptr, N, H, W, C) and read the image as contiguous: a
    channel slice (ld != C or off != 0) would be read as if it were whole, so refuse it."""
    if x.off != 0 or x.ld != x.C:
        raise ValueError(f"{what} reads a contiguous NHWC image, not a channel slice "
                         f"(off {x.off}, C {x.C}, ld {x.ld})")


def tv(x: Feat, w: float, g: torch.Tensor, loss: torch.Tensor):
    _whole(x, "ops.tv: x")
    _lib.call("irgan_tv", x.ptr, x.N, x.H, x.W, x.C, ctypes.c_float(w), P(g), P(loss), stream())


def ssim(a: Feat, b: Feat, w: float, g: torch.Tensor, loss: torch.Tensor, work: torch.Tensor, window: int = 11):
    _whole(a, "ops.ssim: a")
    _whole(b, "ops.ssim: b")
    _lib.call("irgan_ssim_ws", a.ptr, b.ptr, a.N, a.H, a.W, a.C, ctypes.c_float(w), P(g), P(loss), P(work), window,
              stream())


def ema_weight(decay: float, t: int) -> float:
    """The weight of the new parameters in the EMA update after optimizer step ``t`` (1-based):
    ``1 - min(decay, (1 + t) / (10 + t))``, so ``e += w * (p - e)``.  The warm-up term lets a
    short run's average follow the weights instead of the initialisation.  fp64; the kernels
    take it rounded to fp32 (irgan_adam_ema_prep evaluates the same formula on the device)."""
    return 1.0 - min(float(decay), (1.0 + t) / (10.0 + t))


def _adam_call(form, p, g, m, v, ema, *args):
    """irgan_adam<form> or, with ``ema``, irgan_adam_ema<form>, which takes it after ``v``."""
    if ema is None:
        return _lib.call(f"irgan_adam{form}", P(p), P(g), P(m), P(v), p.numel(), *args, stream())
    if any(t.numel() != p.numel() for t in (g, m, v, ema)):
        raise ValueError(f"ops.adam{form}: p, g, m, v and ema must have one element count")
    _lib.call(f"irgan_adam_ema{form}", P(p), P(g), P(m), P(v), P(ema), p.numel(), *args, stream())


def _adam_clip_call(form, p, g, m, v, ema, *args):
    """irgan_adam_clip<form>: one entry with and without ``ema`` (a null pointer)."""
    if any(t.numel() != p.numel() for t in (g, m, v) + (() if ema is None else (ema,))):
        raise ValueError(f"ops.adam{form}: p, g, m, v and ema must have one element count")
    _lib.call(f"irgan_adam_clip{form}", P(p), P(g), P(m), P(v), P(ema), p.numel(), *args, stream())


def adam(p, g, m, v, step: int, lr: float, b1: float, b2: float, eps: float, ema=None, decay: float = 0.0,
         coef: float = None):
    """One Adam step with host-side bias corrections (irgan_adam).  With ``ema`` also, in the
    same pass, ema += ema_weight(decay, step) * (p_new - ema) (irgan_adam_ema); p, m, v come
    out the same with and without it, bit for bit.  With ``coef`` (gradient-norm clipping,
    clip_coef) the update consumes float32(g * float32(coef)); g is not written
    (irgan_adam_clip)."""
    bc1 = 1 - b1 ** step
    bc2 = 1 - b2 ** step
    head = (ctypes.c_float(lr / bc1), ctypes.c_float(b1), ctypes.c_float(b2), ctypes.c_float(math.sqrt(bc2)),
            ctypes.c_float(eps))
    if coef is not None:
        return _adam_clip_call("", p, g, m, v, ema, *head,
                               ctypes.c_float(0.0 if ema is None else ema_weight(decay, step)), ctypes.c_float(coef))
    tail = () if ema is None else (ctypes.c_float(ema_weight(decay, step)),)
    _adam_call("", p, g, m, v, ema, *head, *tail)


def clip_coef(norm: float, max_norm: float) -> float:
    """torch.nn.utils.clip_grad_norm_'s factor for a gradient of L2 norm ``norm``:
    ``min(1, max_norm / (norm + 1e-6))`` in fp64 (NaN stays NaN); the kernels take it rounded
    to fp32 (irgan_adam_clip_prep evaluates the same formula on the device)."""
    c = float(max_norm) / (float(norm) + 1e-6)
    return 1.0 if c > 1.0 else c


def grad_sumsq_parts(n: int) -> int:
    """The number of fp64 partials ops.grad_sumsq writes for n elements (a function of n alone)."""
    return int(_lib.load().irgan_grad_sumsq_parts(int(n)))


def grad_sumsq(g: torch.Tensor, partials: torch.Tensor):
    """Deterministic sum of squares of the flat fp32 ``g`` as grad_sumsq_parts(n) fp64 per-block
    partials (irgan_grad_sumsq): their sum IN INDEX ORDER is the squared L2 norm, the same bits
    on every launch and every rank."""
    if g.dtype != torch.float32 or partials.dtype != torch.float64:
        raise ValueError("ops.grad_sumsq: g is fp32, partials fp64")
    _lib.call("irgan_grad_sumsq", P(g), g.numel(), P(partials), partials.numel(), stream())


def grad_norm(g: torch.Tensor, partials: torch.Tensor = None) -> float:
    """The L2 norm of ``g`` on the host (one sync): ops.grad_sumsq's partials added in index
    order in fp64, as irgan_adam_clip_prep adds them on the device."""
    if partials is None:
        partials = torch.empty(grad_sumsq_parts(g.numel()), dtype=torch.float64, device=g.device)
    grad_sumsq(g, partials)
    s = 0.0
    for x in partials.tolist():
        s += x
    return math.sqrt(s)


def adam_prep(count: torch.Tensor, lr: float, b1: float, b2: float, prm: torch.Tensor, decay: float = None):
    """Device-side step count + bias corrections (irgan_adam_prep): count (int32[1]) += 1,
    prm[:2] = {lr / (1 - b1^t), sqrt(1 - b2^t)} -- ops.adam's host formula.  With ``decay``
    also prm[2] = ema_weight(decay, t), so prm holds three floats (irgan_adam_ema_prep)."""
    lrb = (ctypes.c_double(lr), ctypes.c_double(b1), ctypes.c_double(b2))
    if decay is None:
        return _lib.call("irgan_adam_prep", P(count), *lrb, P(prm), stream())
    if prm.numel() < 3:
        raise ValueError("ops.adam_prep: with decay, prm holds three floats")
    _lib.call("irgan_adam_ema_prep", P(count), *lrb, ctypes.c_double(decay), P(prm), stream())


def adam_clip_prep(count: torch.Tensor, lr: float, b1: float, b2: float, prm: torch.Tensor, partials: torch.Tensor,
                   n: int, max_norm: float, norm_out: torch.Tensor = None, decay: float = 0.0):
    """ops.adam_prep's count and prm[:3] (``decay`` 0 where there is no average) and, from
    ops.grad_sumsq's ``partials`` of a buffer of ``n`` elements: norm_out[0] = its L2 norm (fp64,
    optional), prm[3] = clip_coef(norm, max_norm) -- prm holds four floats
    (irgan_adam_clip_prep).  No launch beyond this one, no host sync."""
    if prm.numel() < 4:
        raise ValueError("ops.adam_clip_prep: prm holds four floats")
    if partials.dtype != torch.float64 or (norm_out is not None and norm_out.dtype != torch.float64):
        raise ValueError("ops.adam_clip_prep: partials and norm_out are fp64")
    _lib.call("irgan_adam_clip_prep", P(count), ctypes.c_double(lr), ctypes.c_double(b1), ctypes.c_double(b2),
              ctypes.c_double(decay), P(partials), partials.numel(), int(n), ctypes.c_double(max_norm), P(norm_out),
              P(prm), stream())


def adam_dev(p, g, m, v, prm: torch.Tensor, b1: float, b2: float, eps: float, ema=None, clip: bool = False):
    """ops.adam with step_size / bc2_sqrt and, with ``ema``, the EMA weight read from prm on the
    device (irgan_adam_dev / irgan_adam_ema_dev); with ``clip`` the gradient times prm[3]
    (ops.adam_clip_prep; irgan_adam_clip_dev)."""
    tail = (P(prm), ctypes.c_float(b1), ctypes.c_float(b2), ctypes.c_float(eps))
    if clip:
        if prm.numel() < 4:
            raise ValueError("ops.adam_dev: with clip, prm holds four floats")
        return _adam_clip_call("_dev", p, g, m, v, ema, *tail)
    _adam_call("_dev", p, g, m, v, ema, *tail)


# ----------------------------------------------------------------------------
# fp8 (OCP e4m3) operands: BASELINE config 5
# ----------------------------------------------------------------------------

def fp8_quant(x: Feat, y: Feat = None, q=None, amax=None):
    """y = e4m3(clamp(x * q, +-448)); amax = max(amax, max|x|) (irgan_fp8_quant).
    q / amax: ctypes pointers to one float / uint32 slot (Pi), or None."""
    assert y is None or (y.dt == FP8 and (y.N, y.H, y.W, y.C) == (x.N, x.H, x.W, x.C))
    _lib.call("irgan_fp8_quant", x.ptr, x.dt, x.P, x.C, x.ld, x.off, y.ptr if y is not None else None,
              y.ld if y is not None else 0, y.off if y is not None else 0, q, amax, stream())


FP8_AMAX_PARTS = _lib.header_enum("IRGAN_FP8_AMAX_PARTS")


def amax_slots(n, device):
    """n amax slots of FP8_AMAX_PARTS partial maxima each (irgan.h)."""
    return torch.zeros(n * FP8_AMAX_PARTS, dtype=torch.int32, device=device)


def amax_ptr(amax: torch.Tensor, slot: int):
    return Pi(amax, slot * FP8_AMAX_PARTS)


def fp8_scale(amax: torch.Tensor, q: torch.Tensor, dq: torch.Tensor, reset=True, start=0, n=None):
    """Slots [start, start+n): q = 2^floor(log2(448 / amax)), dq = 1 / q (irgan_fp8_scale)."""
    n = q.numel() - start if n is None else n
    _lib.call("irgan_fp8_scale", amax_ptr(amax, start), n, Pi(q, start), Pi(dq, start), int(reset), stream())


class Fp8Job(ctypes.Structure):
    """irgan_fp8_job (include/irgan.h)."""
    _fields_ = [("src", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("slot", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Fp8Weights:
    """fp8 copies of bf16 packed weight images, re-quantised after every re-pack with
    per-tensor current scaling: one amax launch, irgan_fp8_scale, one quantise launch
    for all of them.  ``dst[k]`` / slot k belongs to the k-th (src) image."""

    def __init__(self, srcs, device):
        self.srcs = list(srcs)
        self.dst = [torch.empty(t.numel(), dtype=torch.float8_e4m3fn, device=device) for t in self.srcs]
        n = len(self.srcs)
        self.amax = amax_slots(n, device)
        self.q = torch.ones(n, dtype=torch.float32, device=device)
        self.dq = torch.ones(n, dtype=torch.float32, device=device)
        jobs = (Fp8Job * n)(*[Fp8Job(s.data_ptr(), d.data_ptr(), s.numel(), k, 0)
                              for k, (s, d) in enumerate(zip(self.srcs, self.dst))])
        assert all(s.numel() % 8 == 0 and s.dtype == torch.bfloat16 and s.is_contiguous() for s in self.srcs)
        self.table = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(device)
        self.max_n = max(s.numel() for s in self.srcs)

    def run(self):
        n = len(self.srcs)
        _lib.call("irgan_fp8_quant_batch", P(self.table), n, self.max_n, None, P(self.amax), stream())
        fp8_scale(self.amax, self.q, self.dq, reset=True)
        _lib.call("irgan_fp8_quant_batch", P(self.table), n, self.max_n, P(self.q), None, stream())


class Fp8Acts:
    """Per-tensor scales of fp8 activation operands with delayed scaling: a slot's
    tensor is quantised with the q made from the amax it had at the previous step
    (its first use calibrates from its own amax).  update() turns the recorded maxima
    into the next step's q / dq.  A slot is unseen (``seen`` False: its next use calibrates it),
    delayed (a training pass records its amax and update() moves its scale) or, for an eval-mode
    forward, frozen: read with ``record=False`` / an Fp8Out(record=False), never written.
    The tensors are allocated once and only ever changed in place, so a Pi() pointer into them
    stays valid across reset() and load_state_dict()."""

    def __init__(self, n, device):
        self.amax = amax_slots(n, device)
        self.q = torch.ones(n, dtype=torch.float32, device=device)
        self.dq = torch.ones(n, dtype=torch.float32, device=device)
        self.seen = [False] * n

    def quant(self, slot, x: Feat, y: Feat, record=True):
        """Standalone quantisation of x into y (irgan_fp8_quant).  record False: with the slot's
        scale as it stands, nothing written to the slot."""
        if not record:
            fp8_quant(x, y, Pi(self.q, slot), None)
            return
        if not self.seen[slot]:
            fp8_quant(x, None, None, amax_ptr(self.amax, slot))
            fp8_scale(self.amax, self.q, self.dq, reset=False, start=slot, n=1)
            self.seen[slot] = True
        fp8_quant(x, y, Pi(self.q, slot), amax_ptr(self.amax, slot))

    def calibrate(self, slot, x: Feat, y: Feat):
        """Current scaling of slot from x alone, whatever was recorded before (the slot's
        partial maxima are cleared first), then the quantisation of x into y."""
        self.clear_amax(slot, 1)
        self.seen[slot] = False
        self.quant(slot, x, y)

    def dqp(self, slot):
        return Pi(self.dq, slot)

    def update(self, start=0, n=None):
        fp8_scale(self.amax, self.q, self.dq, reset=True, start=start, n=n)

    def clear_amax(self, start=0, n=None):
        """Forget the maxima recorded in slots [start, start+n)."""
        n = self.q.numel() - start if n is None else n
        self.amax[start * FP8_AMAX_PARTS:(start + n) * FP8_AMAX_PARTS].zero_()

    def reset(self):
        """Every slot unseen, as constructed (in place)."""
        self.amax.zero_()
        self.q.fill_(1.0)
        self.dq.fill_(1.0)
        self.seen[:] = [False] * len(self.seen)

    def state_dict(self):
        """q, dq, the amax partials and seen as CPU tensors (torch.load(weights_only=True) takes
        them)."""
        return {"q": self.q.detach().cpu().clone(), "dq": self.dq.detach().cpu().clone(),
                "amax": self.amax.detach().cpu().clone(), "seen": torch.tensor(self.seen, dtype=torch.bool)}

    def load_state_dict(self, sd):
        """Copies a state_dict() into the slots in place (the pointers handed out stay valid)."""
        have, want = len(self.seen), int(sd["seen"].numel())
        if want != have or sd["q"].numel() != have or sd["dq"].numel() != have or \
                sd["amax"].numel() != have * FP8_AMAX_PARTS:
            raise ValueError(f"fp8 scale state of {want} slots does not fit this generator's {have} slots")
        self.q.copy_(sd["q"].to(torch.float32))
        self.dq.copy_(sd["dq"].to(torch.float32))
        self.amax.copy_(sd["amax"].to(torch.int32))
        self.seen[:] = [bool(v) for v in sd["seen"].tolist()]


class Fp8Out:
    """What a producer receives as ``q8``: the e4m3 copy of its output for one Fp8Acts slot.
    ``side`` is the (y8, q pointer, amax pointer) triple of the ops that write the copy in their
    own store pass (in_apply, in_backward, the fused resamplers), or None before the slot is
    calibrated.  The producer calls finish() directly after its launch.
    record False (an eval-mode forward): the read-only form, side = (y8, q pointer, None) --
    the slot's scale as it stands, and finish() never falls back to a recording quantise."""
    __slots__ = ("acts", "slot", "y8", "side", "record")

    def __init__(self, acts: Fp8Acts, slot, y8: Feat, record=True):
        self.acts, self.slot, self.y8, self.record = acts, slot, y8, record
        if record:
            self.side = (y8, Pi(acts.q, slot), amax_ptr(acts.amax, slot)) if acts.seen[slot] else None
        else:
            self.side = (y8, Pi(acts.q, slot), None)

    def finish(self, x: Feat, taken=True):
        """Quantise x standalone if the side output was not taken: the slot was not calibrated
        (this calibrates it from x), or the producer ran a launch without the fused copy."""
        if self.side is None:
            self.acts.quant(self.slot, x, self.y8)
        elif not taken:
            fp8_quant(x, *self.side)


def conv_fwd_fp8(pc: PackedConv, w8: torch.Tensor, dqw, x8: Feat, dqx, y: Feat, part: torch.Tensor = None,
                 act=ACT_NONE, bias=True, accumulate=False) -> int:
    """conv_fwd on fp8 operands (irgan_conv_fwd_fp8): x8 e4m3 NHWC, w8 the e4m3 copy
    of pc.fwd; dqx / dqw: pointers to the dequantisation multipliers.  With ``part``
    also the InstanceNorm partials of y; returns their count per image (else 0)."""
    s = pc.spec
    assert y.C == s.cout and x8.C == s.cin and x8.dt == FP8
    d = _fwd_desc(s, x8, y, s.cin, FP8, y.dt, act, accumulate)
    nb = ctypes.c_int32(0)
    TIMER.wrap(conv_tag("fwd8", s, (x8.H, x8.W), x8.N), lambda: _lib.call(
        "irgan_conv_fwd_fp8", ctypes.byref(d), x8.ptr, P(w8), dqx, dqw, P(pc.bias if bias else None), y.ptr,
        P(part), ctypes.byref(nb), stream()))
    return int(nb.value)


def conv_wgrad_fp8(spec: ConvSpec, x8: Feat, dy8: Feat, dqx, dqdy, dw: torch.Tensor) -> bool:
    """dw (fp32 KRSC view, accumulated) += weight gradient of conv(x) given dy, on the fp8
    copies x8 / dy8 with their dequantisation pointers (irgan_conv_wgrad_fp8).  False when
    the kernel does not take the layer -- then NOTHING ran (the caller runs the bf16 conv_wgrad)."""
    assert dy8.C == spec.cout and x8.C == spec.cin and x8.dt == FP8 and dy8.dt == FP8
    d = _fwd_desc(spec, x8, dy8, spec.cin, FP8, F32, accumulate=1, flags=CONV_DETERMINISTIC if _DET[0] else 0)
    ws = _wgrad_ws(dw.device)
    return TIMER.wrap(conv_tag("wgrad8", spec, (x8.H, x8.W), x8.N), lambda: _try(
        "irgan_conv_wgrad_fp8", ctypes.byref(d), x8.ptr, dy8.ptr, dqx, dqdy, P(dw), P(ws), ws.numel(), stream()))


def conv_dgrad_fp8(pc: PackedConv, wd8: torch.Tensor, dqw, dy8: Feat, dqx, dy: Feat, dx: Feat, accumulate=False):
    """Backward-data of a stride-1 3x3 layer on fp8 operands (dy8 = e4m3(dy), wd8 = e4m3
    copy of the flipped image pc.dg[0]).  Reflect padding: the interior on fp8, the padded
    ring from the bf16 dy (_dgrad_reflect, as conv_dgrad); zero padding (down2 / up1_conv of
    config 5): the flipped conv alone (irgan_conv_fwd_fp8; dy unused)."""
    s = pc.spec
    assert s.stride == 1 and dy8.dt == FP8 and dx.C == s.cin
    if pc.reflect:
        assert dy.dt == BF16
        _dgrad_reflect(pc, dy, dx, accumulate, f8=(wd8, dqw, dy8, dqx))
        return
    assert len(pc.dg) == 1 and (dy8.H, dy8.W, dy8.C) == (dx.H, dx.W, pc.cout_eff)
    d8 = _dgrad_desc(pc, pc.dg[0], dy8, dx, accumulate, dtype=FP8)
    TIMER.wrap(conv_tag("dgrad8", s, (dx.H, dx.W), dx.N), lambda: _lib.call(
        "irgan_conv_fwd_fp8", ctypes.byref(d8), dy8.ptr, P(wd8), dqx, dqw, None, dx.ptr, None,
        ctypes.byref(ctypes.c_int32(0)), stream()))
