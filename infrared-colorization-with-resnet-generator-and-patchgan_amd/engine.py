"""The fused GAN train step on HIP kernels (the product hot path).

One ``GANStep.step(ir, rgb)`` = the reference's inner-loop body
(ir:1636-1681) in its minimal form: one G forward reused (detached) for the D
step; D forward/backward on the batched [real; fake] pair; D Adam; D forward on
fake with the updated D; GAN (hinge, or Config.gan_mode's LSGAN / BCE) + L1 +
VGG-perceptual + TV + SSIM losses with their gradients written directly; G
backward; G Adam.  No autograd tape: every backward is an explicit HIP kernel sequence over activations kept in static
NHWC buffers (capturable in a HIP graph).

Parameters live in flat fp32 buffers (one per network) whose per-key slices are
KRSC conv weights; the reference's OIHW ``state_dict`` tensors are permuted
*views* of those slices (``ParamStore.oihw``), so checkpoints load/save in the
reference layout while the kernels and the single-launch Adam read the flat
buffer.  Data-parallel: each rank owns a batch shard and all-reduces the flat
gradient buffers (RCCL) before each Adam.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from contextlib import nullcontext as _nullcontext
from typing import NamedTuple

import torch

from . import ops
from .ops import (ACT_LRELU, ACT_NONE, ACT_RELU, ACT_TANH, BF16, F32, PAD_REFLECT, PAD_ZERO, ConvSpec, Feat,
                  PackedConv)

IMAGENET_MEAN = (0.485, 0.456, 0.406)   # ir:672
IMAGENET_STD = (0.229, 0.224, 0.225)    # ir:673


# ----------------------------------------------------------------------------
# parameter layout (reference state_dict keys / OIHW shapes / order)
# ----------------------------------------------------------------------------

def g_param_shapes(input_nc=1, output_nc=3, ngf=64, n_blocks=9, no_antialias=False, no_antialias_up=False,
                   use_bias=True, padding_type="reflect", use_dropout=False, batch_norm=False):
    """ResnetUNetGenerator state_dict layout (ir:443-531), buffers included.  use_bias:
    the reference's ``norm_layer == nn.InstanceNorm2d`` (ir:450-455); without it (norm
    'none' / 'batch') every conv but outc, and the ConvTranspose2d, has no bias.
    batch_norm: nn.BatchNorm2d's entries (bn_param_shapes) at the module index after each
    normalised conv."""
    s = OrderedDict()
    use_bias = use_bias and not batch_norm

    def conv(key, shape, normed=True):
        s[key + ".weight"] = shape
        if use_bias:
            s[key + ".bias"] = (shape[0],)
        if batch_norm and normed:
            seq, idx = key.rsplit(".", 1)
            s.update(bn_param_shapes(f"{seq}.{int(idx) + 1}", shape[0]))
    conv("inc.1", (ngf, input_nc, 7, 7))
    conv("down1.0", (2 * ngf, ngf, 3, 3))
    if not no_antialias:
        s["down1_down.filt"] = (2 * ngf, 1, 3, 3)
    conv("down2.0", (4 * ngf, 2 * ngf, 3, 3))
    if not no_antialias:
        s["down2_down.filt"] = (4 * ngf, 1, 3, 3)
    for b in range(n_blocks):
        for c in res_conv_keys(padding_type, use_dropout):
            conv(f"resblocks.{b}.conv_block.{c}", (4 * ngf, 4 * ngf, 3, 3))
    for name, ch, cat in (("up1", 4 * ngf, 6 * ngf), ("up2", 2 * ngf, 3 * ngf)):
        if no_antialias_up:
            conv(f"{name}_up", (ch, ch, 3, 3), normed=False)
        else:
            s[f"{name}_up.filt"] = (ch, 1, 3, 3)
        conv(f"{name}_conv.0", (ch // 2, cat, 3, 3))
    s["outc.1.weight"] = (output_nc, ngf, 7, 7); s["outc.1.bias"] = (output_nc,)
    return s


def bn_param_shapes(key, C):
    """nn.BatchNorm2d's state_dict entries under module ``key``, in its order."""
    return OrderedDict([(key + ".weight", (C,)), (key + ".bias", (C,)), (key + ".running_mean", (C,)),
                        (key + ".running_var", (C,)), (key + ".num_batches_tracked", ())])


BN_BUFFERS = (".running_mean", ".running_var", ".num_batches_tracked")


def d_layers(n_layers=3):
    """PatchGAN layer table (ir:585-632): (state key, stride, normalised) per conv.
    model.0 (s2, LeakyReLU), n_layers - 1 s2 conv/norm/LeakyReLU blocks, one s1
    conv/norm/LeakyReLU, the s1 1-channel output conv."""
    out = [("model.0", 2, False)]
    idx = 2
    for _ in range(1, n_layers):
        out.append((f"model.{idx}", 2, True))
        idx += 3
    out.append((f"model.{idx}", 1, True))
    out.append((f"model.{idx + 3}", 1, False))
    return out


def d_channels(input_nc=4, ndf=64, n_layers=3):
    """Channel counts along the PatchGAN (ir:598-632): ndf * min(2^n, 8)."""
    return [input_nc] + [ndf * min(2 ** n, 8) for n in range(n_layers + 1)] + [1]


def d_param_shapes(input_nc=4, ndf=64, n_layers=3, use_bias=True, batch_norm=False):
    """NLayerDiscriminator layout (ir:585-632); the first and last convs always carry a
    bias, the normalised ones only with InstanceNorm (use_bias, ir:588-593); batch_norm:
    nn.BatchNorm2d's entries after each normalised conv."""
    s = OrderedDict()
    use_bias = use_bias and not batch_norm
    ch = d_channels(input_nc, ndf, n_layers)
    for i, (key, _, normed) in enumerate(d_layers(n_layers)):
        s[key + ".weight"] = (ch[i + 1], ch[i], 4, 4)
        if use_bias or not normed:
            s[key + ".bias"] = (ch[i + 1],)
        if batch_norm and normed:
            s.update(bn_param_shapes(f"model.{int(key.split('.')[1]) + 1}", ch[i + 1]))
    return s


class VGGConv(NamedTuple):
    """One conv + ReLU of vgg16.features[:16]."""
    index: int    # torchvision's index of the conv in vgg16.features (its ReLU is index + 1)
    relu: str     # torchvision's name of its ReLU map
    cin: int
    cout: int
    pool: bool    # MaxPool2d(2) follows the ReLU


# the one description of the stack; everything below that names a VGG layer is derived from it
VGG_STACK = (VGGConv(0, "relu1_1", 3, 64, False), VGGConv(2, "relu1_2", 64, 64, True),
             VGGConv(5, "relu2_1", 64, 128, False), VGGConv(7, "relu2_2", 128, 128, True),
             VGGConv(10, "relu3_1", 128, 256, False), VGGConv(12, "relu3_2", 256, 256, False),
             VGGConv(14, "relu3_3", 256, 256, False))
VGG_CONVS = tuple((c.index, c.cin, c.cout) for c in VGG_STACK)


def vgg_param_shapes():
    s = OrderedDict()
    for i, ci, co in VGG_CONVS:
        s[f"{i}.weight"] = (co, ci, 3, 3); s[f"{i}.bias"] = (co,)
    return s


class ParamStore:
    """Flat fp32 parameter / gradient / Adam-moment buffers for one network.

    BatchNorm's running statistics (``buffers``) are tensors of their own, outside the flat
    range Adam and the gradient reduce walk: fp32 on the device, num_batches_tracked an int64
    scalar on the host (momentum is fixed, so no kernel reads it)."""

    def __init__(self, shapes: "OrderedDict[str, tuple]", device, with_grad=True, with_adam=True):
        self.layout = [k for k in shapes if not k.endswith(".filt")]   # state order, buffers included
        self.buffers = OrderedDict()
        for k in self.layout:
            if k.endswith(".running_mean"):
                self.buffers[k] = torch.zeros(shapes[k], device=device)
            elif k.endswith(".running_var"):
                self.buffers[k] = torch.ones(shapes[k], device=device)
            elif k.endswith(".num_batches_tracked"):
                self.buffers[k] = torch.zeros((), dtype=torch.int64)
        self.shapes = OrderedDict((k, tuple(shapes[k])) for k in self.layout if k not in self.buffers)
        self.offsets, off = {}, 0
        for k, shp in self.shapes.items():
            self.offsets[k] = off
            off += math.prod(shp)
            off = (off + 63) // 64 * 64  # 256-byte aligned slices
        self.numel = off
        self.device = device
        self.flat = torch.zeros(off, device=device)
        self.grad = torch.zeros(off, device=device) if with_grad else None
        self.m = torch.zeros(off, device=device) if with_adam else None
        self.v = torch.zeros(off, device=device) if with_adam else None
        self.ema = None         # enable_ema(): the parameters' moving average, updated by Adam's pass
        self.step_count = 0
        self.dev_adam = False   # GANStep: step count on the device (irgan_adam_prep)
        self._count = self._prm = None
        self._count_host = 0
        self._clip_ws = None    # adam_begin(max_norm=): the norm reduction's fp64 partials

    def krsc(self, k, buf=None):
        buf = self.flat if buf is None else buf
        o = self.offsets[k]
        return buf[o:o + math.prod(self.shapes[k])]

    def oihw(self, k, buf=None):
        """The reference-layout view: OIHW shape over KRSC storage."""
        shp = self.shapes[k]
        t = self.krsc(k, buf)
        if len(shp) == 4:
            O, I, KH, KW = shp
            return t.view(O, KH, KW, I).permute(0, 3, 1, 2)
        return t.view(shp)

    @torch.no_grad()
    def load(self, state: dict, strict=False):
        """Copy OIHW tensors (reference checkpoint / state_dict) into the store."""
        missing = []
        for k in self.layout:
            if k not in state:
                missing.append(k)
                continue
            src = state[k]
            dst = self.buffers[k] if k in self.buffers else self.oihw(k)
            if tuple(src.shape) != tuple(dst.shape):
                raise RuntimeError(f"size mismatch for {k}: copying {tuple(src.shape)} into {tuple(dst.shape)}")
            dst.copy_(src.to(dst.device, dst.dtype))
        if strict and missing:
            raise RuntimeError(f"missing keys {missing}")
        return missing

    def state(self, buf=None):
        """Parameters (of ``buf``, default the weights) and, for the weights, BatchNorm's buffers,
        in state_dict order."""
        if buf is not None:
            return OrderedDict((k, self.oihw(k, buf)) for k in self.shapes)
        return OrderedDict((k, self.buffers[k] if k in self.buffers else self.oihw(k)) for k in self.layout)

    def zero_grad(self):
        self.grad.zero_()

    def adam_state_dict(self, lr, betas=(0.5, 0.999), eps=1e-8, initial_lr=None):
        """The Adam moments as a ``torch.optim.Adam.state_dict()`` (ir:1601-1609):
        parameter indices follow the module's ``parameters()`` order (the
        state_dict order without buffers), tensors in OIHW fp32 on the CPU, so the
        file loads into the reference's optimizer unchanged."""
        state = {}
        if self.step_count > 0:
            for i, k in enumerate(self.shapes):
                state[i] = {"step": torch.tensor(float(self.step_count)),
                            "exp_avg": self.oihw(k, self.m).detach().cpu().contiguous(),
                            "exp_avg_sq": self.oihw(k, self.v).detach().cpu().contiguous()}
        group = {"lr": lr, "betas": tuple(betas), "eps": eps, "weight_decay": 0, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(self.shapes)))}
        if initial_lr is not None:
            group["initial_lr"] = initial_lr   # LambdaLR's key (ir:1606-1609)
        return {"state": state, "param_groups": [group]}

    @torch.no_grad()
    def load_adam_state_dict(self, sd):
        """Inverse of adam_state_dict (also accepts a reference optimizer file)."""
        st = sd["state"]
        if not st:
            self.m.zero_()
            self.v.zero_()
            self.step_count = 0
            return
        steps = set()
        for i, k in enumerate(self.shapes):
            e = st[i]
            self.oihw(k, self.m).copy_(e["exp_avg"].to(self.device, torch.float32))
            self.oihw(k, self.v).copy_(e["exp_avg_sq"].to(self.device, torch.float32))
            steps.add(int(float(e["step"])))
        if len(steps) != 1:
            raise RuntimeError(f"per-parameter Adam step counts differ: {sorted(steps)}")
        self.step_count = steps.pop()

    def adam_step(self, lr, b1=0.5, b2=0.999, eps=1e-8, max_norm=0.0):
        self.adam_begin(lr, b1, b2, eps, max_norm=max_norm)(0, self.numel)

    @torch.no_grad()
    def enable_ema(self):
        """Allocate ``ema`` as a copy of the parameters as they are now (once; a second call
        keeps the average)."""
        if self.ema is None:
            self.ema = self.flat.clone()

    @torch.no_grad()
    def swap_ema(self):
        """Exchange the CONTENTS of ``flat`` and ``ema``: the packs and the modules' parameters
        point into ``flat``, so the tensors stay where they are.  The caller repacks."""
        if self.ema is None:
            raise RuntimeError("swap_ema: no EMA buffer (enable_ema() first)")
        tmp = self.flat.clone()
        self.flat.copy_(self.ema)
        self.ema.copy_(tmp)

    def adam_begin(self, lr, b1=0.5, b2=0.999, eps=1e-8, ema_decay=0.0, max_norm=0.0, norm_out=None):
        """Count one optimizer step and return apply(start, end), the Adam update of
        the flat slice [start, end): a step may be applied bucket by bucket as each
        bucket's gradient all-reduce completes (BucketedAllreduce.finish).  With ``ema_decay``
        and an ``ema`` buffer the same launch also moves ema[start:end] towards the new
        parameters (ops.ema_weight); otherwise ``ema`` is not touched.

        ``max_norm`` > 0 clips by the global L2 norm (torch.nn.utils.clip_grad_norm_ in front of
        the optimizer step): the norm is taken over the WHOLE ``grad`` buffer when apply runs,
        so apply is marked ``whole`` and takes (0, numel) only, once, after the gradient is
        final; Adam consumes grad * coef in its own launch and ``grad`` stays unscaled.
        ``norm_out`` (fp64[1] on the device, optional) receives the norm."""
        ema = self.ema if ema_decay else None
        self.step_count += 1
        t = self.step_count
        if max_norm:
            return self._adam_begin_clip(t, lr, b1, b2, eps, ema, ema_decay, float(max_norm), norm_out)
        if self.dev_adam:
            # the count and the bias corrections on the device (a captured step replays with
            # the right t); the device count is resynced to the host's after a state load
            if self._count is None:
                self._dev_state()
            if self._count_host != t - 1:
                self._count.fill_(t - 1)
            ops.adam_prep(self._count, lr, b1, b2, self._prm, None if ema is None else ema_decay)
            self._count_host = t

            def apply_dev(a, b):
                ops.adam_dev(self.flat[a:b], self.grad[a:b], self.m[a:b], self.v[a:b], self._prm, b1, b2, eps,
                             None if ema is None else ema[a:b])
            return apply_dev

        def apply(a, b):
            ops.adam(self.flat[a:b], self.grad[a:b], self.m[a:b], self.v[a:b], t, lr, b1, b2, eps,
                     None if ema is None else ema[a:b], ema_decay)
        return apply

    def _dev_state(self):
        """The device step count and the Adam launches' coefficients, allocated once."""
        self._count = torch.zeros(1, dtype=torch.int32, device=self.device)
        # {step_size, bc2_sqrt, EMA weight, clip coefficient}: the last two written only when used
        self._prm = torch.zeros(4, dtype=torch.float32, device=self.device)
        self._count_host = 0

    def _adam_begin_clip(self, t, lr, b1, b2, eps, ema, ema_decay, max_norm, norm_out):
        """adam_begin with ``max_norm``: reduction over the whole buffer -> coefficient -> Adam,
        queued when apply runs.  Device count: the clip form of the prep (ops.adam_clip_prep)
        sums the partials, so there is no host sync and no launch beyond the reduction.  Host
        count (ParamStore.adam_step users): the norm is read back (ops.grad_norm, one sync)."""
        if self._clip_ws is None:
            self._clip_ws = torch.zeros(ops.grad_sumsq_parts(self.numel), dtype=torch.float64, device=self.device)
        ws, n = self._clip_ws, self.numel
        if self.dev_adam:
            if self._count is None:
                self._dev_state()
            if self._count_host != t - 1:
                self._count.fill_(t - 1)
            self._count_host = t

        def apply(a, b):
            if (a, b) != (0, n):
                raise ValueError(f"a clipped Adam step is applied once over the whole buffer (0, {n}), got ({a}, {b})")
            if self.dev_adam:
                ops.grad_sumsq(self.grad, ws)
                ops.adam_clip_prep(self._count, lr, b1, b2, self._prm, ws, n, max_norm, norm_out,
                                   ema_decay if ema is not None else 0.0)
                ops.adam_dev(self.flat, self.grad, self.m, self.v, self._prm, b1, b2, eps, ema, clip=True)
                return
            norm = ops.grad_norm(self.grad, ws)
            if norm_out is not None:
                norm_out.fill_(norm)
            ops.adam(self.flat, self.grad, self.m, self.v, t, lr, b1, b2, eps, ema, ema_decay,
                     coef=ops.clip_coef(norm, max_norm))
        apply.whole = True
        return apply


def _pc(store: ParamStore, key: str, spec: ConvSpec, dtype, need_dgrad=True):
    """Packed conv of state key ``key``; its bias only if the layout has one (use_bias)."""
    bias = store.krsc(key + ".bias") if key + ".bias" in store.shapes else None
    return PackedConv(spec, store.krsc(key + ".weight"), bias, dtype, need_dgrad=need_dgrad)


class Buffers:
    """Device buffers keyed by name (allocated once per shape) plus the forward
    state a backward needs (``state``: activation lists, the input shape).

    The fused step reuses one long-lived set per engine.  The module API
    (autograd.Function wrappers) gives every forward call a fresh set that its
    ctx keeps until the backward, so interleaved calls -- netD(real), netD(fake),
    then backward (ir:1642-1650) -- each back-propagate through their own
    activations and InstanceNorm statistics."""

    def __init__(self, device):
        self.device, self.d, self.state = device, {}, {}

    def get(self, name, shape, dtype):
        t = self.d.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self.d[name] = t
        return t

    def zeros(self, name, shape, dtype):
        """Like get(), zero-filled when (re)allocated: padding channels stay 0."""
        t = self.d.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            t = torch.zeros(shape, dtype=dtype, device=self.device)
            self.d[name] = t
        return t

    def flat(self, name, numel, dtype=torch.float32):
        t = self.d.get(name)
        if t is None or t.numel() < numel or t.dtype != dtype:
            t = torch.empty(numel, dtype=dtype, device=self.device)
            self.d[name] = t
        return t


class INLayer:
    """Per-layer InstanceNorm statistics kept from forward to backward.

    The conv bias in front of an InstanceNorm has an exactly-zero gradient
    (IN subtracts the per-channel mean, so the bias never reaches any output);
    the reference's fp32 autograd produces rounding noise there.
    By default the exact zero is kept (no reduction, no atomics); set
    ``INLayer.sum_bias_grad = True`` to accumulate the fp32 sum of dx instead.
    ``fused_stats``: take the forward statistics from the producing conv's epilogue
    where a fused kernel exists (irgan_conv_fwd_stats) instead of a separate pass.
    """
    fused_stats = True
    fused_resample = True
    sum_bias_grad = False

    @staticmethod
    def _work(bufs: Buffers, N, C):
        """The norm kernels' shared fp64 scratch: ops.IN_PARTS doubles per (n, c)."""
        return bufs.flat("in_work", ops.IN_PARTS * N * C, torch.float64)

    @staticmethod
    def _red(bufs: Buffers, N, C):
        """The backward's {mean g, mean g*xhat} per (n, c)."""
        return bufs.flat("in_red", 2 * N * C)

    @staticmethod
    def _no_fp8():
        raise NotImplementedError("the fp8 path runs with InstanceNorm (norm='instance')")

    def fwd(self, bufs: Buffers, name: str, x: Feat, y: Feat, act, res: Feat = None, xhat=None, nb=0, q8=None):
        """nb > 0: x's statistics partials are already in the shared work buffer
        (written by the producing conv, conv_fwd); only the reduction runs.
        The {mean, rstd} table stays in ``bufs`` under ``name`` for bwd().
        q8 (an ops.Fp8Out): also write y's fp8 copy (ops.in_apply)."""
        mr = self._stats(bufs, name, x, nb)
        ops.in_apply(x, mr, y, act=act, res=res, xhat=xhat, q8=q8 and q8.side)
        if q8 is not None:
            q8.finish(y)

    def _stats(self, bufs: Buffers, name: str, x: Feat, nb):
        """x's {mean, rstd} table (kept for bwd()), from the nb partials per image a conv left
        in the work buffer or, with none, from a statistics pass over x."""
        work = self._work(bufs, x.N, x.C)
        mr = bufs.get("mr_" + name, (x.N * x.C * 2,), torch.float32)
        if nb:
            ops.in_finalize(x, work, nb, mr)
        else:
            ops.in_stats(x, work, mr)
        return mr

    def _conv(self, bufs: Buffers, pc, x: Feat, z: Feat, conv8=None):
        """z = conv(x); returns the statistics partials per image the conv's epilogue left in the
        work buffer (0: none).  conv8 = (w8, dqw, x8, dqx): the conv on fp8 operands
        (ops.conv_fwd_fp8; x unused) -- the one way a norm layer is handed an fp8 conv."""
        work = self._work(bufs, z.N, z.C)
        if conv8 is not None:
            w8, dqw, x8, dqx = conv8
            return ops.conv_fwd_fp8(pc, w8, dqw, x8, dqx, z, part=work)
        nb = ops.conv_fwd_stats(pc, x, z, work) if INLayer.fused_stats else 0
        if not nb:
            ops.conv_fwd(pc, x, z)
        return nb

    def conv_fwd(self, bufs: Buffers, name: str, pc, x: Feat, z: Feat, y: Feat, act, res: Feat = None, conv8=None,
                 q8=None):
        """z = conv(x) (kept for the backward), y = act(norm(z) [+ res]): the statistics come
        from the conv's epilogue when it has a fused kernel (_conv)."""
        self.fwd(bufs, name, z, y, act, res=res, nb=self._conv(bufs, pc, x, z, conv8), q8=q8)

    def conv_stats(self, bufs: Buffers, name: str, pc, x: Feat, z: Feat, conv8=None):
        """z = conv(x) and z's {mean, rstd} table (returned, kept for bwd()) -- no apply:
        the consumer normalises on load (ops.blur_down_in / ops.upsample_in)."""
        return self._stats(bufs, name, z, self._conv(bufs, pc, x, z, conv8))

    def resample_fwd(self, bufs: Buffers, name: str, pc, x: Feat, z: Feat, a_name: str, act, y: Feat, fused, plain,
                     conv8=None, q8=None):
        """y = resample(act(IN(conv(x)))): the IN apply fused into the resample when
        ``fused(z, mr, act, y)`` takes the shapes, else apply into bufs[a_name] + ``plain``.
        conv8: the conv on fp8 operands (_conv); q8 (an ops.Fp8Out): also y's e4m3 copy."""
        mr = self.conv_stats(bufs, name, pc, x, z, conv8=conv8)
        side = q8.side if q8 is not None else None
        taken = INLayer.fused_resample and (fused(z, mr, act, y, q8=side) if side is not None else
                                            fused(z, mr, act, y))
        if not taken:
            a = Feat(bufs.get(a_name, (z.N, z.H, z.W, z.C), z.t.dtype))
            ops.in_apply(z, mr, a, act=act)
            plain(a, y)
        if q8 is not None:
            q8.finish(y, taken)

    def bwd(self, bufs: Buffers, name: str, dy: Feat, z: Feat, act, dx: Feat, db=None, dy2: Feat = None, q8=None,
            wgrad=True):
        """z: the PRE-norm input kept from forward; act: the activation after IN.
        q8 (an ops.Fp8Out): also write dx's fp8 copy (ops.in_backward).  wgrad: accumulate the
        norm's own parameter gradients (BNLayer; InstanceNorm has none)."""
        N, C = z.N, z.C
        work = self._work(bufs, N, C)
        red = self._red(bufs, N, C)
        mr = bufs.d["mr_" + name]
        ops.in_backward(dy, z, act, mr, work, red, dx, db=db if INLayer.sum_bias_grad else None, dy2=dy2,
                        q8=q8.side if q8 is not None and not INLayer.sum_bias_grad else None)
        if q8 is not None:
            q8.finish(dx)

    def _resample_bwd_plain(self, bufs, name, dy_small, z, act, dz, plain, db=None, q8=None):
        """``plain(dy_small, dz)`` writes the resampled gradient, bwd() turns it into dz in place."""
        plain(dy_small, dz)
        self.bwd(bufs, name, dz, z, act, dz, db=db, q8=q8)

    def resample_bwd(self, bufs: Buffers, name: str, dy_small: Feat, z: Feat, act, dz: Feat, fused, plain, db=None,
                     q8=None):
        """Backward of resample_fwd() from the resample's output gradient ``dy_small`` to dz:
        ``fused(dy_small, z, act, mr, work, red, dz)`` where it takes the call (the resample's
        adjoint with the IN backward on its output, ops.blur_down_bwd_in), else
        ``plain(dy_small, dz)`` + bwd().  A bias-gradient sum and an e4m3 copy keep the plain path."""
        want_db = db is not None and INLayer.sum_bias_grad
        if ops.RESAMPLE_BWD_FUSED[0] and q8 is None and not want_db:
            N, C = z.N, z.C
            if fused(dy_small, z, act, bufs.d["mr_" + name], self._work(bufs, N, C), self._red(bufs, N, C), dz):
                return
        self._resample_bwd_plain(bufs, name, dy_small, z, act, dz, plain, db=db, q8=q8)

class NoNorm(INLayer):
    """norm='none' (ir:162-163: ``lambda num_features: Identity()``): the layer is just its
    activation, y = act(z) [+ res], and the conv in front has no bias (use_bias is False,
    ir:450-455, 588-593).  Same interface as INLayer: the forward applies an identity
    {mean 0, rstd 1} table through the same apply / fused-resample kernels ((z - 0) * 1 = z
    exactly), the backward is the activation's derivative."""

    def _ident(self, bufs: Buffers, name: str, N: int, C: int) -> torch.Tensor:
        mr = bufs.get("mr_" + name, (N * C * 2,), torch.float32)
        if bufs.state.get("ident_" + name) is not mr:
            mr.view(-1, 2)[:, 0] = 0.0
            mr.view(-1, 2)[:, 1] = 1.0
            bufs.state["ident_" + name] = mr
        return mr

    def fwd(self, bufs, name, x, y, act, res=None, xhat=None, nb=0, q8=None):
        if q8 is not None:
            self._no_fp8()
        ops.in_apply(x, self._ident(bufs, name, x.N, x.C), y, act=act, res=res)

    def _conv(self, bufs, pc, x, z, conv8=None):
        if conv8 is not None:
            self._no_fp8()
        ops.conv_fwd(pc, x, z, bias=pc.bias is not None)
        return 0

    def conv_stats(self, bufs, name, pc, x, z, conv8=None):
        self._conv(bufs, pc, x, z, conv8)
        return self._ident(bufs, name, z.N, z.C)

    def bwd(self, bufs, name, dy, z, act, dx, db=None, dy2=None, q8=None, wgrad=True):
        if dy2 is not None or q8 is not None:
            raise NotImplementedError("NoNorm.bwd: dy2 / q8 are InstanceNorm-path features")
        if act == ACT_NONE and dx.t.data_ptr() == dy.t.data_ptr() and dx.off == dy.off:
            pass                                   # identity, in place
        else:
            ops.act_bwd(dy, z, act, dx)            # z > 0 <=> act(z) > 0 for ReLU / LeakyReLU
        if db is not None:
            ops.channel_sum(dx, db)

    def resample_bwd(self, bufs, name, dy_small, z, act, dz, fused, plain, db=None, q8=None):
        self._resample_bwd_plain(bufs, name, dy_small, z, act, dz, plain, db=db, q8=q8)

class BNSync:
    """The SyncBN handle of BNLayer: the process group whose ranks share BatchNorm statistics
    (``group`` None is the default group, so "no synchronisation" is a missing handle, not a
    None group).  ``all_reduce`` sums an fp64 device buffer over the ranks in place, as a
    synchronous-semantics collective on the CURRENT stream: the layer's next kernel on that
    stream reads the reduced values.  Every rank issues these calls in program order -- the
    same order on all of them -- so they pair up with each other across the main and the side
    stream and with the asynchronous gradient buckets (BucketedAllreduce) on the same group.
    RCCL ('nccl') reduces the device tensor; any other backend (gloo in the tests) is staged
    through the host, as replicas_identical does."""

    def __init__(self, group=None):
        import torch.distributed as dist
        self.group = group
        self.on_device = dist.get_backend(group) == "nccl"

    def all_reduce(self, t: torch.Tensor):
        import torch.distributed as dist
        if self.on_device:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
            return
        h = t.cpu()                # waits for the current stream's local sums
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group)
        t.copy_(h)                 # on the current stream, in front of the finishing half


class BNLayer(INLayer):
    """norm='batch' (ir:158-159: nn.BatchNorm2d, eps 1e-5, momentum 0.1, affine, running
    statistics); the conv in front has no bias (ir:450-455, 588-593).  Same
    interface as INLayer.  gamma / beta (and their gradients) are the layer's slices of the
    ParamStore flat buffers, so Adam, the optimizer state and the gradient reduce cover them
    like any conv weight; the running buffers are ``store.buffers`` tensors.

    ``groups``: statistics per group of N / groups consecutive samples (csrc/batchnorm.hip):
    1 is nn.BatchNorm2d over the batch; the fused step's D forward on [real; fake] runs with 2,
    which is the reference's netD(real), netD(fake) (ir:1642-1643) -- the running buffers take
    the groups in that order.  ``repeat``: the running update of one forward applied that many
    times, for a forward that stands for several identical ones of the reference (the fused step
    runs G once where ir:1638 and ir:1657 run it twice on the same weights and input).
    ``training`` False: the running statistics normalise and nothing is updated (model.eval()).

    ``sync`` (a BNSync, or None: the local batch): in training mode the statistics of a group are
    those of the group's samples on every rank of the handle's process group, nn.SyncBatchNorm's
    semantics.  The forward runs local sums -> one all-reduce(SUM) of groups * (2C + 1) doubles ->
    finish, the backward the same with {sum g, sum g * xhat}; the buffers are this layer's own
    entries of ``bufs`` ("bnsync_" / "bnsyncb_" + name), never a shared scratch: BatchNorm layers
    run on the main and on the side stream, and the collective is asynchronous to the host.
    Every rank finishes from the same reduced bytes, so tables and running buffers stay
    bit-identical over the replicas.  dgamma / dbeta take the LOCAL sums: they lie in the flat
    gradient buffer, whose all-reduce averages them as DDP does around nn.SyncBatchNorm."""

    def __init__(self, store: "ParamStore", key: str):
        self.store, self.key = store, key
        self.gamma, self.beta = store.krsc(key + ".weight"), store.krsc(key + ".bias")
        self.dgamma = store.krsc(key + ".weight", store.grad) if store.grad is not None else None
        self.dbeta = store.krsc(key + ".bias", store.grad) if store.grad is not None else None
        self.running_mean = store.buffers[key + ".running_mean"]
        self.running_var = store.buffers[key + ".running_var"]
        self.num_batches_tracked = store.buffers[key + ".num_batches_tracked"]
        self.training, self.groups, self.repeat, self.sync = True, 1, 1, None

    def configure(self, training=True, groups=1, repeat=1, sync: BNSync = None):
        self.training, self.groups, self.repeat, self.sync = bool(training), int(groups), int(repeat), sync

    def _tables(self, bufs: Buffers, name: str, x: Feat, nb=0, want_ab=False):
        """x's {mean, rstd} table (kept for bwd()) and, if asked, the {shift, scale} one."""
        N, C = x.N, x.C
        mr = bufs.get("mr_" + name, (N * C * ops.BN_TABLE,), torch.float32)
        ab = bufs.get("ab_" + name, (N * C * 2,), torch.float32) if want_ab else None
        sync = self.sync if self.training else None   # eval mode reads no batch statistics
        bufs.state["bn_" + name] = (self.training, self.groups, sync)
        if not self.training:
            ops.bn_eval_table(self.running_mean, self.running_var, self.gamma, self.beta, N, mr, ab)
            return mr, ab
        work = self._work(bufs, N, C)
        if sync is not None:
            sums = bufs.get("bnsync_" + name, (ops.bn_sync_numel(self.groups, C),), torch.float64)
            ops.bn_sync_sums(x, work, sums, self.groups, nb=nb)
            sync.all_reduce(sums)
            ops.bn_sync_finalize(sums, N, C, mr, self.groups, self.gamma, self.beta, self.running_mean,
                                 self.running_var, self.repeat, ab=ab)
        else:
            ops.bn_stats(x, work, mr, self.groups, self.gamma, self.beta, self.running_mean, self.running_var,
                         self.repeat, ab=ab, nb=nb)
        self.num_batches_tracked += self.repeat * self.groups
        return mr, ab

    def fwd(self, bufs, name, x, y, act, res=None, xhat=None, nb=0, q8=None):
        if q8 is not None or xhat is not None:
            self._no_fp8()
        mr, _ = self._tables(bufs, name, x, nb)
        ops.bn_apply(x, mr, self.gamma, self.beta, y, act=act, res=res)

    def _conv(self, bufs, pc, x, z, conv8=None):
        """z = conv(x); the partials per image in the work buffer (0: none were written)."""
        if conv8 is not None:
            self._no_fp8()
        nb = 0
        if self.training and INLayer.fused_stats:
            nb = ops.conv_fwd_stats(pc, x, z, self._work(bufs, z.N, z.C))
        if not nb:
            ops.conv_fwd(pc, x, z, bias=pc.bias is not None)
        return nb

    def conv_stats(self, bufs, name, pc, x, z, conv8=None):
        """z = conv(x); returns the {shift, scale} table the fused resample consumers read with
        ops.NORM_AFFINE (the {mean, rstd} table stays in ``bufs`` for bwd())."""
        return self._tables(bufs, name, z, self._conv(bufs, pc, x, z, conv8), want_ab=True)[1]

    def resample_fwd(self, bufs, name, pc, x, z, a_name, act, y, fused, plain, conv8=None, q8=None):
        if q8 is not None:
            self._no_fp8()
        ab = self.conv_stats(bufs, name, pc, x, z, conv8=conv8)
        if INLayer.fused_resample and fused(z, ab, act | ops.NORM_AFFINE, y):
            return
        a = Feat(bufs.get(a_name, (z.N, z.H, z.W, z.C), z.t.dtype))
        ops.bn_apply(z, bufs.d["mr_" + name], self.gamma, self.beta, a, act=act)
        plain(a, y)

    def bwd(self, bufs, name, dy, z, act, dx, db=None, dy2=None, q8=None, wgrad=True):
        if q8 is not None:
            self._no_fp8()
        training, groups, sync = bufs.state["bn_" + name]
        N, C = z.N, z.C
        work = self._work(bufs, N, C)
        if sync is not None:   # the forward was synchronised: so are the dx means (wgrad or not)
            mr = bufs.d["mr_" + name]
            bsums = bufs.get("bnsyncb_" + name, (ops.bn_sync_numel(groups, C),), torch.float64)
            ops.bn_sync_backward_sums(dy, z, act, mr, self.gamma, self.beta, work, bsums,
                                      dgamma=self.dgamma if wgrad else None, dbeta=self.dbeta if wgrad else None,
                                      groups=groups, dy2=dy2)
            sync.all_reduce(bsums)
            ops.bn_sync_backward_dx(dy, z, act, mr, self.gamma, self.beta, bsums, dx, groups=groups, dy2=dy2)
            return
        red = self._red(bufs, N, C)
        ops.bn_backward(dy, z, act, bufs.d["mr_" + name], self.gamma, self.beta, work, red, dx,
                        dgamma=self.dgamma if wgrad else None, dbeta=self.dbeta if wgrad else None, groups=groups,
                        eval_mode=not training, dy2=dy2)

    def resample_bwd(self, bufs, name, dy_small, z, act, dz, fused, plain, db=None, q8=None):
        self._resample_bwd_plain(bufs, name, dy_small, z, act, dz, plain, db=db, q8=q8)


def make_norm(norm: str, store: "ParamStore" = None, key: str = None) -> INLayer:
    """The engine's per-layer norm for Config.norm (ir:154-165): 'instance', 'none' or 'batch'.
    'batch' (BNLayer) takes the layer's ParamStore and the state key of its nn.BatchNorm2d
    module.  Its statistics are the local batch's unless the layer is handed a BNSync handle
    (BNLayer.sync): GANStep does that for the fused step under Config.sync_bn with more than one
    data-parallel rank, where the reference semantics need the global batch (SyncBN); without
    the option GANTrainer refuses that combination."""
    if norm == "instance":
        return INLayer()
    if norm in ("none", None):
        return NoNorm()
    if norm == "batch":
        return BNLayer(store, key)
    raise NotImplementedError(f"norm '{norm}': the HIP engines implement 'instance', 'none' and 'batch'")


def res_conv_keys(padding_type="reflect", use_dropout=False):
    """Indices of the two convs inside ResnetBlock.conv_block (ir:375-411): the pad
    modules exist only for reflect / replicate, the Dropout only with use_dropout."""
    if padding_type not in ("reflect", "replicate", "zero"):
        raise NotImplementedError(f"Padding [{padding_type}] is not implemented")
    first = 0 if padding_type == "zero" else 1
    second = first + 3 + (1 if use_dropout else 0) + (0 if padding_type == "zero" else 1)
    return first, second


class Fp8Conv(NamedTuple):
    """One conv of the fp8 path (fp8_plan): its parameter key, the indices of the e4m3 copies of
    its forward and flipped weight images (Fp8Weights) and the scale slots (Fp8Acts) of its
    operand and of its dY."""
    key: str
    w_fwd: int
    w_flip: int
    s_x: int
    s_dy: int


def fp8_plan(n_blocks: int, fp8_ud: bool):
    """The fp8 layout of a generator, the one place that numbers it (table: DESIGN.md s.2): a
    record per e4m3 conv -- the two convs of every ResnetBlock, then down2 and up1_conv when
    ``fp8_ud`` -- and the named (start, count) slot ranges the per-call snapshot and
    Fp8Acts.update() run over.  down2 and up1_conv share the operand slot: down2 reads the x1
    slice of up1_conv's concat.  Pure host arithmetic, no device."""
    n = n_blocks
    k1, k2 = res_conv_keys()   # the fp8 path runs the default ResnetBlock
    convs = []
    for b in range(n):
        convs.append(Fp8Conv(f"resblocks.{b}.conv_block.{k1}", 4 * b, 4 * b + 1, 2 * b, 2 * n + 2 * b + 1))
        convs.append(Fp8Conv(f"resblocks.{b}.conv_block.{k2}", 4 * b + 2, 4 * b + 3, 2 * b + 1, 2 * n + 2 * b))
    if fp8_ud:
        convs.append(Fp8Conv("down2.0", 4 * n, 4 * n + 1, 4 * n, 4 * n + 2))
        convs.append(Fp8Conv("up1_conv.0", 4 * n + 2, 4 * n + 3, 4 * n, 4 * n + 1))
    slots = {"fwd": (0, 2 * n),         # the ResnetBlock convs' operands
             "dy": (2 * n, 2 * n),      # their dY
             "cat": (4 * n, 1),         # the [up(h) | x1] concat
             "ud_dy": (4 * n + 1, 2),   # up1_conv's, down2's dY
             "x1": (4 * n + 3, 1)}      # down2's own x1 copy on the calibration step
    return convs, slots


class Fp8Call:
    """The fp8 side of one forward call, kept in ``bufs.state["fp8"]`` -- all its backward reads:
    ``on``: which groups run on e4m3 for the call's shape ('res': the ResnetBlock convs, 'ud':
    down2 / up1_conv; GeneratorEngine.fp8_layers); ``calib``: the first 'ud' step (current
    scaling): down2 reads its own copy of x1 (``x1_8c``), scaled from x1 alone, for its forward
    AND its weight gradient, and up1_conv's concat is then scaled as a whole; ``x8``: the e4m3
    operand buffer by layer name, which the weight gradients re-read; ``dq_used``: the
    de-quantisation factors this call's forward made those operands with (one per slot, filled by
    _fp8_roll before the shared slots move on) -- the call's own, so no other forward between
    this one and its backward can change them; ``frozen``: an eval-mode call, whose forward
    reads the shared scales and writes none of them (a backward of it treats its dY slots as
    every backward does)."""

    def __init__(self, on_res, on_ud, calib, dq_used, frozen=False):
        self.on, self.calib, self.x1_8c, self.x8 = {"res": on_res, "ud": on_ud}, calib, None, {}
        self.dq_used, self.frozen = dq_used, frozen


class GenConv:
    """A generator conv in front of its norm layer, as the step names it: the PackedConv, its
    parameter key, the norm and, for the layers of fp8_plan, the record ``rec``.  Whether a call
    runs the layer on e4m3 or on the engine's dtype is the Fp8Call's decision for the layer's
    ``group``, taken once when the forward starts; the methods here are the same call either way.
    ``xp``: buffer name of the ReplicationPad2d(1) copy of the input (padding 'replicate': the
    conv reads it, it is kept for the weight gradient, and the input gradient is folded back);
    ``dy8``: buffer name of dY's e4m3 copy; ``s_calib``: down2's slot of its own x1 copy."""

    def __init__(self, eng, pc, key, name, group, rec=None, xp=None, dy8="dy8", s_calib=None):
        self.eng, self.pc, self.key, self.name, self.group, self.rec = eng, pc, key, name, group, rec
        self.norm, self.xp, self.dy8, self.s_calib = eng.norms[name], xp, dy8, s_calib

    def _w8(self, k):
        return self.eng.f8w.dst[k], ops.Pi(self.eng.f8w.dq, k)

    def _x8(self, st, used=False):
        """The e4m3 operand and the pointer to its dequantisation factor; ``used``: the one it
        was made with, kept in the call (Fp8Call.dq_used) before the forward moved the slot on."""
        A = self.eng.f8a
        if st.calib and self.s_calib is not None:
            return st.x1_8c, A.dqp(self.s_calib)
        return st.x8[self.name], ops.Pi(st.dq_used, self.rec.s_x) if used else A.dqp(self.rec.s_x)

    def _conv8(self, st):
        return (*self._w8(self.rec.w_fwd), *self._x8(st)) if st.on[self.group] else None

    def feed(self, st, x: Feat):
        """The operand x from a producer without an e4m3 output: a quantise launch."""
        if st.on[self.group]:
            self.eng.f8a.quant(self.rec.s_x, x, st.x8[self.name], record=not st.frozen)

    def side(self, st, sl=None):
        """The ``q8`` of the launch that produces this layer's operand (``sl`` = (off, C): the
        channel slice of it that the launch writes); None on a bf16 call and on the calibration
        step, where calibrate() quantises instead.  A frozen call gets the read-only form."""
        if not st.on[self.group] or (st.calib and self.group == "ud"):
            return None
        x8 = st.x8[self.name]
        return ops.Fp8Out(self.eng.f8a, self.rec.s_x, x8.sl(*sl) if sl else x8, record=not st.frozen)

    def calibrate(self, st, x: Feat):
        """Calibration step: the operand's scale from x alone, then its quantisation."""
        if st.calib and self.group == "ud":
            slot, x8 = (self.s_calib, st.x1_8c) if self.s_calib is not None else (self.rec.s_x, st.x8[self.name])
            self.eng.f8a.calibrate(slot, x, x8)

    def fwd(self, g: Buffers, st, x: Feat, z: Feat, y: Feat, act, res: Feat = None, nxt: "GenConv" = None):
        """z = conv(x) (kept for the backward), y = act(norm(z)) [+ res].  ``nxt``: the layer that
        reads y; the norm's apply writes its e4m3 operand along."""
        if self.xp:
            xp = Feat(g.get(self.xp, (x.N, x.H + 2, x.W + 2, x.C), self.eng.tdt))
            ops.pad(x, xp, 1, "replicate")
            x = xp
        self.norm.conv_fwd(g, self.name, self.pc, x, z, y, act, res=res, conv8=self._conv8(st),
                           q8=nxt.side(st) if nxt else None)

    def resample_fwd(self, g: Buffers, st, x: Feat, z: Feat, a_name, act, y: Feat, fused, plain):
        """z = conv(x), y = resample(act(norm(z))) (INLayer.resample_fwd)."""
        self.norm.resample_fwd(g, self.name, self.pc, x, z, a_name, act, y, fused, plain, conv8=self._conv8(st))

    def bwd(self, g: Buffers, st, dy: Feat, z: Feat, act, dz: Feat, x: Feat, dx: Feat, accumulate=False, padbuf=None,
            pend: list = None, resample=None):
        """Backward of fwd(): dz = the norm's backward of dy (in place when dz is dy), the weight
        gradient from x and dz, dx (+)= backward-data of dz.  The bf16 ResnetBlock convs launch
        the backward-data first, every other case the weight gradient.  ``pend`` (the ResnetBlock
        convs off the e4m3 path): the weight gradient is not launched but appended to it as
        (layer, x, dz) -- the caller launches several at once (wgrad_flush) and keeps x and dz
        unchanged until then.  ``resample`` = (fused, plain): the backward of resample_fwd() --
        dy is the gradient of the resample's output (INLayer.resample_bwd)."""
        e, on = self.eng, st.on[self.group]
        dz8 = Feat(g.get(self.dy8, (*dz.t.shape[:3], dz.C), torch.float8_e4m3fn)) if on else None
        db, q8 = e._bgrad(self.key + ".bias"), ops.Fp8Out(e.f8a, self.rec.s_dy, dz8) if on else None
        if resample is not None:
            self.norm.resample_bwd(g, self.name, dy, z, act, dz, *resample, db=db, q8=q8)
        else:
            self.norm.bwd(g, self.name, dy, z, act, dz, db=db, q8=q8)
        if on:
            self._wgrad(st, x, dz, dz8)
            if self.s_calib is not None:
                st.x1_8c = None   # the calibration step's x1 copy is released here
            ops.conv_dgrad_fp8(self.pc, *self._w8(self.rec.w_flip), dz8, e.f8a.dqp(self.rec.s_dy), dz, dx,
                               accumulate=accumulate)
            return
        if self.group != "res":
            self._wgrad(st, x, dz)
        if self.xp:
            dxp = Feat(g.get("res_dxp", (dx.N, dx.H + 2, dx.W + 2, dx.C), e.tdt))
            ops.conv_dgrad(self.pc, dz, dxp)
            ops.pad_fold(dxp, dx, 1, "replicate", accumulate=accumulate)
        else:
            ops.conv_dgrad(self.pc, dz, dx, accumulate=accumulate, pad_buf=padbuf)
        if self.group == "res":
            xw = Feat(g.d[self.xp]) if self.xp else x
            if pend is None:
                self._wgrad(st, xw, dz)
            else:
                pend.append((self, xw, dz))

    def _wgrad(self, st, x: Feat, dz: Feat, dz8: Feat = None):
        """The weight gradient: on the e4m3 copies (the operand with the scale it was made
        with), on x and dz where that kernel does not take the layer or the call is bf16."""
        e = self.eng
        dw = e.store.krsc(self.key + ".weight", e.store.grad)
        if dz8 is not None:
            x8, dqx = self._x8(st, used=True)
            if ops.conv_wgrad_fp8(self.pc.spec, x8, dz8, dqx, e.f8a.dqp(self.rec.s_dy), dw):
                return
        ops.conv_wgrad(self.pc.spec, x, dz, dw, e.dtype)


def wgrad_flush(eng, pend):
    """Launch the deferred weight gradients ``pend`` (GenConv.bwd; one conv shape): as one grouped
    launch where the library takes them (ops.conv_wgrad_group), else layer by layer."""
    if not pend:
        return
    dws = [eng.store.krsc(c.key + ".weight", eng.store.grad) for c, _, _ in pend]
    if not ops.conv_wgrad_group(pend[0][0].pc.spec, [x for _, x, _ in pend], [dz for _, _, dz in pend], dws,
                                eng.dtype):
        for (c, x, dz), dw in zip(pend, dws):
            ops.conv_wgrad(c.pc.spec, x, dz, dw, eng.dtype)


# ----------------------------------------------------------------------------
# generator  (ir:425-569)
# ----------------------------------------------------------------------------

class GeneratorEngine:
    _pack_batch = None  # ops.PackBatch of self.packs, built on the first pack()

    def __init__(self, store: ParamStore, dtype=BF16, ngf=64, input_nc=1, output_nc=3, n_blocks=9,
                 no_antialias=False, no_antialias_up=False, fp8=False, norm="instance", padding_type="reflect",
                 use_dropout=False, dropout_seed=0):
        """fp8: the ResnetBlock convs and, with the anti-aliased resamplers (the default),
        down2 and up1_conv run on OCP e4m3 operands (BASELINE config 5: forward, backward-
        data interior, weight gradient): per-tensor power-of-two scales, current scaling
        for the re-packed weights, delayed scaling for the activations and gradients they
        read; everything else stays bf16.
        norm / padding_type / use_dropout: the reference's constructor options (ir:154-165,
        375-411, 443-447); the ResnetBlock convs of padding 'replicate' read an explicitly
        padded copy of their input (ops.pad) and fold their input gradient back (ops.pad_fold)."""
        self.store, self.dtype, self.ngf = store, dtype, ngf
        self.fp8 = bool(fp8)
        if self.fp8 and (dtype != BF16 or 4 * ngf % 128):
            raise ValueError("the fp8 path runs on the bf16 engine with 4*ngf % 128 == 0")
        if self.fp8 and (norm != "instance" or padding_type != "reflect" or use_dropout):
            raise ValueError("the fp8 path runs the default ResnetBlock (InstanceNorm, reflect, no dropout)")
        self.norm_type, self.padding_type, self.use_dropout = norm, padding_type, bool(use_dropout)
        self.dropout_seed, self.dropout_calls = int(dropout_seed), 0
        self.training = True
        self.fp8_prepasses = 0   # calibration pre-passes eval-mode forwards have run (forward)
        self.bn_sync = None   # BNSync handle of the fused step's forwards (GANStep, Config.sync_bn)
        self.input_nc, self.output_nc, self.n_blocks = input_nc, output_nc, n_blocks
        self.no_aa, self.no_aa_up = no_antialias, no_antialias_up
        self.tdt = ops.TORCH_DT[dtype]
        c0, c1, c2 = ngf, 2 * ngf, 4 * ngf
        sd = 2 if no_antialias else 1
        S = store
        self.inc = _pc(S, "inc.1", ConvSpec(input_nc, c0, 7, 1, 3, PAD_REFLECT), dtype, need_dgrad=False)
        self.down1 = _pc(S, "down1.0", ConvSpec(c0, c1, 3, sd, 1, PAD_ZERO), dtype)
        self.down2 = _pc(S, "down2.0", ConvSpec(c1, c2, 3, sd, 1, PAD_ZERO), dtype)
        k1, k2 = self.res_keys = res_conv_keys(padding_type, use_dropout)
        rspec = {"reflect": ConvSpec(c2, c2, 3, 1, 1, PAD_REFLECT), "zero": ConvSpec(c2, c2, 3, 1, 1, PAD_ZERO),
                 "replicate": ConvSpec(c2, c2, 3, 1, 0, PAD_ZERO)}[padding_type]   # replicate: on the padded copy
        res = [_pc(S, f"resblocks.{b}.conv_block.{k}", rspec, dtype) for b in range(n_blocks) for k in (k1, k2)]
        if no_antialias_up:
            # ConvTranspose2d(C, C, 3, s2, p1, op1) == backward-data of conv(3, s2, p1)
            self.up1_up = _pc(S, "up1_up", ConvSpec(c2, c2, 3, 2, 1, PAD_ZERO), dtype)
            self.up2_up = _pc(S, "up2_up", ConvSpec(c1, c1, 3, 2, 1, PAD_ZERO), dtype)
        self.up1 = _pc(S, "up1_conv.0", ConvSpec(c2 + c1, c1, 3, 1, 1, PAD_ZERO), dtype)
        self.up2 = _pc(S, "up2_conv.0", ConvSpec(c1 + c0, c0, 3, 1, 1, PAD_ZERO), dtype)
        self.outc = _pc(S, "outc.1", ConvSpec(c0, output_nc, 7, 1, 3, PAD_REFLECT), dtype)
        self.packs = [self.inc, self.down1, self.down2, self.up1, self.up2, self.outc] + res + \
            ([self.up1_up, self.up2_up] if no_antialias_up else [])
        # fp8 on down2 / up1_conv too (ir:477-482, 557-558): their operands come from the
        # fused resamplers (x1 from down1's Downsample, the up-sampled bottleneck)
        # (their kernels take 128-channel K chunks: down2's Cin = 2*ngf must be a multiple of 128)
        self.fp8_ud = self.fp8 and not no_antialias and not no_antialias_up and c1 % 128 == 0
        # name -> state key of the layer's norm module (the index after its conv)
        nkeys = {"inc": "inc.2", "down1": "down1.1", "down2": "down2.1", "up1": "up1_conv.1", "up2": "up2_conv.1"}
        for b in range(n_blocks):
            nkeys[f"r{b}_1"] = f"resblocks.{b}.conv_block.{k1 + 1}"
            nkeys[f"r{b}_2"] = f"resblocks.{b}.conv_block.{k2 + 1}"
        self.norms = {k: make_norm(norm, S, key) for k, key in nkeys.items()}
        assert len(self.norms) == 5 + 2 * n_blocks
        # the layers fp8_plan knows, as the step names them (GenConv); fp8: each with its record,
        # and the e4m3 weight images and scale slots numbered by the plan alone
        recs, self.fp8_slots = fp8_plan(n_blocks, self.fp8_ud) if self.fp8 else ([], {})
        rec = {r.key: r for r in recs}
        xp = "xp{j}_{b}" if padding_type == "replicate" else ""
        convs = [GenConv(self, res[2 * b + j - 1], key, f"r{b}_{j}", "res", rec.get(key), xp=xp.format(j=j, b=b))
                 for b in range(n_blocks) for j, key in ((1, f"resblocks.{b}.conv_block.{k1}"),
                                                         (2, f"resblocks.{b}.conv_block.{k2}"))]
        self.blocks = list(zip(convs[0::2], convs[1::2]))
        self.c_down2 = GenConv(self, self.down2, "down2.0", "down2", "ud", rec.get("down2.0"), dy8="dz2_8",
                               s_calib=self.fp8_slots["x1"][0] if self.fp8_ud else None)
        self.c_up1 = GenConv(self, self.up1, "up1_conv.0", "up1", "ud", rec.get("up1_conv.0"), dy8="dz3_8")
        if self.fp8:
            images = [None] * (2 * len(recs))
            for c in convs + [self.c_down2, self.c_up1]:
                if c.rec is not None:
                    images[c.rec.w_fwd], images[c.rec.w_flip] = c.pc.fwd, c.pc.dg[0][2]
            self.f8w = ops.Fp8Weights(images, store.device)
            self.f8a = ops.Fp8Acts(sum(n for _, n in self.fp8_slots.values()), store.device)
        self.bufs = Buffers(store.device)

    def pack(self):
        if self._pack_batch is None:
            self._pack_batch = ops.PackBatch(self.packs)
        self._pack_batch.run()
        if self.fp8:
            self.f8w.run()

    def _fp8_call(self, g: Buffers, B, H, W, frozen=False) -> Fp8Call:
        """The call's Fp8Call, with the e4m3 operand buffers of the groups that run on fp8: one per
        ResnetBlock conv input; ``cat1_8`` for up1_conv's concat, whose x1 slice is down2's operand
        except on the calibration step (never a frozen call: its slots are calibrated before)."""
        f8, ud = self.fp8_layers(B, H, W)
        dq_used = g.get("fp8_dq_used", (len(self.f8a.seen),), torch.float32) if f8 else None
        st = Fp8Call(f8, ud, ud and not frozen and not self.f8a.seen[self.fp8_slots["cat"][0]], dq_used, frozen)
        H1, W1, H2, W2 = self._dims(H, W)
        c1, c2, e4m3 = 2 * self.ngf, 4 * self.ngf, torch.float8_e4m3fn
        if f8:
            for k, c in enumerate(c for pair in self.blocks for c in pair):
                st.x8[c.name] = Feat(g.get(f"x8_{k}", (B, H2, W2, c2), e4m3))
        if ud:
            st.x8["up1"] = Feat(g.get("cat1_8", (B, H1, W1, c2 + c1), e4m3))
            st.x8["down2"] = st.x8["up1"].sl(c2, c1)
        if st.calib:
            st.x1_8c = Feat(torch.empty((B, H1, W1, c1), dtype=e4m3, device=g.device))
        return st

    def _fp8_roll(self, st: Fp8Call, group, rng, snapshot=False):
        """After the last use of the named slot range ``rng`` (fp8_plan) in a pass: the recorded
        maxima become the next step's scales.  snapshot: first keep the factors just used in the
        call -- the backward's weight gradients re-read the forward's e4m3 copies with them.
        The forward of a frozen call (its ``snapshot`` rolls) keeps its factors and moves nothing;
        its backward, if one runs, records and rolls the dY slots like any other backward."""
        if st.on[group]:
            start, n = self.fp8_slots[rng]
            if snapshot:
                st.dq_used[start:start + n].copy_(self.f8a.dq[start:start + n])
            if not (snapshot and st.frozen):
                self.f8a.update(start, n)

    def reset_fp8_scales(self):
        """Every fp8 scale slot unseen again: the next forward calibrates from its own batch."""
        if self.fp8:
            self.f8a.reset()

    def _fp8_needs_calibration(self, B, H, W):
        """An eval-mode forward of this shape would read a forward slot nothing has calibrated."""
        res, ud = self.fp8_layers(B, H, W)
        (f0, fn), cat = self.fp8_slots["fwd"], self.fp8_slots["cat"][0]
        return (res and not all(self.f8a.seen[f0:f0 + fn])) or (ud and not self.f8a.seen[cat])

    def _bgrad(self, key):
        """Flat-buffer slice of parameter ``key``'s gradient, None when the layout has no
        such parameter (use_bias False: no conv biases)."""
        return self.store.krsc(key, self.store.grad) if key in self.store.shapes else None

    # -- shapes
    def _dims(self, H, W):
        H1, W1 = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        H2, W2 = (H1 - 1) // 2 + 1, (W1 - 1) // 2 + 1
        return H1, W1, H2, W2

    def fp8_layers(self, B, H, W):
        """(resblocks, down2 / up1_conv) on e4m3 for a (B, H, W) input: the fp8 conv fuses the
        InstanceNorm partials of at most IN_PARTS 16x16 output tiles per image and addresses
        fewer than 2^30 operand bytes (irgan_conv_fwd_fp8); a size beyond either runs that
        group on the bf16 kernels for this call (no EUNSUPPORTED mid-step)."""
        if not self.fp8:
            return False, False
        H1, W1, H2, W2 = self._dims(H, W)
        c1, c2 = 2 * self.ngf, 4 * self.ngf

        def ok(h, w, cin):
            return -(-h // 16) * -(-w // 16) <= ops.IN_PARTS and B * h * w * cin < (1 << 30)
        res = ok(H2, W2, c2)
        return res, res and self.fp8_ud and ok(H1, W1, c2 + c1)

    def forward(self, ir_nchw: torch.Tensor, bufs: Buffers = None, training: bool = None,
                bn_repeat: int = 1, bn_sync: bool = False, tape: bool = False) -> torch.Tensor:
        """ir (B, input_nc, H, W) fp32 in [-1,1] -> fake NHWC fp32 (B, H, W, 3).
        Activations land in ``bufs`` (default: the engine's own set).  ``training``
        (default: self.training) decides nn.Dropout's and nn.BatchNorm2d's mode (ir:394-395):
        callers outside the module forward / GANStep pass the module's train()/eval() state.
        bn_repeat: BatchNorm's running update applied that many times (BNLayer.repeat).
        bn_sync: synchronise the BatchNorm statistics over the engine's ``bn_sync`` handle (if it
        has one; GANStep's forwards) -- every other caller, the module API among them, normalises
        with the local batch, as nn.BatchNorm2d does under DDP.
        fp8: a training-mode call records every operand's amax and rolls the forward scales on
        (delayed scaling); an eval-mode call (``training`` False) reads the scales and writes
        nothing -- no producer records, nothing rolls, and the first norm of each ResnetBlock
        writes its e4m3 output alone (no ``t{b}`` map; ``tape``: the call's backward will run, the
        module API under autograd, so the bf16 maps it may read are kept).  Its one possible
        state change comes first: when a forward slot it will read is unseen, a training-mode
        forward of the same input calibrates the slots (its output is dropped, the maxima it
        recorded are cleared), so the call returns what every later call on this input returns."""
        B, _, H, W = ir_nchw.shape
        g, T = bufs or self.bufs, self.tdt
        train = self.training if training is None else bool(training)
        frozen = self.fp8 and not train
        if frozen and self._fp8_needs_calibration(B, H, W):
            self.fp8_prepasses += 1
            self.forward(ir_nchw, bufs=g, training=True)
            for rng in ("fwd", "cat", "x1"):
                self.f8a.clear_amax(*self.fp8_slots[rng])
        if self.norm_type == "batch":
            for n in self.norms.values():
                n.configure(training=train, groups=1, repeat=bn_repeat, sync=self.bn_sync if bn_sync else None)
        c0, c1, c2 = self.ngf, 2 * self.ngf, 4 * self.ngf
        H1, W1, H2, W2 = self._dims(H, W)
        g.state["shape"] = (B, H, W)
        g.state.pop("dropout_seed", None)
        if self.use_dropout and train:   # a fresh mask per forward call; the backward reuses it
            self.dropout_calls += 1
            g.state["dropout_seed"] = (self.dropout_seed << 32) ^ (self.dropout_calls << 8)
        ir_buf = g.zeros("ir", (B, H, W, max(8, self.input_nc)), T)   # narrow input zero-padded to 8 ch
        ops.nchw_to_nhwc(ir_nchw.contiguous(), Feat(ir_buf, 0, self.input_nc))
        ir_t = Feat(ir_buf, 0, self.inc.cin_eff)
        cat2 = g.get("cat2", (B, H, W, c1 + c0), T)       # [up2 out | x0]
        cat1 = g.get("cat1", (B, H1, W1, c2 + c1), T)     # [up1 out | x1]
        x0 = Feat(cat2, c1, c0)
        x1 = Feat(cat1, c2, c1)
        st = g.state["fp8"] = self._fp8_call(g, B, H, W, frozen)
        D2, U1 = self.c_down2, self.c_up1
        t8_only = frozen and st.on["res"] and not tape   # conv2 reads t's e4m3 copy alone
        # inc: reflect-pad 3, conv7x7, IN, ReLU  (ir:458-463)
        z0 = Feat(g.get("z0", (B, H, W, c0), T))
        self.norms["inc"].conv_fwd(g, "inc", self.inc, ir_t, z0, x0, ACT_RELU)   # statistics fused where taken
        # down1 (+ blur-down)  (ir:469-474)
        if self.no_aa:
            z1 = Feat(g.get("z1", (B, H1, W1, c1), T))
            ops.conv_fwd(self.down1, x0, z1)
            self.norms["down1"].fwd(g, "down1", z1, x1, ACT_RELU)
        else:
            z1 = Feat(g.get("z1", (B, H, W, c1), T))
            self.norms["down1"].resample_fwd(g, "down1", self.down1, x0, z1, "a1", ACT_RELU, x1, ops.blur_down_in,
                                             ops.blur_down, q8=D2.side(st))
            D2.calibrate(st, x1)   # down2's operand scaled from x1 alone on the first step
        # down2 (+ blur-down)  (ir:477-482)
        h = Feat(g.get("h0", (B, H2, W2, c2), T))
        if self.no_aa:
            z2 = Feat(g.get("z2", (B, H2, W2, c2), T))
            ops.conv_fwd(self.down2, x1, z2)
            self.norms["down2"].fwd(g, "down2", z2, h, ACT_RELU)
        else:
            z2 = Feat(g.get("z2", (B, H1, W1, c2), T))
            D2.resample_fwd(g, st, x1, z2, "a2", ACT_RELU, h, ops.blur_down_in, ops.blur_down)
        # 9 ResnetBlocks  (ir:362-418, 485-490); fp8: h_0 (from blur-down) by a quantise launch
        if self.blocks:
            self.blocks[0][0].feed(st, h)
        for b, (ra, rb) in enumerate(self.blocks):
            r1 = Feat(g.get(f"r1_{b}", (B, H2, W2, c2), T))
            t = None if t8_only else Feat(g.get(f"t{b}", (B, H2, W2, c2), T))
            ra.fwd(g, st, h, r1, t, ACT_RELU, nxt=rb)
            if self.use_dropout and train:   # nn.Dropout(0.5) after the ReLU (ir:394-395)
                t, t1 = Feat(g.get(f"td{b}", (B, H2, W2, c2), T)), t
                ops.dropout(t1, t, g.state["dropout_seed"] + 2 * b)
            r2 = Feat(g.get(f"r2_{b}", (B, H2, W2, c2), T))
            hn = Feat(g.get(f"h{b + 1}", (B, H2, W2, c2), T))
            rb.fwd(g, st, t, r2, hn, ACT_NONE, res=h, nxt=self.blocks[b + 1][0] if b + 1 < self.n_blocks else None)
            h = hn
        self._fp8_roll(st, "res", "fwd", snapshot=True)   # next step's forward scales
        # up1 -> cat with x1 -> conv/IN/ReLU  (ir:554-558)
        # (odd sizes: the up-sampled map is 2*H2 x 2*W2 != H1 x W1 and is resized to the
        # skip's size, ir:555-556 -- folded into the UpsampleAA table, or a resize launch
        # after the ConvTranspose2d)
        y1 = Feat(cat1, 0, c2)
        if self.no_aa_up:
            self._convt(self.up1_up, h, y1, g, "ut1")
        else:
            q8 = U1.side(st, (0, c2))
            ops.upsample(h, y1, q8=q8 and q8.side)
        U1.calibrate(st, Feat(cat1))   # up1_conv's operand scaled from the whole concat on the first step
        z3 = Feat(g.get("z3", (B, H1, W1, c1), T))
        # up2 -> cat with x0 -> conv/IN/ReLU  (ir:561-565)
        y2 = Feat(cat2, 0, c1)
        if self.no_aa_up:
            a3 = Feat(g.get("a3", (B, H1, W1, c1), T))   # also the ConvTranspose2d's weight-gradient input
            U1.fwd(g, st, Feat(cat1), z3, a3, ACT_RELU)
            self._convt(self.up2_up, a3, y2, g, "ut2")
        else:
            U1.resample_fwd(g, st, Feat(cat1), z3, "a3", ACT_RELU, y2, ops.upsample_in, ops.upsample)
        self._fp8_roll(st, "ud", "cat", snapshot=True)
        z4 = Feat(g.get("z4", (B, H, W, c0), T))
        a4 = Feat(g.get("a4", (B, H, W, c0), T))
        self.norms["up2"].conv_fwd(g, "up2", self.up2, Feat(cat2), z4, a4, ACT_RELU)
        # outc: reflect-pad 3, conv7x7 (+bias), tanh  (ir:527-531)
        fake = g.get("fake", (B, H, W, self.output_nc), torch.float32)
        ops.conv_fwd(self.outc, a4, Feat(fake), act=ACT_TANH)
        return fake

    def _convt(self, pc, x: Feat, y: Feat, g: Buffers, name: str):
        """ConvTranspose2d(k3, s2, p1, op1) (ir:495-500) into y, through a 2H x 2W
        temporary + bilinear resize when y's size is not 2x (ir:555-556)."""
        if (y.H, y.W) == (2 * x.H, 2 * x.W):
            ops.conv_dgrad(pc, x, y, bias=True)
            return
        t = Feat(g.get(name, (x.N, 2 * x.H, 2 * x.W, y.C), self.tdt))
        ops.conv_dgrad(pc, x, t, bias=True)
        ops.resize(t, y)

    def _convt_bwd(self, pc, key, dy: Feat, x: Feat, dx: Feat, g: Buffers, name: str):
        """Backward of _convt: bias grad, weight grad, and dx (the conv forward of the
        transposed conv); dy is the gradient at the skip-sized output."""
        S = self.store
        if (dy.H, dy.W) != (2 * x.H, 2 * x.W):
            t = Feat(g.get(name + "_d", (x.N, 2 * x.H, 2 * x.W, dy.C), self.tdt))
            ops.resize_bwd(dy, t)
            dy = t
        db = self._bgrad(key + ".bias")
        if db is not None:
            ops.channel_sum(dy, db)
        ops.conv_wgrad(pc.spec, dy, x, S.krsc(key + ".weight", S.grad), self.dtype)
        ops.conv_fwd(pc, dy, dx, bias=False)

    def backward(self, dfake: torch.Tensor, ready=None, bufs: Buffers = None):
        """dfake: dL/dfake, NHWC fp32 (B,H,W,3).  Accumulates into store.grad.
        ``bufs``: the set the matching forward wrote (default: the engine's own).

        ``ready(key)``, if given, is called each time every gradient from parameter
        ``key`` to the end of the flat buffer is final (reverse layer order), so the
        caller can start reducing that tail while the rest of the backward runs."""
        ready = ready or (lambda key: None)
        g, T, S, dt = bufs or self.bufs, self.tdt, self.store, self.dtype
        B, H, W = g.state["shape"]
        c0, c1, c2 = self.ngf, 2 * self.ngf, 4 * self.ngf
        H1, W1, H2, W2 = self._dims(H, W)
        G = S.grad
        cat1, cat2 = Feat(g.d["cat1"]), Feat(g.d["cat2"])
        x0, x1 = cat2.sl(c1, c0), cat1.sl(c2, c1)
        padbuf = g.flat("dpad", max(B * (H + 6) * (W + 6) * c0, B * (H2 + 2) * (W2 + 2) * c2))

        def wg(pc, key, x, dy):
            ops.conv_wgrad(pc.spec, x, dy, S.krsc(key + ".weight", G), dt)

        # outc: tanh' then conv backward
        fake = Feat(g.d["fake"])
        dzo_buf = g.zeros("dz_out", (B, H, W, max(8, self.output_nc)), T)   # zero-padded to 8 ch
        dzo = Feat(dzo_buf, 0, self.output_nc)
        ops.act_bwd(Feat(dfake), fake, ACT_TANH, dzo)
        a4 = Feat(g.d["a4"])
        wg(self.outc, "outc.1", a4, dzo)
        ops.channel_sum(dzo, S.krsc("outc.1.bias", G))
        da4 = Feat(g.get("da4", (B, H, W, c0), T))
        ops.conv_dgrad(self.outc, Feat(dzo_buf, 0, self.outc.cout_eff), da4, pad_buf=padbuf)
        # up2_conv
        self.norms["up2"].bwd(g, "up2", da4, Feat(g.d["z4"]), ACT_RELU, da4, db=self._bgrad("up2_conv.0.bias"))
        wg(self.up2, "up2_conv.0", cat2, da4)
        dcat2 = Feat(g.get("dcat2", (B, H, W, c1 + c0), T))
        ops.conv_dgrad(self.up2, da4, dcat2)
        # up2_up
        da3 = Feat(g.get("da3", (B, H1, W1, c1), T))
        dy2 = dcat2.sl(0, c1)
        if self.no_aa_up:
            self._convt_bwd(self.up2_up, "up2_up", dy2, Feat(g.d["a3"]), da3, g, "ut2")
        else:
            ops.upsample_bwd(dy2, da3)
        # up1_conv
        st = g.state["fp8"]
        dcat1 = Feat(g.get("dcat1", (B, H1, W1, c2 + c1), T))
        self.c_up1.bwd(g, st, da3, Feat(g.d["z3"]), ACT_RELU, da3, cat1, dcat1)
        # up1_up
        h9 = Feat(g.d[f"h{self.n_blocks}"])
        dh = Feat(g.get("dh", (B, H2, W2, c2), T))
        dy1 = dcat1.sl(0, c2)
        if self.no_aa_up:
            self._convt_bwd(self.up1_up, "up1_up", dy1, h9, dh, g, "ut1")
        else:
            ops.upsample_bwd(dy1, dh)
        ready("up1_up.weight" if self.no_aa_up else "up1_conv.0.weight")
        # resblocks, reversed: dh holds d h_{b+1}; becomes d h_b in place
        # Off the e4m3 path their weight gradients -- which nothing in the backward reads -- are
        # deferred and launched ``ngrp`` layers at a time (wgrad_flush).  Each deferred layer's dz
        # then lands in its own slot of a ring of ngrp buffers, rewritten only after the flush that
        # read it (same stream), and ready() follows the flush that made its tail final.
        ngrp = 0 if st.on["res"] else ops.WGRAD_GROUP[0]
        dr = Feat(g.get("dtmp2", (B, H2, W2, c2), T))
        if ngrp:
            ring = [Feat(g.get(f"dz_ring{i}", (B, H2, W2, c2), T)) for i in range(ngrp)]
            pend = []
        else:
            ring, pend = [Feat(g.get("dtmp", (B, H2, W2, c2), T)), dr], None   # rb's dz; ra's in place

        def flush(full):
            if pend and (full or len(pend) >= ngrp):
                wgrad_flush(self, pend)
                ready(f"{pend[-1][0].key}.weight")   # final from the last flushed layer to the end
                pend.clear()

        drop = self.use_dropout and "dropout_seed" in g.state
        for b in reversed(range(self.n_blocks)):
            ra, rb = self.blocks[b]
            k = 2 * (self.n_blocks - 1 - b)   # rb is the backward's k-th ResnetBlock conv, ra its k+1-th
            t = Feat(g.d[f"td{b}"] if drop else g.d[f"t{b}"])   # rb's input: the dropped-out t
            rb.bwd(g, st, dh, Feat(g.d[f"r2_{b}"]), ACT_NONE, ring[k % len(ring)], t, dr, padbuf=padbuf,
                   pend=pend)
            flush(False)
            if drop:   # backward of the dropout: the same mask and scale on the gradient
                ops.dropout(dr, dr, g.state["dropout_seed"] + 2 * b)
            ra.bwd(g, st, dr, Feat(g.d[f"r1_{b}"]), ACT_RELU, ring[(k + 1) % len(ring)], Feat(g.d[f"h{b}"]),
                   dh, accumulate=True, padbuf=padbuf, pend=pend)
            if ngrp:
                flush(False)
            else:
                ready(f"{ra.key}.weight")
        if ngrp:
            flush(True)
        self._fp8_roll(st, "res", "dy")   # next step's backward-data scales
        # down2 (+ blur-down)
        dx1 = dcat1.sl(c2, c1)
        # (accumulated: x1 feeds down2 and the up1 concat)
        if self.no_aa:
            self.c_down2.bwd(g, st, dh, Feat(g.d["z2"]), ACT_RELU, dh, x1, dx1, accumulate=True)
        else:
            dz2 = Feat(g.get("da2", (B, H1, W1, c2), T))
            self.c_down2.bwd(g, st, dh, Feat(g.d["z2"]), ACT_RELU, dz2, x1, dx1, accumulate=True,
                             resample=(ops.blur_down_bwd_in, ops.blur_down_bwd))
        self._fp8_roll(st, "ud", "ud_dy")   # next step's scales of the two dY slots
        # down1 (+ blur-down)
        z1 = Feat(g.d["z1"])
        if self.no_aa:
            dz1 = Feat(g.get("da1", (B, H1, W1, c1), T))
            self.norms["down1"].bwd(g, "down1", dx1, z1, ACT_RELU, dz1, db=self._bgrad("down1.0.bias"))
        else:
            dz1 = Feat(g.get("da1", (B, H, W, c1), T))
            self.norms["down1"].resample_bwd(g, "down1", dx1, z1, ACT_RELU, dz1, ops.blur_down_bwd_in,
                                             ops.blur_down_bwd, db=self._bgrad("down1.0.bias"))
        wg(self.down1, "down1.0", x0, dz1)
        dx0 = dcat2.sl(c1, c0)
        ops.conv_dgrad(self.down1, dz1, dx0, accumulate=True)
        # inc
        self.norms["inc"].bwd(g, "inc", dx0, Feat(g.d["z0"]), ACT_RELU, dx0, db=self._bgrad("inc.1.bias"))
        wg(self.inc, "inc.1", Feat(g.d["ir"]), dx0)
        ready("inc.1.weight")


# ----------------------------------------------------------------------------
# discriminator  (ir:576-635)
# ----------------------------------------------------------------------------

class DiscriminatorEngine:
    _pack_batch = None  # ops.PackBatch of self.packs, built on the first pack()

    def __init__(self, store: ParamStore, dtype=BF16, input_nc=4, ndf=64, n_layers=3, norm="instance"):
        """PatchGAN with ``n_layers`` stride-2 stages (ir:585-632; train_kaist builds 3) and
        norm 'instance' or 'none' (the normalised convs then have no bias)."""
        self.store, self.dtype, self.tdt = store, dtype, ops.TORCH_DT[dtype]
        self.LAYERS = d_layers(n_layers)
        chans = d_channels(input_nc, ndf, n_layers)
        self.chans = chans
        self.packs = [_pc(store, k, ConvSpec(chans[i], chans[i + 1], 4, s, 1, PAD_ZERO), dtype)
                      for i, (k, s, _) in enumerate(self.LAYERS)]
        self.norms = [make_norm(norm, store, f"model.{int(k.split('.')[1]) + 1}") if n else None
                      for (k, _, n) in self.LAYERS]
        self.norm_type, self.training = norm, True
        self.bn_sync = None   # BNSync handle of the fused step's forwards (GANStep, Config.sync_bn)
        self.bufs = Buffers(store.device)

    def pack(self):
        if self._pack_batch is None:
            self._pack_batch = ops.PackBatch(self.packs)
        self._pack_batch.run()

    def forward(self, din: Feat, tag="", bufs: Buffers = None, groups: int = 1, bn_sync: bool = False) -> torch.Tensor:
        """din: NHWC (NB, H, W, 4) compute-dtype -> patch logits (NB, h, w, 1) fp32.
        The activations are kept in ``bufs`` (default: the engine's own) under ``tag``.
        groups: BatchNorm statistics per group of NB / groups samples (BNLayer.groups);
        self.training: BatchNorm's train() / eval() mode; bn_sync: as GeneratorEngine.forward
        (each group is synchronised separately)."""
        g, T = bufs or self.bufs, self.tdt
        if self.norm_type == "batch":
            for nrm in self.norms:
                if nrm is not None:
                    nrm.configure(training=self.training, groups=groups, repeat=1,
                                  sync=self.bn_sync if bn_sync else None)
        x = din
        acts, pre = [din], {}
        g.state[tag] = (acts, pre)
        for i, pc in enumerate(self.packs):
            Ho, Wo = pc.spec.out_hw(x.H, x.W)
            last = i == len(self.packs) - 1
            y = Feat(g.get(f"{tag}e{i}", (x.N, Ho, Wo, pc.spec.cout), torch.float32 if last else T))
            if i == 0:
                ops.conv_fwd(pc, x, y, act=ACT_LRELU)
            elif last:
                if not ops.patch_head_fwd(pc, x, y.t):
                    ops.conv_fwd(pc, x, y)
            else:
                z = Feat(g.get(f"{tag}z{i}", (x.N, Ho, Wo, pc.spec.cout), T))
                self.norms[i].conv_fwd(g, f"{tag}n{i}", pc, x, z, y, ACT_LRELU)
                pre[i] = z
            acts.append(y)
            x = y
        return x.t

    def backward(self, dout: torch.Tensor, want_wgrad=True, want_dinput=False, tag="", bufs: Buffers = None,
                 ready=None):
        """dout: dL/dlogits fp32 (same shape as forward output).  Weight grads
        accumulate into store.grad; returns d input (fp32 NHWC) if asked.
        ``ready(key)`` (as GeneratorEngine.backward): called once every gradient from layer
        ``key``'s weight to the end of the flat buffer is final, so the caller's bucketed
        all-reduce starts on the tail while the earlier layers' backward still runs."""
        g, T, S = bufs or self.bufs, self.tdt, self.store
        acts, pre = g.state[tag]
        G = S.grad
        n = len(self.packs)
        def logits_grad():   # the generic kernels' bf16 copy of dL/dlogits, padded to 8 channels
            dbuf = g.zeros(f"{tag}dout_t", tuple(dout.shape[:3]) + (8,), T)
            ops.axpby(Feat(dout), 1.0, Feat(dbuf, 0, dout.shape[3]))
            return Feat(dbuf, 0, self.packs[-1].cout_eff)
        dy = None   # the PatchGAN head kernels read the fp32 dout itself
        for i in reversed(range(n)):
            pc, key = self.packs[i], self.LAYERS[i][0]
            x = acts[i]
            if dy is None and not (i == n - 1 and ops.is_patch_head(pc, x)):
                dy = logits_grad()
            bias_sum = None
            if i == n - 1:
                if want_wgrad:
                    bias_sum = Feat(dout)
            elif self.norms[i] is not None:
                self.norms[i].bwd(g, f"{tag}n{i}", dy, pre[i], ACT_LRELU, dy,
                                  db=S.krsc(key + ".bias", G) if want_wgrad and key + ".bias" in S.shapes else None,
                                  wgrad=want_wgrad)
            elif want_wgrad:  # layer 0: LReLU mask already folded into dy by the layer-1 dgrad
                bias_sum = dy
            if want_wgrad:
                if bias_sum is not None:
                    ops.channel_sum(bias_sum, S.krsc(key + ".bias", G))
                dw = S.krsc(key + ".weight", G)
                if dy is not None or not ops.patch_head_wgrad(pc, x, dout, dw):
                    dy = dy or logits_grad()
                    ops.conv_wgrad(pc.spec, x, Feat(dy.t, dy.off, pc.spec.cout), dw, self.dtype)
                if ready is not None:
                    ready(key + ".weight")
            if i == 0:
                if not want_dinput:
                    return None
                dx = Feat(g.get(f"{tag}dinput", (x.N, x.H, x.W, pc.spec.cin), torch.float32))
                ops.conv_dgrad(pc, dy or logits_grad(), dx)
                return dx
            dx = Feat(g.get(f"{tag}d{i}", (x.N, x.H, x.W, x.C), T))
            if i == 1:  # previous activation is LReLU without IN: fold its derivative in the epilogue
                ops.conv_dgrad(pc, dy, dx, mask=x, mask_act=2)
            elif not (dy is None and ops.patch_head_dgrad(pc, dout, dx)):   # the head from the fp32 dL/dlogits
                ops.conv_dgrad(pc, dy or logits_grad(), dx)
            dy = dx
        return None


# ----------------------------------------------------------------------------
# VGG-16 features[:16] perceptual extractor  (ir:642-683), frozen
# ----------------------------------------------------------------------------

NO_POOL_FUSION = bool(os.environ.get("IRGAN_NO_POOL_FUSION"))   # A/B: separate conv and maxpool launches
NO_TAP_FUSION = bool(os.environ.get("IRGAN_NO_TAP_FUSION"))     # A/B: maxpool_bwd, then the tap as its own launch

# Config.perc_layers: torchvision's names of the ReLU maps of vgg16.features[:16]; the index is the
# engine's conv number j
PERC_LAYERS = tuple(c.relu for c in VGG_STACK)
DEFAULT_TAPS = (("relu3_3", 1.0),)   # the reference's perceptual term (ir:1667-1669)


def perc_taps(layers, weights=None):
    """The perceptual taps ((name, weight), ...) of ``layers`` / ``weights`` (None: every weight 1),
    sorted by depth, zero-weight layers dropped.  ValueError for an unknown name, a duplicate, an
    empty list, a weights length that differs from the layers', a weight that is not finite or
    is negative, and all-zero weights."""
    if isinstance(layers, str):
        layers = (layers,)
    layers = tuple(layers)
    if not layers:
        raise ValueError(f"perc_layers must name at least one of {PERC_LAYERS}, got an empty list")
    for n in layers:
        if n not in PERC_LAYERS:
            raise ValueError(f"perc_layers: unknown layer {n!r}; the taps are {PERC_LAYERS}")
    if len(set(layers)) != len(layers):
        raise ValueError(f"perc_layers names a layer twice: {layers!r}")
    weights = (1.0,) * len(layers) if weights is None else tuple(float(w) for w in weights)
    if len(weights) != len(layers):
        raise ValueError(f"perc_weights has {len(weights)} entries for {len(layers)} perc_layers")
    for w in weights:
        if not (math.isfinite(w) and w >= 0.0):
            raise ValueError(f"perc_weights must be finite and >= 0, got {w!r}")
    taps = tuple(sorted(((n, w) for n, w in zip(layers, weights) if w > 0.0), key=lambda t: PERC_LAYERS.index(t[0])))
    if not taps:
        raise ValueError("perc_weights are all zero: no perceptual term is left (set lambda_perc = 0 instead)")
    return taps


class VGGEngine:
    _pack_batch = None  # ops.PackBatch of self.packs, built on the first pack()

    def __init__(self, store: ParamStore, dtype=BF16):
        self.store, self.dtype, self.tdt = store, dtype, ops.TORCH_DT[dtype]
        self.packs = [_pc(store, str(i), ConvSpec(ci, co, 3, 1, 1, PAD_ZERO), dtype) for i, ci, co in VGG_CONVS]
        dev = store.device
        std = torch.tensor(IMAGENET_STD)
        mean = torch.tensor(IMAGENET_MEAN)
        # ((x+1)/2 - mean)/std  ==  x * (0.5/std) + (0.5 - mean)/std
        self.scale = (0.5 / std).float().to(dev)
        self.shift = ((0.5 - mean) / std).float().to(dev)
        self.bufs = Buffers(dev)

    def pack(self):
        if self._pack_batch is None:
            self._pack_batch = ops.PackBatch(self.packs)
        self._pack_batch.run()

    def forward(self, vin: Feat, bufs: Buffers = None, part=None, keep=True, taps=None) -> Feat:
        """relu3_3 features of vin.  part = (b0, nb): compute only images [b0, b0+nb)
        into the full-batch activation buffers (the step runs the real and the fake
        half on different streams).  keep=False: no backward will read these images'
        activations (the real half), so a conv followed by MaxPool2d may write the pooled
        map alone (ops.conv_fwd_pool).

        taps (perc_taps' pairs; None: the relu3_3 stack as it always ran): the stack stops at the
        deepest tapped conv, whose map is returned (a pooled layer that ends the stack is not
        pooled), and a tapped conv+pool layer writes its full-size map under keep=False too:
        backward_taps reads it."""
        g, T = bufs or self.bufs, self.tdt
        x = vin
        acts = g.state["acts"] = []   # per conv j run: (its input map, its ReLU output)
        sl = (lambda f: f) if part is None else (lambda f: f.batch(*part))  # noqa: E731
        tapped = () if taps is None else [PERC_LAYERS.index(n) for n, _ in taps]
        last = max(tapped, default=len(self.packs) - 1)
        for j, pc in enumerate(self.packs[:last + 1]):
            y = Feat(g.get(f"v{j}", (x.N, x.H, x.W, pc.spec.cout), T))
            acts.append((x, y))
            if VGG_STACK[j].pool and j < last:
                # conv -> ReLU -> MaxPool2d(2) (ir:664), fused where a kernel takes the layer
                p = Feat(g.get(f"p{j}", (x.N, x.H // 2, x.W // 2, pc.spec.cout), T))
                full = keep or j in tapped
                if NO_POOL_FUSION or not ops.conv_fwd_pool(pc, sl(x), sl(y) if full else None, sl(p)):
                    ops.conv_fwd(pc, sl(x), sl(y), act=ACT_RELU)
                    ops.maxpool(sl(y), sl(p))
                x = p
            else:
                ops.conv_fwd(pc, sl(x), sl(y), act=ACT_RELU)
                x = y
        return x

    def _tap(self, g, nb, j, w, dz, loss, accumulate):
        """The perceptual term of conv j's ReLU map (fake images [0, nb), real images [nb, 2 nb)) at
        weight w: its value into ``loss``, its gradient written or added to dz."""
        y = g.state["acts"][j][1]
        ops.l1_tap(y.batch(0, nb).t, y.batch(nb, nb).t, w, dz.t, loss, accumulate)

    def _walk(self, g, nb, top, dz, wt=(), loss=None) -> Feat:
        """The backward-data walk from dz = dL/d(conv ``top``'s pre-activation) of the first nb
        images down to d(input).  wt ({conv j: weight}, with ``loss``): the perceptual taps below
        ``top``, each added to the dz of its layer on the way down."""
        T, acts = self.tdt, g.state["acts"]
        for j in range(top, 0, -1):
            pc, xin, below = self.packs[j], acts[j][0].batch(0, nb), acts[j - 1][1]   # below: conv j-1's ReLU map
            src = below.batch(0, nb)
            dzn = Feat(g.get(f"dz{j - 1}", (nb, src.H, src.W, src.C), T))
            tap = j - 1 in wt
            if VGG_STACK[j - 1].pool:  # input is a pool output: dgrad -> maxpool bwd (+relu') of the pool input
                dp = Feat(g.get(f"dp{j}", (nb, xin.H, xin.W, xin.C), T))
                ops.conv_dgrad(pc, dz, dp)
                real = below.batch(nb, nb) if tap else None
                if tap and not NO_TAP_FUSION and ops.maxpool_bwd_tap(src, real, dp, dzn, wt[j - 1], loss):
                    tap = False   # applied inside the pool backward
                else:
                    if src.H % 2 or src.W % 2:   # floor pooling: the last odd row / column gets no gradient
                        dzn.t.zero_()
                    ops.maxpool_bwd(src, dp, dzn, relu_mask=True)
            else:  # input is a ReLU output: fold relu' into the dgrad epilogue
                ops.conv_dgrad(pc, dz, dzn, mask=xin, mask_act=1)
            if tap:
                self._tap(g, nb, j - 1, wt[j - 1], dzn, loss, True)
            dz = dzn
        vin = acts[0][0]
        dvin = Feat(g.get("dvin", (nb, vin.H, vin.W, self.packs[0].spec.cin), torch.float32))
        ops.conv_dgrad(self.packs[0], dz, dvin)
        return dvin

    def backward_input(self, dfeat: Feat, nb: int, bufs: Buffers = None) -> Feat:
        """d(input) for the first nb images (frozen weights: backward-data only).
        dfeat = dL/d(relu3_3 output) for those images."""
        g, top = bufs or self.bufs, len(self.packs) - 1
        dz = Feat(g.get(f"dz{top}", tuple(dfeat.t.shape), self.tdt))
        ops.act_bwd(dfeat, g.state["acts"][top][1].batch(0, nb), ACT_RELU, dz)
        return self._walk(g, nb, top, dz)

    def backward_taps(self, taps, nb: int, scale: float, loss: torch.Tensor, bufs: Buffers = None) -> Feat:
        """The multi-layer perceptual term (Config.perc_layers) after forward(..., taps=taps) ran on
        both halves of a 2*nb batch (fake images [0, nb), real images [nb, 2 nb)):
        ``loss`` += scale * sum_l w_l * mean|phi_l(fake) - phi_l(real)|, and d(input) of that sum
        for the fake images is returned.  backward_input's walk, begun at the deepest tap; each
        shallower tap adds its gradient to the dz of its layer on the way down: a tapped pool input
        inside the pool backward (ops.maxpool_bwd_tap; NO_TAP_FUSION or a refused shape: maxpool_bwd,
        then l1_tap over the whole map), any other layer by l1_tap on what the dgrad epilogue wrote."""
        g = bufs or self.bufs
        wt = {PERC_LAYERS.index(n): scale * w for n, w in taps}
        top = max(wt)
        src = g.state["acts"][top][1]
        dz = Feat(g.get(f"dz{top}", (nb, src.H, src.W, src.C), self.tdt))
        self._tap(g, nb, top, wt[top], dz, loss, False)
        return self._walk(g, nb, top, dz, wt, loss)


# ----------------------------------------------------------------------------
# the train step
# ----------------------------------------------------------------------------

def grad_allreduce(t: torch.Tensor, group=None) -> torch.Tensor:
    """In-place mean of a flat gradient buffer over the data-parallel ranks, as
    one blocking collective.

    Every loss of the step is a mean of per-sample terms and InstanceNorm is
    per-sample, so the mean of the per-rank grads over equal shards is the
    global-batch gradient.  GANStep itself uses the overlapped
    form (BucketedAllreduce); this whole-buffer helper is the reference
    semantics the DP tests splice into the oracle step.  RCCL averages
    natively; gloo (the CPU test backend) sums and we scale.
    """
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return t
    world = dist.get_world_size(group)
    if world == 1:
        return t
    if dist.get_backend(group) == "nccl":
        dist.all_reduce(t, op=dist.ReduceOp.AVG, group=group)
    else:
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
        t.div_(world)
    return t


def replica_digest(tensors) -> torch.Tensor:
    """Exact int64 digest of fp32 tensors (their bit patterns): a plain and a
    position-weighted sum per tensor.  Equal digests on every rank = the data-parallel
    replicas hold bit-identical parameters (bench.py's post-run check)."""
    out = []
    for t in tensors:
        b = t.detach().reshape(-1).view(torch.int32).to(torch.int64)
        w = torch.arange(b.numel(), device=b.device, dtype=torch.int64) % 65521 + 1
        out += [b.sum(), (b * w).sum()]
    return torch.stack(out)


def replicas_identical(tensors, group=None, force=False) -> bool:
    """True when every rank of ``group`` holds bit-identical ``tensors`` (max == min of
    the digests over ranks); True without a process group (and at world size 1 unless
    ``force``: then the MAX / MIN collectives run anyway)."""
    import torch.distributed as dist
    d = replica_digest(tensors)
    if not (dist.is_available() and dist.is_initialized()) or (dist.get_world_size(group) == 1 and not force):
        return True
    if dist.get_backend(group) != "nccl":
        d = d.cpu()
    hi, lo = d.clone(), d.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    return bool(torch.equal(hi, lo))


class BucketedAllreduce:
    """Mean of a flat gradient buffer over the ranks, reduced tail-first in buckets
    while the producing backward is still running (SURVEY.md 8e overlap schedule).

    The backward calls ``ready(key)`` when every grad from ``key`` to the end of the
    flat buffer is final.  Once the not-yet-reduced tail reaches ``bucket_bytes`` it
    is handed to the collective with ``async_op=True``: RCCL runs it on its own
    stream after an event on the compute stream, so the all-reduce of layer L
    overlaps the backward of layers < L.  ``finish()`` reduces the remainder and
    makes the compute stream wait for every bucket (Adam reads the result).
    Buckets are contiguous slices of the flat buffer, so the reduction is the
    same element-wise mean as one whole-buffer all-reduce.
    """

    def __init__(self, store: ParamStore, group=None, bucket_bytes=8 << 20, force=False):
        """force: issue the collectives even at world size 1 (a process group must be
        initialised) -- the RCCL path exercised on one GPU (tests/test_gpu_dp.py)."""
        self.store, self.group, self.bucket_bytes = store, group, bucket_bytes
        self.end, self.works, self.world, self.avg = store.numel, [], 1, True
        import torch.distributed as dist
        self.force = False
        if dist.is_available() and dist.is_initialized():
            self.world = dist.get_world_size(group)
            self.avg = dist.get_backend(group) == "nccl"
            self.force = bool(force)

    @property
    def active(self):
        return self.world > 1 or self.force

    def _launch(self, start):
        import torch.distributed as dist
        if start >= self.end:
            return
        t = self.store.grad[start:self.end]
        op = dist.ReduceOp.AVG if self.avg else dist.ReduceOp.SUM
        self.works.append((dist.all_reduce(t, op=op, group=self.group, async_op=True), t, start, self.end))
        self.end = start

    def start(self):
        """Reduce the whole buffer as one asynchronous collective."""
        if self.active:
            self._launch(0)

    def ready(self, key):
        if not self.active:
            return
        start = self.store.offsets[key]
        if (self.end - start) * 4 >= self.bucket_bytes:
            self._launch(start)

    def finish(self, apply=None):
        """Reduce the remainder, then per bucket (in issue order, tail-first): make the
        compute stream wait for that bucket only and call ``apply(start, end)`` -- the
        optimizer update of the bucket is queued behind its own collective and runs
        while the later buckets are still being reduced (the G-Adam of
        bucket k overlaps the all-reduce of bucket k+1).  Each element of the flat
        buffer lies in exactly one bucket, so this is the whole-buffer mean + update.

        An ``apply`` marked ``whole`` (ParamStore.adam_begin with max_norm: the clipping norm
        runs over the whole reduced buffer) is called once with (0, numel) after every bucket
        has been waited for and scaled: that step gives up the Adam-under-all-reduce overlap,
        and its norm does not depend on the bucket layout."""
        if not self.active:
            if apply is not None:
                apply(0, self.store.numel)
            return
        whole = apply is not None and getattr(apply, "whole", False)
        self._launch(0)
        for w, t, a, b in self.works:
            w.wait()
            if not self.avg:
                t.div_(self.world)
            if apply is not None and not whole:
                apply(a, b)
        if whole:
            apply(0, self.store.numel)
        self.works, self.end = [], self.store.numel


# IRGAN_JOIN_TIMING=1: per step, timing events at the phase boundaries of both streams
# (diagnostics: where the D step sits on the critical path).  Keys: start, gfwd (main: G
# forward done), d0 / dend (side: the D step's first / last launch), terms (main: the G-step
# terms done), join (main: after its wait for the side stream), end.
JOIN_TIMES = [] if os.environ.get("IRGAN_JOIN_TIMING") else None


def _mark(ph, key, stream):
    if ph is not None:
        e = torch.cuda.Event(enable_timing=True)
        e.record(stream)
        ph[key] = e


class GANStep:
    """Buffers, engines and the fused step for one rank.

    Loss slots (fp64, device): 0 loss_D, 1 lambda_gan*GAN, 2 L1*l, 3 perc*l, 4 TV*l, 5 SSIM*l;
    6 / 7 the L2 norm of D's / G's (reduced, unclipped) gradient when that network clips
    (Config.clip_grad_D / clip_grad_G), else 0.
    """

    def __init__(self, G: ParamStore, D: ParamStore, V: ParamStore, cfg, dtype=BF16, process_group=None,
                 gen: GeneratorEngine = None, dis: DiscriminatorEngine = None, vgg: VGGEngine = None,
                 force_reduce=False):
        """force_reduce: run the gradient collectives even at world size 1 (see
        BucketedAllreduce): the DP schedule on one device."""
        self.G, self.D, self.V, self.cfg, self.dtype = G, D, V, cfg, dtype
        self.tdt = ops.TORCH_DT[dtype]
        self.gen = gen or GeneratorEngine(G, dtype, ngf=cfg.ngf, input_nc=cfg.input_nc, output_nc=cfg.output_nc,
                                          no_antialias=cfg.no_antialias, no_antialias_up=cfg.no_antialias_up,
                                          fp8=getattr(cfg, "compute_dtype", "bf16") == "fp8", norm=cfg.norm)
        self.dis = dis or DiscriminatorEngine(D, dtype, input_nc=cfg.input_nc + cfg.output_nc, norm=cfg.norm)
        self.dbufs = Buffers(G.device)   # the D step's own G forward when G has dropout
        self.vgg = vgg or VGGEngine(V, dtype)
        self.bufs = Buffers(G.device)
        self.losses = torch.zeros(8, dtype=torch.float64, device=G.device)
        self.pg = process_group
        self.g_reduce = BucketedAllreduce(G, process_group, force=force_reduce)
        self.d_reduce = BucketedAllreduce(D, process_group, force=force_reduce)
        # SyncBN (Config.sync_bn): wherever the gradient collectives run, the BatchNorm layers of
        # both networks take their training statistics over the same ranks -- all four forwards
        # of step() and their backwards; groups / repeat rules unchanged.  Without a process group,
        # or at world size 1 without force_reduce, the plain local path runs.
        if cfg.norm == "batch" and getattr(cfg, "sync_bn", False) and self.g_reduce.active:
            self.gen.bn_sync = self.dis.bn_sync = BNSync(process_group)
        self.lr_scale = 1.0
        # Config.ema_decay > 0: G's Adam launches also update G.ema (ParamStore.adam_begin); the
        # owner allocates it (G.enable_ema()), and 0 is the plain path with no buffer
        self.ema_decay = float(getattr(cfg, "ema_decay", 0.0) or 0.0)
        # Config.clip_grad_G / clip_grad_D > 0: that network's Adam clips by the global gradient
        # norm (ParamStore.adam_begin max_norm) and the norm lands in losses[7] / losses[6]; 0 is
        # the plain path: no reduction, no extra launch, the slot stays 0
        self.clip_G = float(getattr(cfg, "clip_grad_G", 0.0) or 0.0)
        self.clip_D = float(getattr(cfg, "clip_grad_D", 0.0) or 0.0)
        # Config.gan_mode / gan_real_label: the objective of both GAN terms (ops.gan_loss: "hinge",
        # the reference's, is ops.hinge's own launch; "lsgan", "vanilla") and D's real target
        self.gan_mode = getattr(cfg, "gan_mode", "hinge") or "hinge"
        self.gan_real_label = float(getattr(cfg, "gan_real_label", 1.0))
        if self.gan_mode not in ops.GAN_MODES:
            raise ValueError(f"gan_mode must be one of {sorted(ops.GAN_MODES)}, got {self.gan_mode!r}")
        # Config.perc_layers / perc_weights: the VGG maps of the perceptual term.  None is the
        # reference's relu3_3 at weight 1, whose launches (ops.l1 into dfeat, backward_input) are
        # untouched; any other setting goes through VGGEngine.backward_taps
        taps = perc_taps(getattr(cfg, "perc_layers", ("relu3_3",)), getattr(cfg, "perc_weights", None))
        self.perc_taps = None if taps == DEFAULT_TAPS else taps
        # the D step (D forward/backward on [real; fake] and its all-reduce) runs on a
        # side stream, concurrently with the G-step terms that do not read D (L1,
        # VGG, TV, SSIM); IRGAN_NO_D_OVERLAP=1 keeps everything on one stream
        self.side = None
        if G.device.type == "cuda" and not os.environ.get("IRGAN_NO_D_OVERLAP"):
            self.side = torch.cuda.Stream(device=G.device)
        self.G.dev_adam = self.D.dev_adam = G.device.type == "cuda"
        self.vgg.pack()
        self.gen.pack()
        self.dis.pack()

    def step(self, ir: torch.Tensor, rgb: torch.Tensor):
        """One train step on NCHW fp32 device tensors; returns the loss vector (device)."""
        cfg, b, T = self.cfg, self.bufs, self.tdt
        B, _, H, W = ir.shape
        cin, cout = cfg.input_nc, cfg.output_nc
        self.losses.zero_()
        L = self.losses
        main = torch.cuda.current_stream() if self.side is not None else None
        ph = {} if JOIN_TIMES is not None and main is not None else None
        _mark(ph, "start", main)
        side_ctx = (lambda: torch.cuda.stream(self.side)) if main is not None else _nullcontext  # noqa: E731
        rgb_h = b.get("rgb_nhwc", (B, H, W, cout), torch.float32)
        ops.nchw_to_nhwc(rgb.contiguous(), Feat(rgb_h))
        # ---- VGG features of the real images (ir:1668) need nothing from G: side stream,
        # concurrent with the G forward
        vin = Feat(b.zeros("vin", (2 * B, H, W, max(8, cout)), T), 0, self.vgg.packs[0].cin_eff)
        # D input [real; fake] as one 2B batch, cat([ir, img], 1) (ir:1639-1640) zero-padded to
        # 8 channels (narrow-input conv path): the ir channels of both halves and the real
        # images are written beside the G forward; the fake images once G has run
        dpad = max(8, cin + cout)
        din = Feat(b.zeros("din2", (2 * B, H, W, dpad), T), 0, self.dis.packs[0].cin_eff)
        vgg_side = main is not None and not os.environ.get("IRGAN_NO_VGG_OVERLAP")
        ev_in = None
        if vgg_side:
            ev_in = torch.cuda.Event()
            ev_in.record(main)                    # the real images in NHWC, the zeroed VGG input

        def vgg_real():
            with side_ctx() if vgg_side else _nullcontext():
                if ev_in is not None:
                    self.side.wait_event(ev_in)
                for h in (0, B):
                    ops.nchw_to_nhwc(ir.contiguous(), Feat(din.t[h:h + B], 0, cin))
                ops.axpby(Feat(rgb_h), 1.0, Feat(din.t[:B], cin, cout))
                ops.affine(Feat(rgb_h), self.vgg.scale, self.vgg.shift, vin.batch(B, B))
                # no backward through the real half
                self.vgg.forward(vin, part=(B, B), keep=False, taps=self.perc_taps)
            if vgg_side:
                _mark(ph, "vgg_real", self.side)
                ev = torch.cuda.Event()
                ev.record(self.side)
                return ev
            return None

        # enqueued before the G forward's launches (after them measured neutral,
        # profiles/r03_vgg_after_gfwd_ab.txt)
        ev_vgg = vgg_real()
        # ---- G forward once: ir:1638 and ir:1657 compute the same image -- unless G has
        # dropout, whose two calls draw two masks: then the D step gets its own forward
        # (ir:1638-1639, under no_grad: its activations are never read back)
        # BatchNorm: the one forward stands for the reference's two training-mode forwards, so its
        # running update is applied twice (with dropout the two forwards update once each)
        self.gen.training = self.dis.training = True
        fake_d = self.gen.forward(ir, bufs=self.dbufs, bn_sync=True) if self.gen.use_dropout else None
        fake = self.gen.forward(ir, bn_repeat=1 if self.gen.use_dropout else 2, bn_sync=True)
        # ---- D step on [real; fake] as one 2B batch (ir:1636-1651), on the side stream
        dfake = b.get("dfake", (B, H, W, cout), torch.float32)

        def g_terms():
            # ---- G step terms that do not read D (ir:1656-1681)
            self.G.zero_grad()
            dfake.zero_()
            ops.l1(fake, rgb_h, cfg.lambda_L1, dfake, L[2:3], accumulate=True)
            # perceptual (ir:1667-1669): VGG on the fake half; the real half ran on the side stream
            ops.affine(Feat(fake), self.vgg.scale, self.vgg.shift, vin.batch(0, B))
            feat = self.vgg.forward(vin, part=(0, B), taps=self.perc_taps)
            if ev_vgg is not None:
                main.wait_event(ev_vgg)
            if self.perc_taps is None:
                dfeat = b.get("dfeat", (B, feat.H, feat.W, feat.C), T)
                ops.l1(feat.t[:B], feat.t[B:], cfg.lambda_perc, dfeat, L[3:4])
                dv = self.vgg.backward_input(Feat(dfeat), B)
            else:   # Config.perc_layers: every tap's term lands in slot 3, times lambda_perc * w_l
                dv = self.vgg.backward_taps(self.perc_taps, B, cfg.lambda_perc, L[3:4])
            ops.affine(dv, self.vgg.scale, None, Feat(dfake), accumulate=True)
            ops.tv(Feat(fake), cfg.lambda_tv, dfake, L[4:5])
            ssim_work = b.flat("ssim_work", 10 * fake.numel())
            ops.ssim(Feat(fake), Feat(rgb_h), cfg.lambda_ssim, dfake, L[5:6], ssim_work)

        # host enqueue order: the main stream's G-step terms before the side stream's D step --
        # the dependencies are the event edges either way; enqueued first, the terms start
        # right behind the G forward instead of after ~90 D-step launches (1204 vs 1199 img/s,
        # profiles/r03_terms_first_ab.txt)
        terms_first = main is not None
        ev_fwd = None
        if main is not None:
            _mark(ph, "gfwd", main)
            ev_fwd = torch.cuda.Event()
            ev_fwd.record(main)                   # G output, the zeroed losses and D inputs
        if terms_first:
            g_terms()
        with side_ctx():
            if ev_fwd is not None:
                self.side.wait_event(ev_fwd)
                _mark(ph, "d0", self.side)
            # [real; fake] as one 2B batch.  (The real half apart, beside the G forward, measured
            # -0.8 %: the G forward slowed by what it took off the join, profiles/r05_ab1_dsplit.txt)
            self.D.zero_grad()
            ops.axpby(Feat(fake if fake_d is None else fake_d), 1.0, Feat(din.t[B:], cin, cout))
            # BatchNorm: netD(real), netD(fake) statistics (under SyncBN each group over all ranks)
            pred = self.dis.forward(din, tag="d", groups=2, bn_sync=True)
            dpred = b.get("dpred", tuple(pred.shape), torch.float32)
            ops.gan_loss(pred, pred[:B].numel(), 0, self.gan_mode, self.gan_real_label, 1.0, dpred, L[0:1])
            # D grads reduced tail-first under the D backward (8 MB buckets: model.8 + the head
            # go out while model.5 / .2 / .0 still run), each bucket's Adam right behind it
            # (the weight gradients on the main stream instead, beside this chain: -1.4 %, the main
            # stream is still busy with the G-step terms then, profiles/r06_d_ab.txt)
            self.dis.backward(dpred, want_wgrad=True, want_dinput=False, tag="d", ready=self.d_reduce.ready)
            # D Adam, then the G-step GAN term through the updated D (ir:1651, 1659-1662),
            # still on the side stream: the main stream meanwhile runs the G-step terms
            # that do not read D (L1, VGG, TV, SSIM)
            self.d_reduce.finish(self.D.adam_begin(cfg.lr_D * self.lr_scale, cfg.beta1, cfg.beta2,
                                                   max_norm=self.clip_D, norm_out=L[6:7] if self.clip_D else None))
            self.dis.pack()
            # the G-step D pass reads cat([ir, fake]): the fake half of the D input (rewritten
            # when the D step saw the other dropout draw)
            if fake_d is not None:
                ops.axpby(Feat(fake), 1.0, Feat(din.t[B:], cin, cout))
            predg = self.dis.forward(din.batch(B, B), tag="g", bn_sync=True)
            dpg = b.get("dpredg", tuple(predg.shape), torch.float32)
            ops.gan_loss(predg, predg.numel(), 1, self.gan_mode, self.gan_real_label, cfg.lambda_gan, dpg, L[1:2])
            dd = self.dis.backward(dpg, want_wgrad=False, want_dinput=True, tag="g")
            _mark(ph, "dend", self.side)
        if not terms_first:
            g_terms()
        if main is not None:
            _mark(ph, "terms", main)
            main.wait_stream(self.side)           # the GAN term's d fake
            _mark(ph, "join", main)
        ops.axpby(dd.sl(cin, cout), 1.0, Feat(dfake), 1.0)
        self.gen.backward(dfake, ready=self.g_reduce.ready)
        self.g_reduce.finish(self.G.adam_begin(cfg.lr_G * self.lr_scale, cfg.beta1, cfg.beta2,
                                               ema_decay=self.ema_decay, max_norm=self.clip_G,
                                               norm_out=L[7:8] if self.clip_G else None))
        self.gen.pack()
        if ph is not None:
            _mark(ph, "end", main)
            JOIN_TIMES.append(ph)
        return L

    @staticmethod
    def loss_dict(L: torch.Tensor, cfg) -> dict:
        v = L.tolist()
        gan = v[1] / cfg.lambda_gan if cfg.lambda_gan else 0.0
        d = dict(loss_D=v[0], loss_G=v[1] + v[2] + v[3] + v[4] + v[5], loss_G_GAN=gan, loss_G_L1=v[2],
                 loss_G_perc=v[3], loss_G_TV=v[4], loss_G_ssim=v[5])
        # the gradient norms, only for the networks that clip (the key set is unchanged otherwise)
        if getattr(cfg, "clip_grad_D", 0.0):
            d["grad_norm_D"] = v[6]
        if getattr(cfg, "clip_grad_G", 0.0):
            d["grad_norm_G"] = v[7]
        return d
