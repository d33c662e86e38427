"""Bit-level digest of a few fused train steps, for refactors that must change nothing.

Per case a GANTrainer is built from fixed seeds in deterministic mode (ops.set_deterministic) and
stepped; per step one line is printed with the losses (repr), a sha256 over the bytes of G's and
D's flat / grad / m / v, the fake buffer and -- in fp8 -- f8a.q, f8a.amax, f8w.q, and a hash of
the ordered irgan_* entry points called during the step (recorded by wrapping the loaded
library's function attributes here; the package is untouched).  Two trees that compute the same
print the same lines:

    python tools/step_digest.py [--tree DIR] [--cases bf16,fp8_ngf64,...]

--tree: the directory holding the package to import (default: this checkout); with IRGAN_LIB set,
another tree's Python files run against one built library.
"""
import argparse
import hashlib
import importlib
import os
import sys
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "infrared-colorization-with-resnet-generator-and-patchgan_amd"

PERC_THREE = dict(perc_layers=("relu1_2", "relu2_2", "relu3_3"), perc_weights=(1.0, 0.5, 0.25))
# name -> (steps, B, H, W, Config overrides, generator overrides outside Config)
CASES = {
    "bf16": (3, 2, 64, 64, {}, {}),
    "fp8_ngf64": (3, 2, 64, 64, dict(compute_dtype="fp8"), {}),               # step 1 calibrates; (True, True)
    "fp8_ngf32": (3, 2, 64, 64, dict(compute_dtype="fp8", ngf=32), {}),       # (True, False)
    "fp8_576": (2, 1, 576, 576, dict(compute_dtype="fp8"), {}),               # (True, False): the tile limit
    "bf16_66x70": (2, 2, 66, 70, {}, {}),
    "fp32": (2, 2, 64, 64, dict(compute_dtype="fp32"), {}),
    "norm_none": (2, 2, 64, 64, dict(norm="none"), {}),
    "norm_batch": (2, 2, 64, 64, dict(norm="batch"), {}),
    "replicate": (2, 2, 64, 64, {}, dict(padding_type="replicate")),
    "zero": (2, 2, 64, 64, {}, dict(padding_type="zero")),
    "dropout": (2, 2, 64, 64, {}, dict(use_dropout=True)),
    "no_antialias": (2, 2, 64, 64, dict(no_antialias=True), {}),
    "no_antialias_up": (2, 2, 64, 64, dict(no_antialias_up=True), {}),
    # VGGEngine.backward_taps: a tap fused into each pool backward (IRGAN_NO_TAP_FUSION=1: unfused)
    "perc_three": (2, 2, 64, 64, PERC_THREE, {}),
    "perc_three_fp32": (2, 2, 64, 64, dict(PERC_THREE, compute_dtype="fp32"), {}),
}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--cases", default=",".join(CASES))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    irc = importlib.import_module(PKG)
    lib, calls = irc._lib.load(), []
    for name, _, _ in irc._lib.PROTOS:   # record every entry point the step calls, in order

        def wrapped(*a, _fn=getattr(lib, name), _name=name):
            calls.append(_name)
            return _fn(*a)
        setattr(lib, name, wrapped)
    irc.ops.set_deterministic(True)
    print(f"# build {irc._lib.build_id(lib)}  torch {torch.__version__}")

    def digest(tensors):
        h = hashlib.sha256()
        for t in tensors:
            h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
        return h.hexdigest()[:32]

    for case in args.cases.split(","):
        steps, B, H, W, cfg_over, gen_over = CASES[case]
        cfg = irc.Config()
        cfg.device, cfg.batch_size, cfg.img_size = "cuda:0", B, H
        for k, v in cfg_over.items():
            setattr(cfg, k, v)
        torch.manual_seed(1234)
        model = None
        if gen_over:   # constructor options of the generator that Config does not carry
            netG = irc.ResnetUNetGenerator(cfg.input_nc, cfg.output_nc, cfg.ngf, irc.get_norm_layer(cfg.norm),
                                           device=torch.device(cfg.device), compute_dtype=cfg.compute_dtype,
                                           **gen_over)
            model = types.SimpleNamespace(netG=irc.init_net(netG))
        tr = irc.GANTrainer(cfg, model=model)
        eng = tr.netG.engine
        if eng.fp8:
            print(f"# {case}: fp8_layers{(B, H, W)} = {eng.fp8_layers(B, H, W)}")
        g = torch.Generator().manual_seed(7)
        for s in range(steps):
            ir = (torch.rand(B, 1, H, W, generator=g) * 2 - 1).cuda()
            rgb = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
            del calls[:]
            losses = tr.losses(tr.step(ir, rgb))
            torch.cuda.synchronize()
            names = [c for c in calls]
            ts = [getattr(st, n) for st in (tr.netG.store, tr.netD.store) for n in ("flat", "grad", "m", "v")]
            ts.append(eng.bufs.d["fake"])
            if eng.fp8:
                ts += [eng.f8a.q, eng.f8a.amax, eng.f8w.q]
            print(f"{case} step {s + 1}: losses {losses!r} bits {digest(ts)} "
                  f"calls {len(names)} {hashlib.sha256(' '.join(names).encode()).hexdigest()[:16]}", flush=True)
        del tr, eng, model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
