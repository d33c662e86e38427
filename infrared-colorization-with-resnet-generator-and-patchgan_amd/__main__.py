"""``python -m infrared-colorization-with-resnet-generator-and-patchgan_amd [train|test]
[--img-size N | HxW | native] [--load-size N | HxW | native] [--ema-decay D] [--clip-grad-G X]
[--clip-grad-D X] [--gan-mode hinge|lsgan|vanilla] [--gan-real-label T] [--perc-layers L,L,...]
[--perc-weights W,W,...]`` -- the reference's script
entry point (ir:1730-1756) with cfg.mode taken from the command line (default: Config's "test").
``--img-size`` sets cfg.img_size: N for N x N, HxW (height first, e.g. 512x640) or ``native`` for
every frame at its own size; ``--load-size`` sets cfg.load_size, the training crop jitter: every
training pair is resized to N x N, HxW or (``native``) left at its own size, and a random
cfg.img_size window of it is the sample (e.g. ``--load-size 286`` with the default 256; validation
and test ignore it); ``--ema-decay`` sets cfg.ema_decay (e.g. 0.999: train with a moving average
of the generator weights); ``--clip-grad-G`` / ``--clip-grad-D`` set cfg.clip_grad_G / cfg.clip_grad_D, the
maximal L2 norm of the generator's / discriminator's gradient (clipped inside the fused Adam update,
the norms join the step log); ``--gan-mode`` sets cfg.gan_mode, the GAN objective of the fused step
(``hinge``, the reference's; ``lsgan``; ``vanilla`` = BCE with logits), and ``--gan-real-label`` cfg.gan_real_label,
D's target for real patches in (0, 1] (e.g. 0.9: one-sided label smoothing, lsgan / vanilla only);
``--perc-layers`` sets cfg.perc_layers, the VGG maps of the perceptual term (comma-separated names out of
relu1_1 .. relu3_3, e.g. ``relu1_2,relu2_2,relu3_3``), and ``--perc-weights`` cfg.perc_weights, one weight per
layer (e.g. ``1,0.5,0.25``).  Without a flag Config's value stands."""
import argparse
import sys

from .data import parse_img_size, parse_load_size
from .ir_colorization import Config, main
from .ops import GAN_MODES


def config_from_argv(argv):
    ap = argparse.ArgumentParser(prog="python -m infrared-colorization-with-resnet-generator-and-patchgan_amd")
    ap.add_argument("mode", nargs="?", help="train or test (default: Config.mode)")
    ap.add_argument("--img-size", type=parse_img_size, default=argparse.SUPPRESS, metavar="N|HxW|native")
    ap.add_argument("--load-size", type=parse_load_size, default=argparse.SUPPRESS, metavar="N|HxW|native")
    ap.add_argument("--ema-decay", type=float, default=argparse.SUPPRESS, metavar="D")
    ap.add_argument("--clip-grad-G", type=float, default=argparse.SUPPRESS, metavar="X", dest="clip_grad_G")
    ap.add_argument("--clip-grad-D", type=float, default=argparse.SUPPRESS, metavar="X", dest="clip_grad_D")
    ap.add_argument("--gan-mode", choices=sorted(GAN_MODES), default=argparse.SUPPRESS)
    ap.add_argument("--gan-real-label", type=float, default=argparse.SUPPRESS, metavar="T")
    ap.add_argument("--perc-layers", type=lambda v: tuple(n.strip() for n in v.split(",")),
                    default=argparse.SUPPRESS, metavar="L,L,...")
    ap.add_argument("--perc-weights", type=lambda v: tuple(float(w) for w in v.split(",")),
                    default=argparse.SUPPRESS, metavar="W,W,...")
    a = ap.parse_args(argv)
    cfg = Config()
    if a.mode is not None:
        cfg.mode = a.mode
    if hasattr(a, "img_size"):
        cfg.img_size = a.img_size
    if hasattr(a, "load_size"):
        cfg.load_size = a.load_size
    if hasattr(a, "ema_decay"):
        cfg.ema_decay = a.ema_decay
    for name in ("clip_grad_G", "clip_grad_D", "gan_mode", "gan_real_label", "perc_layers", "perc_weights"):
        if hasattr(a, name):
            setattr(cfg, name, getattr(a, name))
    return cfg


if __name__ == "__main__":
    main(config_from_argv(sys.argv[1:]))
