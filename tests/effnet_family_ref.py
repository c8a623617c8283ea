"""CPU reference for the EfficientNet-b0..b7 encoders (test-side only).

efficientnet_pytorch builds all eight variants from the b0 stage table and one compound-scaling rule:
round_filters(f, w) for the channel widths, round_repeats(r, d) for the block counts, and the variant's
own image size for the static "same" pads.  This module applies that rule and reuses everything else
from oracle.unet_oracle (MBConv, _SamePadConv, _static_same_pad, the decoders, OracleUnet.forward).
It builds modules in the oracle's order, so with b4's coefficients and the same seed it equals
O.build("efficientnet-b4") exactly.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from oracle import unet_oracle as O

# b0 stage table: (repeats, kernel, stride, expand, in, out); stem 32
B0_STAGES = [(1, 3, 1, 1, 32, 16), (2, 3, 2, 6, 16, 24), (2, 5, 2, 6, 24, 40), (3, 3, 2, 6, 40, 80),
             (3, 5, 1, 6, 80, 112), (4, 5, 2, 6, 112, 192), (1, 3, 1, 6, 192, 320)]
# (width, depth, image size)
COEFS = {"efficientnet-b0": (1.0, 1.0, 224), "efficientnet-b1": (1.0, 1.1, 240), "efficientnet-b2": (1.1, 1.2, 260),
         "efficientnet-b3": (1.2, 1.4, 300), "efficientnet-b4": (1.4, 1.8, 380), "efficientnet-b5": (1.6, 2.2, 456),
         "efficientnet-b6": (1.8, 2.6, 528), "efficientnet-b7": (2.0, 3.1, 600)}
VARIANTS = tuple(COEFS)


def round_filters(f, w):
    f = f * w
    n = max(8, int(f + 4) // 8 * 8)
    if n < 0.9 * f:
        n += 8
    return n


def round_repeats(r, d):
    return int(math.ceil(d * r))


def stages(name):
    w, d, _ = COEFS[name]
    return [(round_repeats(r, d), k, s, e, round_filters(ci, w), round_filters(co, w)) for r, k, s, e, ci, co in B0_STAGES]


def stem_channels(name):
    return round_filters(32, COEFS[name][0])


def taps(name):
    cum, n = [], 0
    for st in stages(name):
        n += st[0]
        cum.append(n)
    return (cum[1], cum[2], cum[4], cum[6])


def out_channels(name, in_channels=3):
    st = stages(name)
    return (in_channels, stem_channels(name), st[1][5], st[2][5], st[4][5], st[6][5])


def head_params(name):
    """Classifier head efficientnet_pytorch adds on top (_conv_head 1x1 -> round_filters(1280), _bn1, _fc -> 1000 classes)."""
    c_in, c_head = stages(name)[-1][5], round_filters(1280, COEFS[name][0])
    return c_in * c_head + 2 * c_head + c_head * 1000 + 1000


class EfficientNetEncoder(nn.Module):
    """smp EfficientNetEncoder(name): features after the stem and after the blocks of stages 1, 2, 4 and 6."""

    def __init__(self, name, in_channels=3):
        super().__init__()
        stem = stem_channels(name)
        b, e, size = O._static_same_pad(COEFS[name][2], 3, 2)
        self._conv_stem = O._SamePadConv(in_channels, stem, 3, 2, 1, (b, e))
        self._bn0 = nn.BatchNorm2d(stem, eps=1e-3, momentum=0.01)
        table = stages(name)
        nblocks = sum(st[0] for st in table)
        blocks = []
        for rep, k, s, ex, ci, co in table:
            for r in range(rep):
                idx = len(blocks)
                blk = O.MBConv(ci if r == 0 else co, co, k, s if r == 0 else 1, ex, size, 0.2 * idx / nblocks)
                size = blk.out_size
                blocks.append(blk)
        self._blocks = nn.ModuleList(blocks)
        self.stage_idxs = taps(name)
        self.out_channels = out_channels(name, in_channels)

    forward = O.EfficientNetB4Encoder.forward


def _init(self, encoder_name="efficientnet-b3", decoder_channels=(256, 128, 64, 32, 16), in_channels=3, classes=1):
    # OracleUnet.__init__ with the family encoder: same module order, same initialisers
    nn.Module.__init__(self)
    self.encoder = EfficientNetEncoder(encoder_name, in_channels)
    self.decoder = self._DECODER(self.encoder.out_channels, tuple(decoder_channels))
    head = nn.Conv2d(decoder_channels[-1], classes, 3, 1, 1)
    nn.init.xavier_uniform_(head.weight)
    nn.init.constant_(head.bias, 0)
    self.segmentation_head = nn.Sequential(head, nn.Identity(), nn.Identity())


class FamilyUnet(O.OracleUnet):
    __init__ = _init


class FamilyUnetPlusPlus(O.OracleUnetPlusPlus):
    __init__ = _init


def build(encoder_name, seed=42, arch="Unet", **kw):
    torch.manual_seed(seed)
    return {"Unet": FamilyUnet, "UnetPlusPlus": FamilyUnetPlusPlus}[arch](encoder_name=encoder_name, **kw)


def encoder_params(model):
    return sum(p.numel() for p in model.encoder.parameters())


def conv_flops(model, h, w, in_channels=3):
    """Algorithmic conv FLOPs per image, (forward, forward + backward), counted over the module's own Conv2d layers in one
    eval forward: 2 * Ho*Wo*Cout*(Cin/groups)*k*k each, times 3 with the backward except for the stem (no input gradient)."""
    macs = []

    def hook(mod, inp, out):
        k = mod.kernel_size[0] * mod.kernel_size[1]
        macs.append((out.shape[2] * out.shape[3] * mod.out_channels * (mod.in_channels // mod.groups) * k, mod))

    hs = [m.register_forward_hook(hook) for m in model.modules() if isinstance(m, nn.Conv2d)]
    was = model.training
    model.eval()
    try:
        with torch.no_grad():
            model(torch.zeros(1, in_channels, h, w))
    finally:
        for hd in hs:
            hd.remove()
        model.train(was)
    stem = model.encoder._conv_stem
    fwd = 2.0 * sum(m for m, _ in macs)
    fb = 2.0 * sum(m * (2.0 if mod is stem else 3.0) for m, mod in macs)
    return fwd, fb
