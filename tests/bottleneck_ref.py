"""Test-only CPU oracle of the ResNet-50/101 backbones (torchvision v1.5 bottleneck): plain F.conv2d, NCHW, any dtype.

oracle/ref_cpu.backbone_features is the BasicBlock oracle (conv1 carries the stride, conv3 does not exist), so it cannot serve here; the neck and
heads are ref_cpu's own (neck_forward / head_forward).  The reference tree has no ResNet source: this parity is unpinned, as for ResNet-34 —
what is restated is torchvision's public topology (conv1 1x1 -> conv2 3x3 with the stride -> conv3 1x1 x4, downsample 1x1 + BN in the first block
of every stage, ReLU after the residual sum)."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

import ref_cpu
from ref_cpu import _bn, _conv_bn_relu


def is_bottleneck(sd):
    return "backbone.layer1.0.conv3.weight" in sd


def backbone_features(sd, x, stats=None):
    """-> [f/2, f/4, f/8, f/16, f/32] with channels [64, 256, 512, 1024, 2048]."""
    p = "backbone."
    x = _conv_bn_relu(x, sd, p + "conv1", p + "bn1", stride=2, stats=stats)
    feats = [x]
    x = F.max_pool2d(x, 3, 2, 1)
    for li in range(1, 5):
        bi = 0
        while f"{p}layer{li}.{bi}.conv1.weight" in sd:
            q = f"{p}layer{li}.{bi}."
            stride = 2 if (bi == 0 and li > 1) else 1
            out = _conv_bn_relu(x, sd, q + "conv1", q + "bn1", stats=stats)
            out = _conv_bn_relu(out, sd, q + "conv2", q + "bn2", stride=stride, stats=stats)
            out = _conv_bn_relu(out, sd, q + "conv3", q + "bn3", relu=False, stats=stats)
            if q + "downsample.0.weight" in sd:
                idn = _bn(F.conv2d(x, sd[q + "downsample.0.weight"], None, stride=stride), sd, q + "downsample.1", stats)
            else:
                idn = x
            x = F.relu(out + idn)
            bi += 1
        feats.append(x)
    return feats


@torch.no_grad()
def forward(sd, x, sigmoid=True, stats=None, return_intermediates=False, upsample_type="nearest"):
    """ref_cpu.forward with the bottleneck backbone."""
    feats = backbone_features(sd, x, stats)
    neck = ref_cpu.neck_forward(sd, feats, stats, upsample_type)
    out, head_feats = OrderedDict(), OrderedDict()
    for name in ref_cpu.head_names(sd):
        y, head_feats[name] = ref_cpu.head_forward(sd, name, neck, stats, return_features=True)
        out[name] = y.sigmoid() if (name == "heatmap" and sigmoid) else y
    if return_intermediates == "heads":
        return out, feats, neck, head_feats
    if return_intermediates:
        return out, feats, neck
    return out


@torch.no_grad()
def forward_float64(sd, x, **kw):
    sd64 = OrderedDict((k, v.double() if v.is_floating_point() else v) for k, v in sd.items())
    return forward(sd64, x.double(), **kw)


@torch.no_grad()
def synth_state_dict(model_state_dict, seed=0, calib_shape=(2, 3, 128, 128), calib_seed=1234, upsample_type="nearest", bn3_gamma=(0.1, 0.3)):
    """ref_cpu.synth_state_dict's recipe (Kaiming convs, BN gamma ~ U(0.5, 1.5), beta ~ N(0, 0.1), out_conv ~ N(0, 0.01^2), running stats
    calibrated by one CPU forward) with two changes for 16 .. 33 residual blocks: every bn3 gets gamma ~ U(bn3_gamma) (torchvision's
    zero_init_residual in spirit: a block adds a small correction to its identity, so the residual stream stays O(1) through a stage), and the
    calibration pass runs THIS module's forward."""
    g = torch.Generator().manual_seed(seed)
    sd = OrderedDict((k, v.detach().clone().float().cpu() if v.is_floating_point() else v.detach().clone().cpu())
                     for k, v in model_state_dict.items())
    lo, hi = bn3_gamma
    for k, v in sd.items():
        if k.endswith("running_var"):
            base = k[: -len("running_var")]
            gam = torch.rand(v.shape, generator=g)
            sd[base + "weight"].copy_(gam * (hi - lo) + lo if base.endswith(".bn3.") else gam + 0.5)
            sd[base + "bias"].copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith("out_conv.weight"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.01)
        elif k.endswith("weight") and v.dim() == 4:
            fan_out = v.shape[0] * v.shape[2] * v.shape[3]
            v.copy_(torch.randn(v.shape, generator=g) * (2.0 / fan_out) ** 0.5)
            if k.endswith("offset_conv.weight"):
                v.mul_(0.02)
        elif k.endswith(("top_conv.bias", "project.0.bias", "project.1.bias")):
            v.copy_(torch.randn(v.shape, generator=g) * 0.05)
        elif k.endswith(".weights") and v.dim() == 1:
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
    xg = torch.Generator().manual_seed(calib_seed)
    forward(sd, torch.rand(*calib_shape, generator=xg), stats=True, upsample_type=upsample_type)
    return sd
