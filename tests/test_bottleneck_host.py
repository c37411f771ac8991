"""CPU: the ResNet-50 / 101 bottleneck backbones — parameter layout (torchvision's resnet50 / resnet101 minus fc), the feature contract the
necks build on (reference tests/test_models.py:38 builds every neck on resnet50; tests/test_backbones.py covers 18 / 34 / 50 / 101), checkpoint
loading, the C-ABI entry point of the fused 1x1 kernel, and the test oracle's own calibration."""
import ctypes
import os
import re

import pytest
import torch

import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, formats
from centernet_lightning_amd.params import ResNetBackbone

import bottleneck_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = {"heatmap": {"num_classes": 20}, "box_2d": {}}


@pytest.mark.parametrize("name, params, keys", [("resnet50", 23_508_032, 318), ("resnet101", 42_500_160, 624)])
def test_parameter_and_key_counts_equal_torchvision_without_fc(name, params, keys):
    # torchvision resnet50 / resnet101: 25,557,032 / 44,549,160 parameters, of which fc holds 2048 * 1000 + 1000 = 2,049,000
    b = ResNetBackbone(name)
    assert sum(p.numel() for p in b.parameters()) == params
    assert len(b.state_dict()) == keys
    assert b.out_channels == [64, 256, 512, 1024, 2048] and b.output_stride == 32


def test_bottleneck_shapes_and_v15_stride():
    b = ResNetBackbone("resnet50")
    sd = b.state_dict()
    assert tuple(sd["layer1.0.conv3.weight"].shape) == (256, 64, 1, 1)
    assert tuple(sd["layer4.0.downsample.0.weight"].shape) == (2048, 1024, 1, 1)
    assert tuple(sd["layer1.0.downsample.0.weight"].shape) == (256, 64, 1, 1)          # channels change in layer1.0: a stride-1 downsample
    assert b.layer2[0].conv2.stride == (2, 2) and b.layer2[0].conv1.stride == (1, 1)    # torchvision v1.5: the stride sits on the 3x3
    assert b.layer2[0].downsample[0].stride == (2, 2) and b.layer1[0].downsample[0].stride == (1, 1)
    for li, n in zip(range(1, 5), (3, 4, 6, 3)):
        layer = getattr(b, f"layer{li}")
        assert len(layer) == n
        assert layer[0].downsample is not None and all(blk.downsample is None for blk in list(layer)[1:])
    assert len(ResNetBackbone("resnet101").layer3) == 23


def test_torchvision_state_dict_loads_key_for_key():
    # a torchvision-layout state dict (the backbone's keys + fc.*): only fc is left over, as INTEGRATION.md says for ResNet-34
    m = cl.CenterNet({"name": "resnet50"}, {"name": "simple"}, HEADS, "detection")
    g = torch.Generator().manual_seed(0)
    tv = {k: torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone() for k, v in m.backbone.state_dict().items()}
    tv["fc.weight"], tv["fc.bias"] = torch.zeros(1000, 2048), torch.zeros(1000)
    missing, unexpected = m.backbone.load_state_dict(tv, strict=False)
    assert missing == [] and sorted(unexpected) == ["fc.bias", "fc.weight"]
    assert torch.equal(m.backbone.layer3[5].conv3.weight, tv["layer3.5.conv3.weight"])


@pytest.mark.parametrize("neck", ["simple", "fpn", "ida", "bifpn"])
def test_every_neck_on_resnet50(neck):
    m = cl.CenterNet({"name": "resnet50"}, {"name": neck}, HEADS, "detection")
    assert m.output_stride == 4 and m.stride == 4                                      # reference tests/test_models.py:61-66
    # simple / fpn / bifpn end in their own 64 channels; the IDA neck ends with the stride-4 feature's channel count (params.IDANeck): 256 here
    assert m.neck.out_channels == (256 if neck == "ida" else 64)
    assert m.heads["heatmap"].in_channels == m.neck.out_channels
    assert m.backbone.out_channels == [64, 256, 512, 1024, 2048]


def test_configs_build():
    for cfg, neck in (("resnet50_simple.yaml", "SimpleNeck"), ("resnet50_fpn.yaml", "FPNNeck")):
        m = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", cfg))
        assert m.backbone.name == "resnet50" and type(m.neck).__name__ == neck and m.num_classes == 80
    # the FPN's projections follow the wider skips
    m = cl.build_centernet(os.path.join(ROOT, "centernet-lightning_amd", "configs", "resnet50_fpn.yaml"))
    assert tuple(m.state_dict()["neck.fuse.0.project.0.weight"].shape) == (256, 1024, 1, 1)
    assert tuple(m.state_dict()["neck.top_conv.weight"].shape) == (256, 2048, 1, 1)


def test_lightning_checkpoint_of_a_resnet50_model_loads():
    src = cl.CenterNet({"name": "resnet50"}, {"name": "fpn"}, HEADS, "detection")
    dst = cl.CenterNet({"name": "resnet50"}, {"name": "fpn"}, HEADS, "detection")
    g = torch.Generator().manual_seed(3)
    sd = {k: (torch.randn(v.shape, generator=g) if v.is_floating_point() else v.clone()) for k, v in src.state_dict().items()}
    ckpt = {"epoch": 1, "state_dict": {"model." + k.replace("heads.", "output_heads.", 1): v for k, v in sd.items()}, "hyper_parameters": {}}
    missing, unexpected = formats.load_checkpoint(dst, ckpt)
    assert missing == [] and unexpected == []
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_unsupported_backbones_still_raise():
    for name in ("mobilenet_v2", "resnet152", "resnext50_32x4d", "timm_efficientnet_b0"):
        with pytest.raises(ValueError):
            cl.CenterNet({"name": name}, {"name": "simple"}, HEADS, "detection")


def test_pointwise_entry_point_declared_exported_and_validating():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    assert re.search(r"\bint cnl_pointwise_nhwc_f32\s*\(", header)
    assert "cnl_pointwise_nhwc_f32" in _lib.EXPORTED_SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, "cnl_pointwise_nhwc_f32")
    assert lib.cnl_version() == 13
    assert lib.cnl_pointwise_nhwc_f32(None, None, 0, 0, 0, 0, 1, None, None) == _lib.CNL_E_BAD_ARG
    p = _lib.ConvParams()
    p.x = p.w = p.bias = p.y = p.x_absmax = 0x1000
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = 1, 8, 8, 64, 256
    p.KH = p.KW = 1
    p.stride, p.pad, p.ldx, p.ldy = 1, 0, 64, 256
    p.flags = _lib.CNL_RELU                                                              # no CNL_W_SPLIT: the kernel reads pre-split weights only
    assert lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), None, 0, 0, 0, 0, 1, None, None) == _lib.CNL_E_BAD_ARG
    assert "CNL_W_SPLIT" in _lib.last_error()
    p.flags = _lib.CNL_RELU | _lib.CNL_W_SPLIT
    p.algo = _lib.CNL_ALGO_F32
    assert lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), None, 0, 0, 0, 0, 1, None, None) == _lib.CNL_E_UNSUPPORTED
    p.algo = _lib.CNL_ALGO_AUTO
    p.KH = p.KW = 3
    assert lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), None, 0, 0, 0, 0, 1, None, None) == _lib.CNL_E_UNSUPPORTED
    p.KH = p.KW = 1
    # two-source: x2 must give the output size at its stride, and carry its own maxima
    assert lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), 0x2000, 15, 15, 64, 64, 2, None, None) == _lib.CNL_E_BAD_ARG
    assert "x2_absmax" in _lib.last_error()
    assert lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), 0x2000, 17, 16, 64, 64, 2, 0x3000, None) == _lib.CNL_E_BAD_ARG
    assert lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), 0x2000, 16, 16, 64, 64, 3, 0x3000, None) == _lib.CNL_E_UNSUPPORTED
    # the conv params layout and its ABI check are untouched
    assert [lib.cnl_sizeof_params(i) for i in range(4)] == [ctypes.sizeof(_lib.ConvParams), ctypes.sizeof(_lib.DecodeParams),
                                                          ctypes.sizeof(_lib.DeconvParams), 0]


def test_oracle_bottleneck_backbone_and_calibration():
    m = cl.CenterNet({"name": "resnet50"}, {"name": "simple"}, HEADS, "detection")
    sd = bottleneck_ref.synth_state_dict(m.state_dict(), seed=0, calib_shape=(2, 3, 128, 128))
    assert bottleneck_ref.is_bottleneck(sd)
    x = torch.rand(1, 3, 128, 128, generator=torch.Generator().manual_seed(5))
    out, feats, neck = bottleneck_ref.forward(sd, x, return_intermediates=True)
    assert [tuple(f.shape[1:]) for f in feats] == [(64, 64, 64), (256, 32, 32), (512, 16, 16), (1024, 8, 8), (2048, 4, 4)]
    assert all(0.5 < float(f.abs().max()) < 50 for f in feats), [float(f.abs().max()) for f in feats]     # O(1) through the 16 blocks
    assert tuple(out["heatmap"].shape) == (1, 20, 32, 32) and tuple(out["box_2d"].shape) == (1, 4, 32, 32)
    # one oracle block against torch's own modules holding the same weights: layer2.0 (stride 2, downsample), through a state dict whose
    # layer2 stops after that block
    blk = m.backbone.layer2[0]
    blk.load_state_dict({k[len("backbone.layer2.0."):]: v for k, v in sd.items() if k.startswith("backbone.layer2.0.")})
    blk.eval()
    with torch.no_grad():
        t = torch.relu(blk.bn1(blk.conv1(feats[1])))
        t = torch.relu(blk.bn2(blk.conv2(t)))
        want = torch.relu(blk.bn3(blk.conv3(t)) + blk.downsample(feats[1]))
    one = {k: v for k, v in sd.items() if not re.match(r"backbone\.layer2\.[1-9]\.", k)}
    got = bottleneck_ref.backbone_features(one, x)[2]
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
