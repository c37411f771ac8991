"""Fine-tuning the heads on the GPU: a convolution torch.autograd can differentiate, and the trainer built on it.

    trainer = model.head_trainer()                       # parameters() ARE model.heads' parameters
    optimiser = torch.optim.SGD(trainer.parameters(), lr=0.01, momentum=0.9)
    out = trainer(images)                                # {"heatmap" (logits), "box_2d"[, "reid"]} with a grad_fn
    criterion(out, targets)["total"].backward()
    optimiser.step()                                     # the next model(images) sees the trained heads (the engine re-folds by itself)

Scope: the heads only (GenericHead: 3x3 conv + BatchNorm + ReLU blocks, then a 1x1 out_conv), stride 1, fp32.  Backbone and neck are frozen and
run as the inference plan (CenterNet.neck_features, no grad); BatchNorm uses its running statistics, frozen, which is what the engine folds — the
fold is written with torch ops here, so autograd carries the folded gradients back to conv weight, gamma and beta.  The HIP layer sees folded OHWI
weights only: forward is one cnl_conv2d_nhwc_f32 call (fp32 matrix cores), backward is cnl_relu_grad_f32, then cnl_conv_wgrad_nhwc_f32 and the input
gradient (cnl_conv1x1_dgrad_nhwc_f32, or for 3x3 the forward conv on the rotated, transposed weights) for the inputs that require grad.  No
double backward, no CPU path.
"""
import ctypes

import torch
from torch import nn
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import CNL_RELU, ConvParams

__all__ = ["conv2d_nhwc", "relu_grad", "conv_wgrad", "conv1x1_dgrad", "conv3x3_dgrad", "HeadTrainer"]


def _require_cuda_f32(name, t):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"conv_grad: {name} must be a tensor on a HIP device (there is no CPU path)")
    if t.dtype != torch.float32:
        raise ValueError(f"conv_grad: {name} must be float32, got {t.dtype}")


def _nhwc(name, t):
    """A logical [N, C, H, W] tensor whose memory is NHWC with a pixel stride (a channels-last tensor or a channel slice of one) ->
    (tensor, ld); anything else is copied to channels-last."""
    N, C, H, W = t.shape
    ok = (t.stride(1) == 1 and t.stride(3) % 4 == 0 and t.stride(3) >= C and t.stride(2) == W * t.stride(3) and t.stride(0) == H * t.stride(2)
          and t.data_ptr() % 16 == 0)
    if not ok:
        ld = (C + 3) // 4 * 4
        buf = torch.empty((N, H, W, ld), device=t.device, dtype=torch.float32)
        buf[..., :C].copy_(t.permute(0, 2, 3, 1))
        t = buf[..., :C].permute(0, 3, 1, 2)
    return t, t.stride(3)


def _conv_forward(x, ldx, w_ohwi, bias, relu):
    """One cnl_conv2d_nhwc_f32 launch, the default kernel choice without hints (fp32 matrix cores) -> y [N, H, W, Cout] contiguous."""
    lib = _lib.load()
    N, Cin, H, W = x.shape
    Cout, KH, KW, _ = w_ohwi.shape
    y = torch.empty((N, H, W, Cout), device=x.device, dtype=torch.float32)
    p = ConvParams()
    p.x, p.w, p.bias, p.y = x.data_ptr(), w_ohwi.data_ptr(), bias.data_ptr(), y.data_ptr()
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = N, H, W, Cin, Cout
    p.KH, p.KW, p.stride, p.pad = KH, KW, 1, (KH - 1) // 2
    p.ldx, p.ldy, p.ldr = ldx, Cout, 0
    p.flags = CNL_RELU if relu else 0
    with torch.cuda.device(x.device):
        _lib.check(lib.cnl_conv2d_nhwc_f32(ctypes.byref(p), _lib.stream(x.device)), "conv2d_nhwc: cnl_conv2d_nhwc_f32")
    return y


def relu_grad(dy, y=None, want_bias=True):
    """dy: logical [N, C, H, W], any strides; y: the conv's output [N, H, W, C] (NHWC, contiguous or a channel slice) or None
    -> (dz [N, H, W, ld] with ld = C rounded up to 4 — its first C channels are written —, dbias [C] or None)"""
    lib = _lib.load()
    _require_cuda_f32("dy", dy)
    N, C, H, W = dy.shape
    ld = (C + 3) // 4 * 4
    dz = torch.empty((N, H, W, ld), device=dy.device, dtype=torch.float32)
    dbias = torch.empty((C,), device=dy.device, dtype=torch.float32) if want_bias else None
    nbytes = lib.cnl_relu_grad_workspace_bytes(N, C, H, W) if want_bias else 0
    ws = torch.empty((max(nbytes, 4) // 4,), device=dy.device, dtype=torch.float32) if want_bias else None
    sn, sc, sh, sw = dy.stride()
    with torch.cuda.device(dy.device):
        _lib.check(lib.cnl_relu_grad_f32(dy.data_ptr(), sn, sc, sh, sw, y.data_ptr() if y is not None else None, y.stride(2) if y is not None else 0,
                                         N, C, H, W, dz.data_ptr(), ld, dbias.data_ptr() if want_bias else None, ws.data_ptr() if want_bias else None,
                                         nbytes, _lib.stream(dy.device)), "cnl_relu_grad_f32")
    return dz, dbias


def conv_wgrad(x, ldx, dz, lddz, Cout, KH, KW):
    """x: logical [N, Cin, H, W] NHWC memory with pixel stride ldx; dz: [N, H, W, lddz] -> dW [Cout, KH, KW, Cin] (OHWI)"""
    lib = _lib.load()
    N, Cin, H, W = x.shape
    nbytes = lib.cnl_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout, KH, KW)
    dw = torch.empty((Cout, KH, KW, Cin), device=x.device, dtype=torch.float32)
    ws = torch.empty((max(nbytes, 16) // 4,), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _lib.check(lib.cnl_conv_wgrad_nhwc_f32(x.data_ptr(), ldx, dz.data_ptr(), lddz, dw.data_ptr(), N, H, W, Cin, Cout, KH, KW, (KH - 1) // 2,
                                               ws.data_ptr(), nbytes, _lib.stream(x.device)), "cnl_conv_wgrad_nhwc_f32")
    return dw


def conv1x1_dgrad(dz, lddz, w_ohwi, N, H, W):
    """dz [N, H, W, lddz], w [Cout, 1, 1, Cin] -> dx, logical [N, Cin, H, W] (a channels-last view)"""
    lib = _lib.load()
    Cout, _, _, Cin = w_ohwi.shape
    dx = torch.empty((N, H, W, Cin), device=dz.device, dtype=torch.float32)
    with torch.cuda.device(dz.device):
        _lib.check(lib.cnl_conv1x1_dgrad_nhwc_f32(dz.data_ptr(), lddz, w_ohwi.data_ptr(), dx.data_ptr(), Cin, N, H, W, Cin, Cout, _lib.stream(dz.device)),
                   "cnl_conv1x1_dgrad_nhwc_f32")
    return dx.permute(0, 3, 1, 2)


def conv3x3_dgrad(dz, lddz, w_ohwi):
    """dx = conv3x3(dz, w rotated by 180 degrees with O and I swapped): the existing forward entry point on the fp32 matrix cores (no hints).
    dz [N, H, W, lddz], w [Cout, 3, 3, Cin] -> dx, logical [N, Cin, H, W] (a channels-last view)"""
    Cout, KH, KW, Cin = w_ohwi.shape
    if Cout % 32:
        raise ValueError(f"conv2d_nhwc: the input gradient of a {KH} x {KW} conv runs as a forward conv over its {Cout} output channels, which must be a "
                         "multiple of 32")
    N, H, W, _ = dz.shape
    w_rot = w_ohwi.flip(1, 2).permute(3, 1, 2, 0).contiguous()
    zero = torch.zeros((Cin,), device=dz.device, dtype=torch.float32)
    dx = _conv_forward(dz[..., :Cout].permute(0, 3, 1, 2), lddz, w_rot, zero, False)
    return dx.permute(0, 3, 1, 2)


class _Conv2dNHWC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w_ohwi, bias, relu):
        x_, ldx = _nhwc("x", x.detach())
        w_ = w_ohwi.detach().contiguous()
        b_ = bias.detach().contiguous() if bias is not None else torch.zeros((w_.shape[0],), device=x.device, dtype=torch.float32)
        y = _conv_forward(x_, ldx, w_, b_, relu)
        ctx.relu, ctx.has_bias = relu, bias is not None
        ctx.save_for_backward(x_, w_, y)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        _require_cuda_f32("the output gradient", dy)
        Cout, KH, KW, Cin = w.shape
        N, _, H, W = x.shape
        dz, db = relu_grad(dy, y if ctx.relu else None, want_bias=need_b)
        lddz = dz.shape[3]
        dw = conv_wgrad(x, x.stride(3), dz, lddz, Cout, KH, KW) if need_w else None
        dx = None
        if need_x:
            dx = conv1x1_dgrad(dz, lddz, w, N, H, W) if KH == 1 else conv3x3_dgrad(dz, lddz, w)
        return dx, dw, db, None


def conv2d_nhwc(x, w_ohwi, bias=None, relu=True):
    """relu(conv(x, w) + bias) (relu=False: no activation) for a stride-1 3x3 / pad 1 or 1x1 conv, differentiable once.
    x: logical [N, Cin, H, W], fp32 on a HIP device, Cin % 32 == 0 — a channels-last tensor (as the engine's outputs are) is read in place, any
    other layout is copied; w_ohwi: [Cout, KH, KW, Cin] (the engine's weight layout); bias: [Cout] or None.  -> logical [N, Cout, H, W], a
    channels-last view.  Gradients arrive for x, w_ohwi and bias, each only where it requires grad."""
    for name, t in (("x", x), ("w_ohwi", w_ohwi)) + ((("bias", bias),) if bias is not None else ()):
        _require_cuda_f32(name, t)
    if x.dim() != 4 or w_ohwi.dim() != 4 or w_ohwi.shape[3] != x.shape[1]:
        raise ValueError(f"conv2d_nhwc: x {tuple(x.shape)} [N, Cin, H, W] against w_ohwi {tuple(w_ohwi.shape)} [Cout, KH, KW, Cin]")
    if tuple(w_ohwi.shape[1:3]) not in ((3, 3), (1, 1)):
        raise ValueError(f"conv2d_nhwc: kernel {tuple(w_ohwi.shape[1:3])}: 3 x 3 (pad 1) and 1 x 1 only, stride 1")
    if x.shape[1] % 32:
        raise ValueError(f"conv2d_nhwc: Cin = {x.shape[1]} is not a multiple of 32")
    if bias is not None and tuple(bias.shape) != (w_ohwi.shape[0],):
        raise ValueError(f"conv2d_nhwc: bias {tuple(bias.shape)} against Cout = {w_ohwi.shape[0]}")
    return _Conv2dNHWC.apply(x, w_ohwi, bias, bool(relu))


class HeadTrainer(nn.Module):
    """The heads of a CenterNet as a trainable module over the frozen trunk.  parameters() are model.heads' own parameters (the state-dict keys
    are model.heads'); BatchNorm runs on its running statistics, which stay as they are."""

    def __init__(self, model):
        super().__init__()
        for name, head in model.heads.items():
            for blk in head.blocks():
                if type(blk).__name__ != "ConvBn":
                    raise ValueError(f"HeadTrainer: heads.{name} has a {type(blk).__name__} block: only conv_type 'normal' heads (3x3 conv + BatchNorm + ReLU) "
                                     "can be trained here")
            conv_type = (model.config_section["output_heads"].get(name) or {}).get("conv_type", "normal")
            if conv_type != "normal":
                raise ValueError(f"HeadTrainer: heads.{name} is configured with conv_type {conv_type!r}: only 'normal' heads can be trained here")
        self.heads = model.heads
        self._model_ref = [model]          # list: keep the model out of the module tree (the trunk's parameters are not this module's)

    def train(self, mode: bool = True):
        """BatchNorm statistics are frozen either way: the heads stay in eval mode (the model they belong to refuses train(True))."""
        self.training = bool(mode)
        return self

    @staticmethod
    def _folded(blk):
        conv, bn = blk.conv_module, blk.bn_module
        scale = bn.weight / torch.sqrt(bn.running_var + bn.eps)
        w = (conv.weight * scale.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).contiguous()
        b = bn.bias - bn.running_mean * scale
        if conv.bias is not None:
            b = b + conv.bias * scale
        return w, b

    def forward_features(self, f):
        """f: the neck map [N, C, H, W] (neck_features' tensor; no gradient flows into it) -> {"heatmap" (logits), "box_2d"[, "reid"]}"""
        f = f.detach()
        out = {}
        for name, head in self.heads.items():
            t = f
            for blk in head.blocks():
                w, b = self._folded(blk)
                t = conv2d_nhwc(t, w, b, relu=True)
            oc = head.out_conv
            out[name] = conv2d_nhwc(t, oc.weight.permute(0, 2, 3, 1).contiguous(), oc.bias, relu=False)
        return out

    def forward(self, x):
        with torch.no_grad():
            f = self._model_ref[0].neck_features(x)
        return self.forward_features(f)
