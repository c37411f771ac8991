"""GPU: the ResNet-50 / 101 bottleneck backbones and their fused 1x1 kernel (cnl_pointwise_nhwc_f32, csrc/pointwise.hip).

Kernel level: single- and two-source launches against float64 (max |gpu - f64| / max |f64| <= 1e-5) over the ResNet-50 channel counts, odd map sizes,
residual / no residual, stride 1 / 2 on the second source; y_absmax equals max |y| per image; an outlier inside one image changes no bit of another
image; a shard gives the bits of the full batch.  Plan level: every bottleneck conv3 with a downsample is ONE two-source launch, no ResNet-18 / 34
launch reaches the new entry point, and a resnet50 plan replays launch by launch against float64 (tests/test_gpu_plan_replay.py's stepper and
checker, with a checker for the new launch kind).  End to end: resnet50 simple / fpn, resnet101 simple and a resnet50-fpn tracking model against
the CPU oracle of tests/bottleneck_ref.py."""
import ctypes
import os
import re
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import bottleneck_ref
import recipes
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd._lib import CNL_ALGO_FORCE, CNL_RELU, CNL_W_SPLIT, ConvParams

import test_gpu_plan_replay as rp

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _slots(x):
    """cnl_absmax_per_image_f32 of an NHWC device tensor -> the strided slot array."""
    lib = _lib.load()
    ams = _lib.absmax_stride()
    N, H, W, C = x.shape
    out = torch.zeros(N * ams, device="cuda")
    _lib.check(lib.cnl_absmax_per_image_f32(x.data_ptr(), N, H * W, C, C, out.data_ptr(), _stream()), "absmax")
    return out


def pointwise(x1, w1, b, x2=None, w2=None, s2=1, res=None, relu=True, algo=0):
    """One cnl_pointwise_nhwc_f32 launch on NHWC device tensors; w1 [Cout, C1], w2 [Cout, C2] (fp32).  -> (y, per-image y_absmax)."""
    lib = _lib.load()
    ams = _lib.absmax_stride()
    N, H, W, C1 = x1.shape
    cout = w1.shape[0]
    wcat = (torch.cat([w1, w2], 1) if x2 is not None else w1).contiguous().cuda()
    K = wcat.shape[1]
    wbuf = torch.empty(lib.cnl_conv_split_weight_floats(K, cout, 1, 1), device="cuda")
    _lib.check(lib.cnl_conv_split_weights_f32(wcat.data_ptr(), wbuf.data_ptr(), K, cout, 1, 1, _stream()), "split")
    xs1 = _slots(x1)
    xs2 = _slots(x2) if x2 is not None else None
    y = torch.full((N, H, W, cout), float("nan"), device="cuda")
    ys = torch.zeros(N * ams, device="cuda")
    bias = b.contiguous().cuda()
    p = ConvParams()
    p.x, p.w, p.bias, p.y = x1.data_ptr(), wbuf.data_ptr(), bias.data_ptr(), y.data_ptr()
    p.residual = res.data_ptr() if res is not None else None
    p.N, p.H_in, p.W_in, p.Cin, p.Cout = N, H, W, C1, cout
    p.KH = p.KW = p.stride = 1
    p.pad = 0
    p.ldx, p.ldy, p.ldr = C1, cout, cout if res is not None else 0
    p.flags = (CNL_RELU if relu else 0) | CNL_W_SPLIT
    p.algo = algo
    p.x_absmax, p.y_absmax = xs1.data_ptr(), ys.data_ptr()
    if x2 is not None:
        _, H2, W2, C2 = x2.shape
        rc = lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), x2.data_ptr(), H2, W2, C2, C2, s2, xs2.data_ptr(), _stream())
    else:
        rc = lib.cnl_pointwise_nhwc_f32(ctypes.byref(p), None, 0, 0, 0, 0, 1, None, _stream())
    _lib.check(rc, "cnl_pointwise_nhwc_f32")
    torch.cuda.synchronize()
    return y, ys.view(N, ams)[:, 0].clone()


def ref64(x1, w1, b, x2=None, w2=None, s2=1, res=None, relu=True):
    z = x1.double().cpu().reshape(-1, x1.shape[-1]) @ w1.double().cpu().t()
    if x2 is not None:
        z = z + x2[:, ::s2, ::s2, :].double().cpu().reshape(-1, x2.shape[-1]) @ w2.double().cpu().t()
    z = z.reshape(*x1.shape[:3], -1) + b.double().cpu()
    if res is not None:
        z = z + res.double().cpu()
    return z.clamp_min(0) if relu else z


def _act(shape, seed, scale=1.0, relu=True):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g) * scale
    return (t.clamp_min(0) if relu else t).cuda()


def _w(cout, cin, seed, gain=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(cout, cin, generator=g) * (2.0 / cin) ** 0.5 * gain


def _rel(y, y64):
    return float((y.double().cpu() - y64).abs().max() / y64.abs().max())


def _check_ymax(y, ys):
    assert torch.equal(ys.cpu(), y.abs().amax(dim=(1, 2, 3)).cpu()), (ys, y.abs().amax(dim=(1, 2, 3)))


# ------------------------------------------------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("cin", [64, 256, 512, 1024, 2048])
@pytest.mark.parametrize("cout", [64, 128, 256, 512, 1024, 2048])
def test_single_source_against_float64(cin, cout):
    x = _act((2, 19, 34, cin), cin + cout)
    w, b = _w(cout, cin, 1), torch.randn(cout) * 0.1
    y, ys = pointwise(x, w, b)
    e = _rel(y, ref64(x, w, b))
    assert e <= 1e-5, e
    _check_ymax(y, ys)
    res = _act((2, 19, 34, cout), 7, relu=False)
    y, ys = pointwise(x, w, b, res=res, relu=False)
    e = _rel(y, ref64(x, w, b, res=res, relu=False))
    assert e <= 1e-5, e
    _check_ymax(y, ys)


# (C1, C2, Cout, stride of x2, output map): the four ResNet-50 stage entries (conv3 + downsample), at odd 608 x 1088 / 16, 32 sizes and the 512^2 sizes
TWO_SOURCE = [(64, 64, 256, 1, (38, 68)), (128, 256, 512, 2, (19, 34)), (256, 512, 1024, 2, (19, 34)), (512, 1024, 2048, 2, (16, 16)),
              (128, 256, 512, 2, (64, 64)), (512, 1024, 2048, 2, (19, 34))]


@pytest.mark.parametrize("c1,c2,cout,s2,hw", TWO_SOURCE)
def test_two_source_against_float64(c1, c2, cout, s2, hw):
    H, W = hw
    H2, W2 = (H, W) if s2 == 1 else (2 * H - H % 2, 2 * W)        # (odd H: an odd x2 height, (37 - 1) // 2 + 1 = 19)
    x1 = _act((2, H, W, c1), c1)
    x2 = _act((2, H2, W2, c2), c2, scale=3.0)                 # the larger source sets the shared scale
    w1, w2 = _w(cout, c1, 2, gain=0.2), _w(cout, c2, 3)
    b = torch.randn(cout) * 0.1
    y, ys = pointwise(x1, w1, b, x2=x2, w2=w2, s2=s2)
    y64 = ref64(x1, w1, b, x2=x2, w2=w2, s2=s2)
    e = _rel(y, y64)
    print(f"two-source {c1}+{c2}->{cout} s{s2} {hw}: max err / max ref {e:.3g}")
    assert e <= 1e-5, e
    _check_ymax(y, ys)
    # the per-element bound of DESIGN.md §11: |y - y64| <= c (u s + 2^-38 (xmax_n sum |W| + wmax sum |x|)), s = |x1| |W1| + |x2| |W2| + |b|, with
    # xmax_n the LARGER of the two sources' maxima of image n (their shared scale) and c the direct fp16-split class's R_CLASS
    s = (x1.double().cpu().abs().reshape(-1, c1) @ w1.double().abs().t() +
         x2[:, ::s2, ::s2].double().cpu().abs().reshape(-1, c2) @ w2.double().abs().t()).reshape(y64.shape) + b.double().abs()
    xm = torch.maximum(x1.abs().amax(dim=(1, 2, 3)), x2.abs().amax(dim=(1, 2, 3))).double().cpu().view(-1, 1, 1, 1)
    wc = torch.cat([w1, w2], 1).double()
    floor = rp.FLOOR * (xm * wc.abs().sum(1) + float(wc.abs().max()) *
                        (x1.double().cpu().abs().sum(-1, keepdim=True) + x2[:, ::s2, ::s2].double().cpu().abs().sum(-1, keepdim=True)))
    ratio = float(((y.double().cpu() - y64).abs() / (rp.U * s + floor)).max())
    print(f"    per-element ratio {ratio:.3g} (R_CLASS direct_split {rp.R_CLASS['direct_split']})")
    assert ratio <= rp.R_CLASS["direct_split"], ratio


def test_tile_shapes_give_the_same_bits():
    x1, x2 = _act((2, 19, 34, 256), 1), _act((2, 38, 68, 512), 2)
    w1, w2, b = _w(1024, 256, 3), _w(1024, 512, 4), torch.randn(1024) * 0.1
    base, _ = pointwise(x1, w1, b, x2=x2, w2=w2, s2=2)
    for t in (1, 2, 3):
        y, _ = pointwise(x1, w1, b, x2=x2, w2=w2, s2=2, algo=CNL_ALGO_FORCE + t)
        assert torch.equal(y, base), t


def test_outlier_in_one_image_and_shard_equals_full_batch():
    """Scales are per image: a 1e4 outlier in image 1 (of either source) leaves images 0 and 2 bit for bit what they are alone, and every image's
    result equals its one-image shard."""
    c1, c2, cout = 256, 512, 1024
    x1, x2 = _act((3, 19, 34, c1), 11), _act((3, 37, 68, c2), 12)
    x2[1, 5, 7, 3] = 1e4
    x1[1, 2, 2, 9] = -3e3
    w1, w2, b = _w(cout, c1, 5), _w(cout, c2, 6), torch.randn(cout) * 0.1
    full, ys = pointwise(x1, w1, b, x2=x2, w2=w2, s2=2)
    _check_ymax(full, ys)
    for n in range(3):
        one, _ = pointwise(x1[n:n + 1].contiguous(), w1, b, x2=x2[n:n + 1].contiguous(), w2=w2, s2=2)
        assert torch.equal(one, full[n:n + 1]), n
    calm = x2.clone()
    calm[1, 5, 7, 3] = 0.5
    ref, _ = pointwise(x1, w1, b, x2=calm, w2=w2, s2=2)
    assert torch.equal(ref[0], full[0]) and torch.equal(ref[2], full[2])
    e = _rel(full[1:2], ref64(x1[1:2], w1, b, x2=x2[1:2], w2=w2, s2=2))
    assert e <= 1e-5, e
    # single source, residual: the same per-image property
    r = _act((3, 19, 34, c1), 13, relu=False)
    ya, _ = pointwise(x1, _w(c1, c1, 7), torch.zeros(c1), res=r)
    yb, _ = pointwise(x1[2:].contiguous(), _w(c1, c1, 7), torch.zeros(c1), res=r[2:].contiguous())
    assert torch.equal(ya[2:], yb)


# ------------------------------------------------------------------------------------------------------------------- plans
def _model(cfg, seed=0, calib=(2, 3, 128, 128), **options):
    torch.manual_seed(0)
    model = cl.build_centernet(os.path.join(CONFIGS, cfg) if isinstance(cfg, str) else cfg)
    if "backbone.layer1.0.conv3.weight" in model.state_dict():
        sd = bottleneck_ref.synth_state_dict(model.state_dict(), seed=seed, calib_shape=calib)
    else:
        import ref_cpu
        sd = ref_cpu.synth_state_dict(model.state_dict(), seed=seed, calib_shape=calib)
    model.load_state_dict(sd)
    if options:
        model.set_kernel_options(**options)
    return model.cuda(), sd


def _plan(model, x):
    model(x)
    torch.cuda.synchronize()
    return model._engine.plan_for(x)


def test_plan_shape_two_source_launches_and_untouched_basic_block_plans():
    x = recipes.images(3, (2, 3, 128, 160)).cuda()
    model, _ = _model("resnet50_simple.yaml")
    plan = _plan(model, x)
    pw = plan.lib.cnl_pointwise_nhwc_f32
    two = [L for L in plan.launches if L.fn is pw and L.aux is not None]
    assert [L.what.split(" ")[0] for L in two] == [f"layer{i}.0.conv3+downsample" for i in range(1, 5)]
    assert not any("downsample" in L.what and L.fn is not pw for L in plan.launches)
    assert [L.aux[5] for L in two] == [1, 2, 2, 2]
    conv3 = [L for L in plan.launches if re.match(r"layer\d\.\d+\.conv3", L.what) and L.fn in (pw, plan.lib.cnl_conv2d_nhwc_f32)]
    assert len(conv3) == 16
    # the stop rule keeps every single-source 1x1 conv on the generic kernel in its split form (engine._POINTWISE_WINS is empty)
    assert all(L.fn is plan.lib.cnl_conv2d_nhwc_f32 and plan.lib.cnl_conv2d_kernel(ctypes.byref(L.args)) == 5
               for L in plan.launches if re.match(r"layer\d\.\d+\.(conv1|conv3) ", L.what + " ") and L.fn is not pw)
    for name in ("resnet34_simple.yaml", "resnet34_fpn.yaml"):
        m, _ = _model(name)
        p = _plan(m, x)
        assert not any(L.fn is p.lib.cnl_pointwise_nhwc_f32 for L in p.launches)
    m18 = cl.build_centernet({"model": {"backbone": {"name": "resnet18"}, "neck": {"name": "simple"}, "output_heads": {"heatmap": {"num_classes": 4}, "box_2d": {}}}})
    p = _plan(m18.cuda(), x)
    assert not any(L.fn is p.lib.cnl_pointwise_nhwc_f32 for L in p.launches)
    # the fp32 class keeps every 1x1 conv on the generic kernel (no split arithmetic anywhere)
    model.set_kernel_options(algo="f32")
    p = _plan(model, x)
    assert not any(L.fn is pw for L in p.launches)


def _pw_io(plan, L, x, at):
    p = L.args
    N = plan.N
    ins = {"x": at.nhwc(p.x, N, p.H_in, p.W_in, p.Cin, p.ldx), "xslot": at.slots(p.x_absmax, N), "xfull": plan.tensor(L.keep[0])}
    if p.residual:
        ins["res"] = at.nhwc(p.residual, N, p.H_in, p.W_in, p.Cout, p.ldr)
    if L.aux is not None:
        x2, h2, w2, c2, ldx2, s2, s2ptr = L.aux
        ins["x2"] = at.nhwc(x2, N, h2, w2, c2, ldx2)
        ins["x2slot"] = at.slots(s2ptr, N)
    outs = {"y": at.nhwc(p.y, N, p.H_in, p.W_in, p.Cout, p.ldy)}
    if p.y_absmax:
        outs["yslot"] = at.slots(p.y_absmax, N)
    return ins, outs


def _check_pw(chk, i, L, pre, post):
    """float64 check of one pointwise launch: z = x1 W1 (+ x2[::s, ::s] W2) + b (+ R), s = |x1| |W1| (+ ...) + |b| + |R|, the split floor from the
    larger of the two sources' maxima (one scale per image for both) — held to direct_split's R_CLASS and to 2 x the fp32 CPU conv's ratio."""
    p, layer = L.args, L.keep[3]
    chk._slots(i, L, pre, post)
    chk.forms.add("pointwise two-source" if L.aux is not None else "pointwise")
    W = layer.w[:, 0, 0, :].double().cpu()
    b = layer.b.double().cpu()
    k1 = p.Cin
    X = pre["x"].double()
    parts = [(X, W[:, :k1])]
    if L.aux is not None:
        s2 = L.aux[5]
        X2 = pre["x2"][:, ::s2, ::s2, :].double()
        parts.append((X2, W[:, k1:]))
        if not torch.equal(pre["x2slot"], rp._amax(pre["x2"])):
            chk.flag(i, L, f"x2_absmax slot {pre['x2slot'].tolist()} != max |x2| {rp._amax(pre['x2']).tolist()}")
    z = sum(t.reshape(-1, t.shape[-1]) @ w.t() for t, w in parts).reshape(*X.shape[:3], -1) + b
    s = sum(t.abs().reshape(-1, t.shape[-1]) @ w.abs().t() for t, w in parts).reshape(z.shape) + b.abs()
    xm = torch.stack([t.abs().amax(dim=(1, 2, 3)) for t, _ in parts]).amax(0).view(-1, 1, 1, 1)
    fl = rp.FLOOR * (xm * W.abs().sum(1) + W.abs().max() * sum(t.abs().sum(-1, keepdim=True) for t, _ in parts))
    if "res" in pre:
        z, s = z + pre["res"].double(), s + pre["res"].double().abs()
    y64 = z.clamp_min(0) if p.flags & CNL_RELU else z
    den = rp.U * s + fl
    r, where = rp._worst(post["y"], y64, den)
    # the yardsticks of the other direct launches (rp.Checker._conv): torch's CPU fp32 conv and the fp32 matrix-core kernel, both on the concatenated
    # input [x1 | x2[::s, ::s]] with the launch's fp32 weights [W3 | Wds] and summed bias
    Xc = torch.cat([pre["x"], pre["x2"][:, ::L.aux[5], ::L.aux[5], :]], -1) if L.aux is not None else pre["x"]
    R = pre.get("res")
    z32 = F.conv2d(rp._nchw(Xc), layer.w.permute(0, 3, 1, 2).cpu(), layer.b.cpu()).permute(0, 2, 3, 1)
    if R is not None:
        z32 = z32 + R
    y32 = z32.clamp_min(0) if p.flags & CNL_RELU else z32
    q = ConvParams()
    q.N, q.H_in, q.W_in, q.Cin, q.Cout = p.N, p.H_in, p.W_in, layer.cin, p.Cout
    q.KH = q.KW = q.stride = 1
    q.pad, q.flags = 0, p.flags
    yb = rp._f32_matrix_core(chk.lib, q, layer, Xc, R)
    ra, _ = rp._worst(y32, y64, den)
    rb, _ = rp._worst(yb, y64, den)
    chk.record(i, L, "direct_split", r, ra, rb, where=where)


def test_resnet50_plan_replays_launch_by_launch_against_float64(capsys):
    model, sd = _model("resnet50_fpn.yaml")
    x = rp.structured_images(2, 128, 160, 50).cuda()
    model._engine.forward(x, sigmoid=True)
    torch.cuda.synchronize()
    plan = next(iter(model._engine.plans.values()))
    want = OrderedDict((k, v.clone()) for k, v in plan.run(x).items())
    torch.cuda.synchronize()
    chk = rp.Checker(plan, "resnet50_fpn")
    pw = plan.lib.cnl_pointwise_nhwc_f32
    outs = OrderedDict()
    oh, ow = plan.out_hw
    for name, (p, c) in plan.out_params.items():
        t = torch.empty((plan.N, oh, ow, c), device=plan.device)
        p.y = t.data_ptr()
        outs[name] = t
    plan.absmax.zero_()
    at = rp._At([plan.arena, plan.absmax, x] + list(outs.values()))
    n_pw = 0
    for i, L in enumerate(plan.launches):
        ins, res = _pw_io(plan, L, x, at) if L.fn is pw else rp.launch_io(plan, L, x, at)
        torch.cuda.synchronize()
        pre = {k: v.cpu().clone() for k, v in ins.items()}
        _lib.check(plan.launch(L, x, _stream()), L.what)
        torch.cuda.synchronize()
        post = {k: v.cpu().clone() for k, v in res.items()}
        if L.fn is pw:
            _check_pw(chk, i, L, pre, post)
            n_pw += 1
        else:
            chk(i, L, pre, post)
    with capsys.disabled():
        print("\n" + chk.report())
    assert not chk.fail, chk.report()
    assert n_pw == 4 and "pointwise two-source" in chk.forms
    for k in want:
        assert torch.equal(outs[k].permute(0, 3, 1, 2), want[k]), k


def test_resnet50_launches_write_only_their_declared_outputs_and_arena_reuse_changes_no_byte(capsys):
    """The footprint and lock-step replays of tests/test_gpu_plan_replay.py on the bottleneck plan (the pointwise launches through _pw_io): every launch
    changes only its declared outputs, and the plan that reuses its arena gives the bits of the one that does not at every launch."""
    x = rp.structured_images(2, 128, 160, 50).cuda()
    pw = _lib.load().cnl_pointwise_nhwc_f32

    model, _ = _model("resnet50_fpn.yaml")
    rec = rp.footprint_and_lockstep(lambda reuse: (rp.plan_with(model, x, reuse_buffers=reuse), x, None), capsys, io=lambda plan, L, x_, at: _pw_io(plan, L, x_, at) if L.fn is pw else rp.launch_io(plan, L, x_, at))
    assert sum("conv3+downsample" in what for what, _, _ in rec) == 4


# ------------------------------------------------------------------------------------------------------------------- end to end
def _features(model, plan):
    nb, nh, nw, nc, nup = plan.neck_out
    neck = plan.tensor(nb)[..., :nc].permute(0, 3, 1, 2).cpu()
    if nup:
        neck = F.interpolate(neck, scale_factor=2, mode="nearest")
    heads = {name: plan.tensor(buf)[..., off:off + c].permute(0, 3, 1, 2).cpu() for name, (buf, ld, off, c, _, _, _) in plan.head_features.items()}
    return neck, heads


TRACK = {"model": {"task": "tracking", "backbone": {"name": "resnet50"},
                   "neck": {"name": "fpn", "upsample_channels": [256, 128, 64], "upsample_type": "nearest", "conv_type": "normal"},
                   "output_heads": {"heatmap": {"num_classes": 2, "init_bias": -2.19}, "box_2d": {"init_bias": 10},
                                    "reid": {"init_bias": 0, "max_track_ids": 800}}}}
RN101 = {"model": {"backbone": {"name": "resnet101"}, "neck": {"name": "simple"},
                   "output_heads": {"heatmap": {"num_classes": 80, "init_bias": -2.19}, "box_2d": {"init_bias": 10}}}}


@pytest.mark.parametrize("cfg,shape", [("resnet50_simple.yaml", (2, 3, 512, 512)), ("resnet50_fpn.yaml", (2, 3, 512, 512)),
                                       ("resnet101", (1, 3, 256, 256)), ("tracking_resnet50", (1, 3, 608, 1088))])
def test_end_to_end_against_cpu_oracle(cfg, shape):
    spec = {"resnet101": RN101, "tracking_resnet50": TRACK}.get(cfg, cfg)
    model, sd = _model(spec, reuse_buffers=False)
    x = recipes.images(4242, shape)
    out = model.get_encoded_outputs(x.cuda()) if hasattr(model, "get_encoded_outputs") else None
    torch.cuda.synchronize()
    plan = model._engine.plan_for(x.cuda(), sigmoid=False)
    neck, heads = _features(model, plan)
    ref, _, neck32, heads32 = bottleneck_ref.forward(sd, x, sigmoid=False, return_intermediates="heads")
    _, _, neck64, heads64 = bottleneck_ref.forward_float64(sd, x, sigmoid=False, return_intermediates="heads")
    errs = {"neck": _rel(neck, neck64), "cpu.neck": _rel(neck32, neck64)}
    for name in heads64:
        errs["head." + name] = _rel(heads[name], heads64[name])
        errs["cpu.head." + name] = _rel(heads32[name], heads64[name])
    outs = {k: v.cpu() for k, v in out.items()}
    ref64 = bottleneck_ref.forward_float64(sd, x, sigmoid=False)
    for name in ref:
        errs["out." + name] = float((outs[name].double() - ref64[name]).abs().max() / ref64[name].abs().max())
        errs["cpu.out." + name] = float((ref[name].double() - ref64[name]).abs().max() / ref64[name].abs().max())
    print(cfg, shape, errs)
    for k, e in errs.items():
        assert e <= 1e-4, (k, errs)                                           # the float64 feature gate (GPU and CPU fp32 alike)
    for name in ref:
        assert errs["out." + name] <= 1e-5, (name, errs)                     # every head, max-normalised, against the oracle in float64
        torch.testing.assert_close(outs[name], ref[name], rtol=1e-4, atol=1e-4)


def test_forward_uint8_and_torchscript_export_on_resnet50(tmp_path):
    model, _ = _model("resnet50_fpn.yaml")
    g = torch.Generator().manual_seed(17)
    u8 = torch.randint(0, 256, (2, 128, 160, 3), generator=g, dtype=torch.uint8).cuda()
    a = model(model.preprocess_uint8(u8))
    b = model.forward_uint8(u8)
    for ta, tb in zip(a, b):
        assert torch.equal(ta, tb)
    x = recipes.images(5, (2, 3, 128, 160)).cuda()
    ref = model(x)
    traced = cl.export_torchscript(model, save_path=str(tmp_path / "m.pt"), example_inputs=x)
    out = traced(x)
    assert len(out) == 2 and all(torch.equal(p, q) for p, q in zip(out, ref))
    loaded = torch.jit.load(str(tmp_path / "m.pt"))
    assert all(torch.equal(p, q) for p, q in zip(loaded(x), ref))


def test_shard_equals_full_batch_resnet50():
    model, _ = _model("resnet50_simple.yaml")
    x = recipes.images(9, (3, 3, 128, 128)).cuda()
    full = model(x)
    one = model(x[1:2].contiguous())
    for a, b in zip(full, one):
        assert torch.equal(a[1:2], b)
