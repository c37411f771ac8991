"""GPU: the launch plans the engine actually runs, replayed ONE LAUNCH AT A TIME, every launch recomputed in float64 on the CPU from the GPU's own input
bytes and the fp32 weights it was built from (layer.w, OHWI with BatchNorm folded; layer.b) — never from the transformed or split buffers, so errors do
not compound across launches and an error that stays inside one launch, one ragged tile, one image or one small-magnitude channel is not diluted by the
33 layers behind it (tests/test_gpu_e2e.py measures only max |err| / max |ref| at the neck and head outputs).

Per-element criterion of a conv-like launch (u = 2^-24):
    s     = conv(|X|~, |W|) + |b| + |R|          (R: the residual; with CNL_UPSAMPLE_OUT_ADD the conv part is upsampled first)
    floor = 2^-38 (xmax_n conv(1, |W|) + wmax conv(|X|, 1))      — split arithmetic only: include/centernet_gfx950.h, x_absmax: a value 2^-n below its
            image's maximum keeps min(22, 38 - n) significant bits, i.e. an absolute error of about 2^-38 xmax_n per operand element (the same for the
            weights under their power-of-two scale)
    ratio = |y_gpu - y64| / (u s + floor)
|X|~ is |X| for the direct kernels; the Winograd kernels' transforms mix the inputs of a tile, so |X|~ is |X| max-pooled over the input window that a
transform position mixes around an output's taps:
    F(2x2, 3x3) (winograd2 / 5 / 6) and F(2,3) along x (winograd9 / 10 / 11): outputs 2t, 2t+1 read the 4 x 4 (rows x 4 columns for the row kernels)
        patch starting at 2t - 1, i.e. at most one pixel beyond each 3 x 3 window: a 3 x 3 max-pool;
    F(4,3) along x (winograd13): the six columns 4t - 1 .. 4t + 4 enter every output of the four-pixel tile: 3 rows x 9 columns.
Each launch must satisfy max ratio <= 2 x the max ratio of the SAME launch computed (a) by torch's CPU fp32 conv and (b) by the fp32 matrix-core kernel
(cnl_conv2d_nhwc_f32, algo CNL_ALGO_F32, OHWI weights, no hints) on the same input — the yardstick KernelOptions' "auto" promises; the opt-in F(4,3) class
<= 6 x (its documented 2.4-4.6 x) — and max ratio <= R_CLASS[class], an absolute constant per arithmetic class measured on the MI355X (below).
Bit-exact launches (max-pool, nearest upsample, cnl_absmax_per_image_f32, unweighted fuse sums) must match bit for bit; the other elementwise launches are
held to their own R_CLASS.  The per-image max |x| hand-over is checked exactly: a slot a launch reads equals max |x| of each image of ITS input (or of
the documented superset it belongs to), a slot a launch fills equals max |y| of what it wrote."""
import ctypes
import hashlib
import os
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import recipes
import ref_cpu
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd._lib import (CNL_ALGO_F32, CNL_RELU, CNL_RELU6, CNL_SIGMOID, CNL_UPSAMPLE_IN, CNL_UPSAMPLE_OUT_ADD, CNL_W_SPLIT,
                                          ConvParams, DeconvParams)

pytestmark = pytest.mark.gpu
CONFIGS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "centernet-lightning_amd", "configs")
U = 2.0 ** -24
FLOOR = 2.0 ** -38
TINY = 64 * 2.0 ** -126     # results and products below FLT_MIN may be flushed to zero (the sigmoid of a logit below -87, a bilinear weight times a tiny
                            # activation): an absolute error of a few FLT_MIN per output, added to every denominator

# Largest per-launch max ratio allowed per arithmetic class (|y - y64| / (u s + floor), see the module docstring).  Measured on the MI355X over every launch
# of every plan below (the largest max ratio of any launch of the class in brackets); the bound leaves about 1.5 x headroom.
R_CLASS = {
    "direct_f32": 14.0,         # [9.21] conv_mfma.hip, fp32 matrix cores (the deformable conv's K = 9 Cin GEMM; its fp32 CPU conv: 9.21 too)
    "direct_split": 8.0,        # [5.06] conv_f16x2.hip (pre-split weights, split-K included)
    "subpixel_f32": 6.5,        # [4.03] cnl_conv3x3_up2_nhwc_f32 on the fp32 matrix cores
    "subpixel_split": 8.0,      # [not reached by these plans: the row-Winograd kernels take its layers] as direct_split
    "wino_f32": 4.5,            # [3.01] winograd2
    "wino_split": 3.0,          # [1.96] winograd5 / 6
    "row_wino": 6.5,            # [4.18] winograd9 / 10 / 11 (row-pair weights, folded out_conv included)
    "f43": 4.5,                 # [2.82] winograd13
    "stem_f32": 9.5,            # [6.09]
    "stem_split": 9.0,          # [5.92] fp32 and uint8 input, with and without the fused max-pool
    "fused_out_part": 5.5,      # [3.48] the partial sums a folded out_conv leaves in winograd9's epilogue
    "fused_out_reduce": 4.0,    # [2.42]
    "deconv": 8.0,              # [5.10]
    "depthwise": 4.5,           # [2.79]
    "deform_sample": 6.0,       # [3.73]
    "bilinear": 4.5,            # [2.85]
    "fuse_sum": 6.0,            # [3.81] weighted / bilinear fusion sums
}
YARDSTICK_FACTOR = {"f43": 6.0}             # every other conv class: 2.0
WINDOW = {"wino_f32": (3, 3), "wino_split": (3, 3), "row_wino": (3, 3), "f43": (3, 9)}
SPLIT_CLASSES = {"direct_split", "subpixel_split", "wino_split", "row_wino", "f43", "stem_split"}


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _amax(t):
    """max |t| per image (dim 0) of a CPU tensor."""
    return t.abs().reshape(t.shape[0], -1).amax(dim=1)


# ---------------------------------------------------------------------------------------------------------------------------- structured inputs
def structured_images(N, H, W, seed):
    """Letterboxed frames: constant bands top and bottom (an eighth of the height each), a dark region (a quarter of the map at 10^-4 of the scene), and
    — with two or more images — image 1 at 10^-3 of image 0's magnitude.  Values in the range of a normalised 8-bit image."""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(N, 3, H, W, generator=g) * 4.2 - 2.1
    band = H // 8
    x[:, :, :band] = 0.35
    x[:, :, H - band:] = 0.35
    x[:, :, H // 4:H // 2, W // 2:W // 2 + W // 4] *= 1e-4
    if N > 1:
        x[1] *= 1e-3
    return x


def dark_region_images(N, H, W, seed):
    """The sensitivity tests' input: the images of the end-to-end tests (recipes.images, uniform in [0, 1]) with the dark region of structured_images —
    well conditioned end to end (the outputs stay within 1e-4 of the CPU oracle), unlike the letterboxed frames, whose box_2d moves by 3e-4 with fp32
    rounding alone."""
    x = recipes.images(seed, (N, 3, H, W))
    x[:, :, H // 4:H // 2, W // 2:W // 2 + W // 4] *= 1e-4
    return x


def structured_frames(N, H, W, seed):
    """uint8 frames [N, H, W, 3] for the tracking model's normalising stem: letterbox bands of the usual grey (114), a dark region at the
    normalisation mean (values within a pixel of it: |x| <= 0.02 after A.Normalize, 10^-2 of the scene), noise elsewhere."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    band = H // 8
    x[:, :band] = 114
    x[:, H - band:] = 114
    mean = torch.tensor([0.485, 0.456, 0.406]) * 255
    dark = (mean.round() + torch.randint(-1, 2, (N, H // 4, W // 4, 3), generator=g)).clamp(0, 255).to(torch.uint8)
    x[:, H // 4:H // 2, W // 2:W // 2 + W // 4] = dark
    return x


# ---------------------------------------------------------------------------------------------------------------------------- plans
DET = {"task": "detection", "backbone": {"name": "resnet34", "pretrained": False},
       "output_heads": {"heatmap": {"num_classes": 5, "init_bias": -2.19}, "box_2d": {"init_bias": 10}}}


def _neck_cfg(neck):
    neck = dict(neck)
    if neck["name"] in ("simple", "fpn"):
        neck["upsample_channels"] = [256, 128, 64]
    return {**DET, "neck": neck}


# name -> (config, N, H, W, kernel options, mutate the state dict, uint8 frames)
PLANS = OrderedDict([
    ("C1", ("resnet34_simple.yaml", 2, 512, 512, {}, None, False)),
    ("C2", ("resnet34_fpn.yaml", 2, 512, 512, {}, None, False)),
    ("C4", ("tracking_resnet34_fpn.yaml", 2, 608, 1088, {}, None, True)),
    ("latency_split_small", ("resnet34_simple.yaml", 1, 512, 512, {"latency": True, "split_small": True}, None, False)),
    ("f43", ("resnet34_simple.yaml", 2, 256, 512, {"f43": True}, None, False)),     # (F(4,3) takes maps >= 128 pixels wide: the head blocks at 64 x 128)
    ("alternate_forms", ("resnet34_simple.yaml", 2, 256, 256, {"stem_fused_pool": False, "presplit_weights": False, "up_rows": False, "up2": True},
                         None, False)),
    ("f32", ("resnet34_simple.yaml", 2, 256, 256, {"algo": "f32"}, None, False)),
    ("C2_trained_like", ("resnet34_fpn.yaml", 2, 256, 256, {}, recipes._trained_checkpoint_like, False)),
    # neck options (tests/test_gpu_neck_options.py NECKS), together every non-conv launch kind: deconv K = 2 / 3 / 4, deformable v1 / v2, separable,
    # bilinear, weighted fusion, IDA, BiFPN
    ("neck_simple_deconv4_separable", ({"name": "simple", "upsample_type": "conv_transpose", "deconv_kernel": 4, "conv_type": "separable"},
                                       2, 96, 128, {}, None, False)),
    ("neck_fpn_deconv2_separable", ({"name": "fpn", "upsample_type": "conv_transpose", "deconv_kernel": 2, "conv_type": "separable"},
                                    2, 96, 128, {}, None, False)),
    ("neck_fpn_deformable", ({"name": "fpn", "upsample_type": "nearest", "conv_type": "deformable"}, 2, 96, 128, {}, None, False)),
    ("neck_simple_deformable_v1_bilinear", ({"name": "simple", "upsample_type": "bilinear", "conv_type": "deformable", "version": 1},
                                            2, 96, 128, {}, None, False)),
    ("neck_fpn_deconv_weighted", ({"name": "fpn", "upsample_type": "conv_transpose", "weighted_fusion": True}, 2, 96, 128, {}, None, False)),
    ("neck_ida_bilinear_weighted", ({"name": "ida", "upsample_type": "bilinear", "weighted_fusion": True}, 2, 96, 128, {}, None, False)),
    ("neck_bifpn_nearest", ({"name": "bifpn", "num_channels": 64, "num_layers": 2}, 2, 96, 128, {}, None, False)),
])


SMALL_PLANS = {"C1_256": ("resnet34_simple.yaml", 2, 256, 256, {}, None, False),        # the sensitivity tests' plan
               "C2_256": ("resnet34_fpn.yaml", 2, 256, 256, {}, None, False),           # (with the two below: the footprint / lock-step replays)
               "C4_96x160": ("tracking_resnet34_fpn.yaml", 2, 96, 160, {}, None, True)}
# the plans small enough for a device-side clone-and-compare around every launch (not the 512 x 512 or 608 x 1088 ones)
FOOTPRINT_PLANS = list(SMALL_PLANS) + ["neck_simple_deconv4_separable", "neck_fpn_deconv2_separable", "neck_fpn_deformable", "neck_simple_deformable_v1_bilinear",
                                       "neck_fpn_deconv_weighted", "neck_ida_bilinear_weighted", "neck_bifpn_nearest"]


def build_plan(name, spec=None):
    """-> (model, sd, plan, x, norm): the model of PLANS[name] with synthetic weights, its structured input, and the plan a forward of that input uses.
    spec: a tuple like the PLANS entries, for a variant of an entry at another batch or frame size (tests/test_gpu_nonfinite.py)."""
    cfg, N, H, W, opts, mutate, u8 = spec if spec is not None else PLANS[name] if name in PLANS else SMALL_PLANS[name]
    torch.manual_seed(0)
    if isinstance(cfg, str):
        model = cl.build_centernet(os.path.join(CONFIGS, cfg))
        sd = ref_cpu.synth_state_dict(model.state_dict(), seed=0, calib_shape=(2, 3, 128, 128))
    else:
        model = cl.build_centernet(_neck_cfg(cfg))
        ups = cfg.get("upsample_type", "nearest")
        sd = ref_cpu.synth_state_dict(model.state_dict(), seed=1, calib_shape=(2, 3, 128, 128), upsample_type=ups)
        if cfg.get("weighted_fusion"):                           # (as test_model_with_neck_option_matches_cpu_oracle: fusion weights that matter)
            keys = sorted(k for k in sd if k.endswith(".weights"))
            sd[keys[1]][0] = -0.3
            for i, k in enumerate(keys[2:]):
                sd[k] = torch.rand(sd[k].shape, generator=torch.Generator().manual_seed(i)) + 0.25
    if mutate is not None:
        mutate(sd)
    model.load_state_dict(sd)
    if opts:
        model.set_kernel_options(**opts)
    model = model.cuda()
    seed = sum(map(ord, name))
    if u8:
        x = structured_frames(N, H, W, seed).cuda()
        norm = model._norm_constants(model.IMAGENET_MEAN, model.IMAGENET_STD)
        model._engine.forward_u8(x, norm[0], norm[1], sigmoid=True)
    else:
        x = (structured_images(N, H, W, seed) if name in PLANS else dark_region_images(N, H, W, seed)).cuda()
        norm = None
        model._engine.forward(x, sigmoid=True)           # (what model(x) runs: the heatmap's sigmoid epilogue included)
    torch.cuda.synchronize()
    assert len(model._engine.plans) == 1
    plan = next(iter(model._engine.plans.values()))
    return model, sd, plan, x, norm


# ---------------------------------------------------------------------------------------------------------------------------- the stepper
class _At:
    """Device views at raw pointers inside the tensors a plan's launches address (its arena, the outputs of this call, the absmax slots, the input)."""

    def __init__(self, tensors):
        self.tensors = [t for t in tensors if t is not None]

    def __call__(self, ptr, shape, strides):
        for t in self.tensors:
            b, es = t.data_ptr(), t.element_size()
            if b <= ptr < b + t.numel() * es:
                assert (ptr - b) % es == 0
                return t.as_strided(shape, strides, t.storage_offset() + (ptr - b) // es)      # (as_strided refuses a view beyond the storage)
        raise AssertionError(f"pointer {ptr:#x} is in none of the plan's tensors")

    def nhwc(self, ptr, n, h, w, c, ld):
        return self(ptr, (n, h, w, c), (h * w * ld, w * ld, ld, 1))

    def slots(self, ptr, n):
        return self(ptr, (n,), (_lib.absmax_stride(),))


def _out_hw(lib, p):
    ho, wo = ctypes.c_int32(), ctypes.c_int32()
    _lib.check(lib.cnl_conv2d_out_hw(ctypes.byref(p), ctypes.byref(ho), ctypes.byref(wo)))
    up = 2 if p.flags & CNL_UPSAMPLE_OUT_ADD else 1
    return ho.value * up, wo.value * up


def launch_io(plan, L, x, at):
    """-> (inputs, outputs): the device views launch L reads and writes (outputs are read back after it ran)."""
    lib, N = plan.lib, plan.N
    ins, outs = {}, {}
    if L.fn == "stem":
        ins["x"] = x
        outs["y"] = plan.tensor(plan.stem_out)
        if plan.stem_absmax:
            outs["yslot"] = at.slots(plan.stem_absmax, N)
    elif L.fn == "maxpool":
        ins["x"], outs["y"] = plan.tensor(L.args[0]), plan.tensor(L.args[1])
    elif isinstance(L.args, ConvParams):
        p = L.args
        ho, wo = _out_hw(lib, p)
        ins["x"] = at.nhwc(p.x, N, p.H_in, p.W_in, p.Cin, p.ldx)
        if p.residual:
            ins["res"] = at.nhwc(p.residual, N, ho, wo, p.Cout, p.ldr)
        if p.x_absmax:
            ins["xslot"] = at.slots(p.x_absmax, N)
            ins["xfull"] = plan.tensor(L.keep[0])
        outs["y"] = at.nhwc(p.y, N, ho, wo, p.Cout, p.ldy)
        if p.y_absmax:
            outs["yslot"] = at.slots(p.y_absmax, N)
        if p.splitk > 1 and p.splitk_scratch:                    # the partial sums of a split reduction: scratch this launch owns
            outs["scratch"] = at(p.splitk_scratch, (lib.cnl_conv2d_splitk_scratch_bytes(ctypes.byref(p)) // (4 * p.Cout), p.Cout), (p.Cout, 1))
        if p.fuse_w:
            outs["part"] = at(p.fuse_part, ((p.Cout + 63) // 64 * 2, N * ho * wo, 4), (N * ho * wo * 4, 4, 1))
    elif isinstance(L.args, DeconvParams):
        p = L.args
        ins["x"] = at.nhwc(p.x, N, p.H_in, p.W_in, p.Cin, p.ldx)
        if p.residual:
            ins["res"] = at.nhwc(p.residual, N, 2 * p.H_in, 2 * p.W_in, p.Cout, p.ldr)
        outs["y"] = at.nhwc(p.y, N, 2 * p.H_in, 2 * p.W_in, p.Cout, p.ldy)
    elif L.fn is lib.cnl_absmax_per_image_f32:
        xp, n, pix, c, ld, out = L.args
        ins["x"] = at(xp, (n, pix, c), (pix * ld, ld, 1))
        outs["slot"] = at.slots(out, n)
    elif L.fn is lib.cnl_fused_out_reduce_f32:
        part, nb, M, c2, _, y, ldy, _ = L.args
        ins["part"] = at(part, (nb, M, 4), (M * 4, 4, 1))
        outs["y"] = at(y, (M, c2), (ldy, 1))
    elif L.fn is lib.cnl_depthwise3x3_nhwc_f32:
        xp, _, _, y, n, h, w, c, ldx, ldy, _ = L.args
        ins["x"], outs["y"] = at.nhwc(xp, n, h, w, c, ldx), at.nhwc(y, n, h, w, c, ldy)
    elif L.fn is lib.cnl_deform_sample_nhwc_f32:
        xp, om, col, n, h, w, c, ldx, no, k, _ = L.args
        ins["x"], ins["om"] = at.nhwc(xp, n, h, w, c, ldx), at.nhwc(om, n, h, w, no, no)
        outs["y"] = at.nhwc(col, n, h, w, k * k * c, k * k * c)
    elif L.fn is lib.cnl_upsample2x_nhwc_f32:
        xp, r, y, n, h, w, c, ldx, ldr, ldy, _ = L.args
        ins["x"] = at.nhwc(xp, n, h, w, c, ldx)
        if r:
            ins["res"] = at.nhwc(r, n, 2 * h, 2 * w, c, ldr)
        outs["y"] = at.nhwc(y, n, 2 * h, 2 * w, c, ldy)
    elif L.fn is lib.cnl_fuse_sum_nhwc_f32:
        a, b, last, y, n, h, w, c, ld0, ld1, ldl, ldy = L.args[:12]
        mode = L.args[16]
        lh, lw = {0: (h // 2, w // 2), 1: (h // 2, w // 2), 2: (2 * h, 2 * w), 3: (h, w)}[mode]
        ins["in0"], ins["last"] = at.nhwc(a, n, h, w, c, ld0), at.nhwc(last, n, lh, lw, c, ldl)
        if b:
            ins["in1"] = at.nhwc(b, n, h, w, c, ld1)
        outs["y"] = at.nhwc(y, n, h, w, c, ldy)
    else:
        raise AssertionError(f"launch {L.what!r}: unknown launch kind {L.fn!r} — the replay has no checker for it")
    return ins, outs


class Footprint:
    """"Declared outputs only": device clones of everything a plan's launches may write (its arena, its absmax array, the output tensors of this call)
    taken before a launch; after it, every int32 word that changed must lie inside the views launch_io declares as the launch's outputs — y, the
    absmax slots it fills, splitk_scratch, fuse_part.  A store past a ragged edge, into a padding channel or into a neighbour's buffer shows up at the
    launch that made it, although no later launch of the replay would ever notice (each is recomputed from its own input bytes)."""

    def __init__(self, plan, tensors):
        self.plan = plan
        self.tensors = OrderedDict((k, t) for k, t in tensors.items() if t is not None)
        self.saved = None

    def arm(self):
        self.saved = {k: t.detach().clone() for k, t in self.tensors.items()}

    def _where(self, name, word):
        if name == "arena":
            for k, b in enumerate(self.plan.buffers):
                if b.offset is not None and b.offset // 4 <= word < (b.offset + b.nbytes) // 4:
                    e, idx = word - b.offset // 4, []
                    for d in reversed(b.shape):
                        e, r = divmod(e, d)
                        idx.append(r)
                    return f"arena word {word}: buffer #{k} {tuple(b.shape)} at {tuple(reversed(idx))}" + (" (+ wrapped: in the buffer's 256-byte padding)" if e else "")
            return f"arena word {word}: in no buffer of the plan"
        t = self.tensors[name]
        return f"{name} at {tuple(int(v) for v in torch.unravel_index(torch.tensor(word), t.shape))}"

    def verify(self, outs):
        """-> None, or a description of the first word that changed outside the declared outputs `outs` (device views)."""
        for name, t in self.tensors.items():
            changed = t.reshape(-1).view(torch.int32) != self.saved[name].reshape(-1).view(torch.int32)
            if not bool(changed.any()):
                continue
            lo, hi = t.data_ptr(), t.data_ptr() + t.numel() * 4
            for v in outs.values():
                if lo <= v.data_ptr() < hi:
                    assert v.dtype == torch.float32 and (v.data_ptr() - lo) % 4 == 0
                    changed.as_strided(v.shape, v.stride(), (v.data_ptr() - lo) // 4).fill_(False)
            n = int(changed.sum())
            if n:
                first = int(torch.nonzero(changed)[0])
                return f"{n} word(s) changed outside the declared outputs {sorted(outs)}; first: {self._where(name, first)}"
        return None


def replay(plan, x, norm=None, check=None, before=None, after=None, stop=None, footprint=False, violations=None, io=None):
    """Plan.run one launch at a time (engine.py Plan.run: fresh output tensors patched into out_params, absmax slots zeroed, plan.launch per launch).
    Before a launch its inputs are copied to the CPU, after it (and a synchronisation) its outputs; check(i, L, pre, post) sees both — so arena reuse
    and in-place writes of the default plans need no special handling.  before / after(i, L, ins, outs) may edit the device views (sensitivity
    tests).  footprint=True: the words a launch (and its `after` hook) changes must lie inside its declared outputs (class Footprint); an offender
    is appended to `violations` as (launch index, what, description), or raised when no list is given.  io: launch_io, or a function with its
    signature that also knows launch kinds launch_io does not.  Returns the outputs as Plan.run does."""
    io = io or launch_io
    outs = OrderedDict()
    oh, ow = plan.out_hw
    for name, (p, c) in plan.out_params.items():
        t = torch.empty((plan.N, oh, ow, c), device=plan.device, dtype=torch.float32)
        p.y = t.data_ptr()
        outs[name] = t
    plan._norm = norm
    if plan.absmax is not None:
        plan.absmax.zero_()
    at = _At([plan.arena, plan.absmax, x] + list(outs.values()))
    stream = _stream()
    fp = Footprint(plan, OrderedDict([("arena", plan.arena), ("absmax", plan.absmax)] + [(f"output {k}", v) for k, v in outs.items()])) if footprint else None
    for i, L in enumerate(plan.launches):
        ins, res = io(plan, L, x, at)
        if before is not None:
            before(i, L, ins, res)
        torch.cuda.synchronize()
        pre = {k: v.cpu().clone() for k, v in ins.items()} if check is not None else None
        if fp is not None:
            fp.arm()
        _lib.check(plan.launch(L, x, stream), L.what)
        torch.cuda.synchronize()
        if after is not None:
            after(i, L, ins, res)
            torch.cuda.synchronize()
        if fp is not None:
            why = fp.verify(res)
            if why is not None:
                if violations is None:
                    raise AssertionError(f"launch {i} {L.what}: {why}")
                violations.append((i, L.what, why))
        if check is not None:
            check(i, L, pre, {k: v.cpu().clone() for k, v in res.items()})
        if stop is not None and i == stop:
            return None
    return OrderedDict((k, v.permute(0, 3, 1, 2)) for k, v in outs.items())


# ---------------------------------------------------------------------------------------------------------------------------- float64 references
def conv_class(lib, L):
    """-> (arithmetic class, coverage form) of a conv launch."""
    p = L.args
    if L.fn is lib.cnl_conv2d_nhwc_f32:
        k = lib.cnl_conv2d_kernel(ctypes.byref(p))
        if k != 5:
            return "direct_f32", "direct fp32"
        if p.splitk > 1:
            return "direct_split", "split-K"
        return "direct_split", "direct fp16-split" + (", pre-split weights" if p.flags & CNL_W_SPLIT else "")
    if L.fn is lib.cnl_conv3x3_up2_nhwc_f32:
        return ("subpixel_split", "sub-pixel phases fp16-split") if lib.cnl_conv3x3_up2_kernel(ctypes.byref(p)) == 5 else ("subpixel_f32", "sub-pixel phases fp32")
    if L.fn is lib.cnl_conv3x3_winograd_f32:
        v = lib.cnl_conv3x3_winograd_variant(ctypes.byref(p))
        form = f"winograd{v}" + (" + folded out_conv" if p.fuse_w else "") + (" + row-pair weights" if p.w_up and not p.fuse_w else "")
        return {2: "wino_f32", 5: "wino_split", 6: "wino_split", 9: "row_wino", 10: "row_wino", 11: "row_wino", 13: "f43"}[v], form
    raise AssertionError(L.what)


def _conv_parts(X, W, b, stride, pad, flags, R, window, split):
    """float64 pre-activation z, the condition scale s and the split floor of one conv (NCHW, one or more images)."""
    if flags & CNL_UPSAMPLE_IN:
        X = F.interpolate(X, scale_factor=2, mode="nearest")
    z = F.conv2d(X, W, b, stride=stride, padding=pad)
    A = X.abs()
    if window is not None:
        A = F.max_pool2d(A, window, 1, (window[0] // 2, window[1] // 2))
    s = F.conv2d(A, W.abs(), b.abs(), stride=stride, padding=pad)
    fl = torch.zeros_like(s[:, :1])
    if split:
        kh, kw = W.shape[2:]
        w1 = F.conv2d(torch.ones_like(X[:1, :1]), W.abs().sum(1, keepdim=True), None, stride=stride, padding=pad)
        x1 = F.conv2d(X.abs().sum(1, keepdim=True), torch.ones(1, 1, kh, kw, dtype=X.dtype), None, stride=stride, padding=pad)
        xmax = X.abs().reshape(X.shape[0], -1).amax(1).view(-1, 1, 1, 1)
        fl = FLOOR * (xmax * w1 + W.abs().max() * x1)
    if flags & CNL_UPSAMPLE_OUT_ADD:
        up = lambda t: F.interpolate(t, scale_factor=2, mode="nearest")
        z, s, fl = up(z) + R, up(s) + R.abs(), up(fl)
    elif R is not None:
        z, s = z + R, s + R.abs()
    return z, s, fl


def _act(z, flags):
    if flags & CNL_RELU:
        z = z.clamp_min(0)
    if flags & CNL_RELU6:
        z = z.clamp(0, 6)
    if flags & CNL_SIGMOID:
        z = torch.sigmoid(z)
    return z


def _den(z, y64, s, fl, flags):
    if flags & CNL_SIGMOID:                      # sigmoid' <= 1/4 carries the conv's error; the epilogue's exp / division add a few ulp of y
        d = y64 * (1 - y64)
        return (U * s + fl) * d + U * y64.abs()
    return U * s + fl


def _ratio(y, y64, den):
    return (y.double() - y64).abs() / (den + TINY)


def _worst(y, y64, den):
    """-> (max ratio, where / what at the worst element) of one output."""
    r = _ratio(y, y64, den)
    j = int(r.reshape(-1).argmax())
    at = tuple(int(v) for v in torch.unravel_index(torch.tensor(j), r.shape))
    return float(r.reshape(-1)[j]), f"at {at}: gpu {float(y.reshape(-1)[j]):.9g}, float64 {float(y64.reshape(-1)[j]):.9g}, u s + floor {float(den.reshape(-1)[j]):.3g}"


def _f32_matrix_core(lib, p, layer, X, R):
    """The same launch on the fp32 matrix cores: cnl_conv2d_nhwc_f32 with CNL_ALGO_F32, the layer's fp32 OHWI weights, no hints, no fuse_w / w_up /
    CNL_W_SPLIT, on a device copy of the launch's input bytes; -> NHWC CPU."""
    q = ConvParams()
    xd = X.contiguous().cuda()
    rd = R.contiguous().cuda() if R is not None else None
    q.x, q.w, q.bias = xd.data_ptr(), layer.w.data_ptr(), layer.b.data_ptr()
    q.residual = rd.data_ptr() if rd is not None else None
    q.N, q.H_in, q.W_in, q.Cin, q.Cout = p.N, p.H_in, p.W_in, p.Cin, p.Cout
    q.KH, q.KW, q.stride, q.pad = p.KH, p.KW, p.stride, p.pad
    q.flags, q.algo = p.flags & ~CNL_W_SPLIT, CNL_ALGO_F32
    ho, wo = _out_hw(lib, q)
    y = torch.full((p.N, ho, wo, p.Cout), float("nan"), device="cuda")
    q.y, q.ldx, q.ldy, q.ldr = y.data_ptr(), p.Cin, p.Cout, p.Cout
    assert lib.cnl_conv2d_kernel(ctypes.byref(q)) == 2
    _lib.check(lib.cnl_conv2d_nhwc_f32(ctypes.byref(q), _stream()), "fp32 yardstick")
    torch.cuda.synchronize()
    return y.cpu()


def _stem_f32_matrix_core(lib, plan, xf):
    xd = xf.contiguous().cuda()
    N, _, H, W = xf.shape
    y = torch.full((N, (H - 1) // 2 + 1, (W - 1) // 2 + 1, 64), float("nan"), device="cuda")
    _lib.check(lib.cnl_stem_conv7x7_f32(xd.data_ptr(), 3 * H * W, H * W, W, 1, plan._wt_stem_packed.data_ptr(), plan._wt_stem.b.data_ptr(), y.data_ptr(),
                                        None, N, H, W, CNL_ALGO_F32, _stream()), "fp32 stem yardstick")
    torch.cuda.synchronize()
    return y.cpu()


class Checker:
    """Per-launch checks of one replay: failures are collected (and printed with the per-class table) rather than raised at the first one."""

    def __init__(self, plan, name, norm=None, quiet=False):
        self.plan, self.lib, self.name, self.norm = plan, plan.lib, name, norm
        self.fail = []              # (launch index, what, reason)
        self.stats = {}             # class -> [max ratio, max fp32-CPU ratio, max fp32-matrix-core ratio, launches]
        self.forms = set()
        self.launch_ratio = {}      # launch index -> max ratio
        self.quiet = quiet
        self.out_of = {}            # fuse_part buffer -> the folded out_conv layer
        for L in plan.launches:
            if L.fn is plan.lib.cnl_fused_out_reduce_f32:
                self.out_of[id(L.keep[0])] = L.keep[1]

    def flag(self, i, L, why):
        self.fail.append((i, L.what, why))

    def record(self, i, L, cls, r, ra=None, rb=None, where=""):
        st = self.stats.setdefault(cls, [0.0, 0.0, 0.0, 0])
        st[0] = max(st[0], r)
        st[1] = max(st[1], ra or 0.0)
        st[2] = max(st[2], rb or 0.0)
        st[3] += 1
        self.launch_ratio[i] = max(self.launch_ratio.get(i, 0.0), r)
        if not r <= R_CLASS[cls]:
            self.flag(i, L, f"{cls}: max ratio {r:.3g} > R_CLASS {R_CLASS[cls]} {where}")
        if ra is not None:
            f = YARDSTICK_FACTOR.get(cls, 2.0)
            if not r <= f * max(ra, rb):
                self.flag(i, L, f"{cls}: max ratio {r:.3g} > {f} x the fp32 yardsticks (CPU {ra:.3g}, matrix core {rb:.3g}) {where}")

    def __call__(self, i, L, pre, post):
        lib = self.lib
        self._slots(i, L, pre, post)
        if L.fn == "stem":
            self._stem(i, L, pre, post)
        elif L.fn == "maxpool":
            want = _nchw(F.max_pool2d(_nchw(pre["x"]), 3, 2, 1).permute(0, 2, 3, 1))
            if not torch.equal(_nchw(post["y"]), want):
                self.flag(i, L, "max-pool not bit-exact")
        elif isinstance(L.args, ConvParams):
            self._conv(i, L, pre, post)
        elif isinstance(L.args, DeconvParams):
            self._deconv(i, L, pre, post)
        elif L.fn is lib.cnl_absmax_per_image_f32:
            pass                                             # (_slots: bit-exact against the input it read)
        elif L.fn is lib.cnl_fused_out_reduce_f32:
            self._reduce(i, L, pre, post)
        elif L.fn is lib.cnl_depthwise3x3_nhwc_f32:
            layer = L.keep[2]
            X = _nchw(pre["x"]).double()
            C = X.shape[1]
            Wd = layer.dw_w.permute(2, 0, 1).unsqueeze(1).double().cpu()
            bd = layer.dw_b.double().cpu()
            z = F.conv2d(X, Wd, bd, padding=1, groups=C)
            s = F.conv2d(X.abs(), Wd.abs(), bd.abs(), padding=1, groups=C)
            flags = L.args[10]
            y64 = _act(z, flags)
            r, where = _worst(_nchw(post["y"]), y64, U * s)
            self.record(i, L, "depthwise", r, where=where)
        elif L.fn is lib.cnl_deform_sample_nhwc_f32:
            self._deform(i, L, pre, post)
        elif L.fn is lib.cnl_upsample2x_nhwc_f32:
            X, mode = _nchw(pre["x"]), L.args[10]
            R = _nchw(pre["res"]) if "res" in pre else None
            if mode == 0:
                want = F.interpolate(X, scale_factor=2, mode="nearest")
                if R is not None:
                    want = R + want
                if not torch.equal(_nchw(post["y"]), want):
                    self.flag(i, L, "nearest upsample not bit-exact")
            else:
                z = F.interpolate(X.double(), scale_factor=2, mode="bilinear", align_corners=False)
                s = F.interpolate(X.double().abs(), scale_factor=2, mode="bilinear", align_corners=False)
                if R is not None:
                    z, s = z + R.double(), s + R.double().abs()
                r, where = _worst(_nchw(post["y"]), z, U * s)
                self.record(i, L, "bilinear", r, where=where)
        elif L.fn is lib.cnl_fuse_sum_nhwc_f32:
            self._fuse_sum(i, L, pre, post)
        else:
            raise AssertionError(f"launch {L.what!r}: no checker")

    # -- the per-image max |x| hand-over, exactly
    def _slots(self, i, L, pre, post):
        if "xslot" in pre:
            own = _amax(pre["x"])
            slot = pre["xslot"]
            if pre["xfull"].shape[-1] != pre["x"].shape[-1] and not torch.equal(slot, own):
                # documented superset: a head's first block runs fused along Cout with the other heads' (engine.py _build); the consumer of ONE head's channel
                # slice reads the slot its producer filled for the whole buffer (include/centernet_gfx950.h: "a maximum over a superset of the consumer's channels
                # is a valid, slightly conservative bound")
                full = _amax(pre["xfull"])
                if not (torch.equal(slot, full) and bool((slot >= own).all())):
                    self.flag(i, L, f"x_absmax slot {slot.tolist()} != max |x| of the fused buffer {full.tolist()} (own slice {own.tolist()})")
            elif not torch.equal(slot, own):
                self.flag(i, L, f"x_absmax slot {slot.tolist()} != max |x| of its input {own.tolist()}")
        if "yslot" in post and not torch.equal(post["yslot"], _amax(post["y"])):
            self.flag(i, L, f"y_absmax slot {post['yslot'].tolist()} != max |y| {_amax(post['y']).tolist()}")
        if "slot" in post and not torch.equal(post["slot"], _amax(pre["x"])):
            self.flag(i, L, f"absmax pass {post['slot'].tolist()} != max |x| {_amax(pre['x']).tolist()}")

    def _conv(self, i, L, pre, post):
        lib, p = self.lib, L.args
        layer = L.keep[3]
        cls, form = conv_class(lib, L)
        self.forms.add(form)
        W32, b32 = layer.w.permute(0, 3, 1, 2).cpu(), layer.b.cpu()
        W64, b64 = W32.double(), b32.double()
        X32 = _nchw(pre["x"])
        R32 = _nchw(pre["res"]) if "res" in pre else None
        y = _nchw(post["y"])
        ya = F.conv2d(F.interpolate(X32, scale_factor=2, mode="nearest") if p.flags & CNL_UPSAMPLE_IN else X32, W32, b32, stride=p.stride, padding=p.pad)
        if p.flags & CNL_UPSAMPLE_OUT_ADD:
            ya = F.interpolate(ya, scale_factor=2, mode="nearest") + R32
        elif R32 is not None:
            ya = ya + R32
        ya = _act(ya, p.flags)
        yb = _nchw(_f32_matrix_core(lib, p, layer, pre["x"], pre.get("res")))
        r = ra = rb = 0.0
        where = ""
        for n in range(p.N):                                  # one image at a time: the C4 head blocks are 500 MB per float64 tensor
            R = R32[n:n + 1].double() if R32 is not None else None
            z, s, fl = _conv_parts(X32[n:n + 1].double(), W64, b64, p.stride, p.pad, p.flags, R, WINDOW.get(cls), cls in SPLIT_CLASSES)
            y64 = _act(z, p.flags)
            den = _den(z, y64, s, fl, p.flags)
            rn, wn = _worst(y[n:n + 1], y64, den)
            if rn >= r:
                r, where = rn, f"image {n} {wn}"
            ra = max(ra, float(_ratio(ya[n:n + 1], y64, den).max()))
            rb = max(rb, float(_ratio(yb[n:n + 1], y64, den).max()))
        self.record(i, L, cls, r, ra, rb, where)
        if "part" in post:
            self._part(i, L, post)

    def _part(self, i, L, post):
        """The folded out_conv's partial sums (winograd9 epilogue): part[b][pixel][c] = sum over the 32 channels of block b of y[pixel][co] * w[c][co],
        from the launch's own fp32 y."""
        p = L.args
        outl = self.out_of[id(L.keep[4])]
        c2 = outl.cout
        nb = post["part"].shape[0]
        Y = post["y"].reshape(-1, p.Cout).double()
        Wt = torch.zeros(nb * 32, 4, dtype=torch.float64)
        Wt[:p.Cout, :c2] = outl.w.reshape(c2, p.Cout).t().double().cpu()
        Yp = torch.zeros(Y.shape[0], nb * 32, dtype=torch.float64)
        Yp[:, :p.Cout] = Y
        Yb = Yp.view(-1, nb, 32).transpose(0, 1)             # [nb, M, 32]
        Wb = Wt.view(nb, 32, 4)
        z = torch.bmm(Yb, Wb)
        s = torch.bmm(Yb.abs(), Wb.abs())
        part = post["part"]
        if not bool((part[..., c2:] == 0).all()):
            self.flag(i, L, "fuse_part columns beyond the out_conv's channels are not zero")
        r, where = _worst(part, z, U * s)
        self.record(i, L, "fused_out_part", r, where=where)

    def _reduce(self, i, L, pre, post):
        _, nb, M, c2, _, _, _, flags = L.args
        outl = L.keep[1]
        part = pre["part"][..., :c2].double()
        b = outl.b.double().cpu()
        z = part.sum(0) + b
        s = part.abs().sum(0) + b.abs()
        y64 = _act(z, flags)
        r, where = _worst(post["y"], y64, _den(z, y64, s, torch.zeros_like(s), flags))
        self.record(i, L, "fused_out_reduce", r, where=where)

    def _stem(self, i, L, pre, post):
        lib, plan = self.lib, self.plan
        x = pre["x"]
        if x.dtype == torch.uint8:              # cnl_stem_conv7x7_u8: (float(x) - mean255) * inv_std255 in fp32 (cnl_normalize_u8_nhwc_f32), then the conv
            m = torch.tensor(list(self.norm[0]), dtype=torch.float32)
            r = torch.tensor(list(self.norm[1]), dtype=torch.float32)
            xf = ((x.float() - m) * r).permute(0, 3, 1, 2).contiguous()
            form = "stem (uint8)"
        else:
            xf = x.contiguous()
            form = "stem"
        pooled = plan.stem_fused_pool
        self.forms.add(form + (" + fused max-pool" if pooled else ""))
        split = pooled or plan.algo != CNL_ALGO_F32
        cls = "stem_split" if split else "stem_f32"
        layer = plan._wt_stem
        W32, b32 = layer.w.permute(0, 3, 1, 2).cpu(), layer.b.cpu()
        pool = (lambda t: F.max_pool2d(t, 3, 2, 1)) if pooled else (lambda t: t)
        y = _nchw(post["y"])
        ya = pool(F.relu(F.conv2d(xf, W32, b32, stride=2, padding=3)))
        yb = pool(_nchw(_stem_f32_matrix_core(lib, plan, xf)))
        r = ra = rb = 0.0
        for n in range(xf.shape[0]):
            z, s, fl = _conv_parts(xf[n:n + 1].double(), W32.double(), b32.double(), 2, 3, CNL_RELU, None, None, split)
            y64, den = pool(F.relu(z)), pool(U * s + fl)
            r = max(r, float(_ratio(y[n:n + 1], y64, den).max()))
            ra = max(ra, float(_ratio(ya[n:n + 1], y64, den).max()))
            rb = max(rb, float(_ratio(yb[n:n + 1], y64, den).max()))
        self.record(i, L, cls, r, ra, rb)

    def _deconv(self, i, L, pre, post):
        """cnl_deconv2x_nhwc_f32 against ConvTranspose2d in float64 with the weights the phase blocks were packed from (engine._DeconvLayer: a permutation
        of the BN-folded fp32 weights, every tap in exactly one phase block)."""
        p, layer, lib = L.args, L.keep[3], self.lib
        K, cin, cout = layer.k, layer.cin, layer.cout
        pk = (K + K % 2) // 2 - 1
        Wf = torch.full((cin, cout, K, K), float("nan"), dtype=torch.float64)
        wp = layer.w.double().cpu()
        o = 0
        for dy in range(2):
            for dx in range(2):
                geo = []
                for d in (dy, dx):
                    t, pd = ctypes.c_int32(), ctypes.c_int32()
                    _lib.check(lib.cnl_deconv_phase_geometry(K, d, ctypes.byref(t), ctypes.byref(pd)))
                    geo.append((t.value, pd.value))
                (ty, py), (tx, px) = geo
                blk = wp[o:o + cout * ty * tx * cin].view(cout, ty, tx, cin)
                o += blk.numel()
                for jy in range(ty):
                    for jx in range(tx):
                        Wf[:, :, dy + pk + 2 * (py - jy), dx + pk + 2 * (px - jx)] = blk[:, jy, jx, :].t()
        assert not torch.isnan(Wf).any()
        X = _nchw(pre["x"]).double()
        b = layer.b.double().cpu()
        ct = lambda t, w, bb: F.conv_transpose2d(t, w, bb, stride=2, padding=pk, output_padding=K % 2)
        z = _act(ct(X, Wf, b), p.flags)
        s = ct(X.abs(), Wf.abs(), b.abs())
        if "res" in pre:
            R = _nchw(pre["res"]).double()
            z, s = z + R, s + R.abs()
        r, where = _worst(_nchw(post["y"]), z, U * s)
        self.record(i, L, "deconv", r, where=where)

    def _deform(self, i, L, pre, post):
        """cnl_deform_sample_nhwc_f32: torchvision's bilinear rule (ref_cpu._bilinear_zero) in float64 at the fp32 sampling positions the kernel forms."""
        _, _, _, N, H, W, C, _, no, K, has_mask = L.args
        X = _nchw(pre["x"]).double()
        om = _nchw(pre["om"])
        pad = (K - 1) // 2
        ys = torch.arange(H, dtype=torch.float32).view(1, H, 1)
        xs = torch.arange(W, dtype=torch.float32).view(1, 1, W)
        z, s = [], []
        for k in range(K * K):
            py = (ys - pad + k // K + om[:, 2 * k]).double()
            px = (xs - pad + k % K + om[:, 2 * k + 1]).double()
            v, va = ref_cpu._bilinear_zero(X, py, px), ref_cpu._bilinear_zero(X.abs(), py, px)
            if has_mask:
                m = torch.sigmoid(om[:, 2 * K * K + k].double()).unsqueeze(1)
                v, va = v * m, va * m
            z.append(v)
            s.append(va)
        z = torch.stack(z, 1).permute(0, 3, 4, 1, 2).reshape(N, H, W, K * K * C)
        s = torch.stack(s, 1).permute(0, 3, 4, 1, 2).reshape(N, H, W, K * K * C)
        r, where = _worst(post["y"], z, U * s)
        self.record(i, L, "deform_sample", r, where=where)

    def _fuse_sum(self, i, L, pre, post):
        g0, g1, gl, den, mode = L.args[12:17]
        res = {0: lambda t: F.interpolate(t, scale_factor=2, mode="nearest"),
               1: lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=False),
               2: lambda t: F.max_pool2d(t, 2, 2), 3: lambda t: t}[mode]
        ins = [_nchw(pre["in0"])] + ([_nchw(pre["in1"])] if "in1" in pre else []) + [res(_nchw(pre["last"]))]
        gs = [g0] + ([g1] if "in1" in pre else []) + [gl]
        y = _nchw(post["y"])
        if all(g == 1.0 for g in gs) and den == 1.0 and mode != 1:
            if not torch.equal(y, torch.stack(ins, dim=-1).sum(dim=-1)):      # (test_fuse_sum_kernel: the plain sum is bit-exact)
                self.flag(i, L, "plain fuse sum not bit-exact")
            return
        raw = [_nchw(pre["in0"]).double()] + ([_nchw(pre["in1"]).double()] if "in1" in pre else []) + [_nchw(pre["last"]).double()]
        z = sum(float(g) * (res(t) if j == len(raw) - 1 else t) for j, (g, t) in enumerate(zip(gs, raw))) / float(den)
        s = sum(abs(float(g)) * (res(t.abs()) if j == len(raw) - 1 else t.abs()) for j, (g, t) in enumerate(zip(gs, raw))) / float(den)
        r, where = _worst(y, z, U * s)
        self.record(i, L, "fuse_sum", r, where=where)

    def report(self):
        lines = [f"[replay {self.name}] {len(self.plan.launches)} launches; max ratio per class (fp32 CPU conv | fp32 matrix core yardsticks):"]
        for cls, (r, ra, rb, n) in sorted(self.stats.items()):
            lines.append(f"    {cls:18s} x{n:3d}  {r:8.4f}" + (f"   ({ra:8.4f} | {rb:8.4f})" if rb else "") + f"   R_CLASS {R_CLASS[cls]}")
        for f in self.fail:
            lines.append(f"    FLAGGED launch {f[0]} {f[1]}: {f[2]}")
        return "\n".join(lines)


def replay_and_check(name, capsys):
    model, sd, plan, x, norm = build_plan(name)
    want = plan.run(x, norm)                                  # the real run, for the stepper's bit-identity
    want = OrderedDict((k, v.clone()) for k, v in want.items())
    torch.cuda.synchronize()
    chk = Checker(plan, name, norm)
    got = replay(plan, x, norm, check=chk)
    with capsys.disabled():
        print("\n" + chk.report())
    for k in want:
        assert torch.equal(got[k], want[k]), f"the stepper's {k} differs from Plan.run's"
    return chk


@pytest.mark.parametrize("name", list(PLANS))
def test_every_launch_of_the_plan_against_float64(name, capsys):
    chk = replay_and_check(name, capsys)
    assert not chk.fail, chk.report()
    assert chk.stats                                          # (something was measured)


# ---------------------------------------------------------------------------------------------------------------------------- coverage
REQUIRED_FORMS = {"direct fp32", "direct fp16-split, pre-split weights", "winograd9", "winograd10", "winograd11", "winograd13", "split-K",
                  "winograd9 + folded out_conv", "winograd9 + row-pair weights", "stem + fused max-pool", "stem", "stem (uint8) + fused max-pool"}


def test_the_replayed_plans_reach_every_kernel_form():
    """Across PLANS, the conv launches reach every kernel form of the path.  The fp16-split sub-pixel phases (cnl_conv3x3_up2_nhwc_f32 with x_absmax)
    are unreachable from these plans — the row-Winograd kernels take their layers whenever the split arithmetic is allowed (engine.py _conv: `not
    rowwino`) — and are checked at kernel level by test_gpu_conv.py::test_conv3x3_on_upsampled_input_as_subpixel_phases[True-*]; the fp32 form is
    reached by the algo="f32" plan."""
    forms = set()
    for name in PLANS:
        _, _, plan, _, _ = build_plan(name)
        lib = plan.lib
        for L in plan.launches:
            if isinstance(L.args, ConvParams):
                form = conv_class(lib, L)[1]
                forms.update({form, form.split(" + ")[0]})
            elif L.fn == "stem":
                forms.add(("stem (uint8)" if PLANS[name][6] else "stem") + (" + fused max-pool" if plan.stem_fused_pool else ""))
        del plan
        torch.cuda.empty_cache()
    print("kernel forms reached:", sorted(forms))
    missing = REQUIRED_FORMS - forms
    assert not missing, (missing, sorted(forms))
    assert "sub-pixel phases fp32" in forms


# ---------------------------------------------------------------------------------------------------------------------------- sensitivity
SENS_PLAN = "C1_256"


def _split_reader(plan):
    """The first fp16-split Winograd launch that reads a handed-over slot (its producer's y_absmax)."""
    lib = plan.lib
    for i, L in enumerate(plan.launches):
        if isinstance(L.args, ConvParams) and L.args.x_absmax and L.fn is lib.cnl_conv3x3_winograd_f32 and conv_class(lib, L)[0] == "row_wino" \
                and not any(isinstance(M.args, list) and M.fn is lib.cnl_absmax_per_image_f32 and M.args[5] == L.args.x_absmax for M in plan.launches):
            return i
    raise AssertionError("no split launch with a handed-over slot")


def test_a_doctored_absmax_slot_is_caught(capsys):
    """A handed-over per-image maximum 2^k too large leaves every output finite and inside the path's 1e-4 against the CPU oracle (precision is lost
    only far below the image maximum) — the gap this file closes.  The replay flags the launch: the slot check at any k >= 1, the per-element float64
    gate on its own from the smallest k printed, at which the final outputs still pass the end-to-end comparison."""
    model, sd, plan, x, norm = build_plan(SENS_PLAN)
    target = _split_reader(plan)
    L = plan.launches[target]

    def doctor(k):
        def before(i, L_, ins, outs):
            if i == target:
                ins["xslot"].mul_(2.0 ** k)
        return before

    k_gate = None
    for k in range(1, 25):
        chk = Checker(plan, SENS_PLAN)
        only = lambda i, L_, pre, post: chk(i, L_, pre, post) if i == target else None
        replay(plan, x, norm, check=only, before=doctor(k), stop=target)
        assert any(f[0] == target and "x_absmax slot" in f[2] for f in chk.fail)          # the wiring check, whatever k
        if any(f[0] == target and "x_absmax slot" not in f[2] for f in chk.fail):
            k_gate = k
            break
    assert k_gate is not None
    ref = ref_cpu.forward(sd, x.cpu(), sigmoid=True)
    outs = replay(plan, x, norm, before=doctor(k_gate))
    worst = {n: float(((outs[n].cpu() - ref[n]).abs() - 1e-4 - 1e-4 * ref[n].abs()).max()) for n in ref}
    with capsys.disabled():
        print(f"\n[doctored slot] launch {target} ({L.what}): max |x| slot x 2^k is caught by the float64 gate from k = {k_gate}; the final outputs "
              f"then exceed the 1e-4 comparison with the CPU oracle by {worst} (<= 0: pass)")
    for n in ref:
        torch.testing.assert_close(outs[n].cpu(), ref[n], rtol=1e-4, atol=1e-4)


def test_one_bad_element_flags_that_launch_only(capsys):
    """After one launch, 16 x (u s_e + floor_e) is added to ONE output element with a small scale, inside the dark region of image 0: the replay flags
    that launch and no other (every later launch is checked on its own input, the bad element included)."""
    model, sd, plan, x, norm = build_plan(SENS_PLAN)
    target = _split_reader(plan)
    lib = plan.lib
    hit = {}

    def after(i, L, ins, outs):
        if i != target:
            return
        p = L.args
        cls = conv_class(lib, L)[0]
        X = _nchw(ins["x"].cpu()).double()[:1]
        layer = L.keep[3]
        R = _nchw(ins["res"].cpu()).double()[:1] if "res" in ins else None
        z, s, fl = _conv_parts(X, layer.w.permute(0, 3, 1, 2).double().cpu(), layer.b.double().cpu(), p.stride, p.pad, p.flags, R, WINDOW.get(cls), True)
        den = (U * s + fl)[0]                                     # [C, H, W]
        C, H, W = den.shape
        region = den[:, H // 4 + 2:H // 2 - 2, W // 2 + 2:W // 2 + W // 4 - 2]        # the dark region (structured_images), away from its border
        pos = region.reshape(-1)
        j = int(torch.where(pos > 0, pos, torch.full_like(pos, float("inf"))).argmin())
        c, yy, xx = j // (region.shape[1] * region.shape[2]), (j // region.shape[2]) % region.shape[1], j % region.shape[2]
        yy, xx = yy + H // 4 + 2, xx + W // 2 + 2
        delta = 16.0 * float(den[c, yy, xx])
        hit.update(c=c, y=yy, x=xx, delta=delta, median=float(den.median()))
        outs["y"][0, yy, xx, c] += delta

    chk = Checker(plan, SENS_PLAN)
    replay(plan, x, norm, check=chk, after=after)
    flagged = sorted({f[0] for f in chk.fail})
    with capsys.disabled():
        print(f"\n[one bad element] launch {target} ({plan.launches[target].what}): +{hit['delta']:.3g} at (0, {hit['y']}, {hit['x']}, {hit['c']}) "
              f"(median u s + floor of the launch {hit['median']:.3g}); flagged launches {flagged}, ratio {chk.launch_ratio.get(target, 0):.3g}")
    assert flagged == [target], chk.report()


# ---------------------------------------------------------------------------------------------------------------------------- where a launch writes
def _digest(t):
    return hashlib.blake2b(t.contiguous().numpy().tobytes(), digest_size=16).digest()


def footprint_and_lockstep(build, capsys=None, io=None):
    """build(reuse_buffers) -> (plan, x, norm), the same model and input twice.  Both plans are replayed with footprint=True (every launch changes
    only its declared outputs), and in lock step: the same launch list, and at every launch index the same input and output BITS — the plan without
    reuse is alias-free by construction, so a liveness mistake of Plan._bind (a pointer field it does not enumerate, two live buffers on one range)
    shows at the launch where it bites, not only — or not at all — in the final outputs.  splitk_scratch is zeroed before its launch in both replays
    (slices the launcher drops as empty are never written), so the partial sums are part of the comparison too.  -> the per-launch digests."""
    seen = []
    for reuse in (True, False):
        plan, x, norm = build(reuse)
        rec, bad = [], []

        def check(i, L, pre, post, rec=rec):
            rec.append((L.what, {("pre", k): _digest(v) for k, v in pre.items()}, {("post", k): _digest(v) for k, v in post.items()}))

        def before(i, L, ins, outs_):
            if "scratch" in outs_:
                outs_["scratch"].zero_()

        outs = replay(plan, x, norm, check=check, before=before, footprint=True, violations=bad, io=io)
        assert not bad, "\n".join(f"launch {i} {what}: {why}" for i, what, why in bad)
        seen.append((plan, rec, OrderedDict((k, v.clone()) for k, v in outs.items())))
        del plan
    (pa, a, oa), (pb, b, ob) = seen
    assert pa.options.reuse_buffers and not pb.options.reuse_buffers and pa.arena_bytes < pb.arena_bytes
    assert [w for w, _, _ in a] == [w for w, _, _ in b], "the launch lists differ"
    for i, ((what, pre_a, post_a), (_, pre_b, post_b)) in enumerate(zip(a, b)):
        diff = sorted(k for k in set(pre_a) | set(pre_b) | set(post_a) | set(post_b) if {**pre_a, **post_a}.get(k) != {**pre_b, **post_b}.get(k))
        assert not diff, f"launch {i} {what}: {diff} differ between the plan that reuses its arena and the one that does not"
    for k in oa:
        assert torch.equal(oa[k], ob[k]), k
    if capsys is not None:
        with capsys.disabled():
            print(f"\n[footprint + lock step] {len(a)} launches, arena {pa.arena_bytes} bytes with reuse / {pb.arena_bytes} without")
    return a


def plan_with(model, x, norm=None, **options):
    """The plan the same model (same packed weights) uses for the same input under other kernel options: the engine keys its plans by them."""
    opts = model.set_kernel_options(**options)
    if norm is not None:
        model._engine.forward_u8(x, norm[0], norm[1], sigmoid=True)
    else:
        model._engine.forward(x, sigmoid=True)
    torch.cuda.synchronize()
    (plan,) = [p for p in model._engine.plans.values() if p.options == opts]
    return plan


@pytest.mark.parametrize("name", FOOTPRINT_PLANS)
def test_launches_write_only_their_declared_outputs_and_arena_reuse_changes_no_byte(name, capsys):
    model, _, plan, x, norm = build_plan(name)
    footprint_and_lockstep(lambda reuse: (plan if reuse else plan_with(model, x, norm, reuse_buffers=False), x, norm), capsys)


def test_one_float_past_an_output_view_flags_that_launch_only(capsys):
    """With footprint=True, an `after` hook changes ONE word of the arena just behind a launch's output view: the replay flags that launch and no
    other — every other launch is compared against the bytes as they were just before it ran, the planted word included."""
    model, sd, plan, x, norm = build_plan(SENS_PLAN)
    target = _split_reader(plan)
    hit = {}

    def after(i, L, ins, outs):
        if i != target:
            return
        v = outs["y"]
        word = (v.data_ptr() - plan.arena.data_ptr()) // 4 + sum((d - 1) * s for d, s in zip(v.shape, v.stride())) + 1
        assert 0 < word < plan.arena.numel()
        plan.arena.view(torch.int32)[word] += 1                 # (an integer add: the old bytes may be a NaN, which a float add would keep)
        hit["word"] = word

    bad = []
    replay(plan, x, norm, after=after, footprint=True, violations=bad)
    with capsys.disabled():
        print(f"\n[one float past the view] launch {target} ({plan.launches[target].what}): arena word {hit['word']}; flagged: {bad}")
    assert [b[0] for b in bad] == [target] and f"arena word {hit['word']}" in bad[0][2], bad
    clean = []
    replay(plan, x, norm, footprint=True, violations=clean)
    assert not clean, clean
