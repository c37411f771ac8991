"""The validation value of the detection losses on the GPU: the reference's CenterNet.compute_loss (models/centernet.py:123-200: Gaussian target
heatmap, heatmap loss, 3x3 centre-sampled box loss) without its Python loops over images and boxes, without a second N x C x H x W tensor and
without the logits leaving the device.

detection_loss() is ONE call of cnl_detection_loss_f64 (csrc/det_loss.hip: four launches, the logits read once); render_targets() runs the same
kernel for the target heatmap alone; LossMeter accumulates the per-batch values on the device as Lightning's self.log averaging would.  The
rule is stated in include/centernet_gfx950.h and restated in numpy in tests/loss_ref.py.

detection_loss_grad() is ONE call of cnl_detection_loss_grad_f32 (at most four launches): the analytic gradient of that value with respect to the
logits and the box values (tests/loss_grad_ref.py).  DetectionLoss is the criterion training calls: an nn.Module whose "heatmap", "box_2d" and
"total" carry a grad_fn, so criterion(outputs, targets)["total"].backward() works on the head outputs of any torch model on the device.  fp32 inputs
only, no double backward, no backward through the conv engine.  The re-ID loss of the tracking model is the second half of this file: reid_loss() /
reid_loss_grad() (csrc/reid_loss.hip), the ReIDLoss criterion that owns the reference's classifier, and TrackingLoss, which adds it to DetectionLoss's total
(the reference leaves it out at validation, fairmot.py:87-91: TrackingLoss(...)(outputs, targets, ignore_reid=True)).
No CPU fallback: a missing device or library raises.
"""
import ctypes
import math

import numpy as np
import torch

from . import _gather, _lib
from . import _targets as _t

MAX_PER_IMAGE = 1024          # boxes per image (csrc/det_loss.hip)
MAX_CLASSES, MAX_SIDE, MAX_IMAGES = 1 << 16, 1 << 15, 1 << 16
TARGET_METHODS = {"cornernet": (0, "min_overlap", 0.3), "ttfnet": (1, "alpha", 0.54), "fixed": (2, "r", 1.0)}
# Gen-A YAML spelling (configs/base_resnet34.yaml:17-24) and Gen-B class names (losses/__init__.py)
HEATMAP_LOSSES = {"cornernet_focal": 0, "CornerNetFocalLoss": 0, "quality": 1, "QualityFocalLoss": 1}
BOX_LOSSES = {"l1": 0, "L1Loss": 0, "smooth_l1": 1, "SmoothL1Loss": 1, "iou": 2, "IoULoss": 2, "giou": 3, "GIoULoss": 3, "diou": 4, "DIoULoss": 4,
              "ciou": 5, "CIoULoss": 5}
METRIC_NAMES = ("heatmap_loss", "box_2d_loss", "total_loss")
GEN_B_KEYS = ("heatmap_loss", "box_loss", "heatmap_loss_weight", "box_loss_weight", "heatmap_target", "heatmap_target_params")


def _number(value, name, what, positive=False):
    if isinstance(value, bool) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(float(value)) or \
            (positive and float(value) <= 0):
        raise ValueError(f"{what}: {name} must be a finite {'positive ' if positive else ''}number, got {value!r}")
    return float(value)


def loss_params(stride=4, heatmap_target="cornernet", heatmap_target_params=None, heatmap_loss="cornernet_focal", box_loss="giou",
                heatmap_loss_weight=1.0, box_loss_weight=1.0, box_log=False, box_multiplier=1.0, what="detection_loss"):
    """The checked cnl_loss_params block of these settings (needs neither a device nor the library)."""
    if heatmap_target not in TARGET_METHODS:
        raise ValueError(f"{what}: heatmap_target must be one of {sorted(TARGET_METHODS)}, got {heatmap_target!r}")
    method, key, param = TARGET_METHODS[heatmap_target]
    if heatmap_target_params is not None:
        if not isinstance(heatmap_target_params, dict) or set(heatmap_target_params) - {key}:
            raise ValueError(f"{what}: heatmap_target_params of '{heatmap_target}' may hold '{key}' only, got {heatmap_target_params!r}")
        param = _number(heatmap_target_params.get(key, param), f"heatmap_target_params['{key}']", what)
    if method == 0 and not 0.0 < param < 1.0:
        raise ValueError(f"{what}: cornernet min_overlap must lie in (0, 1), got {param!r}")
    if heatmap_loss not in HEATMAP_LOSSES:
        raise ValueError(f"{what}: heatmap_loss must be one of {sorted(HEATMAP_LOSSES)}, got {heatmap_loss!r}")
    if box_loss not in BOX_LOSSES:
        raise ValueError(f"{what}: box_loss must be one of {sorted(BOX_LOSSES)}, got {box_loss!r}")
    p = _lib.LossParams()
    p.stride = _number(stride, "stride", what, positive=True)
    p.target_param, p.target_method = param, method
    p.heatmap_loss, p.box_loss = HEATMAP_LOSSES[heatmap_loss], BOX_LOSSES[box_loss]
    p.hm_alpha, p.hm_beta = (2.0, 4.0) if p.heatmap_loss == 0 else (0.0, 2.0)          # the reference's defaults (heatmap_losses.py:15, 52)
    p.heatmap_weight = _number(heatmap_loss_weight, "heatmap_loss_weight", what)
    p.box_weight = _number(box_loss_weight, "box_loss_weight", what)
    p.box_multiplier = _number(box_multiplier, "box_multiplier", what)
    p.box_log = 1 if box_log else 0
    return p


def settings_from_config(output_heads=None, **gen_b):
    """The keyword arguments of detection_loss a config asks for.  Gen-A: `output_heads.heatmap.{target_method, loss_function, loss_weight}` and
    `output_heads.box_2d.{loss_function, loss_weight}`; Gen-B: `heatmap_loss`, `box_loss`, `heatmap_loss_weight`, `box_loss_weight`,
    `heatmap_target`, `heatmap_target_params` (these win).  Keys that are absent leave detection_loss's defaults."""
    out = {}
    heads = output_heads or {}
    hm, box = dict(heads.get("heatmap") or {}), dict(heads.get("box_2d") or {})
    for src, key, name in ((hm, "target_method", "heatmap_target"), (hm, "loss_function", "heatmap_loss"), (hm, "loss_weight", "heatmap_loss_weight"),
                           (box, "loss_function", "box_loss"), (box, "loss_weight", "box_loss_weight")):
        if key in src:
            out[name] = src[key]
    for name in GEN_B_KEYS:
        if gen_b.get(name) is not None:
            out[name] = gen_b[name]
    loss_params(what="loss settings of the config", **out)       # a misspelt name fails where the model is built
    return out


def _read(targets, N, spec, length, row_ok, cannot, what):
    """targets in either form (_targets.py) -> (device or None, (boxes [N,Gmax,4] f64, the column [N,Gmax] i64, count [N] i32) as device tensors or
    numpy, Gmax).  The padded form is a dict or a tuple of `length` tensors; only the list form is judged by row_ok / cannot."""
    if isinstance(targets, dict) or _t.is_padded(targets, (length,)):
        t, Gmax, dev = _t.read_padded(targets, N, spec, what, cap=MAX_PER_IMAGE)
    else:
        (t, Gmax), dev = _t.read_list(targets, N, spec, what, cap=MAX_PER_IMAGE, row_ok=row_ok, cannot=cannot), None
    return dev, (t["boxes"], t[spec[1].name], t["count"]), Gmax


def _targets(targets, N, C, H, W, stride, what):
    """detection_loss's targets: the list, the dict {"boxes", "labels", "count"} or the tuple (boxes, labels, count)"""
    def row_ok(boxes, labels):             # the record rule of include/centernet_gfx950.h, in numpy float64
        with np.errstate(all="ignore"):
            b = boxes / float(stride)
            cx, cy = np.rint(b[:, 0] + b[:, 2] / 2), np.rint(b[:, 1] + b[:, 3] / 2)
            return np.isfinite(b).all(axis=1) & (b[:, 2] >= 0) & (b[:, 3] >= 0) & (cx >= 0) & (cx <= W) & (cy >= 0) & (cy <= H) & (labels >= 0) & (labels < C)

    return _read(targets, N, _t.LABELS, 3, row_ok,
                 lambda label: f"(label {label}) cannot be a target on a {H} x {W} map of {C} classes at stride {stride}: non-finite, negative "
                               f"size, centre outside the map or label outside 0..{C - 1}", what)


def _same_device(g_dev, dev, what, outputs="outputs"):
    if g_dev is not None and g_dev != dev:
        raise ValueError(f"{what}: {outputs} on {dev}, targets on {g_dev}")


def _on_device(g_dev, gts, N, dev, what, outputs="outputs", keep=False):
    """_read's result on the outputs' device: device tensors must live there, host arrays go up in one copy.  keep: the result is saved for a
    backward, so the caller's own device tensors are copied (a loop that refills its target buffers before the backward runs changes nothing)."""
    _same_device(g_dev, dev, what, outputs)
    if g_dev is None:
        with torch.cuda.device(dev):
            gts = [torch.from_numpy(a).to(dev) for a in gts] if N == 0 else _gather.upload_parts(list(gts), dev)      # (an empty batch: nothing to stage)
    elif keep:
        gts = [t.clone() for t in gts]
    return tuple(gts)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _map_args(t):
    """The pointer and the four strides of a map, or NULL and zeros"""
    return (None, 0, 0, 0, 0) if t is None else (t.data_ptr(), *t.stride())


def _call(name, workspace_bytes, dev, *args):
    """One entry point on dev's current stream, inside the caller's `with torch.cuda.device(dev)`: args are its arguments up to the workspace,
    workspace_bytes = (the name of its size query, the query's arguments)."""
    lib = _lib.load()
    nbytes = getattr(lib, workspace_bytes[0])(*workspace_bytes[1:])
    ws = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=dev)
    _lib.check(getattr(lib, name)(*args, ws.data_ptr(), nbytes, _lib.stream(dev)), name)


def _check_want(want, allowed, what):
    """-> a flag per name of `allowed`"""
    if isinstance(want, str) or not isinstance(want, (tuple, list)) or not want or any(w not in allowed for w in want) or len(set(want)) != len(want):
        raise ValueError(f"{what}: want must be a non-empty tuple out of {allowed}, got {want!r}")
    return tuple(w in want for w in allowed)


def _outputs(outputs, keys, who):
    if not isinstance(outputs, dict) or any(k not in outputs for k in keys):
        raise ValueError(f"{who}: outputs must be the dict of get_encoded_outputs with {' and '.join(repr(k) for k in keys)}")
    return [outputs[k] for k in keys]


def _check_map(t, name, channels, what):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 4:
        raise ValueError(f"{what}: {name} must be a float32 tensor [N, {channels}, H, W], got "
                         f"{(t.dtype, tuple(t.shape)) if isinstance(t, torch.Tensor) else type(t).__name__}")


def _check_sizes(N, C, H, W, what):
    if not (0 <= N <= MAX_IMAGES and 1 <= C <= MAX_CLASSES and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"{what}: N x C x H x W = {N} x {C} x {H} x {W} outside 0..{MAX_IMAGES} x 1..{MAX_CLASSES} x 1..{MAX_SIDE} x 1..{MAX_SIDE}")


def _check_outputs(heatmap, box_2d, what):
    """The head outputs of one call -> (N, C, H, W)"""
    _check_map(heatmap, "heatmap", "C", what)
    _check_map(box_2d, "box_2d", 4, what)
    N, C, H, W = (int(v) for v in heatmap.shape)
    if tuple(box_2d.shape) != (N, 4, H, W):
        raise ValueError(f"{what}: heatmap {tuple(heatmap.shape)} needs box_2d [{N}, 4, {H}, {W}], got {tuple(box_2d.shape)}")
    _check_sizes(N, C, H, W, what)
    _gather.require_hip([heatmap, box_2d], what)
    if box_2d.device != heatmap.device:
        raise ValueError(f"{what}: heatmap on {heatmap.device}, box_2d on {box_2d.device}")
    return N, C, H, W


def _run(heatmap, box_2d, targets, shape, params, want_targets, dev, what):
    """The one call.  heatmap / box_2d None: targets only.  -> (out [N*4 + 3] f64, skipped [1] i32, target map or None)."""
    N, C, H, W = shape
    g_dev, gts, Gmax = _targets(targets, N, C, H, W, params.stride, what)
    if dev is None:
        dev = g_dev
    if dev is None or dev.index is None:
        if not torch.cuda.is_available():
            raise RuntimeError(f"{what} runs on HIP devices only (no CPU fallback)")
        dev = torch.device("cuda", torch.cuda.current_device())
    _same_device(g_dev, dev, what)
    with torch.cuda.device(dev):
        out = torch.zeros((N * 4 + 3,), dtype=torch.float64, device=dev)
        skipped = torch.zeros((1,), dtype=torch.int32, device=dev)
        tmap = torch.empty((N, C, H, W), dtype=torch.float32, device=dev, memory_format=torch.channels_last) if want_targets else None
        if N:
            if g_dev is None:
                gts = _gather.upload_parts(list(gts), dev)
            _call("cnl_detection_loss_f64", ("cnl_detection_loss_workspace_bytes", N, Gmax, H, W), dev, *_map_args(heatmap), *_map_args(box_2d),
                  N, C, H, W, gts[0].data_ptr(), gts[1].data_ptr(), gts[2].data_ptr(), Gmax, ctypes.byref(params), *_map_args(tmap),
                  out.data_ptr(), out.data_ptr() + 8 * 4 * N, skipped.data_ptr())
    return out, skipped, tmap


def detection_loss(heatmap, box_2d, targets, stride=4, heatmap_target="cornernet", heatmap_target_params=None, heatmap_loss="cornernet_focal",
                   box_loss="giou", heatmap_loss_weight=1.0, box_loss_weight=1.0, box_log=False, box_multiplier=1.0, return_targets=False):
    """The reference's compute_loss on the device.  heatmap [N, C, H, W] fp32 LOGITS and box_2d [N, 4, H, W] fp32 as get_encoded_outputs returns
    them (any strides; channels-last is the fast path).  targets: the reference's list of per-image {"boxes" [m, 4] x y w h in input pixels,
    "labels" [m]} (checked on the host: a box that cannot be a target raises ValueError; padded and uploaded in one copy), or padded device tensors
    (boxes [N, Gmax, 4] float64, labels [N, Gmax] int64, count [N] int32) as a tuple or dict (a bad box is skipped and counted in "skipped").
    At most 1024 boxes per image.  Loss names in the Gen-A YAML spelling or as Gen-B class names.
    -> {"heatmap", "box_2d", "total"}: 0-dim float64 device tensors; "per_image" [N, 4] float64 rows (heatmap_sum, box_sum, num_dets, num_boxes);
    "skipped": 0-dim int32; with return_targets also "targets", the fp32 target heatmap [N, C, H, W] (channels-last).  No synchronisation."""
    what = "detection_loss"
    params = loss_params(stride, heatmap_target, heatmap_target_params, heatmap_loss, box_loss, heatmap_loss_weight, box_loss_weight, box_log,
                         box_multiplier, what)
    N, C, H, W = _check_outputs(heatmap, box_2d, what)
    out, skipped, tmap = _run(heatmap, box_2d, targets, (N, C, H, W), params, bool(return_targets), heatmap.device, what)
    res = {"heatmap": out[4 * N], "box_2d": out[4 * N + 1], "total": out[4 * N + 2], "per_image": out[:4 * N].view(N, 4), "skipped": skipped[0]}
    if return_targets:
        res["targets"] = tmap
    return res


WANT = ("heatmap", "box_2d")


def _device_targets(targets, shape, stride, dev, what, keep=False):
    """targets in either form -> the padded (boxes, labels, count) device tensors of one call; a host list is checked, padded and uploaded in one copy."""
    N, C, H, W = shape
    g_dev, gts, _ = _targets(targets, N, C, H, W, stride, what)
    return _on_device(g_dev, gts, N, dev, what, keep=keep)


def _scale(value, name, dev, what):
    """A Python number, or a 0-dim / 1-element float64 tensor on the device -> a number or a 0-dim float64 device tensor"""
    if isinstance(value, torch.Tensor):
        if value.dtype != torch.float64 or value.numel() != 1:
            raise ValueError(f"{what}: {name} as a tensor must be float64 with one element, got {value.dtype} {tuple(value.shape)}")
        if value.device != dev:
            raise ValueError(f"{what}: {name} on {value.device}, outputs on {dev}")
        return value.detach().reshape(())
    return _number(value, name, what)


def _scale_arg(values, dev):
    """The checked scales of one call (_scale) -> what the entry point reads: None (all 1) or a float64 device tensor [len(values)]"""
    on_device = any(isinstance(v, torch.Tensor) for v in values)
    if not on_device and all(v == 1.0 for v in values):
        return None
    if on_device and len(values) == 1:
        return values[0].reshape(1)
    with torch.cuda.device(dev):
        if on_device:
            return torch.stack([v if isinstance(v, torch.Tensor) else torch.full((), v, dtype=torch.float64, device=dev) for v in values])
        return _gather.upload_parts([np.array(values, dtype=np.float64)], dev)[0]


def _like(t):
    """An uninitialised tensor of t's shape: t's strides when t is dense (contiguous or channels-last), else contiguous."""
    if t.is_contiguous() or t.is_contiguous(memory_format=torch.channels_last):
        return torch.empty_strided(tuple(t.shape), t.stride(), dtype=t.dtype, device=t.device)
    return torch.empty(tuple(t.shape), dtype=t.dtype, device=t.device)


def _run_grad(heatmap, box_2d, gts, shape, params, scales, want):
    """The one call.  gts: padded device targets; scales: None (1, 1) or a float64 device tensor [2]; want: (heatmap?, box_2d?).
    -> (heatmap gradient or None, box_2d gradient or None, skipped [1] i32)"""
    N, C, H, W = shape
    dev = heatmap.device
    with torch.cuda.device(dev):
        gh = _like(heatmap) if want[0] else None
        gb = _like(box_2d) if want[1] else None
        skipped = torch.zeros((1,), dtype=torch.int32, device=dev)
        if N:
            Gmax = int(gts[0].shape[1])
            _call("cnl_detection_loss_grad_f32", ("cnl_detection_loss_grad_workspace_bytes", N, Gmax, H, W), dev, *_map_args(heatmap),
                  *_map_args(box_2d), N, C, H, W, gts[0].data_ptr(), gts[1].data_ptr(), gts[2].data_ptr(), Gmax, ctypes.byref(params), _ptr(scales),
                  *_map_args(gh), *_map_args(gb), skipped.data_ptr())
    return gh, gb, skipped


def detection_loss_grad(heatmap, box_2d, targets, stride=4, heatmap_target="cornernet", heatmap_target_params=None, heatmap_loss="cornernet_focal",
                        box_loss="giou", heatmap_loss_weight=1.0, box_loss_weight=1.0, box_log=False, box_multiplier=1.0, heatmap_scale=1.0,
                        box_scale=1.0, want=WANT):
    """The gradient of heatmap_scale * res["heatmap"] + box_scale * res["box_2d"] (res = detection_loss(...) on the same arguments) with respect to
    the fp32 logits and box values, analytic, float64 rounded once to fp32 (the rule: include/centernet_gfx950.h).  The two loss weights are NOT
    applied: the gradient of "total" is the one with scales (heatmap_loss_weight, box_loss_weight).  Each scale is a Python number or a 0-dim /
    1-element float64 tensor on the device (read there).  want: which gradients to compute, a subset of ("heatmap", "box_2d").
    -> {"heatmap_grad", "box_2d_grad": fp32 of the input's shape (None when not wanted), with the input's strides when it is dense (contiguous or
    channels-last), else contiguous; "skipped": 0-dim int32}.  One call of cnl_detection_loss_grad_f32, no synchronisation, no atomics: the same
    bits on every run."""
    what = "detection_loss_grad"
    params = loss_params(stride, heatmap_target, heatmap_target_params, heatmap_loss, box_loss, heatmap_loss_weight, box_loss_weight, box_log,
                         box_multiplier, what)
    want = _check_want(want, WANT, what)
    _check_map(heatmap, "heatmap", "C", what)
    _check_map(box_2d, "box_2d", 4, what)
    dev = heatmap.device
    s_heat, s_box = _scale(heatmap_scale, "heatmap_scale", dev, what), _scale(box_scale, "box_scale", dev, what)
    shape = _check_outputs(heatmap, box_2d, what)
    gts = _device_targets(targets, shape, params.stride, dev, what)
    gh, gb, skipped = _run_grad(heatmap.detach(), box_2d.detach(), gts, shape, params, _scale_arg((s_heat, s_box), dev), want)
    return {"heatmap_grad": gh, "box_2d_grad": gb, "skipped": skipped[0]}


class _DetectionLossFunction(torch.autograd.Function):
    """detection_loss with the backward of cnl_detection_loss_grad_f32: one call forward, one call backward."""

    @staticmethod
    def forward(ctx, heatmap, box_2d, targets, settings):
        what = "DetectionLoss"
        params = loss_params(what=what, **settings)
        shape = _check_outputs(heatmap, box_2d, what)
        # a host list: padded and uploaded once, kept for the backward; the caller's device tensors: copied, so that the backward reads this call's targets
        gts = _device_targets(targets, shape, params.stride, heatmap.device, what, keep=True)
        out, skipped, _ = _run(heatmap, box_2d, gts, shape, params, False, heatmap.device, what)
        N = shape[0]
        ctx.save_for_backward(heatmap, box_2d, *gts)
        ctx.params, ctx.shape = params, shape
        per_image, skip = out[:4 * N].view(N, 4), skipped[0]
        ctx.mark_non_differentiable(per_image, skip)
        return out[4 * N], out[4 * N + 1], out[4 * N + 2], per_image, skip

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_heatmap, g_box_2d, g_total, _g_rows, _g_skipped):
        heatmap, box_2d, *gts = ctx.saved_tensors
        p = ctx.params
        scales = torch.stack([g_heatmap + g_total * p.heatmap_weight, g_box_2d + g_total * p.box_weight]).to(torch.float64)      # on the device: no synchronisation
        gh, gb, _ = _run_grad(heatmap, box_2d, tuple(gts), ctx.shape, p, scales, (ctx.needs_input_grad[0], ctx.needs_input_grad[1]))
        return gh, gb, None, None


class DetectionLoss(torch.nn.Module):
    """The criterion of a training step: DetectionLoss(**settings)(outputs, targets) -> the dict detection_loss returns, bit for bit, where "heatmap",
    "box_2d" and "total" carry a grad_fn when an output requires grad: criterion(outputs, targets)["total"].backward() reaches the head that produced
    `outputs` (any torch model on the device).  outputs: the dict of get_encoded_outputs ("heatmap" LOGITS, "box_2d"), fp32; targets as for
    detection_loss (a host list is padded and uploaded once, and kept for the backward; padded device tensors are copied for the backward, so the caller
    may refill them, as a loop that reuses augment_batch's out= buffers does, before it runs).  `settings`: detection_loss's keyword arguments
    (model.criterion() fills them from the model).  "per_image" and "skipped" are not differentiable; no double backward.  Under torch.no_grad(),
    or when no output requires grad, it is detection_loss."""

    def __init__(self, **settings):
        super().__init__()
        settings.pop("return_targets", None)
        loss_params(what="DetectionLoss", **settings)
        self.settings = settings

    def extra_repr(self):
        return ", ".join(f"{k}={v!r}" for k, v in self.settings.items())

    def forward(self, outputs, targets):
        heatmap, box_2d = _outputs(outputs, ("heatmap", "box_2d"), "DetectionLoss")
        needs = torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (heatmap, box_2d))
        if not needs:
            return detection_loss(heatmap, box_2d, targets, **self.settings)
        heat, box, total, per_image, skipped = _DetectionLossFunction.apply(heatmap, box_2d, targets, self.settings)
        return {"heatmap": heat, "box_2d": box, "total": total, "per_image": per_image, "skipped": skipped}


def render_targets(targets, num_classes, height, width, stride=4, heatmap_target="cornernet", heatmap_target_params=None, device=None):
    """The fp32 target heatmap [N, num_classes, height, width] (channels-last) of the targets, from the kernel detection_loss runs (no logits are
    read).  targets as for detection_loss; `device`: where to render when the targets come from the host (default: the current device)."""
    what = "render_targets"
    params = loss_params(stride, heatmap_target, heatmap_target_params, what=what)
    for name, v in (("num_classes", num_classes), ("height", height), ("width", width)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"{what}: {name} must be an int, got {v!r}")
    if _t.is_padded(targets):
        first = targets["boxes"] if isinstance(targets, dict) and "boxes" in targets else targets[0] if not isinstance(targets, dict) else None
        N = int(first.shape[0]) if isinstance(first, torch.Tensor) and first.dim() else 0
    elif isinstance(targets, (list, tuple)):
        N = len(targets)
    else:
        raise ValueError(f"{what}: targets must be a list of per-image dicts or padded device tensors, got {type(targets).__name__}")
    _check_sizes(N, int(num_classes), int(height), int(width), what)
    dev = None if device is None else torch.device(device)
    if dev is not None and dev.type != "cuda":
        raise RuntimeError(f"{what} runs on HIP devices only (no CPU fallback)")
    _, _, tmap = _run(None, None, targets, (N, int(num_classes), int(height), int(width)), params, True, dev, what)
    return tmap


class LossMeter:
    """The validation curves of an epoch: update(outputs, targets) per batch, get_metrics() -> {"heatmap_loss", "box_2d_loss", "total_loss"}, the
    per-batch values weighted by batch size (what Lightning's self.log averaging gives for val/heatmap_loss, val/box_2d_loss, val/total_loss).
    It accumulates on the device; get_metrics makes the one download and raises if any box was skipped.  `settings`: detection_loss's keyword
    arguments (model.loss_meter() fills them from the model)."""
    metric_names = METRIC_NAMES

    def __init__(self, **settings):
        settings.pop("return_targets", None)
        loss_params(what="LossMeter", **settings)
        self.settings = settings
        self._acc = None          # [5] float64 on the device: the three weighted sums, the images, the skipped boxes
        self.reset()

    def reset(self):
        self.num_batches = 0
        if self._acc is not None:
            self._acc.zero_()

    def update(self, outputs, targets):
        """outputs: the dict of get_encoded_outputs ("heatmap" logits, "box_2d").  One call of detection_loss, no synchronisation."""
        heatmap, box_2d = _outputs(outputs, ("heatmap", "box_2d"), "LossMeter.update")
        res = detection_loss(heatmap, box_2d, targets, **self.settings)
        n = int(heatmap.shape[0])
        step = torch.stack([res["heatmap"] * n, res["box_2d"] * n, res["total"] * n, res["total"].new_tensor(float(n)), res["skipped"].to(torch.float64)])
        if self._acc is None:
            self._acc = step
        else:
            if self._acc.device != step.device:
                raise ValueError(f"LossMeter: state on {self._acc.device}, input on {step.device}")
            self._acc += step
        self.num_batches += 1

    def state(self):
        """{"sums" [5] float64 device tensor (a copy), "num_batches"}: what another meter's merge() takes."""
        if self._acc is None:
            raise RuntimeError("LossMeter.state: nothing has been measured yet")
        return {"sums": self._acc.clone(), "num_batches": self.num_batches}

    def merge(self, state):
        """Add another meter's state() (how shards and ranks combine; no collective is involved)."""
        if not isinstance(state, dict) or "sums" not in state or "num_batches" not in state:
            raise ValueError("LossMeter.merge expects the dict another meter's state() returned")
        sums = state["sums"]
        if not isinstance(sums, torch.Tensor) or sums.dtype != torch.float64 or tuple(sums.shape) != (5,):
            raise ValueError("LossMeter.merge: 'sums' must be float64 [5]")
        _gather.require_hip([sums], "LossMeter.merge")
        if self._acc is None:
            self._acc = sums.clone()
        else:
            self._acc += sums.to(self._acc.device)
        self.num_batches += int(state["num_batches"])

    def get_metrics(self):
        if self._acc is None:
            raise RuntimeError("LossMeter.get_metrics: nothing has been measured yet")
        heat, box, total, images, skipped = self._acc.cpu().tolist()
        if skipped:
            raise ValueError(f"LossMeter.get_metrics: {int(skipped)} target box(es) were skipped (non-finite, negative size, centre outside the map or "
                             "label outside the classes): the reference's loss is not defined for them")
        images = max(images, 1.0)
        return dict(zip(METRIC_NAMES, (heat / images, box / images, total / images)))


# ------------------------------------------------------------------------------------------------------------------------ re-ID loss
# The tracking model's third loss (reference models/fairmot.py:34-61 EmbeddingHead.compute_loss): the embedding at every box centre through the training-only
# classifier Linear / BatchNorm1d / ReLU / Linear and a cross entropy over the track identities.  reid_loss() is ONE call of cnl_reid_loss_f64,
# reid_loss_grad() ONE call of cnl_reid_loss_grad_f32 (csrc/reid_loss.hip; the rule: include/centernet_gfx950.h; in numpy: tests/reid_loss_ref.py).
MAX_EMB, MAX_TRACK_IDS = 256, 1 << 20
CENTERS = {"trunc": 0, "round": 1}
REID_KEYS = ("W1", "gamma", "beta", "running_mean", "running_var", "W2", "b2")
REID_WANT = ("reid", "W1", "gamma", "beta", "W2", "b2")


def reid_params(training=True, stride=4, center="trunc", padded_rows=False, ignore_index=-1, bn_eps=1e-5, momentum=0.1, what="reid_loss"):
    """The checked cnl_reid_loss_params block of these settings (needs neither a device nor the library)."""
    if center not in CENTERS:
        raise ValueError(f"{what}: center must be one of {sorted(CENTERS)}, got {center!r}")
    if isinstance(ignore_index, bool) or not isinstance(ignore_index, (int, np.integer)):
        raise ValueError(f"{what}: ignore_index must be an int, got {ignore_index!r}")
    if momentum is None:
        raise ValueError(f"{what}: BatchNorm1d with momentum=None (a cumulative average) is not supported")
    p = _lib.ReidLossParams()
    p.stride = _number(stride, "stride", what, positive=True)
    p.bn_eps = _number(bn_eps, "eps", what, positive=True)
    p.momentum = _number(momentum, "momentum", what)
    if not 0.0 <= p.momentum <= 1.0:
        raise ValueError(f"{what}: momentum must lie in 0..1, got {momentum!r}")
    p.ignore_index, p.center, p.padded_rows, p.training = int(ignore_index), CENTERS[center], 1 if padded_rows else 0, 1 if training else 0
    return p


def _classifier(classifier, what):
    """A ReIDLoss or a dict of the seven tensors -> (the seven tensors by REID_KEYS, eps, momentum, num_batches_tracked or None), shapes checked."""
    if isinstance(classifier, ReIDLoss):
        lin1, bn, _, lin2 = classifier.classifier
        t = dict(W1=lin1.weight, gamma=bn.weight, beta=bn.bias, running_mean=bn.running_mean, running_var=bn.running_var, W2=lin2.weight, b2=lin2.bias)
        eps, momentum, steps = bn.eps, bn.momentum, bn.num_batches_tracked
    elif isinstance(classifier, dict):
        missing = [k for k in REID_KEYS if k not in classifier]
        if missing:
            raise ValueError(f"{what}: the classifier dict lacks {missing}; it holds {REID_KEYS} (and optionally 'eps', 'momentum', 'num_batches_tracked')")
        t = {k: classifier[k] for k in REID_KEYS}
        eps, momentum, steps = classifier.get("eps", 1e-5), classifier.get("momentum", 0.1), classifier.get("num_batches_tracked")
    else:
        raise ValueError(f"{what}: classifier must be a ReIDLoss or a dict of {REID_KEYS}, got {type(classifier).__name__}")
    for k, v in t.items():
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32:
            raise ValueError(f"{what}: classifier tensor '{k}' must be a float32 tensor, got {v.dtype if isinstance(v, torch.Tensor) else type(v).__name__}")
    if t["W1"].dim() != 2 or t["W1"].shape[0] != t["W1"].shape[1] or t["W2"].dim() != 2:
        raise ValueError(f"{what}: W1 must be [D, D] and W2 [K, D], got {tuple(t['W1'].shape)} and {tuple(t['W2'].shape)}")
    D, K = int(t["W1"].shape[0]), int(t["W2"].shape[0])
    for k, shape in (("gamma", (D,)), ("beta", (D,)), ("running_mean", (D,)), ("running_var", (D,)), ("W2", (K, D)), ("b2", (K,))):
        if tuple(t[k].shape) != shape:
            raise ValueError(f"{what}: classifier tensor '{k}' must be {list(shape)} beside W1 [{D}, {D}], got {tuple(t[k].shape)}")
    if not (1 <= D <= MAX_EMB and 2 <= K <= MAX_TRACK_IDS):
        raise ValueError(f"{what}: D = {D}, K = {K} outside 1..{MAX_EMB}, 2..{MAX_TRACK_IDS}")
    return t, eps, momentum, steps


def _reid_targets(targets, N, H, W, K, stride, center, ignore_index, what):
    """reid_loss's targets: the list, the dict {"boxes", "ids", "count"} or the tuple (boxes, labels, count, ids), whose labels are not read
    -> (device or None, (boxes [N,Gmax,4] f64, ids [N,Gmax] i64, count [N] i32) as device tensors or numpy, Gmax)"""
    def row_ok(b, ident):                  # the row rule of include/centernet_gfx950.h; a box without identity is never a bad one
        with np.errstate(all="ignore"):
            c = (b[:, :2] + b[:, 2:] / 2.0) / float(stride)
            c = np.rint(c) if center == "round" else np.trunc(c)
            return (np.isfinite(b).all(axis=1) & (b[:, 2] >= 0) & (b[:, 3] >= 0) & (c[:, 0] >= 0) & (c[:, 0] <= W - 1) & (c[:, 1] >= 0) & (c[:, 1] <= H - 1) &
                    (ident >= 0) & (ident < K)) | (ident == ignore_index)

    return _read(targets, N, _t.IDS, 4, row_ok,
                 lambda ident: f"(id {ident}) cannot be a row on a {H} x {W} map with {K} identities at stride {stride}: non-finite, negative size, "
                               f"centre cell outside the map or id outside 0..{K - 1}", what)


def _reid_inputs(reid, targets, classifier, params, center, what, keep=False):
    """Everything one call reads, checked -> (shape (N, D, H, W), K, the seven tensors (detached, dense) by REID_KEYS, num_batches_tracked, device targets;
    keep: copies of the caller's own, see _on_device)"""
    _check_map(reid, "reid", "D", what)
    N, D, H, W = (int(v) for v in reid.shape)
    t, eps, momentum, steps = classifier
    if int(t["W1"].shape[0]) != D:
        raise ValueError(f"{what}: reid has {D} channels, the classifier expects {int(t['W1'].shape[0])}")
    K = int(t["W2"].shape[0])
    _check_sizes(N, 1, H, W, what)
    _gather.require_hip([reid] + list(t.values()), what)
    dev = reid.device
    for k, v in t.items():
        if v.device != dev:
            raise ValueError(f"{what}: reid on {dev}, classifier tensor '{k}' on {v.device}")
    g_dev, gts, _ = _reid_targets(targets, N, H, W, K, params.stride, center, params.ignore_index, what)
    return (N, D, H, W), K, {k: v.detach().contiguous() for k, v in t.items()}, steps, _on_device(g_dev, gts, N, dev, what, "reid", keep=keep)


def _reid_common(reid, shape, K, t, gts, params):
    N, D, H, W = shape
    return (reid.data_ptr(), *reid.stride(), N, D, H, W, gts[0].data_ptr(), gts[1].data_ptr(), gts[2].data_ptr(), int(gts[0].shape[1]),
            *(t[k].data_ptr() for k in REID_KEYS), K, ctypes.byref(params))


def _run_reid(reid, shape, K, t, gts, params):
    """The one call -> (per_row [N, Gmax] f64, total [1] f64, counts [4] i32 (rows, top-1 hits, skipped, stepped), new statistics [2, D] f32)"""
    N, D, H, W = shape
    dev = reid.device
    Gmax = int(gts[0].shape[1])
    with torch.cuda.device(dev):
        per_row = torch.zeros((N, Gmax), dtype=torch.float64, device=dev) if N == 0 else torch.empty((N, Gmax), dtype=torch.float64, device=dev)
        total = torch.zeros((1,), dtype=torch.float64, device=dev)
        counts = torch.zeros((4,), dtype=torch.int32, device=dev)
        new_stats = torch.stack([t["running_mean"], t["running_var"]])
        if N:
            _call("cnl_reid_loss_f64", ("cnl_reid_loss_workspace_bytes", N, Gmax, D), dev, *_reid_common(reid, shape, K, t, gts, params),
                  per_row.data_ptr(), total.data_ptr(), counts.data_ptr(), new_stats.data_ptr())
    return per_row, total, counts, new_stats


def _run_reid_grad(reid, shape, K, t, gts, params, scale, want):
    """The one call.  scale: None (1) or a float64 device tensor [1]; want: six flags by REID_WANT -> (six gradients or None, skipped [1] i32)"""
    N, D, H, W = shape
    dev = reid.device
    with torch.cuda.device(dev):
        empty = torch.zeros if N == 0 else torch.empty
        grads = [(_like(reid) if N else torch.zeros_like(reid)) if want[0] else None]
        grads += [empty(tuple(t[k].shape), dtype=torch.float32, device=dev) if w else None for k, w in zip(REID_WANT[1:], want[1:])]
        skipped = torch.zeros((1,), dtype=torch.int32, device=dev)
        if N:
            _call("cnl_reid_loss_grad_f32", ("cnl_reid_loss_grad_workspace_bytes", N, int(gts[0].shape[1]), D), dev,
                  *_reid_common(reid, shape, K, t, gts, params), _ptr(scale), *_map_args(grads[0]), *(_ptr(g) for g in grads[1:]), skipped.data_ptr())
    return grads, skipped


def _reid_result(per_row, total, counts):
    return {"reid": total[0], "per_row": per_row, "num_rows": counts[0], "correct": counts[1], "skipped": counts[2]}


def _step_statistics(t_live, steps, new_stats, counts):
    """The BatchNorm buffers after a training call (t_live: the classifier's own tensors, written in place on the device)."""
    with torch.no_grad():
        t_live["running_mean"].copy_(new_stats[0])
        t_live["running_var"].copy_(new_stats[1])
        if isinstance(steps, torch.Tensor):
            steps += counts[3].to(steps.dtype)


def reid_loss(reid, targets, classifier, training=True, stride=4, center="trunc", padded_rows=False, ignore_index=-1, update_stats=True):
    """The reference's EmbeddingHead.compute_loss on the device.  reid [N, D, H, W] fp32 as get_encoded_outputs returns it (any strides).  targets:
    detection_loss's forms plus the identities: a list of per-image {"boxes" [m, 4] x y w h in input pixels, "ids" [m]} (checked on the host: a box that
    cannot be a row raises ValueError), or padded device tensors as a dict {"boxes" [N, Gmax, 4] float64, "ids" [N, Gmax] int64, "count" [N] int32} or the
    tuple (boxes, labels, count, ids) (a bad row is skipped and counted in "skipped").  classifier: a ReIDLoss, or a dict of the seven fp32 tensors
    W1 [D, D], gamma, beta, running_mean, running_var [D], W2 [K, D], b2 [K] (optionally "eps", "momentum", "num_batches_tracked").
    center: "trunc" (the reference's cell) or "round" (the cell the decode reads).  padded_rows: the slots beyond count enter the BatchNorm statistics at
    cell (0, 0), as the reference's zero-padded boxes do.  ignore_index: the identity of a box without one (dropped silently).  training: batch
    statistics, and with update_stats the running statistics and num_batches_tracked make their step in place; else the running statistics are used.
    -> {"reid": 0-dim float64, "per_row" [N, Gmax] float64 (0 for rows not in the loss), "num_rows", "correct" (top-1 hits), "skipped": 0-dim int32}.
    Training with fewer than two rows in the statistics gives 0 and leaves the buffers alone.  No synchronisation."""
    what = "reid_loss"
    cls = _classifier(classifier, what)
    params = reid_params(training, stride, center, padded_rows, ignore_index, cls[1], cls[2], what)
    shape, K, t, steps, gts = _reid_inputs(reid, targets, cls, params, center, what)
    per_row, total, counts, new_stats = _run_reid(reid.detach(), shape, K, t, gts, params)
    if training and update_stats:
        _step_statistics(cls[0], steps, new_stats, counts)
    return _reid_result(per_row, total, counts)


def reid_loss_grad(reid, targets, classifier, training=True, stride=4, center="trunc", padded_rows=False, ignore_index=-1, scale=1.0, want=REID_WANT):
    """The gradient of scale * reid_loss(...)["reid"] with respect to the map and the five trainable classifier tensors, analytic, float64 rounded once to
    fp32 (the rule: include/centernet_gfx950.h).  scale: a Python number or a 0-dim / 1-element float64 tensor on the device (read there).  want: which
    gradients to compute, a subset of ("reid", "W1", "gamma", "beta", "W2", "b2").
    -> {"reid_grad" (the map's shape; its strides when it is dense, else contiguous; exactly 0 wherever no row reads), "W1_grad", "gamma_grad",
    "beta_grad", "W2_grad", "b2_grad" (None when not wanted), "skipped": 0-dim int32}.  The running statistics are never touched.  One call of
    cnl_reid_loss_grad_f32, no synchronisation, no atomics: the same bits on every run."""
    what = "reid_loss_grad"
    want = _check_want(want, REID_WANT, what)
    cls = _classifier(classifier, what)
    params = reid_params(training, stride, center, padded_rows, ignore_index, cls[1], cls[2], what)
    _check_map(reid, "reid", "D", what)
    s = _scale(scale, "scale", reid.device, what)
    shape, K, t, _, gts = _reid_inputs(reid, targets, cls, params, center, what)
    grads, skipped = _run_reid_grad(reid.detach(), shape, K, t, gts, params, _scale_arg((s,), reid.device), want)
    out = {f"{k}_grad": g for k, g in zip(REID_WANT, grads)}
    out["skipped"] = skipped[0]
    return out


class _ReIDLossFunction(torch.autograd.Function):
    """reid_loss with the backward of cnl_reid_loss_grad_f32: one call forward, one call backward."""

    @staticmethod
    def forward(ctx, reid, W1, gamma, beta, W2, b2, running, gts, params, shape, K):
        t = dict(W1=W1, gamma=gamma, beta=beta, running_mean=running[0], running_var=running[1], W2=W2, b2=b2)
        t = {k: v.detach().contiguous() for k, v in t.items()}
        per_row, total, counts, new_stats = _run_reid(reid.detach(), shape, K, t, gts, params)
        ctx.save_for_backward(reid, W1, gamma, beta, W2, b2, *gts)
        # (the running statistics are not saved tensors: a training step writes them in place after this call, and only an eval-mode backward reads them)
        ctx.running, ctx.params, ctx.shape, ctx.K = running, params, shape, K
        ctx.mark_non_differentiable(per_row, counts, new_stats)
        return total, per_row, counts, new_stats

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_total, _g_rows, _g_counts, _g_stats):
        reid, W1, gamma, beta, W2, b2, *gts = ctx.saved_tensors
        t = dict(W1=W1, gamma=gamma, beta=beta, running_mean=ctx.running[0], running_var=ctx.running[1], W2=W2, b2=b2)
        t = {k: v.detach().contiguous() for k, v in t.items()}
        scale = g_total.detach().to(torch.float64).reshape(1)                 # on the device: no synchronisation
        grads, _ = _run_reid_grad(reid.detach(), ctx.shape, ctx.K, t, tuple(gts), ctx.params, scale, tuple(ctx.needs_input_grad[:6]))
        return (*grads, None, None, None, None, None)


class ReIDLoss(torch.nn.Module):
    """The tracking model's re-ID criterion: the reference's EmbeddingHead classifier and loss (models/fairmot.py:20-61).  `classifier` is the reference's
    nn.Sequential(Linear(D, D, bias=False), BatchNorm1d(D), ReLU, Linear(D, K)) with torch's initialisation, so state_dict() has the reference's keys
    classifier.{0,1,3}.* (formats.reid_classifier_state takes them out of a reference checkpoint).  The Sequential owns the parameters and buffers; its
    own forward is never used.  ReIDLoss(...)(outputs, targets) -> reid_loss's dict, where "reid" carries a grad_fn when the map or a parameter requires
    grad (one call forward, one call backward, only for the inputs that need a gradient; the backward reads its own copy of padded device targets, so
    the caller may refill them before it runs).  .train() / .eval() pick batch or running statistics; a training call steps running_mean, running_var
    and num_batches_tracked.  loss_weight is NOT applied to the value (TrackingLoss applies it to the total).  `settings`: stride, center, padded_rows,
    ignore_index of reid_loss."""

    def __init__(self, emb_dim=64, max_track_ids=1000, loss_weight=1.0, **settings):
        super().__init__()
        unknown = set(settings) - {"stride", "center", "padded_rows", "ignore_index"}
        if unknown:
            raise ValueError(f"ReIDLoss: unknown settings {sorted(unknown)}; stride, center, padded_rows and ignore_index are understood")
        for name, v, hi in (("emb_dim", emb_dim, MAX_EMB), ("max_track_ids", max_track_ids, MAX_TRACK_IDS)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not (2 if name == "max_track_ids" else 1) <= v <= hi:
                raise ValueError(f"ReIDLoss: {name} must be an int up to {hi}, got {v!r}")
        reid_params(what="ReIDLoss", **settings)
        self.emb_dim, self.max_track_ids = int(emb_dim), int(max_track_ids)
        self.loss_weight = _number(loss_weight, "loss_weight", "ReIDLoss")
        self.settings = settings
        self.classifier = torch.nn.Sequential(torch.nn.Linear(self.emb_dim, self.emb_dim, bias=False), torch.nn.BatchNorm1d(self.emb_dim),
                                              torch.nn.ReLU(inplace=True), torch.nn.Linear(self.emb_dim, self.max_track_ids))

    def extra_repr(self):
        return ", ".join([f"loss_weight={self.loss_weight!r}"] + [f"{k}={v!r}" for k, v in self.settings.items()])

    def forward(self, outputs, targets):
        what = "ReIDLoss"
        (reid,) = _outputs(outputs, ("reid",), what)
        cls = _classifier(self, what)
        t, _, _, steps = cls
        trainable = (reid, t["W1"], t["gamma"], t["beta"], t["W2"], t["b2"])
        needs = torch.is_grad_enabled() and any(isinstance(v, torch.Tensor) and v.requires_grad for v in trainable)
        if not needs:
            return reid_loss(reid, targets, self, training=self.training, **self.settings)
        params = reid_params(self.training, bn_eps=cls[1], momentum=cls[2], what=what, **self.settings)
        shape, K, _, _, gts = _reid_inputs(reid, targets, cls, params, self.settings.get("center", "trunc"), what, keep=True)
        total, per_row, counts, new_stats = _ReIDLossFunction.apply(*trainable, (t["running_mean"], t["running_var"]), gts, params, shape, K)
        if self.training:
            _step_statistics(t, steps, new_stats, counts)
        return _reid_result(per_row, total, counts)


class TrackingLoss(torch.nn.Module):
    """The criterion of a tracking model's training step: TrackingLoss(detection_settings, reid_loss_module)(outputs, targets) ->
    {"heatmap", "box_2d", "reid", "total", "per_image", "skipped", "per_row", "num_rows", "correct", "reid_skipped"} with
    total = DetectionLoss's total + loss_weight * reid; "heatmap", "box_2d", "per_image" and "skipped" are DetectionLoss's, bit for bit.  outputs: the
    dict of get_encoded_outputs with "heatmap", "box_2d" and "reid"; targets: a list of per-image {"boxes", "labels", "ids"}, the dict of padded device
    tensors {"boxes", "labels", "ids", "count"} or the tuple (boxes, labels, count, ids).  ignore_reid=True at call time leaves the re-ID loss out, as the
    reference's validation step does (models/fairmot.py:89): "total" is the detection total and "reid" is 0."""

    def __init__(self, detection_settings, reid_loss_module):
        super().__init__()
        if not isinstance(reid_loss_module, ReIDLoss):
            raise ValueError(f"TrackingLoss: reid_loss_module must be a ReIDLoss, got {type(reid_loss_module).__name__}")
        self.detection = DetectionLoss(**dict(detection_settings or {}))
        self.reid = reid_loss_module

    def forward(self, outputs, targets, ignore_reid=False):
        det_targets = tuple(targets[:3]) if not isinstance(targets, dict) and _t.is_padded(targets, (4,)) else targets
        out = dict(self.detection(outputs, det_targets))
        if ignore_reid:
            out["reid"] = torch.zeros((), dtype=torch.float64, device=out["total"].device)
            return out
        res = self.reid(outputs, targets)
        out["reid_skipped"] = res.pop("skipped")
        out.update(res)
        out["total"] = out["total"] + self.reid.loss_weight * res["reid"]
        return out
