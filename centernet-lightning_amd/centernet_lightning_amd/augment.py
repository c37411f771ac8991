"""Training augmentation of a batch on the GPU: crop, flip, colour, cutout and mosaic in one call, from the frames and targets of a batch
to N network-input canvases and the padded target dict DetectionLoss / TrackingLoss take.

The reference augments on the host, one image at a time in DataLoader workers (datasets/builder.py::parse_transforms: an albumentations
Compose of HorizontalFlip, RandomResizedCrop, ColorJitter and, for tracking, Cutout, with BboxParams(min_area=1) and a numpy collate), and
declares a batch-level Mosaic (datasets/transforms.py) whose body is `pass`.  Here all randomness is drawn on the host into a PLAN
(sample_augment -> AugmentPlan: pure numpy, no device, no library), and the device work is a deterministic function of that plan
(augment_batch: one pinned upload, two launches — cnl_augment_u8 and cnl_augment_boxes_f64 of csrc/augment.hip — no device sync, no per-box
Python).  The rules are stated in include/centernet_gfx950.h and restated in numpy by tests/augment_ref.py.

Two stated deviations from albumentations' ColorJitter, so that the whole jitter is ONE integer 3 x 4 matrix per pixel and needs no reduction
over the image (what DALI's ColorTwist does): contrast pivots on the constant `contrast_center` instead of the image's mean, and hue turns in
YIQ instead of HSV.  Rotation, shear (Affine) and RandomCrop / SmallestMaxSize are warp.py's (a rule and a kernel of their own; this module's
behaviour is unchanged); MixUp and YUV sources are out of scope.
"""
import dataclasses
import math

import numpy as np
import torch

from . import _frames, _gather, _lib, _targets
from .loss import MAX_PER_IMAGE, MAX_SIDE

MAX_PLACE, MAX_HOLES = 4, 16                      # placement and hole slots per canvas (csrc/augment.hip)
Q12 = 4096
MAX_ENTRY, MAX_OFFSET = 32767, 1 << 21            # bounds of the nine matrix entries / the three offsets (already times 4096)
IDENTITY_Q12 = np.array([Q12, 0, 0, 0, Q12, 0, 0, 0, Q12, 0, 0, 0], dtype=np.int32)
BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3

_COLUMNS = _targets.columns(("labels", "int64"), ("ids", "int64"))          # of the targets; the ids are optional
_LUMA = np.array([0.299, 0.587, 0.114], dtype=np.float64)
_YIQ = np.array([[0.299, 0.587, 0.114], [0.5959, -0.2746, -0.3213], [0.2115, -0.5227, 0.3112]], dtype=np.float64)


def colour_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, order=(BRIGHTNESS, CONTRAST, SATURATION, HUE), contrast_center=128):
    """The four ColorJitter FACTORS (1, 1, 1 and 0 turns change nothing), applied in `order`, composed in float64 into one affine colour
    matrix and quantised with rint to Q12 -> int32 [12]: entries [3c + k] weigh source channel k in channel c, [9 + c] is channel c's
    offset times 4096.  Brightness is b I; contrast c I with offset (1 - c) contrast_center; saturation s I + (1 - s) 1 w^T with
    w = (0.299, 0.587, 0.114); hue T^-1 Rot(2 pi h) T with the YIQ matrix T.  Values outside +-32767 / +-2^21 are clipped."""
    M, o = np.eye(3), np.zeros(3)
    for op in order:
        a = np.zeros(3)
        if op == BRIGHTNESS:
            A = float(brightness) * np.eye(3)
        elif op == CONTRAST:
            A = float(contrast) * np.eye(3)
            a = (1.0 - float(contrast)) * float(contrast_center) * np.ones(3)
        elif op == SATURATION:
            A = float(saturation) * np.eye(3) + (1.0 - float(saturation)) * np.outer(np.ones(3), _LUMA)
        elif op == HUE:
            t = 2.0 * math.pi * float(hue)
            rot = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(t), -math.sin(t)], [0.0, math.sin(t), math.cos(t)]])
            A = np.linalg.inv(_YIQ) @ rot @ _YIQ
        else:
            raise ValueError(f"order names the operations 0..3, got {op!r}")
        M, o = A @ M, A @ o + a
    q = np.empty(12, dtype=np.int32)
    q[:9] = np.clip(np.rint(M * Q12), -MAX_ENTRY, MAX_ENTRY).reshape(9)
    q[9:] = np.clip(np.rint(o * Q12), -MAX_OFFSET, MAX_OFFSET)
    return q


_HEAD = (("n_place", np.int32, ()), ("frame", np.int32, (MAX_PLACE,)), ("window", np.int32, (MAX_PLACE, 4)), ("dest", np.int32, (MAX_PLACE, 4)))
_TAIL = (("colour", np.int32, (MAX_PLACE, 12)), ("holes", np.int32, (MAX_HOLES, 4)))


class _Plan:
    """What AugmentPlan and warp.WarpPlan share.  A plan class is a dataclass of sizes, height, width and the arrays of its _FIELDS
    [(name, dtype, shape of one canvas)], and names what a slot starts as where that is not zero (_INITIAL), the int64 words of one
    placement record (RECORD_WORDS) and its two library entry points (IMAGE_ENTRY, BOXES_ENTRY)."""

    @classmethod
    def empty(cls, sizes, height, width, N=None):
        """A plan of N canvases (default: one per frame) with no live placement yet, identity maps and colours and no holes."""
        sizes = [(int(h), int(w)) for (h, w) in sizes]
        N = len(sizes) if N is None else int(N)
        arrays = {name: np.zeros((N,) + shape, dtype) for name, dtype, shape in cls._FIELDS}
        for name, value in cls._INITIAL.items():
            arrays[name][...] = value
        return cls(sizes, int(height), int(width), **arrays)

    def __len__(self):
        return int(self.n_place.shape[0])

    @property
    def max_place(self):
        return int(self.n_place.max()) if len(self) else 1

    def single(self, n):
        """The plan of canvas n alone (same frames)."""
        s = slice(n, n + 1)
        return type(self)(self.sizes, self.height, self.width, **{name: getattr(self, name)[s].copy() for name, _, _ in self._FIELDS})

    def check(self):
        """Every bound of the plan; ValueError naming the canvas and placement otherwise.  -> self"""
        N, H, W, F = len(self), self.height, self.width, len(self.sizes)
        if not (1 <= H <= MAX_SIDE and 4 <= W <= MAX_SIDE and W % 4 == 0):
            raise ValueError(f"plan: canvas {H} x {W} needs sides of at most {MAX_SIDE} and a width that is a positive multiple of 4")
        for name, dtype, shape in self._FIELDS:
            a = getattr(self, name)
            if not isinstance(a, np.ndarray) or a.dtype != dtype or a.shape != (N,) + shape:
                raise ValueError(f"plan: {name} must be {'an' if dtype != np.float64 else 'a'} {np.dtype(dtype).name} array of shape {[N] + list(shape)}")
        for (h, w) in self.sizes:
            if h < 1 or w < 1:
                raise ValueError(f"plan: frame size {h} x {w}")
        # vectorised over all slots (a per-slot Python loop costs more than both launches); each rule names its first offender
        k = self.n_place.astype(np.int64)
        bad = np.nonzero((k < 1) | (k > MAX_PLACE))[0]
        if bad.size:
            raise ValueError(f"plan: canvas {int(bad[0])} has {int(k[bad[0]])} placements; 1..{MAX_PLACE} are supported")
        live = np.arange(MAX_PLACE)[None, :] < k[:, None]

        def first(mask):
            at = np.argwhere(mask & live)
            return (int(at[0, 0]), int(at[0, 1])) if at.size else None

        frame = self.frame.astype(np.int64)
        at = first((frame < 0) | (frame >= F))
        if at:
            raise ValueError(f"plan: canvas {at[0]} placement {at[1]}: frame {int(frame[at])} outside 0..{F - 1}")
        size = np.asarray(self.sizes, dtype=np.int64).reshape(F, 2)[np.where(live, frame, 0)]            # [N, 4, (h, w)]
        x0, y0, w, h = (self.window[..., i].astype(np.int64) for i in range(4))
        at = first((w < 1) | (h < 1) | (x0 < 0) | (y0 < 0) | (x0 + w > size[..., 1]) | (y0 + h > size[..., 0]))
        if at:
            raise ValueError(f"plan: canvas {at[0]} placement {at[1]}: window (x0 {x0[at]}, y0 {y0[at]}, w {w[at]}, h {h[at]}) is empty or leaves its "
                             f"{size[at][0]} x {size[at][1]} frame")
        dx0, dy0, dw, dh = (self.dest[..., i].astype(np.int64) for i in range(4))
        at = first((dw < 4) | (dh < 1) | (dx0 < 0) | (dy0 < 0) | (dx0 % 4 != 0) | (dw % 4 != 0) | (dx0 + dw > W) | (dy0 + dh > H))
        if at:
            raise ValueError(f"plan: canvas {at[0]} placement {at[1]}: rectangle (dx0 {dx0[at]}, dy0 {dy0[at]}, dw {dw[at]}, dh {dh[at]}) needs dx0 and dw "
                             f"multiples of 4, dh >= 1, inside the {H} x {W} canvas")
        self._check_geometry(first)
        c = np.abs(self.colour.astype(np.int64))
        at = first((c[..., :9].max(axis=-1) > MAX_ENTRY) | (c[..., 9:].max(axis=-1) > MAX_OFFSET))
        if at:
            raise ValueError(f"plan: canvas {at[0]} placement {at[1]}: colour matrix outside +-{MAX_ENTRY} (entries) / +-{MAX_OFFSET} (offsets)")
        for p in range(1, MAX_PLACE):
            for q in range(p):
                both = live[:, p] & (dx0[:, p] < dx0[:, q] + dw[:, q]) & (dx0[:, q] < dx0[:, p] + dw[:, p]) & \
                    (dy0[:, p] < dy0[:, q] + dh[:, q]) & (dy0[:, q] < dy0[:, p] + dh[:, p])
                if both.any():
                    raise ValueError(f"plan: canvas {int(np.nonzero(both)[0][0])} placement {p}: its rectangle overlaps placement {q}'s")
        hl = self.holes.astype(np.int64)
        at = np.argwhere((hl[..., 2] < 0) | (hl[..., 3] < 0) | (hl[..., 2:] > MAX_SIDE).any(axis=-1) | (np.abs(hl[..., :2]) > MAX_SIDE).any(axis=-1))
        if at.size:
            n, j = int(at[0, 0]), int(at[0, 1])
            raise ValueError(f"plan: canvas {n} hole {j} = {hl[n, j].tolist()} needs 0 <= w, h <= {MAX_SIDE} and |x0|, |y0| <= {MAX_SIDE}")
        return self

    def pack(self, places, holes, n_place):
        """Fill the upload's views: places [N * 4, 2 * RECORD_WORDS] int32 (the placement records, zeroed), holes [N * 16, 4] int32, n_place [N].
        -> the records as [N, 4, 2 * RECORD_WORDS], for the words a plan class adds."""
        N = len(self)
        rec = places.reshape(N, MAX_PLACE, 2 * self.RECORD_WORDS)
        rec[:, :, 0] = self.frame
        rec[:, :, 1:5] = self.window
        rec[:, :, 5:9] = self.dest
        rec[:, :, 10:22] = self.colour
        holes.reshape(N, MAX_HOLES, 4)[:] = self.holes
        n_place[:] = self.n_place
        return rec


@dataclasses.dataclass
class AugmentPlan(_Plan):
    """What augment_batch does to a batch of F frames, as numpy arrays (N canvases; slot p of canvas n is live when p < n_place[n]):
    sizes [(h, w)] of the F frames; n_place [N] int32 (1..4); frame [N, 4] int32; window [N, 4, 4] int32 (x0, y0, w, h) in the frame;
    dest [N, 4, 4] int32 (dx0, dy0, dw, dh) in the canvas; flip [N, 4] int32; colour [N, 4, 12] int32 (colour_matrix); holes
    [N, 16, 4] int32 (x0, y0, w, h) in canvas pixels, w == 0 marking a dead slot.  The plan is the interface: build one by hand with
    AugmentPlan.empty and fill its arrays, then check()."""
    sizes: list
    height: int
    width: int
    n_place: np.ndarray
    frame: np.ndarray
    window: np.ndarray
    dest: np.ndarray
    flip: np.ndarray
    colour: np.ndarray
    holes: np.ndarray

    _FIELDS = _HEAD + (("flip", np.int32, (MAX_PLACE,)),) + _TAIL
    _INITIAL = {"colour": IDENTITY_Q12}
    RECORD_WORDS, IMAGE_ENTRY, BOXES_ENTRY = 12, "cnl_augment_u8", "cnl_augment_boxes_f64"          # cnl_augment_placement: 96 bytes

    def _check_geometry(self, first):
        at = first((self.flip != 0) & (self.flip != 1))
        if at:
            raise ValueError(f"plan: canvas {at[0]} placement {at[1]}: flip must be 0 or 1")

    def pack(self, places, holes, n_place):
        super().pack(places, holes, n_place)[:, :, 9] = self.flip


# ----------------------------------------------------------------------------- drawing a plan
def _pair(v, name, low=None):
    try:
        a, b = (float(x) for x in v)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a pair of numbers, got {v!r}") from None
    if not (math.isfinite(a) and math.isfinite(b)) or a > b or (low is not None and a <= low):
        raise ValueError(f"{name} must be an increasing pair{'' if low is None else f' above {low}'}, got {v!r}")
    return a, b


def _factor_range(v, name, hue=False):
    """torchvision's ColorJitter ranges: a number v -> [max(0, 1 - v), 1 + v] (hue: [-v, v]); a pair is taken as it is.  None: no jitter."""
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        v = float(v)
        if not math.isfinite(v) or v < 0 or (hue and v > 0.5):
            raise ValueError(f"{name} must be >= 0{' and <= 0.5' if hue else ''}, got {v!r}")
        if v == 0:
            return None
        return (-v, v) if hue else (max(0.0, 1.0 - v), 1.0 + v)
    lo, hi = _pair(v, name)
    if (hue and (lo < -0.5 or hi > 0.5)) or (not hue and lo < 0):
        raise ValueError(f"{name} range {v!r} outside {'[-0.5, 0.5]' if hue else '[0, inf)'}")
    return lo, hi


def _window(rng, fh, fw, dw, dh, height, width, scale, ratio):
    """torchvision's / albumentations' RandomResizedCrop window of an fh x fw frame for a dw x dh rectangle of a height x width canvas:
    ten tries of an area fraction uniform in `scale` and an aspect r log-uniform in `ratio`, the window's own aspect being
    w / h = r (dw height) / (dh width) so that a mosaic quadrant sees the distortion range of a whole canvas; then the centre crop."""
    k = (dw * height) / (dh * width)
    area = fh * fw
    log_lo, log_hi = math.log(ratio[0]), math.log(ratio[1])
    for _ in range(10):
        target = area * rng.uniform(scale[0], scale[1])
        a = math.exp(rng.uniform(log_lo, log_hi)) * k
        w, h = int(round(math.sqrt(target * a))), int(round(math.sqrt(target / a)))
        if 0 < w <= fw and 0 < h <= fh:
            y0 = int(rng.integers(0, fh - h + 1))
            x0 = int(rng.integers(0, fw - w + 1))
            return x0, y0, w, h
    in_ratio, lo, hi = fw / fh, ratio[0] * k, ratio[1] * k
    if in_ratio < lo:
        w, h = fw, int(round(fw / lo))
    elif in_ratio > hi:
        w, h = int(round(fh * hi)), fh
    else:
        w, h = fw, fh
    w, h = min(max(w, 1), fw), min(max(h, 1), fh)
    return (fw - w) // 2, (fh - h) // 2, w, h


def sample_augment(sizes, height, width, rng, *, mosaic=0.0, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip=0.5, brightness=0.0, contrast=0.0,
                   saturation=0.0, hue=0.0, contrast_center=128, cutout=None, crop=True) -> AugmentPlan:
    """Draw the plan of one batch: N = F canvases of height x width (width % 4 == 0, sides <= loss.MAX_SIDE) from F frames of `sizes`
    [(h, w)], with `rng` a numpy.random.Generator.  Pure host arithmetic: no device, no library.

    Canvas n has one placement (frame n stretched over the whole canvas, as RandomResizedCrop does; crop=False takes the whole frame,
    which is A.Resize) or, with probability `mosaic`, four: frame n and three other frames of the batch (without replacement; with
    replacement when F < 4) in the quadrants top-left, top-right, bottom-left, bottom-right around a centre drawn uniformly in the
    middle half of the canvas, its x rounded to a multiple of 4.  Every placement draws its own window (RandomResizedCrop's rule with
    `scale` and `ratio`, see _window), flip bit (probability `flip`) and colour: the four ColorJitter factors as torchvision draws them
    (a number v: [max(0, 1 - v), 1 + v], hue [-v, v] turns; or a (low, high) pair), composed in a random order into one Q12 matrix
    (colour_matrix).  Contrast pivots on `contrast_center` and hue turns in YIQ: the two stated deviations from albumentations.
    cutout=(num_holes, max_h, max_w), the reference's Cutout parameters: num_holes (<= 16) rectangles of max_h x max_w per canvas,
    centred on uniformly drawn canvas pixels, so they may overlap each other and the canvas edge."""
    sizes = [(int(h), int(w)) for (h, w) in sizes]
    F = len(sizes)
    height, width = int(height), int(width)
    if not (1 <= height <= MAX_SIDE and 4 <= width <= MAX_SIDE and width % 4 == 0):
        raise ValueError(f"canvas {height} x {width} needs sides of at most {MAX_SIDE} and a width that is a positive multiple of 4")
    if F < 1 or any(h < 1 or w < 1 for (h, w) in sizes):
        raise ValueError(f"sizes must be the (h, w) >= 1 of at least one frame, got {sizes!r}")
    for name, v in (("mosaic", mosaic), ("flip", flip)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
            raise ValueError(f"{name} must be a probability, got {v!r}")
    if mosaic > 0 and (width < 8 or height < 2):
        raise ValueError(f"a mosaic needs a canvas of at least 2 x 8, got {height} x {width}")
    scale, ratio = _pair(scale, "scale", low=0.0), _pair(ratio, "ratio", low=0.0)
    ranges = [_factor_range(brightness, "brightness"), _factor_range(contrast, "contrast"), _factor_range(saturation, "saturation"),
              _factor_range(hue, "hue", hue=True)]
    if cutout is not None:
        try:
            num_holes, max_h, max_w = (int(v) for v in cutout)
        except (TypeError, ValueError):
            raise ValueError(f"cutout must be (num_holes, max_h, max_w), got {cutout!r}") from None
        if not (0 <= num_holes <= MAX_HOLES and 1 <= max_h <= MAX_SIDE and 1 <= max_w <= MAX_SIDE):
            raise ValueError(f"cutout = {cutout!r}: at most {MAX_HOLES} holes of 1..{MAX_SIDE} pixels a side")

    plan = AugmentPlan.empty(sizes, height, width)
    for n in range(F):
        if mosaic > 0 and rng.random() < mosaic:
            if F >= 4:
                others = rng.choice(np.array([f for f in range(F) if f != n]), size=3, replace=False)
            else:
                others = rng.integers(0, F, size=3)
            cx = min(max(4 * int(round(rng.uniform(width / 4, 3 * width / 4) / 4)), 4), width - 4)
            cy = min(max(int(round(rng.uniform(height / 4, 3 * height / 4))), 1), height - 1)
            frames = [n] + [int(f) for f in others]
            rects = [(0, 0, cx, cy), (cx, 0, width - cx, cy), (0, cy, cx, height - cy), (cx, cy, width - cx, height - cy)]
        else:
            frames, rects = [n], [(0, 0, width, height)]
        plan.n_place[n] = len(frames)
        for p, (f, (dx0, dy0, dw, dh)) in enumerate(zip(frames, rects)):
            fh, fw = sizes[f]
            plan.frame[n, p] = f
            plan.dest[n, p] = (dx0, dy0, dw, dh)
            plan.window[n, p] = _window(rng, fh, fw, dw, dh, height, width, scale, ratio) if crop else (0, 0, fw, fh)
            plan.flip[n, p] = int(flip > 0 and rng.random() < flip)
            if any(r is not None for r in ranges):
                b, c, s, h = (float(rng.uniform(*r)) if r is not None else neutral for r, neutral in zip(ranges, (1.0, 1.0, 1.0, 0.0)))
                plan.colour[n, p] = colour_matrix(b, c, s, h, order=[int(v) for v in rng.permutation(4)], contrast_center=contrast_center)
        if cutout is not None:
            for k in range(num_holes):
                y, x = int(rng.integers(0, height)), int(rng.integers(0, width))
                plan.holes[n, k] = (x - max_w // 2, y - max_h // 2, max_w, max_h)
    return plan


# ----------------------------------------------------------------------------- the call
def _out(out, name, dtype, shape, dev, what):
    """The caller's buffer for one result (out[name]: a contiguous tensor of exactly that type, shape and device), or a fresh one."""
    t = out.get(name) if out else None
    if t is None:
        return torch.empty(shape, device=dev, dtype=dtype)
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != dev or not t.is_contiguous():
        raise ValueError(f"{what}: out[{name!r}] must be a contiguous {dtype} tensor of shape {list(shape)} on {dev}")
    return t


def augment_batch(frames, plan, targets=None, fill=(0, 0, 0), hole_fill=(0, 0, 0), min_area=1.0, min_visibility=0.0, out=None):
    """frames: a sequence of uint8 [h_i, w_i, 3] tensors on one HIP device or one [F, h, w, 3] tensor (read in place where pixels are packed
    and rows do not overlap), of the sizes the plan was drawn for; plan: an AugmentPlan (checked here)
    -> (canvas [N, height, width, 3] uint8, targets or None), on the device.

    targets: a list of per-image {"boxes" [n, 4] (x, y, w, h in the frame's pixels, top-left origin: what detection_loss takes),
    "labels" [n][, "ids" [n]]}, padded and uploaded with the plan, or the padded device dict {"boxes" [F, Gmax, 4] f64, "labels"
    [F, Gmax] i64, "count" [F] i32[, "ids"]} / tuple (boxes, labels, count[, ids]), used in place.  Returned: {"boxes" [N, Gout, 4] f64 in
    canvas pixels, "labels", "count"[, "ids"]} with Gout = (most placements of a canvas) x Gmax, which goes straight into DetectionLoss /
    TrackingLoss.  A box is carried through its placement's geometry, clipped to the placement's rectangle and kept when its clipped area
    is >= min_area (the reference's BboxParams(min_area=1)) and >= min_visibility times its full area; kept boxes keep placement order,
    then source order; slots beyond count are zero.  Holes do not touch boxes.  out: optionally a dict of the caller's own buffers to
    write into, by the names "canvas", "boxes", "labels", "ids", "count" (a training loop reuses them; every element is written).
    One pinned upload, two launches, no device sync."""
    return _batch("augment_batch", AugmentPlan, (fill, hole_fill), frames, plan, targets, min_area, min_visibility, out)


def _batch(what, plan_type, fills, frames, plan, targets, min_area, min_visibility, out):
    """The host path of augment_batch and warp.warp_batch: a plan of `plan_type`, which names its record words, its image entry (which
    takes the colour words of `fills` in order) and its box entry."""
    if not isinstance(plan, plan_type):
        raise ValueError(f"{what}: plan must be {'an' if plan_type.__name__[0] in 'AEIOU' else 'a'} {plan_type.__name__}, got {type(plan).__name__}")
    plan.check()
    for name, v in (("min_area", min_area), ("min_visibility", min_visibility)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v):
            raise ValueError(f"{what}: {name} must be a number, got {v!r}")
    if out is not None and not isinstance(out, dict):
        raise ValueError(f"{what}: out must be a dict of tensors by name, got {type(out).__name__}")
    src = _frames.open_frames(frames, "rgb", what, copy=_frames.ROWS)
    dev, F, N = src.check_device(), len(src), len(plan)
    if src.C != 3:
        raise ValueError(f"{what}: frames must have 3 channels, got {src.C}")
    if list(src.sizes) != list(plan.sizes):
        raise ValueError(f"{what}: the plan was drawn for frames of sizes {plan.sizes}, got {list(src.sizes)}")
    words = [_frames.fill_word(f, 3) for f in fills]
    max_place = plan.max_place

    host = None                                  # a list of targets travels in the same upload; nothing in it is judged: the kernel's keep rule does that
    if targets is not None:
        if _targets.is_padded(targets, (3, 4)):
            t, Gmax, _ = _targets.read_padded(targets, F, _COLUMNS, what, optional=("ids",), device=dev)
        else:
            t, Gmax = _targets.read_list(targets, F, _COLUMNS, what, against="frames", optional=("ids",))
            host = t
        with_ids = t["ids"] is not None
        if max_place * Gmax > MAX_PER_IMAGE:
            raise ValueError(f"{what}: {max_place} placements x Gmax = {Gmax} boxes give Gout = {max_place * Gmax}; at most {MAX_PER_IMAGE} per image "
                             "are supported")

    # [F x 5] frame records | (pad to 16 bytes) | [N x 4 x RECORD_WORDS] placements | [N x 16 x 2] holes | n_place | boxes | labels | ids | count, in int64 words
    o_place = F * 5 + (F * 5) % 2
    o_holes = o_place + N * MAX_PLACE * plan.RECORD_WORDS
    o_np = o_holes + N * MAX_HOLES * 2
    o_boxes = o_np + (N + 1) // 2
    o_labels = o_ids = o_count = end = o_boxes
    if host is not None:
        o_labels = o_boxes + F * Gmax * 4
        o_ids = o_labels + F * Gmax
        o_count = o_ids + (F * Gmax if with_ids else 0)
        end = o_count + (F + 1) // 2
    windows = src.whole()
    buf = _gather.pack_records(windows, *src.records(windows), tail_words=end - F * 5)
    plan.pack(buf[o_place:o_holes].view(np.int32).reshape(N * MAX_PLACE, 2 * plan.RECORD_WORDS), buf[o_holes:o_np].view(np.int32).reshape(N * MAX_HOLES, 4),
              buf[o_np:o_boxes].view(np.int32)[:N])
    if host is not None:
        buf[o_boxes:o_labels].view(np.float64)[:] = t["boxes"].reshape(-1)
        buf[o_labels:o_ids] = t["labels"].reshape(-1)
        if with_ids:
            buf[o_ids:o_count] = t["ids"].reshape(-1)
        buf[o_count:end].view(np.int32)[:F] = t["count"]

    lib = _lib.load()
    with torch.cuda.device(dev):
        d = _gather.upload(buf, dev)
        canvas = _out(out, "canvas", torch.uint8, (N, plan.height, plan.width, 3), dev, what)
        stream = _lib.stream(dev)
        places, n_place = d[o_place:o_holes], d[o_np:o_boxes]
        _lib.check(getattr(lib, plan.IMAGE_ENTRY)(d.data_ptr(), F, places.data_ptr(), n_place.data_ptr(), max_place, d[o_holes:o_np].data_ptr(),
                                                  canvas.data_ptr(), N, plan.height, plan.width, *words, stream), plan.IMAGE_ENTRY)
        if targets is None:
            return canvas, None
        if host is not None:
            t = {"boxes": d[o_boxes:o_labels].view(torch.float64).view(F, Gmax, 4), "labels": d[o_labels:o_ids].view(F, Gmax),
                 "ids": d[o_ids:o_count].view(F, Gmax) if with_ids else None, "count": d[o_count:end].view(torch.int32)[:F]}
        Gout = max_place * Gmax
        res = {"boxes": _out(out, "boxes", torch.float64, (N, Gout, 4), dev, what), "labels": _out(out, "labels", torch.int64, (N, Gout), dev, what),
               "count": _out(out, "count", torch.int32, (N,), dev, what)}
        if with_ids:
            res["ids"] = _out(out, "ids", torch.int64, (N, Gout), dev, what)
        _lib.check(getattr(lib, plan.BOXES_ENTRY)(places.data_ptr(), n_place.data_ptr(), max_place, N, F, t["boxes"].data_ptr(), t["labels"].data_ptr(),
                                                  t["ids"].data_ptr() if with_ids else None, t["count"].data_ptr(), Gmax, res["boxes"].data_ptr(),
                                                  res["labels"].data_ptr(), res["ids"].data_ptr() if with_ids else None, res["count"].data_ptr(), Gout,
                                                  float(min_area), float(min_visibility), stream), plan.BOXES_ENTRY)
    return canvas, res


def _frame_sizes(frames):
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4:
            raise ValueError(f"expected a sequence of uint8 [h,w,3] frames or one [F,h,w,3] tensor, got {tuple(frames.shape)}")
        return [(int(frames.shape[1]), int(frames.shape[2]))] * int(frames.shape[0])
    sizes = []
    for f in frames:
        if not isinstance(f, torch.Tensor) or f.dim() != 3:
            raise ValueError("expected a sequence of uint8 [h,w,3] frames or one [F,h,w,3] tensor")
        sizes.append((int(f.shape[0]), int(f.shape[1])))
    return sizes


_IGNORED = ("Normalize",)                        # the stem and preprocess_uint8 normalise


def _config_items(transforms, unsupported):
    """The reference's YAML transform list in its forms ([{name, params}], `init_args` for `params`, or a {name: params} mapping)
    -> [(name, params dict)]."""
    if unsupported not in ("raise", "skip"):
        raise ValueError(f"unsupported must be 'raise' or 'skip', got {unsupported!r}")
    if isinstance(transforms, dict):
        return [(name, dict(params or {})) for name, params in transforms.items()]
    items = []
    for t in transforms or []:
        if not isinstance(t, dict) or "name" not in t:
            raise ValueError(f"a transform must be a mapping with 'name', got {t!r}")
        items.append((t["name"], dict(t.get("params", t.get("init_args")) or {})))
    return items


def _read_common(name, params, settings, size, resized):
    """One transform that TrainAugment and warp.TrainWarp read alike, into `settings` (and `size`, the canvas it names; `resized`: what crop
    is for a RandomResizedCrop) -> whether it was one."""
    if name == "HorizontalFlip":
        settings["flip"] = float(params.get("p", 0.5))
    elif name in ("RandomResizedCrop", "Resize"):
        size.clear()
        size.update({k: int(params[k]) for k in ("height", "width") if k in params})
        settings["crop"] = resized if name == "RandomResizedCrop" else False
        if name == "RandomResizedCrop":
            settings["scale"] = tuple(params.get("scale", (0.08, 1.0)))
            settings["ratio"] = tuple(params.get("ratio", (3 / 4, 4 / 3)))
    elif name == "ColorJitter":
        for k in ("brightness", "contrast", "saturation", "hue"):
            v = params.get(k, 0.0)
            settings[k] = tuple(v) if isinstance(v, (list, tuple)) else v
    elif name == "Cutout":
        settings["cutout"] = (int(params.get("num_holes", 8)), int(params.get("max_h_size", 8)), int(params.get("max_w_size", 8)))
    elif name not in _IGNORED:
        return False
    return True


class _Transform:
    """What TrainAugment and warp.TrainWarp share: the training transform of a run, callable as (frames, targets) -> (canvas, targets).  It owns
    a numpy Generator (`seed`); every call draws a fresh plan with its sampler (kept as .last_plan) and runs its batch call.  A transform
    class names its sampler and the settings that takes (_sample, _SETTINGS), its batch call (_run), what crop is for a RandomResizedCrop
    (_RESIZED), the transforms that name the canvas size and the ones it reads (_SIZED, _SUPPORTED, for the messages) and how it reads a
    transform _read_common does not know (_read_other); its own __init__ states which colours its batch call takes."""
    _RESIZED = True

    def _setup(self, height, width, seed, fills, min_area, min_visibility, settings):
        unknown = [k for k in settings if k not in self._SETTINGS]
        if unknown:
            raise ValueError(f"{type(self).__name__}: unknown settings {unknown}; {self._sample.__name__} takes {list(self._SETTINGS)}")
        self.height, self.width, self.settings = int(height), int(width), dict(settings)
        for name, colour in fills.items():          # .fill, .hole_fill (and .border): read again at every call
            setattr(self, name, colour)
        self._fills, self.min_area, self.min_visibility = tuple(fills), min_area, min_visibility
        self.rng = np.random.default_rng(seed)
        self.skipped, self.last_plan = [], None
        self._sample([(self.height, self.width)], self.height, self.width, np.random.default_rng(0), **self.settings)      # bad settings fail here

    def __repr__(self):
        return f"{type(self).__name__}({self.height}, {self.width}, {', '.join(f'{k}={v!r}' for k, v in self.settings.items())})"

    def __call__(self, frames, targets=None):
        if not isinstance(frames, torch.Tensor):
            frames = list(frames)
        self.last_plan = self._sample(_frame_sizes(frames), self.height, self.width, self.rng, **self.settings)
        return self._run(frames, self.last_plan, targets, min_area=self.min_area, min_visibility=self.min_visibility,
                         **{k: getattr(self, k) for k in self._fills})

    @staticmethod
    def _read_other(name, params, settings, size):
        """A transform _read_common does not know, read into settings and size -> None, or what to add to its name in the refusal."""
        return ""

    @classmethod
    def from_config(cls, transforms, height=None, width=None, unsupported="raise", **kwargs):
        """The reference's YAML transform list ([{name, params}], `init_args` for `params` and a {name: params} mapping are read too), read as
        the class states.  Any name it does not read raises ValueError naming it, or with unsupported="skip" is listed in .skipped.
        `height` / `width` override the size the list names."""
        settings, skipped, size = {"flip": 0.0, "crop": False}, [], {}
        for name, params in _config_items(transforms, unsupported):
            if _read_common(name, params, settings, size, cls._RESIZED):
                continue
            detail = cls._read_other(name, params, settings, size)
            if detail is None:
                continue
            if unsupported != "skip":
                raise ValueError(f"{cls.__name__}.from_config: transform {name!r}{detail} is not supported ({cls._SUPPORTED} are)")
            skipped.append(name)
        height = size.get("height") if height is None else height
        width = size.get("width") if width is None else width
        if height is None or width is None:
            raise ValueError(f"{cls.__name__}.from_config: no {cls._SIZED} names the canvas size; give height and width")
        out = cls(height, width, **kwargs, **settings)
        out.skipped = skipped
        return out


class TrainAugment(_Transform):
    """The training transform of a run: callable as (frames, targets) -> (canvas, targets).  Owns a numpy Generator (`seed`); every
    call draws a fresh plan with sample_augment(**settings) (kept as .last_plan) and runs augment_batch.
    from_config reads HorizontalFlip.p -> flip; RandomResizedCrop.{height, width, scale, ratio}; ColorJitter.{brightness, contrast, saturation,
    hue}; Cutout.{num_holes, max_h_size, max_w_size}; Resize.{height, width} -> crop=False; Normalize is accepted and ignored (the stem and
    preprocess_uint8 normalise).  Any other name (Affine, RandomCrop, ...) is not supported."""
    _sample, _run = staticmethod(sample_augment), staticmethod(augment_batch)
    _SETTINGS = ("mosaic", "scale", "ratio", "flip", "brightness", "contrast", "saturation", "hue", "contrast_center", "cutout", "crop")
    _SIZED, _SUPPORTED = "RandomResizedCrop / Resize", "HorizontalFlip, RandomResizedCrop, ColorJitter, Cutout, Resize and Normalize"

    def __init__(self, height, width, seed=0, fill=(0, 0, 0), hole_fill=(0, 0, 0), min_area=1.0, min_visibility=0.0, **settings):
        self._setup(height, width, seed, dict(fill=fill, hole_fill=hole_fill), min_area, min_visibility, settings)
