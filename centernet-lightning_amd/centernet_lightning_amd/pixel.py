"""Pixel-level training augmentation of a batch of finished canvases on the GPU: the transforms of the reference's training lists that need a
neighbourhood or a histogram — MotionBlur (configs/crowdhuman_tracking.yaml) and the photometric members of
datasets/transforms.py::TrivialAugmentWide (Sharpen, Posterize, Solarize, Equalize) — and TrainTransform, the composite that reads every
training transform list of the reference with nothing skipped.

As in augment.py and warp.py all randomness is drawn on the host into a PLAN (sample_pixel -> PixelPlan: pure numpy), and the device work is a
deterministic function of that plan (pixel_batch: one pinned upload, cnl_augment_pixel_u8 of csrc/augment_pixel.hip — two or three launches, one
when no canvas needs a table — no device sync).  A canvas goes through ONE operation (a filter of up to 32 integer taps, or a 256-entry table
per channel), then its holes are punched: the reference's order, Cutout last.  The rule is stated in include/centernet_gfx950.h and restated
in numpy by tests/pixel_ref.py; everything is integer arithmetic.

Stated deviations: the operation acts on the FINISHED canvas (a blur length is in canvas pixels, after the jitter; a mosaic canvas is treated
as a whole) and one operation applies per canvas; the MotionBlur line is the rule of motion_blur_taps, not guaranteed to be cv2.line's pixel
set; Equalize rounds exactly where cv2.equalizeHist rounds in fp32 (a few table entries differ by one level); Sharpen takes lightness = 1 only.
"""
import collections
import dataclasses
import math

import numpy as np
import torch

from . import _frames, _gather, _lib
from . import augment as _augment
from . import warp as _warp
from .augment import BRIGHTNESS, CONTRAST, MAX_ENTRY, MAX_HOLES, MAX_OFFSET, MAX_PLACE, Q12, SATURATION

NONE, FILTER, POSTERIZE, SOLARIZE, EQUALIZE = range(5)             # CNL_PIXEL_* of include/centernet_gfx950.h
MAX_TAPS, MAX_RADIUS = 32, 15
ONE, ABS_MAX = 1 << 16, 1 << 23                                    # the taps' weights sum to ONE; sum |w| <= ABS_MAX
HAS_TABLE, HAS_EQUALIZE = 1, 2                                     # cnl_augment_pixel_u8's `launches`
RECORD_WORDS = 50                                                  # int64 words of one cnl_pixel_op record (400 bytes)
_OP_NAMES = ("NONE", "FILTER", "POSTERIZE", "SOLARIZE", "EQUALIZE")


# ----------------------------------------------------------------------------- the taps
def motion_blur_taps(k, p1, p2) -> np.ndarray:
    """The taps of albumentations' MotionBlur kernel of odd size k (3..31) whose line runs from p1 = (x1, y1) to p2 = (x2, y2), two distinct
    integer points of [0, k - 1]^2 -> int32 [c, 3] rows (dx, dy, w) relative to the centre (k - 1) / 2.  With dx = x2 - x1, dy = y2 - y1 and
    m = max(|dx|, |dy|), tap s = 0..m sits at (x1 + sign(dx) * ((2 s |dx| + m) // (2 m)), y1 + sign(dy) * ((2 s |dy| + m) // (2 m))); of the
    c = m + 1 taps each weighs 65536 // c and the first 65536 - c * (65536 // c) one more.  The taps are distinct, 8-connected and inside the
    kernel; not guaranteed to be cv2.line's pixel set."""
    k = int(k)
    (x1, y1), (x2, y2) = (int(v) for v in p1), (int(v) for v in p2)
    if not (3 <= k <= 2 * MAX_RADIUS + 1 and k % 2 == 1):
        raise ValueError(f"motion blur: the kernel size must be odd and in 3..{2 * MAX_RADIUS + 1}, got {k}")
    if not all(0 <= v < k for v in (x1, y1, x2, y2)) or (x1, y1) == (x2, y2):
        raise ValueError(f"motion blur: the line's ends must be two distinct points of [0, {k - 1}]^2, got {(x1, y1)} and {(x2, y2)}")
    dx, dy = x2 - x1, y2 - y1
    m, c0 = max(abs(dx), abs(dy)), (k - 1) // 2
    sx, sy = (dx > 0) - (dx < 0), (dy > 0) - (dy < 0)
    c = m + 1
    base, more = ONE // c, ONE - c * (ONE // c)
    return np.array([(x1 + sx * ((2 * s * abs(dx) + m) // (2 * m)) - c0, y1 + sy * ((2 * s * abs(dy) + m) // (2 * m)) - c0, base + (s < more))
                     for s in range(c)], dtype=np.int32)


def sharpen_taps(alpha) -> np.ndarray:
    """albumentations' Sharpen matrix with lightness = 1, (1 - alpha) * identity + alpha * [[-1, -1, -1], [-1, 9, -1], [-1, -1, -1]], in
    Q16: a = rint(alpha * 65536), the eight neighbours weigh -a and the centre 65536 + 8 a -> int32 [9, 3] rows (dx, dy, w)."""
    alpha = float(alpha)
    if not 0.0 <= alpha <= 1.0:
        raise ValueError(f"sharpen: alpha must be in [0, 1], got {alpha!r}")
    a = int(np.rint(alpha * ONE))
    return np.array([(dx, dy, ONE + 8 * a if (dx, dy) == (0, 0) else -a) for dy in (-1, 0, 1) for dx in (-1, 0, 1)], dtype=np.int32)


# ----------------------------------------------------------------------------- the plan
@dataclasses.dataclass
class PixelPlan:
    """What pixel_batch does to a batch of N canvases, as numpy arrays: op [N] int32 (NONE, FILTER, POSTERIZE, SOLARIZE, EQUALIZE); param [N]
    int32 (POSTERIZE: bits 0..8; SOLARIZE: the threshold 0..255); n_taps [N] int32 and taps [N, 32, 3] int32 rows (dx, dy, w) of a FILTER:
    |dx|, |dy| <= 15, the w sum to exactly 65536 with sum |w| <= 2^23.  Build one with PixelPlan.empty and the set_* methods, then check()."""
    op: np.ndarray
    param: np.ndarray
    n_taps: np.ndarray
    taps: np.ndarray

    _FIELDS = (("op", ()), ("param", ()), ("n_taps", ()), ("taps", (MAX_TAPS, 3)))

    @classmethod
    def empty(cls, N):
        """A plan of N canvases that copies every one."""
        return cls(**{name: np.zeros((int(N),) + shape, np.int32) for name, shape in cls._FIELDS})

    def __len__(self):
        return int(self.op.shape[0])

    def single(self, n):
        """The plan of canvas n alone."""
        return type(self)(**{name: getattr(self, name)[n:n + 1].copy() for name, _ in self._FIELDS})

    def _set(self, n, op, param=0, taps=None):
        self.op[n], self.param[n], self.n_taps[n], self.taps[n] = op, param, 0, 0
        if taps is not None:
            taps = np.asarray(taps, dtype=np.int64).reshape(-1, 3)
            if not 1 <= len(taps) <= MAX_TAPS:
                raise ValueError(f"plan: canvas {n}: a filter has 1..{MAX_TAPS} taps, got {len(taps)}")
            self.n_taps[n] = len(taps)
            self.taps[n, :len(taps)] = taps

    def set_filter(self, n, taps):
        """Canvas n: the filter of the rows (dx, dy, w)."""
        self._set(n, FILTER, taps=taps)

    def set_motion_blur(self, n, k, p1, p2):
        self._set(n, FILTER, taps=motion_blur_taps(k, p1, p2))

    def set_sharpen(self, n, alpha):
        self._set(n, FILTER, taps=sharpen_taps(alpha))

    def set_posterize(self, n, bits):
        self._set(n, POSTERIZE, int(bits))

    def set_solarize(self, n, threshold):
        self._set(n, SOLARIZE, int(threshold))

    def set_equalize(self, n):
        self._set(n, EQUALIZE)

    @property
    def launches(self):
        """cnl_augment_pixel_u8's `launches`: which of the table and histogram launches the plan needs."""
        table = bool((self.op >= POSTERIZE).any())
        return (HAS_TABLE if table else 0) | (HAS_EQUALIZE if bool((self.op == EQUALIZE).any()) else 0)

    def check(self):
        """Every bound of the plan; ValueError naming the canvas otherwise.  -> self"""
        N = len(self)
        for name, shape in self._FIELDS:
            a = getattr(self, name)
            if not isinstance(a, np.ndarray) or a.dtype != np.int32 or a.shape != (N,) + shape:
                raise ValueError(f"plan: {name} must be an int32 array of shape {[N] + list(shape)}")

        def first(mask):
            at = np.nonzero(mask)[0]
            return int(at[0]) if at.size else None

        n = first((self.op < NONE) | (self.op > EQUALIZE))
        if n is not None:
            raise ValueError(f"plan: canvas {n}: op {int(self.op[n])} is none of {', '.join(_OP_NAMES)} (0..4)")
        n = first((self.op == POSTERIZE) & ((self.param < 0) | (self.param > 8)))
        if n is not None:
            raise ValueError(f"plan: canvas {n}: posterize bits {int(self.param[n])} outside 0..8")
        n = first((self.op == SOLARIZE) & ((self.param < 0) | (self.param > 255)))
        if n is not None:
            raise ValueError(f"plan: canvas {n}: solarize threshold {int(self.param[n])} outside 0..255")
        filt = self.op == FILTER
        n = first(filt & ((self.n_taps < 1) | (self.n_taps > MAX_TAPS)))
        if n is not None:
            raise ValueError(f"plan: canvas {n}: n_taps {int(self.n_taps[n])} outside 1..{MAX_TAPS}")
        live = filt[:, None] & (np.arange(MAX_TAPS)[None, :] < self.n_taps[:, None])
        t = self.taps.astype(np.int64)
        n = first((live & (np.abs(t[..., :2]).max(axis=-1) > MAX_RADIUS)).any(axis=1))
        if n is not None:
            raise ValueError(f"plan: canvas {n}: a tap offset lies beyond +-{MAX_RADIUS}")
        w = np.where(live, t[..., 2], 0)
        n = first(filt & (w.sum(axis=1) != ONE))
        if n is not None:
            raise ValueError(f"plan: canvas {n}: the weights sum to {int(w[n].sum())}, not {ONE}")
        n = first(filt & (np.abs(w).sum(axis=1) > ABS_MAX))
        if n is not None:
            raise ValueError(f"plan: canvas {n}: sum |w| = {int(np.abs(w[n]).sum())} exceeds 2^23")
        return self

    def pack(self, records):
        """Fill records [N, 100] int32 (zeroed): the cnl_pixel_op records."""
        records[:, 0], records[:, 1], records[:, 2] = self.op, self.param, self.n_taps
        records[:, 4:] = self.taps.reshape(len(self), 3 * MAX_TAPS)


# ----------------------------------------------------------------------------- drawing a plan
def _int_range(v, name, low, high):
    """A number v -> (v, v); a (lo, hi) pair of integers inside low..high."""
    pair = (v, v) if isinstance(v, (int, float)) and not isinstance(v, bool) else _augment._pair(v, name)
    lo, hi = (int(x) for x in pair)
    if (lo, hi) != tuple(float(x) for x in pair) or not low <= lo <= hi <= high:
        raise ValueError(f"{name} must be an integer or an increasing pair of integers in {low}..{high}, got {v!r}")
    return lo, hi


def _blur_sizes(v):
    """albumentations' blur_limit (a number v: (3, v)) -> the odd kernel sizes it draws from."""
    lo, hi = _int_range((3, v) if isinstance(v, (int, float)) and not isinstance(v, bool) else v, "motion_blur", 3, 2 * MAX_RADIUS + 1)
    sizes = [k for k in range(lo, hi + 1) if k % 2 == 1]
    if not sizes:
        raise ValueError(f"motion_blur = {v!r} holds no odd kernel size")
    return sizes


def _alpha_range(v):
    pair = (v, v) if isinstance(v, (int, float)) and not isinstance(v, bool) else _augment._pair(v, "sharpen")
    if not 0.0 <= pair[0] <= pair[1] <= 1.0:
        raise ValueError(f"sharpen's alpha must lie in [0, 1], got {v!r}")
    return float(pair[0]), float(pair[1])


def _probability(v, name):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
        raise ValueError(f"{name} must be a probability, got {v!r}")
    return float(v)


def _draw_motion_blur(plan, n, rng, sizes):
    """albumentations' MotionBlur.get_params: an odd size, then the line's ends (x1 == x2: two distinct y)."""
    k = sizes[int(rng.integers(0, len(sizes)))]
    x1, x2 = int(rng.integers(0, k)), int(rng.integers(0, k))
    if x1 == x2:
        y1, y2 = (int(v) for v in rng.choice(k, size=2, replace=False))
    else:
        y1, y2 = int(rng.integers(0, k)), int(rng.integers(0, k))
    plan.set_motion_blur(n, k, (x1, y1), (x2, y2))


_KINDS = ("motion_blur", "sharpen", "posterize", "solarize", "equalize")


def _drawers(motion_blur, sharpen, posterize, solarize, equalize):
    """The kinds that are given -> [(name, draw(plan, n, rng))], their parameters judged."""
    draw = []
    if motion_blur is not None:
        sizes = _blur_sizes(motion_blur)
        draw.append(("motion_blur", lambda plan, n, rng: _draw_motion_blur(plan, n, rng, sizes)))
    if sharpen is not None:
        alpha = _alpha_range(sharpen)
        draw.append(("sharpen", lambda plan, n, rng: plan.set_sharpen(n, float(rng.uniform(*alpha)))))
    if posterize is not None:
        bits = _int_range(posterize, "posterize", 0, 8)
        draw.append(("posterize", lambda plan, n, rng: plan.set_posterize(n, int(rng.integers(bits[0], bits[1] + 1)))))
    if solarize is not None:
        t = _int_range(solarize, "solarize", 0, 255)
        draw.append(("solarize", lambda plan, n, rng: plan.set_solarize(n, int(rng.integers(t[0], t[1] + 1)))))
    if not isinstance(equalize, bool):
        raise ValueError(f"equalize must be True or False, got {equalize!r}")
    if equalize:
        draw.append(("equalize", lambda plan, n, rng: plan.set_equalize(n)))
    return draw


def sample_pixel(N, rng, *, motion_blur=None, sharpen=None, posterize=None, solarize=None, equalize=False, p=0.5, one_of=False) -> PixelPlan:
    """Draw the plan of N canvases with `rng`, a numpy.random.Generator.  Pure host arithmetic.  The kinds, each as albumentations takes it:
    motion_blur = blur_limit (a number v: (3, v); an odd size in 3..31 is drawn uniformly, then the line as MotionBlur draws it);
    sharpen = alpha (a pair inside [0, 1], drawn uniformly; lightness is 1); posterize = num_bits (an integer or a pair in 0..8, drawn
    uniformly); solarize = threshold (an integer or a pair in 0..255, drawn uniformly among the integers); equalize = True.
    With one kind given every canvas gets it with probability p; with several and one_of=True it is A.OneOf's rule: with probability p one
    of the given kinds, uniformly.  Several kinds without one_of are refused: one operation applies per canvas."""
    draw = _drawers(motion_blur, sharpen, posterize, solarize, equalize)
    p = _probability(p, "p")
    if len(draw) > 1 and not one_of:
        raise ValueError(f"sample_pixel: {', '.join(name for name, _ in draw)} are given, but one operation applies per canvas: choose one, or one_of=True")
    plan = PixelPlan.empty(N)
    for n in range(len(plan)):
        if draw and rng.random() < p:
            draw[int(rng.integers(0, len(draw))) if len(draw) > 1 else 0][1](plan, n, rng)
    return plan


# ----------------------------------------------------------------------------- the call
def pixel_batch(canvas, plan, holes=None, hole_fill=(0, 0, 0), out=None):
    """canvas: a contiguous uint8 [N, height, width, 3] tensor on a HIP device (what warp_batch / augment_batch return; width % 4 == 0), only
    read; plan: a PixelPlan of N canvases (checked here); holes: None or an int32 [N, 16, 4] numpy array of (x0, y0, w, h) as a WarpPlan's
    holes, punched with hole_fill AFTER the operation -> a new canvas of the same shape (or `out`, a tensor of that shape that does not
    overlap canvas).  One pinned upload, two or three launches (one when no canvas needs a table), no device sync."""
    what = "pixel_batch"
    if not isinstance(plan, PixelPlan):
        raise ValueError(f"{what}: plan must be a PixelPlan, got {type(plan).__name__}")
    plan.check()
    if not isinstance(canvas, torch.Tensor) or canvas.dtype != torch.uint8 or canvas.dim() != 4 or canvas.shape[3] != 3:
        raise ValueError(f"{what}: canvas must be a uint8 [N, height, width, 3] tensor")
    N, H, W = (int(v) for v in canvas.shape[:3])
    if N != len(plan):
        raise ValueError(f"{what}: the plan holds {len(plan)} canvases, the batch {N}")
    if holes is not None:
        holes = np.asarray(holes)
        if holes.dtype != np.int32 or holes.shape != (N, MAX_HOLES, 4):
            raise ValueError(f"{what}: holes must be an int32 array of shape {[N, MAX_HOLES, 4]}")
    word = _frames.fill_word(hole_fill, 3)
    _gather.require_hip([canvas], what)
    if not canvas.is_contiguous():
        raise ValueError(f"{what}: canvas must be contiguous")
    dev = canvas.device
    if out is None:
        out = torch.empty_like(canvas)
    elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.shape != canvas.shape or out.device != dev or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous uint8 tensor of shape {list(canvas.shape)} on {dev}")
    if N == 0:
        return out
    o_holes = N * RECORD_WORDS
    buf = np.zeros(o_holes + (N * MAX_HOLES * 2 if holes is not None else 0), dtype=np.int64)
    plan.pack(buf[:o_holes].view(np.int32).reshape(N, 2 * RECORD_WORDS))
    if holes is not None:
        buf[o_holes:].view(np.int32).reshape(N, MAX_HOLES, 4)[:] = holes
    lib = _lib.load()
    need = int(lib.cnl_augment_pixel_workspace_bytes(N, H, W))
    with torch.cuda.device(dev):
        d = _gather.upload(buf, dev)
        space = torch.empty((need,), device=dev, dtype=torch.uint8)
        _lib.check(lib.cnl_augment_pixel_u8(canvas.data_ptr(), N, H, W, d.data_ptr(), plan.launches, d[o_holes:].data_ptr() if holes is not None else None,
                                            word, out.data_ptr(), space.data_ptr(), need, _lib.stream(dev)), "cnl_augment_pixel_u8")
    return out


# ----------------------------------------------------------------------------- TrivialAugmentWide's colour members
def _colour_step(op, value, contrast_center):
    """One ColorJitter operation as (A, a) in float64: colour_matrix's brightness, contrast and saturation."""
    if op == BRIGHTNESS:
        return float(value) * np.eye(3), np.zeros(3)
    if op == CONTRAST:
        return float(value) * np.eye(3), (1.0 - float(value)) * float(contrast_center) * np.ones(3)
    if op == SATURATION:
        return float(value) * np.eye(3) + (1.0 - float(value)) * np.outer(np.ones(3), _augment._LUMA), np.zeros(3)
    raise ValueError(f"a colour member is brightness, contrast or saturation (0..2), got {op!r}")


def colour_words(base=None, member=None, contrast_center=128):
    """The Q12 colour words of a placement whose ColorJitter factors are `base` = (brightness, contrast, saturation, hue, order) as
    colour_matrix takes them (None: the identity), followed by a TrivialAugmentWide colour `member` = (op, factor), composed in float64
    before the ONE rounding to Q12 -> int32 [12].  Without a member these are colour_matrix's words exactly."""
    b, c, s, h, order = base if base is not None else (1.0, 1.0, 1.0, 0.0, ())
    if member is None:
        return _augment.colour_matrix(b, c, s, h, order=order, contrast_center=contrast_center)
    M, o = np.eye(3), np.zeros(3)
    for op in order:
        if op == _augment.HUE:
            t = 2.0 * math.pi * float(h)
            rot = np.array([[1.0, 0.0, 0.0], [0.0, math.cos(t), -math.sin(t)], [0.0, math.sin(t), math.cos(t)]])
            A, a = np.linalg.inv(_augment._YIQ) @ rot @ _augment._YIQ, np.zeros(3)
        else:
            A, a = _colour_step(op, (b, c, s)[op], contrast_center)
        M, o = A @ M, A @ o + a
    A, a = _colour_step(member[0], member[1], contrast_center)
    M, o = A @ M, A @ o + a
    q = np.empty(12, dtype=np.int32)
    q[:9] = np.clip(np.rint(M * Q12), -MAX_ENTRY, MAX_ENTRY).reshape(9)
    q[9:] = np.clip(np.rint(o * Q12), -MAX_OFFSET, MAX_OFFSET)
    return q


# datasets/transforms.py::TrivialAugmentWide: twelve members, one of them with probability 12 / 13
TRIVIAL_MEMBERS = ("shear_x", "shear_y", "translate_x", "translate_y", "rotate", "brightness", "contrast", "saturation", "sharpen", "posterize",
                   "solarize", "equalize")
TRIVIAL_P = len(TRIVIAL_MEMBERS) / (len(TRIVIAL_MEMBERS) + 1)
_COLOUR_KEYS = ("brightness", "contrast", "saturation", "hue")


def sample_trivial(sizes, height, width, rng, **settings):
    """The plans of one batch under TrivialAugmentWide -> (WarpPlan, PixelPlan, members [N] of names or None).  sample_warp(**settings) draws
    the canvases, maps and holes with the colour jitter taken out; then every canvas draws, with probability 12 / 13, one of the twelve
    members uniformly, and every placement its ColorJitter factors (as sample_augment draws them).  An Affine member (shear x or y uniform in
    +-45 degrees, translate x or y an integer in -32..32 pixels, rotate uniform in +-135 degrees: as A.Affine draws them) is composed into
    every placement's map on the source-frame side, fwd @ affine_matrix(...); a ColorJitter member (factor uniform in [0.01, 1.99]) goes
    into the colour words after the placement's own jitter, in float64 before the one Q12 rounding (colour_words); Sharpen (alpha uniform in
    (0, 0.99)), Posterize (2..8 bits), Solarize (threshold 0..255) and Equalize go into the PixelPlan."""
    ranges = [_augment._factor_range(settings.get(k, 0.0), k, hue=(k == "hue")) for k in _COLOUR_KEYS]
    center = settings.get("contrast_center", 128)
    plan = _warp.sample_warp(sizes, height, width, rng, **{k: v for k, v in settings.items() if k not in _COLOUR_KEYS})
    pixel, members = PixelPlan.empty(len(plan)), []
    for n in range(len(plan)):
        member = TRIVIAL_MEMBERS[int(rng.integers(0, len(TRIVIAL_MEMBERS)))] if rng.random() < TRIVIAL_P else None
        members.append(member)
        affine = colour = None
        if member in ("shear_x", "shear_y"):
            angle = float(rng.uniform(-45, 45))
            affine = dict(shear=(angle, 0.0) if member == "shear_x" else (0.0, angle))
        elif member in ("translate_x", "translate_y"):
            shift = float(rng.integers(-32, 33))
            affine = dict(translate=(shift, 0.0) if member == "translate_x" else (0.0, shift))
        elif member == "rotate":
            affine = dict(rotate=float(rng.uniform(-135, 135)))
        elif member in ("brightness", "contrast", "saturation"):
            colour = ((BRIGHTNESS, CONTRAST, SATURATION)[_COLOUR_KEYS.index(member)], float(rng.uniform(0.01, 1.99)))
        elif member == "sharpen":
            pixel.set_sharpen(n, float(rng.uniform(0.0, 0.99)))
        elif member == "posterize":
            pixel.set_posterize(n, int(rng.integers(2, 9)))
        elif member == "solarize":
            pixel.set_solarize(n, int(rng.integers(0, 256)))
        elif member == "equalize":
            pixel.set_equalize(n)
        for p in range(int(plan.n_place[n])):
            if affine is not None:
                fh, fw = plan.sizes[int(plan.frame[n, p])]
                fwd = np.vstack([plan.fwd[n, p].reshape(2, 3), (0.0, 0.0, 1.0)]) @ _warp.affine_matrix(fh, fw, **affine)
                fwd[2] = (0.0, 0.0, 1.0)
                plan.set_map(n, p, fwd)
            base = None
            if any(r is not None for r in ranges):
                factors = [float(rng.uniform(*r)) if r is not None else neutral for r, neutral in zip(ranges, (1.0, 1.0, 1.0, 0.0))]
                base = (*factors, [int(v) for v in rng.permutation(4)])
            if base is not None or colour is not None:
                plan.colour[n, p] = colour_words(base, colour, center)
    return plan, pixel, members


# ----------------------------------------------------------------------------- the composite transform
TransformPlan = collections.namedtuple("TransformPlan", "warp pixel")        # pixel: None without a pixel-level entry

_PIXEL_SETTINGS = _KINDS + ("pixel_p", "trivial_augment")
_PIXEL_NAMES = ("MotionBlur", "Sharpen", "Posterize", "Solarize", "Equalize", "TrivialAugmentWide")


def _is_one(v):
    return v == 1 or (isinstance(v, (list, tuple)) and len(v) == 2 and v[0] == 1 and v[1] == 1)


def _read_pixel(name, params):
    """One pixel-level transform of a list -> its settings; ValueError for what is not taken."""
    def only(*known):
        other = sorted(set(params) - set(known))
        if other:
            raise ValueError(f"TrainTransform.from_config: transform {name!r} with {other} is not supported ({name} takes {list(known)})")

    settings = {"pixel_p": float(params.get("p", 0.5))}
    if name == "MotionBlur":
        only("blur_limit", "p")
        settings["motion_blur"] = _warp._plain(params.get("blur_limit", 7))
    elif name == "Sharpen":
        only("alpha", "lightness", "p")
        if not _is_one(params.get("lightness")):
            raise ValueError(f"TrainTransform.from_config: 'Sharpen' with lightness = {params.get('lightness')!r} is not supported: the filter's weights sum to "
                             "one, which is lightness = 1 (albumentations' default is (0.5, 1.0): state lightness: [1, 1])")
        settings["sharpen"] = _warp._plain(params.get("alpha", (0.2, 0.5)))
    elif name == "Posterize":
        only("num_bits", "p")
        settings["posterize"] = _warp._plain(params.get("num_bits", 4))
    elif name == "Solarize":
        only("threshold", "p")
        settings["solarize"] = _warp._plain(params.get("threshold", 128))
    elif name == "Equalize":
        only("mode", "by_channels", "p")
        if params.get("mode", "cv") != "cv" or params.get("by_channels", True) is not True:
            raise ValueError("TrainTransform.from_config: 'Equalize' is read with mode='cv' and by_channels=True only, got "
                             f"mode={params.get('mode')!r}, by_channels={params.get('by_channels')!r}")
        settings["equalize"] = True
    else:
        only()
        settings = {"trivial_augment": True}
    return settings


class TrainTransform:
    """TrainWarp with the pixel-level transforms: callable as (frames, targets) -> (canvas, targets).  It takes TrainWarp's arguments and
    settings plus motion_blur, sharpen, posterize, solarize, equalize (ONE of them, as sample_pixel takes it, applied with probability
    pixel_p) or trivial_augment=True (sample_trivial).  Every call draws a WarpPlan and then, from the same Generator, a PixelPlan, kept as
    .last_plan = TransformPlan(warp, pixel); sample(sizes) draws them without a device.  With a pixel plan, warp_batch runs a copy of the
    warp plan without its holes and pixel_batch punches them after its operation (Cutout last, as the reference's lists order it);
    without a pixel-level setting pixel_batch is never called and the output is TrainWarp's byte for byte for the same seed.
    from_config reads what TrainWarp.from_config reads (it delegates to it with the pixel-level entries taken out: one reader), plus
    MotionBlur.{blur_limit, p}, Sharpen.{alpha, lightness, p} (lightness 1 only), Posterize.{num_bits, p}, Solarize.{threshold, p},
    Equalize.{p} (mode "cv", by_channels True only) and TrivialAugmentWide.  More than one pixel-level entry is refused: one operation
    applies per canvas."""

    def __init__(self, height, width, seed=0, fill=(0, 0, 0), hole_fill=(0, 0, 0), border=(0, 0, 0), min_area=1.0, min_visibility=0.0, **settings):
        pixel = {k: settings.pop(k) for k in _PIXEL_SETTINGS if k in settings}
        self._warp = _warp.TrainWarp(height, width, seed, fill, hole_fill, border, min_area, min_visibility, **settings)
        self.height, self.width, self.rng = self._warp.height, self._warp.width, self._warp.rng
        self.settings = dict(self._warp.settings, **pixel)
        self.trivial = pixel.pop("trivial_augment", False)
        if not isinstance(self.trivial, bool):
            raise ValueError(f"TrainTransform: trivial_augment must be True or False, got {self.trivial!r}")
        self.pixel_p = _probability(pixel.pop("pixel_p", 0.5), "pixel_p")
        self.kinds = {k: v for k, v in pixel.items() if not (k == "equalize" and v is False) and v is not None}
        given = list(self.kinds) + (["trivial_augment"] if self.trivial else [])
        if len(given) > 1:
            raise ValueError(f"TrainTransform: {', '.join(given)} are given, but one operation applies per canvas: choose one")
        _drawers(**{k: self.kinds.get(k, False if k == "equalize" else None) for k in _KINDS})        # bad settings fail here
        self.skipped, self.last_plan = [], None

    def __repr__(self):
        return f"TrainTransform({self.height}, {self.width}, {', '.join(f'{k}={v!r}' for k, v in self.settings.items())})"

    # the colours and the box rule are TrainWarp's, read again at every call
    fill = property(lambda self: self._warp.fill, lambda self, v: setattr(self._warp, "fill", v))
    hole_fill = property(lambda self: self._warp.hole_fill, lambda self, v: setattr(self._warp, "hole_fill", v))
    border = property(lambda self: self._warp.border, lambda self, v: setattr(self._warp, "border", v))
    min_area = property(lambda self: self._warp.min_area, lambda self, v: setattr(self._warp, "min_area", v))
    min_visibility = property(lambda self: self._warp.min_visibility, lambda self, v: setattr(self._warp, "min_visibility", v))

    def sample(self, sizes) -> TransformPlan:
        """Draw the plans of one batch of frames of `sizes` [(h, w)] (kept as .last_plan): pure host arithmetic."""
        if self.trivial:
            plan, pixel, _ = sample_trivial(sizes, self.height, self.width, self.rng, **self._warp.settings)
        else:
            plan = _warp.sample_warp(sizes, self.height, self.width, self.rng, **self._warp.settings)
            pixel = sample_pixel(len(plan), self.rng, p=self.pixel_p, **self.kinds) if self.kinds else None
        self.last_plan = TransformPlan(plan, pixel)
        return self.last_plan

    def __call__(self, frames, targets=None):
        if not isinstance(frames, torch.Tensor):
            frames = list(frames)
        plan, pixel = self.sample(_augment._frame_sizes(frames))
        w = self._warp
        colours = dict(fill=w.fill, hole_fill=w.hole_fill, border=w.border, min_area=w.min_area, min_visibility=w.min_visibility)
        if pixel is None:
            return _warp.warp_batch(frames, plan, targets, **colours)
        canvas, targets = _warp.warp_batch(frames, dataclasses.replace(plan, holes=np.zeros_like(plan.holes)), targets, **colours)
        return pixel_batch(canvas, pixel, holes=plan.holes, hole_fill=w.hole_fill), targets

    @classmethod
    def from_config(cls, transforms, height=None, width=None, unsupported="raise", **kwargs):
        """The reference's YAML transform list, in the forms TrainWarp.from_config reads.  The pixel-level entries are read here, everything
        else by TrainWarp.from_config (names neither reads raise ValueError, or with unsupported="skip" are listed in .skipped)."""
        rest, pixel, seen = [], {}, []
        for name, params in _augment._config_items(transforms, unsupported):
            if name in _PIXEL_NAMES:
                seen.append(name)
                pixel = _read_pixel(name, params)
            else:
                rest.append({"name": name, "params": params})
        if len(seen) > 1:
            raise ValueError(f"TrainTransform.from_config: the list holds {len(seen)} pixel-level transforms ({', '.join(seen)}), but one operation "
                             "applies per canvas (the filter or table of one transform): keep one, or TrivialAugmentWide, which draws one of its own")
        read = _warp.TrainWarp.from_config(rest, height, width, unsupported)
        out = cls(read.height, read.width, **kwargs, **read.settings, **pixel)
        out.skipped = read.skipped
        return out
