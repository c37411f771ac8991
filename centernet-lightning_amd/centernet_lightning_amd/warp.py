"""Affine training augmentation of a batch on the GPU: albumentations' Affine (scale, rotate, shear, translate), RandomResizedCrop /
RandomCrop / SmallestMaxSize and HorizontalFlip composed into ONE affine map per placement, then colour, cutout and mosaic as augment.py does
them — every canvas pixel is resampled once (albumentations resamples twice: Affine, then the crop).

As in augment.py all randomness is drawn on the host into a PLAN (sample_warp -> WarpPlan: pure numpy), and the device work is a
deterministic function of that plan (warp_batch: one pinned upload, two launches — cnl_augment_warp_u8 and cnl_augment_warp_boxes_f64 of
csrc/augment_warp.hip — no device sync).  A placement carries a forward map `fwd` (continuous source-frame coordinates -> continuous
rectangle coordinates, float64: the boxes go through it and come out as the enclosing box of their four corners, albumentations'
rotate_method="largest_box") and its inverse `inv` in Q20 integers (canvas pixel -> source pixel index: the pixels come through it, bilinear
with 11-bit weights, all in integers).  The rules are stated in include/centernet_gfx950.h and restated in numpy by tests/warp_ref.py; the
pixel rule is deliberately neither cv2.warpAffine's nor the letterbox rule.

Out of scope: rotate_method="ellipse", reflect or replicate borders (everything outside the clip window is one `border` colour),
area-averaged minification (a strong reduction aliases, as bilinear sampling does), YUV sources, perspective.  MotionBlur and the
photometric members of TrivialAugmentWide (Sharpen, Posterize, Solarize, Equalize) are pixel.py's: a pass of its own over the finished
canvas, and pixel.TrainTransform reads the lists that name them; TrainWarp.from_config still refuses them by name.
"""
import dataclasses
import math

import numpy as np

from . import augment as _augment
from .augment import IDENTITY_Q12, MAX_ENTRY, MAX_HOLES, MAX_OFFSET, MAX_PLACE, colour_matrix
from .loss import MAX_SIDE

Q20 = 1 << 20
INV_LINEAR_MAX, INV_OFFSET_MAX = 1 << 30, 1 << 44          # bounds of inv[0, 1, 3, 4] / inv[2, 5] (csrc/augment_warp.hip)
RECORD_WORDS = 24                                          # int64 words of one cnl_warp_placement record (192 bytes)


def _six(m, name):
    a = np.asarray(m, dtype=np.float64)
    if a.shape == (3, 3):
        if not np.array_equal(a[2], (0.0, 0.0, 1.0)):
            raise ValueError(f"{name}: the last row of a 3 x 3 affine map must be (0, 0, 1), got {a[2].tolist()}")
        a = a[:2]
    if a.shape == (2, 3):
        a = a.reshape(6)
    if a.shape != (6,):
        raise ValueError(f"{name} must be 6 numbers, a 2 x 3 or a 3 x 3 matrix, got shape {a.shape}")
    return a


def warp_inverse(fwd) -> np.ndarray:
    """The forward map fwd (6 numbers row by row, 2 x 3 or 3 x 3: continuous source coordinates -> continuous rectangle coordinates)
    -> inv int64 [6], the Q20 map from a canvas pixel (dx, dy) of the rectangle to a source pixel INDEX.  Pure float64, each operation
    rounded on its own in this order:
        det = f0*f4 - f1*f3;  A00 = f4/det, A01 = -f1/det, A10 = -f3/det, A11 = f0/det          (the explicit 2 x 2 adjugate)
        A02 = -(A00*f2 + A01*f5),  A12 = -(A10*f2 + A11*f5)
        inv[0, 1, 3, 4] = rint(A00, A01, A10, A11 * 2^20)
        inv[2] = rint((((0.5*A00 + 0.5*A01) + A02) - 0.5) * 2^20),  inv[5] = rint((((0.5*A10 + 0.5*A11) + A12) - 0.5) * 2^20)
    which is the pixel-centre convention (pixel k covers [k, k + 1)).  ValueError for a singular or non-finite map and for one whose
    inverse leaves |inv[0, 1, 3, 4]| <= 2^30, |inv[2, 5]| <= 2^44."""
    f = [np.float64(v) for v in _six(fwd, "fwd")]
    if not all(np.isfinite(v) for v in f):
        raise ValueError(f"warp_inverse: the map {[float(v) for v in f]} is not finite")
    det = f[0] * f[4] - f[1] * f[3]
    if det == 0:
        raise ValueError(f"warp_inverse: the map {[float(v) for v in f]} is singular")
    with np.errstate(all="ignore"):
        A00, A01, A10, A11 = f[4] / det, -f[1] / det, -f[3] / det, f[0] / det
        A02, A12 = -(A00 * f[2] + A01 * f[5]), -(A10 * f[2] + A11 * f[5])
        half, scale = np.float64(0.5), np.float64(Q20)
        q = [A00 * scale, A01 * scale, (((half * A00 + half * A01) + A02) - half) * scale,
             A10 * scale, A11 * scale, (((half * A10 + half * A11) + A12) - half) * scale]
    if not all(np.isfinite(v) for v in q):
        raise ValueError(f"warp_inverse: the inverse of {[float(v) for v in f]} is not finite")
    q = [int(np.rint(v)) for v in q]
    if max(abs(q[0]), abs(q[1]), abs(q[3]), abs(q[4])) > INV_LINEAR_MAX or max(abs(q[2]), abs(q[5])) > INV_OFFSET_MAX:
        raise ValueError(f"warp_inverse: the inverse of {[float(v) for v in f]} is outside +-2^30 (its matrix) / +-2^44 (its offsets) in Q20")
    return np.array(q, dtype=np.int64)


def _turn(degrees):
    """(cos, sin) of an angle in degrees, exact at the quarter turns."""
    quarter = {0.0: (1.0, 0.0), 90.0: (0.0, 1.0), 180.0: (-1.0, 0.0), 270.0: (0.0, -1.0)}.get(float(degrees) % 360.0)
    return quarter if quarter is not None else (math.cos(math.radians(degrees)), math.sin(math.radians(degrees)))


def _translation(tx, ty):
    return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]])


def affine_matrix(fh, fw, scale=(1.0, 1.0), rotate=0.0, shear=(0.0, 0.0), translate=(0.0, 0.0)) -> np.ndarray:
    """The 3 x 3 float64 forward map of an fh x fw frame onto itself, about the frame centre c = (fw / 2, fh / 2):
        T(c + translate) . Rot(rotate) . Shear(shear) . Scale(scale) . T(-c)
    scale = (sx, sy) (a number: both); rotate in degrees, counter-clockwise as the image is seen (y points down: Rot = [[cos, sin],
    [-sin, cos]]), exact at multiples of 90; shear = (x, y) in degrees, Shear = [[1, tan x], [tan y, 1]]; translate = (tx, ty) in pixels."""
    sx, sy = (float(scale), float(scale)) if isinstance(scale, (int, float)) else (float(v) for v in scale)
    shx, shy = (float(v) for v in shear)
    tx, ty = (float(v) for v in translate)
    c, s = _turn(rotate)
    rot = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])
    sh = np.array([[1.0, math.tan(math.radians(shx)), 0.0], [math.tan(math.radians(shy)), 1.0, 0.0], [0.0, 0.0, 1.0]])
    sc = np.diag([sx, sy, 1.0])
    m = _translation(fw / 2 + tx, fh / 2 + ty) @ rot @ sh @ sc @ _translation(-fw / 2, -fh / 2)
    m[2] = (0.0, 0.0, 1.0)
    return m


@dataclasses.dataclass
class WarpPlan(_augment._Plan):
    """What warp_batch does to a batch of F frames, as numpy arrays (N canvases; slot p of canvas n is live when p < n_place[n]): AugmentPlan's
    fields with two maps in place of the flip bit.  sizes [(h, w)] of the F frames; n_place [N] int32 (1..4); frame [N, 4] int32; window
    [N, 4, 4] int32 (x0, y0, w, h): the CLIP window in the frame, outside which everything is the border colour (the whole frame:
    0, 0, w, h); dest [N, 4, 4] int32 (dx0, dy0, dw, dh) in the canvas; fwd [N, 4, 6] float64, the forward map (continuous frame coordinates
    -> continuous rectangle coordinates: the boxes); inv [N, 4, 6] int64, its Q20 inverse (warp_inverse(fwd): the pixels); colour [N, 4, 12]
    int32; holes [N, 16, 4] int32.  Build one by hand with WarpPlan.empty, fill its arrays (set_map fills fwd and inv), then check()."""
    sizes: list
    height: int
    width: int
    n_place: np.ndarray
    frame: np.ndarray
    window: np.ndarray
    dest: np.ndarray
    fwd: np.ndarray
    inv: np.ndarray
    colour: np.ndarray
    holes: np.ndarray

    _FIELDS = _augment._HEAD + (("fwd", np.float64, (MAX_PLACE, 6)), ("inv", np.int64, (MAX_PLACE, 6))) + _augment._TAIL
    _INITIAL = {"colour": IDENTITY_Q12, "fwd": (1.0, 0.0, 0.0, 0.0, 1.0, 0.0), "inv": (Q20, 0, 0, 0, Q20, 0)}
    RECORD_WORDS, IMAGE_ENTRY, BOXES_ENTRY = RECORD_WORDS, "cnl_augment_warp_u8", "cnl_augment_warp_boxes_f64"

    def set_map(self, n, p, fwd):
        """fwd and inv = warp_inverse(fwd) of slot p of canvas n."""
        self.fwd[n, p] = _six(fwd, "fwd")
        self.inv[n, p] = warp_inverse(fwd)

    def _check_geometry(self, first):
        at = first(~np.isfinite(self.fwd).all(axis=-1))
        if at:
            raise ValueError(f"plan: canvas {at[0]} placement {at[1]}: forward map {self.fwd[at].tolist()} is not finite")
        # (magnitudes in float64: |int64 min| does not exist as an int64)
        q = np.abs(self.inv.astype(np.float64))
        at = first((q[..., [0, 1, 3, 4]].max(axis=-1) > INV_LINEAR_MAX) | (q[..., [2, 5]].max(axis=-1) > INV_OFFSET_MAX))
        if at:
            raise ValueError(f"plan: canvas {at[0]} placement {at[1]}: inverse map {self.inv[at].tolist()} outside +-2^30 (entries 0, 1, 3, 4) / "
                             "+-2^44 (entries 2, 5)")

    def pack(self, places, holes, n_place):
        rec = super().pack(places, holes, n_place)
        rec[:, :, 22:34] = np.ascontiguousarray(self.inv).view(np.int32).reshape(len(self), MAX_PLACE, 12)
        rec[:, :, 34:46] = np.ascontiguousarray(self.fwd).view(np.int32).reshape(len(self), MAX_PLACE, 12)


# ----------------------------------------------------------------------------- drawing a plan
def _range(v, name, neutral, symmetric=True, low=None):
    """A.Affine's parameter forms -> ((lo, hi) for x, (lo, hi) for y) or None: a number v (symmetric: (-v, v); else the constant), a (lo, hi)
    pair for both axes, or a {"x": .., "y": ..} mapping of either form."""
    if v is None:
        return None
    if isinstance(v, dict):
        if set(v) - {"x", "y"}:
            raise ValueError(f"{name} as a mapping has the keys 'x' and 'y', got {sorted(v)}")
        axes = [_range(v.get(k), f"{name}[{k!r}]", neutral, symmetric, low) for k in ("x", "y")]
        axes = [a[0] if a is not None else (neutral, neutral) for a in axes]
        return tuple(axes)
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        v = float(v)
        pair = (-abs(v), abs(v)) if symmetric else (v, v)
    else:
        pair = _augment._pair(v, name)
    if not all(math.isfinite(x) for x in pair) or (low is not None and pair[0] <= low):
        raise ValueError(f"{name} must be finite{'' if low is None else f' and above {low}'}, got {v!r}")
    return pair, pair


def _draw(rng, r, neutral, same=False):
    if r is None:
        return neutral, neutral
    x = float(rng.uniform(*r[0]))
    return x, (x if same else float(rng.uniform(*r[1])))


def sample_warp(sizes, height, width, rng, *, affine_scale=None, rotate=None, shear=None, translate_percent=None, translate_px=None, keep_ratio=False,
                affine_p=1.0, crop="resized", smallest_max_size=None, mosaic=0.0, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip=0.5, brightness=0.0,
                contrast=0.0, saturation=0.0, hue=0.0, contrast_center=128, cutout=None) -> WarpPlan:
    """Draw the plan of one batch: everything sample_augment takes (canvases, mosaic, the RandomResizedCrop window, flip, the colour jitter,
    cutout: drawn as there), plus the affine transform of every placement, drawn uniformly as A.Affine draws it, with probability affine_p:
    affine_scale (a number s: the constant s; a (lo, hi) pair; {"x": .., "y": ..}; x and y are drawn independently unless keep_ratio),
    rotate (degrees, counter-clockwise; a number v: (-v, v)), shear (degrees; number, pair or {"x", "y"}), translate_percent (fractions
    of the frame's width / height) or translate_px (pixels).  A.Affine's own rotation is about the frame centre, as affine_matrix's.

    crop: "resized" (True) takes a RandomResizedCrop window of the affine output (the frame's own size, as A.Affine with fit_output=False)
    and stretches it over the placement's rectangle; False stretches the whole frame (A.Resize); "random" is SmallestMaxSize + RandomCrop:
    the frame scaled by smallest_max_size / min(fh, fw) (1 when smallest_max_size is None) and a rectangle-sized window of it at a uniformly
    drawn integer offset.  DEVIATION: a scaled frame smaller than the rectangle is centred on the border colour, where albumentations'
    RandomCrop raises.

    Per placement fwd = Flip . (window -> rectangle) . Affine and inv = warp_inverse(fwd); the clip window is the whole frame, so what the
    affine transform or the crop pulls in from outside the frame is the border colour.  Pure host arithmetic."""
    sizes = [(int(h), int(w)) for (h, w) in sizes]
    F = len(sizes)
    height, width = int(height), int(width)
    if crop is True:
        crop = "resized"
    if crop not in ("resized", "random", False):
        raise ValueError(f"crop must be 'resized', 'random' or False, got {crop!r}")
    if smallest_max_size is not None and (isinstance(smallest_max_size, bool) or not isinstance(smallest_max_size, (int, float)) or not
                                          1 <= smallest_max_size <= MAX_SIDE):
        raise ValueError(f"smallest_max_size must be in 1..{MAX_SIDE}, got {smallest_max_size!r}")
    if isinstance(affine_p, bool) or not isinstance(affine_p, (int, float)) or not 0 <= affine_p <= 1:
        raise ValueError(f"affine_p must be a probability, got {affine_p!r}")
    if translate_percent is not None and translate_px is not None:
        raise ValueError("translate_percent and translate_px exclude each other")
    r_scale = _range(affine_scale, "affine_scale", 1.0, symmetric=False, low=0.0)
    r_rotate = _range(rotate, "rotate", 0.0)
    r_shear = _range(shear, "shear", 0.0)
    r_shift = _range(translate_percent if translate_percent is not None else translate_px, "translate", 0.0)
    if r_shear is not None and max(abs(v) for axis in r_shear for v in axis) >= 90:
        raise ValueError(f"shear must stay inside (-90, 90) degrees, got {shear!r}")
    affine = any(r is not None for r in (r_scale, r_rotate, r_shear, r_shift))
    # the canvases, rectangles, frames of a mosaic, colours and holes are sample_augment's own draws: one rule, one copy
    base = _augment.sample_augment(sizes, height, width, rng, mosaic=mosaic, scale=scale, ratio=ratio, flip=0.0, brightness=brightness, contrast=contrast,
                                   saturation=saturation, hue=hue, contrast_center=contrast_center, cutout=cutout, crop=False)
    if isinstance(flip, bool) or not isinstance(flip, (int, float)) or not 0 <= flip <= 1:
        raise ValueError(f"flip must be a probability, got {flip!r}")
    scale, ratio = _augment._pair(scale, "scale", low=0.0), _augment._pair(ratio, "ratio", low=0.0)
    plan = WarpPlan.empty(sizes, height, width)
    plan.n_place, plan.frame, plan.dest, plan.colour, plan.holes = base.n_place, base.frame, base.dest, base.colour, base.holes
    for n in range(F):
        for p in range(int(plan.n_place[n])):
            fh, fw = sizes[int(plan.frame[n, p])]
            dx0, dy0, dw, dh = (int(v) for v in plan.dest[n, p])
            plan.window[n, p] = (0, 0, fw, fh)
            m = np.eye(3)
            if affine and (affine_p >= 1 or rng.random() < affine_p):
                sx, sy = _draw(rng, r_scale, 1.0, same=keep_ratio)
                angle = _draw(rng, r_rotate, 0.0, same=True)[0]
                shx, shy = _draw(rng, r_shear, 0.0)
                tx, ty = _draw(rng, r_shift, 0.0)
                if translate_percent is not None:
                    tx, ty = tx * fw, ty * fh
                m = affine_matrix(fh, fw, (sx, sy), angle, (shx, shy), (tx, ty))
            if crop == "random":
                s = 1.0 if smallest_max_size is None else float(smallest_max_size) / min(fh, fw)
                sh_, sw_ = max(int(round(fh * s)), 1), max(int(round(fw * s)), 1)
                ox = int(rng.integers(0, sw_ - dw + 1)) if sw_ >= dw else -((dw - sw_) // 2)
                oy = int(rng.integers(0, sh_ - dh + 1)) if sh_ >= dh else -((dh - sh_) // 2)
                to_rect = np.array([[sw_ / fw, 0.0, -float(ox)], [0.0, sh_ / fh, -float(oy)], [0.0, 0.0, 1.0]])
            else:
                x0, y0, w, h = _augment._window(rng, fh, fw, dw, dh, height, width, scale, ratio) if crop else (0, 0, fw, fh)
                to_rect = np.array([[dw / w, 0.0, -x0 * (dw / w)], [0.0, dh / h, -y0 * (dh / h)], [0.0, 0.0, 1.0]])
            m = to_rect @ m
            if flip > 0 and rng.random() < flip:
                m = np.array([[-1.0, 0.0, float(dw)], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ m
            m[2] = (0.0, 0.0, 1.0)
            plan.set_map(n, p, m)
    return plan


# ----------------------------------------------------------------------------- the call
def warp_batch(frames, plan, targets=None, fill=(0, 0, 0), hole_fill=(0, 0, 0), border=(0, 0, 0), min_area=1.0, min_visibility=0.0, out=None):
    """augment_batch for a WarpPlan: the same frames (read in place where their rows allow), target forms, `out` buffers and returned
    (canvas [N, height, width, 3] uint8, targets dict or None).  border: the colour of everything outside a placement's clip window (it goes
    through the placement's colour matrix, as albumentations' ColorJitter after Affine jitters the border).  A box comes out as the
    enclosing box of its four mapped corners, clipped to the placement's rectangle and kept by augment_batch's rule.  One pinned upload,
    two launches (cnl_augment_warp_u8, cnl_augment_warp_boxes_f64), no device sync."""
    return _augment._batch("warp_batch", WarpPlan, (fill, hole_fill, border), frames, plan, targets, min_area, min_visibility, out)


_AFFINE = {"scale": "affine_scale", "rotate": "rotate", "shear": "shear", "translate_percent": "translate_percent", "translate_px": "translate_px",
           "keep_ratio": "keep_ratio", "p": "affine_p"}


def _plain(v):
    """A YAML value as sample_warp takes it: lists become tuples, inside a mapping too."""
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    return tuple(v) if isinstance(v, list) else v


class TrainWarp(_augment._Transform):
    """TrainAugment with the affine transforms: callable as (frames, targets) -> (canvas, targets).  Owns a numpy Generator (`seed`); every
    call draws a fresh plan with sample_warp(**settings) (kept as .last_plan) and runs warp_batch.
    from_config reads what TrainAugment.from_config reads (HorizontalFlip, RandomResizedCrop, Resize, ColorJitter, Cutout, Normalize), plus
    Affine.{scale, rotate, shear, translate_percent, translate_px, keep_ratio, p}; SmallestMaxSize.max_size -> smallest_max_size;
    RandomCrop.{height, width} -> crop="random" and the canvas size.  Any other name (MotionBlur, TrivialAugmentWide's photometric members,
    ...) and any other Affine parameter is not supported here; pixel.TrainTransform reads the pixel-level ones."""
    _sample, _run, _RESIZED = staticmethod(sample_warp), staticmethod(warp_batch), "resized"
    _SETTINGS = ("affine_scale", "rotate", "shear", "translate_percent", "translate_px", "keep_ratio", "affine_p", "crop", "smallest_max_size", "mosaic",
                 "scale", "ratio", "flip", "brightness", "contrast", "saturation", "hue", "contrast_center", "cutout")
    _SIZED = "RandomResizedCrop / RandomCrop / Resize"
    _SUPPORTED = "Affine, SmallestMaxSize, RandomCrop, HorizontalFlip, RandomResizedCrop, ColorJitter, Cutout, Resize and Normalize"

    def __init__(self, height, width, seed=0, fill=(0, 0, 0), hole_fill=(0, 0, 0), border=(0, 0, 0), min_area=1.0, min_visibility=0.0, **settings):
        self._setup(height, width, seed, dict(fill=fill, hole_fill=hole_fill, border=border), min_area, min_visibility, settings)

    @staticmethod
    def _read_other(name, params, settings, size):
        other = sorted(set(params) - set(_AFFINE)) if name == "Affine" else []
        if name == "Affine" and not other:
            settings.update({_AFFINE[k]: _plain(v) for k, v in params.items()})
            return None
        if name == "SmallestMaxSize" and "max_size" in params:
            settings["smallest_max_size"] = int(params["max_size"])
            return None
        if name == "RandomCrop":
            size.clear()
            size.update({k: int(params[k]) for k in ("height", "width") if k in params})
            settings["crop"] = "random"
            return None
        return f" with {other}" if other else ""
