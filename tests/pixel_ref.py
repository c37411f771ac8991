"""Test-only yardstick for the pixel-level training augmentation (numpy): the rule of include/centernet_gfx950.h (cnl_augment_pixel_u8) and the
host rules of the taps (MotionBlur's line, Sharpen's matrix) restated on their own.  A plan is read through its arrays only (op, param,
n_taps, taps): nothing of the package is imported here.  Everything is integer arithmetic in int64."""
import numpy as np

NONE, FILTER, POSTERIZE, SOLARIZE, EQUALIZE = range(5)
MAX_TAPS, MAX_RADIUS, ONE, ABS_MAX = 32, 15, 1 << 16, 1 << 23


# ----------------------------------------------------------------------------- the host rules
def reflect(i, n):
    """cv2's BORDER_REFLECT_101 made total: the index into an axis of n >= 1 elements that position i (any integer) reads."""
    if n == 1:
        return 0
    period = 2 * (n - 1)
    m = i % period                               # Python's %: non-negative
    return m if m < n else period - m


def line_taps(k, p1, p2):
    """MotionBlur's taps [(dx, dy, w)] for a kernel of odd size k and the line from p1 = (x1, y1) to p2 = (x2, y2)."""
    (x1, y1), (x2, y2) = p1, p2
    dx, dy = x2 - x1, y2 - y1
    m = max(abs(dx), abs(dy))
    sx, sy = int(np.sign(dx)), int(np.sign(dy))
    c, centre = m + 1, (k - 1) // 2
    w = ONE // c
    extra = ONE - c * w
    return [(x1 + sx * ((2 * s * abs(dx) + m) // (2 * m)) - centre, y1 + sy * ((2 * s * abs(dy) + m) // (2 * m)) - centre, w + (1 if s < extra else 0))
            for s in range(c)]


def sharpen_taps(alpha):
    a = int(np.rint(np.float64(alpha) * ONE))
    return [(dx, dy, ONE + 8 * a if dx == 0 and dy == 0 else -a) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


# ----------------------------------------------------------------------------- one canvas
def apply_filter(img, taps):
    """img [H, W, 3] uint8, taps [(dx, dy, w)] -> [H, W, 3] uint8."""
    H, W = img.shape[:2]
    src = img.astype(np.int64)
    acc = np.full(img.shape, 32768, dtype=np.int64)
    for dx, dy, w in taps:
        rows = np.array([reflect(y + int(dy), H) for y in range(H)])
        cols = np.array([reflect(x + int(dx), W) for x in range(W)])
        acc += int(w) * src[rows][:, cols]
    assert np.abs(acc).max() < 2 ** 31
    return np.clip(acc >> 16, 0, 255).astype(np.uint8)           # >> on int64 arrays is an arithmetic shift


def posterize_lut(bits):
    return np.array([v & (0xFF << (8 - bits)) & 0xFF for v in range(256)], dtype=np.uint8)


def solarize_lut(t):
    return np.array([255 - v if v >= t else v for v in range(256)], dtype=np.uint8)


def equalize_lut(channel):
    """The table of one channel [H, W] uint8 (Python integers: exact)."""
    h = np.bincount(channel.reshape(-1), minlength=256).tolist()
    i0 = next(i for i in range(256) if h[i])
    d = channel.size - h[i0]
    if d == 0:
        return np.arange(256, dtype=np.uint8)
    lut, cum = [0] * 256, 0
    for v in range(i0 + 1, 256):
        cum += h[v]
        lut[v] = (510 * cum + d) // (2 * d)
    return np.array(lut, dtype=np.uint8)


def record_op(op, param, n_taps, taps):
    """The operation a record runs as: a bad record runs as NONE (the header's rule)."""
    op, param, n_taps = int(op), int(param), int(n_taps)
    if op == FILTER:
        if not 1 <= n_taps <= MAX_TAPS:
            return NONE
        t = np.asarray(taps[:n_taps], dtype=np.int64)
        return FILTER if np.abs(t[:, :2]).max() <= MAX_RADIUS and np.abs(t[:, 2]).sum() <= ABS_MAX else NONE
    if op == POSTERIZE:
        return op if 0 <= param <= 8 else NONE
    if op == SOLARIZE:
        return op if 0 <= param <= 255 else NONE
    return op if op == EQUALIZE else NONE


def apply_op(img, op, param=0, n_taps=0, taps=None):
    """One canvas [H, W, 3] uint8 through one record, before the holes."""
    op = record_op(op, param, n_taps, taps)
    if op == FILTER:
        return apply_filter(img, [tuple(int(v) for v in t) for t in taps[:int(n_taps)]])
    if op == NONE:
        return img.copy()
    out = np.empty_like(img)
    for c in range(3):
        lut = posterize_lut(int(param)) if op == POSTERIZE else solarize_lut(int(param)) if op == SOLARIZE else equalize_lut(img[..., c])
        out[..., c] = lut[img[..., c]]
    return out


def punch(img, holes, hole_fill):
    """The live slots of holes [16, 4] (x0, y0, w, h), clipped to the canvas, filled in place."""
    H, W = img.shape[:2]
    for (x0, y0, w, h) in np.asarray(holes).tolist():
        if w > 0 and h > 0:
            img[max(y0, 0):max(min(y0 + h, H), 0), max(x0, 0):max(min(x0 + w, W), 0)] = np.asarray(hole_fill[:3], dtype=np.uint8)
    return img


def expected(canvas, plan, holes=None, hole_fill=(0, 0, 0)):
    """canvas [N, H, W, 3] uint8, plan with op / param / n_taps / taps, holes [N, 16, 4] or None -> [N, H, W, 3] uint8."""
    out = np.empty_like(canvas)
    for n in range(canvas.shape[0]):
        out[n] = apply_op(canvas[n], plan.op[n], plan.param[n], plan.n_taps[n], plan.taps[n])
        if holes is not None:
            punch(out[n], holes[n], hole_fill)
    return out
