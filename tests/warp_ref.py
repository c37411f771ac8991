"""Test-only yardstick for the affine training augmentation (numpy): the rules of include/centernet_gfx950.h (cnl_augment_warp_u8,
cnl_augment_warp_boxes_f64, warp_inverse) restated on their own.  A plan is read through its arrays only (n_place, frame, window, dest,
fwd, inv, colour, holes, height, width): nothing of the package is imported here.  The colour step and the box rule from `full` on are
those of tests/augment_ref.py, as the header says."""
import numpy as np

import augment_ref

INV_LINEAR_MAX, INV_OFFSET_MAX = 1 << 30, 1 << 44


# ----------------------------------------------------------------------------- the host rule
def warp_inverse(fwd):
    """fwd: 6 float64 (continuous source coordinates -> continuous rectangle coordinates) -> int64 [6], the Q20 map from a canvas pixel of
    the rectangle to a source pixel index; ValueError for a singular, non-finite or out-of-bounds map."""
    f = [np.float64(v) for v in np.asarray(fwd, dtype=np.float64).reshape(-1)[:6]]
    if not np.isfinite(f).all():
        raise ValueError("not finite")
    det = f[0] * f[4] - f[1] * f[3]
    if det == 0:
        raise ValueError("singular")
    half, one = np.float64(0.5), np.float64(2 ** 20)
    with np.errstate(all="ignore"):
        A00, A01, A10, A11 = f[4] / det, -f[1] / det, -f[3] / det, f[0] / det
        A02 = -(A00 * f[2] + A01 * f[5])
        A12 = -(A10 * f[2] + A11 * f[5])
        q = [A00 * one, A01 * one, (((half * A00 + half * A01) + A02) - half) * one, A10 * one, A11 * one, (((half * A10 + half * A11) + A12) - half) * one]
    if not np.isfinite(q).all():
        raise ValueError("inverse not finite")
    q = [int(np.rint(v)) for v in q]
    if not inv_ok(q):
        raise ValueError("inverse out of bounds")
    return np.array(q, dtype=np.int64)


def inv_ok(inv):
    q = [int(v) for v in inv]
    return max(abs(q[0]), abs(q[1]), abs(q[3]), abs(q[4])) <= INV_LINEAR_MAX and max(abs(q[2]), abs(q[5])) <= INV_OFFSET_MAX


# ----------------------------------------------------------------------------- pixels
def sample(frame, window, dw, dh, inv, border):
    """The rectangle [dh, dw, 3] uint8 of one placement before the colour step, and per pixel the number of its four taps that lie inside
    the clip window [dh, dw], sx and sy [dh, dw] (int64) and X, Y.  Integers only; >> on int64 arrays is an arithmetic shift."""
    x0, y0, w, h = (int(v) for v in window)
    i = [int(v) for v in inv]
    dx, dy = np.meshgrid(np.arange(dw, dtype=np.int64), np.arange(dh, dtype=np.int64))
    X = i[0] * dx + i[1] * dy + i[2]
    Y = i[3] * dx + i[4] * dy + i[5]
    sx, sy = X >> 20, Y >> 20
    a1, b1 = (X >> 9) & 2047, (Y >> 9) & 2047
    a0, b0 = 2048 - a1, 2048 - b1
    fh, fw = frame.shape[:2]
    src = frame.astype(np.int64)
    edge = np.asarray(border[:3], dtype=np.int64)

    def tap(ix, iy):
        inside = (ix >= x0) & (ix < x0 + w) & (iy >= y0) & (iy < y0 + h)
        v = src[np.clip(iy, 0, fh - 1), np.clip(ix, 0, fw - 1)]
        return np.where(inside[..., None], v, edge), inside

    t00, in00 = tap(sx, sy)
    t10, in10 = tap(sx + 1, sy)
    t01, in01 = tap(sx, sy + 1)
    t11, in11 = tap(sx + 1, sy + 1)
    t = t00 * a0[..., None] + t10 * a1[..., None]
    u = t01 * a0[..., None] + t11 * a1[..., None]
    v = (t * b0[..., None] + u * b1[..., None] + (1 << 21)) >> 22
    assert v.min() >= 0 and v.max() <= 255 and (t * b0[..., None] + u * b1[..., None] + (1 << 21)).max() < 2 ** 31
    inside = in00.astype(np.int64) + in10 + in01 + in11
    return v.astype(np.uint8), inside, sx, sy, X, Y


def live(plan, n, p):
    """Whether the pixel kernel paints record (n, p): the header's degenerate-record rule."""
    F = len(plan.sizes)
    f = int(plan.frame[n, p])
    if not 0 <= f < F:
        return False
    fh, fw = plan.sizes[f]
    x0, y0, w, h = (int(v) for v in plan.window[n, p])
    dx0, dy0, dw, dh = (int(v) for v in plan.dest[n, p])
    window = w >= 1 and h >= 1 and x0 >= 0 and y0 >= 0 and x0 + w <= fw and y0 + h <= fh
    rect = dw >= 4 and dh >= 1 and dx0 >= 0 and dy0 >= 0 and dx0 % 4 == 0 and dw % 4 == 0 and dx0 + dw <= plan.width and dy0 + dh <= plan.height
    return window and rect and inv_ok(plan.inv[n, p])


def expected_canvas(frames, plan, fill=(0, 0, 0), hole_fill=(0, 0, 0), border=(0, 0, 0)):
    """frames: list of uint8 arrays [h_i, w_i, 3] -> [N, height, width, 3] uint8."""
    N, H, W = len(plan.n_place), plan.height, plan.width
    out = np.empty((N, H, W, 3), dtype=np.uint8)
    out[...] = np.asarray(fill[:3], dtype=np.uint8)
    for n in range(N):
        for p in reversed(range(min(max(int(plan.n_place[n]), 0), 4))):          # where two rectangles overlap, the lower slot wins
            if not live(plan, n, p):
                continue
            dx0, dy0, dw, dh = (int(v) for v in plan.dest[n, p])
            v = sample(frames[int(plan.frame[n, p])], plan.window[n, p], dw, dh, plan.inv[n, p], border)[0]
            out[n, dy0:dy0 + dh, dx0:dx0 + dw] = augment_ref.apply_colour(v, plan.colour[n, p])
        for (x0, y0, w, h) in plan.holes[n].tolist():
            if w > 0 and h > 0:
                out[n, max(y0, 0):max(min(y0 + h, H), 0), max(x0, 0):max(min(x0 + w, W), 0)] = np.asarray(hole_fill[:3], dtype=np.uint8)
    return out


# ----------------------------------------------------------------------------- boxes
def map_box(box, label, fwd, dest, min_area=1.0, min_visibility=0.0):
    """One box (x, y, w, h) through one placement's forward map -> (x, y, w, h) in canvas pixels, or None when it is dropped.  Every step
    is one float64 operation (numpy float64 scalars), in the order the header writes them."""
    f = np.float64
    x, y, bw, bh = (f(v) for v in box)
    m = [f(v) for v in fwd]
    dx0, dy0, dw, dh = (f(int(v)) for v in dest)
    with np.errstate(all="ignore"):
        xe, ye = x + bw, y + bh
        us, vs = [], []
        for (X, Y) in ((x, y), (xe, y), (x, ye), (xe, ye)):
            us.append((m[0] * X + m[1] * Y) + m[2])
            vs.append((m[3] * X + m[4] * Y) + m[5])
        if not all(np.isfinite(v) for v in [x, y, bw, bh] + us + vs):
            return None
        u1, u2 = min(min(min(us[0], us[1]), us[2]), us[3]), max(max(max(us[0], us[1]), us[2]), us[3])
        v1, v2 = min(min(min(vs[0], vs[1]), vs[2]), vs[3]), max(max(max(vs[0], vs[1]), vs[2]), vs[3])
        full = (u2 - u1) * (v2 - v1)
        if not np.isfinite(full):
            return None
        cu1, cu2 = min(max(u1, f(0)), dw), min(max(u2, f(0)), dw)
        cv1, cv2 = min(max(v1, f(0)), dh), min(max(v2, f(0)), dh)
        cw, ch = cu2 - cu1, cv2 - cv1
        area = cw * ch
        if not (cw > 0 and ch > 0 and area >= f(min_area) and area >= f(min_visibility) * full and int(label) >= 0):
            return None
        return (dx0 + cu1, dy0 + cv1, cw, ch)


def carries_boxes(plan, n, p):
    """The box kernel's view of a record: frame, w, h, dw, dh and the bounds of inv."""
    x0, y0, w, h = (int(v) for v in plan.window[n, p])
    dx0, dy0, dw, dh = (int(v) for v in plan.dest[n, p])
    return 0 <= int(plan.frame[n, p]) < len(plan.sizes) and w >= 1 and h >= 1 and dw >= 1 and dh >= 1 and inv_ok(plan.inv[n, p])


def expected_boxes(plan, boxes, labels, ids, count, Gout=None, min_area=1.0, min_visibility=0.0):
    """boxes [F, Gmax, 4] f64, labels / ids [F, Gmax] i64 (ids may be None), count [F] -> (boxes [N, Gout, 4] f64, labels, ids or None,
    count [N] i32): kept boxes in placement order, then source order; slots beyond count are zero."""
    boxes = np.asarray(boxes, dtype=np.float64)
    N, Gmax = len(plan.n_place), boxes.shape[1]
    Gout = int(plan.n_place.max()) * Gmax if Gout is None else Gout
    ob, ol, oc = np.zeros((N, Gout, 4), np.float64), np.zeros((N, Gout), np.int64), np.zeros((N,), np.int32)
    oi = np.zeros((N, Gout), np.int64) if ids is not None else None
    for n in range(N):
        k = 0
        for p in range(min(max(int(plan.n_place[n]), 0), 4)):
            if not carries_boxes(plan, n, p):
                continue
            fr = int(plan.frame[n, p])
            for j in range(min(max(int(count[fr]), 0), Gmax)):
                b = map_box(boxes[fr, j], labels[fr, j], plan.fwd[n, p], plan.dest[n, p], min_area, min_visibility)
                if b is None:
                    continue
                ob[n, k], ol[n, k] = b, labels[fr, j]
                if oi is not None:
                    oi[n, k] = ids[fr, j]
                k += 1
        oc[n] = k
    return ob, ol, oi, oc
