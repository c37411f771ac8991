"""Test-only yardstick for the training augmentation (numpy): the two rules of include/centernet_gfx950.h (cnl_augment_u8,
cnl_augment_boxes_f64) restated on their own, the canvas built on the resize of tests/letterbox_ref.py's yardstick
(oracle/decode_ref.resize_bilinear_u8), plus a restatement of the colour composition.  A plan is read through its arrays only
(n_place, frame, window, dest, flip, colour, holes, height, width): nothing of the package is imported here."""
import math

import numpy as np

import decode_ref

LUMA = (0.299, 0.587, 0.114)
YIQ = ((0.299, 0.587, 0.114), (0.5959, -0.2746, -0.3213), (0.2115, -0.5227, 0.3112))


# ----------------------------------------------------------------------------- colour
def compose_colour(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, order=(0, 1, 2, 3), contrast_center=128):
    """The four ColorJitter factors applied in `order` (0 brightness, 1 contrast, 2 saturation, 3 hue) as 4 x 4 homogeneous matrices in
    float64, multiplied up and quantised with rint to Q12: int32 [12], nine entries (|.| <= 32767) row by row, then three offsets times
    4096 (|.| <= 2^21)."""
    T = np.array(YIQ, dtype=np.float64)
    total = np.eye(4)
    for op in order:
        A = np.eye(4)
        if op == 0:
            A[:3, :3] *= brightness
        elif op == 1:
            A[:3, :3] *= contrast
            A[:3, 3] = (1.0 - contrast) * contrast_center
        elif op == 2:
            A[:3, :3] = saturation * np.eye(3) + (1.0 - saturation) * np.tile(np.array(LUMA, dtype=np.float64), (3, 1))
        else:
            c, s = math.cos(2.0 * math.pi * hue), math.sin(2.0 * math.pi * hue)
            A[:3, :3] = np.linalg.inv(T) @ np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]]) @ T
        total = A @ total
    q = np.empty(12, dtype=np.int32)
    q[:9] = np.clip(np.rint(total[:3, :3] * 4096.0), -32767, 32767).reshape(9)
    q[9:] = np.clip(np.rint(total[:3, 3] * 4096.0), -2 ** 21, 2 ** 21)
    return q


def apply_colour(rgb, q):
    """uint8 [..., 3] -> uint8 [..., 3]: out_c = clamp((q[3c] R + q[3c + 1] G + q[3c + 2] B + q[9 + c] + 2048) >> 12, 0, 255), >> a floor."""
    q = np.asarray(q, dtype=np.int64)
    x = np.asarray(rgb).astype(np.int64)
    out = np.empty(x.shape, dtype=np.uint8)
    for c in range(3):
        t = (q[3 * c] * x[..., 0] + q[3 * c + 1] * x[..., 1] + q[3 * c + 2] * x[..., 2] + q[9 + c] + 2048) >> 12
        out[..., c] = np.clip(t, 0, 255)
    return out


# ----------------------------------------------------------------------------- canvas
def expected_canvas(frames, plan, fill=(0, 0, 0), hole_fill=(0, 0, 0)):
    """frames: list of uint8 arrays [h_i, w_i, 3] -> [N, height, width, 3] uint8."""
    N, H, W = len(plan.n_place), plan.height, plan.width
    out = np.empty((N, H, W, 3), dtype=np.uint8)
    out[...] = np.asarray(fill[:3], dtype=np.uint8)
    for n in range(N):
        for p in reversed(range(int(plan.n_place[n]))):          # where two rectangles overlap, the lower slot wins
            x0, y0, w, h = (int(v) for v in plan.window[n, p])
            dx0, dy0, dw, dh = (int(v) for v in plan.dest[n, p])
            window = frames[int(plan.frame[n, p])][y0:y0 + h, x0:x0 + w]
            r = decode_ref.resize_bilinear_u8(window[None], dh, dw)[0]
            if plan.flip[n, p]:
                r = r[:, ::-1]
            out[n, dy0:dy0 + dh, dx0:dx0 + dw] = apply_colour(r, plan.colour[n, p])
        for (x0, y0, w, h) in plan.holes[n].tolist():
            if w > 0 and h > 0:
                out[n, max(y0, 0):max(min(y0 + h, H), 0), max(x0, 0):max(min(x0 + w, W), 0)] = np.asarray(hole_fill[:3], dtype=np.uint8)
    return out


# ----------------------------------------------------------------------------- boxes
def map_box(box, label, window, dest, flip, min_area=1.0, min_visibility=0.0):
    """One box (x, y, w, h) through one placement -> (x, y, w, h) in canvas pixels, or None when it is dropped.  Every step is one
    float64 operation (numpy float64 scalars), in the order the header writes them."""
    f = np.float64
    x, y, bw, bh = (f(v) for v in box)
    x0, y0, w, h = (f(int(v)) for v in window)
    dx0, dy0, dw, dh = (f(int(v)) for v in dest)
    with np.errstate(all="ignore"):
        sx, sy = dw / w, dh / h
        u1, u2 = (x - x0) * sx, ((x + bw) - x0) * sx
        v1, v2 = (y - y0) * sy, ((y + bh) - y0) * sy
        if flip:
            u1, u2 = dw - u2, dw - u1
        full = (u2 - u1) * (v2 - v1)
        if not all(np.isfinite(v) for v in (x, y, bw, bh, u1, u2, v1, v2, full)):
            return None
        cu1, cu2 = min(max(u1, f(0)), dw), min(max(u2, f(0)), dw)
        cv1, cv2 = min(max(v1, f(0)), dh), min(max(v2, f(0)), dh)
        cw, ch = cu2 - cu1, cv2 - cv1
        area = cw * ch
        if not (cw > 0 and ch > 0 and area >= f(min_area) and area >= f(min_visibility) * full and int(label) >= 0):
            return None
        return (dx0 + cu1, dy0 + cv1, cw, ch)


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
        for p in range(int(plan.n_place[n])):
            fr = int(plan.frame[n, p])
            for j in range(min(max(int(count[fr]), 0), Gmax)):
                b = map_box(boxes[fr, j], labels[fr, j], plan.window[n, p], plan.dest[n, p], int(plan.flip[n, p]), min_area, min_visibility)
                if b is None:
                    continue
                ob[n, k], ol[n, k] = b, labels[fr, j]
                if oi is not None:
                    oi[n, k] = ids[fr, j]
                k += 1
        oc[n] = k
    return ob, ol, oi, oc
