"""Test-only yardstick for draw_detections / cnl_draw_boxes_u8 (numpy), written from the rule in include/centernet_gfx950.h: the live
rule, the corners in np.float32 (rint, the two clamps, the conversion), and the three layers of a slot (interior blend, ring, tag) as
boolean masks over the coordinates of a plane's samples, applied from slot k - 1 down to 0.  A plane is [h, w, channels] samples with
`sub`: sample (sy, sx) is the pixel (sy << sub, sx << sub), so the Y plane (sub 0) and the chroma planes (sub 1) go through the same
function.  Everything after the corners is integer: the comparisons are equality on bytes."""
import math

import numpy as np

f32 = np.float32

GLYPH_ROWS = {
    0: "01110 10001 10011 10101 11001 10001 01110", 1: "00100 01100 00100 00100 00100 00100 01110",
    2: "01110 10001 00001 00010 00100 01000 11111", 3: "11111 00010 00100 00010 00001 10001 01110",
    4: "00010 00110 01010 10010 11111 00010 00010", 5: "11111 10000 11110 00001 00001 10001 01110",
    6: "00110 01000 10000 11110 10001 10001 01110", 7: "11111 00001 00010 00100 01000 01000 01000",
    8: "01110 10001 10001 01110 10001 10001 01110", 9: "01110 10001 10001 01111 00001 00010 01100",
}
# GLYPHS[digit, row, column] (column 0 = the most significant of the five bits = the left column)
GLYPHS = np.array([[[ch == "1" for ch in row] for row in GLYPH_ROWS[d].split()] for d in range(10)], dtype=bool)
assert GLYPHS.shape == (10, 7, 5)


def is_live(j, n_count=None, score=None, threshold=None):
    """j < count[n] and score >= threshold (in float32; a NaN score is not live); an absent input does not gate."""
    return (n_count is None or j < int(n_count)) and (score is None or bool(f32(score) >= f32(threshold)))


def corner(x):
    """rintf, then v > -32768 ? v : -32768, then v < 32767 ? v : 32767, then int: one float32 operation per step."""
    with np.errstate(all="ignore"):
        v = np.rint(f32(x))
    v = v if v > f32(-32768) else f32(-32768)
    v = v if v < f32(32767) else f32(32767)
    return int(v)


def corners(box, live=True):
    """(X1, Y1, X2, Y2), or None for a dead slot."""
    if not live or not all(math.isfinite(float(f32(v))) for v in box):
        return None
    X1, Y1, X2, Y2 = (corner(v) for v in box)
    if X2 < X1 or Y2 < Y1:
        return None
    return X1, Y1, X2, Y2


def tag_bitmap(number, s):
    """The tag of `number` at scale s as a boolean [9 s, (6 d + 1) s] array: True where the pixel is text."""
    digits = [int(ch) for ch in str(int(number))]
    d = len(digits)
    out = np.zeros((9 * s, (6 * d + 1) * s), dtype=bool)
    for ty in range(out.shape[0]):
        for tx in range(out.shape[1]):
            gy, gx = ty // s - 1, tx // s - 1
            if 0 <= gy < 7 and gx >= 0:
                q, c = gx // 6, gx % 6
                out[ty, tx] = q < d and c < 5 and GLYPHS[digits[q], gy, c]
    return out


def paint_slot(plane, sub, cs, colour, text, thickness=2, fill_alpha=0, tag_scale=2, number=-1):
    """One slot with corners cs onto plane [h, w, nc] (modified); colour / text: nc values each."""
    X1, Y1, X2, Y2 = cs
    t, a, s = thickness, fill_alpha, tag_scale
    o = (t - 1) // 2
    i = t - o
    h, w = plane.shape[:2]
    y = (np.arange(h, dtype=np.int64) << sub)[:, None]
    x = (np.arange(w, dtype=np.int64) << sub)[None, :]
    colour, text = np.asarray(colour, dtype=np.int64), np.asarray(text, dtype=np.int64)
    if a > 0:
        inside = (X1 <= x) & (x <= X2) & (Y1 <= y) & (y <= Y2)
        plane[inside] = ((plane[inside].astype(np.int64) * (256 - a) + colour * a + 128) >> 8).astype(np.uint8)
    outer = (X1 - o <= x) & (x <= X2 + o) & (Y1 - o <= y) & (y <= Y2 + o)
    inner = (X1 + i <= x) & (x <= X2 - i) & (Y1 + i <= y) & (y <= Y2 - i)
    plane[outer & ~inner] = colour.astype(np.uint8)
    if s > 0 and number is not None and int(number) >= 0:
        bits = tag_bitmap(number, s)
        L, T = X1 - o, Y1 - o - 9 * s
        if T < 0:
            T = Y1 - o
        ty, tx = y - T, x - L
        in_tag = (0 <= ty) & (ty < bits.shape[0]) & (0 <= tx) & (tx < bits.shape[1])
        on = in_tag & bits[np.clip(ty, 0, bits.shape[0] - 1), np.clip(tx, 0, bits.shape[1] - 1)]
        plane[in_tag] = colour.astype(np.uint8)
        plane[on] = text.astype(np.uint8)


def paint_plane(plane, sub, boxes, colours, text, numbers=None, scores=None, threshold=None, n_count=None, **style):
    """All k slots of one frame onto one plane [h, w, nc] (modified), from k - 1 down to 0; colours [k, nc]: the slot colours."""
    k = len(boxes)
    for j in range(k - 1, -1, -1):
        cs = corners(boxes[j], is_live(j, n_count, None if scores is None else scores[j], threshold))
        if cs is not None:
            paint_slot(plane, sub, cs, colours[j], text, number=-1 if numbers is None else numbers[j], **style)


def slot_colours(palette, labels, k):
    """palette [P, 3] -> [k, 3]: palette[labels[j] mod P] (numpy's % is the non-negative modulus), entry 0 without labels."""
    palette = np.asarray(palette, dtype=np.uint8)
    idx = np.zeros(k, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64) % len(palette)
    return palette[idx]


def _per_frame(a, n):
    return None if a is None else a[n]


def draw_reference(frames, boxes, palette, text=(255, 255, 255), labels=None, numbers=None, scores=None, threshold=None, count=None, **style):
    """frames: list of N uint8 [h_i, w_i, C] arrays (C = 3 or 4) -> painted copies.  palette, text: RGB bytes; channel 3 is carried."""
    out = [f.copy() for f in frames]
    for n, f in enumerate(out):
        k = len(boxes[n])
        paint_plane(f[:, :, :3], 0, boxes[n], slot_colours(palette, _per_frame(labels, n), k), text, _per_frame(numbers, n),
                    _per_frame(scores, n), threshold, _per_frame(count, n), **style)
    return out


def draw_reference_yuv(planes, boxes, palette, text, labels=None, numbers=None, scores=None, threshold=None, count=None, **style):
    """planes: list of (y [h, w], u [h/2, w/2], v [h/2, w/2]); palette [P, 3], text: ALREADY (Y, U, V) bytes -> painted copies."""
    out = []
    text = np.asarray(text)
    for n, (y, u, v) in enumerate(planes):
        y, u, v = y.copy(), u.copy(), v.copy()
        k = len(boxes[n])
        col = slot_colours(palette, _per_frame(labels, n), k)
        for plane, sub, ch in ((y, 0, 0), (u, 1, 1), (v, 1, 2)):
            paint_plane(plane[:, :, None], sub, boxes[n], col[:, ch:ch + 1], text[ch:ch + 1], _per_frame(numbers, n), _per_frame(scores, n),
                        threshold, _per_frame(count, n), **style)
        out.append((y, u, v))
    return out
