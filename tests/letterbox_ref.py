"""Test-only yardstick for the letterbox path (numpy, float64): the expected canvas built from oracle/decode_ref.resize_bilinear_u8,
and the box un-map in float64.  The geometry rule is restated here on its own (albumentations LongestMaxSize + PadIfNeeded(position=
"center") with a constant border, "parity unpinned": neither albumentations nor OpenCV is a dependency of the tests)."""
import numpy as np

import decode_ref


def geometry(h, w, height, width):
    """(new_h, new_w, pad_top, pad_left): r = min(height / h, width / w) in float64, sizes rounded half to even (py3round), clamped to
    1..target, centred with the odd pixel at the bottom / right."""
    r = min(float(height) / float(h), float(width) / float(w))
    new_h = min(height, max(1, int(round(h * r))))
    new_w = min(width, max(1, int(round(w * r))))
    return new_h, new_w, (height - new_h) // 2, (width - new_w) // 2


def expected_canvas(frames, height, width, fill):
    """frames: list of uint8 arrays [h_i, w_i, C] -> ([N, height, width, C] uint8, list of (h, w, new_h, new_w, pad_top, pad_left))."""
    C = frames[0].shape[2]
    out = np.empty((len(frames), height, width, C), dtype=np.uint8)
    out[...] = np.asarray(fill[:C], dtype=np.uint8)
    geo = []
    for i, f in enumerate(frames):
        h, w = f.shape[:2]
        nh, nw, pt, pl = geometry(h, w, height, width)
        out[i, pt:pt + nh, pl:pl + nw] = decode_ref.resize_bilinear_u8(f[None], nh, nw)[0]
        geo.append((h, w, nh, nw, pt, pl))
    return out, geo


def letterbox_points(xy, g):
    """Frame coordinates -> canvas coordinates (float64): x * (new_w / w) + pad_left, y * (new_h / h) + pad_top."""
    h, w, nh, nw, pt, pl = g
    xy = np.asarray(xy, dtype=np.float64)
    return np.stack([xy[..., 0] * (nw / w) + pl, xy[..., 1] * (nh / h) + pt], axis=-1)


def unletterbox_boxes(boxes, geo, clip=True):
    """boxes [N, k, 4] x1 y1 x2 y2 in canvas pixels -> float64 boxes in each frame's own pixels."""
    b = np.asarray(boxes, dtype=np.float64).copy()
    for n, (h, w, nh, nw, pt, pl) in enumerate(geo):
        sx, sy = nw / w, nh / h
        b[n, :, 0::2] = (b[n, :, 0::2] - pl) / sx
        b[n, :, 1::2] = (b[n, :, 1::2] - pt) / sy
        if clip:
            b[n, :, 0::2] = np.clip(b[n, :, 0::2], 0.0, float(w))
            b[n, :, 1::2] = np.clip(b[n, :, 1::2], 0.0, float(h))
    return b


def unletterbox_bound(boxes, geo):
    """Per-coordinate bound on |fp32 result - float64 result| of x' = (x - pad) / s with s = float(new) / float(old) formed in fp32.
    Each of the three fp32 operations (the ratio, the subtraction, the division) rounds once, relative error u = 2^-24 each:
        fl(s) = s (1 + e1),  fl(x - pad) = (x - pad)(1 + e2),  result = (x - pad)(1 + e2) / (s (1 + e1)) * (1 + e3)
    so |err| <= |x - pad| / s * (3u + O(u^2)) <= 4u (|x| + pad) / s.  Clamping to [0, size] (exact in fp32) cannot increase it."""
    b = np.abs(np.asarray(boxes, dtype=np.float64))
    out = np.empty_like(b)
    for n, (h, w, nh, nw, pt, pl) in enumerate(geo):
        out[n, :, 0::2] = 4.0 * 2.0 ** -24 * (b[n, :, 0::2] + pl) / (nw / w)
        out[n, :, 1::2] = 4.0 * 2.0 ** -24 * (b[n, :, 1::2] + pt) / (nh / h)
    return out
