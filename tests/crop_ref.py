"""Test-only yardstick for crop_detections / cnl_crop_boxes_u8 (numpy): the window, live and target rules restated on their own in
np.float32 / float64 scalars, and the pixels composed from the existing rules: oracle/decode_ref.resize_bilinear_u8 of the sliced
frame pasted onto the fill, as letterbox_ref.expected_canvas does, after yuv_ref.yuv420_to_rgb for YUV frames."""
import math

import numpy as np

import decode_ref
import yuv_ref

f32 = np.float32


def _clamp_to_int(v, limit):
    """Clamp in float32, then convert: t = v > 0 ? v : 0, then t < limit ? t : limit (a NaN becomes 0)."""
    v = v if v > f32(0) else f32(0)
    return int(v if v < limit else limit)


def window(box, H, W, pad=0.0, live=True):
    """box (x1, y1, x2, y2) in an H x W frame -> (x0, y0, w, h), or None for a dead slot.  Every step is one float32 operation."""
    x1, y1, x2, y2 = (f32(v) for v in box)
    pad, Wf, Hf = f32(pad), f32(W), f32(H)
    with np.errstate(all="ignore"):
        bw, bh = x2 - x1, y2 - y1
        px, py = pad * bw, pad * bh                                  # the product rounds, then the sum
        x0, xe = _clamp_to_int(np.floor(x1 - px), Wf), _clamp_to_int(np.ceil(x2 + px), Wf)
        y0, ye = _clamp_to_int(np.floor(y1 - py), Hf), _clamp_to_int(np.ceil(y2 + py), Hf)
    w, h = xe - x0, ye - y0
    if not live or not all(math.isfinite(float(v)) for v in (x1, y1, x2, y2)) or w < 1 or h < 1:
        return None
    return x0, y0, w, h


def is_live(j, n_count=None, score=None, threshold=None):
    """j < count[n] and score >= threshold (both in float32; a NaN score is not live); an absent input does not gate."""
    return (n_count is None or j < int(n_count)) and (score is None or bool(f32(score) >= f32(threshold)))


def geometry(h, w, crop_h, crop_w, keep_aspect):
    """(new_h, new_w, pad_top, pad_left) of an h x w window in a crop_h x crop_w crop: stretched, or letterbox_ref.geometry's rule
    (float64, round half to even, clamped to 1..target, centred with the odd pixel at the bottom / right)."""
    if not keep_aspect:
        return crop_h, crop_w, 0, 0
    r = min(float(crop_h) / float(h), float(crop_w) / float(w))
    new_h = min(crop_h, max(1, int(round(h * r))))
    new_w = min(crop_w, max(1, int(round(w * r))))
    return new_h, new_w, (crop_h - new_h) // 2, (crop_w - new_w) // 2


def crop_reference(frames, boxes, size, scores=None, threshold=None, count=None, pad=0.0, keep_aspect=False, fill=(0, 0, 0)):
    """frames: list of N uint8 arrays [h_i, w_i, C]; boxes [N, k, 4] float32 -> (crops [N, k, ch, cw, C] uint8, windows [N, k, 4] int32).
    Equal boxes of a frame are worked out once and equal windows resized once."""
    ch, cw = size
    boxes = np.asarray(boxes, dtype=np.float32)
    N, k = boxes.shape[:2]
    C = frames[0].shape[2]
    crops = np.empty((N, k, ch, cw, C), dtype=np.uint8)
    crops[...] = np.asarray(fill[:C], dtype=np.uint8)
    windows = np.zeros((N, k, 4), dtype=np.int32)
    for n, f in enumerate(frames):
        H, W = f.shape[:2]
        done, seen = {}, {}
        for j in range(k):
            live = is_live(j, None if count is None else count[n], None if scores is None else scores[n, j], threshold)
            key = (boxes[n, j].tobytes(), live)
            if key not in seen:
                seen[key] = window(boxes[n, j], H, W, pad, live)
            win = seen[key]
            if win is None:
                continue
            if win not in done:
                x0, y0, w, h = win
                nh, nw, pt, pl = geometry(h, w, ch, cw, keep_aspect)
                done[win] = (pt, pl, decode_ref.resize_bilinear_u8(f[y0:y0 + h, x0:x0 + w][None], nh, nw)[0])
            pt, pl, px = done[win]
            crops[n, j, pt:pt + px.shape[0], pl:pl + px.shape[1]] = px
            windows[n, j] = win
    return crops, windows


def crop_reference_yuv(planes, boxes, size, matrix="bt601", full_range=False, **kwargs):
    """planes: list of (y, u, v) -> crop_reference of the converted frames."""
    return crop_reference([yuv_ref.yuv420_to_rgb(y, u, v, matrix, full_range) for (y, u, v) in planes], boxes, size, **kwargs)
