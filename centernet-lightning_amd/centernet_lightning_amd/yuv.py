"""YUV 4:2:0 video surfaces (NV12 from hardware decoders, I420 from software decoders) straight to the network-sized RGB canvas.

letterbox.letterbox_yuv420 is letterbox_uint8 and tiles.tile_yuv420 is tile_uint8 for frames that are still Y / U / V planes: the colour
conversion is fused into the resize taps of ONE launch of cnl_letterbox_yuv420_u8 (csrc/letterbox.hip), so no RGB frame is written.
The result is bit for bit "convert with the integer rule of include/centernet_gfx950.h, then letterbox_uint8 / tile_uint8".  The
planes are read in place, whatever their row pitch.  This module holds what is YUV about that: the plane forms and the two colour
rules; the frame source (_frames.open_frames) turns the planes into records.

A frame is given as
    (a) one 2-D uint8 tensor [h * 3 / 2, w], the decoder / cv2 layout, read as NV12 or I420 according to `layout`,
    (b) (y [h, w], uv [h / 2, w / 2, 2]): NV12 planes, or
    (c) (y [h, w], u [h / 2, w / 2], v [h / 2, w / 2]): I420 planes
and `frames` is a sequence of such frames (or one [N, h * 3 / 2, w] tensor: N equal frames of form (a)).
"""
from fractions import Fraction
from typing import Tuple

import torch

LAYOUTS = ("nv12", "i420")
# (Kr, Kb) of Y = Kr R + (1 - Kr - Kb) G + Kb B
MATRICES = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}
# OpenCV's cvtColor constants (ITUR_BT_601_SHIFT = 20: 1.164, 1.596, -0.813, -0.391, 2.018 times 2^20, truncated)
_OPENCV_BT601 = (16, 1220542, 1673527, -852492, -409993, 2116026)


def yuv_coefficients(matrix: str = "bt601", full_range: bool = False) -> Tuple[int, int, int, int, int, int]:
    """(y_off, CY, CVR, CVG, CUG, CUB): the six integers of cnl_letterbox_yuv420_u8's conversion rule (20 fractional bits).

    bt601 limited range is OpenCV's own constant set, so that the result is cvtColor's.  Every other combination is
    round(c * 2**20) of the standard matrix: with Kg = 1 - Kr - Kb and s the chroma excursion scale (255 / 224 limited, 1 full),
    CVR = 2 (1 - Kr) s, CVG = -2 (1 - Kr) Kr / Kg s, CUG = -2 (1 - Kb) Kb / Kg s, CUB = 2 (1 - Kb) s; CY = 255 / 219 with y_off = 16 for
    limited range, exactly 1 << 20 with y_off = 0 for full range."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    full_range = bool(full_range)
    if matrix == "bt601" and not full_range:
        return _OPENCV_BT601
    kr, kb = MATRICES[matrix]
    kg = 1 - kr - kb
    s = Fraction(1) if full_range else Fraction(255, 224)
    c = (2 * (1 - kr) * s, -2 * (1 - kr) * kr / kg * s, -2 * (1 - kb) * kb / kg * s, 2 * (1 - kb) * s)
    cy = 1 << 20 if full_range else round(Fraction(255, 219) * 2 ** 20)
    return (0 if full_range else 16, cy) + tuple(round(v * 2 ** 20) for v in c)


def rgb_to_yuv(color, matrix: str = "bt601", full_range: bool = False) -> Tuple[int, int, int]:
    """(R, G, B) bytes -> (Y, U, V) bytes of the standard matrix, exact in Fractions: with (Kr, Kb) = MATRICES[matrix] and
    Kg = 1 - Kr - Kb, Y = Kr R + Kg G + Kb B, Cb = (B - Y) / (2 (1 - Kb)), Cr = (R - Y) / (2 (1 - Kr)); limited range gives
    16 + 219/255 Y, 128 + 224/255 Cb, 128 + 224/255 Cr, full range Y, 128 + Cb, 128 + Cr; each rounded half to even and clamped to
    0..255.  The forward direction of yuv_coefficients: what draw_detections paints a YUV surface with."""
    if matrix not in MATRICES:
        raise ValueError(f"matrix must be one of {sorted(MATRICES)}, got {matrix!r}")
    try:
        r, g, b = (int(v) for v in color)
    except (TypeError, ValueError):
        raise ValueError(f"a colour is three bytes (R, G, B), got {color!r}") from None
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError(f"a colour is three bytes (R, G, B), got {color!r}")
    kr, kb = MATRICES[matrix]
    y = kr * r + (1 - kr - kb) * g + kb * b
    cb, cr = (b - y) / (2 * (1 - kb)), (r - y) / (2 * (1 - kr))
    if bool(full_range):
        out = (y, 128 + cb, 128 + cr)
    else:
        out = (16 + Fraction(219, 255) * y, 128 + Fraction(224, 255) * cb, 128 + Fraction(224, 255) * cr)
    return tuple(min(max(round(v), 0), 255) for v in out)


def split_planes(frame, layout: str = "nv12"):
    """One frame in form (a), (b) or (c) -> (y [h, w], u [h / 2, w / 2], v [h / 2, w / 2]) as VIEWS of the given memory (for NV12, u and
    v are the two interleaved halves of the UV plane: element stride 2).  Nothing is copied except a form-(a) I420 tensor whose rows
    are not packed (its chroma planes are flat byte ranges).  ValueError for a wrong dtype, odd sizes, plane shapes that do not match,
    an innermost stride other than 1, or planes on different devices."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {list(LAYOUTS)}, got {layout!r}")
    planes = [frame] if isinstance(frame, torch.Tensor) else list(frame) if isinstance(frame, (tuple, list)) else None
    if planes is None or not 1 <= len(planes) <= 3 or not all(isinstance(p, torch.Tensor) for p in planes):
        raise ValueError("a YUV 4:2:0 frame is one [h*3/2, w] tensor, (y, uv) or (y, u, v)")
    for p in planes:
        if p.dtype != torch.uint8:
            raise ValueError(f"expected uint8 planes, got {p.dtype}")
        if p.device != planes[0].device:
            raise ValueError(f"the planes of a frame live on different devices ({planes[0].device}, {p.device})")
    if len(planes) == 1:
        t = planes[0]
        if t.dim() != 2 or t.shape[0] % 3 or t.shape[0] == 0:
            raise ValueError(f"expected one uint8 [h*3/2, w] tensor per frame, got {tuple(t.shape)}")
        h, w = t.shape[0] // 3 * 2, t.shape[1]
        if h % 2 or w % 2 or w == 0:
            raise ValueError(f"YUV 4:2:0 frames have even height and width, got {h} x {w}")
        if t.stride(1) != 1:
            raise ValueError(f"the innermost stride of a plane must be 1, got strides {t.stride()}")
        if layout == "nv12":
            y, uv = t[:h], t[h:].unflatten(1, (w // 2, 2))
            return y, uv[..., 0], uv[..., 1]
        flat = t.contiguous().view(-1)
        n = (h // 2) * (w // 2)
        return flat[:h * w].view(h, w), flat[h * w:h * w + n].view(h // 2, w // 2), flat[h * w + n:].view(h // 2, w // 2)
    y = planes[0]
    if y.dim() != 2:
        raise ValueError(f"expected a [h, w] Y plane, got {tuple(y.shape)}")
    h, w = y.shape
    if h % 2 or w % 2 or h == 0 or w == 0:
        raise ValueError(f"YUV 4:2:0 frames have even height and width, got {h} x {w}")
    if len(planes) == 2:
        uv = planes[1]
        if tuple(uv.shape) != (h // 2, w // 2, 2):
            raise ValueError(f"expected a [{h // 2}, {w // 2}, 2] UV plane beside a {h} x {w} Y plane, got {tuple(uv.shape)}")
        if uv.stride(2) != 1:
            raise ValueError(f"the innermost stride of a plane must be 1, got strides {uv.stride()}")
        u, v = uv[..., 0], uv[..., 1]
    else:
        u, v = planes[1], planes[2]
        if tuple(u.shape) != (h // 2, w // 2) or tuple(v.shape) != (h // 2, w // 2):
            raise ValueError(f"expected [{h // 2}, {w // 2}] U and V planes beside a {h} x {w} Y plane, got {tuple(u.shape)}, {tuple(v.shape)}")
    step = 2 if len(planes) == 2 else 1
    if y.stride(1) != 1 or (w > 2 and (u.stride(1) != step or v.stride(1) != step)):      # (a one-column plane has no element stride)
        raise ValueError(f"the innermost stride of a plane must be 1, got strides {y.stride()}, {u.stride()}, {v.stride()}")
    return y, u, v
