"""YUV 4:2:0 video surfaces (NV12 from hardware decoders, I420 from software decoders) straight to the network-sized RGB canvas.

letterbox_yuv420 is letterbox_uint8 and tile_yuv420 is tile_uint8 for frames that are still Y / U / V planes: the colour conversion is
fused into the resize taps of ONE launch of cnl_letterbox_yuv420_u8 (csrc/letterbox.hip), so no RGB frame is written.  The result
is bit for bit "convert with the integer rule of include/centernet_gfx950.h, then letterbox_uint8 / tile_uint8".  The planes are read
in place, whatever their row pitch.

A frame is given as
    (a) one 2-D uint8 tensor [h * 3 / 2, w], the decoder / cv2 layout, read as NV12 or I420 according to `layout`,
    (b) (y [h, w], uv [h / 2, w / 2, 2]): NV12 planes, or
    (c) (y [h, w], u [h / 2, w / 2], v [h / 2, w / 2]): I420 planes
and `frames` is a sequence of such frames (or one [N, h * 3 / 2, w] tensor: N equal frames of form (a)).
"""
from fractions import Fraction
from typing import Tuple

import torch

from . import _gather
from .letterbox import LetterboxGeometry, _fill_word, letterbox_geometry
from .tiles import TileGeometry, _view_records

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


def _pitch(p: torch.Tensor, step: int) -> int:
    """Bytes between the rows of a plane whose samples are `step` bytes apart (a one-row plane has no pitch: its packed width)."""
    return int(p.stride(0)) if p.shape[0] > 1 else int(p.shape[1]) * step


def _parse(frames, layout: str, what: str):
    """-> [(y, u, v, y_pitch, c_pitch, c_step, h, w)] per frame; ValueError for what split_planes refuses and for pitches the record
    cannot express."""
    if layout not in LAYOUTS:
        raise ValueError(f"layout must be one of {list(LAYOUTS)}, got {layout!r}")
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 3:
            raise ValueError(f"expected a sequence of YUV 4:2:0 frames or one [N, h*3/2, w] tensor, got {tuple(frames.shape)}")
        frames = list(frames.unbind(0))
    frames = list(frames)
    if not frames:
        raise ValueError(f"{what}: no frames")
    parsed = []
    for f in frames:
        y, u, v = split_planes(f, layout)
        step = int(u.stride(1)) if u.shape[1] > 1 else 1
        yp, cp = _pitch(y, 1), _pitch(u, step)
        if _pitch(v, step) != cp:
            raise ValueError(f"the U and V planes of a frame must share one row pitch, got {cp} and {_pitch(v, step)}")
        if not (y.shape[1] <= yp < 2 ** 31 and u.shape[1] * step <= cp < 2 ** 31):
            raise ValueError(f"the rows of a plane must not overlap (pitch {yp} for {y.shape[1]} bytes, {cp} for {u.shape[1] * step})")
        parsed.append((y, u, v, yp, cp, step, int(y.shape[0]), int(y.shape[1])))
    return parsed


def _device(parsed, what: str):
    """The one HIP device all frames live on."""
    _gather.require_hip([p[0] for p in parsed], what)
    dev = parsed[0][0].device
    for p in parsed:
        if p[0].device != dev:
            raise ValueError(f"frames live on different devices ({dev}, {p[0].device})")
    return dev


def _records(parsed, windows):
    """What _gather.gather needs per window besides the window: the window's Y plane as a one-channel packed frame, and the planes."""
    plain = [(parsed[n][0].data_ptr() + y0 * parsed[n][3] + x0, parsed[n][3]) for (n, y0, x0, *_) in windows]
    planes = [(y.data_ptr(), u.data_ptr(), v.data_ptr(), yp, cp, step) for (y, u, v, yp, cp, step, _, _) in (parsed[w[0]] for w in windows)]
    return plain, planes


def letterbox_yuv420(frames, height: int, width: int, layout: str = "nv12", matrix: str = "bt601", full_range: bool = False, fill=(0, 0, 0)):
    """frames: a sequence of YUV 4:2:0 frames on one HIP device (forms (a), (b), (c) of the module docstring; sizes may differ)
    -> (canvas [N, height, width, 3] uint8 RGB, LetterboxGeometry): letterbox_uint8 of the converted frames, bit for bit, without the
    converted frames.  One launch; one pinned-memory upload (the tables); no device sync.  The geometry carries an ordinary
    cnl_letterbox_frame table: unletterbox / unletterbox_ take it as they take letterbox_uint8's."""
    coef = yuv_coefficients(matrix, full_range)
    parsed = _parse(frames, layout, "letterbox_yuv420")
    height, width = int(height), int(width)
    geo = [(p[6], p[7]) + letterbox_geometry(p[6], p[7], height, width) for p in parsed]
    word = _fill_word(fill, 3)
    dev = _device(parsed, "letterbox_yuv420")
    windows = [(n, 0, 0) + g for n, g in enumerate(geo)]
    plain, planes = _records(parsed, windows)
    g = _gather.gather(dev, windows, plain, height, width, 3, word, planes=planes, coef=coef)
    return g.canvas, LetterboxGeometry(g.table, geo, height, width, keep=parsed, yuv_table=g.yuv_table)


def tile_yuv420(frames, tile_h: int = 512, tile_w: int = 512, overlap: float = 0.2, full_frame: bool = True, fill=(0, 0, 0),
                layout: str = "nv12", matrix: str = "bt601", full_range: bool = False):
    """tile_uint8 for YUV 4:2:0 frames -> (views [V, tile_h, tile_w, 3] uint8 RGB, TileGeometry): the tile_grid tiles of every frame
    (windows into its planes; an odd origin takes the chroma sample of its 2 x 2 block) and, with full_frame, the whole frame
    letterboxed, converted and gathered by one launch.  merge_tiles takes the geometry as it takes tile_uint8's."""
    coef = yuv_coefficients(matrix, full_range)
    parsed = _parse(frames, layout, "tile_yuv420")
    word = _fill_word(fill, 3)
    sizes = [(p[6], p[7]) for p in parsed]
    windows, mg, views, ffv = _view_records(sizes, tile_h, tile_w, overlap, full_frame)
    dev = _device(parsed, "tile_yuv420")
    plain, planes = _records(parsed, windows)
    g = _gather.gather(dev, windows, plain, tile_h, tile_w, 3, word, planes=planes, coef=coef, merge_records=mg, frame_first_view=ffv)
    return g.canvas, TileGeometry(g.table, g.merge_table, g.first_view, views, ffv, sizes, tile_h, tile_w, keep=parsed, yuv_table=g.yuv_table)
