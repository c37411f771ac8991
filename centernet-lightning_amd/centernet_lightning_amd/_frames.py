"""The frame source: what letterbox_uint8 / letterbox_yuv420, tile_uint8 / tile_yuv420, crop_detections and draw_detections make of
"the frames" they are given, and the checks of the per-slot tensors (boxes, scores, counts, labels) that go with them.

open_frames turns frames + pixel_format into a Frames: the kept tensors, their device, the channel count, the sizes and the
(address, pitch) of every frame, by name.  Frames.records(windows) is what _gather.gather and _gather.pack_records take.  Host
arithmetic on shapes, strides and addresses only: no device sync, and nothing here loads the library.
"""
import math

import torch

from . import _gather
from . import yuv as _yuv

PACKED, YUV = "packed", "yuv"
# what open_frames may copy (YUV planes are read in place under every rule, with split_planes' one exception)
DENSE = "dense"              # every packed frame is made contiguous: rows w * C apart
ROWS = "rows"                # a packed frame with packed pixels and rows that do not overlap is read in place, any other is copied
IN_PLACE = "in_place"        # nothing is copied: a frame that cannot be read in place is refused


def fill_word(fill, C: int) -> int:
    vals = [fill] * 4 if isinstance(fill, int) else list(fill)
    if len(vals) < C or any((not isinstance(v, int)) or v < 0 or v > 255 for v in vals):
        raise ValueError(f"fill must be one uint8 value or at least {C} of them, got {fill!r}")
    word = 0
    for c, v in enumerate(vals[:4]):
        word |= v << (8 * c)
    return word


def _pitch(t: torch.Tensor, row_bytes: int) -> int:
    """Bytes between the rows of a frame or plane whose rows hold row_bytes bytes (a one-row tensor has no pitch: row_bytes)."""
    return int(t.stride(0)) if t.shape[0] > 1 else row_bytes


class Frames:
    """`kind`: PACKED or YUV; `C`: channels of the frames as the kernels see them (3 for YUV); `sizes`: [(h, w)]; `keep`: the tensors
    whose addresses the records carry (packed: one [h, w, C] tensor per frame, YUV: (y, u, v)); `coef`: the six conversion integers,
    None for packed frames; `device`: the one HIP device of all frames — of YUV frames once check_device has run; None for an
    empty batch."""

    def __init__(self, kind, what, keep, sizes, rows, C=3, planes=None, coef=None, device=None):
        self.kind, self.C, self.sizes, self.keep, self.coef = kind, C, sizes, keep, coef
        self._what, self.device = what, device
        self._rows = rows                        # per frame (address, pitch) of the packed frame / of the Y plane
        self._planes = planes                    # per YUV frame (y, u, v addresses, y_pitch, c_pitch, c_step)

    def __len__(self):
        return len(self.sizes)

    def check_device(self):
        """-> `device`.  Packed frames were checked when they were opened; YUV frames are checked here, a step of its own, because
        their callers have always refused a bad canvas, fill or tile size before frames in host memory."""
        if self.device is None and self.keep:
            ys = [y for (y, _, _) in self.keep]
            _gather.require_hip(ys, self._what)
            for y in ys:
                if y.device != ys[0].device:
                    raise ValueError(f"frames live on different devices ({ys[0].device}, {y.device})")
            self.device = ys[0].device
        return self.device

    def whole(self):
        """One window per frame: the whole frame, 1:1 (crop_detections' and draw_detections' frame records)."""
        return [(n, 0, 0, h, w, 1, 1, 0, 0) for n, (h, w) in enumerate(self.sizes)]

    def records(self, windows):
        """windows [(frame, y0, x0, ...)] -> (plain, planes): plain[i] = (address, row stride) of window i as a packed frame (of a YUV
        frame: its Y plane as one channel), planes[i] = (y, u, v addresses, y_pitch, c_pitch, c_step) of its frame, None for packed."""
        step = 1 if self.kind == YUV else self.C
        rows, plain = self._rows, []
        for w in windows:
            n, y0, x0 = w[:3]
            address, pitch = rows[n]
            plain.append((address + y0 * pitch + x0 * step, pitch))
        return plain, ([self._planes[w[0]] for w in windows] if self.kind == YUV else None)


def yuv_layout(layout):
    """The `layout` of letterbox_yuv420 / tile_yuv420 as a pixel_format."""
    if layout not in _yuv.LAYOUTS:
        raise ValueError(f"layout must be one of {list(_yuv.LAYOUTS)}, got {layout!r}")
    return layout


def open_frames(frames, pixel_format: str, what: str, matrix: str = "bt601", full_range: bool = False, copy: str = DENSE,
                allow_empty: bool = False) -> Frames:
    """pixel_format "rgb": a sequence of uint8 [h_i, w_i, C] tensors on one HIP device (C in 1..4, the same for all) or one [N, h, w, C]
    tensor; "nv12" / "i420": a sequence of YUV 4:2:0 frames in the forms of yuv.split_planes or one [N, h * 3 / 2, w] tensor, with the
    conversion `matrix` / `full_range` choose.  `copy`: DENSE, ROWS or IN_PLACE.  An empty batch is a ValueError unless allow_empty."""
    if pixel_format == "rgb":
        return _open_packed(frames, what, copy, allow_empty)
    if pixel_format in _yuv.LAYOUTS:
        return _open_yuv(frames, pixel_format, what, _yuv.yuv_coefficients(matrix, full_range), copy, allow_empty)
    raise ValueError(f"pixel_format must be 'rgb' or one of {list(_yuv.LAYOUTS)}, got {pixel_format!r}")


def _open_packed(frames, what, copy, allow_empty):
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4:
            raise ValueError(f"expected a sequence of uint8 [h,w,C] frames or one [N,h,w,C] tensor, got {tuple(frames.shape)}")
        _gather.require_hip([frames], what)
        if frames.dtype != torch.uint8:
            raise ValueError(f"expected uint8 frames, got {frames.dtype}")
        frames = (frames.contiguous() if copy == DENSE else frames).unbind(0)
    frames = list(frames)
    if not frames:
        if allow_empty:
            return Frames(PACKED, what, [], [], [], C=None)
        raise ValueError(f"{what}: no frames")
    _gather.require_hip(frames, what)
    dev, C = frames[0].device, frames[0].shape[-1] if frames[0].dim() == 3 else -1
    keep, sizes, rows = [], [], []
    for f in frames:
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[-1] != C or not 1 <= C <= 4:
            raise ValueError(f"expected uint8 [h,w,C<=4] frames with one C, got {f.dtype} {tuple(f.shape)}")
        if f.device != dev:
            raise ValueError(f"frames live on different devices ({dev}, {f.device})")
        h, w, _ = f.shape
        pitch = w * C
        if copy == DENSE:
            f = f.contiguous()
        else:
            # readable where it lies: pixels and channels packed, rows any pitch that does not overlap.  The two rules have always
            # differed on a one-column frame, which has no pixel stride: IN_PLACE takes any, ROWS copies the frame unless it is C.
            _, pixel, channel = f.stride()
            there = _pitch(f, pitch)
            if channel == 1 and (pixel == C or (copy == IN_PLACE and w <= 1)) and pitch <= there < 2 ** 31:
                pitch = there
            elif copy == IN_PLACE:
                raise ValueError(f"a frame painted in place needs packed pixels and rows that do not overlap, got strides {f.stride()}")
            else:
                f = f.contiguous()
        keep.append(f)
        sizes.append((h, w))
        rows.append((f.data_ptr(), pitch))
    return Frames(PACKED, what, keep, sizes, rows, C=C, device=dev)


def _open_yuv(frames, layout, what, coef, copy, allow_empty):
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 3:
            raise ValueError(f"expected a sequence of YUV 4:2:0 frames or one [N, h*3/2, w] tensor, got {tuple(frames.shape)}")
        frames = frames.unbind(0)
    frames = list(frames)
    if not frames and not allow_empty:
        raise ValueError(f"{what}: no frames")
    keep, sizes, rows, planes = [], [], [], []
    for f in frames:
        if copy == IN_PLACE and layout == "i420" and isinstance(f, torch.Tensor) and not f.is_contiguous():
            raise ValueError("an I420 frame given as one tensor must be contiguous to be painted in place (its chroma planes are flat "
                             "byte ranges, which split_planes copies); give (y, u, v) planes instead")
        y, u, v = _yuv.split_planes(f, layout)
        (h, w), cw = y.shape, u.shape[1]
        step = u.stride(1) if cw > 1 else 1
        c_bytes = cw * step
        yp, cp = _pitch(y, w), _pitch(u, c_bytes)
        if _pitch(v, c_bytes) != cp:
            raise ValueError(f"the U and V planes of a frame must share one row pitch, got {cp} and {_pitch(v, c_bytes)}")
        if not (w <= yp < 2 ** 31 and c_bytes <= cp < 2 ** 31):
            raise ValueError(f"the rows of a plane must not overlap (pitch {yp} for {w} bytes, {cp} for {c_bytes})")
        keep.append((y, u, v))
        sizes.append((h, w))
        address = y.data_ptr()
        rows.append((address, yp))
        planes.append((address, u.data_ptr(), v.data_ptr(), yp, cp, step))
    return Frames(YUV, what, keep, sizes, rows, planes=planes, coef=coef)


# ----------------------------------------------------------------------------- the per-slot tensors that come with the frames
def check_boxes(bboxes, N: int, dev, what: str) -> int:
    """bboxes must be a contiguous float32 [N, k, 4] tensor on the frames' HIP device `dev` -> k.  (An empty batch has no device.)"""
    if not isinstance(bboxes, torch.Tensor):
        raise ValueError(f"bboxes must be a tensor, got {type(bboxes).__name__}")
    if N:
        _gather.require_hip([bboxes], what)
    if bboxes.dtype != torch.float32 or bboxes.dim() != 3 or bboxes.shape[-1] != 4 or not bboxes.is_contiguous():
        raise ValueError(f"expected contiguous float32 [N,k,4] boxes, got {bboxes.dtype} {tuple(bboxes.shape)}")
    if bboxes.shape[0] != N or (N and bboxes.device != dev):
        raise ValueError(f"boxes of {bboxes.shape[0]} frames on {bboxes.device} against {N} frames on {dev}")
    return int(bboxes.shape[1])


def per_slot(t, name: str, dtype, shape, dev, what: str):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    _gather.require_hip([t], what)
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"expected contiguous {dtype} {name} of shape {list(shape)}, got {t.dtype} {tuple(t.shape)}")
    if t.device != dev:
        raise ValueError(f"{name} lives on {t.device}, the frames on {dev}")
    return t


def check_score_pair(scores, score_threshold) -> None:
    if (scores is None) != (score_threshold is None):
        raise ValueError("scores and score_threshold are given together")
    if score_threshold is not None and (isinstance(score_threshold, bool) or not isinstance(score_threshold, (int, float))
                                        or math.isnan(score_threshold)):
        raise ValueError(f"score_threshold must be a number, got {score_threshold!r}")
