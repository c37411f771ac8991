"""Letterboxing: frames of different sizes -> one canvas batch, and decoded boxes back into each frame's own pixels.

The reference validates with keep-aspect resize + pad (configs/centernet.yaml val_data.transforms; datasets/inference.py carries
original_height / original_width) one image at a time on the host.  Here the geometry is host arithmetic on tensor SHAPES (no device
sync), the pixels are one launch of cnl_letterbox_bilinear_u8 and the boxes one launch of cnl_unletterbox_boxes_f32.
"""
from typing import List, Tuple

import torch

from . import _frames, _gather, _lib


def letterbox_geometry(h: int, w: int, height: int, width: int) -> Tuple[int, int, int, int]:
    """(new_h, new_w, pad_top, pad_left) of an h x w frame inside a height x width canvas.

    r = min(height / h, width / w) in float64; new_h = min(height, max(1, round(h * r))) and new_w likewise, with Python's round
    (half to even) — what albumentations' LongestMaxSize uses (py3round); for a square target this IS LongestMaxSize(max_size=height).
    pad_top = (height - new_h) // 2, pad_left = (width - new_w) // 2, the rest goes to the bottom / right: albumentations'
    PadIfNeeded(position="center").  The border is a CONSTANT colour, not albumentations' default reflected border: a reflected border
    shows the network real objects twice.  albumentations is restated from its published behaviour ("parity unpinned", as
    oracle/decode_ref.resize_bilinear_u8 states for cv2.resize).

    height and width must be positive multiples of 32 (the model's requirement), h and w at least 1; otherwise ValueError."""
    for name, v in (("h", h), ("w", w), ("height", height), ("width", width)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"letterbox_geometry: {name} must be an int, got {v!r}")
    if h < 1 or w < 1:
        raise ValueError(f"letterbox_geometry: frame size {h} x {w} must be at least 1 x 1")
    if height < 32 or width < 32 or height % 32 or width % 32:
        raise ValueError(f"letterbox_geometry: target {height} x {width} must be positive multiples of 32")
    r = min(height / h, width / w)
    new_h = min(height, max(1, round(h * r)))
    new_w = min(width, max(1, round(w * r)))
    return new_h, new_w, (height - new_h) // 2, (width - new_w) // 2


MAX_SCALES = 8          # the engine keeps up to 8 plans, one per input shape


def multiscale_sizes(height: int, width: int, scales) -> List[Tuple[int, int]]:
    """The canvases of a multi-scale test: [(h_s, w_s)] with h_s = 32 * max(1, floor(height * s / 32 + 0.5)) and w_s likewise, in the
    order of `scales` (1 to 8 finite positive numbers).  Two scales that give the same canvas are a ValueError, like any other bad value."""
    import math
    for name, v in (("height", height), ("width", width)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"multiscale_sizes: {name} must be a positive int, got {v!r}")
    if isinstance(scales, (str, bytes)) or not hasattr(scales, "__iter__"):
        raise ValueError(f"multiscale_sizes: scales must be a sequence of numbers, got {scales!r}")
    scales = list(scales)
    if not 1 <= len(scales) <= MAX_SCALES:
        raise ValueError(f"multiscale_sizes: 1 to {MAX_SCALES} scales, got {len(scales)}")
    sizes = []
    for s in scales:
        if isinstance(s, bool) or not isinstance(s, (int, float)) or not math.isfinite(s) or s <= 0:
            raise ValueError(f"multiscale_sizes: a scale must be a finite positive number, got {s!r}")
        size = tuple(32 * max(1, math.floor(v * s / 32 + 0.5)) for v in (height, width))
        if size in sizes:
            raise ValueError(f"multiscale_sizes: scales {scales[sizes.index(size)]!r} and {s!r} both give the canvas {size[0]} x {size[1]}")
        sizes.append(size)
    return sizes


class LetterboxGeometry:
    """What letterbox_uint8 did to each frame: `table` is the device array of cnl_letterbox_frame records the kernels read,
    `frames` the host-side list of (h, w, new_h, new_w, pad_top, pad_left), `height` / `width` the canvas size; `yuv_table` is the
    device array of cnl_yuv420_frame records letterbox_yuv420's launch read, None for packed frames."""

    def __init__(self, table: torch.Tensor, frames: List[Tuple[int, int, int, int, int, int]], height: int, width: int, keep=(),
                 yuv_table=None):
        self.table = table
        self.yuv_table = yuv_table
        self.frames = frames
        self.height = height
        self.width = width
        self._keep = keep          # the (possibly copied) source frames: the table holds their addresses

    def __len__(self):
        return len(self.frames)

    def __repr__(self):
        return f"LetterboxGeometry(n={len(self.frames)}, canvas={self.height}x{self.width})"


def letterbox_frames(frames, height: int, width: int, fill=(0, 0, 0), pixel_format: str = "rgb", matrix: str = "bt601", full_range: bool = False):
    """The one function behind letterbox_uint8 (pixel_format "rgb") and letterbox_yuv420 ("nv12" / "i420"), which detect_frames calls with
    its pixel_format: frame source -> geometry -> one gather."""
    src = _frames.open_frames(frames, pixel_format, "letterbox_uint8" if pixel_format == "rgb" else "letterbox_yuv420", matrix, full_range)
    height, width = int(height), int(width)
    geo = [(h, w) + letterbox_geometry(h, w, height, width) for (h, w) in src.sizes]
    word = _frames.fill_word(fill, src.C)
    windows = [(n, 0, 0) + g for n, g in enumerate(geo)]
    plain, planes = src.records(windows)
    dev = src.check_device()                     # (YUV frames: only now, after the canvas and the fill)
    g = _gather.gather(dev, windows, plain, height, width, src.C, word, planes=planes, coef=src.coef)
    return g.canvas, LetterboxGeometry(g.table, geo, height, width, keep=src.keep, yuv_table=g.yuv_table)


def letterbox_uint8(frames, height: int, width: int, fill=(0, 0, 0)):
    """frames: a sequence of uint8 [h_i, w_i, C] tensors on one HIP device (C in 1..4, the same for all), or one [N, h, w, C] tensor
    -> (canvas [N, height, width, C] uint8, LetterboxGeometry).  One launch; one pinned-memory upload (the table); no device sync."""
    return letterbox_frames(frames, height, width, fill)


def letterbox_yuv420(frames, height: int, width: int, layout: str = "nv12", matrix: str = "bt601", full_range: bool = False, fill=(0, 0, 0)):
    """frames: a sequence of YUV 4:2:0 frames on one HIP device (forms (a), (b), (c) of yuv.py's docstring; sizes may differ)
    -> (canvas [N, height, width, 3] uint8 RGB, LetterboxGeometry): letterbox_uint8 of the converted frames, bit for bit, without the
    converted frames.  One launch; one pinned-memory upload (the tables); no device sync.  The geometry carries an ordinary
    cnl_letterbox_frame table: unletterbox / unletterbox_ take it as they take letterbox_uint8's."""
    return letterbox_frames(frames, height, width, fill, _frames.yuv_layout(layout), matrix, full_range)


def unletterbox_(bboxes: torch.Tensor, geom: LetterboxGeometry, clip: bool = True) -> torch.Tensor:
    """In place: [N, k, 4] x1 y1 x2 y2 in canvas pixels -> each frame's own pixels."""
    _gather.require_hip([bboxes], "unletterbox")                  # first and whatever N: anything but a device tensor is a RuntimeError here
    _frames.check_boxes(bboxes, len(geom), geom.table.device, "unletterbox")
    lib = _lib.load()
    with torch.cuda.device(bboxes.device):
        _lib.check(lib.cnl_unletterbox_boxes_f32(bboxes.data_ptr(), geom.table.data_ptr(), bboxes.shape[0], bboxes.shape[1], int(bool(clip)),
                                                 _lib.stream(bboxes.device)), "cnl_unletterbox_boxes_f32")
    return bboxes


def unletterbox(bboxes: torch.Tensor, geom: LetterboxGeometry, clip: bool = True) -> torch.Tensor:
    """A new tensor: the boxes gather_detection2d / gather_tracking2d return for normalize_bbox=False, in each frame's own pixel
    coordinates; clip=True clamps them to [0, w] x [0, h]."""
    _gather.require_hip([bboxes], "unletterbox")
    return unletterbox_(bboxes.clone(memory_format=torch.contiguous_format), geom, clip)
