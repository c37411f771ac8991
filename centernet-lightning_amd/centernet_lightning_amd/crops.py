"""Detected objects cut out of their frames at one fixed size, on the GPU: the step between the detector and a second-stage network
(re-ID, attributes, helmet / no helmet) or event thumbnails.

crop_detections takes the frames detect_frames / detect_tiled were given (packed uint8 or YUV 4:2:0 surfaces, mixed sizes, read in place)
and the boxes they returned, still on the device, and makes one call of cnl_crop_boxes_u8 (csrc/letterbox.hip): a record kernel turns every
box into a window record of its frame, and the letterbox kernel body runs over those records.  A crop is therefore bit for bit
letterbox_uint8 of the sliced frame.  The host uploads the N whole-frame records and nothing else: no device sync, no per-box work.

The window, live and target rules are stated in include/centernet_gfx950.h (cnl_crop_boxes_u8) and restated in numpy by
tests/crop_ref.py.
"""
import ctypes
import math

import torch

from . import _frames, _gather, _lib


def _size(size):
    try:
        ch, cw = size
    except (TypeError, ValueError):
        raise ValueError(f"size must be (height, width), got {size!r}") from None
    for v in (ch, cw):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"size must be two ints, got {size!r}")
    if ch < 1 or cw < 4 or cw % 4:
        raise ValueError(f"crop size {ch} x {cw} needs a height >= 1 and a width that is a positive multiple of 4")
    return ch, cw


def crop_detections(frames, bboxes, size=(128, 64), scores=None, score_threshold=None, count=None, pad: float = 0.0,
                    keep_aspect: bool = False, fill=(0, 0, 0), pixel_format: str = "rgb", matrix: str = "bt601", full_range: bool = False):
    """frames: what letterbox_uint8 (pixel_format "rgb": a sequence of uint8 [h_i, w_i, C] tensors or one [N, h, w, C] tensor) or
    letterbox_yuv420 ("nv12" / "i420": any of its plane forms at any pitch, read in place) accept; bboxes: contiguous float32 [N, k, 4]
    x1 y1 x2 y2 on the same device, in each frame's own pixels
    -> (crops [N, k, size[0], size[1], C] uint8, windows [N, k, 4] int32 (x0, y0, w, h)), both on the device.

    The window of a box is floor / ceil of its corners after growing it by `pad` times its size on every side, clipped to the frame.
    keep_aspect=False stretches the window to `size`; True letterboxes it (letterbox_geometry's rule) on `fill`.  A slot is dead, its
    crop all `fill` and its window (0, 0, 0, 0), when j >= count[n] (count: int32 [N], detect_tiled's), when scores[n, j] <
    score_threshold (scores: float32 [N, k], given together with the threshold), when a coordinate is not finite or when the window is
    empty.  size[1] must be a multiple of 4.  `matrix` and `full_range` choose the YUV conversion as in letterbox_yuv420; "rgb" ignores
    both (nothing is converted).  One pinned upload (the N frame records), two launches, no device sync."""
    what = "crop_detections"
    ch, cw = _size(size)
    if isinstance(pad, bool) or not isinstance(pad, (int, float)) or not math.isfinite(pad) or pad < 0:
        raise ValueError(f"pad must be a finite number >= 0, got {pad!r}")
    _frames.check_score_pair(scores, score_threshold)
    src = _frames.open_frames(frames, pixel_format, what, matrix, full_range)
    dev, C, N = src.check_device(), src.C, len(src)
    word = _frames.fill_word(fill, C)
    k = _frames.check_boxes(bboxes, N, dev, what)
    if scores is not None:
        scores = _frames.per_slot(scores, "scores", torch.float32, (N, k), dev, what)
    if count is not None:
        count = _frames.per_slot(count, "count", torch.int32, (N,), dev, what)

    windows = src.whole()
    buf = _gather.pack_records(windows, *src.records(windows))
    words = 9 if src.kind == _frames.YUV else 5                   # int64 words of a cnl_yuv420_frame / cnl_letterbox_frame
    coef = (ctypes.c_int32 * 6)(*src.coef) if src.coef is not None else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        table = _gather.upload(buf, dev)
        crops = torch.empty((N, k, ch, cw, C), device=dev, dtype=torch.uint8)
        out_windows = torch.empty((N, k, 4), device=dev, dtype=torch.int32)
        records = torch.empty((max(N * k, 1) * words,), device=dev, dtype=torch.int64)
        stream = _lib.stream(dev)
        _lib.check(lib.cnl_crop_boxes_u8(table.data_ptr(), bboxes.data_ptr(), scores.data_ptr() if scores is not None else None,
                                         float(score_threshold) if scores is not None else 0.0, count.data_ptr() if count is not None else None,
                                         N, k, C, coef, float(pad), int(bool(keep_aspect)), records.data_ptr(), out_windows.data_ptr(),
                                         crops.data_ptr(), ch, cw, word, stream), "cnl_crop_boxes_u8")
    return crops, out_windows
