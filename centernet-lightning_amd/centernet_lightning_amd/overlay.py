"""Detections drawn onto the frames they were found in, on the GPU: the output side of the frame pipeline (live preview, evidence
clips, the surface handed to a hardware encoder).  The reference does this on a host copy of every frame, one cv2.rectangle +
cv2.putText per box (utils/image_annotate.py::draw_boxes).

draw_detections takes the frames detect_frames / detect_tiled / crop_detections were given (packed uint8 RGB / RGBA or YUV 4:2:0
surfaces, mixed sizes, painted where they lie or as copies) and the boxes, labels and scores they returned, still on the device, and
makes one call of cnl_draw_boxes_u8 (csrc/overlay.hip): a record kernel turns every slot into an integer record, and a paint kernel
over the tiles of the frames applies the records that touch each tile, in order.  The host uploads the N whole-frame records and the
palette and nothing else: no device sync, no per-box work.

The rule (corners, ring, fill, tag, order, chroma) is stated in include/centernet_gfx950.h (cnl_draw_boxes_u8) and restated in numpy
by tests/overlay_ref.py.

DEFAULT_PALETTE is a fixed table of 20 distinct RGB colours (Sasha Trubetskoy's list of visually distinct colours, without its white
and black, which are the usual text colours): label l is drawn in entry l mod 20.
"""
import ctypes
import functools
import math

import numpy as np
import torch

from . import _gather, _lib
from . import yuv as _yuv

DEFAULT_PALETTE = ((230, 25, 75), (60, 180, 75), (255, 225, 25), (0, 130, 200), (245, 130, 48), (145, 30, 180), (70, 240, 240),
                   (240, 50, 230), (210, 245, 60), (250, 190, 212), (0, 128, 128), (220, 190, 255), (170, 110, 40), (255, 250, 200),
                   (128, 0, 0), (170, 255, 195), (128, 128, 0), (255, 215, 180), (0, 0, 128), (128, 128, 128))
MAX_SIDE = 32768
_WHAT = "draw_detections"


def _int_in(v, name, lo, hi):
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an int in {lo}..{hi}, got {v!r}")
    return v


def _colours(palette, text_color):
    """-> uint8 [P + 1, 3]: the palette, then the text colour."""
    try:
        pal = np.asarray(palette.cpu() if isinstance(palette, torch.Tensor) else palette)
        txt = np.asarray(text_color)
    except (TypeError, ValueError):
        raise ValueError("palette must be [P, 3] bytes and text_color three bytes") from None
    for a, name in ((pal, "palette"), (txt, "text_color")):
        if a.dtype.kind not in "iu" or a.size == 0 or a.min() < 0 or a.max() > 255:
            raise ValueError(f"{name} must hold integers in 0..255, got {a.dtype} {a.shape}")
    if pal.ndim != 2 or pal.shape[1] != 3 or not 1 <= pal.shape[0] <= 256:
        raise ValueError(f"palette must be [P, 3] with 1 <= P <= 256, got {pal.shape}")
    if txt.shape != (3,):
        raise ValueError(f"text_color must be three bytes, got {txt.shape}")
    return np.concatenate([pal, txt[None]]).astype(np.uint8)


@functools.lru_cache(maxsize=16)
def _to_yuv(rgb_bytes: bytes, matrix: str, full_range: bool) -> bytes:
    rgb = np.frombuffer(rgb_bytes, dtype=np.uint8).reshape(-1, 3)
    return np.array([_yuv.rgb_to_yuv(c, matrix, full_range) for c in rgb.tolist()], dtype=np.uint8).tobytes()


def _per_slot(t, name, dtype, shape, dev):
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a tensor, got {type(t).__name__}")
    _gather.require_hip([t], _WHAT)
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"expected contiguous {dtype} {name} of shape {list(shape)}, got {t.dtype} {tuple(t.shape)}")
    if t.device != dev:
        raise ValueError(f"{name} lives on {t.device}, the frames on {dev}")
    return t


def _dense(t):
    return t.clone(memory_format=torch.contiguous_format)


def _packed(frames, inplace):
    """-> (what to return, the per-frame views to paint, their device, C); device and C are None for an empty batch."""
    if isinstance(frames, torch.Tensor):
        if frames.dim() != 4:
            raise ValueError(f"expected a sequence of uint8 [h,w,C] frames or one [N,h,w,C] tensor, got {tuple(frames.shape)}")
        _gather.require_hip([frames], _WHAT)
        if frames.dtype != torch.uint8:
            raise ValueError(f"expected uint8 frames, got {frames.dtype}")
        out = frames if inplace else _dense(frames)
        views = list(out.unbind(0))
    else:
        views = list(frames)
        if views:
            views, _, _ = _gather.uint8_frames(views, _WHAT)
            if not inplace:
                views = [_dense(f) for f in views]
        out = tuple(views) if isinstance(frames, tuple) else views
    if not views:
        return out, views, None, None
    views, dev, C = _gather.uint8_frames(views, _WHAT)
    if C not in (3, 4):
        raise ValueError(f"packed frames have 3 or 4 channels (RGB / RGBA), got C = {C}")
    return out, views, dev, C


def _packed_records(views, C):
    plain = []
    for f in views:
        h, w = int(f.shape[0]), int(f.shape[1])
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"frame sides must be in 1..{MAX_SIDE}, got {h} x {w}")
        pitch = int(f.stride(0)) if h > 1 else w * C
        if f.stride(2) != 1 or (w > 1 and f.stride(1) != C) or not w * C <= pitch < 2 ** 31:
            raise ValueError(f"a frame painted in place needs packed pixels and rows that do not overlap, got strides {f.stride()}")
        plain.append((f.data_ptr(), pitch))
    return plain


def _yuv_copy(frames, layout):
    if isinstance(frames, torch.Tensor):
        return _dense(frames)
    out = []
    for f in frames:
        if isinstance(f, torch.Tensor):
            out.append(_dense(f))
        elif isinstance(f, (tuple, list)) and all(isinstance(p, torch.Tensor) for p in f):
            out.append(type(f)(_dense(p) for p in f))
        else:
            raise ValueError("a YUV 4:2:0 frame is one [h*3/2, w] tensor, (y, uv) or (y, u, v)")
    return tuple(out) if isinstance(frames, tuple) else out


def draw_detections(frames, bboxes, labels=None, scores=None, score_threshold=None, count=None, numbers=None, palette=DEFAULT_PALETTE,
                    text_color=(255, 255, 255), thickness: int = 2, fill_alpha: int = 0, tag_scale: int = 2, pixel_format: str = "rgb",
                    matrix: str = "bt601", full_range: bool = False, inplace: bool = False):
    """frames: what crop_detections accepts (pixel_format "rgb": a sequence of uint8 [h_i, w_i, C] tensors or one [N, h, w, C] tensor,
    C = 3 or 4; "nv12" / "i420": any plane form of letterbox_yuv420 at any pitch); bboxes: contiguous float32 [N, k, 4] x1 y1 x2 y2 on the
    same device, in each frame's own pixels -> the painted frames in the form they were given (a list stays a list, one tensor one
    tensor, YUV forms keep their form).

    inplace=False paints dense copies and leaves the given memory as it is; inplace=True paints the given memory and returns it.
    Slot (n, j) is drawn when it is live (j < count[n], count: int32 [N]; scores[n, j] >= score_threshold, scores: float32 [N, k], given
    together with the threshold; a NaN score is not live), its coordinates are finite and, rounded half to even, x2 >= x1 and y2 >= y1.
    It is drawn in palette[labels[n, j] mod P] (labels: int64 [N, k]; entry 0 without): a ring `thickness` pixels wide with square
    corners, centred on the rounded box; the interior blended with fill_alpha / 256 of the colour (256: solid, 0: none); and, when
    tag_scale > 0 and numbers[n, j] >= 0 (numbers: int32 [N, k], e.g. track or class ids), the number in a 5 x 7 font scaled by
    tag_scale, `text_color` on the slot colour, above the box's top left corner (inside the box where there is no room above).  Slots
    are applied from k - 1 down to 0, so the top score ends on top.  palette ([P, 3], 1 <= P <= 256) and text_color are RGB bytes; for
    YUV frames they are converted by yuv.rgb_to_yuv(colour, matrix, full_range), the Y plane is painted per pixel and a chroma sample
    as its top left pixel.  Channel 3 of a 4-channel frame and every byte outside the visible pixels (pitch padding) keep their
    values.  One pinned upload (the N frame records and the palette), two launches, no device sync."""
    thickness = _int_in(thickness, "thickness", 1, 32)
    fill_alpha = _int_in(fill_alpha, "fill_alpha", 0, 256)
    tag_scale = _int_in(tag_scale, "tag_scale", 0, 8)
    colours = _colours(palette, text_color)
    if (scores is None) != (score_threshold is None):
        raise ValueError("scores and score_threshold are given together")
    if score_threshold is not None and (isinstance(score_threshold, bool) or not isinstance(score_threshold, (int, float))
                                        or math.isnan(score_threshold)):
        raise ValueError(f"score_threshold must be a number, got {score_threshold!r}")
    inplace = bool(inplace)
    if pixel_format == "rgb":
        out, views, dev, C = _packed(frames, inplace)
        planes = None
        if views:
            plain = _packed_records(views, C)
            windows = [(n, 0, 0, f.shape[0], f.shape[1], 1, 1, 0, 0) for n, f in enumerate(views)]
    elif pixel_format in _yuv.LAYOUTS:
        colours = np.frombuffer(_to_yuv(colours.tobytes(), _check_matrix(matrix), bool(full_range)), dtype=np.uint8).reshape(-1, 3)
        empty = frames.shape[0] == 0 if isinstance(frames, torch.Tensor) and frames.dim() == 3 else \
            (not isinstance(frames, torch.Tensor) and len(frames) == 0)
        if inplace:
            out = frames
            if pixel_format == "i420" and not empty:     # a form-(a) I420 tensor with a pitch is copied by split_planes: not paintable
                for f in (frames.unbind(0) if isinstance(frames, torch.Tensor) else frames):
                    if isinstance(f, torch.Tensor) and not f.is_contiguous():
                        raise ValueError("an I420 frame given as one tensor must be contiguous to be painted in place (its chroma planes "
                                         "are flat byte ranges); give (y, u, v) planes instead")
        else:
            out = _yuv_copy(frames, pixel_format)
        views, dev, C = [], None, 3
        if not empty:
            views = _yuv._parse(out, pixel_format, _WHAT)
            dev = _yuv._device(views, _WHAT)
            for p in views:
                if not (p[6] <= MAX_SIDE and p[7] <= MAX_SIDE):
                    raise ValueError(f"frame sides must be in 1..{MAX_SIDE}, got {p[6]} x {p[7]}")
            windows = [(n, 0, 0, p[6], p[7], 1, 1, 0, 0) for n, p in enumerate(views)]
            plain, planes = _yuv._records(views, windows)
    else:
        raise ValueError(f"pixel_format must be 'rgb' or one of {list(_yuv.LAYOUTS)}, got {pixel_format!r}")
    N = len(views)
    if not isinstance(bboxes, torch.Tensor):
        raise ValueError(f"bboxes must be a tensor, got {type(bboxes).__name__}")
    if bboxes.dtype != torch.float32 or bboxes.dim() != 3 or bboxes.shape[-1] != 4 or not bboxes.is_contiguous():
        raise ValueError(f"expected contiguous float32 [N,k,4] boxes, got {bboxes.dtype} {tuple(bboxes.shape)}")
    if bboxes.shape[0] != N:
        raise ValueError(f"boxes of {bboxes.shape[0]} frames against {N} frames")
    k = int(bboxes.shape[1])
    if N == 0:
        return out                               # no frames: nothing to paint
    _gather.require_hip([bboxes], _WHAT)
    if bboxes.device != dev:
        raise ValueError(f"boxes on {bboxes.device} against frames on {dev}")
    if labels is not None:
        labels = _per_slot(labels, "labels", torch.int64, (N, k), dev)
    if numbers is not None:
        numbers = _per_slot(numbers, "numbers", torch.int32, (N, k), dev)
    if scores is not None:
        scores = _per_slot(scores, "scores", torch.float32, (N, k), dev)
    if count is not None:
        count = _per_slot(count, "count", torch.int32, (N,), dev)
    if N > 65535:
        raise ValueError(f"at most 65535 frames per call, got {N}")
    if k == 0:
        return out

    words = 9 if planes is not None else 5                        # int64 words of a cnl_yuv420_frame / cnl_letterbox_frame
    P = colours.shape[0] - 1
    buf = np.zeros(N * words + (P + 2) // 2, dtype=np.int64)
    if planes is not None:
        _gather.pack_yuv(buf[:N * words].reshape(N, 9), windows, planes)
    else:
        _gather.pack_plain(buf[:N * words].reshape(N, 5), windows, plain)
    buf[N * words:].view(np.uint8)[:(P + 1) * 4].reshape(P + 1, 4)[:, :3] = colours       # P four-byte entries, then the text colour
    max_h, max_w = max(w[3] for w in windows), max(w[4] for w in windows)
    lib = _lib.load()
    with torch.cuda.device(dev):
        table = _gather.upload(buf, dev)
        records = torch.empty((N * k * 8,), device=dev, dtype=torch.int64)      # 64 bytes per slot
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def ptr(t):
            return t.data_ptr() if t is not None else None
        _lib.check(lib.cnl_draw_boxes_u8(table.data_ptr(), bboxes.data_ptr(), ptr(labels), ptr(numbers), ptr(scores),
                                         float(score_threshold) if scores is not None else 0.0, ptr(count), N, k, C, int(planes is not None),
                                         table[N * words:].data_ptr(), P, thickness, fill_alpha, tag_scale, int(max_h), int(max_w),
                                         records.data_ptr(), stream), "cnl_draw_boxes_u8")
    return out


def _check_matrix(matrix):
    if matrix not in _yuv.MATRICES:
        raise ValueError(f"matrix must be one of {sorted(_yuv.MATRICES)}, got {matrix!r}")
    return matrix
