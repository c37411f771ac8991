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
import functools

import numpy as np
import torch

from . import _frames, _gather, _lib
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


def _clone(x):
    """Dense clones of a tensor, or of the tensors in a list / tuple of frames or planes, in the form given."""
    if isinstance(x, torch.Tensor):
        return x.clone(memory_format=torch.contiguous_format)
    return type(x)(_clone(p) for p in x) if isinstance(x, (tuple, list)) else x          # (not a frame: left for open_frames to refuse)


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
    _frames.check_score_pair(scores, score_threshold)
    if not isinstance(frames, (torch.Tensor, tuple, list)):
        frames = list(frames)
    out = frames if inplace else _clone(frames)
    src = _frames.open_frames(out, pixel_format, _WHAT, matrix, full_range, copy=_frames.IN_PLACE, allow_empty=True)
    dev, C, N = src.check_device(), src.C, len(src)
    if N and C not in (3, 4):
        raise ValueError(f"packed frames have 3 or 4 channels (RGB / RGBA), got C = {C}")
    for (h, w) in src.sizes:
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f"frame sides must be in 1..{MAX_SIDE}, got {h} x {w}")
    k = _frames.check_boxes(bboxes, N, dev, _WHAT)
    if N == 0:
        return out                               # no frames: nothing to paint
    if labels is not None:
        labels = _frames.per_slot(labels, "labels", torch.int64, (N, k), dev, _WHAT)
    if numbers is not None:
        numbers = _frames.per_slot(numbers, "numbers", torch.int32, (N, k), dev, _WHAT)
    if scores is not None:
        scores = _frames.per_slot(scores, "scores", torch.float32, (N, k), dev, _WHAT)
    if count is not None:
        count = _frames.per_slot(count, "count", torch.int32, (N,), dev, _WHAT)
    if N > 65535:
        raise ValueError(f"at most 65535 frames per call, got {N}")
    if k == 0:
        return out

    is_yuv = src.kind == _frames.YUV
    if is_yuv:
        colours = np.frombuffer(_to_yuv(colours.tobytes(), matrix, bool(full_range)), dtype=np.uint8).reshape(-1, 3)
    P = colours.shape[0] - 1
    windows = src.whole()
    buf = _gather.pack_records(windows, *src.records(windows), tail_words=(P + 2) // 2)
    words = 9 if is_yuv else 5                   # int64 words of a cnl_yuv420_frame / cnl_letterbox_frame
    buf[N * words:].view(np.uint8)[:(P + 1) * 4].reshape(P + 1, 4)[:, :3] = colours       # P four-byte entries, then the text colour
    max_h, max_w = max(h for (h, _) in src.sizes), max(w for (_, w) in src.sizes)
    lib = _lib.load()
    with torch.cuda.device(dev):
        table = _gather.upload(buf, dev)
        records = torch.empty((N * k * 8,), device=dev, dtype=torch.int64)      # 64 bytes per slot
        stream = _lib.stream(dev)

        def ptr(t):
            return t.data_ptr() if t is not None else None
        _lib.check(lib.cnl_draw_boxes_u8(table.data_ptr(), bboxes.data_ptr(), ptr(labels), ptr(numbers), ptr(scores),
                                         float(score_threshold) if scores is not None else 0.0, ptr(count), N, k, C, int(is_yuv),
                                         table[N * words:].data_ptr(), P, thickness, fill_alpha, tag_scale, int(max_h), int(max_w),
                                         records.data_ptr(), stream), "cnl_draw_boxes_u8")
    return out
