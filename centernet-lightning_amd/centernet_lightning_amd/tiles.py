"""Sliced inference: frames larger than the network input are cut into overlapping network-sized tiles, the tiles run as one batch,
and the boxes of all views of a frame are merged in the frame's own pixels (duplicates from the overlaps removed on the GPU).

The geometry is host arithmetic on tensor SHAPES (no device sync).  The tile gather is ONE launch of cnl_letterbox_bilinear_u8: a tile
is a record whose src points inside a frame and whose resize is 1:1 (the kernel then returns the source bytes); the optional full-frame
view is the plain letterbox record.  The merge is cnl_merge_tiles_f32 (csrc/tile_merge.hip; the rule: include/centernet_gfx950.h).
"""
from typing import List, Tuple

import numpy as np
import torch

from . import _frames, _gather, _lib
from .letterbox import letterbox_geometry

METRICS = {"iou": 0, "ios": 1}


def _axis(size: int, tile: int, overlap: float) -> List[Tuple[int, int]]:
    """[(start, length)] of the tiles along one axis."""
    if size <= tile:
        return [(0, size)]
    step = tile - round(tile * overlap)
    n = -(-(size - tile) // step) + 1
    return [(min(i * step, size - tile), tile) for i in range(n)]


def tile_grid(h: int, w: int, tile_h: int = 512, tile_w: int = 512, overlap: float = 0.2) -> List[Tuple[int, int, int, int]]:
    """[(y0, x0, th, tw)], row-major, of the tiles of an h x w frame.

    Per axis (x shown): ov = round(tile_w * overlap) with Python's round, step = tile_w - ov.  w <= tile_w gives one tile x0 = 0, tw = w
    (the gather pads it to tile_w on the right).  Otherwise n = ceil((w - tile_w) / step) + 1 tiles of width tile_w at
    x0_i = min(i * step, w - tile_w): the last tile is shifted back so that every tile lies inside the frame.

    tile_h and tile_w must be positive multiples of 32, overlap in [0, 0.5], h and w at least 1; otherwise ValueError."""
    for name, v in (("h", h), ("w", w), ("tile_h", tile_h), ("tile_w", tile_w)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"tile_grid: {name} must be an int, got {v!r}")
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float)) or not 0.0 <= overlap <= 0.5:       # (NaN fails the comparison)
        raise ValueError(f"tile_grid: overlap must be a number in [0, 0.5], got {overlap!r}")
    if h < 1 or w < 1:
        raise ValueError(f"tile_grid: frame size {h} x {w} must be at least 1 x 1")
    if tile_h < 32 or tile_w < 32 or tile_h % 32 or tile_w % 32:
        raise ValueError(f"tile_grid: tile {tile_h} x {tile_w} must be positive multiples of 32")
    return [(y0, x0, th, tw) for (y0, th) in _axis(h, tile_h, overlap) for (x0, tw) in _axis(w, tile_w, overlap)]


class TileGeometry:
    """What tile_uint8 did.  `table`: the device array of cnl_letterbox_frame records, one per view; `merge_table`: the device array of
    the merge's view records ([V, 8] int32 words: frame_w, frame_h, x0, y0, pad_left, pad_top, and the bits of the floats sx, sy);
    `first_view`: device int32 [N + 1], frame n owns views first_view[n] .. first_view[n + 1] - 1 (`frame_first_view` is the same list
    on the host); `views`: the host list of (frame, y0, x0, th, tw) — the full-frame view is (frame, 0, 0, h, w); `sizes`: (h, w) per frame;
    `yuv_table`: the device array of cnl_yuv420_frame records tile_yuv420's launch read, None for packed frames.
    tile_uint8 is the constructor users need; from_records (below) builds a merge-only geometry for tests and tools."""

    def __init__(self, table, merge_table, first_view, views, frame_first_view, sizes, tile_h, tile_w, keep=(), yuv_table=None):
        self.table = table
        self.yuv_table = yuv_table
        self.merge_table = merge_table
        self.first_view = first_view
        self.views = views
        self.frame_first_view = frame_first_view
        self.sizes = sizes
        self.tile_h = tile_h
        self.tile_w = tile_w
        self._keep = keep          # the source frames: the table holds their addresses

    @property
    def num_frames(self):
        return len(self.frame_first_view) - 1

    def __len__(self):
        return len(self.views)

    def __repr__(self):
        return f"TileGeometry(frames={self.num_frames}, views={len(self.views)}, tile={self.tile_h}x{self.tile_w})"

    @classmethod
    def from_records(cls, records, frame_first_view, device):
        """Advanced / testing constructor: a geometry for merge_tiles ALONE, from merge records [(frame_w, frame_h, x0, y0, pad_left,
        pad_top, sx, sy)] and the list frame_first_view (N + 1 entries), for detections that did not come from tile_uint8.  There are no
        pixels behind it: `table` is None, `sizes` is empty and the `views` entries carry th = tw = 0.  One blocking upload."""
        V = len(records)
        ffv = [int(v) for v in frame_first_view]
        if len(ffv) < 1 or ffv[0] != 0 or ffv[-1] != V or any(b < a for a, b in zip(ffv, ffv[1:])):
            raise ValueError(f"frame_first_view must run from 0 to {V} without decreasing, got {ffv!r}")
        rec = np.zeros((V, 8), dtype=np.int32)
        if V:
            rec[:, :6] = [[int(x) for x in r[:6]] for r in records]
            rec[:, 6:] = np.array([[r[6], r[7]] for r in records], dtype=np.float32).view(np.int32)
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the tile merge runs on HIP devices only (no CPU fallback)")
        views = [(n, int(r[3]), int(r[2]), 0, 0) for n in range(len(ffv) - 1) for r in records[ffv[n]:ffv[n + 1]]]
        return cls._merge_only(rec, ffv, views, [], device, lambda parts, dev: [torch.from_numpy(p).to(dev) for p in parts])

    @classmethod
    def _merge_only(cls, rec, ffv, views, sizes, device, upload):
        """A geometry without pixels (`table` is None, tile_h = tile_w = 0) from the [V, 8] int32 merge records and the host lists; `upload`
        takes the two numpy tables to the device: blocking copies for from_records, _gather.upload_parts for scale_geometry."""
        with torch.cuda.device(device):
            merge_table, first_view = upload([rec, np.array(ffv, dtype=np.int32)], device)
        return cls(None, merge_table, first_view, views, ffv, sizes, 0, 0)


def _full_frame_record(h: int, w: int, new_h: int, new_w: int, pad_top: int, pad_left: int):
    """The merge record of a whole h x w frame letterboxed to new_h x new_w behind the pads: 8 int32 words, the last two the float bits."""
    sx, sy = np.float32(new_w) / np.float32(w), np.float32(new_h) / np.float32(h)         # as cnl_unletterbox_boxes_f32 forms them
    return (w, h, 0, 0, pad_left, pad_top, sx.view(np.int32), sy.view(np.int32))


def _view_records(sizes, tile_h: int, tile_w: int, overlap: float, full_frame: bool):
    """The views of frames of the given (h, w) sizes -> (windows [(frame, y0, x0, h, w, new_h, new_w, pad_top, pad_left)]: what the
    gather kernel needs per view, the merge records, TileGeometry.views, frame_first_view).  A tile is a 1:1 window at the canvas'
    top left; the full-frame view is the whole frame letterboxed."""
    windows, mg, views, ffv = [], [], [], [0]
    one = np.float32(1.0).view(np.int32)
    for n, (h, w) in enumerate(sizes):
        for (y0, x0, th, tw) in tile_grid(h, w, tile_h, tile_w, overlap):
            windows.append((n, y0, x0, th, tw, th, tw, 0, 0))
            mg.append((w, h, x0, y0, 0, 0, one, one))
            views.append((n, y0, x0, th, tw))
        if full_frame:
            nh, nw, pt, pl = letterbox_geometry(h, w, tile_h, tile_w)
            windows.append((n, 0, 0, h, w, nh, nw, pt, pl))
            mg.append(_full_frame_record(h, w, nh, nw, pt, pl))
            views.append((n, 0, 0, h, w))
        ffv.append(len(views))
    return windows, mg, views, ffv


def tile_frames(frames, tile_h: int = 512, tile_w: int = 512, overlap: float = 0.2, full_frame: bool = True, fill=(0, 0, 0),
                pixel_format: str = "rgb", matrix: str = "bt601", full_range: bool = False):
    """The one function behind tile_uint8 (pixel_format "rgb") and tile_yuv420 ("nv12" / "i420"), which detect_tiled calls with its
    pixel_format: frame source (rows read in place) -> views -> one gather."""
    src = _frames.open_frames(frames, pixel_format, "tile_uint8" if pixel_format == "rgb" else "tile_yuv420", matrix, full_range,
                              copy=_frames.ROWS)
    word = _frames.fill_word(fill, src.C)
    windows, mg, views, ffv = _view_records(src.sizes, tile_h, tile_w, overlap, full_frame)
    plain, planes = src.records(windows)
    dev = src.check_device()                     # (YUV frames: only now, after the fill and the tile grid)
    g = _gather.gather(dev, windows, plain, tile_h, tile_w, src.C, word, planes=planes, coef=src.coef, merge_records=mg,
                       frame_first_view=ffv)
    return g.canvas, TileGeometry(g.table, g.merge_table, g.first_view, views, ffv, src.sizes, tile_h, tile_w, keep=src.keep,
                                  yuv_table=g.yuv_table)


def tile_uint8(frames, tile_h: int = 512, tile_w: int = 512, overlap: float = 0.2, full_frame: bool = True, fill=(0, 0, 0)):
    """frames: a sequence of uint8 [h_i, w_i, C] tensors on one HIP device (C in 1..4, the same for all; rows may be strided), or one
    [N, h, w, C] tensor -> (views [V, tile_h, tile_w, C] uint8, TileGeometry).  The views of a frame are its tile_grid tiles, row-major
    (a frame smaller than a tile is padded with `fill` on the right / bottom), then with full_frame=True the whole frame letterboxed to
    the tile size.  One launch for all views of all frames; one pinned-memory upload (the tables); no device sync."""
    return tile_frames(frames, tile_h, tile_w, overlap, full_frame, fill)


def tile_yuv420(frames, tile_h: int = 512, tile_w: int = 512, overlap: float = 0.2, full_frame: bool = True, fill=(0, 0, 0),
                layout: str = "nv12", matrix: str = "bt601", full_range: bool = False):
    """tile_uint8 for YUV 4:2:0 frames -> (views [V, tile_h, tile_w, 3] uint8 RGB, TileGeometry): the tile_grid tiles of every frame
    (windows into its planes; an odd origin takes the chroma sample of its 2 x 2 block) and, with full_frame, the whole frame
    letterboxed, converted and gathered by one launch.  merge_tiles takes the geometry as it takes tile_uint8's."""
    return tile_frames(frames, tile_h, tile_w, overlap, full_frame, fill, _frames.yuv_layout(layout), matrix, full_range)


def _launch_merge(entry: str, bboxes, scores, labels, geom, max_detections: int, max_candidates: int, rule):
    """The part merge_tiles and merge_soft share, after their checks: the workspace <entry>_workspace_bytes asks for, the five outputs and
    the call of <entry>_f32, whose arguments differ only in `rule`, the values between max_candidates and the outputs."""
    bboxes, scores, labels = bboxes.contiguous(), scores.contiguous(), labels.contiguous()
    (V, k), N, dev = bboxes.shape[:2], geom.num_frames, bboxes.device
    lib = _lib.load()
    ws_bytes = int(getattr(lib, entry + "_workspace_bytes")(N, V, k, max_candidates))
    if ws_bytes == 0:
        _lib.check(_lib.CNL_E_BAD_ARG, entry + "_workspace_bytes")
    with torch.cuda.device(dev):
        ws = torch.empty((ws_bytes + 256,), device=dev, dtype=torch.uint8)
        ws_ptr = (ws.data_ptr() + 255) & ~255
        out_boxes = torch.empty((N, max_detections, 4), device=dev, dtype=torch.float32)
        out_scores = torch.empty((N, max_detections), device=dev, dtype=torch.float32)
        out_labels = torch.empty((N, max_detections), device=dev, dtype=torch.int64)
        out_source = torch.empty((N, max_detections), device=dev, dtype=torch.int32)
        out_count = torch.empty((N,), device=dev, dtype=torch.int32)
        _lib.check(getattr(lib, entry + "_f32")(bboxes.data_ptr(), scores.data_ptr(), labels.data_ptr(), geom.merge_table.data_ptr(),
                                                geom.first_view.data_ptr(), N, V, k, max_detections, max_candidates, *rule, out_boxes.data_ptr(),
                                                out_scores.data_ptr(), out_labels.data_ptr(), out_source.data_ptr(), out_count.data_ptr(),
                                                ws_ptr, ws_bytes, _lib.stream(dev)),
                   entry + "_f32")
    return {"bboxes": out_boxes, "scores": out_scores, "labels": out_labels, "source": out_source, "count": out_count}


def positive_int(who: str, name: str, v, most=None) -> None:
    """v must be an int (not a bool) of at least 1, and of at most `most` where there is a limit; otherwise ValueError."""
    if isinstance(v, bool) or not isinstance(v, int) or v < 1 or (most is not None and v > most):
        raise ValueError(f"{who}: {name} must be " + ("a positive int" if most is None else f"an int in 1..{most}") + f", got {v!r}")


def _check_detections(who: str, bboxes, scores, labels) -> Tuple[int, int]:
    """What the detections are, not where they live (that half is _gather.require_hip): float32 [V, k, 4] boxes, float32 [V, k] scores
    and int64 [V, k] labels, all tensors -> (V, k); otherwise ValueError."""
    for name, t in (("bboxes", bboxes), ("scores", scores), ("labels", labels)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{who}: {name} must be a tensor, got {type(t).__name__}")
    if bboxes.dtype != torch.float32 or bboxes.dim() != 3 or bboxes.shape[-1] != 4 or scores.dtype != torch.float32 or labels.dtype != torch.int64:
        raise ValueError(f"{who}: expected float32 [V,k,4] boxes, float32 [V,k] scores and int64 [V,k] labels, got {bboxes.dtype} "
                         f"{tuple(bboxes.shape)}, {scores.dtype} {tuple(scores.shape)}, {labels.dtype} {tuple(labels.shape)}")
    V, k = int(bboxes.shape[0]), int(bboxes.shape[1])
    if tuple(scores.shape) != (V, k) or tuple(labels.shape) != (V, k):
        raise ValueError(f"{who}: scores {tuple(scores.shape)} and labels {tuple(labels.shape)} must both be [{V}, {k}]")
    return V, k


def merge_tiles(bboxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, geom: TileGeometry, max_detections: int = 300,
                score_threshold: float = 0.1, match_threshold: float = 0.5, match_metric: str = "iou", class_aware: bool = True,
                max_candidates: int = 4096):
    """The decoded detections of all views ([V, k, 4] boxes in view pixels, [V, k] scores, [V, k] int64 labels: gather_* with
    normalize_bbox=False) -> per frame, in the frame's own pixels and with the duplicates removed:
    {"bboxes" [N, max_detections, 4], "scores", "labels" (int64), "source" (int32: the candidate number v * k + r relative to the frame's
    first view, -1 past the count), "count" [N] int32}.  Three launches for the whole batch, no device sync."""
    _gather.require_hip((bboxes, scores, labels), "merge_tiles")
    if match_metric not in METRICS:
        raise ValueError(f"merge_tiles: match_metric must be one of {sorted(METRICS)}, got {match_metric!r}")
    V, _ = _check_detections("merge_tiles", bboxes, scores, labels)
    if V != len(geom) or bboxes.device != geom.merge_table.device:
        raise ValueError(f"merge_tiles: detections of {V} views on {bboxes.device} against a geometry of {len(geom)} views on {geom.merge_table.device}")
    positive_int("merge_tiles", "max_detections", max_detections)
    positive_int("merge_tiles", "max_candidates", max_candidates)
    return _launch_merge("cnl_merge_tiles", bboxes, scores, labels, geom, max_detections, max_candidates,
                         (float(score_threshold), float(match_threshold), METRICS[match_metric], int(bool(class_aware))))


SOFT_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}
SOFT_MAX_CANDIDATES = 4096


def _number(name: str, v, who: str) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
        raise ValueError(f"{who}: {name} must be a number that is not NaN, got {v!r}")
    return float(v)


def check_soft_arguments(who: str, method, sigma, iou_threshold, score_threshold, max_detections, max_candidates) -> None:
    """The value checks merge_soft and detect_multiscale share (the latter makes them before its first launch)."""
    if method not in SOFT_METHODS:
        raise ValueError(f"{who}: method must be one of {sorted(SOFT_METHODS)}, got {method!r}")
    sigma = _number("sigma", sigma, who)
    if not 0.0 < sigma < float("inf"):
        raise ValueError(f"{who}: sigma must be positive and finite, got {sigma!r}")
    _number("iou_threshold", iou_threshold, who)
    _number("score_threshold", score_threshold, who)
    positive_int(who, "max_detections", max_detections)
    positive_int(who, "max_candidates", max_candidates, SOFT_MAX_CANDIDATES)


def merge_soft(bboxes: torch.Tensor, scores: torch.Tensor, labels: torch.Tensor, geom: TileGeometry, method: str = "gaussian",
               sigma: float = 0.5, iou_threshold: float = 0.5, score_threshold: float = 0.001, max_detections: int = 100,
               class_aware: bool = True, max_candidates: int = 4096):
    """merge_tiles with soft-NMS as the rule (cnl_merge_soft_f32; the rule: include/centernet_gfx950.h): a kept box multiplies the
    working scores of its same-label neighbours by exp(-iou^2 / sigma) ("gaussian"), by 1 - iou where iou > iou_threshold ("linear"),
    or by 0 where merge_tiles' IoU predicate holds ("hard": merge_tiles itself); the next pick is the best remaining score above
    score_threshold.  Same inputs and the same dict as merge_tiles; "scores" are the decayed scores, in non-increasing order.
    Works on any TileGeometry: one view per frame is the soft-NMS of a single pass, one view per (frame, scale) the multi-scale merge
    of detect_multiscale.  max_candidates is at most 4096.  Two launches for the whole batch, no device sync.
    Checks, all before any launch: the values and the tensors' dtypes and shapes (ValueError), then where the tensors live."""
    check_soft_arguments("merge_soft", method, sigma, iou_threshold, score_threshold, max_detections, max_candidates)
    V, _ = _check_detections("merge_soft", bboxes, scores, labels)
    _gather.require_hip((bboxes, scores, labels), "merge_soft")
    if not isinstance(geom, TileGeometry) or V != len(geom) or bboxes.device != geom.merge_table.device:
        raise ValueError(f"merge_soft: detections of {V} views on {bboxes.device} against {geom!r}")
    return _launch_merge("cnl_merge_soft", bboxes, scores, labels, geom, max_detections, max_candidates,
                         (float(score_threshold), SOFT_METHODS[method], float(sigma), float(iou_threshold), int(bool(class_aware))))


def scale_geometry(per_scale, dev) -> TileGeometry:
    """The merge geometry of a multi-scale pass: per_scale[s] is the host list LetterboxGeometry.frames of scale s, [(h, w, new_h,
    new_w, pad_top, pad_left)] for the same N frames -> one full-frame view per (frame, scale), frame-major (view n * S + s), each
    record what _view_records writes for its full-frame view.  Host arithmetic on shapes and one pinned upload: no device sync."""
    S, N = len(per_scale), len(per_scale[0])
    frames = [per_scale[s][n] for n in range(N) for s in range(S)]
    rec = np.array([_full_frame_record(*f) for f in frames], dtype=np.int32).reshape(N * S, 8)
    views = [(i // S, 0, 0, f[0], f[1]) for i, f in enumerate(frames)]
    return TileGeometry._merge_only(rec, [n * S for n in range(N + 1)], views, [per_scale[0][n][:2] for n in range(N)], dev, _gather.upload_parts)


def pick_embeddings(embeddings: torch.Tensor, source: torch.Tensor, first_view: torch.Tensor) -> torch.Tensor:
    """The embeddings [V, k, E] of all views, picked by a merge's `source` [N, K] (candidate numbers relative to the frame's first
    view; -1 past the count gives a zero row) -> [N, K, E].  What detect_tiled and detect_multiscale return for tracking models."""
    k, E, N = embeddings.shape[1], embeddings.shape[2], source.shape[0]
    src = source.long()
    index = (src.clamp_min(0) + first_view[:N].long()[:, None] * k).reshape(-1, 1).expand(-1, E)
    picked = torch.gather(embeddings.reshape(-1, E), 0, index).view(N, -1, E)
    return picked.masked_fill((src < 0).unsqueeze(-1), 0.0)          # (not a product: -x * 0 is -0)
