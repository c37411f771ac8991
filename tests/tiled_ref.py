"""Test-only yardstick for sliced inference (numpy, float32 / int only): the tile grid, the way back into the frame and the merge rule
of include/centernet_gfx950.h (cnl_merge_tiles_f32), restated literally — one numpy float32 operation per operation of the rule, so
that the GPU's result can be compared bit for bit.  The pixel oracle of the full-frame view is tests/letterbox_ref.py."""
import math

import numpy as np

F = np.float32


def axis_ref(size, tile, overlap):
    """[(start, length)] along one axis: ov = round(tile * overlap), step = tile - ov; one short tile when size <= tile, otherwise
    ceil((size - tile) / step) + 1 tiles, the last shifted back inside."""
    if size <= tile:
        return [(0, size)]
    ov = round(tile * overlap)
    step = tile - ov
    n = math.ceil((size - tile) / step) + 1
    return [(min(i * step, size - tile), tile) for i in range(n)]


def tile_grid_ref(h, w, tile_h=512, tile_w=512, overlap=0.2):
    return [(y0, x0, th, tw) for (y0, th) in axis_ref(h, tile_h, overlap) for (x0, tw) in axis_ref(w, tile_w, overlap)]


def view_records(sizes, tile_h, tile_w, overlap, full_frame, geometry):
    """-> (records [(frame_w, frame_h, x0, y0, pad_left, pad_top, sx, sy)], frame_first_view, views [(frame, y0, x0, th, tw)]) of frames of
    the given (h, w) sizes; `geometry` is letterbox_ref.geometry."""
    rec, ffv, views = [], [0], []
    for n, (h, w) in enumerate(sizes):
        for (y0, x0, th, tw) in tile_grid_ref(h, w, tile_h, tile_w, overlap):
            rec.append((w, h, x0, y0, 0, 0, F(1), F(1)))
            views.append((n, y0, x0, th, tw))
        if full_frame:
            nh, nw, pt, pl = geometry(h, w, tile_h, tile_w)
            rec.append((w, h, 0, 0, pl, pt, F(nw) / F(w), F(nh) / F(h)))
            views.append((n, 0, 0, h, w))
        ffv.append(len(rec))
    return rec, ffv, views


def crop_view(frame, y0, x0, th, tw, tile_h, tile_w, fill):
    """The tile the gather must produce: the frame's window at the top left of a tile_h x tile_w canvas of `fill`."""
    C = frame.shape[2]
    out = np.empty((tile_h, tile_w, C), dtype=np.uint8)
    out[...] = np.asarray(fill[:C], dtype=np.uint8)
    out[:th, :tw] = frame[y0:y0 + th, x0:x0 + tw]
    return out


def map_boxes_ref(boxes, record):
    """[..., 4] x1 y1 x2 y2 in view pixels -> the frame's pixels: (x - pad_left) / sx + x0, clamped to [0, frame_w]; y alike.  The clamp
    is fminf(fmaxf(v, 0), limit), which returns the other operand for a NaN: a NaN coordinate maps to 0."""
    fw, fh, x0, y0, pl, pt, sx, sy = record
    b = np.asarray(boxes, dtype=F)
    out = np.empty_like(b)
    for c, (pad, s, o, lim) in enumerate(((pl, sx, x0, fw), (pt, sy, y0, fh), (pl, sx, x0, fw), (pt, sy, y0, fh))):
        v = (b[..., c] - F(pad)) / F(s)
        v = v + F(o)
        out[..., c] = np.fmin(np.fmax(v, F(0)), F(lim))        # C's fmaxf / fminf: a NaN coordinate becomes 0
    return out


def match_ref(box, others, threshold, metric):
    """Does `box` match each of `others` [m, 4]?  inter > threshold * denom, all in float32."""
    iw = np.maximum(np.minimum(box[2], others[:, 2]) - np.maximum(box[0], others[:, 0]), F(0))
    ih = np.maximum(np.minimum(box[3], others[:, 3]) - np.maximum(box[1], others[:, 1]), F(0))
    inter = iw * ih
    area = (box[2] - box[0]) * (box[3] - box[1])
    areas = (others[:, 2] - others[:, 0]) * (others[:, 3] - others[:, 1])
    denom = np.minimum(area, areas) if metric == 1 else (area + areas) - inter
    return inter > F(threshold) * denom


def merge_ref(boxes, scores, labels, records, frame_first_view, K_out, max_candidates=4096, score_threshold=0.1, match_threshold=0.5,
              metric=0, class_aware=True):
    """Rules 1-6.  boxes [V, k, 4] float32, scores [V, k] float32, labels [V, k] int64 -> {"bboxes" [N, K_out, 4], "scores", "labels",
    "source" int32, "count" int32}."""
    boxes, scores, labels = np.asarray(boxes, dtype=F), np.asarray(scores, dtype=F), np.asarray(labels, dtype=np.int64)
    N, k = len(frame_first_view) - 1, boxes.shape[1]
    out = {"bboxes": np.zeros((N, K_out, 4), F), "scores": np.zeros((N, K_out), F), "labels": np.zeros((N, K_out), np.int64),
           "source": np.full((N, K_out), -1, np.int32), "count": np.zeros((N,), np.int32)}
    for n in range(N):
        v0, v1 = frame_first_view[n], frame_first_view[n + 1]
        if v1 == v0:
            continue
        s = scores[v0:v1].reshape(-1)
        lab = labels[v0:v1].reshape(-1)
        mapped = np.concatenate([map_boxes_ref(boxes[v], records[v]) for v in range(v0, v1)], axis=0)       # rule 2
        c = np.nonzero(s > F(score_threshold))[0]                                                              # rule 1
        c = c[np.lexsort((c, -s[c]))][:max_candidates]                                                         # rules 3, 4
        kept = []
        kb, kl = np.zeros((K_out, 4), F), np.zeros((K_out,), np.int64)
        for i in c:                                                                                            # rule 5
            m = len(kept)
            if m:
                hit = match_ref(mapped[i], kb[:m], match_threshold, metric)
                if class_aware:
                    hit &= kl[:m] == lab[i]
                if hit.any():
                    continue
            kb[m], kl[m] = mapped[i], lab[i]
            kept.append(i)
            if len(kept) == K_out:                                                                             # rule 6
                break
        m = len(kept)
        out["bboxes"][n, :m], out["scores"][n, :m], out["labels"][n, :m] = mapped[kept], s[kept], lab[kept]
        out["source"][n, :m], out["count"][n] = kept, m
    return out
