"""TEST INFRASTRUCTURE — the COCO box evaluation rule (COCOeval, iouType "bbox", on the records the reference's CocoEvaluator builds: no
crowds, no per-annotation ignore, area = w * h) restated in numpy / plain Python from its statement in include/centernet_gfx950.h.
pycocotools is not available here; hand-derived cases in tests/test_coco_eval_host.py pin this restatement itself.

Everything is float64 (Python floats and numpy float64: one rounding per operation, nothing fused), so the kernels of
csrc/coco_eval.hip are compared with it for equality of bits.  The matching is the SEQUENTIAL walk of the statement (ground truths
ordered not-ignored first, `best` rising as the walk goes), not the wave form the kernel uses.
"""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
METRIC_NAMES = ("mAP", "AP50", "AP75", "AP_small", "AP_medium", "AP_large", "AR1", "AR10", "mAR", "AR_small", "AR_medium", "AR_large")
T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RANGES), len(MAX_DETS)


def iou_xywh(D, G):
    """IoU of two boxes given as float64 (x, y, w, h)."""
    w = min(D[0] + D[2], G[0] + G[2]) - max(D[0], G[0])
    if w <= 0:
        return 0.0
    h = min(D[1] + D[3], G[1] + G[3]) - max(D[1], G[1])
    if h <= 0:
        return 0.0
    i = w * h
    u = D[2] * D[3] + G[2] * G[3] - i
    return i / u


def detections_xywh(boxes_xyxy):
    """fp32 x1 y1 x2 y2 -> float64 x y w h with w and h formed in fp32 first (the reference's box_convert), as a list of float tuples."""
    b = np.asarray(boxes_xyxy, dtype=np.float32).reshape(-1, 4)
    w, h = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
    assert w.dtype == np.float32
    return [(float(b[i, 0]), float(b[i, 1]), float(w[i]), float(h[i])) for i in range(len(b))]


def out_of_range(area, a):
    lo, hi = AREA_RANGES[a]
    return area < lo or area > hi


def match_image(boxes_xyxy, scores, labels, gt_xywh, gt_labels, num_classes, trace=None):
    """One image -> (rank [n] int32: the class rank, -1 for a dropped detection (label outside 0..K-1 or rank >= 100);
    matched [n], ignored [n] int64: bit a * 10 + t; npig [K, 4] int64: this image's not ignored ground truths).
    trace: a dict that receives {(a, t, detection): ground truth} for every match made."""
    D = detections_xywh(boxes_xyxy)
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    labels = np.asarray(labels, dtype=np.int64).reshape(-1)
    G = [tuple(float(v) for v in g) for g in np.asarray(gt_xywh, dtype=np.float64).reshape(-1, 4)]
    gt_labels = np.asarray(gt_labels, dtype=np.int64).reshape(-1)
    n = len(D)
    rank, matched, ignored = np.full(n, -1, dtype=np.int32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    npig = np.zeros((num_classes, A), dtype=np.int64)
    d_area = [d[2] * d[3] for d in D]
    g_area = [g[2] * g[3] for g in G]
    for c in sorted(set(labels.tolist()) | set(gt_labels.tolist())):
        if not 0 <= c < num_classes:
            continue
        mine = np.flatnonzero(labels == c)
        dets = mine[np.argsort(-scores[mine], kind="stable")][:MAX_DETS[-1]].tolist()
        rank[dets] = np.arange(len(dets))
        gts = np.flatnonzero(gt_labels == c).tolist()
        iou = {(d, g): iou_xywh(D[d], G[g]) for d in dets for g in gts}
        for a in range(A):
            g_ign = {g: out_of_range(g_area[g], a) for g in gts}
            npig[c, a] += sum(1 for g in gts if not g_ign[g])
            walk = [g for g in gts if not g_ign[g]] + [g for g in gts if g_ign[g]]          # not ignored first, stably
            for t in range(T):
                bit = 1 << (a * T + t)
                taken = set()
                for d in dets:
                    best, m = min(float(IOU_THRS[t]), 1 - 1e-10), None
                    for g in walk:
                        if g in taken:
                            continue
                        if m is not None and not g_ign[m] and g_ign[g]:
                            break
                        if iou[d, g] < best:
                            continue
                        best, m = iou[d, g], g
                    if m is not None:
                        taken.add(m)
                        if trace is not None:
                            trace[a, t, d] = m
                        matched[d] |= bit
                        if g_ign[m]:
                            ignored[d] |= bit
                    elif out_of_range(d_area[d], a):
                        ignored[d] |= bit
    return rank, matched, ignored, npig


def match_images(dets, gts, num_classes):
    """dets: per image (boxes_xyxy [n, 4], scores [n], labels [n]); gts: per image (boxes xywh [g, 4], labels [g]) ->
    (records: per image (scores f32, labels i64, rank, matched, ignored), npig [K, 4])."""
    assert len(dets) == len(gts)
    records, npig = [], np.zeros((num_classes, A), dtype=np.int64)
    for (b, s, l), (gb, gl) in zip(dets, gts):
        rank, matched, ignored, inc = match_image(b, s, l, gb, gl, num_classes)
        records.append((np.asarray(s, dtype=np.float32).reshape(-1), np.asarray(l, dtype=np.int64).reshape(-1), rank, matched, ignored))
        npig += inc
    return records, npig


def accumulate(records, npig, num_classes):
    """-> (precision [T, R, K, A, M], recall [T, K, A, M]) float64; -1 where a category has no ground truth in a range."""
    precision = -np.ones((T, R, num_classes, A, M))
    recall = -np.ones((T, num_classes, A, M))
    eps = np.spacing(1)
    for c in range(num_classes):
        # the category's detections in order of arrival: image by image, inside an image by class rank
        parts = []
        for (s, l, rank, matched, ignored) in records:
            idx = np.flatnonzero((l == c) & (rank >= 0))
            idx = idx[np.argsort(rank[idx], kind="stable")]
            parts.append((s[idx], rank[idx], matched[idx], ignored[idx]))
        s, rank, matched, ignored = (np.concatenate([p[i] for p in parts]) if parts else np.zeros(0, dt)
                                     for i, dt in enumerate((np.float32, np.int32, np.int64, np.int64)))
        for a in range(A):
            if npig[c, a] == 0:
                continue
            for mi, max_det in enumerate(MAX_DETS):
                keep = np.flatnonzero(rank < max_det)
                keep = keep[np.argsort(-s[keep], kind="stable")]
                nd = len(keep)
                for t in range(T):
                    bit = a * T + t
                    dm = ((matched[keep] >> bit) & 1).astype(bool)
                    dig = ((ignored[keep] >> bit) & 1).astype(bool)
                    tp = np.cumsum(dm & ~dig, dtype=np.float64)
                    fp = np.cumsum(~dm & ~dig, dtype=np.float64)
                    rc = tp / npig[c, a]
                    pr = tp / (fp + tp + eps)
                    recall[t, c, a, mi] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds = np.searchsorted(rc, REC_THRS, side="left")
                    q = np.zeros(R)
                    for ri, pi in enumerate(inds):
                        if pi < nd:
                            q[ri] = pr[pi]
                    precision[t, :, c, a, mi] = q
    return precision, recall


def summarize(precision, recall):
    def mean(x):
        x = x[x > -1]
        return float(np.mean(x)) if x.size else -1.0

    def ap(t=None, a=0):
        s = precision[:, :, :, a, M - 1]
        return mean(s if t is None else s[t])

    def ar(a=0, m=M - 1):
        return mean(recall[:, :, a, m])
    t50, t75 = int(np.flatnonzero(IOU_THRS == .5)[0]), int(np.flatnonzero(IOU_THRS == .75)[0])
    values = (ap(), ap(t50), ap(t75), ap(a=1), ap(a=2), ap(a=3), ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2), ar(a=3))
    return dict(zip(METRIC_NAMES, values))


def evaluate(dets, gts, num_classes):
    """The whole evaluation -> {"records", "npig", "precision", "recall", "metrics"}."""
    records, npig = match_images(dets, gts, num_classes)
    precision, recall = accumulate(records, npig, num_classes)
    return {"records": records, "npig": npig, "precision": precision, "recall": recall, "metrics": summarize(precision, recall)}


def xywh_to_xyxy32(boxes_xywh):
    """x y w h -> fp32 x1 y1 x2 y2 (exact on grids where x + w is exact in fp32)."""
    b = np.asarray(boxes_xywh, dtype=np.float32).reshape(-1, 4)
    return np.concatenate([b[:, :2], b[:, :2] + b[:, 2:]], axis=1)
