"""The validation-loss rule of include/centernet_gfx950.h (cnl_detection_loss_f64) restated in numpy float64, with the same fp32 roundings at
the same places.  Plain helper for tests/test_loss_host.py, tests/test_gpu_loss.py and tools/: imports nothing from the reference.

    boxes [M, 4] x y w h in input pixels (float64), labels [M]  ->  records  ->  target map (fp32) / samples  ->  rows and totals

Sums are numpy's (pairwise) sums: the device's fixed order differs from them in the last bits only (terms are non-negative)."""
import math

import numpy as np

TARGET_METHODS = {"cornernet": 0, "ttfnet": 1, "fixed": 2}
TARGET_DEFAULTS = {"cornernet": 0.3, "ttfnet": 0.54, "fixed": 1.0}
HEATMAP_LOSSES = ("cornernet_focal", "quality")
BOX_LOSSES = ("l1", "smooth_l1", "iou", "giou", "diou", "ciou")
F32_EPS = np.float32(np.finfo(np.float32).eps)


def cornernet_radius(w, h, mo):
    b1 = h + w
    c1 = w * h * (1 - mo) / (1 + mo)
    r1 = (b1 - math.sqrt(b1 * b1 - 4 * c1)) / 2
    b2 = 2 * (h + w)
    c2 = (1 - mo) * w * h
    r2 = (b2 - math.sqrt(b2 * b2 - 16 * c2)) / 8
    a3 = 4 * mo
    b3 = -2 * mo * (h + w)
    c3 = (mo - 1) * w * h
    r3 = (b3 + math.sqrt(b3 * b3 - 4 * a3 * c3)) / (2 * a3)
    return min(r1, r2, r3)


def records(boxes, labels, C, H, W, stride=4, method="cornernet", param=None):
    """-> list of dicts, one per box: state 0 (skipped) or 1, cx, cy, rx, ry (int), den_x, den_y (float32), label."""
    param = TARGET_DEFAULTS[method] if param is None else float(param)
    out = []
    for box, label in zip(np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray(labels).reshape(-1)):
        rec = {"state": 0, "label": int(label)}
        out.append(rec)
        x, y, w, h = (float(v) / float(stride) for v in box)
        if not all(math.isfinite(v) for v in (x, y, w, h)) or w < 0 or h < 0 or not 0 <= int(label) < C:
            continue
        cx, cy = float(np.rint(x + w / 2)), float(np.rint(y + h / 2))
        try:
            if method == "cornernet":
                rx = ry = cornernet_radius(w, h, param)
            elif method == "ttfnet":
                rx, ry = w / 2 * param, h / 2 * param
            else:
                rx = ry = param
        except (ValueError, OverflowError):
            continue
        if not (math.isfinite(rx) and math.isfinite(ry)) or not (0 <= cx <= W and 0 <= cy <= H):
            continue
        rx, ry = max(0.0, float(np.rint(rx))), max(0.0, float(np.rint(ry)))
        sx, sy = rx / 3 + 1 / 6, ry / 3 + 1 / 6
        with np.errstate(over="ignore"):
            rec.update(state=1, cx=int(cx), cy=int(cy), rx=int(min(rx, 2.0 ** 24)), ry=int(min(ry, 2.0 ** 24)),
                       den_x=np.float32(2 * (sx * sx)), den_y=np.float32(2 * (sy * sy)))
    return out


def window(rec, H, W):
    """The rendered window of a record: (y0, y1, x0, x1), exclusive ends (possibly empty); None for a skipped box.  A centre ON cx == W or cy == H
    keeps the part of its window inside the map, as the reference's slices do (centernet.py:187-199)."""
    if not rec["state"]:
        return None
    return (max(rec["cy"] - rec["ry"], 0), min(rec["cy"] + rec["ry"] + 1, H), max(rec["cx"] - rec["rx"], 0), min(rec["cx"] + rec["rx"] + 1, W))


def gaussian(rec, y0, y1, x0, x1):
    """The record's target values on the window, float32."""
    dx = (np.arange(x0, x1, dtype=np.int64) - rec["cx"]).reshape(1, -1)
    dy = (np.arange(y0, y1, dtype=np.int64) - rec["cy"]).reshape(-1, 1)
    with np.errstate(under="ignore"):
        g = (dx * dx).astype(np.float32) / rec["den_x"] + (dy * dy).astype(np.float32) / rec["den_y"]      # fp32 quotients, fp32 sum
        assert g.dtype == np.float32
        t = np.exp(-g.astype(np.float64)).astype(np.float32)
    t[t < F32_EPS] = 0
    return t


def render(recs, C, H, W):
    """-> the target heatmap [C, H, W] float32 of one image."""
    out = np.zeros((C, H, W), np.float32)
    for rec in recs:
        win = window(rec, H, W)
        if win is None:
            continue
        y0, y1, x0, x1 = win
        view = out[rec["label"], y0:y1, x0:x1]
        np.maximum(view, gaussian(rec, y0, y1, x0, x1), out=view)
    return out


def _power(v, e):
    if e == 2:
        return v * v
    if e == 4:
        return (v * v) * (v * v)
    return np.power(v, e)


def heatmap_terms(logits, target, loss="cornernet_focal", alpha=2.0, beta=None):
    """Per-element loss terms, float64, of fp32 logits and fp32 targets of one shape."""
    x, t = np.asarray(logits, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    beta = (4.0 if loss == "cornernet_focal" else 2.0) if beta is None else beta
    with np.errstate(over="ignore", under="ignore"):
        p = 1 / (1 + np.exp(-x))
        l1p = np.log1p(np.exp(-np.abs(x)))
        if loss == "cornernet_focal":
            pos = -_power(1 - p, alpha) * (np.minimum(x, 0) - l1p) * (t == 1)
            neg = -_power(p, alpha) * (np.minimum(-x, 0) - l1p) * _power(1 - t, beta)
            return pos + neg
        return _power(np.abs(t - p), beta) * (np.maximum(x, 0) - x * t + l1p)


def samples(rec, H, W):
    """The (x, y) sample points of a counted record, x outer (itertools.product)."""
    if not rec["state"]:
        return []
    xs = [v for v in (rec["cx"] - 1, rec["cx"], rec["cx"] + 1) if 0 <= v <= W - 1]
    ys = [v for v in (rec["cy"] - 1, rec["cy"], rec["cy"] + 1) if 0 <= v <= H - 1]
    return [(x, y) for x in xs for y in ys]


def decode_box(box, x, y, stride=4, box_log=False, box_multiplier=1.0):
    """The decode's fp32 rule at pixel (x, y) of box [4, H, W]: -> x1 y1 x2 y2 float32."""
    f = np.float32
    v = np.asarray(box, np.float32)[:, y, x]
    if box_log:
        v = np.exp(v)
    g = np.maximum(v * f(box_multiplier), f(0))
    cx, cy = f(x) + f(0.5), f(y) + f(0.5)
    return np.array([(cx - g[0]) * f(stride), (cy - g[1]) * f(stride), (cx + g[2]) * f(stride), (cy + g[3]) * f(stride)], np.float32)


def box_target(box):
    x, y, w, h = (float(v) for v in box)
    return np.array([x, y, x + w, y + h], np.float64).astype(np.float32)


def box_term(kind, pred, target):
    """losses/box_losses.py on one (pred, target) pair of fp32 boxes, float64."""
    p, t = [float(v) for v in pred], [float(v) for v in target]
    if kind in ("l1", "smooth_l1"):
        s = 0.0
        for a, b in zip(p, t):
            d = abs(a - b)
            s += d if kind == "l1" else (0.5 * d * d if d < 1 else d - 0.5)
        return s
    eps = 1e-8
    with np.errstate(all="ignore"):
        p, t = [np.float64(v) for v in p], [np.float64(v) for v in t]
        area1, area2 = (p[2] - p[0]) * (p[3] - p[1]), (t[2] - t[0]) * (t[3] - t[1])
        inter = max(min(p[2], t[2]) - max(p[0], t[0]), 0.0) * max(min(p[3], t[3]) - max(p[1], t[1]), 0.0)
        union = area1 + area2 - inter
        iou = inter / (union + eps)
        if kind == "iou":
            return float(1 - iou)
        ex1, ey1, ex2, ey2 = min(p[0], t[0]), min(p[1], t[1]), max(p[2], t[2]), max(p[3], t[3])
        if kind == "giou":
            return float(1 - (iou - (1 - union / ((ex2 - ex1) * (ey2 - ey1)))))
        ew, eh = ex2 - ex1, ey2 - ey1
        dx, dy = (t[0] + t[2]) / 2 - (p[0] + p[2]) / 2, (t[1] + t[3]) / 2 - (p[1] + p[3]) / 2
        penalty = (dx * dx + dy * dy) / (ew * ew + eh * eh)
        if kind == "diou":
            return float(1 - iou + penalty)
        assert kind == "ciou", kind
        angle = (np.arctan((p[2] - p[0]) / (p[3] - p[1] + eps)) - np.arctan((t[2] - t[0]) / (t[3] - t[1] + eps))) * 2 / math.pi
        v = angle * angle
        return float(1 - iou + penalty + v / (1 - iou + v + eps) * v)


def detection_loss(heatmap, box_2d, targets, stride=4, heatmap_target="cornernet", heatmap_target_params=None, heatmap_loss="cornernet_focal",
                   box_loss="giou", heatmap_loss_weight=1.0, box_loss_weight=1.0, box_log=False, box_multiplier=1.0, alpha=2.0, beta=None):
    """heatmap [N, C, H, W] fp32 logits, box_2d [N, 4, H, W] fp32, targets [(boxes [M, 4] f64, labels [M])] ->
    {"heatmap", "box_2d", "total" (float), "per_image" [N, 4] f64, "skipped" int, "targets" [N, C, H, W] f32, "records", "samples"}."""
    heatmap, box_2d = np.asarray(heatmap, np.float32), np.asarray(box_2d, np.float32)
    N, C, H, W = heatmap.shape
    param = None
    if heatmap_target_params:
        (param,) = heatmap_target_params.values()
    rows, maps, all_recs, all_samples, skipped = np.zeros((N, 4)), np.zeros((N, C, H, W), np.float32), [], [], 0
    for n, (boxes, labels) in enumerate(targets):
        recs = records(boxes, labels, C, H, W, stride, heatmap_target, param)
        maps[n] = render(recs, C, H, W)
        terms, idx = [], []
        for rec, box in zip(recs, np.asarray(boxes, np.float64).reshape(-1, 4)):
            skipped += not rec["state"]
            for (x, y) in samples(rec, H, W):
                idx.append(y * W + x)
                terms.append(box_term(box_loss, decode_box(box_2d[n], x, y, stride, box_log, box_multiplier), box_target(box)))
        rows[n] = (heatmap_terms(heatmap[n], maps[n], heatmap_loss, alpha, beta).sum(), float(np.sum(np.array(terms, np.float64))), sum(r["state"] for r in recs), len(terms))
        all_recs.append(recs)
        all_samples.append(idx)
    heat = rows[:, 0].sum() / max(1.0, rows[:, 2].sum())
    box = rows[:, 1].sum() / max(1.0, rows[:, 3].sum())
    return {"heatmap": heat, "box_2d": box, "total": heat * heatmap_loss_weight + box * box_loss_weight, "per_image": rows, "skipped": int(skipped),
            "targets": maps, "records": all_recs, "samples": all_samples}
