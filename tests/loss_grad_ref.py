"""The gradient rule of include/centernet_gfx950.h (cnl_detection_loss_grad_f32) restated in numpy float64, analytic, on tests/loss_ref.py's records,
samples, decode_box and box_target.  Plain helper for tests/test_loss_grad_host.py, tests/test_gpu_loss_grad.py and tools/: imports nothing from the
reference.

    d(s_heat heatmap_loss + s_box box_2d_loss) / d(logits, box_2d),   the target map and the [t == 1] weight constants

Operations are written in the order csrc/det_loss.hip writes them (heat_dterm, box_dterm), so the two differ only where exp / log1p / atan / pow do.
A pixel's box contributions are added in slot order.  Non-differentiable points follow torch's autograd (see the header)."""
import math

import numpy as np

import loss_ref


def heatmap_dterms(logits, target, loss="cornernet_focal", alpha=2.0, beta=None):
    """d(loss_ref.heatmap_terms) / d(logits), float64, of fp32 logits and fp32 targets of one shape."""
    x, t = np.asarray(logits, np.float32).astype(np.float64), np.asarray(target, np.float32).astype(np.float64)
    beta = (4.0 if loss == "cornernet_focal" else 2.0) if beta is None else beta
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        e = np.exp(-np.abs(x))
        l1p = np.log1p(e)
        inv = 1 / (1 + e)
        p = np.where(x >= 0, inv, e * inv)
        q = 1 - p
        pq = p * q
        if loss == "cornernet_focal":
            ls, lsn = np.minimum(x, 0) - l1p, np.minimum(-x, 0) - l1p
            dq = 2 * q if alpha == 2 else alpha * np.power(q, alpha - 1)
            dp = 2 * p if alpha == 2 else alpha * np.power(p, alpha - 1)
            pos = np.where(t == 1, dq * pq * ls - loss_ref._power(q, alpha) * q, 0.0)
            neg = (loss_ref._power(p, alpha) * p - dp * pq * lsn) * loss_ref._power(1 - t, beta)
            return pos + neg
        d = t - p
        ad = np.abs(d)
        sg = np.sign(d)
        ce = np.maximum(x, 0) - x * t + l1p
        dm = 2 * ad if beta == 2 else beta * np.power(ad, beta - 1)
        return np.where(d == 0, 0.0, loss_ref._power(ad, beta) * (p - t) - sg * (dm * pq) * ce)


def _d_max(a, b):
    return 1.0 if a > b else (0.5 if a == b else 0.0)


def _d_min(a, b):
    return 1.0 if a < b else (0.5 if a == b else 0.0)


def box_dterm(kind, pred, target):
    """d(loss_ref.box_term) / d(pred): four float64 values of one (pred, target) pair of fp32 boxes."""
    p, t = [np.float64(v) for v in pred], [np.float64(v) for v in target]
    if kind in ("l1", "smooth_l1"):
        g = []
        for a, b in zip(p, t):
            d = a - b
            sg = 1.0 if d > 0 else (-1.0 if d < 0 else 0.0)
            g.append(sg if kind == "l1" else (float(d) if abs(d) < 1 else sg))
        return np.array(g, np.float64)
    eps = 1e-8
    with np.errstate(all="ignore"):
        w1, h1 = p[2] - p[0], p[3] - p[1]
        area1, area2 = w1 * h1, (t[2] - t[0]) * (t[3] - t[1])
        iwr, ihr = min(p[2], t[2]) - max(p[0], t[0]), min(p[3], t[3]) - max(p[1], t[1])
        iw, ih = max(iwr, 0.0), max(ihr, 0.0)
        inter = iw * ih
        uni = area1 + area2 - inter
        U = uni + eps
        iou = inter / U
        g_iou, g_uni, g_ew, g_eh, g_ddx, g_ddy, g_w1, g_h1 = -1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0
        if kind != "iou":
            ew, eh = max(p[2], t[2]) - min(p[0], t[0]), max(p[3], t[3]) - min(p[1], t[1])
            if kind == "giou":
                enclosing = ew * eh
                g_enc = uni / (enclosing * enclosing)
                g_uni = -1.0 / enclosing
                g_ew, g_eh = g_enc * eh, g_enc * ew
            else:
                assert kind in ("diou", "ciou"), kind
                diagonal = ew * ew + eh * eh
                ddx, ddy = (t[0] + t[2]) / 2 - (p[0] + p[2]) / 2, (t[1] + t[3]) / 2 - (p[1] + p[3]) / 2
                g_diag = -(ddx * ddx + ddy * ddy) / (diagonal * diagonal)
                g_ew, g_eh = g_diag * (2 * ew), g_diag * (2 * eh)
                g_ddx, g_ddy = 2 * ddx / diagonal, 2 * ddy / diagonal
                if kind == "ciou":
                    w2, h2 = t[2] - t[0], t[3] - t[1]
                    hq = h1 + eps
                    q = w1 / hq
                    angle = (np.arctan(q) - np.arctan(w2 / (h2 + eps))) * 2 / math.pi
                    v = angle * angle
                    r = v / (1 - iou + v + eps)
                    g_iou = -1.0 + r * r
                    g_q = (2 * r - r * r) * (2 * angle) * (2 / math.pi) / (1 + q * q)
                    g_w1, g_h1 = g_q / hq, -(g_q * w1) / (hq * hq)
        g_uni_t = g_uni - g_iou * (inter / (U * U))
        g_inter = g_iou / U - g_uni_t
        g_iw = g_inter * ih if iwr >= 0 else 0.0
        g_ih = g_inter * iw if ihr >= 0 else 0.0
        ax, ay = g_uni_t * h1, g_uni_t * w1
        return np.array([-(g_iw * _d_max(p[0], t[0])) - ax - g_ew * _d_min(p[0], t[0]) - 0.5 * g_ddx - g_w1,
                         -(g_ih * _d_max(p[1], t[1])) - ay - g_eh * _d_min(p[1], t[1]) - 0.5 * g_ddy - g_h1,
                         g_iw * _d_min(p[2], t[2]) + ax + g_ew * _d_max(p[2], t[2]) - 0.5 * g_ddx + g_w1,
                         g_ih * _d_min(p[3], t[3]) + ay + g_eh * _d_max(p[3], t[3]) - 0.5 * g_ddy + g_h1], np.float64)


def decode_chain(box, x, y, stride=4, box_log=False, box_multiplier=1.0):
    """d(loss_ref.decode_box) / d(the four box values at the pixel), float64, from the decode's own fp32 intermediates."""
    f = np.float32
    v = np.asarray(box, np.float32)[:, y, x]
    if box_log:
        with np.errstate(over="ignore"):
            v = np.exp(v)
    m = v * f(box_multiplier)
    side = np.array([-1.0, -1.0, 1.0, 1.0])
    chain = side * float(f(stride)) * float(f(box_multiplier)) * (v.astype(np.float64) if box_log else 1.0)
    return np.where(m >= 0, chain, 0.0)


def detection_loss_grad(heatmap, box_2d, targets, stride=4, heatmap_target="cornernet", heatmap_target_params=None, heatmap_loss="cornernet_focal",
                        box_loss="giou", heatmap_loss_weight=1.0, box_loss_weight=1.0, box_log=False, box_multiplier=1.0, alpha=2.0, beta=None,
                        heatmap_scale=1.0, box_scale=1.0):
    """heatmap [N, C, H, W] fp32 logits, box_2d [N, 4, H, W] fp32, targets [(boxes [M, 4] f64, labels [M])] ->
    {"heatmap_grad", "box_2d_grad": fp32; "heatmap_grad64", "box_2d_grad64": the same before the rounding; "touched" [N, H, W] bool: pixels some
    sample touches; "contributions" [N, H, W] int; "skipped", "num_dets", "num_boxes"}.  (The loss weights are not applied: the scales are.)"""
    heatmap, box_2d = np.asarray(heatmap, np.float32), np.asarray(box_2d, np.float32)
    N, C, H, W = heatmap.shape
    param = None
    if heatmap_target_params:
        (param,) = heatmap_target_params.values()
    recs = [loss_ref.records(boxes, labels, C, H, W, stride, heatmap_target, param) for boxes, labels in targets]
    num_dets = sum(r["state"] for rs in recs for r in rs)
    num_boxes = sum(len(loss_ref.samples(r, H, W)) for rs in recs for r in rs)
    skipped = sum(1 - r["state"] for rs in recs for r in rs)
    s_heat, s_box = float(heatmap_scale) / max(1.0, float(num_dets)), float(box_scale) / max(1.0, float(num_boxes))
    gh = np.zeros((N, C, H, W), np.float64)
    gb = np.zeros((N, 4, H, W), np.float64)
    hits = np.zeros((N, H, W), np.int64)
    for n, (boxes, labels) in enumerate(targets):
        gh[n] = s_heat * heatmap_dterms(heatmap[n], loss_ref.render(recs[n], C, H, W), heatmap_loss, alpha, beta)
        for rec, box in zip(recs[n], np.asarray(boxes, np.float64).reshape(-1, 4)):      # slot order, then the forward's sample order
            for (x, y) in loss_ref.samples(rec, H, W):
                g = box_dterm(box_loss, loss_ref.decode_box(box_2d[n], x, y, stride, box_log, box_multiplier), loss_ref.box_target(box))
                gb[n, :, y, x] += g * decode_chain(box_2d[n], x, y, stride, box_log, box_multiplier)
                hits[n, y, x] += 1
    gb *= s_box
    gb[np.broadcast_to((hits == 0)[:, None], gb.shape)] = 0.0
    with np.errstate(over="ignore", under="ignore"):
        return {"heatmap_grad": gh.astype(np.float32), "box_2d_grad": gb.astype(np.float32), "heatmap_grad64": gh, "box_2d_grad64": gb, "touched": hits > 0,
                "contributions": hits, "skipped": int(skipped), "num_dets": int(num_dets), "num_boxes": int(num_boxes)}


def tie_distance(box_2d, targets, C, stride=4, heatmap_target="cornernet", heatmap_target_params=None, box_loss="giou", box_log=False,
                 box_multiplier=1.0, **_):
    """How far the box samples are from every non-differentiable point of the rule, in input pixels (the units of the decoded box): the smallest of
    |pred - target| per coordinate, | |pred - target| - 1 | (smooth_l1), the raw intersection's |width| and |height| (the IoU family) and
    |fl32(v box_multiplier)| stride (the decode's clamp) over all samples.  inf without samples."""
    box_2d = np.asarray(box_2d, np.float32)
    N, _, H, W = box_2d.shape
    param = None
    if heatmap_target_params:
        (param,) = heatmap_target_params.values()
    best = math.inf
    for n, (boxes, labels) in enumerate(targets):
        for rec, box in zip(loss_ref.records(boxes, labels, C, H, W, stride, heatmap_target, param), np.asarray(boxes, np.float64).reshape(-1, 4)):
            t = loss_ref.box_target(box).astype(np.float64)
            for (x, y) in loss_ref.samples(rec, H, W):
                p = loss_ref.decode_box(box_2d[n], x, y, stride, box_log, box_multiplier).astype(np.float64)
                v = box_2d[n, :, y, x]
                m = (np.exp(v) if box_log else v) * np.float32(box_multiplier)
                d = np.abs(p - t)
                near = [d.min(), float(np.abs(m).min()) * float(stride)]
                if box_loss == "smooth_l1":
                    near.append(np.abs(d - 1).min())
                if box_loss not in ("l1", "smooth_l1"):
                    near += [abs(min(p[2], t[2]) - max(p[0], t[0])), abs(min(p[3], t[3]) - max(p[1], t[1]))]
                best = min(best, float(min(near)))
    return best
