"""Test-only yardstick for the soft merge (numpy): the rule of include/centernet_gfx950.h (cnl_merge_soft_f32) restated literally, TWICE.

soft_merge_ref   the rule as it is written and as the kernel runs it: ONE loop over all classes that always picks the best live working
                 score.  Float64, one numpy operation per operation of the rule, so methods "hard" and "linear" can be compared with the
                 GPU bit for bit; "gaussian" goes through exp, which two platforms round differently by a few float64 ulp.
two_step_ref     what the original CenterNet does: soft-NMS of every class on its own, to exhaustion, then the K best over all classes.
                 Written separately (per class, scalar intersection-over-union, its own bookkeeping); the two must agree exactly.
The candidates (filter, order, cap, the way into the frame) are those of the hard merge: tests/tiled_ref.py.
"""
import numpy as np

import letterbox_ref
import tiled_ref

F = np.float32
D = np.float64
METHODS = {"hard": 0, "linear": 1, "gaussian": 2}


def candidates_ref(boxes, scores, labels, records, v0, v1, max_candidates, score_threshold):
    """Rule 1 for the frame that owns views v0 .. v1 - 1 -> (boxes [M, 4] float32 in the frame, scores [M] float32, labels [M] int64,
    source [M]: the candidate number), in the order of the positions."""
    s = scores[v0:v1].reshape(-1)
    lab = labels[v0:v1].reshape(-1)
    if v1 == v0:
        return np.zeros((0, 4), F), s, lab, np.zeros((0,), np.int64)
    mapped = np.concatenate([tiled_ref.map_boxes_ref(boxes[v], records[v]) for v in range(v0, v1)], axis=0)
    c = np.nonzero(s > F(score_threshold))[0]
    c = c[np.lexsort((c, -s[c]))][:max_candidates]
    return mapped[c], s[c], lab[c], c


def weights_ref(pick, others, method, sigma, iou_threshold):
    """Rule 5: the weights the box `pick` [4] float32 puts on `others` [m, 4] float32 -> [m] float64."""
    if method == 0:
        return np.where(tiled_ref.match_ref(pick, others, iou_threshold, 0), D(0), D(1))
    p, o = pick.astype(D), others.astype(D)
    iw = np.maximum(np.minimum(p[2], o[:, 2]) - np.maximum(p[0], o[:, 0]), D(0))
    ih = np.maximum(np.minimum(p[3], o[:, 3]) - np.maximum(p[1], o[:, 1]), D(0))
    inter = iw * ih
    ua = ((p[2] - p[0]) * (p[3] - p[1]) + (o[:, 2] - o[:, 0]) * (o[:, 3] - o[:, 1])) - inter
    ok = ua > 0
    ov = np.divide(inter, ua, out=np.zeros_like(inter), where=ok)
    if method == 2:
        w = np.exp(-(ov * ov) / D(F(sigma)))
    else:
        w = np.where(ov > D(F(iou_threshold)), D(1) - ov, D(1))
    return np.where(ok, w, D(1))


def soft_merge_ref(boxes, scores, labels, records, frame_first_view, K_out, method="gaussian", sigma=0.5, iou_threshold=0.5,
                   score_threshold=0.001, class_aware=True, max_candidates=4096):
    """Rules 1-6 -> {"bboxes" [N, K_out, 4], "scores" (float32), "labels", "source" int32, "count" int32, "scores64" (the working scores
    before the one rounding to float32), "margin"}.
    "margin": what the comparison of a GAUSSIAN run with another platform rests on, the minimum over the run of (a) the relative gap
    between each pick and the runner-up and (b) the relative distance of every score a pick has changed from score_threshold.  An exact
    tie of two scores that nothing has changed yet is exact on every platform and does not count."""
    boxes, scores, labels = np.asarray(boxes, dtype=F), np.asarray(scores, dtype=F), np.asarray(labels, dtype=np.int64)
    method = METHODS[method]
    N, thr = len(frame_first_view) - 1, D(F(score_threshold))
    out = {"bboxes": np.zeros((N, K_out, 4), F), "scores": np.zeros((N, K_out), F), "labels": np.zeros((N, K_out), np.int64),
           "source": np.full((N, K_out), -1, np.int32), "count": np.zeros((N,), np.int32), "scores64": np.zeros((N, K_out), D), "margin": np.inf}
    for n in range(N):
        cb, cs, cl_, src = candidates_ref(boxes, scores, labels, records, frame_first_view[n], frame_first_view[n + 1], max_candidates,
                                          score_threshold)
        M = len(cs)
        work = cs.astype(D)
        first = work.copy()
        picked = np.zeros(M, dtype=bool)
        for r in range(K_out):
            live = np.nonzero(~picked & (work > thr))[0]
            if len(live) == 0:
                break
            order = live[np.lexsort((live, -work[live]))]                 # the largest working score, among equals the lowest position
            i = order[0]
            if len(order) > 1:
                j = order[1]
                if not (work[i] == work[j] and work[i] == first[i] and work[j] == first[j]):
                    out["margin"] = min(out["margin"], (work[i] - work[j]) / max(abs(work[i]), abs(work[j])))
            out["bboxes"][n, r], out["labels"][n, r], out["source"][n, r] = cb[i], cl_[i], src[i]
            out["scores64"][n, r], out["scores"][n, r] = work[i], F(work[i])
            out["count"][n] = r + 1
            picked[i] = True
            hit = ~picked
            if class_aware:
                hit &= cl_ == cl_[i]
            hit = np.nonzero(hit)[0]
            if len(hit):
                w = weights_ref(cb[i], cb[hit], method, sigma, iou_threshold)
                new = work[hit] * w
                moved = new[(w != 1) & (new != 0)]                           # (x * 1 and 0 * w are exact everywhere)
                if len(moved):
                    out["margin"] = min(out["margin"], float(np.min(np.abs(moved - thr) / np.maximum(np.abs(moved), abs(thr)))))
                work[hit] = new
    return out


# ----------------------------------------------------------------------------- the second restatement
def _overlap(a, b):
    """Intersection over union of two boxes given as Python floats (IEEE float64, one rounding per operation) -> (ov, defined)."""
    iw = max(min(a[2], b[2]) - max(a[0], b[0]), 0.0)
    ih = max(min(a[3], b[3]) - max(a[1], b[1]), 0.0)
    inter = iw * ih
    ua = ((a[2] - a[0]) * (a[3] - a[1]) + (b[2] - b[0]) * (b[3] - b[1])) - inter
    if not ua > 0:
        return 0.0, False
    return inter / ua, True


def _soft_nms_one_class(cb, cs, members, method, sigma, iou_threshold, thr):
    """Plain soft-NMS of the candidates `members` (positions, ascending) to exhaustion -> [(float64 score, position)] in pick order."""
    alive = list(members)
    score = {p: float(cs[p]) for p in members}
    box = {p: [float(v) for v in cb[p]] for p in members}
    picks = []
    while True:
        best = None
        for p in alive:                                                    # ascending positions: a later equal score does not replace
            if score[p] > thr and (best is None or score[p] > score[best]):
                best = p
        if best is None:
            return picks
        picks.append((score[best], best))
        alive.remove(best)
        removed = tiled_ref.match_ref(cb[best], cb[alive], iou_threshold, 0) if method == 0 and alive else ()
        for at, p in enumerate(alive):
            if method == 0:
                w = 0.0 if removed[at] else 1.0                            # the float32 predicate of the hard merge, as it stands
            else:
                ov, defined = _overlap(box[best], box[p])
                if not defined:
                    w = 1.0
                elif method == 2:
                    w = float(np.exp(D(-(ov * ov) / float(F(sigma)))))
                else:
                    w = 1.0 - ov if ov > float(F(iou_threshold)) else 1.0
            score[p] = score[p] * w


def two_step_ref(boxes, scores, labels, records, frame_first_view, K_out, method="gaussian", sigma=0.5, iou_threshold=0.5,
                 score_threshold=0.001, class_aware=True, max_candidates=4096):
    """Soft-NMS per class to exhaustion, then the K_out best over all classes: a stable sort by descending score of the picks listed
    by position -> {"source", "labels", "scores64", "count"}."""
    boxes, scores, labels = np.asarray(boxes, dtype=F), np.asarray(scores, dtype=F), np.asarray(labels, dtype=np.int64)
    method = METHODS[method]
    N, thr = len(frame_first_view) - 1, float(F(score_threshold))
    out = {"labels": np.zeros((N, K_out), np.int64), "source": np.full((N, K_out), -1, np.int32), "count": np.zeros((N,), np.int32),
           "scores64": np.zeros((N, K_out), D)}
    for n in range(N):
        cb, cs, cl_, src = candidates_ref(boxes, scores, labels, records, frame_first_view[n], frame_first_view[n + 1], max_candidates,
                                          score_threshold)
        groups = [np.nonzero(cl_ == c)[0].tolist() for c in np.unique(cl_)] if class_aware else [list(range(len(cs)))]
        picks = []
        for members in groups:
            if members:
                picks += _soft_nms_one_class(cb, cs, members, method, sigma, iou_threshold, thr)
        picks.sort(key=lambda sp: sp[1])                                  # by position ...
        picks.sort(key=lambda sp: -sp[0])                                 # ... then stably by descending score
        for r, (s, p) in enumerate(picks[:K_out]):
            out["scores64"][n, r], out["source"][n, r], out["labels"][n, r] = s, src[p], cl_[p]
        out["count"][n] = min(len(picks), K_out)
    return out


# ----------------------------------------------------------------------------- the candidates the host and the GPU tests share
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5)
FRAME_SIZES = [(480, 640), (375, 500), (600, 333)]


def scale_records(sizes, S, canvas=512):
    """One full-frame view per (frame, scale), frame-major, as detect_multiscale builds them -> (records, frame_first_view)."""
    rec = []
    for (h, w) in sizes:
        for s in SCALES[:S]:
            side = 32 * max(1, int(np.floor(canvas * s / 32 + 0.5)))
            nh, nw, pt, pl = letterbox_ref.geometry(h, w, side, side)
            rec.append((w, h, 0, 0, pl, pt, F(nw) / F(w), F(nh) / F(h)))
    return rec, [n * S for n in range(len(sizes) + 1)]


def planted_candidates(rng, records, ffv, k, n_objects=40, n_classes=3):
    """Objects planted with jittered duplicates, as random_candidates of tests/test_gpu_tiles.py plants them, but with continuous
    scores (ties are the business of the edge cases) and the object's class as the label: each frame has n_objects true boxes, every
    candidate of a view is one of them seen through the view, jittered by a few pixels (30 % exact repeats), in view pixels."""
    V = len(records)
    boxes, labels = np.zeros((V, k, 4), dtype=F), np.zeros((V, k), dtype=np.int64)
    for n in range(len(ffv) - 1):
        fw, fh = records[ffv[n]][0], records[ffv[n]][1]
        cx, cy = rng.uniform(0, fw, n_objects), rng.uniform(0, fh, n_objects)
        bw, bh = rng.uniform(20, 200, n_objects), rng.uniform(20, 200, n_objects)
        cls = rng.integers(0, n_classes, n_objects)
        for v in range(ffv[n], ffv[n + 1]):
            _, _, x0, y0, pl, pt, sx, sy = records[v]
            o = rng.integers(0, n_objects, k)
            j = rng.uniform(-6, 6, (k, 4)) * (rng.random((k, 1)) < 0.7)
            fb = np.stack([cx[o] - bw[o] / 2, cy[o] - bh[o] / 2, cx[o] + bw[o] / 2, cy[o] + bh[o] / 2], axis=1) + j
            boxes[v] = np.stack([(fb[:, 0] - x0) * sx + pl, (fb[:, 1] - y0) * sy + pt, (fb[:, 2] - x0) * sx + pl, (fb[:, 3] - y0) * sy + pt], axis=1).astype(F)
            labels[v] = cls[o]
    scores = rng.uniform(0.02, 1.0, (V, k)).astype(F)
    return boxes, scores, labels


# (N, S, seed): the cases of the comparison with the restatement on the GPU; tests/test_multiscale_host.py proves the gaussian margin of
# every one of them.  A seed whose margin is too small is REPLACED here, never tolerated there.
RANDOM_CASES = [(N, S, 1000 + 10 * N + S) for N in (1, 3) for S in (1, 2, 3, 4, 5)]
RANDOM_KW = dict(sigma=0.5, iou_threshold=0.5, score_threshold=0.05, class_aware=True)
RANDOM_K, RANDOM_K_OUT = 100, 100
MIN_MARGIN = 1e-9


def random_case(N, S, seed):
    rec, ffv = scale_records(FRAME_SIZES[:N], S)
    return planted_candidates(np.random.default_rng(seed), rec, ffv, RANDOM_K) + (rec, ffv)


ONE_VIEW = (1000, 1000, 0, 0, 0, 0, F(1), F(1))          # a view that is the frame: boxes map to themselves


def _grid_boxes(rng, m, step=37.0, size=60.0):
    """m boxes of about size x size on a grid of `step`: neighbours overlap, each box is different."""
    i = np.arange(m)
    x, y = (i % 24) * step, (i // 24) * step
    b = np.stack([x, y, x + size, y + size], axis=1) + rng.uniform(-3, 3, (m, 4))
    return b.astype(F)


def edge_cases():
    """name -> (boxes [V, k, 4], scores, labels, records, frame_first_view, K_out, kwargs): the sizes and values at which the kernel takes
    another path.  Every case holds for all three methods."""
    cases = {}
    rng = np.random.default_rng(424242)

    def one_frame(name, boxes, scores, labels, K_out=100, views=1, **kw):
        m = len(scores) // views
        cases[name] = (np.asarray(boxes, F).reshape(views, m, 4), np.asarray(scores, F).reshape(views, m), np.asarray(labels, np.int64).reshape(views, m),
                       [ONE_VIEW] * views, [0, views], K_out, dict({"score_threshold": 0.05}, **kw))

    for m in (1, 64, 65, 256, 257):                                       # lane, wave and workgroup boundaries of the strided ownership
        one_frame(f"M={m}", _grid_boxes(rng, m), rng.uniform(0.1, 1, m), rng.integers(0, 2, m), K_out=300)
    one_frame("M=2500", _grid_boxes(rng, 2500, 23.0), rng.uniform(0.1, 1, 2500), rng.integers(0, 3, 2500), K_out=120, views=25)      # > 256 x 8
    one_frame("K_out=1", _grid_boxes(rng, 90), rng.uniform(0.1, 1, 90), rng.integers(0, 2, 90), K_out=1)
    one_frame("one class", _grid_boxes(rng, 300), rng.uniform(0.1, 1, 300), np.zeros(300), K_out=80)
    one_frame("distinct classes", _grid_boxes(rng, 300), rng.uniform(0.1, 1, 300), np.arange(300), K_out=400)
    one_frame("class_aware=False", _grid_boxes(rng, 300), rng.uniform(0.1, 1, 300), rng.integers(0, 5, 300), K_out=80, class_aware=False)
    s = rng.uniform(0.02, 1, 400)
    assert (s.astype(F) > F(0.05)).sum() > 300
    one_frame("cap bites", _grid_boxes(rng, 400), s, rng.integers(0, 2, 400), K_out=150, max_candidates=130)
    one_frame("equal scores", _grid_boxes(rng, 200), rng.choice([0.25, 0.5, 0.75], 200), rng.integers(0, 2, 200), K_out=200)
    s = rng.uniform(-0.5, 1, 300)
    s[rng.choice(300, 60, replace=False)] = np.nan
    z = rng.choice(300, 80, replace=False)
    s[z[:40]], s[z[40:]] = 0.0, -0.0
    one_frame("signed zero and NaN scores", _grid_boxes(rng, 300), s, rng.integers(0, 2, 300), K_out=300, score_threshold=-1.0)
    one_frame("signed zero and NaN scores, threshold -0", _grid_boxes(rng, 300), s, rng.integers(0, 2, 300), K_out=300, score_threshold=-0.0)
    b = _grid_boxes(rng, 300)
    b.reshape(-1)[rng.choice(1200, 100, replace=False)] = np.nan          # a NaN coordinate maps to 0
    d = rng.choice(300, 60, replace=False)
    b[d[:30], 2], b[d[30:], 3] = b[d[:30], 0], b[d[30:], 1]                # zero width / zero height
    b[d[:10]] = 0.0                                                        # and the empty box at the origin, ten times: ua = 0 among them
    one_frame("NaN and degenerate boxes", b, rng.uniform(0.1, 1, 300), rng.integers(0, 2, 300), K_out=300)
    # two frames: none of the first one's scores passes, the second has one candidate
    bx = _grid_boxes(rng, 20).reshape(2, 10, 4)
    sc = np.full((2, 10), 0.01, F)
    sc[1, 7] = 0.9
    cases["0 and 1 candidates"] = (bx, sc, np.zeros((2, 10), np.int64), [ONE_VIEW] * 2, [0, 1, 2], 5, {"score_threshold": 0.05})
    return cases


# the other parameters of the decay, run on the edge case "M=257" with K_out = 1000
DECAY_VARIANTS = [{"method": "gaussian", "sigma": 0.1}, {"method": "gaussian", "sigma": 3.0}, {"method": "linear", "iou_threshold": 0.1},
                  {"method": "linear", "iou_threshold": -0.5}, {"method": "hard", "iou_threshold": 0.05}, {"method": "hard", "iou_threshold": -0.5},
                  {"method": "gaussian", "class_aware": False}]


def planted_pair():
    """The point of the feature: two objects of one class that overlap at IoU 0.6 ([0,100]^2 and [25,125] x [0,100]: 7500 / 12500), each
    seen at three scales (views of a 200 x 200 frame at 0.5, 1 and 1.5 times 128) with a sub-pixel jitter -> (boxes, scores, labels,
    records, frame_first_view)."""
    rec = []
    for side in (64, 128, 192):
        nh, nw, pt, pl = letterbox_ref.geometry(200, 200, side, side)
        rec.append((200, 200, 0, 0, pl, pt, F(nw) / F(200), F(nh) / F(200)))
    rng = np.random.default_rng(6)
    objects = np.array([[20, 30, 120, 130], [45, 30, 145, 130]], dtype=D)
    boxes, scores, labels = np.zeros((3, 4, 4), F), np.zeros((3, 4), F), np.zeros((3, 4), np.int64)
    for v, r in enumerate(rec):
        for o in range(2):
            fb = objects[o] + rng.uniform(-0.2, 0.2, 4)
            boxes[v, o] = (fb * np.array([r[6], r[7], r[6], r[7]], D) + np.array([r[4], r[5], r[4], r[5]], D)).astype(F)
            scores[v, o] = F(0.9 - 0.1 * o - 0.02 * v)
    return boxes, scores, labels, rec, [0, 3]
