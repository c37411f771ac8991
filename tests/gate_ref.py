"""TEST INFRASTRUCTURE ONLY: the class / motion gates of include/centernet_gfx950.h (cnl_track_gate) restated pair by pair in Python floats, a
reference tracking loop built from that restatement and the package's host pieces, and a seeded two-class crossing scene.

`gate_costs` walks the pairs one at a time with Python floats (IEEE float64, one rounding per operation, no fused multiply-add, no BLAS, no
np.sum), every product and sum written out in the header's order: it is the yardstick for the gated kernels' matrices (bit for bit) and for the
vectorised host function `_track_host.gate_costs` that a redone TrackerBank stream goes through.

`Tracker` is the reference loop: numpy tables in place of the device table, the cost kernels' cosine restated here and the oracle's box costs for
the ungated matrices (what the cost kernels produce bit for bit), `gate_costs`, then the package's own host pieces — two_stage_assignment, low_stage, life_cycle — and
tests/kalman_ref.py for the device filter; the table update (cnl_track_apply_f32 / _keep_f32) is restated here, its float32 norm in the kernel's
butterfly order.  It never touches a GPU.
"""
import math

import numpy as np

import kalman_ref
import tracker_ref
from centernet_lightning_amd import _track_host as th

GATE_COST = 1e5
CHI2INV95_4 = 9.4877


def _label(v):
    """A label as the kernels read it: cast to int32 (float labels truncate, as the record's label section does)."""
    return int(np.int32(np.int64(v)))


def mahalanobis(z, x, P):
    """One pair: z the detection's box (4 float32 values), x [8] / P [64] the track's rows of kx / kP -> (m, ok).  Python floats throughout."""
    z = [float(np.float32(v)) for v in z]
    x = [float(v) for v in np.asarray(x, np.float64).reshape(8)[:4]]
    P = np.asarray(P, np.float64).reshape(8, 8)
    a = lambda i, j: float(P[j, i])                # i >= j: the upper triangle, as the filter reads P
    w, h = x[2] - x[0], x[3] - x[1]
    r, y = [], []
    for i in range(4):
        q = (h if i & 1 else w) / 20.0
        r.append(q * q)
        y.append(z[i] - x[i])
    c = [[0.0] * 4 for _ in range(4)]
    L = [[0.0] * 4 for _ in range(4)]
    d = [0.0] * 4
    ok = True

    def div(p, q):                                  # IEEE division where Python raises
        if q == 0.0:
            return math.nan if (p == 0.0 or p != p) else math.copysign(math.inf, p) * math.copysign(1.0, q)
        return p / q

    for j in range(4):
        for i in range(j, 4):
            v = a(i, i) + r[i] if i == j else a(i, j)
            if j > 0:
                acc = c[i][0] * L[j][0]
                for k in range(1, j):
                    acc = acc + c[i][k] * L[j][k]
                v = v - acc
            c[i][j] = v
        d[j] = c[j][j]
        ok = ok and d[j] > 0.0 and d[j] < math.inf
        for i in range(j + 1, 4):
            L[i][j] = div(c[i][j], d[j])
    u = [0.0] * 4
    for i in range(4):
        v = y[i]
        if i > 0:
            acc = L[i][0] * u[0]
            for k in range(1, i):
                acc = acc + L[i][k] * u[k]
            v = v - acc
        u[i] = v
    vv = [div(u[i], d[i]) for i in range(4)]
    m = ((vv[0] * u[0] + vv[1] * u[1]) + vv[2] * u[2]) + vv[3] * u[3]
    return m, ok


def gate_costs(reid, box, low_box, det_labels, trk_labels, det_boxes, kx, kP, motion_gate, motion_weight, det_index=None, low_index=None):
    """The header's rule on ungated matrices: reid float64 [n, T], box float32 [n, T] | None, low_box float32 [n_low, T] | None.  det_labels [k] /
    det_boxes [k, 4]: the frame's arrays; det_index / low_index: the original detection of every row (None: rows 0, 1, ...).  trk_labels None: no
    class gate; motion_gate None (or kx None): no motion gate.  -> gated copies (reid, box, low_box)."""
    reid = np.array(reid, np.float64)
    n, T = reid.shape
    box = None if box is None else np.array(box, np.float32)
    low_box = None if low_box is None else np.array(low_box, np.float32)
    det_index = list(range(n)) if det_index is None else [int(v) for v in det_index]
    if low_box is not None:
        low_index = list(range(low_box.shape[0])) if low_index is None else [int(v) for v in low_index]
    for r in range(n):
        dl = _label(det_labels[det_index[r]]) if trk_labels is not None else 0
        for t in range(T):
            if trk_labels is not None and dl != _label(trk_labels[t]):
                reid[r, t] = GATE_COST
                if box is not None:
                    box[r, t] = np.float32(GATE_COST)
                continue
            if motion_gate is None or kx is None:
                continue
            m, ok = mahalanobis(det_boxes[det_index[r]], kx[t], kP[t])
            if not ok or not (m <= motion_gate):
                reid[r, t] = GATE_COST
            elif motion_weight != 1.0:
                reid[r, t] = motion_weight * float(reid[r, t]) + (1.0 - motion_weight) * m
    if low_box is not None and trk_labels is not None:
        for x in range(low_box.shape[0]):
            dl = _label(det_labels[low_index[x]])
            for t in range(T):
                if dl != _label(trk_labels[t]):
                    low_box[x, t] = np.float32(GATE_COST)
    return reid, box, low_box


def cosine_costs(det_emb, trk_emb):
    """The cost kernels' "cosine" re-ID matrix (csrc/track_costs.h) in numpy: u.u, v.v and u.v in float64, each accumulated sequentially over the
    elements, then 1 - clamp(u.v / (sqrt(u.u) * sqrt(v.v))).  (scipy's cdist agrees to a few ulp only: it is not the yardstick for bits.)"""
    u, v = np.asarray(det_emb, np.float32).astype(np.float64), np.asarray(trk_emb, np.float32).astype(np.float64)
    n, T = len(u), len(v)
    uu, vv, uv = np.zeros((n, 1)), np.zeros((1, T)), np.zeros((n, T))
    for e in range(u.shape[1]):
        uu = uu + u[:, e, None] * u[:, e, None]
        vv = vv + v[None, :, e] * v[None, :, e]
        uv = uv + u[:, e, None] * v[None, :, e]
    with np.errstate(all="ignore"):
        c = uv / (np.sqrt(uu) * np.sqrt(vv))
    c = np.where(np.abs(c) > 1.0, np.copysign(1.0, c), c)
    return 1.0 - c


# ----------------------------------------------------------------------------------------------------------------------- the table update
def apply_rows(emb, box, det_emb, det_box, src_trk, src_det, smoothing, keep_emb=None):
    """cnl_track_apply_f32 / cnl_track_apply_keep_f32 in numpy float32: |e| is the kernel's — lane l sums e[l], e[l + 64], ... squared, then the
    64 lanes combine through the xor butterfly (offsets 32 .. 1) — and the blend (keep * old) + (blend * e / |e|) with float32 scalars."""
    E = det_emb.shape[1]
    rows = len(src_trk)
    new_emb, new_box = np.zeros((rows, E), np.float32), np.zeros((rows, 4), np.float32)
    keep, blend = np.float32(1.0 - smoothing), np.float32(smoothing)
    lanes = np.arange(64)
    for r, (t, d) in enumerate(zip(src_trk, src_det)):
        carry = d < 0 or (keep_emb is not None and t >= 0 and keep_emb[r])
        if carry:
            new_emb[r] = emb[t]
        else:
            e = det_emb[d]
            s = np.zeros(64, np.float32)
            for q in range(E):
                s[q & 63] = s[q & 63] + e[q] * e[q]
            for o in (32, 16, 8, 4, 2, 1):
                s = s + s[lanes ^ o]
            unit = e / np.sqrt(s[0])
            new_emb[r] = unit if t < 0 else (keep * emb[t]) + (blend * unit)
        new_box[r] = det_box[d] if d >= 0 else box[t]
    return new_emb, new_box


class _Table:
    """What a Track of the reference loop reads its embedding from."""

    def __init__(self, owner):
        self.owner = owner

    def read_row(self, name, row, cur=None):
        return getattr(self.owner, name)[row].copy()


class Tracker:
    """The reference loop: cl.Tracker's constructor arguments (host-side costs excepted), `update`, `tracks`, `last_matches`,
    `last_low_matches`, `last_costs`; `emb` / `box` / `kx` / `kP` are the tables as numpy arrays."""

    def __init__(self, detection_threshold=0.3, reid_threshold=0.2, box_cost="iou", box_threshold=0.5, smoothing_factor=0.5, use_kalman=False,
                 max_inactive_age=30, min_birth_age=2, low_threshold=None, low_box_threshold=None, low_match="active", class_aware=False,
                 motion_gate=None, motion_weight=1.0, kalman="host"):
        self.detection_threshold, self.reid_threshold, self.box_cost, self.box_threshold = detection_threshold, reid_threshold, box_cost, box_threshold
        self.smoothing_factor, self.use_kalman, self.kalman = smoothing_factor, bool(use_kalman), kalman
        self.max_inactive_age, self.min_birth_age = max_inactive_age, min_birth_age
        self.low_threshold, self.low_match = low_threshold, low_match
        self.low_box_threshold = box_threshold if low_box_threshold is None else low_box_threshold
        self.class_aware, self.motion_weight = class_aware, motion_weight
        self.motion_gate = CHI2INV95_4 if motion_gate is True else motion_gate
        assert self.motion_gate is None or (self.use_kalman and kalman == "device")
        self._table = _Table(self)
        self.tracks, self.next_track_id = [], 0
        self.emb = self.box = self.kx = self.kP = None
        self.last_costs = self.last_matches = self.last_low_matches = None
        self.stage1 = None          # the stage-1 (re-ID) matches of the last update: (kept row, track)

    def update(self, bboxes, labels, scores, embeddings):
        bboxes, scores, embeddings = (np.ascontiguousarray(a, np.float32) for a in (bboxes, scores, embeddings))
        labels = np.asarray(labels)
        det_index = np.flatnonzero(scores >= np.float32(self.detection_threshold))
        low = self.low_threshold is not None
        low_index = np.flatnonzero((scores >= np.float32(self.low_threshold)) & (scores < np.float32(self.detection_threshold))) if low else np.zeros(0, np.int64)
        T, n = len(self.tracks), len(det_index)
        reid, box, low_box = np.zeros((n, T)), None, np.zeros((len(low_index), T), np.float32)
        self.last_costs = None
        with np.errstate(all="ignore"):
            if T:
                reid = cosine_costs(embeddings[det_index], self.emb).reshape(n, T)
                if self.box_cost is not None:
                    cost = tracker_ref.BOX_COSTS[self.box_cost]
                    box = cost(bboxes[det_index], self.box).astype(np.float32).reshape(n, T)
                    low_box = cost(bboxes[low_index], self.box).astype(np.float32).reshape(len(low_index), T)
                motion = self.motion_gate is not None
                reid, box, low_box = gate_costs(reid, box, low_box, labels, [t.label for t in self.tracks] if self.class_aware else None, bboxes,
                                                self.kx if motion else None, self.kP if motion else None, self.motion_gate, self.motion_weight,
                                                det_index, low_index)
                self.last_costs = (reid, box, det_index)
                self.stage1 = th.match_with_threshold(reid, self.reid_threshold)[0]
            else:
                self.stage1 = []
            matches, unmatched_dets, unmatched_tracks = th.two_stage_assignment(reid, self.reid_threshold, self.box_threshold, box)
        self.last_matches = matches
        eligible = None if self.low_match == "all" else [t.state is th.TrackState.ACTIVE for t in self.tracks]
        keep_emb = None
        if low:
            low_matches, unmatched_tracks = th.low_stage(low_box, low_index, unmatched_tracks, eligible, self.low_box_threshold)
            self.last_low_matches = low_matches
            self.tracks, self.next_track_id, old_rows, det_rows, keep_emb = th.life_cycle(
                self.tracks, matches, unmatched_dets, unmatched_tracks, det_index, bboxes.copy(), labels.astype(np.int64), self.next_track_id, self,
                low_matches)
        else:
            self.last_low_matches = None
            self.tracks, self.next_track_id, old_rows, det_rows = th.life_cycle(self.tracks, matches, unmatched_dets, unmatched_tracks, det_index,
                                                                                bboxes.copy(), labels.astype(np.int64), self.next_track_id, self)
        rows = len(self.tracks)
        for r, t in enumerate(self.tracks):
            t._row = r
        if rows == 0:
            return                      # (the device tables keep their old rows; nothing reads them)
        self.emb, self.box = apply_rows(self.emb, self.box, embeddings, bboxes, old_rows, det_rows, self.smoothing_factor, keep_emb)
        if self.use_kalman and self.kalman == "device":
            self.kx, self.kP, self.box, out_box, _ = kalman_ref.track_kalman(self.kx, self.kP, bboxes, old_rows, det_rows, np.ones(rows, np.int32), rows,
                                                                            self.box)
            for r, d in enumerate(det_rows):
                if d >= 0:
                    self.tracks[r].bbox = out_box[r].copy()
        elif self.use_kalman:
            self.box = np.asarray([np.asarray(t.bbox, np.float64) for t in self.tracks], np.float32).reshape(rows, 4)
            for t in self.tracks:
                t.kalman_predict()


# ----------------------------------------------------------------------------------------------------------------------- the scene
A, B, C, D = 0, 1, 2, 3         # objects of the crossing scene; classes 0, 1, 0, 2
CLASSES = (0, 1, 0, 2)
JUMP_FRAME = 14
CROSS_FRAMES = (9, 10, 11)


def crossing_scene(frames=30, k=12, emb_dim=8, seed=5):
    """A and B (classes 0 and 1, IDENTICAL embeddings) move towards each other along one line and cross: their boxes overlap with IoU > 0.5 in
    CROSS_FRAMES, and from the first of those frames on B scores higher than A, so the (score-sorted) rows list B first.  C (class 0, an embedding of its own) stands still except at JUMP_FRAME,
    where it is detected on the far side of the frame.  D (class 2) drifts slowly.  Two low-score detections (0.15 .. 0.25) sit on A and D in a
    few frames in which their confident detection is missing (the BYTE stage's case); the rest of the k rows are clutter below 0.05.
    -> (list of (bboxes (k,4) f32, labels (k,) i64, scores (k,) f32, embeddings (k,E) f32), per frame {object: detection row})."""
    rng = np.random.default_rng(seed)
    ident = rng.standard_normal((4, emb_dim))
    ident[B] = ident[A]
    size = np.array([0.16, 0.3])
    out, where = [], []
    for f in range(frames):
        centre = {A: np.array([0.2 + 0.0125 * f, 0.5]), B: np.array([0.45 - 0.0125 * f, 0.5]), C: np.array([0.15, 0.15]),
                  D: np.array([0.7 + 0.002 * f, 0.8])}
        if f == JUMP_FRAME:
            centre[C] = np.array([0.85, 0.15])
        order = [B, A, C, D] if f >= CROSS_FRAMES[0] else [A, B, C, D]          # by score: the rows come out sorted, as the detector's do
        dip = {A: f in (20, 21), D: f in (5, 6)}
        boxes, labs, scores, embs, who = [], [], [], [], []
        for rank, o in enumerate(order):
            c = centre[o]
            who.append(o)
            boxes.append([c[0] - size[0] / 2, c[1] - size[1] / 2, c[0] + size[0] / 2, c[1] + size[1] / 2])
            labs.append(CLASSES[o])
            scores.append(0.2 + 0.01 * o if dip.get(o) else 0.9 - 0.01 * rank)
            embs.append(ident[o])
        while len(boxes) < k:
            c = rng.random(2) * 0.9 + 0.05
            boxes.append([c[0] - 0.01, c[1] - 0.01, c[0] + 0.01, c[1] + 0.01])
            labs.append(int(rng.integers(0, 3)))
            scores.append(0.05 * rng.random())
            embs.append(rng.standard_normal(emb_dim))
        by_score = np.argsort(-np.asarray(scores), kind="stable")
        out.append((np.asarray(boxes, np.float32)[by_score], np.asarray(labs, np.int64)[by_score], np.asarray(scores, np.float32)[by_score],
                    np.asarray(embs, np.float32)[by_score]))
        where.append({o: int(np.flatnonzero(by_score == i)[0]) for i, o in enumerate(who)})
    return out, where


def iou(a, b):
    return 1.0 - float(tracker_ref.box_iou_distance_matrix(np.asarray(a, np.float64)[None], np.asarray(b, np.float64)[None])[0, 0])
