"""TEST INFRASTRUCTURE ONLY: the BYTE low-score association rule of include/centernet_gfx950.h restated in numpy + scipy on top of
oracle/tracker_ref.py, and a seeded occlusion scene on which its effect can be counted.

`Tracker` is tracker_ref.Tracker with one more association stage: after the re-ID and box stages (run on the detections with score >=
detection_threshold exactly as there, the reference's indexing quirk included), the tracks still unmatched — under low_match="active" only those
ACTIVE at the start of the step — are matched by box cost alone (float32) against the detections with low_threshold <= score < detection_threshold;
pairs with cost < low_box_threshold are kept.  Such a track takes the detection's box (ORIGINAL index; a measurement for its Kalman filter) and
keeps its embedding; unmatched low detections are dropped, births come from the unmatched high detections only.  low_threshold=None: no stage.
"""
import numpy as np

import tracker_ref
from tracker_ref import TrackState, match_with_threshold


class Tracker(tracker_ref.Tracker):
    def __init__(self, low_threshold=None, low_box_threshold=None, low_match="active", **kw):
        super().__init__(**kw)
        if low_match not in ("active", "all"):
            raise ValueError(low_match)
        if low_threshold is not None and (self.box_cost is None or not 0 <= low_threshold <= self.detection_threshold):
            raise ValueError(low_threshold)
        self.low_threshold = low_threshold
        self.low_box_threshold = self.box_threshold if low_box_threshold is None else low_box_threshold
        self.low_match = low_match
        self.last_matches = None            # stages 1 and 2: (row of the thresholded arrays, track)
        self.last_low_matches = None        # stage 3: (original detection index, track)
        self.last_unmatched_tracks = self.last_unmatched_dets = None

    def update(self, bboxes, labels, scores, embeddings):
        mask = scores >= self.detection_threshold
        low = np.flatnonzero((scores >= self.low_threshold) & (scores < self.detection_threshold)) if self.low_threshold is not None else np.zeros(0, np.int64)
        det_bboxes, det_labels, det_embeddings = bboxes[mask], labels[mask], embeddings[mask]
        self.last_costs = None
        matches, low_matches, unmatched_tracks = [], [], []
        if len(self.tracks) == 0:
            unmatched_dets = range(len(det_bboxes))
        else:
            eligible = [self.low_match == "all" or t.state is TrackState.ACTIVE for t in self.tracks]      # by the state at the start of the step
            trk_emb = np.stack([t.embedding for t in self.tracks], axis=0)
            trk_box = np.stack([t.bbox for t in self.tracks], axis=0)
            reid = self.reid_cost(det_embeddings, trk_emb)
            matches, unmatched_dets, unmatched_tracks = match_with_threshold(reid, self.reid_threshold)
            full_box = None
            if self.box_cost is not None:
                full_box = self.box_cost(det_bboxes, trk_box)
                sub = self.box_cost(det_bboxes[unmatched_dets], trk_box[unmatched_tracks])
                new_matches, ud, ut = match_with_threshold(sub, self.box_threshold)
                matches.extend((unmatched_dets[x], unmatched_tracks[y]) for x, y in new_matches)
                unmatched_dets, unmatched_tracks = [unmatched_dets[x] for x in ud], [unmatched_tracks[y] for y in ut]
            self.last_costs = (reid, full_box)
            U = [t for t in unmatched_tracks if eligible[t]]
            if len(low) and U:
                # the table's boxes are float32 (the filtered ones with a Kalman filter); the cost is float32, scipy converts it to float64
                cost = self.box_cost(bboxes[low].astype(np.float32), trk_box[U].astype(np.float32))
                pairs, _, _ = match_with_threshold(cost, self.low_box_threshold)
                low_matches = [(int(low[x]), U[y]) for x, y in pairs]
                hit = {t for _, t in low_matches}
                unmatched_tracks = [t for t in unmatched_tracks if t not in hit]
            for d, t in matches:
                self.tracks[t].update_matched(bboxes[d], embeddings[d])     # unfiltered arrays: reference quirk
            for d, t in low_matches:                                        # the box of detection d, the embedding as it was
                trk = self.tracks[t]
                emb = trk.embedding
                trk.update_matched(bboxes[d], emb)
                trk.embedding = emb
            for t in unmatched_tracks:
                self.tracks[t].update_unmatched()
        self.last_matches, self.last_low_matches, self.last_unmatched_tracks = matches, low_matches, list(unmatched_tracks)
        self.last_unmatched_dets = list(unmatched_dets)
        for d in unmatched_dets:
            self.tracks.append(tracker_ref.Track(self.next_track_id, det_bboxes[d], det_labels[d], det_embeddings[d],
                                                 min_birth_age=self.min_birth_age, max_inactive_age=self.max_inactive_age,
                                                 smoothing_factor=self.smoothing_factor, use_kalman=self.use_kalman))
            self.next_track_id += 1
        self.tracks = [t for t in self.tracks if not t.to_delete]
        for t in self.tracks:
            if t.kf is not None:
                t.kf.predict()
        self.frame += 1


def synth_occlusion(seed, frames=30, objects=6, k=70, emb_dim=32, sort_scores=True):
    """`objects` boxes on a grid of a unit image (they never overlap one another), drifting slowly, with fixed identity embeddings plus noise and
    scores in [0.5, 0.95) — except for a 4-frame dip per object, staggered from frame 5 on, in which the object is still detected at its place but
    with a score in [0.12, 0.28) and a RANDOM embedding (a half-occluded object).  The other detections of the k are clutter: small boxes anywhere,
    mostly below 0.1, a fifth of them in [0.1, 0.29).
    -> (list of (bboxes (k,4) f32, labels (k,) i64, scores (k,) f32, embeddings (k,E) f32), list of ground-truth boxes (objects,4) f64)."""
    rng = np.random.default_rng(seed)
    cols = int(np.ceil(np.sqrt(objects)))
    rows = -(-objects // cols)
    cell = np.array([1.0 / cols, 1.0 / rows])
    grid = np.array([[(o % cols) + 0.5, (o // cols) + 0.5] for o in range(objects)]) * cell
    centre = grid + (rng.random((objects, 2)) - 0.5) * 0.1 * cell
    vel = (rng.random((objects, 2)) - 0.5) * 0.004 * cell * cols
    size = (rng.random((objects, 2)) * 0.2 + 0.4) * cell
    ident = rng.standard_normal((objects, emb_dim))
    span = max(frames - 5 - 4 - 2, 1)
    dip = [5 + (o * span) // max(objects, 1) for o in range(objects)]
    out, truth = [], []
    for f in range(frames):
        centre = centre + vel
        boxes, scores, embs = [], [], []
        for o in range(objects):
            c = centre[o] + rng.standard_normal(2) * 0.001
            s = size[o] * (1 + rng.standard_normal(2) * 0.01)
            boxes.append([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2])
            if dip[o] <= f < dip[o] + 4:
                scores.append(0.12 + 0.16 * rng.random())
                embs.append(rng.standard_normal(emb_dim))
            else:
                scores.append(0.5 + 0.45 * rng.random())
                embs.append(ident[o] * (1.0 + 0.1 * rng.random()) + 0.08 * rng.standard_normal(emb_dim))
        truth.append(np.array([[c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2] for c, s in zip(centre, size)]))
        for _ in range(k - objects):
            c = rng.random(2)
            s = rng.random(2) * 0.03 + 0.01
            boxes.append([c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2])
            scores.append(0.1 + 0.19 * rng.random() if rng.random() < 0.2 else 0.1 * rng.random())
            embs.append(rng.standard_normal(emb_dim))
        boxes = np.asarray(boxes, np.float32)
        scores = np.asarray(scores, np.float32)
        embs = np.asarray(embs, np.float32)
        order = np.argsort(-scores, kind="stable") if sort_scores else rng.permutation(k)
        out.append((boxes[order], np.zeros(k, np.int64), scores[order], embs[order]))
    return out, truth


def occlusion_counts(tracker, seq, truth):
    """Run `tracker` (anything with update / tracks of bbox, state, track_id) over the scene -> (object-frames without an ACTIVE track within IoU
    distance 0.5, ACTIVE tracks that match no object that way summed over frames, distinct track ids seen per object)."""
    missed, stray = 0, 0
    ids = [set() for _ in range(len(truth[0]))]
    for fr, gt in zip(seq, truth):
        tracker.update(*fr)
        act = [t for t in tracker.tracks if t.state.name == "ACTIVE"]
        if not act:
            missed += len(gt)
            continue
        dist = tracker_ref.box_iou_distance_matrix(gt, np.array([np.asarray(t.bbox, np.float64) for t in act]))
        near = dist < 0.5
        missed += int((~near.any(axis=1)).sum())
        stray += int((~near.any(axis=0)).sum())
        for o in range(len(gt)):
            ids[o].update(act[j].track_id for j in np.flatnonzero(near[o]))
    return missed, stray, [len(x) for x in ids]
