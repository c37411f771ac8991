"""Tracker — host side of the tracking association step.

Mirrors the reference's `Tracker` / `Track` / `match_with_threshold` / `build_tracker`
(centernet_lightning/models/tracker.py:27-43, 45-201, 217-353): same constructor arguments, `step_batch`, `step_single`,
`update`, `reset`, same track life cycle, same outputs ({"bboxes": [...], "track_ids": [...]} per frame).

What moved to the GPU (csrc/track.hip): the detection-threshold mask, the cosine (re-ID) and IoU / GIoU cost matrices, and the
track table itself — per-track embedding and box live in HBM and are updated there.  Per frame only the n x T cost matrices
come to the host, where the Hungarian assignment runs on scipy exactly as in the reference (tracker.py:28), and the short
match list goes back.  The reference instead copies every frame's k x (6+E) detections to the host (tracker.py:107).

`use_kalman=True` (tracker.py:243-262, 281-323): the per-track 8-state filter is a float64 numpy restatement of filterpy's
KalmanFilter (third-party, absent) on the host, beside the life cycle; the filtered boxes are uploaded to the device table.
Per frame: ONE kernel launch (cnl_track_frame_f32) writes the frame record — kept-detection indices, boxes / scores / labels, cost
matrices — straight into mapped host memory, ONE stream synchronisation makes it readable; no copy operation in either direction.
`reid_cost`: "cosine" / "euclidean" / "sqeuclidean" / "cityblock" / "chebyshev" / "canberra" / "braycurtis" / "correlation" have kernels; any other scipy
cdist name or a callable, and a callable `box_cost`
(tracker.py:51, 62-64), are computed on the host from copies only with `allow_host_cost=True` (otherwise the constructor raises).
There is no CPU fallback for the device path: without the HIP library or a GPU, `update` raises.
"""
import contextlib
import ctypes
import warnings
import weakref
from enum import Enum, auto
from typing import List

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import _lib
from .config import load_config

_BOX_MODES = {None: 0, "iou": 1, "giou": 2}
_LABEL_KINDS = {torch.int64: 1, torch.int32: 2, torch.float32: 3}     # det_label element types cnl_track_frame_f32 reads
_REID_METRICS = {"cosine": 0, "euclidean": 1, "sqeuclidean": 2, "cityblock": 3, "chebyshev": 4, "canberra": 5, "braycurtis": 6, "correlation": 7}
# ^ the scipy cdist metrics with a gfx950 kernel (float64, scipy's operation order); "manhattan" etc. are scipy aliases -> host path


_NO_GUARD = contextlib.nullcontext()


def _on(dev):
    """Device guard for the launches below — skipped when `dev` is the current device already (torch.cuda.device() costs ~6 us per use,
    twice per frame)."""
    return _NO_GUARD if torch.cuda.current_device() == dev.index else torch.cuda.device(dev)


class _Mapped:
    """Page-locked host memory that the device addresses through the same pointer (cnl_host_alloc): the frame record the association
    kernel writes and the index lists the table update reads cross PCIe as the kernels' own stores / loads — no copy operation, and one
    stream synchronisation per frame.  `np` is a uint8 view of the whole block (valid while this object lives)."""

    def __init__(self, nbytes):
        lib = _lib.load()
        p = ctypes.c_void_p()
        _lib.check(lib.cnl_host_alloc(nbytes, ctypes.byref(p)), "cnl_host_alloc")
        self.ptr, self.nbytes = p.value, nbytes
        self.np = np.ctypeslib.as_array((ctypes.c_uint8 * nbytes).from_address(self.ptr))
        self._finalizer = weakref.finalize(self, lib.cnl_host_free, ctypes.c_void_p(self.ptr))
        self._finalizer.atexit = False          # at interpreter exit the HIP runtime may be gone already; the process frees the pages


class TrackState(Enum):
    UNCONFIRMED = auto()
    ACTIVE = auto()
    INACTIVE = auto()
    TO_DELETE = auto()


def match_with_threshold(cost_matrix, threshold):
    """tracker.py:27-43: optimal assignment, keeping only pairs with cost < threshold.  Same result and order as the reference's loop
    (matches in row order, unmatched rows / columns ascending), vectorised: the loop over sets cost more than the Hungarian step itself."""
    row_ind, col_ind = linear_sum_assignment(cost_matrix)
    keep = cost_matrix[row_ind, col_ind] < threshold
    rows, cols = row_ind[keep], col_ind[keep]
    free_r = np.ones(cost_matrix.shape[0], dtype=bool)
    free_c = np.ones(cost_matrix.shape[1], dtype=bool)
    free_r[rows] = False
    free_c[cols] = False
    return list(zip(rows.tolist(), cols.tolist())), np.flatnonzero(free_r).tolist(), np.flatnonzero(free_c).tolist()


class BoxKalman:
    """The 8-state constant-velocity Kalman filter the reference builds per track with filterpy (tracker.py:243-262, 281-301, 317-323):
    state = box corners x1 y1 x2 y2 + their velocities, measurement = the corners.  filterpy is third-party and absent from the image;
    its published predict / update equations (filterpy/kalman/kalman_filter.py: x = Fx, P = FPF' + Q;  y = z - Hx, S = HPH' + R,
    K = PH'S^-1, x += Ky, P = (I-KH)P(I-KH)' + KRK') are restated in float64 numpy — "parity unpinned" (no reference test pins it)."""

    def __init__(self, bbox):
        self.x = np.zeros(8)
        self.x[:4] = bbox
        self.F = np.eye(8)
        self.F[:4, 4:] = np.eye(4)
        self.H = np.eye(4, 8)
        wh = np.asarray(bbox[2:], np.float64) - np.asarray(bbox[:2], np.float64)
        std = np.tile(wh, 4)                                  # adapted from DeepSORT (tracker.py:256-260)
        std[:4] /= 10
        std[4:] /= 16
        self.P = np.diag(std ** 2)

    def predict(self):
        wh = self.x[2:4] - self.x[:2]
        std = np.tile(wh, 4)                                  # tracker.py:284-289
        std[:4] /= 20
        std[4:] /= 160
        self.x = self.F @ self.x
        self.P = self.F @ self.P @ self.F.T + np.diag(np.square(std))

    def update(self, z):
        wh = self.x[2:4] - self.x[:2]
        R = np.diag((np.tile(wh, 2) / 20) ** 2)               # tracker.py:318-320
        y = np.asarray(z, np.float64) - self.H @ self.x
        PHT = self.P @ self.H.T
        S = self.H @ PHT + R
        K = PHT @ np.linalg.inv(S)
        self.x = self.x + K @ y
        I_KH = np.eye(8) - K @ self.H
        self.P = I_KH @ self.P @ I_KH.T + K @ R @ K.T
        return self.x[:4].copy()


class Track:
    """Host record of one track (tracker.py:217-347).  bbox / label live here (they are reported every frame); the embedding
    lives in the tracker's device table and is fetched on access."""

    def __init__(self, tracker, track_id, bbox, label, min_birth_age=2, max_inactive_age=30, smoothing_factor=0.9, use_kalman=False):
        self._tracker = tracker
        self.kf = BoxKalman(bbox) if use_kalman else None
        self._row = -1
        self.track_id = track_id
        self.state = TrackState.UNCONFIRMED
        self.birth_age = 0
        self.inactive_age = 0
        self.bbox = bbox
        self.label = label
        self.min_birth_age = min_birth_age
        self.max_inactive_age = max_inactive_age
        self.smoothing_factor = smoothing_factor

    @property
    def active(self):
        return self.state == TrackState.ACTIVE

    @property
    def confirmed(self):
        return self.state != TrackState.UNCONFIRMED

    @property
    def to_delete(self):
        return self.state == TrackState.TO_DELETE

    @property
    def embedding(self):
        return self._tracker._emb[self._row].cpu().numpy()

    def update_matched(self, bbox):
        if self.state == TrackState.UNCONFIRMED:
            self.birth_age += 1
            if self.birth_age >= self.min_birth_age:
                self.state = TrackState.ACTIVE
        elif self.state == TrackState.INACTIVE:
            self.state = TrackState.ACTIVE
            self.inactive_age = 0
        # tracker.py:311-323: the detection's box, or the filtered state when the track carries a Kalman filter
        self.bbox = bbox if self.kf is None else self.kf.update(bbox)

    def kalman_predict(self):
        """tracker.py:281-290 (called at the end of every Tracker.update; `bbox` keeps the last UPDATED state, as in the reference,
        where it is a view of the array that filterpy's predict replaces)."""
        if self.kf is not None:
            self.kf.predict()

    def update_unmatched(self):
        if self.state == TrackState.UNCONFIRMED:
            self.state = TrackState.TO_DELETE
        elif self.state == TrackState.ACTIVE:
            self.state = TrackState.INACTIVE
            self.inactive_age = 0
        elif self.state == TrackState.INACTIVE:
            self.inactive_age += 1
            if self.inactive_age >= self.max_inactive_age:
                self.state = TrackState.TO_DELETE

    def __repr__(self):
        return f"track id: {self.track_id}, bbox: {self.bbox}, label: {self.label}, state: {self.state.name}"


class Tracker:
    """Multiple-object tracking on top of `CenterNet.gather_tracking2d` (tracker.py:45-201)."""

    def __init__(self, model=None, nms_kernel=3, num_detections=300, detection_threshold=0.3, reid_cost="cosine",
                 reid_threshold=0.2, box_cost="iou", box_threshold=0.5, smoothing_factor=0.5, use_kalman=False,
                 max_inactive_age=30, min_birth_age=2, device=None, allow_host_cost=False):
        """reid_cost: "cosine" (default), "euclidean", "sqeuclidean", "cityblock", "chebyshev", "canberra", "braycurtis", "correlation" run on the device.  The reference accepts ANY scipy cdist metric name or
        a callable (tracker.py:51, 62-64), and a callable box_cost: those are computed on the HOST from copies of the frame's kept embeddings /
        boxes and the track table (two more device -> host copies per frame) — only with allow_host_cost=True, otherwise they raise: a silent
        CPU detour is not what a caller of a gfx950 tracker expects."""
        self.model = model
        if model is None:
            warnings.warn("A model was not provided. Only `.update()` will work")
        self._host_reid = None if reid_cost in _REID_METRICS else reid_cost
        self._host_box = box_cost if callable(box_cost) else None
        if (self._host_reid is not None or self._host_box is not None) and not allow_host_cost:
            raise ValueError(f"reid_cost={reid_cost!r} / box_cost={box_cost!r}: only {sorted(_REID_METRICS)} and 'iou' / 'giou' / None have gfx950 "
                             "kernels; pass allow_host_cost=True to compute other scipy metrics or callables on the host (slower: the embeddings "
                             "then travel to the host every frame)")
        if self._host_box is None and box_cost not in _BOX_MODES:
            raise ValueError(f"box_cost={box_cost!r}: expected 'iou', 'giou', None or (with allow_host_cost=True) a callable")
        self.nms_kernel = nms_kernel
        self.num_detections = num_detections
        self.detection_threshold = detection_threshold
        self.reid_cost = reid_cost
        self.reid_threshold = reid_threshold
        self.box_cost = box_cost
        self.box_threshold = box_threshold
        self.smoothing_factor = smoothing_factor
        self.use_kalman = bool(use_kalman)
        self.max_inactive_age = max_inactive_age
        self.min_birth_age = min_birth_age
        self._device = torch.device(device) if device is not None else None
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self):
        self.frame = 0
        self.next_track_id = 0
        self.tracks: List[Track] = []
        self._emb = None            # device track table [capacity, E] / [capacity, 4]; rows 0..len(tracks)-1 are live
        self._box = None
        self._spare = None          # the other half of the ping-pong pair
        self.last_costs = None      # (reid [n,T] f64, box [n,T] f32 | None, det_index [n]) of the last update (host numpy)
        self._rec = None            # mapped host memory the association kernel writes the frame record into (cnl_track_frame_f32)
        self._src = None            # mapped host memory holding the two index lists cnl_track_apply_f32 reads
        self._apply_stream = None   # the stream the last cnl_track_apply_f32 was launched on

    @property
    def device(self):
        if self._device is None:
            if self.model is not None:
                self._device = next(self.model.parameters()).device
            else:
                self._device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        if self._device.type != "cuda":
            raise RuntimeError("the tracker's association kernels need a HIP device ('cuda'); there is no CPU fallback")
        return self._device

    def _tables(self, rows, E):
        """Return (new_emb, new_box) with room for `rows` rows, distinct from the live table."""
        dev = self.device
        if self._spare is None or self._spare[0].shape[0] < rows or self._spare[0].shape[1] != E:
            cap = max(64, 1 << (max(rows, 1) - 1).bit_length())
            self._spare = (torch.empty((cap, E), device=dev, dtype=torch.float32), torch.empty((cap, 4), device=dev, dtype=torch.float32))
        return self._spare

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def step_batch(self, images: torch.Tensor, **kwargs):
        """Run the model on a batch of consecutive frames and update the tracks frame by frame (tracker.py:84-121).
        Returns {"bboxes": [...], "track_ids": [...]} with one list per frame (active tracks only)."""
        nms_kernel = kwargs.get("nms_kernel", self.nms_kernel)
        num_detections = kwargs.get("num_detections", self.num_detections)
        self.model.eval()
        images = images.to(self.device)
        heatmap, box_2d, reid = self.model(images)
        det = self.model.gather_tracking2d(heatmap, box_2d, reid, nms_kernel=nms_kernel, num_detections=num_detections,
                                           normalize_bbox=True)
        # the kernel that computes a frame's costs also writes its boxes / scores / labels into the frame record: no separate copy
        out = {"bboxes": [], "track_ids": []}
        for i in range(images.shape[0]):
            self._update_device(det["bboxes"][i], det["scores"][i], det["embeddings"][i], det["labels"][i], None, **kwargs)
            self.frame += 1
            out["bboxes"].append([x.bbox for x in self.tracks if x.active])
            out["track_ids"].append([x.track_id for x in self.tracks if x.active])
        return out

    @torch.no_grad()
    def step_single(self, img: torch.Tensor, **kwargs):
        out = self.step_batch(img.unsqueeze(0), **kwargs)
        return {k: v[0] for k, v in out.items()}

    def update(self, bboxes, labels, scores, embeddings, **kwargs):
        """Update current tracks with one frame's detections (tracker.py:123-201).  Accepts numpy arrays (as the reference) or
        torch tensors; the arrays are moved to the HIP device, where the association costs are computed."""
        dev = self.device

        def to_dev(a):
            if isinstance(a, torch.Tensor) and a.device == dev and a.dtype == torch.float32 and a.is_contiguous():
                return a                                   # already where the kernels read it (each .to() costs ~7 us of host time)
            return torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if all(isinstance(a, torch.Tensor) and a.is_cuda for a in (bboxes, labels, scores)) and bboxes.dim() == 2:
            # device inputs: the three small arrays the host-side life cycle reads come back inside the frame record
            self._update_device(to_dev(bboxes), to_dev(scores), to_dev(embeddings), labels.to(dev), None, **kwargs)
        else:
            self._update_device(to_dev(bboxes), to_dev(scores), to_dev(embeddings), None, (host(bboxes), host(labels), host(scores)), **kwargs)

    # ------------------------------------------------------------------ one frame
    def _update_device(self, d_box, d_score, d_emb, d_label, host, **kwargs):
        """`host`: (boxes, labels, scores) as numpy arrays when the caller holds them on the host already; None: the frame record
        brings them (d_label: the labels on the device)."""
        detection_threshold = kwargs.get("detection_threshold", self.detection_threshold)
        reid_threshold = kwargs.get("reid_threshold", self.reid_threshold)
        box_threshold = kwargs.get("box_threshold", self.box_threshold)
        lib = _lib.load()
        dev = self.device
        k, E = d_emb.shape
        if d_box.shape != (k, 4) or d_score.shape != (k,):
            raise ValueError(f"detections: boxes {tuple(d_box.shape)}, scores {tuple(d_score.shape)}, embeddings {tuple(d_emb.shape)}")
        d_box, d_score, d_emb = d_box.contiguous(), d_score.contiguous(), d_emb.contiguous()
        T = len(self.tracks)
        box_mode = 0 if self._host_box is not None else _BOX_MODES[self.box_cost]
        reid_metric = _REID_METRICS.get(self.reid_cost, 0)
        with_dets = host is None
        label_kind = 0
        if with_dets and d_label is not None:
            if d_label.shape != (k,):
                raise ValueError(f"detections: labels {tuple(d_label.shape)}, expected ({k},)")
            label_kind = _LABEL_KINDS.get(d_label.dtype, 0)
            if not label_kind:
                d_label, label_kind = d_label.to(torch.int64), 1
            d_label = d_label.contiguous()
        # cnl_track_frame_bytes(k, T, with_dets), in Python (a ctypes call costs ~2 us of a 150 us frame)
        need = ((((32 + 4 * k + 7) & ~7) + (24 * k if with_dets else 0) + 7) & ~7) + 12 * k * T
        with _on(dev):
            cur = torch.cuda.current_stream(dev)
            stream = ctypes.c_void_p(cur.cuda_stream)
            if self._apply_stream is not None and self._apply_stream != cur:
                # the caller changed streams between frames: the previous frame's table update (which reads the mapped index lists and
                # writes the tables this frame reads) ran on another stream — finish it first (same stream: stream order does it)
                self._apply_stream.synchronize()
            if self._rec is None or self._rec.nbytes < need:
                self._rec = _Mapped(max(2 * need, 1 << 18))          # persistent: nothing allocated per frame
            rec = self._rec
            # ONE launch writes the record [header | det_index | boxes scores labels | reid f64 n*T | box f32 n*T] straight into host
            # memory (packed by the n the kernel finds), ONE synchronisation makes it readable: the frame's only device -> host traffic
            _lib.check(lib.cnl_track_frame_f32(d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr() if label_kind else None,
                                               label_kind, k, E, float(detection_threshold), self._emb.data_ptr() if T else None,
                                               self._box.data_ptr() if T else None, T, box_mode, reid_metric, int(with_dets), rec.ptr, rec.nbytes,
                                               stream), "cnl_track_frame_f32")
            cur.synchronize()
        h = rec.np
        hdr = h[:32].view(np.int32)
        n, off_dets, off_reid, off_box = int(hdr[0]), int(hdr[5]), int(hdr[6]), int(hdr[7])
        if with_dets:
            # copies: a Track keeps its box, and the record is overwritten by the next frame
            f = h[off_dets:off_dets + 20 * k].view(np.float32)
            h_box, h_score = f[:4 * k].reshape(k, 4).copy(), f[4 * k:].copy()
            h_label = h[off_dets + 20 * k:off_dets + 24 * k].view(np.int32).astype(np.int64)
        else:
            h_box, h_label, h_score = host
            n_host = int(np.count_nonzero(np.asarray(h_score, dtype=np.float32) >= np.float32(detection_threshold)))
            if n_host != n:
                raise RuntimeError(f"detection count mismatch between host ({n_host}) and device ({n}): scores on the host and on the device differ")
        det_index = h[32:32 + 4 * n].view(np.int32).copy()
        self.d2h_bytes = 32 + 4 * n + (24 * k if with_dets else 0) + (12 if box_mode else 8) * n * T      # bytes the kernel stored over PCIe
        self.last_costs = None

        # ---- assignment on the host: tracker.py:139-176 ----
        if T == 0:
            matches, unmatched_dets, unmatched_tracks = [], list(range(n)), []
        else:
            reid = h[off_reid:off_reid + 8 * n * T].view(np.float64).reshape(n, T)
            if self._host_reid is not None or self._host_box is not None:
                # opt-in host fallback (allow_host_cost=True): the reference's own expressions on copies of the operands
                from scipy.spatial.distance import cdist
                sel = torch.from_numpy(np.ascontiguousarray(det_index[:n]).astype(np.int64)).to(dev)
                if self._host_reid is not None:
                    h_de, h_te = d_emb.index_select(0, sel).cpu().numpy(), self._emb[:T].cpu().numpy()
                    reid = self._host_reid(h_de, h_te) if callable(self._host_reid) else cdist(h_de, h_te, self._host_reid)
                    reid = np.asarray(reid, np.float64).reshape(n, T)
            matches, unmatched_dets, unmatched_tracks = match_with_threshold(reid, reid_threshold)
            box = None
            if self._host_box is not None:
                # tracker.py:157-162 as written: the callable sees the REMAINING detections' and tracks' boxes
                h_db, h_tb = d_box.index_select(0, sel).cpu().numpy(), self._box[:T].cpu().numpy()
                sub = np.asarray(self._host_box(h_db[unmatched_dets], h_tb[unmatched_tracks])).reshape(len(unmatched_dets), len(unmatched_tracks))
                new_matches, ud, ut = match_with_threshold(sub, box_threshold)
                matches.extend((unmatched_dets[x], unmatched_tracks[y]) for x, y in new_matches)
                unmatched_dets, unmatched_tracks = [unmatched_dets[x] for x in ud], [unmatched_tracks[y] for y in ut]
            elif box_mode:
                box = h[off_box:off_box + 4 * n * T].view(np.float32).reshape(n, T)
            if box is not None:
                # element-wise costs: the remaining-pairs matrix of tracker.py:157-162 is a sub-matrix of the full one
                sub = box[np.ix_(unmatched_dets, unmatched_tracks)]
                new_matches, ud, ut = match_with_threshold(sub, box_threshold)
                matches.extend((unmatched_dets[x], unmatched_tracks[y]) for x, y in new_matches)
                unmatched_dets, unmatched_tracks = [unmatched_dets[x] for x in ud], [unmatched_tracks[y] for y in ut]
            self.last_costs = (reid.copy(), None if box is None else box.copy(), det_index.copy())

        # ---- track life cycle (host) + the rows of the new device table ----
        row_det = {}                                  # old track index -> detection row feeding its update
        for det_idx, track_idx in matches:
            # reference quirk kept (tracker.py:171): the match indexes the thresholded arrays but the update reads the
            # unfiltered ones at the same position; identical when scores are sorted descending (gather_tracking2d output)
            self.tracks[track_idx].update_matched(h_box[det_idx])
            row_det[track_idx] = det_idx
        for track_idx in unmatched_tracks:
            self.tracks[track_idx].update_unmatched()
        old_rows = list(range(T))
        for det_idx in unmatched_dets:
            src = int(det_index[det_idx])
            self.tracks.append(Track(self, self.next_track_id, h_box[src], h_label[src], min_birth_age=self.min_birth_age,
                                     max_inactive_age=self.max_inactive_age, smoothing_factor=self.smoothing_factor,
                                     use_kalman=self.use_kalman))
            self.next_track_id += 1
            old_rows.append(-1)
            row_det[len(self.tracks) - 1] = src
        keep = [i for i, t in enumerate(self.tracks) if not t.to_delete]
        self.tracks = [self.tracks[i] for i in keep]
        T_new = len(self.tracks)
        if T_new:
            src = np.empty((2, T_new), np.int32)
            src[0] = [old_rows[i] for i in keep]
            src[1] = [row_det.get(i, -1) for i in keep]
            with _on(dev):
                # the two index lists sit in mapped host memory that the kernel reads directly (2 x T_new int32 over PCIe): no host ->
                # device copy; the synchronisation at the top of the next frame orders the kernel's reads before the next overwrite
                if self._src is None or self._src.nbytes < 8 * T_new:
                    self._src = _Mapped(8 * max(256, 1 << (T_new - 1).bit_length()))
                cap = self._src.nbytes // 8
                self._src.np.view(np.int32).reshape(2, cap)[:, :T_new] = src
                d_src = (self._src.ptr, self._src.ptr + 4 * cap)
                new_emb, new_box = self._tables(T_new, E)
                _lib.check(lib.cnl_track_apply_f32(self._emb.data_ptr() if T else None, self._box.data_ptr() if T else None,
                                                   d_emb.data_ptr(), d_box.data_ptr(), d_src[0], d_src[1],
                                                   T_new, E, float(self.smoothing_factor), new_emb.data_ptr(), new_box.data_ptr(),
                                                   stream), "cnl_track_apply_f32")
                self._apply_stream = cur
            self._spare, (self._emb, self._box) = ((self._emb, self._box) if self._emb is not None else None), (new_emb, new_box)
        for r, t in enumerate(self.tracks):
            t._row = r
        if self.use_kalman and T_new:
            # the device table's boxes are the detections' (cnl_track_apply_f32); a Kalman track's box is its filtered state, computed on
            # the host with the rest of the life cycle (8x8 float64 algebra per track): upload the T x 4 boxes (16 B per track)
            boxes = np.asarray([np.asarray(t.bbox, np.float64) for t in self.tracks], np.float32).reshape(T_new, 4)
            with torch.cuda.device(dev):
                self._box[:T_new].copy_(torch.from_numpy(boxes), non_blocking=False)
            for t in self.tracks:
                t.kalman_predict()

    def track_embeddings(self):
        """Device view [T, E] of the live track table (row order = self.tracks)."""
        return self._emb[:len(self.tracks)] if self._emb is not None else None


class _StreamState:
    """What `TrackerBank[s]` returns: the per-stream state, named as Tracker's (`tracks` are Track objects)."""
    __slots__ = ("tracks", "frame", "next_track_id")

    def __init__(self):
        self.tracks: List[Track] = []
        self.frame = 0
        self.next_track_id = 0


class TrackerBank:
    """S independent trackers whose unit of work is ONE FRAME FROM EACH STREAM (csrc/track_streams.hip): `step_batch(images)` takes frame i
    as the next frame of stream i — what a live deployment with S cameras has in hand — where `Tracker.step_batch` takes the batch as
    consecutive frames of one video.  Per step: one association pass on the device for all streams (threshold mask, cost matrices, BOTH
    assignment stages — the Hungarian step runs on the GPU, one workgroup per stream, with scipy's exact result), ONE stream
    synchronisation, the track life cycle per stream on the host from the match lists, one pooled table update.  No cost matrix crosses
    PCIe.  Same constructor arguments, defaults and results as `Tracker`, one setting for all streams; host-side costs
    (`allow_host_cost` metrics, callables) are refused: the bank exists to keep the matrices on the device.

    A stream whose costs are not finite (e.g. a zero embedding under "cosine") is redone through the single-stream host path, so the
    caller sees what `Tracker` raises there (scipy's ValueError); the exception leaves EVERY stream of the bank as it was before the step."""

    def __init__(self, num_streams, model=None, nms_kernel=3, num_detections=300, detection_threshold=0.3, reid_cost="cosine",
                 reid_threshold=0.2, box_cost="iou", box_threshold=0.5, smoothing_factor=0.5, use_kalman=False,
                 max_inactive_age=30, min_birth_age=2, device=None, allow_host_cost=False):
        if isinstance(num_streams, bool) or not isinstance(num_streams, (int, np.integer)) or num_streams < 1:
            raise ValueError(f"num_streams={num_streams!r}: expected an integer >= 1")
        if callable(reid_cost) or callable(box_cost) or reid_cost not in _REID_METRICS:
            raise ValueError(f"reid_cost={reid_cost!r} / box_cost={box_cost!r}: a TrackerBank keeps the cost matrices on the device; only "
                             f"{sorted(_REID_METRICS)} and 'iou' / 'giou' / None have gfx950 kernels (allow_host_cost does not apply: use one "
                             "Tracker per stream for host-side costs)")
        if box_cost not in _BOX_MODES:
            raise ValueError(f"box_cost={box_cost!r}: expected 'iou', 'giou' or None")
        self.model = model
        if model is None:
            warnings.warn("A model was not provided. Only `.update_batch()` will work")
        self.num_streams = int(num_streams)
        self.nms_kernel = nms_kernel
        self.num_detections = num_detections
        self.detection_threshold = detection_threshold
        self.reid_cost = reid_cost
        self.reid_threshold = reid_threshold
        self.box_cost = box_cost
        self.box_threshold = box_threshold
        self.smoothing_factor = smoothing_factor
        self.use_kalman = bool(use_kalman)
        self.max_inactive_age = max_inactive_age
        self.min_birth_age = min_birth_age
        self._device = torch.device(device) if device is not None else None
        self._streams = [_StreamState() for _ in range(self.num_streams)]
        self._emb = self._box = self._spare = None      # pooled device table: stream s owns rows _off[s] .. _off[s + 1]
        self._off = np.zeros(self.num_streams + 1, np.int64)
        self._rec = self._ctl = self._src = self._ws = None     # mapped records / live list + trk_off / apply index lists; device workspace
        self._apply_stream = None
        self.d2h_bytes = 0
        self.last_matches = [None] * self.num_streams

    device = Tracker.device
    _tables = Tracker._tables

    def __len__(self):
        return self.num_streams

    def __getitem__(self, s):
        return self._streams[s]

    def track_embeddings(self, s):
        """Device view [T_s, E] of stream s's rows of the pooled table (row order = self[s].tracks)."""
        return self._emb[int(self._off[s]):int(self._off[s + 1])] if self._emb is not None else None

    # ------------------------------------------------------------------ state
    def reset(self, stream=None):
        """Forget every stream (None) or one stream; the other streams keep tracks, counters and table rows."""
        if stream is None:
            if self._apply_stream is not None:
                self._apply_stream.synchronize()
            self._streams = [_StreamState() for _ in range(self.num_streams)]
            self._emb = self._box = self._spare = None
            self._off[:] = 0
            self.last_matches = [None] * self.num_streams
            return
        s = self._check_streams([stream])[0]
        self._streams[s] = _StreamState()
        self.last_matches[s] = None
        if self._off[s + 1] == self._off[s]:
            return
        # repack the pooled table without stream s's rows: the pooled apply launch with every kept row copied through (src_det = -1)
        E = self._emb.shape[1]
        rows = np.concatenate([np.arange(self._off[t], self._off[t + 1]) for t in range(self.num_streams) if t != s] + [np.zeros(0, np.int64)])
        dev = self.device
        with _on(dev):
            cur = torch.cuda.current_stream(dev)
            if self._apply_stream is not None:
                self._apply_stream.synchronize()      # its reads of the index lists come before this overwrite
            self._apply(rows.astype(np.int32), np.full(len(rows), -1, np.int32), E, self._emb, self._box, cur)
        self._set_offsets()

    def _set_offsets(self):
        r = 0
        for s, st in enumerate(self._streams):
            self._off[s] = r
            for t in st.tracks:
                t._row = r
                r += 1
        self._off[self.num_streams] = r

    def _check_streams(self, streams):
        S = self.num_streams
        live = list(range(S)) if streams is None else [int(x) for x in streams]
        if not live or any(x < 0 or x >= S for x in live) or len(set(live)) != len(live):
            raise ValueError(f"streams={streams!r}: expected distinct stream indices in 0..{S - 1}, at least one")
        return live

    def _apply(self, src_trk, src_det, E, d_emb, d_box, cur):
        """The pooled table update: one cnl_track_apply_f32 launch over the rows of all streams, index lists in mapped host memory."""
        lib = _lib.load()
        R_new = len(src_trk)
        if R_new == 0:
            return
        if self._src is None or self._src.nbytes < 8 * R_new:
            self._src = _Mapped(8 * max(1024, 1 << (R_new - 1).bit_length()))
        cap = self._src.nbytes // 8
        lists = self._src.np.view(np.int32).reshape(2, cap)
        lists[0, :R_new] = src_trk
        lists[1, :R_new] = src_det
        new_emb, new_box = self._tables(R_new, E)
        has_old = self._emb is not None
        _lib.check(lib.cnl_track_apply_f32(self._emb.data_ptr() if has_old else None, self._box.data_ptr() if has_old else None,
                                           d_emb.data_ptr(), d_box.data_ptr(), self._src.ptr, self._src.ptr + 4 * cap, R_new, E,
                                           float(self.smoothing_factor), new_emb.data_ptr(), new_box.data_ptr(),
                                           ctypes.c_void_p(cur.cuda_stream)), "cnl_track_apply_f32")
        self._apply_stream = cur
        self._spare, (self._emb, self._box) = ((self._emb, self._box) if has_old else None), (new_emb, new_box)

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def step_batch(self, images: torch.Tensor, streams=None, **kwargs):
        """Run the model on one frame from each participating stream (images[i] is the next frame of stream streams[i]; default: stream i)
        and advance those streams.  Returns {"bboxes": [...], "track_ids": [...]} with one list per image (active tracks only)."""
        live = self._check_streams(streams)
        if images.dim() != 4 or images.shape[0] != len(live):
            raise ValueError(f"images {tuple(images.shape)}: expected [{len(live)}, 3, H, W], one frame per participating stream")
        nms_kernel = kwargs.get("nms_kernel", self.nms_kernel)
        num_detections = kwargs.get("num_detections", self.num_detections)
        self.model.eval()
        images = images.to(self.device)
        heatmap, box_2d, reid = self.model(images)
        det = self.model.gather_tracking2d(heatmap, box_2d, reid, nms_kernel=nms_kernel, num_detections=num_detections,
                                           normalize_bbox=True)
        self._step(det["bboxes"], det["scores"], det["embeddings"], det["labels"], None, live, **kwargs)
        out = {"bboxes": [], "track_ids": []}
        for s in live:
            st = self._streams[s]
            st.frame += 1
            out["bboxes"].append([x.bbox for x in st.tracks if x.active])
            out["track_ids"].append([x.track_id for x in st.tracks if x.active])
        return out

    def update_batch(self, bboxes, labels, scores, embeddings, streams=None, **kwargs):
        """One frame's detections for each participating stream: [L, k, 4], [L, k], [L, k], [L, k, E] (numpy arrays or torch tensors; L =
        len(streams), default every stream).  As `Tracker.update`, it does not advance `frame`."""
        live = self._check_streams(streams)
        dev = self.device
        for name, a, nd in (("bboxes", bboxes, 3), ("labels", labels, 2), ("scores", scores, 2), ("embeddings", embeddings, 3)):
            if a.ndim != nd or a.shape[0] != len(live):
                raise ValueError(f"{name} {tuple(a.shape)}: expected {nd} dimensions with {len(live)} streams in front")

        def to_dev(a):
            if isinstance(a, torch.Tensor) and a.device == dev and a.dtype == torch.float32 and a.is_contiguous():
                return a
            return torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()
        host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if all(isinstance(a, torch.Tensor) and a.is_cuda for a in (bboxes, labels, scores)):
            self._step(to_dev(bboxes), to_dev(scores), to_dev(embeddings), labels.to(dev), None, live, **kwargs)
        else:
            self._step(to_dev(bboxes), to_dev(scores), to_dev(embeddings), None, (host(bboxes), host(labels), host(scores)), live, **kwargs)

    # ------------------------------------------------------------------ one step
    def _host_association(self, i, s, d_box, d_score, d_emb, detection_threshold, reid_threshold, box_threshold):
        """Stream s's association through the single-stream path (cnl_track_frame_f32 + scipy on the host) on its slice of the operands:
        what a stream with non-finite costs is redone with, so that the caller sees what Tracker raises (scipy: ValueError)."""
        lib = _lib.load()
        dev = self.device
        k, E = d_emb.shape[1], d_emb.shape[2]
        t0, T = int(self._off[s]), int(self._off[s + 1] - self._off[s])
        box_mode, metric = _BOX_MODES[self.box_cost], _REID_METRICS[self.reid_cost]
        rec = _Mapped(int(lib.cnl_track_frame_bytes(k, T, 0)))
        with _on(dev):
            cur = torch.cuda.current_stream(dev)
            _lib.check(lib.cnl_track_frame_f32(d_emb[i].data_ptr(), d_box[i].data_ptr(), d_score[i].data_ptr(), None, 0, k, E,
                                               float(detection_threshold), self._emb[t0:].data_ptr() if T else None,
                                               self._box[t0:].data_ptr() if T else None, T, box_mode, metric, 0, rec.ptr, rec.nbytes,
                                               ctypes.c_void_p(cur.cuda_stream)), "cnl_track_frame_f32")
            cur.synchronize()
        h = rec.np
        hdr = h[:32].view(np.int32)
        n, off_reid, off_box = int(hdr[0]), int(hdr[6]), int(hdr[7])
        if T == 0:
            return [], list(range(n)), []
        reid = h[off_reid:off_reid + 8 * n * T].view(np.float64).reshape(n, T)
        matches, ud, ut = match_with_threshold(reid, reid_threshold)
        if box_mode:
            box = h[off_box:off_box + 4 * n * T].view(np.float32).reshape(n, T)
            new_matches, ud2, ut2 = match_with_threshold(box[np.ix_(ud, ut)], box_threshold)
            matches.extend((ud[x], ut[y]) for x, y in new_matches)
            ud, ut = [ud[x] for x in ud2], [ut[y] for y in ut2]
        return matches, ud, ut

    def _step(self, d_box, d_score, d_emb, d_label, host, live, **kwargs):
        detection_threshold = kwargs.get("detection_threshold", self.detection_threshold)
        reid_threshold = kwargs.get("reid_threshold", self.reid_threshold)
        box_threshold = kwargs.get("box_threshold", self.box_threshold)
        lib = _lib.load()
        dev = self.device
        S, L = self.num_streams, len(live)
        if d_emb.dim() != 3 or d_emb.shape[0] != L:
            raise ValueError(f"detections: embeddings {tuple(d_emb.shape)}, expected [{L}, k, E]")
        k, E = int(d_emb.shape[1]), int(d_emb.shape[2])
        if d_box.shape != (L, k, 4) or d_score.shape != (L, k):
            raise ValueError(f"detections: boxes {tuple(d_box.shape)}, scores {tuple(d_score.shape)}, embeddings {tuple(d_emb.shape)}")
        d_box, d_score, d_emb = d_box.contiguous(), d_score.contiguous(), d_emb.contiguous()
        with_dets = host is None
        label_kind = 0
        if with_dets and d_label is not None:
            if d_label.shape != (L, k):
                raise ValueError(f"detections: labels {tuple(d_label.shape)}, expected ({L}, {k})")
            label_kind = _LABEL_KINDS.get(d_label.dtype, 0)
            if not label_kind:
                d_label, label_kind = d_label.to(torch.int64), 1
            d_label = d_label.contiguous()
        elif not with_dets and any(a.shape[:2] != (L, k) for a in host):
            raise ValueError(f"detections: boxes {host[0].shape}, labels {host[1].shape}, scores {host[2].shape}, expected [{L}, {k}, ...]")
        off = self._off
        R = int(off[S])
        T_max = max(int(off[s + 1] - off[s]) for s in live)
        box_mode, metric = _BOX_MODES[self.box_cost], _REID_METRICS[self.reid_cost]
        # cnl_track_streams_record_bytes / cnl_track_streams_workspace_bytes, in Python (a ctypes call costs ~2 us)
        off_dets = (64 + 4 * k + 7) & ~7
        off_match = off_dets + (24 * k if with_dets else 0)
        off_udet, off_utrk = off_match + 8 * k, off_match + 12 * k
        stride = (off_utrk + 4 * T_max + 7) & ~7
        ws_need = 20 * k * R + 4 * (S + 2 * S * k + 2 * R)
        with _on(dev):
            cur = torch.cuda.current_stream(dev)
            stream = ctypes.c_void_p(cur.cuda_stream)
            if self._apply_stream is not None and self._apply_stream != cur:
                self._apply_stream.synchronize()        # the previous step's table update ran on another stream: finish it first
            if self._rec is None or self._rec.nbytes < S * stride:
                self._rec = _Mapped(max(2 * S * stride, 1 << 16))
            if self._ws is None or self._ws.numel() < ws_need:
                self._ws = torch.empty(max(2 * ws_need, 1 << 20), device=dev, dtype=torch.uint8)
            if self._ctl is None:
                self._ctl = _Mapped(4 * (2 * S + 1))
            # live list and trk_off sit in mapped memory of their own: the association kernels that read them have finished at this step's
            # synchronisation, whereas the apply launch still reads ITS lists (self._src) after the host has moved on — those are
            # overwritten only behind the next step's synchronisation, which follows that launch in stream order
            ctl = self._ctl.np.view(np.int32)
            ctl[:L] = live
            ctl[S:2 * S + 1] = off
            rec = self._rec
            _lib.check(lib.cnl_track_streams_f32(d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr() if label_kind else None,
                                                 label_kind, S, L, self._ctl.ptr, k, E, float(detection_threshold), float(reid_threshold),
                                                 float(box_threshold), self._emb.data_ptr() if R else None, self._box.data_ptr() if R else None,
                                                 self._ctl.ptr + 4 * S, R, T_max, box_mode, metric, int(with_dets), self._ws.data_ptr(),
                                                 self._ws.numel(), rec.ptr, stride, stream), "cnl_track_streams_f32")
            cur.synchronize()
        h = rec.np
        # ---- read every stream's lists first: an exception leaves all streams untouched ----
        assoc, d2h = [], 0
        for i, s in enumerate(live):
            r = h[s * stride:(s + 1) * stride]
            hdr = r[:64].view(np.int32)
            n, T, status, m, nu, nt = int(hdr[0]), int(hdr[2]), int(hdr[3]), int(hdr[9]), int(hdr[11]), int(hdr[12])
            det_index = r[64:64 + 4 * n].view(np.int32).copy()
            if status in (3, 4, 19):
                raise ValueError(f"stream {s}: association status {status} (k = {k}, T = {T}: beyond the supported sizes)")
            if status:
                matches, ud, ut = self._host_association(i, s, d_box, d_score, d_emb, detection_threshold, reid_threshold, box_threshold)
            else:
                matches = r[off_match:off_match + 8 * m].view(np.int32).reshape(m, 2).tolist()
                matches = [tuple(p) for p in matches]
                ud = r[off_udet:off_udet + 4 * nu].view(np.int32).tolist()
                ut = r[off_utrk:off_utrk + 4 * nt].view(np.int32).tolist()
            if with_dets:
                f = r[off_dets:off_dets + 20 * k].view(np.float32)
                h_box, h_score = f[:4 * k].reshape(k, 4).copy(), None
                h_label = r[off_dets + 20 * k:off_dets + 24 * k].view(np.int32).astype(np.int64)
            else:
                h_box, h_label, h_score = host[0][i], host[1][i], host[2][i]
                n_host = int(np.count_nonzero(np.asarray(h_score, dtype=np.float32) >= np.float32(detection_threshold)))
                if n_host != n:
                    raise RuntimeError(f"stream {s}: detection count mismatch between host ({n_host}) and device ({n})")
            d2h += 64 + 4 * n + (24 * k if with_dets else 0) + 8 * m + 4 * nu + 4 * nt
            assoc.append((matches, ud, ut, det_index, h_box, h_label))
        self.d2h_bytes = d2h

        # ---- track life cycle per stream (host) + the rows of the new pooled table ----
        slot = {s: i for i, s in enumerate(live)}
        src_trk, src_det = [], []
        for s, st in enumerate(self._streams):
            base = int(off[s])
            if s not in slot:
                src_trk.extend(range(base, base + len(st.tracks)))
                src_det.extend([-1] * len(st.tracks))
                continue
            i = slot[s]
            matches, unmatched_dets, unmatched_tracks, det_index, h_box, h_label = assoc[i]
            self.last_matches[s] = matches
            tracks = st.tracks
            T = len(tracks)
            row_det = {}
            for det_idx, track_idx in matches:
                # reference quirk kept (tracker.py:171), as in Tracker._update_device: the match indexes the thresholded arrays, the update
                # reads the unfiltered ones at the same position
                tracks[track_idx].update_matched(h_box[det_idx])
                row_det[track_idx] = det_idx
            for track_idx in unmatched_tracks:
                tracks[track_idx].update_unmatched()
            old_rows = list(range(T))
            for det_idx in unmatched_dets:
                src = int(det_index[det_idx])
                tracks.append(Track(self, st.next_track_id, h_box[src], h_label[src], min_birth_age=self.min_birth_age,
                                    max_inactive_age=self.max_inactive_age, smoothing_factor=self.smoothing_factor, use_kalman=self.use_kalman))
                st.next_track_id += 1
                old_rows.append(-1)
                row_det[len(tracks) - 1] = src
            keep = [j for j, t in enumerate(tracks) if not t.to_delete]
            st.tracks = [tracks[j] for j in keep]
            src_trk.extend(base + old_rows[j] if old_rows[j] >= 0 else -1 for j in keep)
            src_det.extend(i * k + row_det[j] if j in row_det else -1 for j in keep)
        with _on(dev):
            self._apply(src_trk, src_det, E, d_emb, d_box, cur)
        self._set_offsets()
        R_new = int(off[S])
        if self.use_kalman and R_new:
            # a Kalman track's box is its filtered state, computed on the host with the life cycle: the boxes of all streams go up in ONE copy
            boxes = np.asarray([np.asarray(t.bbox, np.float64) for st in self._streams for t in st.tracks], np.float32).reshape(R_new, 4)
            with torch.cuda.device(dev):
                self._box[:R_new].copy_(torch.from_numpy(boxes), non_blocking=False)
            for s in live:
                for t in self._streams[s].tracks:
                    t.kalman_predict()


def build_tracker(config, model=None, num_streams=None):
    """tracker.py:349-353; with `num_streams`, a TrackerBank of that many streams with the same settings."""
    if isinstance(config, str):
        config = load_config(config)["tracker"]
    if num_streams is not None:
        return TrackerBank(num_streams, model=model, **config)
    return Tracker(model=model, **config)
