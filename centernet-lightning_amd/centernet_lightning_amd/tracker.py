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
`kalman="device"` (opt-in; the default "host" is the path above, bit for bit) moves that last per-track state to the device: the table gains
x [T, 8] / P [T, 64] float64, and ONE launch (cnl_track_kalman_f64, csrc/track_kalman.hip) behind the table update initialises the born rows,
updates the matched ones with their detection, carries the others, predicts the rows of the streams that took part and writes the filtered
boxes into the box table and into a mapped record; a SECOND stream synchronisation at the end of the step makes that record readable, so
`Track.bbox` holds the filtered box when update / update_batch / step_batch return.  No BoxKalman exists in that mode, no box upload, no
per-track arithmetic in Python; `Track.kf` is a view (`.x`, `.P`) that fetches the track's row on access.  The rule is the header's
(filterpy's equations, S^-1 through LDL', every sum in index order; tests/kalman_ref.py restates it bit for bit); its one deviation from the
host path: a row whose S has no positive finite pivots (zero-area box, non-finite state) skips its update where np.linalg.inv raises.
Per frame: ONE kernel launch (cnl_track_frame_f32) writes the frame record — kept-detection indices, boxes / scores / labels, cost
matrices — straight into mapped host memory, ONE stream synchronisation makes it readable; no copy operation in either direction.
`reid_cost`: "cosine" / "euclidean" / "sqeuclidean" / "cityblock" / "chebyshev" / "canberra" / "braycurtis" / "correlation" have kernels; any other scipy
cdist name or a callable, and a callable `box_cost`
(tracker.py:51, 62-64), are computed on the host from copies only with `allow_host_cost=True` (otherwise the constructor raises).
There is no CPU fallback for the device path: without the HIP library or a GPU, `update` raises.
`low_threshold` (opt-in; None is the path above, entry points and bytes included): BYTE's low-score association — after the two stages the
tracks still unmatched (`low_match`: the ACTIVE ones, or all) are matched by box cost alone against the detections with low_threshold <=
score < detection_threshold; a match gives the track the detection's box and leaves its embedding row untouched, and a low detection never
starts a track.  `Tracker` reads the low detections' box costs from a larger frame record (cnl_track_frame_low_f32) and assigns on the host
as it does stages 1 and 2; `TrackerBank` runs the stage on the device behind stage 2 (cnl_track_streams_low_f32).  `last_low_matches` lists
the stage's (original detection index, track row) pairs.
`class_aware` / `motion_gate` / `motion_weight` (opt-in; off is the paths above, entry points and bytes included): gates inside the per-pair cost
functions.  A detection may only take a track of its own label (all three stages), and a re-ID pair must lie within the chi-square gate of the
track's predicted filter state (stage 1; needs kalman="device").  A gated pair costs 1e5 — finite, so that scipy never sees an infeasible matrix —
and the assignment code is the one above: it solves the gated matrices and its thresholds reject the gated pairs.  Both paths launch one gated
entry (cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32) that covers the step with and without the low-score stage on the `_low` layouts.
`TrackerBank(lifecycle="device")` (opt-in; "host" is everything above) also runs the track life cycle on the device (cnl_track_lifecycle_i32,
csrc/track_lifecycle.hip): a step is 6 or 7 launches without a synchronisation and returns device tensors; the host reads tracks, counters and
match lists from one download on demand (`snapshot()`, `bank[s].tracks`) and the status words through `check()`.  See its constructor.

`Tracker` (one video) and `TrackerBank` (S videos, one frame each per step) are thin callers of the shared host side in _track_host.py:
normalise the inputs, launch, read the record, assign (or take the device's lists), life cycle, table update, Kalman.
"""
import ctypes
import functools
from typing import List

import numpy as np
import torch

from . import _lib
from ._track_host import (_BOX_MODES, _LIFECYCLE_MODES, _REID_METRICS, _STATES, _STATUS_TOO_LARGE, STATUS_BAD_SHIFT, STATUS_OVERFLOW, BoxKalman,  # noqa: F401
                          ResidentKalman, ResidentState, ResidentTrack, Track, TrackerSettings, TrackState, _grown,
                          _Mapped, _on, check_kept_count, frame_layout, frame_low_layout, gate_costs, launch_frame, launch_frame_gated, launch_frame_low,
                          life_cycle, low_stage,
                          match_with_threshold, normalise_detections, read_stream_low_record, read_stream_record, streams_layout,
                          streams_low_layout, streams_low_workspace_bytes, streams_workspace_bytes, two_stage_assignment)
from .config import load_config


def _active(tracks, out):
    out["bboxes"].append([x.bbox for x in tracks if x.active])
    out["track_ids"].append([x.track_id for x in tracks if x.active])


class Tracker(TrackerSettings):
    """Multiple-object tracking on top of `CenterNet.gather_tracking2d` (tracker.py:45-201)."""

    # ------------------------------------------------------------------ state
    def reset(self):
        self.frame = 0
        self.next_track_id = 0
        self.tracks: List[Track] = []
        self.last_costs = None      # (reid [n,T] f64, box [n,T] f32 | None, det_index [n]) of the last update (host numpy)
        self.last_matches = None    # (kept-detection row, track row) pairs of stages 1 and 2 of the last update
        self.last_low_matches = None        # low_threshold set: (original detection index, track row) pairs of the low-score stage
        self._table.clear()

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def step_batch(self, images: torch.Tensor, **kwargs):
        """Run the model on a batch of consecutive frames and update the tracks frame by frame (tracker.py:84-121).
        Returns {"bboxes": [...], "track_ids": [...]} with one list per frame (active tracks only).
        (kalman="device": two stream synchronisations per frame instead of one, see `update`.)"""
        self._refuse_camera_motion(kwargs, "Tracker")
        det = self._detect(images, kwargs)
        out = {"bboxes": [], "track_ids": []}
        for i in range(images.shape[0]):
            self.update(det["bboxes"][i], det["labels"][i], det["scores"][i], det["embeddings"][i], **kwargs)
            self.frame += 1
            _active(self.tracks, out)
        return out

    @torch.no_grad()
    def step_single(self, img: torch.Tensor, **kwargs):
        out = self.step_batch(img.unsqueeze(0), **kwargs)
        return {k: v[0] for k, v in out.items()}

    # ------------------------------------------------------------------ one frame
    def update(self, bboxes, labels, scores, embeddings, **kwargs):
        """Update current tracks with one frame's detections (tracker.py:123-201).  Accepts numpy arrays (as the reference) or
        torch tensors; the arrays are moved to the HIP device, where the association costs are computed.
        With use_kalman=True, kalman="device" the filter runs in one launch behind the table update, and the call ends with a SECOND stream
        synchronisation (the first makes the frame record readable), so that the filtered boxes are in `Track.bbox` when it returns."""
        self._refuse_camera_motion(kwargs, "Tracker")
        dev = self.device
        d_box, d_score, d_emb, d_label, host, label_kind = normalise_detections(dev, bboxes, labels, scores, embeddings)
        detection_threshold, reid_threshold, box_threshold, low_threshold, low_box_threshold = self._thresholds(kwargs)
        k, E = d_emb.shape
        T = len(self.tracks)
        table = self._table
        box_mode = 0 if self._host_box is not None else _BOX_MODES[self.box_cost]
        with_dets = host is None
        low = low_threshold is not None
        gated = self._gated
        with _on(dev):
            cur = torch.cuda.current_stream(dev)
            table.wait_for_other_stream(cur)
            rec = self._rec = _grown(self._rec, (frame_low_layout if low or gated else frame_layout)(k, T, with_dets).bytes, 1 << 18)
            if gated:
                if self.class_aware and not label_kind:         # host arrays: the class gate reads the labels on the device
                    d_label, label_kind = torch.from_numpy(np.ascontiguousarray(host[1]).astype(np.int64)).to(dev), 1
                # one entry with and without the low-score stage: none = an empty score window
                n, det_index, h_box, h_score, h_label, reid, box, low_index, low_box = launch_frame_gated(
                    _lib.load(), rec, d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr() if label_kind else None, label_kind,
                    k, E, detection_threshold, low_threshold if low else detection_threshold, table.emb.data_ptr() if T else None,
                    table.box.data_ptr() if T else None, T, box_mode, _REID_METRICS.get(self.reid_cost, 0), with_dets,
                    self._gate([(0, self.tracks)], T, table.kx, table.kP), cur)
            elif low:
                n, det_index, h_box, h_score, h_label, reid, box, low_index, low_box = launch_frame_low(
                    _lib.load(), rec, d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr() if label_kind else None, label_kind,
                    k, E, detection_threshold, low_threshold, table.emb.data_ptr() if T else None, table.box.data_ptr() if T else None, T, box_mode,
                    _REID_METRICS.get(self.reid_cost, 0), with_dets, cur)
            else:
                n, det_index, h_box, h_score, h_label, reid, box = launch_frame(
                    _lib.load(), rec, d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr() if label_kind else None, label_kind,
                    k, E, detection_threshold, table.emb.data_ptr() if T else None, table.box.data_ptr() if T else None, T, box_mode,
                    _REID_METRICS.get(self.reid_cost, 0), with_dets, cur)
        if not with_dets:
            h_box, h_label, h_score = host
            check_kept_count(h_score, detection_threshold, n)
        self.d2h_bytes = 32 + 4 * n + (24 * k if with_dets else 0) + (12 if box_mode else 8) * n * T      # bytes the kernel stored over PCIe
        if low or gated:
            self.d2h_bytes += 16 + 4 * len(low_index) * (1 + T)
        self.last_costs = None

        # ---- assignment on the host (tracker.py:139-176), track life cycle, the rows of the new device table ----
        if T and (self._host_reid is not None or self._host_box is not None):
            reid, box = self._host_costs(d_emb, d_box, det_index, reid, box)
        matches, unmatched_dets, unmatched_tracks = two_stage_assignment(reid, reid_threshold, box_threshold, box)
        if T:
            self.last_costs = (reid.copy(), None if box is None or callable(box) else box.copy(), det_index)
        self.last_matches = matches
        keep_emb = None
        if low:
            low_matches, unmatched_tracks = low_stage(low_box, low_index, unmatched_tracks, self._eligible(self.tracks), low_box_threshold)
            self.last_low_matches = low_matches
            self.tracks, self.next_track_id, old_rows, det_rows, keep_emb = life_cycle(
                self.tracks, matches, unmatched_dets, unmatched_tracks, det_index, h_box, h_label, self.next_track_id, self, low_matches)
        else:
            self.last_low_matches = None
            self.tracks, self.next_track_id, old_rows, det_rows = life_cycle(self.tracks, matches, unmatched_dets, unmatched_tracks, det_index,
                                                                             h_box, h_label, self.next_track_id, self)
        if self._device_kalman:             # every track predicts at the end of the step, as on the host path below
            with _on(dev):
                self._apply_with_kalman(self.tracks, old_rows, det_rows, 1, d_emb, d_box, E, cur, keep_emb)
            self.d2h_bytes += 36 * len(self.tracks)
            for r, t in enumerate(self.tracks):
                t._row = r
            return
        with _on(dev):
            table.apply(old_rows, det_rows, d_emb, d_box, E, self.smoothing_factor, cur, keep_emb)
        for r, t in enumerate(self.tracks):
            t._row = r
        if self.use_kalman and self.tracks:
            table.upload_boxes(self.tracks)
            for t in self.tracks:
                t.kalman_predict()

    def _host_costs(self, d_emb, d_box, det_index, reid, box):
        """Opt-in host fallback (allow_host_cost=True): the reference's own expressions on copies of the operands in place of
        the device's -> (re-ID matrix, box matrix | the second stage's callable | None)."""
        from scipy.spatial.distance import cdist
        n, T = reid.shape
        sel = torch.from_numpy(np.ascontiguousarray(det_index).astype(np.int64)).to(d_emb.device)
        if self._host_reid is not None:
            h_de, h_te = d_emb.index_select(0, sel).cpu().numpy(), self._emb[:T].cpu().numpy()
            reid = self._host_reid(h_de, h_te) if callable(self._host_reid) else cdist(h_de, h_te, self._host_reid)
            reid = np.asarray(reid, np.float64).reshape(n, T)
        if self._host_box is None:
            return reid, box
        # tracker.py:157-162 as written: the callable sees the REMAINING detections' and tracks' boxes
        h_db, h_tb = d_box.index_select(0, sel).cpu().numpy(), self._box[:T].cpu().numpy()
        return reid, lambda ud, ut: np.asarray(self._host_box(h_db[ud], h_tb[ut])).reshape(len(ud), len(ut))

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


class _ResidentStream:
    """What `TrackerBank[s]` returns with lifecycle="device": the same names, read from the bank's last download (made on first use after a
    step; ONE device -> host copy for all streams)."""
    __slots__ = ("_bank", "_s")

    def __init__(self, bank, s):
        self._bank, self._s = bank, s

    tracks = property(lambda self: self._bank._resident_tracks(self._s))
    next_track_id = property(lambda self: int(self._bank._download()["next_track_id"][self._s]))
    frame = property(lambda self: self._bank._frames[self._s])


class _ResidentLists:
    """`last_matches` / `last_low_matches` with lifecycle="device": a sequence over the streams, read from the records of the last download."""
    __slots__ = ("_bank", "_low")

    def __init__(self, bank, low):
        self._bank, self._low = bank, low

    def __len__(self):
        return self._bank.num_streams

    def __getitem__(self, s):
        return self._bank._resident_matches(range(self._bank.num_streams)[s], self._low)

    def __iter__(self):
        return (self[s] for s in range(len(self)))


def _lifecycle_options(init):
    """TrackerBank.__init__ with the keyword-only options `lifecycle` and `max_tracks`.  They are taken here, in front of the constructor, so
    that its own parameter list stays the one callers and introspection know: it still ends with `kalman`."""
    @functools.wraps(init)
    def with_options(self, *args, lifecycle="host", max_tracks=256, **kwargs):
        if lifecycle not in _LIFECYCLE_MODES:
            raise ValueError(f"lifecycle={lifecycle!r}: expected 'host' or 'device'")
        if isinstance(max_tracks, bool) or not isinstance(max_tracks, (int, np.integer)) or max_tracks < 1:
            raise ValueError(f"max_tracks={max_tracks!r}: expected an integer >= 1")
        if lifecycle == "device" and max_tracks > 4096:
            raise ValueError(f"max_tracks={max_tracks!r} with lifecycle='device': the device assignment takes at most 4096 tracks per stream")
        self.lifecycle, self.max_tracks = lifecycle, int(max_tracks)
        self._resident = lifecycle == "device"
        self._res = self._snap = None       # lifecycle="device": the ResidentState (allocated by the first step); the last download
        self._step_no = 0
        init(self, *args, **kwargs)
    return with_options


class TrackerBank(TrackerSettings):
    """S independent trackers whose unit of work is ONE FRAME FROM EACH STREAM (csrc/track_streams.hip): `step_batch(images)` takes frame i
    as the next frame of stream i — what a live deployment with S cameras has in hand — where `Tracker.step_batch` takes the batch as
    consecutive frames of one video.  Per step: one association pass on the device for all streams (threshold mask, cost matrices, BOTH
    assignment stages — the Hungarian step runs on the GPU, one workgroup per stream, with scipy's exact result), ONE stream
    synchronisation, the track life cycle per stream on the host from the match lists, one pooled table update.  No cost matrix crosses
    PCIe.  Same constructor arguments, defaults and results as `Tracker`, one setting for all streams; host-side costs
    (`allow_host_cost` metrics, callables) are refused: the bank exists to keep the matrices on the device.

    A stream whose costs are not finite (e.g. a zero embedding under "cosine") is redone through the single-stream host path, so the
    caller sees what `Tracker` raises there (scipy's ValueError); the exception leaves EVERY stream of the bank as it was before the step."""
    _update_name = "update_batch"

    @_lifecycle_options
    def __init__(self, num_streams, model=None, nms_kernel=3, num_detections=300, detection_threshold=0.3, reid_cost="cosine",
                 reid_threshold=0.2, box_cost="iou", box_threshold=0.5, smoothing_factor=0.5, use_kalman=False,
                 max_inactive_age=30, min_birth_age=2, device=None, allow_host_cost=False, low_threshold=None,
                 low_box_threshold=None, low_match="active", class_aware=False, motion_gate=None, motion_weight=1.0, kalman="host"):
        """lifecycle, max_tracks (keyword-only, taken by _lifecycle_options around this constructor): "host" (default) is the bank described
        above — same launches, same bytes; max_tracks is accepted and has no effect.  "device" moves the track life cycle to the device (cnl_track_lifecycle_i32, csrc/track_lifecycle.hip): a
        step is a fixed sequence of launches on the caller's current stream — association (2), life cycle + pack (2), table update (1), the
        filter with kalman="device" (1), emit (1): 6 or 7 — with NO synchronisation and no per-track Python.  `step_batch` / `update_batch`
        then return device tensors ordered on that stream, for L = len(streams): "bboxes" [L, max_tracks, 4] (float32; float64 with the
        filter), "track_ids" / "labels" [L, max_tracks] int64, "count" [L] int32 — the ACTIVE tracks of each participating stream compacted in
        row order, zeros from `count` on; `draw_detections(..., numbers=, count=)` and `crop_detections` take them as they are.
        `bank[s].tracks` / `.next_track_id`, `last_matches[s]`, `last_low_matches[s]` and `snapshot()` are read from ONE download made on
        first use after a step (it finishes the table's stream first); `check()` downloads the sticky status words.
        Every stream owns at most max_tracks (<= 4096) rows; the state is allocated once at S * max_tracks rows, the association workspace
        at 20 (24 with low_threshold / gates) bytes per (detection, row) pair: about 49 MB at S = 32, k = 300, max_tracks = 256.  Births
        beyond max_tracks are dropped (the first unmatched detections are born first, a dropped one takes no id) and `check()` reports it.
        Detections are tensors on the bank's device (host arrays are refused), k and E are fixed by the first step.
        The mode's one deviation: a stream whose costs are not finite cannot be redone on the host without reading; it is SKIPPED for that
        step — rows carried, nothing aged, no prediction, as if it had not been in `streams` — and `check()` raises for it later.
        Refused: use_kalman=True with kalman="host" (per-track host arithmetic is what the mode removes)."""
        if self._resident and use_kalman and kalman == "host":
            raise ValueError("lifecycle='device' with use_kalman=True, kalman='host': the host filter is per-track arithmetic on the host; "
                             "pass kalman='device'")
        if isinstance(num_streams, bool) or not isinstance(num_streams, (int, np.integer)) or num_streams < 1:
            raise ValueError(f"num_streams={num_streams!r}: expected an integer >= 1")
        if callable(reid_cost) or callable(box_cost) or reid_cost not in _REID_METRICS:
            raise ValueError(f"reid_cost={reid_cost!r} / box_cost={box_cost!r}: a TrackerBank keeps the cost matrices on the device; only "
                             f"{sorted(_REID_METRICS)} and 'iou' / 'giou' / None have gfx950 kernels (allow_host_cost does not apply: use one "
                             "Tracker per stream for host-side costs)")
        if box_cost not in _BOX_MODES:
            raise ValueError(f"box_cost={box_cost!r}: expected 'iou', 'giou' or None")
        self.num_streams = int(num_streams)
        self._off = np.zeros(self.num_streams + 1, np.int64)        # pooled device table: stream s owns rows _off[s] .. _off[s + 1]
        self._ctl = self._ws = self._redo_rec = None    # mapped live list + trk_off; device workspace; mapped record of a redone stream
        self._elig = None           # low_match="active": mapped eligibility bytes of the pooled table's rows (cnl_track_streams_low_f32)
        super().__init__(model, nms_kernel, num_detections, detection_threshold, reid_cost, reid_threshold, box_cost, box_threshold,
                         smoothing_factor, use_kalman, max_inactive_age, min_birth_age, device, kalman=kalman, low_threshold=low_threshold,
                         low_box_threshold=low_box_threshold, low_match=low_match, class_aware=class_aware, motion_gate=motion_gate,
                         motion_weight=motion_weight)

    def __len__(self):
        return self.num_streams

    def __getitem__(self, s):
        return _ResidentStream(self, range(self.num_streams)[s]) if self._resident else self._streams[s]

    def track_embeddings(self, s):
        """Device view [T_s, E] of stream s's rows of the pooled table (row order = self[s].tracks)."""
        if self._resident:
            off = self._download()["trk_off"] if self._res is not None else None
            return self._emb[int(off[s]):int(off[s + 1])] if off is not None else None
        return self._emb[int(self._off[s]):int(self._off[s + 1])] if self._emb is not None else None

    # ------------------------------------------------------------------ state
    def reset(self, stream=None):
        """Forget every stream (None) or one stream; the other streams keep tracks, counters and table rows.
        lifecycle="device": stream-ordered, no synchronisation (a zeroing of the state; for one stream, the step's launches with that stream
        marked)."""
        if self._resident:
            return self._reset_device(stream)
        if stream is None:
            self._streams = [_StreamState() for _ in range(self.num_streams)]
            self._table.clear()
            self._off[:] = 0
            self.last_matches = [None] * self.num_streams
            self.last_low_matches = [None] * self.num_streams      # low_threshold set: (original detection index, track row) pairs per stream
            return
        s = self._check_streams([stream])[0]
        self._streams[s] = _StreamState()
        self.last_matches[s] = self.last_low_matches[s] = None
        if self._off[s + 1] == self._off[s]:
            return
        # repack the pooled table without stream s's rows: the pooled apply launch with every kept row copied through (src_det = -1)
        table = self._table
        rows = np.concatenate([np.arange(self._off[t], self._off[t + 1]) for t in range(self.num_streams) if t != s] + [np.zeros(0, np.int64)])
        dev = self.device
        with _on(dev):
            table.wait_for_other_stream()             # its reads of the index lists come before this overwrite
            # (kalman="device": the filter state moves with the rows — no row is updated or predicted)
            args = (table.emb, table.box, table.emb.shape[1], self.smoothing_factor, torch.cuda.current_stream(dev))
            if self._device_kalman:
                table.apply_kalman(rows.astype(np.int32), np.full(len(rows), -1, np.int32), 0, *args)
            else:
                table.apply(rows.astype(np.int32), np.full(len(rows), -1, np.int32), *args)
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

    # ------------------------------------------------------------------ inference
    @torch.no_grad()
    def step_batch(self, images: torch.Tensor, streams=None, **kwargs):
        """Run the model on one frame from each participating stream (images[i] is the next frame of stream streams[i]; default: stream i)
        and advance those streams.  Returns {"bboxes": [...], "track_ids": [...]} with one list per image (active tracks only).
        (kalman="device": two stream synchronisations per step instead of one, see `update_batch`.)
        camera_motion (lifecycle="device" only): see `update_batch`; the boxes here are normalised, so a pixel shift is scaled first:
        `camera_motion=cm.update(frames)["shift"] * torch.tensor([1 / width, 1 / height], device=dev)`."""
        live = self._check_streams(streams)
        camera_motion = self._camera_motion(kwargs, len(live))
        if images.dim() != 4 or images.shape[0] != len(live):
            raise ValueError(f"images {tuple(images.shape)}: expected [{len(live)}, 3, H, W], one frame per participating stream")
        det = self._detect(images, kwargs)
        if self._resident:
            out = self._step_device(det["bboxes"], det["labels"], det["scores"], det["embeddings"], live, kwargs, camera_motion)
            for s in live:
                self._frames[s] += 1
            return out
        self._step(det["bboxes"], det["labels"], det["scores"], det["embeddings"], live, kwargs)
        out = {"bboxes": [], "track_ids": []}
        for s in live:
            self._streams[s].frame += 1
            _active(self._streams[s].tracks, out)
        return out

    # ------------------------------------------------------------------ one step
    def _host_association(self, i, s, d_box, d_score, d_emb, detection_threshold, reid_threshold, box_threshold, low_threshold=None,
                          low_box_threshold=None, gate_dets=None):
        """Stream s's association through the single-stream path (cnl_track_frame_f32 + scipy on the host) on its slice of the operands:
        what a stream with non-finite costs is redone with, so that the caller sees what Tracker raises (scipy: ValueError).  With
        low_threshold the low-score stage too (cnl_track_frame_low_f32): the three lists, then its matches.  With a gate on (gate_dets: the
        slot's (det_index, boxes, labels) as the life cycle reads them) the matrices go through the host's gate_costs before the assignment."""
        dev = self.device
        k, E = d_emb.shape[1], d_emb.shape[2]
        t0, T = int(self._off[s]), int(self._off[s + 1] - self._off[s])
        table = self._table
        low = low_threshold is not None
        rec = self._redo_rec = _grown(self._redo_rec, (frame_low_layout if low else frame_layout)(k, T, 0).bytes, 0)
        operands = (d_emb[i].data_ptr(), d_box[i].data_ptr(), d_score[i].data_ptr(), None, 0, k, E)
        table_args = (table.emb[t0:].data_ptr() if T else None, table.box[t0:].data_ptr() if T else None, T, _BOX_MODES[self.box_cost],
                      _REID_METRICS[self.reid_cost], 0)
        low_index = low_box = None
        with _on(dev):
            if low:
                *_, reid, box, low_index, low_box = launch_frame_low(_lib.load(), rec, *operands, detection_threshold, low_threshold, *table_args,
                                                                     torch.cuda.current_stream(dev))
            else:
                _, _, _, _, _, reid, box = launch_frame(_lib.load(), rec, *operands, detection_threshold, *table_args, torch.cuda.current_stream(dev))
            if self._gated and T:
                det_index, h_box, h_label = gate_dets
                motion = self.motion_gate is not None
                kx, kP = (table.kx[t0:t0 + T].cpu().numpy(), table.kP[t0:t0 + T].cpu().numpy()) if motion else (None, None)
                reid, box, low_box = gate_costs(reid, box, low_box, h_label, [t.label for t in self._streams[s].tracks] if self.class_aware else None,
                                                h_box, kx, kP, self.motion_gate, self.motion_weight, det_index, low_index)
        matches, unmatched_dets, unmatched_tracks = two_stage_assignment(reid, reid_threshold, box_threshold, box)
        if not low:
            return matches, unmatched_dets, unmatched_tracks
        low_matches, unmatched_tracks = low_stage(low_box, low_index, unmatched_tracks, self._eligible(self._streams[s].tracks), low_box_threshold)
        return matches, unmatched_dets, unmatched_tracks, low_matches

    def update_batch(self, bboxes, labels, scores, embeddings, streams=None, **kwargs):
        """One frame's detections for each participating stream: [L, k, 4], [L, k], [L, k], [L, k, E] (numpy arrays or torch tensors; L =
        len(streams), default every stream).  As `Tracker.update`, it does not advance `frame`.  With use_kalman=True, kalman="device" the
        step ends with a SECOND stream synchronisation, behind the filter launch (see `Tracker.update`); a stream that takes no part keeps
        its filter state unpredicted, as on the host path.
        lifecycle="device": returns the step's device tensors (see the constructor); None on the host path.
        camera_motion (lifecycle="device" only; None, the default, is the step without it, launch for launch): a float32 [L, 2] tensor on the
        bank's device, the global image shift (dx, dy) of each participating stream since its previous frame, in the units of `bboxes`
        (`CameraMotion.update(frames)["shift"]` for boxes in frame pixels).  One launch in front of the association (cnl_track_shift_f64) adds
        (dx, dy, dx, dy) to every position the stream's rows hold — the box table, the reported boxes and, with kalman="device", the positions
        of the filter state — so that IoU costs and the motion gate see the tracks where the camera moved them.  A non-finite shift skips its
        stream and `check()` reports it.  Every other mode raises ValueError: there the boxes live in host records."""
        live = self._check_streams(streams)
        camera_motion = self._camera_motion(kwargs, len(live))
        if self._resident:
            return self._step_device(bboxes, labels, scores, embeddings, live, kwargs, camera_motion)
        self._step(bboxes, labels, scores, embeddings, live, kwargs)

    def _camera_motion(self, kwargs, L):
        """Takes `camera_motion` out of a step's keywords -> the shift tensor or None, checked as far as the host can without a device."""
        if not self._resident:
            return self._refuse_camera_motion(kwargs, f"lifecycle={self.lifecycle!r}" + (", kalman='host'" if self.use_kalman and self.kalman == "host" else ""))
        shift = kwargs.pop("camera_motion", None)
        if shift is not None and not (isinstance(shift, torch.Tensor) and shift.dtype == torch.float32 and tuple(shift.shape) == (L, 2)):
            got = f"{shift.dtype} {tuple(shift.shape)}" if isinstance(shift, torch.Tensor) else type(shift).__name__
            raise ValueError(f"camera_motion: expected a float32 [{L}, 2] tensor (dx, dy per participating stream), got {got}")
        return shift

    def _step(self, bboxes, labels, scores, embeddings, live, kwargs):
        dev = self.device
        S, L = self.num_streams, len(live)
        d_box, d_score, d_emb, d_label, host, label_kind = normalise_detections(dev, bboxes, labels, scores, embeddings, (L,))
        detection_threshold, reid_threshold, box_threshold, low_threshold, low_box_threshold = self._thresholds(kwargs)
        low = low_threshold is not None
        gated = self._gated
        low_rec = low or gated          # the gated entry writes the `_low` record whether the stage runs or not
        lib = _lib.load()
        k, E = int(d_emb.shape[1]), int(d_emb.shape[2])
        with_dets = host is None
        table, off = self._table, self._off
        R = int(off[S])
        T_max = max(int(off[s + 1] - off[s]) for s in live)
        stride = (streams_low_layout if low_rec else streams_layout)(k, T_max, with_dets).bytes
        ws_need = (streams_low_workspace_bytes if low_rec else streams_workspace_bytes)(S, k, R)
        with _on(dev):
            cur = torch.cuda.current_stream(dev)
            table.wait_for_other_stream(cur)
            rec = self._rec = _grown(self._rec, S * stride, 1 << 16)
            if self._ws is None or self._ws.numel() < ws_need:
                self._ws = torch.empty(max(2 * ws_need, 1 << 20), device=dev, dtype=torch.uint8)
            if self._ctl is None:
                self._ctl = _Mapped(4 * (2 * S + 1))
            # live list and trk_off sit in mapped memory of their own: the association kernels that read them have finished at this step's
            # synchronisation, whereas the apply launch still reads ITS lists after the host has moved on (TrackTable.apply)
            ctl = self._ctl.np.view(np.int32)
            ctl[:L] = live
            ctl[S:2 * S + 1] = off
            if self.class_aware and not label_kind:             # host arrays: the class gate reads the labels on the device
                d_label, label_kind = torch.from_numpy(np.ascontiguousarray(host[1]).astype(np.int64)).to(dev), 1
            operands = (d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr() if label_kind else None, label_kind, S, L,
                        self._ctl.ptr, k, E, float(detection_threshold), float(reid_threshold), float(box_threshold))
            tables = (table.emb.data_ptr() if R else None, table.box.data_ptr() if R else None, self._ctl.ptr + 4 * S)
            rest = (R, T_max, _BOX_MODES[self.box_cost], _REID_METRICS[self.reid_cost], int(with_dets), self._ws.data_ptr(), self._ws.numel(), rec.ptr,
                    stride, ctypes.c_void_p(cur.cuda_stream))
            if low_rec:
                eligible = None
                if low and self.low_match != "all" and R:
                    # the rows' eligibility sits in mapped memory the assign kernel reads (the rows of this step's streams only): finished
                    # with at this step's synchronisation
                    self._elig = _grown(self._elig, R, 1 << 12)
                    for s in live:
                        flags = bytes([t.state is TrackState.ACTIVE for t in self._streams[s].tracks])
                        self._elig.np[off[s]:off[s] + len(flags)] = np.frombuffer(flags, np.uint8)
                    eligible = self._elig.ptr
                if gated:       # one entry with and without the low-score stage: none = an empty score window
                    gate = self._gate([(int(off[s]), self._streams[s].tracks) for s in live], R, table.kx, table.kP)
                    _lib.check(lib.cnl_track_streams_gated_f32(*operands, float(low_threshold if low else detection_threshold), float(low_box_threshold),
                                                               *tables, eligible, *rest[:-1], ctypes.byref(gate), rest[-1]),
                               "cnl_track_streams_gated_f32")
                else:
                    _lib.check(lib.cnl_track_streams_low_f32(*operands, float(low_threshold), float(low_box_threshold), *tables, eligible, *rest),
                               "cnl_track_streams_low_f32")
            else:
                _lib.check(lib.cnl_track_streams_f32(*operands, *tables, *rest), "cnl_track_streams_f32")
            cur.synchronize()
        # ---- read every stream's lists first: an exception leaves all streams untouched ----
        assoc, d2h = {}, 0
        for i, s in enumerate(live):
            n, T, status, det_index, h_box, _, h_label, *lists = (read_stream_low_record if low_rec else read_stream_record)(rec.np[s * stride:(s + 1) * stride])
            if status in _STATUS_TOO_LARGE:
                raise ValueError(f"stream {s}: association status {status} (k = {k}, T = {T}: beyond the supported sizes)")
            d2h += 64 + 4 * n + (24 * k if with_dets else 0) + 8 * len(lists[0]) + 4 * len(lists[1]) + 4 * len(lists[2])
            if low_rec:
                n_low = lists.pop(3)
                d2h += 32 + 4 * n_low + 8 * len(lists[3])
                if not low:
                    lists = lists[:3]
            if not with_dets:
                h_box, h_label = host[0][i], host[1][i]
                check_kept_count(host[2][i], detection_threshold, n, f"stream {s}: ")
            if status:
                lists = self._host_association(i, s, d_box, d_score, d_emb, detection_threshold, reid_threshold, box_threshold, low_threshold,
                                               low_box_threshold, (det_index, h_box, h_label))
            assoc[s] = (i * k, *lists[:3], det_index, h_box, h_label, *lists[3:])
        self.d2h_bytes = d2h

        # ---- track life cycle per stream (host) + the rows of the new pooled table ----
        keep_emb = [] if low else None              # low: per row of the new pooled table, 1 = a low-score match (the embedding is carried over)
        src_trk, src_det, predict = [], [], []      # predict: (flag, rows) per stream for cnl_track_kalman_f64 — only the streams of this step predict
        for s, st in enumerate(self._streams):
            base = int(off[s])
            if s not in assoc:              # took no part in this step: its rows are copied through
                src_trk.extend(range(base, base + len(st.tracks)))
                src_det.extend([-1] * len(st.tracks))
                predict.append((0, len(st.tracks)))
                if low:
                    keep_emb.extend([0] * len(st.tracks))
                continue
            det_base, matches, *rest = assoc[s]
            self.last_matches[s] = matches
            if low:
                self.last_low_matches[s] = rest[5]
                st.tracks, st.next_track_id, old_rows, det_rows, kept = life_cycle(st.tracks, matches, *rest[:5], st.next_track_id, self, rest[5])
                keep_emb.extend(kept)
            else:
                self.last_low_matches[s] = None
                st.tracks, st.next_track_id, old_rows, det_rows = life_cycle(st.tracks, matches, *rest, st.next_track_id, self)
            src_trk.extend(base + r if r >= 0 else -1 for r in old_rows)
            src_det.extend(det_base + d if d >= 0 else -1 for d in det_rows)
            predict.append((1, len(old_rows)))
        if self._device_kalman:
            flags = np.repeat(np.array([p for p, _ in predict], np.int32), [n for _, n in predict])
            with _on(dev):
                self._apply_with_kalman([t for st in self._streams for t in st.tracks], src_trk, src_det, flags, d_emb, d_box, E, cur, keep_emb)
            self.d2h_bytes += 36 * len(src_trk)
            self._set_offsets()
            return
        with _on(dev):
            table.apply(src_trk, src_det, d_emb, d_box, E, self.smoothing_factor, cur, keep_emb)
        self._set_offsets()
        if self.use_kalman and off[S]:
            # the boxes of all streams go up in ONE copy; only the streams of this step predict
            table.upload_boxes([t for st in self._streams for t in st.tracks])
            for s in live:
                for t in self._streams[s].tracks:
                    t.kalman_predict()


    # ------------------------------------------------------------------ lifecycle="device"
    def _reset_device(self, stream):
        S = self.num_streams
        res = self._res
        self._snap = None
        if stream is None:
            self._frames = [0] * S
            self._has_rec = [False] * S
            self.last_matches, self.last_low_matches = _ResidentLists(self, False), _ResidentLists(self, True)
            if res is not None:
                with _on(res.dev):
                    cur = torch.cuda.current_stream(res.dev)
                    self._table.wait_for_other_stream(cur)
                    res.ctl[:res.down_bytes].zero_()        # offsets, counters, states, status words, records: behind the last step, in stream order
                    self._table.stream = cur
            return
        s = self._check_streams([stream])[0]
        self._frames[s] = 0
        self._has_rec[s] = False
        if res is None:
            return
        with _on(res.dev):
            cur = torch.cuda.current_stream(res.dev)
            self._table.wait_for_other_stream(cur)
            # the step's launches without a slot: stream s loses its rows and its counter, every other row is carried (no update, no prediction)
            self._lifecycle_launches(res, res.live_list(()), 0, res.emb[res.cur], res.box[res.cur], None, 0, None, cur, reset_stream=s)

    def _lifecycle_launches(self, res, lv, L, d_emb, d_box, d_label, label_kind, outs, cur, reset_stream=-1):
        """Life cycle + pack, table update, filter, emit on `cur`, then the banks and tables change places.  lv: ResidentState.live_list;
        outs: the step's four output tensors (None with L == 0).  The caller holds the device guard."""
        lib = _lib.load()
        b, C = res.cur, res.C
        stream = ctypes.c_void_p(cur.cuda_stream)
        a = res.args[b]
        a.live, a.slot_of, a.S_live = lv.data_ptr(), lv.data_ptr() + 4 * L, L
        a.det_label, a.label_kind, a.det_box = (d_label.data_ptr() if label_kind else None), label_kind, d_box.data_ptr()
        a.min_birth_age, a.max_inactive_age, a.step = int(self.min_birth_age), int(self.max_inactive_age), self._step_no & 0x7fffffff
        a.reset_stream = reset_stream
        a.out_box, a.out_track_id, a.out_label, a.out_count = (t.data_ptr() for t in outs) if outs is not None else (None,) * 4
        _lib.check(lib.cnl_track_lifecycle_i32(ctypes.byref(a), stream), "cnl_track_lifecycle_i32")
        new_emb, new_box = res.emb[1 - b], res.box[1 - b]
        _lib.check(lib.cnl_track_apply_keep_f32(res.emb[b].data_ptr(), res.box[b].data_ptr(), d_emb.data_ptr(), d_box.data_ptr(), res.ptr("src_trk"),
                                                res.ptr("src_det"), C, res.E, float(self.smoothing_factor), new_emb.data_ptr(), new_box.data_ptr(),
                                                res.ptr("keep_emb"), stream), "cnl_track_apply_keep_f32")
        if res.kalman:
            _lib.check(lib.cnl_track_kalman_f64(res.kx[b].data_ptr(), res.kP[b].data_ptr(), d_box.data_ptr(), res.ptr("src_trk"), res.ptr("src_det"),
                                                res.ptr("flags"), C, res.kx[1 - b].data_ptr(), res.kP[1 - b].data_ptr(), new_box.data_ptr(),
                                                res.ptr("kalman_box"), res.ptr("kalman_status"), stream), "cnl_track_kalman_f64")
        _lib.check(lib.cnl_track_lifecycle_emit_f64(ctypes.byref(a), stream), "cnl_track_lifecycle_emit_f64")
        res.cur = 1 - b
        table = self._table
        table.emb, table.box, table.stream = new_emb, new_box, cur
        if res.kalman:
            table.kx, table.kP = res.kx[1 - b], res.kP[1 - b]
        self._snap = None
        self._step_no += 1

    def _step_device(self, bboxes, labels, scores, embeddings, live, kwargs, camera_motion=None):
        S, L, M = self.num_streams, len(live), self.max_tracks
        for name, t in (("bboxes", bboxes), ("labels", labels), ("scores", scores), ("embeddings", embeddings)) + \
                ((("camera_motion", camera_motion),) if camera_motion is not None else ()):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.device == self.device):
                raise ValueError(f"lifecycle='device': {name} must be a tensor on the bank's device, got {type(t).__name__}"
                                 f"{' on ' + str(t.device) if isinstance(t, torch.Tensor) else ''} (host arrays are refused: the mode exists to "
                                 "stay on the device)")
        dev = self.device
        d_box, d_score, d_emb, d_label, _, label_kind = normalise_detections(dev, bboxes, labels, scores, embeddings, (L,))
        detection_threshold, reid_threshold, box_threshold, low_threshold, low_box_threshold = self._thresholds(kwargs)
        low = low_threshold is not None
        gated = self._gated
        low_rec = low or gated
        k, E = int(d_emb.shape[1]), int(d_emb.shape[2])
        lib = _lib.load()
        table = self._table
        with _on(dev):
            cur = torch.cuda.current_stream(dev)
            table.wait_for_other_stream(cur)
            res = self._res
            if res is None:
                res = self._res = ResidentState(S, M, k, E, dev, self._device_kalman, low_rec)
            if (k, E) != (res.k, res.E):
                raise ValueError(f"lifecycle='device': detections [{L}, {k}, {E}] after [.., {res.k}, {res.E}]: the buffers are sized by the first "
                                 "step (keep num_detections and the embedding size fixed)")
            if low_rec != res.low_rec:
                raise ValueError("lifecycle='device': low_threshold cannot be switched on or off per call (the records are laid out by the first step)")
            lv = res.live_list(tuple(live))
            b, C = res.cur, res.C
            if camera_motion is not None:       # the tracks go where the camera moved them, in front of the association that reads them
                shift = camera_motion.contiguous()
                _lib.check(lib.cnl_track_shift_f64(res.box[b].data_ptr(), res.ptr("box", b), res.kx[b].data_ptr() if res.kalman else None,
                                                   res.ptr("trk_off", b), lv.data_ptr(), shift.data_ptr(), res.ptr("status"), S, L, M,
                                                   self._step_no & 0x7fffffff, ctypes.c_void_p(cur.cuda_stream)), "cnl_track_shift_f64")
            operands = (d_emb.data_ptr(), d_box.data_ptr(), d_score.data_ptr(), d_label.data_ptr() if label_kind else None, label_kind, S, L,
                        lv.data_ptr(), k, E, float(detection_threshold), float(reid_threshold), float(box_threshold))
            tables = (res.emb[b].data_ptr(), res.box[b].data_ptr(), res.ptr("trk_off", b))
            rest = (C, M, _BOX_MODES[self.box_cost], _REID_METRICS[self.reid_cost], 0, res.ws.data_ptr(), res.ws.numel(), res.ptr("record"), res.stride,
                    ctypes.c_void_p(cur.cuda_stream))
            if low_rec:
                eligible = res.ptr("trk_eligible") if low and self.low_match != "all" else None
                if gated:
                    gate = _lib.TrackGate(res.ptr("label", b) if self.class_aware else None, None, None, 0.0, 1.0)
                    if self.motion_gate is not None:
                        gate.kx, gate.kP, gate.motion_gate, gate.motion_weight = res.kx[b].data_ptr(), res.kP[b].data_ptr(), self.motion_gate, self.motion_weight
                    _lib.check(lib.cnl_track_streams_gated_f32(*operands, float(low_threshold if low else detection_threshold), float(low_box_threshold),
                                                               *tables, eligible, *rest[:-1], ctypes.byref(gate), rest[-1]),
                               "cnl_track_streams_gated_f32")
                else:
                    _lib.check(lib.cnl_track_streams_low_f32(*operands, float(low_threshold), float(low_box_threshold), *tables, eligible, *rest),
                               "cnl_track_streams_low_f32")
            else:
                _lib.check(lib.cnl_track_streams_f32(*operands, *tables, *rest), "cnl_track_streams_f32")
            outs = (torch.empty((L, M, 4), device=dev, dtype=torch.float64 if res.kalman else torch.float32),
                    torch.empty((L, M), device=dev, dtype=torch.int64), torch.empty((L, M), device=dev, dtype=torch.int64),
                    torch.empty((L,), device=dev, dtype=torch.int32))
            self._lifecycle_launches(res, lv, L, d_emb, d_box, d_label, label_kind, outs, cur)
        for s in live:
            self._has_rec[s] = True
        self.d2h_bytes = 0
        return {"bboxes": outs[0], "track_ids": outs[1], "labels": outs[2], "count": outs[3]}

    def _download(self):
        """The last download (ResidentState.download), made now if a step or reset came after it: finishes the table's stream first when the
        caller is on another one (TrackTable's stream rule)."""
        if self._snap is None:
            res = self._res
            if res is None:
                S = self.num_streams
                return {"trk_off": np.zeros(S + 1, np.int32), "next_track_id": np.zeros(S, np.int64), "status": np.zeros((S, 2), np.int32)}
            with _on(res.dev):
                self._table.wait_for_other_stream(torch.cuda.current_stream(res.dev))
                self._snap = res.download()
        return self._snap

    def _resident_tracks(self, s):
        d = self._download()
        if self._res is None:
            return []
        kal = self._res.kalman
        out = []
        for r in range(int(d["trk_off"][s]), int(d["trk_off"][s + 1])):
            bbox = d["bbox"][r].copy() if kal else d["bbox"][r].astype(np.float32)
            out.append(ResidentTrack(int(d["track_id"][r]), bbox, int(d["label"][r]), _STATES[int(d["state"][r])], int(d["birth_age"][r]),
                                     int(d["inactive_age"][r]), d["emb"][r].copy(),
                                     ResidentKalman(d["kx"][r].copy(), d["kP"][r].reshape(8, 8).copy()) if kal else None))
        return out

    def _resident_matches(self, s, low):
        if not self._has_rec[s] or (low and self.low_threshold is None):
            return None
        rec = self._download()["records"][s]
        if not self._res.low_rec:
            return read_stream_record(rec)[7]
        out = read_stream_low_record(rec)
        return out[-1] if low else out[7]

    def snapshot(self, streams=None):
        """lifecycle="device": the state of the given streams (default: all) as numpy arrays from ONE download: "offsets" int64 [n + 1] (the
        rows of streams[i] are offsets[i] .. offsets[i + 1] of the arrays below), "track_ids" int64, "states" (TrackState values) / "birth_age"
        / "inactive_age" int32, "labels" int64, "bboxes" (the reported boxes: float32, float64 with the filter) [R, 4], "embeddings" float32
        [R, E], "table_boxes" float32 [R, 4], with the filter "kx" [R, 8] / "kP" [R, 64] float64, and "next_track_id" int64 [n]."""
        if not self._resident:
            raise ValueError("snapshot() reads the device state of lifecycle='device'; with lifecycle='host' the tracks are bank[s].tracks")
        live = self._check_streams(streams)
        d = self._download()
        off = d["trk_off"]
        rows = np.concatenate([np.arange(off[s], off[s + 1], dtype=np.int64) for s in live] + [np.zeros(0, np.int64)])
        out = {"offsets": np.concatenate([[0], np.cumsum([int(off[s + 1] - off[s]) for s in live])]).astype(np.int64),
               "next_track_id": d["next_track_id"][live].copy()}
        if self._res is None:
            return out
        kal = self._res.kalman
        out.update(track_ids=d["track_id"][rows], states=d["state"][rows], birth_age=d["birth_age"][rows], inactive_age=d["inactive_age"][rows],
                   labels=d["label"][rows].astype(np.int64), bboxes=d["bbox"][rows] if kal else d["bbox"][rows].astype(np.float32),
                   embeddings=d["emb"][rows], table_boxes=d["box"][rows])
        if kal:
            out.update(kx=d["kx"][rows], kP=d["kP"][rows])
        return out

    def check(self):
        """lifecycle="device": download the streams' sticky status words; if any is set, clear them all and raise ValueError naming each
        stream, its code (the association status of its first skipped step; "overflow": births were dropped at max_tracks; a non-finite camera_motion shift that was skipped) and the step
        counter of its first event."""
        if not self._resident or self._res is None:
            return
        res = self._res
        with _on(res.dev):
            cur = torch.cuda.current_stream(res.dev)
            self._table.wait_for_other_stream(cur)
            o = res.off["status"]
            words = res.ctl[o:o + 8 * self.num_streams]
            status = words.cpu().numpy().view(np.int32).reshape(-1, 2)
            if not status[:, 0].any():
                return
            words.zero_()
            self._table.stream = cur
            self._snap = None
        said = []
        for s in np.flatnonzero(status[:, 0]).tolist():
            code, step = int(status[s, 0]), int(status[s, 1])
            what = [f"association status {code & 0xffff} (skipped)"] if code & 0xffff else []
            what += ["overflow (births dropped at max_tracks)"] if code & STATUS_OVERFLOW else []
            what += ["a non-finite camera_motion shift (skipped)"] if code & STATUS_BAD_SHIFT else []
            said.append(f"stream {s}: {' and '.join(what)}, first at step {step}")
        raise ValueError("TrackerBank(lifecycle='device'): " + "; ".join(said))


def build_tracker(config, model=None, num_streams=None):
    """tracker.py:349-353; with `num_streams`, a TrackerBank of that many streams with the same settings."""
    if isinstance(config, str):
        config = load_config(config)["tracker"]
    if num_streams is not None:
        return TrackerBank(num_streams, model=model, **config)
    config = dict(config)
    if config.pop("lifecycle", "host") != "host":
        raise ValueError("lifecycle='device' is a TrackerBank mode (pass num_streams): one stream on one wave loses to a CPU core")
    config.pop("max_tracks", None)
    return Tracker(model=model, **config)
