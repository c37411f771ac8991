"""Host side of the tracking association that `Tracker` and `TrackerBank` (tracker.py) share: layouts and readers of the records the
association kernels write, the single-stream launch, the two-stage assignment, the track life cycle, the device track table, the settings
and the input normaliser — each once."""
import contextlib
import ctypes
import warnings
import weakref
from collections import namedtuple
from enum import Enum, auto

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from . import _lib

_BOX_MODES = {None: 0, "iou": 1, "giou": 2}
_LABEL_KINDS = {torch.int64: 1, torch.int32: 2, torch.float32: 3}     # det_label element types cnl_track_frame_f32 reads
_REID_METRICS = {"cosine": 0, "euclidean": 1, "sqeuclidean": 2, "cityblock": 3, "chebyshev": 4, "canberra": 5, "braycurtis": 6, "correlation": 7}
# ^ the scipy cdist metrics with a gfx950 kernel (float64, scipy's operation order); "manhattan" etc. are scipy aliases -> host path

_NO_GUARD = contextlib.nullcontext()


def _on(dev):
    """Device guard for the launches — skipped when `dev` is the current device already (torch.cuda.device() costs ~6 us per use,
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


def _grown(buf, need, floor):
    """`buf` if it holds `need` bytes, else a new block of twice that (at least `floor`): persistent, nothing allocated per frame."""
    return buf if buf is not None and buf.nbytes >= need else _Mapped(max(2 * need, floor))


# ---------------------------------------------------------------------------------------------------------------- record layouts
# The size helpers of the library (cnl_track_frame_bytes, cnl_track_streams_record_bytes / _workspace_bytes) restated in Python: a ctypes
# call costs ~2 us of a 150 us frame.  tests/test_track_host.py holds them to the C helpers.
FrameLayout = namedtuple("FrameLayout", "off_index off_dets off_reid bytes")
StreamsLayout = namedtuple("StreamsLayout", "off_index off_dets off_match off_udet off_utrk bytes")
# int32 header words of the frame record (csrc/track.hip: frame_kernel) ...
F_N, F_K, F_T, F_WITH_DETS, F_OFF_INDEX, F_OFF_DETS, F_OFF_REID, F_OFF_BOX = range(8)
# ... and of one stream's record (csrc/track_streams.hip: streams_costs_kernel, streams_assign_kernel); M1 = matches of stage 1 alone
(S_N, S_K, S_T, S_STATUS, S_OFF_INDEX, S_OFF_DETS, S_OFF_MATCH, S_OFF_UDET, S_OFF_UTRK, S_M, S_M1, S_NUDET, S_NUTRK, S_WITH_DETS, S_SLOT,
 S_STREAM) = range(16)
_STATUS_TOO_LARGE = (3, 4, 19, 35)      # status words of a stream whose k / T lie beyond the supported sizes
# The BYTE stage's additions (low_threshold set): the frame record's header grows to int32[12], a stream's to int32[24]
FrameLowLayout = FrameLayout
StreamsLowLayout = namedtuple("StreamsLowLayout", "off_index off_dets off_match off_udet off_utrk off_low_index off_low_match bytes")
F_NLOW, F_OFF_LOW_INDEX, F_OFF_LOW_BOX = 8, 9, 10
S_NLOW, S_NLOW_MATCH, S_OFF_LOW_INDEX, S_OFF_LOW_MATCH = 16, 17, 18, 19
_LOW_MATCH = ("active", "all")
# The gates (class_aware / motion_gate): a gated pair's cost, CNL_TRACK_GATE_COST of the header, and motion_gate=True's threshold (the 0.95
# quantile of chi-square with 4 degrees of freedom, DeepSORT's chi2inv95[4])
GATE_COST = 1e5
CHI2INV95_4 = 9.4877


def frame_layout(k, T, with_dets):
    """[header 32 B | det_index[k] | (boxes[k][4] scores[k] labels[k]) | reid f64 n*T | box f32 n*T]; `bytes` is the worst case n = k (the
    box matrix follows the re-ID matrix of the n the kernel found: header word F_OFF_BOX)."""
    off_dets = (32 + 4 * k + 7) & ~7
    off_reid = (off_dets + (24 * k if with_dets else 0) + 7) & ~7
    return FrameLayout(32, off_dets, off_reid, off_reid + 12 * k * T)


def streams_layout(k, T_max, with_dets):
    """One stream's record: [header 64 B | det_index[k] | (boxes scores labels) | matches[k][2] | unmatched dets[k] | unmatched tracks[T_max]];
    `bytes` is the stride between the streams' records."""
    off_dets = (64 + 4 * k + 7) & ~7
    off_match = off_dets + (24 * k if with_dets else 0)
    off_utrk = off_match + 12 * k
    return StreamsLayout(64, off_dets, off_match, off_match + 8 * k, off_utrk, (off_utrk + 4 * T_max + 7) & ~7)


def streams_workspace_bytes(S, k, R):
    """Device workspace of one step over S streams whose pooled table has R rows: 20 B per (detection, row) pair + the index lists."""
    return 20 * k * R + 4 * (S + 2 * S * k + 2 * R)


def frame_low_layout(k, T, with_dets):
    """cnl_track_frame_low_bytes: [header 48 B | det_index[k] | (boxes scores labels) | reid f64 n*T | box f32 n*T | low_index[k] | low_box f32
    n_low*T]; the kept and the low detections are disjoint (n + n_low <= k), so 12 k T bounds the three matrices."""
    off_dets = (48 + 4 * k + 7) & ~7
    off_reid = (off_dets + (24 * k if with_dets else 0) + 7) & ~7
    return FrameLowLayout(48, off_dets, off_reid, off_reid + 12 * k * T + 4 * k)


def streams_low_layout(k, T_max, with_dets):
    """cnl_track_streams_low_record_bytes: streams_layout behind a 96-byte header, then low_index[k] | low_matches[k][2]."""
    off_dets = (96 + 4 * k + 7) & ~7
    off_match = off_dets + (24 * k if with_dets else 0)
    off_utrk = off_match + 12 * k
    off_low_index = off_utrk + 4 * T_max
    return StreamsLowLayout(96, off_dets, off_match, off_match + 8 * k, off_utrk, off_low_index, off_low_index + 4 * k,
                            (off_low_index + 12 * k + 7) & ~7)


def streams_low_workspace_bytes(S, k, R):
    """streams_workspace_bytes + the low detections' box costs (4 B per pair) and their count per stream."""
    return streams_workspace_bytes(S, k, R) + 4 * k * R + 4 * S


def _read_dets(r, off, k):
    """(boxes f32 [k,4], scores f32 [k], labels i64 [k]) at byte `off` of a record.  Boxes and labels are copies: a Track keeps its box,
    and the record is overwritten by the next frame; nothing keeps the scores (a view)."""
    f = r[off:off + 20 * k].view(np.float32)
    return f[:4 * k].reshape(k, 4).copy(), f[4 * k:], r[off + 20 * k:off + 24 * k].view(np.int32).astype(np.int64)


def read_frame_record(h, with_box):
    """uint8 view of a frame record -> (n, det_index, boxes, scores, labels, reid f64 [n,T], box f32 [n,T] | None).  boxes / scores / labels
    are None when the record carries no detections; the matrices are views (valid until the next launch into the record)."""
    hdr = h[:32].view(np.int32).tolist()
    n, k, T = hdr[F_N], hdr[F_K], hdr[F_T]
    dets = _read_dets(h, hdr[F_OFF_DETS], k) if hdr[F_WITH_DETS] else (None, None, None)
    off_index, off_reid, off_box = hdr[F_OFF_INDEX], hdr[F_OFF_REID], hdr[F_OFF_BOX]
    reid = h[off_reid:off_reid + 8 * n * T].view(np.float64).reshape(n, T)
    box = h[off_box:off_box + 4 * n * T].view(np.float32).reshape(n, T) if with_box else None
    return (n, h[off_index:off_index + 4 * n].view(np.int32).copy(), *dets, reid, box)


def read_stream_record(r):
    """uint8 view of one stream's record -> (n, T, status, det_index, boxes, scores, labels, matches, unmatched_dets, unmatched_tracks):
    the three lists as `match_with_threshold` twice yields them (empty when status != 0: the device did not assign)."""
    hdr = r[:64].view(np.int32).tolist()
    n, k, m = hdr[S_N], hdr[S_K], hdr[S_M]
    dets = _read_dets(r, hdr[S_OFF_DETS], k) if hdr[S_WITH_DETS] else (None, None, None)
    off_index, off_match, off_udet, off_utrk = hdr[S_OFF_INDEX], hdr[S_OFF_MATCH], hdr[S_OFF_UDET], hdr[S_OFF_UTRK]
    matches = [tuple(p) for p in r[off_match:off_match + 8 * m].view(np.int32).reshape(m, 2).tolist()]
    return (n, hdr[S_T], hdr[S_STATUS], r[off_index:off_index + 4 * n].view(np.int32).copy(), *dets, matches,
            r[off_udet:off_udet + 4 * hdr[S_NUDET]].view(np.int32).tolist(), r[off_utrk:off_utrk + 4 * hdr[S_NUTRK]].view(np.int32).tolist())


def read_frame_low_record(h):
    """uint8 view of a cnl_track_frame_low_f32 record -> read_frame_record's tuple + (low_index int32 [n_low] copy, low_box f32 [n_low, T] view)."""
    hdr = h[:48].view(np.int32).tolist()
    n_low, T, off_li, off_lb = hdr[F_NLOW], hdr[F_T], hdr[F_OFF_LOW_INDEX], hdr[F_OFF_LOW_BOX]
    return (*read_frame_record(h, True), h[off_li:off_li + 4 * n_low].view(np.int32).copy(),
            h[off_lb:off_lb + 4 * n_low * T].view(np.float32).reshape(n_low, T))


def read_stream_low_record(r):
    """uint8 view of one stream's cnl_track_streams_low_f32 record -> read_stream_record's tuple (its unmatched tracks: after all three
    stages) + (n_low, low_matches as (ORIGINAL detection index, track), in low-row order)."""
    hdr = r[64:96].view(np.int32).tolist()
    n_low, m, off_li, off_lm = hdr[S_NLOW - 16], hdr[S_NLOW_MATCH - 16], hdr[S_OFF_LOW_INDEX - 16], hdr[S_OFF_LOW_MATCH - 16]
    low_index = r[off_li:off_li + 4 * n_low].view(np.int32)
    pairs = r[off_lm:off_lm + 8 * m].view(np.int32).reshape(m, 2).tolist()
    return (*read_stream_record(r), n_low, [(int(low_index[x]), t) for x, t in pairs])


def launch_frame_low(lib, rec, d_emb, d_box, d_score, d_label, label_kind, k, E, detection_threshold, low_threshold, t_emb, t_box, T, box_mode,
                     reid_metric, with_dets, cur):
    """launch_frame with the BYTE stage's sections (cnl_track_frame_low_f32) -> read_frame_low_record's tuple."""
    _lib.check(lib.cnl_track_frame_low_f32(d_emb, d_box, d_score, d_label, label_kind, k, E, float(detection_threshold), float(low_threshold), t_emb,
                                           t_box, T, box_mode, reid_metric, int(with_dets), rec.ptr, rec.nbytes, ctypes.c_void_p(cur.cuda_stream)),
               "cnl_track_frame_low_f32")
    cur.synchronize()
    return read_frame_low_record(rec.np)


def launch_frame_gated(lib, rec, d_emb, d_box, d_score, d_label, label_kind, k, E, detection_threshold, low_threshold, t_emb, t_box, T, box_mode,
                       reid_metric, with_dets, gate, cur):
    """launch_frame_low through cnl_track_frame_gated_f32 (`gate`: a _lib.TrackGate; low_threshold == detection_threshold: no low-score stage,
    and then box_mode may be 0) -> read_frame_low_record's tuple, the box matrix None without a box cost."""
    _lib.check(lib.cnl_track_frame_gated_f32(d_emb, d_box, d_score, d_label, label_kind, k, E, float(detection_threshold), float(low_threshold), t_emb,
                                             t_box, T, box_mode, reid_metric, int(with_dets), rec.ptr, rec.nbytes, ctypes.byref(gate),
                                             ctypes.c_void_p(cur.cuda_stream)), "cnl_track_frame_gated_f32")
    cur.synchronize()
    out = read_frame_low_record(rec.np)
    return out if box_mode else (*out[:6], None, *out[7:])


def _seq_sum(terms):
    acc = terms[0]
    for t in terms[1:]:
        acc = acc + t
    return acc


def mahalanobis_sq(det_boxes, kx, kP):
    """The motion gate's squared Mahalanobis distance (include/centernet_gfx950.h: cnl_track_gate) of every (detection box, track) pair in the
    header's operation order, float64, one numpy operation = one IEEE operation per pair: det_boxes float32 [n, 4], kx [T, 8], kP [T, 64]
    -> (m float64 [n, T], ok bool [T]: every pivot of the track's S = P[:4, :4] + diag(r) = L D L' finite and strictly positive)."""
    z = np.asarray(det_boxes, np.float32).reshape(-1, 4).astype(np.float64)
    x = np.asarray(kx, np.float64).reshape(-1, 8)
    P = np.asarray(kP, np.float64).reshape(-1, 8, 8)
    with np.errstate(all="ignore"):
        wh = (x[:, 2] - x[:, 0], x[:, 3] - x[:, 1])
        r = []
        for i in range(4):
            q = wh[i & 1] / 20.0
            r.append(q * q)
        c = [[None] * 4 for _ in range(4)]
        L = [[None] * 4 for _ in range(4)]
        d = [None] * 4
        ok = np.ones(x.shape[0], bool)
        for j in range(4):
            for i in range(j, 4):
                v = P[:, i, i] + r[i] if i == j else P[:, j, i]      # the upper triangle, as the filter reads P
                if j > 0:
                    v = v - _seq_sum([c[i][k] * L[j][k] for k in range(j)])
                c[i][j] = v
            d[j] = c[j][j]
            ok &= np.isfinite(d[j]) & (d[j] > 0.0)
            for i in range(j + 1, 4):
                L[i][j] = c[i][j] / d[j]
        u = [None] * 4
        for i in range(4):
            v = z[:, i, None] - x[None, :, i]
            if i > 0:
                v = v - _seq_sum([L[i][k][None, :] * u[k] for k in range(i)])
            u[i] = v
        m = _seq_sum([(u[i] / d[i][None, :]) * u[i] for i in range(4)])
    return m, ok


def gate_costs(reid, box, low_box, det_labels, trk_labels, det_boxes, kx, kP, motion_gate, motion_weight, det_index=None, low_index=None):
    """The gates of cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32 applied on the host to ungated matrices (what a redone stream of a
    TrackerBank goes through): reid float64 [n, T], box float32 [n, T] | None, low_box float32 [n_low, T] | None; det_labels / det_boxes: the
    frame's [k] / [k, 4] arrays, det_index / low_index the rows' original detections (None: rows 0, 1, ...).  trk_labels None: no class gate;
    kx / kP None or motion_gate None: no motion gate.  -> gated copies (reid, box, low_box)."""
    reid = np.array(reid, np.float64)
    n, T = reid.shape
    box = None if box is None else np.array(box, np.float32)
    low_box = None if low_box is None else np.array(low_box, np.float32)
    det_index = np.arange(n) if det_index is None else np.asarray(det_index, np.int64)
    cross = np.zeros((n, T), bool)
    if trk_labels is not None:
        lab = np.asarray(det_labels).astype(np.int64).astype(np.int32)
        trk = np.asarray(trk_labels).astype(np.int64).astype(np.int32)
        cross = lab[det_index][:, None] != trk[None, :T]
        if low_box is not None:
            low_index = np.arange(low_box.shape[0]) if low_index is None else np.asarray(low_index, np.int64)
            low_box[lab[low_index][:, None] != trk[None, :T]] = np.float32(GATE_COST)
    if motion_gate is not None and kx is not None and n and T:
        m, ok = mahalanobis_sq(np.asarray(det_boxes, np.float32).reshape(-1, 4)[det_index], np.asarray(kx)[:T], np.asarray(kP)[:T])
        with np.errstate(all="ignore"):
            inside = ok[None, :] & (m <= motion_gate)
            if motion_weight != 1.0:
                reid = motion_weight * reid + (1.0 - motion_weight) * m
        reid[~inside] = GATE_COST
    reid[cross] = GATE_COST
    if box is not None:
        box[cross] = np.float32(GATE_COST)
    return reid, box, low_box


def launch_frame(lib, rec, d_emb, d_box, d_score, d_label, label_kind, k, E, detection_threshold, t_emb, t_box, T, box_mode, reid_metric,
                 with_dets, cur):
    """ONE launch (operands as device addresses, None = absent) writes the frame record straight into the mapped host memory `rec`, packed by
    the n the kernel finds; ONE synchronisation makes it readable: the frame's only device -> host traffic.  -> read_frame_record's tuple."""
    _lib.check(lib.cnl_track_frame_f32(d_emb, d_box, d_score, d_label, label_kind, k, E, float(detection_threshold), t_emb, t_box, T, box_mode,
                                       reid_metric, int(with_dets), rec.ptr, rec.nbytes, ctypes.c_void_p(cur.cuda_stream)), "cnl_track_frame_f32")
    cur.synchronize()
    return read_frame_record(rec.np, box_mode)


def check_kept_count(h_score, detection_threshold, n, where=""):
    n_host = int(np.count_nonzero(np.asarray(h_score, dtype=np.float32) >= np.float32(detection_threshold)))
    if n_host != n:
        raise RuntimeError(f"{where}detection count mismatch between host ({n_host}) and device ({n}): scores on the host and on the device differ")


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


def two_stage_assignment(reid, reid_threshold, box_threshold, box=None):
    """tracker.py:139-176: re-ID costs first, then box costs on the pairs that remain -> (matches, unmatched_dets, unmatched_tracks).
    `box`: the full [n, T] matrix (element-wise costs: the remaining-pairs matrix of tracker.py:157-162 is a sub-matrix of it), a callable
    (unmatched_dets, unmatched_tracks) -> that sub-matrix, or None (no second stage)."""
    if reid.shape[1] == 0:
        return [], list(range(reid.shape[0])), []
    matches, unmatched_dets, unmatched_tracks = match_with_threshold(reid, reid_threshold)
    if box is not None:
        sub = box(unmatched_dets, unmatched_tracks) if callable(box) else box[np.ix_(unmatched_dets, unmatched_tracks)]
        new_matches, ud, ut = match_with_threshold(sub, box_threshold)
        matches.extend((unmatched_dets[x], unmatched_tracks[y]) for x, y in new_matches)
        unmatched_dets, unmatched_tracks = [unmatched_dets[x] for x in ud], [unmatched_tracks[y] for y in ut]
    return matches, unmatched_dets, unmatched_tracks


def low_stage(low_box, low_index, unmatched_tracks, eligible, low_box_threshold):
    """The BYTE stage (include/centernet_gfx950.h): the tracks still unmatched after two_stage_assignment, restricted to those with
    eligible[t] (None: all), against the low-score detections by box cost alone.  `low_box` float32 [n_low, T] (rows: low_index).
    -> (low matches as (ORIGINAL detection index, track) in low-row order, the tracks unmatched after all three stages)."""
    U = [t for t in unmatched_tracks if eligible is None or eligible[t]]
    if not U or low_box.shape[0] == 0:
        return [], unmatched_tracks
    pairs, _, _ = match_with_threshold(low_box[:, U], low_box_threshold)
    hit = {U[y] for _, y in pairs}
    return [(int(low_index[x]), U[y]) for x, y in pairs], [t for t in unmatched_tracks if t not in hit]


class TrackState(Enum):
    UNCONFIRMED = auto()
    ACTIVE = auto()
    INACTIVE = auto()
    TO_DELETE = auto()


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


_KALMAN_MODES = ("host", "device")


class DeviceKalman:
    """`Track.kf` with kalman="device": a view of the track's row of the device state tables (cnl_track_kalman_f64), fetched on access
    as `Track.embedding` is.  `x` float64 [8] (corners, velocities), `P` float64 [8, 8]; there is nothing to call: the filter runs in the
    launch behind the table update."""
    __slots__ = ("_track",)

    def __init__(self, track):
        self._track = track

    @property
    def x(self):
        return self._track._tracker._table.read_row("kx", self._track._row)

    @property
    def P(self):
        return self._track._tracker._table.read_row("kP", self._track._row).reshape(8, 8)


class Track:
    """Host record of one track (tracker.py:217-347).  bbox / label live here (they are reported every frame); the embedding
    lives in the tracker's device table and is fetched on access.  `use_kalman`: False, True / "host" (a BoxKalman beside the record) or
    "device" (the state lives in the device table; `kf` is a DeviceKalman view and `bbox` is set from the launch's record)."""

    def __init__(self, tracker, track_id, bbox, label, min_birth_age=2, max_inactive_age=30, smoothing_factor=0.9, use_kalman=False):
        self._tracker = tracker
        self._device_kalman = use_kalman == "device"
        self.kf = DeviceKalman(self) if self._device_kalman else BoxKalman(bbox) if use_kalman else None
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
        return self._tracker._table.read_row("emb", self._row)

    def update_matched(self, bbox):
        if self.state == TrackState.UNCONFIRMED:
            self.birth_age += 1
            if self.birth_age >= self.min_birth_age:
                self.state = TrackState.ACTIVE
        elif self.state == TrackState.INACTIVE:
            self.state = TrackState.ACTIVE
            self.inactive_age = 0
        # tracker.py:311-323: the detection's box, or the filtered state when the track carries a Kalman filter (a device filter: the
        # detection's box until TrackTable.apply_kalman's caller replaces it with the filtered one of the launch's record)
        self.bbox = bbox if self.kf is None or self._device_kalman else self.kf.update(bbox)

    def kalman_predict(self):
        """tracker.py:281-290 (called at the end of every Tracker.update; `bbox` keeps the last UPDATED state, as in the reference,
        where it is a view of the array that filterpy's predict replaces).  A device filter predicts in its launch, not here."""
        if self.kf is not None and not self._device_kalman:
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


def life_cycle(tracks, matches, unmatched_dets, unmatched_tracks, det_index, boxes, labels, next_id, settings, low_matches=None):
    """One frame of the track life cycle (tracker.py:164-196) from an assignment; pure host code (no torch, no library call).  `boxes` /
    `labels`: the frame's UNfiltered [k, ...] arrays; `settings`: the tracker or bank (its min_birth_age, max_inactive_age, smoothing_factor
    and use_kalman / kalman go to the tracks born now, whose `embedding` reads its device table; with kalman="device" no BoxKalman is built
    or called here: the tracks' filtered boxes come from TrackTable.apply_kalman afterwards).
    Returns (tracks, next_id, old_rows, det_rows): per surviving track its row in `tracks` as given (-1: born now) and the detection row
    that feeds its table row (-1: carried over) — the two index lists of cnl_track_apply_f32.
    `low_matches` (None: no low-score stage, the four values above): the BYTE stage's (ORIGINAL detection index, track) pairs, possibly none
    — no quirk: the track takes that detection's box and keeps its embedding.  When given, a fifth value is returned: per surviving track 1
    if its table row keeps the old embedding (cnl_track_apply_keep_f32)."""
    use_kalman = settings.use_kalman and getattr(settings, "kalman", "host")     # False | "host" | "device" (Track.__init__)
    old_rows = list(range(len(tracks)))
    det_rows = [-1] * len(tracks)
    for det_idx, track_idx in matches:
        # reference quirk kept (tracker.py:171): the match indexes the thresholded arrays but the update reads the
        # unfiltered ones at the same position; identical when scores are sorted descending (gather_tracking2d output)
        tracks[track_idx].update_matched(boxes[det_idx])
        det_rows[track_idx] = det_idx
    keep_emb = [0] * len(tracks)
    for det_idx, track_idx in low_matches or ():
        tracks[track_idx].update_matched(boxes[det_idx])
        det_rows[track_idx] = det_idx
        keep_emb[track_idx] = 1
    for track_idx in unmatched_tracks:
        tracks[track_idx].update_unmatched()
    tracks = list(tracks)
    for det_idx in unmatched_dets:
        src = int(det_index[det_idx])
        tracks.append(Track(settings, next_id, boxes[src], labels[src], min_birth_age=settings.min_birth_age,
                            max_inactive_age=settings.max_inactive_age, smoothing_factor=settings.smoothing_factor,
                            use_kalman=use_kalman))
        next_id += 1
        old_rows.append(-1)
        det_rows.append(src)
    keep = [i for i, t in enumerate(tracks) if t.state is not TrackState.TO_DELETE]
    out = [tracks[i] for i in keep], next_id, [old_rows[i] for i in keep], [det_rows[i] for i in keep]
    return out if low_matches is None else (*out, [keep_emb[i] if i < len(keep_emb) else 0 for i in keep])


class TrackTable:
    """The device track table: `emb` [capacity, E] / `box` [capacity, 4] float32 (first rows live), the spare pair the next update writes
    (ping-pong), the mapped host memory holding the two index lists cnl_track_apply_f32 reads, the stream of the last update.
    With `kalman` (use_kalman=True, kalman="device") also the filter state `kx` [capacity, 8] / `kP` [capacity, 64] float64 and its spare
    pair, at the capacities of emb / box; the mapped index block then holds a third list, the flags of cnl_track_kalman_f64, and a second
    mapped block receives that launch's record (filtered boxes, status words).
    The stream rule: every launch that writes the tables goes to the caller's current stream, remembered in `stream`, and may still be queued
    when the caller gets control back.  Whoever touches the tables or the mapped index lists from the host side under ANOTHER stream finishes
    `stream` first, with a host-blocking synchronize: the next update (wait_for_other_stream) and the host reads of a row (read_row, behind
    Track.embedding and DeviceKalman).  Under the same stream, stream order does it and nothing blocks.  The device views (`emb`, `box`,
    `kx`, `kP`, track_embeddings()) are ordered on `stream` alone: a caller that reads them on another stream orders that stream itself."""
    __slots__ = ("emb", "box", "stream", "_spare", "_src", "_lists", "kalman", "kx", "kP", "_kspare", "_kout")

    def __init__(self, kalman=False):
        self.emb = self.box = self.stream = self._spare = self._src = self._lists = None
        self.kalman = bool(kalman)
        self.kx = self.kP = self._kspare = self._kout = None

    def wait_for_other_stream(self, cur=None):
        """The caller changed streams between frames: the previous table update (which reads the mapped index lists and writes the tables
        this frame reads) ran on another stream — finish it first (same stream: stream order does it; None: finish it anyway)."""
        if self.stream is not None and (cur is None or self.stream != cur):
            self.stream.synchronize()

    def read_row(self, name, row, cur=None):
        """Host copy of row `row` of the table `name` ("emb", "box", "kx", "kP"), read under the stream `cur` (default: the current stream of
        the table's device): the bytes of the finished last update, which may have run on another stream (wait_for_other_stream's rule)."""
        table = getattr(self, name)
        if cur is None:
            cur = torch.cuda.current_stream(table.device)
        self.wait_for_other_stream(cur)
        with torch.cuda.stream(cur) if table.is_cuda else _NO_GUARD:
            return table[row].cpu().numpy()

    def clear(self):
        """Forget the rows, behind the last update (the mapped index lists stay)."""
        self.wait_for_other_stream()
        self.emb = self.box = self.stream = self._spare = None
        self.kx = self.kP = self._kspare = None

    def apply(self, src_trk, src_det, d_emb, d_box, E, smoothing_factor, cur, keep_emb=None):
        """One cnl_track_apply_f32 launch on `cur` builds the new table: row r is old row src_trk[r] (-1: a birth), updated from detection
        row src_det[r] of d_emb / d_box (-1: copied through).  The caller holds the device guard.
        `keep_emb` (the BYTE stage; None: the launch above, unchanged): one flag per row, a matched row with its flag set takes the detection's
        box and keeps the old embedding (cnl_track_apply_keep_f32); the flags are one more row of the mapped index block, one byte each."""
        rows = len(src_trk)
        if rows == 0:
            return
        # the two index lists sit in mapped host memory that the kernel reads directly (2 x rows int32 over PCIe): no host -> device
        # copy.  The kernel still reads them after the host has moved on: they are overwritten only behind the synchronisation of the
        # next frame's association, which follows this launch in stream order (another stream: wait_for_other_stream)
        nl = (3 if self.kalman else 2) + (keep_emb is not None)     # the third list: the flags of cnl_track_kalman_f64 (apply_kalman); last: keep_emb
        if self._src is None or self._lists.shape[0] < nl or self._lists.shape[1] < rows:
            self._src = _Mapped(4 * nl * max(1024, 1 << (rows - 1).bit_length()))
            self._lists = self._src.np.view(np.int32).reshape(nl, -1)
        lists = self._lists
        lists[0, :rows] = src_trk
        lists[1, :rows] = src_det
        if self._spare is None or self._spare[0].shape[0] < rows or self._spare[0].shape[1] != E:
            cap = max(64, 1 << (rows - 1).bit_length())
            self._spare = (torch.empty((cap, E), device=d_emb.device, dtype=torch.float32),
                           torch.empty((cap, 4), device=d_emb.device, dtype=torch.float32))
        new_emb, new_box = self._spare
        old = self.emb is not None
        n = lists.shape[1]
        args = (self.emb.data_ptr() if old else None, self.box.data_ptr() if old else None, d_emb.data_ptr(), d_box.data_ptr(), self._src.ptr,
                self._src.ptr + 4 * n, rows, E, float(smoothing_factor), new_emb.data_ptr(), new_box.data_ptr())
        if keep_emb is None:
            _lib.check(_lib.load().cnl_track_apply_f32(*args, ctypes.c_void_p(cur.cuda_stream)), "cnl_track_apply_f32")
        else:
            lists[nl - 1].view(np.uint8)[:rows] = keep_emb
            _lib.check(_lib.load().cnl_track_apply_keep_f32(*args, self._src.ptr + 4 * n * (nl - 1), ctypes.c_void_p(cur.cuda_stream)),
                       "cnl_track_apply_keep_f32")
        self.stream = cur
        self._spare, self.emb, self.box = ((self.emb, self.box) if old else None), new_emb, new_box

    def apply_kalman(self, src_trk, src_det, flags, d_emb, d_box, E, smoothing_factor, cur, keep_emb=None):
        """kalman="device": `apply`, then ONE cnl_track_kalman_f64 launch behind it on `cur`, driven by the same two lists plus `flags` (bit 0:
        predict the row at the end; a sequence, or one int for every row), then the step's SECOND stream synchronisation, which makes the
        launch's record readable -> (the born / matched rows int64 [m], their filtered boxes float64 [m, 4] — one copy the tracks' `bbox` may
        keep views of —, out_status int32 [rows] view).  Births are initialised from their detection, matched rows updated with it (their
        rows of `box` become the filtered boxes), carried rows copied through.  The caller holds the device guard."""
        rows = len(src_trk)
        if rows == 0:
            return np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros(0, np.int32)
        old_x, old_P = self.kx, self.kP
        self.apply(src_trk, src_det, d_emb, d_box, E, smoothing_factor, cur, keep_emb)
        lists = self._lists
        lists[2, :rows] = flags
        cap = self.emb.shape[0]                 # the state tables grow with the emb / box pair, at the same capacities
        if self._kspare is None or self._kspare[0].shape[0] != cap:
            self._kspare = (torch.empty((cap, 8), device=self.emb.device, dtype=torch.float64),
                            torch.empty((cap, 64), device=self.emb.device, dtype=torch.float64))
        new_x, new_P = self._kspare
        if self._kout is None or self._kout.nbytes < 36 * rows:
            self._kout = _Mapped(36 * max(1024, 1 << (rows - 1).bit_length()))
        out, n = self._kout, lists.shape[1]
        old = old_x is not None
        _lib.check(_lib.load().cnl_track_kalman_f64(old_x.data_ptr() if old else None, old_P.data_ptr() if old else None, d_box.data_ptr(),
                                                    self._src.ptr, self._src.ptr + 4 * n, self._src.ptr + 8 * n, rows, new_x.data_ptr(),
                                                    new_P.data_ptr(), self.box.data_ptr(), out.ptr, out.ptr + 32 * rows,
                                                    ctypes.c_void_p(cur.cuda_stream)), "cnl_track_kalman_f64")
        self._kspare, self.kx, self.kP = ((old_x, old_P) if old else None), new_x, new_P
        cur.synchronize()
        hit = np.flatnonzero(lists[1, :rows] >= 0)
        return hit, out.np[:32 * rows].view(np.float64).reshape(rows, 4)[hit], out.np[32 * rows:36 * rows].view(np.int32)

    def upload_boxes(self, tracks):
        """use_kalman: the table's boxes are the detections' (cnl_track_apply_f32); a Kalman track's box is its filtered state, computed on
        the host with the life cycle (8x8 float64 algebra per track): the boxes of `tracks` (rows 0..len - 1) go up in ONE copy."""
        boxes = np.asarray([np.asarray(t.bbox, np.float64) for t in tracks], np.float32).reshape(len(tracks), 4)
        with torch.cuda.device(self.box.device):
            self.box[:len(tracks)].copy_(torch.from_numpy(boxes), non_blocking=False)


_LIFECYCLE_MODES = ("host", "device")
_STATES = (None, TrackState.UNCONFIRMED, TrackState.ACTIVE, TrackState.INACTIVE, TrackState.TO_DELETE)      # the device's state words
STATUS_OVERFLOW = 1 << 16       # bit of a stream's sticky status word: births were dropped at max_tracks (cnl_track_lifecycle_i32)
STATUS_BAD_SHIFT = 1 << 17      # ... a non-finite camera_motion shift was skipped (cnl_track_shift_f64)


class ResidentKalman:
    """`kf` of a ResidentTrack: the filter state of its row at the download, `x` float64 [8], `P` float64 [8, 8]."""
    __slots__ = ("x", "P")

    def __init__(self, x, P):
        self.x, self.P = x, P


class ResidentTrack:
    """A track of a TrackerBank with lifecycle="device" as one download found it: Track's fields as plain values (`embedding` and `kf` are
    copies of the row, not views of the device table; nothing here changes the device state)."""
    __slots__ = ("track_id", "bbox", "label", "state", "birth_age", "inactive_age", "embedding", "kf")

    def __init__(self, track_id, bbox, label, state, birth_age, inactive_age, embedding, kf):
        self.track_id, self.bbox, self.label, self.state = track_id, bbox, label, state
        self.birth_age, self.inactive_age, self.embedding, self.kf = birth_age, inactive_age, embedding, kf

    active = property(lambda self: self.state == TrackState.ACTIVE)
    confirmed = property(lambda self: self.state != TrackState.UNCONFIRMED)
    to_delete = property(lambda self: self.state == TrackState.TO_DELETE)

    def __repr__(self):
        return f"track id: {self.track_id}, bbox: {self.bbox}, label: {self.label}, state: {self.state.name}"


class ResidentState:
    """Device memory of a TrackerBank with lifecycle="device" (cnl_track_lifecycle_i32): everything a step reads or writes, allocated ONCE at
    the capacity C = S * max_tracks rows and zeroed.
    One control block (uint8) holds the two banks of per-row state (track_id int64, reported box float64 [C, 4], state / birth_age /
    inactive_age / label int32, trk_off int32 [S + 1]; one is current, the next step writes the other), next_track_id int64 [S], the sticky
    status words int32 [S, 2], the S association records; and, behind what a download copies, the index lists of the table update (src_trk,
    src_det, flags, keep_emb), the eligibility bytes, the filter launch's record and the life cycle's staging.  Beside it the ping-pong
    pairs of the pooled tables (emb / box float32, kx / kP float64 with the device filter) and the association workspace:
    streams(_low)_workspace_bytes(S, k, C), 20 (24) bytes per (detection, row) pair — about 49 MB at S = 32, k = 300, max_tracks = 256.
    `args[b]` is the cnl_track_lifecycle of a step whose current bank is b; `live_lists` keeps one device copy per distinct `live` tuple
    (never rewritten, so a queued launch can never see another step's list)."""

    def __init__(self, S, M, k, E, dev, kalman, low_rec):
        lib = _lib.load()
        self.S, self.M, self.k, self.E, self.dev, self.kalman, self.low_rec = S, M, k, E, dev, kalman, low_rec
        C = self.C = S * M
        self.stride = (streams_low_layout if low_rec else streams_layout)(k, M, 0).bytes
        self.cur = 0
        off, at = {}, 0

        def carve(name, nbytes):
            nonlocal at
            off[name] = at
            at = (at + nbytes + 7) & ~7

        for b in (0, 1):
            for name, nbytes in (("track_id", 8 * C), ("box", 32 * C), ("state", 4 * C), ("birth_age", 4 * C), ("inactive_age", 4 * C),
                                 ("label", 4 * C), ("trk_off", 4 * (S + 1))):
                carve((name, b), nbytes)
        carve("next_track_id", 8 * S)
        carve("status", 8 * S)
        carve("record", S * self.stride)
        self.down_bytes = at            # a download copies the block up to here
        for name, nbytes in (("src_trk", 4 * C), ("src_det", 4 * C), ("flags", 4 * C), ("keep_emb", C), ("trk_eligible", C),
                             ("kalman_box", 32 * C if kalman else 0), ("kalman_status", 4 * C if kalman else 0)):
            carve(name, nbytes)
        lc_bytes = int(lib.cnl_track_lifecycle_workspace_bytes(S, M))
        carve("workspace", lc_bytes)
        self.off = off
        self.ctl = torch.zeros(at, device=dev, dtype=torch.uint8)
        ws_bytes = (streams_low_workspace_bytes if low_rec else streams_workspace_bytes)(S, k, C)
        self.ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        self.emb = [torch.zeros((C, E), device=dev, dtype=torch.float32) for _ in (0, 1)]
        self.box = [torch.zeros((C, 4), device=dev, dtype=torch.float32) for _ in (0, 1)]
        self.kx = [torch.zeros((C, 8), device=dev, dtype=torch.float64) for _ in (0, 1)] if kalman else None
        self.kP = [torch.zeros((C, 64), device=dev, dtype=torch.float64) for _ in (0, 1)] if kalman else None
        self.live_lists = {}
        self.live_list(())
        base = self.ctl.data_ptr()
        self.args = []
        for b in (0, 1):
            a = _lib.TrackLifecycle()
            for rows, bank in ((a.old_rows, b), (a.new_rows, 1 - b)):
                for name in ("track_id", "state", "birth_age", "inactive_age", "label", "box", "trk_off"):
                    setattr(rows, name, base + off[(name, bank)])
            a.record, a.record_stride = base + off["record"], self.stride
            for name in ("next_track_id", "status", "src_trk", "src_det", "flags", "keep_emb", "trk_eligible", "workspace"):
                setattr(a, name, base + off[name])
            a.kalman_box = base + off["kalman_box"] if kalman else None
            a.workspace_bytes = lc_bytes
            a.S, a.k, a.max_tracks, a.low_record, a.out_box_f64 = S, k, M, int(low_rec), int(kalman)
            self.args.append(a)

    def ptr(self, name, bank=None):
        return self.ctl.data_ptr() + self.off[name if bank is None else (name, bank)]

    def live_list(self, live):
        """Device int32 [L + S]: the `live` list of a step, then slot_of (stream -> slot, -1: no part); () — nobody, what reset(stream) runs
        with — is uploaded with the allocation."""
        t = self.live_lists.get(live)
        if t is None:
            slot_of = [-1] * self.S
            for i, s in enumerate(live):
                slot_of[s] = i
            t = self.live_lists[live] = torch.tensor(list(live) + slot_of, dtype=torch.int32).to(self.dev)
        return t

    def download(self):
        """ONE device -> host copy: the control block's state part and the current tables -> dict of numpy arrays over all C rows
        (`trk_off` says which are live) + `records`, the uint8 records of the S streams."""
        b, C, S = self.cur, self.C, self.S
        parts = [self.ctl[:self.down_bytes], self.emb[b].view(-1).view(torch.uint8), self.box[b].view(-1).view(torch.uint8)]
        if self.kalman:
            parts += [self.kx[b].view(-1).view(torch.uint8), self.kP[b].view(-1).view(torch.uint8)]
        h = torch.cat(parts).cpu().numpy()
        off = self.off

        def take(name, dtype, count, bank=None):
            o = off[name if bank is None else (name, bank)]
            return h[o:o + count * np.dtype(dtype).itemsize].view(dtype)

        out = {"track_id": take("track_id", np.int64, C, b), "bbox": take("box", np.float64, 4 * C, b).reshape(C, 4),
               "trk_off": take("trk_off", np.int32, S + 1, b), "next_track_id": take("next_track_id", np.int64, S),
               "status": take("status", np.int32, 2 * S).reshape(S, 2),
               "records": h[off["record"]:off["record"] + S * self.stride].reshape(S, self.stride)}
        for name in ("state", "birth_age", "inactive_age", "label"):
            out[name] = take(name, np.int32, C, b)
        at = self.down_bytes
        for name, dtype, width in (("emb", np.float32, self.E), ("box", np.float32, 4)) + ((("kx", np.float64, 8), ("kP", np.float64, 64)) if self.kalman else ()):
            n = C * width * np.dtype(dtype).itemsize
            out[name] = h[at:at + n].view(dtype).reshape(C, width)
            at += n
        return out


class TrackerSettings:
    """What `Tracker` and `TrackerBank` share: the reference's constructor arguments (tracker.py:50), the device, the model run."""
    _update_name = "update"
    d2h_bytes = 0               # bytes the association kernels stored over PCIe in the last update

    def __init__(self, model=None, nms_kernel=3, num_detections=300, detection_threshold=0.3, reid_cost="cosine",
                 reid_threshold=0.2, box_cost="iou", box_threshold=0.5, smoothing_factor=0.5, use_kalman=False,
                 max_inactive_age=30, min_birth_age=2, device=None, allow_host_cost=False, low_threshold=None,
                 low_box_threshold=None, low_match="active", class_aware=False, motion_gate=None, motion_weight=1.0, kalman="host"):
        """class_aware / motion_gate / motion_weight (off by default: the entry points and bytes without them): gates inside the cost kernels
        (cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32; the rule is the header's).  class_aware: a detection and a track may only be
        matched, in any of the three stages, if the detection's label equals the track's `label` (the label at birth).  motion_gate (True: 9.4877,
        DeepSORT's chi2inv95[4]; or a threshold; needs use_kalman=True, kalman="device"): a re-ID pair whose squared Mahalanobis distance m from
        the track's predicted filter state fails m <= motion_gate cannot be matched in stage 1 (the box stages are not motion-gated, as in
        DeepSORT); motion_weight (FairMOT's lambda): inside the gate the stage-1 cost is motion_weight * reid + (1 - motion_weight) * m, the re-ID
        cost itself at 1.  A gated pair costs 1e5 in the matrices (`last_costs` shows them), so every threshold must stay below that.
        low_threshold (None: off, the path and results without it): BYTE's second association (Zhang et al., ByteTrack) — the tracks still
        unmatched after the re-ID and box stages are matched by box cost alone (cost < low_box_threshold, default box_threshold) against the
        detections with low_threshold <= score < detection_threshold; such a match gives the track the detection's box (a measurement for
        its Kalman filter) and leaves its embedding as it was, and a low detection never starts a track.  low_match: "active" (only tracks
        that are ACTIVE at the start of the step take part) or "all".  Needs box_cost "iou" / "giou"; the rule is the header's.
        kalman (with use_kalman=True; without it, accepted and without effect): "host" (default) keeps a float64 numpy filter per track
        beside the life cycle (`Track.kf` is a BoxKalman) and uploads the filtered boxes; "device" keeps the filter state in the device
        table and runs the filter in ONE launch behind the table update (cnl_track_kalman_f64; `Track.kf` is a DeviceKalman view) — no
        per-track arithmetic and no box upload on the host, at the price of a SECOND stream synchronisation at the end of every step, which
        makes the filtered boxes readable when the step returns.  A track whose innovation covariance has no positive finite pivots (a
        zero-area box, a non-finite state) skips its update there (`kalman_skipped` counts them per step) where the host filter raises
        numpy's LinAlgError.
        reid_cost: "cosine" (default), "euclidean", "sqeuclidean", "cityblock", "chebyshev", "canberra", "braycurtis", "correlation" run on the device.  The reference accepts ANY scipy cdist metric name or
        a callable (tracker.py:51, 62-64), and a callable box_cost: those are computed on the HOST from copies of the frame's kept embeddings /
        boxes and the track table (two more device -> host copies per frame) — only with allow_host_cost=True, otherwise they raise: a silent
        CPU detour is not what a caller of a gfx950 tracker expects."""
        self.model = model
        if model is None:
            warnings.warn(f"A model was not provided. Only `.{self._update_name}()` will work")
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
        if kalman not in _KALMAN_MODES:
            raise ValueError(f"kalman={kalman!r}: expected 'host' or 'device'")
        self.kalman = kalman
        self.kalman_skipped = 0     # kalman="device": rows of the last step whose update was skipped (status bit 0 of cnl_track_kalman_f64)
        self.max_inactive_age = max_inactive_age
        self.min_birth_age = min_birth_age
        if low_match not in _LOW_MATCH:
            raise ValueError(f"low_match={low_match!r}: expected 'active' or 'all'")
        if low_threshold is not None and (self._host_box is not None or box_cost is None):
            raise ValueError(f"low_threshold={low_threshold!r} with box_cost={box_cost!r}: the low-score stage matches by the 'iou' / 'giou' box cost")
        self.low_threshold, self.low_box_threshold, self.low_match = low_threshold, low_box_threshold, low_match
        self._check_low(low_threshold, detection_threshold)
        if not isinstance(class_aware, (bool, int, np.bool_, np.integer)):
            # the three gate keywords stand in front of `kalman`, which stays the last parameter: a caller written against the earlier signature
            # who passed kalman by position lands here — refused by name, never taken for a truth value
            raise ValueError(f"class_aware={class_aware!r}: expected a bool (pass kalman, class_aware, motion_gate and motion_weight by keyword)")
        self.class_aware = bool(class_aware)
        if motion_gate is True:
            motion_gate = CHI2INV95_4
        elif motion_gate is False:
            motion_gate = None
        if motion_gate is not None:
            if not (self.use_kalman and kalman == "device"):
                raise ValueError(f"motion_gate={motion_gate!r} needs use_kalman=True, kalman='device': the gate reads the filter state of the device table")
            if not 0 <= motion_gate < GATE_COST:
                raise ValueError(f"motion_gate={motion_gate!r}: expected True, None or a threshold in [0, {GATE_COST:g})")
            motion_gate = float(motion_gate)
        if not 0 <= motion_weight <= 1:
            raise ValueError(f"motion_weight={motion_weight!r}: expected a value in [0, 1]")
        if motion_weight != 1 and motion_gate is None:
            raise ValueError(f"motion_weight={motion_weight!r} without motion_gate: the weight applies inside the motion gate")
        self.motion_gate, self.motion_weight = motion_gate, float(motion_weight)
        for name, on in (("class_aware", self.class_aware), ("motion_gate", motion_gate is not None)):
            if on and (self._host_reid is not None or self._host_box is not None):
                raise ValueError(f"{name} with reid_cost={reid_cost!r} / box_cost={box_cost!r}: the gates sit inside the gfx950 cost kernels; host-side "
                                 "costs (allow_host_cost) are not gated")
        self._check_gate_thresholds(reid_threshold, box_threshold, low_box_threshold)
        self._lab = None            # gates: mapped int32 labels of the table's rows (cnl_track_gate.trk_label)
        self._device = torch.device(device) if device is not None else None
        self._table = TrackTable(kalman=self._device_kalman)
        self._rec = None            # mapped host memory the association kernel writes its record(s) into
        self.reset()

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

    _emb = property(lambda self: self._table.emb)       # device track table [capacity, E] / [capacity, 4] (Track.embedding, tests, tools)
    _box = property(lambda self: self._table.box)
    _device_kalman = property(lambda self: self.use_kalman and self.kalman == "device")

    def _apply_with_kalman(self, tracks, src_trk, src_det, flags, d_emb, d_box, E, cur, keep_emb=None):
        """kalman="device": the table update and the filter launch for `tracks` (row order of the new table), then the filtered box of every
        born / matched track from the launch's record (a carried track keeps its `bbox`).  The caller holds the device guard."""
        hit, boxes, status = self._table.apply_kalman(src_trk, src_det, flags, d_emb, d_box, E, self.smoothing_factor, cur, keep_emb)
        for r, b in zip(hit.tolist(), boxes):
            tracks[r].bbox = b
        self.kalman_skipped = int(np.count_nonzero(status))

    _gated = property(lambda self: self.class_aware or self.motion_gate is not None)

    @staticmethod
    def _refuse_camera_motion(kwargs, who):
        """camera_motion= shifts the resident bank's tables on the device; every other mode keeps its track boxes in host records."""
        if kwargs.pop("camera_motion", None) is not None:
            raise ValueError(f"camera_motion= with {who}: TrackerBank(lifecycle='device') is required (here the track boxes live in host records, "
                             "and a device shift would cost the synchronisation the option exists to avoid)")

    def _check_gate_thresholds(self, *thresholds):
        """With a gate on, a threshold at or above the gated pairs' cost would accept them."""
        if self._gated:
            for t in thresholds:
                if t is not None and not t < GATE_COST:
                    raise ValueError(f"threshold {t!r} with class_aware / motion_gate: gated pairs cost {GATE_COST:g}, every threshold must be below it")

    def _gate(self, spans, rows, kx, kP):
        """The cnl_track_gate of one launch over a table of `rows` rows.  spans: (first row, tracks in row order) of every stream that takes
        part — their labels go into mapped memory that the cost kernel reads, as it reads the eligibility bytes (finished with at the step's
        synchronisation).  kx / kP: the table's state tensors (None: no rows yet)."""
        gate = _lib.TrackGate(None, None, None, 0.0, 1.0)
        if self.class_aware and rows:
            self._lab = _grown(self._lab, 4 * rows, 1 << 12)
            lab = self._lab.np.view(np.int32)
            for row0, tracks in spans:
                lab[row0:row0 + len(tracks)] = [int(t.label) for t in tracks]
            gate.trk_label = self._lab.ptr
        if self.motion_gate is not None and rows and kx is not None:
            gate.kx, gate.kP, gate.motion_gate, gate.motion_weight = kx.data_ptr(), kP.data_ptr(), self.motion_gate, self.motion_weight
        return gate

    @staticmethod
    def _check_low(low_threshold, detection_threshold):
        if low_threshold is not None and not 0 <= low_threshold <= detection_threshold:
            raise ValueError(f"low_threshold={low_threshold!r}: expected a value in [0, detection_threshold = {detection_threshold!r}]")

    def _thresholds(self, kwargs):
        """(detection, re-ID, box, low, low box) thresholds of one call: the settings unless the call overrides them (low: None = no low-score
        stage; low box: the call's box threshold unless set)."""
        if not kwargs:
            low_box = self.box_threshold if self.low_box_threshold is None else self.low_box_threshold
            return self.detection_threshold, self.reid_threshold, self.box_threshold, self.low_threshold, low_box
        det, box = kwargs.get("detection_threshold", self.detection_threshold), kwargs.get("box_threshold", self.box_threshold)
        low, low_box = kwargs.get("low_threshold", self.low_threshold), kwargs.get("low_box_threshold", self.low_box_threshold)
        self._check_low(low, det)
        self._check_gate_thresholds(kwargs.get("reid_threshold"), box, low_box)
        if low is not None and (self._host_box is not None or self.box_cost is None):
            raise ValueError(f"low_threshold={low!r} with box_cost={self.box_cost!r}: the low-score stage matches by the 'iou' / 'giou' box cost")
        return det, kwargs.get("reid_threshold", self.reid_threshold), box, low, box if low_box is None else low_box

    def _eligible(self, tracks):
        """low_match: which of `tracks` may be matched in the low-score stage, by their state at the start of the step (None: all)."""
        return None if self.low_match == "all" else [t.state is TrackState.ACTIVE for t in tracks]

    def _detect(self, images, kwargs):
        """The model's detections for a batch of frames (tracker.py:98-104); the kernel that computes a frame's costs also writes its
        boxes / scores / labels into the frame record: no separate copy."""
        self.model.eval()
        heatmap, box_2d, reid = self.model(images.to(self.device))
        return self.model.gather_tracking2d(heatmap, box_2d, reid, nms_kernel=kwargs.get("nms_kernel", self.nms_kernel),
                                            num_detections=kwargs.get("num_detections", self.num_detections), normalize_bbox=True)


def _to_dev(a, dev):
    if isinstance(a, torch.Tensor) and a.device == dev and a.dtype == torch.float32 and a.is_contiguous():
        # already where the kernels read it (each .to() costs ~7 us of host time) — unless it is a view that starts off a 16-byte boundary: the cost
        # kernels read boxes and embedding rows 16 bytes at a time and their launchers refuse such a pointer, so it is copied to an allocation of its own
        return a if a.data_ptr() % 16 == 0 else a.clone()
    return torch.as_tensor(a).to(device=dev, dtype=torch.float32).contiguous()


def _to_host(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def normalise_detections(dev, bboxes, labels, scores, embeddings, lead=()):
    """[*lead, k, 4], [*lead, k], [*lead, k], [*lead, k, E] (`lead` = () for one frame, (L,) for one frame per stream) as numpy arrays or torch
    tensors anywhere -> (d_box, d_score, d_emb, d_label, host, label_kind): contiguous float32 tensors on `dev`, and EITHER the labels on
    `dev` + the element type the kernel reads them as (device inputs: the three small arrays the host-side life cycle reads come back inside
    the record, `host` None) OR `host` = (boxes, labels, scores) as numpy arrays, which the caller holds already (d_label None, kind 0)."""
    try:
        shape = embeddings.shape[:-1]               # [*lead, k]; checked before anything moves to the device
        if len(shape) != len(lead) + 1 or shape[:-1] != lead or bboxes.shape != (*shape, 4) or scores.shape != shape or \
                labels.shape[:len(shape)] != shape:
            raise ValueError(f"detections: boxes {tuple(bboxes.shape)}, labels {tuple(labels.shape)}, scores {tuple(scores.shape)}, embeddings "
                             f"{tuple(embeddings.shape)}, expected [{', '.join(map(str, lead + ('k', 'E')))}] embeddings and k boxes / labels / scores")
    except AttributeError:                          # nested lists: as arrays
        return normalise_detections(dev, *(np.asarray(a) for a in (bboxes, labels, scores, embeddings)), lead)
    d_box, d_score, d_emb = _to_dev(bboxes, dev), _to_dev(scores, dev), _to_dev(embeddings, dev)
    if not all(isinstance(a, torch.Tensor) and a.is_cuda for a in (bboxes, labels, scores)):
        return d_box, d_score, d_emb, None, (_to_host(bboxes), _to_host(labels), _to_host(scores)), 0
    d_label = labels.to(dev)
    label_kind = _LABEL_KINDS.get(d_label.dtype, 0)
    if not label_kind:
        d_label, label_kind = d_label.to(torch.int64), 1
    return d_box, d_score, d_emb, d_label.contiguous(), None, label_kind
