"""Zone occupancy, line crossings and dwell events on the GPU: the stage behind `TrackerBank(lifecycle="device")` that turns tracks into facts
— how many are in this area, who crossed this line and which way, who has stood here too long.

`ZoneCounter.update` takes the dict the bank's `step_batch` / `update_batch` return, as it is, and makes ONE call of cnl_track_zones_f64
(csrc/track_zones.hip) on the caller's current stream: no synchronisation, no upload in steady state, no per-track Python.  The geometry is
uploaded once; the per-stream state (a list of remembered tracks keyed by track id, the cumulative counters) lives on the device in two
banks that change places per call.  The rule is stated in include/centernet_gfx950.h and restated in numpy by tests/zones_ref.py.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib

MAX_ZONES, MAX_LINES, MAX_VERTICES, MAX_LABELS, MAX_TRACKS, MAX_EVENTS = 16, 16, 16, 8, 4096, 65536
ZONE_BYTES, LINE_BYTES = 336, 104                                   # the records of the geometry block (include/centernet_gfx950.h)
ENTER, EXIT, FORWARD, BACKWARD, DWELL = 1, 2, 3, 4, 5               # event kinds
STATUS_NON_FINITE, STATUS_CAPACITY, STATUS_EVENTS = 1, 2, 4         # bits of a stream's sticky status word
ANCHORS = {"bottom_center": 0, "center": 1}


def _int(name, v, lo, hi):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name}={v!r}: expected an integer in {lo}..{hi}")
    return int(v)


def _labels(what, labels):
    if labels is None:
        return ()
    try:
        out = tuple(_int(f"{what}: label", x, -2 ** 63, 2 ** 63 - 1) for x in labels)
    except TypeError:
        raise ValueError(f"{what}: labels={labels!r}: expected None or 1..{MAX_LABELS} class ids") from None
    if not 1 <= len(out) <= MAX_LABELS:
        raise ValueError(f"{what}: labels={labels!r}: expected None or 1..{MAX_LABELS} class ids")
    return out


def _finite(what, v):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: {v!r} is not a number") from None
    if not math.isfinite(f):
        raise ValueError(f"{what}: non-finite coordinate {v!r}")
    return f


class Zone:
    """A polygon of 3..16 (x, y) vertices in the units of the boxes that will be passed (normalised coordinates for `step_batch`), even-odd
    rule.  labels: None, or up to 8 class ids a track must have to count.  dwell_alert: a step count; a track whose consecutive steps inside
    reach exactly it makes one DWELL event (0: off)."""

    def __init__(self, vertices, labels=None, dwell_alert=0):
        try:
            pts = [tuple(p) for p in vertices]
        except TypeError:
            raise ValueError(f"Zone: vertices={vertices!r}: expected 3..{MAX_VERTICES} (x, y) pairs") from None
        if not 3 <= len(pts) <= MAX_VERTICES:
            raise ValueError(f"Zone: {len(pts)} vertices: expected 3..{MAX_VERTICES}")
        if any(len(p) != 2 for p in pts):
            raise ValueError(f"Zone: vertices={vertices!r}: expected (x, y) pairs")
        self.vertices = tuple((_finite("Zone", x), _finite("Zone", y)) for x, y in pts)
        self.labels = _labels("Zone", labels)
        self.dwell_alert = _int("Zone: dwell_alert", dwell_alert, 0, 2 ** 31 - 1)

    def __repr__(self):
        return f"Zone({list(self.vertices)!r}, labels={list(self.labels) or None!r}, dwell_alert={self.dwell_alert})"


class Line:
    """A directed segment A = (ax, ay) -> B = (bx, by).  A FORWARD crossing enters the side where cross(B - A, p - A) > 0: on a y-down screen
    the right-hand side of A -> B.  labels as for Zone."""

    def __init__(self, ax, ay, bx, by, labels=None):
        self.a = (_finite("Line", ax), _finite("Line", ay))
        self.b = (_finite("Line", bx), _finite("Line", by))
        if self.a == self.b:
            raise ValueError(f"Line: A equals B ({self.a}): a line needs two distinct points")
        self.labels = _labels("Line", labels)

    def __repr__(self):
        return f"Line({self.a[0]!r}, {self.a[1]!r}, {self.b[0]!r}, {self.b[1]!r}, labels={list(self.labels) or None!r})"


def _per_stream(name, items, kind, S, limit):
    """`items` -> S lists of `kind`: one list shared by every stream, or a list of S lists."""
    items = [] if items is None else list(items)
    if items and all(isinstance(x, (list, tuple)) for x in items):
        if len(items) != S:
            raise ValueError(f"{name}: {len(items)} per-stream lists for {S} streams")
        per = [list(x) for x in items]
    else:
        per = [items] * S
    for s, one in enumerate(per):
        if any(not isinstance(x, kind) for x in one):
            raise ValueError(f"{name}: expected {kind.__name__} objects, one list for every stream or a list of {S} lists")
        if len(one) > limit:
            raise ValueError(f"{name}: {len(one)} for stream {s}: at most {limit} {name} per stream")
    return per


def geometry_records(zones, lines, Z, Ln):
    """The geometry block of cnl_track_zones_f64: uint8 [S, 8 + 336 Z + 104 Ln] from S lists of Zone and of Line."""
    S = len(zones)
    rec = np.zeros((S, 8 + ZONE_BYTES * Z + LINE_BYTES * Ln), np.uint8)
    for s in range(S):
        rec[s, :8].view(np.int32)[:] = len(zones[s]), len(lines[s])
        for z, zone in enumerate(zones[s]):
            r = rec[s, 8 + ZONE_BYTES * z:8 + ZONE_BYTES * (z + 1)]
            r[:16].view(np.int32)[:3] = len(zone.vertices), zone.dwell_alert, len(zone.labels)
            r[16:80].view(np.int64)[:len(zone.labels)] = zone.labels
            r[80:].view(np.float64)[:2 * len(zone.vertices)] = np.asarray(zone.vertices, np.float64).reshape(-1)
        for l, line in enumerate(lines[s]):
            r = rec[s, 8 + ZONE_BYTES * Z + LINE_BYTES * l:8 + ZONE_BYTES * Z + LINE_BYTES * (l + 1)]
            r[:32].view(np.float64)[:] = line.a + line.b
            r[32:40].view(np.int32)[0] = len(line.labels)
            r[40:].view(np.int64)[:len(line.labels)] = line.labels
    return rec


class ZoneCounter:
    """Zones and lines for `num_streams` video streams.

        zc = ZoneCounter(num_streams=S, zones=[Zone([(0.1, 0.5), (0.9, 0.5), (0.9, 1.0), (0.1, 1.0)], dwell_alert=250)],
                         lines=[Line(0.0, 0.5, 1.0, 0.5)], max_tracks=256)
        tracks = bank.step_batch(images)            # TrackerBank(lifecycle="device")
        out = zc.update(tracks)                     # one launch behind the bank's, nothing read

    zones / lines: one list shared by every stream, or a list of S lists; at most 16 of each per stream.  anchor: the point of a box that is
    tested, "bottom_center" ((x1 + x2) / 2, y2) or "center".  max_tracks: the bank's (rows per stream, <= 4096); a stream remembers at most
    2 * max_tracks tracks.  max_absent: steps a track may be missing from the bank's output before the counter forgets it (with an EXIT event per
    zone it was in); 30 mirrors the bank's max_inactive_age default — a stated default, not a measurement.  max_events: rows of the event
    list per stream and step.  The device is that of the first update's tensors unless given."""

    def __init__(self, num_streams, zones=None, lines=None, max_tracks=256, anchor="bottom_center", max_absent=30, max_events=64, device=None):
        S = self.num_streams = _int("num_streams", num_streams, 1, 65535)
        self.zones = _per_stream("zones", zones, Zone, S, MAX_ZONES)
        self.lines = _per_stream("lines", lines, Line, S, MAX_LINES)
        self.Z, self.Ln = max(len(x) for x in self.zones), max(len(x) for x in self.lines)
        self.max_tracks = _int("max_tracks", max_tracks, 1, MAX_TRACKS)
        if anchor not in ANCHORS:
            raise ValueError(f"anchor={anchor!r}: expected one of {sorted(ANCHORS)}")
        self.anchor = anchor
        self.max_absent = _int("max_absent", max_absent, 0, 2 ** 31 - 2)
        self.max_events = _int("max_events", max_events, 1, MAX_EVENTS)
        self.device = None if device is None else torch.device(device)
        if self.device is not None and self.device.type != "cuda":
            raise ValueError(f"device={device!r}: ZoneCounter runs on HIP devices only (no CPU fallback)")
        self._geometry = geometry_records(self.zones, self.lines, self.Z, self.Ln)
        self._state = None              # device memory, allocated by the first update
        self._stream = None             # the stream of the last launch (a call under another stream finishes it first)
        self._bank = 0
        self._step_no = 0

    @classmethod
    def from_config(cls, section, num_streams):
        """A counter from a plain dict {"zones": [...], "lines": [...], **settings}.  A zone is a dict of Zone's arguments or a bare vertex
        list; a line is a dict of Line's arguments or [ax, ay, bx, by]; either list may instead be a list of num_streams such lists."""
        cfg = dict(section)

        def number(x):
            return isinstance(x, (int, float, np.integer, np.floating)) and not isinstance(x, bool)

        def zone(x):
            return x if isinstance(x, Zone) else Zone(**x) if isinstance(x, dict) else Zone(x)

        def line(x):
            return x if isinstance(x, Line) else Line(**x) if isinstance(x, dict) else Line(*x)

        def is_zone(x):
            return isinstance(x, (Zone, dict)) or (isinstance(x, (list, tuple)) and len(x) > 0 and isinstance(x[0], (list, tuple)) and
                                                   len(x[0]) > 0 and number(x[0][0]))

        def is_line(x):
            return isinstance(x, (Line, dict)) or (isinstance(x, (list, tuple)) and len(x) > 0 and number(x[0]))

        def build(items, one, is_one):
            items = list(items or [])
            if all(is_one(x) for x in items):
                return [one(x) for x in items]
            return [[one(y) for y in x] for x in items]

        zones, lines = build(cfg.pop("zones", None), zone, is_zone), build(cfg.pop("lines", None), line, is_line)
        return cls(num_streams, zones=zones, lines=lines, **cfg)

    # ------------------------------------------------------------------------------------------------------------------ device memory
    def _allocate(self, dev):
        S, Z, Ln = self.num_streams, self.Z, self.Ln
        nbytes = int(_lib.load().cnl_track_zones_state_bytes(S, self.max_tracks, Z, Ln))
        if nbytes <= 0:
            raise ValueError(f"ZoneCounter: cnl_track_zones_state_bytes({S}, {self.max_tracks}, {Z}, {Ln}) refused the sizes")
        self.device = dev
        self._stream_bytes = nbytes // (2 * S)
        self._state = torch.zeros(nbytes, device=dev, dtype=torch.uint8)
        self._status = torch.zeros((S, 2), device=dev, dtype=torch.int32)
        self._geometry_dev = torch.from_numpy(self._geometry).to(dev)
        self._live_lists = {}

    def _live_list(self, live):
        """Device int32 [S]: the participating streams in slot order, then the others; one copy per distinct tuple, never rewritten, so a
        queued launch can never see another step's list."""
        t = self._live_lists.get(live)
        if t is None:
            rest = [s for s in range(self.num_streams) if s not in set(live)]
            t = self._live_lists[live] = torch.tensor(list(live) + rest, dtype=torch.int32).to(self.device)
        return t

    def _check_streams(self, streams):
        S = self.num_streams
        live = list(range(S)) if streams is None else [int(x) for x in streams]
        if not live or any(x < 0 or x >= S for x in live) or len(set(live)) != len(live):
            raise ValueError(f"streams={streams!r}: expected distinct stream indices in 0..{S - 1}, at least one")
        return tuple(live)

    def _enter(self, dev):
        """The caller's current stream; a launch queued under another stream is finished first."""
        cur = torch.cuda.current_stream(dev)
        if self._stream is not None and self._stream != cur:
            self._stream.synchronize()
        return cur

    # ------------------------------------------------------------------------------------------------------------------ the step
    def update(self, tracks, streams=None):
        """tracks: the dict of TrackerBank(lifecycle="device").step_batch / update_batch — "bboxes" [L, M, 4] float32 or float64 (x1 y1 x2
        y2), "track_ids" and "labels" [L, M] int64, "count" [L] int32, tensors on the counter's device, M <= max_tracks; row i belongs to
        stream streams[i] (default: stream i).  A stream that takes no part is carried untouched: nothing ages.
        -> dict of device tensors, ordered on the current stream: "inside" [L, M] int32 (bit z: the track's anchor is in zone z; 0 from count
        on), "dwell" [L, M, Z] int32 (consecutive counted steps inside, this one included), "occupancy" [L, Z] int32, "zone_counts" [L, Z, 2]
        int64 (enters, exits since reset), "line_counts" [L, Ln, 2] int64 (forward, backward since reset), "events" [L, max_events, 4] int64
        (track_id, kind, index, value; zero rows behind the live ones), "event_count" [L] int32 (the true number: it may exceed max_events)."""
        what = "ZoneCounter.update"
        try:
            boxes, ids, labels, count = tracks["bboxes"], tracks["track_ids"], tracks["labels"], tracks["count"]
        except (KeyError, TypeError):
            raise ValueError(f"{what}: expected the dict of a device life-cycle step (bboxes, track_ids, labels, count)") from None
        dev = self.device
        for name, t in (("bboxes", boxes), ("track_ids", ids), ("labels", labels), ("count", count)):
            if not (isinstance(t, torch.Tensor) and t.is_cuda and (dev is None or t.device == dev)):
                raise ValueError(f"{what}: {name} must be a tensor on the counter's device, got {type(t).__name__}"
                                 f"{' on ' + str(t.device) if isinstance(t, torch.Tensor) else ''} (host arrays are refused: the counter "
                                 "exists to stay on the device)")
            dev = t.device
        live = self._check_streams(streams)
        L = len(live)
        if boxes.dim() != 3 or boxes.shape[0] != L or boxes.shape[2] != 4 or boxes.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"{what}: bboxes {tuple(boxes.shape)} {boxes.dtype}: expected [{L}, M, 4] float32 or float64")
        M = int(boxes.shape[1])
        if not 1 <= M <= self.max_tracks:
            raise ValueError(f"{what}: M = {M} rows per stream: expected 1..max_tracks = {self.max_tracks}")
        for name, t, shape, dtype in (("track_ids", ids, (L, M), torch.int64), ("labels", labels, (L, M), torch.int64),
                                      ("count", count, (L,), torch.int32)):
            if tuple(t.shape) != shape or t.dtype != dtype:
                raise ValueError(f"{what}: {name} {tuple(t.shape)} {t.dtype}: expected {list(shape)} {dtype}")
        S, Z, Ln, K = self.num_streams, self.Z, self.Ln, self.max_events
        lib = _lib.load()
        with torch.cuda.device(dev):
            cur = self._enter(dev)
            if self._state is None:
                self._allocate(dev)
            lv = self._live_list(live)
            boxes, ids, labels, count = boxes.contiguous(), ids.contiguous(), labels.contiguous(), count.contiguous()
            out = {"inside": torch.empty((L, M), device=dev, dtype=torch.int32), "dwell": torch.empty((L, M, Z), device=dev, dtype=torch.int32),
                   "occupancy": torch.empty((L, Z), device=dev, dtype=torch.int32),
                   "zone_counts": torch.empty((L, Z, 2), device=dev, dtype=torch.int64),
                   "line_counts": torch.empty((L, Ln, 2), device=dev, dtype=torch.int64),
                   "events": torch.empty((L, K, 4), device=dev, dtype=torch.int64), "event_count": torch.empty((L,), device=dev, dtype=torch.int32)}

            def ptr(t):
                return t.data_ptr() if t.numel() else None

            args = _lib.TrackZones(boxes.data_ptr(), ids.data_ptr(), labels.data_ptr(), count.data_ptr(), lv.data_ptr(), self._geometry_dev.data_ptr(),
                                   self._state.data_ptr(), self._status.data_ptr(), out["inside"].data_ptr(), ptr(out["dwell"]), ptr(out["occupancy"]),
                                   ptr(out["zone_counts"]), ptr(out["line_counts"]), out["events"].data_ptr(), out["event_count"].data_ptr(),
                                   S, L, M, self.max_tracks, Z, Ln, K, self.max_absent, ANCHORS[self.anchor], int(boxes.dtype == torch.float64),
                                   self._bank, self._step_no & 0x7fffffff)
            _lib.check(lib.cnl_track_zones_f64(ctypes.byref(args), ctypes.c_void_p(cur.cuda_stream)), "cnl_track_zones_f64")
            self._stream = cur
        self._bank = 1 - self._bank
        self._step_no += 1
        return out

    def reset(self, stream=None):
        """Forget every stream's tracks and counters (None) or one stream's: a zeroing queued on the current stream, no synchronisation."""
        live = None if stream is None else self._check_streams([stream])
        if self._state is None:
            return
        with torch.cuda.device(self.device):
            cur = self._enter(self.device)
            if live is None:
                self._state.zero_()
            else:
                self._state.view(2, self.num_streams, self._stream_bytes)[self._bank, live[0]].zero_()
            self._stream = cur

    def totals(self):
        """ONE download: {"zone_counts": int64 [S, Z, 2] (enters, exits), "line_counts": int64 [S, Ln, 2] (forward, backward)} since reset."""
        S, Z, Ln = self.num_streams, self.Z, self.Ln
        if self._state is None:
            return {"zone_counts": np.zeros((S, Z, 2), np.int64), "line_counts": np.zeros((S, Ln, 2), np.int64)}
        with torch.cuda.device(self.device):
            self._enter(self.device)
            head = self._state.view(2, S, self._stream_bytes)[self._bank, :, :16 * (Z + Ln)].cpu().numpy()
        words = np.ascontiguousarray(head).view(np.int64).reshape(S, 2 * (Z + Ln))
        return {"zone_counts": words[:, :2 * Z].reshape(S, Z, 2).copy(), "line_counts": words[:, 2 * Z:].reshape(S, Ln, 2).copy()}

    def check(self):
        """Download the streams' sticky status words; if any is set, clear them all and raise ValueError naming each stream, what happened
        (a non-finite anchor was left out; remembered tracks were dropped at the capacity 2 * max_tracks; events beyond max_events were not
        stored) and the step counter of its first event."""
        if self._state is None:
            return
        with torch.cuda.device(self.device):
            cur = self._enter(self.device)
            status = self._status.cpu().numpy()
            if not status[:, 0].any():
                return
            self._status.zero_()
            self._stream = cur
        said = []
        for s in np.flatnonzero(status[:, 0]).tolist():
            code, step = int(status[s, 0]), int(status[s, 1])
            what = ["a non-finite anchor (the row was left out)"] if code & STATUS_NON_FINITE else []
            what += [f"capacity (remembered tracks dropped at {2 * self.max_tracks})"] if code & STATUS_CAPACITY else []
            what += [f"event overflow (more than max_events = {self.max_events} in a step)"] if code & STATUS_EVENTS else []
            said.append(f"stream {s}: {' and '.join(what)}, first at step {step}")
        raise ValueError("ZoneCounter: " + "; ".join(said))
