"""The rule of cnl_track_zones_f64 (include/centernet_gfx950.h, csrc/track_zones.hip) restated in numpy float64: zone membership, line
crossings, identity across steps, events.  `ZoneCounterRef` has ZoneCounter's constructor and `update`, on host arrays; every output is held
equal to the device's, call by call, as integers and bit patterns.  Every float64 operation below is one numpy operation — one rounding, as in
the kernel, which is built without contraction."""
import numpy as np

ENTER, EXIT, FORWARD, BACKWARD, DWELL = 1, 2, 3, 4, 5


# ------------------------------------------------------------------------------------------------------------------- the two predicates
def inside_polygon(vertices, px, py):
    """Even-odd rule without a division.  vertices: n (x, y) pairs; px, py: float64 arrays (or scalars) -> bool of their shape."""
    v = np.asarray(vertices, np.float64)
    px, py = np.asarray(px, np.float64), np.asarray(py, np.float64)
    inside = np.zeros(px.shape, bool)
    n = len(v)
    for i in range(n):
        xi, yi = v[i]
        xj, yj = v[(i + 1) % n]
        straddles = (yi > py) != (yj > py)
        t = (xj - xi) * (py - yi) - (px - xi) * (yj - yi)
        inside ^= straddles & ((t > 0) if yj > yi else (t < 0))
    return inside


def cross(ux, uy, vx, vy):
    return ux * vy - uy * vx


def line_crossing(a, b, p0x, p0y, p1x, p1y):
    """The segment p0 -> p1 against the directed line a -> b -> 0 (none), FORWARD or BACKWARD, of the points' shape."""
    ax, ay, bx, by = np.float64(a[0]), np.float64(a[1]), np.float64(b[0]), np.float64(b[1])
    p0x, p0y, p1x, p1y = (np.asarray(x, np.float64) for x in (p0x, p0y, p1x, p1y))
    dx, dy = bx - ax, by - ay
    d0 = cross(dx, dy, p0x - ax, p0y - ay) > 0
    d1 = cross(dx, dy, p1x - ax, p1y - ay) > 0
    sx, sy = p1x - p0x, p1y - p0y
    e0 = cross(sx, sy, ax - p0x, ay - p0y) > 0
    e1 = cross(sx, sy, bx - p0x, by - p0y) > 0
    hit = (d0 != d1) & (e0 != e1)
    return np.where(hit, np.where(d1, FORWARD, BACKWARD), 0)


def anchors(boxes, anchor):
    """boxes [n, 4] of any float type -> (px, py) float64, computed on the widened values."""
    b = np.asarray(boxes).astype(np.float64)
    px = (b[:, 0] + b[:, 2]) * 0.5
    py = b[:, 3].copy() if anchor == "bottom_center" else (b[:, 1] + b[:, 3]) * 0.5
    return px, py


# ------------------------------------------------------------------------------------------------------------------- the counter
def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def _per_stream(items, S):
    items = [] if items is None else list(items)
    if items and all(isinstance(x, (list, tuple)) for x in items):
        assert len(items) == S
        return [list(x) for x in items]
    return [list(items) for _ in range(S)]


class ZoneCounterRef:
    """zones: objects with .vertices, .labels (a tuple, empty: every label) and .dwell_alert; lines: objects with .a, .b and .labels — the
    package's Zone and Line are such objects.  The lists have ZoneCounter's two forms."""

    def __init__(self, num_streams, zones=None, lines=None, max_tracks=256, anchor="bottom_center", max_absent=30, max_events=64, device=None):
        S = self.num_streams = num_streams
        self.zones, self.lines = _per_stream(zones, S), _per_stream(lines, S)
        self.Z, self.Ln = max(len(z) for z in self.zones), max(len(l) for l in self.lines)
        self.max_tracks, self.anchor, self.max_absent, self.max_events = max_tracks, anchor, max_absent, max_events
        self.status = np.zeros((S, 2), np.int32)        # sticky: bits, the step of the first event
        self.step_no = 0
        self.reset()

    def reset(self, stream=None):
        S, Z, Ln = self.num_streams, self.Z, self.Ln
        if stream is None:
            self.entries = [[] for _ in range(S)]       # dicts: id, x, y, inside, dwell [Z], age
            self.zone_counts, self.line_counts = np.zeros((S, Z, 2), np.int64), np.zeros((S, Ln, 2), np.int64)
        else:
            self.entries[stream] = []
            self.zone_counts[stream] = 0
            self.line_counts[stream] = 0

    def totals(self):
        return {"zone_counts": self.zone_counts.copy(), "line_counts": self.line_counts.copy()}

    def remembered_inside(self, s):
        """[Z]: the absent entries of stream s that are remembered inside each zone."""
        return np.array([sum(1 for e in self.entries[s] if e["age"] > 0 and (e["inside"] >> z) & 1) for z in range(self.Z)], np.int64)

    def update(self, tracks, streams=None):
        boxes, ids, labels, count = (_host(tracks[k]) for k in ("bboxes", "track_ids", "labels", "count"))
        S, Z, Ln, K = self.num_streams, self.Z, self.Ln, self.max_events
        live = list(range(S)) if streams is None else [int(s) for s in streams]
        L, M = boxes.shape[0], boxes.shape[1]
        assert L == len(live) and M <= self.max_tracks
        out = {"inside": np.zeros((L, M), np.int32), "dwell": np.zeros((L, M, Z), np.int32), "occupancy": np.zeros((L, Z), np.int32),
               "zone_counts": np.zeros((L, Z, 2), np.int64), "line_counts": np.zeros((L, Ln, 2), np.int64),
               "events": np.zeros((L, K, 4), np.int64), "event_count": np.zeros((L,), np.int32)}
        for i, s in enumerate(live):
            bits, events = self._step_stream(s, boxes[i], ids[i], labels[i], int(np.clip(count[i], 0, M)), out, i)
            if len(events) > K:
                bits |= 4
            out["event_count"][i] = len(events)
            for k, ev in enumerate(events[:K]):
                out["events"][i, k] = ev
            out["zone_counts"][i], out["line_counts"][i] = self.zone_counts[s], self.line_counts[s]
            if bits:
                if self.status[s, 0] == 0:
                    self.status[s, 1] = self.step_no & 0x7fffffff
                self.status[s, 0] |= bits
        self.step_no += 1
        return out

    def _step_stream(self, s, boxes, ids, labels, n, out, i):
        Z = self.Z
        zones, lines, prev = self.zones[s], self.lines[s], self.entries[s]
        with np.errstate(invalid="ignore", over="ignore"):
            px, py = anchors(boxes[:n], self.anchor)
        present = np.isfinite(px) & np.isfinite(py)
        bits = 0 if present.all() else 1
        member = np.zeros((n, Z), bool)
        with np.errstate(invalid="ignore", over="ignore"):
            for z, zone in enumerate(zones):
                ok = np.isin(labels[:n], zone.labels) if len(zone.labels) else np.ones(n, bool)
                member[:, z] = present & ok & inside_polygon(zone.vertices, px, py)
        taken, events, new = set(), [], []
        for r in range(n):
            if not present[r]:
                continue
            tid, label = int(ids[r]), int(labels[r])
            e = next((j for j, old in enumerate(prev) if old["id"] == tid), None)
            old = prev[e] if e is not None else None
            if e is not None:
                taken.add(e)
            was = old["inside"] if old else 0
            entry = {"id": tid, "x": px[r], "y": py[r], "inside": 0, "dwell": [0] * Z, "age": 0}
            for z, zone in enumerate(zones):
                inside, before = bool(member[r, z]), bool((was >> z) & 1)
                if inside:
                    entry["dwell"][z] = (old["dwell"][z] if before else 0) + 1
                    entry["inside"] |= 1 << z
                    out["occupancy"][i, z] += 1
                if before and not inside:
                    events.append((tid, EXIT, z, old["dwell"][z]))
                    self.zone_counts[s, z, 1] += 1
                if inside and not before:
                    events.append((tid, ENTER, z, 1 if old is None else 0))
                    self.zone_counts[s, z, 0] += 1
                if inside and zone.dwell_alert > 0 and entry["dwell"][z] == zone.dwell_alert:
                    events.append((tid, DWELL, z, entry["dwell"][z]))
            if old is not None:
                for l, line in enumerate(lines):
                    if len(line.labels) and label not in line.labels:
                        continue
                    with np.errstate(invalid="ignore", over="ignore"):
                        kind = int(line_crossing(line.a, line.b, old["x"], old["y"], px[r], py[r]))
                    if kind:
                        events.append((tid, kind, l, 0))
                        self.line_counts[s, l, kind - FORWARD] += 1
            out["inside"][i, r] = entry["inside"]
            out["dwell"][i, r] = entry["dwell"]
            new.append(entry)
        for j, old in enumerate(prev):
            if j in taken:
                continue
            age = old["age"] + 1
            if age > self.max_absent:
                for z in range(Z):
                    if (old["inside"] >> z) & 1:
                        events.append((old["id"], EXIT, z, old["dwell"][z]))
                        self.zone_counts[s, z, 1] += 1
            else:
                new.append(dict(old, age=age))
        cap = 2 * self.max_tracks
        if len(new) > cap:
            bits |= 2
            new = new[:cap]
        self.entries[s] = new
        return bits, events


# ------------------------------------------------------------------------------------------------------------------- a scene for the tests
def walk_scene(seed, S, steps, M, objects, dtype=np.float32, p_hide=0.08, longest=4, stride=0.09):
    """Seeded random walks: `objects` (<= M) tracks per stream wander over [-0.1, 1.1]^2, are hidden now and then for 1..longest steps, and come
    out in a row order that is permuted every step.  -> a list over the steps of dicts of host arrays shaped like a device life-cycle step's:
    bboxes [S, M, 4] `dtype`, track_ids / labels [S, M] int64, count [S] int32.  Rows from count on hold junk the counter must not read."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0.0, 1.0, (S, objects, 2))
    hidden = np.zeros((S, objects), np.int64)
    out = []
    for _ in range(steps):
        pos += rng.normal(0.0, stride, pos.shape)
        pos = np.where(pos < -0.1, -0.2 - pos, pos)
        pos = np.where(pos > 1.1, 2.2 - pos, pos)
        hidden = np.where(hidden > 0, hidden - 1, np.where(rng.random(hidden.shape) < p_hide, rng.integers(1, longest + 1, hidden.shape), 0))
        boxes = rng.uniform(-1.0, 2.0, (S, M, 4))
        ids = np.full((S, M), -7, np.int64)
        labels = np.full((S, M), 1, np.int64)
        count = np.zeros(S, np.int32)
        for s in range(S):
            seen = rng.permutation(np.flatnonzero(hidden[s] == 0))
            n = count[s] = len(seen)
            w, h = 0.04 + 0.01 * (seen % 3), 0.1 + 0.02 * (seen % 2)
            cx, cy = pos[s, seen, 0], pos[s, seen, 1]
            boxes[s, :n] = np.stack([cx - w, cy - h, cx + w, cy], 1)
            ids[s, :n] = 1000 * s + seen + 1
            labels[s, :n] = seen % 3
        out.append({"bboxes": boxes.astype(dtype), "track_ids": ids, "labels": labels, "count": count})
    return out


# Geometry in multiples of 1/64 (exact in float32, and so are the anchors of boxes built around such points): a triangle, a concave 7-gon
# with a horizontal edge and a 16-gon.
TRIANGLE = [(8 / 64, 8 / 64), (40 / 64, 8 / 64), (8 / 64, 40 / 64)]
HEPTAGON = [(16 / 64, 16 / 64), (56 / 64, 16 / 64), (56 / 64, 56 / 64), (40 / 64, 40 / 64), (32 / 64, 56 / 64), (24 / 64, 40 / 64), (16 / 64, 56 / 64)]
HEXADECAGON = [(float(np.rint(32 + 22 * np.cos(k * np.pi / 8))) / 64, float(np.rint(32 + 22 * np.sin(k * np.pi / 8))) / 64) for k in range(16)]
LINE_H = (0.0, 0.5, 1.0, 0.5)
LINE_V = (0.5, 56 / 64, 0.5, 8 / 64)


def pinned_points():
    """Anchors that sit exactly on the geometry above: every vertex, every edge midpoint (multiples of 1/128), points of the horizontal
    edges, the lines' endpoints and points on them."""
    pts = []
    for poly in (TRIANGLE, HEPTAGON, HEXADECAGON):
        for i, (x, y) in enumerate(poly):
            u, v = poly[(i + 1) % len(poly)]
            pts += [(x, y), ((x + u) / 2, (y + v) / 2)]
    pts += [(20 / 64, 8 / 64), (30 / 64, 16 / 64), (50 / 64, 16 / 64), (0.0, 0.5), (1.0, 0.5), (0.25, 0.5), (0.5, 0.5), (0.5, 56 / 64), (0.5, 8 / 64),
            (0.5, 0.25)]
    return pts


def pinned_scene(seed, S, steps, M, objects, max_absent, dtype=np.float32, anchor="bottom_center"):
    """`objects` (<= M) tracks per stream jump between pinned_points() and points of the 1/64 grid; the rows are permuted every step.  Object 0
    is away for one step, object 1 for max_absent steps, object 2 for max_absent + 1 steps, and each comes back on the other side of
    LINE_H; object 3 keeps to the middle of the 16-gon, object 4 stands still; the others hide now and then.  Labels are object % 3.
    -> the steps' dicts of host arrays, as walk_scene's."""
    assert objects >= 6 and steps >= 16 + 2 * max_absent
    rng = np.random.default_rng(seed)
    pool = pinned_points()
    away = {0: (5, 1), 1: (8, max_absent), 2: (10 + max_absent, max_absent + 1)}        # object -> (first step away, steps away)
    out = []
    for f in range(steps):
        boxes = rng.uniform(-1.0, 2.0, (S, M, 4))
        ids, labels, count = np.full((S, M), -7, np.int64), np.full((S, M), 1, np.int64), np.zeros(S, np.int32)
        for s in range(S):
            rows = []
            for o in range(objects):
                x, y = pool[rng.integers(len(pool))] if rng.random() < 0.6 else tuple(rng.integers(0, 65, 2) / 64)
                if o in away:
                    start, length = away[o]
                    if start <= f < start + length:
                        continue
                    if f == start - 1:
                        x, y = 20 / 64, 24 / 64                     # above LINE_H on the screen, inside the triangle and the 7-gon
                    if f == start + length:
                        x, y = 20 / 64, 44 / 64                     # below it
                elif o == 3:
                    x, y = (30 + rng.integers(0, 5)) / 64, (30 + rng.integers(0, 5)) / 64
                elif o == 4:
                    x, y = 36 / 64, 24 / 64
                elif rng.random() < 0.15:
                    continue
                rows.append((o, x, y))
            order = rng.permutation(len(rows))
            count[s] = len(rows)
            for r, j in enumerate(order):
                o, x, y = rows[j]
                w, h = (2 + o % 3) / 64, (4 + o % 2) / 64
                boxes[s, r] = (x - w, y - 2 * h, x + w, y) if anchor == "bottom_center" else (x - w, y - h, x + w, y + h)
                ids[s, r], labels[s, r] = 100 * s + o + 1, o % 3
        out.append({"bboxes": boxes.astype(dtype), "track_ids": ids, "labels": labels, "count": count})
    return out
