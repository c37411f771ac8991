"""CPU: zone occupancy, line crossings and dwell events without a device — tests/zones_ref.py (the numpy restatement of cnl_track_zones_f64's
rule): its zone predicate against exact rational arithmetic and on a tiling, its crossing predicate on the pinned edge cases, the invariants
of the counters over seeded random walks, expiry, the two overflows, partial steps and resets; the C-ABI entries (declared, exported, bound,
struct and state sizes, every argument error); ZoneCounter's constructor, from_config and refusals."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import zones_ref as zr
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, zones

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cnl_track_zones_f64", "cnl_track_zones_state_bytes")
SQUARE = [(0.25, 0.25), (0.75, 0.25), (0.75, 0.75), (0.25, 0.75)]
FAR = cl.Line(-10.0, 0.5, 10.0, 0.5)           # no segment of a walk over [-0.1, 1.1]^2 misses its extent


# ----------------------------------------------------------------------------------------------------------------------- the zone predicate
def exact_inside(vertices, px, py):
    """The even-odd rule of the header in exact rational arithmetic."""
    inside, n = False, len(vertices)
    for i in range(n):
        (xi, yi), (xj, yj) = vertices[i], vertices[(i + 1) % n]
        if (yi > py) != (yj > py):
            t = Fraction(xj - xi) * (py - yi) - (px - xi) * Fraction(yj - yi)
            if (t > 0) if yj > yi else (t < 0):
                inside = not inside
    return inside


def test_zone_predicate_agrees_with_exact_arithmetic_on_grid_and_half_grid_points():
    rng = np.random.default_rng(0)
    half = np.arange(-1, 25) / 2.0                                 # -0.5 .. 12, integers and half-integers: 26 x 26 points
    gx, gy = (a.reshape(-1) for a in np.meshgrid(half, half))
    checked = inside_some = 0
    for case in range(28):
        n = 3 + case % 14                                           # 3 .. 16 vertices
        if case % 2:                                                # a star-shaped (mostly concave) polygon around (6, 6)
            ang = np.sort(rng.uniform(0, 2 * np.pi, n))
            rad = rng.uniform(1.5, 6.0, n)
            verts = [(int(round(6 + r * np.cos(a))), int(round(6 + r * np.sin(a)))) for a, r in zip(ang, rad)]
        else:                                                       # any closed chain, self-intersecting ones included: even-odd covers them
            verts = [tuple(int(c) for c in rng.integers(0, 13, 2)) for _ in range(n)]
        got = zr.inside_polygon(verts, gx, gy)
        want = np.array([exact_inside(verts, Fraction(x).limit_denominator(2), Fraction(y).limit_denominator(2)) for x, y in zip(gx.tolist(), gy.tolist())])
        assert np.array_equal(got, want), (case, verts)
        checked += len(gx)
        inside_some += int(got.sum())
    assert checked >= 18000 and inside_some > 1000


def test_every_point_of_a_tiling_lies_in_exactly_one_tile():
    tiles = [[(x, y), (x + 1, y), (x + 1, y + 1), (x, y + 1)] for y in range(4) for x in range(4)]
    tiles += [[(x, y), (x, y + 1), (x + 1, y + 1), (x + 1, y)] for y in range(4) for x in range(4, 6)]          # two columns wound the other way
    q = np.arange(0, 25) / 4.0
    px, py = (a.reshape(-1) for a in np.meshgrid(q[q < 6], q[q < 4]))       # shared edges and corners included; the far outer edges are open
    hits = sum(zr.inside_polygon(t, px, py).astype(np.int64) for t in tiles)
    assert np.array_equal(hits, np.ones_like(hits))
    outer = np.concatenate([zr.inside_polygon(t, np.full(25, 6.0), q) for t in tiles] + [zr.inside_polygon(t, q, np.full(25, 4.0)) for t in tiles])
    assert not outer.any()


def test_a_triangle_sharing_an_oblique_edge_splits_a_square_without_overlap():
    lower, upper = [(0, 0), (4, 0), (4, 4)], [(0, 0), (4, 4), (0, 4)]
    q = np.arange(0, 16) / 4.0
    px, py = (a.reshape(-1) for a in np.meshgrid(q, q))
    hits = zr.inside_polygon(lower, px, py).astype(int) + zr.inside_polygon(upper, px, py).astype(int)
    assert np.array_equal(hits, np.ones_like(hits))


# ----------------------------------------------------------------------------------------------------------------------- the crossing predicate
A, B, C = (0.0, 0.0), (10.0, 0.0), (20.0, 0.0)         # cross(B - A, p - A) = 10 * p.y: the positive side is y > 0


def _kind(a, b, p0, p1):
    return int(zr.line_crossing(a, b, p0[0], p0[1], p1[0], p1[1]))


def test_pinned_line_cases():
    assert _kind(A, B, (5, -1), (5, 1)) == zr.FORWARD and _kind(A, B, (5, 1), (5, -1)) == zr.BACKWARD
    # touch and return from the side where cross <= 0: the line itself belongs to that side, nothing is counted
    assert _kind(A, B, (5, -1), (5, 0)) == 0 and _kind(A, B, (5, 0), (5, -1)) == 0
    # from the other side the touch is a BACKWARD crossing and the return a FORWARD one: two events, net zero
    assert _kind(A, B, (5, 1), (5, 0)) == zr.BACKWARD and _kind(A, B, (5, 0), (5, 1)) == zr.FORWARD
    # exactly through an endpoint: each endpoint belongs to the segment for one direction of travel only
    assert _kind(A, B, (0, -1), (0, 1)) == 0 and _kind(A, B, (10, -1), (10, 1)) == zr.FORWARD
    assert _kind(A, B, (0, 1), (0, -1)) == zr.BACKWARD and _kind(A, B, (10, 1), (10, -1)) == 0
    # a pass beyond the segment on its carrier line, and a walk along the carrier
    assert _kind(A, B, (12, -1), (12, 1)) == 0 and _kind(A, B, (-2, 1), (-2, -1)) == 0
    assert _kind(A, B, (-5, 0), (15, 0)) == 0 and _kind(A, B, (3, 0), (7, 0)) == 0
    # standing still
    assert _kind(A, B, (5, 1), (5, 1)) == 0


@pytest.mark.parametrize("p0, p1, kind", [((10, -1), (10, 1), zr.FORWARD), ((10, 1), (10, -1), zr.BACKWARD), ((9, -1), (11, 1), zr.FORWARD),
                                          ((11, 2), (9, -2), zr.BACKWARD)])
def test_a_crossing_through_the_shared_endpoint_of_a_polyline_counts_once(p0, p1, kind):
    kinds = [_kind(A, B, p0, p1), _kind(B, C, p0, p1)]
    assert sorted(kinds) == [0, kind]


# ----------------------------------------------------------------------------------------------------------------------- the counter
def _tracks(rows, M=8, dtype=np.float32):
    """One stream per list of (id, x, y[, label]) anchors -> a step's dict; boxes are built around a bottom-centre anchor."""
    S = len(rows)
    out = {"bboxes": np.zeros((S, M, 4), dtype), "track_ids": np.zeros((S, M), np.int64), "labels": np.zeros((S, M), np.int64),
           "count": np.zeros(S, np.int32)}
    for s, one in enumerate(rows):
        out["count"][s] = len(one)
        for r, (tid, x, y, *label) in enumerate(one):
            out["bboxes"][s, r] = (x - 0.125, y - 0.25, x + 0.125, y)
            out["track_ids"][s, r] = tid
            out["labels"][s, r] = label[0] if label else 0
    return out


def _events(out, i=0):
    return [tuple(ev) for ev in out["events"][i, :min(int(out["event_count"][i]), out["events"].shape[1])].tolist()]


def test_invariants_over_seeded_random_walks():
    S, steps, M = 3, 200, 8
    zone_list = [cl.Zone(SQUARE, dwell_alert=3), cl.Zone([(0.0, 0.0), (1.0, 0.0), (0.5, 0.5), (1.0, 1.0), (0.0, 1.0)], labels=[0, 2]),
                 cl.Zone([(0.5, -0.5), (1.5, 0.5), (0.5, 1.5)], dwell_alert=1)]
    line_list = [FAR, cl.Line(0.5, 10.0, 0.5, -10.0, labels=[1])]
    ref = zr.ZoneCounterRef(S, zones=zone_list, lines=line_list, max_tracks=M, max_absent=1000, max_events=64)
    scene = zr.walk_scene(11, S, steps, M, objects=6)
    first, last, net = {}, {}, {}
    before = ref.totals()
    seen_kinds = set()
    for f, tracks in enumerate(scene):
        out = ref.update(tracks)
        after = ref.totals()
        for s in range(S):
            evs = _events(out, s)
            assert out["event_count"][s] == len(evs) <= 64
            seen_kinds |= {k for _, k, _, _ in evs}
            alerts = sum(1 for _, k, _, _ in evs if k == zr.DWELL)
            grown = int((after["zone_counts"][s] - before["zone_counts"][s]).sum() + (after["line_counts"][s] - before["line_counts"][s]).sum())
            assert out["event_count"][s] == grown + alerts, (f, s)
            zc = after["zone_counts"][s]
            assert np.array_equal(zc[:, 0] - zc[:, 1], out["occupancy"][s] + ref.remembered_inside(s)), (f, s)
            assert np.array_equal(out["zone_counts"][s], zc) and np.array_equal(out["line_counts"][s], after["line_counts"][s])
            n = int(tracks["count"][s])
            px, py = zr.anchors(tracks["bboxes"][s, :n], "bottom_center")
            for r in range(n):
                tid = int(tracks["track_ids"][s, r])
                side = bool(zr.cross(20.0, 0.0, px[r] + 10.0, py[r] - 0.5) > 0)
                first.setdefault(tid, side)
                last[tid] = side
            for tid, k, idx, _ in evs:
                if idx == 0 and k in (zr.FORWARD, zr.BACKWARD):
                    net[tid] = net.get(tid, 0) + (1 if k == zr.FORWARD else -1)
            assert np.array_equal(out["inside"][s, n:], np.zeros(M - n, np.int32)) and not out["dwell"][s, n:].any()
        before = after
    assert seen_kinds == {1, 2, 3, 4, 5}
    assert len(first) == 18 and any(net.values())
    for tid in first:
        assert net.get(tid, 0) == int(last[tid]) - int(first[tid]), tid
    assert not ref.status.any()


@pytest.mark.parametrize("max_absent", [0, 2])
def test_an_absent_track_expires_after_max_absent_steps_with_its_exit(max_absent):
    def seen_twice_then_absent():
        ref = zr.ZoneCounterRef(1, zones=[cl.Zone(SQUARE)], lines=[FAR], max_tracks=8, max_absent=max_absent)
        out = ref.update(_tracks([[(7, 0.5, 0.4)]]))
        assert _events(out) == [(7, zr.ENTER, 0, 1)] and out["occupancy"][0, 0] == 1
        out = ref.update(_tracks([[(7, 0.5, 0.45)]]))
        assert _events(out) == [] and out["dwell"][0, 0, 0] == 2
        for _ in range(max_absent):
            out = ref.update(_tracks([[]]))
            assert _events(out) == [] and out["occupancy"][0, 0] == 0 and ref.remembered_inside(0)[0] == 1
        return ref

    ref = seen_twice_then_absent()
    out = ref.update(_tracks([[]]))                                 # one step more: forgotten, with the dwell it had
    assert _events(out) == [(7, zr.EXIT, 0, 2)] and ref.entries[0] == [] and ref.zone_counts[0, 0].tolist() == [1, 1]
    ref = seen_twice_then_absent()                                  # back at age max_absent, across the line: the crossing counts, the dwell goes on
    out = ref.update(_tracks([[(7, 0.5, 0.6)]]))
    assert _events(out) == [(7, zr.FORWARD, 0, 0)] and out["dwell"][0, 0, 0] == 3 and ref.line_counts[0, 0].tolist() == [1, 0]


def test_entries_beyond_the_capacity_are_dropped_without_events():
    ref = zr.ZoneCounterRef(1, zones=[cl.Zone(SQUARE)], max_tracks=2, max_absent=30)
    for ids in ((1, 2), (3, 4)):
        ref.update(_tracks([[(i, 0.5, 0.5) for i in ids]], M=2))
    assert [e["id"] for e in ref.entries[0]] == [3, 4, 1, 2] and not ref.status.any()
    out = ref.update(_tracks([[(5, 0.5, 0.5), (6, 0.5, 0.5)]], M=2))
    assert [e["id"] for e in ref.entries[0]] == [5, 6, 3, 4]
    assert ref.status.tolist() == [[2, 2]] and [k for _, k, _, _ in _events(out)] == [zr.ENTER, zr.ENTER]
    assert ref.zone_counts[0, 0].tolist() == [6, 0]


def test_events_beyond_max_events_are_counted_but_not_stored():
    ref = zr.ZoneCounterRef(1, zones=[cl.Zone(SQUARE)], max_tracks=8, max_events=2)
    out = ref.update(_tracks([[(i, 0.5, 0.5) for i in range(1, 6)]]))
    assert out["event_count"][0] == 5 and out["events"][0].tolist() == [[1, 1, 0, 1], [2, 1, 0, 1]]
    assert ref.status.tolist() == [[4, 0]] and ref.zone_counts[0, 0].tolist() == [5, 0] and out["occupancy"][0, 0] == 5


def test_a_stream_that_takes_no_part_is_carried_untouched_and_reset_forgets_one_stream():
    ref = zr.ZoneCounterRef(3, zones=[cl.Zone(SQUARE)], max_tracks=8, max_absent=1)
    ref.update(_tracks([[(1, 0.5, 0.5)], [(2, 0.5, 0.5)], [(3, 0.5, 0.5)]]))
    for _ in range(3):                                              # stream 1 sits out: it does not age, so it does not expire
        out = ref.update(_tracks([[], [(1, 0.5, 0.5)]]), streams=[2, 0])
    assert out["occupancy"].tolist() == [[0], [1]] and out["dwell"][1, 0, 0] == 4
    assert [e["age"] for e in ref.entries[1]] == [0] and ref.entries[2] == [] and ref.zone_counts[:, 0].tolist() == [[1, 0], [1, 0], [1, 1]]
    ref.reset(0)
    assert ref.entries[0] == [] and ref.zone_counts[:, 0].tolist() == [[0, 0], [1, 0], [1, 1]]
    out = ref.update(_tracks([[(1, 0.5, 0.5)]]), streams=[0])
    assert _events(out) == [(1, zr.ENTER, 0, 1)]


def test_a_non_finite_anchor_is_left_out_and_reported():
    ref = zr.ZoneCounterRef(1, zones=[cl.Zone(SQUARE)], max_tracks=8)
    tracks = _tracks([[(1, 0.5, 0.5), (2, 0.5, 0.5)]])
    tracks["bboxes"][0, 0, 2] = np.nan
    out = ref.update(tracks)
    assert out["inside"][0, :2].tolist() == [0, 1] and [e["id"] for e in ref.entries[0]] == [2] and ref.status.tolist() == [[1, 0]]


# ----------------------------------------------------------------------------------------------------------------------- the C ABI
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.cnl_version() == _lib.ABI_VERSION == 13
    assert ctypes.sizeof(_lib.TrackZones) == 168 and "/* 168 bytes */" in header
    assert {"ZoneCounter", "Zone", "Line"} <= set(cl.__all__)
    makefile = open(os.path.join(ROOT, "centernet-lightning_amd", "csrc", "Makefile")).read()
    assert "track_zones.hip" in makefile and "build/track_zones.o: CXXFLAGS += -ffp-contract=off" in makefile
    assert "#pragma clang fp contract(off)" in open(os.path.join(ROOT, "centernet-lightning_amd", "csrc", "track_zones.hip")).read()


@pytest.mark.parametrize("S, T, Z, Ln", [(1, 1, 0, 0), (3, 8, 3, 2), (32, 256, 4, 2), (2, 4096, 16, 16)])
def test_the_state_block_has_the_documented_size(S, T, Z, Ln):
    E = 2 * T
    assert _lib.load().cnl_track_zones_state_bytes(S, T, Z, Ln) == 2 * S * (16 * Z + 16 * Ln + 8 + E * (8 + 16 + 4 + 4 + 4 * Z))


@pytest.mark.parametrize("args", [(0, 8, 1, 1), (70000, 8, 1, 1), (1, 0, 1, 1), (1, 4097, 1, 1), (1, 8, -1, 1), (1, 8, 17, 1), (1, 8, 1, 17)])
def test_the_state_query_answers_zero_outside_the_limits(args):
    assert _lib.load().cnl_track_zones_state_bytes(*args) == 0


def _args(**kw):
    a = _lib.TrackZones()
    for name, _ in _lib.TrackZones._fields_[:15]:
        setattr(a, name, 0x1000)
    a.S, a.L, a.M, a.max_tracks, a.Z, a.Ln, a.max_events, a.max_absent, a.anchor, a.boxes_f64, a.bank, a.step = 3, 3, 8, 8, 3, 2, 64, 30, 0, 0, 0, 0
    for name, v in kw.items():
        setattr(a, name, v)
    return a


BAD = [dict(S=0), dict(S=70000, L=70000), dict(L=0), dict(L=4), dict(M=9), dict(M=0), dict(max_tracks=4097, M=4097), dict(max_tracks=0), dict(Z=17),
       dict(Z=-1), dict(Ln=17), dict(Ln=-1), dict(max_events=0), dict(max_events=65537), dict(max_absent=-1), dict(anchor=2), dict(boxes_f64=2),
       dict(bank=2), dict(bank=-1)] + \
      [{name: None} for name, _ in _lib.TrackZones._fields_[:15]] + \
      [{name: 0x1004} for name in ("track_ids", "labels", "geometry", "state", "zone_counts", "line_counts", "events")] + \
      [{name: 0x1002} for name in ("boxes", "count", "live", "status", "inside", "dwell", "occupancy", "event_count")] + [dict(boxes=0x1004, boxes_f64=1)]


@pytest.mark.parametrize("bad", BAD, ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_the_entry_refuses_bad_arguments_without_a_device(bad):
    rc = _lib.load().cnl_track_zones_f64(ctypes.byref(_args(**bad)), None)
    assert rc == _lib.CNL_E_BAD_ARG, _lib.last_error()
    assert "cnl_track_zones_f64" in _lib.last_error()


def test_the_entry_refuses_a_null_struct_and_lets_unused_outputs_be_null():
    lib = _lib.load()
    assert lib.cnl_track_zones_f64(None, None) == _lib.CNL_E_BAD_ARG and "cnl_track_zones_f64" in _lib.last_error()
    # with Z = 0 / Ln = 0 the arrays of that extent may be null: the refusal that remains is the next one (here: a misaligned pointer)
    rc = lib.cnl_track_zones_f64(ctypes.byref(_args(Z=0, Ln=0, dwell=None, occupancy=None, zone_counts=None, line_counts=None, events=0x1004)), None)
    assert rc == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error()


# ----------------------------------------------------------------------------------------------------------------------- the Python surface
TRI = [(0, 0), (1, 0), (0, 1)]


@pytest.mark.parametrize("make, match", [
    (lambda: cl.Zone([(0, 0), (1, 0)]), "2 vertices"), (lambda: cl.Zone([(i, i * i) for i in range(17)]), "17 vertices"),
    (lambda: cl.Zone([(0, 0), (1, float("nan")), (0, 1)]), "non-finite"), (lambda: cl.Zone([(0, 0), (float("inf"), 0), (0, 1)]), "non-finite"),
    (lambda: cl.Zone([(0, 0, 0), (1, 0, 0), (0, 1, 0)]), "pairs"), (lambda: cl.Zone(TRI, labels=[]), "labels"),
    (lambda: cl.Zone(TRI, labels=list(range(9))), "labels"), (lambda: cl.Zone(TRI, labels=[1.5]), "label"), (lambda: cl.Zone(TRI, dwell_alert=-1), "dwell_alert"),
    (lambda: cl.Line(0.5, 0.5, 0.5, 0.5), "A equals B"), (lambda: cl.Line(0, 0, float("nan"), 1), "non-finite"),
    (lambda: cl.Line(0, 0, 1, 1, labels=list(range(9))), "labels"),
    (lambda: cl.ZoneCounter(2, zones=[cl.Zone(TRI)] * 17), "at most 16 zones"), (lambda: cl.ZoneCounter(2, lines=[cl.Line(0, 0, 1, 1)] * 17), "at most 16 lines"),
    (lambda: cl.ZoneCounter(2, zones=[[cl.Zone(TRI)]]), "per-stream lists"), (lambda: cl.ZoneCounter(2, zones=[cl.Zone(TRI), "door"]), "Zone objects"),
    (lambda: cl.ZoneCounter(2, zones=[[cl.Zone(TRI)], [TRI]]), "Zone objects"),
    (lambda: cl.ZoneCounter(0), "num_streams"), (lambda: cl.ZoneCounter(2, max_tracks=4097), "max_tracks"), (lambda: cl.ZoneCounter(2, max_tracks=0), "max_tracks"),
    (lambda: cl.ZoneCounter(2, anchor="top"), "anchor"), (lambda: cl.ZoneCounter(2, max_absent=-1), "max_absent"),
    (lambda: cl.ZoneCounter(2, max_events=0), "max_events"), (lambda: cl.ZoneCounter(2, device="cpu"), "HIP devices only")])
def test_constructors_refuse_by_name(make, match):
    with pytest.raises(ValueError, match=match):
        make()


def test_geometry_forms_and_records():
    tri, seven = cl.Zone(TRI, labels=[3, 5], dwell_alert=9), cl.Zone([(i, (i * i) % 5) for i in range(7)])
    line = cl.Line(0.0, 0.5, 1.0, 0.25, labels=[2])
    shared = cl.ZoneCounter(2, zones=[tri, seven], lines=[line])
    assert (shared.Z, shared.Ln) == (2, 1) and shared.zones[0] == shared.zones[1] == [tri, seven]
    per = cl.ZoneCounter(3, zones=[[tri], [], [seven, tri, tri]], lines=[[], [line, line], []])
    assert (per.Z, per.Ln) == (3, 2) and [len(z) for z in per.zones] == [1, 0, 3]
    rec = per._geometry
    assert rec.shape == (3, 8 + 336 * 3 + 104 * 2) and rec[:, :8].view(np.int32).tolist() == [[1, 0], [0, 2], [3, 0]]
    z0 = rec[0, 8:8 + 336]
    assert z0[:16].view(np.int32).tolist() == [3, 9, 2, 0] and z0[16:80].view(np.int64).tolist() == [3, 5, 0, 0, 0, 0, 0, 0]
    assert z0[80:].view(np.float64)[:8].tolist() == [0, 0, 1, 0, 0, 1, 0, 0]
    assert not rec[1, 8:8 + 336 * 3].any()                          # padding zones: no vertices, nothing is inside them
    l1 = rec[1, 8 + 336 * 3 + 104:]
    assert l1[:32].view(np.float64).tolist() == [0.0, 0.5, 1.0, 0.25] and l1[32:40].view(np.int32).tolist() == [1, 0] and l1[40:48].view(np.int64)[0] == 2
    empty = cl.ZoneCounter(2)
    assert (empty.Z, empty.Ln) == (0, 0) and empty.totals()["zone_counts"].shape == (2, 0, 2)
    empty.check()
    empty.reset()
    empty.reset(1)
    with pytest.raises(ValueError, match="streams="):
        empty.reset(2)


def test_from_config_takes_a_plain_dict():
    section = {"zones": [{"vertices": SQUARE, "labels": [0], "dwell_alert": 25}, [[0, 0], [1, 0], [0, 1]]],
               "lines": [{"ax": 0.0, "ay": 0.5, "bx": 1.0, "by": 0.5}, [0.5, 0.0, 0.5, 1.0]], "max_tracks": 64, "anchor": "center", "max_absent": 5,
               "max_events": 16}
    zc = cl.ZoneCounter.from_config(section, 4)
    assert (zc.num_streams, zc.Z, zc.Ln, zc.max_tracks, zc.anchor, zc.max_absent, zc.max_events) == (4, 2, 2, 64, "center", 5, 16)
    assert zc.zones[3][0].labels == (0,) and zc.zones[3][0].dwell_alert == 25 and zc.zones[0][1].vertices == ((0.0, 0.0), (1.0, 0.0), (0.0, 1.0))
    assert zc.lines[2][1].a == (0.5, 0.0) and zc.lines[2][1].b == (0.5, 1.0)
    assert "zones" in section and len(section) == 6                 # the caller's dict is not consumed
    per = cl.ZoneCounter.from_config({"zones": [[SQUARE], []], "lines": [[], [[0, 0, 1, 1]]]}, 2)
    assert [len(z) for z in per.zones] == [1, 0] and [len(l) for l in per.lines] == [0, 1]
    with pytest.raises(ValueError, match="A equals B"):
        cl.ZoneCounter.from_config({"lines": [[0, 0, 0, 0]]}, 1)
    with pytest.raises(TypeError):
        cl.ZoneCounter.from_config({"zones": [SQUARE], "no_such_setting": 1}, 1)


def test_update_refuses_host_arrays_and_a_dict_that_is_not_a_steps():
    zc = cl.ZoneCounter(1, zones=[cl.Zone(SQUARE)], max_tracks=8)
    with pytest.raises(ValueError, match="host arrays are refused"):
        zc.update(_tracks([[(1, 0.5, 0.5)]]))
    with pytest.raises(ValueError, match="host arrays are refused"):
        zc.update({k: torch.from_numpy(v) for k, v in _tracks([[(1, 0.5, 0.5)]]).items()})
    with pytest.raises(ValueError, match="expected the dict"):
        zc.update({"bboxes": None})
    assert zones.MAX_ZONES == zones.MAX_LINES == zones.MAX_VERTICES == 16 and zones.MAX_LABELS == 8
