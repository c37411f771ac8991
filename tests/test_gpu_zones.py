"""GPU: ZoneCounter / cnl_track_zones_f64 (csrc/track_zones.hip) held equal to tests/zones_ref.py after every call — every output and the
sticky status words, as integers — at the smallest shapes where the kernel can go wrong: per-stream geometry of different sizes, anchors
exactly on vertices, edges and horizontal edges, permuted rows, absences of 1, max_absent and max_absent + 1 steps, label filters, dwell
alerts, float32 / float64 boxes and both anchors; more than a wave of tracks; the two overflows; non-finite boxes; partial steps and resets;
non-default streams; no host synchronisation; the C ABI inside guard bytes; and a real TrackerBank(lifecycle="device") chained into it."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import strided_io
import tracker_ref
import zones_ref as zr
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, zones

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, M, STEPS, MAX_ABSENT = 3, 8, 30, 2
KEYS = ("inside", "dwell", "occupancy", "zone_counts", "line_counts", "events", "event_count")
DTYPES = {"inside": torch.int32, "dwell": torch.int32, "occupancy": torch.int32, "zone_counts": torch.int64, "line_counts": torch.int64,
          "events": torch.int64, "event_count": torch.int32}


def geometry():
    """Z = 3 and Ln = 2 as padded maxima over streams whose own lists differ in size."""
    tri, hept = cl.Zone(zr.TRIANGLE, dwell_alert=2), cl.Zone(zr.HEPTAGON, labels=[0, 2])
    gon = cl.Zone(zr.HEXADECAGON, dwell_alert=3)
    lh, lv = cl.Line(*zr.LINE_H), cl.Line(*zr.LINE_V, labels=[1, 2])
    return dict(zones=[[tri, hept, gon], [hept], [gon, tri]], lines=[[lh, lv], [], [lv]])


def pair(num_streams=S, max_tracks=M, **kw):
    kw = {"max_absent": MAX_ABSENT, **geometry(), **kw}
    return cl.ZoneCounter(num_streams, max_tracks=max_tracks, device=DEV, **kw), zr.ZoneCounterRef(num_streams, max_tracks=max_tracks, **kw)


def to_dev(tracks, idx=None):
    return {k: torch.from_numpy(v if idx is None else np.ascontiguousarray(v[idx])).to(DEV) for k, v in tracks.items()}


def rows(tracks, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in tracks.items()}


def same(got, want, where):
    assert set(got) == set(KEYS)
    for key in KEYS:
        g = got[key].cpu().numpy()
        assert got[key].dtype == DTYPES[key] and g.dtype == want[key].dtype and g.shape == want[key].shape, (where, key, g.dtype, g.shape)
        assert np.array_equal(g, want[key]), (where, key, g.tolist(), want[key].tolist())


def same_status(zc, ref, where):
    assert np.array_equal(zc._status.cpu().numpy(), ref.status), (where, zc._status.tolist(), ref.status.tolist())


_scenes = {}


def scene(dtype=np.float32, anchor="bottom_center"):
    key = (np.dtype(dtype).name, anchor)
    if key not in _scenes:
        _scenes[key] = zr.pinned_scene(3, S, STEPS, M, objects=7, max_absent=MAX_ABSENT, dtype=dtype, anchor=anchor)
    return _scenes[key]


# ----------------------------------------------------------------------------------------------------------------------- the base shape
@pytest.mark.parametrize("anchor", ["bottom_center", "center"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_call_equals_the_restatement(dtype, anchor):
    zc, ref = pair(anchor=anchor)
    kinds, expired, returned, on_geometry = set(), 0, 0, 0
    pinned = set(zr.pinned_points())
    for f, tracks in enumerate(scene(dtype, anchor)):
        want = ref.update(tracks)
        same(zc.update(to_dev(tracks)), want, f)
        same_status(zc, ref, f)
        for s in range(S):
            n = min(int(want["event_count"][s]), want["events"].shape[1])
            evs = want["events"][s, :n].tolist()
            kinds |= {e[1] for e in evs}
            present = set(tracks["track_ids"][s, :tracks["count"][s]].tolist())
            expired += sum(1 for e in evs if e[1] == zr.EXIT and e[0] not in present)
            returned += sum(1 for e in evs if e[1] in (zr.FORWARD, zr.BACKWARD) and e[0] % 100 in (1, 2) and e[2] == 0)
            px, py = zr.anchors(tracks["bboxes"][s, :tracks["count"][s]], anchor)
            on_geometry += sum((x, y) in pinned for x, y in zip(px.tolist(), py.tolist()))
    # the scene did what it is for: every kind of event, exits of forgotten tracks, crossings made while away, anchors exactly on the geometry
    assert kinds == {1, 2, 3, 4, 5} and expired >= S and returned >= 2 and on_geometry > 100
    t = zc.totals()
    assert np.array_equal(t["zone_counts"], ref.zone_counts) and np.array_equal(t["line_counts"], ref.line_counts) and t["zone_counts"].sum() > 50
    assert not ref.status.any()
    zc.check()


def test_more_than_a_wave_of_tracks_per_stream():
    """max_tracks = 128, about 100 present tracks: the ranks cross wave boundaries, the id walk goes beyond 64 entries, the list holds hidden tracks."""
    zc, ref = pair(2, 128, zones=[cl.Zone(zr.TRIANGLE), cl.Zone(zr.HEPTAGON, dwell_alert=2), cl.Zone(zr.HEXADECAGON, labels=[1])],
                   lines=[cl.Line(*zr.LINE_H), cl.Line(*zr.LINE_V)], max_events=512)
    most = remembered = 0
    for f, tracks in enumerate(zr.walk_scene(5, 2, 8, 128, objects=110, p_hide=0.1)):
        want = ref.update(tracks)
        same(zc.update(to_dev(tracks)), want, f)
        most, remembered = max(most, int(tracks["count"].min())), max(remembered, max(len(e) for e in ref.entries))
        assert int(want["event_count"].max()) <= 512
    assert most > 64 and remembered > 100 and int(want["event_count"].min()) >= 32
    same_status(zc, ref, "end")
    zc.check()


def test_events_beyond_max_events_are_counted_not_stored():
    zc, ref = pair(max_events=4)
    over = 0
    for f, tracks in enumerate(scene()[:12]):
        want = ref.update(tracks)
        same(zc.update(to_dev(tracks)), want, f)
        over += int((want["event_count"] > 4).sum())
    assert over >= 3 and (ref.status[:, 0] & 4).any()
    same_status(zc, ref, "end")
    with pytest.raises(ValueError, match=r"stream 0: event overflow \(more than max_events = 4 in a step\), first at step 0"):
        zc.check()
    zc.check()                  # reported once: the words were cleared


def test_the_list_overflows_at_twice_max_tracks():
    zc, ref = pair(1, M, zones=[cl.Zone(zr.HEPTAGON)], lines=[cl.Line(*zr.LINE_H)], max_absent=30)
    base = scene()[3]
    for f in range(4):          # eight new ids per step, nobody expires: 8 + 24 remembered > 16
        tracks = rows(base, [0])
        tracks["count"][:] = M
        tracks["track_ids"][0] = np.arange(M) + 1 + 10 * f
        want = ref.update(tracks)
        same(zc.update(to_dev(tracks)), want, f)
        same_status(zc, ref, f)
    assert ref.status.tolist() == [[2, 2]] and len(ref.entries[0]) == 2 * M
    tracks["track_ids"][0] = [31, 21, 11, 1, 32, 22, 12, 2]       # remembered: 31 21 (32 22 too); dropped, so new again: 11 1 12 2
    want = ref.update(tracks)
    same(zc.update(to_dev(tracks)), want, "return")
    with pytest.raises(ValueError, match=r"stream 0: capacity \(remembered tracks dropped at 16\), first at step 2"):
        zc.check()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_non_finite_box_is_left_out_and_reported(dtype):
    zc, ref = pair()
    sc = [{k: v.copy() for k, v in t.items()} for t in scene(dtype)[:6]]
    sc[2]["bboxes"][0, 1, 0] = np.nan           # x1: the anchor's x
    sc[2]["bboxes"][2, 0, 3] = np.inf           # y2: the anchor's y
    sc[3]["bboxes"][0, 0, 1] = np.nan           # y1 alone: not part of a bottom-centre anchor, the row counts
    sc[4]["bboxes"][1, M - 1, :] = np.nan       # beyond count: not read
    sc[4]["count"][1] = min(sc[4]["count"][1], M - 1)
    for f, tracks in enumerate(sc):
        want = ref.update(tracks)
        same(zc.update(to_dev(tracks)), want, f)
    assert ref.status.tolist() == [[1, 2], [0, 0], [1, 2]]
    same_status(zc, ref, "end")
    with pytest.raises(ValueError, match=r"stream 0: a non-finite anchor \(the row was left out\), first at step 2; stream 2: a non-finite anchor"):
        zc.check()


def test_partial_steps_and_resets_in_the_middle_of_a_sequence():
    zc, ref = pair()
    for f, tracks in enumerate(scene()):
        if f == 9:
            zc.reset(1), ref.reset(1)
        if f == 19:
            zc.reset(), ref.reset()
        live = (None, [2, 0], [1], [0, 1, 2], [1, 2])[f % 5]
        if live is None:
            want, got = ref.update(tracks), zc.update(to_dev(tracks))
        else:
            want, got = ref.update(rows(tracks, live), streams=live), zc.update(to_dev(tracks, live), streams=live)
        same(got, want, (f, live))
        same_status(zc, ref, f)
        t = zc.totals()
        assert np.array_equal(t["zone_counts"], ref.zone_counts) and np.array_equal(t["line_counts"], ref.line_counts), f
    assert ref.zone_counts.sum() > 20
    zc.check()


def test_two_alternating_streams_give_the_default_streams_bits():
    sc = scene()[:12]
    dev_in = [to_dev(t) for t in sc]
    plain, _ = pair()
    want = [plain.update(t) for t in dev_in]
    torch.cuda.synchronize()
    zc, _ = pair()
    side = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    got = []
    for f, t in enumerate(dev_in):
        with torch.cuda.stream(side[f % 2]):
            got.append(zc.update(t))
    with torch.cuda.stream(side[0]):
        totals = zc.totals()
    torch.cuda.synchronize()
    for f, (g, w) in enumerate(zip(got, want)):
        for key in KEYS:
            assert torch.equal(g[key], w[key]), (f, key)
    assert np.array_equal(totals["zone_counts"], plain.totals()["zone_counts"])


BLOCKED = [(torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"),
           (torch.Tensor, "numpy")]


def _boom(*a, **kw):
    raise AssertionError("host synchronisation inside a step")


def test_steady_state_calls_never_synchronise(monkeypatch):
    sc = scene()[:14]
    dev_in = [to_dev(t) for t in sc]
    zc, ref = pair()
    for t in dev_in[:4]:        # (the first call allocates the state and uploads the geometry)
        zc.update(t)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        for owner, attr in BLOCKED:
            m.setattr(owner, attr, _boom)
        got = [zc.update(t) for t in dev_in[4:]]
    assert len(got) == 10 and len(zc._live_lists) == 1
    for f, t in enumerate(sc):
        want = ref.update(t)
        if f >= 4:
            same(got[f - 4], want, f)


# ----------------------------------------------------------------------------------------------------------------------- the C ABI
def test_the_entry_writes_inside_its_outputs_and_the_state_block_of_the_queried_size():
    lib = _lib.load()
    kw = {"max_absent": MAX_ABSENT, **geometry()}
    host = cl.ZoneCounter(S, max_tracks=M, **kw)            # the geometry records; it never touches a device
    ref = zr.ZoneCounterRef(S, max_tracks=M, max_events=4, **kw)
    Z, Ln, K, L = host.Z, host.Ln, 4, 2
    live = [2, 0]
    state_bytes = lib.cnl_track_zones_state_bytes(S, M, Z, Ln)
    state = strided_io.GuardedBytes(state_bytes, align=8, device=DEV, name="state")
    status = strided_io.GuardedBytes(8 * S, align=4, device=DEV, name="status")
    state.body.zero_(), status.body.zero_()
    shapes = {"inside": (L, M), "dwell": (L, M, Z), "occupancy": (L, Z), "zone_counts": (L, Z, 2), "line_counts": (L, Ln, 2), "events": (L, K, 4),
              "event_count": (L,)}
    outs = {k: strided_io.GuardedBytes(int(np.prod(shp)) * (8 if DTYPES[k] == torch.int64 else 4), align=8 if DTYPES[k] == torch.int64 else 4,
                                       device=DEV, name=k) for k, shp in shapes.items()}
    geo = torch.from_numpy(host._geometry).to(DEV)
    lv = torch.tensor(live + [1], dtype=torch.int32, device=DEV)
    for f, tracks in enumerate(scene(np.float64)[:10]):
        t = to_dev(tracks, live)
        for g in outs.values():
            g.refill()
        a = _lib.TrackZones(t["bboxes"].data_ptr(), t["track_ids"].data_ptr(), t["labels"].data_ptr(), t["count"].data_ptr(), lv.data_ptr(), geo.data_ptr(),
                            state.ptr, status.ptr, *(outs[k].ptr for k in KEYS), S, L, M, M, Z, Ln, K, MAX_ABSENT, 0, 1, f & 1, f)
        _lib.check(lib.cnl_track_zones_f64(ctypes.byref(a), _lib.stream(torch.device(DEV))), "cnl_track_zones_f64")
        want = ref.update(rows(tracks, live), streams=live)
        for key in KEYS:
            ok, msg = outs[key].verdict()
            assert ok, (f, msg)
            assert np.array_equal(outs[key].result(DTYPES[key], shapes[key]).numpy(), want[key]), (f, key)
        for g in (state, status):
            ok, msg = g.verdict()
            assert ok, (f, msg)
        assert np.array_equal(status.result(torch.int32, (S, 2)).numpy(), ref.status), f
    assert (ref.status[[0, 2], 0] == 4).all() and not ref.status[1].any()
    banks = state.result(torch.uint8).numpy().reshape(2, S, -1)
    assert banks[:, [0, 2]].any() and not banks[:, 1].any()         # stream 1 took no part: its zeros were carried from bank to bank


# ----------------------------------------------------------------------------------------------------------------------- behind a real bank
def test_a_device_bank_chained_into_the_counter_without_a_host_read():
    E, K = 8, 14
    seqs = [tracker_ref.synth_sequence(10 + s, frames=12, objects=5, k=K, emb_dim=E) for s in range(S)]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        bank = cl.TrackerBank(S, device=DEV, lifecycle="device", max_tracks=16, max_inactive_age=6)
    kw = dict(zones=[cl.Zone([(0.1, 0.1), (0.9, 0.1), (0.9, 0.6), (0.1, 0.6)], dwell_alert=3),
                     cl.Zone([(-1.0, -1.0), (2.0, -1.0), (2.0, 2.0), (-1.0, 2.0)], dwell_alert=2)],
              lines=[cl.Line(0.0, 0.5, 1.0, 0.5), cl.Line(0.5, 1.0, 0.5, 0.0)], max_absent=MAX_ABSENT)
    zc, ref = cl.ZoneCounter(S, max_tracks=16, device=DEV, **kw), zr.ZoneCounterRef(S, max_tracks=16, **kw)
    dets = [tuple(torch.from_numpy(np.stack([seq[f][j] for seq in seqs])).to(DEV) for j in range(4)) for f in range(12)]
    torch.cuda.synchronize()
    tracks, outs = [], []
    for f in range(12):             # launches only: nothing is read before the last step is queued
        tracks.append(bank.update_batch(*dets[f]))
        outs.append(zc.update(tracks[-1]))
    events = 0
    for f in range(12):
        want = ref.update({k: v.cpu().numpy() for k, v in tracks[f].items()})
        same(outs[f], want, f)
        events += int(want["event_count"].sum())
    assert events >= 2 * S and int(tracks[-1]["count"].sum()) >= S
    bank.check()
    zc.check()
    frames = torch.from_numpy(np.random.default_rng(3).integers(0, 255, (S, 96, 96, 3), dtype=np.uint8)).to(DEV)
    last = tracks[-1]
    drawn = cl.draw_detections(frames, last["bboxes"] * 96, labels=last["labels"], numbers=last["track_ids"].to(torch.int32), count=last["count"])
    assert drawn.shape == frames.shape and not torch.equal(drawn, frames)
