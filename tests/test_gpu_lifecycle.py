"""GPU: TrackerBank(lifecycle="device") — the track life cycle on the device (csrc/track_lifecycle.hip).

Yardstick: a TrackerBank with lifecycle="host" on the same device, given the same detection tensors step by step.  After every step the device
bank's snapshot (ids, states, ages, labels, reported boxes, counters), the live rows of its tables (emb, box, kx, kP), its returned tensors and
its match lists are EQUAL (floats: bit-equal) to the host bank's tracks, table rows, `_active()` lists and match lists.  The capacity and
skipped-stream rules, where the host path does something else by design, are held to tests/lifecycle_ref.py fed with the device's own records."""
import warnings

import numpy as np
import pytest
import torch

import byte_ref
import gate_ref
import lifecycle_ref as lr
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _track_host as th

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, E, M, STEPS = 3, 8, 16, 30
KAL = dict(use_kalman=True, kalman="device")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def _bank(lifecycle, S=S, max_tracks=M, **kw):
    """max_inactive_age = 6: in 30 steps INACTIVE tracks do get deleted, and a stream of five or six objects stays below max_tracks = 16
    (test_every_step... ends with check(): no births were dropped)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cl.TrackerBank(S, device=DEV, lifecycle=lifecycle, max_tracks=max_tracks, max_inactive_age=6, **kw)


def _plain(seed, k=14, sort_scores=True, frames=STEPS, objects=5):
    return tracker_ref.synth_sequence(seed, frames=frames, objects=objects, k=k, emb_dim=E, sort_scores=sort_scores)


def _scene(per_stream):
    """per_stream: S sequences of (boxes, labels, scores, embeddings) -> per step the four [S, k, ...] device tensors."""
    out = []
    for f in range(len(per_stream[0])):
        out.append(tuple(torch.from_numpy(np.stack([seq[f][j] for seq in per_stream])).to(DEV) for j in range(4)))
    torch.cuda.synchronize()
    return out


SCENES = {
    "plain": (lambda: [_plain(10 + s) for s in range(S)], {}),
    "unsorted": (lambda: [_plain(20 + s, sort_scores=False) for s in range(S)], {}),
    "low": (lambda: [byte_ref.synth_occlusion(30 + s, frames=STEPS, objects=6, k=16, emb_dim=E)[0] for s in range(S)], dict(low_threshold=0.1)),
    "kalman": (lambda: [_plain(40 + s) for s in range(S)], KAL),
    "gated": (lambda: [gate_ref.crossing_scene(frames=STEPS, k=12, emb_dim=E, seed=5 + s)[0] for s in range(S)],
              dict(class_aware=True, motion_gate=True, **KAL)),
    "no_box": (lambda: [_plain(50 + s) for s in range(S)], dict(box_cost=None)),
}
_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = _scene(SCENES[name][0]())
    return _scenes[name], SCENES[name][1]


def sub(det, idx):
    return tuple(t[idx].contiguous() for t in det)


def compare(host, dev, out, live, where, skipped=()):
    """The device bank against the host bank, every stream; `out`: the device step's tensors for slots `live` (None: state only); `skipped`:
    streams whose record holds no lists (the host bank kept its earlier ones)."""
    n = host.num_streams
    streams = list(range(n))
    snap = dev.snapshot()
    d = dev._download()
    kal = host._device_kalman
    assert snap["offsets"].tolist() == host._off.tolist(), where
    assert snap["next_track_id"].tolist() == [host[s].next_track_id for s in range(n)], where
    for s in streams:
        r0, r1 = int(host._off[s]), int(host._off[s + 1])
        tracks = host[s].tracks
        assert snap["track_ids"][r0:r1].tolist() == [t.track_id for t in tracks], (where, s)
        assert snap["states"][r0:r1].tolist() == [t.state.value for t in tracks], (where, s)
        assert snap["birth_age"][r0:r1].tolist() == [t.birth_age for t in tracks] and snap["inactive_age"][r0:r1].tolist() == [t.inactive_age for t in tracks]
        assert snap["labels"][r0:r1].tolist() == [int(t.label) for t in tracks], (where, s)
        dt = np.float64 if kal else np.float32
        assert snap["bboxes"].dtype == dt and all(np.asarray(t.bbox).dtype == dt for t in tracks)
        assert np.array_equal(_bits(snap["bboxes"][r0:r1]), _bits(np.asarray([t.bbox for t in tracks], dt).reshape(-1, 4))), (where, s)
        if r1 > r0:
            for name, key in (("emb", "embeddings"), ("box", "table_boxes")) + ((("kx", "kx"), ("kP", "kP")) if kal else ()):
                assert np.array_equal(_bits(getattr(host._table, name)[r0:r1].cpu().numpy()), _bits(snap[key][r0:r1])), (where, s, name)
        if s not in skipped:
            assert dev.last_matches[s] == host.last_matches[s], (where, s)
            assert dev.last_low_matches[s] == host.last_low_matches[s], (where, s)
        assert d["trk_off"][s + 1] - d["trk_off"][s] == r1 - r0
    if out is not None:
        compare_outputs(host, dev, out, live, where)


def compare_outputs(host, dev, out, live, where):
    """The step's tensors against _active() of the host bank."""
    kal = host._device_kalman
    got = {key: v.cpu().numpy() for key, v in out.items()}
    assert got["bboxes"].dtype == (np.float64 if kal else np.float32) and got["track_ids"].dtype == np.int64 and got["labels"].dtype == np.int64
    assert got["count"].dtype == np.int32 and got["bboxes"].shape == (len(live), dev.max_tracks, 4)
    for i, s in enumerate(live):
        act = [t for t in host[s].tracks if t.active]               # what _active() lists on the host path
        c = len(act)
        assert got["count"][i] == c and got["track_ids"][i, :c].tolist() == [t.track_id for t in act], (where, s)
        assert np.array_equal(_bits(got["bboxes"][i, :c]), _bits(np.asarray([t.bbox for t in act], got["bboxes"].dtype).reshape(-1, 4))), (where, s)
        assert got["labels"][i, :c].tolist() == [int(t.label) for t in act]
        assert not got["bboxes"][i, c:].any() and not got["track_ids"][i, c:].any() and not got["labels"][i, c:].any()


@pytest.mark.parametrize("name", list(SCENES))
def test_every_step_equals_the_host_bank(name):
    dets, kw = scene(name)
    host, dev = _bank("host", **kw), _bank("device", **kw)
    seen = {"rows": 0, "low": 0, "active": 0}
    for f, det in enumerate(dets):
        assert host.update_batch(*det) is None
        out = dev.update_batch(*det)
        compare(host, dev, out, list(range(S)), (name, f))
        seen["rows"] = max(seen["rows"], int(host._off[S]))
        seen["low"] += sum(len(m or ()) for m in host.last_low_matches)
        seen["active"] += int(out["count"].sum())
    dev.check()                                         # no stream was skipped, none overflowed
    assert seen["rows"] >= 3 * S and seen["active"] > 10 * S and (name != "low" or seen["low"] > 0)
    # the Track-like records of one download
    for s in range(S):
        for a, b in zip(dev[s].tracks, host[s].tracks):
            assert (a.track_id, a.state, a.birth_age, a.inactive_age, a.label, a.active) == (b.track_id, b.state, b.birth_age, b.inactive_age, int(b.label), b.active)
            assert np.array_equal(_bits(a.embedding), _bits(b.embedding)) and np.array_equal(_bits(a.bbox), _bits(np.asarray(b.bbox)))
            if host._device_kalman:
                assert np.array_equal(_bits(a.kf.x), _bits(b.kf.x)) and np.array_equal(_bits(a.kf.P), _bits(b.kf.P))
            else:
                assert a.kf is None
        assert dev[s].next_track_id == host[s].next_track_id
        assert torch.equal(dev.track_embeddings(s), host.track_embeddings(s))


def test_rows_detections_and_pairs_beyond_one_wave():
    """k = 70 detections, up to 128 rows per stream: every loop of the three kernels runs more than one round of 64 lanes."""
    k, objects, steps = 70, 68, 12
    dets = _scene([_plain(60 + s, k=k, frames=steps, objects=objects, sort_scores=bool(s)) for s in range(S)])
    kw = dict(low_threshold=0.1, **KAL)
    host, dev = _bank("host", max_tracks=128, **kw), _bank("device", max_tracks=128, **kw)
    most = 0
    for f, det in enumerate(dets):
        host.update_batch(*det)
        compare(host, dev, dev.update_batch(*det), list(range(S)), f)
        most = max(most, max(int(host._off[s + 1] - host._off[s]) for s in range(S)))
    dev.check()
    assert most > 64


def test_partial_steps_and_resets_equal_the_host_bank():
    dets, kw = scene("low")
    kw = dict(kw, **KAL)
    host, dev = _bank("host", **kw), _bank("device", **kw)
    plan = {3: [2, 0], 4: [1], 7: [0, 1], 11: [2], 12: [1, 2, 0]}
    for f, det in enumerate(dets[:22]):
        if f == 9:
            host.reset(1), dev.reset(1)
            compare(host, dev, None, [], (f, "reset 1"))
            assert dev.last_matches[1] is None and dev[1].tracks == [] and dev[1].next_track_id == 0
        if f == 10:
            host.reset(0), dev.reset(0), host.reset(0), dev.reset(0)           # twice: the second finds no rows
        if f == 15:
            host.reset(), dev.reset()
            assert dev.snapshot()["offsets"].tolist() == [0] * (S + 1) and list(dev.last_matches) == [None] * S
        live = plan.get(f, list(range(S)))
        part = sub(det, live)
        host.update_batch(*part, streams=live)
        compare(host, dev, dev.update_batch(*part, streams=live), live, f)
    dev.check()


BLOCKED = [(torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"),
           (torch.Tensor, "numpy")]


def _boom(*a, **kw):
    raise AssertionError("host synchronisation inside a step")


@pytest.mark.parametrize("name", list(SCENES))
def test_steady_state_steps_never_synchronise(name, monkeypatch):
    dets, kw = scene(name)
    host, dev = _bank("host", **kw), _bank("device", **kw)
    for det in dets[:5]:
        host.update_batch(*det), dev.update_batch(*det)
    with monkeypatch.context() as m:
        for owner, attr in BLOCKED:
            m.setattr(owner, attr, _boom)
        outs = [dev.update_batch(*det) for det in dets[5:15]]
        dev.reset(1)                                                    # stream-ordered too
        outs.append(dev.update_batch(*dets[15]))
        with pytest.raises(AssertionError, match="host synchronisation"):      # the patches do see the host path's synchronisation
            host.update_batch(*dets[5])
    host = _bank("host", **kw)                      # (the refused step stopped half way: a fresh host bank replays the calls)
    for f, det in enumerate(dets[:16]):
        if f == 15:
            host.reset(1)
        host.update_batch(*det)
        if f >= 5:
            compare_outputs(host, dev, outs[f - 5], list(range(S)), (name, f))
    compare(host, dev, None, [], name)


def _assoc(dev, live):
    """The device's own records of the last step as lifecycle_ref reads an association."""
    recs, low = dev._download()["records"], dev._res.low_rec
    out = {}
    for s in live:
        r = (th.read_stream_low_record if low else th.read_stream_record)(recs[s])
        out[s] = dict(status=r[2], det_index=r[3], matches=r[7], unmatched_dets=r[8], low_matches=r[11] if low else [])
    return out


def _guarded(res, guard=8):
    """Replace the tables of a ResidentState by views inside 0xFF guards of `guard` rows -> the allocations."""
    allocs = []
    for tables in (res.emb, res.box) + ((res.kx, res.kP) if res.kalman else ()):
        for b in (0, 1):
            big = torch.full((res.C + 2 * guard, tables[b].shape[1]), float("nan"), device=DEV, dtype=tables[b].dtype)
            big.view(torch.uint8).fill_(0xFF)
            big[guard:guard + res.C] = 0
            tables[b] = big[guard:guard + res.C]
            allocs.append((big, guard))
    return allocs


@pytest.mark.parametrize("kalman", [False, True])
def test_capacity_rule_inside_guards(kalman):
    """max_tracks = 4 on a scene of six objects: births are dropped by the rule of tests/lifecycle_ref.py (fed with the device's own records), the
    overflow bit is reported and cleared by check(), and no table row outside the S * max_tracks is touched."""
    dets, _ = scene("plain")
    kw = KAL if kalman else {}
    k, cap = int(dets[0][0].shape[1]), 4
    dev = _bank("device", max_tracks=cap, **kw)
    dev._res = th.ResidentState(S, cap, k, E, torch.device(DEV), kalman, False)
    allocs = _guarded(dev._res)
    st = lr.new_state(S, cap)
    dropped = 0
    for f, det in enumerate(dets[:12]):
        out = dev.update_batch(*det)
        assoc = _assoc(dev, range(S))
        d = dev._download()
        box = det[0].cpu().numpy().reshape(-1, 4)
        kbox = None
        if kalman:      # the filter's record is device memory beside the lists: read it for the rule's emit
            o = dev._res.off["kalman_box"]
            kbox = dev._res.ctl[o:o + 32 * S * cap].cpu().numpy().view(np.float64).reshape(-1, 4)
        st, lists, want = lr.step(st, assoc, list(range(S)), k, cap, box, det[1].cpu().numpy().reshape(-1), dev.min_birth_age, dev.max_inactive_age, f, kbox)
        dropped += sum(len(a["unmatched_dets"]) for a in assoc.values()) - int((lists["src_trk"][:st["trk_off"][S]] == -1).sum())
        for name in lr.ROW_FIELDS + ("trk_off", "next_track_id", "status"):
            assert np.array_equal(d[name], st[name]), (f, name)
        assert np.array_equal(_bits(d["bbox"]), _bits(st["box"])), f
        for key, v in out.items():
            assert np.array_equal(v.cpu().numpy(), want[key]), (f, key)
        assert (np.diff(d["trk_off"]) <= cap).all()
    assert dropped > 0 and (st["status"][:, 0] & lr.OVERFLOW).any()
    with pytest.raises(ValueError, match=r"stream \d: overflow") as e:
        dev.check()
    for s in np.flatnonzero(st["status"][:, 0]):
        assert f"stream {s}: overflow" in str(e.value) and f"first at step {st['status'][s, 1]}" in str(e.value)
    dev.check()                                                         # cleared
    assert not dev._download()["status"].any()
    for big, g in allocs:
        raw = big.view(torch.uint8)
        assert bool((raw[:g] == 0xFF).all()) and bool((raw[-g:] == 0xFF).all())


def test_a_stream_with_non_finite_costs_is_skipped_and_reported():
    dets, kw = scene("plain")
    host, dev = _bank("host", **kw), _bank("device", **kw)
    for f, det in enumerate(dets[:14]):
        if f != 6:
            host.update_batch(*det)
            compare(host, dev, dev.update_batch(*det), [0, 1, 2], f)
            continue
        emb = det[3].clone()
        emb[1, 0] = 0                                   # a zero embedding under "cosine": stream 1's costs are not finite
        assert float(det[2][1, 0]) >= host.detection_threshold and host._off[2] > host._off[1]
        before = dev._download()
        others = [0, 2]
        host.update_batch(*sub(det, others), streams=others)
        out = dev.update_batch(det[0], det[1], det[2], emb)
        compare(host, dev, out, [0, 1, 2], f, skipped=[1])          # stream 1 included: the host bank left it alone
        after = dev._download()
        r0, r1 = int(before["trk_off"][1]), int(before["trk_off"][2])
        q0, q1 = int(after["trk_off"][1]), int(after["trk_off"][2])
        assert q1 - q0 == r1 - r0 and after["next_track_id"][1] == before["next_track_id"][1]
        for name in lr.ROW_FIELDS + ("bbox", "emb", "box"):
            assert np.array_equal(_bits(after[name][q0:q1]), _bits(before[name][r0:r1])), name
        with pytest.raises(ValueError, match=r"stream 1: association status 1 \(skipped\), first at step 6") as e:
            dev.check()
        assert "stream 0" not in str(e.value) and "stream 2" not in str(e.value)
    dev.check()


def test_steps_alternating_between_two_streams_equal_the_default_stream_run():
    dets, kw = scene("kalman")
    one, two = _bank("device", **kw), _bank("device", **kw)
    lanes = [torch.cuda.Stream(DEV), torch.cuda.Stream(DEV)]
    for f, det in enumerate(dets[:12]):
        want = {key: v.cpu() for key, v in one.update_batch(*det).items()}
        a = one._download()
        with torch.cuda.stream(lanes[f % 2]):
            got = {key: v.cpu() for key, v in two.update_batch(*det).items()}
            b = two._download()
        for key in got:
            assert torch.equal(got[key], want[key]), (f, key)
        for key in a:
            assert np.array_equal(_bits(a[key]) if a[key].dtype.kind == "f" else a[key], _bits(b[key]) if b[key].dtype.kind == "f" else b[key]), (f, key)


def test_outputs_go_to_draw_detections_as_they_are():
    dets, kw = scene("plain")
    host, dev = _bank("host", **kw), _bank("device", **kw)
    side = 96
    frames = torch.from_numpy(np.random.default_rng(3).integers(0, 255, (S, side, side, 3), dtype=np.uint8)).to(DEV)
    for det in dets[:10]:
        det = (det[0] * side,) + det[1:]                # boxes in the frames' pixels
        host.update_batch(*det)
        out = dev.update_batch(*det)
    got = cl.draw_detections(frames, out["bboxes"], labels=out["labels"], numbers=out["track_ids"].to(torch.int32), count=out["count"])
    boxes, numbers, count = np.zeros((S, M, 4), np.float32), np.zeros((S, M), np.int32), np.zeros(S, np.int32)
    for s in range(S):                                  # the host path's lists packed into the same arrays
        act = [t for t in host[s].tracks if t.active]
        count[s] = len(act)
        boxes[s, :len(act)] = [t.bbox for t in act]
        numbers[s, :len(act)] = [t.track_id for t in act]
    assert count.sum() >= S
    d = lambda a: torch.from_numpy(a).to(DEV)
    want = cl.draw_detections(frames, d(boxes), labels=d(np.zeros((S, M), np.int64)), numbers=d(numbers), count=d(count))
    assert torch.equal(got, want) and not torch.equal(got, frames)
