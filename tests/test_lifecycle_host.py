"""CPU: the device track life cycle's host side — tests/lifecycle_ref.py (the three kernels' rule on plain arrays) held equal to the host path's
`_track_host.life_cycle` + `Track` on random assignments, its capacity and skipped-stream rules, the C-ABI entries (declared, exported, bound,
argument validation without a device) and the options of `TrackerBank(lifecycle=, max_tracks=)`."""
import ctypes
import inspect
import os
import re
import types
import warnings

import numpy as np
import pytest
import torch

import lifecycle_ref as lr
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd import _track_host as th
from centernet_lightning_amd import tracker as trk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cnl_track_lifecycle_workspace_bytes", "cnl_track_lifecycle_i32", "cnl_track_lifecycle_emit_f64")


def _settings(min_birth_age, max_inactive_age):
    return types.SimpleNamespace(use_kalman=False, kalman="host", min_birth_age=min_birth_age, max_inactive_age=max_inactive_age, smoothing_factor=0.5,
                                 _table=None)


def random_assoc(rng, T, k, thr=0.5, low_thr=0.2, sort_scores=False, empty=False):
    """A random VALID assignment for a stream of T tracks and k detections -> (assoc dict of lifecycle_ref, unmatched_tracks, boxes, labels)."""
    scores = rng.random(k).astype(np.float32)
    if sort_scores:
        scores = -np.sort(-scores)
    if empty:
        scores[:] = 0.0
    det_index = np.flatnonzero(scores >= thr).astype(np.int32)
    low_index = np.flatnonzero((scores >= low_thr) & (scores < thr))
    n = len(det_index)
    m = int(rng.integers(0, min(n, T) + 1))
    rows, tracks = rng.permutation(n)[:m], rng.permutation(T)
    matches = [(int(d), int(t)) for d, t in zip(rows, tracks[:m])]
    rest = tracks[m:]
    m3 = int(rng.integers(0, min(len(low_index), len(rest)) + 1))
    low_matches = [(int(d), int(t)) for d, t in zip(rng.permutation(low_index)[:m3], rest[:m3])]
    unmatched_dets = sorted(set(range(n)) - {d for d, _ in matches})
    unmatched_tracks = sorted(int(t) for t in rest[m3:])
    boxes = rng.random((k, 4)).astype(np.float32)
    labels = rng.integers(0, 5, k).astype(np.int64)
    return dict(status=0, matches=matches, low_matches=low_matches, unmatched_dets=unmatched_dets, det_index=det_index), unmatched_tracks, boxes, labels


@pytest.mark.parametrize("min_birth_age", [1, 3])
@pytest.mark.parametrize("sort_scores", [False, True])
def test_rule_equals_the_host_life_cycle_on_random_assignments(min_birth_age, sort_scores):
    S, M, k, steps, max_inactive_age = 4, 64, 14, 40, 3
    rng = np.random.default_rng(100 * min_birth_age + sort_scores)
    settings = _settings(min_birth_age, max_inactive_age)
    host = [dict(tracks=[], next_id=0) for _ in range(S)]
    st = lr.new_state(S, M)
    quirk = low = births = deleted = 0
    for step_no in range(steps):
        live = sorted(rng.permutation(S)[:int(rng.integers(1, S + 1))].tolist())
        if step_no % 7 == 3:
            live = live[::-1]               # slots need not be in stream order
        L = len(live)
        det_box, det_label = np.zeros((L * k, 4), np.float32), np.zeros(L * k, np.int64)
        assoc, want = {}, {}
        off = st["trk_off"].copy()
        for i, s in enumerate(live):
            T = len(host[s]["tracks"])
            # stream 1 never sees a detection until step 20 (an empty stream), stream 2 gets empty frames now and then
            a, ut, boxes, labels = random_assoc(rng, T, k, sort_scores=sort_scores, empty=(s == 1 and step_no < 20) or (s == 2 and step_no % 5 == 0))
            det_box[i * k:(i + 1) * k], det_label[i * k:(i + 1) * k] = boxes, labels
            assoc[s] = a
            quirk += sum(int(a["det_index"][d]) != d for d, _ in a["matches"])
            low += len(a["low_matches"])
            before = len(host[s]["tracks"])
            tracks, next_id, old_rows, det_rows, keep = th.life_cycle(host[s]["tracks"], a["matches"], a["unmatched_dets"], ut, a["det_index"], boxes,
                                                                      labels, host[s]["next_id"], settings, a["low_matches"])
            births += sum(r < 0 for r in old_rows)
            deleted += before - sum(r >= 0 for r in old_rows)
            host[s] = dict(tracks=tracks, next_id=next_id)
            want[s] = ([off[s] + r if r >= 0 else -1 for r in old_rows], [i * k + d if d >= 0 else -1 for d in det_rows], keep)
        st, lists, out = lr.step(st, assoc, live, k, M, det_box, det_label, min_birth_age, max_inactive_age, step_no)
        assert not st["status"].any()
        for s in range(S):
            r0, r1 = int(st["trk_off"][s]), int(st["trk_off"][s + 1])
            tracks = host[s]["tracks"]
            assert r1 - r0 == len(tracks) and st["next_track_id"][s] == host[s]["next_id"], (step_no, s)
            assert st["track_id"][r0:r1].tolist() == [t.track_id for t in tracks]
            assert st["state"][r0:r1].tolist() == [t.state.value for t in tracks]
            assert st["birth_age"][r0:r1].tolist() == [t.birth_age for t in tracks]
            assert st["inactive_age"][r0:r1].tolist() == [t.inactive_age for t in tracks]
            assert st["label"][r0:r1].tolist() == [int(t.label) for t in tracks]
            assert np.array_equal(st["box"][r0:r1], np.asarray([t.bbox for t in tracks], np.float64).reshape(-1, 4))
            assert lists["eligible"][r0:r1].tolist() == [int(t.active) for t in tracks]
            if s in want:
                assert lists["src_trk"][r0:r1].tolist() == want[s][0] and lists["src_det"][r0:r1].tolist() == want[s][1]
                assert lists["keep_emb"][r0:r1].tolist() == want[s][2] and lists["flags"][r0:r1].tolist() == [1] * (r1 - r0)
            else:           # carried: old rows in order, no detection, no prediction
                assert lists["src_trk"][r0:r1].tolist() == list(range(off[s], off[s + 1]))
                assert (lists["src_det"][r0:r1] == -1).all() and not lists["flags"][r0:r1].any() and not lists["keep_emb"][r0:r1].any()
        R = int(st["trk_off"][S])
        assert lists["src_trk"][R:].tolist() == list(range(R, S * M)) and (lists["src_det"][R:] == -1).all() and not lists["flags"][R:].any()
        assert not st["state"][R:].any() and not st["track_id"][R:].any() and not st["box"][R:].any()
        for i, s in enumerate(live):        # the outputs: _active() of the host path
            act = [t for t in host[s]["tracks"] if t.active]
            assert out["count"][i] == len(act) and out["track_ids"][i, :len(act)].tolist() == [t.track_id for t in act]
            assert np.array_equal(out["bboxes"][i, :len(act)], np.asarray([t.bbox for t in act], np.float32).reshape(-1, 4))
            assert out["labels"][i, :len(act)].tolist() == [int(t.label) for t in act]
            assert not out["bboxes"][i, len(act):].any() and not out["track_ids"][i, len(act):].any() and not out["labels"][i, len(act):].any()
    # the cases the comparison is about did occur
    assert low > 10 and births > 20 and deleted > 10 and (quirk > 10) == (not sort_scores)


def _birth_assoc(k, n):
    return dict(status=0, matches=[], low_matches=[], unmatched_dets=list(range(n)), det_index=np.arange(k - n, k, dtype=np.int32))


def test_capacity_rule():
    S, M, k = 2, 4, 8
    st = lr.new_state(S, M)
    box, lab = np.arange(2 * k * 4, dtype=np.float32).reshape(-1, 4), np.arange(2 * k, dtype=np.int64)
    st, lists, _ = lr.step(st, {0: _birth_assoc(k, 3), 1: _birth_assoc(k, 6)}, [0, 1], k, M, box, lab, 2, 30, 0)
    assert st["trk_off"].tolist() == [0, 3, 7] and st["next_track_id"].tolist() == [3, 4]       # stream 1: the FIRST four are born, two dropped, no id used
    assert st["status"].tolist() == [[0, 0], [lr.OVERFLOW, 0]]
    assert lists["src_det"][:7].tolist() == [5, 6, 7, k + 2, k + 3, k + 4, k + 5] and st["label"][:7].tolist() == [5, 6, 7, 10, 11, 12, 13]
    assert st["track_id"][:7].tolist() == [0, 1, 2, 0, 1, 2, 3] and (lists["src_trk"][:7] == -1).all()
    assert lists["src_trk"][7] == 7 and lists["src_det"][7] == -1
    # survivors keep their rows, births take what is left: stream 0 matches two of three (the unmatched UNCONFIRMED one is deleted) and wants 4 births
    a0 = dict(status=0, matches=[(0, 0), (1, 2)], low_matches=[], unmatched_dets=[2, 3, 4, 5], det_index=np.arange(k, dtype=np.int32))
    st2, lists2, _ = lr.step(st, {0: a0}, [0], k, M, box, lab, 2, 30, 5)
    assert st2["trk_off"].tolist() == [0, 4, 8] and st2["track_id"][:4].tolist() == [0, 2, 3, 4] and st2["next_track_id"].tolist() == [5, 4]
    assert st2["status"].tolist() == [[lr.OVERFLOW, 5], [lr.OVERFLOW, 0]]                            # sticky: stream 1's word is still there
    assert lists2["src_trk"].tolist() == [0, 2, -1, -1, 3, 4, 5, 6] and lists2["src_det"].tolist() == [0, 1, 2, 3, -1, -1, -1, -1]
    assert lists2["flags"].tolist() == [1, 1, 1, 1, 0, 0, 0, 0]


def test_skipped_stream_rule():
    S, M, k = 2, 4, 8
    st = lr.new_state(S, M)
    box, lab = np.ones((2 * k, 4), np.float32), np.zeros(2 * k, np.int64)
    st, _, _ = lr.step(st, {0: _birth_assoc(k, 2), 1: _birth_assoc(k, 2)}, [0, 1], k, M, box, lab, 1, 30, 0)
    bad = dict(_birth_assoc(k, 3), status=1)
    new, lists, out = lr.step(st, {0: bad, 1: dict(status=0, matches=[(0, 0), (1, 1)], low_matches=[], unmatched_dets=[], det_index=np.arange(2))},
                              [0, 1], k, M, box, lab, 1, 30, 7)
    assert new["status"].tolist() == [[1, 7], [0, 0]] and new["next_track_id"].tolist() == [2, 2]
    for name in lr.ROW_FIELDS + ("box",):               # rows and counters of the skipped stream: as before the step
        assert np.array_equal(new[name][:2], st[name][:2]), name
    assert lists["src_trk"][:2].tolist() == [0, 1] and (lists["src_det"][:2] == -1).all() and not lists["flags"][:2].any()
    assert new["state"][2:4].tolist() == [lr.ACTIVE] * 2 and lists["flags"][2:4].tolist() == [1, 1]
    assert out["count"].tolist() == [0, 2]
    # the first code and its step stay; an overflow later is or-ed in
    newer, _, _ = lr.step(new, {0: dict(_birth_assoc(k, 5), status=17)}, [0], k, M, box, lab, 1, 30, 8)
    assert newer["status"][0].tolist() == [1, 7]
    newest, _, _ = lr.step(newer, {0: _birth_assoc(k, 5)}, [0], k, M, box, lab, 1, 30, 9)
    assert newest["status"][0].tolist() == [1 | lr.OVERFLOW, 7]
    # reset of one stream: rows and counter gone, the other stream carried
    after, lists, _ = lr.step(newest, {}, [], k, M, box, lab, 1, 30, 10, reset=1)
    assert after["trk_off"].tolist() == [0, 4, 4] and after["next_track_id"].tolist() == [6, 0] and not lists["flags"].any()


def test_entry_points_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.cnl_version() == _lib.ABI_VERSION == 13           # new entry points only: the ABI version stays
    assert ctypes.sizeof(_lib.TrackRows) == 56 and ctypes.sizeof(_lib.TrackLifecycle) == 320
    assert re.search(r"int32_t reset_stream, reserved;[^}]*}\s*cnl_track_lifecycle;", header)
    assert lib.cnl_track_lifecycle_workspace_bytes(32, 256) == 36 * 32 * 256 + 8 * 32 and lib.cnl_track_lifecycle_workspace_bytes(0, 4) == 0
    assert [s.value for s in th._STATES[1:]] == [lr.UNCONFIRMED, lr.ACTIVE, lr.INACTIVE, lr.TO_DELETE] and th.STATUS_OVERFLOW == lr.OVERFLOW
    # the workspace of the issue's example: about 49 MB at S = 32, k = 300, max_tracks = 256
    assert 49e6 < lib.cnl_track_streams_workspace_bytes(32, 300, 256) == th.streams_workspace_bytes(32, 300, 32 * 256) < 50e6


def _args(**kw):
    p = 0x1000                      # never dereferenced: every call below is refused on its arguments
    a = _lib.TrackLifecycle()
    for rows, base in ((a.old_rows, p), (a.new_rows, 2 * p)):
        for i, (name, _) in enumerate(_lib.TrackRows._fields_):
            setattr(rows, name, base + 64 * i)
    for name in ("record", "live", "slot_of", "det_label", "det_box", "next_track_id", "status", "src_trk", "src_det", "flags", "keep_emb", "trk_eligible",
                 "kalman_box", "out_box", "out_track_id", "out_label", "out_count", "workspace"):
        setattr(a, name, p)
    a.record_stride, a.S, a.S_live, a.k, a.max_tracks, a.label_kind, a.low_record = 1 << 12, 3, 3, 12, 16, 1, 1
    a.min_birth_age, a.max_inactive_age, a.reset_stream = 2, 30, -1
    a.workspace_bytes = _lib.load().cnl_track_lifecycle_workspace_bytes(3, 16) - 1     # one byte short: a call that passes every other check stops here
    for name, v in kw.items():
        obj, _, field = name.rpartition(".")
        setattr(getattr(a, obj) if obj else a, field, v)
    return a


def test_argument_errors_without_touching_a_device():
    lib = _lib.load()
    for entry in (lib.cnl_track_lifecycle_i32, lib.cnl_track_lifecycle_emit_f64):
        def call(**kw):
            return entry(ctypes.byref(_args(**kw)), None)

        assert entry(None, None) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error()
        assert call() == _lib.CNL_E_BAD_ARG and "workspace holds" in _lib.last_error()
        for name in ("src_trk", "src_det", "flags", "keep_emb", "trk_eligible", "workspace", "live", "old_rows.state", "new_rows.box", "new_rows.trk_off"):
            assert call(**{name: None}) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error(), name
        for name, v in (("src_trk", 0x1002), ("flags", 0x1001), ("workspace", 0x1004), ("old_rows.track_id", 0x1004), ("new_rows.box", 0x2004),
                        ("new_rows.label", 0x2002)):
            assert call(**{name: v}) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error(), name
        assert call(**{"new_rows.state": 0x1000 + 64}) == _lib.CNL_E_BAD_ARG and "alias" in _lib.last_error()
        assert call(max_tracks=4097) == _lib.CNL_E_UNSUPPORTED and "max_tracks" in _lib.last_error()
        assert call(S=4096, S_live=4096, k=1 << 19) == _lib.CNL_E_UNSUPPORTED and "int32" in _lib.last_error()
        assert call(S=4097) == _lib.CNL_E_UNSUPPORTED
        for name, v in (("S", 0), ("S_live", 4), ("S_live", -1), ("k", 0), ("max_tracks", 0)):
            assert call(**{name: v}) == _lib.CNL_E_BAD_ARG and "bad S" in _lib.last_error(), name
    full = lib.cnl_track_lifecycle_workspace_bytes(3, 16)       # with the workspace in place, the entry's own checks

    def life(**kw):
        return lib.cnl_track_lifecycle_i32(ctypes.byref(_args(workspace_bytes=full, **kw)), None)

    for name in ("slot_of", "record", "next_track_id", "status"):
        assert life(**{name: None}) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error(), name
    for name, v in (("record", 0x1004), ("record_stride", 4100), ("next_track_id", 0x1004), ("status", 0x1002)):
        assert life(**{name: v}) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error(), name
    assert life(record_stride=88) == _lib.CNL_E_BAD_ARG and "header" in _lib.last_error()
    assert life(label_kind=4) == _lib.CNL_E_BAD_ARG and life(label_kind=1, det_label=None) == _lib.CNL_E_BAD_ARG and "label_kind" in _lib.last_error()
    assert life(min_birth_age=-1) == _lib.CNL_E_BAD_ARG

    def emit(**kw):
        return lib.cnl_track_lifecycle_emit_f64(ctypes.byref(_args(workspace_bytes=full, **kw)), None)

    assert emit(det_box=None) == _lib.CNL_E_BAD_ARG and emit(kalman_box=0x1004) == _lib.CNL_E_BAD_ARG and "kalman_box" in _lib.last_error()
    for name in ("out_box", "out_track_id", "out_label", "out_count"):
        assert emit(**{name: None}) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error(), name
    assert emit(out_track_id=0x1004) == _lib.CNL_E_BAD_ARG and emit(out_count=0x1002) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error()


def test_options():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        # lifecycle="host": the bank as it was — the constructor's own parameters, the per-stream records, the lists
        for bank in (cl.TrackerBank(3), cl.TrackerBank(3, lifecycle="host", max_tracks=7)):
            assert bank.lifecycle == "host" and not bank._resident and bank._res is None
            assert type(bank[0]) is trk._StreamState and bank[0].tracks == [] and bank.last_matches == [None] * 3 and bank.last_low_matches == [None] * 3
            with pytest.raises(ValueError, match="lifecycle"):
                bank.snapshot()
            bank.check()
        assert cl.TrackerBank(3, max_tracks=7).max_tracks == 7
        assert list(inspect.signature(cl.TrackerBank.__init__).parameters)[-1] == "kalman"
        with pytest.raises(TypeError):
            cl.Tracker(lifecycle="device")                  # one stream on one wave loses to a CPU core: the bank's option only
        # refused by name
        with pytest.raises(ValueError, match="lifecycle='gpu'"):
            cl.TrackerBank(3, lifecycle="gpu")
        for bad in (0, -1, 2.5, True, None):
            with pytest.raises(ValueError, match="max_tracks"):
                cl.TrackerBank(3, max_tracks=bad)
        with pytest.raises(ValueError, match="max_tracks=4097"):
            cl.TrackerBank(3, lifecycle="device", max_tracks=4097)
        assert cl.TrackerBank(3, lifecycle="host", max_tracks=4097).max_tracks == 4097       # without effect there
        with pytest.raises(ValueError, match="kalman='host'"):
            cl.TrackerBank(3, lifecycle="device", use_kalman=True)
        with pytest.raises(ValueError, match="kalman='host'"):
            cl.TrackerBank(3, None, 3, 300, 0.3, "cosine", 0.2, "iou", 0.5, 0.5, True, lifecycle="device")
        with pytest.raises(ValueError, match="reid_cost"):
            cl.TrackerBank(3, lifecycle="device", reid_cost="jaccard")
        # accepted
        for kw in (dict(), dict(use_kalman=True, kalman="device"), dict(use_kalman=False, kalman="host"), dict(low_threshold=0.1, low_match="all"),
                   dict(low_threshold=0.1, low_box_threshold=0.4), dict(class_aware=True), dict(box_cost=None), dict(box_cost="giou", reid_cost="euclidean"),
                   dict(use_kalman=True, kalman="device", motion_gate=True, motion_weight=0.9, class_aware=True)):
            bank = cl.TrackerBank(3, lifecycle="device", max_tracks=16, **kw)
            assert bank.lifecycle == "device" and bank.max_tracks == 16 and bank._resident
            # before the first step nothing lives on a device: the host views are empty, reset and check need none
            assert type(bank[1]) is trk._ResidentStream and bank[1].tracks == [] and bank[1].next_track_id == 0 and bank[1].frame == 0
            assert len(bank.last_matches) == 3 and list(bank.last_matches) == [None] * 3 and bank.last_low_matches[2] is None
            snap = bank.snapshot()
            assert snap["offsets"].tolist() == [0, 0, 0, 0] and snap["next_track_id"].tolist() == [0, 0, 0]
            bank.reset()
            bank.reset(stream=2)
            bank.check()
            with pytest.raises(ValueError):
                bank.reset(stream=3)
            # host arrays are refused by name, before any device is touched
            z = np.zeros
            with pytest.raises(ValueError, match="host arrays are refused"):
                bank.update_batch(z((3, 8, 4), np.float32), z((3, 8), np.int64), z((3, 8), np.float32), z((3, 8, 16), np.float32))
            with pytest.raises(ValueError, match="host arrays are refused"):
                bank.update_batch(*(torch.zeros(s) for s in ((3, 8, 4), (3, 8), (3, 8), (3, 8, 16))))
        # build_tracker and the YAML section
        cfg = dict(cl.load_config(os.path.join(ROOT, "centernet-lightning_amd", "configs", "tracking_resnet34_fpn.yaml"))["tracker"])
        assert cfg["lifecycle"] == "host" and cfg["max_tracks"] == 256
        assert type(cl.build_tracker(cfg)) is cl.Tracker
        bank = cl.build_tracker(dict(cfg, lifecycle="device", max_tracks=32), num_streams=2)
        assert type(bank) is cl.TrackerBank and bank.lifecycle == "device" and bank.max_tracks == 32
        with pytest.raises(ValueError, match="lifecycle"):
            cl.build_tracker(dict(cfg, lifecycle="device"))
