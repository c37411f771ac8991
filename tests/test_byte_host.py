"""CPU: the BYTE low-score association's host side — the new C-ABI entry points (declared, exported, bound, sizes, argument validation without
a device), the settings' validation, the rule's restatement (tests/byte_ref.py) against oracle/tracker_ref.py, a hand-worked frame, the life
cycle with low matches, and the stage's effect on a seeded occlusion scene."""
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import byte_ref
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd import _track_host as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cnl_track_frame_low_f32", "cnl_track_frame_low_bytes", "cnl_track_streams_low_f32", "cnl_track_streams_low_workspace_bytes",
       "cnl_track_streams_low_record_bytes", "cnl_track_apply_keep_f32")


def test_new_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.cnl_version() == _lib.ABI_VERSION == 13           # new entry points only: the ABI version stays


def test_size_helpers_equal_their_python_restatements():
    lib = _lib.load()
    for k, T, wd in [(48, 0, 1), (70, 65, 1), (70, 1, 0), (300, 70, 1), (300, 70, 0), (1024, 4096, 1), (7, 3, 0), (1, 1, 1)]:
        assert lib.cnl_track_frame_low_bytes(k, T, wd) == th.frame_low_layout(k, T, wd).bytes
        assert lib.cnl_track_frame_bytes(k, T, wd) == th.frame_layout(k, T, wd).bytes
        assert lib.cnl_track_frame_low_bytes(k, T, wd) >= lib.cnl_track_frame_bytes(k, T, wd) + 16 + 4 * k
        lay = th.streams_low_layout(k, T, wd)
        assert lib.cnl_track_streams_low_record_bytes(k, T, wd) == lay.bytes and lay.bytes % 8 == 0
        assert lay.bytes >= lib.cnl_track_streams_record_bytes(k, T, wd) + 32 + 12 * k
        assert lay.off_low_index == lay.off_utrk + 4 * T and lay.off_low_match == lay.off_low_index + 4 * k and lay.off_low_match + 8 * k <= lay.bytes
        for S in (1, 5, 32):
            assert lib.cnl_track_streams_low_workspace_bytes(S, k, T) == th.streams_low_workspace_bytes(S, k, S * T)
            assert lib.cnl_track_streams_low_workspace_bytes(S, k, T) == lib.cnl_track_streams_workspace_bytes(S, k, T) + 4 * k * S * T + 4 * S
    assert lib.cnl_track_frame_low_bytes(0, 3, 1) == 0 and lib.cnl_track_frame_low_bytes(4, -1, 1) == 0
    assert lib.cnl_track_streams_low_record_bytes(0, 3, 1) == 0 and lib.cnl_track_streams_low_workspace_bytes(0, 300, 70) == 0


def test_argument_errors_without_touching_a_device():
    lib = _lib.load()
    p = 0x1000                       # never dereferenced: every call below is refused on its arguments

    def frame(**kw):
        a = dict(det_emb=p, det_box=p, det_score=p, det_label=None, label_kind=0, k=48, E=64, thr=0.3, low=0.1, trk_emb=p, trk_box=p, T=12, box_cost=1,
                 reid_metric=0, with_dets=1, rec=p, rec_bytes=1 << 30, stream=None)
        a.update(kw)
        return lib.cnl_track_frame_low_f32(*a.values())
    assert frame(box_cost=0) == _lib.CNL_E_BAD_ARG and "box_cost" in _lib.last_error()
    assert frame(low=0.31) == _lib.CNL_E_BAD_ARG and "low_threshold" in _lib.last_error()
    assert frame(low=-0.01) == _lib.CNL_E_BAD_ARG and "low_threshold" in _lib.last_error()
    assert frame(low=float("nan")) == _lib.CNL_E_BAD_ARG
    assert frame(det_emb=None) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error()
    assert frame(k=2000) == _lib.CNL_E_UNSUPPORTED
    assert frame(rec=p + 4) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error()
    assert frame(det_box=p + 4) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error()
    assert frame(trk_emb=p + 8) == _lib.CNL_E_BAD_ARG
    need = lib.cnl_track_frame_low_bytes(48, 12, 1)
    assert frame(rec_bytes=need - 1) == _lib.CNL_E_BAD_ARG and "cnl_track_frame_low_bytes" in _lib.last_error()
    assert frame(rec_bytes=lib.cnl_track_frame_bytes(48, 12, 1)) == _lib.CNL_E_BAD_ARG           # the plain record is too short

    def streams(**kw):
        a = dict(det_emb=p, det_box=p, det_score=p, det_label=None, label_kind=0, S=4, S_live=4, live=p, k=48, E=64, thr=0.3, reid_thr=0.2,
                 box_thr=0.5, low=0.1, low_box=0.5, trk_emb=p, trk_box=p, trk_off=p, elig=None, R=40, T_max=12, box_cost=1, reid_metric=0, with_dets=1,
                 ws=p, ws_bytes=1 << 30, rec=p, stride=1 << 16, stream=None)
        a.update(kw)
        return lib.cnl_track_streams_low_f32(*a.values())
    assert streams(box_cost=0) == _lib.CNL_E_BAD_ARG and "box_cost" in _lib.last_error()
    assert streams(low=0.5) == _lib.CNL_E_BAD_ARG and "low_threshold" in _lib.last_error()
    assert streams(low=-1.0) == _lib.CNL_E_BAD_ARG and "low_threshold" in _lib.last_error()
    assert streams(live=None) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error()
    assert streams(S_live=5) == _lib.CNL_E_BAD_ARG
    assert streams(k=2000) == _lib.CNL_E_UNSUPPORTED and "1024" in _lib.last_error()
    assert streams(T_max=5000) == _lib.CNL_E_UNSUPPORTED and "4096" in _lib.last_error()
    assert streams(rec=p + 4) == _lib.CNL_E_BAD_ARG and streams(ws=p + 4) == _lib.CNL_E_BAD_ARG and streams(stride=(1 << 16) + 4) == _lib.CNL_E_BAD_ARG
    assert streams(det_box=p + 8) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error()
    rec_need, ws_need = lib.cnl_track_streams_low_record_bytes(48, 12, 1), th.streams_low_workspace_bytes(4, 48, 40)
    assert streams(stride=rec_need - 8) == _lib.CNL_E_BAD_ARG and "cnl_track_streams_low_record_bytes" in _lib.last_error()
    assert streams(stride=lib.cnl_track_streams_record_bytes(48, 12, 1)) == _lib.CNL_E_BAD_ARG      # the plain stride is too short
    assert streams(ws_bytes=ws_need - 1) == _lib.CNL_E_BAD_ARG and "workspace" in _lib.last_error()
    assert streams(ws_bytes=th.streams_workspace_bytes(4, 48, 40)) == _lib.CNL_E_BAD_ARG

    def keep(**kw):
        a = dict(trk_emb=p, trk_box=p, det_emb=p, det_box=p, src_trk=p, src_det=p, T_new=8, E=32, s=0.5, new_emb=2 * p, new_box=2 * p, keep=p, stream=None)
        a.update(kw)
        return lib.cnl_track_apply_keep_f32(*a.values())
    assert keep(T_new=-1) == _lib.CNL_E_BAD_ARG and keep(E=0) == _lib.CNL_E_BAD_ARG
    assert keep(src_det=None) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error()
    assert keep(new_emb=p) == _lib.CNL_E_BAD_ARG and "alias" in _lib.last_error()
    assert keep(T_new=0) == 0                                                                    # nothing to launch


def test_settings_validation():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for make in (cl.Tracker, lambda **kw: cl.TrackerBank(num_streams=2, **kw)):
            with pytest.raises(ValueError, match="low_threshold"):
                make(low_threshold=0.1, box_cost=None)
            with pytest.raises(ValueError, match="low_threshold"):
                make(low_threshold=0.31)
            with pytest.raises(ValueError, match="low_threshold"):
                make(low_threshold=-0.1)
            with pytest.raises(ValueError, match="low_match"):
                make(low_match="confirmed")
            with pytest.raises(ValueError, match="low_match"):
                make(low_threshold=0.1, low_match=None)
            t = make(low_threshold=0.3, low_box_threshold=0.4, low_match="all")                  # == detection_threshold is legal
            assert (t.low_threshold, t.low_box_threshold, t.low_match) == (0.3, 0.4, "all")
            assert t._thresholds({}) == (0.3, 0.2, 0.5, 0.3, 0.4)
            t = make()
            assert (t.low_threshold, t.low_box_threshold, t.low_match) == (None, None, "active")
            assert t._thresholds({}) == (0.3, 0.2, 0.5, None, 0.5)
            # per call: both thresholds may be overridden, and are checked against each other again
            assert t._thresholds(dict(low_threshold=0.1, box_threshold=0.6)) == (0.3, 0.2, 0.6, 0.1, 0.6)
            assert t._thresholds(dict(low_threshold=0.1, low_box_threshold=0.7)) == (0.3, 0.2, 0.5, 0.1, 0.7)
            with pytest.raises(ValueError, match="low_threshold"):
                t._thresholds(dict(low_threshold=0.35))
            with pytest.raises(ValueError, match="low_threshold"):
                make(low_threshold=0.2)._thresholds(dict(detection_threshold=0.15))
            with pytest.raises(ValueError, match="low_threshold"):
                make(box_cost=None)._thresholds(dict(low_threshold=0.1))
        with pytest.raises(ValueError, match="low_threshold"):
            cl.Tracker(low_threshold=0.1, box_cost=lambda a, b: a @ b.T, allow_host_cost=True)
        t = cl.build_tracker(dict(low_threshold=0.1, low_match="all"))
        b = cl.build_tracker(dict(low_threshold=0.1, low_box_threshold=0.3), num_streams=3)
        assert type(t) is cl.Tracker and t.low_threshold == 0.1 and t.low_match == "all"
        assert type(b) is cl.TrackerBank and b.low_box_threshold == 0.3 and b.last_low_matches == [None] * 3


def _same_tracks(a, b, tag):
    assert [t.track_id for t in a.tracks] == [t.track_id for t in b.tracks], tag
    assert [(t.state.name, t.birth_age, t.inactive_age) for t in a.tracks] == [(t.state.name, t.birth_age, t.inactive_age) for t in b.tracks], tag
    for x, y in zip(a.tracks, b.tracks):
        assert np.array_equal(x.bbox, y.bbox) and np.array_equal(x.embedding, y.embedding), tag
    assert a.next_track_id == b.next_track_id, tag


@pytest.mark.parametrize("kw", [dict(), dict(use_kalman=True), dict(box_cost="giou", box_threshold=0.7), dict(box_cost=None)], ids=str)
@pytest.mark.parametrize("sort_scores", [True, False])
def test_restatement_without_the_stage_is_the_oracle(kw, sort_scores):
    seq = tracker_ref.synth_sequence(3, sort_scores=sort_scores)
    for low in (None,) if kw.get("box_cost", "iou") is None else (None, 0.3):                    # an empty low set gives the results of None
        ref, got = tracker_ref.Tracker(**kw), byte_ref.Tracker(low_threshold=low, **kw)
        for f, fr in enumerate(seq):
            ref.update(*fr)
            got.update(*fr)
            _same_tracks(got, ref, (f, low))
            assert got.last_low_matches == []


def _hand_frame(low_match):
    """Three tracks — 0 ACTIVE, 1 INACTIVE, 2 UNCONFIRMED — at boxes A, B, C, with orthogonal embeddings; one frame of four detections:
         0: score 0.9, far from every track, a fourth embedding          -> a birth
         1: score 0.2 on A (shifted a little), embedding of NO track     -> low: matches track 0 by box alone
         2: score 0.2 on B                                               -> low: track 1 is INACTIVE — eligible only under "all"
         3: score 0.05 on C                                              -> below low_threshold: ignored; track 2 stays unmatched and is deleted"""
    trk = byte_ref.Tracker(low_threshold=0.1, low_match=low_match)
    A, B, C = [0.1, 0.1, 0.3, 0.3], [0.5, 0.1, 0.7, 0.3], [0.1, 0.5, 0.3, 0.7]
    eye = np.eye(8, dtype=np.float32)
    for i, (box, state) in enumerate(zip((A, B, C), (tracker_ref.TrackState.ACTIVE, tracker_ref.TrackState.INACTIVE, tracker_ref.TrackState.UNCONFIRMED))):
        t = tracker_ref.Track(i, np.array(box, np.float32), 0, eye[i], smoothing_factor=0.5)
        t.state = state
        trk.tracks.append(t)
    trk.next_track_id = 3
    shift = np.array([0.01, 0.0, 0.01, 0.0], np.float32)
    boxes = np.array([[0.8, 0.8, 0.9, 0.9], A, B, C], np.float32) + np.array([0, 1, 1, 0], np.float32)[:, None] * shift
    scores = np.array([0.9, 0.2, 0.2, 0.05], np.float32)
    embs = np.stack([eye[3], eye[4], eye[5], eye[2]])
    trk.update(boxes, np.zeros(4, np.int64), scores, embs)
    return trk, boxes, eye


def test_hand_worked_frame():
    trk, boxes, eye = _hand_frame("active")
    assert trk.last_matches == [] and trk.last_low_matches == [(1, 0)]
    assert [(t.track_id, t.state.name) for t in trk.tracks] == [(0, "ACTIVE"), (1, "INACTIVE"), (3, "UNCONFIRMED")]      # track 2 deleted, one birth
    assert trk.tracks[1].inactive_age == 1                                                       # not eligible: unmatched once more
    assert np.array_equal(trk.tracks[0].bbox, boxes[1]) and np.array_equal(trk.tracks[0].embedding, eye[0])      # the box moved, the embedding did not
    assert np.array_equal(trk.tracks[1].bbox, np.array([0.5, 0.1, 0.7, 0.3], np.float32))
    assert np.array_equal(trk.tracks[2].bbox, boxes[0]) and trk.next_track_id == 4               # the birth is the HIGH detection; no low one is born

    trk, boxes, eye = _hand_frame("all")
    assert trk.last_matches == [] and trk.last_low_matches == [(1, 0), (2, 1)]
    assert [(t.track_id, t.state.name) for t in trk.tracks] == [(0, "ACTIVE"), (1, "ACTIVE"), (3, "UNCONFIRMED")]        # the INACTIVE track came back
    assert np.array_equal(trk.tracks[1].bbox, boxes[2]) and np.array_equal(trk.tracks[1].embedding, eye[1])
    assert trk.next_track_id == 4 and trk.last_unmatched_tracks == [2]


def test_life_cycle_with_low_matches():
    settings = SimpleNamespace(min_birth_age=2, max_inactive_age=30, smoothing_factor=0.5, use_kalman=False)
    S = th.TrackState

    def tracks():
        out = []
        for i, state in enumerate((S.ACTIVE, S.INACTIVE, S.UNCONFIRMED, S.ACTIVE, S.UNCONFIRMED)):
            t = th.Track(settings, 10 + i, np.full(4, float(i), np.float32), 0)
            t.state = state
            out.append(t)
        return out
    boxes = np.arange(32, dtype=np.float32).reshape(8, 4)
    labels = np.arange(8)
    det_index = np.array([0, 2, 5], np.int32)                                                    # kept detections; 3, 4, 6 are low
    # stage 1 / 2: kept row 1 -> track 3 (quirk: the box read is boxes[1]); stage 3: detection 6 -> track 0, detection 4 -> track 1, 3 -> track 4
    got = th.life_cycle(tracks(), [(1, 3)], [0, 2], [2], det_index, boxes, labels, 7, settings, low_matches=[(6, 0), (4, 1), (3, 4)])
    assert len(got) == 5
    new, next_id, old_rows, det_rows, keep_emb = got
    assert [t.track_id for t in new] == [10, 11, 13, 14, 7, 8] and next_id == 9                   # track 12 (UNCONFIRMED, unmatched) is deleted
    assert [t.state for t in new] == [S.ACTIVE, S.ACTIVE, S.ACTIVE, S.UNCONFIRMED, S.UNCONFIRMED, S.UNCONFIRMED]
    assert new[3].birth_age == 1                                                                 # a low match counts towards confirmation
    assert old_rows == [0, 1, 3, 4, -1, -1]
    assert det_rows == [6, 4, 1, 3, 0, 5]                                                        # low: ORIGINAL indices; births: det_index[0], det_index[2]
    assert keep_emb == [1, 1, 0, 1, 0, 0]
    assert np.array_equal(new[0].bbox, boxes[6]) and np.array_equal(new[1].bbox, boxes[4]) and np.array_equal(new[2].bbox, boxes[1])
    # without the stage (None, the default): the four values of before; with the stage and no low match: the same, and no row keeps its embedding
    for kw, n_out in ((dict(), 4), (dict(low_matches=None), 4), (dict(low_matches=()), 5), (dict(low_matches=[]), 5)):
        out = th.life_cycle(tracks(), [(1, 3)], [0, 2], [0, 1, 2, 4], det_index, boxes, labels, 7, settings, **kw)
        assert len(out) == n_out and out[2] == [0, 1, 3, -1, -1] and out[3] == [-1, -1, 1, 0, 5]
        assert [t.state for t in out[0]] == [S.INACTIVE, S.INACTIVE, S.ACTIVE, S.UNCONFIRMED, S.UNCONFIRMED]
        assert n_out == 4 or out[4] == [0, 0, 0, 0, 0]


def test_low_stage_of_the_host_path():
    low_box = np.array([[0.9, 0.2, 0.3, 1.0], [0.1, 0.2, 0.6, 1.0], [1.0, 1.0, 1.0, 1.0]], np.float32)
    low_index = np.array([4, 7, 9], np.int32)
    assert th.low_stage(low_box, low_index, [0, 1, 3], None, 0.5) == ([(4, 1), (7, 0)], [3])
    assert th.low_stage(low_box, low_index, [0, 1, 3], [False, True, True, True], 0.5) == ([(4, 1)], [0, 3])     # track 0 not eligible: it stays unmatched
    assert th.low_stage(low_box, low_index, [0, 1, 3], [False] * 4, 0.5) == ([], [0, 1, 3])
    assert th.low_stage(low_box[:0], low_index[:0], [0, 1], None, 0.5) == ([], [0, 1])
    assert th.low_stage(low_box, low_index, [], None, 0.5) == ([], [])
    thr = 0.2                                                                                     # float32 compare: float32(0.2) is not below 0.2
    assert th.low_stage(low_box, low_index, [1], None, thr) == ([], [1])


@pytest.mark.parametrize("use_kalman", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5])
def test_the_stage_keeps_occluded_objects_tracked(seed, use_kalman):
    seq, truth = byte_ref.synth_occlusion(seed, frames=30, objects=6, k=70, sort_scores=True)
    missed0, stray0, ids0 = byte_ref.occlusion_counts(byte_ref.Tracker(low_threshold=None, use_kalman=use_kalman), seq, truth)
    missed1, stray1, ids1 = byte_ref.occlusion_counts(byte_ref.Tracker(low_threshold=0.1, use_kalman=use_kalman), seq, truth)
    print(f"seed {seed} use_kalman {use_kalman}: object-frames without an ACTIVE track {missed0} -> {missed1}, stray ACTIVE tracks {stray0} -> {stray1}, "
          f"ids per object {ids0} -> {ids1}")
    assert missed1 < missed0
    assert stray1 <= stray0
    assert all(b <= a for a, b in zip(ids0, ids1))
