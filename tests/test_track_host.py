"""CPU: the host side that Tracker and TrackerBank share (centernet_lightning_amd/_track_host.py) — the record layouts against the
library's size helpers, the record readers on hand-built records, the two-stage assignment in its three forms, and the life cycle
driven frame by frame against the goldens of the reference's own Tracker.update (no device: the cost matrices come from the oracle and
the track table is a numpy restatement of cnl_track_apply_f32)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import tracker_ref
from test_oracle_tracker import SEQS, load_case, unpack
from centernet_lightning_amd import _lib
from centernet_lightning_amd import _track_host as th


def test_record_layouts_equal_the_c_helpers():
    lib = _lib.load()
    for k, T, wd in [(1, 0, 0), (1, 0, 1), (7, 3, 0), (48, 0, 1), (300, 70, 1), (300, 70, 0), (1024, 4096, 1)]:
        f, s = th.frame_layout(k, T, wd), th.streams_layout(k, T, wd)
        assert f.bytes == lib.cnl_track_frame_bytes(k, T, wd), (k, T, wd)
        assert s.bytes == lib.cnl_track_streams_record_bytes(k, T, wd), (k, T, wd)
        for S in (1, 4, 32):
            assert th.streams_workspace_bytes(S, k, S * T) == lib.cnl_track_streams_workspace_bytes(S, k, T), (S, k, T)
        assert all(x % 4 == 0 for x in f + s)
        # the float64 matrix, the streams' records themselves (stride), the (detection, track) pair list and every list that starts a section
        assert all(x % 8 == 0 for x in (f.off_index, f.off_dets, f.off_reid, s.off_index, s.off_dets, s.off_match, s.off_udet, s.bytes))
        # the unmatched-tracks list follows k int32: csrc/track_streams.hip (stream_rec) aligns it to 4 bytes only, e.g. for k = 7
        assert s.off_utrk == s.off_udet + 4 * k
        # the box matrix follows the re-ID matrix of the n the kernel found: 8-byte aligned for every n
        assert all((f.off_reid + 8 * n * T) % 8 == 0 for n in (0, 1, k))


@pytest.mark.parametrize("with_dets", [1, 0])
def test_record_readers_round_trip(with_dets):
    k, n, T = 7, 3, 2
    rng = np.random.default_rng(3)
    det_index = np.array([0, 2, 5], np.int32)
    boxes, scores = rng.random((k, 4)).astype(np.float32), rng.random(k).astype(np.float32)
    labels = rng.integers(0, 80, k).astype(np.int32)
    reid, box = rng.random((n, T)), rng.random((n, T)).astype(np.float32)

    def put(buf, off, a):
        buf[off:off + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).ravel()

    def put_dets(buf, off):
        put(buf, off, boxes)
        put(buf, off + 16 * k, scores)
        put(buf, off + 20 * k, labels)

    def check_dets(b, s, lab):
        if not with_dets:
            assert b is None and s is None and lab is None
            return
        assert b.dtype == np.float32 and b.shape == (k, 4) and np.array_equal(b, boxes)
        assert s.dtype == np.float32 and np.array_equal(s, scores)
        assert lab.dtype == np.int64 and np.array_equal(lab, labels)

    lay = th.frame_layout(k, T, with_dets)
    h = np.full(lay.bytes, 0xEE, np.uint8)
    hdr = np.zeros(8, np.int32)
    hdr[[th.F_N, th.F_K, th.F_T, th.F_WITH_DETS, th.F_OFF_INDEX, th.F_OFF_DETS, th.F_OFF_REID, th.F_OFF_BOX]] = \
        [n, k, T, with_dets, lay.off_index, lay.off_dets, lay.off_reid, lay.off_reid + 8 * n * T]
    put(h, 0, hdr)
    put(h, lay.off_index, det_index)
    if with_dets:
        put_dets(h, lay.off_dets)
    put(h, lay.off_reid, reid)
    put(h, lay.off_reid + 8 * n * T, box)
    got_n, got_index, b, s, lab, got_reid, got_box = th.read_frame_record(h, with_box=True)
    assert got_n == n and got_index.dtype == np.int32 and np.array_equal(got_index, det_index)
    check_dets(b, s, lab)
    assert got_reid.dtype == np.float64 and got_reid.shape == (n, T) and np.array_equal(got_reid, reid)
    assert got_box.dtype == np.float32 and got_box.shape == (n, T) and np.array_equal(got_box, box)
    assert th.read_frame_record(h, with_box=False)[6] is None
    h[:] = 0                                                            # what a Track keeps is a copy: the next frame overwrites the record
    assert np.array_equal(got_index, det_index) and (not with_dets or (np.array_equal(b, boxes) and np.array_equal(lab, labels)))

    matches, ud, ut = [(1, 0)], [0, 2], [1]
    lay = th.streams_layout(k, T + 3, with_dets)                        # a stream with fewer tracks than the step's T_max
    r = np.full(lay.bytes, 0xEE, np.uint8)
    hdr = np.zeros(16, np.int32)
    hdr[[th.S_N, th.S_K, th.S_T, th.S_STATUS, th.S_OFF_INDEX, th.S_OFF_DETS, th.S_OFF_MATCH, th.S_OFF_UDET, th.S_OFF_UTRK, th.S_M, th.S_M1,
         th.S_NUDET, th.S_NUTRK, th.S_WITH_DETS, th.S_SLOT, th.S_STREAM]] = \
        [n, k, T, 0, lay.off_index, lay.off_dets, lay.off_match, lay.off_udet, lay.off_utrk, len(matches), 1, len(ud), len(ut), with_dets, 4, 9]
    put(r, 0, hdr)
    put(r, lay.off_index, det_index)
    if with_dets:
        put_dets(r, lay.off_dets)
    put(r, lay.off_match, np.array(matches, np.int32))
    put(r, lay.off_udet, np.array(ud, np.int32))
    put(r, lay.off_utrk, np.array(ut, np.int32))
    got_n, got_T, status, got_index, b, s, lab, got_matches, got_ud, got_ut = th.read_stream_record(r)
    assert (got_n, got_T, status) == (n, T, 0) and got_index.dtype == np.int32 and np.array_equal(got_index, det_index)
    check_dets(b, s, lab)
    assert got_matches == matches and got_ud == ud and got_ut == ut
    assert all(type(x) is int for p in got_matches for x in p) and type(got_matches[0]) is tuple
    hdr[[th.S_STATUS, th.S_M, th.S_NUDET, th.S_NUTRK]] = [1, 0, 0, 0]   # non-finite costs: the device assigned nothing
    put(r, 0, hdr)
    assert th.read_stream_record(r)[2] == 1 and th.read_stream_record(r)[7:] == ([], [], [])


def test_two_stage_assignment_forms_agree():
    rng = np.random.default_rng(11)
    cases = []
    reid, box = 0.12 + rng.random((9, 6)), rng.random((9, 6)).astype(np.float32)     # few re-ID costs below 0.2: pairs remain for the boxes
    cases.append((reid, box))
    cases.append((np.full((9, 6), 0.1), np.full((9, 6), 0.25, np.float32)))          # equal costs: scipy's tie rule decides, in stage 1 ...
    cases.append((np.full((9, 6), 0.3), np.full((9, 6), 0.25, np.float32)))          # ... and in stage 2
    cases.append((np.where(rng.random((9, 6)) < 0.5, 0.1, 0.6), np.ones((9, 6), np.float32)))     # ... and box costs of disjoint boxes
    r2, b2 = reid.copy(), box.copy()
    r2[4, :] = np.inf                                                                # a detection no track may take
    b2[7, :] = np.inf
    cases.append((r2, b2))
    stage1 = stage2 = 0
    for reid, box in cases:
        m, ud, ut = th.match_with_threshold(reid, 0.2)
        new, ud2, ut2 = th.match_with_threshold(box[np.ix_(ud, ut)], 0.5)
        want = (m + [(ud[x], ut[y]) for x, y in new], [ud[x] for x in ud2], [ut[y] for y in ut2])
        stage1, stage2 = stage1 + len(m), stage2 + len(new)
        seen = []

        def sub_matrix(dets, tracks):
            seen.append((dets, tracks))
            return box[np.ix_(dets, tracks)]
        assert th.two_stage_assignment(reid, 0.2, 0.5, box) == want
        assert th.two_stage_assignment(reid, 0.2, 0.5, sub_matrix) == want
        assert seen == [(ud, ut)]                                                    # the callable sees the REMAINING pairs, once
        assert th.two_stage_assignment(reid, 0.2, 0.5, None) == (m, ud, ut)
    assert stage1 >= 8 and stage2 >= 8                                               # both stages really matched
    # no track yet: every kept detection is unmatched, scipy is not asked
    assert th.two_stage_assignment(np.zeros((4, 0)), 0.2, 0.5, np.zeros((4, 0), np.float32)) == ([], [0, 1, 2, 3], [])


@pytest.mark.parametrize("path", SEQS, ids=lambda p: os.path.basename(p)[6:-4])
def test_host_life_cycle_follows_the_oracle(path):
    g, seq, tk = load_case(path)
    ref = tracker_ref.Tracker(**tk)                                     # the settings with the reference's defaults; never updated
    settings = SimpleNamespace(min_birth_age=ref.min_birth_age, max_inactive_age=ref.max_inactive_age, smoothing_factor=ref.smoothing_factor,
                               use_kalman=False)
    g_ids, g_boxes = unpack(g, "ids"), unpack(g, "boxes")
    tracks, next_id = [], 0
    E = seq[0][3].shape[1]
    emb, box = np.zeros((0, E), np.float32), np.zeros((0, 4), np.float32)        # the track table, rows in the order of `tracks`
    births = 0
    for f, (bboxes, labels, scores, embeddings) in enumerate(seq):
        T = len(tracks)
        det_index = np.flatnonzero(scores >= ref.detection_threshold).astype(np.int32)
        reid = tracker_ref.cosine_distance_matrix(embeddings[det_index], emb) if T else np.zeros((len(det_index), 0))
        box_cost = ref.box_cost(bboxes[det_index], box) if ref.box_cost is not None and T else None
        lists = th.two_stage_assignment(reid, ref.reid_threshold, ref.box_threshold, box_cost)
        tracks, next_id, old_rows, det_rows = th.life_cycle(tracks, *lists, det_index, bboxes, labels, next_id, settings)
        # the row lists are what cnl_track_apply_f32 is given: consistent with the table they index
        assert len(old_rows) == len(det_rows) == len(tracks), f
        kept = [r for r in old_rows if r >= 0]
        assert all(-1 <= r < T for r in old_rows) and len(set(kept)) == len(kept) and kept == sorted(kept), f
        assert all(-1 <= d < len(scores) for d in det_rows), f
        for t, r, d in zip(tracks, old_rows, det_rows):
            if r < 0:
                births += 1
                assert d in det_index and t.birth_age == 0 and np.array_equal(t.bbox, bboxes[d]), f
        # cnl_track_apply_f32, restated: a birth takes the row-normalised detection embedding, a match mixes it in (tracker_ref.Track)
        new_emb, new_box = np.zeros((len(tracks), E), np.float32), np.zeros((len(tracks), 4), np.float32)
        for r, (t, d) in enumerate(zip(old_rows, det_rows)):
            if d < 0:
                new_emb[r], new_box[r] = emb[t], box[t]
                continue
            unit = embeddings[d] / np.linalg.norm(embeddings[d])
            new_emb[r] = unit if t < 0 else (1 - ref.smoothing_factor) * emb[t] + ref.smoothing_factor * unit
            new_box[r] = bboxes[d]
        emb, box = new_emb, new_box
        assert len(tracks) == int(g["n_tracks"][f]), f
        assert [t.track_id for t in tracks if t.active] == g_ids[f].tolist(), f
        assert np.array_equal(np.array([t.bbox for t in tracks if t.active], np.float32).reshape(-1, 4), g_boxes[f].reshape(-1, 4)), f
        assert np.array_equal(box, np.array([t.bbox for t in tracks], np.float32).reshape(-1, 4)), f
    assert births > 0 and next_id == births
    assert [t.track_id for t in tracks] == g["final_ids"].tolist()
    np.testing.assert_allclose(emb, g["final_emb"], rtol=0, atol=2e-6)             # the table's tolerance in tests/test_gpu_tracker.py
