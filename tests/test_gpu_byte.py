"""GPU: the BYTE low-score association (cnl_track_frame_low_f32, cnl_track_streams_low_f32, cnl_track_apply_keep_f32; Tracker / TrackerBank
with low_threshold).

Yardsticks: the entry points without the stage (byte for byte where the stage adds nothing), numpy for the low set, the existing
cnl_track_costs_f32 for the low detections' box costs (bit for bit), tests/byte_ref.py (the rule in numpy + scipy on oracle/tracker_ref.py)
for every assignment and for Tracker, one cl.Tracker per stream for TrackerBank (table rows bit-equal).

Shapes: k = 70 (more than one wave of rows in the assign loops, not a multiple of 4 for the compaction), E = 32, T in {0, 1, 65}, n_low in
{0, fewer than |U|, more than |U| (the transposed assignment)}, |U| = 0, duplicate boxes (equal costs: scipy's tie order), unsorted scores."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import byte_ref
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd import _track_host as th
from strided_io import GuardedBytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K, E = 70, 32
DET_THR, LOW_THR = 0.3, 0.1
STATES = (tracker_ref.TrackState.ACTIVE, tracker_ref.TrackState.INACTIVE, tracker_ref.TrackState.UNCONFIRMED)


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _ok(g, mask=None):
    ok, msg = g.verdict(mask)
    assert ok, msg


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _box(c, s):
    return [c[0] - s[0] / 2, c[1] - s[1] / 2, c[0] + s[0] / 2, c[1] + s[1] / 2]


def make_case(seed, T, high_on, high_free, low_on, low_free, dup=False, k=K):
    """One frame against T tracks, in random (unsorted) order: `high_on` confident detections on tracks 0.. with the track's embedding (stage 1),
    `high_free` confident ones elsewhere, `low_on` low-score ones on the NEXT tracks (random embeddings, jittered boxes), `low_free` low-score
    ones elsewhere, the rest below low_threshold.  dup: the last two tracks share one box and two low detections sit exactly on it.
    -> (det_emb, trk_emb, det_box, trk_box, score, track states)"""
    rng = np.random.default_rng(seed)
    assert high_on <= T and high_on + high_free + low_on + low_free <= k
    tb = np.array([_box(rng.random(2) * 0.8 + 0.1, rng.random(2) * 0.05 + 0.05) for _ in range(T)], np.float32).reshape(T, 4)
    te = rng.standard_normal((T, E)).astype(np.float32)
    if dup and T >= 2:
        tb[T - 1] = tb[T - 2]
    boxes, scores, embs = [], [], []
    for j in range(high_on):
        boxes.append(tb[j] + rng.standard_normal(4).astype(np.float32) * 0.002)
        scores.append(0.4 + 0.5 * rng.random())
        embs.append(te[j] + 0.05 * rng.standard_normal(E))
    for _ in range(high_free):
        boxes.append(_box(rng.random(2), rng.random(2) * 0.05 + 0.02))
        scores.append(0.4 + 0.5 * rng.random())
        embs.append(rng.standard_normal(E))
    for j in range(low_on):
        t = (high_on + j) % T if T else 0
        exact = dup and T >= 2 and j < 2
        base = tb[T - 2] if exact else tb[t] if T else np.array(_box(rng.random(2), [0.05, 0.05]), np.float32)
        boxes.append(base + (0 if exact else rng.standard_normal(4).astype(np.float32) * 0.003))
        scores.append(LOW_THR + (DET_THR - LOW_THR) * 0.98 * rng.random())
        embs.append(rng.standard_normal(E))
    for _ in range(low_free):
        boxes.append(_box(rng.random(2), rng.random(2) * 0.05 + 0.02))
        scores.append(LOW_THR + (DET_THR - LOW_THR) * 0.98 * rng.random())
        embs.append(rng.standard_normal(E))
    while len(boxes) < k:
        boxes.append(_box(rng.random(2), rng.random(2) * 0.05 + 0.02))
        scores.append(0.09 * rng.random())
        embs.append(rng.standard_normal(E))
    scores = np.asarray(scores, np.float32)
    if low_on + low_free:
        scores[high_on + high_free] = np.float32(LOW_THR)                   # exactly at the low threshold: in the low set (>=)
    order = rng.permutation(k)
    states = [STATES[t % 3] for t in range(T)]
    return (np.asarray(embs, np.float32)[order], te, np.asarray(boxes, np.float32)[order], tb, scores[order], states)


# T / n_low / |U| coverage: (name, T, high_on, high_free, low_on, low_free, dup)
CASES = [("T65_few_low", 65, 30, 6, 5, 2, False),          # n_low = 7 < |U| ~ 35
         ("T1_many_low", 1, 0, 8, 3, 9, False),            # n_low = 12 > |U| = 1: transposed
         ("T0", 0, 0, 10, 0, 6, False),
         ("T65_no_low", 65, 30, 6, 0, 0, False),           # n_low = 0
         ("T4_no_U", 4, 4, 3, 5, 2, False),                # every track matched in stage 1: |U| = 0
         ("T65_dup_many_low", 65, 25, 1, 40, 4, True)]     # n_low = 44 > |U| = 40, duplicate boxes: ties


def expected(case, box_cost, low_match, low_thr=LOW_THR, low_box_thr=0.5):
    """byte_ref on the case: (matches, unmatched detection rows, unmatched tracks, low matches), tracks pre-set with the case's table."""
    de, te, db, tb, score, states = case
    trk = byte_ref.Tracker(low_threshold=low_thr, low_box_threshold=low_box_thr, low_match=low_match, box_cost=box_cost)
    for t in range(len(te)):
        x = tracker_ref.Track(t, tb[t], 0, te[t])
        x.embedding, x.state = te[t], states[t]
        trk.tracks.append(x)
    trk.next_track_id = len(te)
    with np.errstate(all="ignore"):
        trk.update(db, np.zeros(len(db), np.int64), score, de)
    return trk.last_matches, trk.last_unmatched_dets, trk.last_unmatched_tracks, trk.last_low_matches


# ----------------------------------------------------------------------------------------------------------------------- the frame record
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name,T,high_on,high_free,low_on,low_free,dup", CASES, ids=[c[0] for c in CASES])
def test_frame_low_record(name, T, high_on, high_free, low_on, low_free, dup, mode):
    lib = _lib.load()
    de, te, db, tb, score, _ = make_case(11, T, high_on, high_free, low_on, low_free, dup)
    score = score.copy()
    score[np.flatnonzero(score < 0.09)[:2]] = np.nan                                       # a NaN score belongs to neither set
    labels = np.random.default_rng(1).integers(0, 80, K)
    d_de, d_db, d_s, d_lab = _dev(de), _dev(db), _dev(score), _dev(labels.astype(np.int64))
    d_te, d_tb = (_dev(te), _dev(tb)) if T else (None, None)
    tp = lambda t: t.data_ptr() if t is not None else None
    old_need, need = int(lib.cnl_track_frame_bytes(K, T, 1)), int(lib.cnl_track_frame_low_bytes(K, T, 1))
    old = GuardedBytes(old_need, align=8, device=DEV, name="frame record")
    rec = GuardedBytes(need, align=8, device=DEV, name="frame low record")
    _lib.check(lib.cnl_track_frame_f32(d_de.data_ptr(), d_db.data_ptr(), d_s.data_ptr(), d_lab.data_ptr(), 1, K, E, DET_THR, tp(d_te), tp(d_tb), T, mode, 0, 1,
                                       old.ptr, old_need, _stream()))
    _lib.check(lib.cnl_track_frame_low_f32(d_de.data_ptr(), d_db.data_ptr(), d_s.data_ptr(), d_lab.data_ptr(), 1, K, E, DET_THR, LOW_THR, tp(d_te), tp(d_tb), T,
                                           mode, 0, 1, rec.ptr, need, _stream()))
    torch.cuda.synchronize()
    _ok(old)
    _ok(rec)
    h0, h = old.body.cpu().numpy(), rec.body.cpu().numpy()
    a, b = h0[:32].view(np.int32).tolist(), h[:48].view(np.int32).tolist()
    n = a[0]
    assert b[:4] == a[:4] and b[4] == 48 and b[11] == 0
    # every section of the plain record, byte for byte
    for off0, off1, size in ((a[4], b[4], 4 * n), (a[5], b[5], 24 * K), (a[6], b[6], 8 * n * T), (a[7], b[7], 4 * n * T)):
        assert np.array_equal(h0[off0:off0 + size], h[off1:off1 + size])
    low = np.flatnonzero((score >= np.float32(LOW_THR)) & (score < np.float32(DET_THR)))
    n_low, off_li, off_lb = b[8], b[9], b[10]
    assert n_low == len(low) == low_on + low_free and off_li == b[7] + 4 * n * T and off_lb == off_li + 4 * K
    assert np.array_equal(h[off_li:off_li + 4 * n_low].view(np.int32), low)
    assert off_lb + 4 * n_low * T <= need
    # low_box: the rows of the box matrix the existing cost entry gives when its threshold is the low one
    if T:
        n_all = torch.full((1,), -1, device=DEV, dtype=torch.int32)
        idx = torch.full((K,), -1, device=DEV, dtype=torch.int32)
        reid = torch.zeros(K * T, device=DEV, dtype=torch.float64)
        box = torch.zeros(K * T, device=DEV, dtype=torch.float32)
        _lib.check(lib.cnl_track_costs_f32(d_de.data_ptr(), d_db.data_ptr(), d_s.data_ptr(), K, E, LOW_THR, d_te.data_ptr(), d_tb.data_ptr(), T, mode,
                                           n_all.data_ptr(), idx.data_ptr(), reid.data_ptr(), box.data_ptr(), _stream()))
        torch.cuda.synchronize()
        m = int(n_all.item())
        kept = idx.cpu().numpy()[:m]
        rows = np.flatnonzero(np.isin(kept, low))
        assert np.array_equal(kept[rows], low)
        want = box.cpu().numpy()[:m * T].reshape(m, T)[rows]
        got = h[off_lb:off_lb + 4 * n_low * T].view(np.float32).reshape(n_low, T)
        assert np.array_equal(_bits(got), _bits(want))
    # read through the host module: the same tuple as the plain reader, then the two sections
    out = th.read_frame_low_record(h)
    assert out[0] == n and np.array_equal(out[7], low) and out[8].shape == (n_low, T)
    written = off_lb + 4 * n_low * T
    assert (rec.body[written:].cpu().numpy() == rec.sentinel).all()                         # nothing behind the low_box rows the kernel found


# ----------------------------------------------------------------------------------------------------------------------- the streams entry
def _low_mask(r, stride):
    """The bytes of one live stream's low record the kernels may write, from the record's own header."""
    hdr = r[:96].view(np.int32).tolist()
    m = torch.zeros(stride, dtype=torch.bool)
    m[:96] = True
    m[hdr[th.S_OFF_INDEX]:hdr[th.S_OFF_INDEX] + 4 * hdr[th.S_N]] = True
    if hdr[th.S_WITH_DETS]:
        m[hdr[th.S_OFF_DETS]:hdr[th.S_OFF_DETS] + 24 * hdr[th.S_K]] = True
    m[hdr[th.S_OFF_MATCH]:hdr[th.S_OFF_MATCH] + 8 * hdr[th.S_M]] = True
    m[hdr[th.S_OFF_UDET]:hdr[th.S_OFF_UDET] + 4 * hdr[th.S_NUDET]] = True
    m[hdr[th.S_OFF_UTRK]:hdr[th.S_OFF_UTRK] + 4 * hdr[th.S_NUTRK]] = True
    m[hdr[th.S_OFF_LOW_INDEX]:hdr[th.S_OFF_LOW_INDEX] + 4 * hdr[th.S_NLOW]] = True
    m[hdr[th.S_OFF_LOW_MATCH]:hdr[th.S_OFF_LOW_MATCH] + 8 * hdr[th.S_NLOW_MATCH]] = True
    return m


class _Streams:
    """The six cases as six live streams of seven (stream 2 takes no part, and owns rows), in a live order that is not the stream order."""

    def __init__(self, mode):
        self.mode = mode
        self.S, self.live = 7, [5, 0, 6, 3, 1, 4]
        self.cases = [make_case(40 + i, *c[1:]) for i, c in enumerate(CASES)]
        T_of = [0] * self.S
        for i, s in enumerate(self.live):
            T_of[s] = len(self.cases[i][1])
        T_of[2] = 9
        self.T_of = T_of
        self.off = np.concatenate([[0], np.cumsum(T_of)]).astype(np.int32)
        self.R, self.T_max = int(self.off[-1]), 65
        rng = np.random.default_rng(2)
        pool_e, pool_b = rng.standard_normal((self.R, E)).astype(np.float32), rng.random((self.R, 4)).astype(np.float32)
        self.states = [tracker_ref.TrackState.ACTIVE] * self.R
        for i, s in enumerate(self.live):
            lo, hi = self.off[s], self.off[s + 1]
            pool_e[lo:hi], pool_b[lo:hi] = self.cases[i][1], self.cases[i][3]
            self.states[lo:hi] = self.cases[i][5]
        self.ops = [_dev(np.stack([c[j] for c in self.cases])) for j in (0, 2, 4)] + [_dev(pool_e), _dev(pool_b)]
        self.live_d, self.off_d = _dev(np.array(self.live, np.int32)), _dev(self.off)
        self.snap = [t.clone() for t in self.ops]

    def run(self, eligible, low=True, low_thr=LOW_THR, gap=40):
        """-> (records uint8 [S * stride], stride); guards, gaps, non-live records and the workspace past its size checked here."""
        lib = _lib.load()
        S, T_max = self.S, self.T_max
        ws_bytes = int((lib.cnl_track_streams_low_workspace_bytes if low else lib.cnl_track_streams_workspace_bytes)(S, K, T_max))
        rec_bytes = int((lib.cnl_track_streams_low_record_bytes if low else lib.cnl_track_streams_record_bytes)(K, T_max, 1))
        stride = rec_bytes + gap
        ws = GuardedBytes(ws_bytes, align=8, device=DEV, name="streams workspace")
        rec = GuardedBytes(S * stride, align=8, device=DEV, name="stream records")
        de, db, ds, pe, pb = self.ops
        head = (de.data_ptr(), db.data_ptr(), ds.data_ptr(), None, 0, S, len(self.live), self.live_d.data_ptr(), K, E, DET_THR, 0.2, 0.5)
        tail = (self.R, T_max, self.mode, 0, 1, ws.ptr, ws_bytes, rec.ptr, stride, _stream())
        if low:
            el = None if eligible is None else _dev(np.asarray(eligible, np.uint8))
            rc = lib.cnl_track_streams_low_f32(*head, low_thr, 0.5, pe.data_ptr(), pb.data_ptr(), self.off_d.data_ptr(), el.data_ptr() if el is not None else None, *tail)
        else:
            rc = lib.cnl_track_streams_f32(*head, pe.data_ptr(), pb.data_ptr(), self.off_d.data_ptr(), *tail)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        _ok(ws)
        h = rec.body.cpu().numpy().copy()
        mask = torch.zeros(S * stride, dtype=torch.bool)
        for s in self.live:
            r = h[s * stride:(s + 1) * stride]
            mask[s * stride:(s + 1) * stride] = _low_mask(r, stride) if low else torch.from_numpy(np.arange(stride) < rec_bytes)
            assert not mask[s * stride + rec_bytes:(s + 1) * stride].any()
        _ok(rec, mask)                                                                      # gaps and the records of stream 2 untouched
        assert all(torch.equal(a, b) for a, b in zip(self.ops, self.snap))
        return h, stride


@pytest.mark.parametrize("mode,box_cost", [(1, "iou"), (2, "giou")])
def test_streams_low_equals_the_rule(mode, box_cost):
    st = _Streams(mode)
    h_null, stride = st.run(None)
    h_ones, _ = st.run([1] * st.R)
    assert np.array_equal(h_null, h_ones)                                                   # null = every row eligible: the same bytes
    active = [s is tracker_ref.TrackState.ACTIVE for s in st.states]
    h_act, _ = st.run(active)
    h_zero, _ = st.run([0] * st.R)
    h_plain, stride_plain = st.run(None, low=False)
    seen = set()
    for h, low_match in ((h_null, "all"), (h_act, "active")):
        for i, s in enumerate(st.live):
            want = expected(st.cases[i], box_cost, low_match)
            n, T, status, idx, _, _, _, matches, udet, utrk, n_low, low_matches = th.read_stream_low_record(h[s * stride:(s + 1) * stride])
            score = st.cases[i][4]
            assert status == 0 and T == st.T_of[s] and np.array_equal(idx, np.flatnonzero(score >= np.float32(DET_THR))), (s, status)
            assert n_low == int(((score >= np.float32(LOW_THR)) & (score < np.float32(DET_THR))).sum())
            assert (matches, udet, utrk, low_matches) == tuple(list(x) for x in want), (CASES[i][0], low_match)
            hdr = h[s * stride:s * stride + 96].view(np.int32)
            assert hdr[th.S_SLOT] == i and hdr[th.S_STREAM] == s and not hdr[20:24].any()
            U = T - len(matches)
            seen.add("T=%d" % T)
            seen.add("n_low=0" if n_low == 0 else "U=0" if U == 0 else "n_low<U" if n_low < U else "n_low>U")
            if low_matches:
                seen.add("matched")
            if CASES[i][0] == "T65_dup_many_low" and low_match == "all":
                assert len(low_matches) >= 30 and {T - 1, T - 2} <= {t for _, t in low_matches}       # the tied pairs were assigned, in scipy's order
    assert seen >= {"T=0", "T=1", "T=65", "n_low=0", "U=0", "n_low<U", "n_low>U", "matched"}, seen
    # no eligible row: no low match, and the lists of the plain entry
    for i, s in enumerate(st.live):
        a = th.read_stream_low_record(h_zero[s * stride:(s + 1) * stride])
        b = th.read_stream_record(h_plain[s * stride_plain:(s + 1) * stride_plain])
        assert a[11] == [] and a[:3] == b[:3] and np.array_equal(a[3], b[3]), s
        assert a[7:10] == b[7:10], s
        hz = h_zero[s * stride:s * stride + 96].view(np.int32)
        assert hz[th.S_NLOW_MATCH] == 0 and hz[th.S_NLOW] == a[10]


def test_streams_low_with_an_empty_low_set_gives_the_plain_lists():
    st = _Streams(1)
    h, stride = st.run(None, low_thr=DET_THR)                                               # low_threshold == detection_threshold: L is empty
    h_plain, stride_plain = st.run(None, low=False)
    for s in st.live:
        a = th.read_stream_low_record(h[s * stride:(s + 1) * stride])
        b = th.read_stream_record(h_plain[s * stride_plain:(s + 1) * stride_plain])
        assert a[10] == 0 and a[11] == [] and a[7:10] == b[7:10] and np.array_equal(a[3], b[3]), s


# ----------------------------------------------------------------------------------------------------------------------- the table update
def test_apply_keep():
    lib = _lib.load()
    rng = np.random.default_rng(3)
    T, k = 9, 20
    old_e, old_b = rng.standard_normal((T, E)).astype(np.float32), rng.random((T, 4)).astype(np.float32)
    det_e, det_b = rng.standard_normal((k, E)).astype(np.float32), rng.random((k, 4)).astype(np.float32)
    src_trk = np.array([0, 2, 3, -1, 8, -1, 5, 6], np.int32)
    src_det = np.array([-1, 4, 11, 7, 19, 0, -1, 3], np.int32)
    keep = np.array([1, 1, 0, 1, 1, 0, 1, 0], np.uint8)            # set on a carried row (0, 6) and on a birth (3) too: no effect there
    rows = len(src_trk)
    oe, ob, de, db, st, sd, kp = map(_dev, (old_e, old_b, det_e, det_b, src_trk, src_det, keep))

    def run(fn, *extra):
        ne, nb = GuardedBytes(rows * E * 4, align=4, device=DEV, name="new_emb"), GuardedBytes(rows * 16, align=4, device=DEV, name="new_box")
        _lib.check(fn(oe.data_ptr(), ob.data_ptr(), de.data_ptr(), db.data_ptr(), st.data_ptr(), sd.data_ptr(), rows, E, 0.3, ne.ptr, nb.ptr, *extra, _stream()))
        torch.cuda.synchronize()
        _ok(ne)
        _ok(nb)
        return ne.result(torch.float32, (rows, E)), nb.result(torch.float32, (rows, 4))
    plain = run(lib.cnl_track_apply_f32)
    null = run(lib.cnl_track_apply_keep_f32, None)
    no_keep = _dev(np.zeros(rows, np.uint8))                        # (named: the flags must outlive the launch)
    zeros = run(lib.cnl_track_apply_keep_f32, no_keep.data_ptr())
    assert torch.equal(null[0], plain[0]) and torch.equal(null[1], plain[1])
    assert torch.equal(zeros[0], plain[0]) and torch.equal(zeros[1], plain[1])
    ne, nb = (x.numpy() for x in run(lib.cnl_track_apply_keep_f32, kp.data_ptr()))
    pe, pb = (x.numpy() for x in plain)
    for r, (t, d, kf) in enumerate(zip(src_trk, src_det, keep)):
        if t >= 0 and d >= 0 and kf:
            assert np.array_equal(_bits(ne[r]), _bits(old_e[t])) and np.array_equal(_bits(nb[r]), _bits(det_b[d])), r     # old embedding, new box
            assert not np.array_equal(ne[r], pe[r])
        else:
            assert np.array_equal(_bits(ne[r]), _bits(pe[r])) and np.array_equal(_bits(nb[r]), _bits(pb[r])), r
    # through the table object: the flags travel as one more row of the mapped index block
    table = th.TrackTable()
    cur = torch.cuda.current_stream(torch.device(DEV))
    with torch.cuda.device(DEV):
        table.apply(np.full(T, -1, np.int32), np.arange(T, dtype=np.int32), de, db, E, 0.3, cur)            # T births
        first = table.emb[:T].clone()
        table.apply(src_trk, src_det, de, db, E, 0.3, cur, keep_emb=keep)
        cur.synchronize()
    for r, (t, d, kf) in enumerate(zip(src_trk, src_det, keep)):
        if t >= 0 and d >= 0 and kf:
            assert torch.equal(table.emb[r], first[t]) and np.array_equal(table.box[r].cpu().numpy(), det_b[d])


# ----------------------------------------------------------------------------------------------------------------------- Tracker
def _check_tracker(trk, ref, tag, kalman):
    assert [t.track_id for t in trk.tracks] == [t.track_id for t in ref.tracks], tag
    assert [t.state.name for t in trk.tracks] == [t.state.name for t in ref.tracks], tag
    assert [tuple(p) for p in trk.last_matches] == [tuple(p) for p in ref.last_matches], tag
    assert [tuple(p) for p in trk.last_low_matches] == [tuple(p) for p in ref.last_low_matches], tag
    a = np.array([np.asarray(t.bbox, np.float64) for t in trk.tracks]).reshape(-1, 4)
    b = np.array([np.asarray(t.bbox, np.float64) for t in ref.tracks]).reshape(-1, 4)
    if kalman:
        np.testing.assert_allclose(a, b, rtol=0, atol=1e-6, err_msg=str(tag))              # float32 table vs float64 filter state
    else:
        assert np.array_equal(a, b), tag
    if trk.tracks:
        emb = trk.track_embeddings().cpu().numpy()
        np.testing.assert_allclose(emb, np.stack([t.embedding for t in ref.tracks]), rtol=0, atol=2e-6, err_msg=str(tag))


@pytest.mark.parametrize("use_kalman", [False, "host", "device"])
@pytest.mark.parametrize("sort_scores", [True, False], ids=["sorted", "unsorted"])
@pytest.mark.parametrize("low_match", ["active", "all"])
@pytest.mark.parametrize("box_cost", ["iou", "giou"])
def test_tracker_equals_the_rule(box_cost, low_match, sort_scores, use_kalman):
    seq, _ = byte_ref.synth_occlusion(7, frames=30, objects=6, k=K, emb_dim=E, sort_scores=sort_scores)
    kw = dict(box_cost=box_cost, box_threshold=0.5 if box_cost == "iou" else 0.7, use_kalman=bool(use_kalman))
    trk = _quiet(cl.Tracker, device=DEV, low_threshold=LOW_THR, low_match=low_match, kalman=use_kalman or "host", **kw)
    ref = byte_ref.Tracker(low_threshold=LOW_THR, low_match=low_match, **kw)
    low = 0
    for f, fr in enumerate(seq):
        trk.update(*(fr if f % 2 else [torch.from_numpy(a).to(DEV) for a in fr]))          # device tensors and numpy inputs on alternating frames
        ref.update(*fr)
        _check_tracker(trk, ref, (f,), use_kalman)
        low += len(trk.last_low_matches)
        assert trk.d2h_bytes > 0
    if sort_scores:
        assert low == 24                                                                    # every occluded object-frame was matched in the new stage
    elif low_match == "all":
        assert low > 0


def test_low_threshold_at_the_detection_threshold_is_the_tracker_without_the_stage():
    seq, _ = byte_ref.synth_occlusion(3, k=K, emb_dim=E)
    a = _quiet(cl.Tracker, device=DEV, low_threshold=DET_THR)
    b = _quiet(cl.Tracker, device=DEV, low_threshold=None)
    bank_a = _quiet(cl.TrackerBank, num_streams=2, device=DEV, low_threshold=DET_THR)
    bank_b = _quiet(cl.TrackerBank, num_streams=2, device=DEV)
    for f, fr in enumerate(seq):
        a.update(*fr)
        b.update(*fr)
        two = [np.stack([x, x]) for x in fr]
        bank_a.update_batch(*two)
        bank_b.update_batch(*two)
        assert a.last_low_matches == [] and b.last_low_matches is None and bank_a.last_low_matches == [[], []] and bank_b.last_low_matches == [None, None]
        assert a.last_matches == b.last_matches and bank_a.last_matches == bank_b.last_matches
        assert [(t.track_id, t.state, np.asarray(t.bbox).tobytes()) for t in a.tracks] == [(t.track_id, t.state, np.asarray(t.bbox).tobytes()) for t in b.tracks], f
        assert torch.equal(a.track_embeddings(), b.track_embeddings()) and torch.equal(a._box[:len(a.tracks)], b._box[:len(b.tracks)])
        for s in range(2):
            assert torch.equal(bank_a.track_embeddings(s), bank_b.track_embeddings(s)) and torch.equal(bank_a.track_embeddings(s), b.track_embeddings())


# ----------------------------------------------------------------------------------------------------------------------- TrackerBank
def _stack(frames, as_torch):
    cols = [np.stack([fr[j] for fr in frames]) for j in range(4)]
    return [torch.from_numpy(c).to(DEV) for c in cols] if as_torch else cols


def _check_bank_stream(bank, s, trk, tag):
    st = bank[s]
    assert [t.track_id for t in st.tracks] == [t.track_id for t in trk.tracks], tag
    assert [(t.state, t.birth_age, t.inactive_age) for t in st.tracks] == [(t.state, t.birth_age, t.inactive_age) for t in trk.tracks], tag
    assert [np.asarray(t.bbox).tobytes() for t in st.tracks] == [np.asarray(t.bbox).tobytes() for t in trk.tracks], tag
    assert st.next_track_id == trk.next_track_id, tag
    if trk.tracks:
        lo, hi = int(bank._off[s]), int(bank._off[s + 1])
        assert torch.equal(bank.track_embeddings(s), trk.track_embeddings()), tag           # same kernels, same order: bit-equal rows
        assert torch.equal(bank._box[lo:hi], trk._box[:len(trk.tracks)]), tag


@pytest.mark.parametrize("use_kalman", [False, "host", "device"])
@pytest.mark.parametrize("low_match", ["active", "all"])
@pytest.mark.parametrize("S", [1, 5])
def test_bank_equals_independent_trackers(S, low_match, use_kalman):
    frames = 26
    kw = dict(low_threshold=LOW_THR, low_match=low_match, use_kalman=bool(use_kalman), kalman=use_kalman or "host")
    seqs = [byte_ref.synth_occlusion(20 + s, frames=frames, objects=3 + s, k=K, emb_dim=E, sort_scores=s != 3)[0] for s in range(S)]
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **kw)
    trks = [_quiet(cl.Tracker, device=DEV, **kw) for _ in range(S)]
    nxt = [0] * S
    low = 0

    def step(live, as_torch):
        nonlocal low
        fr = [seqs[s][nxt[s]] for s in live]
        bank.update_batch(*_stack(fr, as_torch), streams=None if len(live) == S and live == sorted(live) else live)
        for s, x in zip(live, fr):
            trks[s].update(*x)
            nxt[s] += 1
            assert [tuple(p) for p in bank.last_matches[s]] == [tuple(p) for p in trks[s].last_matches], (live, s)
            assert [tuple(p) for p in bank.last_low_matches[s]] == [tuple(p) for p in trks[s].last_low_matches], (live, s)
            low += len(bank.last_low_matches[s])
        for s in range(S):
            _check_bank_stream(bank, s, trks[s], (live, s, nxt[s]))
        assert bank.d2h_bytes > 0

    for f in range(12):
        step(list(range(S)), as_torch=f % 2 == 0)
    if S > 1:
        step([3, 0], True)                                                                  # a partial step, in another order
        step([1, 4, 2], False)
        bank.reset(stream=1)
        trks[1].reset()
        nxt[1] = 0
        assert bank.last_low_matches[1] is None
    for f in range(10):
        step(list(range(S)), as_torch=f % 2 == 1)
    assert low > 0


def test_nan_box_in_a_low_detection_is_status_33_and_raises_what_tracker_raises():
    S = 3
    kw = dict(low_threshold=LOW_THR, low_match="all")
    seqs = [byte_ref.synth_occlusion(30 + s, frames=8, objects=4, k=K, emb_dim=E)[0] for s in range(S)]
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **kw)
    trks = [_quiet(cl.Tracker, device=DEV, **kw) for _ in range(S)]
    for f in range(6):                                                                      # frame 5: the first object's dip has begun
        bank.update_batch(*_stack([seqs[s][f] for s in range(S)], True))
        for s in range(S):
            trks[s].update(*seqs[s][f])
    assert sum(len(x) for x in bank.last_low_matches) > 0
    bad = 1
    fr = [list(seqs[s][6]) for s in range(S)]
    score = fr[bad][2]
    lows = np.flatnonzero((score >= np.float32(LOW_THR)) & (score < np.float32(DET_THR)))
    assert len(lows) >= 2
    fr[bad][0] = fr[bad][0].copy()
    fr[bad][0][lows[-1], 2] = np.nan                                                        # one coordinate of one low detection
    with pytest.raises(ValueError) as want:
        trks[bad].update(*fr[bad])

    def snapshot(s):
        st = bank[s]
        return ([(t.track_id, t.state.name, t.birth_age, t.inactive_age, np.asarray(t.bbox).tobytes()) for t in st.tracks], st.frame, st.next_track_id,
                bank.track_embeddings(s).clone())
    before = [snapshot(s) for s in range(S)]
    T_max = max(len(bank[s].tracks) for s in range(S))
    with pytest.raises(ValueError) as got:
        bank.update_batch(*_stack(fr, True))
    assert str(got.value) == str(want.value)
    stride = th.streams_low_layout(K, T_max, True).bytes
    status = [int(bank._rec.np[s * stride:s * stride + 96].view(np.int32)[th.S_STATUS]) for s in range(S)]
    assert status == [0, 33, 0]                                                             # a status word of that stream alone, not a fault
    for s in range(S):
        after = snapshot(s)
        assert before[s][:3] == after[:3] and torch.equal(before[s][3], after[3]), s       # every stream as it was
    bank.update_batch(*_stack([seqs[s][6] for s in range(S)], True))                        # and the bank goes on with a clean frame
    for s in range(S):
        trks[s].update(*seqs[s][6])
        _check_bank_stream(bank, s, trks[s], ("after", s))


# ----------------------------------------------------------------------------------------------------------------------- the effect, measured
def test_mot_evaluator_counts_fewer_misses_with_the_stage():
    seq, truth = byte_ref.synth_occlusion(4, frames=30, objects=6, k=K, emb_dim=E)
    xywh = lambda b: np.concatenate([b[:, :2], b[:, 2:] - b[:, :2]], 1) if len(b) else np.zeros((0, 4))
    res = {}
    for low in (None, LOW_THR):
        trk = _quiet(cl.Tracker, device=DEV, low_threshold=low)
        pb, pi = [], []
        for fr in seq:
            trk.update(*fr)
            act = [t for t in trk.tracks if t.active]
            pb.append(xywh(np.array([np.asarray(t.bbox, np.float64) for t in act]).reshape(-1, 4)))
            pi.append(np.array([t.track_id for t in act], np.int64))
        ev = cl.MotEvaluator(device=DEV)
        ev.update(pb, pi, [xywh(g) for g in truth], [np.arange(len(g)) for g in truth])
        res[low] = ev.get_metrics()["sequence_0"]
        print(f"low_threshold={low}: CLR_FN {res[low]['CLR_FN']}, IDSW {res[low]['IDSW']}, MOTA {res[low]['MOTA']:.4f}")
    assert res[LOW_THR]["CLR_FN"] < res[None]["CLR_FN"]
    assert res[LOW_THR]["IDSW"] <= res[None]["IDSW"]
