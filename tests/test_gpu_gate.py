"""GPU: class-aware and Kalman-gated association (cnl_track_frame_gated_f32 / cnl_track_streams_gated_f32; `class_aware`, `motion_gate`,
`motion_weight` of Tracker / TrackerBank).

Yardsticks: tests/gate_ref.py — the header's rule pair by pair in Python floats, applied to the matrices the UNGATED entries write for the same
inputs, and the reference tracking loop built from it — and the `_low` entries themselves for everything the gates do not touch.  Every comparison
is an equality (bit patterns for the costs and boxes)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import gate_ref
import kalman_ref
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd import _track_host as th
from strided_io import SENTINEL_BYTE, GuardedBytes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 12
DET_THR, LOW_THR = 0.3, 0.1
KAL = dict(use_kalman=True, kalman="device")
GATES = {"class": (True, None, 1.0), "motion": (False, 9.4877, 1.0), "both": (True, 9.4877, 1.0), "weight": (True, 9.4877, 0.98)}
LABEL_DTYPES = {1: np.int64, 2: np.int32, 3: np.float32}


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
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _ptr(t):
    return t.data_ptr() if t is not None else None


# ----------------------------------------------------------------------------------------------------------------------- cases
def make_case(T, E, seed, cross_all=False, flat_track=False, nan_det=False):
    """K detections against T tracks of 3 classes whose filter states went through birth, a prediction, an update and a prediction (P has its
    off-diagonal blocks).  Detections 0..: on the predicted box of track j % T with a jitter inside the gate for two in three, a few box sizes
    away for the others; the label is the track's for two in three.  Seven scores >= DET_THR, three in [LOW_THR, DET_THR), two below, in random
    order.  cross_all: every detection is class 0, every track class 1.  flat_track: track 0 has the state a birth from a zero-area box leaves (P = 0: no positive
    pivot).  nan_det: one coordinate of the first kept detection is NaN."""
    rng = np.random.default_rng(seed)
    c, s = rng.uniform(0.2, 0.8, (T, 2)), rng.uniform(0.05, 0.2, (T, 2))
    born = np.concatenate([c - s / 2, c + s / 2], 1).astype(np.float32).reshape(T, 4)
    kx, kP = kalman_ref.init(born)
    kx, kP = kalman_ref.predict(kx, kP)
    with np.errstate(all="ignore"):
        ux, uP, ok = kalman_ref.update(kx, kP, (born + rng.standard_normal((T, 4)).astype(np.float32) * 0.004).astype(np.float32))
    kx, kP = kalman_ref.predict(ux, uP)
    trk_label = rng.integers(0, 3, T).astype(np.int32)
    trk_emb = rng.standard_normal((T, E)).astype(np.float32)
    trk_box = kx[:, :4].astype(np.float32).reshape(T, 4)
    det_box, det_emb, labels = [], [], []
    for j in range(K):
        if T:
            t = j % T
            w = kx[t, 2:4] - kx[t, 0:2]
            far = j % 3 == 2
            jitter = rng.standard_normal(4) * (np.tile(w, 2) * (2.0 if far else 0.02))
            det_box.append(kx[t, :4] + jitter)
            det_emb.append(trk_emb[t] + 0.05 * rng.standard_normal(E))
            labels.append(int(trk_label[t]) if j % 3 != 1 else int(rng.integers(0, 3)))
        else:
            cc, ss = rng.uniform(0.2, 0.8, 2), rng.uniform(0.05, 0.2, 2)
            det_box.append(np.concatenate([cc - ss / 2, cc + ss / 2]))
            det_emb.append(rng.standard_normal(E))
            labels.append(int(rng.integers(0, 3)))
    score = np.concatenate([rng.uniform(0.35, 0.95, 7), rng.uniform(0.12, 0.28, 3), rng.uniform(0.0, 0.08, 2)]).astype(np.float32)
    order = rng.permutation(K)
    det_box, det_emb = np.asarray(det_box, np.float32)[order], np.asarray(det_emb, np.float32)[order]
    labels, score = np.asarray(labels, np.int64)[order], score[order]
    if cross_all:
        labels[:], trk_label[:] = 0, 1
    kP = kP.reshape(T, 64)
    if flat_track and T:                   # what a birth from a zero-area box leaves: zero width and height, P = 0 (the other tracks and the detections stay)
        kx[0, 2:4], kx[0, 4:], kP[0] = kx[0, 0:2], 0.0, 0.0
        trk_box[0] = kx[0, :4].astype(np.float32)
    if nan_det:
        det_box[np.flatnonzero(score >= np.float32(DET_THR))[0], 2] = np.nan
    return dict(det_emb=det_emb, det_box=det_box, score=score, labels=labels, trk_emb=trk_emb, trk_box=trk_box, trk_label=trk_label, kx=kx,
                kP=kP, T=T, E=E)


def _gate_struct(case, cls, motion_gate, weight, keep):
    """A _lib.TrackGate over the case's tables on the device (`keep` holds the tensors)."""
    g = _lib.TrackGate(None, None, None, 0.0, 1.0)
    if case["T"] == 0:
        return g
    if cls:
        keep.append(_dev(case["trk_label"]))
        g.trk_label = keep[-1].data_ptr()
    if motion_gate is not None:
        keep.extend([_dev(case["kx"]), _dev(case["kP"])])
        g.kx, g.kP, g.motion_gate, g.motion_weight = keep[-2].data_ptr(), keep[-1].data_ptr(), motion_gate, weight
    return g


def run_frame(case, gate, label_kind=1, mode=1, low_thr=LOW_THR):
    """One guarded launch of the `_low` entry (gate None) or the gated one (gate: "off", "null" or (class, motion_gate, weight))
    -> the record's bytes as numpy."""
    lib = _lib.load()
    T, E = case["T"], case["E"]
    ops = [_dev(case[n]) for n in ("det_emb", "det_box", "score")] + [_dev(case["labels"].astype(LABEL_DTYPES[label_kind]))]
    tab = [_dev(case["trk_emb"]), _dev(case["trk_box"])] if T else [None, None]
    need = int(lib.cnl_track_frame_low_bytes(K, T, 1))
    rec = GuardedBytes(need, align=8, device=DEV, name="frame record")
    args = (*(t.data_ptr() for t in ops), label_kind, K, E, DET_THR, low_thr, _ptr(tab[0]), _ptr(tab[1]), T, mode, 0, 1, rec.ptr, need)
    keep = []
    if gate is None:
        rc = lib.cnl_track_frame_low_f32(*args, _stream())
    elif gate == "null":
        rc = lib.cnl_track_frame_gated_f32(*args, None, _stream())
    else:
        g = _lib.TrackGate(None, None, None, 0.0, 1.0) if gate == "off" else _gate_struct(case, *gate, keep)
        rc = lib.cnl_track_frame_gated_f32(*args, ctypes.byref(g), _stream())
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    _ok(rec)
    return rec.body.cpu().numpy().copy()


def _expected(case, reid, box, low_box, det_index, low_index, gate):
    cls, motion_gate, weight = gate
    with np.errstate(all="ignore"):
        return gate_ref.gate_costs(reid, box, low_box, case["labels"], case["trk_label"] if cls else None, case["det_box"],
                                   case["kx"] if motion_gate is not None else None, case["kP"], motion_gate, weight, det_index, low_index)


def _same_matrix(got, want, tag):
    """Bit-equal, a NaN counting as equal to a NaN (its payload is the arithmetic unit's, not the rule's)."""
    assert got.shape == want.shape and got.dtype == want.dtype, tag
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), tag
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan]), (tag, int(np.count_nonzero(_bits(got)[~nan] != _bits(want)[~nan])))


# ----------------------------------------------------------------------------------------------------------------------- the frame entry
FRAME_CASES = [(0, 8, 1), (1, 8, 1), (1, 5, 3), (7, 8, 1), (7, 8, 2), (7, 8, 3), (7, 5, 1), (70, 8, 1), (70, 5, 2)]


@pytest.mark.parametrize("T,E,label_kind", FRAME_CASES)
def test_frame_gated_matrices_equal_the_rule(T, E, label_kind):
    case = make_case(T, E, 100 + T + E)
    base = run_frame(case, None, label_kind)
    # every gate off: the bytes of cnl_track_frame_low_f32, guard bytes of the unwritten tail included
    for off in ("off", "null", (False, None, 1.0)):
        assert np.array_equal(run_frame(case, off, label_kind), base), off
    n, det_index, _, score, labels, reid, box, low_index, low_box = th.read_frame_low_record(base)
    assert n == 7 and len(low_index) == 3 and np.array_equal(labels, case["labels"])
    hdr = base[:48].view(np.int32).tolist()
    seen = set()
    for name, gate in GATES.items():
        h = run_frame(case, gate, label_kind)
        got = th.read_frame_low_record(h)
        want = _expected(case, reid, box, low_box, det_index, low_index, gate)
        for which, a, b in zip(("reid", "box", "low_box"), (got[5], got[6], got[8]), want):
            _same_matrix(a, b, (name, which))
        # everything outside the three matrices: the `_low` record's bytes
        other = np.ones(len(h), bool)
        for off, size in ((hdr[th.F_OFF_REID], 8 * n * T), (hdr[th.F_OFF_BOX], 4 * n * T), (hdr[th.F_OFF_LOW_BOX], 4 * len(low_index) * T)):
            other[off:off + size] = False
        assert np.array_equal(h[other], base[other]), name
        if T:
            g = got[5] == 1e5
            seen.add("gated" if g.any() else "none gated")
            seen.add("kept" if (~g).any() else "none kept")
            if gate[2] != 1.0:
                inside = ~g
                assert inside.any() and not np.array_equal(_bits(got[5][inside]), _bits(reid[inside]))      # the weight moved the costs inside the gate
            elif gate[1] is not None:
                assert np.array_equal(_bits(got[5][~g]), _bits(reid[~g]))                                  # weight 1: untouched bits
    if T >= 7:
        assert seen == {"gated", "kept"}


def test_every_pair_cross_class_is_an_all_gated_matrix_and_every_detection_a_birth():
    case = make_case(7, 8, 5, cross_all=True)
    got = th.read_frame_low_record(run_frame(case, GATES["class"]))
    n, reid, box, low_box = got[0], got[5], got[6], got[8]
    assert (reid == 1e5).all() and (box == np.float32(1e5)).all() and (low_box == np.float32(1e5)).all() and reid.shape == (7, 7)
    matches, unmatched_dets, unmatched_tracks = th.two_stage_assignment(reid, 0.2, 0.5, box)          # scipy solves it: finite, feasible
    assert matches == [] and unmatched_dets == list(range(n)) and unmatched_tracks == list(range(7))
    assert th.low_stage(low_box, got[7], unmatched_tracks, None, 0.5) == ([], unmatched_tracks)
    # the Tracker: 7 births per frame, no match, and the same tracks again unmatched
    trk = _quiet(cl.Tracker, model=None, device=DEV, class_aware=True, min_birth_age=1)
    args = (case["det_box"], case["labels"], case["score"], case["det_emb"])
    trk.update(*args)
    for t in trk.tracks:
        t.label = 1
    trk.update(*args)
    assert trk.last_matches == [] and (trk.last_costs[0] == 1e5).all() and len(trk.tracks) == 7 and trk.next_track_id == 14


def test_zero_area_track_and_nan_coordinate_gate_their_own_pairs_only():
    clean = make_case(7, 8, 9)
    flat = make_case(7, 8, 9, flat_track=True)
    nan = make_case(7, 8, 9, nan_det=True)
    gate = GATES["motion"]
    r_clean, r_flat, r_nan = (th.read_frame_low_record(run_frame(c, gate)) for c in (clean, flat, nan))
    # the pivot rule: the zero-area track (P = 0) is gated for every detection; the other columns keep their bits
    assert not (flat["kP"][0] != 0).any() and (r_flat[5][:, 0] == 1e5).all()
    assert np.array_equal(_bits(r_flat[5][:, 1:]), _bits(r_clean[5][:, 1:])) and (r_clean[5][:, 1:] != 1e5).any()
    # a NaN coordinate: its row is gated (NaN <= gate is false), the neighbouring rows keep their bits; its box costs are NaN as before
    row = 0
    assert np.isnan(nan["det_box"][r_nan[1][row]]).any() and (r_nan[5][row] == 1e5).all()
    assert np.array_equal(_bits(r_nan[5][1:]), _bits(r_clean[5][1:])) and np.array_equal(_bits(r_nan[6][1:]), _bits(r_clean[6][1:]))
    assert np.isnan(r_nan[6][row]).all()
    for c, r in ((flat, r_flat), (nan, r_nan)):
        base = th.read_frame_low_record(run_frame(c, None))
        want = _expected(c, base[5], base[6], base[8], base[1], base[7], gate)
        _same_matrix(r[5], want[0], "reid")
        _same_matrix(r[6], want[1], "box")


def test_gated_frame_without_a_low_stage_or_a_box_cost():
    """low_threshold == detection_threshold is "no low-score stage": n_low = 0, and then the entry takes box_cost 0 (class_aware with box_cost=None)."""
    case = make_case(7, 8, 3)
    h = run_frame(case, GATES["class"], mode=0, low_thr=DET_THR)
    base = run_frame(case, None, mode=1, low_thr=DET_THR)
    a, b = th.read_frame_low_record(h), th.read_frame_low_record(base)
    assert len(a[7]) == 0 and a[0] == b[0] == 7
    _same_matrix(a[5], _expected(case, b[5], None, None, b[1], None, GATES["class"])[0], "reid")
    hdr = h[:48].view(np.int32).tolist()
    box_bytes = h[hdr[th.F_OFF_BOX]:hdr[th.F_OFF_BOX] + 4 * 7 * 7]
    assert (box_bytes == SENTINEL_BYTE).all()                       # no box matrix was written


# ----------------------------------------------------------------------------------------------------------------------- the streams entry
class _Streams:
    """S = 4, live order [3, 0, 2]: stream 0 has no tracks, stream 1 takes no part (and owns rows), stream 2 has tracks but no kept detection
    (its three low-score detections remain), stream 3 has 70 tracks (more than one wave in the assign kernel)."""

    def __init__(self, E, label_kind, T_of=(0, 5, 7, 70), live=(3, 0, 2), planted=None):
        """planted (the second layout: every stream live, one of them with T = 1): per stream the keyword of make_case that plants its case."""
        self.E, self.label_kind = E, label_kind
        self.S, self.live, self.T_of = 4, list(live), list(T_of)
        self.cases = {s: make_case(self.T_of[s], E, 300 + s + E, **({(planted or {}).get(s): True} if (planted or {}).get(s) else {})) for s in range(4)}
        self.no_kept = None if planted else 2
        if planted is None:
            self.cases[2]["score"] = np.where(self.cases[2]["score"] >= DET_THR, np.float32(0.01), self.cases[2]["score"]).astype(np.float32)
        self.off = np.concatenate([[0], np.cumsum(self.T_of)]).astype(np.int32)
        self.R, self.T_max = int(self.off[-1]), max(self.T_of)
        pool = lambda n: np.concatenate([self.cases[s][n] for s in range(4)])
        self.tables = {n: pool(n) for n in ("trk_emb", "trk_box", "trk_label", "kx", "kP")}
        slot = lambda n: np.stack([self.cases[s][n] for s in self.live])
        self.ops = [_dev(slot("det_emb")), _dev(slot("det_box")), _dev(slot("score")), _dev(slot("labels").astype(LABEL_DTYPES[label_kind]))]
        self.tab = [_dev(self.tables["trk_emb"]), _dev(self.tables["trk_box"])]
        self.live_d, self.off_d = _dev(np.array(self.live, np.int32)), _dev(self.off)

    def run(self, gate, low_thr=LOW_THR):
        """-> (records uint8 [S * stride], stride, workspace bytes); guards checked."""
        lib = _lib.load()
        S, T_max, E = self.S, self.T_max, self.E
        ws_bytes, rec_bytes = int(lib.cnl_track_streams_low_workspace_bytes(S, K, T_max)), int(lib.cnl_track_streams_low_record_bytes(K, T_max, 1))
        assert ws_bytes >= th.streams_low_workspace_bytes(S, K, self.R)
        stride = rec_bytes + 40
        ws = GuardedBytes(ws_bytes, align=8, device=DEV, name="streams workspace")
        rec = GuardedBytes(S * stride, align=8, device=DEV, name="stream records")
        args = (*(t.data_ptr() for t in self.ops), self.label_kind, S, len(self.live), self.live_d.data_ptr(), K, E, DET_THR, 0.2, 0.5, low_thr, 0.5,
                self.tab[0].data_ptr(), self.tab[1].data_ptr(), self.off_d.data_ptr(), None, self.R, T_max, 1, 0, 1, ws.ptr, ws_bytes, rec.ptr, stride)
        keep = []
        if gate is None:
            rc = lib.cnl_track_streams_low_f32(*args, _stream())
        elif gate == "null":
            rc = lib.cnl_track_streams_gated_f32(*args, None, _stream())
        else:
            pooled = dict(self.tables, T=self.R)
            g = _lib.TrackGate(None, None, None, 0.0, 1.0) if gate == "off" else _gate_struct(pooled, *gate, keep)
            rc = lib.cnl_track_streams_gated_f32(*args, ctypes.byref(g), _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        _ok(ws)
        _ok(rec)
        return rec.body.cpu().numpy().copy(), stride, ws.body.cpu().numpy().copy()

    def matrices(self, ws, s, n, n_low):
        """Stream s's (reid, box, low_box) out of a workspace."""
        P, t0, T = K * self.R, int(self.off[s]), self.T_of[s]
        reid = ws[8 * K * t0:8 * K * t0 + 8 * n * T].view(np.float64).reshape(n, T)
        box = ws[16 * P + 4 * K * t0:16 * P + 4 * K * t0 + 4 * n * T].view(np.float32).reshape(n, T)
        low0 = th.streams_workspace_bytes(self.S, K, self.R) + 4 * K * t0
        return reid, box, ws[low0:low0 + 4 * n_low * T].view(np.float32).reshape(n_low, T)


def _check_streams(st):
    """Every gate combination on the layout `st`: all gates off = the `_low` entry's bytes; the three matrices of every live stream against the rule
    applied to the `_low` entry's; the lists against scipy on the gated matrices — or, where scipy refuses those (a NaN that survives the gates),
    a non-zero status and no list.  -> what was seen."""
    base, stride, ws0 = st.run(None)
    for off in ("off", "null"):
        h, _, ws = st.run(off)
        assert np.array_equal(h, base) and np.array_equal(ws, ws0), off           # every gate off: records (and workspace) byte for byte
    absent = [s for s in range(st.S) if s not in st.live]
    for s in absent:
        assert (base[s * stride:(s + 1) * stride] == SENTINEL_BYTE).all()         # a stream that took no part
    seen = set()
    for name, gate in GATES.items():
        h, _, ws = st.run(gate)
        for s in absent:
            assert (h[s * stride:(s + 1) * stride] == SENTINEL_BYTE).all()
        for s in st.live:
            case = st.cases[s]
            rec0, rec = base[s * stride:(s + 1) * stride], h[s * stride:(s + 1) * stride]
            n, T, status0, det_index, _, _, labels, *_ = th.read_stream_low_record(rec0)
            out = th.read_stream_low_record(rec)
            assert out[:2] == (n, T) and np.array_equal(out[3], det_index) and np.array_equal(out[6], case["labels"]), (name, s)
            low_index = np.flatnonzero((case["score"] >= np.float32(LOW_THR)) & (case["score"] < np.float32(DET_THR)))
            assert out[10] == len(low_index) == 3 and n == (0 if s == st.no_kept else 7) and T == st.T_of[s]
            if T == 0:
                assert out[2] == 0 and out[7] == [] and out[8] == list(range(n)) and out[9] == [] and out[11] == []
                continue
            reid, box, low_box = st.matrices(ws0, s, n, 3)
            want = _expected(case, reid, box, low_box, det_index, low_index, gate)
            for which, a, b in zip(("reid", "box", "low_box"), st.matrices(ws, s, n, 3), want):
                _same_matrix(a, b, (name, s, which))
            # the lists: the unchanged assign kernel on the gated matrices = scipy on them
            try:
                matches, unmatched_dets, unmatched_tracks = th.two_stage_assignment(want[0], 0.2, 0.5, want[1])
                low_matches, unmatched_tracks = th.low_stage(want[2], low_index, unmatched_tracks, None, 0.5)
            except ValueError:
                assert out[2] != 0 and out[7] == [] and out[11] == [], (name, s)
                seen.add("refused")
                continue
            assert out[2] == 0 and (out[7], out[8], out[9], out[11]) == (matches, unmatched_dets, unmatched_tracks, low_matches), (name, s)
            seen.add("T=%d" % T)
            if want[0].size and all((m == 1e5).all() for m in want):      # every pair cross-class
                seen.add("all gated")
                assert matches == [] and low_matches == []
            if gate[0]:
                pairs = [(det_index[r], t) for r, t in matches] + low_matches
                assert all(case["labels"][d] == case["trk_label"][t] for d, t in pairs), (name, s)
                seen.add("class pairs" if pairs else "no class pairs")
    return seen


@pytest.mark.parametrize("E,label_kind", [(8, 1), (5, 2), (8, 3)])
def test_streams_gated_equal_the_rule(E, label_kind):
    seen = _check_streams(_Streams(E, label_kind))
    assert seen >= {"T=7", "T=70", "class pairs"} and "refused" not in seen, seen


def test_streams_gated_planted_cases():
    """The streams entry on the cases the frame entry is shown, each in a stream of its own whose rows start inside the pooled tables: T = 1; every
    pair cross-class (an all-1e5 matrix: no match, every detection unmatched); a zero-area track (pivot rule: its column is gated, the others keep
    the bits the rule gives); a NaN coordinate (its re-ID row is gated; where its NaN box cost reaches stage 2 the stream is refused, as by scipy)."""
    st = _Streams(8, 1, T_of=(1, 7, 7, 7), live=(3, 1, 0, 2), planted={1: "cross_all", 2: "flat_track", 3: "nan_det"})
    seen = _check_streams(st)
    assert seen >= {"T=1", "T=7", "all gated", "refused"}, seen
    # the planted properties themselves: the motion gate for the pivot rule and the NaN, the class gate for the all-gated stream
    _, _, ws = st.run(GATES["motion"])
    reid_flat, reid_nan = (st.matrices(ws, s, 7, 3)[0] for s in (2, 3))
    assert (reid_flat[:, 0] == 1e5).all() and (reid_flat[:, 1:] != 1e5).any() and (reid_nan[0] == 1e5).all() and (reid_nan[1:] != 1e5).any()
    h, stride, ws = st.run(GATES["class"])
    assert all((m == 1e5).all() for m in st.matrices(ws, 1, 7, 3))
    out = th.read_stream_low_record(h[stride:2 * stride])
    assert out[2] == 0 and out[7] == [] and out[8] == list(range(7)) and out[9] == list(range(7))       # every detection a birth, every track unmatched


# ----------------------------------------------------------------------------------------------------------------------- sequences
def _snapshot(tracks):
    return ([t.track_id for t in tracks], [(t.state.name, t.birth_age, t.inactive_age) for t in tracks], [int(t.label) for t in tracks],
            [_bits(np.asarray(t.bbox, np.float64)).tolist() for t in tracks])


def _frame_inputs(fr, how):
    """A frame of the scene as host arrays ("host") or device tensors with labels of the kernel's three element types."""
    if how == "host":
        return fr
    box, lab, score, emb = fr
    return _dev(box), _dev(lab.astype(LABEL_DTYPES[how])), _dev(score), _dev(emb)


OPTIONS = [dict(class_aware=True), dict(class_aware=True, use_kalman=True), dict(class_aware=True, **KAL), dict(motion_gate=True, **KAL),
           dict(class_aware=True, motion_gate=True, **KAL), dict(class_aware=True, motion_gate=True, motion_weight=0.98, **KAL)]


@pytest.fixture(scope="module")
def scene():
    return gate_ref.crossing_scene()


@pytest.fixture(scope="module")
def reference(scene):
    """The reference loop's per-frame snapshots, computed once per option set."""
    cache = {}

    def get(opts, low, frames=None, tag=None):
        key = (tuple(sorted(opts.items())), low, tag)
        if key not in cache:
            ref = gate_ref.Tracker(low_threshold=low, **opts)
            out = []
            for f in (range(len(scene[0])) if frames is None else frames):
                fr = scene[0][f] if isinstance(f, int) else f
                ref.update(*fr)
                out.append((_snapshot(ref.tracks), list(ref.last_matches), ref.last_low_matches, ref.last_costs))
            cache[key] = out
        return cache[key]
    return get


@pytest.mark.parametrize("low", [None, LOW_THR], ids=["nolow", "low"])
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join(k for k in o if k != "kalman"))
def test_tracker_equals_the_reference_loop(scene, reference, opts, low):
    want = reference(opts, low)
    for how in ("host", 1, 3):
        trk = _quiet(cl.Tracker, model=None, device=DEV, low_threshold=low, **opts)
        for f, fr in enumerate(scene[0]):
            trk.update(*_frame_inputs(fr, how))
            snap, matches, low_matches, costs = want[f]
            assert _snapshot(trk.tracks) == snap, (how, f)
            assert trk.last_matches == matches and trk.last_low_matches == low_matches, (how, f)
            if costs is not None:                                  # last_costs shows the gated matrices
                _same_matrix(trk.last_costs[0], costs[0], (how, f))
                _same_matrix(trk.last_costs[1], costs[1], (how, f))
            hdr = trk._rec.np[:48].view(np.int32)
            assert hdr[th.F_OFF_INDEX] == 48 and (low is not None or hdr[th.F_NLOW] == 0)           # the `_low` layout, with or without the stage


def _bank_frames(scene, S):
    """Per step, {stream: frame}: stream 0 sees the scene; stream 1 (S = 3) joins at step 2 (it has no tracks while the others do) and is absent
    from every fourth step, so it sees the scene late; stream 2 sees it with every detection below the threshold in frames 12 and 13 (no kept
    detection)."""
    seq = scene[0]
    steps = []
    nxt = [0] * S
    for step in range(len(seq)):
        cur = {}
        for s in range(S):
            if s == 1 and (step < 2 or step % 4 == 3):
                continue
            fr = seq[nxt[s]]
            if s == 2 and nxt[s] in (12, 13):
                fr = (fr[0], fr[1], np.full_like(fr[2], 0.01), fr[3])
            cur[s] = fr
            nxt[s] += 1
        steps.append(cur)
    return steps


@pytest.mark.parametrize("S", [3, 1])
@pytest.mark.parametrize("low", [None, LOW_THR], ids=["nolow", "low"])
@pytest.mark.parametrize("opts", OPTIONS, ids=lambda o: "-".join(k for k in o if k != "kalman"))
def test_bank_equals_the_reference_loop_and_independent_trackers(scene, reference, opts, low, S):
    steps = _bank_frames(scene, S)
    per_stream = [[cur[s] for cur in steps if s in cur] for s in range(S)]
    want = [reference(opts, low, None if s == 0 else per_stream[s], None if s == 0 else ("bank", s)) for s in range(S)]
    how = "host" if S == 1 else 2
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, low_threshold=low, **opts)
    singles = [_quiet(cl.Tracker, model=None, device=DEV, low_threshold=low, **opts) for _ in range(S)]
    seen = [0] * S
    for step, cur in enumerate(steps):
        live = sorted(cur, reverse=True)                                  # a live order that is not the stream order
        frames = [cur[s] for s in live]
        batch = tuple(np.stack([fr[i] for fr in frames]) for i in range(4))
        bank.update_batch(*_frame_inputs(batch, how), streams=live)
        for s in live:
            singles[s].update(*_frame_inputs(cur[s], how))
            snap, matches, low_matches, _ = want[s][seen[s]]
            seen[s] += 1
            assert _snapshot(bank[s].tracks) == snap == _snapshot(singles[s].tracks), (step, s)
            assert bank.last_matches[s] == matches == singles[s].last_matches, (step, s)
            assert bank.last_low_matches[s] == low_matches == singles[s].last_low_matches, (step, s)
            lo, hi = int(bank._off[s]), int(bank._off[s + 1])
            for name in ("emb", "box") + (("kx", "kP") if opts.get("kalman") == "device" else ()):
                a, b = getattr(bank._table, name)[lo:hi].cpu().numpy(), getattr(singles[s]._table, name)[:hi - lo].cpu().numpy()
                assert np.array_equal(_bits(a), _bits(b)), (step, s, name)
        hdr = bank._rec.np[:96].view(np.int32)
        assert hdr[th.S_OFF_INDEX] == 96                                  # the `_low` layout
    assert seen == [len(p) for p in per_stream]


# ----------------------------------------------------------------------------------------------------------------------- defaults
def test_defaults_call_the_old_entry_points(scene, monkeypatch):
    """Default-constructed trackers: the plain entries' record headers and d2h_bytes, the oracle's tracks — and the gated entries are never
    called.  With low_threshold alone: the `_low` entries, as before."""
    lib = _lib.load()

    def refuse(*a, **k):
        raise AssertionError("a tracker without class_aware / motion_gate must not call a gated entry")
    monkeypatch.setattr(lib, "cnl_track_frame_gated_f32", refuse)
    monkeypatch.setattr(lib, "cnl_track_streams_gated_f32", refuse)
    seq = scene[0]
    for low, off_frame, off_stream in ((None, 32, 64), (LOW_THR, 48, 96)):
        trk = _quiet(cl.Tracker, model=None, device=DEV, low_threshold=low)
        bank = _quiet(cl.TrackerBank, num_streams=2, device=DEV, low_threshold=low)
        oracle = tracker_ref.Tracker() if low is None else None
        for f, fr in enumerate(seq):
            T = len(trk.tracks)
            trk.update(*fr)
            bank.update_batch(*(np.stack([a, a]) for a in fr))
            hdr = trk._rec.np[:48].view(np.int32)
            n = int(hdr[th.F_N])
            assert hdr[th.F_OFF_INDEX] == off_frame and hdr[th.F_T] == T
            want = 32 + 4 * n + 12 * n * T + (0 if low is None else 16 + 4 * int(hdr[th.F_NLOW]) * (1 + T))      # host arrays: no detections section
            assert trk.d2h_bytes == want, f
            assert bank._rec.np[:96].view(np.int32)[th.S_OFF_INDEX] == off_stream
            for s in range(2):
                assert _snapshot(bank[s].tracks) == _snapshot(trk.tracks), (f, s)
            if oracle is not None:
                oracle.update(*fr)
                assert [t.track_id for t in trk.tracks] == [t.track_id for t in oracle.tracks]
                assert [t.state.name for t in trk.tracks] == [t.state.name for t in oracle.tracks]
                assert np.array_equal(np.array([t.bbox for t in trk.tracks]), np.array([t.bbox for t in oracle.tracks]))
    with pytest.raises(AssertionError, match="gated entry"):
        _quiet(cl.Tracker, model=None, device=DEV, class_aware=True).update(*seq[0])


def test_bank_redoes_a_stream_with_non_finite_costs_through_the_gated_host_path(scene):
    """A zero embedding under "cosine" leaves NaN costs in its row (same-class pairs: the class gate does not touch them): the bank's assign kernel
    reports it, the stream goes through the host path — the ungated frame entry, then _track_host.gate_costs — and the caller sees what a gated
    Tracker raises (scipy's ValueError), every stream as it was.  The same zero embedding on a detection of a class without tracks is gated away."""
    seq = scene[0]
    for opts in (dict(class_aware=True), dict(class_aware=True, motion_gate=True, **KAL)):
        bank = _quiet(cl.TrackerBank, num_streams=2, device=DEV, **opts)
        one = _quiet(cl.Tracker, model=None, device=DEV, **opts)
        for fr in seq[:3]:
            bank.update_batch(*(np.stack([a, a]) for a in fr))
            one.update(*fr)
        bad = tuple(a.copy() for a in seq[3])
        bad[3][0] = 0.0                                                # object A's embedding (class 0; tracks of class 0 exist)
        before = [_snapshot(bank[s].tracks) for s in range(2)]
        with pytest.raises(ValueError, match="invalid numeric"):
            one.update(*bad)
        with pytest.raises(ValueError, match="invalid numeric"):
            bank.update_batch(*(np.stack([a, b]) for a, b in zip(seq[3], bad)))
        assert [_snapshot(bank[s].tracks) for s in range(2)] == before
        gone = tuple(a.copy() for a in seq[3])
        gone[3][0], gone[1][0] = 0.0, 7                                # ... of a class no track has: every pair of the row is gated, nothing is NaN
        bank.update_batch(*(np.stack([a, b]) for a, b in zip(seq[3], gone)))
        assert len(bank[1].tracks) == len(bank[0].tracks) + 1 and bank[1].tracks[-1].label == 7
