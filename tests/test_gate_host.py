"""CPU: the class / motion gates' host side — the two gated C-ABI entry points (declared, exported, bound, argument validation without a device),
the options' validation, the rule's restatement (tests/gate_ref.py) against a textbook evaluation and against the package's vectorised host
function, the per-class equivalence of assigning a gated matrix, and the crossing scene on the reference loop."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest

import gate_ref
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd import _track_host as th

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cnl_track_frame_gated_f32", "cnl_track_streams_gated_f32")
KAL = dict(use_kalman=True, kalman="device")
# Largest relative difference, over every (detection, track) pair of test_mahalanobis_against_the_textbook_inverse's seeded states, between the
# restatement's m and y @ np.linalg.inv(S) @ y, as measured when the test was written; the test asserts 100 times this: the
# cases are seeded, the margin is for other BLAS builds.
MEASURED_M_REL = 3.9e-16


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def test_new_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.cnl_version() == _lib.ABI_VERSION == 13           # new entry points only: the ABI version stays
    assert re.search(r"#define\s+CNL_TRACK_GATE_COST\s+1e5\b", header) and th.GATE_COST == gate_ref.GATE_COST == 1e5
    assert float(np.float32(1e5)) == 1e5                          # exact in float32 and float64
    assert ctypes.sizeof(_lib.TrackGate) == 40
    assert th.CHI2INV95_4 == gate_ref.CHI2INV95_4 == 9.4877


def test_argument_errors_without_touching_a_device():
    lib = _lib.load()
    p = 0x1000                       # never dereferenced: every call below is refused on its arguments

    def gate(**kw):
        g = dict(trk_label=p, kx=p, kP=p, motion_gate=9.4877, motion_weight=1.0)
        g.update(kw)
        return _lib.TrackGate(*g.values())

    def frame(g, **kw):
        a = dict(det_emb=p, det_box=p, det_score=p, det_label=p, label_kind=1, k=12, E=8, thr=0.3, low=0.1, trk_emb=p, trk_box=p, T=7, box_cost=1,
                 reid_metric=0, with_dets=1, rec=p, rec_bytes=lib.cnl_track_frame_low_bytes(12, 7, 1) - 1, gate=ctypes.byref(g) if g else None,
                 stream=None)
        a.update(kw)
        return lib.cnl_track_frame_gated_f32(*a.values())

    def streams(g, **kw):
        a = dict(det_emb=p, det_box=p, det_score=p, det_label=p, label_kind=1, S=3, S_live=3, live=p, k=12, E=8, thr=0.3, reid_thr=0.2, box_thr=0.5,
                 low=0.1, low_box=0.5, trk_emb=p, trk_box=p, trk_off=p, elig=None, R=21, T_max=7, box_cost=1, reid_metric=0, with_dets=1, ws=p,
                 ws_bytes=th.streams_low_workspace_bytes(3, 12, 21) - 1, rec=p, stride=1 << 16, gate=ctypes.byref(g) if g else None, stream=None)
        a.update(kw)
        return lib.cnl_track_streams_gated_f32(*a.values())

    # (every call that passes the gate's checks is stopped by the record / workspace size, one byte short: no launch)
    for call in (frame, streams):
        assert call(gate()) == _lib.CNL_E_BAD_ARG and ("record holds" in _lib.last_error() or "workspace" in _lib.last_error())
        assert call(None) == _lib.CNL_E_BAD_ARG and ("record holds" in _lib.last_error() or "workspace" in _lib.last_error())
        assert call(gate(kP=None)) == _lib.CNL_E_BAD_ARG and "kx and kP" in _lib.last_error()
        assert call(gate(kx=None)) == _lib.CNL_E_BAD_ARG and "kx and kP" in _lib.last_error()
        assert call(gate(kx=p + 4)) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error()
        assert call(gate(trk_label=p + 2)) == _lib.CNL_E_BAD_ARG and "aligned" in _lib.last_error()
        for bad in (1e5, 2e5, -1.0, float("nan"), float("inf")):
            assert call(gate(motion_gate=bad)) == _lib.CNL_E_BAD_ARG and "motion_gate" in _lib.last_error(), bad
        for bad in (-0.1, 1.5, float("nan")):
            assert call(gate(motion_weight=bad)) == _lib.CNL_E_BAD_ARG and "motion_weight" in _lib.last_error(), bad
        assert call(gate(), det_box=p + 8, trk_box=None, box_cost=0, low=0.3) == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error()
        # the checks of the _low entries are kept
        assert call(gate(), low=0.31) == _lib.CNL_E_BAD_ARG and "low_threshold" in _lib.last_error()
        assert call(gate(), box_cost=0) == _lib.CNL_E_BAD_ARG and "box_cost" in _lib.last_error()
        assert call(gate(), det_emb=None) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error()
        # ... except that without a low-score stage (an empty score window) there may be no box cost
        assert call(gate(), box_cost=0, low=0.3) == _lib.CNL_E_BAD_ARG and ("record holds" in _lib.last_error() or "workspace" in _lib.last_error())
    # a threshold that would accept gated pairs
    for name in ("reid_thr", "box_thr", "low_box"):
        assert streams(gate(), **{name: 1e5}) == _lib.CNL_E_BAD_ARG and "threshold" in _lib.last_error(), name
        assert streams(gate(kx=None, kP=None), **{name: 1e6}) == _lib.CNL_E_BAD_ARG and "threshold" in _lib.last_error(), name
        assert streams(gate(trk_label=None, kx=None, kP=None), **{name: 1e6}) == _lib.CNL_E_BAD_ARG and "workspace" in _lib.last_error()    # gates off


def test_option_checks():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for make in (cl.Tracker, lambda **kw: cl.TrackerBank(num_streams=2, **kw)):
            t = make()
            assert (t.class_aware, t.motion_gate, t.motion_weight, t._gated) == (False, None, 1.0, False)
            t = make(class_aware=True)
            assert t.class_aware is True and t._gated
            t = make(motion_gate=True, **KAL)
            assert t.motion_gate == 9.4877 and t._gated
            t = make(motion_gate=5, motion_weight=0.98, class_aware=1, **KAL)
            assert (t.class_aware, t.motion_gate, t.motion_weight) == (True, 5.0, 0.98)
            assert make(motion_gate=False).motion_gate is None
            for old_positional_kalman in ("host", "device"):         # the slot `kalman` had before the gate keywords: refused by name, never truthy
                with pytest.raises(ValueError, match="class_aware"):
                    make(class_aware=old_positional_kalman)
            for kw in (dict(), dict(use_kalman=True), dict(use_kalman=True, kalman="host"), dict(kalman="device")):
                with pytest.raises(ValueError, match="motion_gate"):
                    make(motion_gate=True, **kw)
            for bad in (1e5, 3e5, -1.0, float("nan")):
                with pytest.raises(ValueError, match="motion_gate"):
                    make(motion_gate=bad, **KAL)
            for bad in (-0.1, 1.01, float("nan")):
                with pytest.raises(ValueError, match="motion_weight"):
                    make(motion_gate=True, motion_weight=bad, **KAL)
            with pytest.raises(ValueError, match="motion_weight"):
                make(motion_weight=0.98)
            # a threshold at or above the gated pairs' cost, at construction and per call
            for name in ("reid_threshold", "box_threshold", "low_box_threshold"):
                with pytest.raises(ValueError, match="every threshold must be below"):
                    make(class_aware=True, **{name: 1e5})
                with pytest.raises(ValueError, match="every threshold must be below"):
                    make(motion_gate=True, **KAL, **{name: 2e5})
                assert getattr(make(**{name: 1e5}), name) == 1e5         # without a gate the thresholds are the caller's business, as before
                with pytest.raises(ValueError, match="every threshold must be below"):
                    make(class_aware=True)._thresholds({name: 1e5})
            # class_aware alone needs neither a box cost nor a filter, and goes with every Kalman mode and with the low-score stage
            for kw in (dict(box_cost=None), dict(use_kalman=True), KAL, dict(low_threshold=0.1), dict(low_threshold=0.1, **KAL)):
                assert make(class_aware=True, **kw)._gated
        # host-side costs are not gated: both options raise by name
        for kw in (dict(reid_cost="minkowski"), dict(reid_cost=lambda a, b: a @ b.T), dict(box_cost=lambda a, b: a @ b.T)):
            with pytest.raises(ValueError, match="class_aware"):
                cl.Tracker(class_aware=True, allow_host_cost=True, **kw)
            with pytest.raises(ValueError, match="motion_gate"):
                cl.Tracker(motion_gate=True, allow_host_cost=True, **KAL, **kw)
        cfg = dict(cl.load_config(os.path.join(ROOT, "centernet-lightning_amd", "configs", "tracking_resnet34_fpn.yaml"))["tracker"])
        assert (cfg["class_aware"], cfg["motion_gate"], cfg["motion_weight"]) == (False, None, 1.0)
        t = cl.build_tracker(cfg)
        assert type(t) is cl.Tracker and not t._gated
        cfg.update(class_aware=True, motion_gate=True, motion_weight=0.98, **KAL)
        t, b = cl.build_tracker(cfg), cl.build_tracker(cfg, num_streams=3)
        assert type(t) is cl.Tracker and type(b) is cl.TrackerBank
        for x in (t, b):
            assert (x.class_aware, x.motion_gate, x.motion_weight) == (True, 9.4877, 0.98)


# ----------------------------------------------------------------------------------------------------------------------- the restatement
def _filter_states():
    """The filter states tests/kalman_ref.py produces over the 30-frame crossing scene (the reference loop with the device filter), per frame
    (kx [T, 8], kP [T, 64]) as the NEXT frame's gate reads them, with that frame's boxes [k, 4]."""
    seq, _ = gate_ref.crossing_scene()
    trk = gate_ref.Tracker(**KAL)
    out = []
    for f, fr in enumerate(seq):
        if f and len(trk.tracks):
            out.append((trk.kx.copy(), trk.kP.copy(), fr[0]))
        trk.update(*fr)
    return out


def test_mahalanobis_against_the_textbook_inverse():
    worst, pairs = 0.0, 0
    for kx, kP, boxes in _filter_states():
        m_vec, ok_vec = th.mahalanobis_sq(boxes, kx, kP)
        for t in range(len(kx)):
            x, P = kx[t], kP[t].reshape(8, 8)
            wh = np.array([x[2] - x[0], x[3] - x[1]] * 2)
            S = P[:4, :4] + np.diag((wh / 20.0) ** 2)
            Sinv = np.linalg.inv(S)
            for d in range(len(boxes)):
                m, ok = gate_ref.mahalanobis(boxes[d], kx[t], kP[t])
                y = boxes[d].astype(np.float64) - x[:4]
                want = float(y @ Sinv @ y)
                assert ok and ok_vec[t] and m >= 0
                if want == 0.0:                                         # a detection exactly on the predicted state (the standing object)
                    assert m == 0.0
                else:
                    worst = max(worst, abs(m - want) / want)
                pairs += 1
                assert _bits(np.float64(m)) == _bits(m_vec[d, t])        # the package's vectorised host function: the same bits
    print(f"largest relative difference of m over {pairs} pairs: {worst:.3e}")
    assert pairs > 1000
    assert worst <= 100 * MEASURED_M_REL, worst


def test_host_function_equals_the_restatement():
    """_track_host.gate_costs (what a redone TrackerBank stream goes through) against gate_ref.gate_costs, bit for bit: every gate combination,
    the weight, float labels, a zero P (pivot rule), a NaN coordinate, index lists."""
    rng = np.random.default_rng(3)
    states = _filter_states()
    kx, kP, _ = states[-1]
    T = len(kx)
    kP = kP.copy()
    kP[1] = 0.0
    kx = kx.copy()
    kx[1, 2:4] = kx[1, 0:2]                                           # a zero-area track whose P is zero: no positive pivot
    k, n, n_low = 12, 7, 3
    boxes = np.concatenate([kx[rng.integers(0, T, k), :4] + rng.standard_normal((k, 4)) * 0.01]).astype(np.float32)
    boxes[4, 1] = np.nan
    perm = rng.permutation(k)
    det_index, low_index = np.sort(perm[:n]), np.sort(perm[n:n + n_low])
    reid, box, low_box = rng.random((n, T)), rng.random((n, T)).astype(np.float32), rng.random((n_low, T)).astype(np.float32)
    trk_labels = [t % 3 for t in range(T)]
    for labels in (rng.integers(0, 3, k), rng.integers(0, 3, k).astype(np.float32) + 0.5):
        for cls, gate, w in [(True, None, 1.0), (False, 9.4877, 1.0), (True, 9.4877, 1.0), (True, 9.4877, 0.98), (False, 50.0, 0.5), (False, None, 1.0)]:
            args = (reid, box, low_box, labels, trk_labels if cls else None, boxes, kx, kP, gate, w, det_index, low_index)
            want, got = gate_ref.gate_costs(*args), th.gate_costs(*args)
            for a, b in zip(want, got):
                assert a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b)), (cls, gate, w)
            if gate is not None:
                assert (got[0][:, 1] == 1e5).all()                   # the pivot rule
                assert (got[0][list(det_index).index(4)] == 1e5).all() if 4 in det_index else True      # the NaN coordinate gates its row
            if not cls and gate is None:
                assert np.array_equal(_bits(got[0]), _bits(reid)) and np.array_equal(_bits(got[1]), _bits(box))
    assert th.gate_costs(reid, None, None, None, None, boxes, None, None, None, 1.0)[1:] == (None, None)


# ----------------------------------------------------------------------------------------------------------------------- assignment
def test_gated_assignment_equals_per_class_assignment():
    """Solving the gated matrix and thresholding gives exactly the matches of solving each class on its own: 300 seeded problems of up to 12 x 12,
    1 to 3 classes, a fifth of the same-class pairs motion-gated."""
    rng = np.random.default_rng(17)
    for case in range(300):
        n, T, C = int(rng.integers(1, 13)), int(rng.integers(1, 13)), int(rng.integers(1, 4))
        cost = rng.random((n, T))
        dl, tl = rng.integers(0, C, n), rng.integers(0, C, T)
        motion = rng.random((n, T)) < 0.2
        gated = cost.copy()
        gated[motion | (dl[:, None] != tl[None, :])] = 1e5
        thr = float(rng.choice([0.3, 0.6, 1.5]))
        got, _, _ = th.match_with_threshold(gated, thr)
        want = []
        for c in range(C):
            rows, cols = np.flatnonzero(dl == c), np.flatnonzero(tl == c)
            if len(rows) and len(cols):
                sub = cost[np.ix_(rows, cols)].copy()
                sub[motion[np.ix_(rows, cols)]] = 1e5
                m, _, _ = th.match_with_threshold(sub, thr)
                want.extend((int(rows[x]), int(cols[y])) for x, y in m)
        assert sorted(got) == sorted(want), case
        assert all(dl[r] == tl[t] and not motion[r, t] for r, t in got)


# ----------------------------------------------------------------------------------------------------------------------- the crossing scene
def _run(seq, where, **kw):
    """The reference loop over the scene -> (cross-class matches of all stages, the jump detection's stage-1 match or None, its match of stages 1 /
    2 or None, the number of low-score matches)."""
    trk = gate_ref.Tracker(**kw)
    cross = lows = 0
    jump1 = jump = None
    for f, fr in enumerate(seq):
        labels_before = [t.label for t in trk.tracks]
        trk.update(*fr)
        det_index = trk.last_costs[2] if trk.last_costs else []
        pairs = [(det_index[r], t) for r, t in trk.last_matches] + list(trk.last_low_matches or [])
        cross += sum(int(fr[1][d]) != int(labels_before[t]) for d, t in pairs)
        lows += len(trk.last_low_matches or [])
        if f == gate_ref.JUMP_FRAME:
            row = where[f][gate_ref.C]
            jump1 = next((t for r, t in trk.stage1 if det_index[r] == row), None)
            jump = next((t for r, t in trk.last_matches if det_index[r] == row), None)
    return cross, jump1, jump, lows


def test_crossing_scene_on_the_reference_loop():
    seq, where = gate_ref.crossing_scene()
    A, B, C = gate_ref.A, gate_ref.B, gate_ref.C
    assert len(seq) == 30
    for f in gate_ref.CROSS_FRAMES:
        assert gate_ref.iou(seq[f][0][where[f][A]], seq[f][0][where[f][B]]) > 0.5
        assert np.array_equal(seq[f][3][where[f][A]], seq[f][3][where[f][B]]) and seq[f][1][where[f][A]] != seq[f][1][where[f][B]]
    f = gate_ref.JUMP_FRAME
    assert gate_ref.iou(seq[f][0][where[f][C]], seq[f - 1][0][where[f - 1][C]]) == 0 and np.array_equal(seq[f + 1][0][where[f + 1][C]], seq[f - 1][0][where[f - 1][C]])
    for fr in seq:
        assert (np.diff(fr[2]) <= 0).all()                       # score-sorted rows, as the detector's
    # ungated: at least one cross-class match, and the jump is matched (by appearance alone)
    for kw in (dict(), KAL, dict(low_threshold=0.1)):
        cross, jump1, jump, lows = _run(seq, where, **kw)
        assert cross >= 1 and jump1 is not None and jump is not None, kw
        assert lows >= 1 or "low_threshold" not in kw
    # class_aware: no cross-class match in any stage, with every Kalman mode and with the low-score stage (which does match)
    for kw in (dict(), dict(use_kalman=True), KAL, dict(low_threshold=0.1), dict(low_threshold=0.1, **KAL)):
        cross, jump1, jump, lows = _run(seq, where, class_aware=True, **kw)
        assert cross == 0 and jump1 is not None, kw
        assert lows >= 1 or "low_threshold" not in kw
    # motion_gate: the jump is not matched in stage 1 (nor by its box: it does not overlap)
    for kw in (dict(), dict(motion_weight=0.98), dict(class_aware=True), dict(class_aware=True, low_threshold=0.1)):
        cross, jump1, jump, _ = _run(seq, where, motion_gate=True, **KAL, **kw)
        assert jump1 is None and jump is None, kw
        assert cross == 0 or not kw.get("class_aware")
