"""GPU: the per-track Kalman filter on the device (csrc/track_kalman.hip, `kalman="device"` of Tracker / TrackerBank).

Yardsticks: tests/kalman_ref.py, the numpy restatement of the header's rule, for the entry point (uint64 / uint32 bit patterns, guarded outputs);
the host path (`kalman="host"`, BoxKalman) and oracle/tracker_ref.py for the trackers (ids and states equal, boxes to 1e-6 — the bar the
existing Kalman tests hold the host path to —, velocities within the bound tests/test_kalman_host.py measures for the restatement)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import kalman_ref
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, _track_host
from strided_io import GuardedBytes
from test_kalman_host import BOUND_DX

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW = dict(detection_threshold=0.3, reid_threshold=0.2, box_cost="iou", box_threshold=0.5, smoothing_factor=0.5, use_kalman=True)


def _quiet(cls, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cls(*a, **kw)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


# ----------------------------------------------------------------------------- the entry point
def launch(x, P, det, src_trk, src_det, flags, new_box, mapped=False):
    """One guarded cnl_track_kalman_f64 launch.  x / P: numpy or None; new_box: what cnl_track_apply_f32 "left" (pre-fill).  mapped: the three
    lists, out_box and out_status in cnl_host_alloc memory.  -> (new_x, new_P [T, 64], new_box, out_box, out_status) as numpy."""
    lib = _lib.load()
    T = len(src_trk)
    dx, dP, dd = (None if x is None else _dev(x)), (None if P is None else _dev(P)), _dev(det)
    lists = np.stack([src_trk, src_det, flags]).astype(np.int32)
    keep = []
    if mapped:
        m = _track_host._Mapped(lists.nbytes)
        m.np.view(np.int32)[:] = lists.ravel()
        lp = [m.ptr + 4 * T * i for i in range(3)]
        keep.append(m)
    else:
        dl = _dev(lists)
        lp = [dl.data_ptr() + 4 * T * i for i in range(3)]
    g = {}
    for name, per, align in (("new_x", 64, 8), ("new_P", 512, 8), ("new_box", 16, 4), ("out_box", 32, 8), ("out_status", 4, 4)):
        if mapped and name.startswith("out"):
            need = GuardedBytes.wrapped_bytes(T * per, align=align)
            mm = _track_host._Mapped(need)
            keep.append(mm)
            g[name] = GuardedBytes(T * per, align=align, name=name, wrap=(mm.ptr, need))
        else:
            g[name] = GuardedBytes(T * per, align=align, device=DEV, name=name)
    g["new_box"].typed(torch.float32, (T, 4)).copy_(_dev(new_box))
    rc = lib.cnl_track_kalman_f64(dx.data_ptr() if dx is not None else None, dP.data_ptr() if dP is not None else None, dd.data_ptr(), *lp, T,
                                  g["new_x"].ptr, g["new_P"].ptr, g["new_box"].ptr, g["out_box"].ptr, g["out_status"].ptr,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    for b in g.values():
        ok, msg = b.verdict()
        assert ok, msg
    if dx is not None:
        assert np.array_equal(_bits(dx.cpu().numpy()), _bits(x)) and np.array_equal(_bits(dP.cpu().numpy()), _bits(P))      # the old tables are inputs
    return (g["new_x"].result(torch.float64, (T, 8)).numpy(), g["new_P"].result(torch.float64, (T, 64)).numpy(),
            g["new_box"].result(torch.float32, (T, 4)).numpy(), g["out_box"].result(torch.float64, (T, 4)).numpy(),
            g["out_status"].result(torch.int32, (T,)).numpy())


def case(T, seed, k=200):
    """Three chained steps at T rows: step 0 all births; steps 1, 2 mix births, matched and carried rows, rows without the predict bit, and a
    non-monotone src_trk with deleted old rows.  -> list of (det, src_trk, src_det, flags, new_box pre-fill)."""
    rng = np.random.default_rng(seed)
    steps = []
    for step in range(3):
        c, s = rng.uniform(0, 0.7, (k, 2)), rng.uniform(0.03, 0.3, (k, 2))
        det = np.concatenate([c, c + s], 1).astype(np.float32)
        src_trk = np.full(T, -1, np.int32)
        if step:
            n_old = max(1, 2 * T // 3)
            src_trk[rng.permutation(T)[:n_old]] = rng.permutation(T)[:n_old]
        src_det = rng.permutation(k)[:T].astype(np.int32)
        carried = (src_trk >= 0) & (rng.random(T) < 0.35)
        if T == 1:                          # the one row: born, matched, carried
            carried[:] = step == 2
        src_det[carried] = -1
        flags = (rng.random(T) < 0.7).astype(np.int32) | (rng.integers(0, 2, T).astype(np.int32) << 1)       # bit 1 means nothing
        if T == 1:
            flags |= 1                      # (without the prediction behind its birth, the update of the one row would leave its velocities at 0)
        if step and T > 8:
            live = np.flatnonzero(src_trk >= 0)
            assert carried.any() and (~carried[live]).any() and (src_trk < 0).any() and (flags & 1 == 0).any()
            assert (np.diff(src_trk[live]) < 0).any() and len(set(src_trk[live])) < T
        steps.append((det, src_trk, src_det, flags, rng.random((T, 4)).astype(np.float32)))
    return steps


def run_case(steps, mapped=False, check=True):
    x = P = None
    outs = []
    for det, src_trk, src_det, flags, pre in steps:
        got = launch(x, P, det, src_trk, src_det, flags, pre, mapped)
        if check:
            ref = kalman_ref.track_kalman(x, P, det, src_trk, src_det, flags, len(src_trk), pre)
            for name, a, b in zip(("new_x", "new_P", "new_box", "out_box", "out_status"), ref, got):
                assert np.array_equal(_bits(a), _bits(b)), (name, len(src_trk), int(np.count_nonzero(_bits(a) != _bits(b))))
            carried = src_det < 0
            assert np.array_equal(_bits(got[2][carried]), _bits(pre[carried]))            # carried rows of new_box: untouched
            assert not got[4].any()
        outs.append(got)
        x, P = got[0], got[1]
    return outs


@pytest.mark.parametrize("T,mapped", [(1, False), (63, False), (64, False), (65, False), (130, False), (65, True)])
def test_kernel_bits_against_the_restatement(T, mapped):
    outs = run_case(case(T, 100 + T), mapped)
    P = outs[-1][1].reshape(T, 8, 8)
    assert np.array_equal(_bits(P), _bits(P.transpose(0, 2, 1).copy()))        # stored exactly symmetric
    assert np.abs(outs[-1][0][:, 4:]).max() > 0                                # the state left its initial diagonal: velocities moved


def test_degenerate_and_non_finite_rows_stay_in_their_rows():
    """65 rows that all live through three steps (births, then two matched steps through a permutation): one born from a zero-area box, one
    measured as NaN at step 1.  Their status and outputs follow the rule (NaN positions equal, every finite value bit-equal — the payload of a
    NaN is the arithmetic unit's, not the rule's); the other 63 rows equal the run without the two, bit for bit."""
    T, k = 65, 80
    rng = np.random.default_rng(9)
    perm = rng.permutation(T).astype(np.int32)
    dets = []
    for step in range(3):
        c, s = rng.uniform(0, 0.7, (k, 2)), rng.uniform(0.03, 0.3, (k, 2))
        dets.append(np.concatenate([c, c + s], 1).astype(np.float32))
    sd = [rng.permutation(k)[:T].astype(np.int32) for _ in range(3)]
    flags = np.ones(T, np.int32)
    flags[::7] = 0
    pre = np.zeros((T, 4), np.float32)

    def run(dets):
        x = P = None
        outs, refs = [], []
        for step in range(3):
            st = np.full(T, -1, np.int32) if step == 0 else perm
            refs.append(kalman_ref.track_kalman(x, P, dets[step], st, sd[step], flags, T, pre))
            outs.append(launch(x, P, dets[step], st, sd[step], flags, pre))
            x, P = outs[-1][0], outs[-1][1]
        return outs, refs

    clean, _ = run(dets)
    planted = [d.copy() for d in dets]
    flat, nan = 10, 20                                              # rows of step 0; where they sit later: through perm
    planted[0][sd[0][flat], 2:] = planted[0][sd[0][flat], :2]
    row1 = {r: int(np.flatnonzero(perm == r)[0]) for r in (flat, nan)}         # the row of step 1 that continues row r of step 0
    row2 = {r: int(np.flatnonzero(perm == row1[r])[0]) for r in (flat, nan)}
    planted[1][sd[1][row1[nan]], 1] = np.nan
    got, refs = run(planted)
    assert got[0][4].tolist() == [0] * T
    assert np.flatnonzero(got[1][4]).tolist() == [row1[flat]] and got[1][4][row1[flat]] == 1          # S = 0: no pivot
    assert sorted(np.flatnonzero(got[2][4]).tolist()) == sorted(row2.values()) and np.isnan(got[1][0][row1[nan]]).any()
    hit = [{flat}, set(row1.values()), set(row2.values())]
    for step in range(3):
        rest = [r for r in range(T) if r not in hit[step]]
        for name, a, b, r in zip(("new_x", "new_P", "new_box", "out_box", "out_status"), clean[step], got[step], refs[step]):
            assert np.array_equal(_bits(a[rest]), _bits(b[rest])), (step, name)
            assert np.array_equal(_bits(r[rest]), _bits(b[rest])), (step, name)
            for q in hit[step]:                                     # the planted rows' own outputs follow the rule
                fin = np.isfinite(r[q])
                assert np.array_equal(np.isnan(r[q]), np.isnan(b[q])) and np.array_equal(_bits(r[q][fin]), _bits(b[q][fin])), (step, name, q)
    # the zero-area row: kept as loaded at step 1 (then predicted: nothing to add to a zero P), its box row = its state
    assert np.array_equal(got[1][3][row1[flat]], got[0][3][flat]) and not got[1][1][row1[flat]].any()


def test_two_runs_give_equal_bytes():
    steps = case(130, 230)
    a, b = run_case(steps, check=False), run_case(steps, check=False)
    for s in range(3):
        for u, v in zip(a[s], b[s]):
            assert np.array_equal(_bits(u), _bits(v))


# ----------------------------------------------------------------------------- Tracker
def _boxes(tracks):
    return np.array([np.asarray(t.bbox, np.float64) for t in tracks]).reshape(-1, 4)


def _host_run(seq, tracker):
    """Per frame (ids, states, boxes, filter states x) of a tracker whose tracks carry host filters (cl.Tracker kalman="host", or the oracle)."""
    out = []
    for fr in seq:
        tracker.update(*fr)
        out.append(([t.track_id for t in tracker.tracks], [t.state.name for t in tracker.tracks], _boxes(tracker.tracks),
                    np.array([t.kf.x for t in tracker.tracks]).reshape(-1, 8)))
    return out


def _no_host_filter(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("kalman='device' must not build or call a host filter")
    for name in ("__init__", "predict", "update"):
        monkeypatch.setattr(_track_host.BoxKalman, name, refuse)


def _check_against(tracks, rec, f):
    ids, states, boxes, _ = rec
    assert [t.track_id for t in tracks] == ids, f
    assert [t.state.name for t in tracks] == states, f
    np.testing.assert_allclose(_boxes(tracks), boxes, rtol=0, atol=1e-6)


def test_tracker_device_filter_on_a_sequence(monkeypatch):
    seq = tracker_ref.synth_sequence(11, frames=30, objects=10, k=40)
    host = _host_run(seq, _quiet(cl.Tracker, model=None, device=DEV, kalman="host", **KW))
    oracle = _host_run(seq, tracker_ref.Tracker(**KW))
    _no_host_filter(monkeypatch)
    trk = _quiet(cl.Tracker, model=None, device=DEV, kalman="device", **KW)
    moved = fresh = 0
    for f, fr in enumerate(seq):
        before = {t.track_id: t.bbox for t in trk.tracks}
        trk.update(*fr)
        _check_against(trk.tracks, host[f], f)
        _check_against(trk.tracks, oracle[f], f)
        table = trk._box[:len(trk.tracks)].cpu().numpy()
        xs = np.array([t.kf.x for t in trk.tracks]).reshape(-1, 8)
        for r, t in enumerate(trk.tracks):
            assert isinstance(t.kf, _track_host.DeviceKalman) and isinstance(t.bbox, np.ndarray) and t.bbox.dtype == np.float64 and t.bbox.shape == (4,)
            if t.track_id in before and t.bbox is before[t.track_id]:
                continue                                            # carried: keeps its bbox (and its table row keeps the last updated box)
            fresh += 1
            assert np.array_equal(_bits(table[r]), _bits(t.bbox.astype(np.float32))), (f, r)
            P = t.kf.P
            assert P.shape == (8, 8) and np.array_equal(_bits(P), _bits(P.T.copy()))
        if len(xs):                                                 # positions and velocities against the host filters'
            assert np.abs(xs - host[f][3]).max() <= BOUND_DX * np.abs(host[f][3]).max(), f
            assert np.abs(xs - oracle[f][3]).max() <= BOUND_DX * np.abs(oracle[f][3]).max(), f
        moved += int((np.abs(xs[:, 4:]).max(1) > 1e-4).sum()) if len(xs) else 0
        assert trk.kalman_skipped == 0
    assert moved > 20 and fresh > 100


# ----------------------------------------------------------------------------- TrackerBank
def _stack(frames):
    return tuple(np.stack([fr[i] for fr in frames]) for i in range(4))


def test_bank_device_filter_on_sequences(monkeypatch):
    """Three streams whose pooled table crosses 64 rows after a first step of stream 0 alone (the state tables are reallocated once), the
    partial steps at frames 7 and 8 (stream 1 absent: its filter state must not move), reset(stream=1) mid-sequence."""
    S = 3
    seqs = [tracker_ref.synth_sequence(11 + s, frames=31, objects=22 + 2 * s, k=40) for s in range(S)]
    oracles = [tracker_ref.Tracker(**KW) for _ in range(S)]
    _no_host_filter(monkeypatch)
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, kalman="device", **KW)
    singles = [_quiet(cl.Tracker, model=None, device=DEV, kalman="device", **KW) for _ in range(S)]
    caps, moved = set(), 0

    def rows(s):
        lo, hi = int(bank._off[s]), int(bank._off[s + 1])
        t = bank._table
        return tuple(a[lo:hi].cpu().numpy() for a in (t.kx, t.kP, t.box, t.emb))

    for f in range(31):
        live = [0] if f == 0 else [0, 2] if f in (7, 8) else list(range(S))
        if f == 16:
            keep = [rows(s) for s in (0, 2)]
            bank.reset(stream=1)
            singles[1].reset()
            oracles[1] = tracker_ref.Tracker(**KW)
            for s, before in zip((0, 2), keep):
                for a, b in zip(before, rows(s)):
                    assert np.array_equal(_bits(a), _bits(b))
            assert bank[1].tracks == [] and bank._off[2] == bank._off[1]
        still = rows(1) if 1 not in live and f else None
        fr = [seqs[s][oracles[s].frame] for s in live]
        prev = {id(t): t.bbox for s in range(S) for t in bank[s].tracks}
        bank.update_batch(*_stack(fr), streams=live)
        for s, x in zip(live, fr):
            oracles[s].update(*x)
            singles[s].update(*x)
        if still is not None:
            for a, b in zip(still, rows(1)):
                assert np.array_equal(_bits(a), _bits(b)), f           # not predicted, not moved
        caps.add(bank._table.kx.shape[0])
        assert bank._table.kx.shape[0] == bank._table.emb.shape[0] == bank._table.kP.shape[0]
        for s in range(S):
            tr, orc, one = bank[s].tracks, oracles[s].tracks, singles[s].tracks
            assert [t.track_id for t in tr] == [t.track_id for t in orc] == [t.track_id for t in one], (f, s)
            assert [t.state.name for t in tr] == [t.state.name for t in orc] == [t.state.name for t in one], (f, s)
            a = _boxes(tr)
            np.testing.assert_allclose(a, _boxes(orc), rtol=0, atol=1e-6)
            assert np.array_equal(_bits(a), _bits(_boxes(one))), (f, s)
            kx, kP, box, emb = rows(s)
            n, t1 = len(one), singles[s]._table
            if n:
                assert np.array_equal(_bits(kx), _bits(t1.kx[:n].cpu().numpy())) and np.array_equal(_bits(kP), _bits(t1.kP[:n].cpu().numpy())), (f, s)
                assert np.array_equal(_bits(box), _bits(t1.box[:n].cpu().numpy())) and np.array_equal(_bits(emb), _bits(t1.emb[:n].cpu().numpy())), (f, s)
                hx = np.array([t.kf.x for t in orc])
                assert np.abs(kx - hx).max() <= BOUND_DX * np.abs(hx).max(), (f, s)
                moved += int((np.abs(kx[:, 4:]).max(1) > 1e-4).sum())
            for r, t in enumerate(tr):
                assert isinstance(t.kf, _track_host.DeviceKalman)
                if prev.get(id(t)) is not t.bbox:                   # born or matched in this step: its table row is its filtered box
                    assert np.array_equal(_bits(box[r]), _bits(t.bbox.astype(np.float32))), (f, s, r)
    assert caps == {64, 128}, caps
    assert moved > 60 and int(bank._off[S]) > 64


# ----------------------------------------------------------------------------- host mode
def test_host_mode_is_untouched():
    """kalman="host" spelled out gives what the keyword's absence gives: ids, boxes and table bytes, for a Tracker and for a bank."""
    seq = tracker_ref.synth_sequence(11, frames=12, objects=10, k=40)
    a = _quiet(cl.Tracker, model=None, device=DEV, **KW)
    b = _quiet(cl.Tracker, model=None, device=DEV, kalman="host", **KW)
    c = _quiet(cl.Tracker, model=None, device=DEV, kalman="device", **dict(KW, use_kalman=False))       # accepted, without effect
    plain = _quiet(cl.Tracker, model=None, device=DEV, **dict(KW, use_kalman=False))
    for fr in seq:
        for t in (a, b, c, plain):
            t.update(*fr)
        for u, v in ((a, b), (plain, c)):
            n = len(u.tracks)
            assert [t.track_id for t in u.tracks] == [t.track_id for t in v.tracks]
            assert np.array_equal(_bits(_boxes(u.tracks)), _bits(_boxes(v.tracks)))
            assert np.array_equal(_bits(u._box[:n].cpu().numpy()), _bits(v._box[:n].cpu().numpy()))
            assert np.array_equal(_bits(u._emb[:n].cpu().numpy()), _bits(v._emb[:n].cpu().numpy()))
            assert v._table.kx is None and all(type(t.kf) is (_track_host.BoxKalman if v.use_kalman else type(None)) for t in v.tracks)
    S = 2
    seqs = [tracker_ref.synth_sequence(11 + s, frames=12, objects=10 + s, k=40) for s in range(S)]
    x = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **KW)
    y = _quiet(cl.TrackerBank, num_streams=S, device=DEV, kalman="host", **KW)
    for f in range(12):
        batch = _stack([seqs[s][f] for s in range(S)])
        x.update_batch(*batch)
        y.update_batch(*batch)
        n = int(x._off[S])
        assert np.array_equal(x._off, y._off) and y._table.kx is None
        assert np.array_equal(_bits(x._box[:n].cpu().numpy()), _bits(y._box[:n].cpu().numpy()))
        assert np.array_equal(_bits(x._emb[:n].cpu().numpy()), _bits(y._emb[:n].cpu().numpy()))
        for s in range(S):
            assert [t.track_id for t in x[s].tracks] == [t.track_id for t in y[s].tracks]
            assert np.array_equal(_bits(_boxes(x[s].tracks)), _bits(_boxes(y[s].tracks)))
