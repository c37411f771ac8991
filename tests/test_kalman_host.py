"""CPU: the device Kalman filter's rule and interface without a device — the numpy restatement of cnl_track_kalman_f64 (tests/kalman_ref.py)
held to the host filter (`_track_host.BoxKalman`) and to the oracle's (`tracker_ref.BoxKalman`), its exact symmetry, its degenerate rows, and
the entry point's declaration, export, argument checks and the `kalman` keyword of Tracker / TrackerBank / build_tracker."""
import os
import re
import warnings

import numpy as np
import pytest

import kalman_ref
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, _track_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Restatement (LDL', sums in index order) against BoxKalman (np.linalg.inv, BLAS products), 200 tracks x 60 frames, relative to the frame's
# max |x| / max |P|: the maxima MEASURED by test_restatement_against_boxkalman on the CPU, and 64 times them — the margin covers the
# conditioning of other seeds' S; without it the test would pin one run's rounding.
MEASURED_DX, MEASURED_DP = 5.435e-16, 1.082e-15
BOUND_DX, BOUND_DP = 64 * MEASURED_DX, 64 * MEASURED_DP


def synth_tracks(seed, tracks=200, frames=60, missing=0.2):
    """-> (z float32 [frames, tracks, 4] measurements of drifting boxes, seen bool [frames, tracks]; frame 0 is always seen: the birth)."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0.05, 0.7, (tracks, 2))
    wh = rng.uniform(0.04, 0.25, (tracks, 2))
    v = rng.normal(0, 0.004, (tracks, 2))
    z = np.empty((frames, tracks, 4), np.float32)
    for f in range(frames):
        c = xy + f * v + rng.normal(0, 0.002, (tracks, 2))
        s = wh * (1 + rng.normal(0, 0.02, (tracks, 2)))
        z[f] = np.concatenate([c, c + s], 1).astype(np.float32)
    seen = rng.random((frames, tracks)) >= missing
    seen[0] = True
    return z, seen


def run_restatement(z, seen, on_frame=None):
    """The life of Tracker's filters through kalman_ref.track_kalman: birth at frame 0, update where seen, predict every frame."""
    frames, T = seen.shape
    x = P = None
    rows = np.arange(T, dtype=np.int32)
    for f in range(frames):
        src_trk = rows if f else np.full(T, -1, np.int32)
        src_det = np.where(seen[f], rows, -1).astype(np.int32)
        x, P, _, _, status = kalman_ref.track_kalman(x, P, z[f], src_trk, src_det, np.ones(T, np.int32), T, np.zeros((T, 4), np.float32))
        if on_frame is not None:
            on_frame(f, x, P.reshape(T, 8, 8), status)
    return x, P


@pytest.mark.parametrize("host", [_track_host.BoxKalman, tracker_ref.BoxKalman], ids=["package", "oracle"])
def test_restatement_against_boxkalman(host):
    """200 synthetic tracks, 60 frames, measurements rounded through float32, 20 % of the frames without one.  Measured on the CPU against either
    BoxKalman (the two give the same figures): max|dx| / max|x| = 5.435e-16, max|dP| / max|P| = 1.082e-15 (the order of the 4e-16 / 5e-15 a
    Cholesky variant of the update differs from the `inv` form by); asserted: 64 times these, 3.48e-14 and 6.92e-14."""
    z, seen = synth_tracks(3)
    frames, T = seen.shape
    filters = [None] * T
    worst = [0.0, 0.0]

    def compare(f, x, P, status):
        assert not status.any()
        for t in range(T):
            if f == 0:
                filters[t] = host(z[0, t])
            elif seen[f, t]:
                filters[t].update(z[f, t])
            filters[t].predict()
        hx, hP = np.array([k.x for k in filters]), np.array([k.P for k in filters])
        worst[0] = max(worst[0], np.abs(x - hx).max() / np.abs(hx).max())
        worst[1] = max(worst[1], np.abs(P - hP).max() / np.abs(hP).max())

    run_restatement(z, seen, compare)
    print(f"restatement vs {host.__module__}.BoxKalman: max|dx|/max|x| = {worst[0]:.3e}, max|dP|/max|P| = {worst[1]:.3e}")
    assert worst[0] <= BOUND_DX and worst[1] <= BOUND_DP, worst


def test_restatement_is_exactly_symmetric_after_every_step():
    z, seen = synth_tracks(4, tracks=50, frames=40)
    checked = []

    def symmetric(f, x, P, status):
        assert np.array_equal(P.view(np.uint64), P.transpose(0, 2, 1).copy().view(np.uint64)), f
        checked.append(f)

    run_restatement(z, seen, symmetric)
    # ... and after an update without the prediction behind it
    x, P = kalman_ref.init(z[0])
    x, P = kalman_ref.predict(x, P)
    x, P, ok = kalman_ref.update(x, P, z[1])
    assert ok.all() and np.array_equal(P.view(np.uint64), P.transpose(0, 2, 1).copy().view(np.uint64)) and len(checked) == 40


def test_degenerate_and_non_finite_rows():
    z, seen = synth_tracks(5, tracks=9, frames=4, missing=0.0)
    T = 9
    rows = np.arange(T, dtype=np.int32)
    ones, nb = np.ones(T, np.int32), np.zeros((T, 4), np.float32)
    born = np.full(T, -1, np.int32)

    def life(zs):
        x, P, _, _, st = kalman_ref.track_kalman(None, None, zs[0], born, rows, ones, T, nb)
        out = [(x, P, st)]
        for f in (1, 2, 3):
            x, P, box, _, st = kalman_ref.track_kalman(x, P, zs[f], rows, rows, ones, T, nb)
            out.append((x, P, st, box))
        return out

    clean = life(z)
    # a zero-area box: born with P = 0, so S = 0 at its first update — the status bit, the row as loaded (then predicted)
    flat = z.copy()
    flat[0, 4, 2:] = flat[0, 4, :2]
    got = life(flat)
    assert got[0][2].tolist() == [0] * T and not got[0][1][4].any()
    x0, P0, _ = got[0]
    x1, P1, st1, box1 = got[1]
    assert st1.tolist() == [0, 0, 0, 0, 1, 0, 0, 0, 0]
    px, pP = kalman_ref.predict(x0[4:5], P0[4:5].reshape(1, 8, 8))
    assert np.array_equal(x1[4], px[0]) and np.array_equal(P1[4], pP[0].ravel())
    assert np.array_equal(box1[4], x0[4, :4].astype(np.float32))       # its box row: the state it kept
    # a NaN measurement in row 6 at frame 2: the update goes through (S does not depend on z), x turns NaN, the next update finds no pivot
    bad = z.copy()
    bad[2, 6, 1] = np.nan
    got = life(bad)
    assert got[2][2].tolist() == [0] * T and np.isnan(got[2][0][6]).any() and got[3][2].tolist() == [0, 0, 0, 0, 0, 0, 1, 0, 0]
    others = [r for r in range(T) if r != 6]
    for (cx, cP, *_), (gx, gP, *_) in zip(clean, got):
        assert np.array_equal(cx[others].view(np.uint64), gx[others].view(np.uint64))
        assert np.array_equal(cP[others].view(np.uint64), gP[others].view(np.uint64))
    # a row without a source: zeros, bit 1
    x, P, box, ob, st = kalman_ref.track_kalman(None, None, z[0], np.array([-1, 0, -1], np.int32), np.array([0, 1, -1], np.int32),
                                                np.ones(3, np.int32), 3, np.full((3, 4), 7, np.float32))
    assert st.tolist() == [0, 2, 2] and not x[1:].any() and not P[1:].any() and (box[1:] == 7).all()


def test_entry_point_is_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    for name in ("cnl_track_kalman_f64", "cnl_track_kalman_out_bytes"):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert lib.cnl_version() == _lib.ABI_VERSION == 13
    assert len(_lib._SIGNATURES["cnl_track_kalman_f64"][1]) == 13
    assert lib.cnl_track_kalman_out_bytes(70) == 36 * 70 and lib.cnl_track_kalman_out_bytes(0) == 0 and lib.cnl_track_kalman_out_bytes(-3) == 0
    for word in ("L D L'", "out_status", "deviation", "ascending"):        # the rule is written in the header
        assert word in header[header.index("cnl_track_kalman_f64") - 6000:header.index("int cnl_track_kalman_f64")], word


def test_argument_errors_without_touching_a_device():
    lib = _lib.load()
    p = 0x1000                       # never dereferenced: every call below is refused on its arguments

    def call(**kw):
        a = dict(x=p, P=p + 0x1000, det_box=p, src_trk=p, src_det=p, flags=p, T_new=5, new_x=p + 0x2000, new_P=p + 0x3000, new_box=p, out_box=p,
                 out_status=p, stream=None)
        a.update(kw)
        return lib.cnl_track_kalman_f64(*a.values())
    assert call(T_new=-1) == _lib.CNL_E_BAD_ARG
    assert call(T_new=0) == 0                                                  # nothing to launch
    for name in ("det_box", "src_trk", "src_det", "flags", "new_x", "new_P", "new_box", "out_box", "out_status"):
        assert call(**{name: None}) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error(), name
    assert call(x=None) == _lib.CNL_E_BAD_ARG and call(P=None) == _lib.CNL_E_BAD_ARG       # both or neither
    assert call(new_x=p) == _lib.CNL_E_BAD_ARG and "alias" in _lib.last_error()
    for name in ("x", "P", "new_x", "new_P", "out_box"):
        assert call(**{name: p + 0x4004}) == _lib.CNL_E_BAD_ARG and "8-byte" in _lib.last_error(), name
    assert call(det_box=p + 8) == _lib.CNL_E_BAD_ARG and "16-byte" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(call(det_box=p + 8), "cnl_track_kalman_f64")


def test_kalman_keyword(configs_dir):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="'host'.*'device'"):
            cl.Tracker(use_kalman=True, kalman="bogus")
        with pytest.raises(ValueError, match="'host'.*'device'"):
            cl.TrackerBank(num_streams=2, use_kalman=True, kalman="gpu")
        t = cl.Tracker(use_kalman=True)
        assert t.kalman == "host" and not t._device_kalman and not t._table.kalman
        t = cl.Tracker(use_kalman=False, kalman="device")                      # accepted, without effect
        assert not t._device_kalman and not t._table.kalman and t._table.kx is None
        t = cl.Tracker(use_kalman=True, kalman="device")
        assert t._device_kalman and t._table.kalman
        import inspect
        for f in (cl.Tracker.__init__, cl.TrackerBank.__init__):
            assert list(inspect.signature(f).parameters)[-1] == "kalman" and inspect.signature(f).parameters["kalman"].default == "host"
        cfg = dict(cl.load_config(os.path.join(configs_dir, "tracking_resnet34_fpn.yaml"))["tracker"])
        cfg.update(use_kalman=True, kalman="device")
        bank = cl.build_tracker(cfg, num_streams=3)
        assert type(bank) is cl.TrackerBank and bank.kalman == "device" and bank._device_kalman and bank._table.kalman
        single = cl.build_tracker(cfg)
        assert type(single) is cl.Tracker and single._device_kalman
        # the host record of a track in either mode: no BoxKalman in device mode
        h = _track_host.Track(t, 0, np.zeros(4, np.float32), 0, use_kalman=True)
        d = _track_host.Track(t, 0, np.zeros(4, np.float32), 0, use_kalman="device")
        assert type(h.kf) is _track_host.BoxKalman and type(d.kf) is _track_host.DeviceKalman
        assert type(_track_host.Track(t, 0, np.zeros(4, np.float32), 0, use_kalman="host").kf) is _track_host.BoxKalman
