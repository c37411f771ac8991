"""CPU: the many-streams tracker's host side — the new C-ABI entry points (declared, exported, bound, argument validation without a
device), TrackerBank's argument validation, and the assignment algorithm the kernel is written against (tests/lsap_ref.py) held
to scipy.optimize.linear_sum_assignment, ties included."""
import ctypes
import os
import re
import warnings

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import lsap_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cnl_lsap_batch_f64", "cnl_track_streams_f32", "cnl_track_streams_workspace_bytes", "cnl_track_streams_record_bytes")


def test_new_entry_points_are_declared_exported_and_bound():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    declared = set(re.findall(r"\b(cnl_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None
    assert lib.cnl_version() == _lib.ABI_VERSION == 13           # new entry points only: the ABI version stays
    assert lib.cnl_sizeof_params(3) == 0                         # ... and no new params struct


def test_size_helpers():
    lib = _lib.load()
    for k, T, wd in [(48, 0, 1), (300, 70, 1), (300, 70, 0), (1024, 4096, 1), (7, 3, 0)]:
        need = lib.cnl_track_streams_record_bytes(k, T, wd)
        assert need % 8 == 0 and need >= 64 + 4 * k + 24 * k * wd + 12 * k + 4 * T
        assert need <= 64 + 24 * k * wd + 4 * (4 * k + T) + 16
    assert lib.cnl_track_streams_record_bytes(0, 3, 1) == 0 and lib.cnl_track_streams_record_bytes(4, -1, 1) == 0
    # 20 bytes per pair of the pooled table (f64 re-ID, f64 stage-2 sub-matrix, f32 box) + the index lists
    assert lib.cnl_track_streams_workspace_bytes(32, 300, 70) >= 20 * 32 * 300 * 70
    assert lib.cnl_track_streams_workspace_bytes(0, 300, 70) == 0 and lib.cnl_track_streams_workspace_bytes(2, 0, 70) == 0


def test_argument_errors_without_touching_a_device():
    lib = _lib.load()
    p = 0x1000                       # never dereferenced: every call below is refused on its arguments
    L = lib.cnl_lsap_batch_f64
    assert L(None, p, p, p, p, 2, 8, 8, p, p, p, None) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error()
    assert L(p, p, p, p, p, -1, 8, 8, p, p, p, None) == _lib.CNL_E_BAD_ARG
    assert L(p, p, p, p, p, 2, -8, 8, p, p, p, None) == _lib.CNL_E_BAD_ARG
    assert L(p, p, p, p, p, 2, 1025, 1025, p, p, p, None) == _lib.CNL_E_UNSUPPORTED and "1024" in _lib.last_error()
    assert L(p, p, p, p, p, 2, 8, 4097, p, p, p, None) == _lib.CNL_E_UNSUPPORTED and "4096" in _lib.last_error()
    assert L(p, p, p, p, p, 0, 8, 8, p, p, p, None) == 0                     # no problems: nothing to launch

    def streams(**kw):
        a = dict(det_emb=p, det_box=p, det_score=p, det_label=None, label_kind=0, S=4, S_live=4, live=p, k=48, E=64, thr=0.3, reid_thr=0.2,
                 box_thr=0.5, trk_emb=p, trk_box=p, trk_off=p, R=40, T_max=12, box_cost=1, reid_metric=0, with_dets=1, ws=p, ws_bytes=1 << 30,
                 rec=p, stride=1 << 16, stream=None)
        a.update(kw)
        return lib.cnl_track_streams_f32(*a.values())
    assert streams(det_emb=None) == _lib.CNL_E_BAD_ARG and "null" in _lib.last_error()
    assert streams(live=None) == _lib.CNL_E_BAD_ARG
    assert streams(S=0) == _lib.CNL_E_BAD_ARG
    assert streams(S_live=5) == _lib.CNL_E_BAD_ARG
    assert streams(k=-1) == _lib.CNL_E_BAD_ARG
    assert streams(R=-1) == _lib.CNL_E_BAD_ARG
    assert streams(k=2000) == _lib.CNL_E_UNSUPPORTED and "1024" in _lib.last_error()
    assert streams(T_max=5000) == _lib.CNL_E_UNSUPPORTED and "4096" in _lib.last_error()
    assert streams(box_cost=3) == _lib.CNL_E_BAD_ARG
    assert streams(reid_metric=8) == _lib.CNL_E_BAD_ARG
    assert streams(label_kind=2) == _lib.CNL_E_BAD_ARG                       # labels announced, none given
    assert streams(trk_emb=None) == _lib.CNL_E_BAD_ARG
    assert streams(rec=p + 4) == _lib.CNL_E_BAD_ARG
    assert streams(stride=64) == _lib.CNL_E_BAD_ARG and "cnl_track_streams_record_bytes" in _lib.last_error()
    assert streams(ws_bytes=1024) == _lib.CNL_E_BAD_ARG and "workspace" in _lib.last_error()
    with pytest.raises(ValueError):
        _lib.check(streams(k=2000), "cnl_track_streams_f32")


def test_tracker_bank_argument_validation(configs_dir):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert "TrackerBank" in cl.__all__
        for bad in (0, -3, 2.5, None, True):
            with pytest.raises(ValueError):
                cl.TrackerBank(num_streams=bad)
        # host-side costs are refused whatever allow_host_cost says: the bank keeps the matrices on the device
        for kw in (dict(reid_cost="minkowski"), dict(reid_cost="minkowski", allow_host_cost=True), dict(reid_cost=lambda a, b: a @ b.T, allow_host_cost=True),
                   dict(box_cost=lambda a, b: a @ b.T, allow_host_cost=True), dict(box_cost="diou")):
            with pytest.raises(ValueError):
                cl.TrackerBank(num_streams=2, **kw)
        bank = cl.TrackerBank(num_streams=4, device="cuda:0", reid_cost="euclidean", box_cost=None, use_kalman=True)
        ref = cl.Tracker(device="cuda:0")
        assert len(bank) == 4 and bank.use_kalman and bank.box_cost is None
        for name in ("nms_kernel", "num_detections", "detection_threshold", "reid_threshold", "box_threshold", "smoothing_factor", "max_inactive_age",
                     "min_birth_age"):
            assert getattr(cl.TrackerBank(num_streams=1), name) == getattr(ref, name), name
        for s in range(4):
            assert bank[s].tracks == [] and bank[s].frame == 0 and bank[s].next_track_id == 0
        z = lambda *shape: np.zeros(shape, np.float32)
        for streams in ([0, 4], [-1], [1, 1], []):
            with pytest.raises(ValueError):
                bank.update_batch(z(len(streams), 8, 4), z(len(streams), 8), z(len(streams), 8), z(len(streams), 8, 16), streams=streams)
        with pytest.raises(ValueError):                      # three streams' worth of detections for four streams
            bank.update_batch(z(3, 8, 4), z(3, 8), z(3, 8), z(3, 8, 16))
        with pytest.raises(ValueError):                      # one frame's arrays, not a batch of streams
            bank.update_batch(z(8, 4), z(8), z(8), z(8, 16), streams=[0])
        with pytest.raises(ValueError):
            bank.reset(stream=7)
        with pytest.raises(ValueError):
            bank.step_batch(__import__("torch").zeros(3, 3, 32, 32), streams=[0, 1])
        bank.reset()
        bank.reset(stream=2)
        # build_tracker: without num_streams exactly what it returned before
        cfg = os.path.join(configs_dir, "tracking_resnet34_fpn.yaml")
        t = cl.build_tracker(cfg)
        assert type(t) is cl.Tracker
        b = cl.build_tracker(cfg, num_streams=3)
        assert type(b) is cl.TrackerBank and len(b) == 3 and b.detection_threshold == t.detection_threshold and b.reid_cost == t.reid_cost


def _cases():
    out = []
    for seed in range(160):
        rng = np.random.default_rng(1000 + seed)
        for kind in lsap_ref.KINDS:
            n, T = (int(x) for x in rng.integers(1, 41, 2))
            out.append((kind, n, T, lsap_ref.matrices(kind, n, T, rng)))
    return out


def test_assignment_specification_equals_scipy_ties_included():
    """The restatement of tests/lsap_ref.py (the algorithm and the parallel selection key of csrc/track_streams.hip) returns scipy's
    rows and columns on 640 seeded matrices of four kinds with n, T in 1..40, n < T and n > T, for several lane counts (the merge of
    per-lane candidates must not depend on how the positions are dealt to lanes)."""
    cases = _cases()
    assert len(cases) >= 600
    shapes = {(n < T) - (n > T) for _, n, T, _ in cases}
    assert shapes == {-1, 0, 1}
    tied = 0
    for idx, (kind, n, T, m) in enumerate(cases):
        rows, cols = linear_sum_assignment(m)
        for lanes in ((64, 1, 7)[idx % 3], 4):
            r, c = lsap_ref.linear_sum_assignment(m, lanes=lanes)
            assert np.array_equal(r, rows) and np.array_equal(c, cols), (kind, n, T, lanes, idx)
        tied += kind != "uniform"
    assert tied >= 450


def test_assignment_specification_refuses_what_scipy_refuses():
    rng = np.random.default_rng(5)
    for bad in (np.nan, -np.inf):
        m = rng.random((6, 9))
        m[2, 3] = bad
        with pytest.raises(ValueError):
            linear_sum_assignment(m)
        with pytest.raises(ValueError):
            lsap_ref.linear_sum_assignment(m)
    m = rng.random((5, 8))
    m[1, :] = np.inf
    with pytest.raises(ValueError):
        linear_sum_assignment(m)
    with pytest.raises(ValueError):
        lsap_ref.linear_sum_assignment(m)
    m = rng.random((5, 8))
    m[1, 2:] = np.inf                                           # +inf entries are fine while an assignment exists
    assert np.array_equal(lsap_ref.linear_sum_assignment(m)[1], linear_sum_assignment(m)[1])


def test_threshold_comparison_types_of_the_host_path():
    """The device compares stage-1 costs as float64 against the double and stage-2 costs as float32 against the threshold rounded to
    float32: what `cost_matrix[rows, cols] < threshold` does under the installed numpy for a float64 / float32 matrix and a Python float."""
    thr = 0.7                                                   # float32(0.7) = 0.69999998807... lies BELOW the double 0.7
    c32 = np.float32(thr)
    assert float(c32) < thr
    # float32 matrix (the box stage): the threshold is rounded to float32 first, so a cost equal to float32(thr) is NOT below it ...
    assert not (np.array([c32], np.float32) < thr)[0]
    assert (np.array([np.nextafter(c32, np.float32(0))], np.float32) < thr)[0]
    # ... float64 matrix (the re-ID stage): compared as doubles, the same value IS below the threshold
    assert (np.array([float(c32)], np.float64) < thr)[0]
