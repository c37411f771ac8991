"""No GPU: the tracking evaluation's numpy + scipy restatement (tests/mot_eval_ref.py) on hand-worked cases — TrackEval is not available,
so these pin the restatement itself —, the entry points' C-ABI declarations and argument checks, and the Python surface's refusals."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import mot_eval_ref as ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib, mot_eval

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("cnl_mot_similarity_f64", "cnl_mot_hota_workspace_bytes", "cnl_mot_hota_f64", "cnl_mot_clear_workspace_bytes", "cnl_mot_clear_f64",
                "cnl_mot_identity_workspace_bytes", "cnl_mot_identity_f64")
BOX = np.array([[10.0, 10.0, 20.0, 40.0]])


def one_object(tracker_ids):
    """One object with box [10, 10, 20, 40], identical on both sides, ground-truth id 1, one frame per tracker id."""
    return [(BOX, [1], BOX, [t]) for t in tracker_ids]


# ----------------------------------------------------------------------------- 1. hand-worked values
def test_a_perfect_track_scores_one():
    m = ref.evaluate_sequence(one_object([7, 7, 7, 7]))
    assert (m["HOTA"] == 1.0).all() and m["MOTA"] == 1.0 and m["IDF1"] == 1.0
    assert ref.evaluate_mot_tracking_sequence([BOX] * 4, [[7]] * 4, [BOX] * 4, [[1]] * 4) == {"HOTA": 1.0, "MOTA": 1.0, "IDF1": 1.0}
    assert list(ref.evaluate_mot_tracking_sequence([BOX], [[7]], [BOX], [[1]])) == ["HOTA", "MOTA", "IDF1"]
    assert (m["HOTA_TP"] == 4).all() and (m["LocA"] == 1.0).all() and m["MT"] == 1 and m["Frag"] == 0 and m["CLR_Frames"] == 4


def test_one_identity_switch_by_hand():
    """Tracker id 7 in frames 1-2, 9 in frames 3-4.  CLEAR: 4 TP, one switch: MOTA = (4 - 0 - 1) / 4.  Identity: the ground truth keeps one
    of the two trackers (2 frames): IDTP 2, IDFN 2, IDFP 2, IDF1 = 2 / (2 + 1 + 1).  HOTA: every frame matches at s = 1, so DetA = 1; each
    of the two pairs has m = 2 of gt_count + trk_count - m = 4 + 2 - 2 = 4: AssA = (2 * 2/4 + 2 * 2/4) / 4 = 0.5; HOTA = sqrt(0.5)."""
    m = ref.evaluate_sequence(one_object([7, 7, 9, 9]))
    assert m["IDSW"] == 1 and m["MOTA"] == 0.75
    assert (m["IDTP"], m["IDFN"], m["IDFP"], m["IDF1"]) == (2, 2, 2, 0.5)
    assert (m["AssA"] == 0.5).all() and (m["DetA"] == 1.0).all()
    assert (m["HOTA"] == 0.7071067811865476).all() and 0.7071067811865476 == np.sqrt(0.5)
    assert (m["AssRe"] == 0.5).all() and (m["AssPr"] == 1.0).all() and m["Frag"] == 0 and m["MOTP"] == 1.0


def test_exact_half_counts_as_a_match():
    s = ref.similarity([[0, 0, 2, 1]], [[0, 0, 1, 1]])
    assert s[0, 0] == 0.5
    m = ref.evaluate_sequence([(np.array([[0.0, 0, 2, 1]]), [3], np.array([[0.0, 0, 1, 1]]), [5])])
    assert m["CLR_TP"] == 1 and m["IDTP"] == 1 and list(m["HOTA_TP"]) == [1] * 10 + [0] * 9      # alpha 0.05 .. 0.5 reach 0.5
    assert ref.similarity([[0, 0, 0, 5]], [[0, 0, 1, 1]])[0, 0] == 0.0                             # an empty box


# ----------------------------------------------------------------------------- 2. the early returns
def test_no_predictions_at_all():
    frames = [(np.array([[0.0, 0, 4, 4], [8.0, 8, 4, 4]]), [1, 2], np.zeros((0, 4)), []), (np.array([[0.0, 0, 4, 4]]), [1], np.zeros((0, 4)), [])]
    m = ref.evaluate_sequence(frames)
    assert (m["HOTA_FN"] == 3).all() and (m["LocA"] == 1.0).all() and not m["HOTA"].any() and not m["HOTA_TP"].any() and not m["HOTA_FP"].any()
    assert m["CLR_FN"] == 3 and m["ML"] == 2 and m["MLR"] == 1.0 and m["CLR_Frames"] == 0 and m["MOTA"] == 0.0 and m["CLR_TP"] == 0
    assert (m["IDFN"], m["IDFP"], m["IDTP"], m["IDF1"]) == (3, 0, 0, 0.0)


def test_no_ground_truth_at_all():
    frames = [(np.zeros((0, 4)), [], np.array([[0.0, 0, 4, 4], [8.0, 8, 4, 4]]), [4, 6])]
    m = ref.evaluate_sequence(frames)
    assert (m["HOTA_FP"] == 2).all() and (m["LocA"] == 1.0).all() and not m["HOTA_FN"].any()
    assert m["CLR_FP"] == 2 and m["MLR"] == 1.0 and m["ML"] == 0 and m["CLR_FN"] == 0
    assert (m["IDFN"], m["IDFP"], m["IDTP"]) == (0, 2, 0)


# ----------------------------------------------------------------------------- 3. the CLEAR quirk
@pytest.mark.parametrize("empty_side", ["gt", "pred"])
def test_prev_step_survives_a_frame_that_is_empty_on_one_side(empty_side):
    """Ground truth 1 is tracked by 7, then a frame without ground truth (or without predictions), then trackers 7 and 9 both sit on it:
    the 1000 bonus of prev_step still favours 7 — and the object's track does not count as fragmented."""
    both = np.array([[10.0, 10, 20, 40], [10.0, 10, 20, 40]])
    gap = (np.zeros((0, 4)), [], BOX, [7]) if empty_side == "gt" else (BOX, [1], np.zeros((0, 4)), [])
    frames = [(BOX, [1], BOX, [7]), gap, (BOX, [1], both, [9, 7])]
    data, trace = ref.prepare(frames), []
    m = ref.clear(data, trace)
    assert trace[0][0] == 0 and trace[1][0] == 0 and trace[2][0] == 0        # relabelled tracker id 0 = 7, kept across the gap
    assert m["IDSW"] == 0 and m["Frag"] == 0 and m["CLR_TP"] == 2
    assert (m["CLR_FP"], m["CLR_FN"]) == ((2, 0) if empty_side == "gt" else (1, 1))
    # without the gap's special treatment (had the state been cleared) tracker 9, the first column, would win the tie
    cost = -ref.similarity(BOX, both)
    assert linear_sum_assignment(cost)[1][0] == 0


def test_idsw_through_prev_and_fragments():
    """The object leaves for a frame, returns under another tracker id: one switch through prev (not prev_step), two fragments -> Frag 1."""
    far = np.array([[100.0, 100, 5, 5]])
    frames = [(BOX, [1], BOX, [7]), (BOX, [1], far, [7]), (BOX, [1], BOX, [9])]
    m = ref.evaluate_sequence(frames)
    assert m["IDSW"] == 1 and m["Frag"] == 1 and m["CLR_TP"] == 2 and m["CLR_FN"] == 1 and m["CLR_FP"] == 1


# ----------------------------------------------------------------------------- 4. the assignments
def test_the_restatements_assignments_are_scipys_and_optimal():
    rng = np.random.default_rng(5)
    frames = []
    for _ in range(6):
        n, k = rng.integers(1, 5), rng.integers(1, 5)
        frames.append((np.concatenate([rng.integers(0, 8, (n, 2)), rng.integers(1, 8, (n, 2))], 1).astype(np.float64), rng.permutation(9)[:n],
                       np.concatenate([rng.integers(0, 8, (k, 2)), rng.integers(1, 8, (k, 2))], 1).astype(np.float64), rng.permutation(9)[:k]))
    del ref.solves[:]
    ref.evaluate_sequence(frames)
    assert len(ref.solves) == 6 + 6 + 1                                       # HOTA and CLEAR per frame, Identity once
    for cost, rows, cols in ref.solves:
        r2, c2 = linear_sum_assignment(cost)
        assert (rows == r2).all() and (cols == c2).all()
        n, k = cost.shape
        if max(n, k) <= 6:                                                    # brute force: no cheaper complete assignment exists
            small, large = min(n, k), max(n, k)
            c = cost if n <= k else cost.T
            best = min(sum(c[i, p[i]] for i in range(small)) for p in itertools.permutations(range(large), small))
            assert cost[rows, cols].sum() == pytest.approx(best, abs=1e-12)
    del ref.solves[:]


# ----------------------------------------------------------------------------- 5. / 6. the entry points
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "centernet_gfx950.h")).read()
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\(", header), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert "typedef struct cnl_mot_tables" in header and ctypes.sizeof(_lib.MotTables) == 8 * 28
    members = re.search(r"typedef struct cnl_mot_tables \{(.*?)\} cnl_mot_tables;", header, re.S).group(1)
    members = re.sub(r"/\*.*?\*/", "", members, flags=re.S)
    names = re.findall(r"(\w+)\s*[;,]", members)
    assert tuple(names) == _lib.MotTables.POINTERS + _lib.MotTables.SCALARS                          # the binding's layout is the header's
    assert "MotEvaluator" in cl.__all__ and "evaluate_mot_tracking_sequence" in cl.__all__ and cl.MotEvaluator is mot_eval.MotEvaluator
    assert "mot_eval.hip" in open(os.path.join(ROOT, "centernet-lightning_amd", "csrc", "Makefile")).read()


def test_abi_version_stays_13():
    assert _lib.load().cnl_version() == 13 and _lib.ABI_VERSION == 13


def _host_tables(**change):
    """Tables of one 1 x 1 frame whose pointers are (aligned) HOST buffers: every check below must answer before anything is launched."""
    keep = {n: np.zeros(8, np.int64) for n in _lib.MotTables.POINTERS}
    scalars = dict(F=1, S=1, n_gt=1, n_pr=1, sim_total=1, pair_total=1, sum_g=1, sum_t=1, id_total=4, max_gids=1, max_gt_frame=1, max_pr_frame=1,
                   max_frame_pairs=1)
    scalars.update({k: v for k, v in change.items() if k in scalars})
    ptrs = {n: keep[n].ctypes.data for n in keep}
    ptrs.update({k: v for k, v in change.items() if k in ptrs})
    return _lib.MotTables(**ptrs, **scalars), keep


@pytest.mark.parametrize("change", [dict(S=0), dict(F=-1), dict(n_gt=-1), dict(sim_total=-5), dict(gt_off=None), dict(seq_idm=None), dict(gt_ids=None),
                                    dict(gt_count=None), dict(max_gt_frame=2), dict(max_frame_pairs=2), dict(max_gids=3), dict(gt_off="odd"),
                                    dict(S=70000), dict(out="null"), dict(out="odd"), dict(ws_bytes=0)])
def test_bad_arguments_are_refused_without_a_device(change):
    lib = _lib.load()
    out_mode, ws_bytes = change.pop("out", None), change.pop("ws_bytes", 1 << 20)
    if change.get("gt_off") == "odd":
        change["gt_off"] = np.zeros(8, np.int64).ctypes.data + 4          # (never read: the check comes first)
    tab, keep = _host_tables(**change)
    space = np.zeros(1 << 17, np.int64)
    out = None if out_mode == "null" else space.ctypes.data + (4 if out_mode == "odd" else 0)
    ref_ = ctypes.byref(tab)
    calls = [lambda: lib.cnl_mot_hota_f64(ref_, space.ctypes.data, space.ctypes.data, out, out, out, space.ctypes.data, ws_bytes, None),
             lambda: lib.cnl_mot_clear_f64(ref_, space.ctypes.data, out, out, out, space.ctypes.data, ws_bytes, None),
             lambda: lib.cnl_mot_identity_f64(ref_, space.ctypes.data, space.ctypes.data, out, out, space.ctypes.data, ws_bytes, None)]
    for call in calls:
        assert call() == _lib.CNL_E_BAD_ARG
        assert "cnl_mot_" in _lib.last_error()
    if out_mode is None and ws_bytes and "gt_ids" not in change and "gt_count" not in change:      # (what the similarity and the queries judge too)
        assert lib.cnl_mot_similarity_f64(ref_, space.ctypes.data, None) == _lib.CNL_E_BAD_ARG
        for q in ("hota", "clear", "identity"):
            assert getattr(lib, f"cnl_mot_{q}_workspace_bytes")(ref_) == 0


def test_null_tables_and_oversized_frames():
    lib = _lib.load()
    assert lib.cnl_mot_similarity_f64(None, None, None) == _lib.CNL_E_BAD_ARG
    assert lib.cnl_mot_hota_workspace_bytes(None) == 0
    # 1025 x 1025 objects in a frame: the solver's LDS does not hold it
    tab, keep = _host_tables(n_gt=1025, n_pr=1025, sim_total=1025 * 1025, max_gt_frame=1025, max_pr_frame=1025, max_frame_pairs=1025 * 1025)
    assert lib.cnl_mot_similarity_f64(ctypes.byref(tab), keep["gt_off"].ctypes.data, None) == _lib.CNL_E_UNSUPPORTED
    tab, keep = _host_tables(n_gt=4097, n_pr=1, sim_total=4097, max_gt_frame=4097, max_pr_frame=1, max_frame_pairs=4097)
    assert lib.cnl_mot_similarity_f64(ctypes.byref(tab), keep["gt_off"].ctypes.data, None) == _lib.CNL_E_UNSUPPORTED


def test_workspace_queries_are_pure_host_functions():
    lib = _lib.load()
    tab, _ = _host_tables(F=3, n_gt=5, n_pr=7, sim_total=12, pair_total=6, sum_g=2, sum_t=3, id_total=25, max_gids=2, max_gt_frame=2, max_pr_frame=3,
                          max_frame_pairs=6, S=2)
    r = ctypes.byref(tab)
    assert lib.cnl_mot_hota_workspace_bytes(r) == 8 * (5 + 7 + 6 + 12 + 3 * 19 + 2 * 57) + 4 * (6 * 19 + 5 + 3 * 19 + 3) + 4
    assert lib.cnl_mot_clear_workspace_bytes(r) == 8 * 2 * 6 + 40
    assert lib.cnl_mot_identity_workspace_bytes(r) == 8 * 25


# ----------------------------------------------------------------------------- 7. the Python refusals
def test_python_refusals():
    ev = cl.MotEvaluator()
    with pytest.raises(ValueError, match="repeats an id"):
        ev.update([np.zeros((2, 4))], [[3, 3]], [np.zeros((0, 4))], [[]])
    with pytest.raises(ValueError, match="repeats an id"):
        ev.update([np.zeros((0, 4))], [[]], [np.ones((2, 4))], [torch.tensor([5, 5])])
    with pytest.raises(ValueError, match="frames"):
        ev.update([BOX, BOX], [[1], [1]], [BOX], [[1]])
    with pytest.raises(ValueError, match="boxes for"):
        ev.update([BOX], [[1, 2]], [BOX], [[1]])
    with pytest.raises(ValueError, match="boxes for"):
        ev.update([BOX], [[1]], [BOX], [[]])
    with pytest.raises(ValueError, match="x y w h"):
        ev.update([np.zeros((1, 5))], [[1]], [BOX], [[1]])
    with pytest.raises(ValueError, match="not finite"):
        ev.update([np.array([[0.0, 0, np.inf, 1]])], [[1]], [BOX], [[1]])
    with pytest.raises(ValueError, match="one entry per frame"):
        ev.update(BOX, [[1]], [BOX], [[1]])
    with pytest.raises(RuntimeError, match="nothing"):
        ev.get_metrics()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        cl.MotEvaluator("cpu")


def test_pooling_relabels_per_sequence_and_refuses_oversized_frames():
    ev = cl.MotEvaluator()
    ev.update([BOX, np.concatenate([BOX, BOX])], [[40], [9, 40]], [BOX, BOX], [[5], [5]], sequence="a")
    ev.update([BOX], [torch.tensor([3])], [torch.tensor(BOX)], [[8]], sequence="b")
    arrays, scalars, facts = mot_eval.pool(list(ev._sequences.items()))
    assert list(arrays["pr_ids"]) == [1, 0, 1, 0] and list(arrays["gt_ids"]) == [0, 0, 0]
    assert list(arrays["gt_off"]) == [0, 1, 2, 3] and list(arrays["pr_off"]) == [0, 1, 3, 4] and list(arrays["sim_off"]) == [0, 1, 3, 4]
    assert list(arrays["seq_frm"]) == [0, 2, 3] and list(arrays["seq_tid"]) == [0, 2, 3] and list(arrays["seq_pair"]) == [0, 2, 3]
    assert list(arrays["seq_idm"]) == [0, 9, 13] and list(arrays["pr_count"]) == [1, 2, 1] and list(arrays["gt_count"]) == [2, 1]
    assert scalars["max_frame_pairs"] == 2 and scalars["max_gids"] == 1 and [f["name"] for f in facts] == ["a", "b"]
    ev.reset()
    assert not ev._sequences
    big = cl.MotEvaluator()
    big.update([np.ones((1025, 4))], [np.arange(1025)], [np.ones((1025, 4))], [np.arange(1025)])
    with pytest.raises(ValueError, match="at most 1024"):
        mot_eval.pool(list(big._sequences.items()))


def test_host_fields_and_combination_equal_the_restatement():
    """The evaluator's host arithmetic (final fields, COMBINED_SEQ) on the restatement's own sums gives the restatement's fields, bit for bit."""
    rng = np.random.default_rng(2)
    seqs = {}
    for name, n_frames in (("x", 6), ("y", 4)):
        frames = []
        for _ in range(n_frames):
            n, k = rng.integers(0, 4), rng.integers(0, 4)
            frames.append((np.concatenate([rng.integers(0, 6, (n, 2)), rng.integers(1, 6, (n, 2))], 1).astype(np.float64), rng.permutation(5)[:n],
                           np.concatenate([rng.integers(0, 6, (k, 2)), rng.integers(1, 6, (k, 2))], 1).astype(np.float64), rng.permutation(5)[:k]))
        seqs[name] = frames
    want = ref.evaluate(seqs)
    mine = mot_eval.combine_sequences({k: want[k] for k in seqs})
    for key, v in want["COMBINED_SEQ"].items():
        if isinstance(v, np.ndarray):
            assert v.tobytes() == np.asarray(mine[key]).astype(v.dtype).tobytes(), key
        else:
            assert v == mine[key] and type(v) is type(mine[key]), key
