"""GPU: the many-streams tracker (csrc/track_streams.hip, TrackerBank).

Yardsticks: scipy.optimize.linear_sum_assignment for the assignment kernel (EXACT: the assignment, not its cost), oracle/tracker_ref.py
and one cl.Tracker per stream for the bank (ids, boxes, states and match lists equal; the pooled table's rows bit-equal to the
per-stream Tracker's: same kernels, same order), and the track_seq_*.npz goldens produced by the reference's own Tracker.update."""
import ast
import ctypes
import glob
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import lsap_ref
import recipes
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _lib
from centernet_lightning_amd.tracker import match_with_threshold

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SEQS = sorted(glob.glob(os.path.join(GOLDEN, "track_seq_*.npz")))
DEV = "cuda:0"


# ----------------------------------------------------------------------------- the assignment kernel
def run_lsap(mats, max_rows=None, max_cols=None, pad=0):
    """mats: list of float64 [n, T] -> (list of col4row arrays, status array); row stride = T + pad."""
    lib = _lib.load()
    B = len(mats)
    offs, outs, flat, o, q = [], [], [], 0, 0
    for m in mats:
        n, T = m.shape
        buf = np.full((n, T + pad), -123.0)
        buf[:, :T] = m
        flat.append(buf.ravel())
        offs.append(o)
        outs.append(q)
        o += buf.size
        q += n
    d = lambda a, t: torch.from_numpy(np.ascontiguousarray(np.asarray(a, t))).to(DEV)
    cost = d(np.concatenate(flat) if o else np.zeros(1), np.float64)
    c_off, o_off = d(offs, np.int64), d(outs, np.int64)
    ld, nr, nc = d([m.shape[1] + pad for m in mats], np.int32), d([m.shape[0] for m in mats], np.int32), d([m.shape[1] for m in mats], np.int32)
    col = torch.full((max(q, 1),), -7, device=DEV, dtype=torch.int32)
    status = torch.full((B,), -7, device=DEV, dtype=torch.int32)
    mr = max(m.shape[0] for m in mats) if max_rows is None else max_rows
    mc = max(m.shape[1] for m in mats) if max_cols is None else max_cols
    _lib.check(lib.cnl_lsap_batch_f64(cost.data_ptr(), c_off.data_ptr(), ld.data_ptr(), nr.data_ptr(), nc.data_ptr(), B, mr, mc, col.data_ptr(),
                                      o_off.data_ptr(), status.data_ptr(), None), "cnl_lsap_batch_f64")
    torch.cuda.synchronize()
    col, status = col.cpu().numpy(), status.cpu().numpy()
    return [col[outs[b]:outs[b] + mats[b].shape[0]] for b in range(B)], status


def scipy_col4row(m):
    rows, cols = linear_sum_assignment(m)
    out = np.full(m.shape[0], -1, np.int32)
    out[rows] = cols
    return out


def test_assignment_kernel_equals_scipy_on_the_four_kinds():
    mats = []
    for seed in range(160):
        rng = np.random.default_rng(1000 + seed)
        for kind in lsap_ref.KINDS:
            n, T = (int(x) for x in rng.integers(1, 41, 2))
            mats.append(lsap_ref.matrices(kind, n, T, rng))
    got, status = run_lsap(mats, pad=3)
    assert (status == 0).all()
    for b, m in enumerate(mats):
        assert np.array_equal(got[b], scipy_col4row(m)), (b, m.shape)


@pytest.mark.parametrize("shape", [(300, 70), (58, 70), (70, 58), (1024, 3), (7, 200), (1, 1), (1, 50), (50, 1), (640, 640)])
def test_assignment_kernel_shapes(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    mats = [rng.random(shape)]
    if shape != (640, 640):
        mats += [lsap_ref.matrices(kind, *shape, rng) for kind in ("ties", "iou", "decimal")]
    got, status = run_lsap(mats)
    again, _ = run_lsap(mats)
    assert (status == 0).all()
    for b, m in enumerate(mats):
        assert np.array_equal(got[b], scipy_col4row(m)), b
        assert np.array_equal(got[b], again[b])                     # two runs, identical outputs


@pytest.mark.parametrize("B", [1, 5, 32, 64, 257])
def test_assignment_kernel_batches_of_different_shapes(B):
    rng = np.random.default_rng(B)
    mats = []
    for b in range(B):
        n, T = (int(x) for x in rng.integers(1, 90, 2))
        mats.append(lsap_ref.matrices(lsap_ref.KINDS[b % 4], n, T, rng))
    got, status = run_lsap(mats, pad=b % 2)
    assert (status == 0).all()
    for b, m in enumerate(mats):
        assert np.array_equal(got[b], scipy_col4row(m)), (b, m.shape)


def test_assignment_kernel_status_words():
    rng = np.random.default_rng(9)
    mats = [lsap_ref.matrices(lsap_ref.KINDS[b % 4], 12 + b, 20 - b, rng) for b in range(8)]
    mats[1][3, 4] = np.nan
    mats[4][0, 0] = -np.inf
    mats[6][:, 2] = np.inf                                           # infeasible (18 x 14: every column must be assigned, this one cannot)
    mats[2][5, :] = np.inf
    mats[7][2, 1:] = np.inf                                          # +inf is fine while an assignment exists
    for b in (1, 2, 4, 6):
        with pytest.raises(ValueError):
            linear_sum_assignment(mats[b])
    got, status = run_lsap(mats)
    assert status.tolist() == [0, 1, 2, 0, 1, 0, 2, 0]       # an all-+inf row (problem 2, 14 x 18) is infeasible too
    for b in (0, 3, 5, 7):
        assert np.array_equal(got[b], scipy_col4row(mats[b])), b
    for b in (1, 2, 4, 6):
        assert (got[b] == -7).all()                                  # no assignment written
    # a problem beyond the bounds the launch was sized for is flagged, not run
    got, status = run_lsap(mats[:3], max_rows=13, max_cols=20)
    assert status.tolist() == [0, 1, 3] and np.array_equal(got[0], scipy_col4row(mats[0]))


# ----------------------------------------------------------------------------- the bank against independent trackers
def _load_case(path):
    g = dict(np.load(path))
    rk = dict(ast.literal_eval(str(g["recipe"])))
    tk = dict(ast.literal_eval(str(g["tracker"])))
    seq = tracker_ref.synth_sequence(int(g["seed"]), **rk)
    assert recipes.sha256(*[a for fr in seq for a in fr]) == str(g["sha"])
    return g, seq, tk


def _unpack(g, prefix):
    out, o = [], 0
    for n in g[f"{prefix}_len"]:
        out.append(g[f"{prefix}_cat"][o:o + n])
        o += n
    return out


def _settings():
    seen, out = [], []
    for p in SEQS:
        g = np.load(p)
        tk = dict(ast.literal_eval(str(g["tracker"])))
        rk = dict(ast.literal_eval(str(g["recipe"])))
        key = (sorted(tk.items()), rk.get("sort_scores", True))
        if key not in seen:
            seen.append(key)
            out.append((os.path.basename(p)[10:-4], tk, rk.get("sort_scores", True)))
    return out


def _quiet(fn, *a, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn(*a, **kw)


def _stack(frames, as_torch):
    cols = [np.stack([fr[j] for fr in frames]) for j in range(4)]
    return [torch.from_numpy(c).to(DEV) for c in cols] if as_torch else cols


def _expected_matches(trk, tk):
    """match_with_threshold on the per-stream Tracker's cost matrices, both stages, as tracker.py composes them."""
    if trk.last_costs is None:
        return []
    reid, box, _ = trk.last_costs
    matches, ud, ut = match_with_threshold(reid, tk.get("reid_threshold", 0.2))
    if box is not None:
        new, _, _ = match_with_threshold(box[np.ix_(ud, ut)], tk.get("box_threshold", 0.5))
        matches.extend((ud[x], ut[y]) for x, y in new)
    return matches


def _check_stream(bank, s, trk, oracle, tk, tag):
    st = bank[s]
    assert len(st.tracks) == len(trk.tracks) == len(oracle.tracks), tag
    assert [t.track_id for t in st.tracks] == [t.track_id for t in trk.tracks] == [t.track_id for t in oracle.tracks], tag
    assert [t.state.name for t in st.tracks] == [t.state.name for t in trk.tracks] == [t.state.name for t in oracle.tracks], tag
    assert [(t.birth_age, t.inactive_age) for t in st.tracks] == [(t.birth_age, t.inactive_age) for t in oracle.tracks], tag
    a = np.array([t.bbox for t in st.tracks if t.active], np.float32).reshape(-1, 4)
    assert np.array_equal(a, np.array([t.bbox for t in trk.tracks if t.active], np.float32).reshape(-1, 4)), tag
    assert np.array_equal(a, np.array([t.bbox for t in oracle.tracks if t.active], np.float32).reshape(-1, 4)), tag
    assert st.next_track_id == trk.next_track_id == oracle.next_track_id, tag


def _run_bank_against_trackers(S, tk, sort_scores, frames, k, objects_of):
    seqs = [tracker_ref.synth_sequence(100 + 7 * s, frames=frames, objects=objects_of(s), k=k, sort_scores=sort_scores) for s in range(S)]
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **tk)
    trks = [_quiet(cl.Tracker, device=DEV, **tk) for _ in range(S)]
    oracles = [tracker_ref.Tracker(**tk) for _ in range(S)]
    for f in range(frames):
        fr = [seqs[s][f] for s in range(S)]
        bank.update_batch(*_stack(fr, as_torch=f % 2 == 0))             # device tensors in and numpy in (reference style)
        for s in range(S):
            trks[s].update(*fr[s])
            oracles[s].update(*fr[s])
            _check_stream(bank, s, trks[s], oracles[s], tk, (f, s))
            assert [tuple(p) for p in bank.last_matches[s]] == _expected_matches(trks[s], tk), (f, s)
    for s in range(S):
        want = trks[s].track_embeddings()
        assert torch.equal(bank.track_embeddings(s), want), s            # same kernels, same order: bit-equal
        assert np.array_equal(bank[s].tracks[0].embedding, trks[s].tracks[0].embedding)
    assert len({len(bank[s].tracks) for s in range(S)}) > 1 or S == 1     # the streams really differ in T


@pytest.mark.parametrize("S", [1, 5, 32])
@pytest.mark.parametrize("name,tk,sort_scores", _settings(), ids=[x[0] for x in _settings()])
def test_bank_equals_independent_trackers(S, name, tk, sort_scores):
    _run_bank_against_trackers(S, tk, sort_scores, frames=24, k=48, objects_of=lambda s: 6 + (5 * s) % 11)


def test_bank_equals_independent_trackers_k300():
    _run_bank_against_trackers(5, dict(detection_threshold=0.3), True, frames=40, k=300, objects_of=lambda s: 30 + 9 * s)


@pytest.mark.parametrize("path", SEQS, ids=lambda p: os.path.basename(p)[6:-4])
def test_goldens_as_one_stream_of_a_bank(path):
    g, seq, tk = _load_case(path)
    rk = dict(ast.literal_eval(str(g["recipe"])))
    others = [tracker_ref.synth_sequence(500 + j, **{**rk, "objects": rk.get("objects", 12) + 2 * j - 3}) for j in range(3)]
    gs = 2                                                               # the golden runs as stream 2 of 4
    order = others[:gs] + [seq] + others[gs:]
    bank = _quiet(cl.TrackerBank, num_streams=4, device=DEV, **tk)
    g_ids, g_boxes = _unpack(g, "ids"), _unpack(g, "boxes")
    for f in range(len(seq)):
        bank.update_batch(*_stack([order[s][f] for s in range(4)], as_torch=f % 2 == 1))
        st = bank[gs]
        assert len(st.tracks) == int(g["n_tracks"][f]), f
        assert [t.track_id for t in st.tracks if t.active] == g_ids[f].tolist(), f
        b = np.array([t.bbox for t in st.tracks if t.active], np.float32).reshape(-1, 4)
        assert np.array_equal(b, g_boxes[f].reshape(-1, 4)), f
    assert [t.track_id for t in bank[gs].tracks] == g["final_ids"].tolist()
    np.testing.assert_allclose(bank.track_embeddings(gs).cpu().numpy(), g["final_emb"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(bank[gs].tracks[0].embedding, g["final_emb"][0], rtol=0, atol=2e-6)


def _snapshot(bank, s):
    st = bank[s]
    return ([(t.track_id, t.state.name, t.birth_age, t.inactive_age, np.asarray(t.bbox).tobytes()) for t in st.tracks], st.frame, st.next_track_id,
            bank.track_embeddings(s).clone() if bank.track_embeddings(s) is not None else None)


def _same(a, b):
    return a[:3] == b[:3] and ((a[3] is None and b[3] is None) or torch.equal(a[3], b[3]))


def test_partial_steps_and_reset():
    S, frames = 4, 20
    tk = dict(detection_threshold=0.3)
    seqs = [tracker_ref.synth_sequence(40 + s, frames=frames, objects=8 + 2 * s, k=48) for s in range(S)]
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **tk)
    trks = [_quiet(cl.Tracker, device=DEV, **tk) for _ in range(S)]
    oracles = [tracker_ref.Tracker(**tk) for _ in range(S)]
    nxt = [0] * S                                                        # next frame of each stream

    def step(live):
        fr = [seqs[s][nxt[s]] for s in live]
        bank.update_batch(*_stack(fr, as_torch=True), streams=live)
        for s, x in zip(live, fr):
            trks[s].update(*x)
            oracles[s].update(*x)
            nxt[s] += 1
        for s in range(S):
            _check_stream(bank, s, trks[s], oracles[s], tk, (live, s))

    for _ in range(3):
        step([0, 1, 2, 3])
    before = [_snapshot(bank, s) for s in range(S)]
    step([0, 3])                                                         # streams 1 and 2 keep everything, bit for bit
    for s in (1, 2):
        assert _same(before[s], _snapshot(bank, s)), s
    assert bank.last_matches[1] is not None
    for _ in range(5):                                                   # stream 2 skips 5 steps, in another order of the live list
        step([3, 1, 0])
    step([2])
    step([0, 1, 2, 3])
    for s in range(S):
        assert torch.equal(bank.track_embeddings(s), trks[s].track_embeddings()), s
    keep = [_snapshot(bank, s) for s in range(S)]
    bank.reset(stream=2)
    assert bank[2].tracks == [] and bank[2].next_track_id == 0 and bank[2].frame == 0 and bank.track_embeddings(2).shape[0] == 0
    for s in (0, 1, 3):
        assert _same(keep[s], _snapshot(bank, s)), s
    trks[2].reset()
    oracles[2] = tracker_ref.Tracker(**tk)
    nxt[2] = 0
    step([0, 1, 2, 3])                                                   # stream 2 has no track yet (T = 0) beside streams that have
    # a step in which a stream keeps no detection (n = 0), and n = 0 with T = 0 at once (stream 1 of a fresh bank)
    fr = [list(seqs[s][nxt[s]]) for s in range(S)]
    fr[3][2] = np.zeros_like(fr[3][2])
    bank.update_batch(*_stack(fr, as_torch=False))
    for s in range(S):
        trks[s].update(*fr[s])
        oracles[s].update(*fr[s])
        _check_stream(bank, s, trks[s], oracles[s], tk, ("n0", s))
    assert bank.last_matches[3] == []
    fresh = _quiet(cl.TrackerBank, num_streams=2, device=DEV, **tk)
    two = [list(seqs[0][0]), list(seqs[1][0])]
    two[1][2] = np.zeros_like(two[1][2])
    fresh.update_batch(*_stack(two, as_torch=True))
    assert len(fresh[0].tracks) > 0 and fresh[1].tracks == [] and fresh.last_matches == [[], []]
    bank.reset()
    assert all(bank[s].tracks == [] for s in range(S)) and bank.track_embeddings(0) is None


def test_what_crosses_pcie():
    S, k = 8, 300
    tk = dict(detection_threshold=0.3)
    seqs = [tracker_ref.synth_sequence(70 + s, frames=12, objects=50 + s, k=k) for s in range(S)]
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **tk)
    one = _quiet(cl.Tracker, device=DEV, **tk)
    for f in range(12):
        Ts = [len(bank[s].tracks) for s in range(S)]
        bank.update_batch(*_stack([seqs[s][f] for s in range(S)], as_torch=True))
        bound = sum((64 + 24 * k + 4 * (3 * k + T) + 7) & ~7 for T in Ts)
        assert 0 < bank.d2h_bytes <= bound, f
        one.update(*(torch.from_numpy(a).to(DEV) for a in seqs[0][f]))
        if Ts[0] > 20:
            n, T = one.last_costs[0].shape
            assert one.d2h_bytes >= 12 * n * T                          # the single-stream path ships the matrices ...
            assert bank.d2h_bytes / S < one.d2h_bytes                    # ... the bank's per-stream traffic has no n x T term
    live = [1, 4]
    Ts = [len(bank[s].tracks) for s in live]
    bank.update_batch(*_stack([seqs[s][0] for s in live], as_torch=False), streams=live)     # host inputs: the detections do not come back
    assert bank.d2h_bytes <= sum(64 + 4 * (3 * k + T) for T in Ts)
    # the 58 x 70 case of the README: one stream's step against one Tracker.update on the same frame
    b1 = _quiet(cl.TrackerBank, num_streams=1, device=DEV, **tk)
    t1 = _quiet(cl.Tracker, device=DEV, **tk)
    for fr in tracker_ref.synth_sequence(3, frames=10, objects=58, k=k):
        b1.update_batch(*_stack([fr], as_torch=True))
        t1.update(*(torch.from_numpy(a).to(DEV) for a in fr))
    assert t1.last_costs[0].shape[0] > 30 and t1.last_costs[0].shape[1] > 40
    assert b1.d2h_bytes < t1.d2h_bytes


def test_non_finite_costs_raise_what_tracker_raises_and_leave_every_stream_untouched():
    S = 4
    tk = dict(detection_threshold=0.3, reid_cost="cosine")
    seqs = [tracker_ref.synth_sequence(20 + s, frames=6, objects=9 + s if s < 3 else 30, k=48) for s in range(S)]
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **tk)
    trks = [_quiet(cl.Tracker, device=DEV, **tk) for _ in range(S)]
    for f in range(4):
        bank.update_batch(*_stack([seqs[s][f] for s in range(S)], as_torch=True))
        for s in range(S):
            trks[s].update(*seqs[s][f])
    # two consecutive steps that each redo one stream through the single-stream path: stream 1, then stream 3 with about three times the
    # tracks — its record is more than twice the first one's, so the mapped buffer the bank keeps for redone streams has to grow
    sizes = []
    for bad in (1, 3):
        fr = [list(seqs[s][4]) for s in range(S)]
        fr[bad][3] = fr[bad][3].copy()
        fr[bad][3][0] = 0.0                                              # a zero embedding on a kept detection: cosine = 0 / 0
        with pytest.raises(ValueError) as want:
            trks[bad].update(*fr[bad])
        before = [_snapshot(bank, s) for s in range(S)]
        with pytest.raises(ValueError) as got:
            bank.update_batch(*_stack(fr, as_torch=True))
        assert str(got.value) == str(want.value)
        for s in range(S):                                               # documented: the exception leaves EVERY stream as it was
            assert _same(before[s], _snapshot(bank, s)), s
        sizes.append((len(bank[bad].tracks), bank._redo_rec.nbytes))
    assert sizes[1][0] > 2 * sizes[0][0] and sizes[1][1] > sizes[0][1]
    bank.update_batch(*_stack([seqs[s][4] for s in range(S)], as_torch=True))        # and the bank goes on with a clean frame
    for s in range(S):
        trks[s].update(*seqs[s][4])
    for s in range(S):
        assert [t.track_id for t in bank[s].tracks] == [t.track_id for t in trks[s].tracks]
        assert torch.equal(bank.track_embeddings(s), trks[s].track_embeddings())


def test_bank_with_kalman_filter_matches_oracle():
    S = 3
    kw = dict(detection_threshold=0.3, reid_threshold=0.2, box_cost="iou", box_threshold=0.5, smoothing_factor=0.5, use_kalman=True)
    seqs = [tracker_ref.synth_sequence(11 + s, frames=30, objects=10 + s, k=40) for s in range(S)]
    bank = _quiet(cl.TrackerBank, num_streams=S, device=DEV, **kw)
    oracles = [tracker_ref.Tracker(**kw) for _ in range(S)]
    moved = 0
    for f in range(30):
        live = [0, 2] if f in (7, 8) else list(range(S))                 # a partial step: stream 1's filters must not be predicted
        fr = [seqs[s][oracles[s].frame] for s in live]
        bank.update_batch(*_stack(fr, as_torch=False), streams=live)
        for s, x in zip(live, fr):
            oracles[s].update(*x)
        for s in range(S):
            assert [t.track_id for t in bank[s].tracks] == [t.track_id for t in oracles[s].tracks], (f, s)
            assert [t.state.name for t in bank[s].tracks] == [t.state.name for t in oracles[s].tracks], (f, s)
            a = np.array([np.asarray(t.bbox, np.float64) for t in bank[s].tracks]).reshape(-1, 4)
            b = np.array([np.asarray(t.bbox, np.float64) for t in oracles[s].tracks]).reshape(-1, 4)
            np.testing.assert_allclose(a, b, rtol=0, atol=1e-6)
            lo, hi = int(bank._off[s]), int(bank._off[s + 1])
            np.testing.assert_allclose(bank._box[lo:hi].cpu().numpy(), a.astype(np.float32), rtol=0, atol=1e-7)
            moved += sum(1 for t in bank[s].tracks if t.kf is not None and np.abs(t.kf.x[4:]).max() > 1e-4)
    assert moved > 60


def test_bank_step_batch_end_to_end(configs_dir):
    """model forward -> gather_tracking2d -> one association pass for 4 streams, against four oracle trackers fed with the same detections
    and four cl.Tracker.step_single calls."""
    torch.manual_seed(0)
    cfg = os.path.join(configs_dir, "tracking_resnet34_fpn.yaml")
    model = cl.build_centernet(cfg).cuda().eval()
    bank = cl.build_tracker(cfg, model=model, num_streams=4)
    singles = [cl.build_tracker(cfg, model=model) for _ in range(4)]
    kw = dict(num_detections=50, detection_threshold=0.05)
    oracles = [tracker_ref.Tracker(detection_threshold=0.05) for _ in range(4)]
    base = torch.rand(4, 3, 128, 160, generator=torch.Generator().manual_seed(5))
    for step in range(4):
        frames = base + 0.01 * step * torch.rand(4, 3, 128, 160, generator=torch.Generator().manual_seed(6 + step))
        out = bank.step_batch(frames, **kw)
        assert len(out["bboxes"]) == len(out["track_ids"]) == 4
        heat, box, reid = model(frames.cuda())
        det = {k: v.cpu().numpy() for k, v in model.gather_tracking2d(heat, box, reid, num_detections=50, normalize_bbox=True).items()}
        for s in range(4):
            oracles[s].update(det["bboxes"][s], det["labels"][s], det["scores"][s], det["embeddings"][s])
            ids, boxes = oracles[s].active()
            assert out["track_ids"][s] == ids, (step, s)
            assert len(out["bboxes"][s]) == len(boxes) and all(np.array_equal(a, b) for a, b in zip(out["bboxes"][s], boxes))
            one = singles[s].step_single(frames[s], **kw)
            assert one["track_ids"] == ids and all(np.array_equal(a, b) for a, b in zip(one["bboxes"], boxes))
            assert bank[s].frame == step + 1
    part = bank.step_batch(base[:2], streams=[3, 1], **kw)
    assert len(part["track_ids"]) == 2 and [bank[s].frame for s in range(4)] == [4, 5, 4, 5]


def test_pooled_apply_with_global_index_lists():
    """cnl_track_apply_f32 does the pooled update unchanged: src_trk = rows of the old pooled table, src_det = slot * k + d over the
    flattened [S, k, ...] detections — equal, stream by stream, to per-stream calls on the slices."""
    lib = _lib.load()
    rng = np.random.default_rng(8)
    S, k, E = 3, 10, 32
    Ts = [4, 0, 5]
    off = np.concatenate([[0], np.cumsum(Ts)])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    old_e, old_b = d(rng.standard_normal((off[-1], E)).astype(np.float32)), d(rng.random((off[-1], 4)).astype(np.float32))
    det_e, det_b = d(rng.standard_normal((S, k, E)).astype(np.float32)), d(rng.random((S, k, 4)).astype(np.float32))
    local = [(np.array([0, 2, 3, -1], np.int32), np.array([-1, 4, 9, 7], np.int32)), (np.array([-1, -1], np.int32), np.array([0, 5], np.int32)),
             (np.array([0, 1, 2, 3, 4], np.int32), np.array([-1, -1, -1, -1, -1], np.int32))]      # stream 2 takes no part: rows copied through
    g_trk = np.concatenate([np.where(t >= 0, t + off[s], -1) for s, (t, _) in enumerate(local)]).astype(np.int32)
    g_det = np.concatenate([np.where(x >= 0, x + s * k, -1) for s, (_, x) in enumerate(local)]).astype(np.int32)
    R_new = len(g_trk)
    ne, nb = torch.zeros((R_new, E), device=DEV), torch.zeros((R_new, 4), device=DEV)
    dt, dd = d(g_trk), d(g_det)                                          # (named: the index lists must outlive the launch)
    _lib.check(lib.cnl_track_apply_f32(old_e.data_ptr(), old_b.data_ptr(), det_e.data_ptr(), det_b.data_ptr(), dt.data_ptr(), dd.data_ptr(),
                                       R_new, E, 0.3, ne.data_ptr(), nb.data_ptr(), None))
    r = 0
    for s, (t, x) in enumerate(local):
        pe, pb = torch.zeros((len(t), E), device=DEV), torch.zeros((len(t), 4), device=DEV)
        oe, ob = old_e[off[s]:off[s + 1]].contiguous(), old_b[off[s]:off[s + 1]].contiguous()
        lt, lx = d(t), d(x)
        _lib.check(lib.cnl_track_apply_f32(oe.data_ptr() if Ts[s] else None, ob.data_ptr() if Ts[s] else None, det_e[s].data_ptr(), det_b[s].data_ptr(),
                                           lt.data_ptr(), lx.data_ptr(), len(t), E, 0.3, pe.data_ptr(), pb.data_ptr(), None))
        assert torch.equal(ne[r:r + len(t)], pe) and torch.equal(nb[r:r + len(t)], pb), s
        r += len(t)
