"""GPU: `camera_motion=` on TrackerBank(lifecycle="device") — cnl_track_shift_f64 (csrc/track_lifecycle.hip).

A zero shift changes nothing, bit for bit; a bank that sees translated detections together with the translation's increments does what a bank
that sees the untranslated ones does, with its boxes translated (as equality without a filter: every number is dyadic; to 1e-9 with the float64
filter and the motion gate); streams that take no part are untouched; a non-finite shift is skipped and reported; and the shake scene of
tests/camera_motion_ref.py, estimated by CameraMotion from rendered frames, gives the ids of the restatement."""
import warnings

import numpy as np
import pytest
import torch

import byte_ref
import camera_motion_ref as cr
import tracker_ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import _track_host as th

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S, K, E, M, STEPS = 2, 16, 8, 16, 12
KAL = dict(use_kalman=True, kalman="device")
INT_KEYS = ("offsets", "next_track_id", "track_ids", "states", "birth_age", "inactive_age", "labels")


def _bank(S=S, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return cl.TrackerBank(S, device=DEV, lifecycle="device", max_tracks=M, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({8: np.uint64, 4: np.uint32, 1: np.uint8}[a.dtype.itemsize])


def _stack(per_stream, f):
    return tuple(torch.from_numpy(np.stack([seq[f][j] for seq in per_stream])).to(DEV) for j in range(4))


def _lists(bank, n):
    return [(bank.last_matches[s], bank.last_low_matches[s]) for s in range(n)]


# ----------------------------------------------------------------------------------------------------------------------- a zero shift
ZERO_CASES = {
    "plain": (lambda s: tracker_ref.synth_sequence(60 + s, frames=STEPS, objects=5, k=K, emb_dim=E), {}),
    "kalman": (lambda s: tracker_ref.synth_sequence(70 + s, frames=STEPS, objects=5, k=K, emb_dim=E), KAL),
    "low": (lambda s: byte_ref.synth_occlusion(80 + s, frames=STEPS, objects=6, k=K, emb_dim=E)[0], dict(low_threshold=0.1)),
    "class_aware": (lambda s: tracker_ref.synth_sequence(90 + s, frames=STEPS, objects=5, k=K, emb_dim=E), dict(class_aware=True)),
    "gated_kalman_low": (lambda s: byte_ref.synth_occlusion(95 + s, frames=STEPS, objects=6, k=K, emb_dim=E)[0],
                         dict(low_threshold=0.1, class_aware=True, motion_gate=True, **KAL)),
}


@pytest.mark.parametrize("name", list(ZERO_CASES))
def test_a_zero_shift_changes_no_bit(name):
    make, kw = ZERO_CASES[name]
    seqs = [make(s) for s in range(S)]
    plain, zero = _bank(**kw), _bank(**kw)
    shift = torch.zeros((S, 2), device=DEV)
    rows = 0
    for f in range(STEPS):
        det = _stack(seqs, f)
        a, b = plain.update_batch(*det), zero.update_batch(*det, camera_motion=shift)
        for key in a:
            assert a[key].dtype == b[key].dtype and torch.equal(a[key].view(torch.uint8), b[key].view(torch.uint8)), (name, f, key)
        sa, sb = plain.snapshot(), zero.snapshot()
        assert sa.keys() == sb.keys()
        for key in sa:
            assert np.array_equal(_bits(sa[key]), _bits(sb[key])), (name, f, key)
        assert _lists(plain, S) == _lists(zero, S), (name, f)
        rows = max(rows, int(sa["offsets"][-1]))
    assert rows >= 2 * S
    plain.check()
    zero.check()


# ----------------------------------------------------------------------------------------------------------------------- equivariance
def dyadic_scene(seed, frames=STEPS, objects=5):
    """Boxes, velocities and sizes in multiples of 1/64, every coordinate below 32: fp32 sums, areas and intersections of such boxes are exact,
    also after an offset below 16.  Objects blink (a missed detection: INACTIVE tracks get shifted too); clutter sits below every threshold."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(2 * 64, 20 * 64, (objects, 2))
    pos[:, 0] = np.linspace(2 * 64, 20 * 64, objects).astype(np.int64)[rng.permutation(objects)]
    vel = rng.integers(-16, 17, (objects, 2))
    size = rng.integers(2 * 64, 4 * 64, (objects, 2))
    ident = rng.standard_normal((objects, E)).astype(np.float32)
    out = []
    for f in range(frames):
        boxes, scores, embs = np.zeros((K, 4)), np.zeros(K), rng.standard_normal((K, E))
        for o in range(objects):
            p = pos[o] + f * vel[o]
            boxes[o] = (p[0], p[1], p[0] + size[o, 0], p[1] + size[o, 1])
            blink = f >= 3 and (f + 2 * o) % 7 == 0
            scores[o] = 0.01 if blink else 0.9 - 0.01 * o
            embs[o] = ident[o]
        for j in range(objects, K):
            c = rng.integers(64, 24 * 64, 2)
            boxes[j] = (c[0], c[1], c[0] + 32, c[1] + 32)
            scores[j] = 0.02
        out.append(((boxes / 64).astype(np.float32), np.zeros(K, np.int64), scores.astype(np.float32), embs.astype(np.float32)))
    return out


def dyadic_offsets(seed, frames=STEPS):
    """Per step one (cx, cy) per stream, multiples of 1/64 below 16 in magnitude: a walk with a jump in the middle."""
    rng = np.random.default_rng(seed)
    c = np.cumsum(rng.integers(-48, 49, (frames, S, 2)), axis=0)
    c[frames // 2:frames // 2 + 3] += rng.integers(4 * 64, 6 * 64, (S, 2))         # more than a box for three steps, then back
    assert np.abs(c).max() < 16 * 64
    return (c / 64).astype(np.float32)


def _translated(det, c):
    """The step's detections with offset c [S, 2] added to every box (exact in fp32 for the dyadic scenes)."""
    boxes = det[0] + torch.from_numpy(np.concatenate([c, c], 1)).to(DEV)[:, None, :]
    return (boxes.contiguous(),) + tuple(det[1:])


def _equivariant_run(kw, exact):
    seqs = [dyadic_scene(100 + s) for s in range(S)]
    offs = dyadic_offsets(7)
    a, b = _bank(**kw), _bank(**kw)
    prev = np.zeros((S, 2), np.float32)
    worst, shifted_inactive = 0.0, 0
    for f in range(STEPS):
        det = _stack(seqs, f)
        c = offs[f]
        oa = a.update_batch(*det)
        ob = b.update_batch(*_translated(det, c), camera_motion=torch.from_numpy(c - prev).to(DEV))
        prev = c
        sa, sb = a.snapshot(), b.snapshot()
        for key in INT_KEYS:
            assert np.array_equal(sa[key], sb[key]), (f, key)
        assert _lists(a, S) == _lists(b, S), f
        assert torch.equal(oa["track_ids"], ob["track_ids"]) and torch.equal(oa["count"], ob["count"]) and torch.equal(oa["labels"], ob["labels"])
        assert np.array_equal(_bits(sa["embeddings"]), _bits(sb["embeddings"])), f
        off = sa["offsets"]
        per_row = np.concatenate([np.tile(np.concatenate([c[s], c[s]]), (int(off[s + 1] - off[s]), 1)) for s in range(S)] + [np.zeros((0, 4), np.float32)])
        live = (torch.arange(M, device=DEV)[None, :] < oa["count"][:, None])[..., None]
        out_want = torch.where(live, oa["bboxes"] + torch.from_numpy(np.concatenate([c, c], 1)).to(DEV)[:, None, :].to(oa["bboxes"].dtype), oa["bboxes"])
        if exact:
            assert np.array_equal(sb["table_boxes"], sa["table_boxes"] + per_row), f
            assert np.array_equal(sb["bboxes"], sa["bboxes"] + per_row.astype(sa["bboxes"].dtype)), f
            assert torch.equal(ob["bboxes"], out_want), f
        else:
            errs = [np.abs(sb["bboxes"] - (sa["bboxes"] + per_row)).max(initial=0.0), np.abs(sb["kx"][:, :4] - (sa["kx"][:, :4] + per_row)).max(initial=0.0),
                    np.abs(sb["kx"][:, 4:] - sa["kx"][:, 4:]).max(initial=0.0), float((ob["bboxes"] - out_want).abs().max())]
            worst = max(worst, *errs)
            assert np.abs(sa["bboxes"]).max(initial=0.0) < 64
        # a row that is INACTIVE now was carried through this step, shifted, and is shifted again in front of the next association
        shifted_inactive += int((sb["states"] == th.TrackState.INACTIVE.value).sum())
    a.check()
    b.check()
    assert shifted_inactive > 0 and int(sa["offsets"][-1]) >= 2 * S
    return worst


def test_translation_equivariance_is_exact_without_a_filter():
    _equivariant_run({}, exact=True)


def test_translation_equivariance_with_the_filter_and_the_motion_gate():
    """Ids, states, ages and match lists equal; reported boxes and filter positions within 1e-9 of the translated ones (coordinates below 64:
    float64 rounding over 12 steps, about 1e-13 per step), velocities within 1e-9 of the untranslated run's."""
    worst = _equivariant_run(dict(motion_gate=True, **KAL), exact=False)
    print(f"largest deviation from the translated run over {STEPS} steps: {worst:.3e}")
    assert worst <= 1e-9


# ----------------------------------------------------------------------------------------------------------------------- who is shifted
@pytest.mark.parametrize("kalman", [False, True])
def test_only_the_participating_streams_rows_move_and_inactive_rows_move_too(kalman):
    kw = KAL if kalman else {}
    seqs = [dyadic_scene(200 + s) for s in range(3)]
    bank = _bank(3, **kw)
    for f in range(4):      # (object 2 of every stream blinks in frame 3: one row is INACTIVE already)
        bank.update_batch(*_stack(seqs, f))
    # stream 1 alone, with NO confident detection: every ACTIVE row turns INACTIVE, every row is carried — and shifted
    det = tuple(t[1:2].clone() for t in _stack(seqs, 4))
    det[2].fill_(0.0)
    before = bank.snapshot()
    shift = np.array([[3.25, -1.5]], np.float32)
    bank.update_batch(*det, streams=[1], camera_motion=torch.from_numpy(shift).to(DEV))
    after = bank.snapshot()
    off = before["offsets"]
    r0, r1 = int(off[1]), int(off[2])
    keep = np.flatnonzero(before["states"][r0:r1] != th.TrackState.UNCONFIRMED.value) + r0          # UNCONFIRMED rows die unmatched
    assert len(keep) >= 2 and (before["states"][keep] == th.TrackState.INACTIVE.value).any()
    o1 = int(after["offsets"][1])
    rows_after = np.arange(o1, o1 + len(keep))
    assert np.array_equal(after["track_ids"][rows_after], before["track_ids"][keep])
    assert (after["states"][rows_after] == th.TrackState.INACTIVE.value).all()
    v = np.concatenate([shift[0], shift[0]])
    if kalman:          # the filter predicts the carried rows of a participating stream: positions + velocities, then the shift is in both
        assert np.allclose(after["kx"][rows_after, :4], before["kx"][keep, :4] + before["kx"][keep, 4:] + v, rtol=0, atol=1e-9)
        assert np.array_equal(_bits(after["bboxes"][rows_after]), _bits(before["bboxes"][keep] + v.astype(np.float64)))
    else:
        assert np.array_equal(after["table_boxes"][rows_after], before["table_boxes"][keep] + v)
        assert np.array_equal(after["bboxes"][rows_after], before["bboxes"][keep] + v)
    for s in (0, 2):    # the other streams: every array, bit for bit
        b0, b1, a0, a1 = int(off[s]), int(off[s + 1]), int(after["offsets"][s]), int(after["offsets"][s + 1])
        assert b1 - b0 == a1 - a0 and b1 > b0
        for key in after:
            if key not in ("offsets", "next_track_id"):
                assert np.array_equal(_bits(after[key][a0:a1]), _bits(before[key][b0:b1])), (s, key)
    assert np.array_equal(after["next_track_id"], before["next_track_id"])
    bank.check()


def test_a_non_finite_shift_skips_its_stream_and_is_reported():
    seqs = [dyadic_scene(300 + s) for s in range(S)]
    bad, ref = _bank(**KAL), _bank(**KAL)
    for f in range(4):
        det = _stack(seqs, f)
        bad.update_batch(*det)
        ref.update_batch(*det)
    det = _stack(seqs, 4)
    for shift in ([[float("nan"), 1.0], [2.0, -3.0]], [[0.5, float("inf")], [0.0, 0.0]]):
        finite = [[0.0, 0.0], shift[1]]
        out = bad.update_batch(*det, camera_motion=torch.tensor(shift, device=DEV))
        want = ref.update_batch(*det, camera_motion=torch.tensor(finite, device=DEV))
        assert all(torch.equal(out[k].view(torch.uint8), want[k].view(torch.uint8)) for k in out)
        sa, sb = bad.snapshot(), ref.snapshot()
        assert all(np.array_equal(_bits(sa[k]), _bits(sb[k])) for k in sa)
        with pytest.raises(ValueError, match=r"stream 0: a non-finite camera_motion shift \(skipped\), first at step"):
            bad.check()
        bad.check()         # reported once: the words were cleared
        ref.check()


# ----------------------------------------------------------------------------------------------------------------------- the scene
def test_the_shake_scene_from_rendered_frames_gives_the_restatements_ids():
    dets, _, _ = cr.shake_scene()
    offs = cr.offsets()
    true = [(0, 0)] + [(offs[f][0] - offs[f - 1][0], offs[f][1] - offs[f - 1][1]) for f in range(1, cr.FRAMES)]
    _, want = cr.run_scene(dets, true)
    _, want_plain = cr.run_scene(dets, None)
    canvas = cr.textured(np.random.default_rng(1), cr.H + 2 * cr.MARGIN, cr.W + 2 * cr.MARGIN)
    frames = [torch.from_numpy(cr.render(canvas, dets, f)).to(DEV) for f in range(cr.FRAMES)]
    d_dets = [tuple(torch.from_numpy(a[None]).to(DEV) for a in det) for det in dets]
    cm = cl.CameraMotion(1, **cr.ESTIMATOR)
    bank, plain = _bank(1, **cr.TRACKER), _bank(1, **cr.TRACKER)
    for f in range(cr.FRAMES):
        est = cm.update([frames[f]], boxes=d_dets[f][0], count=torch.full((1,), 5, dtype=torch.int32, device=DEV))
        out = bank.update_batch(*d_dets[f], camera_motion=est["shift"])
        plain.update_batch(*d_dets[f])
        assert est["shift"][0].tolist() == list(true[f]), f
        snap = bank.snapshot()
        assert list(zip(snap["track_ids"].tolist(), snap["states"].tolist())) == [(i, st.value) for i, st in want[f]], f
        active = [i for i, st in want[f] if st is th.TrackState.ACTIVE]
        assert out["track_ids"][0, :int(out["count"][0])].tolist() == active, f
        snap = plain.snapshot()
        assert list(zip(snap["track_ids"].tolist(), snap["states"].tolist())) == [(i, st.value) for i, st in want_plain[f]], f
    assert sorted(i for i, _ in want[-1]) == [0, 1, 2, 3, 4] and len(want_plain[-1]) > 5
    bank.check()
    plain.check()


def _boom(*a, **kw):
    raise AssertionError("host synchronisation inside a step")


def test_estimating_and_applying_never_synchronises(monkeypatch):
    """Frames in, tracks out, on one stream: CameraMotion.update, the scaling multiply and the bank's step queue launches and nothing else."""
    dets, _, _ = cr.shake_scene()
    canvas = cr.textured(np.random.default_rng(1), cr.H + 2 * cr.MARGIN, cr.W + 2 * cr.MARGIN)
    frames = [torch.from_numpy(cr.render(canvas, dets, f)).to(DEV) for f in range(10)]
    d_dets = [tuple(torch.from_numpy(a[None]).to(DEV) for a in det) for det in dets[:10]]
    cm = cl.CameraMotion(1, **cr.ESTIMATOR)
    bank, ref = _bank(1, **cr.TRACKER), _bank(1, **cr.TRACKER)
    one = torch.ones(2, device=DEV)
    for f in range(3):          # (the first steps allocate the state)
        bank.update_batch(*d_dets[f], camera_motion=cm.update([frames[f]])["shift"] * one)
    torch.cuda.synchronize()
    with monkeypatch.context() as m:
        for owner, attr in ((torch.cuda.Stream, "synchronize"), (torch.cuda, "synchronize"), (torch.Tensor, "cpu"), (torch.Tensor, "item"),
                            (torch.Tensor, "tolist"), (torch.Tensor, "numpy")):
            m.setattr(owner, attr, _boom)
        outs = [bank.update_batch(*d_dets[f], camera_motion=cm.update([frames[f]])["shift"] * one) for f in range(3, 10)]
    offs = cr.offsets()
    for f in range(10):
        shift = torch.tensor([[offs[f][0] - offs[f - 1][0], offs[f][1] - offs[f - 1][1]] if f else [0, 0]], dtype=torch.float32, device=DEV)
        want = ref.update_batch(*d_dets[f], camera_motion=shift)
        if f >= 3:
            assert all(torch.equal(outs[f - 3][k], want[k]) for k in want), f
    assert int(want["count"][0]) == 5
