"""GPU: MotEvaluator (csrc/mot_eval.hip) against the numpy + scipy restatement of the rule (tests/mot_eval_ref.py).  Every comparison is an
EQUALITY: integer fields as integers, float64 fields by their bits.  Boxes sit on an integer grid (corners 0..40, sizes 1..40) with most
predictions crowding around a ground truth, so IoU ties and exact hits of 0.5 occur; ids are sparse and shuffled within frames."""
import numpy as np
import pytest
import torch

import mot_eval_ref as ref
import centernet_lightning_amd as cl
from centernet_lightning_amd import mot_eval
from strided_io import GuardedBytes

pytestmark = pytest.mark.gpu
EMPTY = np.zeros((0, 4))
BOX = np.array([[10.0, 10.0, 20.0, 40.0]])


def world_sequence(seed, n_frames, max_objects, n_world, forced=()):
    """Objects that persist and move on the grid; a tracker that follows them, sometimes under a new id, plus false positives.
    forced: {frame: "no_pred" | "no_gt" | "none"}"""
    rng = np.random.default_rng(seed)
    gids = rng.permutation(900)[:n_world] + 1
    trk = dict(zip(gids.tolist(), (rng.permutation(900)[:n_world] + 1000).tolist()))
    next_trk = 3000
    pos = {g: rng.integers(0, 41, 2) for g in gids.tolist()}
    size = {g: rng.integers(1, 41, 2) for g in gids.tolist()}
    forced, frames = dict(forced), []
    for f in range(n_frames):
        n = int(rng.integers(0, max_objects + 1)) if max_objects < n_world else n_world
        visible = rng.permutation(gids)[:n].tolist()
        gt = np.array([[*pos[g], *size[g]] for g in visible], np.float64).reshape(-1, 4)
        pb, pi = [], []
        for g in visible:
            u = rng.random()
            if u < 0.2:
                continue                                                      # missed
            if rng.random() < 0.12:
                trk[g], next_trk = next_trk, next_trk + int(rng.integers(1, 9))      # the tracker loses the identity
            box = np.array([*pos[g], *size[g]])
            if u > 0.55:                                                      # crowding: a grid step off, or half / double the width
                box = box + np.array([*rng.integers(-1, 2, 2), *rng.integers(-1, 2, 2)])
                if rng.random() < 0.2:
                    box[2] = box[2] * 2
            box[2:] = np.maximum(box[2:], 1)
            pb.append(box); pi.append(trk[g])
        for fp_id in (rng.permutation(500)[:int(rng.integers(0, 3))] + 5000).tolist():          # false positives
            pb.append(np.array([*rng.integers(0, 41, 2), *rng.integers(1, 41, 2)])); pi.append(fp_id)
        order = rng.permutation(len(pi))
        pred, pids = np.array(pb, np.float64).reshape(-1, 4)[order], np.array(pi, np.int64)[order]
        gid_arr = np.array(visible, np.int64)
        kind = forced.get(f)
        if kind in ("no_pred", "none"):
            pred, pids = EMPTY, np.zeros(0, np.int64)
        if kind in ("no_gt", "none"):
            gt, gid_arr = EMPTY, np.zeros(0, np.int64)
        frames.append((gt, gid_arr, pred, pids))
        for g in gids.tolist():
            pos[g] = np.clip(pos[g] + rng.integers(-2, 3, 2), 0, 40)
    return frames


def wide_sequence(seed=11, n_frames=20, per_frame=55, n_ids=515):
    """515 ground-truth and 515 tracker ids (G + T = 1030 > 1024: Identity's assignment is solved on the host), 20 frames of 55 objects."""
    rng = np.random.default_rng(seed)
    g_pool, t_pool = np.sort(rng.permutation(9000)[:n_ids]) + 1, np.sort(rng.permutation(9000)[:n_ids]) + 1
    boxes = np.concatenate([rng.integers(0, 41, (n_ids, 2)), rng.integers(1, 41, (n_ids, 2))], 1).astype(np.float64)
    frames = []
    for f in range(n_frames):
        start = round(f * (n_ids - per_frame) / (n_frames - 1))
        idx = np.arange(start, start + per_frame)
        jitter = np.concatenate([rng.integers(-1, 2, (per_frame, 2)), rng.integers(0, 2, (per_frame, 2))], 1)
        go, po = rng.permutation(per_frame), rng.permutation(per_frame)
        frames.append((boxes[idx][go], g_pool[idx][go], (boxes[idx] + jitter)[po], t_pool[idx][po]))
    return frames


def _update(ev, frames, name):
    ev.update([f[2] for f in frames], [f[3] for f in frames], [f[0] for f in frames], [f[1] for f in frames], sequence=name)


def same(got, want, where):
    """Every field of the restatement's result, as an equality."""
    for key, w in want.items():
        assert key in got, f"{where}: {key} missing"
        g = got[key]
        if isinstance(w, np.ndarray):
            assert isinstance(g, np.ndarray) and g.shape == w.shape, f"{where}: {key}"
            if np.issubdtype(w.dtype, np.integer):
                assert np.issubdtype(g.dtype, np.integer) and (g == w).all(), f"{where}: {key} {g} != {w}"
            else:
                assert g.dtype == np.float64 and g.tobytes() == w.tobytes(), f"{where}: {key} {g} != {w} (max |diff| {np.abs(g - w).max()})"
        elif isinstance(w, int):
            assert isinstance(g, int) and g == w, f"{where}: {key} {g} != {w}"
        else:
            assert isinstance(g, float) and np.float64(g).tobytes() == np.float64(w).tobytes(), f"{where}: {key} {g!r} != {w!r}"


def check(sequences):
    ev = cl.MotEvaluator()
    for name, frames in sequences.items():
        _update(ev, frames, name)
    got, want = ev.get_metrics(), ref.evaluate(sequences)
    assert list(got) == list(want)
    for name in want:
        same(got[name], want[name], name)
    return ev, got


MIXED = {"a": world_sequence(1, 40, 8, 10, {3: "no_pred", 7: "no_gt", 12: "none", 13: "no_gt", 20: "no_pred"}),
         "b": world_sequence(2, 5, 8, 9, {0: "none"}),
         "c": world_sequence(3, 17, 8, 12, {16: "no_pred"}),
         "only_gt": [(f[0], f[1], EMPTY, np.zeros(0, np.int64)) for f in world_sequence(4, 6, 5, 6)],
         "only_pred": [(EMPTY, np.zeros(0, np.int64), f[2], f[3]) for f in world_sequence(5, 6, 5, 6)]}


def test_sequences_together_per_sequence_and_combined():
    assert sum(len(f[1]) for f in MIXED["only_gt"]) and sum(len(f[3]) for f in MIXED["only_pred"])
    sims = [ref.similarity(f[0], f[2]) for f in MIXED["a"] + MIXED["c"]]
    assert any((s == 0.5).any() for s in sims) and any((s == 1.0).sum() > 0 for s in sims)          # the data does hit 0.5 and ties
    ev, got = check(MIXED)
    assert got["a"]["IDSW"] > 0 and got["a"]["Frag"] > 0 and got["COMBINED_SEQ"]["CLR_Frames"] == 40 + 5 + 17
    again = ev.get_metrics()                                                  # two consecutive calls agree
    for name in got:
        same(again[name], {k: v for k, v in got[name].items() if k != "summary"}, name)
        assert again[name]["summary"] == got[name]["summary"]
    ev.reset()
    with pytest.raises(RuntimeError):
        ev.get_metrics()
    _update(ev, MIXED["b"], "b")
    same(ev.get_metrics()["b"], ref.evaluate_sequence(MIXED["b"]), "b alone after reset")


def test_a_frame_of_70_objects_on_both_sides():
    """More than one lane pass everywhere (64 lanes): the similarity rows, pass 1, the solver's scans, CLEAR's and Identity's matrices."""
    frames = world_sequence(6, 3, 70, 70)
    assert len(frames[0][1]) == 70 and min(len(f[3]) for f in frames) > 50
    frames[1] = (frames[1][0], frames[1][1], np.concatenate([frames[1][2], frames[1][0][:70 - len(frames[1][3])]]),
                 np.concatenate([frames[1][3], 7000 + np.arange(70 - len(frames[1][3]))]))
    assert len(frames[1][3]) == 70
    check({"wide_frames": frames})


def test_an_object_that_returns_under_another_tracker_id():
    far = np.array([[100.0, 100, 5, 5]])
    frames = [(BOX, [1], BOX, [7]), (BOX, [1], far, [7]), (EMPTY, [], far, [7]), (BOX, [1], BOX, [9]), (BOX, [1], EMPTY, []), (BOX, [1], np.concatenate([BOX, BOX]), [7, 9])]
    _, got = check({"returns": frames})
    assert got["returns"]["IDSW"] == 1 and got["returns"]["Frag"] == 1


def test_identity_of_1030_ids_is_solved_on_the_host():
    frames = wide_sequence()
    data = ref.prepare(frames)
    assert data["G"] + data["T"] == 1030
    _, got = check({"many_ids": frames, "small": MIXED["b"]})
    assert got["many_ids"]["IDTP"] > 0


def test_evaluate_mot_tracking_sequence_on_the_hand_worked_cases():
    for tids, want in (([7, 7, 7, 7], {"HOTA": 1.0, "MOTA": 1.0, "IDF1": 1.0}), ([7, 7, 9, 9], {"HOTA": 0.7071067811865476, "MOTA": 0.75, "IDF1": 0.5})):
        got = cl.evaluate_mot_tracking_sequence([BOX] * 4, [[t] for t in tids], [torch.tensor(BOX)] * 4, [torch.tensor([1], device="cuda")] * 4)
        assert list(got) == ["HOTA", "MOTA", "IDF1"] and got == want, got


def test_launches_write_inside_guarded_outputs_and_exactly_sized_workspaces():
    """Every output, the similarity pool, pm and the three workspaces (each exactly the queried size) inside sentinel guards at the
    header's alignment; the results equal the unguarded run's."""
    sequences = list({"a": MIXED["a"], "only_gt": MIXED["only_gt"], "c": MIXED["c"]}.items())
    ev = cl.MotEvaluator()
    for name, frames in sequences:
        _update(ev, frames, name)
    arrays, scalars, facts = mot_eval.pool(list(ev._sequences.items()))
    dev = torch.device("cuda", torch.cuda.current_device())
    plain, _, _ = mot_eval.run(arrays, scalars, dev)
    made = []

    def guarded(nbytes, align, device, name):
        g = GuardedBytes(nbytes, align=align, device=device, name=name)
        made.append(g)
        return g
    got, pm, kept = mot_eval.run(arrays, scalars, dev, alloc=guarded)
    torch.cuda.synchronize()
    assert len(made) == 1 + 8 + 1 + 3 and kept["ws_bytes"]["hota"] > 0 and kept["ws_bytes"]["clear"] > 0 and kept["ws_bytes"]["identity"] > 0
    for g in made:
        ok, message = g.verdict()
        assert ok, message
    for key in plain:
        assert plain[key].tobytes() == got[key].tobytes(), key
    assert not got["status_hota"].any() and not got["status_clear"].any() and not got["status_identity"].any()
    want = ref.evaluate(dict(sequences))
    result = mot_eval.assemble(got, arrays, scalars, facts, pm)
    for name in want:
        same(result[name], want[name], name)
